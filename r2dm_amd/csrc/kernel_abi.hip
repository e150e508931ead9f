// Single-kernel entry points of the C ABI (include/r2dm_hip.h): one kernel, or one short pair, on caller-provided tensors -- the unit parity tests
// and the probes under scripts/ drive them.  Their precision mode is r2dm_set_conv_pieces(NULL, ...) (g_single_kernel_pieces).
#include <algorithm>

#include "engine.h"

using namespace r2dm;

extern "C" {

// ---- single-kernel entry points (unit parity tests) ---------------------------------------------
int64_t r2dm_conv_packed_elems(int32_t cout, int32_t cin, int32_t ksize, int32_t B, int32_t H, int32_t W) {
    const int taps = ksize * ksize;
    int algo = conv_pick_algo(cin, cout, taps);
    if (algo == ALGO_DIRECT) algo = ALGO_F32;  // scratch sized for the larger (fp32-MFMA) packing: either may be chosen
    const int ct = conv_base_co_tile(algo, cin, cout, taps, (long)B * H * W);
    int64_t n = (int64_t)conv_packed_floats(algo, cin, cout, taps, ct, conv_base_cin_pad(algo, cin, taps, ct));
    if (algo == ALGO_BF16X3 && conv_f16x2_supported(cin, cout, taps, H, W)) n = std::max<int64_t>(n, conv_f16x2_packed_floats(cin, cout) + 64);
    if (proj_f16x2_supported(cin, cout, taps, H, W)) n = std::max<int64_t>(n, proj_f16x2_packed_floats(cin, cout) + 64);
    return n;
}

// (per-kernel tests of the fp16 activation storage: R2DM_TEST_IO16 bit 0 -- x holds fp16, bit 1 -- y will; the caller passes tensors of that type)
static int test_io16() {
    const char* e = getenv("R2DM_TEST_IO16");
    return e ? atoi(e) : 0;
}

// what r2dm_conv2d_ring_ex sets beyond r2dm_conv2d_ring: the ConvParams fields that otherwise only forward.hip fills
struct ConvExtras {
    const float* x1 = nullptr;  // second input allocation: the last c1 of the cin channels (Src::p1)
    int c1 = 0;
    int res_broadcast = 0;      // the residual is one (cout, H, W) map for the whole batch (res_bs = 0)
    double* stat = nullptr;     // fused statistics sink [B][stat_G][conv_stat_slots(H, W)][2]
    int stat_G = 0, stat_goff = 0, stat_cpg = 0;
    int* range = nullptr;       // device int[2]: [1] takes the running maximum
    int reverse = 0;
    int32_t* chosen = nullptr;  // HOST int32[3] <- algo, co_tile, px_rows
};

// One convolution launch on caller-provided tensors: the algorithm and tile selection, the packing, and the IO16 test hook of the
// single-kernel entries.  Every combination a launcher would refuse, ignore or run past the caller's buffers is refused HERE, before the first
// launch: nothing is written then.
static int conv2d_ring_impl(const float* x, const float* w, const float* bias, float* w_packed, const float* aff, int32_t prologue, const float* residual,
                            const float* scale, float* y, int32_t B, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t ksize, void* stream,
                            const ConvExtras& ex) {
    if (!x || !w || !bias || !w_packed || !y) return fail(1, "null argument");
    if (ksize != 1 && ksize != 3) return fail(1, "kernel size must be 1 or 3");
    hipStream_t st = (hipStream_t)stream;
    const int taps = ksize * ksize;
    int pieces = 3, px_rows = 4;
    int algo = conv_pick_algo(cin, cout, taps);
    if (g_single_kernel_pieces >= 4 && algo != ALGO_DIRECT) {  // (test hook: the fp32-input MFMA kernel)
        algo = ALGO_F32;
        pieces = g_single_kernel_pieces;
    }
    // (the few-input kernel -- in_conv in the engine -- where the fp16-storage test hook asks for it: plain convolutions only)
    if (test_io16() && conv_few_in_supported(cin, cout, taps, H, W) && prologue == PRO_NONE && !scale) algo = ALGO_DIRECT;
    if (algo == ALGO_DIRECT && cout <= 4 && (prologue != PRO_NONE || residual || scale || W % 4 != 0)) algo = ALGO_F32;  // plain convolutions of 16-byte rows only
                                                                                                             // (any other width runs on the fp32-MFMA kernel)
    // per-op tests: with pieces = 2 every shape the f16x2 kernel covers goes there (the engine restricts it to normalised inputs)
    if (algo == ALGO_BF16X3 && g_single_kernel_pieces != 3 && conv_f16x2_supported(cin, cout, taps, H, W)) algo = ALGO_F16X2;
    if (algo == ALGO_F32 && g_single_kernel_pieces < 3 && prologue != PRO_AFFINE_SILU && proj_f16x2_supported(cin, cout, taps, H, W)) algo = ALGO_P1F16;
    if (algo == ALGO_F16X2 || algo == ALGO_P1F16) pieces = g_single_kernel_pieces;
    const int co_tile = algo == ALGO_F16X2 ? conv_f16x2_pick_co_tile(cin, cout, H, W, (long)B * H * W, &px_rows) : algo == ALGO_P1F16 ? 64 : conv_base_co_tile(algo, cin, cout, taps, (long)B * H * W);
    const int cin_pad = conv_base_cin_pad(algo, cin, taps, co_tile);
    if (ex.chosen) {
        ex.chosen[0] = algo;
        ex.chosen[1] = co_tile;
        ex.chosen[2] = px_rows;
    }
    // ---- the extended entry's fields: what the launchers refuse (conv_direct / conv_bf16x3 / conv_f16x2 / proj_f16x2 .hip), what they would silently ignore,
    // and what would send a kernel past the caller's sink
    if ((ex.res_broadcast | ex.reverse) & ~1) return fail(1, "conv2d_ring_ex: res_broadcast and reverse are 0 or 1");
    if (ex.res_broadcast && !residual) return fail(1, "conv2d_ring_ex: res_broadcast without a residual");
    if (ex.c1 < 0 || ex.c1 >= cin) return fail(1, "conv2d_ring_ex: c1 = %d outside [0, cin = %d)", ex.c1, cin);
    if ((ex.x1 != nullptr) != (ex.c1 > 0)) return fail(1, "conv2d_ring_ex: x1 and c1 go together");
    if (ex.x1) {
        const int c0 = cin - ex.c1;
        if (algo == ALGO_DIRECT) return fail(1, "conv2d_ring_ex: the direct kernels take one input allocation");  // (launch_conv_direct; the engine's in / out convolutions)
        if ((algo == ALGO_BF16X3 || algo == ALGO_F16X2) && c0 % 16) return fail(1, "conv2d_ring_ex: the concat seam (%d) must lie on a 16-channel chunk boundary", c0);
        if (algo == ALGO_P1F16 && c0 % 8) return fail(1, "conv2d_ring_ex: the concat seam (%d) must lie on an 8-channel boundary", c0);
    }
    if (ex.range && algo == ALGO_DIRECT) return fail(1, "conv2d_ring_ex: the direct kernels record no range");
    if (ex.reverse && algo != ALGO_F16X2 && algo != ALGO_P1F16) return fail(1, "conv2d_ring_ex: this kernel has no descending tile walk");
    if (ex.stat) {
        // (this entry knows the kernel it launches; the engine asks about the layer's own kernel, whichever packing runs: forward.hip choose)
        const bool emits = algo == ALGO_F16X2 || algo == ALGO_P1F16 || conv_emits_stats(algo, co_tile, cout);
        if (!emits) return fail(1, "conv2d_ring_ex: this kernel (algo %d, tile %d) emits no statistics", algo, co_tile);
        const int cpg = ex.stat_cpg;
        if (cpg != 8 && cpg != 16 && cpg != 32 && cpg != 64) return fail(1, "conv2d_ring_ex: stat_cpg = %d (8, 16, 32 or 64 channels per group)", cpg);
        if (cout % cpg) return fail(1, "conv2d_ring_ex: %d output channels do not split into groups of %d", cout, cpg);
        if (ex.stat_goff < 0 || ex.stat_goff + cout / cpg > ex.stat_G) return fail(1, "conv2d_ring_ex: groups [%d, %d) outside a sink of %d", ex.stat_goff, ex.stat_goff + cout / cpg, ex.stat_G);
        if (test_io16() & 3) return fail(1, "conv2d_ring_ex: no statistics together with the fp16 storage hook");
    }
    // per-kernel tests of the fp16 activation storage (conv_f16x2.hip, one-plane mode): R2DM_TEST_IO16 = 1 (x holds fp16), 2 (y and the
    // residual hold fp16) or 3 -- the caller passes tensors of that type behind the float pointers.  (Bit 2 alone: only the kernel selection
    // above -- the fp32 twin of a storage test.)  What the launchers refuse of it is refused here, before the weights are packed.
    const int io16 = test_io16() & 3;
    if (io16) {
        if (!((algo == ALGO_F16X2 && pieces == 1) || algo == ALGO_DIRECT || (algo == ALGO_P1F16 && pieces == 1)))
            return fail(1, "R2DM_TEST_IO16: this shape / mode runs on a kernel without fp16 storage");  // (never write a type the caller did not allocate)
        // proj_f16x2.hip: one fp16-storage instantiation -- fp16 on both sides, raw input, no residual (launch_proj_f16x2)
        if (algo == ALGO_P1F16 && (io16 != 3 || prologue != PRO_NONE || residual))
            return fail(1, "R2DM_TEST_IO16 = %d: the fp16-operand 1 x 1 convolution stores fp16 on both sides or on neither, and then takes no prologue and no residual", io16);
        // conv_direct.hip: the few-input kernel reads fp32 (the network input), the few-output kernel writes fp32 and reads fp16 two channels at a time
        if (algo == ALGO_DIRECT && (cout > 4 ? (io16 & 1) != 0 : (io16 & 2) != 0 || cin % 2 != 0))
            return fail(1, "R2DM_TEST_IO16 = %d: the direct kernels store fp16 on the side of the network's interior only", io16);
    }
    const float* wscale = nullptr;
    if (algo == ALGO_F16X2) {  // the range flag and the weight scale: behind the packed weights (r2dm_conv_packed_elems reserves 64 floats)
        float* tail = w_packed + conv_f16x2_packed_floats(cin, cout);
        HIP_TRY(hipMemsetAsync(tail, 0, sizeof(int), st));
        HIP_TRY(launch_pack_conv_f16x2(w, w_packed, cout, cin, (int*)tail, st, tail + 2, co_tile, px_rows));
        wscale = tail + 3;
    } else if (algo == ALGO_P1F16) {
        float* tail = w_packed + proj_f16x2_packed_floats(cin, cout);
        HIP_TRY(hipMemsetAsync(tail, 0, sizeof(int), st));
        HIP_TRY(launch_pack_proj_f16x2(w, w_packed, cout, cin, (int*)tail, st, tail + 2));
        wscale = tail + 3;
    } else {
        HIP_TRY(launch_pack_conv(w, w_packed, cout, cin, taps, co_tile, cin_pad, st, algo));
    }
    const long hw = (long)H * W;
    const Src src = ex.x1 ? Src{x, ex.x1, cin - ex.c1, ex.c1, (cin - ex.c1) * hw, ex.c1 * hw} : Src{x, nullptr, cin, 0, cin * hw, 0};
    ConvParams p = conv_params(src, w_packed, bias, y, (long)cout * H * W, B, H, W, cin, cin_pad, cout, taps, co_tile, algo, prologue);
    p.px_rows = px_rows;
    p.pieces = pieces;
    p.wscale = wscale;
    p.aff = (const float2*)aff;
    p.res = residual;
    p.res_bs = ex.res_broadcast ? 0 : (long)cout * H * W;
    p.scale = scale;
    p.range = ex.range;
    p.reverse = ex.reverse;
    if (ex.stat) conv_stat_sink(p, ex.stat, ex.stat_G, ex.stat_goff, ex.stat_cpg, conv_stat_slots(H, W));
    p.x16 = io16 & 1;  // (round 6: also the in / out convolutions -- bit 1 / bit 0 -- and, with both bits, the fp16-operand 1 x 1 convolution)
    p.y16 = (io16 >> 1) & 1;
    // perf probe (scripts/conv_phases.py): per-block s_memtime stamps into a caller-provided device buffer
    if (const char* e = getenv("R2DM_CONV_PROF_PTR")) p.prof = (unsigned long long*)strtoull(e, nullptr, 0);
    HIP_TRY(launch_conv(p, st));
    return 0;
}

int r2dm_conv2d_ring(const float* x, const float* w, const float* bias, float* w_packed, const float* aff,
                     int32_t prologue, const float* residual, const float* scale, float* y, int32_t B, int32_t cin,
                     int32_t cout, int32_t H, int32_t W, int32_t ksize, void* stream) {
    return conv2d_ring_impl(x, w, bias, w_packed, aff, prologue, residual, scale, y, B, cin, cout, H, W, ksize, stream, ConvExtras{});
}

int32_t r2dm_conv_stat_slots(int32_t H, int32_t W) { return conv_stat_slots(H, W); }

int r2dm_conv2d_ring_ex(const float* x, const float* x1, int32_t c1, const float* w, const float* bias, float* w_packed, const float* aff, int32_t prologue,
                        const float* residual, int32_t res_broadcast, const float* scale, float* y, double* stat, int32_t stat_G, int32_t stat_goff,
                        int32_t stat_cpg, int32_t* range, int32_t reverse, int32_t* chosen, int32_t B, int32_t cin, int32_t cout, int32_t H, int32_t W,
                        int32_t ksize, void* stream) {
    const ConvExtras ex{x1, c1, res_broadcast, stat, stat_G, stat_goff, stat_cpg, range, reverse, chosen};  // (the struct's order)
    return conv2d_ring_impl(x, w, bias, w_packed, aff, prologue, residual, scale, y, B, cin, cout, H, W, ksize, stream, ex);
}

size_t r2dm_group_norm_scratch_bytes(int32_t B, int32_t groups) { return (size_t)B * groups * 256 * (2 * sizeof(double) + sizeof(float)); }

// range (the _ex entries of the guard's producers): device int32[2] or NULL -- [1] takes the running maximum of the producer's bound as float bits,
// [0] (the packers' weight flag in the engine) is never written
int r2dm_group_norm_affine_ex(const float* x, const float* gamma, const float* beta, const float* ada, void* scratch, float* aff, float* stats, int32_t B,
                              int32_t C, int32_t H, int32_t W, int32_t groups, float eps, void* stream, int32_t* range) {
    if (!x || !scratch || !aff) return fail(1, "null argument");
    GNParams g{Src{x, nullptr, C, 0, (long)C * H * W, 0}, B, H, W, groups, eps, gamma, beta, ada, 2L * C,
               (double*)scratch, (float2*)aff, stats};
    g.partial_max = (float*)((double*)scratch + (size_t)B * groups * 256 * 2);
    g.range_flag = range;  // (M = the recorded max|x|: gn_partial_kernel's partial_max)
    HIP_TRY(launch_group_norm(g, (hipStream_t)stream));
    return 0;
}

int r2dm_group_norm_affine(const float* x, const float* gamma, const float* beta, const float* ada, void* scratch,
                           float* aff, float* stats, int32_t B, int32_t C, int32_t H, int32_t W, int32_t groups,
                           float eps, void* stream) {
    return r2dm_group_norm_affine_ex(x, gamma, beta, ada, scratch, aff, stats, B, C, H, W, groups, eps, stream, nullptr);
}

// ada_stride: floats between two samples' [scale(C) | shift(C)] rows -- the engine reads them out of the packed [B][ada_rows] projection buffer
int r2dm_group_norm_from_stats_strided(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, int64_t ada_stride, float* aff,
                                       float* stats, int32_t B, int32_t C, int32_t H, int32_t W, int32_t groups, float eps, void* stream, int32_t* range) {
    if (!stat || !aff) return fail(1, "null argument");
    if (B < 1 || slots < 1 || groups < 1 || C % groups) return fail(1, "group_norm_from_stats: %d slots, %d channels in %d groups", slots, C, groups);
    if (ada && ada_stride < 2L * C) return fail(1, "group_norm_from_stats: ada rows of %ld floats do not hold 2 x %d", (long)ada_stride, C);
    GNParams g{Src{nullptr, nullptr, C, 0, (long)C * H * W, 0}, B, H, W, groups, eps, gamma, beta, ada, (long)ada_stride, const_cast<double*>(stat), (float2*)aff, stats};
    g.range_flag = range;  // (no partial_max: the finalize kernel reads the sink alone, M = the square root of the largest slot energy)
    HIP_TRY(launch_group_norm_finalize(g, C, slots, (hipStream_t)stream));
    return 0;
}

int r2dm_group_norm_from_stats_ex(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, float* aff, float* stats,
                                  int32_t B, int32_t C, int32_t H, int32_t W, int32_t groups, float eps, void* stream, int32_t* range) {
    return r2dm_group_norm_from_stats_strided(stat, slots, gamma, beta, ada, 2L * C, aff, stats, B, C, H, W, groups, eps, stream, range);
}

int r2dm_group_norm_from_stats(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, float* aff, float* stats,
                               int32_t B, int32_t C, int32_t H, int32_t W, int32_t groups, float eps, void* stream) {
    return r2dm_group_norm_from_stats_ex(stat, slots, gamma, beta, ada, aff, stats, B, C, H, W, groups, eps, stream, nullptr);
}

int r2dm_affine_act(const float* x, const float* aff, float* y, int32_t B, int32_t C, int64_t hw, int32_t silu,
                    void* stream) {
    HIP_TRY(launch_gn_apply(x, (const float2*)aff, y, B, C, hw, silu, (hipStream_t)stream));
    return 0;
}

int r2dm_fir_down2(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    HIP_TRY(launch_fir_down2(x, (long)C * H * W, y, (long)C * (H / 2) * (W / 2), B, C, H, W, (hipStream_t)stream, nullptr, 0, test_io16() & 1, (test_io16() >> 1) & 1));
    return 0;
}

int32_t r2dm_fir_down2_stat_slots(int32_t C, int32_t G, int32_t H, int32_t W) {
    return fir_down2_stat_slots(C, G, H, W) ? conv_stat_slots(H / 2, W / 2) : 0;
}

int r2dm_fir_down2_stats(const float* x, float* y, double* stat, int32_t B, int32_t C, int32_t G, int32_t H, int32_t W, void* stream) {
    if (!stat || !fir_down2_stat_slots(C, G, H, W)) return fail(1, "fir_down2_stats: geometry without a statistics variant");
    HIP_TRY(launch_fir_down2(x, (long)C * H * W, y, (long)C * (H / 2) * (W / 2), B, C, H, W, (hipStream_t)stream, stat, G, test_io16() & 1, (test_io16() >> 1) & 1));
    return 0;
}

int r2dm_down_planes_ex(const float* x, float* planes, int32_t B, int32_t C, int32_t H, int32_t W, void* stream, int32_t* range) {
    if (!x || !planes) return fail(1, "null argument");
    if (B < 1 || C < 1 || !down_planes_supported(H, W)) return fail(1, "down_planes: needs height %% 4 == 0 and width %% 8 == 0 (>= 16)");
    HIP_TRY(launch_down_planes(x, (long)C * H * W, planes, 9L * C * (H / 2) * (W / 2), B, C, H, W, (hipStream_t)stream, range));
    return 0;
}

int r2dm_down_planes(const float* x, float* planes, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    return r2dm_down_planes_ex(x, planes, B, C, H, W, stream, nullptr);
}

int32_t r2dm_down_gemm_stat_slots(int32_t cin, int32_t cout, int32_t G, int32_t H, int32_t W) {
    if (H < 4 || W < 16 || !down_planes_supported(H, W) || !proj_f16x2_supported(9 * cin, cout, 1, H / 2, W / 2)) return 0;
    const int cpg = G > 0 && cout % G == 0 ? cout / G : 0;
    return cpg >= 8 && cpg <= 64 && !(cpg & (cpg - 1)) ? conv_stat_slots(H / 2, W / 2) : 0;
}

int r2dm_down_phase_planes_ex(const float* x, float* planes, int32_t B, int32_t C, int32_t H, int32_t W, void* stream, int32_t* range) {
    if (!x || !planes) return fail(1, "null argument");
    if (B < 1 || C < 1 || !down_phase_planes_supported(H, W)) return fail(1, "down_phase_planes: needs height %% 4 == 0 and width %% 8 == 0 (>= 16)");
    HIP_TRY(launch_down_phase_planes(x, (long)C * H * W, planes, down_phase_planes_floats(C, H, W), B, C, H, W, (hipStream_t)stream, range));
    return 0;
}

int r2dm_down_phase_planes(const float* x, float* planes, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    return r2dm_down_phase_planes_ex(x, planes, B, C, H, W, stream, nullptr);
}

int64_t r2dm_down_phase_planes_floats(int32_t C, int32_t H, int32_t W) {
    return C < 1 || !down_phase_planes_supported(H, W) ? 0 : down_phase_planes_floats(C, H, W);
}

// phase: the operand with every distinct plane stored once (r2dm_down_gemm) | all nine planes (r2dm_down_gemm_nine); `planes` is sized for nine either way
static int down_gemm_entry(const float* x, const float* w, const float* bias, float* w_packed, float* planes, float* y, double* stat, int32_t B, int32_t cin,
                           int32_t cout, int32_t G, int32_t H, int32_t W, void* stream, bool phase) {
    if (!x || !w || !bias || !w_packed || !planes || !y) return fail(1, "null argument");
    if (B < 1 || H < 4 || W < 16 || !down_planes_supported(H, W) || !proj_f16x2_supported(9 * cin, cout, 1, H / 2, W / 2))
        return fail(1, "down_gemm: needs cin %% 32 == 0, cout %% 64 == 0, height %% 8 == 0, width %% 128 == 0");
    if (stat && !r2dm_down_gemm_stat_slots(cin, cout, G, H, W)) return fail(1, "down_gemm: no statistics for %d groups of %d channels", G, cout);
    hipStream_t st = (hipStream_t)stream;
    // the range flag and the weight scale: behind the packed weights (the caller reserves 64 floats), as r2dm_conv2d_ring
    float* tail = w_packed + proj_f16x2_packed_floats(9 * cin, cout);
    HIP_TRY(hipMemsetAsync(tail, 0, sizeof(int), st));
    HIP_TRY(launch_pack_proj_f16x2(w, w_packed, cout, 9 * cin, (int*)tail, st, tail + 2, 9));
    const int Ho = H / 2, Wo = W / 2;
    if (phase) HIP_TRY(launch_down_phase_planes(x, (long)cin * H * W, planes, down_phase_planes_floats(cin, H, W), B, cin, H, W, st));
    else HIP_TRY(launch_down_planes(x, (long)cin * H * W, planes, 9L * cin * Ho * Wo, B, cin, H, W, st));
    const ConvParams p = down_gemm_params(planes, w_packed, bias, tail + 3, y, B, cin, cout, Ho, Wo, stat, G, phase);
    HIP_TRY(launch_proj_f16x2(p, st, phase ? DOWN_PHASE : DOWN_NINE));
    return 0;
}

int r2dm_down_gemm(const float* x, const float* w, const float* bias, float* w_packed, float* planes, float* y, double* stat, int32_t B, int32_t cin,
                   int32_t cout, int32_t G, int32_t H, int32_t W, void* stream) {
    return down_gemm_entry(x, w, bias, w_packed, planes, y, stat, B, cin, cout, G, H, W, stream, true);
}

int r2dm_down_gemm_nine(const float* x, const float* w, const float* bias, float* w_packed, float* planes, float* y, double* stat, int32_t B, int32_t cin,
                        int32_t cout, int32_t G, int32_t H, int32_t W, void* stream) {
    return down_gemm_entry(x, w, bias, w_packed, planes, y, stat, B, cin, cout, G, H, W, stream, false);
}

// (R2DM_TEST_IO16 and R2DM_FIR_UP_WIDE as for r2dm_fir_up2: launch_fir_up2 reads the second, the record is that of the STORED values)
int r2dm_fir_up2_ex(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream, int32_t* range) {
    HIP_TRY(launch_fir_up2(x, (long)C * H * W, y, (long)C * H * W * 4, B, C, H, W, (hipStream_t)stream, range, test_io16() & 1, (test_io16() >> 1) & 1));
    return 0;
}

int r2dm_fir_up2(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream) {
    return r2dm_fir_up2_ex(x, y, B, C, H, W, stream, nullptr);
}

int r2dm_attention(const float* qkv, float* out, int32_t B, int32_t C, int32_t heads, int32_t N, void* stream) {
    if (!attention_supported(C, heads, N)) return fail(1, "attention: unsupported shape C=%d heads=%d N=%d", C, heads, N);
    HIP_TRY(launch_attention(qkv, out, B, C, heads, N, (hipStream_t)stream, g_single_kernel_pieces >= 3 ? 0 : g_single_kernel_pieces));  // (per-op tests cover all three)
    return 0;
}

int r2dm_time_embedding(const float* cond, const float* freqs, const float* w1, const float* b1, const float* w2,
                        const float* b2, float* act, float* hidden, int32_t B, int32_t base, int32_t T, void* stream) {
    if (!cond || !freqs || !w1 || !b1 || !w2 || !b2 || !act || !hidden) return fail(1, "null argument");
    EmbedParams e{cond, freqs, w1, b1, w2, b2, act, hidden, B, base, T};
    HIP_TRY(launch_time_embedding(e, (hipStream_t)stream));
    return 0;
}

// (16-byte loads of act and w where T % 256 == 0: ada_proj_kernel)
int r2dm_ada_proj(const float* act, const float* w, const float* bias, float* out, int32_t B, int32_t T, int32_t rows, void* stream) {
    if (!act || !w || !bias || !out) return fail(1, "null argument");
    if (B < 1 || T < 1 || rows < 1) return fail(1, "ada_proj: batch %d, %d inputs, %d rows", B, T, rows);
    if (T % 256 == 0 && (((uintptr_t)act | (uintptr_t)w) & 15)) return fail(1, "ada_proj: act and w must be 16-byte aligned where T %% 256 == 0");
    HIP_TRY(launch_ada_proj(act, w, bias, out, B, T, rows, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
