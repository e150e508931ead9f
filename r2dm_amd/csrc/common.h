// Shared declarations for libr2dm_hip.so (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace r2dm {

constexpr int kWave = 64;  // CDNA wavefront
constexpr float kInvSqrt2 = 0.70710678118654752440f;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// fp16 STORAGE of activations (the one-plane mode, round 5 / 6): four consecutive pixels of one channel are 8 bytes.  Pointers stay typed float*; an
// element index e of an fp16 tensor is the byte offset 2 e.  Conversions are RNE (v_cvt_pk_f16_f32) / exact (fp16 -> fp32).
using f16x2v = __attribute__((ext_vector_type(2))) _Float16;
__device__ __forceinline__ f32x4 f16x4_to_f32(unsigned long long r) {
    return f32x4{(float)__builtin_bit_cast(_Float16, (unsigned short)r), (float)__builtin_bit_cast(_Float16, (unsigned short)(r >> 16)),
                 (float)__builtin_bit_cast(_Float16, (unsigned short)(r >> 32)), (float)__builtin_bit_cast(_Float16, (unsigned short)(r >> 48))};
}
__device__ __forceinline__ unsigned long long f32_to_f16x4(const f32x4& v) {
    using f32x2v = __attribute__((ext_vector_type(2))) float;
    return (unsigned long long)__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{v[0], v[1]}, f16x2v)) |
           ((unsigned long long)__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{v[2], v[3]}, f16x2v)) << 32);
}
// four consecutive elements starting at element index `e` (a multiple of 4) of a tensor stored as fp32 (X16 = false) or fp16
template <bool X16>
__device__ __forceinline__ f32x4 load4(const float* base, long e) {
    if constexpr (X16) return f16x4_to_f32(*reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned short*>(base) + e));
    else return *reinterpret_cast<const f32x4*>(base + e);
}
template <bool X16>
__device__ __forceinline__ float load1(const float* base, long e) {
    if constexpr (X16) return (float)__builtin_bit_cast(_Float16, reinterpret_cast<const unsigned short*>(base)[e]);
    else return base[e];
}
// stores v (RNE for fp16) and returns the values AS STORED (what a consumer will read: statistics and range maxima are taken of those)
template <bool Y16>
__device__ __forceinline__ f32x4 store4(float* base, long e, const f32x4& v) {
    if constexpr (Y16) {
        const unsigned long long pk = f32_to_f16x4(v);
        *reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned short*>(base) + e) = pk;
        return f16x4_to_f32(pk);
    } else {
        *reinterpret_cast<f32x4*>(base + e) = v;
        return v;
    }
}

// A (B, C0+C1, H, W) activation that may live in two allocations (channel concat without a copy,
// reference efficient_unet.py:11-12,290-292).  Planes are H*W contiguous floats; `bs` is the batch
// stride in floats (0 = broadcast over the batch, used for the constant coordinate encoding).
struct Src {
    const float* p0;
    const float* p1;
    int c0, c1;
    long bs0, bs1;
    __host__ __device__ int channels() const { return c0 + c1; }
    __device__ __forceinline__ const float* plane(int b, int c, long hw) const {
        return c < c0 ? p0 + b * bs0 + (long)c * hw : p1 + b * bs1 + (long)(c - c0) * hw;
    }
};

__device__ __forceinline__ float silu_f(float v) {
    // x * sigmoid(x) on the transcendental unit: v_exp_f32 + v_rcp_f32 (1 ulp each).  Absolute error
    // <= ~2e-7*|v|, i.e. fp32-roundoff class like the convolution it feeds (parity budget ~1e-6).
#ifdef R2DM_ACCURATE_SILU
    return v / (1.0f + expf(-v));
#else
    return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
#endif
}

// XCD-aware bijective block remap (8 XCDs, block b is dispatched to XCD b % 8): logical ids that
// are neighbours (share input halo / weights) land on the same XCD's L2.
__host__ __device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

// ---- kernel launchers (each in its own .hip) ------------------------------------------

enum Prologue { PRO_NONE = 0, PRO_AFFINE = 1, PRO_AFFINE_SILU = 2 };
// ALGO_F32: fp32-input MFMA (conv_mfma.hip).  ALGO_BF16X3: fp32 operands split exactly into three bf16 pieces, six
// bf16 MFMA products per fp32 product, fp32 accumulation (conv_bf16x3.hip) -- same accuracy class, 2.7x fewer
// matrix-pipe cycles; needs 3x3, Cin % 16 == 0, Cout % 64 == 0.
// ALGO_DIRECT: Cout <= 4 (out_conv): HBM-bound, direct fp32 FMA convolution, weights kept OIHW (conv_direct.hip).
// ALGO_F16X2: fp32 operands split exactly to 22 bits into an fp16 piece and a 2^11-scaled fp16 residual, three fp16 MFMA
// products per fp32 product, two fp32 accumulators (conv_f16x2.hip): more accurate than either of the above on the
// matrix pipe (profiles/r02_f16x2_probe.txt) at half the products of ALGO_BF16X3, but operands must fit the fp16 range
// -- the engine uses it for GroupNorm-normalised inputs only, behind a range flag.
// ALGO_P1F16: the 1x1 convolutions around the attention core in the ALGO_F16X2 arithmetic (proj_f16x2.hip)
enum ConvAlgo { ALGO_F32 = 0, ALGO_BF16X3 = 1, ALGO_DIRECT = 2, ALGO_F16X2 = 3, ALGO_P1F16 = 4 };

struct ConvParams {
    Src x;               // input activation
    const float* w;      // packed weights [nCoT][CinPad][taps][CO_T]
    const float* bias;   // [Cout]
    const float2* aff;   // [B][Cin] (a, d): GroupNorm folded to x*a+d, or nullptr
    const float* res;    // residual added before scaling, Cout planes, or nullptr
    long res_bs;
    const float* scale;  // device scalar multiplied after the residual add, or nullptr
    float* y;            // output, Cout planes
    long y_bs;
    int B, H, W, Cin, CinPad, Cout;
    int taps;            // 9 or 1
    int co_tile;         // 32 / 64 / 128 (must match the packing)
    int px_rows = 4;     // ALGO_F16X2: image rows per pixel tile -- 4, or 8 with co_tile 64 (conv_f16x2.hip's one-accumulator "tall" tile; must match the packing)
    int prologue;        // Prologue
    int algo = ALGO_F32; // ConvAlgo (must match the packing of `w`)
    int pieces = 3;      // ALGO_BF16X3: bf16 pieces per fp32 operand (3 = exact split, 6 products; the 2-piece variant of
                         // round 1 is superseded by ALGO_F16X2 and no longer dispatched).  ALGO_F16X2 / ALGO_P1F16: 1 = the h plane
                         // alone, one fp16 product per MAC (the reduced-precision bulk mode); anything else = the split arithmetic
    int sign_shift = 0;  // ALGO_BF16X3 shallow kernel: accumulator sign flips every 2^sign_shift chunks (set by the launcher)
    // optional fused GroupNorm statistics of the OUTPUT (for the GroupNorm that consumes it): per (sample, group)
    // partial (sum, sum of squares) in fp64, one slot per (pixel tile, pixel wave): [B][stat_G][stat_slots][2]
    double* stat = nullptr;
    int stat_G = 0, stat_goff = 0, stat_cpg = 0, stat_slots = 0;
    // (the slots double as the fp16 range guard of the GroupNorm's consumers: every element of a slot is bounded by the
    // square root of the slot's sum of squares -- gn_finalize, norm.hip: data-driven and free for the producer)
    // optional device scalar multiplied into the matrix product before the bias: the inverse of the power-of-two scale the
    // fp16 packers apply to a layer's weights (f16x2.h: max|w| is brought to [2^9, 2^10) so that tiny weights keep 22 bits)
    const float* wscale = nullptr;
    // optional: range[1] takes the running maximum of |output| as float bits -- the engine asks for it when the consumer runs on
    // the fp16 matrix pipe with no GroupNorm in between (a down-sampling convolution; the attention core behind the qkv projection)
    int* range = nullptr;
    // walk the launch's tiles in descending order (conv_f16x2.hip): consecutive layers then alternate direction, so a layer starts on the
    // part of its input that its producer wrote LAST -- the part most likely still in the 256 MB Infinity Cache (level-1 tensors are 134 MB)
    int reverse = 0;
    // GroupNorm folded into its CONSUMER (conv_f16x2.hip, round 5): instead of `aff` the launch gets the producers' statistics slots
    // and the norm's parameters; every block's staging waves reduce the slots of the block's sample in gn_finalize_kernel's order
    // (norm.hip: bit-identical (a, d)) while the first pixels are on their way -- one launch less per GroupNorm.  Only where
    // conv_f16x2_fold_supported says so; `aff` must be nullptr then.
    const double* gn_partial = nullptr;  // [B][8][gn_stride][2] fp64 (sum, sum of squares); slots [0, gn_slots) are read
    int gn_slots = 0, gn_stride = 0, gn_cpg = 0;
    float gn_eps = 0.f;
    const float* gn_gamma = nullptr;     // [Cin] / nullptr
    const float* gn_beta = nullptr;
    const float* gn_ada = nullptr;       // [B][gn_ada_stride] rows = [scale(Cin) | shift(Cin)] (AdaGN) / nullptr
    long gn_ada_stride = 0;
    int* gn_range = nullptr;             // the engine's range flag (the bound gn_finalize would have recorded) / nullptr
    // fp16 STORAGE of activations (conv_f16x2.hip, the one-plane mode: round 5): x16 -- the input tensor(s) hold fp16; y16 -- the output and
    // the residual do.  Pointers stay typed float*, batch strides stay in ELEMENTS.
    int x16 = 0, y16 = 0;
    unsigned long long* prof = nullptr;  // optional [nblk][4] s_memtime stamps (perf probe; nullptr in production)
};
int conv_pick_algo(int Cin, int Cout, int taps);  // env R2DM_CONV_ALGO=f32 forces ALGO_F32 everywhere
long conv_packed_floats(int algo, int Cin, int Cout, int taps, int co_tile, int cin_pad);
int conv_pick_co_tile(int Cout, int taps, long pixels_times_batch);
int conv_cin_pad(int Cin, int taps, int co_tile);
hipError_t launch_conv(const ConvParams& p, hipStream_t s);
// src_cin / src_off: pack input channels [src_off, src_off + Cin) of a (Cout, src_cin, k, k) source (0 = whole tensor)
hipError_t launch_pack_conv(const float* w_oihw, float* dst, int Cout, int Cin, int taps, int co_tile,
                            int cin_pad, hipStream_t s, int algo = ALGO_F32, int src_cin = 0, int src_off = 0);
bool conv_bf16x3_supported(int Cin, int Cout, int taps);
bool conv_direct_supported(int Cout, int taps);
bool conv_few_in_supported(int Cin, int Cout, int taps, int H, int W);  // ALGO_DIRECT's second kernel (in_conv over the data channels)
hipError_t launch_conv_direct(const ConvParams& p, hipStream_t s);
long conv_bf16x3_packed_floats(int Cin, int Cout);
int conv_bf16x3_co_tile(int Cin, int Cout, long pixels_times_batch);
hipError_t launch_pack_conv_bf16x3(const float* w_oihw, float* dst, int Cout, int Cin, int co_tile, hipStream_t s);
hipError_t launch_conv_bf16x3(const ConvParams& p, hipStream_t s);
bool conv_f16x2_supported(int Cin, int Cout, int taps, int H, int W, int co_tile = 64, int px_rows = 4);  // tiles 64 x 4 | 128 x 4 | 64 x 8 (conv_f16x2.hip)
long conv_f16x2_packed_floats(int Cin, int Cout);
// One-accumulator tiles where the launch still has a tile per CU at the planned batch -- 128 channels x 4 rows, or 64 x 8 for layers with
// fewer than 128 output channels --, else 64 x 4 (two accumulators).  Returns the channels, *px_rows the rows (nullptr: 4-row tiles only);
// env R2DM_F2_CO_TILE = 64 | 128 | 64x8 forces one of them where the shape allows (experiments, per-kernel tests)
int conv_f16x2_pick_co_tile(int Cin, int Cout, int H, int W, long pixels_times_batch, int* px_rows = nullptr);
// range_flag (device int, may be nullptr): bit 0 is set if a weight does not fit the fp16 range
// wscale (device float[2], may be nullptr = unscaled): [0] scratch (max|w| as float bits), [1] <- the inverse of the power-of-two
// scale applied to the layer's weights (ConvParams::wscale points there)
hipError_t launch_pack_conv_f16x2(const float* w_oihw, float* dst, int Cout, int Cin, int* range_flag, hipStream_t s, float* wscale = nullptr, int co_tile = 64,
                                  int px_rows = 4);
hipError_t launch_weight_absmax(const float* w, long n, int* max_bits, hipStream_t s);  // max_bits <- float bits of max|w| (zeroed first)
hipError_t launch_conv_f16x2(const ConvParams& p, hipStream_t s);
// can this launch (shape, tile, batch: everything but the gn_* fields) take its GroupNorm folded -- 8 groups of 8 .. 64 channels, at
// most 4 x 256 statistics slots per group to read, every block's tiles inside ONE sample
bool conv_f16x2_fold_supported(const ConvParams& p, int groups, int slots);
bool proj_f16x2_supported(int Cin, int Cout, int taps, int H, int W);
long proj_f16x2_packed_floats(int Cin, int Cout);
// taps = 9: w is the OIHW tensor of a 3x3 convolution over Cin / 9 channels, packed as the (Cout, Cin) matrix of the down-sampling GEMM (column = tap * Cin / 9 + ci)
hipError_t launch_pack_proj_f16x2(const float* w_oi, float* dst, int Cout, int Cin, int* range_flag, hipStream_t s, float* wscale = nullptr, int taps = 1);
// down != DOWN_NONE: the down-sampling GEMM -- the bias is scaled by the FIR's row factor (7/8 on the first and last row); DOWN_NINE: x is launch_down_planes'
// output, DOWN_PHASE: launch_down_phase_planes' (x.bs0 = down_phase_planes_floats; Cin stays 9 x the convolution's input channels: the K order is the same)
enum DownOperand { DOWN_NONE = 0, DOWN_NINE = 1, DOWN_PHASE = 2 };
hipError_t launch_proj_f16x2(const ConvParams& p, hipStream_t s, int down = DOWN_NONE);

struct GNParams {
    Src x;
    int B, H, W, groups;
    float eps;
    const float* gamma;  // [C] or nullptr  (affine GroupNorm)
    const float* beta;
    const float* ada;    // [B][ada_stride] rows = [scale(C) | shift(C)] or nullptr (AdaGN)
    long ada_stride;
    double* partial;     // scratch [B][G][splits][2]
    float2* aff;         // out [B][C]
    float* stats;        // optional out [B][G][2] (mean, rstd) for tests, may be nullptr
    // optional device int[2]: [1] takes the running maximum (as float bits) of a bound |a| M + |d| on the normalised, affine-
    // transformed tensor, M >= max|x| taken from the DATA: the maximum gn_partial recorded (partial_max), or the square root of
    // the largest slot energy (fused statistics) -- the fp16-operand consumers need it below 65504 ([0]: weight flag of the packer)
    int* range_flag = nullptr;
    float* partial_max = nullptr;  // [B][G][splits]: largest |x| of every split (written by gn_partial), or nullptr
};
int gn_splits(int B, int groups, long group_elems);
int conv_stat_slots(int H, int W);  // slots per (sample, group) a convolution's fused statistics occupy
// finalize only: partial [B][G][splits][2] already filled (by a convolution epilogue)
hipError_t launch_group_norm_finalize(const GNParams& p, int C, int splits, hipStream_t s);
hipError_t launch_group_norm(const GNParams& p, hipStream_t s);
hipError_t launch_gn_apply(const float* x, const float2* aff, float* y, int B, int C, long hw, int silu,
                           hipStream_t s);

// stat != nullptr: the GroupNorm statistics of the OUTPUT (G groups) go to the convolution epilogues' slot grid
// ([B][G][conv_stat_slots(H / 2, W / 2)][2] doubles); only where fir_down2_stat_slots(C, G, H, W) != 0
hipError_t launch_fir_down2(const float* x, long xbs, float* y, long ybs, int B, int C, int H, int W,
                            hipStream_t s, double* stat = nullptr, int G = 0, int x16 = 0, int y16 = 0);  // x16 / y16: fp16 storage of the input / output (round 6)
int fir_down2_stat_slots(int C, int G, int H, int W);
// FIR-down BEFORE the stage's 3x3 convolution (resample.hip): a <- [B][9 C][H/2][W/2], the nine filtered planes per channel the stride-2 convolution reads
// (plane (ky 3 + kx) C + c); FIR(conv(x) + b) = the 1x1 convolution of `a` with the weights permuted to [Cout][(ky, kx, ci)] + b x row factor.
// range (optional): range[1] takes the running maximum of |a| as float bits.  Needs H % 4 == 0, W % 8 == 0.
bool down_planes_supported(int H, int W);
hipError_t launch_down_planes(const float* x, long xbs, float* a, long abs_, int B, int C, int H, int W, hipStream_t s, int* range = nullptr);
// ... the same operand with every distinct plane stored once (resample.hip down_planes_phase_kernel): a <- [B][phase E, O][C][H + 3 rows][W/2 + 4], per sample
// down_phase_planes_floats(C, H, W) floats -- 0.47 .. 0.53 of the nine planes; launch_proj_f16x2(p, s, DOWN_PHASE) maps the nine taps onto it
bool down_phase_planes_supported(int H, int W);
long down_phase_planes_floats(int C, int H, int W);
hipError_t launch_down_phase_planes(const float* x, long xbs, float* a, long abs_, int B, int C, int H, int W, hipStream_t s, int* range = nullptr);
// row of a channel's (Ho + Ho + 3)-row block that holds V[ky][i]: V[0] | V[1] | V[2][0], V[2][Ho - 2], V[2][Ho - 1]; every other V[2][i] is V[0][i + 1]
__host__ __device__ inline int down_phase_row(int ky, int i, int Ho) {
    return ky == 0 ? i : ky == 1 ? Ho + i : i == 0 ? 2 * Ho : i == Ho - 1 ? 2 * Ho + 2 : i == Ho - 2 ? 2 * Ho + 1 : i + 1;
}
hipError_t launch_fir_up2(const float* x, long xbs, float* y, long ybs, int B, int C, int H, int W,
                          hipStream_t s, int* range = nullptr, int x16 = 0, int y16 = 0);  // range[1]: running max |output| as float bits (may be nullptr)

// the feature cache's store (cache.hip): cached <- fresh bit for bit, (B, n) values of fp32 / fp16; sums[b] = {sum (fresh - old)^2, sum old^2} in float64;
// partial: 2 * cache_store_blocks(B, n) * B doubles (at most 2 * 512 * B).  Both tensors 16-byte aligned.
hipError_t launch_cache_store(const void* fresh, void* cached, int B, long n, int f16, double* partial, double* sums, hipStream_t s);
int cache_store_blocks(int B, long n);

// qkv: (B, 3C, N) channel-major [q | k | v]; out (B, C, N)
// planes: 0 = fp32-input MFMA, 2 = fp16 matrix pipe with split operands, 1 = fp16 matrix pipe, one product (attention.hip)
hipError_t launch_attention(const float* qkv, float* out, int B, int C, int heads, int N, hipStream_t s, int planes = 0);
bool attention_supported(int C, int heads, int N);

struct EmbedParams {
    const float* cond;  // [B]
    const float* freqs; // [base/2] sinusoid frequencies (host-precomputed)
    const float* w1;    // [T][base]
    const float* b1;
    const float* w2;    // [T][T]
    const float* b2;
    float* act;         // out [B][T] = SiLU(time embedding)
    float* hidden;      // scratch [B][T]
    int B, base, T;
};
hipError_t launch_time_embedding(const EmbedParams& p, hipStream_t s);
// out[b][r] = dot(act[b], w[r]) + bias[r]   for all AdaGN projections at once
hipError_t launch_ada_proj(const float* act, const float* w, const float* bias, float* out, int B, int T,
                           int rows, hipStream_t s);

// ---- sampler steps (posterior.hip, latent.hip) ----
enum { OBJ_EPS = 0, OBJ_V = 1, OBJ_X0 = 2 };  // what the denoiser predicts

// launch shape of the kernels that stream B samples of per_sample floats in 16-byte quads, grid-stride: 256 threads, at most 1024 blocks a sample
inline dim3 quad_grid(int B, long per_sample) {
    const long bx = (per_sample / 4 + 255) / 256;
    return dim3((unsigned)(bx < 1 ? 1 : bx > 1024 ? 1024 : bx), (unsigned)B);
}

struct PosteriorParams {
    const float* x_t;
    const float* pred;
    const float* noise;  // nullptr for mode 3 (discrete DDIM, eta = 0), which reads none
    const float* coef;   // [B][8]
    float* x_s;
    int B;
    long per_sample;
    int mode, objective;
    float clip;  // < 0: no clamping
};
hipError_t launch_posterior(const PosteriorParams& p, hipStream_t s);
// the same step with the measurement written over the x_0 estimate: x0 = mask * known + (1 - mask) * x0 (continuous-time modes 0 / 1)
hipError_t launch_posterior_known(const PosteriorParams& p, const float* known, const float* mask, int channels, int mask_c,
                                  hipStream_t s);
// DPM-Solver++(2M) update: x_s = c_x x_t + c_0 x0 [+ c_1 x0_prev] with x0 the clamped estimate of the posterior step, also written out;
// coef [B][8] = (alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0).  x0_prev null: the first-order row.  x0 may be x0_prev's buffer.
// (launch_dpm_step is launch_dpm_step_known without noise and measurement)
struct DpmParams {
    const float* x_t;
    const float* pred;
    const float* x0_prev;  // may be nullptr
    const float* coef;
    float* x_s;
    float* x0;
    int B;
    long per_sample;
    int objective;
    float clip;  // < 0: no clamping
};
hipError_t launch_dpm_step(const DpmParams& p, hipStream_t s);
// the same update with coef[5] = c_z: x0 = mask * known + (1 - mask) * x0 before it (known, mask: both or neither), + c_z * noise behind it (noise may be nullptr)
hipError_t launch_dpm_step_known(const DpmParams& p, const float* noise, const float* known, const float* mask, int channels, int mask_c,
                                 hipStream_t s);
// RePaint (reference continuous_time.py:169-190,287-303): forward re-noising and known/unknown blend
hipError_t launch_repaint_blend(const float* known, const float* noise, const float* unknown, const float* mask,
                                const float* coef, float* out, int B, long per_sample, int channels, int mask_c,
                                hipStream_t s);
hipError_t launch_q_step(const float* x, const float* noise, const float* coef, float* out, int B, long per_sample,
                         hipStream_t s);
// denoising loss (reference base.py:122-139): per-(sample, channel) sums of criterion(prediction - target) * mask and the mask's own sum, in float64
size_t diffusion_loss_scratch_bytes(int B, int C, long plane);
hipError_t launch_diffusion_loss(const float* pred, const float* x_0, const float* noise, const float* mask, int mask_c, const float* coef,
                                 int objective, int criterion, int B, int C, long plane, void* scratch, double* num, double* den, hipStream_t s);
// latent space (latent.hip): the DDIM transfer x_t -> x_u with coef (B,4) = (alpha_t, sigma_t, alpha_u, sigma_u), and spherical interpolation at K
// host weights -> out (K,B,per_sample), coef64 (K,B,2)
hipError_t launch_ddim_transfer(const float* x_t, const float* pred, const float* coef, float* x_u, int B, long per_sample, int objective,
                                hipStream_t s);
constexpr int kSlerpMaxWeights = 64;  // weights of one r2dm_slerp call (they travel as a kernel argument)
size_t slerp_scratch_bytes(int B, long per_sample);
hipError_t launch_slerp(const float* a, const float* b, const float* weights, int K, float* out, double* coef64, int B, long per_sample,
                        void* scratch, hipStream_t s);

// (B,2,H,W) in [-1,1] -> (B,5,H,W) [depth, x, y, z, reflectance]  (reference sample_and_save.py:52-57)
hipError_t launch_lidar_postprocess(const float* x, const float* angles, float* y, int B, int H, int W,
                                    float min_depth, float max_depth, hipStream_t s, int depth_format = 0);  // 0 log_depth, 1 inverse_depth, 2 depth

// BEV metrics of evaluate.py (metrics.hip): histograms (layout 0: (B,5,H,W) samples, 1: (B,N,3) clouds), their batch sum, the MMD's three means
hipError_t launch_bev_histogram(const float* src, int layout, const float* edges, int32_t* hist, int64_t* sum, int B, long n, int bins,
                                float min_d, float max_d, float img_min, float img_max, hipStream_t s);
hipError_t launch_bev_hist_sum(const void* hist, int is_int32, int64_t* sum, long batch, long cells, hipStream_t s);
size_t mmd_scratch_bytes(int np, int nq);
hipError_t launch_bev_mmd(const float* P, const float* Q, int np, int nq, long D, double sigma, void* scratch, double* out, hipStream_t s);

// distribution metrics of feature sets (metrics.hip): fp64 mean / unbiased covariance; the polynomial-kernel MMD's three sums per subset
hipError_t launch_feature_moments(const float* f, long n, int D, double* mean, double* cov, hipStream_t s);
size_t poly_mmd_scratch_bytes(int subsets, int m);
hipError_t launch_poly_mmd(const float* X, const float* Y, const long long* ix, const long long* iy, int subsets, int m, int D, void* scratch,
                           double* out, hipStream_t s);

// k-NN manifold primitives of feature sets (features.hip): per row of x the k-th smallest / smallest (and its column) squared distance to the
// admissible rows of y and the number of y's balls it falls in, fp64, Gram term on the fp64 matrix pipe; the launch it picks for (m, n)
void feature_knn_launch_shape(long m, long n, int* row_tiles, int* splits);
size_t feature_knn_scratch_bytes(long m, long n, int k);
hipError_t launch_feature_knn(const float* x, long m, const float* y, long n, int dim, int same, int k, const double* y_radius2, double* kth2,
                              double* min2, int* argmin, int* count, void* scratch, long long* status, hipStream_t s);

// Fragment-order weight packing of the split arithmetic (f16x2.h) for the kernels that read their A operand straight from global memory -- PointNet's
// layers 2 and 3, every RangeNet layer (the kernel is in rangenet.hip): (Cout, taps, Cin) fp32 -> [chunk of 32 rows][tap][k-step of 16][plane h / l][lane]
// [8 halves], Cout padded to 32 and Cin to 16 with zeros, scaled by a power of two; wscale[0] <- bits of max|w|, [1] <- the inverse scale;
// *flag |= PACK_FLAG_WEIGHT for a weight that is not finite.  dst holds ceil(Cout / 32) taps ceil(Cin / 16) 2048 bytes.
constexpr int PACK_FLAG_WEIGHT = 4;
hipError_t launch_pack_frag_f16x2(const float* w, int Cout, int Cin, int taps, void* dst, float* wscale, int* flag, hipStream_t s);

// PointNet feature extractor of the FPD (pointnet.hip): weight packing, the fused trunk (layout 0 (B,5,H,W) samples, 1 (B,N,3), 2 (B,3,N)), the per-cloud MLPs
hipError_t launch_pointnet_pack(const float* w, int Cout, int Cin, void* dst, float* wscale, int* flag, hipStream_t s);
size_t pointnet_scratch_bytes(int B);
hipError_t launch_pointnet_trunk(const float* src, int layout, int B, long n, const float* trans, float img_min, float img_max, float divisor,
                                 const float* w1b, const void* w2p, const float* w2inv, const float* b2, const void* w3p, void* scratch, int* flag,
                                 hipStream_t s);
hipError_t launch_pointnet_head(const void* scratch, const float* w3inv, const float* b3, int stn, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* bo, int kout, float* out, int B, hipStream_t s);

// RangeNet extractor of the FRD and the segmentation (rangenet.hip): weight packing, the implicit-GEMM convolution of every layer kind, the label argmax
size_t rangenet_packed_bytes(int Cout, int Cin, int taps);
hipError_t launch_rangenet_pack(const float* w, int Cout, int Cin, int taps, void* dst, float* wscale, int* flag, hipStream_t s);
hipError_t launch_rangenet_conv(const float* in, const float* mask, const float* norm, float lo, float hi, const void* wp, const float* winv,
                                const float* bias, const float* add, const float* add2, float* out, int B, int Cin, int H, int Win, int Cout, int kind,
                                float slope, int* flag, hipStream_t s);
hipError_t launch_rangenet_argmax(const float* logits, long long* labels, int B, int C, long hw, hipStream_t s);

// post-processing of the labels (postproc.hip): the kNN vote of RangeNet++ and one mean-field iteration of the CRF-RNN, each one launch
bool postproc_window_supported(int kh, int kw);
hipError_t launch_knn_vote(const float* depth, const long long* label, const float* weight, long long* out, int B, int H, int W, int kh, int kw, int k,
                           int classes, float cutoff, int* flag, hipStream_t s);
hipError_t launch_crf_iter(const float* q_in, const float* unary, const float* xyz, const float* mask, const float* params, float* q_out, int B, int N,
                           int H, int W, int kh, int kw, int uniform_beta, hipStream_t s);

// completion metrics (completion.hip): per-sample error sums over the inpainted pixels, the confusion matrix of two label images (counts and *bad are
// zeroed by the call), the nearest / linear beam interpolation baselines (mode 0 / 1)
size_t completion_error_scratch_bytes(int B, long plane);
hipError_t launch_completion_error(const float* pred, const float* target, const float* known, float lo, float hi, int B, long plane, void* scratch,
                                   double* out, hipStream_t s);
hipError_t launch_confusion_matrix(const long long* pred, const long long* target, const float* mask, int B, long n, int classes, long long* counts,
                                   long long* bad, hipStream_t s);
hipError_t launch_fill_beams(const float* x, const unsigned char* rows, float* out, int B, int C, int H, int W, float nodata, int mode, hipStream_t s);
// ... and K completions of a scan scored as an ensemble: raw (B,13), member (B,2,K), rank (B,K+1) (zeroed by the call), maps (B,8,plane) or null
size_t ensemble_score_scratch_bytes(int B, int K, long plane);
hipError_t launch_ensemble_score(const float* samples, const float* target, const float* known, float lo, float hi, int B, int K, long plane,
                                 void* scratch, double* raw, double* member, long long* rank, float* maps, hipStream_t s);
// ... and its coherence across pixels: counts (B,2), dist (B,2,K+1,K+1) or null, vario (B,2,offsets,4) or null; offsets_hw (offsets,2) on the host
size_t ensemble_coherence_scratch_bytes(int B, int K, long plane, int offsets);
hipError_t launch_ensemble_coherence(const float* samples, const float* target, const float* known, float lo, float hi, int B, int K, int H, int W,
                                     const int* offsets_hw, int offsets, void* scratch, double* counts, double* dist, double* vario, hipStream_t s);

// geometry metrics (geometry.hip): nearest neighbours of P pairs of ragged clouds in both directions -- optional per-point d^2 / index, always
// sums (P,8) = [sum d^2, sum d, #{d <= tau}] a -> b, the same b -> a, |a|, |b|; status[2] = non-finite points met, pairs that do not check out
size_t nn_pairs_scratch_bytes(long P, long max_points);
long nn_pairs_chunks(long max_points);
hipError_t launch_nn_pairs(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b, long clouds_b,
                           long total_b, const long long* pairs, long P, long max_points, double tau, float* d2_ab, int* idx_ab,
                           const long long* out_ab, float* d2_ba, int* idx_ba, const long long* out_ba, void* scratch, double* sums,
                           long long* status, hipStream_t s);

// voxel occupancy (voxel.hip): G groups of one target cloud (from b) and K member clouds (from a) at S voxel sizes (HOST floats) -- a hash set of
// voxel keys per (group, size) with one membership bit per cloud; member_out (G,S,K,2) = |V(M_k)|, |V(M_k) n V(T)|, hist_out (G,S,2,K+1) =
// #{voxels: in the target or not, in c members}; status[4] = non-finite points, points outside the grid, groups that do not check out, inserts
// that found the table full
long voxel_capacity(long max_group_points);
bool voxel_geometry_ok(long G, long S, long max_group_points);
size_t voxel_occupancy_scratch_bytes(long G, long S, long max_group_points);
hipError_t launch_voxel_occupancy(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b,
                                  long clouds_b, long total_b, const long long* members, const long long* targets, long G, long K, const float* sizes,
                                  long S, long max_group_points, void* scratch, long long* member_out, long long* hist_out, long long* status,
                                  hipStream_t s);

// earth mover's distance (emd.hip): a forward auction per pair of equally sized clouds -- out (P,4) = emd, lower, rounds, converged; optional
// assignment / prices (P, max_points); scratch = one code per pair; status[5] = pairs ended as bad pair, unequal counts, non-finite, eps below
// its floor, round cap
long emd_max_points();
size_t emd_pairs_scratch_bytes(long P);
hipError_t launch_emd_pairs(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b, long clouds_b,
                            long total_b, const long long* pairs, long P, long max_points, double eps, long long max_rounds, int* assignment,
                            float* prices, double* out, void* scratch, long long* status, hipStream_t s);

// rendering of generate.py (render.hip): colour maps, the bilinear splat with 64-bit fixed-point accumulators, the fused frame renderer
hipError_t launch_colorize(const float* x, const float* lut, uint8_t* out, long B, long hw, hipStream_t s);
size_t rasterize_scratch_bytes(int B, int C, int H, int W);
// ratio 0: out (B,C,H,W) sums; 1 (C = 4): out (B,3,H,W) = sum_c / (sum_3 + 1e-8)
hipError_t launch_rasterize(const float* coords, const float* values, float* out, int B, long N, int C, int H, int W, void* scratch, int ratio,
                            hipStream_t s);
// Rt: 12 HOST floats, R row-major then t
hipError_t launch_project_points(const float* points, const float* colors, const float* Rt, float focal, int size, float* uv, float* vals, long n,
                                 hipStream_t s);
size_t render_frames_scratch_bytes(int frames, int size);
hipError_t launch_render_frames(const float* x, const float* trig, const float* turbo, const float* viridis, float* img, float* bev, long N, int H, int W,
                                int size, float min_depth, float max_depth, const float* Rt, float focal, void* scratch, size_t scratch_bytes,
                                hipStream_t s);
// estimate_surface_normal and train.py's log_images view (render.hip): nullptr if (B, H, W, d, mode) can be launched, else what is wrong with them
const char* surface_normals_error(long B, int H, int W, int d, int mode);
hipError_t launch_surface_normals(const float* xyz, float* normals, int B, int H, int W, int d, int mode, hipStream_t s);
hipError_t launch_normal_frames(const float* metric, const float* trig, float* colors, float* bev, long N, int H, int W, int size, float min_depth,
                                float max_depth, int d, int mode, const float* Rt, float focal, void* scratch, size_t scratch_bytes, hipStream_t s);

// raw scans -> range images (projection.hip): offsets are B + 1 HOST values (validated by the caller), Wo <= W the written width
size_t project_scratch_bytes(long long total, int B, int H, int W, int unfold);
hipError_t launch_project_scans(const float* points, const long long* offsets, float* out, int B, int H, int W, int Wo, int unfold, float min_depth,
                                float max_depth, int apply_mask, int layout, void* scratch, hipStream_t s);

// range images -> point clouds (pointcloud.hip): layout 0 (B,2,H,W) model samples, 1 (B,5,H,W) post-processed; row_start nullptr = image order
size_t unproject_scratch_bytes(int B, int H, int W);
hipError_t launch_unproject(const float* src, int layout, const float* angles, const int* row_start, float* points, int* index, long long* offsets,
                            int B, int H, int W, float min_depth, float max_depth, int depth_format, float keep_min, float keep_max, void* scratch,
                            hipStream_t s);

}  // namespace r2dm
