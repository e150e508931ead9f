// Internal declarations shared by the engine's translation units (not part of the C ABI, include/r2dm_hip.h):
//   plan.hip        the blob layout: which packings every layer gets and where they live (build_plan, r2dm_blob_layout_hash)
//   forward.hip     the walk over the eight U-Net stages that enqueues the kernels (Ctx, run_forward)
//   engine.hip      the model's C ABI: create / bind / load / workspace / forward / range guard / profiling
//   ops_abi.hip     the stand-alone operators' entry points
//   kernel_abi.hip  the single-kernel test entries
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/r2dm_hip.h"
#include "common.h"

namespace r2dm {

// records the message r2dm_last_error returns to this thread (defined once, in engine.hip) and returns `code`
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return r2dm::fail(2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

constexpr size_t kAlign = 256;
inline size_t align_up(size_t v, size_t a = kAlign) { return (v + a - 1) / a * a; }

// ---- plan -----------------------------------------------------------------------------------
struct ConvLayer {
    int cin = 0, cout = 0, taps = 0, co_tile = 0, cin_pad = 0, algo = 0;
    int src_cin = 0, src_off = 0;  // packs input channels [src_off, src_off + cin) of a (cout, src_cin, k, k) tensor
    size_t w = 0, b = 0;  // blob offsets in floats
    // second packing of the same weights for ALGO_F16X2 (conv_f16x2.hip): the residual blocks' 3x3 convolutions, whose
    // input is GroupNorm-normalised; selected per launch by the handle's precision mode (r2dm_set_conv_pieces)
    bool f2 = false;
    int f2_cot = 64;  // output channels per tile of that packing: 64 or 128 (conv_f16x2_pick_co_tile)
    int f2_rows = 4;  // ... and its image rows: 4, or 8 (the one-accumulator 64 x 8 tile: its own packing, residual planes at their true scale)
    size_t w_f2 = 0, ws_f2 = 0;  // ws_*: two floats -- [0] max|w| (packer scratch), [1] inverse of the packer's power-of-two weight scale
    // ... and for ALGO_P1F16 (proj_f16x2.hip): the 1x1 projections of the attention block
    bool p1 = false;
    size_t w_p1 = 0, ws_p1 = 0;
    // ... and, for a stage's down-sampling 3x3 convolution, the (Cout, 9 Cin) matrix of the down-sampling GEMM (FIR first, then a 1x1 convolution over the nine
    // filtered planes at the output resolution: resample.hip down_planes_phase_kernel / down_planes_kernel + proj_f16x2.hip), columns (ky, kx, ci)
    bool dg = false;
    size_t w_dg = 0, ws_dg = 0;
    size_t packed_elems() const { return (size_t)conv_packed_floats(algo, cin, cout, taps, co_tile, cin_pad); }
};

struct ResLayer {
    int cin = 0, cout = 0;
    size_t g1 = 0, b1 = 0, scale = 0;
    int ada_row = 0;  // first row of this block's [scale|shift] projection in the packed matrix
    ConvLayer conv1, conv2, skip;
    bool has_skip = false;
};

struct AttnLayer {
    int C = 0;
    size_t gamma = 0, beta = 0, scale = 0;
    ConvLayer qkv, proj;
};

struct Stage {
    std::string name;
    int cin = 0, cout = 0;
    bool down = false, up = false, attn = false;
    ConvLayer dconv, uconv;
    bool out_tracked = false;  // the stage's last convolution records max|output| in the range flag (its consumer is the next
                               // stage's down-sampling convolution on the f16x2 path)
    // the 1x1 skip convolution of an up stage's first block reads the raw concatenation [previous up stage | down-path skip
    // tensor]: it runs on the fp16 matrix pipe (proj_f16x2.hip) if BOTH tensors' producers record max|output|
    bool track_final = false;     // whichever convolution produces the stage's output records max|output|
    bool skip_in_bounded = false;  // ... which every producer of this stage's input does
    std::vector<ResLayer> res;
    AttnLayer at;
};

enum SlotKind { SLOT_RAW, SLOT_CONV };
struct Slot {
    std::string key;
    int64_t numel;
    SlotKind kind;
    size_t off;  // destination offset in floats
    ConvLayer conv;  // for SLOT_CONV
};

}  // namespace r2dm

struct r2dm_handle {
    r2dm_config cfg;
    int device = 0;
    std::vector<r2dm::Slot> slots;
    size_t blob_floats = 0;
    float* blob = nullptr;
    r2dm::Stage stages[8];
    r2dm::ConvLayer in_conv, out_conv;
    // in_conv over cat([x, cenc]) = conv(x, W[:, :C]) + [conv(cenc, W[:, C:]) + bias]: the bracket is constant over steps
    // and batch (efficient_unet.py:278-281), computed once per weight load into `cmap` (Cout, H, W)
    r2dm::ConvLayer in_conv_c;
    size_t cmap = 0, zero_bias = 0;
    bool cmap_ready = false;
    // split of the fp32 operands of the convolutions on the matrix pipe (r2dm_set_conv_pieces): 2 = fp16 + scaled fp16
    // residual (ALGO_F16X2 / ALGO_P1F16) wherever a second packing exists, three bf16 pieces elsewhere; 3 = three bf16 pieces
    // everywhere; 1 = the kernels of mode 2 with the fp16 piece alone (one product per MAC: reduced precision, bulk sampling)
    int conv_pieces = 2;
    // R2DM_DOWN_GEMM (read once, at r2dm_create): 1 (default) = FIR first, then the GEMM over the phase planes (every distinct plane stored once: resample.hip
    // down_planes_phase_kernel); 9 = the same GEMM over all nine planes (down_planes_kernel: the A/B twin, bit-identical); 0 = the down stages keep Conv3x3 at the
    // finer resolution + fir_down2, as until round 6 (A/B, the parity test)
    int down_gemm = 1;
    bool plan_fits16 = false;  // every layer of levels 1 and 2 got a packing whose kernel has fp16 activation storage (build_plan; the mode's part: run_forward)
    bool f16_path() const { return conv_pieces != 3; }  // operands go through fp16: their range is guarded
    bool flags_fresh = false;  // the blob's range flags have been cleared since the last r2dm_bind_blob (first load does it)
    size_t range_flag = 0;  // blob slot (RANGE_SITES pairs of ints, ALGO_F16X2): [0] != 0: a weight outside the fp16 range; [2 k + 1]: float
                            // bits of the largest operand bound site k has recorded since the last r2dm_check_range.  A SITE is one guarded
                            // producer of a forward, in walk order (round 6: one pair per site instead of one for the whole forward, so that
                            // r2dm_range_sites can say WHICH layer ran how close to 65504 -- python -m r2dm_amd.check); site 0: the test hook
                            // and anything beyond the table.  Kernels only ever atomicMax `pair + 1`.
    static constexpr int RANGE_SITES = 256;
    std::vector<std::string> site_names;  // labels of the last real walk (index = site)
    // A handle that has run a cached walk (r2dm_unet_forward_cached) keys its sites by the producer's identity (layer + what it records) and gives a producer its
    // index when it first sees it: a shallow walk hands out fewer sites than a full one, and walk-order numbers would mix two layers' maxima in one slot.  A handle
    // that only ever runs the plain forward numbers in walk order, as ever.
    bool sites_keyed = false;
    float site_bounds[RANGE_SITES] = {};  // what the last r2dm_check_range read (before it reset the device copy)
    int sites_read = 0;
    size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, freqs = 0, cenc = 0, ada_w = 0, ada_b = 0;
    int ada_rows = 0;
    std::map<int, size_t> ws_cache;
    // optional in-stream timing of the dominant kernel class (r2dm_profile_*)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;  // pairs
    size_t prof_used = 0;
    double prof_flop = 0.0;
    std::vector<int> prof_cls;        // per bracketed launch: 0 = f16x2, 1 = bf16x3, 2 = fp32 MFMA / direct
    std::vector<double> prof_lflop;   // ... and its algorithmic flops

    void prof_reset() {
        prof_used = 0;
        prof_flop = 0.0;
        prof_cls.clear();
        prof_lflop.clear();
    }

    // the plan's builders (plan.hip): each reserves blob space and lists the state-dict tensor that fills it
    size_t take(size_t floats);
    size_t raw(const std::string& key, int64_t numel);
    void raw_at(const std::string& key, int64_t numel, size_t off);
    r2dm::ConvLayer conv_slice(const std::string& wkey, int src_cin, int src_off, int cin, int cout, int ksize, long px_batch, int H = 0, int W = 0);
    r2dm::ConvLayer conv(const std::string& wkey, const std::string& bkey, int cin, int cout, int ksize, long px_batch, int H = 0, int W = 0, bool down = false);
};

namespace r2dm {

extern int g_single_kernel_pieces;  // precision mode of the single-kernel entries (r2dm_set_conv_pieces(NULL, ...); kernel_abi.hip)

void build_plan(r2dm_handle* h);
// a layer's own packing (plan.hip): the tile and the input-channel padding of the kernel `algo` names, and whether that kernel writes fused statistics
int conv_base_co_tile(int algo, int cin, int cout, int taps, long px_batch);
int conv_base_cin_pad(int algo, int cin, int taps, int co_tile);
bool conv_emits_stats(int algo, int co_tile, int cout);
int check_config(const r2dm_config& c);

// ---- workspace arena -------------------------------------------------------------------------
struct Arena {
    char* base;
    size_t cap;
    bool dry;
    size_t peak = 0;
    struct Blk { size_t off, size; bool used; };
    std::vector<Blk> blks;
    bool overflow = false;

    void* alloc(size_t bytes) {
        bytes = align_up(bytes ? bytes : 1);
        for (size_t i = 0; i < blks.size(); ++i) {
            if (!blks[i].used && blks[i].size >= bytes) {
                if (blks[i].size > bytes) {
                    Blk rest{blks[i].off + bytes, blks[i].size - bytes, false};
                    blks[i].size = bytes;
                    blks.insert(blks.begin() + i + 1, rest);
                }
                blks[i].used = true;
                return base + blks[i].off;
            }
        }
        size_t end = blks.empty() ? 0 : blks.back().off + blks.back().size;
        if (!blks.empty() && !blks.back().used) {  // grow the trailing free block
            end = blks.back().off;
            blks.pop_back();
        }
        blks.push_back({end, bytes, true});
        if (end + bytes > peak) peak = end + bytes;
        if (!dry && end + bytes > cap) overflow = true;
        return base + end;
    }
    void release(const void* p) {
        const size_t off = (const char*)p - base;
        for (size_t i = 0; i < blks.size(); ++i) {
            if (blks[i].off == off && blks[i].used) {
                blks[i].used = false;
                if (i + 1 < blks.size() && !blks[i + 1].used) {
                    blks[i].size += blks[i + 1].size;
                    blks.erase(blks.begin() + i + 1);
                }
                if (i > 0 && !blks[i - 1].used) {
                    blks[i - 1].size += blks[i].size;
                    blks.erase(blks.begin() + i);
                }
                return;
            }
        }
    }
};

struct Tensor {
    float* p = nullptr;
    int C = 0, H = 0, W = 0;
    bool f16 = false;  // stored as fp16 (the one-plane mode's activation storage: ConvParams::x16 / y16); `p` stays typed float*
    long bs() const { return (long)C * H * W; }  // batch stride in ELEMENTS
    size_t bytes(int B) const { return (size_t)B * C * H * W * (f16 ? 2 : sizeof(float)); }
};

// The feature cache of a cached walk (r2dm_unet_forward_cached): the caller's buffer, laid out by cache_layout.
struct CacheWalk {
    void* buf = nullptr;
    int depth = 0;            // 1..3: stages [0, depth) and [8 - depth, 8) are live, stage 7 - depth produces the cached tensor
    int mode = 0;             // 1: store (the full walk), 2: reuse (the live stages only)
    double* drift = nullptr;  // store: (B, 2) sums of r2dm_cache_store, device
};
// [feature: (B, C, H, W) of stage 7 - depth's output, sized for fp32 | sink: the join's statistics slots ([B][G][slots][2] doubles; 0 bytes where the walk
// has no fused sink for that join) | partial: scratch of the drift reduction]
struct CacheLayout {
    int C = 0, H = 0, W = 0;
    size_t sink_off = 0, sink_bytes = 0, partial_off = 0, total = 0;
};
// whether a GroupNorm over C_total channels takes fused statistics, and its group size (Ctx::make_sink's rule: the epilogue reduction merges whole
// 8-channel blocks of one wave, so groups are 8, 16, 32 or 64 channels)
inline bool sink_shape(const r2dm_config& c, int C_total, int* cpg) {
    const int G = c.gn_num_groups;
    *cpg = C_total / G;
    return !(C_total % G || *cpg < 8 || *cpg > 64 || (*cpg & (*cpg - 1)));
}
inline CacheLayout cache_layout(const r2dm_handle* h, int B, int depth) {
    CacheLayout l;
    const r2dm::Stage& s = h->stages[7 - depth];
    l.C = s.cout;
    l.H = h->cfg.height >> (depth - 1);
    l.W = h->cfg.width >> (depth - 1);
    l.sink_off = align_up((size_t)B * l.C * l.H * l.W * sizeof(float));
    int cpg;
    if (sink_shape(h->cfg, h->stages[8 - depth].cin, &cpg)) l.sink_bytes = (size_t)B * h->cfg.gn_num_groups * conv_stat_slots(l.H, l.W) * 2 * sizeof(double);
    l.partial_off = l.sink_off + align_up(l.sink_bytes);
    l.total = l.partial_off + align_up((size_t)B * 512 * 2 * sizeof(double));
    return l;
}

// one forward over the arena: dry (Arena::dry) it only measures the workspace, else it enqueues every kernel on `st` (forward.hip);
// dry with a `listing`: one line per launch it would enqueue, the handle untouched (r2dm_forward_listing).  `cache`: a cached walk; `keyed`: the table that
// numbers the range sites by identity (null: the handle's own rule -- r2dm_handle::sites_keyed)
int run_forward(r2dm_handle* h, Arena& ar, const float* x, const float* cond, float* out, int B, hipStream_t st, std::string* listing = nullptr,
                const CacheWalk* cache = nullptr, std::vector<std::string>* keyed = nullptr);

// ConvParams with the fields every launch sets, in the struct's order; aff / res / scale are null, everything else keeps its default
inline ConvParams conv_params(const Src& x, const float* w, const float* bias, float* y, long y_bs, int B, int H, int W, int Cin, int CinPad, int Cout, int taps,
                              int co_tile, int algo, int prologue) {
    ConvParams p;
    p.x = x;
    p.w = w;
    p.bias = bias;
    p.aff = nullptr;
    p.res = nullptr;
    p.res_bs = 0;
    p.scale = nullptr;
    p.y = y;
    p.y_bs = y_bs;
    p.B = B;
    p.H = H;
    p.W = W;
    p.Cin = Cin;
    p.CinPad = CinPad;
    p.Cout = Cout;
    p.taps = taps;
    p.co_tile = co_tile;
    p.prologue = prologue;
    p.algo = algo;
    return p;
}

// where a convolution's epilogue leaves the GroupNorm statistics of its output: groups [goff, ...) of a sink of G groups, `slots` slots each
inline void conv_stat_sink(ConvParams& p, double* stat, int G, int goff, int cpg, int slots) {
    p.stat = stat;
    p.stat_G = G;
    p.stat_goff = goff;
    p.stat_cpg = cpg;
    p.stat_slots = slots;
}

// the down-sampling GEMM over launch_down_planes' output (B, 9 cin, Ho, Wo) or, `phase`, launch_down_phase_planes' (B, 2, cin, 2 Ho + 3, Wo + 4: launch it with
// DOWN_PHASE): w / wscale its packed matrix and weight scale; stat (may be null): GroupNorm statistics of y for G groups in the convolution epilogues' slot grid
inline ConvParams down_gemm_params(const float* planes, const float* w, const float* bias, const float* wscale, float* y, int B, int cin, int cout, int Ho,
                                   int Wo, double* stat, int G, bool phase) {
    const int K = 9 * cin;  // a 1x1 convolution over the nine filtered planes of every channel, at the output resolution
    const long bs = phase ? down_phase_planes_floats(cin, 2 * Ho, 2 * Wo) : (long)K * Ho * Wo;
    ConvParams p = conv_params(Src{planes, nullptr, K, 0, bs, 0}, w, bias, y, (long)cout * Ho * Wo, B, Ho, Wo, K, K, cout, 1, 64, ALGO_P1F16, PRO_NONE);
    p.pieces = 2;
    p.wscale = wscale;
    if (stat) conv_stat_sink(p, stat, G, 0, cout / G, conv_stat_slots(Ho, Wo));
    return p;
}

}  // namespace r2dm
