// K3f: 1x1 convolution (the attention block's qkv and output projections) on the fp16 matrix pipe with exactly split fp32
// operands -- the arithmetic of conv_f16x2.hip (v = h + 2^-11 l, three v_mfma_f32_32x32x16_f16 per 16 k-values, two fp32
// accumulators), as a plain LDS-tiled GEMM:  Y[b][co][px] = sum_ci W[co][ci] f(X[b][ci][px]) + bias (+ residual) (* scale).
//
// Reference: nn.MultiheadAttention's in_proj / out_proj inside SelfAttentionBlock (/root/reference/models/efficient_unet.py:
// 23-53); f = the folded GroupNorm affine for the qkv projection (PRO_AFFINE), identity for the output projection.
// On the fp32-input MFMA (conv_mfma.hip) these four launches ran at 23-86 % of a 157 TF/s peak: 0.24 ms per step for 2 % of
// the FLOPs; with a third of the matrix-pipe time per product they are bound by their own staging instead.
//
// Block = 256 threads = 4 waves, tile = 64 output channels x 256 pixels (4 rows x 64 columns: the tile geometry of the other
// convolution kernels, so conv_epilogue_wide and the GroupNorm-statistics slot grid apply unchanged); a wave owns 64 channels
// x 64 pixels (MR = NR = 2).  K loop in chunks of 32 input channels: every thread loads 8 channels x 4 pixels, applies the
// affine, splits and writes [pixel][32 ch] fp16 rows (h and l planes) to LDS; the weights come pre-split ([co tile][chunk]
// [plane][co][32 ch], pack_proj_f16x2_kernel).  The next chunk's global loads are in flight during the current chunk's MFMAs;
// two blocks per CU overlap one block's staging with the other's products.  (This is the kernel's wide shape; where Cout is a
// multiple of 256 the same kernel runs in its TALL shape, 256 channels x 64 pixels per block: p1::Shape below.)
// Range: as conv_f16x2.hip -- MODE.FP16_OVFL, and the engine only routes a projection here whose input is GroupNorm-
// normalised (gn_finalize's bound) or the attention core's output (|o| <= max|v|, tracked by the qkv epilogue).
#include "common.h"
#include "conv_bf16x3.h"
#include "conv_epilogue.h"
#include "f16x2.h"
#include <stdlib.h>
#include <type_traits>

namespace r2dm {

namespace p1 {
using namespace x3;  // CO_T 64, TH 4, TW 64, MR 2, NR 2
constexpr int CKP = 32;                  // input channels per chunk
constexpr int ROWB = CKP * 2 + 16;       // bytes per LDS row (32 fp16 + 16 bytes of padding)
constexpr int WCH = 2 * CO_T * CKP * 2;  // bytes of one (co tile, chunk) in the packed weights: planes h, l
constexpr int COB = 4 * CO_T;            // output channels per block of the tall shape: launch_proj_f16x2 takes it for Cout % COB == 0
using f32x4u = float __attribute__((ext_vector_type(4), aligned(4)));
// The two block shapes of the one kernel.  Either way a block is 256 threads = 4 waves, a wave owns 64 channels x 64 pixels and a staging
// thread 8 channels of the chunk; what the shape decides follows from the number of 64-channel weight tiles:
//   wide (the header's tile):  1 weight tile,  64 channels x 256 pixels (4 rows x 64 columns), 4 consecutive pixels per thread, the wave index picks the pixels
//   TALL:                      4 weight tiles, 256 channels x one 64-pixel row of that tile,   1 pixel per thread,              the wave index picks the channels
template <bool TALL>
struct Shape {
    static constexpr int WT = TALL ? 4 : 1;            // 64-channel weight tiles a block copies per chunk
    static constexpr int CO = WT * CO_T;               // output channels per block
    static constexpr int PPT = TALL ? 1 : 4;           // pixels per staging thread
    static constexpr int PX = 64 * PPT;                // pixels per block
    static constexpr int XPL = PX * ROWB;              // bytes per x plane
    static constexpr int WPL = CO * ROWB;              // bytes per weight plane
    static constexpr int PATCH0 = 2 * XPL + 2 * WPL;   // 51 200 either way
    static constexpr int LDS = PATCH0 + 4 * 1024;      // 55 296: two blocks per CU
    using xvec = std::conditional_t<TALL, float, f32x4>;    // a staging thread's pixels of one channel (a plain float, not a 1-vector: the compiler
    using xvecu = std::conditional_t<TALL, float, f32x4u>;  // addresses the two differently); xvecu: the same at 4-byte alignment (PHP's column shift)
};
__device__ __forceinline__ float pixel(float v, int) { return v; }  // pixel e of an xvec
__device__ __forceinline__ float pixel(f32x4 v, int e) { return v[e]; }
}  // namespace p1

// TALL shapes (Cout a multiple of 256: the attention projections, u_block4's skip, the deeper down-sampling GEMMs) -- round 3.
// With 64-channel output tiles the qkv projection (512 -> 1536 over 8192 tokens: a 1536 x 8192 x 512 GEMM) re-stages --
// loads, normalises, splits -- every pixel 24 times and runs at a fifth of what its MFMAs need (73 us; per-launch table in
// profiles/r03_launch_overhead.txt).  A tall block is 256 output channels x ONE 64-pixel row of the 4 x 64 pixel tile: the four waves
// take 64 channels each over the same pixels, a chunk's x tile is 64 pixels x 32 channels (8 values per thread instead of 32),
// the weights (pre-split, straight copies) 4 x 8 KB.  Same packing, same arithmetic, same epilogue and statistics slots (slot =
// tile x 4 + row: each written once, by the block that owns the row); bit-identical output.  What it bought (j124): the three
// plain-input launches 75 -> 67 us, the two GroupNorm-input ones 98 -> 94 us, -0.3 % on the step -- the transform was NOT what bounds
// these products: either tiling moves ~490 MB from L2 into LDS per qkv launch (a 64 x 256 and a 256 x 64 block tile have the same
// perimeter); the lever left is a larger block tile (8 waves), not taken.
// NPLK = operand planes in use: 2 = the split arithmetic (parity path), 1 = the h plane alone: one fp16 product per MAC, the
// reduced-precision bulk mode (conv_f16x2.hip); the l planes are then neither written nor read.
// IOM (wide shape only): fp16 storage of the input / output tensors, below.
// FIRB: the bias takes the FIR's row factor (conv_epilogue.h) -- the down-sampling GEMM over the nine filtered planes of resample.hip's down_planes_kernel
// PHP (with FIRB): x is the phase layout of down_planes_phase_kernel -- [phase E, O][Cin / 9][2 H + 3 rows][W + 4].  A 32-value chunk lies inside one tap (ky, kx)
// (Cin / 9 is a multiple of 32), so per chunk the loader picks the phase (kx = 1: O), the row (down_phase_row) and the column shift (kx = 0: one to the left --
// 4-byte aligned quads in the wide shape, free with the tall shape's one pixel per thread); same values in the same K order as the nine planes: bit-identical output.
// Four things are written per shape (TALL ? ... : ...) where one expression would do: the pixel offset, the weight unit of store_chunk, the x fragment
// rows, and a thread's pixels as float | f32x4.  The compiler's address arithmetic and register allocation follow the spelling, and with these each of the 13
// instantiations is instruction for instruction what it was when the two shapes were two kernels (profiles/proj_unify.txt).
template <bool TALL, int PRO, int NPLK, int IOM = 0, bool FIRB = false, bool PHP = false>
__global__ __launch_bounds__(256, 2) void proj_f16x2_kernel(const ConvParams p) {
    static_assert(!TALL || IOM == 0, "fp16 storage exists for the 64-channel block only");
    constexpr bool X16 = (IOM & 1) != 0, Y16 = (IOM & 2) != 0;  // (round 6) fp16 storage of the input tensor(s) / of the output (+ residual): the one-plane mode's skip convolutions
    using namespace p1;
    using S = Shape<TALL>;
    constexpr int PPT = S::PPT, XPL = S::XPL, WPL = S::WPL;
    using xvec = typename S::xvec;
    using gcx = const xvec __attribute__((address_space(1)))*;
    using gcxu = const typename S::xvecu __attribute__((address_space(1)))*;
    using gcf4 = const f32x4 __attribute__((address_space(1)))*;
    using gcu4 = const u32x4 __attribute__((address_space(1)))*;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f16_saturate_mode();
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W, HW = H * W;
    const int nTw = W / TW, nTh = H / TH, nCoB = p.Cout / S::CO, nchunks = p.Cin / CKP;
    int L = xcd_remap(blockIdx.x, gridDim.x);
    if (p.reverse) L = (int)gridDim.x - 1 - L;  // (round 6: against the walk of the convolution that read the same tensor last -- Infinity Cache)
    const int cob = L % nCoB;  // (fastest: the tall blocks that share a pixel row follow each other)
    L /= nCoB;
    int row = 0;  // TALL: the block's row of the tile
    if constexpr (TALL) {
        row = L % TH;
        L /= TH;
    }
    const int tw = L % nTw;
    L /= nTw;
    const int th = L % nTh;
    const int b = L / nTh;

    // staging map: thread -> PPT consecutive pixels (q: a quad of the tile, row q / 16, column 4 (q % 16) | TALL: pixel q of the block's row; 64 consecutive
    // lanes = 64 consecutive quads | pixels) of 8 channels (group cg) of the chunk
    const int q = tid & 63, cg = tid >> 6;
    const int poff = TALL ? (th * TH + row) * W + tw * TW + q : (th * TH + (q >> 4)) * W + tw * TW + (q & 15) * 4;
    const float* xb0 = p.x.p0 + b * p.x.bs0;
    const float* xb1 = p.x.p1 ? p.x.p1 + b * p.x.bs1 : p.x.p0;
    const int c0 = p.x.p1 ? p.x.c0 : p.Cin;  // (a chunk group of 8 never straddles the seam: launcher)
    const float* affb = PRO != PRO_NONE ? reinterpret_cast<const float*>(p.aff) + (size_t)b * p.Cin * 2 : nullptr;
    const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(p.w) + (size_t)(cob * S::WT) * nchunks * WCH;
    // (PHP) this thread's pixels in the rows holding V[ky][their image row], the channel stride, and the tap / first channel of the next chunk to load
    const int cin1 = p.Cin / 9, pchan = (2 * H + 3) * (W + 4);
    const int pcol = 4 + tw * TW + (TALL ? q : (q & 15) * 4), irow = th * TH + (TALL ? row : q >> 4);
    int tap_n = 0, ci_n = 0;

    xvec raw[8];
    f32x4 ad4[4];
    u32x4 wv[S::WT][2];
    auto load_chunk = [&](int c) __attribute__((always_inline)) {
        const int ch = c * CKP + cg * 8;
        if constexpr (PHP) {  // (chunks are loaded in order)
            const int ky = tap_n / 3, kx = tap_n - 3 * ky;
            const float* pl = xb0 + (kx == 1 ? (long)cin1 * pchan : 0L) + (long)(ci_n + cg * 8) * pchan + (down_phase_row(ky, irow, H) * (W + 4) + pcol) - (kx == 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) raw[i] = *(gcxu)(pl + (long)i * pchan);
            ci_n += CKP;
            if (ci_n == cin1) {
                ci_n = 0;
                ++tap_n;
            }
        } else if constexpr (X16) {  // (element offsets: load4 addresses halves)
            const float* px = ch < c0 ? p.x.p0 : p.x.p1;
            const long e0 = (ch < c0 ? b * p.x.bs0 + (long)ch * HW : b * p.x.bs1 + (long)(ch - c0) * HW) + poff;
#pragma unroll
            for (int i = 0; i < 8; ++i) raw[i] = load4<true>(px, e0 + (long)i * HW);
        } else {
            const float* pl = ch < c0 ? xb0 + (long)ch * HW : xb1 + (long)(ch - c0) * HW;
#pragma unroll
            for (int i = 0; i < 8; ++i) raw[i] = *(gcx)(pl + (long)i * HW + poff);
        }
        if (PRO != PRO_NONE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ad4[j] = *(gcf4)(affb + (size_t)(ch + 2 * j) * 2);
        }
#pragma unroll
        for (int j = 0; j < S::WT; ++j) {  // co tile WT cob + j of this chunk: 8 KB = 512 16-byte units (256 per plane)
            const unsigned char* ws = wsrc + ((size_t)j * nchunks + c) * WCH;
#pragma unroll
            for (int u = 0; u < NPLK; ++u) wv[j][u] = *(gcu4)(ws + (size_t)(tid + 256 * u) * 16);
        }
    };
    auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < PPT; ++e) {  // pixel e of the thread's: its 8 channels -> one 16-byte vector per plane
            unsigned ph[4], pl[4];
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) {
                float v0 = pixel(raw[2 * i2], e), v1 = pixel(raw[2 * i2 + 1], e);
                if (PRO != PRO_NONE) {
                    v0 = v0 * ad4[i2][0] + ad4[i2][1];
                    v1 = v1 * ad4[i2][2] + ad4[i2][3];
                }
                split_f16x2(v0, v1, ph[i2], pl[i2]);  // (NPLK == 1: the l half is dead code)
            }
            unsigned char* d = smem + (q * PPT + e) * ROWB + cg * 16;
            *reinterpret_cast<u32x4*>(d) = u32x4{ph[0], ph[1], ph[2], ph[3]};
            if (NPLK == 2) *reinterpret_cast<u32x4*>(d + XPL) = u32x4{pl[0], pl[1], pl[2], pl[3]};
        }
#pragma unroll
        for (int j = 0; j < S::WT; ++j)
#pragma unroll
            for (int u = 0; u < NPLK; ++u) {  // unit tid of plane u: output channel tid >> 2 of the tile, 8-channel part tid & 3 (wide: both from tid + 256 u)
                const int plane = TALL ? u : (tid + 256 * u) >> 8, r = TALL ? tid : (tid + 256 * u) & 255;
                *reinterpret_cast<u32x4*>(smem + 2 * XPL + plane * WPL + (j * CO_T + (r >> 2)) * ROWB + (r & 3) * 16) = wv[j][u];
            }
    };

    f32x16 acc[MR][NR], acl[MR][NR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = acl[m][n][r] = 0.f;
    // fragment rows: the wave index selects 64 rows of one operand -- TALL: the wave's channels of the 256, every wave reads all 64 pixels; wide: the wave's
    // pixels of the 256 (segments s = 2 wave + n: row s / 2, column block s % 2 of the tile = LDS rows 32 s ..), every wave reads all 64 channels
    int xrow[TALL ? 1 : NR];
    if constexpr (TALL) {
        xrow[0] = l31 * ROWB + hi * 16;
    } else {
#pragma unroll
        for (int n = 0; n < NR; ++n) xrow[n] = ((wave * NR + n) * 32 + l31) * ROWB + hi * 16;
    }
    auto xfrag = [&](int plane, int n, int st) __attribute__((always_inline)) {  // k-step st of segment n in the x plane at byte `plane` (0 | XPL)
        if constexpr (TALL) return smem + plane + (n * 32) * ROWB + xrow[0] + st * 32;
        else return smem + plane + xrow[n] + st * 32;
    };
    const int wrow = ((TALL ? wave * 64 : 0) + l31) * ROWB + hi * 16;  // + m * 32 channels

    load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();  // the previous chunk's fragments have been read
        store_chunk();
        if (c + 1 < nchunks) load_chunk(c + 1);
        __syncthreads();
#pragma unroll
        for (int st = 0; st < CKP / 16; ++st) {
            f16x8 wh[MR], wl[MR], xh[NR], xl[NR];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                wh[m] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(smem + 2 * XPL + (m * 32) * ROWB + wrow + st * 32));
                if (NPLK == 2) wl[m] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(smem + 2 * XPL + WPL + (m * 32) * ROWB + wrow + st * 32));
            }
#pragma unroll
            for (int n = 0; n < NR; ++n) {
                xh[n] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xfrag(0, n, st)));
                if (NPLK == 2) xl[n] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xfrag(XPL, n, st)));
            }
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int n = 0; n < NR; ++n) mfma_f16x2<NPLK == 1>(acc[m][n], acl[m][n], wh[m], wl[m], xh[n], xl[n]);
        }
    }
    const float wsc = p.wscale ? *p.wscale : 1.0f;  // inverse of the packer's power-of-two weight scale (exact)
    // the epilogue of the other convolution kernels: this wave owns 64 channels of one 64-pixel segment of the tile -- TALL: channels cob * 256 + wave * 64 .. + 63
    // of pixel row `row`; wide: channels cob * 64 .. + 63 of row `wave`
    const int co0 = cob * S::CO + (TALL ? wave * CO_T : 0), seg = TALL ? row : wave;
    float* patch = reinterpret_cast<float*>(smem + S::PATCH0) + wave * 256;
    if constexpr (NPLK == 2) {
        conv_epilogue_wide<TH, TW, MR, NR, true, false, FIRB>(p, acc, acl, b, th, tw, nTw, co0, seg, lane, patch, f2::LINV, wsc);
    } else {
        f32x16 none[1][1];
        conv_epilogue_wide<TH, TW, MR, NR, false, Y16>(p, acc, none, b, th, tw, nTw, co0, seg, lane, patch, 1.0f, wsc);
    }
}

// ---- weight packing: (Cout, Cin) fp32 -> [co tile][chunk][plane h / l][co 64][32 ch] f16 ----
// range[0] is raised to 1 if a weight does not fit the fp16 range (|w| >= 65504); the packed value saturates.
// wscale: as pack_conv_f16x2_kernel (conv_f16x2.hip) -- the layer's weights are scaled by a power of two, [1] <- its inverse
// taps = 9: w is the OIHW tensor of a 3x3 convolution with Cin / 9 input channels, packed as the (Cout, 9 Cin') matrix of the down-sampling GEMM --
// column (ky 3 + kx) Cin' + ci, the plane order of down_planes_kernel (resample.hip)
__global__ void pack_proj_f16x2_kernel(const float* __restrict__ w, unsigned* __restrict__ dst, int Cout, int Cin, long pairs,
                                       int* __restrict__ range, float* __restrict__ wscale, int taps) {
    using namespace p1;
    f16_saturate_mode();
    float inv = 1.0f;
    const float ws = wscale ? f16x2_weight_scale(reinterpret_cast<const int*>(wscale)[0], &inv) : 1.0f;
    if (wscale && blockIdx.x == 0 && threadIdx.x == 0) wscale[1] = inv;
    const int nchunks = Cin / CKP;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < pairs; i += (long)gridDim.x * blockDim.x) {
        long r = i;  // one pair of input channels of one output channel
        const int cp = r % (CKP / 2);
        r /= CKP / 2;
        const int col = r % CO_T;
        r /= CO_T;
        const int c = r % nchunks;
        const int cot = r / nchunks;
        const int co = cot * CO_T + col, ci = c * CKP + 2 * cp;
        const int cs = Cin / taps;  // (even: a pair of columns shares its tap)
        const long s0 = taps == 1 ? (long)co * Cin + ci : ((long)co * cs + ci % cs) * taps + ci / cs;
        const float v0 = w[s0] * ws, v1 = w[s0 + taps] * ws;
        if ((!(fabsf(v0) < 65504.f) || !(fabsf(v1) < 65504.f)) && range) atomicOr(range, 1);
        unsigned ph, pl;
        split_f16x2(v0, v1, ph, pl);
        const size_t base = ((size_t)(cot * nchunks + c) * 2) * (CO_T * CKP / 2);  // in 4-byte units
        dst[base + (size_t)col * (CKP / 2) + cp] = ph;
        dst[base + (size_t)(CO_T * CKP / 2) + (size_t)col * (CKP / 2) + cp] = pl;
    }
}

bool proj_f16x2_supported(int Cin, int Cout, int taps, int H, int W) {
    return taps == 1 && Cin % p1::CKP == 0 && Cout % p1::CO_T == 0 && H % p1::TH == 0 && W % p1::TW == 0;
}
long proj_f16x2_packed_floats(int Cin, int Cout) { return (long)Cin * Cout; }

hipError_t launch_pack_proj_f16x2(const float* w, float* dst, int Cout, int Cin, int* range_flag, hipStream_t s, float* wscale, int taps) {
    if (Cin % p1::CKP || Cout % p1::CO_T || (taps != 1 && taps != 9) || Cin % (2 * taps)) return hipErrorInvalidValue;
    const long pairs = (long)Cout * Cin / 2;
    if (wscale) {
        hipError_t e = launch_weight_absmax(w, (long)Cout * Cin, reinterpret_cast<int*>(wscale), s);
        if (e != hipSuccess) return e;
    }
    const int blocks = (int)((pairs + 255) / 256 < 2048 ? (pairs + 255) / 256 : 2048);
    pack_proj_f16x2_kernel<<<blocks, 256, 0, s>>>(w, reinterpret_cast<unsigned*>(dst), Cout, Cin, pairs, range_flag, wscale, taps);
    return hipGetLastError();
}

template <bool TALL, int PRO, int NPLK, int IOM = 0, bool FIRB = false, bool PHP = false>
static hipError_t launch_p1(const ConvParams& p, hipStream_t s) {
    using S = p1::Shape<TALL>;
    auto kern = proj_f16x2_kernel<TALL, PRO, NPLK, IOM, FIRB, PHP>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    // channel blocks x blocks per 4 x 64 pixel tile x tiles x batch
    const unsigned grid = (unsigned)((p.Cout / S::CO) * (p1::TH * p1::TW / S::PX) * (p.W / p1::TW) * (p.H / p1::TH) * p.B);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), S::LDS, s, p);
    return hipGetLastError();
}

hipError_t launch_proj_f16x2(const ConvParams& p, hipStream_t s, int down) {
    if (!proj_f16x2_supported(p.Cin, p.Cout, p.taps, p.H, p.W)) return hipErrorInvalidValue;
    if (p.x.p1 && p.x.c0 % 8) return hipErrorInvalidValue;  // a thread's 8 channels must not straddle the concat seam
    if (p.prologue == PRO_AFFINE_SILU || (p.prologue != PRO_NONE && p.aff == nullptr)) return hipErrorInvalidValue;
    if (p.stat && p.stat_slots != conv_stat_slots(p.H, p.W)) return hipErrorInvalidValue;
    if (p.x16 || p.y16) {  // fp16 storage (round 6): the skip convolutions of the full-resolution levels in the one-plane mode -- raw fp16 input, fp16 output
        if (!(p.x16 && p.y16) || p.pieces != 1 || p.prologue != PRO_NONE || p.res || p.stat) return hipErrorInvalidValue;
        return launch_p1<false, PRO_NONE, 1, 3>(p, s);
    }
    if (down != DOWN_NONE) {  // the down-sampling GEMM: plain input, the split arithmetic, no residual
        if (p.pieces == 1 || p.prologue != PRO_NONE || p.res || p.x16 || p.y16) return hipErrorInvalidValue;
        if (down == DOWN_PHASE) {  // one source, whole chunks inside a tap
            if (p.x.p1 || p.Cin % (9 * p1::CKP)) return hipErrorInvalidValue;
            return p.Cout % p1::COB == 0 ? launch_p1<true, PRO_NONE, 2, 0, true, true>(p, s) : launch_p1<false, PRO_NONE, 2, 0, true, true>(p, s);
        }
        return p.Cout % p1::COB == 0 ? launch_p1<true, PRO_NONE, 2, 0, true>(p, s) : launch_p1<false, PRO_NONE, 2, 0, true>(p, s);
    }
    if (p.Cout % p1::COB == 0) {  // 256-channel blocks: every pixel staged Cout / 256 times instead of Cout / 64
        if (p.pieces == 1) return p.prologue == PRO_NONE ? launch_p1<true, PRO_NONE, 1>(p, s) : launch_p1<true, PRO_AFFINE, 1>(p, s);
        return p.prologue == PRO_NONE ? launch_p1<true, PRO_NONE, 2>(p, s) : launch_p1<true, PRO_AFFINE, 2>(p, s);
    }
    if (p.pieces == 1) return p.prologue == PRO_NONE ? launch_p1<false, PRO_NONE, 1>(p, s) : launch_p1<false, PRO_AFFINE, 1>(p, s);
    return p.prologue == PRO_NONE ? launch_p1<false, PRO_NONE, 2>(p, s) : launch_p1<false, PRO_AFFINE, 2>(p, s);
}

}  // namespace r2dm
