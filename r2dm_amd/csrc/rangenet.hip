// K18: RangeNet-53 / -21 (metrics/extractor/rangenet.py), the extractor of the evaluation's FRD and the segmentation of completion_demo.py, eval mode.
//
//  rangenet_conv_kernel   ONE implicit-GEMM kernel for every layer kind: out[co, pixel] = sum over (tap, ci) of W[co, tap, ci] x[ci, pixel + tap].
//                         A launch is described by its taps (dh, dw), the input step per output column (stride_w) and where an output
//                         column lands (ow * out_mul + out_off):
//                           1 x 1                     one tap
//                           3 x 3, stride (1,1)       nine taps
//                           3 x 3, stride (1,2)       nine taps, stride_w = 2: only the width halves
//                           transposed 1 x 4, (1,2)   two launches, one per output-column parity, two taps each: even column 2j =
//                                                     in[j] w[..,1] + in[j-1] w[..,3], odd column 2j+1 = in[j] w[..,2] + in[j+1] w[..,0];
//                                                     out_mul = 2, out_off = parity.  No scatter, no atomics.
//                           stem (STEM)               nine taps over the (B,5,H,W) sample; the prologue applies the BINARY mask and the sensor
//                                                     normalisation (v - mean[c]) / std[c] * mask (the reference's ((v mask) - mean) / std * mask
//                                                     for a mask of zeros and ones); the five channels are padded to one 16-wide k-step with zeros.
//                         A wave owns 32 consecutive output pixels (the MFMA's columns, so a channel's 32 values are one 128-byte store) and
//                         MC chunks of 32 output channels; it reads its activations straight from the fp32 NCHW tensor, splits them once per
//                         k-step (f16x2.h: v = h + 2^-11 l) and reuses the split for the MC chunks: three v_mfma_f32_32x32x16_f16 per chunk
//                         and k-step, two fp32 accumulators.  Out-of-range taps and the padding of the last wave are zeros.
//                         Epilogue: (acc + 2^-11 acl) / weight scale + bias, LeakyReLU(slope), + add, + add2 (the residual input, the encoder
//                         skip), fp32 NCHW.  BatchNorm is folded into weights and bias on the host.  A wave sums its k-steps in a fixed
//                         order and no value is shared between pixels: the same bits on every call and for every batch.
//                         *flag |= 1 for a non-finite value of an unmasked input pixel, |= 2 for an activation outside the fp16 operand range.
//  pack_frag_f16x2_kernel (Cout, taps, Cin) fp32 -> [chunk of 32 rows][tap][k-step of 16][plane h / l][lane][8 halves], Cout padded to 32 and
//                         Cin to 16 with zeros, scaled by a power of two (max|w| into [2^9, 2^10)).  *flag |= 4 for a non-finite weight.
//                         PointNet's layers 2 and 3 are packed by it too (one tap, no padding): launch_pack_frag_f16x2 in common.h.
//  rangenet_argmax_kernel (B,C,H,W) logits -> (B,1,H,W) int64 labels, the lowest index on a tie.
#include "common.h"
#include "f16x2.h"

namespace r2dm {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

namespace rn {
constexpr int THREADS = 256, WAVES = 4, PIX = 32;  // a block: 4 waves x 32 pixels
constexpr int MAX_TAPS = 9;
constexpr int FLAG_INPUT = 1, FLAG_RANGE = 2;  // (4: PACK_FLAG_WEIGHT, the packer's)
}  // namespace rn

struct RangeNetConv {
    const float* in;
    const float* mask;  // STEM: (B,1,H,W) or nullptr (lo < depth < hi)
    const float* norm;  // STEM: mean[5], std[5]
    const u32x4* wp;
    const float* winv;
    const float* bias;
    const float* add;
    const float* add2;
    float* out;
    int* flag;
    long npix;          // B * H * Wout
    int Cin, H, Win, Wout, Wfull, Cout;
    int stride_w, out_mul, out_off, ntaps, nks;
    int dh[rn::MAX_TAPS], dw[rn::MAX_TAPS];
    float lo, hi, slope;
};

template <int MC, bool STEM>
__global__ __launch_bounds__(rn::THREADS) void rangenet_conv_kernel(const RangeNetConv p) {
    using namespace rn;
    f16_saturate_mode();
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long pix = ((long)blockIdx.x * WAVES + wave) * PIX + l31;
    const bool pv = pix < p.npix;
    const long q = pv ? pix : 0;
    const int ow = (int)(q % p.Wout);
    const long row = q / p.Wout;
    const int h = (int)(row % p.H);
    const long b = row / p.H;
    const long HW = (long)p.H * p.Win;
    const int mc0 = blockIdx.y * MC;

    f32x16 acc[MC], acl[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = acl[m][r] = 0.f;

    int bad = 0;
    for (int t = 0; t < p.ntaps; ++t) {
        const int ih = h + p.dh[t], iw = ow * p.stride_w + p.dw[t];
        const bool ok = pv && ih >= 0 && ih < p.H && iw >= 0 && iw < p.Win;
        const float* s = p.in + ((b * (STEM ? 5 : p.Cin)) * p.H + (ok ? ih : 0)) * p.Win + (ok ? iw : 0);
        for (int ks = 0; ks < p.nks; ++ks) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
            if (STEM) {
                if (ok && hi == 0) {
                    const float d = s[0];
                    const float m = p.mask ? p.mask[(b * p.H + ih) * p.Win + iw] : ((d > p.lo && d < p.hi) ? 1.0f : 0.0f);
                    if (m != 0.f) {  // (a masked pixel's raw values take no part, whatever they are)
#pragma unroll
                        for (int c = 0; c < 5; ++c) {
                            const float raw = s[c * HW];
                            if (!(fabsf(raw) < __builtin_inff())) bad |= FLAG_INPUT;
                            v[c] = ((raw - p.norm[c]) / p.norm[5 + c]) * m;
                            if (!(fabsf(v[c]) < 65504.f)) bad |= FLAG_RANGE;
                        }
                    }
                }
            } else if (ok) {
                const float* sc = s + (long)(ks * 16 + hi * 8) * HW;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = sc[j * HW];
            }
            unsigned ph[4], pl[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) split_f16x2(v[2 * j2], v[2 * j2 + 1], ph[j2], pl[j2]);
            const f16x8 xh = __builtin_bit_cast(f16x8, u32x4{ph[0], ph[1], ph[2], ph[3]});
            const f16x8 xl = __builtin_bit_cast(f16x8, u32x4{pl[0], pl[1], pl[2], pl[3]});
#pragma unroll
            for (int m = 0; m < MC; ++m) {
                const long f = ((((long)(mc0 + m) * p.ntaps + t) * p.nks + ks) * 2) * 64 + lane;
                const f16x8 wh = __builtin_bit_cast(f16x8, p.wp[f]), wl = __builtin_bit_cast(f16x8, p.wp[f + 64]);
                mfma_f16x2(acc[m], acl[m], wh, wl, xh, xl);
            }
        }
    }

    const float inv = *p.winv;
    const long HWo = (long)p.H * p.Wfull;
    const long o0 = (b * p.Cout * p.H + h) * p.Wfull + (long)ow * p.out_mul + p.out_off;
#pragma unroll
    for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // register r: channel (r >> 2) * 8 + hi * 4 + (r & 3) of this lane's pixel
            const int co = (mc0 + m) * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
            if (pv && co < p.Cout) {
                const long o = o0 + co * HWo;
                float v = fmaf(acl[m][r], f2::LINV, acc[m][r]) * inv + p.bias[co];
                v = v > 0.f ? v : v * p.slope;
                if (p.add) v += p.add[o];
                if (p.add2) v += p.add2[o];
                if (!(fabsf(v) < 65504.f)) bad |= FLAG_RANGE;
                p.out[o] = v;
            }
        }
    if (bad) atomicOr(p.flag, bad);
}

__global__ void pack_frag_f16x2_kernel(const float* __restrict__ w, unsigned* __restrict__ dst, int Cout, int Cin, int T, int nks, long pairs,
                                       int* __restrict__ flag, float* __restrict__ wscale) {
    f16_saturate_mode();
    float inv = 1.0f;
    const float ws = f16x2_weight_scale(reinterpret_cast<const int*>(wscale)[0], &inv);
    if (blockIdx.x == 0 && threadIdx.x == 0) wscale[1] = inv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < pairs; i += (long)gridDim.x * blockDim.x) {
        const int j2 = (int)(i & 3), lane = (int)((i >> 2) & 63);
        long rest = i >> 8;
        const int ks = (int)(rest % nks);
        rest /= nks;
        const int t = (int)(rest % T), mc = (int)(rest / T);
        const int row = mc * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + 2 * j2;
        float v0 = 0.f, v1 = 0.f;
        if (row < Cout) {
            const float* wr = w + ((long)row * T + t) * Cin;
            if (k < Cin) v0 = wr[k] * ws;
            if (k + 1 < Cin) v1 = wr[k + 1] * ws;
        }
        if (!(fabsf(v0) < 65504.f) || !(fabsf(v1) < 65504.f)) atomicOr(flag, PACK_FLAG_WEIGHT);
        unsigned ph, pl;
        split_f16x2(v0, v1, ph, pl);
        const long base = ((((long)mc * T + t) * nks + ks) * 2) * 256 + lane * 4 + j2;
        dst[base] = ph;
        dst[base + 256] = pl;
    }
}

__global__ void rangenet_argmax_kernel(const float* __restrict__ logits, long long* __restrict__ labels, int C, long hw, long n) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* s = logits + (i / hw) * C * hw + i % hw;
    float best = s[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = s[c * hw];
        if (v > best) best = v, arg = c;
    }
    labels[i] = arg;
}

size_t rangenet_packed_bytes(int Cout, int Cin, int taps) {
    if (Cout < 1 || Cin < 1 || taps < 1 || taps > rn::MAX_TAPS) return 0;
    return (size_t)((Cout + 31) / 32 * 32) * taps * ((Cin + 15) / 16 * 16) * 2 * sizeof(_Float16);
}

hipError_t launch_pack_frag_f16x2(const float* w, int Cout, int Cin, int taps, void* dst, float* wscale, int* flag, hipStream_t s) {
    if (Cout < 1 || Cin < 1 || taps < 1) return hipErrorInvalidValue;
    hipError_t e = launch_weight_absmax(w, (long)Cout * taps * Cin, reinterpret_cast<int*>(wscale), s);
    if (e != hipSuccess) return e;
    const int nks = (Cin + 15) / 16;
    const long pairs = (long)((Cout + 31) / 32) * taps * nks * 256;  // 32 rows x 16 k / 2 per (chunk, tap, k-step)
    long blocks = (pairs + 255) / 256;
    if (blocks > 65535) blocks = 65535;  // (grid-stride: every pair is written once either way)
    pack_frag_f16x2_kernel<<<(unsigned)blocks, 256, 0, s>>>(w, static_cast<unsigned*>(dst), Cout, Cin, taps, nks, pairs, flag, wscale);
    return hipGetLastError();
}

hipError_t launch_rangenet_pack(const float* w, int Cout, int Cin, int taps, void* dst, float* wscale, int* flag, hipStream_t s) {
    if (!rangenet_packed_bytes(Cout, Cin, taps)) return hipErrorInvalidValue;
    return launch_pack_frag_f16x2(w, Cout, Cin, taps, dst, wscale, flag, s);
}

// kind 0: 1 x 1; 1: 3 x 3; 2: 3 x 3 stride (1,2) (Win even); 3 / 4: the even / odd output columns of the transposed 1 x 4 stride (1,2); 5: stem
hipError_t launch_rangenet_conv(const float* in, const float* mask, const float* norm, float lo, float hi, const void* wp, const float* winv,
                                const float* bias, const float* add, const float* add2, float* out, int B, int Cin, int H, int Win, int Cout, int kind,
                                float slope, int* flag, hipStream_t s) {
    if (B < 1 || H < 1 || Win < 1 || Cout < 1 || kind < 0 || kind > 5) return hipErrorInvalidValue;
    if (kind == 5 ? Cin != 5 : (Cin < 16 || Cin % 16)) return hipErrorInvalidValue;
    if (kind == 2 && Win % 2) return hipErrorInvalidValue;
    RangeNetConv p{};
    p.in = in, p.mask = mask, p.norm = norm, p.wp = static_cast<const u32x4*>(wp), p.winv = winv, p.bias = bias, p.add = add, p.add2 = add2;
    p.out = out, p.flag = flag, p.Cin = Cin, p.H = H, p.Win = Win, p.Cout = Cout, p.lo = lo, p.hi = hi, p.slope = slope;
    p.nks = (Cin + 15) / 16;
    p.stride_w = kind == 2 ? 2 : 1;
    p.Wout = kind == 2 ? Win / 2 : Win;
    p.out_mul = kind == 3 || kind == 4 ? 2 : 1;
    p.out_off = kind == 4 ? 1 : 0;
    p.Wfull = p.Wout * p.out_mul;
    if (kind == 0) {
        p.ntaps = 1;
    } else if (kind == 3 || kind == 4) {
        p.ntaps = 2;
        p.dw[1] = kind == 3 ? -1 : 1;
    } else {
        p.ntaps = 9;
        for (int t = 0; t < 9; ++t) p.dh[t] = t / 3 - 1, p.dw[t] = t % 3 - 1;
    }
    p.npix = (long)B * H * p.Wout;
    const int chunks = (Cout + 31) / 32;
    const int mc = kind == 5 ? 1 : chunks % 4 == 0 ? 4 : chunks % 2 == 0 ? 2 : 1;
    if (kind == 5 && chunks != 1) return hipErrorInvalidValue;
    const long bx = (p.npix + rn::WAVES * rn::PIX - 1) / (rn::WAVES * rn::PIX);
    if (bx > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)bx, (unsigned)(chunks / mc));
    if (kind == 5) rangenet_conv_kernel<1, true><<<grid, rn::THREADS, 0, s>>>(p);
    else if (mc == 4) rangenet_conv_kernel<4, false><<<grid, rn::THREADS, 0, s>>>(p);
    else if (mc == 2) rangenet_conv_kernel<2, false><<<grid, rn::THREADS, 0, s>>>(p);
    else rangenet_conv_kernel<1, false><<<grid, rn::THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_rangenet_argmax(const float* logits, long long* labels, int B, int C, long hw, hipStream_t s) {
    if (B < 1 || C < 1 || hw < 1) return hipErrorInvalidValue;
    const long n = (long)B * hw;
    rangenet_argmax_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(logits, labels, C, hw, n);
    return hipGetLastError();
}

}  // namespace r2dm
