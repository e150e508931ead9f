// K17: the PointNet feature extractor of the evaluation's FPD (metrics/extractor/pointnet.py: PointNet1, k = 16).
//
//  pointnet_trunk_kernel  one pass over tiles of 128 points of one cloud: layer 1 (3 -> 64, fp32 FMA, in registers, straight into the
//                         matrix-core operand layout), layer 2 (64 -> 128) and layer 3 (128 -> 1024) on the fp16 matrix pipe in the
//                         split arithmetic of f16x2.h (v = h + 2^-11 l, three v_mfma_f32_32x32x16_f16 per 16 k-values, two fp32
//                         accumulators, a power-of-two scale per layer), then the per-channel maximum over the points.
//                         The 64- and 128-channel activations live in registers / LDS, the 1024-channel one only in accumulators:
//                         what reaches HBM is the (B,1024) maximum.  BatchNorm is folded into the weights on the host; the last
//                         layer's inverse scale and bias (and the transformer's ReLU) commute with the maximum and are applied by
//                         the head kernel.
//                         Maximum: per lane over its points, then over the 32 lanes of a channel, then per block in LDS, then
//                         across blocks by an integer atomic max on an order-preserving key of the float bits -- exact in any
//                         order, the same bits on every call.  A padding lane of the last tile is excluded from the maximum (a zero
//                         point is a real point); a block works on one cloud only.
//                         A non-finite coordinate or an activation outside the fp16 operand range raises bits of *flag.
//  pointnet_head_kernel   the per-cloud MLPs 1024 -> 512 -> 256 -> 9 (+ identity: the spatial transformer) and 1024 -> 512 -> 256 -> 16
//                         (the classifier head; writes cat(x1, x2, x3, x4), 1808 values), fp32 FMA, one block per cloud.
//  weights                (Cout, Cin) fp32 -> the A-operand fragment order [32 rows][16 k][plane h / l][lane][8 halves]: pack_frag_f16x2_kernel
//                         (rangenet.hip) with one tap; Cout is a multiple of 32 and Cin of 16, so nothing is padded.
#include "common.h"
#include "f16x2.h"

namespace r2dm {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

namespace pn {
constexpr int THREADS = 512, P = 128;         // 8 waves; points per tile
constexpr int C1 = 64, C2 = 128, C3 = 1024;
constexpr int ROW3 = C2 * 2 + 16;             // bytes of one point's 128 fp16 layer-2 activations + padding (conflict-free 16-byte reads)
constexpr int H2PL = P * ROW3;                // one plane (h or l) of the tile
constexpr int W2B = C2 * C1 * 2 * 2;          // layer-2 weights, both planes: 32 KiB
constexpr int OFF_W2 = 2 * H2PL;
constexpr int OFF_W1 = OFF_W2 + W2B;          // 64 x (w0, w1, w2, bias)
constexpr int OFF_B2 = OFF_W1 + C1 * 16;
constexpr int OFF_MAX = OFF_B2 + C2 * 4;      // the block's running maxima
constexpr int LDS = OFF_MAX + C3 * 4;         // 108 032 bytes: one block per CU
constexpr int FLAG_COORD = 1, FLAG_RANGE = 2;  // (4: PACK_FLAG_WEIGHT, the packer's)
}  // namespace pn

struct PointNetTrunk {
    const float* src;
    long n;
    const float* trans;  // (B,9) or nullptr
    float img_min, img_max, divisor;
    const float* w1b;    // (64,4): folded layer-1 weights and bias
    const u32x4* w2p;
    const float* w2inv;  // inverse of the layer-2 weight scale
    const float* b2;
    const u32x4* w3p;
    int* keys;           // (B,1024) order-preserving keys of the maxima of W3s h2
    int* flag;
    long tiles;
};

// signed-integer key with the order of the floats (-0 below +0)
__device__ __forceinline__ int float_key(float v) {
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// LAYOUT 0: (B,5,H,W) samples, xyz * (img_min < depth < img_max) / divisor; 1: (B,N,3); 2: (B,3,N)
template <int LAYOUT>
__global__ __launch_bounds__(pn::THREADS) void pointnet_trunk_kernel(const PointNetTrunk p) {
    using namespace pn;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f16_saturate_mode();
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const long n = p.n;
    float* smax = reinterpret_cast<float*>(smem + OFF_MAX);
    const float* b2s = reinterpret_cast<const float*>(smem + OFF_B2);
    const f32x4* w1s = reinterpret_cast<const f32x4*>(smem + OFF_W1);
    const u32x4* w2s = reinterpret_cast<const u32x4*>(smem + OFF_W2);

    for (int i = tid; i < W2B / 16; i += THREADS) reinterpret_cast<u32x4*>(smem + OFF_W2)[i] = p.w2p[i];
    if (tid < C1) reinterpret_cast<f32x4*>(smem + OFF_W1)[tid] = reinterpret_cast<const f32x4*>(p.w1b)[tid];
    if (tid < C2) reinterpret_cast<float*>(smem + OFF_B2)[tid] = p.b2[tid];
    for (int i = tid; i < C3; i += THREADS) smax[i] = -__builtin_inff();
    float T[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (p.trans) {
#pragma unroll
        for (int i = 0; i < 9; ++i) T[i] = p.trans[(long)b * 9 + i];
    }
    const float inv2 = *p.w2inv;
    __syncthreads();

    const int sub = wave & 3, half = wave >> 2;  // layers 1 / 2: this wave's 32 points and 64 of the 128 channels
    int bad = 0;
    for (long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        // ---- layer 1 in registers, layer 2 on the matrix pipe ----
        const long i = t * P + sub * 32 + l31;
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < n) {
            if (LAYOUT == 0) {
                const float* s = p.src + (long)b * 5 * n;
                const float dep = s[i];
                const float m = (dep > p.img_min && dep < p.img_max) ? 1.0f : 0.0f;
                x = (s[n + i] * m) / p.divisor;
                y = (s[2 * n + i] * m) / p.divisor;
                z = (s[3 * n + i] * m) / p.divisor;
            } else if (LAYOUT == 1) {
                const float* s = p.src + ((long)b * n + i) * 3;
                x = s[0], y = s[1], z = s[2];
            } else {
                const float* s = p.src + (long)b * 3 * n;
                x = s[i], y = s[n + i], z = s[2 * n + i];
            }
        }
        if (!(fabsf(x) < __builtin_inff()) || !(fabsf(y) < __builtin_inff()) || !(fabsf(z) < __builtin_inff())) bad |= FLAG_COORD;
        {  // points (N,3) @ trans
            const float tx = fmaf(z, T[6], fmaf(y, T[3], x * T[0]));
            const float ty = fmaf(z, T[7], fmaf(y, T[4], x * T[1]));
            const float tz = fmaf(z, T[8], fmaf(y, T[5], x * T[2]));
            x = tx, y = ty, z = tz;
        }
        f32x16 acc[2], acl[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = acl[m][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < C1 / 16; ++ks) {
            unsigned ph[4], pl[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                float v[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const f32x4 w = w1s[ks * 16 + hi * 8 + j2 * 2 + e];
                    const float pre = fmaf(w[2], z, fmaf(w[1], y, fmaf(w[0], x, w[3])));
                    if (!(pre < 65504.f)) bad |= FLAG_RANGE;
                    v[e] = pre > 0.f ? pre : 0.f;
                }
                split_f16x2(v[0], v[1], ph[j2], pl[j2]);
            }
            const f16x8 xh = __builtin_bit_cast(f16x8, u32x4{ph[0], ph[1], ph[2], ph[3]});
            const f16x8 xl = __builtin_bit_cast(f16x8, u32x4{pl[0], pl[1], pl[2], pl[3]});
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int f = (((half * 2 + m) * (C1 / 16) + ks) * 2) * 64 + lane;
                const f16x8 wh = __builtin_bit_cast(f16x8, w2s[f]), wl = __builtin_bit_cast(f16x8, w2s[f + 64]);
                mfma_f16x2(acc[m], acl[m], wh, wl, xh, xl);
            }
        }
        __syncthreads();  // the previous tile's layer 3 has read its activations
        {
            unsigned char* row = smem + (sub * 32 + l31) * ROW3;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {  // registers 4 g .. 4 g + 3: channels ch .. ch + 3 of this lane's point
                    const int ch = half * 64 + m * 32 + g * 8 + hi * 4;
                    float v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float pre = fmaf(acl[m][g * 4 + q], f2::LINV, acc[m][g * 4 + q]) * inv2 + b2s[ch + q];
                        if (!(pre < 65504.f)) bad |= FLAG_RANGE;
                        v[q] = pre > 0.f ? pre : 0.f;
                    }
                    unsigned h0, l0, h1, l1;
                    split_f16x2(v[0], v[1], h0, l0);
                    split_f16x2(v[2], v[3], h1, l1);
                    *reinterpret_cast<uint2*>(row + ch * 2) = uint2{h0, h1};
                    *reinterpret_cast<uint2*>(row + H2PL + ch * 2) = uint2{l0, l1};
                }
        }
        __syncthreads();

        // ---- layer 3: this wave takes 4 of the 32 channel chunks over all points of the tile; weights from L2 into registers ----
        const long left = n - t * P;
        const int nvalid = left < P ? (int)left : P;
#pragma unroll 1
        for (int cc = 0; cc < 4; ++cc) {
            const int chunk = wave * 4 + cc;
            u32x4 wf[C2 / 16][2];
#pragma unroll
            for (int ks = 0; ks < C2 / 16; ++ks)
#pragma unroll
                for (int u = 0; u < 2; ++u) wf[ks][u] = p.w3p[((chunk * (C2 / 16) + ks) * 2 + u) * 64 + lane];
            float mx[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[r] = -__builtin_inff();
#pragma unroll 1
            for (int hf = 0; hf < 2; ++hf) {
                f32x16 a3[2], l3[2];
#pragma unroll
                for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) a3[nn][r] = l3[nn][r] = 0.f;
                const unsigned char* xr = smem + (hf * 64 + l31) * ROW3 + hi * 16;
#pragma unroll
                for (int ks = 0; ks < C2 / 16; ++ks) {
                    const f16x8 wh = __builtin_bit_cast(f16x8, wf[ks][0]), wl = __builtin_bit_cast(f16x8, wf[ks][1]);
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) {
                        const f16x8 xh = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xr + nn * 32 * ROW3 + ks * 32));
                        const f16x8 xl = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xr + H2PL + nn * 32 * ROW3 + ks * 32));
                        mfma_f16x2(a3[nn], l3[nn], wh, wl, xh, xl);
                    }
                }
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) {
                    const bool valid = hf * 64 + nn * 32 + l31 < nvalid;  // a padding lane takes no part
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = fmaf(l3[nn][r], f2::LINV, a3[nn][r]);
                        mx[r] = valid ? fmaxf(mx[r], v) : mx[r];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int off = 1; off < 32; off <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off));
            }
            if (l31 == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = chunk * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);  // (only this wave touches its channels)
                    smax[ch] = fmaxf(smax[ch], mx[r]);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < C3; i += THREADS) atomicMax(p.keys + (long)b * C3 + i, float_key(smax[i]));
    if (bad) atomicOr(p.flag, bad);
}

struct PointNetHead {
    const int* keys;
    const float* w3inv;
    const float* b3;
    const float *w1, *b1, *w2, *b2, *w3, *bo;
    float* out;
    int kout, stn;
};

// y[o] = act(dot(w[o], x) + bias[o]): one wave per output, lanes over k, a fixed butterfly
__device__ __forceinline__ void head_fc(const float* x, int K, const float* __restrict__ w, const float* __restrict__ bias, int O, float* y,
                                        bool relu) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = wave; o < O; o += 4) {
        const float* wr = w + (long)o * K;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s = fmaf(wr[k], x[k], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        s += bias[o];
        if (lane == 0) y[o] = relu ? (s > 0.f ? s : 0.f) : s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void pointnet_head_kernel(const PointNetHead p) {
    __shared__ float x1[1024], x2[512], x3[256], x4[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float inv3 = *p.w3inv;
    for (int i = tid; i < 1024; i += 256) {
        float v = key_float(p.keys[(long)b * 1024 + i]) * inv3 + p.b3[i];
        if (p.stn) v = v > 0.f ? v : 0.f;
        x1[i] = v;
    }
    __syncthreads();
    head_fc(x1, 1024, p.w1, p.b1, 512, x2, true);
    head_fc(x2, 512, p.w2, p.b2, 256, x3, true);
    head_fc(x3, 256, p.w3, p.bo, p.kout, x4, false);
    if (p.stn) {
        if (tid < 9) p.out[(long)b * 9 + tid] = x4[tid] + (tid % 4 == 0 ? 1.0f : 0.0f);
    } else {
        float* o = p.out + (long)b * 1808;
        for (int i = tid; i < 1024; i += 256) o[i] = x1[i];
        for (int i = tid; i < 512; i += 256) o[1024 + i] = x2[i];
        if (tid < 256) o[1536 + tid] = x3[tid];
        if (tid < 16) o[1792 + tid] = x4[tid];
    }
}

hipError_t launch_pointnet_pack(const float* w, int Cout, int Cin, void* dst, float* wscale, int* flag, hipStream_t s) {
    if (Cout < 32 || Cout % 32 || Cin < 16 || Cin % 16) return hipErrorInvalidValue;
    return launch_pack_frag_f16x2(w, Cout, Cin, 1, dst, wscale, flag, s);
}

size_t pointnet_scratch_bytes(int B) { return (size_t)B * pn::C3 * sizeof(int); }

template <int LAYOUT>
static hipError_t launch_trunk(const PointNetTrunk& p, int B, hipStream_t s) {
    auto kern = pointnet_trunk_kernel<LAYOUT>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, pn::LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    // about 1024 blocks over the batch (four per CU's worth of work), every block inside one cloud
    long per = (1024 + B - 1) / B;
    if (per > p.tiles) per = p.tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)per, (unsigned)B), dim3(pn::THREADS), pn::LDS, s, p);
    return hipGetLastError();
}

hipError_t launch_pointnet_trunk(const float* src, int layout, int B, long n, const float* trans, float img_min, float img_max, float divisor,
                                 const float* w1b, const void* w2p, const float* w2inv, const float* b2, const void* w3p, void* scratch, int* flag,
                                 hipStream_t s) {
    if (B < 1 || B > 65535 || n < 1 || layout < 0 || layout > 2) return hipErrorInvalidValue;
    // every key below any float's: a cloud has at least one point, so every channel is overwritten
    hipError_t e = hipMemsetAsync(scratch, 0x80, pointnet_scratch_bytes(B), s);
    if (e != hipSuccess) return e;
    PointNetTrunk p{src, n, trans, img_min, img_max, divisor, w1b, static_cast<const u32x4*>(w2p), w2inv, b2, static_cast<const u32x4*>(w3p),
                    static_cast<int*>(scratch), flag, (n + pn::P - 1) / pn::P};
    return layout == 0 ? launch_trunk<0>(p, B, s) : layout == 1 ? launch_trunk<1>(p, B, s) : launch_trunk<2>(p, B, s);
}

hipError_t launch_pointnet_head(const void* scratch, const float* w3inv, const float* b3, int stn, const float* w1, const float* b1, const float* w2,
                                const float* b2, const float* w3, const float* bo, int kout, float* out, int B, hipStream_t s) {
    if (B < 1 || kout < 1 || kout > 16 || (stn && kout != 9)) return hipErrorInvalidValue;
    PointNetHead p{static_cast<const int*>(scratch), w3inv, b3, w1, b1, w2, b2, w3, bo, out, kout, stn};
    pointnet_head_kernel<<<B, 256, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace r2dm
