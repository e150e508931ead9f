// Latent-space operators: the DDIM transfer between two noise levels (inversion and decoding share it) and spherical interpolation
// of latents.  Both are one pass over HBM in float32 with FMA contraction off, so that the same expressions written in torch ops
// give the same bits.
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

// ---- DDIM transfer  x_t, prediction -> x_u  along the deterministic line, t -> u in either direction, no clipping -------------
// coef[b] = (alpha_t, sigma_t, alpha_u, sigma_u).  x_0 and eps come from the prediction in the DIRECT form of each objective: the
// indirect eps = (x - alpha_t x_0) / sigma_t cancels at t = 0 (sigma_t ~ 5.5e-4), where an inversion starts.
#pragma clang fp contract(off)
template <int OBJ>
__device__ __forceinline__ float transfer_elem(float x, float pr, float a_t, float s_t, float a_u, float s_u) {
    float x0, e;
    if (OBJ == OBJ_EPS) {
        e = pr;
        x0 = (x - s_t * pr) / a_t;
    } else if (OBJ == OBJ_V) {
        x0 = a_t * x - s_t * pr;
        e = s_t * x + a_t * pr;
    } else {
        x0 = pr;
        e = (x - a_t * pr) / s_t;
    }
    return a_u * x0 + s_u * e;
}

template <int OBJ>
__global__ __launch_bounds__(256) void ddim_transfer_kernel(const float* __restrict__ x_t, const float* __restrict__ pred,
                                                            const float* __restrict__ coef, float* __restrict__ x_u, long per_sample) {
    const int b = blockIdx.y;
    const float a_t = coef[4 * b], s_t = coef[4 * b + 1], a_u = coef[4 * b + 2], s_u = coef[4 * b + 3];
    const long n4 = per_sample >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x_t + b * per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(pred + b * per_sample);
    f32x4* o4 = reinterpret_cast<f32x4*>(x_u + b * per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = transfer_elem<OBJ>(x[j], pr[j], a_t, s_t, a_u, s_u);
        o4[i] = o;
    }
}
#pragma clang fp contract(fast)

// (alignment rules of launch_posterior)
hipError_t launch_ddim_transfer(const float* x_t, const float* pred, const float* coef, float* x_u, int B, long per_sample, int objective,
                                hipStream_t s) {
    if ((per_sample & 3) || (reinterpret_cast<uintptr_t>(x_t) & 15) || (reinterpret_cast<uintptr_t>(pred) & 15) ||
        (reinterpret_cast<uintptr_t>(x_u) & 15))
        return hipErrorInvalidValue;
    const dim3 g = quad_grid(B, per_sample);
    switch (objective) {
        case OBJ_EPS: ddim_transfer_kernel<OBJ_EPS><<<g, 256, 0, s>>>(x_t, pred, coef, x_u, per_sample); break;
        case OBJ_V: ddim_transfer_kernel<OBJ_V><<<g, 256, 0, s>>>(x_t, pred, coef, x_u, per_sample); break;
        case OBJ_X0: ddim_transfer_kernel<OBJ_X0><<<g, 256, 0, s>>>(x_t, pred, coef, x_u, per_sample); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- spherical interpolation of two latents at K weights ----------------------------------------------------------------------
// Launch 1: per sample the sums <a,b>, <a,a>, <b,b> in float64 (each float32 product widened before it is added), in a fixed order:
// thread (grid-stride over the sample) -> wave -> the block's four waves -> part[b][block][3].  The number of blocks per sample depends
// on per_sample alone, so a sample's sums do not depend on the batch it is in; no atomics (the scheme of diffusion_loss_kernel).
// Launch 2: every block adds its sample's block partials in index order and evaluates the K coefficient pairs in float64 (all blocks
// by the same instructions on the same values: the same bits), block 0 of a sample writes them to coef64[k][b]; then one pass over a
// and b writes all K outputs, out[k][b] = fl32(c_a) * a + fl32(c_b) * b.
constexpr int kSlerpMaxBlocks = 16;  // blocks per sample of launch 1: 16 x 1024 elements per pass
static int slerp_blocks(long per_sample) {
    const long n = (per_sample + 1023) / 1024;
    return n < 1 ? 1 : n > kSlerpMaxBlocks ? kSlerpMaxBlocks : (int)n;
}
size_t slerp_scratch_bytes(int B, long per_sample) { return (size_t)B * slerp_blocks(per_sample) * 3 * sizeof(double); }

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void slerp_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ part,
                                                        long per_sample) {
    const int s = blockIdx.y;
    const long n4 = per_sample >> 2;
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a + s * per_sample);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b + s * per_sample);
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = a4[i], y = b4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pab = x[e] * y[e], paa = x[e] * x[e], pbb = y[e] * y[e];
            ab += (double)pab;
            aa += (double)paa;
            bb += (double)pbb;
        }
    }
    ab = wave_sum_f64(ab);
    aa = wave_sum_f64(aa);
    bb = wave_sum_f64(bb);
    __shared__ double sh[3][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[0][wave] = ab, sh[1][wave] = aa, sh[2][wave] = bb;
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* v = sh[threadIdx.x];
        part[((long)s * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = ((v[0] + v[1]) + v[2]) + v[3];
    }
}

struct SlerpWeights {
    float w[kSlerpMaxWeights];
};

__global__ __launch_bounds__(256) void slerp_blend_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const double* __restrict__ part, SlerpWeights weights, int K, int blocks,
                                                          float* __restrict__ out, double* __restrict__ coef64, long per_sample) {
    const int s = blockIdx.y, B = gridDim.y;
    __shared__ float c[kSlerpMaxWeights][2];
    if (threadIdx.x < K) {
        const double* p = part + (long)s * blocks * 3;
        double ab = 0.0, aa = 0.0, bb = 0.0;
        for (int j = 0; j < blocks; ++j) ab += p[3 * j], aa += p[3 * j + 1], bb += p[3 * j + 2];
        const double w = (double)weights.w[threadIdx.x];
        double ca = 1.0 - w, cb = w;  // the lerp pair: a zero input, or (anti)parallel inputs
        if (aa > 0.0 && bb > 0.0) {
            double cs = ab / sqrt(aa * bb);
            cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;
            if (!(1.0 - cs * cs < 1e-10)) {
                const double omega = acos(cs), so = sin(omega);
                ca = sin((1.0 - w) * omega) / so;
                cb = sin(w * omega) / so;
            }
        }
        c[threadIdx.x][0] = (float)ca;
        c[threadIdx.x][1] = (float)cb;
        if (blockIdx.x == 0) {
            double* o = coef64 + ((long)threadIdx.x * B + s) * 2;
            o[0] = ca;
            o[1] = cb;
        }
    }
    __syncthreads();
    const long n4 = per_sample >> 2;
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a + s * per_sample);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b + s * per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = a4[i], y = b4[i];
        for (int k = 0; k < K; ++k) {
            const float ca = c[k][0], cb = c[k][1];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ca * x[e] + cb * y[e];
            reinterpret_cast<f32x4*>(out + ((long)k * B + s) * per_sample)[i] = o;
        }
    }
}
#pragma clang fp contract(fast)

// (arguments validated by r2dm_slerp: 1 <= K <= kSlerpMaxWeights, finite host weights, 1 <= B <= 65535, per_sample % 4 == 0, alignment)
hipError_t launch_slerp(const float* a, const float* b, const float* weights, int K, float* out, double* coef64, int B, long per_sample,
                        void* scratch, hipStream_t s) {
    const int blocks = slerp_blocks(per_sample);
    double* part = static_cast<double*>(scratch);
    slerp_dot_kernel<<<dim3((unsigned)blocks, (unsigned)B), 256, 0, s>>>(a, b, part, per_sample);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    SlerpWeights w{};
    for (int k = 0; k < K; ++k) w.w[k] = weights[k];
    slerp_blend_kernel<<<quad_grid(B, per_sample), 256, 0, s>>>(a, b, part, w, K, blocks, out, coef64, per_sample);
    return hipGetLastError();
}

}  // namespace r2dm
