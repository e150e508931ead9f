// K10: fused posterior update  x_t, prediction, noise -> x_s  (one HBM pass: 3 reads + 1 write).
//
// Replays, per element and in the reference's float32 operation order (no FMA contraction, IEEE
// division), the tail of p_step:
//   continuous time  /root/reference/models/diffusion/continuous_time.py:208-229
//   discrete time    /root/reference/models/diffusion/discrete_time.py:140-177
// All schedule scalars arrive in coef[b][8], computed on the host with the reference's torch ops.
//
// also: K12 LiDAR post-processing of finished samples (reference sample_and_save.py:52-57).
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

enum { M_CT_DDPM = 0, M_CT_DDIM = 1, M_DT_DDPM = 2, M_DT_DDIM = 3, M_DT_DDIM_NOISE = 4 };
enum { OBJ_EPS = 0, OBJ_V = 1, OBJ_X0 = 2 };

#pragma clang fp contract(off)
// the two halves of one element's update: the clamped estimate of x_0, and x_s from it (posterior_known_kernel puts the measurement between them)
template <int MODE, int OBJ>
__device__ __forceinline__ float posterior_x0(float x, float pr, const float* k, float clip) {
    float x0;
    if (MODE == M_CT_DDPM || MODE == M_CT_DDIM) {
        const float a_t = k[0], s_t = k[1];
        if (OBJ == OBJ_EPS) x0 = (x - s_t * pr) / a_t;
        else if (OBJ == OBJ_V) x0 = a_t * x - s_t * pr;
        else x0 = pr;
    } else {
        if (OBJ == OBJ_X0) x0 = pr;
        else x0 = k[0] * x - k[1] * pr;
    }
    if (clip >= 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
    return x0;
}

template <int MODE>
__device__ __forceinline__ float posterior_update(float x, float x0, float z, const float* k) {
    if (MODE == M_CT_DDPM) {
        const float a_t = k[0], a_s = k[2], c = k[4], sd = k[5];
        const float mean = a_s * (x * (1.0f - c) / a_t + c * x0);
        return mean + sd * z;
    } else if (MODE == M_CT_DDIM) {
        const float a_t = k[0], s_t = k[1], a_s = k[2], c1 = k[6], c2 = k[7];
        const float eps = (x - a_t * x0) / s_t;
        return a_s * x0 + c1 * z + c2 * eps;
    } else if (MODE == M_DT_DDPM) {
        const float mean = k[2] * x0 + k[3] * x;
        return mean + k[4] * z;
    } else {
        const float eps = (x - k[2] * x0) / k[3];
        float xs = k[5] * x0 + k[4] * eps;
        if (MODE == M_DT_DDIM_NOISE) xs = xs + k[6] * z;
        return xs;
    }
}

template <int MODE, int OBJ>
__device__ __forceinline__ float posterior_elem(float x, float pr, float z, const float* k, float clip) {
    return posterior_update<MODE>(x, posterior_x0<MODE, OBJ>(x, pr, k, clip), z, k);
}

template <int MODE, int OBJ>
__global__ __launch_bounds__(256) void posterior_kernel(PosteriorParams p) {
    const int b = blockIdx.y;
    float k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = p.coef[b * 8 + i];
    const long n4 = p.per_sample >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x_t + b * p.per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p.pred + b * p.per_sample);
    const f32x4* z4 = p.noise ? reinterpret_cast<const f32x4*>(p.noise + b * p.per_sample) : nullptr;
    f32x4* o4 = reinterpret_cast<f32x4*>(p.x_s + b * p.per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (z4) z = z4[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = posterior_elem<MODE, OBJ>(x[j], pr[j], z[j], k, p.clip);
        o4[i] = o;
    }
    // tail (per_sample not a multiple of 4)
    for (long i = (n4 << 2) + blockIdx.x * 256L + threadIdx.x; i < p.per_sample; i += (long)gridDim.x * 256) {
        const long e = b * p.per_sample + i;
        p.x_s[e] = posterior_elem<MODE, OBJ>(p.x_t[e], p.pred[e], p.noise ? p.noise[e] : 0.f, k, p.clip);
    }
}

template <int MODE>
static hipError_t launch_obj(const PosteriorParams& p, dim3 g, hipStream_t s) {
    switch (p.objective) {
        case OBJ_EPS: posterior_kernel<MODE, OBJ_EPS><<<g, 256, 0, s>>>(p); break;
        case OBJ_V: posterior_kernel<MODE, OBJ_V><<<g, 256, 0, s>>>(p); break;
        case OBJ_X0: posterior_kernel<MODE, OBJ_X0><<<g, 256, 0, s>>>(p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_posterior(const PosteriorParams& p, hipStream_t s) {
    if ((p.per_sample & 3) || (reinterpret_cast<uintptr_t>(p.x_t) & 15) || (reinterpret_cast<uintptr_t>(p.pred) & 15) ||
        (reinterpret_cast<uintptr_t>(p.x_s) & 15) || (reinterpret_cast<uintptr_t>(p.noise) & 15))
        return hipErrorInvalidValue;
    if (p.noise == nullptr && p.mode != M_DT_DDIM) return hipErrorInvalidValue;
    long bx = (p.per_sample / 4 + 255) / 256;
    if (bx < 1) bx = 1;
    if (bx > 1024) bx = 1024;
    const dim3 g((unsigned)bx, p.B);
    switch (p.mode) {
        case M_CT_DDPM: return launch_obj<M_CT_DDPM>(p, g, s);
        case M_CT_DDIM: return launch_obj<M_CT_DDIM>(p, g, s);
        case M_DT_DDPM: return launch_obj<M_DT_DDPM>(p, g, s);
        case M_DT_DDIM: return launch_obj<M_DT_DDIM>(p, g, s);
        case M_DT_DDIM_NOISE: return launch_obj<M_DT_DDIM_NOISE>(p, g, s);
    }
    return hipErrorInvalidValue;
}

// ---- data-consistent posterior step (DDNM's null-space projection for a mask operator) ------------------------------------------
// x_t, prediction, noise, known, mask -> x_s in one pass (5 reads + 1 write): posterior_x0, then the measurement written over the
// estimate, x0 = m * y + (1 - m) * x0 (m a per-pixel weight, not necessarily binary), then posterior_update.  Continuous time only.
// mask has mask_c channels (1 = broadcast over the planes of a sample); plane % 4 == 0: a quad never straddles planes.
template <int MODE, int OBJ>
__global__ __launch_bounds__(256) void posterior_known_kernel(PosteriorParams p, const float* __restrict__ known,
                                                              const float* __restrict__ mask, long plane, int mask_c) {
    const int b = blockIdx.y;
    float k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = p.coef[b * 8 + i];
    const long n4 = p.per_sample >> 2, plane4 = plane >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x_t + b * p.per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p.pred + b * p.per_sample);
    const f32x4* z4 = reinterpret_cast<const f32x4*>(p.noise + b * p.per_sample);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(known + b * p.per_sample);
    const f32x4* m4 = reinterpret_cast<const f32x4*>(mask + b * (mask_c == 1 ? plane : p.per_sample));
    f32x4* o4 = reinterpret_cast<f32x4*>(p.x_s + b * p.per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i], z = z4[i], y = y4[i];
        const f32x4 m = m4[mask_c == 1 ? i % plane4 : i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x0 = posterior_x0<MODE, OBJ>(x[j], pr[j], k, p.clip);
            x0 = m[j] * y[j] + (1.0f - m[j]) * x0;
            o[j] = posterior_update<MODE>(x[j], x0, z[j], k);
        }
        o4[i] = o;
    }
}

template <int MODE>
static hipError_t launch_known_obj(const PosteriorParams& p, const float* known, const float* mask, long plane, int mask_c, dim3 g,
                                   hipStream_t s) {
    switch (p.objective) {
        case OBJ_EPS: posterior_known_kernel<MODE, OBJ_EPS><<<g, 256, 0, s>>>(p, known, mask, plane, mask_c); break;
        case OBJ_V: posterior_known_kernel<MODE, OBJ_V><<<g, 256, 0, s>>>(p, known, mask, plane, mask_c); break;
        case OBJ_X0: posterior_known_kernel<MODE, OBJ_X0><<<g, 256, 0, s>>>(p, known, mask, plane, mask_c); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (arguments validated by r2dm_posterior_step_known; checked again here, since the kernel reads quads and has no tail)
hipError_t launch_posterior_known(const PosteriorParams& p, const float* known, const float* mask, int channels, int mask_c,
                                  hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.per_sample < 4 || (p.per_sample & 3) || channels < 1 || p.per_sample % channels ||
        (p.per_sample / channels) % 4 || (mask_c != 1 && mask_c != channels) || !p.noise || !known || !mask)
        return hipErrorInvalidValue;
    long bx = (p.per_sample / 4 + 255) / 256;  // (launch_posterior's shape)
    if (bx > 1024) bx = 1024;
    const dim3 g((unsigned)bx, p.B);
    const long plane = p.per_sample / channels;
    switch (p.mode) {
        case M_CT_DDPM: return launch_known_obj<M_CT_DDPM>(p, known, mask, plane, mask_c, g, s);
        case M_CT_DDIM: return launch_known_obj<M_CT_DDIM>(p, known, mask, plane, mask_c, g, s);
    }
    return hipErrorInvalidValue;
}

// ---- DPM-Solver++(2M) update (Lu et al. 2022, the data-prediction multistep solver on the half-log-SNR axis) --------------------------------
// x_t, prediction[, x0_prev] -> x_s, x0 in one pass (2 or 3 reads + 2 writes).  coef[b] = (alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0), host-computed.
// x0 is the clamped estimate of posterior_x0 (the next step's history); x_s = c_x x + c_0 x0 (first order, x0_prev not read) or
// (c_x x + c_0 x0) + c_1 x0_prev.  x0 may be x0_prev's buffer: a thread reads its quad of x0_prev before it writes the same quad of x0, and no
// other thread touches that quad -- hence no __restrict__ on the two.
template <int OBJ, bool SECOND>
__global__ __launch_bounds__(256) void dpm_step_kernel(const float* __restrict__ x_t, const float* __restrict__ pred, const float* x0_prev,
                                                       const float* __restrict__ coef, float* __restrict__ x_s, float* x0_out, long per_sample,
                                                       float clip) {
    const int b = blockIdx.y;
    float k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = coef[b * 8 + i];
    const float c_x = k[2], c_0 = k[3], c_1 = k[4];
    const long n4 = per_sample >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x_t + b * per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(pred + b * per_sample);
    const f32x4* h4 = SECOND ? reinterpret_cast<const f32x4*>(x0_prev + b * per_sample) : nullptr;
    f32x4* o4 = reinterpret_cast<f32x4*>(x_s + b * per_sample);
    f32x4* e4 = reinterpret_cast<f32x4*>(x0_out + b * per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 h = {0.f, 0.f, 0.f, 0.f};
        if (SECOND) h = h4[i];
        f32x4 o, e;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = posterior_x0<M_CT_DDPM, OBJ>(x[j], pr[j], k, clip);
            o[j] = c_x * x[j] + c_0 * e[j];
            if (SECOND) o[j] = o[j] + c_1 * h[j];
        }
        o4[i] = o;
        e4[i] = e;
    }
}

template <int OBJ>
static hipError_t launch_dpm_obj(const DpmParams& p, dim3 g, hipStream_t s) {
    if (p.x0_prev) dpm_step_kernel<OBJ, true><<<g, 256, 0, s>>>(p.x_t, p.pred, p.x0_prev, p.coef, p.x_s, p.x0, p.per_sample, p.clip);
    else dpm_step_kernel<OBJ, false><<<g, 256, 0, s>>>(p.x_t, p.pred, nullptr, p.coef, p.x_s, p.x0, p.per_sample, p.clip);
    return hipGetLastError();
}

// (arguments validated by r2dm_dpm_step; checked again here, since the kernel reads quads and has no tail)
hipError_t launch_dpm_step(const DpmParams& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.per_sample < 4 || (p.per_sample & 3) || !p.x_t || !p.pred || !p.coef || !p.x_s || !p.x0 || p.x_s == p.x_t)
        return hipErrorInvalidValue;
    long bx = (p.per_sample / 4 + 255) / 256;  // (launch_posterior's shape)
    if (bx > 1024) bx = 1024;
    const dim3 g((unsigned)bx, p.B);
    switch (p.objective) {
        case OBJ_EPS: return launch_dpm_obj<OBJ_EPS>(p, g, s);
        case OBJ_V: return launch_dpm_obj<OBJ_V>(p, g, s);
        case OBJ_X0: return launch_dpm_obj<OBJ_X0>(p, g, s);
    }
    return hipErrorInvalidValue;
}

// ---- DPM-Solver++(2M) update with a measurement and a noise operand: completion and the stochastic member (SDE-DPM-Solver++(2M)) ------------
// x_t, prediction[, x0_prev][, noise][, known, mask] -> x_s, x0 in one pass (2 to 6 reads + 2 writes).  coef[b] = (alpha_t, sigma_t, c_x, c_0, c_1,
// c_z, 0, 0).  dpm_step_kernel's update with DDNM's projection between its halves, x0 = m y + (1 - m) x0 (posterior_known_kernel's), and
// + c_z z behind them; x0 is written AFTER the projection: that is the history the next step extrapolates from.  An absent operand is a
// template argument: no load, no arithmetic.  x0 may be x0_prev's buffer, as in dpm_step_kernel.
template <int OBJ, bool SECOND, bool NOISE, bool KNOWN>
__global__ __launch_bounds__(256) void dpm_step_known_kernel(DpmParams p, const float* __restrict__ noise, const float* __restrict__ known,
                                                             const float* __restrict__ mask, long plane, int mask_c) {
    const int b = blockIdx.y;
    float k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = p.coef[b * 8 + i];
    const float c_x = k[2], c_0 = k[3], c_1 = k[4], c_z = k[5];
    const long n4 = p.per_sample >> 2, plane4 = plane >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x_t + b * p.per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p.pred + b * p.per_sample);
    const f32x4* h4 = SECOND ? reinterpret_cast<const f32x4*>(p.x0_prev + b * p.per_sample) : nullptr;
    const f32x4* z4 = NOISE ? reinterpret_cast<const f32x4*>(noise + b * p.per_sample) : nullptr;
    const f32x4* y4 = KNOWN ? reinterpret_cast<const f32x4*>(known + b * p.per_sample) : nullptr;
    const f32x4* m4 = KNOWN ? reinterpret_cast<const f32x4*>(mask + b * (mask_c == 1 ? plane : p.per_sample)) : nullptr;
    f32x4* o4 = reinterpret_cast<f32x4*>(p.x_s + b * p.per_sample);
    f32x4* e4 = reinterpret_cast<f32x4*>(p.x0 + b * p.per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, z = h, y = h, m = h;
        if (SECOND) h = h4[i];
        if (NOISE) z = z4[i];
        if (KNOWN) y = y4[i], m = m4[mask_c == 1 ? i % plane4 : i];
        f32x4 o, e;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = posterior_x0<M_CT_DDPM, OBJ>(x[j], pr[j], k, p.clip);
            if (KNOWN) e[j] = m[j] * y[j] + (1.0f - m[j]) * e[j];
            o[j] = c_x * x[j] + c_0 * e[j];
            if (SECOND) o[j] = o[j] + c_1 * h[j];
            if (NOISE) o[j] = o[j] + c_z * z[j];
        }
        o4[i] = o;
        e4[i] = e;
    }
}

template <int OBJ, bool SECOND, bool NOISE>
static hipError_t launch_dpm_known_k(const DpmParams& p, const float* noise, const float* known, const float* mask, long plane, int mask_c, dim3 g,
                                     hipStream_t s) {
    if (known) dpm_step_known_kernel<OBJ, SECOND, NOISE, true><<<g, 256, 0, s>>>(p, noise, known, mask, plane, mask_c);
    else dpm_step_known_kernel<OBJ, SECOND, NOISE, false><<<g, 256, 0, s>>>(p, noise, nullptr, nullptr, plane, mask_c);
    return hipGetLastError();
}

template <int OBJ>
static hipError_t launch_dpm_known_obj(const DpmParams& p, const float* noise, const float* known, const float* mask, long plane, int mask_c, dim3 g,
                                       hipStream_t s) {
    if (p.x0_prev) {
        return noise ? launch_dpm_known_k<OBJ, true, true>(p, noise, known, mask, plane, mask_c, g, s)
                     : launch_dpm_known_k<OBJ, true, false>(p, noise, known, mask, plane, mask_c, g, s);
    }
    return noise ? launch_dpm_known_k<OBJ, false, true>(p, noise, known, mask, plane, mask_c, g, s)
                 : launch_dpm_known_k<OBJ, false, false>(p, noise, known, mask, plane, mask_c, g, s);
}

// (arguments validated by r2dm_dpm_step_known; checked again here, since the kernel reads quads and has no tail)
hipError_t launch_dpm_step_known(const DpmParams& p, const float* noise, const float* known, const float* mask, int channels, int mask_c,
                                 hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.per_sample < 4 || (p.per_sample & 3) || !p.x_t || !p.pred || !p.coef || !p.x_s || !p.x0 || p.x_s == p.x_t ||
        channels < 1 || p.per_sample % channels || (p.per_sample / channels) % 4 || (mask_c != 1 && mask_c != channels) || !known != !mask)
        return hipErrorInvalidValue;
    long bx = (p.per_sample / 4 + 255) / 256;  // (launch_posterior's shape)
    if (bx > 1024) bx = 1024;
    const dim3 g((unsigned)bx, p.B);
    const long plane = p.per_sample / channels;
    switch (p.objective) {
        case OBJ_EPS: return launch_dpm_known_obj<OBJ_EPS>(p, noise, known, mask, plane, mask_c, g, s);
        case OBJ_V: return launch_dpm_known_obj<OBJ_V>(p, noise, known, mask, plane, mask_c, g, s);
        case OBJ_X0: return launch_dpm_known_obj<OBJ_X0>(p, noise, known, mask, plane, mask_c, g, s);
    }
    return hipErrorInvalidValue;
}

// ---- LiDAR post-processing ("next" row f.1) ------------------------------------------------
// sample (B,2,H,W) in [-1,1] -> (B,5,H,W): metric depth (decoded by the checkpoint's depth format, masked to
// (min_depth, max_depth)), Cartesian x,y,z along the per-pixel ray angles, reflectance in [0,1].
// /root/reference/utils/lidar.py:49-61,95-120 ; /root/reference/sample_and_save.py:52-57.
// FMT: 0 log_depth  metric = exp2(d log2(max + 1)) - 1 | 1 inverse_depth  metric = (1 / (d + 1e-8)) min | 2 depth  metric = d max
template <int FMT>
__global__ __launch_bounds__(256) void lidar_post_kernel(const float* __restrict__ x, const float* __restrict__ ang,
                                                         float* __restrict__ y, long hw, float min_d, float max_d,
                                                         float log2_range) {
    const int b = blockIdx.y;
    const float* xb = x + (long)b * 2 * hw;
    float* yb = y + (long)b * 5 * hw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
        const float d = (xb[i] + 1.0f) / 2.0f, r = (xb[hw + i] + 1.0f) / 2.0f;
        float metric;
        if (FMT == 0) metric = exp2f(d * log2_range) - 1.0f;
        else if (FMT == 1) metric = __fmul_rn(__frcp_rn(d + 1e-8f), min_d);  // (torch evaluates `scalar / tensor` as tensor.reciprocal() * scalar: two roundings)
        else metric = d * max_d;
        const float m = (metric > min_d && metric < max_d) ? 1.0f : 0.0f;
        metric = metric * m;
        const float m2 = (metric > min_d && metric < max_d) ? 1.0f : 0.0f;
        const float phi = ang[i], theta = ang[hw + i];
        const float cp = cosf(phi);
        yb[i] = metric;
        yb[hw + i] = metric * cp * cosf(theta) * m2;
        yb[2 * hw + i] = metric * cp * sinf(theta) * m2;
        yb[3 * hw + i] = metric * sinf(phi) * m2;
        yb[4 * hw + i] = r;
    }
}

hipError_t launch_lidar_postprocess(const float* x, const float* angles, float* y, int B, int H, int W, float min_d,
                                    float max_d, hipStream_t s, int depth_format) {
    const long hw = (long)H * W;
    long bx = (hw + 255) / 256;
    if (bx > 1024) bx = 1024;
    const dim3 grid((unsigned)bx, B);
    const float l2 = (float)log2((double)max_d + 1.0);
    switch (depth_format) {
        case 0: lidar_post_kernel<0><<<grid, 256, 0, s>>>(x, angles, y, hw, min_d, max_d, l2); break;
        case 1: lidar_post_kernel<1><<<grid, 256, 0, s>>>(x, angles, y, hw, min_d, max_d, l2); break;
        case 2: lidar_post_kernel<2><<<grid, 256, 0, s>>>(x, angles, y, hw, min_d, max_d, l2); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}


// ---- RePaint pieces (reference continuous_time.py:169-190, 287-303), replayed in the reference's op order -------
// blend:  out = mask * (known * alpha + noise * sigma) + (1 - mask) * unknown      (q_step_from_x_0 + mask blend)
// q_step: out = x_s * a_ts + std * noise                                           (forward diffusion s -> t)
// coef[b] = (alpha, sigma) resp. (a_ts, std): host-computed scalars.  mask has mask_c channels (1 = broadcast).
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void repaint_blend_kernel(const float* __restrict__ known, const float* __restrict__ noise,
                                                            const float* __restrict__ unknown, const float* __restrict__ mask,
                                                            const float* __restrict__ coef, float* __restrict__ out,
                                                            long per_sample, long plane, int mask_c) {
    const int b = blockIdx.y;
    const float alpha = coef[2 * b], sigma = coef[2 * b + 1];
    const long base = b * per_sample;
    for (long i = (blockIdx.x * 256L + threadIdx.x) * 4; i < per_sample; i += (long)gridDim.x * 1024) {
        const f32x4 k = *reinterpret_cast<const f32x4*>(known + base + i), z = *reinterpret_cast<const f32x4*>(noise + base + i);
        const f32x4 u = *reinterpret_cast<const f32x4*>(unknown + base + i);
        const long mi = mask_c == 1 ? b * plane + i % plane : base + i;  // plane % 4 == 0: a quad never straddles planes
        const f32x4 m = *reinterpret_cast<const f32x4*>(mask + mi);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ks = k[e] * alpha + z[e] * sigma;
            o[e] = m[e] * ks + (1.0f - m[e]) * u[e];
        }
        *reinterpret_cast<f32x4*>(out + base + i) = o;
    }
}

__global__ __launch_bounds__(256) void q_step_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                     const float* __restrict__ coef, float* __restrict__ out, long per_sample) {
    const int b = blockIdx.y;
    const float a = coef[2 * b], sd = coef[2 * b + 1];
    const long base = b * per_sample;
    for (long i = (blockIdx.x * 256L + threadIdx.x) * 4; i < per_sample; i += (long)gridDim.x * 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + base + i), z = *reinterpret_cast<const f32x4*>(noise + base + i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e] * a + sd * z[e];
        *reinterpret_cast<f32x4*>(out + base + i) = o;
    }
}
#pragma clang fp contract(fast)

hipError_t launch_repaint_blend(const float* known, const float* noise, const float* unknown, const float* mask,
                                const float* coef, float* out, int B, long per_sample, int channels, int mask_c,
                                hipStream_t s) {
    if (per_sample % 4 || channels <= 0 || per_sample % channels || (per_sample / channels) % 4) return hipErrorInvalidValue;
    if (mask_c != 1 && mask_c != channels) return hipErrorInvalidValue;
    long bx = (per_sample / 4 + 255) / 256;
    if (bx > 256) bx = 256;
    repaint_blend_kernel<<<dim3((unsigned)bx, B), 256, 0, s>>>(known, noise, unknown, mask, coef, out, per_sample,
                                                               per_sample / channels, mask_c);
    return hipGetLastError();
}

hipError_t launch_q_step(const float* x, const float* noise, const float* coef, float* out, int B, long per_sample,
                         hipStream_t s) {
    if (per_sample % 4) return hipErrorInvalidValue;
    long bx = (per_sample / 4 + 255) / 256;
    if (bx > 256) bx = 256;
    q_step_kernel<<<dim3((unsigned)bx, B), 256, 0, s>>>(x, noise, coef, out, per_sample);
    return hipGetLastError();
}

// ---- denoising loss (reference base.py:122-139 p_loss: target, criterion, mask, the two sums) -----------------------------
// One pass over prediction, x_0, noise and the mask.  Per element, float32 in the reference's operation order:
//   target  eps: noise | x_0: x_0 | v: alpha * noise - sigma * x_0          (continuous_time.py:140-151, discrete_time.py:93-102)
//   d = prediction - target;  l2: d * d | l1: |d| | huber: |d| < 1 ? 0.5 d d : |d| - 0.5   (base.py:39-44, SmoothL1Loss with beta = 1)
//   ... times the mask value (base.py:135).
// Sums in float64 and in a fixed order: thread (grid-stride over ONE (sample, channel) plane) -> wave -> the block's four waves ->
// part[b][c][block] = (sum of loss * mask, sum of mask); loss_finalize_kernel then adds a plane's blocks in index order.  The
// number of blocks per plane depends on `plane` alone, so a sample's sums do not depend on the batch it is in; no atomics.
// A plane that is a multiple of 4 is read as 16-byte quads (every plane then starts on a quad); any other plane element by element.
enum { CRIT_L2 = 0, CRIT_L1 = 1, CRIT_HUBER = 2 };
constexpr int kLossMaxBlocks = 16;  // blocks per plane: 16 x 1024 elements per pass
static int loss_blocks(long plane) {
    const long n = (plane + 1023) / 1024;
    return n < 1 ? 1 : n > kLossMaxBlocks ? kLossMaxBlocks : (int)n;
}
size_t diffusion_loss_scratch_bytes(int B, int C, long plane) { return (size_t)B * C * loss_blocks(plane) * 2 * sizeof(double); }

#pragma clang fp contract(off)
template <int OBJ, int CRIT>
__device__ __forceinline__ float loss_elem(float pr, float x0, float z, float alpha, float sigma) {
    float target;
    if (OBJ == OBJ_EPS) target = z;
    else if (OBJ == OBJ_X0) target = x0;
    else target = alpha * z - sigma * x0;
    const float d = pr - target;
    if (CRIT == CRIT_L2) return d * d;
    const float ad = fabsf(d);
    if (CRIT == CRIT_L1) return ad;
    return ad < 1.0f ? 0.5f * ad * ad : ad - 0.5f;
}

template <int OBJ, int CRIT>
__global__ __launch_bounds__(256) void diffusion_loss_kernel(const float* __restrict__ pred, const float* __restrict__ x_0,
                                                             const float* __restrict__ noise, const float* __restrict__ mask,
                                                             const float* __restrict__ coef, double* __restrict__ part, long plane,
                                                             int mask_c) {
    const int c = blockIdx.y, b = blockIdx.z, C = gridDim.y;
    float alpha = 0.f, sigma = 0.f;
    if (OBJ == OBJ_V) alpha = coef[2 * b], sigma = coef[2 * b + 1];
    const long base = ((long)b * C + c) * plane;
    const float *pp = pred + base, *xp = x_0 + base, *zp = noise + base;
    const float* mp = mask ? mask + (mask_c == 1 ? (long)b * plane : base) : nullptr;
    double num = 0.0, den = 0.0;
    if ((plane & 3) == 0) {
        const long n4 = plane >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const f32x4 p = reinterpret_cast<const f32x4*>(pp)[i], x = reinterpret_cast<const f32x4*>(xp)[i];
            const f32x4 z = reinterpret_cast<const f32x4*>(zp)[i];
            f32x4 m = {1.f, 1.f, 1.f, 1.f};
            if (mp) m = reinterpret_cast<const f32x4*>(mp)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float l = loss_elem<OBJ, CRIT>(p[e], x[e], z[e], alpha, sigma);
                if (mp) l = l * m[e];
                num += (double)l;
                den += (double)m[e];
            }
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < plane; i += (long)gridDim.x * 256) {
            const float m = mp ? mp[i] : 1.f;
            float l = loss_elem<OBJ, CRIT>(pp[i], xp[i], zp[i], alpha, sigma);
            if (mp) l = l * m;
            num += (double)l;
            den += (double)m;
        }
    }
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    __shared__ double sh[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[0][wave] = num, sh[1][wave] = den;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = part + (((long)b * C + c) * gridDim.x + blockIdx.x) * 2;
        o[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
        o[1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    }
}
#pragma clang fp contract(fast)

// num[b][c] = a plane's block sums in index order; den[b] = the mask's own elements: its `den_c` planes (1 or C) in channel order, or, with
// no mask, C * plane exactly
__global__ __launch_bounds__(64) void loss_finalize_kernel(const double* __restrict__ part, double* __restrict__ num, double* __restrict__ den,
                                                           int C, int blocks, int den_c, double den_all) {
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 64) {
        const double* p = part + ((long)b * C + c) * blocks * 2;
        double s = 0.0;
        for (int j = 0; j < blocks; ++j) s += p[2 * j];
        num[(long)b * C + c] = s;
    }
    if (threadIdx.x == 0) {
        double s = den_all;
        if (den_c > 0) {
            s = 0.0;
            for (int c = 0; c < den_c; ++c)
                for (int j = 0; j < blocks; ++j) s += part[(((long)b * C + c) * blocks + j) * 2 + 1];
        }
        den[b] = s;
    }
}

template <int OBJ>
static hipError_t launch_loss_crit(int crit, dim3 g, hipStream_t s, const float* pred, const float* x_0, const float* noise, const float* mask,
                                   const float* coef, double* part, long plane, int mask_c) {
    switch (crit) {
        case CRIT_L2: diffusion_loss_kernel<OBJ, CRIT_L2><<<g, 256, 0, s>>>(pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        case CRIT_L1: diffusion_loss_kernel<OBJ, CRIT_L1><<<g, 256, 0, s>>>(pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        case CRIT_HUBER: diffusion_loss_kernel<OBJ, CRIT_HUBER><<<g, 256, 0, s>>>(pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (arguments validated by r2dm_diffusion_loss: 1 <= B, C <= 65535, plane >= 1, mask_c in {1, C}, alignment)
hipError_t launch_diffusion_loss(const float* pred, const float* x_0, const float* noise, const float* mask, int mask_c, const float* coef,
                                 int objective, int criterion, int B, int C, long plane, void* scratch, double* num, double* den, hipStream_t s) {
    const int blocks = loss_blocks(plane);
    const dim3 g((unsigned)blocks, (unsigned)C, (unsigned)B);
    double* part = static_cast<double*>(scratch);
    hipError_t e;
    switch (objective) {
        case OBJ_EPS: e = launch_loss_crit<OBJ_EPS>(criterion, g, s, pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        case OBJ_V: e = launch_loss_crit<OBJ_V>(criterion, g, s, pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        case OBJ_X0: e = launch_loss_crit<OBJ_X0>(criterion, g, s, pred, x_0, noise, mask, coef, part, plane, mask_c); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    loss_finalize_kernel<<<B, 64, 0, s>>>(part, num, den, C, blocks, mask ? mask_c : 0, (double)C * (double)plane);
    return hipGetLastError();
}

}  // namespace r2dm
