// K10: fused posterior update  x_t, prediction, noise -> x_s  (one HBM pass: 3 reads + 1 write).
//
// Replays, per element and in the reference's float32 operation order (no FMA contraction, IEEE
// division), the tail of p_step:
//   continuous time  /root/reference/models/diffusion/continuous_time.py:208-229
//   discrete time    /root/reference/models/diffusion/discrete_time.py:140-177
// All schedule scalars arrive in coef[b][8], computed on the host with the reference's torch ops.
//
// The sampler steps are two kernels over the same two halves (posterior_x0, then the update from it):
//   posterior_kernel<MODE, OBJ, KNOWN>          r2dm_posterior_step, and with a measurement r2dm_posterior_step_known (DDNM)
//   dpm_step_kernel<OBJ, SECOND, NOISE, KNOWN>  r2dm_dpm_step and r2dm_dpm_step_known (DPM-Solver++(2M))
//
// also: K12 LiDAR post-processing of finished samples (reference sample_and_save.py:52-57), the RePaint pieces and the denoising loss.
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

enum { M_CT_DDPM = 0, M_CT_DDIM = 1, M_DT_DDPM = 2, M_DT_DDIM = 3, M_DT_DDIM_NOISE = 4 };

// The measurement of a data-consistent step: known (B, per_sample) and its per-pixel weight mask, which has mask_c channels of `plane`
// elements (1 = broadcast over the planes of a sample).  plane % 4 == 0: a quad never straddles planes.
struct Measurement {
    const float* known;
    const float* mask;
    long plane;
    int mask_c;
};

// the mask's quad for quad i of sample b
__device__ __forceinline__ f32x4 mask_quad(const float* mask, int b, long i, long per_sample, long plane, int mask_c) {
    return *reinterpret_cast<const f32x4*>(mask + (mask_c == 1 ? b * plane + (i << 2) % plane : b * per_sample + (i << 2)));
}

__device__ __forceinline__ void load_coef_row(const float* coef, int b, float (&k)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = coef[b * 8 + i];
}

#pragma clang fp contract(off)
// the two halves of one element's update: the clamped estimate of x_0, and x_s from it (a measurement goes between them: project_known)
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

// DDNM's null-space projection for a mask operator: the measurement y written over the estimate with weight m (not necessarily binary)
__device__ __forceinline__ float project_known(float m, float y, float x0) { return m * y + (1.0f - m) * x0; }

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

// x_t, prediction[, noise][, known, mask] -> x_s in one pass of 16-byte quads (2 to 5 reads + 1 write).  The noise is a property of MODE: M_DT_DDIM
// reads none, every other mode needs it.  KNOWN: project_known between the two halves (r2dm_posterior_step_known); ms is not read without it.
template <int MODE, int OBJ, bool KNOWN>
__global__ __launch_bounds__(256) void posterior_kernel(PosteriorParams p, Measurement ms) {
    constexpr bool NOISE = MODE != M_DT_DDIM;
    const int b = blockIdx.y;
    float k[8];
    load_coef_row(p.coef, b, k);
    const long n4 = p.per_sample >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x_t + b * p.per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p.pred + b * p.per_sample);
    const f32x4* z4 = NOISE ? reinterpret_cast<const f32x4*>(p.noise + b * p.per_sample) : nullptr;
    const f32x4* y4 = KNOWN ? reinterpret_cast<const f32x4*>(ms.known + b * p.per_sample) : nullptr;
    f32x4* o4 = reinterpret_cast<f32x4*>(p.x_s + b * p.per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 z = {0.f, 0.f, 0.f, 0.f}, y = z, m = z;
        if (NOISE) z = z4[i];
        if (KNOWN) y = y4[i], m = mask_quad(ms.mask, b, i, p.per_sample, ms.plane, ms.mask_c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x0 = posterior_x0<MODE, OBJ>(x[j], pr[j], k, p.clip);
            if (KNOWN) x0 = project_known(m[j], y[j], x0);
            o[j] = posterior_update<MODE>(x[j], x0, z[j], k);
        }
        o4[i] = o;
    }
}

template <int MODE, bool KNOWN>
static hipError_t launch_posterior_obj(const PosteriorParams& p, const Measurement& ms, hipStream_t s) {
    const dim3 g = quad_grid(p.B, p.per_sample);
    switch (p.objective) {
        case OBJ_EPS: posterior_kernel<MODE, OBJ_EPS, KNOWN><<<g, 256, 0, s>>>(p, ms); break;
        case OBJ_V: posterior_kernel<MODE, OBJ_V, KNOWN><<<g, 256, 0, s>>>(p, ms); break;
        case OBJ_X0: posterior_kernel<MODE, OBJ_X0, KNOWN><<<g, 256, 0, s>>>(p, ms); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (the kernel reads quads and has no tail)
hipError_t launch_posterior(const PosteriorParams& p, hipStream_t s) {
    if ((p.per_sample & 3) || (reinterpret_cast<uintptr_t>(p.x_t) & 15) || (reinterpret_cast<uintptr_t>(p.pred) & 15) ||
        (reinterpret_cast<uintptr_t>(p.x_s) & 15) || (reinterpret_cast<uintptr_t>(p.noise) & 15))
        return hipErrorInvalidValue;
    if (p.noise == nullptr && p.mode != M_DT_DDIM) return hipErrorInvalidValue;
    switch (p.mode) {
        case M_CT_DDPM: return launch_posterior_obj<M_CT_DDPM, false>(p, {}, s);
        case M_CT_DDIM: return launch_posterior_obj<M_CT_DDIM, false>(p, {}, s);
        case M_DT_DDPM: return launch_posterior_obj<M_DT_DDPM, false>(p, {}, s);
        case M_DT_DDIM: return launch_posterior_obj<M_DT_DDIM, false>(p, {}, s);
        case M_DT_DDIM_NOISE: return launch_posterior_obj<M_DT_DDIM_NOISE, false>(p, {}, s);
    }
    return hipErrorInvalidValue;
}

// the geometry a measurement needs: whole planes of whole quads, a mask of one plane or of all
static bool measurement_ok(long per_sample, int channels, int mask_c) {
    return channels >= 1 && per_sample % channels == 0 && (per_sample / channels) % 4 == 0 && (mask_c == 1 || mask_c == channels);
}

// The data-consistent posterior step, continuous time only.  (arguments validated by r2dm_posterior_step_known; checked again here, since the kernel
// reads quads and has no tail)
hipError_t launch_posterior_known(const PosteriorParams& p, const float* known, const float* mask, int channels, int mask_c,
                                  hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.per_sample < 4 || (p.per_sample & 3) || !measurement_ok(p.per_sample, channels, mask_c) || !p.noise || !known || !mask)
        return hipErrorInvalidValue;
    const Measurement ms{known, mask, p.per_sample / channels, mask_c};
    switch (p.mode) {
        case M_CT_DDPM: return launch_posterior_obj<M_CT_DDPM, true>(p, ms, s);
        case M_CT_DDIM: return launch_posterior_obj<M_CT_DDIM, true>(p, ms, s);
    }
    return hipErrorInvalidValue;
}

// ---- DPM-Solver++(2M) update (Lu et al. 2022, the data-prediction multistep solver on the half-log-SNR axis) --------------------------------
// x_t, prediction[, x0_prev][, noise][, known, mask] -> x_s, x0 in one pass (2 to 6 reads + 2 writes).  coef[b] = (alpha_t, sigma_t, c_x, c_0, c_1,
// c_z, 0, 0), host-computed.  x0 is the clamped estimate of posterior_x0, with a measurement projected like posterior_kernel's; it is written AFTER
// the projection: that is the history the next step extrapolates from.  x_s = c_x x + c_0 x0 (first order, x0_prev not read) or
// (c_x x + c_0 x0) + c_1 x0_prev, then + c_z z: completion and the stochastic member (SDE-DPM-Solver++(2M)).  An absent operand is a template
// argument: no load, no arithmetic; r2dm_dpm_step is <OBJ, SECOND, false, false>.  x0 may be x0_prev's buffer: a thread reads its quad of x0_prev
// before it writes the same quad of x0, and no other thread touches that quad -- hence no __restrict__ on the two (DpmParams' members).
template <int OBJ, bool SECOND, bool NOISE, bool KNOWN>
__global__ __launch_bounds__(256) void dpm_step_kernel(DpmParams p, const float* __restrict__ noise, Measurement ms) {
    const int b = blockIdx.y;
    float k[8];
    load_coef_row(p.coef, b, k);
    const float c_x = k[2], c_0 = k[3], c_1 = k[4], c_z = k[5];
    const long n4 = p.per_sample >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x_t + b * p.per_sample);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p.pred + b * p.per_sample);
    const f32x4* h4 = SECOND ? reinterpret_cast<const f32x4*>(p.x0_prev + b * p.per_sample) : nullptr;
    const f32x4* z4 = NOISE ? reinterpret_cast<const f32x4*>(noise + b * p.per_sample) : nullptr;
    const f32x4* y4 = KNOWN ? reinterpret_cast<const f32x4*>(ms.known + b * p.per_sample) : nullptr;
    f32x4* o4 = reinterpret_cast<f32x4*>(p.x_s + b * p.per_sample);
    f32x4* e4 = reinterpret_cast<f32x4*>(p.x0 + b * p.per_sample);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 x = x4[i], pr = p4[i];
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, z = h, y = h, m = h;
        if (SECOND) h = h4[i];
        if (NOISE) z = z4[i];
        if (KNOWN) y = y4[i], m = mask_quad(ms.mask, b, i, p.per_sample, ms.plane, ms.mask_c);
        f32x4 o, e;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = posterior_x0<M_CT_DDPM, OBJ>(x[j], pr[j], k, p.clip);
            if (KNOWN) e[j] = project_known(m[j], y[j], e[j]);
            o[j] = c_x * x[j] + c_0 * e[j];
            if (SECOND) o[j] = o[j] + c_1 * h[j];
            if (NOISE) o[j] = o[j] + c_z * z[j];
        }
        o4[i] = o;
        e4[i] = e;
    }
}

template <int OBJ, bool SECOND, bool NOISE>
static hipError_t launch_dpm_k(const DpmParams& p, const float* noise, const Measurement& ms, hipStream_t s) {
    const dim3 g = quad_grid(p.B, p.per_sample);
    if (ms.known) dpm_step_kernel<OBJ, SECOND, NOISE, true><<<g, 256, 0, s>>>(p, noise, ms);
    else dpm_step_kernel<OBJ, SECOND, NOISE, false><<<g, 256, 0, s>>>(p, noise, ms);
    return hipGetLastError();
}

template <int OBJ>
static hipError_t launch_dpm_obj(const DpmParams& p, const float* noise, const Measurement& ms, hipStream_t s) {
    if (p.x0_prev) return noise ? launch_dpm_k<OBJ, true, true>(p, noise, ms, s) : launch_dpm_k<OBJ, true, false>(p, noise, ms, s);
    return noise ? launch_dpm_k<OBJ, false, true>(p, noise, ms, s) : launch_dpm_k<OBJ, false, false>(p, noise, ms, s);
}

// (arguments validated by r2dm_dpm_step_known; checked again here, since the kernel reads quads and has no tail)
hipError_t launch_dpm_step_known(const DpmParams& p, const float* noise, const float* known, const float* mask, int channels, int mask_c,
                                 hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.per_sample < 4 || (p.per_sample & 3) || !p.x_t || !p.pred || !p.coef || !p.x_s || !p.x0 || p.x_s == p.x_t ||
        !measurement_ok(p.per_sample, channels, mask_c) || !known != !mask)
        return hipErrorInvalidValue;
    const Measurement ms{known, mask, p.per_sample / channels, mask_c};
    switch (p.objective) {
        case OBJ_EPS: return launch_dpm_obj<OBJ_EPS>(p, noise, ms, s);
        case OBJ_V: return launch_dpm_obj<OBJ_V>(p, noise, ms, s);
        case OBJ_X0: return launch_dpm_obj<OBJ_X0>(p, noise, ms, s);
    }
    return hipErrorInvalidValue;
}

// no noise, no measurement: one plane, which asks nothing of per_sample beyond whole quads
hipError_t launch_dpm_step(const DpmParams& p, hipStream_t s) { return launch_dpm_step_known(p, nullptr, nullptr, nullptr, 1, 1, s); }

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
        const f32x4 m = mask_quad(mask, b, i >> 2, per_sample, plane, mask_c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = project_known(m[e], k[e] * alpha + z[e] * sigma, u[e]);
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
    if (per_sample % 4 || !measurement_ok(per_sample, channels, mask_c)) return hipErrorInvalidValue;
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
