// K20: completion metrics -- how good an inpainted scan is (the second results table of the R2DM paper: beam-level upsampling scored by
// the mean absolute error of range and reflectance and by the IoU of segmentation labels, next to interpolation baselines).
//
//  completion_error_kernel   per sample, over the pixels RePaint had to fill in: four counts and six error sums of depth and reflectance,
//                            float64, fixed order, no atomics (the scheme of posterior.hip's diffusion_loss_kernel).
//  confusion_kernel          per sample the classes x classes table of (target label, predicted label): one int32 histogram per block in LDS,
//                            merged into int64 counts by integer atomics (the scheme of metrics.hip's bev_hist_kernel): exact in any order.
//  fill_beams_kernel         the baselines: an unknown beam (image row) from the nearest known beam above and below it, nearest or linear.
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

#pragma clang fp contract(off)

// ---- range / reflectance error ---------------------------------------------------------------------------------------------------------
// pred, target (B,5,plane) [depth, x, y, z, reflectance] (planes 0 and 4 are read), known (B,1,plane) zeros and ones.  Per sample:
//   U = {known == 0}   G = {lo < target depth < hi}   P = {lo < pred depth < hi}   (a NaN depth is in neither: "no return")
//   E = U & G          Bo = E & P                      r^ = pred depth on P, else 0 (what postprocess stores for a dropped ray)
//   out[b] = |U|, |E|, |Bo|, |U & P \ G|, sum_E |r^ - r|, sum_E (r^ - r)^2, sum_Bo |dr|, sum_Bo dr^2, sum_E |drho|, sum_E drho^2
// Every fp32 value is widened to float64 first, so the differences are exact; squares and sums are float64.  Order: thread (grid-stride over
// ONE sample's plane) -> wave -> the block's four waves -> part[b][block][10]; completion_finalize_kernel adds a sample's blocks in index
// order.  The number of blocks depends on `plane` alone: a sample's numbers do not depend on the batch it is in.
constexpr int kErrValues = 10;
constexpr int kErrMaxBlocks = 16;  // blocks per sample: 16 x 1024 pixels per pass
static int error_blocks(long plane) {
    const long n = (plane + 1023) / 1024;
    return n < 1 ? 1 : n > kErrMaxBlocks ? kErrMaxBlocks : (int)n;
}
size_t completion_error_scratch_bytes(int B, long plane) { return (size_t)B * error_blocks(plane) * kErrValues * sizeof(double); }

__device__ __forceinline__ void error_elem(double (&acc)[kErrValues], float k, float r, float pd, float tr, float pr, float lo, float hi) {
    if (!(k == 0.f)) return;
    const bool g = lo < r && r < hi, p = lo < pd && pd < hi;
    acc[0] += 1.0;
    if (g) {
        const double d = (double)(p ? pd : 0.f) - (double)r, ad = fabs(d), dd = d * d;
        const double e = (double)pr - (double)tr;
        acc[1] += 1.0;
        acc[4] += ad;
        acc[5] += dd;
        acc[8] += fabs(e);
        acc[9] += e * e;
        if (p) {
            acc[2] += 1.0;
            acc[6] += ad;
            acc[7] += dd;
        }
    } else if (p) {
        acc[3] += 1.0;
    }
}

__global__ __launch_bounds__(256) void completion_error_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               const float* __restrict__ known, double* __restrict__ part, long plane, float lo,
                                                               float hi) {
    const int b = blockIdx.y;
    const float *pd = pred + (long)b * 5 * plane, *pr = pd + 4 * plane;
    const float *td = target + (long)b * 5 * plane, *tr = td + 4 * plane;
    const float* kn = known + (long)b * plane;
    double acc[kErrValues];
#pragma unroll
    for (int j = 0; j < kErrValues; ++j) acc[j] = 0.0;
    if ((plane & 3) == 0) {
        const long n4 = plane >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const f32x4 k = reinterpret_cast<const f32x4*>(kn)[i];
            const f32x4 r = reinterpret_cast<const f32x4*>(td)[i], q = reinterpret_cast<const f32x4*>(pd)[i];
            const f32x4 a = reinterpret_cast<const f32x4*>(tr)[i], c = reinterpret_cast<const f32x4*>(pr)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) error_elem(acc, k[e], r[e], q[e], a[e], c[e], lo, hi);
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < plane; i += (long)gridDim.x * 256)
            error_elem(acc, kn[i], td[i], pd[i], tr[i], pr[i], lo, hi);
    }
    __shared__ double sh[kErrValues][4];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kErrValues; ++j) {
        const double v = wave_sum_f64(acc[j]);
        if ((threadIdx.x & 63) == 0) sh[j][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < kErrValues) {
        const int j = threadIdx.x;
        part[((long)b * gridDim.x + blockIdx.x) * kErrValues + j] = ((sh[j][0] + sh[j][1]) + sh[j][2]) + sh[j][3];
    }
}

__global__ __launch_bounds__(64) void completion_finalize_kernel(const double* __restrict__ part, double* __restrict__ out, int blocks) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= kErrValues) return;
    double s = 0.0;
    for (int k = 0; k < blocks; ++k) s += part[((long)b * blocks + k) * kErrValues + j];
    out[(long)b * kErrValues + j] = s;
}

// (arguments validated by r2dm_completion_error: 1 <= B <= 65535, plane >= 1, alignment)
hipError_t launch_completion_error(const float* pred, const float* target, const float* known, float lo, float hi, int B, long plane, void* scratch,
                                   double* out, hipStream_t s) {
    const int blocks = error_blocks(plane);
    double* part = static_cast<double*>(scratch);
    completion_error_kernel<<<dim3((unsigned)blocks, (unsigned)B), 256, 0, s>>>(pred, target, known, part, plane, lo, hi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    completion_finalize_kernel<<<B, 64, 0, s>>>(part, out, blocks);
    return hipGetLastError();
}

// ---- confusion matrix ------------------------------------------------------------------------------------------------------------------
// counts[b][t][p] += 1 for every pixel of sample b whose mask is not 0 (mask nullptr: every pixel) with target label t and predicted label
// p.  A label outside [0, classes) indexes nothing: the pixel is counted in *bad.  A block takes a contiguous run of fewer than 2^31 pixels,
// so its int32 counters cannot overflow.
constexpr int kConfThreads = 256;
constexpr int kConfMaxClasses = 64;    // 64 x 64 int32 = 16 KiB of LDS
constexpr long kConfMaxSplit = 1024;   // blocks per sample; with pixels <= 2^40 a block takes at most 2^30
constexpr long kConfMinRun = 16L * kConfThreads;

__global__ __launch_bounds__(kConfThreads) void confusion_kernel(const long long* __restrict__ pred, const long long* __restrict__ target,
                                                                 const float* __restrict__ mask, unsigned long long* __restrict__ counts,
                                                                 unsigned long long* __restrict__ bad, long n, int classes) {
    __shared__ int h[kConfMaxClasses * kConfMaxClasses];
    __shared__ int nbad;
    const int b = blockIdx.y, cells = classes * classes;
    for (int i = threadIdx.x; i < cells; i += kConfThreads) h[i] = 0;
    if (threadIdx.x == 0) nbad = 0;
    __syncthreads();
    const long per = (n + gridDim.x - 1) / gridDim.x;
    const long beg = (long)blockIdx.x * per, end = beg + per < n ? beg + per : n;
    const long long *pp = pred + (long)b * n, *tp = target + (long)b * n;
    const float* mp = mask ? mask + (long)b * n : nullptr;
    for (long i = beg + threadIdx.x; i < end; i += kConfThreads) {
        if (mp && mp[i] == 0.f) continue;
        const long long t = tp[i], p = pp[i];
        if (t < 0 || t >= classes || p < 0 || p >= classes) {
            atomicAdd(&nbad, 1);
            continue;
        }
        atomicAdd(&h[(int)t * classes + (int)p], 1);
    }
    __syncthreads();
    unsigned long long* out = counts + (long)b * cells;
    for (int i = threadIdx.x; i < cells; i += kConfThreads)
        if (h[i]) atomicAdd(&out[i], (unsigned long long)h[i]);
    if (threadIdx.x == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// (arguments validated by r2dm_confusion_matrix: 1 <= B <= 65535, 1 <= n <= 2^40, 1 <= classes <= 64)
hipError_t launch_confusion_matrix(const long long* pred, const long long* target, const float* mask, int B, long n, int classes, long long* counts,
                                   long long* bad, hipStream_t s) {
    if (B < 1 || n < 1 || classes < 1 || classes > kConfMaxClasses) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)B * classes * classes, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(bad, 0, sizeof(long long), s);
    if (e != hipSuccess) return e;
    long split = (n + kConfMinRun - 1) / kConfMinRun;
    if (split > kConfMaxSplit) split = kConfMaxSplit;
    if (split < 1) split = 1;
    confusion_kernel<<<dim3((unsigned)split, (unsigned)B), kConfThreads, 0, s>>>(pred, target, mask, reinterpret_cast<unsigned long long*>(counts),
                                                                                reinterpret_cast<unsigned long long*>(bad), n, classes);
    return hipGetLastError();
}

// ---- interpolation baselines -----------------------------------------------------------------------------------------------------------
// x, out (B,C,H,W); rows (B,H) bytes, non-zero = the beam is known.  A known row is copied.  For a pixel (h, w) of an unknown row: `up` / `dn`
// are the nearest known rows above / below (no wrap; found here, by every thread alike, from the sample's row bytes); an endpoint is usable
// if it exists and x[b][0][row][w] != nodata.  MODE 0 nearest: every channel from the usable endpoint at the smaller row distance, `up` on a
// tie.  MODE 1 linear: both usable: a + (b - a) * t, t = float(h - up) / float(dn - up), fp32, IEEE division, no contraction; one usable: a
// copy of it.  No usable endpoint: nodata in every channel.
template <int MODE>
__global__ __launch_bounds__(256) void fill_beams_kernel(const float* __restrict__ x, const unsigned char* __restrict__ rows, float* __restrict__ out,
                                                         int C, int H, int W, float nodata) {
    const int b = blockIdx.z, h = blockIdx.y;
    const int w = blockIdx.x * 256 + threadIdx.x;
    const unsigned char* r = rows + (long)b * H;
    const long plane = (long)H * W;
    const float* xb = x + (long)b * C * plane;
    float* ob = out + (long)b * C * plane;
    if (r[h]) {
        if (w < W)
            for (int c = 0; c < C; ++c) ob[c * plane + (long)h * W + w] = xb[c * plane + (long)h * W + w];
        return;
    }
    int up = h - 1, dn = h + 1;
    while (up >= 0 && !r[up]) --up;
    while (dn < H && !r[dn]) ++dn;
    if (w >= W) return;
    const bool ua = up >= 0 && xb[(long)up * W + w] != nodata;
    const bool ub = dn < H && xb[(long)dn * W + w] != nodata;
    const long o = (long)h * W + w;
    if (!ua && !ub) {
        for (int c = 0; c < C; ++c) ob[c * plane + o] = nodata;
        return;
    }
    if (MODE == 1 && ua && ub) {
        const float t = (float)(h - up) / (float)(dn - up);
        for (int c = 0; c < C; ++c) {
            const float a = xb[c * plane + (long)up * W + w], e = xb[c * plane + (long)dn * W + w];
            ob[c * plane + o] = a + (e - a) * t;
        }
        return;
    }
    const int src = !ub ? up : !ua ? dn : (h - up <= dn - h ? up : dn);
    for (int c = 0; c < C; ++c) ob[c * plane + o] = xb[c * plane + (long)src * W + w];
}

// (arguments validated by r2dm_fill_beams: 1 <= B, H <= 65535, C, W >= 1, mode 0 or 1)
hipError_t launch_fill_beams(const float* x, const unsigned char* rows, float* out, int B, int C, int H, int W, float nodata, int mode, hipStream_t s) {
    const dim3 g((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)B);
    if (mode == 0)
        fill_beams_kernel<0><<<g, 256, 0, s>>>(x, rows, out, C, H, W, nodata);
    else if (mode == 1)
        fill_beams_kernel<1><<<g, 256, 0, s>>>(x, rows, out, C, H, W, nodata);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace r2dm
