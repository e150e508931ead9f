// K20: completion metrics -- how good an inpainted scan is (the second results table of the R2DM paper: beam-level upsampling scored by
// the mean absolute error of range and reflectance and by the IoU of segmentation labels, next to interpolation baselines).
//
//  completion_error_kernel   per sample, over the pixels RePaint had to fill in: four counts and six error sums of depth and reflectance,
//                            float64, fixed order, no atomics (the scheme of posterior.hip's diffusion_loss_kernel).
//  confusion_kernel          per sample the classes x classes table of (target label, predicted label): one int32 histogram per block in LDS,
//                            merged into int64 counts by integer atomics (the scheme of metrics.hip's bev_hist_kernel): exact in any order.
//  ensemble_score_kernel     K completions of a scan scored as an ensemble: per scan thirteen float64 sums (CRPS, spread, Brier score), the
//                            per-member errors, the rank histogram and per-pixel maps; the K members of a pixel sorted in registers.
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

// ---- ensemble scores -------------------------------------------------------------------------------------------------------------------
// samples (B,K,5,plane): K completions ("members") of each scan, planes 0 and 4 read; target, known, lo, hi, U, G, E as above.  Member k
// returns at a pixel iff lo < d_k < hi; r^_k = d_k then, else 0; n = the returning members; a NaN member reflectance counts as 0.  Per scan:
//   raw[13]      |U|, |E|, then over E for depth  sum_k |r^_k - r|, sum_{k<l} |r^_k - r^_l|, (m - r)^2 with m = (1/K) sum_k r^_k,
//                (1/(K-1)) sum_k (r^_k - m)^2 (0 at K = 1), the same four for reflectance, sum_U (n/K - g)^2, sum_E n/K, sum_{U \ G} n/K
//   member[2][K] sum_E |r^_k - r| and sum_E |rho_k - rho| per member, in member order
//   rank[K+1]    over E the histogram of #{k : r^_k < r}
//   maps[8]      per pixel n/K, then over the returning members the mean, population std (two-pass), median, min, max of depth (0 without
//                one, std 0 below two), then mean and population std of reflectance over all members; fp64, rounded once to fp32
// One thread per pixel, the K values of a channel in registers (a bucket KB of 8 / 16 / 32 / 64, padded with +inf, which sorts behind every
// member and is never read back: the loops over sorted values stop at K), sorted ascending by a fully unrolled bitonic network of min / max pairs.  Every sum
// over members runs in sorted order, the pair term as the sum of the sorted gaps i (K - i) (x_(i+1) - x_(i)) (non-negative terms, nothing
// cancels), so everything but `member` has the same bits under any permutation of the members.  Float sums: thread -> wave -> the block's
// four waves -> part[b][block][13 + 2K]; ensemble_finalize_kernel adds a scan's blocks in index order.  The number of blocks depends on
// `plane` alone.  The histogram is one int32 table per block in LDS merged by 64-bit integer atomics (confusion_kernel's scheme, below).
constexpr int kEnsValues = 13;
constexpr int kEnsMaxMembers = 64;
constexpr int kEnsThreads = 256;
constexpr int kEnsMaxBlocks = 512;  // blocks per scan: 512 x 256 pixels per pass
static int ensemble_blocks(long plane) {
    const long n = (plane + kEnsThreads - 1) / kEnsThreads;
    return n < 1 ? 1 : n > kEnsMaxBlocks ? kEnsMaxBlocks : (int)n;
}
size_t ensemble_score_scratch_bytes(int B, int K, long plane) {
    return (size_t)B * ensemble_blocks(plane) * (kEnsValues + 2 * K) * sizeof(double);
}

// the bitonic network on KB registers: stage (K, J) compares x[i] with x[i ^ J], ascending where (i & K) == 0; every index is a constant
template <int KB, int K, int J>
__device__ __forceinline__ void sort_stage(float (&x)[KB]) {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        const int l = i ^ J;
        if (l > i) {
            const float lo = __builtin_fminf(x[i], x[l]), hi = __builtin_fmaxf(x[i], x[l]);  // (no NaN gets here; -0 sorts below +0)
            x[i] = (i & K) == 0 ? lo : hi;
            x[l] = (i & K) == 0 ? hi : lo;
        }
    }
    if constexpr (J > 1)
        sort_stage<KB, K, J / 2>(x);
    else if constexpr (K < KB)
        sort_stage<KB, 2 * K, K>(x);
}

// sum_E |x_k - t| per member: eight members per butterfly; afterwards lane L holds the wave's total of member 8 j + ((L >> 3) & 7) in m[j]
template <int KB>
__device__ __forceinline__ void member_sums(double (&m)[KB / 8], const float (&x)[KB], float t, bool e, int K, int lane) {
#pragma unroll
    for (int j = 0; j < KB / 8; ++j) {
        if (8 * j < K) {  // uniform
            double v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = e && 8 * j + i < K ? fabs((double)x[8 * j + i] - (double)t) : 0.0;
            m[j] += wave_sum8_scatter(v, lane);
        }
    }
}

// the four sums of one channel over the sorted members x[0 .. K): sum |x - t|, the pair term, the mean, sum (x - mean)^2
template <int KB>
__device__ __forceinline__ void sorted_sums(const float (&x)[KB], double t, int K, double& sabs, double& pair, double& mean, double& ss) {
    double s = 0.0;
    sabs = 0.0, pair = 0.0, ss = 0.0;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (i < K) {
            s += (double)x[i];
            sabs += fabs((double)x[i] - t);
        }
    }
    mean = s / (double)K;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (i < K) {
            const double d = (double)x[i] - mean;
            ss += d * d;
        }
    }
#pragma unroll
    for (int i = 0; i + 1 < KB; ++i) {
        if (i + 1 < K) pair += (double)((i + 1) * (K - 1 - i)) * ((double)x[i + 1] - (double)x[i]);
    }
}

// FULL: K == KB, no padding (the usual sizes 8, 16, 32, 64): K is a constant then and every guard on it folds away
template <int KB, bool FULL, bool MAPS>
__global__ __launch_bounds__(kEnsThreads) void ensemble_score_kernel(const float* __restrict__ samples, const float* __restrict__ target,
                                                                     const float* __restrict__ known, double* __restrict__ part,
                                                                     unsigned long long* __restrict__ rank, float* __restrict__ maps, long plane,
                                                                     int members, float lo, float hi) {
    const int K = FULL ? KB : members;
    __shared__ int hist[kEnsMaxMembers + 1];
    __shared__ double sh[4][kEnsValues + 2 * kEnsMaxMembers];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid <= K) hist[tid] = 0;
    __syncthreads();
    const float* sb = samples + (long)b * K * 5 * plane;
    const float *td = target + (long)b * 5 * plane, *tr = td + 4 * plane;
    const float* kn = known + (long)b * plane;
    float* mp = MAPS ? maps + (long)b * 8 * plane : nullptr;
    const float pad = __builtin_inff();
    double acc[kEnsValues], md[KB / 8], mr[KB / 8];
#pragma unroll
    for (int j = 0; j < kEnsValues; ++j) acc[j] = 0.0;
#pragma unroll
    for (int j = 0; j < KB / 8; ++j) md[j] = 0.0, mr[j] = 0.0;

    for (long base = blockIdx.x * (long)kEnsThreads; base < plane; base += (long)gridDim.x * kEnsThreads) {  // uniform over the block
        const long pix = base + tid;
        const bool valid = pix < plane;
        const long at = valid ? pix : plane - 1;  // every lane loads (a lane past the end its scan's last pixel, a padded slot member K - 1)
        const float kv = kn[at], r = td[at], rho = tr[at];
        const bool u = valid && kv == 0.f, g = lo < r && r < hi, e = u && g;
        float x[KB];
        double sabs, pair, mean, ss;

        // depth
        int n = 0, below = 0;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const float d = sb[(long)(k < K ? k : K - 1) * 5 * plane + at];
            const bool ret = k < K && lo < d && d < hi;
            x[k] = k >= K ? pad : ret ? d : 0.f;
            n += ret;
            below += x[k] < r;
        }
        member_sums<KB>(md, x, r, e, K, lane);
        sort_stage<KB, 2, 1>(x);
        sorted_sums<KB>(x, (double)r, K, sabs, pair, mean, ss);
        const double p = (double)n / (double)K;
        if (u) {
            const double q = p - (g ? 1.0 : 0.0);
            acc[0] += 1.0;
            acc[10] += q * q;
            if (!g) acc[12] += p;
        }
        if (e) {
            acc[1] += 1.0;
            acc[2] += sabs;
            acc[3] += pair;
            acc[4] += (mean - (double)r) * (mean - (double)r);
            if (K > 1) acc[5] += ss / (double)(K - 1);
            acc[11] += p;
            atomicAdd(&hist[below], 1);
        }
        if (MAPS && valid) {
            // the returning members are the sorted values without K - n of the zeros (a dropped member is stored as 0)
            int skip = K - n, seen = 0;
            const int h0 = (n - 1) >> 1, h1 = n >> 1;
            double sum = 0.0, mn = 0.0, mx = 0.0, m0 = 0.0, m1 = 0.0;
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                const bool dropped = x[i] == 0.f && skip > 0;
                if (i < K && dropped) --skip;
                if (i < K && !dropped) {
                    const double v = (double)x[i];
                    sum += v;
                    mn = seen == 0 ? v : mn;
                    mx = v;
                    m0 = seen == h0 ? v : m0;
                    m1 = seen == h1 ? v : m1;
                    ++seen;
                }
            }
            const double dm = n > 0 ? sum / (double)n : 0.0;
            double dev = 0.0;
            skip = K - n;
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                const bool dropped = x[i] == 0.f && skip > 0;
                if (i < K && dropped) --skip;
                if (i < K && !dropped) {
                    const double d = (double)x[i] - dm;
                    dev += d * d;
                }
            }
            mp[pix] = (float)p;
            mp[plane + pix] = (float)dm;
            mp[2 * plane + pix] = n > 1 ? (float)sqrt(dev / (double)n) : 0.f;
            mp[3 * plane + pix] = n > 0 ? (float)((m0 + m1) * 0.5) : 0.f;
            mp[4 * plane + pix] = (float)mn;
            mp[5 * plane + pix] = (float)mx;
        }

        // reflectance
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const float v = sb[((long)(k < K ? k : K - 1) * 5 + 4) * plane + at];
            x[k] = k >= K ? pad : v != v ? 0.f : v;
        }
        member_sums<KB>(mr, x, rho, e, K, lane);
        sort_stage<KB, 2, 1>(x);
        sorted_sums<KB>(x, (double)rho, K, sabs, pair, mean, ss);
        if (e) {
            acc[6] += sabs;
            acc[7] += pair;
            acc[8] += (mean - (double)rho) * (mean - (double)rho);
            if (K > 1) acc[9] += ss / (double)(K - 1);
        }
        if (MAPS && valid) {
            mp[6 * plane + pix] = (float)mean;
            mp[7 * plane + pix] = (float)sqrt(ss / (double)K);
        }
    }

    {  // the thirteen sums, eight at a time: lane L ends up with the wave's total of value (L >> 3) & 7
        double lo8[8], hi8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lo8[j] = acc[j], hi8[j] = j + 8 < kEnsValues ? acc[j + 8] : 0.0;
        const double t0 = wave_sum8_scatter(lo8, lane), t1 = wave_sum8_scatter(hi8, lane);
        if ((lane & 7) == 0) {
            sh[wave][lane >> 3] = t0;
            if ((lane >> 3) + 8 < kEnsValues) sh[wave][(lane >> 3) + 8] = t1;
        }
    }
#pragma unroll
    for (int j = 0; j < KB / 8; ++j) {
        const int k = 8 * j + (lane >> 3);
        if ((lane & 7) == 0 && k < K) sh[wave][kEnsValues + k] = md[j], sh[wave][kEnsValues + K + k] = mr[j];
    }
    __syncthreads();
    const int stride = kEnsValues + 2 * K;
    if (tid < stride) part[((long)b * gridDim.x + blockIdx.x) * stride + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    if (tid <= K && hist[tid]) atomicAdd(&rank[(long)b * (K + 1) + tid], (unsigned long long)hist[tid]);
}

__global__ __launch_bounds__(kEnsThreads) void ensemble_finalize_kernel(const double* __restrict__ part, double* __restrict__ raw,
                                                                        double* __restrict__ member, int blocks, int K) {
    const int b = blockIdx.x, j = threadIdx.x, stride = kEnsValues + 2 * K;
    if (j >= stride) return;
    double s = 0.0;
    const double* p = part + (long)b * blocks * stride + j;
    for (int k0 = 0; k0 < blocks; k0 += 32) {  // thirty-two loads in flight, added in index order
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = k0 + i < blocks ? p[(long)(k0 + i) * stride] : 0.0;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (k0 + i < blocks) s += v[i];
    }
    if (j < kEnsValues)
        raw[(long)b * kEnsValues + j] = s;
    else
        member[(long)b * 2 * K + (j - kEnsValues)] = s;
}

template <int KB>
static hipError_t ensemble_launch(const float* samples, const float* target, const float* known, double* part, long long* rank, float* maps,
                                  long plane, int K, float lo, float hi, dim3 grid, hipStream_t s) {
    auto* rk = reinterpret_cast<unsigned long long*>(rank);
    if (K == KB && maps)
        ensemble_score_kernel<KB, true, true><<<grid, kEnsThreads, 0, s>>>(samples, target, known, part, rk, maps, plane, K, lo, hi);
    else if (K == KB)
        ensemble_score_kernel<KB, true, false><<<grid, kEnsThreads, 0, s>>>(samples, target, known, part, rk, nullptr, plane, K, lo, hi);
    else if (maps)
        ensemble_score_kernel<KB, false, true><<<grid, kEnsThreads, 0, s>>>(samples, target, known, part, rk, maps, plane, K, lo, hi);
    else
        ensemble_score_kernel<KB, false, false><<<grid, kEnsThreads, 0, s>>>(samples, target, known, part, rk, nullptr, plane, K, lo, hi);
    return hipGetLastError();
}

// (arguments validated by r2dm_ensemble_score: 1 <= B <= 65535, 1 <= K <= 64, plane >= 1, alignment; maps may be null)
hipError_t launch_ensemble_score(const float* samples, const float* target, const float* known, float lo, float hi, int B, int K, long plane,
                                 void* scratch, double* raw, double* member, long long* rank, float* maps, hipStream_t s) {
    if (B < 1 || K < 1 || K > kEnsMaxMembers || plane < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(rank, 0, sizeof(long long) * (size_t)B * (K + 1), s);
    if (e != hipSuccess) return e;
    const int blocks = ensemble_blocks(plane);
    double* part = static_cast<double*>(scratch);
    const dim3 grid((unsigned)blocks, (unsigned)B);
    if (K <= 8)
        e = ensemble_launch<8>(samples, target, known, part, rank, maps, plane, K, lo, hi, grid, s);
    else if (K <= 16)
        e = ensemble_launch<16>(samples, target, known, part, rank, maps, plane, K, lo, hi, grid, s);
    else if (K <= 32)
        e = ensemble_launch<32>(samples, target, known, part, rank, maps, plane, K, lo, hi, grid, s);
    else
        e = ensemble_launch<64>(samples, target, known, part, rank, maps, plane, K, lo, hi, grid, s);
    if (e != hipSuccess) return e;
    ensemble_finalize_kernel<<<B, kEnsThreads, 0, s>>>(part, raw, member, blocks, K);
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
