// K20: completion metrics -- how good an inpainted scan is (the second results table of the R2DM paper: beam-level upsampling scored by
// the mean absolute error of range and reflectance and by the IoU of segmentation labels, next to interpolation baselines).
//
//  completion_error_kernel   per sample, over the pixels RePaint had to fill in: four counts and six error sums of depth and reflectance,
//                            float64, fixed order, no atomics (the scheme of posterior.hip's diffusion_loss_kernel).
//  confusion_kernel          per sample the classes x classes table of (target label, predicted label): one int32 histogram per block in LDS,
//                            merged into int64 counts by integer atomics (the scheme of metrics.hip's bev_hist_kernel): exact in any order.
//  ensemble_score_kernel     K completions of a scan scored as an ensemble: per scan thirteen float64 sums (CRPS, spread, Brier score), the
//                            per-member errors, the rank histogram and per-pixel maps; the K members of a pixel sorted in registers.
//  coherence_dist_kernel     the same ensemble across pixels: per scan and channel the float64 squared distances between the K members and the
//  coherence_vario_kernel    target (the energy score), and per pixel offset the sums of the variogram score of order 0.5; fixed order.
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

// ---- ensemble coherence ----------------------------------------------------------------------------------------------------------------
// The scores above are per pixel: they cannot tell a coherent draw from one whose pixels were shuffled among the members.  These two can.
// samples, target, known, lo, hi, U, G, E as above; the K + 1 "rows" of a channel are the K members and, as row K, the target.  A member's
// depth is d if lo < d < hi, else 0; a member's reflectance as stored, NaN read as 0; the target's values as stored (its depth is a return
// on E).  Everything is widened to float64 first, so every difference is exact.
//   counts[2]             |U|, |E|
//   dist[2][K+1][K+1]     sum over E of (v_i - v_j)^2, the difference form (a Gram form cancels when members are close)
//   vario[2][offsets][4]  per offset (dh, dw), over the ordered pairs p = (h, w) in E, q = (h + dh, (w + dw) mod W) in E with 0 <= h + dh < H:
//                         the pairs, sum (a - m)^2, sum a^2, sum m^2 with a = sqrt|v_K(p) - v_K(q)| and m = (1/K) sum_k sqrt|v_k(p) - v_k(q)|,
//                         members added in member order
// coherence_dist_kernel: the rows in tiles of 8, one wave per (channel, pair of tiles ti <= tj, slab): pixels across the lanes (pixel = slab
// * 64 + lane, then in steps of slabs * 64), 16 loads per pixel (8 on a diagonal pair), 64 float64 accumulators per lane, a pixel outside E
// enters as zeros (its mask ANDed into the loaded bits: no branch, every load issued); a row past K re-loads row K and is never written out.  At the end the wave reduces its accumulators
// eight at a time (wave_sum8_scatter) into part[b][slab][channel][pair][64].  The order in which pixels enter a sum -- lane, exchange tree,
// slabs in index order in the finalize kernel -- is the same for every (i, j): permuting the members permutes rows and columns bit for bit.
// A diagonal pair computes (i, j) and (j, i) from terms with equal bits; an off-diagonal pair is written to both places.
// coherence_vario_kernel: one thread per pixel p, one block row per offset (grid.y); also the two counts.  thread -> wave -> the block's
// four waves -> part[b][offset][block][9]; the finalize kernel adds a scan's blocks in index order.  Slabs and blocks depend on the plane
// alone.  No float atomics anywhere.
constexpr int kCohTile = 8;
constexpr int kCohMaxSlabs = 256;      // waves per scan, channel and tile pair: 256 x 64 pixels per pass
constexpr int kCohSlabPixels = 1024;   // ... and at least this many pixels each, so the end-of-wave reduction is paid once per 16 pixels a lane
constexpr int kCohValues = 9;          // |U|, |E|, pairs, then per channel sum (a - m)^2, sum a^2, sum m^2
constexpr int kCohMaxOffsets = 16;
constexpr int kCohThreads = 256;
constexpr int kCohMaxBlocks = 512;
struct CohOffsets {
    int dh[kCohMaxOffsets], dw[kCohMaxOffsets];
};
static int coherence_slabs(long plane) {
    const long n = (plane + kCohSlabPixels - 1) / kCohSlabPixels;
    return n < 1 ? 1 : n > kCohMaxSlabs ? kCohMaxSlabs : (int)n;
}
static int coherence_blocks(long plane) {
    const long n = (plane + kCohThreads - 1) / kCohThreads;
    return n < 1 ? 1 : n > kCohMaxBlocks ? kCohMaxBlocks : (int)n;
}
static int coherence_tiles(int K) { return (K + 1 + kCohTile - 1) / kCohTile; }
static size_t coherence_dist_part(int B, int K, long plane) {  // doubles
    const int nt = coherence_tiles(K);
    return (size_t)B * coherence_slabs(plane) * 2 * (nt * (nt + 1) / 2) * kCohTile * kCohTile;
}
static size_t coherence_vario_part(int B, long plane, int offsets) {
    return (size_t)B * (offsets < 1 ? 1 : offsets) * coherence_blocks(plane) * kCohValues;
}
size_t ensemble_coherence_scratch_bytes(int B, int K, long plane, int offsets) {
    return (coherence_dist_part(B, K, plane) + coherence_vario_part(B, plane, offsets)) * sizeof(double);
}

// a row's value at a pixel: channel 0 depth inside the window, else 0 (the target's is inside it wherever the value is used);
// channel 1 reflectance, a member's NaN read as 0
__device__ __forceinline__ float coherence_value(float v, int c, bool member, float lo, float hi) {
    if (c == 0) return lo < v && v < hi ? v : 0.f;
    return member && v != v ? 0.f : v;
}
// the same with the pixel's mask (all ones inside E, else 0) folded in as a bitwise AND: +0 outside E whatever was loaded.  Not a select of
// the loaded value: the compiler turns that into a branch around the load and waits for each of a pixel's sixteen loads in turn.
__device__ __forceinline__ float coherence_value_masked(float v, int c, bool member, float lo, float hi, unsigned mask) {
    const bool window = (lo < v) & (v < hi), number = !(member & (v != v));
    const bool keep = c == 0 ? window : number;
    return __uint_as_float(__float_as_uint(v) & (keep ? mask : 0u));
}

__global__ __launch_bounds__(kCohThreads) void coherence_dist_kernel(const float* __restrict__ samples, const float* __restrict__ target,
                                                                     const float* __restrict__ known, double* __restrict__ part, long plane, int K,
                                                                     int tiles, int pairs, float lo, float hi) {
    constexpr int T = kCohTile;
    const int lane = threadIdx.x & 63;
    const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (kCohThreads / 64) + (threadIdx.x >> 6)));  // (channel, tile pair)
    if (job >= 2 * pairs) return;  // (no barrier below: a wave may leave)
    const int c = job / pairs, pair = job - c * pairs;
    int ti = 0, rest = pair;  // pairs in the order (0,0) (0,1) .. (0,n-1) (1,1) ..
    while (rest >= tiles - ti) rest -= tiles - ti, ++ti;
    const int tj = ti + rest;
    const int b = blockIdx.z, slab = blockIdx.x, slabs = gridDim.x;
    const float* td = target + (long)b * 5 * plane;
    const float* kn = known + (long)b * plane;
    const float* sb = samples + (long)b * K * 5 * plane;
    const float *pa[T], *pb[T];
    bool ma[T], mb[T];
#pragma unroll
    for (int r = 0; r < T; ++r) {
        const int i = ti * T + r, j = tj * T + r;
        ma[r] = i < K, mb[r] = j < K;
        pa[r] = ma[r] ? sb + ((long)i * 5 + 4 * c) * plane : td + 4L * c * plane;
        pb[r] = mb[r] ? sb + ((long)j * 5 + 4 * c) * plane : td + 4L * c * plane;
    }
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;

    for (long base = slab * 64L; base < plane; base += slabs * 64L) {  // uniform over the wave
        const long pix = base + lane;
        const bool valid = pix < plane;
        const long at = valid ? pix : plane - 1;  // every lane loads
        const float kv = kn[at], r0 = td[at];
        const bool e = valid && kv == 0.f && lo < r0 && r0 < hi;
        const unsigned em = e ? 0xffffffffu : 0u;
        float ra[T], rb[T];  // all loads of the pixel in flight together (issuing the next pass's ahead of the arithmetic as well measured no gain)
#pragma unroll
        for (int r = 0; r < T; ++r) ra[r] = pa[r][at];
        if (ti != tj) {  // uniform
#pragma unroll
            for (int r = 0; r < T; ++r) rb[r] = pb[r][at];
        }
        double x[T], y[T];
#pragma unroll
        for (int r = 0; r < T; ++r) x[r] = (double)coherence_value_masked(ra[r], c, ma[r], lo, hi, em);
        if (ti != tj) {
#pragma unroll
            for (int r = 0; r < T; ++r) y[r] = (double)coherence_value_masked(rb[r], c, mb[r], lo, hi, em);
        } else {
#pragma unroll
            for (int r = 0; r < T; ++r) y[r] = x[r];
        }
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const double d = x[i] - y[j];
                acc[i][j] = __builtin_fma(d, d, acc[i][j]);  // (the square is not rounded on its own)
            }
    }
    double* out = part + ((((long)b * slabs + slab) * 2 + c) * pairs + pair) * (T * T);
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const double t = wave_sum8_scatter(acc[i], lane);  // lane L: the wave's total of acc[i][(L >> 3) & 7]
        if ((lane & 7) == 0) out[i * T + (lane >> 3)] = t;
    }
}

__global__ __launch_bounds__(kCohThreads) void coherence_dist_finalize_kernel(const double* __restrict__ part, double* __restrict__ dist, int slabs,
                                                                              int K, int tiles, int pairs) {
    constexpr int T = kCohTile;
    const int R = K + 1, b = blockIdx.y;
    const int idx = blockIdx.x * kCohThreads + threadIdx.x;
    if (idx >= 2 * R * R) return;
    const int c = idx / (R * R), i = (idx - c * R * R) / R, j = idx - c * R * R - i * R;
    const int lo_ = i < j ? i : j, hi_ = i < j ? j : i;       // the pair of tiles holds (lo, hi); on a diagonal pair both orders have equal bits
    const int ti = lo_ / T, tj = hi_ / T;
    const int pair = ti * tiles - ti * (ti - 1) / 2 + (tj - ti);
    const double* p = part + ((long)b * slabs * 2 + c) * pairs * (T * T) + (long)pair * (T * T) + (lo_ - ti * T) * T + (hi_ - tj * T);
    const long stride = 2L * pairs * (T * T);
    double s = 0.0;
    for (int k0 = 0; k0 < slabs; k0 += 16) {  // sixteen loads in flight, added in index order
        double v[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = k0 + n < slabs ? p[(long)(k0 + n) * stride] : 0.0;
#pragma unroll
        for (int n = 0; n < 16; ++n)
            if (k0 + n < slabs) s += v[n];
    }
    dist[(long)b * 2 * R * R + idx] = i == j ? 0.0 : s;
}

__global__ __launch_bounds__(kCohThreads) void coherence_vario_kernel(const float* __restrict__ samples, const float* __restrict__ target,
                                                                      const float* __restrict__ known, double* __restrict__ part, int H, int W, int K,
                                                                      int offsets, CohOffsets off, float lo, float hi) {
    __shared__ double sh[4][kCohValues];
    const int b = blockIdx.z, o = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long plane = (long)H * W;
    const float* sb = samples + (long)b * K * 5 * plane;
    const float* td = target + (long)b * 5 * plane;
    const float* kn = known + (long)b * plane;
    const int dh = offsets ? off.dh[o] : 0, dw = offsets ? off.dw[o] : 0;
    double acc[kCohValues];
#pragma unroll
    for (int j = 0; j < kCohValues; ++j) acc[j] = 0.0;

    for (long base = blockIdx.x * (long)kCohThreads; base < plane; base += (long)gridDim.x * kCohThreads) {
        const long pix = base + tid;
        if (pix >= plane) continue;
        const float rp = td[pix];
        const bool u = kn[pix] == 0.f, e = u && lo < rp && rp < hi;
        if (u) acc[0] += 1.0;
        if (e) acc[1] += 1.0;
        if (!e || !offsets) continue;
        const int h = (int)(pix / W), w = (int)(pix - (long)h * W);
        const int hq = h + dh;
        if (hq < 0 || hq >= H) continue;
        int wq = w + dw;  // |dw| < W
        wq += wq < 0 ? W : 0;
        wq -= wq >= W ? W : 0;
        const long q = (long)hq * W + wq;
        const float rq = td[q];
        if (!(kn[q] == 0.f && lo < rq && rq < hi)) continue;
        acc[2] += 1.0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long ch = 4L * c * plane;
            const double a = sqrt(fabs((double)coherence_value(td[ch + pix], c, false, lo, hi) - (double)coherence_value(td[ch + q], c, false, lo, hi)));
            double s = 0.0;
            for (int k = 0; k < K; ++k) {  // (added in member order; unrolled by 4 the call measured 252 us instead of 189 us)
                const float* m = sb + (long)k * 5 * plane + ch;
                s += sqrt(fabs((double)coherence_value(m[pix], c, true, lo, hi) - (double)coherence_value(m[q], c, true, lo, hi)));
            }
            const double m = s / (double)K;
            acc[3 + 3 * c] += (a - m) * (a - m);
            acc[4 + 3 * c] += a * a;
            acc[5 + 3 * c] += m * m;
        }
    }
    {
        double v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = acc[j];
        const double t0 = wave_sum8_scatter(v8, lane), t1 = wave_sum_f64(acc[8]);
        if ((lane & 7) == 0) sh[wave][lane >> 3] = t0;
        if (lane == 0) sh[wave][8] = t1;
    }
    __syncthreads();
    if (tid < kCohValues)
        part[(((long)b * gridDim.y + o) * gridDim.x + blockIdx.x) * kCohValues + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// counts from the first offset's blocks (every offset's blocks count the same pixels), vario from each offset's
__global__ __launch_bounds__(64) void coherence_vario_finalize_kernel(const double* __restrict__ part, double* __restrict__ counts,
                                                                      double* __restrict__ vario, int blocks, int offsets) {
    const int b = blockIdx.x, rows = offsets < 1 ? 1 : offsets;
    for (int t = threadIdx.x; t < 2 + offsets * 7; t += 64) {
        const int o = t < 2 ? 0 : (t - 2) / 7, j = t < 2 ? t : 2 + (t - 2) % 7;
        const double* p = part + ((long)b * rows + o) * blocks * kCohValues + j;
        double s = 0.0;
        for (int k0 = 0; k0 < blocks; k0 += 16) {
            double v[16];
#pragma unroll
            for (int n = 0; n < 16; ++n) v[n] = k0 + n < blocks ? p[(long)(k0 + n) * kCohValues] : 0.0;
#pragma unroll
            for (int n = 0; n < 16; ++n)
                if (k0 + n < blocks) s += v[n];
        }
        if (t < 2) {
            counts[(long)b * 2 + t] = s;
        } else {  // part: pairs, then per channel (a - m)^2, a^2, m^2  ->  vario[b][c][o][4] = pairs, (a - m)^2, a^2, m^2
            const int v = j - 2;  // 0 pairs, 1..3 channel 0, 4..6 channel 1
            if (v == 0) {
                vario[(((long)b * 2 + 0) * offsets + o) * 4] = s;
                vario[(((long)b * 2 + 1) * offsets + o) * 4] = s;
            } else {
                const int c = (v - 1) / 3, n = 1 + (v - 1) % 3;
                vario[(((long)b * 2 + c) * offsets + o) * 4 + n] = s;
            }
        }
    }
}

// (arguments validated by r2dm_ensemble_coherence: 1 <= B <= 65535, 1 <= K <= 64, H, W >= 1, H * W < 2^31, 0 <= offsets <= 16, every offset
// inside the image and not (0, 0); dist or vario may be null; offsets_hw is a host pointer)
hipError_t launch_ensemble_coherence(const float* samples, const float* target, const float* known, float lo, float hi, int B, int K, int H, int W,
                                     const int* offsets_hw, int offsets, void* scratch, double* counts, double* dist, double* vario, hipStream_t s) {
    if (B < 1 || K < 1 || K > kEnsMaxMembers || H < 1 || W < 1 || offsets < 0 || offsets > kCohMaxOffsets) return hipErrorInvalidValue;
    const long plane = (long)H * W;
    double* dpart = static_cast<double*>(scratch);
    double* vpart = dpart + coherence_dist_part(B, K, plane);
    if (dist) {
        const int tiles = coherence_tiles(K), pairs = tiles * (tiles + 1) / 2, slabs = coherence_slabs(plane);
        const dim3 grid((unsigned)slabs, (unsigned)((2 * pairs + 3) / 4), (unsigned)B);
        coherence_dist_kernel<<<grid, kCohThreads, 0, s>>>(samples, target, known, dpart, plane, K, tiles, pairs, lo, hi);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const int cells = 2 * (K + 1) * (K + 1);
        coherence_dist_finalize_kernel<<<dim3((unsigned)((cells + kCohThreads - 1) / kCohThreads), (unsigned)B), kCohThreads, 0, s>>>(dpart, dist, slabs,
                                                                                                                                    K, tiles, pairs);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int used = vario ? offsets : 0;  // without vario only the counts
    CohOffsets off = {};
    for (int o = 0; o < used; ++o) off.dh[o] = offsets_hw[2 * o], off.dw[o] = offsets_hw[2 * o + 1];
    const int blocks = coherence_blocks(plane);
    coherence_vario_kernel<<<dim3((unsigned)blocks, (unsigned)(used < 1 ? 1 : used), (unsigned)B), kCohThreads, 0, s>>>(samples, target, known, vpart, H,
                                                                                                                       W, K, used, off, lo, hi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    coherence_vario_finalize_kernel<<<B, 64, 0, s>>>(vpart, counts, vario, blocks, used);
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
