// K13: BEV metrics of the reference's evaluate.py (metrics/bev.py, evaluate.py:131-196).
//
//  bev_hist_kernel   point_cloud_to_histogram on a batch: the (x, y) occupancy histogram of the points with
//                    min_depth < |xyz| < max_depth, counts bit-identical to torch.histogramdd on the CPU.
//                    One int32 histogram per block in LDS (integer atomics), one or more blocks per scan,
//                    merged into global memory by integer atomics: the counts do not depend on any order.
//  bev_sum_kernel    the exact int64 sum of a batch of histograms (JSD's numerator), fixed order.
//  mmd_*             RBF-kernel MMD between two sets of normalised histograms, without the N x N matrix:
//                    d^2 = sum_k (p_k - q_k)^2 directly (fp32 within a stage of kBins bins, fp64 across stages),
//                    1 - k = -expm1(-gamma d^2) in fp64, per-block partials summed in a fixed order.
//                    No float atomics anywhere: two calls return the same bits.
#include "common.h"

namespace r2dm {

#pragma clang fp contract(off)

// ---- histogram ---------------------------------------------------------------------------------
constexpr int kHistThreads = 1024;
constexpr int kHistMaxBins = 128;  // 128 x 128 int32 = 64 KiB of LDS: two blocks of 16 waves fill a CU's 32 wave slots

// bin of v as torch.histogramdd's CPU kernel finds it (aten/src/ATen/native/cpu/HistogramKernel.cpp,
// LINEAR_INTERPOLATION_WITH_LOCAL_SEARCH): out-of-range and NaN values are dropped (-1), the position
// from a linear interpolation in fp32 is corrected by an upper_bound over its neighbouring edges, and
// the right edge belongs to the last bin only.
__device__ __forceinline__ int hist_bin(float v, const float* E, int bins) {
    const float L = E[0], R = E[bins];
    if (!(v >= L && v <= R)) return -1;
    const int pos = (int)(((v - L) * (float)bins) / (R - L));
    const int lo = pos - 1 > 0 ? pos - 1 : 0, hi = pos + 2 < bins + 1 ? pos + 2 : bins + 1;
    int k = lo;
    while (k < hi && !(v < E[k])) ++k;  // first edge > v
    int b = k - 1;
    if (b == bins) b = bins - 1;
    return (b >= 0 && b < bins) ? b : -1;
}

// LAYOUT 0: (B,5,H,W) samples [depth, x, y, z, reflectance]: xyz * (img_min < depth < img_max) first (evaluate.py:22-41,150-151);
// LAYOUT 1: (B,N,3) point clouds.
template <int LAYOUT>
__global__ __launch_bounds__(kHistThreads) void bev_hist_kernel(const float* __restrict__ src, const float* __restrict__ edges,
                                                                int32_t* __restrict__ hist, long n, int bins, float min_d,
                                                                float max_d, float img_min, float img_max) {
    __shared__ int h[kHistMaxBins * kHistMaxBins];
    __shared__ float E[kHistMaxBins + 1];
    const int b = blockIdx.y, cells = bins * bins;
    for (int i = threadIdx.x; i < cells; i += kHistThreads) h[i] = 0;
    for (int i = threadIdx.x; i <= bins; i += kHistThreads) E[i] = edges[i];
    __syncthreads();
    const long per = (n + gridDim.x - 1) / gridDim.x;
    const long beg = (long)blockIdx.x * per, end = beg + per < n ? beg + per : n;
    for (long i = beg + threadIdx.x; i < end; i += kHistThreads) {
        float x, y, z;
        if (LAYOUT == 0) {
            const float* s = src + (long)b * 5 * n;
            const float dep = s[i];
            const float m = (dep > img_min && dep < img_max) ? 1.0f : 0.0f;
            x = s[n + i] * m;
            y = s[2 * n + i] * m;
            z = s[3 * n + i] * m;
        } else {
            const float* s = src + ((long)b * n + i) * 3;
            x = s[0];
            y = s[1];
            z = s[2];
        }
        // point_cloud.norm(p=2, dim=1) on the CPU: fma(z, z, fma(y, y, x*x)), correctly rounded sqrt
        const float d = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
        if (!(d > min_d && d < max_d)) continue;
        const int ix = hist_bin(x, E, bins), iy = hist_bin(y, E, bins);
        if (ix < 0 || iy < 0) continue;
        atomicAdd(&h[ix * bins + iy], 1);
    }
    __syncthreads();
    int32_t* out = hist + (long)b * cells;
    if (gridDim.x == 1) {
        for (int i = threadIdx.x; i < cells; i += kHistThreads) out[i] = h[i];
    } else {
        for (int i = threadIdx.x; i < cells; i += kHistThreads)
            if (h[i]) atomicAdd(&out[i], h[i]);
    }
}

// sum over the batch, one thread per cell, batch order fixed (exact in int64)
template <typename T>
__global__ __launch_bounds__(256) void bev_sum_kernel(const T* __restrict__ hist, int64_t* __restrict__ sum, long batch, long cells) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    long long s = 0;
    for (long b = 0; b < batch; ++b) s += (long long)hist[b * cells + c];
    sum[c] = s;
}

hipError_t launch_bev_histogram(const float* src, int layout, const float* edges, int32_t* hist, int64_t* sum, int B, long n,
                                int bins, float min_d, float max_d, float img_min, float img_max, hipStream_t s) {
    if (B < 1 || n < 1 || bins < 1 || bins > kHistMaxBins || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
    const long cells = (long)bins * bins;
    // enough blocks to fill the chip at small batches; a block takes at least 8 points per thread
    long split = (2048 + B - 1) / B;
    const long most = (n + 8L * kHistThreads - 1) / (8L * kHistThreads);
    if (split > most) split = most;
    if (split < 1) split = 1;
    if (split > 1) {
        hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * cells * B, s);
        if (e != hipSuccess) return e;
    }
    const dim3 g((unsigned)split, (unsigned)B);
    if (layout == 0)
        bev_hist_kernel<0><<<g, kHistThreads, 0, s>>>(src, edges, hist, n, bins, min_d, max_d, img_min, img_max);
    else
        bev_hist_kernel<1><<<g, kHistThreads, 0, s>>>(src, edges, hist, n, bins, min_d, max_d, img_min, img_max);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !sum) return e;
    bev_sum_kernel<int32_t><<<(unsigned)((cells + 255) / 256), 256, 0, s>>>(hist, sum, B, cells);
    return hipGetLastError();
}

hipError_t launch_bev_hist_sum(const void* hist, int is_int32, int64_t* sum, long batch, long cells, hipStream_t s) {
    if (batch < 1 || cells < 1) return hipErrorInvalidValue;
    const unsigned g = (unsigned)((cells + 255) / 256);
    if (is_int32)
        bev_sum_kernel<int32_t><<<g, 256, 0, s>>>(static_cast<const int32_t*>(hist), sum, batch, cells);
    else
        bev_sum_kernel<float><<<g, 256, 0, s>>>(static_cast<const float*>(hist), sum, batch, cells);
    return hipGetLastError();
}

// ---- MMD ---------------------------------------------------------------------------------------
// A block takes a 64 x 64 tile of pairs (rows of A against rows of B); each of its 256 threads a 4 x 4 micro-tile.
// The bins stream through LDS kBins at a time, stored bin-major so a thread reads its 4 rows as one float4.
constexpr int kTile = 64, kMicro = 4, kBins = 32, kMmdThreads = 256;
constexpr int kLd = kTile + 4;  // LDS row stride (floats): keeps the float4 reads aligned

__global__ __launch_bounds__(256) void mmd_row_sums_kernel(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ rs,
                                                           int np, int nq, long D) {
    __shared__ double red[256];
    const int r = blockIdx.x;
    const float* row = r < np ? P + (long)r * D : Q + (long)(r - np) * D;
    double s = 0.0;
    for (long k = threadIdx.x; k < D; k += 256) s += (double)row[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) rs[r] = (float)red[0];  // (integer counts: exact, as the reference's fp32 row sum)
}

__device__ __forceinline__ int tri_tiles(int n) { return n * (n + 1) / 2; }

__global__ __launch_bounds__(kMmdThreads) void mmd_pairs_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                                const float* __restrict__ rs, double* __restrict__ partial,
                                                                int np, int nq, long D, double gamma) {
    __shared__ __attribute__((aligned(16))) float As[kBins * kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kBins * kLd];
    __shared__ double red[kMmdThreads];

    // which tile: [0, tPQ) P x Q, then the upper triangle of P x P, then that of Q x Q
    const int tp = (np + kTile - 1) / kTile, tq = (nq + kTile - 1) / kTile;
    int t = blockIdx.x, ti, tj;
    const float *A, *B;
    const float *rsA, *rsB;
    int na, nb;
    bool self;
    if (t < tp * tq) {
        ti = t / tq;
        tj = t % tq;
        A = P, B = Q, rsA = rs, rsB = rs + np, na = np, nb = nq, self = false;
    } else {
        t -= tp * tq;
        int n = tp;
        if (t < tri_tiles(tp)) {
            A = B = P, rsA = rsB = rs, na = nb = np;
        } else {
            t -= tri_tiles(tp);
            n = tq;
            A = B = Q, rsA = rsB = rs + np, na = nb = nq;
        }
        self = true;
        ti = 0;
        while (t >= n - ti) t -= n - ti++;
        tj = ti + t;
    }
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;

    // staging: thread -> row sr of the tile, bins sc .. sc+7 of the stage
    const int sr = threadIdx.x / 4, sc = (threadIdx.x % 4) * 8;
    const bool va = i0 + sr < na, vb = j0 + sr < nb;
    const float* ga = A + (long)(va ? i0 + sr : 0) * D;
    const float* gb = B + (long)(vb ? j0 + sr : 0) * D;
    const float sa = va ? rsA[i0 + sr] : 1.0f, sb = vb ? rsB[j0 + sr] : 1.0f;

    double acc[kMicro][kMicro];
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) acc[a][c] = 0.0;

    for (long k0 = 0; k0 < D; k0 += kBins) {
        float ra[8], rb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long k = k0 + sc + j;
            ra[j] = (va && k < D) ? ga[k] / sa : 0.0f;  // p = h / sum(h) (evaluate.py's normalisation, IEEE division)
            rb[j] = (vb && k < D) ? gb[k] / sb : 0.0f;
        }
        __syncthreads();  // (previous stage fully read)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[(sc + j) * kLd + sr] = ra[j];
            Bs[(sc + j) * kLd + sr] = rb[j];
        }
        __syncthreads();
        float s[kMicro][kMicro];
#pragma unroll
        for (int a = 0; a < kMicro; ++a)
#pragma unroll
            for (int c = 0; c < kMicro; ++c) s[a][c] = 0.0f;
#pragma unroll 8
        for (int k = 0; k < kBins; ++k) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&As[k * kLd + ty * kMicro]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[k * kLd + tx * kMicro]);
#pragma unroll
            for (int a = 0; a < kMicro; ++a)
#pragma unroll
                for (int c = 0; c < kMicro; ++c) {
                    const float df = av[a] - bv[c];
                    s[a][c] = fmaf(df, df, s[a][c]);
                }
        }
#pragma unroll
        for (int a = 0; a < kMicro; ++a)
#pragma unroll
            for (int c = 0; c < kMicro; ++c) acc[a][c] += (double)s[a][c];
    }

    // 1 - k(p_i, q_j) = -expm1(-gamma d^2); the upper triangle of a self tile counts twice, its diagonal once (0 for finite rows)
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) {
            const int i = i0 + ty * kMicro + a, j = j0 + tx * kMicro + c;
            if (i >= na || j >= nb) continue;
            double w = 1.0;
            if (self) {
                if (j < i) continue;
                if (j > i) w = 2.0;
            }
            sum += w * -expm1(-gamma * acc[a][c]);
        }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kMmdThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// the three means from the per-block partials, one block, fixed order
__global__ __launch_bounds__(1024) void mmd_final_kernel(const double* __restrict__ partial, double* __restrict__ out, int n_pq, int n_pp,
                                                         int n_qq, int np, int nq) {
    __shared__ double red[1024];
    const int start[3] = {0, n_pq, n_pq + n_pp}, cnt[3] = {n_pq, n_pp, n_qq};
    const double pairs[3] = {(double)np * nq, (double)np * np, (double)nq * nq};
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < cnt[c]; i += 1024) s += partial[start[c] + i];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[c] = red[0] / pairs[c];
        __syncthreads();
    }
}

static void mmd_grid(int np, int nq, long& n_pq, long& n_pp, long& n_qq) {
    const long tp = (np + kTile - 1) / kTile, tq = (nq + kTile - 1) / kTile;
    n_pq = tp * tq;
    n_pp = tp * (tp + 1) / 2;
    n_qq = tq * (tq + 1) / 2;
}

size_t mmd_scratch_bytes(int np, int nq) {
    long a, b, c;
    mmd_grid(np, nq, a, b, c);
    const size_t rs = ((size_t)(np + nq) * sizeof(float) + 255) / 256 * 256;
    return rs + (size_t)(a + b + c) * sizeof(double);
}

hipError_t launch_bev_mmd(const float* P, const float* Q, int np, int nq, long D, double sigma, void* scratch, double* out, hipStream_t s) {
    if (np < 1 || nq < 1 || D < 1 || !(sigma > 0.0)) return hipErrorInvalidValue;
    long n_pq, n_pp, n_qq;
    mmd_grid(np, nq, n_pq, n_pp, n_qq);
    if (n_pq + n_pp + n_qq > 0x7fffffffL) return hipErrorInvalidValue;
    float* rs = static_cast<float*>(scratch);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + ((size_t)(np + nq) * sizeof(float) + 255) / 256 * 256);
    mmd_row_sums_kernel<<<np + nq, 256, 0, s>>>(P, Q, rs, np, nq, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    mmd_pairs_kernel<<<(unsigned)(n_pq + n_pp + n_qq), kMmdThreads, 0, s>>>(P, Q, rs, partial, np, nq, D, 1.0 / (2.0 * sigma * sigma));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    mmd_final_kernel<<<1, 1024, 0, s>>>(partial, out, (int)n_pq, (int)n_pp, (int)n_qq, np, nq);
    return hipGetLastError();
}

// ---- feature moments (Frechet distance) ----------------------------------------------------------
// mean and unbiased covariance of (n, D) fp32 features in fp64, two passes (the second over centred values), every sum in a
// fixed order: mean[d] one thread per column, cov one 64 x 64 tile per block with the rows staged 16 at a time.
__global__ __launch_bounds__(256) void feat_mean_kernel(const float* __restrict__ f, double* __restrict__ mean, long n, int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (long r = 0; r < n; ++r) s += (double)f[r * D + d];
    mean[d] = s / (double)n;
}

constexpr int kCovRows = 16;

__global__ __launch_bounds__(256) void feat_cov_kernel(const float* __restrict__ f, const double* __restrict__ mean, double* __restrict__ cov,
                                                       long n, int D) {
    __shared__ double As[kCovRows][kTile], Bs[kCovRows][kTile];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const int sc = threadIdx.x % kTile, sr = threadIdx.x / kTile;  // staging: column sc, rows sr + 4 u
    const bool va = i0 + sc < D, vb = j0 + sc < D;
    const double ma = va ? mean[i0 + sc] : 0.0, mb = vb ? mean[j0 + sc] : 0.0;
    double acc[kMicro][kMicro];
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) acc[a][c] = 0.0;
    for (long r0 = 0; r0 < n; r0 += kCovRows) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kCovRows / 4; ++u) {
            const long r = r0 + sr + 4 * u;
            As[sr + 4 * u][sc] = (va && r < n) ? (double)f[r * D + i0 + sc] - ma : 0.0;
            Bs[sr + 4 * u][sc] = (vb && r < n) ? (double)f[r * D + j0 + sc] - mb : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCovRows; ++k)
#pragma unroll
            for (int a = 0; a < kMicro; ++a)
#pragma unroll
                for (int c = 0; c < kMicro; ++c) acc[a][c] = fma(As[k][ty * kMicro + a], Bs[k][tx * kMicro + c], acc[a][c]);
    }
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) {
            const int i = i0 + ty * kMicro + a, j = j0 + tx * kMicro + c;
            if (i < D && j < D) cov[(long)i * D + j] = acc[a][c] / (double)(n - 1);
        }
}

hipError_t launch_feature_moments(const float* f, long n, int D, double* mean, double* cov, hipStream_t s) {
    if (n < 2 || D < 1) return hipErrorInvalidValue;
    feat_mean_kernel<<<(D + 255) / 256, 256, 0, s>>>(f, mean, n, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned t = (unsigned)((D + kTile - 1) / kTile);
    feat_cov_kernel<<<dim3(t, t), 256, 0, s>>>(f, mean, cov, n, D);
    return hipGetLastError();
}

// ---- polynomial-kernel MMD of feature sets (metrics/distribution.py compute_squared_mmd) ---------------------------------------
// Per subset s: x = X[ix[s]], y = Y[iy[s]] (m rows each, gathered here); the three sums of (u.v / D + 1)^3 over the pairs of
// x x x and y x y off the diagonal and of x x y, products and sums in fp64, without an m x m matrix: a block takes a 64 x 64 tile
// of pairs, the features stream through LDS 16 at a time; per-block partials, summed in a fixed order.
constexpr int kPolyK = 16;

__global__ __launch_bounds__(256) void poly_mmd_pairs_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                             const long long* __restrict__ ix, const long long* __restrict__ iy,
                                                             double* __restrict__ partial, int m, int D) {
    __shared__ double As[kPolyK][kTile], Bs[kPolyK][kTile];
    __shared__ double red[256];
    const int s = blockIdx.y;
    const int tm = (m + kTile - 1) / kTile;
    int t = blockIdx.x, ti, tj;
    const float *A, *B;
    const long long *ia, *ib;
    bool self;
    if (t < tm * tm) {
        ti = t / tm, tj = t % tm;
        A = X, B = Y, ia = ix, ib = iy, self = false;
    } else {
        t -= tm * tm;
        if (t < tri_tiles(tm)) {
            A = B = X, ia = ib = ix;
        } else {
            t -= tri_tiles(tm);
            A = B = Y, ia = ib = iy;
        }
        self = true;
        ti = 0;
        while (t >= tm - ti) t -= tm - ti++;
        tj = ti + t;
    }
    ia += (long)s * m, ib += (long)s * m;
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const int sr = threadIdx.x / 4, sc = (threadIdx.x % 4) * 4;  // staging: row sr of the tile, features sc .. sc + 3 of the stage
    const bool va = i0 + sr < m, vb = j0 + sr < m;
    const float* ga = A + (va ? ia[i0 + sr] : 0) * (long)D;
    const float* gb = B + (vb ? ib[j0 + sr] : 0) * (long)D;
    double acc[kMicro][kMicro];
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) acc[a][c] = 0.0;
    for (int k0 = 0; k0 < D; k0 += kPolyK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + sc + j;
            As[sc + j][sr] = (va && k < D) ? (double)ga[k] : 0.0;
            Bs[sc + j][sr] = (vb && k < D) ? (double)gb[k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPolyK; ++k)
#pragma unroll
            for (int a = 0; a < kMicro; ++a)
#pragma unroll
                for (int c = 0; c < kMicro; ++c) acc[a][c] = fma(As[k][ty * kMicro + a], Bs[k][tx * kMicro + c], acc[a][c]);
    }
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < kMicro; ++a)
#pragma unroll
        for (int c = 0; c < kMicro; ++c) {
            const int i = i0 + ty * kMicro + a, j = j0 + tx * kMicro + c;
            if (i >= m || j >= m) continue;
            double w = 1.0;
            if (self) {  // off the diagonal only; the upper triangle counts twice
                if (j <= i) continue;
                w = 2.0;
            }
            const double v = acc[a][c] / (double)D + 1.0;
            sum += w * (v * v * v);
        }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long)s * gridDim.x + blockIdx.x] = red[0];
}

// out[s] = (sum over x x y, over x x x off the diagonal, over y x y off the diagonal), one block per subset, fixed order
__global__ __launch_bounds__(256) void poly_mmd_final_kernel(const double* __restrict__ partial, double* __restrict__ out, int n_xy, int n_tri) {
    __shared__ double red[256];
    const int s = blockIdx.x;
    const double* ps = partial + (long)s * (n_xy + 2 * n_tri);
    const int start[3] = {0, n_xy, n_xy + n_tri}, cnt[3] = {n_xy, n_tri, n_tri};
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int i = threadIdx.x; i < cnt[c]; i += 256) v += ps[start[c] + i];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[s * 3 + c] = red[0];
        __syncthreads();
    }
}

size_t poly_mmd_scratch_bytes(int subsets, int m) {
    const long tm = (m + kTile - 1) / kTile;
    return (size_t)subsets * (size_t)(tm * tm + tm * (tm + 1)) * sizeof(double);
}

hipError_t launch_poly_mmd(const float* X, const float* Y, const long long* ix, const long long* iy, int subsets, int m, int D, void* scratch,
                           double* out, hipStream_t s) {
    if (subsets < 1 || subsets > 65535 || m < 1 || D < 1) return hipErrorInvalidValue;
    const long tm = (m + kTile - 1) / kTile;
    const long n_xy = tm * tm, n_tri = tm * (tm + 1) / 2;
    if (n_xy + 2 * n_tri > 0x7fffffffL) return hipErrorInvalidValue;
    poly_mmd_pairs_kernel<<<dim3((unsigned)(n_xy + 2 * n_tri), (unsigned)subsets), 256, 0, s>>>(X, Y, ix, iy, static_cast<double*>(scratch), m, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    poly_mmd_final_kernel<<<subsets, 256, 0, s>>>(static_cast<const double*>(scratch), out, (int)n_xy, (int)n_tri);
    return hipGetLastError();
}

}  // namespace r2dm
