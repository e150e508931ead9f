// K21: geometry metrics -- how far two scans are from each other in 3-D: the nearest-neighbour search behind Chamfer distance, F-score and the
// set metrics COV / MMD / 1-NNA (r2dm_amd/geometry.py).
//
//  nn_pairs_kernel      for P pairs of clouds (ia, ib) and both directions: for every point x of one cloud the squared distance to its nearest
//                       neighbour in the other and (optionally) that neighbour's index, plus per block the partial sums of d^2, d, #{d <= tau}.
//  nn_finalize_kernel   adds a (pair, direction)'s partials in chunk order (the scheme of completion.hip: float64, fixed order, no floating-point
//                       atomics, bit-reproducible) and writes the pair's two counts.
//
// A VALU kernel on purpose.  The distance is (ax-bx)^2 + (ay-by)^2 + (az-bz)^2 in fp32: the expanded form |a|^2 + |b|^2 - 2ab that would fit the
// matrix cores cancels catastrophically for LiDAR geometry (two 5 cm clusters 70 m from the origin: in error by several times the distance itself).
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kNnThreads = 256;
constexpr int kNnQ = 4;                         // query points per thread, in registers
constexpr int kNnChunk = kNnThreads * kNnQ;     // query points per block
constexpr int kNnTile = 1024;                   // points of the other cloud per LDS tile
constexpr int kNnGroups = kNnTile / 4;          // the tile is kept as groups of four points: x[4], y[4], z[4] = three 16-byte broadcast reads
constexpr int kNnPart = 4;                      // partial values per block: sum d^2, sum d, #{d <= tau}, #{non-finite query points}
constexpr long kNnMaxPoints = 1L << 21;         // per cloud

long nn_pairs_chunks(long max_points) { return max_points < 1 ? 1 : (max_points + kNnChunk - 1) / kNnChunk; }
size_t nn_pairs_scratch_bytes(long P, long max_points) { return (size_t)P * 2 * nn_pairs_chunks(max_points) * kNnPart * sizeof(double); }

// one expression for the search and for the recovery of the index: the same bits both times
__device__ __forceinline__ float nn_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

struct NnCloud {
    long beg, n;
    bool ok;
};
// cloud i of a ragged set: rows [off[i], off[i+1]) of `total`.  Nothing is read through an index or an offset that does not check out.
__device__ __forceinline__ NnCloud nn_cloud(const long long* __restrict__ off, long clouds, long total, long long i, long max_points) {
    NnCloud c = {0, 0, false};
    if (i < 0 || i >= clouds) return c;
    const long long b = off[i], e = off[i + 1];
    if (b < 0 || e < b || e > total || e - b > max_points) return c;
    c.beg = (long)b;
    c.n = (long)(e - b);
    c.ok = true;
    return c;
}

struct NnArgs {
    const f32x4 *a, *b;                 // (total,4) rows [x, y, z, .]
    const long long *off_a, *off_b;     // (clouds + 1)
    long clouds_a, clouds_b, total_a, total_b;
    const long long* pairs;             // (P,2) [ia, ib]
    long max_points;                    // no cloud of a pair has more points (sizes the grid and the scratch)
    double tau2;
    float* d2[2];                       // per direction (0: a -> b, 1: b -> a): nullptr or one value per query point of every pair
    int* idx[2];                        // nullptr or the neighbour's index inside its cloud
    const long long* out_off[2];        // (P) where a pair's per-point values start
    double* part;                       // (2P, chunks, kNnPart)
};

// grid (2P, chunks): block (x, y) owns query points [1024 y, 1024 y + 1024) of direction x & 1 of pair x >> 1; thread t holds the points
// 1024 y + 256 j + t, j < 4.  The other cloud streams through LDS in tiles of 1024 points; every read of the inner loop is one address for the
// whole wave (a broadcast), so three 16-byte reads serve 64 lanes x 4 queries x 4 points.  Per point pair: 3 subtractions, 1 multiply, 2 FMAs
// and 3/4 of a minimum; the running minimum is compared once per group of four points, which also records the group.  The index is recovered
// afterwards from that group's four points in global memory: strict `<` over ascending groups and then over ascending points gives the lowest
// index on an exact tie.  A padding point of the last group is +inf: its distance is +inf and never below the running minimum.
__global__ __launch_bounds__(kNnThreads) void nn_pairs_kernel(const NnArgs g) {
    __shared__ f32x4 tile[kNnGroups][3];
    __shared__ double sh[kNnPart][kNnThreads / 64];
    const long p = blockIdx.x >> 1;
    const int dir = blockIdx.x & 1, tid = threadIdx.x;
    const NnCloud ca = nn_cloud(g.off_a, g.clouds_a, g.total_a, g.pairs[2 * p], g.max_points);
    const NnCloud cb = nn_cloud(g.off_b, g.clouds_b, g.total_b, g.pairs[2 * p + 1], g.max_points);
    if (!ca.ok || !cb.ok) return;  // (nn_finalize_kernel reports the pair)
    const f32x4* Q = dir ? g.b + cb.beg : g.a + ca.beg;
    const f32x4* R = dir ? g.a + ca.beg : g.b + cb.beg;
    const long nq = dir ? cb.n : ca.n, nr = dir ? ca.n : cb.n;
    const long q0 = (long)blockIdx.y * kNnChunk;
    if (q0 >= nq) return;  // (uniform over the block; nn_finalize_kernel reads the chunks below ceil(nq / 1024) only)

    float qx[kNnQ], qy[kNnQ], qz[kNnQ], best[kNnQ];
    int grp[kNnQ];
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const long q = q0 + j * kNnThreads + tid;
        const f32x4 v = q < nq ? Q[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        qx[j] = v[0], qy[j] = v[1], qz[j] = v[2];
        best[j] = INFINITY;
        grp[j] = -1;
    }
    const bool wave_on = q0 + (tid & ~63) < nq;  // a wave whose four slots are all past the cloud's end only helps to load
    float* tf = reinterpret_cast<float*>(&tile[0][0]);
    for (long t0 = 0; t0 < nr; t0 += kNnTile) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kNnTile / kNnThreads; ++i) {
            const int s = i * kNnThreads + tid;
            const f32x4 v = t0 + s < nr ? R[t0 + s] : f32x4{INFINITY, INFINITY, INFINITY, 0.f};
            float* d = tf + (s >> 2) * 12 + (s & 3);
            d[0] = v[0], d[4] = v[1], d[8] = v[2];
        }
        __syncthreads();
        if (!wave_on) continue;
        const long left = nr - t0;
        const int ng = left >= kNnTile ? kNnGroups : (int)((left + 3) >> 2);
        const int g0 = (int)(t0 >> 2);
#pragma unroll 2
        for (int k = 0; k < ng; ++k) {
            const f32x4 X = tile[k][0], Y = tile[k][1], Z = tile[k][2];
#pragma unroll
            for (int j = 0; j < kNnQ; ++j) {
                const float d0 = nn_d2(qx[j], qy[j], qz[j], X[0], Y[0], Z[0]), d1 = nn_d2(qx[j], qy[j], qz[j], X[1], Y[1], Z[1]);
                const float d2 = nn_d2(qx[j], qy[j], qz[j], X[2], Y[2], Z[2]), d3 = nn_d2(qx[j], qy[j], qz[j], X[3], Y[3], Z[3]);
                const float m = __builtin_fminf(__builtin_fminf(d0, d1), __builtin_fminf(d2, d3));
                if (m < best[j]) {
                    best[j] = m;
                    grp[j] = g0 + k;
                }
            }
        }
    }

    double acc[kNnPart] = {0.0, 0.0, 0.0, 0.0};
    const long o = g.d2[dir] ? (long)g.out_off[dir][p] : 0;
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const long q = q0 + j * kNnThreads + tid;
        if (q >= nq) continue;
        const double d2 = (double)best[j];
        acc[0] += d2;
        acc[1] += sqrt(d2);
        acc[2] += d2 <= g.tau2 ? 1.0 : 0.0;
        acc[3] += (isfinite(qx[j]) && isfinite(qy[j]) && isfinite(qz[j])) ? 0.0 : 1.0;
        if (g.d2[dir]) g.d2[dir][o + q] = best[j];
        if (g.idx[dir]) {
            int at = -1;
            if (grp[j] >= 0) {
                float bd = INFINITY;
                for (int k = 0; k < 4; ++k) {
                    const long r = 4L * grp[j] + k;
                    if (r >= nr) break;
                    const f32x4 v = R[r];
                    const float d = nn_d2(qx[j], qy[j], qz[j], v[0], v[1], v[2]);
                    if (d < bd) {
                        bd = d;
                        at = (int)r;
                    }
                }
            }
            g.idx[dir][o + q] = at;
        }
    }
    const int wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < kNnPart; ++j) {
        const double v = wave_sum_f64(acc[j]);
        if ((tid & 63) == 0) sh[j][wave] = v;
    }
    __syncthreads();
    if (tid < kNnPart) g.part[((long)blockIdx.x * gridDim.y + blockIdx.y) * kNnPart + tid] = ((sh[tid][0] + sh[tid][1]) + sh[tid][2]) + sh[tid][3];
}

// sums (P,8) = [sum d^2, sum d, #{d <= tau}] of a -> b, the same of b -> a, |a|, |b|.  status[0] += non-finite query points met, status[1] += pairs
// whose index or offsets do not check out (their eight values are NaN).
__global__ __launch_bounds__(256) void nn_finalize_kernel(const NnArgs g, long P, int chunks, double* __restrict__ sums,
                                                          unsigned long long* __restrict__ status) {
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= 2 * P) return;
    const long p = t >> 1;
    const int dir = (int)(t & 1);
    const NnCloud ca = nn_cloud(g.off_a, g.clouds_a, g.total_a, g.pairs[2 * p], g.max_points);
    const NnCloud cb = nn_cloud(g.off_b, g.clouds_b, g.total_b, g.pairs[2 * p + 1], g.max_points);
    double* out = sums + p * 8;
    if (!ca.ok || !cb.ok) {
        for (int j = 0; j < 3; ++j) out[dir * 3 + j] = NAN;
        out[6 + dir] = NAN;
        if (dir == 0) atomicAdd(&status[1], 1ULL);
        return;
    }
    const long nq = dir ? cb.n : ca.n;
    const long used = (nq + kNnChunk - 1) / kNnChunk;
    double s[kNnPart] = {0.0, 0.0, 0.0, 0.0};
    for (long k = 0; k < used; ++k)
        for (int j = 0; j < kNnPart; ++j) s[j] += g.part[(t * chunks + k) * kNnPart + j];
    for (int j = 0; j < 3; ++j) out[dir * 3 + j] = s[j];
    out[6 + dir] = (double)nq;
    if (s[3] > 0.0) atomicAdd(&status[0], (unsigned long long)s[3]);
}

// (arguments validated by r2dm_nn_pairs: 1 <= P, 1 <= max_points <= 2^21, 2 P chunks < 2^31, alignment)
hipError_t launch_nn_pairs(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b, long clouds_b,
                           long total_b, const long long* pairs, long P, long max_points, double tau, float* d2_ab, int* idx_ab,
                           const long long* out_ab, float* d2_ba, int* idx_ba, const long long* out_ba, void* scratch, double* sums,
                           long long* status, hipStream_t s) {
    if (P < 1 || max_points < 1 || max_points > kNnMaxPoints) return hipErrorInvalidValue;
    const long chunks = nn_pairs_chunks(max_points);
    if (2 * P * chunks > 0x7fffffffL || chunks > 65535) return hipErrorInvalidValue;
    NnArgs g;
    g.a = reinterpret_cast<const f32x4*>(a), g.b = reinterpret_cast<const f32x4*>(b);
    g.off_a = off_a, g.off_b = off_b;
    g.clouds_a = clouds_a, g.clouds_b = clouds_b, g.total_a = total_a, g.total_b = total_b;
    g.pairs = pairs;
    g.max_points = max_points;
    g.tau2 = tau * tau;
    g.d2[0] = d2_ab, g.d2[1] = d2_ba, g.idx[0] = idx_ab, g.idx[1] = idx_ba;
    g.out_off[0] = out_ab, g.out_off[1] = out_ba;
    g.part = static_cast<double*>(scratch);
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(long long), s);
    if (e != hipSuccess) return e;
    nn_pairs_kernel<<<dim3((unsigned)(2 * P), (unsigned)chunks), kNnThreads, 0, s>>>(g);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    nn_finalize_kernel<<<(unsigned)((2 * P + 255) / 256), 256, 0, s>>>(g, P, (int)chunks, sums, reinterpret_cast<unsigned long long*>(status));
    return hipGetLastError();
}

}  // namespace r2dm
