// K22: earth mover's distance between point clouds of equal size -- the assignment solver behind the EMD variants of COV / MMD / 1-NNA
// (r2dm_amd/geometry.py: emd_pairs, pairwise_emd).
//
//  emd_pairs_kernel     for P pairs of clouds (ia, ib) of n points each: a forward auction with epsilon-scaling in Jacobi rounds (Bertsekas),
//                       one workgroup per pair, the whole auction in LDS between block barriers.  Per pair: a permutation sigma, its true cost
//                       emd = (1/n) sum_i |a_i - b_sigma(i)|, and the weak-duality bound lower = (1/n) (sum_i min_j (c_ij + p_j) - sum_j p_j)
//                       from the final prices p, so that lower <= EMD_exact <= emd whatever the solver's arithmetic did.
//
// Persons are the points of a, objects the points of b.  A person minimises w_ij = c_ij + p_j (the same number as maximising -c_ij - p_j), with
// c = sqrt((ax-bx)^2 + (ay-by)^2 + (az-bz)^2) in fp32 in the difference form of geometry.hip, for the reason given there.
//
// Every loop is bounded: the round loop by the counter `rounds` (at most max_rounds over all phases of a pair; a price increment that rounds away
// in fp32 burns rounds and cannot hang anything), the phase loop because every phase starts with all n >= 1 persons unassigned and therefore
// spends at least one round, every other loop by n.  There is no cross-block synchronisation and no wait on memory.
#include "common.h"
#include "wave_ops.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kEmdThreads = 1024;
constexpr int kEmdWaves = kEmdThreads / 64;
constexpr int kEmdMaxPoints = 3072;     // 48 bytes of LDS per point (below): 147 456 of the 163 840 bytes of a CU
constexpr int kEmdStatus = 5;           // status[code - 1] counts the pairs that ended with code 1..5
enum EmdCode { kEmdOk = 0, kEmdBadPair = 1, kEmdUnequal = 2, kEmdNonFinite = 3, kEmdEpsFloor = 4, kEmdRoundCap = 5 };

long emd_max_points() { return kEmdMaxPoints; }
size_t emd_pairs_scratch_bytes(long P) { return (size_t)P * sizeof(long long); }  // one code per pair

struct EmdArgs {
    const f32x4 *a, *b;                 // (total,4) rows [x, y, z, .]
    const long long *off_a, *off_b;     // (clouds + 1)
    long clouds_a, clouds_b, total_a, total_b;
    const long long* pairs;             // (P,2) [ia, ib]
    long max_points;                    // row length of assignment / prices; no cloud of a pair may have more points
    double eps;
    long long max_rounds;
    int* assignment;                    // nullptr or (P, max_points)
    float* prices;                      // nullptr or (P, max_points)
    double* out;                        // (P,4) emd, lower, rounds, converged
    long long* code;                    // (P) EmdCode
    unsigned long long* status;         // (kEmdStatus)
};

struct EmdCloud {
    long beg, n;
    bool ok;
};
// cloud i of a ragged set (the scheme of geometry.hip): nothing is read through an index or an offset that does not check out
__device__ __forceinline__ EmdCloud emd_cloud(const long long* __restrict__ off, long clouds, long total, long long i, long max_points) {
    EmdCloud c = {0, 0, false};
    if (i < 0 || i >= clouds) return c;
    const long long b = off[i], e = off[i + 1];
    if (b < 0 || e < b || e > total || e - b > max_points) return c;
    c.beg = (long)b;
    c.n = (long)(e - b);
    c.ok = true;
    return c;
}

__device__ __forceinline__ float emd_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// (w1, j1) the smallest w and its object, the lowest object on a tie; w2 the second smallest w (equal to w1 when two objects tie).  The merge of
// two disjoint sets of objects is commutative and associative, so any butterfly gives every lane the wave's result.
__device__ __forceinline__ void emd_merge(float& w1, int& j1, float& w2, float ow1, int oj1, float ow2) {
    const bool take = ow1 < w1 || (ow1 == w1 && oj1 < j1);
    const float loser = take ? w1 : ow1;
    w2 = __builtin_fminf(__builtin_fminf(w2, ow2), loser);
    w1 = take ? ow1 : w1;
    j1 = take ? oj1 : j1;
}
template <int CTRL>
__device__ __forceinline__ void emd_merge_dpp(float& w1, int& j1, float& w2) {
    const float ow1 = wave_dpp<CTRL>(w1), ow2 = wave_dpp<CTRL>(w2);
    const int oj1 = __builtin_amdgcn_update_dpp(0, j1, CTRL, 0xf, 0xf, false);
    emd_merge(w1, j1, w2, ow1, oj1, ow2);
}
// the steps of wave_max_i32 (wave_ops.h): lane ^ 1, ^ 2, the other quad of the 8, the other 8 of the row, the other row, the other half
__device__ __forceinline__ void emd_wave_best(float& w1, int& j1, float& w2) {
    emd_merge_dpp<0xB1>(w1, j1, w2);
    emd_merge_dpp<0x4E>(w1, j1, w2);
    emd_merge_dpp<0x141>(w1, j1, w2);
    emd_merge_dpp<0x128>(w1, j1, w2);
    {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(w1), __float_as_uint(w1), false, false);
        const auto b = __builtin_amdgcn_permlane16_swap((unsigned)j1, (unsigned)j1, false, false);
        const auto c = __builtin_amdgcn_permlane16_swap(__float_as_uint(w2), __float_as_uint(w2), false, false);
        w1 = __uint_as_float(a[0]), j1 = (int)b[0], w2 = __uint_as_float(c[0]);
        emd_merge(w1, j1, w2, __uint_as_float(a[1]), (int)b[1], __uint_as_float(c[1]));
    }
    {
        const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(w1), __float_as_uint(w1), false, false);
        const auto b = __builtin_amdgcn_permlane32_swap((unsigned)j1, (unsigned)j1, false, false);
        const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(w2), __float_as_uint(w2), false, false);
        w1 = __uint_as_float(a[0]), j1 = (int)b[0], w2 = __uint_as_float(c[0]);
        emd_merge(w1, j1, w2, __uint_as_float(a[1]), (int)b[1], __uint_as_float(c[1]));
    }
}
__device__ __forceinline__ double emd_wave_min_f64(double v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = fmin(v, __shfl_xor(v, s));
    return v;
}

// a pair that ends without an answer: NaN, -1, its code, and one count in status.  Called by the whole block.
__device__ void emd_refuse(const EmdArgs& g, long p, int code, long long rounds) {
    for (long j = threadIdx.x; j < g.max_points; j += kEmdThreads) {
        if (g.assignment) g.assignment[p * g.max_points + j] = -1;
        if (g.prices) g.prices[p * g.max_points + j] = NAN;
    }
    if (threadIdx.x == 0) {
        double* o = g.out + 4 * p;
        o[0] = NAN, o[1] = NAN, o[2] = (double)rounds, o[3] = 0.0;
        g.code[p] = code;
        atomicAdd(&g.status[code - 1], 1ULL);
    }
}

// grid (P): block p owns pair p.  LDS per point: the two clouds as planes (24 bytes), price, owner of the object, object of the person, the list
// of unassigned persons (16) and one 64-bit bid slot (8); beside them a kilobyte of reduction slots.  The objects' planes and the prices are read
// as quads: lane l scans the objects 4 (l + 64 k) .. + 3; the planes are padded to a multiple of four with +inf (cost +inf: never the best, and
// the second best only for n = 1).
__global__ __launch_bounds__(kEmdThreads) void emd_pairs_kernel(const EmdArgs g) {
    __shared__ float ax[kEmdMaxPoints], ay[kEmdMaxPoints], az[kEmdMaxPoints];
    __shared__ f32x4 bx4[kEmdMaxPoints / 4], by4[kEmdMaxPoints / 4], bz4[kEmdMaxPoints / 4], price4[kEmdMaxPoints / 4];
    __shared__ int owner[kEmdMaxPoints], obj[kEmdMaxPoints], list[kEmdMaxPoints];
    __shared__ unsigned long long slot[kEmdMaxPoints];
    __shared__ double red[3][kEmdWaves];
    __shared__ float box[6][kEmdWaves];
    __shared__ float part_w1[kEmdWaves], part_w2[kEmdWaves];
    __shared__ int part_j1[kEmdWaves];
    __shared__ int cnt;
    float* bx = reinterpret_cast<float*>(bx4);
    float* by = reinterpret_cast<float*>(by4);
    float* bz = reinterpret_cast<float*>(bz4);
    float* price = reinterpret_cast<float*>(price4);

    const long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long limit = g.max_points < kEmdMaxPoints ? g.max_points : kEmdMaxPoints;
    const EmdCloud ca = emd_cloud(g.off_a, g.clouds_a, g.total_a, g.pairs[2 * p], limit);
    const EmdCloud cb = emd_cloud(g.off_b, g.clouds_b, g.total_b, g.pairs[2 * p + 1], limit);
    // (every refusal below is uniform over the block)
    if (!ca.ok || !cb.ok || (ca.n == 0 && cb.n == 0)) return emd_refuse(g, p, kEmdBadPair, 0);
    if (ca.n != cb.n) return emd_refuse(g, p, kEmdUnequal, 0);
    const int n = (int)ca.n, nq = (n + 3) >> 2;  // 1 <= n <= kEmdMaxPoints

    // ---- load, the joint bounding box ----
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = tid; i < 4 * nq; i += kEmdThreads) {
        f32x4 vb = {INFINITY, INFINITY, INFINITY, 0.f};
        if (i < n) {
            const f32x4 va = g.a[ca.beg + i];
            vb = g.b[cb.beg + i];
            ax[i] = va[0], ay[i] = va[1], az[i] = va[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bad |= !(isfinite(va[k]) && isfinite(vb[k]));
                lo[k] = __builtin_fminf(lo[k], __builtin_fminf(va[k], vb[k]));
                hi[k] = __builtin_fmaxf(hi[k], __builtin_fmaxf(va[k], vb[k]));
            }
            owner[i] = -1, obj[i] = -1;
        }
        bx[i] = vb[0], by[i] = vb[1], bz[i] = vb[2], price[i] = 0.f;
        slot[i] = 0ULL;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float l = -wave_max_f32(-lo[k]), h = wave_max_f32(hi[k]);
        if (lane == 0) box[k][wave] = l, box[3 + k][wave] = h;
    }
    if (tid == 0) cnt = 0;
    if (__syncthreads_or(bad)) return emd_refuse(g, p, kEmdNonFinite, 0);
    float ext[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float l = box[k][0], h = box[3 + k][0];
        for (int w = 1; w < kEmdWaves; ++w) l = __builtin_fminf(l, box[k][w]), h = __builtin_fmaxf(h, box[3 + k][w]);
        ext[k] = h - l;
    }
    const float c_hi = __builtin_sqrtf(emd_d2(ext[0], ext[1], ext[2], 0.f, 0.f, 0.f));  // >= every cost of the pair
    if (!isfinite(c_hi)) return emd_refuse(g, p, kEmdNonFinite, 0);                      // (finite points whose distances overflow fp32)
    if (g.eps < ldexp((double)c_hi, -18)) return emd_refuse(g, p, kEmdEpsFloor, 0);      // an increment could vanish against a price of a few c_hi
    const float eps = (float)g.eps;
    float eps_cur = __builtin_fmaxf(0.5f * c_hi, eps);

    // ---- the auction ----
    long long rounds = 0;
    bool capped = false;
    for (;;) {  // a phase at eps_cur: everybody unassigned (done above for the first), the prices kept
        for (;;) {  // a round
            for (int i0 = 0; i0 < n; i0 += kEmdThreads) {  // the unassigned persons, in any order: a bid depends on the prices alone
                const int i = i0 + tid;
                const bool un = i < n && obj[i] < 0;
                const unsigned long long m = __ballot(un);
                int base = 0;
                if (lane == 0 && m) base = atomicAdd(&cnt, __popcll(m));
                base = __shfl(base, 0);
                if (un) list[base + __popcll(m & ((1ULL << lane) - 1ULL))] = i;
            }
            __syncthreads();
            const int U = cnt;
            if (U == 0) break;
            if (rounds == g.max_rounds) {
                capped = true;
                break;
            }
            // bid.  Most rounds have a handful of bidders (the tail of a phase): with U <= 8 of them, and at least 1024 objects, a person's
            // objects are split over S = 16 / U (rounded down to a power of two) waves, whose results the first of them merges after a barrier
            // (below 1024 objects the barrier costs more than the scan); otherwise the waves take the persons round-robin.  The merge selects
            // values and never computes: a bid does not depend on the split.
            auto scan = [&](int i, int first, int step, float& w1, int& j1, float& w2) {
                const float x = ax[i], y = ay[i], z = az[i];
                w1 = INFINITY, w2 = INFINITY, j1 = 0x7fffffff;
#pragma unroll 2
                for (int q = first; q < nq; q += step) {
                    const f32x4 X = bx4[q], Y = by4[q], Z = bz4[q], Pq = price4[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float w = __builtin_sqrtf(emd_d2(x, y, z, X[e], Y[e], Z[e])) + Pq[e];
                        if (w < w1) {
                            w2 = w1, w1 = w, j1 = 4 * q + e;
                        } else if (w < w2) {
                            w2 = w;
                        }
                    }
                }
                emd_wave_best(w1, j1, w2);
            };
            auto bid = [&](int i, float w1, int j1, float w2) {
                if (j1 >= n) return;            // (no finite value: burns the round)
                if (!(w2 < INFINITY)) w2 = w1;  // n = 1: no second object
                const float b = price[j1] + ((w2 - w1) + eps_cur);
                // prices are >= 0: the fp32 bit order is the numeric order; a tie of bids goes to the lowest person
                atomicMax(&slot[j1], ((unsigned long long)__float_as_uint(b) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
            };
            if (U > kEmdWaves / 2 || nq < 256) {
                for (int k = wave; k < U; k += kEmdWaves) {
                    const int i = list[k];
                    float w1, w2;
                    int j1;
                    scan(i, lane, 64, w1, j1, w2);
                    if (lane == 0) bid(i, w1, j1, w2);
                }
            } else {
                const int S = U == 1 ? 16 : U == 2 ? 8 : U <= 4 ? 4 : 2;
                const int k = wave / S, r = wave % S;
                if (k < U) {
                    float w1, w2;
                    int j1;
                    scan(list[k], lane + 64 * r, 64 * S, w1, j1, w2);
                    if (lane == 0) part_w1[wave] = w1, part_j1[wave] = j1, part_w2[wave] = w2;
                }
                __syncthreads();
                if (k < U && r == 0) {  // lane t < S holds the result of wave + t
                    float w1 = lane < S ? part_w1[wave + lane] : INFINITY, w2 = lane < S ? part_w2[wave + lane] : INFINITY;
                    int j1 = lane < S ? part_j1[wave + lane] : 0x7fffffff;
                    emd_wave_best(w1, j1, w2);
                    if (lane == 0) bid(list[k], w1, j1, w2);
                }
            }
            __syncthreads();
            // assign: the highest bidder of an object takes it at the price of the bid
            if (tid == 0) cnt = 0;
            for (int j = tid; j < n; j += kEmdThreads) {
                const unsigned long long s = slot[j];
                if (s) {
                    const int i = (int)(0xFFFFFFFFu - (unsigned)(s & 0xFFFFFFFFULL));
                    const int old = owner[j];
                    if (old >= 0) obj[old] = -1;  // (old did not bid this round: no other thread writes obj[old])
                    owner[j] = i;
                    obj[i] = j;
                    price[j] = __uint_as_float((unsigned)(s >> 32));
                    slot[j] = 0ULL;
                }
            }
            __syncthreads();
            ++rounds;
        }
        if (capped || eps_cur == eps) break;
        eps_cur = __builtin_fmaxf(0.25f * eps_cur, eps);
        for (int j = tid; j < n; j += kEmdThreads) owner[j] = -1, obj[j] = -1;
        __syncthreads();
    }
    if (capped) return emd_refuse(g, p, kEmdRoundCap, rounds);

    // ---- the cost of the assignment and the dual bound, float64 in a fixed order: thread -> wave -> block ----
    double cost = 0.0, psum = 0.0, dual = 0.0;
    for (int i = tid; i < n; i += kEmdThreads) {
        const int j = obj[i];
        cost += sqrt((double)emd_d2(ax[i], ay[i], az[i], bx[j], by[j], bz[j]));
        psum += (double)price[i];
    }
    for (int i = wave; i < n; i += kEmdWaves) {
        const float x = ax[i], y = ay[i], z = az[i];
        double m = INFINITY;
        for (int q = lane; q < nq; q += 64) {
            const f32x4 X = bx4[q], Y = by4[q], Z = bz4[q], Pq = price4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) m = fmin(m, sqrt((double)emd_d2(x, y, z, X[e], Y[e], Z[e])) + (double)Pq[e]);
        }
        dual += emd_wave_min_f64(m);  // (the same value in every lane)
    }
    cost = wave_sum_f64(cost), psum = wave_sum_f64(psum);
    if (lane == 0) red[0][wave] = cost, red[1][wave] = psum, red[2][wave] = dual;
    for (long j = tid; j < g.max_points; j += kEmdThreads) {
        if (g.assignment) g.assignment[p * g.max_points + j] = j < n ? obj[j] : -1;
        if (g.prices) g.prices[p * g.max_points + j] = j < n ? price[j] : NAN;
    }
    __syncthreads();
    if (tid == 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k)
            for (int w = 0; w < kEmdWaves; ++w) s[k] += red[k][w];
        double* o = g.out + 4 * p;
        o[0] = s[0] / n, o[1] = (s[2] - s[1]) / n, o[2] = (double)rounds, o[3] = 1.0;
        g.code[p] = kEmdOk;
    }
}

// (arguments validated by r2dm_emd_pairs: 1 <= P < 2^31, 1 <= max_points <= kEmdMaxPoints, eps, max_rounds, alignment)
hipError_t launch_emd_pairs(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b, long clouds_b,
                            long total_b, const long long* pairs, long P, long max_points, double eps, long long max_rounds, int* assignment,
                            float* prices, double* out, void* scratch, long long* status, hipStream_t s) {
    if (P < 1 || P > 0x7fffffffL || max_points < 1 || max_points > kEmdMaxPoints || !(eps > 0.0) || max_rounds < 1) return hipErrorInvalidValue;
    EmdArgs g;
    g.a = reinterpret_cast<const f32x4*>(a), g.b = reinterpret_cast<const f32x4*>(b);
    g.off_a = off_a, g.off_b = off_b;
    g.clouds_a = clouds_a, g.clouds_b = clouds_b, g.total_a = total_a, g.total_b = total_b;
    g.pairs = pairs;
    g.max_points = max_points;
    g.eps = eps, g.max_rounds = max_rounds;
    g.assignment = assignment, g.prices = prices, g.out = out;
    g.code = static_cast<long long*>(scratch);
    g.status = reinterpret_cast<unsigned long long*>(status);
    hipError_t e = hipMemsetAsync(status, 0, kEmdStatus * sizeof(long long), s);
    if (e != hipSuccess) return e;
    emd_pairs_kernel<<<(unsigned)P, kEmdThreads, 0, s>>>(g);
    return hipGetLastError();
}

}  // namespace r2dm
