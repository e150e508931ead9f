// k-NN manifold primitives of feature sets (improved precision / recall, density / coverage): for every row i of x (m, dim) over the admissible
// columns j of y (n, dim) the k-th smallest, the smallest (with its column) and the number inside the columns' balls of
//     D2(i, j) = max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j),
// fp64 throughout, without an m x n buffer.  The Gram term runs on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64).
//
// Arithmetic of one D2(i, j), the same for every tiling: the norms are a fixed lane-strided sum and shuffle tree of one wave per row; the dot
// product is ONE accumulator chain over the features in steps of kKT = 16 from 0 (no split over the features), and inside a step 4 matrix
// instructions in a fixed order, instruction j summing the step's features {j, 4 + j, 8 + j, 12 + j}; a tail is padded with zeros.
// Selection, minimum (lowest column on a tie) and count are order-free given those values, so neither the row tile a row falls in nor the number
// of column splits changes a bit of its outputs.
//
// Launch: grid (row tiles of 128) x (column splits); 256 threads = 2 x 2 waves of a 64 x 64 sub-tile each (4 x 4 accumulators of 16 x 16),
// two blocks to a CU so that one block's staging and selection run under the other's matrix work.  A block walks its column range in tiles of
// 128: fp32 tiles of x and y go through registers (the next step's loads fly under this step's matrix work) into LDS and are widened as they
// become operands.  After the last step the D2 tile passes through LDS 32 columns at a time, where two threads per row keep a sorted k-list
// (LDS, [slot][thread]), minimum and count across the column tiles.  Partials go to scratch per row and split; knn_merge_kernel folds the
// splits in split order.
#include <math.h>

#include "common.h"

namespace r2dm {

namespace {

constexpr int kTM = 128, kTN = 128;  // block tile: rows of x, columns (rows of y)
constexpr int kKT = 16;              // features per step
constexpr int kLS = 20;              // LDS row stride in floats (16-byte rows; the 16 rows of a quad read fall on 16 distinct bank quads)
constexpr int kPassCols = 32;        // D2 columns per epilogue pass
constexpr int kPS = kPassCols + 1;   // D2 pass row stride in doubles
constexpr int kMaxK = 16;
constexpr int kTargetBlocks = 512;   // blocks aimed at: two resident blocks on each of 256 CUs

using f64x4 = __attribute__((ext_vector_type(4))) double;

// sorted ascending list of k values at list[slot * stride]; v is inserted when it is below the last
__device__ __forceinline__ void list_insert(double* list, int stride, int k, double v) {
    if (!(v < list[(k - 1) * stride])) return;
    int s = k - 1;
    while (s > 0 && v < list[(s - 1) * stride]) {
        list[s * stride] = list[(s - 1) * stride];
        --s;
    }
    list[s * stride] = v;
}

// |row|^2 in fp64, one wave per row; *status counts the rows that hold a non-finite value
__global__ __launch_bounds__(256) void knn_norms_kernel(const float* __restrict__ f, long rows, int dim, double* __restrict__ norm2,
                                                        unsigned long long* __restrict__ status) {
    const long r = (long)blockIdx.x * 4 + threadIdx.x / kWave;
    if (r >= rows) return;
    const int lane = threadIdx.x % kWave;
    const float* p = f + (size_t)r * dim;
    double s = 0.0;
    bool bad = false;
    for (int k = lane; k < dim; k += kWave) {
        const float v = p[k];
        bad |= !(fabsf(v) <= 3.402823466e38f);
        s = fma((double)v, (double)v, s);
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
    const bool any = __any(bad);
    if (lane == 0) {
        norm2[r] = s;
        if (any) atomicAdd(status, 1ULL);
    }
}

struct KnnArgs {
    const float *x, *y;
    const double *nx, *ny, *radius2;
    double *plist, *pmin;  // per split and row: k-list, minimum
    int *parg, *pcount;    // its column, the count
    int m, n, dim, k, same, splits;
};

// rows [r0, r0 + 128) x features [k0, k0 + 16) of f as 2 quads per thread: quad e = threadIdx.x + 256 u is row e / 4, features 4 (e % 4) ...
template <bool VEC>
__device__ __forceinline__ void load_tile(const float* __restrict__ f, int rows, int dim, int r0, int k0, f32x4 (&q)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = threadIdx.x + 256 * u, r = r0 + (e >> 2), k = k0 + 4 * (e & 3);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < rows) {
            const float* p = f + (size_t)r * dim + k;
            if constexpr (VEC) {
                if (k < dim) v = *reinterpret_cast<const f32x4*>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k + j < dim) v[j] = p[j];
            }
        }
        q[u] = v;
    }
}

__device__ __forceinline__ void store_tile(float* lds, const f32x4 (&q)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = threadIdx.x + 256 * u;
        *reinterpret_cast<f32x4*>(lds + (e >> 2) * kLS + 4 * (e & 3)) = q[u];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void knn_tiles_kernel(const KnnArgs a) {
    __shared__ __attribute__((aligned(16))) double stage_d[kTM * kPS];  // x tile, y tile (fp32); the D2 pass (128 x 33 doubles) overlays them
    __shared__ double lists[kMaxK * 256];                                  // [slot][thread]
    static_assert(sizeof(float) * 2 * kTM * kLS <= kTM * kPS * sizeof(double), "the operand tiles fit under the D2 pass");
    float* xs = reinterpret_cast<float*>(stage_d);
    float* ys = xs + kTM * kLS;
    double* pass = stage_d;

    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    const int wr = wave >> 1, wc = wave & 1;  // the wave's 64 x 64 sub-tile
    const int l16 = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * kTM, split = blockIdx.y;
    const int col_tiles = (a.n + kTN - 1) / kTN;
    const int tile_lo = (int)((long)split * col_tiles / a.splits), tile_hi = (int)((long)(split + 1) * col_tiles / a.splits);  // (splits <= col_tiles: none is empty)

    // selection state of thread t: row t % 128, columns 16 (t / 128) ... + 15 of each pass
    const int srow = t & (kTM - 1), shalf = t >> 7;
    const int si = i0 + srow;
    double best = INFINITY;
    int best_j = -1, cnt = 0;
    for (int s = 0; s < a.k; ++s) lists[s * 256 + t] = INFINITY;

    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const int j0 = tile * kTN;
        f64x4 acc[4][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};

        f32x4 qx[2], qy[2];
        load_tile<VEC>(a.x, a.m, a.dim, i0, 0, qx);
        load_tile<VEC>(a.y, a.n, a.dim, j0, 0, qy);
        for (int k0 = 0; k0 < a.dim; k0 += kKT) {
            __syncthreads();  // the previous step's operand reads (or the previous tile's D2 pass) are done
            store_tile(xs, qx);
            store_tile(ys, qy);
            __syncthreads();
            if (k0 + kKT < a.dim) {
                load_tile<VEC>(a.x, a.m, a.dim, i0, k0 + kKT, qx);
                load_tile<VEC>(a.y, a.n, a.dim, j0, k0 + kKT, qy);
            }
            f32x4 af[4], bf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                af[u] = *reinterpret_cast<const f32x4*>(xs + (64 * wr + 16 * u + l16) * kLS + 4 * g);
                bf[u] = *reinterpret_cast<const f32x4*>(ys + (64 * wc + 16 * u + l16) * kLS + 4 * g);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)af[mi][j], (double)bf[ni][j], acc[mi][ni], 0, 0, 0);
        }

        // D2 of the tile, 32 columns a pass: pass p takes accumulator column ni = p of every wave (columns 64 wc + 16 p + l16 of the tile)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            __syncthreads();  // the operand reads / the previous pass's reads are done
            {
                const int j = j0 + 64 * wc + 16 * p + l16;
                const double nyj = j < a.n ? a.ny[j] : 0.0;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 64 * wr + 16 * mi + g + 4 * r;  // f64 C/D layout: row = (lane >> 4) + 4 reg, col = lane & 15
                        const double nxi = i0 + row < a.m ? a.nx[i0 + row] : 0.0;
                        pass[row * kPS + 16 * wc + l16] = fmax(0.0, fma(-2.0, acc[mi][p][r], nxi + nyj));
                    }
            }
            __syncthreads();
            if (si < a.m) {
                for (int c = 0; c < 16; ++c) {
                    const int j = j0 + 64 * shalf + 16 * p + c;
                    if (j >= a.n) break;
                    if (a.same && j == si) continue;
                    const double v = pass[srow * kPS + 16 * shalf + c];
                    if (a.k) list_insert(lists + t, 256, a.k, v);
                    if (v < best) best = v, best_j = j;  // (a thread meets its columns in ascending order)
                    if (a.radius2 && v <= a.radius2[j]) ++cnt;
                }
            }
        }
    }

    // fold the two threads of a row, write the row's partial of this split
    __syncthreads();
    double* fmin = pass;                                          // [128]
    int* farg = reinterpret_cast<int*>(pass + kTM);               // [128]
    int* fcnt = farg + kTM;                                       // [128]
    if (shalf == 1) fmin[srow] = best, farg[srow] = best_j, fcnt[srow] = cnt;
    __syncthreads();
    if (shalf == 0 && si < a.m) {
        for (int s = 0; s < a.k; ++s) list_insert(lists + t, 256, a.k, lists[s * 256 + t + kTM]);
        const double ob = fmin[srow];
        const int oj = farg[srow];
        if (oj >= 0 && (ob < best || best_j < 0 || (ob == best && oj < best_j))) best = ob, best_j = oj;
        cnt += fcnt[srow];
        const size_t o = (size_t)split * a.m + si;
        for (int s = 0; s < a.k; ++s) a.plist[o * a.k + s] = lists[s * 256 + t];
        a.pmin[o] = best;
        a.parg[o] = best_j;
        a.pcount[o] = cnt;
    }
}

// one thread per row: the splits' partials in split order (their column ranges ascend, so the first strict minimum has the lowest column)
__global__ __launch_bounds__(64) void knn_merge_kernel(const double* __restrict__ plist, const double* __restrict__ pmin, const int* __restrict__ parg,
                                                       const int* __restrict__ pcount, int m, int k, int splits, double* __restrict__ kth2,
                                                       double* __restrict__ min2, int* __restrict__ argmin, int* __restrict__ count) {
    __shared__ double lists[kMaxK * 64];
    const int t = threadIdx.x, i = blockIdx.x * 64 + t;
    if (i >= m) return;
    for (int s = 0; s < k; ++s) lists[s * 64 + t] = INFINITY;
    double best = INFINITY;
    int best_j = -1, cnt = 0;
    for (int sp = 0; sp < splits; ++sp) {
        const size_t o = (size_t)sp * m + i;
        for (int s = 0; s < k; ++s) list_insert(lists + t, 64, k, plist[o * k + s]);
        const int oj = parg[o];
        if (oj >= 0 && (best_j < 0 || pmin[o] < best)) best = pmin[o], best_j = oj;
        cnt += pcount[o];
    }
    if (kth2) kth2[i] = lists[(k - 1) * 64 + t];
    if (min2) min2[i] = best;
    if (argmin) argmin[i] = best_j;
    if (count) count[i] = cnt;
}

size_t align8(size_t b) { return (b + 7) / 8 * 8; }

}  // namespace

void feature_knn_launch_shape(long m, long n, int* row_tiles, int* splits) {
    const long rt = (m + kTM - 1) / kTM, ct = (n + kTN - 1) / kTN;
    const long sp = kTargetBlocks / rt;
    *row_tiles = (int)rt;
    *splits = (int)(sp < 1 ? 1 : (sp > ct ? ct : sp));  // split s takes the column tiles [s ct / splits, (s + 1) ct / splits)
}

size_t feature_knn_scratch_bytes(long m, long n, int k) {
    int rt, sp;
    feature_knn_launch_shape(m, n, &rt, &sp);
    const size_t rows = (size_t)sp * (size_t)m;
    return (size_t)(m + n) * sizeof(double) + rows * (size_t)k * sizeof(double) + rows * sizeof(double) + 2 * align8(rows * sizeof(int));
}

hipError_t launch_feature_knn(const float* x, long m, const float* y, long n, int dim, int same, int k, const double* y_radius2, double* kth2,
                              double* min2, int* argmin, int* count, void* scratch, long long* status, hipStream_t s) {
    int rt, sp;
    feature_knn_launch_shape(m, n, &rt, &sp);
    const size_t rows = (size_t)sp * (size_t)m;
    double* nx = static_cast<double*>(scratch);
    double* ny = nx + m;
    double* plist = ny + n;
    double* pmin = plist + rows * (size_t)k;
    int* parg = reinterpret_cast<int*>(pmin + rows);
    int* pcount = reinterpret_cast<int*>(reinterpret_cast<char*>(parg) + align8(rows * sizeof(int)));
    hipError_t e = hipMemsetAsync(status, 0, sizeof(long long), s);
    if (e != hipSuccess) return e;
    knn_norms_kernel<<<(unsigned)((m + 3) / 4), 256, 0, s>>>(x, m, dim, nx, reinterpret_cast<unsigned long long*>(status));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (same) {
        ny = nx;
    } else {
        knn_norms_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(y, n, dim, ny, reinterpret_cast<unsigned long long*>(status));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const KnnArgs a{x, y, nx, ny, count ? y_radius2 : nullptr, plist, pmin, parg, pcount, (int)m, (int)n, dim, kth2 ? k : 0, same, sp};
    if (dim % 4 == 0) knn_tiles_kernel<true><<<dim3((unsigned)rt, (unsigned)sp), 256, 0, s>>>(a);
    else knn_tiles_kernel<false><<<dim3((unsigned)rt, (unsigned)sp), 256, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    knn_merge_kernel<<<(unsigned)((m + 63) / 64), 64, 0, s>>>(plist, pmin, parg, pcount, (int)m, a.k, sp, kth2, min2, argmin, count);
    return hipGetLastError();
}

}  // namespace r2dm
