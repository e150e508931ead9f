// K15: raw LiDAR scans -> range images: load_points_as_images of the reference's dataset builders (data/kitti_360/kitti_360.py:34-93,
// the same in data/kitti_raw) and the builder's xyzrdm *= mask (kitti_360.py:164-165), for a batch of scans in one buffer.
//
//  delim_count_kernel     scan unfolding: the number of ring delimiters in every block of 256 points.
//  block_offsets_kernel   exclusive prefix sum of those counts (one block walks the list).
//  scan_bounds_kernel     the number of delimiters in front of every scan's first point -> per-scan base and total.
//  scatter_kernel         per point: depth, grid cell, and a 64-bit unsigned atomic min of (depth bits << 32 | index in the scan) on the cell.
//  gather_kernel          per output pixel: the winner's six values, masked or not, at the native or a narrower width.
//
// The reference writes the points in order of decreasing depth, so a cell keeps its NEAREST point, inside the depth window or not; among
// equal depths its order is unspecified (unstable argsort) -- here the lowest index in the file wins.  Positive finite floats order like their
// bit patterns, so one integer atomic min gives both, independent of the launch order.  No float atomics.
//
// Scan unfolding's row is a function of the point's position in the file: seg(i) = the number of delimiters at positions <= i of its scan
// (a delimiter: the previous point, cyclically, in the 4th quadrant and this one in the 1st), D = the scan's total:
//     h = 0 if seg == 0;  r = H - 1 - (D - seg);  h = r if r >= 0,  H - 1 if r == -1 (the reference's loop assigns -1 once before it stops and
//     the negative index wraps),  0 if r < -1 (never assigned).
// The delimiter flags of the WHOLE buffer get one prefix count G (block counts, their offsets, a ballot inside the block); with
// base[b] = G in front of scan b:  seg = G(i) - base[b],  D = base[b + 1] - base[b].  Nothing per point is stored.
//
// Undefined input (the reference casts NaN to int there): a point whose depth is not a finite number > 0 -- a NaN or infinite coordinate,
// squares that overflow, (0,0,0) -- never wins a cell, in either mode; it still has a quadrant (NaN compares false: quadrant 0, as numpy
// leaves it) and keeps its position in the sequence for scan unfolding.  Grid coordinates are clamped as floating-point numbers (NaN -> 0)
// before the conversion to an integer.
//
// All arithmetic of the contract is fp32 with one rounding per operation (no contraction); the spherical row is evaluated in fp64 from the
// fp32 asin, as numpy >= 2 promotes it (np.deg2rad returns a float64 scalar).
#include <math.h>

#include "common.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kProjThreads = 256;
constexpr unsigned long long kEmptyCell = ~0ull;

struct ProjParams {
    const float4* points;   // (total) [x, y, z, reflectance]
    const long long* off;   // (B + 1) device copy of the offsets
    int B, H, W;
    long long total;
};

struct OffsetChunk {
    static constexpr int kN = 256;
    int first, count;
    long long v[kN];
};

__global__ __launch_bounds__(OffsetChunk::kN) void store_offsets_kernel(OffsetChunk c, long long* __restrict__ off) {
    if ((int)threadIdx.x < c.count) off[c.first + threadIdx.x] = c.v[threadIdx.x];
}

__device__ __forceinline__ int scan_of(const long long* __restrict__ off, int B, long long i) {  // the b with off[b] <= i < off[b + 1]
    int lo = 0, hi = B;  // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int quadrant(float x, float y) {  // kitti_360.py:55-59 (all comparisons false: stays 0)
    if (x < 0.f) return y >= 0.f ? 1 : (y < 0.f ? 2 : 0);
    if (x >= 0.f && y < 0.f) return 3;
    return 0;
}

// kitti_360.py:62-63: np.roll(quads, 1) - quads == 3
__device__ __forceinline__ bool is_delimiter(const ProjParams& P, long long i, int b, const float4& p) {
    const long long s = P.off[b], e = P.off[b + 1];
    const float4 q = P.points[i == s ? e - 1 : i - 1];
    return quadrant(q.x, q.y) == 3 && quadrant(p.x, p.y) == 0;
}

__device__ __forceinline__ int block_sum(int v, int* lds) {  // all threads get the block's total; lds: kProjThreads / kWave ints
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x / kWave;
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) lds[wave] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int k = 0; k < kProjThreads / kWave; ++k) t += lds[k];
    return t;
}

__global__ __launch_bounds__(kProjThreads) void delim_count_kernel(ProjParams P, int* __restrict__ counts) {
    __shared__ int lds[kProjThreads / kWave];
    const long long i = (long long)blockIdx.x * kProjThreads + threadIdx.x;
    int f = 0;
    if (i < P.total) f = is_delimiter(P, i, scan_of(P.off, P.B, i), P.points[i]);
    const int t = block_sum(f, lds);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// counts[0 .. n] (the last entry is padding) -> exclusive prefix sums in place; counts[n] = the total
__global__ __launch_bounds__(kProjThreads) void block_offsets_kernel(int* __restrict__ counts, long n) {
    __shared__ int lds[kProjThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int carry = 0;
    for (long base = 0; base <= n; base += kProjThreads) {
        const long k = base + threadIdx.x;
        const int v = k < n ? counts[k] : 0;
        int incl = v;
        for (int o = 1; o < kWave; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        __syncthreads();  // (the previous round's reads of lds)
        if (lane == kWave - 1) lds[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kProjThreads / kWave; ++w) {
            before += w < wave ? lds[w] : 0;
            all += lds[w];
        }
        if (k <= n) counts[k] = carry + before + incl - v;
        carry += all;
    }
}

// base[b] = the number of delimiters at positions < off[b], b = 0 .. B
__global__ __launch_bounds__(kProjThreads) void scan_bounds_kernel(ProjParams P, const int* __restrict__ block_off, int* __restrict__ base) {
    __shared__ int lds[kProjThreads / kWave];
    const long long p = P.off[blockIdx.x];
    const long long blk = p / kProjThreads, i = blk * kProjThreads + threadIdx.x;
    int f = 0;
    if (i < p) f = is_delimiter(P, i, scan_of(P.off, P.B, i), P.points[i]);
    const int t = block_sum(f, lds);
    if (threadIdx.x == 0) base[blockIdx.x] = block_off[blk] + t;
}

// a grid coordinate as a number -> an index in [0, n - 1]; NaN -> 0
__device__ __forceinline__ int clamp_index(double v, int n) { return v >= 0.0 ? (v < (double)(n - 1) ? (int)v : n - 1) : 0; }

template <bool UNFOLD>
__global__ __launch_bounds__(kProjThreads) void scatter_kernel(ProjParams P, const int* __restrict__ block_off, const int* __restrict__ base,
                                                               unsigned long long* __restrict__ cells, double h_down, double h_span) {
    __shared__ int lds[kProjThreads / kWave];
    const long long i = (long long)blockIdx.x * kProjThreads + threadIdx.x;
    const bool valid = i < P.total;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    int b = 0;
    if (valid) {
        p = P.points[i];
        b = scan_of(P.off, P.B, i);
    }
    int h = 0;
    bool wins = valid;
    const float depth = sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z);  // np.linalg.norm of a float32 row
    wins = wins && depth > 0.f && depth < INFINITY;
    if (UNFOLD) {
        // inclusive prefix count of the block's delimiter flags: ballot inside the wave, LDS across the waves (the whole block takes part)
        const bool f = valid && is_delimiter(P, i, b, p);
        const unsigned long long m = __ballot(f);
        const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
        if (lane == 0) lds[wave] = __popcll(m);
        __syncthreads();
        int g = __popcll(m & (~0ull >> (kWave - 1 - lane)));
        for (int w = 0; w < wave; ++w) g += lds[w];
        if (valid) {
            const int seg = block_off[blockIdx.x] + g - base[b], D = base[b + 1] - base[b];
            const int r = P.H - 1 - (D - seg);
            h = seg == 0 ? 0 : (r >= 0 ? r : (r == -1 ? P.H - 1 : 0));
        }
    } else if (wins) {
        // kitti_360.py:76-79: float32 arcsin, then float64 (the degrees are float64 scalars)
        const double elevation = (double)asinf(p.z / depth) + h_down;
        const double gh = 1.0 - elevation / h_span;
        h = clamp_index(floor(gh * (double)P.H), P.H);
    }
    if (!wins) return;
    // kitti_360.py:82-84 in float32
    const float azimuth = -atan2f(p.y, p.x);
    float gw = (azimuth / 3.14159274f + 1.0f) / 2.0f;
    gw = gw - floorf(gw);  // % 1 (exact)
    const int w = clamp_index((double)floorf(gw * (float)P.W), P.W);
    const long long s = P.off[b];
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(unsigned)(i - s);
    atomicMin(cells + ((long long)b * P.H + h) * P.W + w, key);
}

// layout 0: out (B,6,H,Wo) [x, y, z, reflectance, depth, mask]; 1: (B,5,H,Wo) [depth, x, y, z, reflectance] (the sample layout)
__global__ __launch_bounds__(kProjThreads) void gather_kernel(ProjParams P, const unsigned long long* __restrict__ cells, float* __restrict__ out,
                                                              int Wo, float min_depth, float max_depth, int apply_mask, int layout) {
    const long long hw = (long long)P.H * Wo, n = (long long)P.B * hw;
    const long long o = (long long)blockIdx.x * kProjThreads + threadIdx.x;
    if (o >= n) return;
    const long long b = o / hw, r = o - b * hw;
    const int h = (int)(r / Wo), j = (int)(r - (long long)h * Wo);
    // F.interpolate(mode="nearest-exact"): source column floor((j + 0.5) W / Wo)
    const int w = Wo == P.W ? j : (int)(((2LL * j + 1) * P.W) / (2LL * Wo));
    const unsigned long long key = cells[(b * P.H + h) * P.W + w];
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (key != kEmptyCell) {
        const float4 p = P.points[P.off[b] + (long long)(unsigned)key];
        const float depth = __uint_as_float((unsigned)(key >> 32));
        const float mask = (depth >= min_depth && depth <= max_depth) ? 1.0f : 0.0f;
        const float m = apply_mask ? mask : 1.0f;  // (x * 0 keeps x's sign, as the reference's product does)
        v[0] = p.x * m, v[1] = p.y * m, v[2] = p.z * m, v[3] = p.w * m, v[4] = depth * m, v[5] = mask;
    }
    if (layout == 0) {
        float* q = out + b * 6 * hw + r;
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k * hw] = v[k];
    } else {
        float* q = out + b * 5 * hw + r;
        q[0] = v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[(k + 1) * hw] = v[k];
    }
}

// ---- launcher -----------------------------------------------------------------------------------
// scratch: [cells: B H W u64][offsets: B + 1 i64][base: B + 1 i32, padded to 8][block offsets: blocks + 1 i32]
static size_t proj_blocks(long long total) { return (size_t)((total + kProjThreads - 1) / kProjThreads); }

size_t project_scratch_bytes(long long total, int B, int H, int W, int unfold) {
    size_t n = (size_t)B * H * W * 8 + (size_t)(B + 1) * 8;
    if (unfold) n += (size_t)(B + 2) / 2 * 8 + (proj_blocks(total) + 1) * 4;
    return n;
}

hipError_t launch_project_scans(const float* points, const long long* offsets, float* out, int B, int H, int W, int Wo, int unfold, float min_depth,
                                float max_depth, int apply_mask, int layout, void* scratch, hipStream_t s) {
    const long long total = offsets[B];
    const size_t blocks = proj_blocks(total);
    char* sp = static_cast<char*>(scratch);
    unsigned long long* cells = reinterpret_cast<unsigned long long*>(sp);
    sp += (size_t)B * H * W * 8;
    long long* off = reinterpret_cast<long long*>(sp);
    sp += (size_t)(B + 1) * 8;
    int* base = reinterpret_cast<int*>(sp);
    sp += (size_t)(B + 2) / 2 * 8;
    int* block_off = reinterpret_cast<int*>(sp);

    hipError_t e = hipMemsetAsync(cells, 0xff, (size_t)B * H * W * 8, s);
    if (e != hipSuccess) return e;
    // the host's offsets travel as kernel arguments: taken at the launch, so the caller's array is free when this returns
    for (int k0 = 0; k0 <= B; k0 += OffsetChunk::kN) {
        OffsetChunk c;
        c.first = k0, c.count = B + 1 - k0 < OffsetChunk::kN ? B + 1 - k0 : OffsetChunk::kN;
        for (int k = 0; k < c.count; ++k) c.v[k] = offsets[k0 + k];
        store_offsets_kernel<<<1, OffsetChunk::kN, 0, s>>>(c, off);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProjParams P;
    P.points = reinterpret_cast<const float4*>(points), P.off = off, P.B = B, P.H = H, P.W = W, P.total = total;
    if (total > 0) {
        if (unfold) {
            delim_count_kernel<<<(unsigned)blocks, kProjThreads, 0, s>>>(P, block_off);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            block_offsets_kernel<<<1, kProjThreads, 0, s>>>(block_off, (long)blocks);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            scan_bounds_kernel<<<(unsigned)(B + 1), kProjThreads, 0, s>>>(P, block_off, base);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            scatter_kernel<true><<<(unsigned)blocks, kProjThreads, 0, s>>>(P, block_off, base, cells, 0.0, 1.0);
        } else {
            // np.deg2rad(3), np.deg2rad(-25): x * (pi / 180) in float64
            const double h_up = 3.0 * (M_PI / 180.0), h_down = -25.0 * (M_PI / 180.0);
            scatter_kernel<false><<<(unsigned)blocks, kProjThreads, 0, s>>>(P, nullptr, nullptr, cells, fabs(h_down), h_up - h_down);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const long long n = (long long)B * H * Wo;
    gather_kernel<<<(unsigned)((n + kProjThreads - 1) / kProjThreads), kProjThreads, 0, s>>>(P, cells, out, Wo, min_depth, max_depth, apply_mask, layout);
    return hipGetLastError();
}

}  // namespace r2dm
