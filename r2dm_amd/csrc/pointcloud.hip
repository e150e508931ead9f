// K16: range images -> point clouds, the inverse of projection.hip: a batch of images becomes a batch of compacted
// [x, y, z, reflectance] scans in one buffer with offsets (Velodyne .bin rows).  A stream compaction whose output ORDER is part of the
// contract:
//
//  count_kernel    one block of 256 positions per (scan, chunk): the number of valid pixels among them.
//  prefix_kernel   exclusive prefix sum of the B * ceil(HW / 256) counts, the total in one more slot (one block walks the list; the
//                  scheme of projection.hip's block_offsets_kernel, restated here so that file stays as it is).
//  write_kernel    validity and the point again, through the same device function as the count; rank inside the wave from a 64-bit
//                  ballot, wave bases through LDS, one 16-byte store per point at points[block offset + rank]; the pixel's index and
//                  the scans' offsets next to it.
//
// Position p in [0, HW) of a scan is pixel (h, w):  image order  h = p / W, w = p % W;  scan order  h = p / W,
// w = (row_start[h] - p % W) mod W -- rows top to bottom, inside a row the columns fall cyclically from row_start[h], the last column
// whose azimuth is >= 0: the azimuth rises from 0+, so a ring ends in the 4th quadrant and the next one starts in the 1st, the
// delimiter that projection.hip (is_delimiter) and the reference's scan unfolding count.
//
// layout 0: src (B,2,H,W), the model's sample in [-1,1]; the point is lidar_post_kernel's (posterior.hip) operation for operation,
// restated: denormalize, revert_depth in the checkpoint's depth format, both masks, metric cos(phi) cos(theta) m2, ...; bit-identical
// to r2dm_lidar_postprocess_fmt.  Valid: m2 == 1, keep_min < metric < keep_max, x, y, z finite (NaN input: every comparison is false).
// layout 1: src (B,5,H,W) [depth, x, y, z, reflectance], copied.  Valid: keep_min < depth < keep_max, x, y, z finite.
//
// No block waits for another block, no atomics: the order of the output does not depend on the schedule.  All stream-ordered.
#include <math.h>

#include "common.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kCloudThreads = 256;

struct CloudParams {
    const float* src;      // (B,2,H,W) or (B,5,H,W)
    const float* ang;      // (2,H,W) [elevation, azimuth], layout 0
    const int* row_start;  // (H) or nullptr: image order
    int W, hw, chunks;     // chunks = ceil(hw / 256)
    float min_d, max_d, log2_range, keep_min, keep_max;
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// position p of scan b -> its pixel (h W + w), its point and whether it is kept; the ONE definition both passes use
template <int LAYOUT, int FMT>
__device__ __forceinline__ bool cloud_point(const CloudParams& P, int b, int p, int& pix, float4& pt) {
    const int h = p / P.W, c = p - h * P.W;
    int w = c;
    if (P.row_start) {
        w = P.row_start[h] % P.W - c;  // in (-2 W, W) whatever the table holds: the pixel stays inside the image
        if (w < 0) w += P.W;
        if (w < 0) w += P.W;
    }
    pix = h * P.W + w;
    const long hw = P.hw;
    if (LAYOUT == 0) {
        const float* xb = P.src + (long)b * 2 * hw;
        // lidar_post_kernel (posterior.hip), operation for operation
        const float d = (xb[pix] + 1.0f) / 2.0f, r = (xb[hw + pix] + 1.0f) / 2.0f;
        float metric;
        if (FMT == 0) metric = exp2f(d * P.log2_range) - 1.0f;
        else if (FMT == 1) metric = __fmul_rn(__frcp_rn(d + 1e-8f), P.min_d);
        else metric = d * P.max_d;
        const float m = (metric > P.min_d && metric < P.max_d) ? 1.0f : 0.0f;
        metric = metric * m;
        const float m2 = (metric > P.min_d && metric < P.max_d) ? 1.0f : 0.0f;
        const float phi = P.ang[pix], theta = P.ang[hw + pix];
        const float cp = cosf(phi);
        pt.x = metric * cp * cosf(theta) * m2;
        pt.y = metric * cp * sinf(theta) * m2;
        pt.z = metric * sinf(phi) * m2;
        pt.w = r;
        return m2 == 1.0f && metric > P.keep_min && metric < P.keep_max && finite3(pt.x, pt.y, pt.z);
    } else {
        const float* sb = P.src + (long)b * 5 * hw;
        const float depth = sb[pix];
        pt.x = sb[hw + pix], pt.y = sb[2 * hw + pix], pt.z = sb[3 * hw + pix], pt.w = sb[4 * hw + pix];
        return depth > P.keep_min && depth < P.keep_max && finite3(pt.x, pt.y, pt.z);
    }
}

template <int LAYOUT, int FMT>
__global__ __launch_bounds__(kCloudThreads) void count_kernel(CloudParams P, int* __restrict__ counts) {
    __shared__ int lds[kCloudThreads / kWave];
    const int b = blockIdx.y;
    const unsigned p = blockIdx.x * kCloudThreads + threadIdx.x;  // < hw + 256 <= 2^31 + 255
    int pix;
    float4 pt;
    const bool keep = p < (unsigned)P.hw && cloud_point<LAYOUT, FMT>(P, b, (int)p, pix, pt);
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) lds[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < kCloudThreads / kWave; ++k) t += lds[k];
        counts[b * P.chunks + blockIdx.x] = t;
    }
}

// counts[0 .. n] (the last entry is padding) -> exclusive prefix sums in place; counts[n] = the total
__global__ __launch_bounds__(kCloudThreads) void prefix_kernel(int* __restrict__ counts, int n) {
    __shared__ int lds[kCloudThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int carry = 0;
    for (long base = 0; base <= n; base += kCloudThreads) {
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
        for (int w = 0; w < kCloudThreads / kWave; ++w) {
            before += w < wave ? lds[w] : 0;
            all += lds[w];
        }
        if (k <= n) counts[k] = carry + before + incl - v;
        carry += all;
    }
}

template <int LAYOUT, int FMT>
__global__ __launch_bounds__(kCloudThreads) void write_kernel(CloudParams P, const int* __restrict__ block_off, float4* __restrict__ points,
                                                              int* __restrict__ index, long long* __restrict__ offsets) {
    __shared__ int lds[kCloudThreads / kWave];
    const int b = blockIdx.y;
    const unsigned p = blockIdx.x * kCloudThreads + threadIdx.x;
    int pix = 0;
    float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool keep = p < (unsigned)P.hw && cloud_point<LAYOUT, FMT>(P, b, (int)p, pix, pt);
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) lds[wave] = __popcll(m);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        offsets[b] = block_off[b * P.chunks];
        if (b == (int)gridDim.y - 1) offsets[gridDim.y] = block_off[gridDim.y * P.chunks];
    }
    if (!keep) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));  // kept lanes below this one
    for (int k = 0; k < wave; ++k) rank += lds[k];
    const long o = (long)block_off[b * P.chunks + blockIdx.x] + rank;  // < B H W < 2^31
    points[o] = pt;
    if (index) index[o] = pix;
}

// ---- launcher -----------------------------------------------------------------------------------
// scratch: [block offsets: B * chunks + 1 i32]
static int cloud_chunks(int H, int W) { return (int)(((long)H * W + kCloudThreads - 1) / kCloudThreads); }

size_t unproject_scratch_bytes(int B, int H, int W) { return (((size_t)B * cloud_chunks(H, W) + 1) * 4 + 255) & ~(size_t)255; }

template <int LAYOUT, int FMT>
static hipError_t launch_cloud(const CloudParams& P, int B, int* block_off, float4* points, int* index, long long* offsets, hipStream_t s) {
    const dim3 grid((unsigned)P.chunks, (unsigned)B);
    hipError_t e;
    count_kernel<LAYOUT, FMT><<<grid, kCloudThreads, 0, s>>>(P, block_off);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    prefix_kernel<<<1, kCloudThreads, 0, s>>>(block_off, B * P.chunks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    write_kernel<LAYOUT, FMT><<<grid, kCloudThreads, 0, s>>>(P, block_off, points, index, offsets);
    return hipGetLastError();
}

hipError_t launch_unproject(const float* src, int layout, const float* angles, const int* row_start, float* points, int* index, long long* offsets,
                            int B, int H, int W, float min_d, float max_d, int depth_format, float keep_min, float keep_max, void* scratch,
                            hipStream_t s) {
    CloudParams P;
    P.src = src, P.ang = angles, P.row_start = row_start, P.W = W, P.hw = H * W, P.chunks = cloud_chunks(H, W);
    P.min_d = min_d, P.max_d = max_d, P.log2_range = (float)log2((double)max_d + 1.0), P.keep_min = keep_min, P.keep_max = keep_max;
    int* block_off = static_cast<int*>(scratch);
    float4* pts = reinterpret_cast<float4*>(points);
    if (layout == 1) return launch_cloud<1, 0>(P, B, block_off, pts, index, offsets, s);
    switch (depth_format) {
        case 0: return launch_cloud<0, 0>(P, B, block_off, pts, index, offsets, s);
        case 1: return launch_cloud<0, 1>(P, B, block_off, pts, index, offsets, s);
        case 2: return launch_cloud<0, 2>(P, B, block_off, pts, index, offsets, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace r2dm
