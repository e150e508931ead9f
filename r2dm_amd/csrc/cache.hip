// The feature cache's one kernel (DeepCache: forward.hip run_forward, CacheWalk): cached <- fresh, bit for bit, while measuring how far the feature has
// drifted since it was last stored -- per sample sum (fresh - old)^2 and sum old^2, in float64 from the stored values.  One pass: 8 bytes read and 4 written
// per fp32 value, nothing else -- HBM-bound; 16-byte accesses, four per lane in flight, at most 2048 blocks that stride the sample.
// No float atomics: every block leaves its pair in `partial`, a second launch of one wave per sample adds them in a fixed order, so the
// sums are the same bits from call to call.
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"
#include "wave_ops.h"

namespace r2dm {

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
constexpr int kMaxBlocks = 512;  // per sample: what `partial` is sized for (include/r2dm_hip.h)

template <bool F16>
__device__ __forceinline__ double stored(unsigned bits, int half_index) {
    if (F16) return (double)__half2float(__ushort_as_half((unsigned short)(half_index ? bits >> 16 : bits & 0xffffu)));
    return (double)__uint_as_float(bits);
}
// one 16-byte quad of each tensor: 4 fp32 or 8 fp16 values
template <bool F16>
__device__ __forceinline__ void add_quad(const u32x4& a, const u32x4& o, double& d2, double& o2) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int hi = 0; hi < (F16 ? 2 : 1); ++hi) {
            const double f = stored<F16>(a[j], hi), c = stored<F16>(o[j], hi), d = f - c;
            d2 = fma(d, d, d2);
            o2 = fma(c, c, o2);
        }
}

// grid (blocks per sample, B) x 256 threads.  A sample's n values start 16-byte aligned only where b * n * sizeof(T) is a multiple of 16 (both tensors are, so
// they share the offset): block 0 takes the `head` values in front of the first aligned one and the tail behind the last whole quad one by one.
template <bool F16>
__global__ __launch_bounds__(256) void cache_store_kernel(const void* __restrict__ fresh, void* __restrict__ cached, long n, double* __restrict__ partial) {
    using T = typename std::conditional<F16, unsigned short, unsigned>::type;
    constexpr int V = 16 / (int)sizeof(T);
    const int b = blockIdx.y, nblk = gridDim.x;
    const T* f = (const T*)fresh + (size_t)b * n;
    T* c = (T*)cached + (size_t)b * n;
    const long mis = (long)(((size_t)b * (size_t)n * sizeof(T)) & 15);
    long head = mis ? (16 - mis) / (long)sizeof(T) : 0;
    if (head > n) head = n;
    const long nvec = (n - head) / V, tail0 = head + nvec * V;
    const u32x4* f4 = reinterpret_cast<const u32x4*>(f + head);
    u32x4* c4 = reinterpret_cast<u32x4*>(c + head);
    double d2 = 0.0, o2 = 0.0;
    const long stride = (long)nblk * 256;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += 4 * stride) {  // four quads of each tensor in flight per lane
        u32x4 a[4], o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < nvec) {
                a[u] = __builtin_nontemporal_load(f4 + i + u * stride);
                o[u] = c4[i + u * stride];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < nvec) {
                c4[i + u * stride] = a[u];
                add_quad<F16>(a[u], o[u], d2, o2);
            }
    }
    if (blockIdx.x == 0) {
        const long loose = head + (n - tail0);
        for (long i = threadIdx.x; i < loose; i += 256) {
            const long j = i < head ? i : tail0 + (i - head);
            const T a = f[j], o = c[j];
            c[j] = a;
            const double fv = stored<F16>((unsigned)a, 0), cv = stored<F16>((unsigned)o, 0), d = fv - cv;
            d2 = fma(d, d, d2);
            o2 = fma(cv, cv, o2);
        }
    }
    __shared__ double red[4][2];
    d2 = wave_sum_f64(d2);
    o2 = wave_sum_f64(o2);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = d2;
        red[wave][1] = o2;
    }
    __syncthreads();
    if (threadIdx.x < 2) partial[((size_t)b * nblk + blockIdx.x) * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one wave per sample: lane l adds blocks l, l + 64, ... in that order, then the wave's fixed-order sum
__global__ __launch_bounds__(64) void cache_store_sum_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ sums) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double d2 = 0.0, o2 = 0.0;
    for (int j = lane; j < nblk; j += 64) {
        d2 += partial[((size_t)b * nblk + j) * 2];
        o2 += partial[((size_t)b * nblk + j) * 2 + 1];
    }
    d2 = wave_sum_f64(d2);
    o2 = wave_sum_f64(o2);
    if (lane == 0) {
        sums[2 * b] = d2;
        sums[2 * b + 1] = o2;
    }
}

}  // namespace

// blocks per sample: about 4096 values each, at most kMaxBlocks and 2048 over the batch; a function of (B, n) alone, so the summation order is too
int cache_store_blocks(int B, long n) {
    long k = (n + 4095) / 4096;
    const long cap = 2048 / B < kMaxBlocks ? (2048 / B > 0 ? 2048 / B : 1) : kMaxBlocks;
    if (k > cap) k = cap;
    return k < 1 ? 1 : (int)k;
}

hipError_t launch_cache_store(const void* fresh, void* cached, int B, long n, int f16, double* partial, double* sums, hipStream_t s) {
    if (!fresh || !cached || !partial || !sums || B < 1 || B > 65535 || n < 1) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(fresh) & 15) || (reinterpret_cast<uintptr_t>(cached) & 15) || (reinterpret_cast<uintptr_t>(partial) & 7) ||
        (reinterpret_cast<uintptr_t>(sums) & 7))
        return hipErrorInvalidValue;
    const int nblk = cache_store_blocks(B, n);
    const dim3 g(nblk, B);
    if (f16) cache_store_kernel<true><<<g, 256, 0, s>>>(fresh, cached, n, partial);
    else cache_store_kernel<false><<<g, 256, 0, s>>>(fresh, cached, n, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cache_store_sum_kernel<<<B, 64, 0, s>>>(partial, nblk, sums);
    return hipGetLastError();
}

}  // namespace r2dm
