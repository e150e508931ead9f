// K22: voxel occupancy -- which cells of an axis-aligned grid two or more clouds occupy: voxel IoU / precision / recall / F1 of a pair, and the
// occupancy scores of an ensemble of K clouds against a target (r2dm_amd/geometry.py).
//
//  voxel_groups_kernel  checks every group's cloud indices and offsets once (nothing is read through one that does not check out) and leaves a flag.
//  voxel_clear_kernel   keys := empty, masks := 0 over every (group, size) table.
//  voxel_insert_kernel  every point of every cloud of a group, at every size: the point's voxel key goes into the (group, size) hash set, the
//                       cloud's bit into the slot's membership mask.
//  voxel_count_kernel   every slot of every table: c = popcount(member bits), o = target bit -> hist[o][c] and the member counters, integers in
//                       LDS, one integer atomic per non-zero counter and block.
//
// Only integers are summed, by integer atomics: every output is independent of point order and thread schedule, bit for bit.
//
// The table is a set with open addressing and linear probing in global memory.  A slot goes from empty to a key exactly once, by a 64-bit
// compare-and-swap; there is no other transition and no locked state, so no thread ever waits for another.  The insert kernel decides from
// the values its atomics return only: a plain load of a slot another XCD has just claimed may be stale.  The probe loop is bounded by the
// capacity (a load factor of at most 0.5 by construction: it cannot run out for valid input; if it did, a status says so).
#include "common.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kVoxThreads = 256;
constexpr int kVoxQ = 4;                               // points per thread and pass
constexpr int kVoxChunk = kVoxThreads * kVoxQ;         // points per block and pass
constexpr int kVoxMaxSizes = 8;
constexpr int kVoxMaxMembers = 63;                     // bit 63 of a mask is the target's
constexpr long kVoxMaxGroupPoints = 1L << 27;          // 64 clouds of 2^21 points
constexpr int kVoxMaxGroups = 65535;                   // (a grid dimension)
constexpr int kVoxSlotsPerBlock = kVoxThreads * 8;     // count pass
constexpr unsigned long long kVoxEmpty = ~0ULL;        // a key has 63 bits
constexpr unsigned long long kVoxTargetBit = 1ULL << 63;
constexpr float kVoxGridHalf = 1048576.0f;             // 2^20 cells each way on every axis

long voxel_capacity(long max_group_points) {
    long cap = 2;
    while (cap < 2 * max_group_points) cap <<= 1;
    return cap;
}
bool voxel_geometry_ok(long G, long S, long max_group_points) {
    return G >= 1 && G <= kVoxMaxGroups && S >= 1 && S <= kVoxMaxSizes && max_group_points >= 1 && max_group_points <= kVoxMaxGroupPoints &&
           G * S <= (1L << 36) / voxel_capacity(max_group_points);
}
// [group flags: G int64, padded to 16 bytes][keys: G S cap][masks: G S cap]
static size_t voxel_flag_bytes(long G) { return (size_t)((G * 8 + 15) & ~15L); }
size_t voxel_occupancy_scratch_bytes(long G, long S, long max_group_points) {
    return voxel_flag_bytes(G) + (size_t)G * S * voxel_capacity(max_group_points) * 16;
}

struct VoxArgs {
    const f32x4 *a, *b;                  // (total,4) rows [x, y, z, .]: members from a, targets from b
    const long long *off_a, *off_b;      // (clouds + 1)
    long clouds_a, clouds_b, total_a, total_b;
    const long long *members, *targets;  // (G,K) into a, (G) into b
    int G, K, S;
    float size[kVoxMaxSizes];
    long max_group_points, cap;          // cap: slots per table, a power of two
    long long* ok;                       // (G) 1: every cloud of the group checks out
    unsigned long long *keys, *masks;    // (G, S, cap)
    unsigned long long *member_out, *hist_out, *status;
};

// rows [off[i], off[i+1]) of `total`: n = -1 if the index or the offsets do not check out (nothing is read through an index out of range)
__device__ __forceinline__ long vox_cloud(const long long* __restrict__ off, long clouds, long total, long long i, long* beg) {
    if (i < 0 || i >= clouds) return -1;
    const long long b = off[i], e = off[i + 1];
    if (b < 0 || e < b || e > total) return -1;
    *beg = (long)b;
    return (long)(e - b);
}

// one thread per group.  status[2] += groups that do not check out: a cloud index outside its set, offsets that are not
// 0 <= begin <= end <= total, or more than max_group_points points in the target and the members together.
__global__ __launch_bounds__(256) void voxel_groups_kernel(const VoxArgs g) {
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= g.G) return;
    long beg, sum = vox_cloud(g.off_b, g.clouds_b, g.total_b, g.targets[t], &beg);
    bool ok = sum >= 0;
    for (int k = 0; ok && k < g.K; ++k) {
        const long n = vox_cloud(g.off_a, g.clouds_a, g.total_a, g.members[t * g.K + k], &beg);
        ok = n >= 0 && n <= g.max_group_points - sum;
        sum += n;
    }
    ok = ok && sum <= g.max_group_points;
    g.ok[t] = ok ? 1 : 0;
    if (!ok) atomicAdd(&g.status[2], 1ULL);
}

__global__ __launch_bounds__(256) void voxel_clear_kernel(unsigned long long* __restrict__ keys, unsigned long long* __restrict__ masks, long slots) {
    using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
    const long stride = (long)gridDim.x * 256;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < slots / 2; i += stride) {  // (slots is even: a capacity is a power of two >= 2)
        reinterpret_cast<u64x2*>(keys)[i] = u64x2{kVoxEmpty, kVoxEmpty};
        reinterpret_cast<u64x2*>(masks)[i] = u64x2{0ULL, 0ULL};
    }
}

__device__ __forceinline__ unsigned long long vox_mix(unsigned long long h) {  // the finaliser of MurmurHash3
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ULL;
    h ^= h >> 33;
    return h;
}

// floor(x / s) on one axis as a biased 21-bit index; false outside [-2^20, 2^20).  The division is the IEEE round-to-nearest fp32 division: a
// reciprocal multiply moves points that sit on a cell face.  The range is compared in floating point, before any conversion.
__device__ __forceinline__ bool vox_axis(float x, float s, unsigned long long* idx) {
    const float f = __builtin_floorf(__fdiv_rn(x, s));
    if (!(f >= -kVoxGridHalf && f < kVoxGridHalf)) return false;
    *idx = (unsigned long long)((int)f + (1 << 20));
    return true;
}

// grid (passes, K + 1, G): block (x, y, z) owns the points [1024 x, 1024 x + 1024), then every gridDim.x-th chunk after it, of cloud y of
// group z (y < K: member y, y = K: the target); thread t holds the points 1024 x + 256 j + t, so neighbouring lanes hold neighbouring points
// of the image-ordered cloud.  A point is read once and inserted at every size.
__global__ __launch_bounds__(kVoxThreads) void voxel_insert_kernel(const VoxArgs g) {
    const int grp = blockIdx.z, which = blockIdx.y;
    if (!g.ok[grp]) return;
    const bool is_target = which == g.K;
    long beg = 0;
    const long n = is_target ? vox_cloud(g.off_b, g.clouds_b, g.total_b, g.targets[grp], &beg)
                             : vox_cloud(g.off_a, g.clouds_a, g.total_a, g.members[(long)grp * g.K + which], &beg);
    const f32x4* P = (is_target ? g.b : g.a) + beg;
    const unsigned long long bit = is_target ? kVoxTargetBit : 1ULL << which;
    const unsigned long long wrap = (unsigned long long)g.cap - 1;
    unsigned long long nonfinite = 0, outside = 0, full = 0;
    for (long c0 = (long)blockIdx.x * kVoxChunk; c0 < n; c0 += (long)gridDim.x * kVoxChunk) {  // (uniform over the block)
#pragma unroll
        for (int j = 0; j < kVoxQ; ++j) {
            const long p = c0 + j * kVoxThreads + threadIdx.x;
            const f32x4 v = p < n ? P[p] : f32x4{0.f, 0.f, 0.f, 0.f};
            const bool finite = isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
            if (p < n && !finite) ++nonfinite;
            const bool live = p < n && finite;
            for (int s = 0; s < g.S; ++s) {
                const float size = g.size[s];
                unsigned long long key = kVoxEmpty, ix = 0, iy = 0, iz = 0;
                if (live) {
                    if (vox_axis(v[0], size, &ix) && vox_axis(v[1], size, &iy) && vox_axis(v[2], size, &iz)) key = ix << 42 | iy << 21 | iz;
                    else ++outside;
                }
                // the lane below holds the previous point of the image row: very often the same voxel, and then its insert is this one's too
                // (every lane of the wave is here: the loops above are uniform)
                const unsigned long long below = __shfl_up(key, 1);
                if ((threadIdx.x & 63) != 0 && below == key) key = kVoxEmpty;
                if (key == kVoxEmpty) continue;
                unsigned long long* keys = g.keys + ((long)grp * g.S + s) * g.cap;
                unsigned long long* masks = g.masks + ((long)grp * g.S + s) * g.cap;
                unsigned long long slot = vox_mix(key) & wrap;
                long probe = 0;
                for (; probe < g.cap; ++probe) {
                    const unsigned long long was = atomicCAS(&keys[slot], kVoxEmpty, key);
                    if (was == kVoxEmpty || was == key) {
                        atomicOr(&masks[slot], bit);
                        break;
                    }
                    slot = (slot + 1) & wrap;
                }
                if (probe == g.cap) ++full;
            }
        }
    }
    if (nonfinite) atomicAdd(&g.status[0], nonfinite);
    if (outside) atomicAdd(&g.status[1], outside);
    if (full) atomicAdd(&g.status[3], full);
}

// grid (passes, S, G): block (x, y, z) owns slots [2048 x, 2048 x + 2048), then every gridDim.x-th chunk after it, of table (z, y).
// member_out (G,S,K,2) = |V(M_k)|, |V(M_k) n V(T)|; hist_out (G,S,2,K+1) = #{v: o(v) = o, c(v) = c}.
__global__ __launch_bounds__(kVoxThreads) void voxel_count_kernel(const VoxArgs g) {
    __shared__ unsigned int hist[2 * (kVoxMaxMembers + 1)];
    __shared__ unsigned int member[2 * kVoxMaxMembers];
    const int grp = blockIdx.z, s = blockIdx.y, tid = threadIdx.x;
    if (!g.ok[grp]) return;
    const int K = g.K;
    for (int i = tid; i < 2 * (K + 1); i += kVoxThreads) hist[i] = 0;
    for (int i = tid; i < 2 * K; i += kVoxThreads) member[i] = 0;
    __syncthreads();
    const long table = ((long)grp * g.S + s) * g.cap;
    const unsigned long long* __restrict__ keys = g.keys + table;
    const unsigned long long* __restrict__ masks = g.masks + table;
    // (a block adds at most cap <= 2^28 to a counter: 32 bits hold it)
    for (long c0 = (long)blockIdx.x * kVoxSlotsPerBlock; c0 < g.cap; c0 += (long)gridDim.x * kVoxSlotsPerBlock) {
#pragma unroll
        for (int j = 0; j < kVoxSlotsPerBlock / kVoxThreads; ++j) {
            const long i = c0 + j * kVoxThreads + tid;
            if (i >= g.cap || keys[i] == kVoxEmpty) continue;
            const unsigned long long m = masks[i];
            const int o = (int)(m >> 63);
            unsigned long long rest = m & ~kVoxTargetBit;
            atomicAdd(&hist[o * (K + 1) + __builtin_popcountll(rest)], 1u);
            while (rest) {
                const int k = __builtin_ctzll(rest);
                rest &= rest - 1;
                atomicAdd(&member[2 * k], 1u);
                if (o) atomicAdd(&member[2 * k + 1], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* ho = g.hist_out + ((long)grp * g.S + s) * 2 * (K + 1);
    unsigned long long* mo = g.member_out + ((long)grp * g.S + s) * 2 * K;
    for (int i = tid; i < 2 * (K + 1); i += kVoxThreads)
        if (hist[i]) atomicAdd(&ho[i], (unsigned long long)hist[i]);
    for (int i = tid; i < 2 * K; i += kVoxThreads)
        if (member[i]) atomicAdd(&mo[i], (unsigned long long)member[i]);
}

// (arguments validated by r2dm_voxel_occupancy: voxel_geometry_ok, 1 <= K <= 63, sizes finite and > 0, alignment)
hipError_t launch_voxel_occupancy(const float* a, const long long* off_a, long clouds_a, long total_a, const float* b, const long long* off_b,
                                  long clouds_b, long total_b, const long long* members, const long long* targets, long G, long K, const float* sizes,
                                  long S, long max_group_points, void* scratch, long long* member_out, long long* hist_out, long long* status,
                                  hipStream_t s) {
    if (!voxel_geometry_ok(G, S, max_group_points) || K < 1 || K > kVoxMaxMembers) return hipErrorInvalidValue;
    VoxArgs g;
    g.a = reinterpret_cast<const f32x4*>(a), g.b = reinterpret_cast<const f32x4*>(b);
    g.off_a = off_a, g.off_b = off_b;
    g.clouds_a = clouds_a, g.clouds_b = clouds_b, g.total_a = total_a, g.total_b = total_b;
    g.members = members, g.targets = targets;
    g.G = (int)G, g.K = (int)K, g.S = (int)S;
    for (int i = 0; i < kVoxMaxSizes; ++i) g.size[i] = i < S ? sizes[i] : 1.0f;
    g.max_group_points = max_group_points;
    g.cap = voxel_capacity(max_group_points);
    const long slots = G * S * g.cap;
    char* base = static_cast<char*>(scratch);
    g.ok = reinterpret_cast<long long*>(base);
    g.keys = reinterpret_cast<unsigned long long*>(base + voxel_flag_bytes(G));
    g.masks = g.keys + slots;
    g.member_out = reinterpret_cast<unsigned long long*>(member_out);
    g.hist_out = reinterpret_cast<unsigned long long*>(hist_out);
    g.status = reinterpret_cast<unsigned long long*>(status);
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(long long), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(member_out, 0, (size_t)G * S * K * 2 * sizeof(long long), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(hist_out, 0, (size_t)G * S * 2 * (K + 1) * sizeof(long long), s);
    if (e != hipSuccess) return e;
    voxel_groups_kernel<<<(unsigned)((G + 255) / 256), 256, 0, s>>>(g);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long clear_blocks = (slots / 2 + 256 * 8 - 1) / (256 * 8);
    voxel_clear_kernel<<<(unsigned)(clear_blocks < 65536 ? clear_blocks : 65536), 256, 0, s>>>(g.keys, g.masks, slots);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long chunks = (max_group_points + kVoxChunk - 1) / kVoxChunk;
    voxel_insert_kernel<<<dim3((unsigned)(chunks < 256 ? chunks : 256), (unsigned)(K + 1), (unsigned)G), kVoxThreads, 0, s>>>(g);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long slot_chunks = (g.cap + kVoxSlotsPerBlock - 1) / kVoxSlotsPerBlock;
    voxel_count_kernel<<<dim3((unsigned)(slot_chunks < 1024 ? slot_chunks : 1024), (unsigned)S, (unsigned)G), kVoxThreads, 0, s>>>(g);
    return hipGetLastError();
}

}  // namespace r2dm
