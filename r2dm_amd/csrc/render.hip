// K14: rendering of the reference's generate.py (utils/render.py): colour maps and the bird's-eye view of a point cloud.
//
//  colorize_kernel        colorize(): look-up table by trunc(clamp(x 256, 0, 255)), uint8 output, bit-identical to the reference.
//  project_kernel         the per-point half of render_point_clouds(): extrinsics, pinhole projection, border mask, depth weight
//                         -> image coordinates (B,N,2) and the four splatted values (B,N,4) = [w c0, w c1, w c2, w].
//  splat_kernel           bilinear_rasterizer(): every point adds value x bilinear weight at its four neighbours.
//  frames_kernel          generate.py's render() fused: one thread per range-image pixel colours the two channels, projects the
//                         pixel's point and splats it; no xyz / colour tensor exists.
//  finish_kernel          accumulators -> fp32 image, or the ratio colour / (weight + 1e-8) of render_point_clouds().
//  surface_normals_kernel estimate_surface_normal(): a 9-point stencil over an LDS tile, bit-exact to the contract of include/r2dm_hip.h.
//  normal_frames_kernel   train.py's log_images view fused: metric depth -> xyz -> normal -> colour, projected and splatted from the same tile.
//
// The splat is a many-to-one sum.  Float atomics would make it depend on the arrival order; here every term is rounded ONCE to a
// 64-bit fixed-point integer (scale 2^s, s from the largest |value| of the call, found on the device) and summed by integer vector
// atomics: integer addition is associative, so the image is the same bits on every call and for every order of the points.  The
// accumulators of a pixel's four channels are 32 contiguous bytes.  Points of a wave with identical coordinates and values (every
// masked pixel of a scan sits on the origin: 10-30 % of a frame) are combined first -- count x term, exact in integers -- and
// added once by one lane.  All arithmetic of the contract is fp32, one rounding per written operation (no contraction).
#include <math.h>

#include "common.h"

namespace r2dm {

#pragma clang fp contract(off)

constexpr int kRenderThreads = 256;
constexpr size_t kRenderHeader = 256;  // scratch: [0] float bits of max|value|, then the accumulators

__device__ __forceinline__ unsigned f2u(float v) { return __builtin_bit_cast(unsigned, v); }

// colorize(): ids = trunc(clamp(x 256, 0, 255)) (NaN -> 0), byte = trunc(clamp(lut 255, 0, 255))
__device__ __forceinline__ int lut_index(float v) {
    const float s = v * 256.0f;
    return s > 0.0f ? (int)(s < 255.0f ? s : 255.0f) : 0;
}
__device__ __forceinline__ float lut_byte(float c) {
    const float s = c * 255.0f;
    return s > 0.0f ? truncf(s < 255.0f ? s : 255.0f) : 0.0f;
}

__global__ __launch_bounds__(kRenderThreads) void colorize_kernel(const float* __restrict__ x, const float* __restrict__ lut,
                                                                  uint8_t* __restrict__ out, long B, long hw) {
    const long i = (long)blockIdx.x * kRenderThreads + threadIdx.x;
    if (i >= B * hw) return;
    const long b = i / hw, p = i - b * hw;
    const float* c = lut + 3 * lut_index(x[i]);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(b * 3 + k) * hw + p] = (uint8_t)lut_byte(c[k]);
}

// ---- fixed-point accumulation -------------------------------------------------------------------
// 2^s with max|value| 2^s < 2^(62 - guard): `guard` bits (>= log2 of the terms a pixel can receive) keep the sum inside int64.
__device__ __forceinline__ double fixed_scale(unsigned max_bits, int guard) {
    const int e = (int)((max_bits >> 23) & 0xff);  // max < 2^(e - 126)
    if (e == 0xff) return 0.0;                     // non-finite values: nothing is accumulated
    if ((max_bits & 0x7fffffffu) == 0) return 1.0;
    return ldexp(1.0, 62 - guard - (e - 126));
}

__global__ __launch_bounds__(kRenderThreads) void absmax_kernel(const float* __restrict__ v, long n, unsigned* __restrict__ max_bits) {
    unsigned m = 0;
    for (long i = (long)blockIdx.x * kRenderThreads + threadIdx.x; i < n; i += (long)gridDim.x * kRenderThreads) {
        const unsigned b = f2u(v[i]) & 0x7fffffffu;  // |v| as bits: ordered like the values (NaN above inf)
        m = b > m ? b : m;
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicMax(max_bits, m);
}

__device__ __forceinline__ void add_fixed(unsigned long long* p, float term, double scale, int count) {
    const long long q = __double2ll_rn((double)term * scale) * (long long)count;
    if (q) atomicAdd(p, (unsigned long long)q);
}

// One point of every lane (valid or not: the whole wave calls this): `acc` the frame's accumulators [H W][4], (h, w) the image
// coordinates [row, column], v the NCH <= 4 values.  utils/render.py:94-139 per point.
template <int NCH>
__device__ __forceinline__ void splat_point(unsigned long long* __restrict__ acc, int H, int W, float h, float w, const float (&v)[4],
                                            double scale, bool valid) {
    valid = valid && isfinite(h) && isfinite(w);  // (the reference adds NaN to a corner pixel; here such a point adds nothing)
    // lanes with the same coordinates and values form a group; its first lane adds count x term
    unsigned long long rem = __ballot(valid);
    const int lane = threadIdx.x & (kWave - 1);
    int count = 0;
    while (rem) {
        const int l = __ffsll((long long)rem) - 1;
        bool same = valid && f2u(h) == (unsigned)__shfl((int)f2u(h), l) && f2u(w) == (unsigned)__shfl((int)f2u(w), l);
#pragma unroll
        for (int c = 0; c < NCH; ++c) same = same && f2u(v[c]) == (unsigned)__shfl((int)f2u(v[c]), l);
        const unsigned long long m = __ballot(same);
        if (lane == l) count = __popcll(m);
        rem &= ~m;
    }
    if (!count) return;
    const float h_t = floorf(h), w_l = floorf(w);
    const float h_b = h_t + 1.0f, w_r = w_l + 1.0f;
    const float hmax = (float)(H - 1), wmax = (float)(W - 1);
    const float h_ts = fminf(fmaxf(h_t, 0.0f), hmax), h_bs = fminf(fmaxf(h_b, 0.0f), hmax);
    const float w_ls = fminf(fmaxf(w_l, 0.0f), wmax), w_rs = fminf(fmaxf(w_r, 0.0f), wmax);
    const float wh[2] = {(h_b - h) * (h_t == h_ts ? 1.0f : 0.0f), (h - h_t) * (h_b == h_bs ? 1.0f : 0.0f)};
    const float ww[2] = {(w_r - w) * (w_l == w_ls ? 1.0f : 0.0f), (w - w_l) * (w_r == w_rs ? 1.0f : 0.0f)};
    const long row[2] = {(long)h_ts, (long)h_bs}, col[2] = {(long)w_ls, (long)w_rs};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float bw = wh[a] * ww[b];
            bw = bw * (bw >= 1e-3f ? 1.0f : 0.0f);
            if (bw == 0.0f) continue;
            unsigned long long* p = acc + (row[a] * W + col[b]) * 4;
#pragma unroll
            for (int c = 0; c < NCH; ++c) add_fixed(p + c, v[c] * bw, scale, count);
        }
}

// bilinear_rasterizer on channels [4 g, 4 g + 4) of values (B,N,C); acc [B][G][H W][4]
__global__ __launch_bounds__(kRenderThreads) void splat_kernel(const float* __restrict__ coords, const float* __restrict__ values,
                                                               unsigned long long* __restrict__ acc, const unsigned* __restrict__ max_bits,
                                                               long N, int C, int H, int W, int guard) {
    const long i = (long)blockIdx.x * kRenderThreads + threadIdx.x;
    const int g = blockIdx.y, G = gridDim.y, b = blockIdx.z;
    const bool valid = i < N;
    float h = 0.f, w = 0.f, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float* c = coords + ((long)b * N + i) * 2;
        h = c[0];
        w = c[1];
        const float* s = values + ((long)b * N + i) * C + 4 * g;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * g + k < C) v[k] = s[k];
    }
    splat_point<4>(acc + ((long)b * G + g) * (long)H * W * 4, H, W, h, w, v, fixed_scale(*max_bits, guard), valid);
}

// RATIO 0: out (B,C,H,W) = the sums; RATIO 1 (C = 4): out (B,3,H,W) = sum_c / (sum_3 + 1e-8); RATIO 2: 1 - that
template <int RATIO>
__global__ __launch_bounds__(kRenderThreads) void finish_kernel(const unsigned long long* __restrict__ acc, const unsigned* __restrict__ max_bits,
                                                                float* __restrict__ out, long hw, int C, int guard, double fixed) {
    const long p = (long)blockIdx.x * kRenderThreads + threadIdx.x;
    if (p >= hw) return;
    const int g = blockIdx.y, G = gridDim.y, b = blockIdx.z;
    const double scale = max_bits ? fixed_scale(*max_bits, guard) : fixed;
    const double inv = scale > 0.0 ? 1.0 / scale : 0.0;  // (a power of two: exact)
    const ulonglong2* a = reinterpret_cast<const ulonglong2*>(acc + (((long)b * G + g) * hw + p) * 4);
    const ulonglong2 lo = a[0], hi = a[1];
    const float s[4] = {(float)((double)(long long)lo.x * inv), (float)((double)(long long)lo.y * inv), (float)((double)(long long)hi.x * inv),
                        (float)((double)(long long)hi.y * inv)};
    if (RATIO == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * g + k < C) out[((long)b * C + 4 * g + k) * hw + p] = s[k];
    } else {
        const float den = s[3] + 1e-8f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float r = s[k] / den;
            out[((long)b * 3 + k) * hw + p] = RATIO == 2 ? 1.0f - r : r;
        }
    }
}

// ---- render_point_clouds: the per-point half (utils/render.py:40-77) -------------------------------
struct View {
    float R[9], t[3], focal, size;  // p' = p R + t (row vector), K = diag(f, f, 1) with cx = cy = 0.5
};

// point (x, y, z) -> image coordinates (u, v) [row, column], depth weight, border mask
__device__ __forceinline__ void project_point(const View& V, float x, float y, float z, float& u, float& v, float& weight, float& mask) {
    z = -z;
    const float px = (x * V.R[0] + y * V.R[3] + z * V.R[6]) + V.t[0];
    const float py = (x * V.R[1] + y * V.R[4] + z * V.R[7]) + V.t[1];
    const float pz = (x * V.R[2] + y * V.R[5] + z * V.R[8]) + V.t[2];
    const float s = fabsf(pz) > 1e-8f ? 1.0f / (pz + 1e-8f) : 1.0f;  // kornia's convert_points_from_homogeneous
    u = ((s * px) * V.focal + 0.5f) * V.size;
    v = ((s * py) * V.focal + 0.5f) * V.size;
    const float hi = V.size - 1.0f;
    mask = (0.0f < u && u < hi && 0.0f < v && v < hi) ? 1.0f : 0.0f;
    u = V.size - u;
    v = V.size - v;
    const float depth = sqrtf((px * px + py * py) + pz * pz);
    weight = (1.0f / expf(3.0f * depth)) * (depth > 1e-8f ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(kRenderThreads) void project_kernel(const float* __restrict__ points, const float* __restrict__ colors, View V,
                                                                 float* __restrict__ uv, float* __restrict__ vals, long n) {
    const long i = (long)blockIdx.x * kRenderThreads + threadIdx.x;
    if (i >= n) return;
    float u, v, w, m;
    project_point(V, points[3 * i], points[3 * i + 1], points[3 * i + 2], u, v, w, m);
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
#pragma unroll
    for (int k = 0; k < 3; ++k) vals[4 * i + k] = w * ((colors ? colors[3 * i + k] : 1.0f) * m);
    vals[4 * i + 3] = w;
}

// ---- generate.py:44-59 fused --------------------------------------------------------------------
struct FrameParams {
    const float* x;        // (N,2,H,W): depth / max_depth and reflectance, both in [0,1]
    const float* trig;     // (4,H,W): cos(elevation), sin(elevation), cos(azimuth), sin(azimuth)
    const float* turbo;    // (256,3)
    const float* viridis;  // (256,3)
    float* img;            // (N,3,2H,W)
    long hw;
    int size;
    float min_depth, max_depth, z_min, z_range;
    View V;
};

__global__ __launch_bounds__(kRenderThreads) void frames_kernel(FrameParams P, unsigned long long* __restrict__ acc, long frame0, double scale) {
    const long i = (long)blockIdx.x * kRenderThreads + threadIdx.x;
    const long f = blockIdx.y, n = frame0 + f;
    const bool valid = i < P.hw;
    float u = 0.f, v = 0.f, vals[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float d = P.x[(n * 2) * P.hw + i], r = P.x[(n * 2 + 1) * P.hw + i];
        const float* cd = P.turbo + 3 * lut_index(d);
        const float* cr = P.turbo + 3 * lut_index(r);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float* o = P.img + (n * 3 + k) * 2 * P.hw + i;
            o[0] = lut_byte(cd[k]) / 255.0f;
            o[P.hw] = lut_byte(cr[k]) / 255.0f;
        }
        // LiDARUtility.to_xyz with its depth window, then / max_depth
        const float metric = d * P.max_depth;
        const float m = (metric > P.min_depth && metric < P.max_depth) ? 1.0f : 0.0f;
        const float cp = P.trig[i], sp = P.trig[P.hw + i], ct = P.trig[2 * P.hw + i], st = P.trig[3 * P.hw + i];
        const float x = (((metric * cp) * ct) * m) / P.max_depth;
        const float y = (((metric * cp) * st) * m) / P.max_depth;
        const float z = ((metric * sp) * m) / P.max_depth;
        const float zc = fminf(fmaxf((z - P.z_min) / P.z_range, 0.0f), 1.0f);
        const float* cz = P.viridis + 3 * lut_index(zc);
        float w, mask;
        project_point(P.V, x, y, z, u, v, w, mask);
#pragma unroll
        for (int k = 0; k < 3; ++k) vals[k] = w * ((1.0f - lut_byte(cz[k]) / 255.0f) * mask);
        vals[3] = w;
    }
    splat_point<4>(acc + f * (long)P.size * P.size * 4, P.size, P.size, u, v, vals, scale, valid);
}

// ---- launchers ----------------------------------------------------------------------------------
static int guard_bits(long points) {  // a pixel receives at most 4 terms per point
    int g = 2;
    while (g < 40 && (1L << (g - 2)) < points) ++g;
    return g;
}

hipError_t launch_colorize(const float* x, const float* lut, uint8_t* out, long B, long hw, hipStream_t s) {
    if (B < 1 || hw < 1) return hipErrorInvalidValue;
    colorize_kernel<<<(unsigned)((B * hw + kRenderThreads - 1) / kRenderThreads), kRenderThreads, 0, s>>>(x, lut, out, B, hw);
    return hipGetLastError();
}

size_t rasterize_scratch_bytes(int B, int C, int H, int W) { return kRenderHeader + (size_t)B * ((C + 3) / 4) * H * W * 4 * sizeof(long long); }

hipError_t launch_rasterize(const float* coords, const float* values, float* out, int B, long N, int C, int H, int W, void* scratch, int ratio,
                            hipStream_t s) {
    if (B < 1 || N < 1 || C < 1 || H < 1 || W < 1 || B > 65535 || (ratio && C != 4)) return hipErrorInvalidValue;
    const int G = (C + 3) / 4, guard = guard_bits(N);
    const long hw = (long)H * W;
    hipError_t e = hipMemsetAsync(scratch, 0, rasterize_scratch_bytes(B, C, H, W), s);
    if (e != hipSuccess) return e;
    unsigned* max_bits = static_cast<unsigned*>(scratch);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + kRenderHeader);
    const long nv = (long)B * N * C;
    long blocks = (nv + kRenderThreads - 1) / kRenderThreads;
    absmax_kernel<<<(unsigned)(blocks < 1024 ? blocks : 1024), kRenderThreads, 0, s>>>(values, nv, max_bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    splat_kernel<<<dim3((unsigned)((N + kRenderThreads - 1) / kRenderThreads), G, B), kRenderThreads, 0, s>>>(coords, values, acc, max_bits, N, C, H, W,
                                                                                                              guard);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 fg((unsigned)((hw + kRenderThreads - 1) / kRenderThreads), G, B);
    if (ratio)
        finish_kernel<1><<<fg, kRenderThreads, 0, s>>>(acc, max_bits, out, hw, C, guard, 0.0);
    else
        finish_kernel<0><<<fg, kRenderThreads, 0, s>>>(acc, max_bits, out, hw, C, guard, 0.0);
    return hipGetLastError();
}

static View make_view(const float* Rt, float focal, int size) {
    View V;
    for (int k = 0; k < 9; ++k) V.R[k] = Rt[k];
    for (int k = 0; k < 3; ++k) V.t[k] = Rt[9 + k];
    V.focal = focal;
    V.size = (float)size;
    return V;
}

hipError_t launch_project_points(const float* points, const float* colors, const float* Rt, float focal, int size, float* uv, float* vals, long n,
                                 hipStream_t s) {
    if (n < 1 || size < 1) return hipErrorInvalidValue;
    project_kernel<<<(unsigned)((n + kRenderThreads - 1) / kRenderThreads), kRenderThreads, 0, s>>>(points, colors, make_view(Rt, focal, size), uv, vals, n);
    return hipGetLastError();
}

size_t render_frames_scratch_bytes(int frames, int size) { return (size_t)frames * size * size * 4 * sizeof(long long); }

hipError_t launch_render_frames(const float* x, const float* trig, const float* turbo, const float* viridis, float* img, float* bev, long N, int H, int W,
                                int size, float min_depth, float max_depth, const float* Rt, float focal, void* scratch, size_t scratch_bytes,
                                hipStream_t s) {
    const long chunk = (long)(scratch_bytes / render_frames_scratch_bytes(1, size));
    if (N < 1 || H < 1 || W < 1 || size < 1 || chunk < 1) return hipErrorInvalidValue;
    FrameParams P;
    P.x = x, P.trig = trig, P.turbo = turbo, P.viridis = viridis, P.img = img;
    P.hw = (long)H * W;
    P.size = size;
    P.min_depth = min_depth, P.max_depth = max_depth;
    // generate.py:49-50: z_min, z_max = -2 / max_depth, 0.5 / max_depth in double, each scalar then enters an fp32 tensor operation
    const double z_min = -2.0 / (double)max_depth, z_max = 0.5 / (double)max_depth;
    P.z_min = (float)z_min;
    P.z_range = (float)(z_max - z_min);
    P.V = make_view(Rt, focal, size);
    // every value is weight x (1 - colour) x mask <= 1: a fixed scale, no pre-pass
    const int guard = guard_bits(P.hw);
    const double scale = ldexp(1.0, 62 - guard - 1);
    unsigned long long* acc = static_cast<unsigned long long*>(scratch);
    const long spx = (long)size * size;
    for (long f0 = 0; f0 < N; f0 += chunk) {
        const long nf = N - f0 < chunk ? N - f0 : chunk;
        for (long g0 = 0; g0 < nf; g0 += 32768) {  // (grid limits)
            const long ng = nf - g0 < 32768 ? nf - g0 : 32768;
            hipError_t e = hipMemsetAsync(acc + g0 * spx * 4, 0, render_frames_scratch_bytes((int)ng, size), s);
            if (e != hipSuccess) return e;
            frames_kernel<<<dim3((unsigned)((P.hw + kRenderThreads - 1) / kRenderThreads), (unsigned)ng), kRenderThreads, 0, s>>>(P, acc + g0 * spx * 4,
                                                                                                                                  f0 + g0, scale);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            finish_kernel<2><<<dim3((unsigned)((spx + kRenderThreads - 1) / kRenderThreads), 1, (unsigned)ng), kRenderThreads, 0, s>>>(
                acc + g0 * spx * 4, nullptr, bev + (f0 + g0) * 3 * spx, spx, 4, guard, scale);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// ---- estimate_surface_normal (utils/render.py:145-236) and train.py:227-239 fused -----------------
// A block owns a 4 x 64 pixel tile, one pixel per thread (a wave is one row of the tile).  The tile and its halo of d rows and d columns are
// staged into three LDS planes, the replicate clamp of the rows and the wrap of the columns applied there, once; every thread then reads its
// anchor and eight neighbours from LDS.  No atomics, no scratch memory: a pixel's normal is a function of its 9 input points.
constexpr int kNormalTileH = 4, kNormalTileW = 64, kNormalMaxD = 8;
static_assert(kNormalTileH * kNormalTileW == kRenderThreads && kNormalTileW == kWave, "one pixel per thread, one tile row per wave");

struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ Vec3 sub3(const Vec3& p, const Vec3& a) { return {p.x - a.x, p.y - a.y, p.z - a.z}; }
__device__ __forceinline__ float norm3(const Vec3& v) { return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z); }
__device__ __forceinline__ Vec3 cross3(const Vec3& u, const Vec3& v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }

// The block's tile: flat block index -> (image, first row, first column)
struct NormalTile {
    long image;
    int row0, col0;
};
__device__ __forceinline__ NormalTile normal_tile(int H, int W) {
    const int tw = (W + kNormalTileW - 1) / kNormalTileW, th = (H + kNormalTileH - 1) / kNormalTileH;
    const long t = blockIdx.x;
    const long b = t / ((long)th * tw);
    const int r = (int)(t - b * th * tw);
    return {b, (r / tw) * kNormalTileH, (r % tw) * kNormalTileW};
}

// Stage the tile and its halo: `point(row, col)` gives the point of an image pixel; planes [3][rows][cols] with rows = 4 + 2d, cols = 64 + 2d
template <class Point>
__device__ __forceinline__ void stage_normal_tile(float* __restrict__ lds, const NormalTile& T, int H, int W, int d, Point point) {
    const int rows = kNormalTileH + 2 * d, cols = kNormalTileW + 2 * d, plane = rows * cols;
    for (int e = threadIdx.x; e < plane; e += kRenderThreads) {
        const int i = e / cols, j = e - i * cols;
        int row = T.row0 - d + i;
        row = row < 0 ? 0 : (row > H - 1 ? H - 1 : row);
        int col = (T.col0 - d + j) % W;  // (a tile may overhang the image by up to 63 columns: a full modulo)
        col = col < 0 ? col + W : col;
        const Vec3 p = point(row, col);
        lds[e] = p.x;
        lds[plane + e] = p.y;
        lds[2 * plane + e] = p.z;
    }
    __syncthreads();
}

// The normal of the thread's pixel from the staged planes; `a` receives its own point
__device__ __forceinline__ Vec3 normal_from_tile(const float* __restrict__ lds, int d, int mode, Vec3& a) {
    const int cols = kNormalTileW + 2 * d, plane = (kNormalTileH + 2 * d) * cols;
    const int ty = threadIdx.x / kNormalTileW, tx = threadIdx.x % kNormalTileW;
    const int c = (ty + d) * cols + tx + d;
    auto at = [&](int e) { return Vec3{lds[e], lds[plane + e], lds[2 * plane + e]}; };
    a = at(c);
    const int up = -d * cols, down = d * cols;
    // k = 0 .. 7: (-d,0) (-d,d) (0,d) (d,d) (d,0) (d,-d) (0,-d) (-d,-d)
    const Vec3 V[8] = {sub3(at(c + up), a),       sub3(at(c + up + d), a),   sub3(at(c + d), a), sub3(at(c + down + d), a),
                       sub3(at(c + down), a),     sub3(at(c + down - d), a), sub3(at(c - d), a), sub3(at(c + up - d), a)};
    Vec3 n;
    if (mode == 0) {
        float len[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) len[k] = norm3(V[k]);
        float best = len[0] + len[2];
        Vec3 u = V[0], v = V[2];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const float dist = len[k] + len[(k + 2) % 8];
            if (dist < best) best = dist, u = V[k], v = V[(k + 2) % 8];  // (strictly smaller: the lowest k keeps a tie)
        }
        n = cross3(u, v);
    } else {
        n = cross3(V[0], V[2]);
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const Vec3 ck = cross3(V[k], V[(k + 2) % 8]);
            n = {n.x + ck.x, n.y + ck.y, n.z + ck.z};
        }
        n = {n.x / 8.0f, n.y / 8.0f, n.z / 8.0f};
    }
    const float den = norm3(n) + 1e-8f;
    return {n.x / den, n.y / den, n.z / den};
}

__global__ __launch_bounds__(kRenderThreads) void surface_normals_kernel(const float* __restrict__ xyz, float* __restrict__ normals, int H, int W, int d,
                                                                         int mode) {
    extern __shared__ float normal_lds[];
    const NormalTile T = normal_tile(H, W);
    const long hw = (long)H * W;
    const float* src = xyz + T.image * 3 * hw;
    stage_normal_tile(normal_lds, T, H, W, d, [&](int row, int col) {
        const long p = (long)row * W + col;
        return Vec3{src[p], src[hw + p], src[2 * hw + p]};
    });
    const int h = T.row0 + threadIdx.x / kNormalTileW, w = T.col0 + threadIdx.x % kNormalTileW;
    if (h >= H || w >= W) return;
    Vec3 a;
    const Vec3 n = normal_from_tile(normal_lds, d, mode, a);
    float* o = normals + T.image * 3 * hw + (long)h * W + w;
    o[0] = n.x;
    o[hw] = n.y;
    o[2 * hw] = n.z;
}

struct NormalFrameParams {
    const float* metric;  // (N,1,H,W): depth in metres
    const float* trig;    // (4,H,W)
    float* colors;        // (N,3,H,W) or nullptr
    int H, W, size, d, mode;
    float min_depth, max_depth;
    View V;
};

__global__ __launch_bounds__(kRenderThreads) void normal_frames_kernel(NormalFrameParams P, unsigned long long* __restrict__ acc, long frame0,
                                                                       double scale) {
    extern __shared__ float normal_lds[];
    const NormalTile T = normal_tile(P.H, P.W);  // (image: the frame inside this launch)
    const long hw = (long)P.H * P.W, n = frame0 + T.image;
    const float* src = P.metric + n * hw;
    stage_normal_tile(normal_lds, T, P.H, P.W, P.d, [&](int row, int col) {
        const long p = (long)row * P.W + col;
        const float metric = src[p];
        const float m = (metric > P.min_depth && metric < P.max_depth) ? 1.0f : 0.0f;
        const float cp = P.trig[p], sp = P.trig[hw + p], ct = P.trig[2 * hw + p], st = P.trig[3 * hw + p];
        // LiDARUtility.to_xyz (its own mask), then / max_depth * mask
        return Vec3{((((metric * cp) * ct) * m) / P.max_depth) * m, ((((metric * cp) * st) * m) / P.max_depth) * m,
                    (((metric * sp) * m) / P.max_depth) * m};
    });
    const int h = T.row0 + threadIdx.x / kNormalTileW, w = T.col0 + threadIdx.x % kNormalTileW;
    bool valid = h < P.H && w < P.W;
    float u = 0.f, v = 0.f, vals[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        Vec3 a;
        const Vec3 nr = normal_from_tile(normal_lds, P.d, P.mode, a);
        const float c[3] = {(-nr.x + 1.0f) / 2.0f, (-nr.y + 1.0f) / 2.0f, (-nr.z + 1.0f) / 2.0f};
        if (P.colors) {
            float* o = P.colors + n * 3 * hw + (long)h * P.W + w;
            o[0] = c[0];
            o[hw] = c[1];
            o[2 * hw] = c[2];
        }
        float weight, mask;
        project_point(P.V, a.x, a.y, a.z, u, v, weight, mask);
#pragma unroll
        for (int k = 0; k < 3; ++k) vals[k] = weight * (c[k] * mask);
        vals[3] = weight;
        valid = isfinite(vals[0]) && isfinite(vals[1]) && isfinite(vals[2]) && isfinite(vals[3]);
    }
    splat_point<4>(acc + T.image * (long)P.size * P.size * 4, P.size, P.size, u, v, vals, scale, valid);
}

static long normal_tiles(int H, int W) { return (long)((H + kNormalTileH - 1) / kNormalTileH) * ((W + kNormalTileW - 1) / kNormalTileW); }
static size_t normal_lds_bytes(int d) { return (size_t)3 * (kNormalTileH + 2 * d) * (kNormalTileW + 2 * d) * sizeof(float); }

const char* surface_normals_error(long B, int H, int W, int d, int mode) {
    if (B < 1 || H < 1 || W < 1) return "empty batch or image";
    if (d < 1 || d > kNormalMaxD) return "the neighbour distance d must be in [1, 8]";
    if (d > W) return "the neighbour distance d must not exceed the width";
    if (mode != 0 && mode != 1) return "mode must be 0 (closest) or 1 (mean)";
    if (normal_tiles(H, W) > 0x7fffffffL / B) return "2^31 or more tiles of 4 x 64 pixels over the batch";
    return nullptr;
}

hipError_t launch_surface_normals(const float* xyz, float* normals, int B, int H, int W, int d, int mode, hipStream_t s) {
    if (surface_normals_error(B, H, W, d, mode)) return hipErrorInvalidValue;
    surface_normals_kernel<<<(unsigned)(normal_tiles(H, W) * B), kRenderThreads, normal_lds_bytes(d), s>>>(xyz, normals, H, W, d, mode);
    return hipGetLastError();
}

hipError_t launch_normal_frames(const float* metric, const float* trig, float* colors, float* bev, long N, int H, int W, int size, float min_depth,
                                float max_depth, int d, int mode, const float* Rt, float focal, void* scratch, size_t scratch_bytes, hipStream_t s) {
    const long chunk = (long)(scratch_bytes / render_frames_scratch_bytes(1, size));
    if (N < 1 || size < 1 || chunk < 1 || surface_normals_error(1, H, W, d, mode)) return hipErrorInvalidValue;
    NormalFrameParams P;
    P.metric = metric, P.trig = trig, P.colors = colors;
    P.H = H, P.W = W, P.size = size, P.d = d, P.mode = mode;
    P.min_depth = min_depth, P.max_depth = max_depth;
    P.V = make_view(Rt, focal, size);
    // every value is weight x colour x mask with weight <= 1 and colour = (1 - n) / 2 < 2: a fixed scale, no pre-pass
    const long hw = (long)H * W, tiles = normal_tiles(H, W), spx = (long)size * size;
    const int guard = guard_bits(hw);
    const double scale = ldexp(1.0, 62 - guard - 1);
    unsigned long long* acc = static_cast<unsigned long long*>(scratch);
    long per_launch = 0x7fffffffL / tiles;  // (grid limit)
    per_launch = per_launch < chunk ? per_launch : chunk;
    per_launch = per_launch < 32768 ? per_launch : 32768;
    for (long f0 = 0; f0 < N; f0 += per_launch) {
        const long nf = N - f0 < per_launch ? N - f0 : per_launch;
        hipError_t e = hipMemsetAsync(acc, 0, render_frames_scratch_bytes((int)nf, size), s);
        if (e != hipSuccess) return e;
        normal_frames_kernel<<<(unsigned)(tiles * nf), kRenderThreads, normal_lds_bytes(d), s>>>(P, acc, f0, scale);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        finish_kernel<1><<<dim3((unsigned)((spx + kRenderThreads - 1) / kRenderThreads), 1, (unsigned)nf), kRenderThreads, 0, s>>>(acc, nullptr,
                                                                                                                                  bev + f0 * 3 * spx, spx, 4, guard, scale);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace r2dm
