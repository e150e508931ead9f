// C ABI of the stand-alone operators (include/r2dm_hip.h): sampler steps, LiDAR post-processing, BEV metrics, rendering, projection and point-cloud
// export.  Each entry validates its arguments and enqueues the operator's kernels (posterior / metrics / render / projection / pointcloud .hip).
#include <cmath>
#include <initializer_list>

#include "engine.h"

using namespace r2dm;

extern "C" {

int r2dm_posterior_step(const float* x_t, const float* pred, const float* noise, const float* coef, float* x_s,
                        int32_t B, int64_t per_sample, int32_t mode, int32_t objective, float clip, void* stream) {
    if (!x_t || !pred || !coef || !x_s) return fail(1, "null argument");
    PosteriorParams p{x_t, pred, noise, coef, x_s, B, per_sample, mode, objective, clip};
    HIP_TRY(launch_posterior(p, (hipStream_t)stream));
    return 0;
}

int r2dm_cache_store(const void* fresh, void* cached, int32_t B, int64_t n_per_sample, int32_t f16, double* partial, double* sums, void* stream) {
    if (!fresh || !cached || !partial || !sums) return fail(1, "cache_store: null argument");
    if (B < 1 || B > 65535) return fail(1, "cache_store: batch must be in [1, 65535], got %d", B);
    if (n_per_sample < 1 || n_per_sample > (1LL << 40) / B) return fail(1, "cache_store: n_per_sample (got %lld) must be in [1, 2^40 / batch]", (long long)n_per_sample);
    if (f16 != 0 && f16 != 1) return fail(1, "cache_store: f16 must be 0 (fp32 values) or 1 (fp16 values), got %d", f16);
    if (fresh == cached) return fail(1, "cache_store: fresh and cached are the same tensor");
    if ((((uintptr_t)fresh | (uintptr_t)cached) & 15) || (((uintptr_t)partial | (uintptr_t)sums) & 7))
        return fail(1, "cache_store: the tensors must be 16-byte aligned, partial and sums 8-byte aligned");
    HIP_TRY(launch_cache_store(fresh, cached, B, (long)n_per_sample, f16, partial, sums, (hipStream_t)stream));
    return 0;
}

// What r2dm_posterior_step_known, r2dm_dpm_step and r2dm_dpm_step_known refuse alike, `name` in front of every message.  `need`: the operands that
// may not be null (`nullable`: the message's word on the rest); `quads`: every tensor the kernel reads or writes as 16-byte quads, absent ones null.  The geometry is
// per_sample in `channels` planes of whole quads under a mask of 1 or `channels` planes (one channel: whole quads, nothing more).  x0 given: the DPM
// entries' two outputs may not alias an input or each other, only x0 may be x0_prev's buffer.
static int step_refused(const char* name, std::initializer_list<const void*> need, const char* nullable, std::initializer_list<const void*> quads,
                        const float* known, const float* mask, const float* coef, int32_t B, int64_t per_sample, int32_t channels, int32_t mask_channels,
                        int32_t objective, const float* x0_prev = nullptr, const float* x_s = nullptr, const float* x0 = nullptr) {
    for (const void* q : need)
        if (!q) return fail(1, "%s: null argument%s", name, nullable);
    if (!known != !mask) return fail(1, "%s: known and mask are given together or not at all (null argument)", name);
    if (objective < 0 || objective > 2) return fail(1, "%s: objective must be 0 (eps), 1 (v) or 2 (x_0), got %d", name, objective);
    if (B < 1 || B > 65535) return fail(1, "%s: batch must be in [1, 65535], got %d", name, B);
    if (per_sample < 4 || per_sample > (1LL << 40) / B || per_sample % 4)
        return fail(1, "%s: per_sample (got %lld) must be a multiple of 4 in [4, 2^40 / batch]", name, (long long)per_sample);
    if (channels < 1 || per_sample % channels) return fail(1, "%s: per_sample (got %lld) must divide into %d channels", name, (long long)per_sample, channels);
    if ((per_sample / channels) % 4)
        return fail(1, "%s: the plane per_sample / channels (got %lld) must be a multiple of 4", name, (long long)(per_sample / channels));
    if (mask_channels != 1 && mask_channels != channels) return fail(1, "%s: mask_channels must be 1 or %d, got %d", name, channels, mask_channels);
    uintptr_t bits = 0;
    for (const void* q : quads) bits |= (uintptr_t)q;
    if ((bits & 15) || ((uintptr_t)coef & 3)) return fail(1, "%s: the tensors must be 16-byte aligned, coef 4-byte aligned", name);
    if (x0) {  // each output stands once among the operands, x0 twice where it is x0_prev
        int n_s = 0, n_0 = 0;
        for (const void* q : quads) n_s += q == x_s, n_0 += q == x0;
        if (n_s != 1 || n_0 != 1 + (x0 == x0_prev))
            return fail(1, "%s: an output may not alias an input or the other output (only x0 may be x0_prev's buffer)", name);
    }
    return 0;
}

int r2dm_posterior_step_known(const float* x_t, const float* pred, const float* noise, const float* known, const float* mask,
                              const float* coef, float* x_s, int32_t B, int64_t per_sample, int32_t channels, int32_t mask_channels,
                              int32_t mode, int32_t objective, float clip, void* stream) {
    if (step_refused("posterior_step_known", {x_t, pred, noise, known, mask, coef, x_s}, "", {x_t, pred, noise, known, mask, x_s}, known, mask, coef,
                     B, per_sample, channels, mask_channels, objective))
        return 1;
    if (mode < 0 || mode > 1) return fail(1, "posterior_step_known: mode must be 0 (continuous DDPM) or 1 (continuous DDIM), got %d", mode);
    PosteriorParams p{x_t, pred, noise, coef, x_s, B, per_sample, mode, objective, clip};
    HIP_TRY(launch_posterior_known(p, known, mask, channels, mask_channels, (hipStream_t)stream));
    return 0;
}

int r2dm_dpm_step(const float* x_t, const float* pred, const float* x0_prev, const float* coef, float* x_s, float* x0, int32_t B,
                  int64_t per_sample, int32_t objective, float clip, void* stream) {
    if (step_refused("dpm_step", {x_t, pred, coef, x_s, x0}, " (only x0_prev may be null)", {x_t, pred, x0_prev, x_s, x0}, nullptr, nullptr, coef, B, per_sample, 1, 1, objective,
                     x0_prev, x_s, x0))
        return 1;
    DpmParams p{x_t, pred, x0_prev, coef, x_s, x0, B, per_sample, objective, clip};
    HIP_TRY(launch_dpm_step(p, (hipStream_t)stream));
    return 0;
}

int r2dm_dpm_step_known(const float* x_t, const float* pred, const float* x0_prev, const float* noise, const float* known, const float* mask,
                        const float* coef, float* x_s, float* x0, int32_t B, int64_t per_sample, int32_t channels, int32_t mask_channels,
                        int32_t objective, float clip, void* stream) {
    if (step_refused("dpm_step_known", {x_t, pred, coef, x_s, x0}, " (only x0_prev, noise and the pair known, mask may be null)", {x_t, pred, x0_prev, noise, known, mask, x_s, x0},
                     known, mask, coef, B, per_sample, channels, mask_channels, objective, x0_prev, x_s, x0))
        return 1;
    DpmParams p{x_t, pred, x0_prev, coef, x_s, x0, B, per_sample, objective, clip};
    HIP_TRY(launch_dpm_step_known(p, noise, known, mask, channels, mask_channels, (hipStream_t)stream));
    return 0;
}

int r2dm_repaint_blend(const float* known, const float* noise, const float* unknown, const float* mask, const float* coef,
                       float* out, int32_t B, int64_t per_sample, int32_t channels, int32_t mask_channels, void* stream) {
    if (!known || !noise || !unknown || !mask || !coef || !out) return fail(1, "null argument");
    HIP_TRY(launch_repaint_blend(known, noise, unknown, mask, coef, out, B, per_sample, channels, mask_channels,
                                 (hipStream_t)stream));
    return 0;
}

int r2dm_q_step(const float* x_s, const float* noise, const float* coef, float* x_t, int32_t B, int64_t per_sample,
                void* stream) {
    if (!x_s || !noise || !coef || !x_t) return fail(1, "null argument");
    HIP_TRY(launch_q_step(x_s, noise, coef, x_t, B, per_sample, (hipStream_t)stream));
    return 0;
}

static bool loss_geometry_ok(int32_t B, int32_t C, int64_t plane) {
    return B >= 1 && B <= 65535 && C >= 1 && C <= 65535 && plane >= 1 && plane <= (1LL << 40) / C / B;
}

size_t r2dm_diffusion_loss_scratch_bytes(int32_t B, int32_t C, int64_t plane) {
    return loss_geometry_ok(B, C, plane) ? diffusion_loss_scratch_bytes(B, C, plane) : 0;
}

int r2dm_diffusion_loss(const float* prediction, const float* x_0, const float* noise, const float* mask, int32_t mask_channels,
                        const float* coef, int32_t objective, int32_t criterion, int32_t B, int32_t C, int64_t plane, void* scratch,
                        double* num, double* den, void* stream) {
    if (!prediction || !x_0 || !noise || !scratch || !num || !den) return fail(1, "null argument");
    if (objective < 0 || objective > 2) return fail(1, "diffusion_loss: objective must be 0 (eps), 1 (v) or 2 (x_0), got %d", objective);
    if (criterion < 0 || criterion > 2) return fail(1, "diffusion_loss: criterion must be 0 (l2), 1 (l1) or 2 (huber), got %d", criterion);
    if (objective == 1 && !coef) return fail(1, "diffusion_loss: the v objective needs coef (null argument)");
    if (!loss_geometry_ok(B, C, plane)) return fail(1, "diffusion_loss: batch and channels must be in [1, 65535], the tensors 1 to 2^40 elements");
    if (mask && mask_channels != 1 && mask_channels != C) return fail(1, "diffusion_loss: mask_channels must be 1 or %d, got %d", C, mask_channels);
    const uintptr_t a = plane % 4 == 0 ? 15 : 3;  // a plane that is a multiple of 4 is read as quads
    if (((uintptr_t)prediction | (uintptr_t)x_0 | (uintptr_t)noise | (uintptr_t)mask) & a)
        return fail(1, "diffusion_loss: prediction, x_0, noise and mask must be %d-byte aligned for a plane of %lld elements", (int)a + 1, (long long)plane);
    if (((uintptr_t)coef & 3) || (((uintptr_t)scratch | (uintptr_t)num | (uintptr_t)den) & 7))
        return fail(1, "diffusion_loss: coef must be 4-byte aligned; scratch, num and den 8-byte aligned");
    HIP_TRY(launch_diffusion_loss(prediction, x_0, noise, mask, mask_channels, coef, objective, criterion, B, C, plane, scratch, num, den,
                                  (hipStream_t)stream));
    return 0;
}

static bool latent_geometry_ok(int32_t B, int64_t per_sample) {
    return B >= 1 && B <= 65535 && per_sample >= 4 && per_sample % 4 == 0 && per_sample <= (1LL << 40) / B;
}

int r2dm_ddim_transfer(const float* x_t, const float* prediction, const float* coef, float* x_u, int32_t B, int64_t per_sample,
                       int32_t objective, void* stream) {
    if (!x_t || !prediction || !coef || !x_u) return fail(1, "null argument");
    if (objective < 0 || objective > 2) return fail(1, "ddim_transfer: objective must be 0 (eps), 1 (v) or 2 (x_0), got %d", objective);
    if (!latent_geometry_ok(B, per_sample))
        return fail(1, "ddim_transfer: batch must be in [1, 65535], per_sample a multiple of 4 (got %lld), the tensors at most 2^40 elements", (long long)per_sample);
    if ((((uintptr_t)x_t | (uintptr_t)prediction | (uintptr_t)x_u) & 15) || ((uintptr_t)coef & 3))
        return fail(1, "ddim_transfer: x_t, prediction and x_u must be 16-byte aligned, coef 4-byte aligned");
    HIP_TRY(launch_ddim_transfer(x_t, prediction, coef, x_u, B, per_sample, objective, (hipStream_t)stream));
    return 0;
}

size_t r2dm_slerp_scratch_bytes(int32_t B, int64_t per_sample) {
    return latent_geometry_ok(B, per_sample) ? slerp_scratch_bytes(B, per_sample) : 0;
}

int r2dm_slerp(const float* a, const float* b, const float* weights, int32_t K, float* out, double* coef64, int32_t B, int64_t per_sample,
               void* scratch, void* stream) {
    if (!a || !b || !weights || !out || !coef64 || !scratch) return fail(1, "null argument");
    if (K < 1 || K > kSlerpMaxWeights) return fail(1, "slerp: the number of weights must be in [1, %d], got %d", kSlerpMaxWeights, K);
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(weights[k])) return fail(1, "slerp: weight %d is not finite", k);
    if (!latent_geometry_ok(B, per_sample) || per_sample > (1LL << 40) / B / K)
        return fail(1, "slerp: batch must be in [1, 65535], per_sample a multiple of 4 (got %lld), the output at most 2^40 elements", (long long)per_sample);
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) || (((uintptr_t)coef64 | (uintptr_t)scratch) & 7))
        return fail(1, "slerp: a, b and out must be 16-byte aligned, coef64 and scratch 8-byte aligned");
    HIP_TRY(launch_slerp(a, b, weights, K, out, coef64, B, per_sample, scratch, (hipStream_t)stream));
    return 0;
}

int r2dm_lidar_postprocess(const float* x, const float* ang, float* out, int32_t B, int32_t H, int32_t W,
                           float min_depth, float max_depth, void* stream) {
    return r2dm_lidar_postprocess_fmt(x, ang, out, B, H, W, min_depth, max_depth, 0, stream);
}

int r2dm_lidar_postprocess_fmt(const float* x, const float* ang, float* out, int32_t B, int32_t H, int32_t W,
                               float min_depth, float max_depth, int32_t depth_format, void* stream) {
    if (!x || !ang || !out) return fail(1, "null argument");
    if (depth_format < 0 || depth_format > 2) return fail(1, "depth_format must be 0 (log_depth), 1 (inverse_depth) or 2 (depth)");
    HIP_TRY(launch_lidar_postprocess(x, ang, out, B, H, W, min_depth, max_depth, (hipStream_t)stream, depth_format));
    return 0;
}

int r2dm_bev_histogram(const float* src, int32_t layout, const float* edges, int32_t* hist, int64_t* sum, int32_t batch,
                       int64_t points, int32_t bins, float min_depth, float max_depth, float image_min_depth,
                       float image_max_depth, void* stream) {
    if (!src || !edges || !hist) return fail(1, "null argument");
    if (layout != 0 && layout != 1) return fail(1, "layout must be 0 ((B,5,H,W) samples) or 1 ((B,N,3) point clouds)");
    if (batch < 1 || points < 1) return fail(1, "empty batch");
    if (bins < 1 || bins > 128) return fail(1, "bins must be in [1, 128] (one histogram per block in LDS), got %d", bins);
    HIP_TRY(launch_bev_histogram(src, layout, edges, hist, sum, batch, points, bins, min_depth, max_depth, image_min_depth,
                                 image_max_depth, (hipStream_t)stream));
    return 0;
}

int r2dm_bev_hist_sum(const void* hist, int32_t is_int32, int64_t* sum, int64_t batch, int64_t cells, void* stream) {
    if (!hist || !sum) return fail(1, "null argument");
    if (batch < 1 || cells < 1) return fail(1, "empty histogram batch");
    HIP_TRY(launch_bev_hist_sum(hist, is_int32, sum, batch, cells, (hipStream_t)stream));
    return 0;
}

size_t r2dm_bev_mmd_scratch_bytes(int32_t np, int32_t nq) { return np < 1 || nq < 1 ? 0 : mmd_scratch_bytes(np, nq); }

int r2dm_bev_mmd(const float* p, const float* q, int32_t np, int32_t nq, int64_t bins, double sigma, void* scratch,
                 size_t scratch_bytes, double* out, void* stream) {
    if (!p || !q || !scratch || !out) return fail(1, "null argument");
    if (np < 1 || nq < 1 || bins < 1) return fail(1, "empty histogram set");
    if (!(sigma > 0.0)) return fail(1, "sigma must be > 0");
    if (scratch_bytes < mmd_scratch_bytes(np, nq)) return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, mmd_scratch_bytes(np, nq));
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_bev_mmd(p, q, np, nq, bins, sigma, scratch, out, (hipStream_t)stream));
    return 0;
}

int r2dm_feature_moments(const float* feats, int64_t rows, int32_t dim, double* mean, double* cov, void* stream) {
    if (!feats || !mean || !cov) return fail(1, "null argument");
    if (rows < 2 || dim < 1) return fail(1, "feature_moments: at least 2 rows and 1 column");
    HIP_TRY(launch_feature_moments(feats, rows, dim, mean, cov, (hipStream_t)stream));
    return 0;
}

size_t r2dm_poly_mmd_scratch_bytes(int32_t subsets, int32_t subset_size) {
    return subsets < 1 || subset_size < 1 ? 0 : poly_mmd_scratch_bytes(subsets, subset_size);
}

int r2dm_poly_mmd(const float* x, const float* y, const int64_t* ix, const int64_t* iy, int32_t subsets, int32_t subset_size, int32_t dim,
                  void* scratch, size_t scratch_bytes, double* out, void* stream) {
    if (!x || !y || !ix || !iy || !scratch || !out) return fail(1, "null argument");
    if (subsets < 1 || subsets > 65535 || subset_size < 1 || dim < 1) return fail(1, "poly_mmd: 1 to 65535 subsets of at least one row");
    if (scratch_bytes < poly_mmd_scratch_bytes(subsets, subset_size))
        return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, poly_mmd_scratch_bytes(subsets, subset_size));
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_poly_mmd(x, y, reinterpret_cast<const long long*>(ix), reinterpret_cast<const long long*>(iy), subsets, subset_size, dim, scratch, out,
                            (hipStream_t)stream));
    return 0;
}

static bool knn_geometry_ok(int64_t m, int64_t n, int32_t dim, int32_t k) {
    return m >= 1 && m <= (1LL << 20) && n >= 1 && n <= (1LL << 20) && dim >= 1 && dim <= 16384 && k >= 0 && k <= 16;
}

size_t r2dm_feature_knn_scratch_bytes(int64_t m, int64_t n, int32_t dim, int32_t k) {
    return knn_geometry_ok(m, n, dim, k) ? feature_knn_scratch_bytes(m, n, k) : 0;
}

int r2dm_feature_knn(const float* x, int64_t m, const float* y, int64_t n, int32_t dim, int32_t same, int32_t k, const double* y_radius2, double* kth2,
                     double* min2, int32_t* argmin, int32_t* count, void* scratch, size_t scratch_bytes, int64_t* status, int32_t* chosen,
                     void* stream) {
    if (!x || !y || !scratch || !status) return fail(1, "feature_knn: null argument");
    if (dim < 1 || dim > 16384) return fail(1, "feature_knn: dim must be in [1, 16384], got %d", dim);
    if (m < 1 || m > (1LL << 20) || n < 1 || n > (1LL << 20))
        return fail(1, "feature_knn: m and n must be in [1, 2^20], got %lld, %lld", (long long)m, (long long)n);
    if (k < 0 || k > 16) return fail(1, "feature_knn: k must be in [0, 16], got %d", k);
    if (same != 0 && same != 1) return fail(1, "feature_knn: same must be 0 or 1");
    if (same && (y != x || m != n)) return fail(1, "feature_knn: same = 1 needs y == x and m == n");
    if (count && !y_radius2) return fail(1, "feature_knn: count needs y_radius2");
    if (kth2 && k < 1) return fail(1, "feature_knn: kth2 needs k >= 1");
    if (n - same < k) return fail(1, "feature_knn: %lld admissible columns, fewer than k = %d", (long long)(n - same), k);
    const uintptr_t al = dim % 4 == 0 ? 15 : 3;  // rows of a multiple of 4 features are read as quads
    if (((uintptr_t)x | (uintptr_t)y) & al) return fail(1, "feature_knn: x and y must be %d-byte aligned for dim = %d", (int)al + 1, dim);
    if (((uintptr_t)kth2 | (uintptr_t)min2 | (uintptr_t)y_radius2 | (uintptr_t)scratch | (uintptr_t)status) & 7)
        return fail(1, "feature_knn: kth2, min2, y_radius2, scratch and status must be 8-byte aligned");
    if (((uintptr_t)argmin | (uintptr_t)count) & 3) return fail(1, "feature_knn: argmin and count must be 4-byte aligned");
    if (scratch_bytes < feature_knn_scratch_bytes(m, n, k))
        return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, feature_knn_scratch_bytes(m, n, k));
    int row_tiles, splits;
    feature_knn_launch_shape(m, n, &row_tiles, &splits);
    HIP_TRY(launch_feature_knn(x, m, y, n, dim, same, k, y_radius2, kth2, min2, argmin, count, scratch, reinterpret_cast<long long*>(status),
                               (hipStream_t)stream));
    if (chosen) chosen[0] = row_tiles, chosen[1] = splits;
    return 0;
}

size_t r2dm_rangenet_packed_bytes(int32_t cout, int32_t cin, int32_t taps) { return rangenet_packed_bytes(cout, cin, taps); }

int r2dm_rangenet_pack(const float* w, int32_t cout, int32_t cin, int32_t taps, void* packed, float* wscale, int32_t* flag, void* stream) {
    if (!w || !packed || !wscale || !flag) return fail(1, "null argument");
    if (!rangenet_packed_bytes(cout, cin, taps)) return fail(1, "rangenet_pack: cout and cin must be positive, taps in [1, 9]");
    if ((uintptr_t)packed & 15) return fail(1, "rangenet_pack: packed must be 16-byte aligned");
    HIP_TRY(launch_rangenet_pack(w, cout, cin, taps, packed, wscale, flag, (hipStream_t)stream));
    return 0;
}

int r2dm_rangenet_conv(const float* in, const float* mask, const float* norm, float min_depth, float max_depth, const void* packed,
                       const float* inv_scale, const float* bias, const float* add, const float* add2, float* out, int32_t batch, int32_t cin,
                       int32_t height, int32_t width, int32_t cout, int32_t kind, float slope, int32_t* flag, void* stream) {
    if (!in || !packed || !inv_scale || !bias || !out || !flag) return fail(1, "null argument");
    if (kind < 0 || kind > 5) return fail(1, "rangenet_conv: kind must be 0 (1x1), 1 (3x3), 2 (3x3 stride (1,2)), 3 / 4 (transposed 1x4, even / odd columns) or 5 (stem)");
    if (batch < 1 || height < 1 || width < 1 || cout < 1) return fail(1, "rangenet_conv: batch, height, width and cout must be positive");
    if (kind == 5 ? (cin != 5 || cout > 32 || !norm) : (cin < 16 || cin % 16))
        return fail(1, "rangenet_conv: cin must be a multiple of 16 (the stem: 5 channels, at most 32 outputs, norm given)");
    if (kind == 2 && width % 2) return fail(1, "rangenet_conv: the stride-(1,2) convolution needs an even width");
    if (in == out || add == out || add2 == out) return fail(1, "rangenet_conv: out must not alias an input");
    if ((uintptr_t)packed & 15) return fail(1, "rangenet_conv: packed must be 16-byte aligned");
    HIP_TRY(launch_rangenet_conv(in, mask, norm, min_depth, max_depth, packed, inv_scale, bias, add, add2, out, batch, cin, height, width, cout, kind,
                                 slope, flag, (hipStream_t)stream));
    return 0;
}

int r2dm_rangenet_argmax(const float* logits, int64_t* labels, int32_t batch, int32_t classes, int64_t pixels, void* stream) {
    if (!logits || !labels) return fail(1, "null argument");
    if (batch < 1 || classes < 1 || pixels < 1) return fail(1, "rangenet_argmax: batch, classes and pixels must be positive");
    HIP_TRY(launch_rangenet_argmax(logits, reinterpret_cast<long long*>(labels), batch, classes, pixels, (hipStream_t)stream));
    return 0;
}

size_t r2dm_pointnet_packed_bytes(int32_t cout, int32_t cin) {
    return cout < 32 || cout % 32 || cin < 16 || cin % 16 ? 0 : (size_t)cout * cin * 4;
}

int r2dm_pointnet_pack(const float* w, int32_t cout, int32_t cin, void* packed, float* wscale, int32_t* flag, void* stream) {
    if (!w || !packed || !wscale || !flag) return fail(1, "null argument");
    if (!r2dm_pointnet_packed_bytes(cout, cin)) return fail(1, "pointnet_pack: cout must be a multiple of 32, cin of 16");
    if ((uintptr_t)packed & 15) return fail(1, "pointnet_pack: packed must be 16-byte aligned");
    HIP_TRY(launch_pointnet_pack(w, cout, cin, packed, wscale, flag, (hipStream_t)stream));
    return 0;
}

size_t r2dm_pointnet_scratch_bytes(int32_t batch) { return batch < 1 || batch > 65535 ? 0 : pointnet_scratch_bytes(batch); }

int r2dm_pointnet_trunk(const float* src, int32_t layout, int32_t batch, int64_t points, const float* trans, float image_min_depth,
                        float image_max_depth, float divisor, const float* w1b, const void* w2_packed, const float* w2_inv_scale, const float* b2,
                        const void* w3_packed, void* scratch, size_t scratch_bytes, int32_t* flag, void* stream) {
    if (!src || !w1b || !w2_packed || !w2_inv_scale || !b2 || !w3_packed || !scratch || !flag) return fail(1, "null argument");
    if (layout < 0 || layout > 2) return fail(1, "layout must be 0 ((B,5,H,W) samples), 1 ((B,N,3) clouds) or 2 ((B,3,N) clouds)");
    if (batch < 1 || batch > 65535 || points < 1) return fail(1, "pointnet_trunk: batch must be in [1, 65535] and a cloud must have a point");
    if (layout == 0 && !(divisor > 0.f)) return fail(1, "pointnet_trunk: divisor must be > 0");
    if (scratch_bytes < pointnet_scratch_bytes(batch)) return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, pointnet_scratch_bytes(batch));
    if (((uintptr_t)w1b | (uintptr_t)w2_packed | (uintptr_t)w3_packed) & 15) return fail(1, "pointnet_trunk: weights must be 16-byte aligned");
    HIP_TRY(launch_pointnet_trunk(src, layout, batch, points, trans, image_min_depth, image_max_depth, divisor, w1b, w2_packed, w2_inv_scale, b2,
                                  w3_packed, scratch, flag, (hipStream_t)stream));
    return 0;
}

int r2dm_pointnet_head(const void* scratch, const float* w3_inv_scale, const float* b3, int32_t stn, const float* fc1_w, const float* fc1_b,
                       const float* fc2_w, const float* fc2_b, const float* fc3_w, const float* fc3_b, int32_t outputs, float* out, int32_t batch,
                       void* stream) {
    if (!scratch || !w3_inv_scale || !b3 || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !fc3_w || !fc3_b || !out) return fail(1, "null argument");
    if (batch < 1 || outputs < 1 || outputs > 16 || (stn && outputs != 9)) return fail(1, "pointnet_head: 1 to 16 outputs (9 for the transformer)");
    HIP_TRY(launch_pointnet_head(scratch, w3_inv_scale, b3, stn, fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b, outputs, out, batch, (hipStream_t)stream));
    return 0;
}

int r2dm_colorize(const float* x, const float* lut, uint8_t* out, int64_t batch, int64_t pixels, void* stream) {
    if (!x || !lut || !out) return fail(1, "null argument");
    if (batch < 1 || pixels < 1) return fail(1, "empty image batch");
    HIP_TRY(launch_colorize(x, lut, out, batch, pixels, (hipStream_t)stream));
    return 0;
}

size_t r2dm_rasterize_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width) {
    return batch < 1 || channels < 1 || height < 1 || width < 1 ? 0 : rasterize_scratch_bytes(batch, channels, height, width);
}

int r2dm_bilinear_rasterize(const float* coords, const float* values, float* out, int32_t batch, int64_t points, int32_t channels, int32_t height,
                            int32_t width, void* scratch, size_t scratch_bytes, int32_t ratio, void* stream) {
    if (!coords || !values || !out || !scratch) return fail(1, "null argument");
    if (batch < 1 || batch > 65535 || points < 1 || channels < 1 || height < 1 || width < 1) return fail(1, "rasterize: empty or oversized batch");
    if (points > (1L << 36)) return fail(1, "rasterize: more than 2^36 points per image");
    if (ratio != 0 && ratio != 1) return fail(1, "ratio must be 0 (sums) or 1 (channels 0-2 over channel 3)");
    if (ratio && channels != 4) return fail(1, "the ratio form takes 4 channels, got %d", channels);
    const size_t need = rasterize_scratch_bytes(batch, channels, height, width);
    if (scratch_bytes < need) return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_rasterize(coords, values, out, batch, points, channels, height, width, scratch, ratio, (hipStream_t)stream));
    return 0;
}

int r2dm_project_points(const float* points, const float* colors, const float* view, float focal_length, int32_t size, float* uv, float* vals,
                        int64_t total_points, void* stream) {
    if (!points || !view || !uv || !vals) return fail(1, "null argument");
    if (total_points < 1 || size < 1) return fail(1, "project_points: empty cloud or image");
    HIP_TRY(launch_project_points(points, colors, view, focal_length, size, uv, vals, total_points, (hipStream_t)stream));
    return 0;
}

size_t r2dm_render_frames_scratch_bytes(int32_t frames, int32_t size) { return frames < 1 || size < 1 ? 0 : render_frames_scratch_bytes(frames, size); }

int r2dm_render_frames(const float* x, const float* trig, const float* turbo, const float* viridis, float* img, float* bev, int64_t frames,
                       int32_t height, int32_t width, int32_t size, float min_depth, float max_depth, const float* view, float focal_length,
                       void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !trig || !turbo || !viridis || !img || !bev || !view || !scratch) return fail(1, "null argument");
    if (frames < 1 || height < 1 || width < 1 || size < 1) return fail(1, "render_frames: empty batch or image");
    if (!(max_depth > 0.f)) return fail(1, "max_depth must be > 0");
    if (scratch_bytes < render_frames_scratch_bytes(1, size))
        return fail(1, "scratch too small: %zu bytes hold no frame of %zu", scratch_bytes, render_frames_scratch_bytes(1, size));
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_render_frames(x, trig, turbo, viridis, img, bev, frames, height, width, size, min_depth, max_depth, view, focal_length, scratch,
                                 scratch_bytes, (hipStream_t)stream));
    return 0;
}

int r2dm_surface_normals(const float* xyz, float* normals, int32_t batch, int32_t height, int32_t width, int32_t d, int32_t mode, void* stream) {
    if (!xyz || !normals) return fail(1, "null argument");
    if (const char* why = surface_normals_error(batch, height, width, d, mode)) return fail(1, "surface_normals: %s", why);
    if ((const void*)xyz == (const void*)normals) return fail(1, "surface_normals: normals must not alias xyz");
    HIP_TRY(launch_surface_normals(xyz, normals, batch, height, width, d, mode, (hipStream_t)stream));
    return 0;
}

size_t r2dm_normal_frames_scratch_bytes(int32_t frames, int32_t size) { return r2dm_render_frames_scratch_bytes(frames, size); }

int r2dm_normal_frames(const float* metric, const float* trig, float* colors, float* bev, int64_t frames, int32_t height, int32_t width, int32_t size,
                       float min_depth, float max_depth, int32_t d, int32_t mode, const float* view, float focal_length, void* scratch,
                       size_t scratch_bytes, void* stream) {
    if (!metric || !trig || !bev || !view || !scratch) return fail(1, "null argument");
    if (frames < 1 || size < 1) return fail(1, "normal_frames: empty batch or image");
    if (const char* why = surface_normals_error(1, height, width, d, mode)) return fail(1, "normal_frames: %s", why);
    if (!(max_depth > 0.f)) return fail(1, "max_depth must be > 0");
    if (scratch_bytes < render_frames_scratch_bytes(1, size))
        return fail(1, "scratch too small: %zu bytes hold no frame of %zu", scratch_bytes, render_frames_scratch_bytes(1, size));
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_normal_frames(metric, trig, colors, bev, frames, height, width, size, min_depth, max_depth, d, mode, view, focal_length, scratch,
                                 scratch_bytes, (hipStream_t)stream));
    return 0;
}

static const char* project_geometry_error(int64_t total, int32_t batch, int32_t H, int32_t W) {
    if (batch < 1 || batch > 65535) return "project: batch must be in [1, 65535]";
    if (H < 1 || W < 1 || (int64_t)batch * H * W >= (1LL << 31)) return "project: the grid must have 1 to 2^31 - 1 cells over the batch";
    if (total < 0 || total >= (1LL << 31)) return "project: 0 to 2^31 - 1 points over the batch";
    return nullptr;
}

size_t r2dm_project_scratch_bytes(int64_t total_points, int32_t batch, int32_t height, int32_t width, int32_t scan_unfolding) {
    return project_geometry_error(total_points, batch, height, width) ? 0 : project_scratch_bytes(total_points, batch, height, width, scan_unfolding);
}

int r2dm_project_scans(const float* points, const int64_t* offsets, float* out, int32_t batch, int32_t height, int32_t width, int32_t out_width,
                       int32_t scan_unfolding, float min_depth, float max_depth, int32_t apply_mask, int32_t layout, void* scratch,
                       size_t scratch_bytes, void* stream) {
    if (!offsets || !out || !scratch) return fail(1, "null argument");
    if (batch < 1 || batch > 65535) return fail(1, "project: batch must be in [1, 65535]");
    if (offsets[0] != 0) return fail(1, "project: offsets[0] must be 0, got %lld", (long long)offsets[0]);
    for (int32_t b = 0; b < batch; ++b)
        if (offsets[b + 1] < offsets[b]) return fail(1, "project: offsets decrease at scan %d (%lld after %lld)", b, (long long)offsets[b + 1], (long long)offsets[b]);
    const int64_t total = offsets[batch];
    if (const char* msg = project_geometry_error(total, batch, height, width)) return fail(1, "%s", msg);
    if (total > 0 && !points) return fail(1, "null argument");
    if ((uintptr_t)points & 15) return fail(1, "project: points must be 16-byte aligned");
    if (out_width < 1 || out_width > width) return fail(1, "project: out_width must be in [1, width], got %d", out_width);
    if (layout != 0 && layout != 1) return fail(1, "layout must be 0 ((B,6,H,W) xyzrdm) or 1 ((B,5,H,W) samples)");
    if ((scan_unfolding != 0 && scan_unfolding != 1) || (apply_mask != 0 && apply_mask != 1)) return fail(1, "project: scan_unfolding and apply_mask are 0 or 1");
    const size_t need = project_scratch_bytes(total, batch, height, width, scan_unfolding);
    if (scratch_bytes < need) return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_project_scans(points, reinterpret_cast<const long long*>(offsets), out, batch, height, width, out_width, scan_unfolding, min_depth,
                                 max_depth, apply_mask, layout, scratch, (hipStream_t)stream));
    return 0;
}

static const char* unproject_geometry_error(int32_t batch, int32_t H, int32_t W) {
    if (batch < 1 || batch > 65535) return "unproject: batch must be in [1, 65535]";
    if (H < 1 || W < 1 || (int64_t)batch * H * W >= (1LL << 31)) return "unproject: the images must have 1 to 2^31 - 1 pixels over the batch";
    return nullptr;
}

size_t r2dm_unproject_scratch_bytes(int32_t batch, int32_t height, int32_t width) {
    return unproject_geometry_error(batch, height, width) ? 0 : unproject_scratch_bytes(batch, height, width);
}

int r2dm_unproject(const float* src, int32_t layout, const float* ray_angles, const int32_t* row_start, float* points, int32_t* index,
                   int64_t* offsets, int32_t batch, int32_t height, int32_t width, float min_depth, float max_depth, int32_t depth_format,
                   float keep_min, float keep_max, void* scratch, size_t scratch_bytes, void* stream) {
    if (!src || !points || !offsets || !scratch) return fail(1, "null argument");
    if (layout != 0 && layout != 1) return fail(1, "layout must be 0 ((B,2,H,W) model samples) or 1 ((B,5,H,W) post-processed samples)");
    if (layout == 0 && !ray_angles) return fail(1, "unproject: layout 0 needs ray_angles (null argument)");
    if (depth_format < 0 || depth_format > 2) return fail(1, "depth_format must be 0 (log_depth), 1 (inverse_depth) or 2 (depth)");
    if (const char* msg = unproject_geometry_error(batch, height, width)) return fail(1, "%s", msg);
    if ((uintptr_t)points & 15) return fail(1, "unproject: points must be 16-byte aligned");
    if ((uintptr_t)offsets & 7) return fail(1, "unproject: offsets must be 8-byte aligned");
    const size_t need = unproject_scratch_bytes(batch, height, width);
    if (scratch_bytes < need) return fail(1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    if ((uintptr_t)scratch & 255) return fail(1, "scratch must be 256-byte aligned");
    HIP_TRY(launch_unproject(src, layout, ray_angles, row_start, points, index, reinterpret_cast<long long*>(offsets), batch, height, width, min_depth,
                             max_depth, depth_format, keep_min, keep_max, scratch, (hipStream_t)stream));
    return 0;
}

int r2dm_knn_vote(const float* depth, const int64_t* label, const float* weight, int64_t* out, int32_t batch, int32_t height, int32_t width,
                  int32_t kh, int32_t kw, int32_t k, int32_t classes, float cutoff, int32_t* flag, void* stream) {
    if (!depth || !label || !weight || !out || !flag) return fail(1, "null argument");
    if (!postproc_window_supported(kh, kw)) return fail(1, "knn_vote: the window sides must be odd and at most 7, got %d x %d", kh, kw);
    if (k < 1 || k > 8 || k > kh * kw) return fail(1, "knn_vote: k must be in [1, min(kh kw, 8)], got %d", k);
    if (classes < 1 || classes > 32) return fail(1, "knn_vote: 1 to 32 classes, got %d", classes);
    if (batch < 1 || batch > 65535 || height < 1 || width < 1 || height > 65535 * 8) return fail(1, "knn_vote: batch must be in [1, 65535], height and width positive");
    if ((const void*)label == (const void*)out) return fail(1, "knn_vote: out must not alias label");
    HIP_TRY(launch_knn_vote(depth, reinterpret_cast<const long long*>(label), weight, reinterpret_cast<long long*>(out), batch, height, width, kh, kw, k,
                            classes, cutoff, flag, (hipStream_t)stream));
    return 0;
}

int r2dm_crf_iter(const float* q_in, const float* unary, const float* xyz, const float* mask, const float* params, float* q_out, int32_t batch,
                  int32_t classes, int32_t height, int32_t width, int32_t kh, int32_t kw, int32_t uniform_beta, void* stream) {
    if (!q_in || !unary || !xyz || !mask || !params || !q_out) return fail(1, "null argument");
    if (!postproc_window_supported(kh, kw)) return fail(1, "crf_iter: the window sides must be odd and at most 7, got %d x %d", kh, kw);
    if (classes < 1 || classes > 32) return fail(1, "crf_iter: 1 to 32 classes, got %d", classes);
    if (batch < 1 || batch > 65535 || height < 1 || width < 1 || height > 65535 * 8) return fail(1, "crf_iter: batch must be in [1, 65535], height and width positive");
    if (q_out == q_in || q_out == unary) return fail(1, "crf_iter: q_out must not alias an input");
    HIP_TRY(launch_crf_iter(q_in, unary, xyz, mask, params, q_out, batch, classes, height, width, kh, kw, uniform_beta, (hipStream_t)stream));
    return 0;
}

static bool error_geometry_ok(int32_t B, int64_t plane) { return B >= 1 && B <= 65535 && plane >= 1 && plane <= (1LL << 40) / 5 / B; }

size_t r2dm_completion_error_scratch_bytes(int32_t B, int64_t plane) {
    return error_geometry_ok(B, plane) ? completion_error_scratch_bytes(B, plane) : 0;
}

int r2dm_completion_error(const float* pred, const float* target, const float* known, float lo, float hi, int32_t B, int64_t plane, void* scratch,
                          double* out, void* stream) {
    if (!pred || !target || !known || !scratch || !out) return fail(1, "null argument");
    if (!error_geometry_ok(B, plane)) return fail(1, "completion_error: batch must be in [1, 65535], the tensors 1 to 2^40 elements");
    const uintptr_t a = plane % 4 == 0 ? 15 : 3;  // a plane that is a multiple of 4 is read as quads
    if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)known) & a)
        return fail(1, "completion_error: pred, target and known must be %d-byte aligned for a plane of %lld elements", (int)a + 1, (long long)plane);
    if (((uintptr_t)scratch | (uintptr_t)out) & 7) return fail(1, "completion_error: scratch and out must be 8-byte aligned");
    HIP_TRY(launch_completion_error(pred, target, known, lo, hi, B, plane, scratch, out, (hipStream_t)stream));
    return 0;
}

static bool ensemble_geometry_ok(int32_t B, int32_t K, int64_t plane) {
    return B >= 1 && B <= 65535 && K >= 1 && K <= 64 && plane >= 1 && plane <= (1LL << 40) / 5 / K / B;
}

size_t r2dm_ensemble_score_scratch_bytes(int32_t B, int32_t K, int64_t plane) {
    return ensemble_geometry_ok(B, K, plane) ? ensemble_score_scratch_bytes(B, K, plane) : 0;
}

int r2dm_ensemble_score(const float* samples, const float* target, const float* known, float lo, float hi, int32_t B, int32_t K, int64_t plane,
                        void* scratch, double* raw, double* member, int64_t* rank, float* maps, void* stream) {
    if (!samples || !target || !known || !scratch || !raw || !member || !rank) return fail(1, "ensemble_score: null argument (only maps may be null)");
    if (B < 1 || B > 65535) return fail(1, "ensemble_score: batch must be in [1, 65535], got %d", B);
    if (K < 1 || K > 64) return fail(1, "ensemble_score: members must be in [1, 64] (the members of a pixel are sorted in registers), got %d", K);
    if (plane < 1 || plane > (1LL << 40)) return fail(1, "ensemble_score: plane must be in [1, 2^40], got %lld", (long long)plane);
    if (!ensemble_geometry_ok(B, K, plane)) return fail(1, "ensemble_score: samples of more than 2^40 elements");
    const uintptr_t a = plane % 4 == 0 ? 15 : 3;
    if (((uintptr_t)samples | (uintptr_t)target | (uintptr_t)known | (uintptr_t)maps) & a)
        return fail(1, "ensemble_score: samples, target, known and maps must be %d-byte aligned for a plane of %lld elements", (int)a + 1,
                    (long long)plane);
    if (((uintptr_t)scratch | (uintptr_t)raw | (uintptr_t)member | (uintptr_t)rank) & 7)
        return fail(1, "ensemble_score: scratch, raw, member and rank must be 8-byte aligned");
    if (maps) {  // the kernel writes a pixel's maps before other threads have read their inputs
        const uintptr_t m0 = (uintptr_t)maps, m1 = m0 + (uintptr_t)B * 8 * plane * 4;
        const uintptr_t in[3][2] = {{(uintptr_t)samples, (uintptr_t)B * K * 5 * plane * 4}, {(uintptr_t)target, (uintptr_t)B * 5 * plane * 4},
                                    {(uintptr_t)known, (uintptr_t)B * plane * 4}};
        for (const auto& r : in)
            if (m0 < r[0] + r[1] && r[0] < m1) return fail(1, "ensemble_score: maps must not alias an input");
    }
    HIP_TRY(launch_ensemble_score(samples, target, known, lo, hi, B, K, plane, scratch, raw, member, reinterpret_cast<long long*>(rank), maps,
                                  (hipStream_t)stream));
    return 0;
}

static bool coherence_geometry_ok(int32_t B, int32_t K, int32_t H, int32_t W, int32_t offsets) {
    return H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31) && offsets >= 0 && offsets <= 16 && ensemble_geometry_ok(B, K, (int64_t)H * W);
}

size_t r2dm_ensemble_coherence_scratch_bytes(int32_t B, int32_t K, int32_t H, int32_t W, int32_t offsets) {
    return coherence_geometry_ok(B, K, H, W, offsets) ? ensemble_coherence_scratch_bytes(B, K, (long)H * W, offsets) : 0;
}

int r2dm_ensemble_coherence(const float* samples, const float* target, const float* known, float lo, float hi, int32_t B, int32_t K, int32_t H,
                            int32_t W, const int32_t* offsets_hw, int32_t offsets, void* scratch, double* counts, double* dist, double* vario,
                            void* stream) {
    if (!samples || !target || !known || !scratch || !counts) return fail(1, "ensemble_coherence: null argument (only dist and vario may be null)");
    if (B < 1 || B > 65535) return fail(1, "ensemble_coherence: batch must be in [1, 65535], got %d", B);
    if (K < 1 || K > 64) return fail(1, "ensemble_coherence: members must be in [1, 64], got %d", K);
    if (H < 1 || W < 1 || (int64_t)H * W >= (1LL << 31))
        return fail(1, "ensemble_coherence: height and width must be >= 1 and height * width < 2^31, got %d x %d", H, W);
    if (offsets < 0 || offsets > 16) return fail(1, "ensemble_coherence: offsets must be in [0, 16], got %d", offsets);
    if (offsets > 0 && !offsets_hw) return fail(1, "ensemble_coherence: null argument (offsets_hw with %d offsets)", offsets);
    for (int32_t o = 0; o < offsets; ++o) {
        const int64_t dh = offsets_hw[2 * o], dw = offsets_hw[2 * o + 1];
        if ((dh == 0 && dw == 0) || dh <= -(int64_t)H || dh >= H || dw <= -(int64_t)W || dw >= W)
            return fail(1, "ensemble_coherence: offset %d = (%lld, %lld) must satisfy |dh| < %d, |dw| < %d and not be (0, 0)", o, (long long)dh,
                        (long long)dw, H, W);
    }
    const int64_t plane = (int64_t)H * W;
    if (!ensemble_geometry_ok(B, K, plane)) return fail(1, "ensemble_coherence: samples of more than 2^40 elements");
    const uintptr_t a = plane % 4 == 0 ? 15 : 3;
    if (((uintptr_t)samples | (uintptr_t)target | (uintptr_t)known) & a)
        return fail(1, "ensemble_coherence: samples, target and known must be %d-byte aligned for a plane of %lld elements", (int)a + 1,
                    (long long)plane);
    if (((uintptr_t)scratch | (uintptr_t)counts | (uintptr_t)dist | (uintptr_t)vario) & 7)
        return fail(1, "ensemble_coherence: scratch, counts, dist and vario must be 8-byte aligned");
    HIP_TRY(launch_ensemble_coherence(samples, target, known, lo, hi, B, K, H, W, offsets_hw, offsets, scratch, counts, dist, vario,
                                      (hipStream_t)stream));
    return 0;
}

int r2dm_confusion_matrix(const int64_t* pred, const int64_t* target, const float* mask, int32_t B, int64_t pixels, int32_t classes, int64_t* counts,
                          int64_t* bad, void* stream) {
    if (!pred || !target || !counts || !bad) return fail(1, "null argument");
    if (classes < 1 || classes > 64) return fail(1, "confusion_matrix: classes must be in [1, 64] (one table per block in LDS), got %d", classes);
    if (B < 1 || B > 65535 || pixels < 1 || pixels > (1LL << 40) / B)
        return fail(1, "confusion_matrix: batch must be in [1, 65535], the label images 1 to 2^40 elements");
    if ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)counts | (uintptr_t)bad) & 7) || ((uintptr_t)mask & 3))
        return fail(1, "confusion_matrix: pred, target, counts and bad must be 8-byte aligned, mask 4-byte aligned");
    HIP_TRY(launch_confusion_matrix(reinterpret_cast<const long long*>(pred), reinterpret_cast<const long long*>(target), mask, B, pixels, classes,
                                    reinterpret_cast<long long*>(counts), reinterpret_cast<long long*>(bad), (hipStream_t)stream));
    return 0;
}

int r2dm_fill_beams(const float* x, const uint8_t* rows, float* out, int32_t B, int32_t C, int32_t H, int32_t W, float nodata, int32_t mode,
                    void* stream) {
    if (!x || !rows || !out) return fail(1, "null argument");
    if (mode != 0 && mode != 1) return fail(1, "fill_beams: mode must be 0 (nearest) or 1 (linear), got %d", mode);
    if (B < 1 || B > 65535 || H < 1 || H > 65535 || C < 1 || W < 1 || (int64_t)C * H > (1LL << 40) / W / B)
        return fail(1, "fill_beams: batch and height must be in [1, 65535], channels and width positive, the tensor at most 2^40 elements");
    if (((uintptr_t)x | (uintptr_t)out) & 3) return fail(1, "fill_beams: x and out must be 4-byte aligned");
    if (x == out) return fail(1, "fill_beams: out must not alias x");
    HIP_TRY(launch_fill_beams(x, rows, out, B, C, H, W, nodata, mode, (hipStream_t)stream));
    return 0;
}

static bool nn_geometry_ok(int64_t P, int64_t max_points) {
    return P >= 1 && max_points >= 1 && max_points <= (1LL << 21) && 2 * P <= 0x7fffffffLL / nn_pairs_chunks(max_points);
}

size_t r2dm_nn_pairs_scratch_bytes(int64_t P, int64_t max_points) { return nn_geometry_ok(P, max_points) ? nn_pairs_scratch_bytes(P, max_points) : 0; }

int r2dm_nn_pairs(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                  int64_t b_clouds, int64_t b_total, const int64_t* pairs, int64_t P, int64_t max_points, double tau, float* d2_ab, int32_t* idx_ab,
                  const int64_t* out_ab, float* d2_ba, int32_t* idx_ba, const int64_t* out_ba, void* scratch, double* sums, int64_t* status,
                  void* stream) {
    if (!a_offsets || !b_offsets || !pairs || !scratch || !sums || !status) return fail(1, "null argument");
    if (a_clouds < 1 || b_clouds < 1 || a_total < 0 || b_total < 0 || (!a && a_total) || (!b && b_total))
        return fail(1, "nn_pairs: each set needs at least one cloud, and a pointer unless it has no points");
    if (max_points > (1LL << 21)) return fail(1, "nn_pairs: clouds of up to 2^21 points, got max_points = %lld", (long long)max_points);
    if (!nn_geometry_ok(P, max_points))
        return fail(1, "nn_pairs: num_pairs and max_points must be >= 1 and 2 * num_pairs * ceil(max_points / 1024) at most 2^31 - 1 blocks, got %lld, %lld",
                    (long long)P, (long long)max_points);
    if (!(tau >= 0.0)) return fail(1, "nn_pairs: tau must be >= 0");
    if ((idx_ab && !d2_ab) || (idx_ba && !d2_ba) || (d2_ab && !out_ab) || (d2_ba && !out_ba))
        return fail(1, "nn_pairs: an index output needs its d2 output, a d2 output its start offsets");
    if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(1, "nn_pairs: a and b must be 16-byte aligned (rows are read as quads)");
    if (((uintptr_t)a_offsets | (uintptr_t)b_offsets | (uintptr_t)pairs | (uintptr_t)out_ab | (uintptr_t)out_ba | (uintptr_t)scratch | (uintptr_t)sums |
         (uintptr_t)status) & 7)
        return fail(1, "nn_pairs: offsets, pairs, scratch, sums and status must be 8-byte aligned");
    if (((uintptr_t)d2_ab | (uintptr_t)idx_ab | (uintptr_t)d2_ba | (uintptr_t)idx_ba) & 3) return fail(1, "nn_pairs: per-point outputs must be 4-byte aligned");
    HIP_TRY(launch_nn_pairs(a, reinterpret_cast<const long long*>(a_offsets), a_clouds, a_total, b, reinterpret_cast<const long long*>(b_offsets), b_clouds,
                            b_total, reinterpret_cast<const long long*>(pairs), P, max_points, tau, d2_ab, idx_ab,
                            reinterpret_cast<const long long*>(out_ab), d2_ba, idx_ba, reinterpret_cast<const long long*>(out_ba), scratch, sums,
                            reinterpret_cast<long long*>(status), (hipStream_t)stream));
    return 0;
}

size_t r2dm_voxel_occupancy_scratch_bytes(int64_t G, int64_t S, int64_t max_group_points) {
    return voxel_geometry_ok(G, S, max_group_points) ? voxel_occupancy_scratch_bytes(G, S, max_group_points) : 0;
}

int r2dm_voxel_occupancy(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                         int64_t b_clouds, int64_t b_total, const int64_t* members, const int64_t* targets, int64_t G, int64_t K, const float* sizes,
                         int64_t S, int64_t max_group_points, void* scratch, int64_t* member_out, int64_t* hist_out, int64_t* status, void* stream) {
    if (!a_offsets || !b_offsets || !members || !targets || !sizes || !scratch || !member_out || !hist_out || !status) return fail(1, "null argument");
    if (a_clouds < 1 || b_clouds < 1 || a_total < 0 || b_total < 0 || (!a && a_total) || (!b && b_total))
        return fail(1, "voxel_occupancy: each set needs at least one cloud, and a pointer unless it has no points");
    if (G < 1 || K < 1 || S < 1) return fail(1, "voxel_occupancy: groups, members and sizes must be >= 1, got %lld, %lld, %lld", (long long)G, (long long)K, (long long)S);
    if (K > 63)
        return fail(1, "voxel_occupancy: at most 63 members per group (a voxel's membership mask has 64 bits and bit 63 is the target's), got %lld", (long long)K);
    if (S > 8) return fail(1, "voxel_occupancy: at most 8 voxel sizes per call, got %lld", (long long)S);
    if ((uintptr_t)sizes & 3) return fail(1, "voxel_occupancy: sizes must be 4-byte aligned");
    for (int64_t i = 0; i < S; ++i)
        if (!(sizes[i] > 0.0f) || !(sizes[i] <= 3.4028234663852886e38f)) return fail(1, "voxel_occupancy: a voxel size must be finite and > 0, got %g", (double)sizes[i]);
    if (!voxel_geometry_ok(G, S, max_group_points))
        return fail(1, "voxel_occupancy: at most 65535 groups, max_group_points in [1, 2^27] and groups * sizes * capacity at most 2^36 slots "
                       "(capacity: the power of two >= 2 * max_group_points), got %lld groups, %lld sizes, max_group_points = %lld",
                    (long long)G, (long long)S, (long long)max_group_points);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)scratch) & 15)
        return fail(1, "voxel_occupancy: a, b and scratch must be 16-byte aligned (rows and slots are accessed as quads and pairs)");
    if (((uintptr_t)a_offsets | (uintptr_t)b_offsets | (uintptr_t)members | (uintptr_t)targets | (uintptr_t)member_out | (uintptr_t)hist_out |
         (uintptr_t)status) & 7)
        return fail(1, "voxel_occupancy: offsets, members, targets, member_out, hist_out and status must be 8-byte aligned");
    HIP_TRY(launch_voxel_occupancy(a, reinterpret_cast<const long long*>(a_offsets), a_clouds, a_total, b, reinterpret_cast<const long long*>(b_offsets),
                                   b_clouds, b_total, reinterpret_cast<const long long*>(members), reinterpret_cast<const long long*>(targets), G, K,
                                   sizes, S, max_group_points, scratch, reinterpret_cast<long long*>(member_out), reinterpret_cast<long long*>(hist_out),
                                   reinterpret_cast<long long*>(status), (hipStream_t)stream));
    return 0;
}

static bool emd_geometry_ok(int64_t P, int64_t max_points, double eps, int64_t max_rounds) {
    // (eps must also be a normal fp32 number: the auction bids in fp32)
    return P >= 1 && P <= 0x7fffffffLL && max_points >= 1 && max_points <= emd_max_points() && eps >= 1.1754943508222875e-38 && eps <= 3.4028234663852886e38 &&
           max_rounds >= 1;
}

int64_t r2dm_emd_max_points(void) { return emd_max_points(); }

size_t r2dm_emd_pairs_scratch_bytes(int64_t P, int64_t max_points) { return emd_geometry_ok(P, max_points, 1.0, 1) ? emd_pairs_scratch_bytes(P) : 0; }

int r2dm_emd_pairs(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                   int64_t b_clouds, int64_t b_total, const int64_t* pairs, int64_t P, int64_t max_points, double eps, int64_t max_rounds,
                   int32_t* assignment, float* prices, double* out, void* scratch, int64_t* status, void* stream) {
    if (!a_offsets || !b_offsets || !pairs || !out || !scratch || !status) return fail(1, "null argument");
    if (a_clouds < 1 || b_clouds < 1 || a_total < 0 || b_total < 0 || (!a && a_total) || (!b && b_total))
        return fail(1, "emd_pairs: each set needs at least one cloud, and a pointer unless it has no points");
    if (max_points > emd_max_points())
        return fail(1, "emd_pairs: clouds of up to %lld points (the auction of a pair lives in one workgroup's LDS), got max_points = %lld",
                    (long long)emd_max_points(), (long long)max_points);
    if (!(eps > 0.0) || !(eps <= 3.4028234663852886e38) || eps < 1.1754943508222875e-38)
        return fail(1, "emd_pairs: eps must be finite and > 0 (a normal fp32 number), got %g", eps);
    if (max_rounds < 1) return fail(1, "emd_pairs: max_rounds must be >= 1, got %lld", (long long)max_rounds);
    if (!emd_geometry_ok(P, max_points, eps, max_rounds))
        return fail(1, "emd_pairs: num_pairs must be in [1, 2^31 - 1] and max_points >= 1, got %lld, %lld", (long long)P, (long long)max_points);
    if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(1, "emd_pairs: a and b must be 16-byte aligned (rows are read as quads)");
    if (((uintptr_t)a_offsets | (uintptr_t)b_offsets | (uintptr_t)pairs | (uintptr_t)out | (uintptr_t)scratch | (uintptr_t)status) & 7)
        return fail(1, "emd_pairs: offsets, pairs, out, scratch and status must be 8-byte aligned");
    if (((uintptr_t)assignment | (uintptr_t)prices) & 3) return fail(1, "emd_pairs: assignment and prices must be 4-byte aligned");
    HIP_TRY(launch_emd_pairs(a, reinterpret_cast<const long long*>(a_offsets), a_clouds, a_total, b, reinterpret_cast<const long long*>(b_offsets), b_clouds,
                             b_total, reinterpret_cast<const long long*>(pairs), P, max_points, eps, max_rounds, assignment, prices, out, scratch,
                             reinterpret_cast<long long*>(status), (hipStream_t)stream));
    return 0;
}

}  // extern "C"
