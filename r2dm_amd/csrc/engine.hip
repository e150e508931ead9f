// The model's C ABI (include/r2dm_hip.h): create / bind / load / workspace / forward / range guard / profiling.  The plan is built in plan.hip,
// the forward walk lives in forward.hip; the stand-alone operators and the single-kernel test entries are in ops_abi.hip and kernel_abi.hip.
#include <stdarg.h>

#include <algorithm>

#include "engine.h"

using namespace r2dm;

namespace r2dm {

static thread_local char g_err[512] = "";  // what r2dm_last_error returns: the only definition, written by every file's fail()

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int g_single_kernel_pieces = 2;  // r2dm_conv2d_ring (per-op tests)

}  // namespace r2dm

// =================================================================================================
extern "C" {

const char* r2dm_last_error(void) { return g_err; }
const char* r2dm_version(void) { return "r2dm_hip 0.5 (gfx950)"; }

int r2dm_create(r2dm_handle** out, const r2dm_config* cfg) {
    if (!out || !cfg) return fail(1, "null argument");
    if (int rc = check_config(*cfg)) return rc;
    r2dm_handle* h = new r2dm_handle();
    h->cfg = *cfg;
    if (const char* e = getenv("R2DM_DOWN_GEMM")) h->down_gemm = atoi(e) == 0 ? 0 : atoi(e) == 9 ? 9 : 1;
    (void)hipGetDevice(&h->device);
    build_plan(h);
    *out = h;
    return 0;
}

void r2dm_destroy(r2dm_handle* h) {
    if (!h) return;
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    delete h;
}

int64_t r2dm_num_tensors(const r2dm_handle* h) { return h ? (int64_t)h->slots.size() : 0; }

int r2dm_tensor_at(const r2dm_handle* h, int64_t i, r2dm_tensor_info* out) {
    if (!h || !out || i < 0 || i >= (int64_t)h->slots.size()) return fail(1, "tensor index out of range");
    out->key = h->slots[i].key.c_str();
    out->numel = h->slots[i].numel;
    return 0;
}

size_t r2dm_blob_bytes(const r2dm_handle* h) { return h ? h->blob_floats * sizeof(float) : 0; }
// The two parts of the blob that are not weights: the range-guard slots -- int[2 RANGE_SITES]: [0] the packers' weight flag, [2 k + 1] the running maximum of
// site k, raised by every forward -- and in_conv's constant coordinate map, which the first forward after a bind computes from the weights.
int r2dm_blob_flag_region(const r2dm_handle* h, size_t* offset, size_t* bytes) {
    if (!h || !offset || !bytes) return fail(1, "null argument");
    *offset = h->range_flag * sizeof(float);
    *bytes = 2 * r2dm_handle::RANGE_SITES * sizeof(int);
    return 0;
}
int r2dm_blob_cmap_region(const r2dm_handle* h, size_t* offset, size_t* bytes) {
    if (!h || !offset || !bytes) return fail(1, "null argument");
    const r2dm_config& c = h->cfg;
    *offset = c.coord_channels > 0 ? h->cmap * sizeof(float) : 0;
    *bytes = c.coord_channels > 0 ? (size_t)c.base_channels * c.height * c.width * sizeof(float) : 0;
    return 0;
}
int r2dm_bind_blob(r2dm_handle* h, void* blob, size_t bytes) {
    if (!h || !blob) return fail(1, "null argument");
    if (bytes < r2dm_blob_bytes(h)) return fail(1, "blob too small: %zu < %zu", bytes, r2dm_blob_bytes(h));
    if ((uintptr_t)blob & (kAlign - 1)) return fail(1, "blob must be %zu-byte aligned", kAlign);
    h->blob = (float*)blob;
    h->cmap_ready = false;
    // The range flags travel WITH the blob: [0] (a weight outside the fp16 range, raised by the packers) must survive a bind
    // on another rank, and nothing here may touch device memory behind the caller's streams.  A blob that is filled through
    // r2dm_load_tensor gets both flags cleared by the first load after this bind, on the packing stream.  The site bounds [1..] of an
    // adopted blob are the SOURCE's running maxima, not this handle's: the caller clears them on its own stream (r2dm_blob_flag_region;
    // unet.py adopt_packed_weights) -- not here, for the same reason.
    h->flags_fresh = false;
    return 0;
}

int r2dm_check_range(r2dm_handle* h, void* stream) {
    if (!h) return fail(1, "null argument");
    if (!h->blob) return 0;
    hipStream_t st = (hipStream_t)stream;
    constexpr int NS = r2dm_handle::RANGE_SITES;
    static_assert(sizeof(int) == sizeof(float), "bounds travel as float bits");
    int v[2 * NS];
    HIP_TRY(hipMemcpyAsync(v, h->blob + h->range_flag, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float bound = 0.f;
    int worst = 0;
    bool any = false;
    for (int k = 0; k < NS; ++k) {  // (bounds are non-negative floats: they order like their bit patterns; a NaN bound compares false below and trips)
        memcpy(&h->site_bounds[k], &v[2 * k + 1], sizeof(float));
        any = any || v[2 * k + 1] != 0;
        if (v[2 * k + 1] > v[2 * worst + 1]) worst = k;
    }
    h->sites_read = (int)h->site_names.size() < NS ? (int)h->site_names.size() : NS;
    bound = h->site_bounds[worst];
    // The bounds are RUNNING maxima and stay after a clean check; they are reset only when this check reports a trip, so that the check after the fallback reports
    // what ran since ([0], the packers' weight flag, stays).  Round 6: with one slot per site a reset at every check (every 8-32 steps of a sampler) sent each tracked
    // site's next launch into a storm of atomicMax on a zeroed slot -- every wave of fir_up2 beats a bound of 0 -- +8 us on each of those launches, 25 us per step in
    // the traced average (scripts/jobs/j425.sh); one slot for the whole forward (round 5) hid that behind the first GroupNorm's bound.
    if (any && !(bound < 65504.f)) {
        HIP_TRY(hipMemsetAsync(h->blob + h->range_flag + 1, 0, (2 * NS - 1) * sizeof(int), st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (v[0] != 0)
        return fail(2, "a convolution weight is not finite (the fp16 packings scale every layer into the fp16 range, so only inf / nan "
                       "get here); the weights are not usable");
    if (!(bound < 65504.f))
        return fail(2, "an input of the fp16-operand convolution path may be outside the fp16 range (65504): largest data-driven bound "
                       "(GroupNorm outputs: |a| M + |d|, M >= max|x| from the statistics slots; raw inputs: recorded max|x|) = %.3g at %s; results of "
                       "this forward are not valid; select the bf16x3 split with r2dm_set_conv_pieces(h, 3)", (double)bound,
                    worst < (int)h->site_names.size() && !h->site_names[worst].empty() ? h->site_names[worst].c_str() : "(unnamed site)");
    return 0;
}

int r2dm_range_sites(r2dm_handle* h, float* bounds, int32_t cap, int32_t* n) {
    if (!h || !n) return fail(1, "null argument");
    *n = h->sites_read;
    for (int k = 0; bounds && k < h->sites_read && k < cap; ++k) bounds[k] = h->site_bounds[k];
    return 0;
}

const char* r2dm_range_site_name(r2dm_handle* h, int32_t k) {
    if (!h || k < 0 || k >= (int)h->site_names.size()) return "";
    return k == 0 && h->site_names[0].empty() ? "(shared slot: test hook / sites beyond the table)" : h->site_names[k].c_str();
}

__global__ void raise_range_bound_kernel(int* flag, float bound) { atomicMax(flag + 1, __float_as_int(bound)); }

int r2dm_test_raise_range_bound(r2dm_handle* h, float bound, void* stream) {
    if (!h || !h->blob) return fail(1, "no weights bound");
    if (!(bound >= 0.f)) return fail(1, "bound must be non-negative");
    raise_range_bound_kernel<<<1, 1, 0, (hipStream_t)stream>>>((int*)(h->blob + h->range_flag), bound);
    HIP_TRY(hipGetLastError());
    return 0;
}

int r2dm_load_tensor(r2dm_handle* h, int64_t i, const float* src, int64_t numel, void* stream) {
    if (!h || !src) return fail(1, "null argument");
    if (!h->blob) return fail(1, "bind a blob first");
    if (i < 0 || i >= (int64_t)h->slots.size()) return fail(1, "tensor index out of range");
    const Slot& s = h->slots[i];
    if (numel != s.numel) return fail(1, "%s: expected %lld elements, got %lld", s.key.c_str(), (long long)s.numel, (long long)numel);
    hipStream_t st = (hipStream_t)stream;
    if (!h->flags_fresh) {  // first load into a freshly bound blob: both range flags start from zero, ordered before the packers
        HIP_TRY(hipMemsetAsync(h->blob + h->range_flag, 0, 2 * r2dm_handle::RANGE_SITES * sizeof(int), st));
        h->flags_fresh = true;
    }
    if (s.kind == SLOT_RAW) {
        HIP_TRY(hipMemcpyAsync(h->blob + s.off, src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        HIP_TRY(launch_pack_conv(src, h->blob + s.off, s.conv.cout, s.conv.cin, s.conv.taps, s.conv.co_tile,
                                 s.conv.cin_pad, st, s.conv.algo, s.conv.src_cin, s.conv.src_off));
        if (s.conv.f2)
            HIP_TRY(launch_pack_conv_f16x2(src, h->blob + s.conv.w_f2, s.conv.cout, s.conv.cin, (int*)(h->blob + h->range_flag), st,
                                           h->blob + s.conv.ws_f2, s.conv.f2_cot, s.conv.f2_rows));
        if (s.conv.p1)
            HIP_TRY(launch_pack_proj_f16x2(src, h->blob + s.conv.w_p1, s.conv.cout, s.conv.cin, (int*)(h->blob + h->range_flag), st,
                                           h->blob + s.conv.ws_p1));
        if (s.conv.dg)
            HIP_TRY(launch_pack_proj_f16x2(src, h->blob + s.conv.w_dg, s.conv.cout, 9 * s.conv.cin, (int*)(h->blob + h->range_flag), st,
                                           h->blob + s.conv.ws_dg, 9));
    }
    h->cmap_ready = false;  // (any reload: cheap to recompute)
    return 0;
}

size_t r2dm_workspace_bytes(const r2dm_handle* hc, int32_t B) {
    r2dm_handle* h = const_cast<r2dm_handle*>(hc);
    if (!h || B < 1) return 0;
    auto it = h->ws_cache.find(B);
    if (it != h->ws_cache.end()) return it->second;
    Arena ar{(char*)kAlign, 0, true};
    run_forward(h, ar, (const float*)kAlign, (const float*)kAlign, (float*)kAlign, B, nullptr);
    const size_t bytes = ar.peak + kAlign;
    h->ws_cache[B] = bytes;
    return bytes;
}

int r2dm_forward_listing(const r2dm_handle* h, int32_t B, char* buf, size_t cap, size_t* need) {
    if (!h || B < 1 || !need) return fail(1, "forward_listing: a handle, a batch >= 1 and `need`");
    std::string s;
    Arena ar{(char*)kAlign, 0, true};
    // (the caller's output: any address the arena never hands out; the walk with a listing changes nothing in the handle)
    if (int rc = run_forward(const_cast<r2dm_handle*>(h), ar, (const float*)kAlign, (const float*)kAlign, (float*)sizeof(float), B, nullptr, &s)) return rc;
    *need = s.size() + 1;
    if (buf && cap) {
        const size_t n = std::min(s.size(), cap - 1);
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return 0;
}

int r2dm_unet_forward(r2dm_handle* h, const float* x, const float* cond, float* out, int32_t B, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!h || !x || !cond || !out || !ws) return fail(1, "null argument");
    if (!h->blob) return fail(1, "weights not loaded (r2dm_bind_blob / r2dm_load_tensor)");
    if (B < 1) return fail(1, "batch must be >= 1");
    char* base = (char*)align_up((size_t)(uintptr_t)ws);
    const size_t cap = ws_bytes - (size_t)(base - (char*)ws);
    Arena ar{base, cap, false};
    return run_forward(h, ar, x, cond, out, B, (hipStream_t)stream);
}

// ---- the feature cache: a second walk over the same stages (forward.hip run_forward, CacheWalk) ----
static int cache_refused(const r2dm_handle* h, int32_t B, int32_t depth, int32_t mode) {
    if (!h) return fail(1, "null argument");
    if (B < 1) return fail(1, "batch must be >= 1");
    if (B > h->cfg.max_batch) return fail(1, "feature cache: batch %d exceeds max_batch %d", B, h->cfg.max_batch);
    if (depth < 1 || depth > 3) return fail(1, "feature cache: depth must be 1, 2 or 3 (the outermost levels that stay live), got %d", depth);
    if (mode != 1 && mode != 2) return fail(1, "feature cache: mode must be 1 (store: the full forward) or 2 (reuse: the live stages only), got %d", mode);
    return 0;
}

size_t r2dm_cache_bytes(const r2dm_handle* h, int32_t B, int32_t depth) {
    if (!h || B < 1 || depth < 1 || depth > 3) return 0;
    return cache_layout(h, B, depth).total;
}

int r2dm_unet_forward_cached(r2dm_handle* h, const float* x, const float* cond, float* out, int32_t B, void* ws, size_t ws_bytes, void* stream, void* cache,
                             size_t cache_bytes, int32_t depth, int32_t mode, double* drift) {
    if (!h || !x || !cond || !out || !ws || !cache) return fail(1, "null argument");
    if (int rc = cache_refused(h, B, depth, mode)) return rc;
    if ((uintptr_t)cache & (kAlign - 1)) return fail(1, "feature cache: the buffer must be %zu-byte aligned", kAlign);
    const size_t need = cache_layout(h, B, depth).total;
    if (cache_bytes < need) return fail(1, "feature cache too small: %zu < %zu bytes (r2dm_cache_bytes)", cache_bytes, need);
    if (drift && ((uintptr_t)drift & 7)) return fail(1, "feature cache: drift must be 8-byte aligned");
    if (!h->blob) return fail(1, "weights not loaded (r2dm_bind_blob / r2dm_load_tensor)");
    char* base = (char*)align_up((size_t)(uintptr_t)ws);
    if (ws_bytes < (size_t)(base - (char*)ws)) return fail(3, "workspace too small");
    Arena ar{base, ws_bytes - (size_t)(base - (char*)ws), false};
    const CacheWalk cw{cache, depth, mode, mode == 1 ? drift : nullptr};
    h->sites_keyed = true;  // (from here on this handle's range sites are numbered by identity: engine.h)
    return run_forward(h, ar, x, cond, out, B, (hipStream_t)stream, nullptr, &cw);
}

int r2dm_forward_listing_cached(const r2dm_handle* hc, int32_t B, int32_t depth, int32_t mode, char* buf, size_t cap, size_t* need) {
    if (!need) return fail(1, "forward_listing_cached: `need` is null");
    if (int rc = cache_refused(hc, B, depth, mode)) return rc;
    r2dm_handle* h = const_cast<r2dm_handle*>(hc);
    // the full walk first, into a table of its own: it gives every site the number the plain listing shows, and the cached walk looks its sites up there
    std::vector<std::string> sites;
    std::string full, s;
    Arena a0{(char*)kAlign, 0, true};
    if (int rc = run_forward(h, a0, (const float*)kAlign, (const float*)kAlign, (float*)sizeof(float), B, nullptr, &full, nullptr, &sites)) return rc;
    Arena ar{(char*)kAlign, 0, true};
    const CacheWalk cw{(void*)(2 * sizeof(float)), depth, mode, nullptr};  // (like the output: an address the arena never hands out)
    if (int rc = run_forward(h, ar, (const float*)kAlign, (const float*)kAlign, (float*)sizeof(float), B, nullptr, &s, &cw, &sites)) return rc;
    *need = s.size() + 1;
    if (buf && cap) {
        const size_t n = std::min(s.size(), cap - 1);
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return 0;
}

int r2dm_set_conv_pieces(r2dm_handle* h, int32_t pieces) {
    if (!h && (pieces == 4 || pieces == 5)) {  // per-op tests only: the fp32-input MFMA kernel as the yardstick of the split-operand kernels --
        g_single_kernel_pieces = pieces;       // 4: as the library runs it (two-level accumulation above 128 channels), 5: a plain fmaf chain
        return 0;
    }
    if (pieces < 1 || pieces > 3)
        return fail(1, "pieces must be 2 (fp16 + scaled fp16 residual: the default parity mode), 3 (three bf16 pieces: fp32 operand range) or "
                       "1 (one fp16 product per MAC: reduced precision)");
    if (h) {
        h->conv_pieces = pieces;
        h->ws_cache.clear();  // (the walk's allocation sequence depends on the mode -- folded GroupNorms)
    } else
        g_single_kernel_pieces = pieces;
    return 0;
}

int r2dm_profile_enable(r2dm_handle* h, int32_t on) {
    if (!h) return fail(1, "null argument");
    h->prof_on = on != 0;
    h->prof_reset();
    return 0;
}

// What a bracketing event pair adds to the kernel it brackets (bench.py prints it next to the per-launch figures): the pair around nothing, and around
// an empty kernel -- marker processing, and marker processing + one dispatch + that kernel's own microsecond.  Medians of 33.
__global__ void empty_kernel() {}
int r2dm_profile_event_overhead(r2dm_handle* h, void* stream, double* empty_pair_us, double* empty_kernel_pair_us) {
    if (!h || !empty_pair_us || !empty_kernel_pair_us) return fail(1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return fail(2, "hipEventCreate"); }
    int rc = 0;
    for (int with_kernel = 0; with_kernel < 2 && rc == 0; ++with_kernel) {
        std::vector<float> t;
        for (int i = 0; i < 36 && rc == 0; ++i) {
            hipError_t e = hipEventRecord(e0, st);
            if (with_kernel) empty_kernel<<<1, 64, 0, st>>>();
            if (e == hipSuccess) e = hipEventRecord(e1, st);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) rc = fail(2, "event pair calibration: %s", hipGetErrorString(e));
            else if (i >= 3) t.push_back(ms);  // (the first pairs pay for the code object)
        }
        if (rc == 0) {
            std::sort(t.begin(), t.end());
            (with_kernel ? *empty_kernel_pair_us : *empty_pair_us) = 1e3 * (double)t[t.size() / 2];
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

// one pass over the bracketed launches since the last read: time, flops and count per class, and the time of all of them
static int prof_collect(r2dm_handle* h, double* ms3, double* flop3, int64_t* launches3, double* total_ms) {
    for (int c = 0; c < 3; ++c) { ms3[c] = 0.0; flop3[c] = 0.0; launches3[c] = 0; }
    *total_ms = 0.0;
    for (size_t i = 0; i + 1 < h->prof_used && i / 2 < h->prof_cls.size(); i += 2) {
        HIP_TRY(hipEventSynchronize(h->prof_ev[i + 1]));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, h->prof_ev[i], h->prof_ev[i + 1]));
        const int c = h->prof_cls[i / 2];
        *total_ms += t;
        ms3[c] += t;
        flop3[c] += h->prof_lflop[i / 2];
        launches3[c] += 1;
    }
    return 0;
}

int r2dm_profile_read_classes(r2dm_handle* h, double* ms3, double* flop3, int64_t* launches3) {
    if (!h || !ms3 || !flop3 || !launches3) return fail(1, "null argument");
    double total_ms;
    if (int rc = prof_collect(h, ms3, flop3, launches3, &total_ms)) return rc;
    h->prof_reset();
    return 0;
}

int r2dm_profile_read(r2dm_handle* h, double* conv_ms, double* conv_flop, int64_t* launches) {
    if (!h || !conv_ms || !conv_flop || !launches) return fail(1, "null argument");
    double ms3[3], flop3[3];
    int64_t launches3[3];
    if (int rc = prof_collect(h, ms3, flop3, launches3, conv_ms)) return rc;
    *conv_flop = h->prof_flop;
    *launches = (int64_t)(h->prof_used / 2);
    h->prof_reset();
    return 0;
}

}  // extern "C"
