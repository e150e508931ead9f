// The forward walk: r2dm_unet_forward replaces EfficientUNet.forward (efficient_unet.py:269-295).  run_forward walks the eight U-Net
// stages and enqueues the HIP kernels of this library on the caller's stream.  Nothing here allocates or synchronises: weights live
// in a caller-owned blob, activations in a caller-owned workspace carved by a deterministic first-fit arena (the same walk run "dry"
// yields r2dm_workspace_bytes).
#include "engine.h"

using namespace r2dm;

namespace {

const bool g_debug_sync = getenv("R2DM_DEBUG_SYNC") != nullptr;  // fault hunting: wait for and name every launch (read once)

inline Src src1(const Tensor& t) { return Src{t.p, nullptr, t.C, 0, t.bs(), 0}; }
inline Src src2(const Tensor& a, const Tensor& b) { return Src{a.p, b.p, a.C, b.C, a.bs(), b.bs()}; }

struct Ctx {
    r2dm_handle* h;
    Arena* ar;
    hipStream_t st;
    int B;
    const float* proj;  // [B][ada_rows]
    double* gn_partial;
    hipError_t err = hipSuccess;
    const char* where = "";
    int f2_launches = 0;  // conv_f16x2 launches of this forward so far (odd ones walk their tiles backwards: ConvParams::reverse)
    int last_reverse = -1;  // direction of the last conv_f16x2 launch (-1: none yet / another kernel)
    // the fp16 operand range guard, one slot per guarded producer ("site") of the forward, in walk order; `ctx`: which layer the walk is in
    int n_sites = 0;
    std::string ctx;
    // `keyed` (a handle that runs cached walks, and their listings): the site's index is the one its producer -- layer and what it records -- got when the table
    // first saw it, so that a shallow walk, which hands out fewer sites, raises the slots the full walk raises for the same layers
    std::vector<std::string>* keyed = nullptr;
    size_t key_hint = 1;  // (walks meet their sites in nearly the same order: the search starts behind the last hit)
    int* range_site(const char* what) {
        int k = 0;
        if (keyed) {
            std::vector<std::string>& v = *keyed;
            const std::string name = ctx.empty() ? std::string(what) : ctx + ": " + what;
            if (v.empty()) v.emplace_back();  // (slot 0: the shared one)
            for (size_t j = 0; j + 1 < v.size() && !k; ++j) {
                const size_t at = 1 + (key_hint - 1 + j) % (v.size() - 1);
                if (v[at] == name) k = (int)at;
            }
            if (!k && (int)v.size() < r2dm_handle::RANGE_SITES) {  // (beyond the table: the shared slot 0 -- still guarded, just not named)
                v.push_back(name);
                k = (int)v.size() - 1;
            }
            if (k) key_hint = (size_t)k + 1;
        } else {
            k = n_sites + 1 < r2dm_handle::RANGE_SITES ? ++n_sites : 0;  // (beyond the table: the shared slot 0 -- still guarded, just not named)
            if (!lst) {
                if ((int)h->site_names.size() <= k) h->site_names.resize(k + 1);
                h->site_names[k] = ctx.empty() ? std::string(what) : ctx + ": " + what;
            }
        }
        if (lst) pend += " site=" + std::to_string(k) + ":\"" + what + "\"";  // (the line already names the layer)
        return (int*)blob(h->range_flag) + 2 * k;
    }

    // ---- [listing> the listing (r2dm_forward_listing): with `lst` set the walk is dry, but builds every launch's parameters and writes a line where it would
    // enqueue; the handle stays as it was (site names, profiling state, cmap_ready)
    std::string* lst = nullptr;
    const void* user_out = nullptr;  // the caller's output tensor ("dst" in the listing)
    const void* cache_out = nullptr;  // a cached walk's feature tensor ("cache")
    std::string pend;                // range sites, profiling class and refusals noted since the last line
    bool skip() const { return dry() && !lst; }  // nothing to launch and nothing to list: only the allocations count
    // "layer | launch | out=<arena offset> [| a convolution's ConvParams: what fixes the kernel instantiation and its side effects; flags only where set] [| notes]"
    void list_line(const char* name, const void* out, const char* tag, const ConvParams* p) {
        static const char* const algos[] = {"F32", "BF16X3", "DIRECT", "F16X2", "P1F16"};
        char b[256];
        std::string& s = *lst;
        s += (ctx.empty() ? std::string("-") : ctx) + " | " + name + " | out=";
        if (tag) s += tag;
        else if (out == user_out) s += "dst";
        else if (out == cache_out) s += "cache";
        else s += std::to_string((size_t)((const char*)out - ar->base));
        if (p) {
            snprintf(b, sizeof(b), " | algo=%s tile=%dx%d pieces=%d pro=%d cin=%d/%d cout=%d taps=%d hw=%dx%d", algos[p->algo], p->co_tile, p->px_rows, p->pieces, p->prologue, p->Cin,
                     p->CinPad, p->Cout, p->taps, p->H, p->W);
            s += b;
            if (p->aff) s += " aff";
            if (p->gn_partial) s += " fold=" + std::to_string(p->gn_slots) + "/" + std::to_string(p->gn_stride);  // (slots read / slot stride)
            if (p->stat) s += " stat=" + std::to_string(p->stat_goff) + "/" + std::to_string(p->stat_cpg);        // (first group / channels per group)
            if (p->res) s += p->res_bs ? " res" : " res=bcast";
            if (p->scale) s += " scale";
            if (p->x16) s += " x16";
            if (p->y16) s += " y16";
            if (p->reverse) s += " rev";
            if (p->range) s += " range";
        }
        s += pend.empty() ? "" : " |" + pend;
        s += "\n";
        pend.clear();
    }
    // one launch: enqueued and noted, or (listing) written down; `out`: what it writes, `p`: a convolution's parameters
    template <class F>
    void run(const char* name, const void* out, F&& launch, const ConvParams* p = nullptr, const char* tag = nullptr) {
        if (lst) list_line(name, out, tag, p);
        else note(launch(), name);
    }
    // <listing] ----

    // (once the arena has handed out a pointer beyond the caller's workspace NOTHING more is launched -- the walk goes on
    // dry, so `peak` still comes out right for the error message -- instead of enqueueing kernels that write outside the workspace)
    bool dry() const { return ar->dry || ar->overflow; }
    void note(hipError_t e, const char* w) {
        if (lst) {  // (a refusal: it surfaces from a real forward only; the listing shows it on the launch's line)
            if (e != hipSuccess) pend += std::string(" refused=\"") + w + "\"";
            return;
        }
        if (g_debug_sync && e == hipSuccess && !dry()) {  // fault hunting: wait for and name every launch
            fprintf(stderr, "[r2dm] %s ...", w);
            fflush(stderr);
            e = hipStreamSynchronize(st);
            fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
        }
        if (e != hipSuccess && err == hipSuccess) {
            err = e;
            where = w;
        }
    }
    const float* blob(size_t off) const { return h->blob + off; }

    Tensor make(int C, int H, int W, bool f16 = false) {
        Tensor t{nullptr, C, H, W, f16};
        t.p = (float*)ar->alloc(t.bytes(B));
        return t;
    }
    // fp16 storage of EVERY activation of the two full-resolution levels (round 6; the one-plane mode = the reference's fp16 autocast, which stores its
    // activations as fp16: sample_and_save.py:45,70): those levels hold 92 % of a forward's activation bytes and their launches are the ones next
    // to the HBM roof; levels 3 and 4 (attention, 1 x 1 projections with residuals and statistics) stay fp32.  all16: decided once per forward (run_forward).
    bool all16 = false;
    bool lvl16(int Hres) const { return all16 && 2 * Hres >= h->cfg.height; }
    void drop(const Tensor& t) { ar->release(t.p); }

    // Fused statistics: a convolution whose output feeds a GroupNorm leaves per-(sample, group) partial sums in a
    // Sink from its epilogue; the GroupNorm then only runs the finalize kernel (no extra pass over the tensor).
    struct Sink {
        double* p = nullptr;
        int C = 0, cpg = 0, slots = 0;  // C: channels of the normalised (possibly concatenated) tensor
        bool incomplete = false;        // a producer could not emit its share: the consumer runs the streaming pass instead
        bool external = false;          // the slots live outside the arena (a cached walk's join: the feature cache)
        explicit operator bool() const { return p != nullptr && !incomplete; }
        int read_slots() const { return cpg < 64 ? slots / 2 : slots; }  // (groups of fewer than 64 channels leave the second half of their slots zero)
    };
    // `at`: the slots' place outside the arena (null: the arena's)
    Sink make_sink(int C_total, int H, int W, double* at = nullptr) {
        Sink k;
        const int G = h->cfg.gn_num_groups;
        int cpg;
        // the epilogue reduction (conv_epilogue.h) merges whole 8-channel blocks of ONE wave: groups must be 8, 16, 32 or
        // 64 channels so that they never straddle waves; anything else takes the separate streaming pass
        if (!sink_shape(h->cfg, C_total, &cpg)) return k;
        k.C = C_total;
        k.cpg = cpg;
        k.slots = conv_stat_slots(H, W);
        k.p = at ? at : (double*)ar->alloc((size_t)B * G * k.slots * 2 * sizeof(double));
        k.external = at != nullptr;
        return k;
    }
    void drop_sink(Sink& k) {
        if (k.p && !k.external) ar->release(k.p);
        k.p = nullptr;
    }
    float2* finalize(const Sink& k, int H, int W, const float* gamma, const float* beta, const float* ada) {
        float2* aff = (float2*)ar->alloc((size_t)B * k.C * sizeof(float2));
        if (!skip()) {
            GNParams g{Src{}, B, H, W, h->cfg.gn_num_groups, h->cfg.gn_eps, gamma, beta, ada, (long)h->ada_rows, k.p, aff,
                       nullptr};
            // (range guard of the fp16 consumers: the slot energies bound max|x| -- norm.hip; no separate maximum is recorded)
            if (h->f16_path()) g.range_flag = range_site("GroupNorm output bound |a| M + |d| (gn_finalize)");  // (only the fp16 operand paths have a range to guard)
            run("group_norm_finalize", aff, [&] { return launch_group_norm_finalize(g, k.C, k.slots, st); });
        }
        return aff;
    }
    // GroupNorm of `x`: from fused statistics when the producer left them, else with the streaming statistics pass
    float2* norm(const Sink& k, const Src& x, int H, int W, const float* gamma, const float* beta, const float* ada) {
        return k ? finalize(k, H, W, gamma, beta, ada) : group_norm(x, H, W, gamma, beta, ada);
    }

    float2* group_norm(const Src& x, int H, int W, const float* gamma, const float* beta, const float* ada) {
        const int C = x.c0 + x.c1;
        float2* aff = (float2*)ar->alloc((size_t)B * C * sizeof(float2));
        if (!skip()) {
            GNParams g{x, B, H, W, h->cfg.gn_num_groups, h->cfg.gn_eps, gamma, beta, ada, (long)h->ada_rows,
                       gn_partial, aff, nullptr};
            g.partial_max = (float*)(gn_partial + (size_t)B * h->cfg.gn_num_groups * 256 * 2);
            if (h->f16_path()) g.range_flag = range_site("GroupNorm output bound |a| max|x| + |d| (streaming statistics)");  // (only the fp16 operand paths have a range to guard)
            run("group_norm", aff, [&] { return launch_group_norm(g, st); });
        }
        return aff;
    }

    // The GroupNorm in front of a convolution: the statistics its producers left (or not: the streaming pass) and its parameters.
    // conv() with a NormSpec runs the norm itself -- folded into the convolution's staging waves where conv_f16x2.hip can do that (no
    // gn_finalize launch: 45 of the 50 GroupNorms of a forward at batch 8), else as the separate launch(es) in front of it.
    struct NormSpec {
        const Sink* stats;
        const float *gamma, *beta, *ada;
    };

    // in-stream timing of a launch: records the opening event and returns the closing one (nullptr: profiling off)
    hipEvent_t prof_begin(int cls, double flop) {
        if (lst) {
            pend += " class=" + std::to_string(cls);
            return nullptr;
        }
        if (!h->prof_on) return nullptr;
        if (h->prof_used + 2 > h->prof_ev.size()) {
            hipEvent_t a, c;
            if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&c) == hipSuccess) {
                h->prof_ev.push_back(a);
                h->prof_ev.push_back(c);
            }
        }
        if (h->prof_used + 2 > h->prof_ev.size()) return nullptr;
        hipEvent_t e0 = h->prof_ev[h->prof_used], e1 = h->prof_ev[h->prof_used + 1];
        h->prof_used += 2;
        h->prof_flop += flop;
        h->prof_cls.push_back(cls);
        h->prof_lflop.push_back(flop);
        (void)hipEventRecord(e0, st);
        return e1;
    }

    // what a convolution launch does beyond its layer, input and resolution
    struct ConvOpts {
        int prologue = PRO_NONE;
        const float2* aff = nullptr;     // (a, d) of the prologue's GroupNorm, unless `norm` gives it
        const NormSpec* norm = nullptr;  // `aff` comes from this GroupNorm (aff must be nullptr)
        const Tensor* res = nullptr;     // residual added to the output ...
        bool res_broadcast = false;      // ... one map for the whole batch
        const float* scale = nullptr;    // device scalar multiplied after the residual add
        float* dst = nullptr;            // the output goes here, not into a fresh tensor
        const Sink* sink = nullptr;      // fused statistics of the output, groups from `goff` on
        int goff = 0;
        bool input_bounded = false;      // its producer tracked max|x| in the range flag
        bool track_out = false;          // record max|y| there (the fp16 operand paths only)
        bool x16 = false, y16 = false;   // fp16 storage of the input / of the output (+ residual): act16(L) launches only
    };

    // What one convolution launch runs on and what it fuses.  choose() decides it from the layer's packings, the precision mode, the prologue, the guard on
    // the input's range, the incoming statistics, the batch and the resolution -- nothing the sizing walk does not know --, so both walks allocate alike;
    // conv() only carries it out.
    enum NormKind { NORM_NONE, NORM_FOLDED, NORM_FINALIZE, NORM_STREAMING };
    struct ConvChoice {
        int algo = ALGO_F32, co_tile = 0, px_rows = 4, pieces = 3;  // the kernel, its tile and its operand pieces
        // the GroupNorm in front: folded into the convolution's staging waves | the finalize launch over fused statistics | the streaming statistics pass
        // (the last two leave `aff` for the prologue)
        NormKind norm = NORM_NONE;
        bool fused_stats = false;      // the epilogue writes the output's statistics into ConvOpts::sink ...
        bool sink_incomplete = false;  // ... or cannot: the sink's consumer runs the streaming pass
        // range sites, in the order they are handed out: the folded GroupNorm's output bound (NORM_FOLDED), then ...
        bool track_out = false;        // ... max|output|
        const char* refused = nullptr;  // x16 / y16 asked of a launch that cannot take them: what a real forward reports
    };
    ConvChoice choose(const ConvLayer& L, int H, int W, const ConvOpts& o) const {
        ConvChoice c;
        // the fp16 split where the input's range is guarded: GroupNorm-normalised (gn_finalize's bound) or tracked by its producer (fir_up2's running maximum)
        const bool guarded = h->f16_path() && (o.prologue != PRO_NONE || o.input_bounded);
        c.algo = L.f2 && guarded ? ALGO_F16X2 : L.p1 && guarded && o.prologue != PRO_AFFINE_SILU ? ALGO_P1F16 : L.algo;
        c.co_tile = c.algo == ALGO_F16X2 ? L.f2_cot : c.algo == ALGO_P1F16 ? 64 : L.co_tile;
        if (c.algo == ALGO_F16X2) c.px_rows = L.f2_rows;
        if (c.algo == ALGO_F16X2 || c.algo == ALGO_P1F16) c.pieces = (c.algo == ALGO_F16X2 && L.f2_cot == 32 && narrow_split()) ? 2 : h->conv_pieces;
        if (const NormSpec* ns = o.norm) {
            const Sink& k = *ns->stats;
            const int G = h->cfg.gn_num_groups;
            c.norm = k ? NORM_FINALIZE : NORM_STREAMING;
            if (k && c.algo == ALGO_F16X2 && k.C == L.cin && G == 8) {
                ConvParams q;
                q.Cin = L.cin; q.Cout = L.cout; q.taps = L.taps; q.H = H; q.W = W; q.co_tile = L.f2_cot; q.px_rows = L.f2_rows; q.B = B; q.prologue = o.prologue;
                bool fold = true;  // (whichever direction this launch will walk its tiles in: that is the walk's state, not the choice's)
                for (q.reverse = 0; q.reverse < 2; ++q.reverse) fold = fold && conv_f16x2_fold_supported(q, G, k.read_slots());
                if (fold) c.norm = NORM_FOLDED;
            }
        }
        // (the layer's own kernel decides, whichever packing runs: conv_f16x2 and proj_f16x2 write what the kernel they stand in for writes)
        c.fused_stats = o.sink && o.sink->p && conv_emits_stats(L.algo, L.co_tile, L.cout);
        c.sink_incomplete = o.sink && o.sink->p && !c.fused_stats;
        // (every MFMA kernel records the maximum; the direct kernels' outputs never feed an fp16 operand unnormalised)
        c.track_out = o.track_out && h->f16_path() && c.algo != ALGO_DIRECT;
        // (conv_f16x2 launches, the direct in / out convolutions and the fp16-operand skip convolutions take fp16 storage; the streaming statistics pass reads fp32)
        if ((o.x16 || o.y16) && c.algo != ALGO_F16X2 && c.algo != ALGO_DIRECT && c.algo != ALGO_P1F16) c.refused = "fp16 storage on a kernel without it";
        else if (o.x16 && c.norm == NORM_STREAMING) c.refused = "fp16 storage behind a streaming GroupNorm";
        return c;
    }

    Tensor conv(const ConvLayer& L, const Src& x, int H, int W, const ConvOpts& o) {
        const ConvChoice c = choose(L, H, W, o);
        const NormSpec* ns = o.norm;
        const float2* aff = o.aff;
        float2* own_aff = nullptr;
        if (c.norm == NORM_FINALIZE) aff = own_aff = finalize(*ns->stats, H, W, ns->gamma, ns->beta, ns->ada);
        if (c.norm == NORM_STREAMING) aff = own_aff = group_norm(x, H, W, ns->gamma, ns->beta, ns->ada);
        Tensor y{o.dst, L.cout, H, W, o.y16};
        if (!y.p) y.p = (float*)ar->alloc(y.bytes(B));
        if (c.sink_incomplete) const_cast<Sink*>(o.sink)->incomplete = true;
        if (!skip()) {
            ConvParams p = conv_params(x, blob(L.w), blob(L.b), y.p, y.bs(), B, H, W, L.cin, L.cin_pad, L.cout, L.taps, c.co_tile, c.algo, o.prologue);
            p.px_rows = c.px_rows;
            p.pieces = c.pieces;
            p.aff = aff;
            p.res = o.res ? o.res->p : nullptr;
            p.res_bs = o.res && !o.res_broadcast ? o.res->bs() : 0;
            p.scale = o.scale;
            p.x16 = o.x16;
            p.y16 = o.y16;
            if (c.algo == ALGO_F16X2) {
                p.reverse = f2_launches++ & 1;
                last_reverse = p.reverse;
                p.w = blob(L.w_f2);
                p.wscale = blob(L.ws_f2) + 1;
            } else if (c.algo == ALGO_P1F16) {
                // (a skip convolution reads the tensor its block's conv1 has just read: start where that walk ended)
                p.reverse = last_reverse == 0;
                p.w = blob(L.w_p1);
                p.wscale = blob(L.ws_p1) + 1;
            }
            if (c.norm == NORM_FOLDED) {
                const Sink& k = *ns->stats;
                p.gn_partial = k.p;
                p.gn_stride = k.slots;
                p.gn_slots = k.read_slots();
                p.gn_cpg = k.cpg;
                p.gn_eps = h->cfg.gn_eps;
                p.gn_gamma = ns->gamma;
                p.gn_beta = ns->beta;
                p.gn_ada = ns->ada;
                p.gn_ada_stride = (long)h->ada_rows;
                p.gn_range = range_site("GroupNorm output bound |a| M + |d| (folded into the convolution)");
            }
            if (c.track_out) p.range = range_site("max|output| (raw input of the next fp16-operand kernel)");
            if (c.fused_stats) conv_stat_sink(p, o.sink->p, h->cfg.gn_num_groups, o.goff, o.sink->cpg, o.sink->slots);
            if (c.refused) note(hipErrorInvalidValue, c.refused);
            // ALGORITHMIC flops of the reference's convolution (in_conv: all 34 input channels, although the
            // constant Fourier half is folded into a bias map here)
            hipEvent_t e1 = prof_begin(p.algo == ALGO_F16X2 ? 0 : p.algo == ALGO_BF16X3 ? 1 : 2, 2.0 * B * (double)L.cout * (L.src_cin ? L.src_cin : L.cin) * L.taps * H * W);
            if (g_debug_sync && !lst)
                fprintf(stderr, "[r2dm] conv algo %d %d->%d taps %d co_tile %d %dx%d B %d pro %d w %p bias %p gn %p blob [%p, +%zu) x %p/%p (c0 %d) y %p res %p aff %p stat %p ws [%p, +%zu)\n", p.algo, p.Cin,
                        p.Cout, p.taps, p.co_tile, H, W, B, o.prologue, (const void*)p.w, (const void*)p.bias, (const void*)p.gn_partial, (void*)h->blob, h->blob_floats * 4, (const void*)p.x.p0, (const void*)p.x.p1, p.x.c0, (void*)p.y, (const void*)p.res, (const void*)p.aff,
                        (void*)p.stat, (void*)ar->base, ar->cap);
            run("conv", y.p, [&] { return launch_conv(p, st); }, &p);
            if (e1) (void)hipEventRecord(e1, st);
        }
        if (own_aff) ar->release(own_aff);
        return y;
    }

    // efficient_unet.py:95-110.  `in_stats`: fused statistics of x (if its producer left them);
    // `out` / `out_goff`: where the statistics of this block's output go (the next GroupNorm's sink).
    // fp16 storage (round 5): in the one-plane mode (the reference's autocast counterpart) the tensor between a residual block's two
    // convolutions is stored as fp16 -- what autocast stores there (sample_and_save.py:45,70) -- when both run on
    // conv_f16x2 (R2DM_FP16_STORAGE=0: fp32 everywhere, as until round 4)
    bool act16(const ConvLayer& L) const {
        static const bool on = !getenv("R2DM_FP16_STORAGE") || atoi(getenv("R2DM_FP16_STORAGE")) != 0;
        return on && h->conv_pieces == 1 && L.f2 && !(L.f2_cot == 32 && narrow_split());
    }
    // (experiment switch, round 5) layers packed for the 32-channel tile run the two-plane kernel in every precision mode
    static bool narrow_split() {
        static const bool on = getenv("R2DM_F2_NARROW_SPLIT") && atoi(getenv("R2DM_F2_NARROW_SPLIT")) != 0;
        return on;
    }

    struct BlockOpts {
        bool track_out = false;     // the block's last convolution records max|output| in the range flag
        bool skip_bounded = false;  // every producer of the block's input has done so: the skip convolution may take the fp16 operand path
        bool x16 = false;           // the block's input (both sources) is stored as fp16
    };
    Tensor residual_block(const ResLayer& r, const Src& x, int H, int W, const Sink& in_stats, const Sink* out, int out_goff, const BlockOpts& bo) {
        const std::string blk = ctx;
        ctx = blk + ".conv1";
        const NormSpec n1{&in_stats, blob(r.g1), blob(r.b1), nullptr};
        Sink s1 = make_sink(r.cout, H, W);
        const bool t1_16 = act16(r.conv1) && act16(r.conv2) && s1.p != nullptr;  // (the streaming statistics pass reads fp32)
        const bool out16 = bo.x16 && lvl16(H) && act16(r.conv2);  // the block's output (and the residual it adds: its input or the skip convolution's output)
        ConvOpts c1;
        c1.prologue = PRO_AFFINE_SILU;
        c1.norm = &n1;
        c1.sink = &s1;
        c1.x16 = bo.x16;
        c1.y16 = t1_16;
        Tensor t1 = conv(r.conv1, x, H, W, c1);
        const NormSpec n2{&s1, nullptr, nullptr, proj + r.ada_row};
        Tensor skip;
        const Tensor ident{const_cast<float*>(x.p0), x.c0, H, W};  // identity skip: the block input is single-source then
        const Tensor* res = &ident;
        if (r.has_skip) {
            ctx = blk + ".skip";
            ConvOpts cs;
            cs.input_bounded = bo.skip_bounded;
            cs.x16 = bo.x16;
            cs.y16 = out16;
            skip = conv(r.skip, x, H, W, cs);
            res = &skip;
        }
        ctx = blk + ".conv2";
        ConvOpts c2;
        c2.prologue = PRO_AFFINE_SILU;
        c2.norm = &n2;
        c2.res = res;
        c2.scale = blob(r.scale);
        c2.sink = out;
        c2.goff = out_goff;
        c2.track_out = bo.track_out;
        c2.x16 = t1_16;
        c2.y16 = out16;
        Tensor o = conv(r.conv2, src1(t1), H, W, c2);
        ctx = blk;
        drop_sink(s1);
        drop(t1);
        if (r.has_skip) drop(skip);
        return o;
    }

    // efficient_unet.py:42-53
    struct AttnOpts {
        bool track_out = false;  // the output projection records max|output| in the range flag
    };
    Tensor attention_block(const AttnLayer& a, const Tensor& x, const Sink& in_stats, const Sink* out, int out_goff, const AttnOpts& ao) {
        const std::string blk = ctx;
        ctx = blk + ".norm";
        float2* aff = norm(in_stats, src1(x), x.H, x.W, blob(a.gamma), blob(a.beta), nullptr);
        ctx = blk + ".qkv";
        // precision mode 2: the attention core runs on the fp16 matrix pipe (attention.hip) and needs |q|, |k|, |v| < 65504: the
        // projection's epilogue records max|qkv| in the range flag
        const bool f2 = h->f16_path();
        ConvOpts cq;
        cq.prologue = PRO_AFFINE;
        cq.aff = aff;
        cq.track_out = f2;
        Tensor qkv = conv(a.qkv, src1(x), x.H, x.W, cq);
        ar->release(aff);
        Tensor o = make(a.C, x.H, x.W);
        if (!skip()) run("attention", o.p, [&] { return launch_attention(qkv.p, o.p, B, a.C, h->cfg.attn_num_heads, x.H * x.W, st, f2 ? h->conv_pieces : 0); });
        drop(qkv);
        // (the core's output is a convex combination of v: |o| <= max|qkv|, which the qkv epilogue has recorded)
        ctx = blk + ".out_proj";
        ConvOpts cp;
        cp.res = &x;
        cp.scale = blob(a.scale);
        cp.sink = out;
        cp.goff = out_goff;
        cp.input_bounded = f2;
        cp.track_out = ao.track_out;
        Tensor y = conv(a.proj, src1(o), x.H, x.W, cp);
        ctx = blk;
        drop(o);
        return y;
    }

    // efficient_unet.py:178-185.  Never frees `in`; returns a fresh tensor.  `in_stats`: fused statistics of `in` for
    // the first residual block (stages without downsampling); `out`/`out_goff`: sink of the GroupNorm that will consume
    // this stage's output (written by whichever convolution produces it last).
    struct StageIn {
        bool tracked = false;  // the input's producer recorded max|x| in the range flag
        bool f16 = false;      // the input is stored as fp16
        // a cached walk's store: the up-sampling convolution writes the stage's output here, and `*twin` takes the arena block the output would have had --
        // allocated all the same, so that every later tensor keeps the offset the plain forward gives it
        float* out_dst = nullptr;
        void** twin = nullptr;
    };
    Tensor stage(const Stage& s, const Src& in, int H, int W, const Sink& in_stats, const Sink* out, int out_goff, const StageIn& si) {
        Tensor cur;
        bool have = false;
        bool c16 = si.f16;  // the current tensor (stage input or `cur`) is stored as fp16
        Sink carry = in_stats;  // statistics of the current tensor, owned elsewhere for the stage input
        bool carry_owned = false;
        // FIR first, then the stride-2 convolution as a GEMM over the nine filtered planes (resample.hip): a quarter of the MACs of conv + fir_down2.  The
        // planes are stored once each (down_planes_phase_kernel: two column phases x 2 Ho + 3 rows, about 1.0 x the input instead of 2.25 x) unless
        // R2DM_DOWN_GEMM=9 asks for all nine (down_planes_kernel); the GEMM's loader maps the taps, the product is the same bits.  Taken where the plan packed the matrix (geometry, R2DM_DOWN_GEMM), the precision is the default three-product split and
        // the input's producer tracks max|x|; everything else -- fp32-bf16x3, the one-plane mode with its fp16 storage, a tripped guard's fallback --
        // keeps conv + FIR.  Leaves what the FIR launch leaves: the tensor and, where fir_down2 would, the statistics of the first block's norm.
        // (a two-source input never reaches a down stage today; if one does it keeps conv + FIR: the pre-pass reads one tensor)
        if (s.down) {
            ctx = s.name + ".downsample";
            const ConvLayer& L = s.dconv;
            const bool gemm = L.dg && h->conv_pieces == 2 && si.tracked && !si.f16 && !in.p1, phase = h->down_gemm != 9;
            Tensor t;  // what the stage's second launch reads: the FIR planes (phase planes: 2 cin channels of (H + 3) x (W / 2 + 4)) | the convolution's output
            if (gemm) {
                t = phase ? make(2 * L.cin, H + 3, W / 2 + 4) : make(9 * L.cin, H / 2, W / 2);
            } else {
                ConvOpts cd;
                cd.input_bounded = si.tracked;
                cd.x16 = si.f16;
                cd.y16 = si.f16 && lvl16(H);
                t = conv(L, in, H, W, cd);
            }
            cur = make(s.cout, H / 2, W / 2, t.f16 && lvl16(H / 2));
            // the FIR pass / the GEMM leaves the statistics of its output for the first residual block's norm (resample.hip; where the geometry
            // does not fit the slot grid: no fused statistics, the streaming pass)
            Sink fs;
            if (fir_down2_stat_slots(s.cout, h->cfg.gn_num_groups, H, W)) fs = make_sink(s.cout, H / 2, W / 2);
            if (gemm && !skip()) {
                // Range: the FIR weights are non-negative and sum to at most 1 per axis, so max|a| <= max|x|, which the producer has recorded at its own site;
                // the pass records max|a| itself all the same (one guarded atomic per wave), so the report names the GEMM's operand.
                // (profiling: both launches in class 2, "1x1 / in / out convolutions" -- the pass with no FLOPs of its own, the GEMM with those it executes)
                int* site = range_site(phase ? "max|FIR planes| (operand of the down-sampling GEMM, every distinct plane once)"
                                             : "max|FIR planes| (operand of the down-sampling GEMM, all nine)");
                hipEvent_t e0 = prof_begin(2, 0.0);
                if (phase) run("down_phase_planes", t.p, [&] { return launch_down_phase_planes(in.p0, in.bs0, t.p, t.bs(), B, L.cin, H, W, st, site); });
                else run("down_planes", t.p, [&] { return launch_down_planes(in.p0, in.bs0, t.p, t.bs(), B, L.cin, H, W, st, site); });
                if (e0) (void)hipEventRecord(e0, st);
                const ConvParams p = down_gemm_params(t.p, blob(L.w_dg), blob(L.b), blob(L.ws_dg) + 1, cur.p, B, L.cin, L.cout, H / 2, W / 2, fs.p, h->cfg.gn_num_groups, phase);
                last_reverse = -1;
                hipEvent_t e1 = prof_begin(2, 2.0 * B * (double)L.cout * 9 * L.cin * (H / 2) * (W / 2));
                run("down_gemm", cur.p, [&] { return launch_proj_f16x2(p, st, phase ? DOWN_PHASE : DOWN_NINE); }, &p);
                if (e1) (void)hipEventRecord(e1, st);
            } else if (!skip()) {
                run("fir_down2", cur.p, [&] { return launch_fir_down2(t.p, t.bs(), cur.p, cur.bs(), B, s.cout, H, W, st, fs.p, h->cfg.gn_num_groups, t.f16, cur.f16); });
            }
            c16 = cur.f16;
            drop(t);
            H /= 2;
            W /= 2;
            have = true;
            carry = fs;
            carry_owned = fs.p != nullptr;
        }
        const int n = (int)s.res.size();
        for (int i = 0; i < n; ++i) {
            const bool last = i == n - 1;
            Sink next;  // sink for the GroupNorm that consumes this block's output inside the stage
            const Sink* dst = nullptr;
            int goff = 0;
            if (!last || s.attn) {
                next = make_sink(s.cout, H, W);
                dst = &next;
            } else if (!s.up) {
                dst = out;
                goff = out_goff;
            }
            BlockOpts bo;
            bo.track_out = h->f16_path() && last && ((s.out_tracked) || (s.track_final && !s.attn && !s.up));
            bo.skip_bounded = i == 0 && s.skip_in_bounded && h->f16_path();
            bo.x16 = c16;
            ctx = s.name + ".residual_blocks." + std::to_string(i);
            Tensor nxt = residual_block(s.res[i], have ? src1(cur) : in, H, W, carry, dst, goff, bo);
            c16 = nxt.f16;
            if (carry_owned) drop_sink(carry);
            if (have) drop(cur);
            cur = nxt;
            have = true;
            carry = next;
            carry_owned = next.p != nullptr;
        }
        if (s.attn) {
            ctx = s.name + ".self_attn_block";
            if (cur.f16) note(hipErrorInvalidValue, "attention block behind fp16 storage");
            AttnOpts ao;
            ao.track_out = s.track_final && !s.up && h->f16_path();
            Tensor nxt = attention_block(s.at, cur, carry, s.up ? nullptr : out, out_goff, ao);
            if (carry_owned) drop_sink(carry);
            carry_owned = false;
            drop(cur);
            cur = nxt;
        }
        if (carry_owned) drop_sink(carry);
        if (s.up) {
            Tensor u = make(s.cout, 2 * H, 2 * W, lvl16(2 * H) && s.uconv.f2);
            const bool track = s.uconv.f2 && h->f16_path();  // the fp16-operand convolution below needs max|u| < 65504
            ctx = s.name + ".upsample";
            if (!skip()) {
                int* site = track ? range_site("max|FIR output| (raw input of the up-sampling convolution)") : nullptr;
                run("fir_up2", u.p, [&] { return launch_fir_up2(cur.p, cur.bs(), u.p, u.bs(), B, s.cout, H, W, st, site, cur.f16, u.f16); });
            }
            drop(cur);
            ConvOpts cu;
            cu.sink = out;
            cu.goff = out_goff;
            cu.input_bounded = track;
            cu.track_out = s.track_final && h->f16_path();
            cu.x16 = cu.y16 = u.f16;
            if (si.out_dst) {
                *si.twin = ar->alloc(Tensor{nullptr, s.uconv.cout, 2 * H, 2 * W, u.f16}.bytes(B));
                cu.dst = si.out_dst;
            }
            cur = conv(s.uconv, src1(u), 2 * H, 2 * W, cu);
            drop(u);
        }
        return cur;
    }
};

}  // namespace

int r2dm::run_forward(r2dm_handle* h, Arena& ar, const float* x, const float* cond, float* out, int B, hipStream_t st, std::string* listing, const CacheWalk* cw,
                      std::vector<std::string>* keyed) {
    const r2dm_config& c = h->cfg;
    Ctx k{h, &ar, st, B, nullptr, nullptr};
    k.lst = listing;
    k.user_out = out;
    k.keyed = keyed ? keyed : h->sites_keyed && !listing ? &h->site_names : nullptr;
    const int H = c.height, W = c.width, T = c.temb_channels;
    float* act = (float*)ar.alloc((size_t)2 * B * T * sizeof(float));  // [SiLU(temb) | hidden scratch]
    float* proj = (float*)ar.alloc((size_t)B * h->ada_rows * sizeof(float));
    k.gn_partial = (double*)ar.alloc((size_t)B * c.gn_num_groups * 256 * (2 * sizeof(double) + sizeof(float)));  // sums | maxima
    k.proj = proj;
    if (!k.skip()) {
        EmbedParams e{cond, k.blob(h->freqs), k.blob(h->w1), k.blob(h->b1), k.blob(h->w2), k.blob(h->b2), act,
                      act + (size_t)B * T, B, c.base_channels, T};
        k.run("time_embedding", act, [&] { return launch_time_embedding(e, st); });
        k.run("ada_proj", proj, [&] { return launch_ada_proj(act, k.blob(h->ada_w), k.blob(h->ada_b), proj, B, T, h->ada_rows, st); });
    }
    // input = cat([x, cenc]) (efficient_unet.py:278-281), never materialised: the constant cenc half of in_conv is the
    // per-pixel bias map `cmap`, the per-step convolution runs over the in_channels data channels only
    Src in{x, nullptr, c.in_channels, 0, (long)c.in_channels * H * W, 0};
    if (c.coord_channels && (listing || (!h->cmap_ready && !k.dry()))) {  // (the listing shows it whether or not this handle has run it yet)
        const ConvLayer& L = h->in_conv_c;
        const ConvParams q = conv_params(Src{k.blob(h->cenc), nullptr, c.coord_channels, 0, 0, 0}, k.blob(L.w), k.blob(L.b), h->blob + h->cmap, 0, 1, H, W, L.cin, L.cin_pad, L.cout, 9,
                                         L.co_tile, ALGO_F32, PRO_NONE);
        if (!listing) k.note(hipMemsetAsync(h->blob + h->zero_bias, 0, h->in_conv.cout * sizeof(float), st), "zero bias");
        k.run("in_conv constant map", nullptr, [&] { return launch_conv(q, st); }, &q, "cmap (first forward after a bind only)");
        if (!listing) h->cmap_ready = true;
    }
    const Tensor cmap_t{h->blob + h->cmap, h->in_conv.cout, H, W};
    const int G = c.gn_num_groups;
    const Stage* S = h->stages;
    // GroupNorm sinks that outlive a stage: the first norm of d_block1 (input = in_conv output) and the first norm of
    // every up stage (input = cat([up-path tensor, skip tensor]): groups [0, G/2) come from the up path, [G/2, G)
    // from the skip tensor produced much earlier on the down path).
    // A cached walk (r2dm_unet_forward_cached) at depth d stops at join d, the first norm of up stage 8 - d: its store is this walk with stage 7 - d's output
    // and the join's sink in the feature cache; its reuse runs stages [0, d) and [8 - d, 8) only and reads both from there.  A convolution writes its own
    // groups' slots and no others (conv_epilogue.h: written, not accumulated), so the cached half [0, G/2) stays put while every forward rewrites [G/2, G).
    const int depth = cw ? cw->depth : 0;
    const bool store = cw && cw->mode == 1, reuse = cw && cw->mode == 2;
    const bool run2 = !reuse || depth >= 2, run3 = !reuse || depth >= 3, run4 = !reuse;  // levels 2, 3 and 4 (with the up stage that returns from each)
    CacheLayout cl;
    if (cw) cl = cache_layout(h, B, depth);
    char* const cbuf = cw ? (char*)cw->buf : nullptr;
    k.cache_out = cbuf;
    void* sink_twin = nullptr;  // (store: the arena block the join's sink would have had -- kept, so that every offset stays the plain forward's)
    auto join_sink = [&](int j) {
        if (reuse && j > depth) return Ctx::Sink{};  // (neither written nor read)
        double* const at = cw && j == depth ? (double*)(cbuf + cl.sink_off) : nullptr;
        Ctx::Sink s = k.make_sink(S[8 - j].cin, H >> (j - 1), W >> (j - 1), reuse ? at : nullptr);
        if (store && at && s.p) {
            sink_twin = s.p;
            s.p = at;
            s.external = true;
        }
        // (reuse: the cached half's producer does not run; where it could not emit its share the store's consumer took the streaming pass, and so does this one)
        const ConvLayer& up = S[7 - depth].uconv;
        if (reuse && at && s.p && !conv_emits_stats(up.algo, up.co_tile, up.cout)) s.incomplete = true;
        return s;
    };
    auto drop_join = [&](int j, Ctx::Sink& s) {
        if (store && j == depth && sink_twin) ar.release(sink_twin);
        k.drop_sink(s);
    };
    Ctx::Sink s_d1 = k.make_sink(S[0].cin, H, W);
    Ctx::Sink s_u1 = join_sink(1);
    Ctx::Sink s_u2 = join_sink(2);
    Ctx::Sink s_u3 = join_sink(3);
    Ctx::Sink s_u4 = join_sink(4);
    {
        // fp16 storage of the full-resolution levels (Ctx::lvl16): the one-plane mode, the default network family (every GroupNorm of levels 1 and 2 on fused
        // statistics -- the streaming pass reads fp32 --, in_conv on the few-input kernel, FIR statistics at both levels).  R2DM_FP16_STORAGE=1: only between a
        // residual block's two convolutions (round 5); 0: nowhere.  Read per forward like R2DM_GN_FOLD (ws_cache: r2dm_set_conv_pieces clears it; tests build one
        // model per setting).
        const char* e = getenv("R2DM_FP16_STORAGE");
        const int level = e ? atoi(e) : 2;
        // ... and a plan whose levels 1 and 2 can all store it (r2dm_handle::plan_fits16, build_plan), FIR statistics at both levels (R2DM_FIR_STATS: read per call)
        k.all16 = level >= 2 && h->conv_pieces == 1 && h->plan_fits16 && fir_down2_stat_slots(S[1].cout, G, H, W) != 0 && fir_down2_stat_slots(S[2].cout, G, H / 2, W / 2) != 0;
    }
    k.ctx = "in_conv";
    Ctx::ConvOpts ci;
    ci.res = c.coord_channels ? &cmap_t : nullptr;
    ci.res_broadcast = true;
    ci.sink = &s_d1;
    ci.y16 = k.lvl16(H) && s_d1.p != nullptr;
    Tensor h0 = k.conv(h->in_conv, in, H, W, ci);
    Ctx::StageIn i0, i1, i2, i3, i4, i5, i6, i7;  // (stages 4 and 5 read untracked fp32 tensors)
    // the cached tensor: stage 7 - depth's output, stored as that stage stores it
    const Tensor cached{(float*)cbuf, cl.C, cl.H, cl.W, cw && k.lvl16(cl.H) && S[7 - depth].uconv.f2};
    void* feat_twin = nullptr;
    // before / after the stage that produces join j's up-path half, and when its consumer is through with it
    auto produce = [&](int j, Ctx::StageIn& si) {
        if (store && j == depth && !cw->drift) {
            si.out_dst = cached.p;
            si.twin = &feat_twin;
        }
    };
    auto produced = [&](int j, const Tensor& t) {
        if (!(store && j == depth && cw->drift) || k.skip()) return;
        if (t.f16 != cached.f16 || t.bs() != cached.bs()) k.note(hipErrorInvalidValue, "feature cache: the stage's output is not what the cache was laid out for");
        k.ctx = "cache";
        k.run("cache_store", cached.p, [&] { return launch_cache_store(t.p, cached.p, B, t.bs(), t.f16, (double*)(cbuf + cl.partial_off), cw->drift, st); }, nullptr, "cache");
    };
    auto consumed = [&](int j, const Tensor& t) {
        if (cw && j == depth && t.p == cached.p) {
            if (feat_twin) ar.release(feat_twin);
        } else
            k.drop(t);
    };
    i0.f16 = h0.f16;
    Tensor h1 = k.stage(S[0], src1(h0), H, W, s_d1, &s_u1, G / 2, i0);
    k.drop(h0);
    k.drop_sink(s_d1);
    Tensor h2, h3, u, u3, u2;
    if (run2) {
        i1.tracked = S[0].out_tracked && h->f16_path();
        i1.f16 = h1.f16;
        h2 = k.stage(S[1], src1(h1), H, W, Ctx::Sink{}, &s_u2, G / 2, i1);
    }
    if (run3) {
        i2.tracked = S[1].out_tracked && h->f16_path();
        i2.f16 = h2.f16;
        h3 = k.stage(S[2], src1(h2), H / 2, W / 2, Ctx::Sink{}, &s_u3, G / 2, i2);
    }
    if (run4) {
        i3.tracked = S[2].out_tracked && h->f16_path();
        Tensor h4 = k.stage(S[3], src1(h3), H / 4, W / 4, Ctx::Sink{}, &s_u4, 0, i3);
        produce(3, i4);
        u = k.stage(S[4], src1(h4), H / 8, W / 8, s_u4, &s_u3, 0, i4);
        k.drop(h4);
        k.drop_sink(s_u4);
        produced(3, u);
    } else if (depth == 3)
        u = cached;
    if (run3) {
        produce(2, i5);
        u3 = k.stage(S[5], src2(u, h3), H / 4, W / 4, s_u3, &s_u2, 0, i5);
        consumed(3, u);
        k.drop(h3);
        drop_join(3, s_u3);
        produced(2, u3);
    } else if (depth == 2)
        u3 = cached;
    if (run2) {
        if (u3.f16 != h2.f16 || h3.f16) k.note(hipErrorInvalidValue, "fp16 storage: the two halves of a skip join differ");
        i6.f16 = u3.f16 && h2.f16;
        produce(1, i6);
        u2 = k.stage(S[6], src2(u3, h2), H / 2, W / 2, s_u2, &s_u1, 0, i6);
        consumed(2, u3);
        k.drop(h2);
        drop_join(2, s_u2);
        produced(1, u2);
    } else
        u2 = cached;
    if (u2.f16 != h1.f16) k.note(hipErrorInvalidValue, "fp16 storage: the two halves of a skip join differ");
    i7.f16 = u2.f16 && h1.f16;
    Tensor u1 = k.stage(S[7], src2(u2, h1), H, W, s_u1, nullptr, 0, i7);
    consumed(1, u2);
    k.drop(h1);
    drop_join(1, s_u1);
    k.ctx = "out_conv";
    Ctx::ConvOpts co;
    co.dst = out;
    co.x16 = u1.f16;
    k.conv(h->out_conv, src1(u1), H, W, co);
    k.drop(u1);
    ar.release(act);
    ar.release(proj);
    ar.release(k.gn_partial);
    if (k.err != hipSuccess) return fail(2, "kernel launch failed in %s: %s", k.where, hipGetErrorString(k.err));
    if (ar.overflow) return fail(3, "workspace too small: need %zu bytes", ar.peak);
    return 0;
}
