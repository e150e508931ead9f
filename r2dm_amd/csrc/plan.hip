// The execution plan: which packings every layer of the U-Net gets (chosen from the planned geometry and batch alone) and where they and
// the raw parameters live in the caller-owned weight blob.  The tensor table (r2dm_tensor_at) and the layout hash are views of it.
#include "engine.h"

using namespace r2dm;

// ---- blob space ------------------------------------------------------------------------------
size_t r2dm_handle::take(size_t floats) {
    const size_t off = blob_floats;
    blob_floats += align_up(floats * sizeof(float)) / sizeof(float);
    return off;
}
size_t r2dm_handle::raw(const std::string& key, int64_t numel) {
    const size_t off = take(numel);
    slots.push_back({key, numel, SLOT_RAW, off, {}});
    return off;
}
void r2dm_handle::raw_at(const std::string& key, int64_t numel, size_t off) { slots.push_back({key, numel, SLOT_RAW, off, {}}); }
// the weight-only half of a convolution whose source tensor is shared with another layer (no bias slot)
// few_in: the slice runs at (H, W) with few input channels -- the direct kernel if the shape fits (conv_direct.hip)
ConvLayer r2dm_handle::conv_slice(const std::string& wkey, int src_cin, int src_off, int cin, int cout, int ksize, long px_batch, int H, int W) {
    ConvLayer L;
    L.cin = cin;
    L.cout = cout;
    L.taps = ksize * ksize;
    static const bool force_f32 = [] {
        const char* e = getenv("R2DM_CONV_ALGO");
        return e && e[0] == 'f';
    }();
    L.algo = (!force_f32 && H > 0 && conv_few_in_supported(cin, cout, L.taps, H, W)) ? ALGO_DIRECT : ALGO_F32;
    L.co_tile = conv_base_co_tile(L.algo, cin, cout, L.taps, px_batch);
    L.cin_pad = conv_base_cin_pad(L.algo, cin, L.taps, L.co_tile);
    L.src_cin = src_cin;
    L.src_off = src_off;
    L.w = take(L.packed_elems());
    slots.push_back({wkey, (int64_t)cout * src_cin * L.taps, SLOT_CONV, L.w, L});
    return L;
}
// H, W > 0: a convolution behind a GroupNorm at that resolution -- gets the ALGO_F16X2 packing too if the shape fits
// down: a stage's down-sampling convolution (followed by fir_down2) -- gets the down-sampling GEMM's packing too if the geometry fits its tiles
ConvLayer r2dm_handle::conv(const std::string& wkey, const std::string& bkey, int cin, int cout, int ksize, long px_batch, int H, int W, bool down) {
    ConvLayer L;
    L.cin = cin;
    L.cout = cout;
    L.taps = ksize * ksize;
    L.algo = conv_pick_algo(cin, cout, L.taps);
    L.co_tile = conv_base_co_tile(L.algo, cin, cout, L.taps, px_batch);
    L.cin_pad = conv_base_cin_pad(L.algo, cin, L.taps, L.co_tile);
    L.w = take(L.packed_elems());
    // (at least half a wave of tiles per CU at the planned batch: below that the persistent kernel leaves CUs idle)
    constexpr long f2_min_tiles = 128;
    if (L.algo == ALGO_BF16X3 && H > 0 && conv_f16x2_supported(cin, cout, L.taps, H, W) && (px_batch / 256) * (cout / 64) >= f2_min_tiles) {
        L.f2 = true;
        L.f2_cot = conv_f16x2_pick_co_tile(cin, cout, H, W, px_batch, &L.f2_rows);
        L.w_f2 = take((size_t)conv_f16x2_packed_floats(cin, cout));
        L.ws_f2 = take(2);
    }
    if (L.algo == ALGO_F32 && H > 0 && proj_f16x2_supported(cin, cout, L.taps, H, W)) {
        L.p1 = true;
        L.w_p1 = take((size_t)proj_f16x2_packed_floats(cin, cout));
        L.ws_p1 = take(2);
    }
    // (from the planned geometry alone, never from a call's batch: a sample's bits must not depend on the batch it is part of)
    if (down && down_gemm && L.taps == 9 && H > 0 && down_planes_supported(H, W) && proj_f16x2_supported(9 * cin, cout, 1, H / 2, W / 2)) {
        L.dg = true;
        L.w_dg = take((size_t)proj_f16x2_packed_floats(9 * cin, cout));
        L.ws_dg = take(2);
    }
    slots.push_back({wkey, (int64_t)cout * cin * L.taps, SLOT_CONV, L.w, L});
    L.b = raw(bkey, cout);
    return L;
}
namespace r2dm {

// The mechanical part of a layer's own (first) packing, shared by the plan and the single-kernel entries: the output-channel tile of the kernel `algo` names, the
// input-channel padding only the fp32-MFMA packing has, and which of those kernels write fused statistics -- the split-bf16 kernels, the fp32-MFMA kernel
// with >= 64-channel tiles and the few-input direct kernel; the 32-channel fp32 tile (Cout <= 32) and the few-output direct kernel do not.
int conv_base_co_tile(int algo, int cin, int cout, int taps, long px_batch) {
    return algo == ALGO_BF16X3 ? conv_bf16x3_co_tile(cin, cout, px_batch) : conv_pick_co_tile(cout, taps, px_batch);
}
int conv_base_cin_pad(int algo, int cin, int taps, int co_tile) { return algo != ALGO_F32 ? cin : conv_cin_pad(cin, taps, co_tile); }
bool conv_emits_stats(int algo, int co_tile, int cout) {
    return algo == ALGO_BF16X3 || (algo == ALGO_F32 && co_tile >= 64) || (algo == ALGO_DIRECT && cout > 4);
}

void build_plan(r2dm_handle* h) {
    const r2dm_config& c = h->cfg;
    const int C0 = c.base_channels, T = c.temb_channels;
    int Cl[5] = {C0, C0 * c.channel_multiplier[0], C0 * c.channel_multiplier[1], C0 * c.channel_multiplier[2],
                 C0 * c.channel_multiplier[3]};
    const long px1 = (long)c.height * c.width * c.max_batch;

    h->range_flag = h->take(2 * r2dm_handle::RANGE_SITES);
    if (c.coord_channels > 0) h->cenc = h->raw("__cenc", (int64_t)c.coord_channels * c.height * c.width);
    h->freqs = h->raw("__sin_freqs", C0 / 2);
    h->w1 = h->raw("time_embedding.1.weight", (int64_t)T * C0);
    h->b1 = h->raw("time_embedding.1.bias", T);
    h->w2 = h->raw("time_embedding.3.weight", (int64_t)T * T);
    h->b2 = h->raw("time_embedding.3.bias", T);
    if (c.coord_channels > 0) {
        const int cin = c.in_channels + c.coord_channels;
        h->in_conv = h->conv_slice("in_conv.weight", cin, 0, c.in_channels, C0, 3, px1, c.height, c.width);
        h->in_conv_c = h->conv_slice("in_conv.weight", cin, c.in_channels, c.coord_channels, C0, 3, (long)c.height * c.width);
        h->in_conv_c.b = h->raw("in_conv.bias", C0);
        h->zero_bias = h->take(C0);
        h->in_conv.b = h->zero_bias;
        h->cmap = h->take((size_t)C0 * c.height * c.width);
    } else {
        h->in_conv = h->conv("in_conv.weight", "in_conv.bias", c.in_channels, C0, 3, px1);
    }

    struct Def { const char* name; int cin, cout, n, level; bool down, up, attn; };
    const Def defs[8] = {
        {"d_block1", Cl[0], Cl[1], c.num_residual_blocks[0], 0, false, false, false},
        {"d_block2", Cl[1], Cl[2], c.num_residual_blocks[1], 1, true, false, false},
        {"d_block3", Cl[2], Cl[3], c.num_residual_blocks[2], 2, true, false, false},
        {"d_block4", Cl[3], Cl[4], c.num_residual_blocks[3], 3, true, false, true},
        {"u_block4", Cl[4], Cl[3], c.num_residual_blocks[3], 3, false, true, true},
        {"u_block3", 2 * Cl[3], Cl[2], c.num_residual_blocks[2], 2, false, true, false},
        {"u_block2", 2 * Cl[2], Cl[1], c.num_residual_blocks[1], 1, false, true, false},
        {"u_block1", 2 * Cl[1], Cl[0], c.num_residual_blocks[0], 0, false, false, false},
    };
    // count AdaGN rows first so the projection matrix is one contiguous [rows][T] block
    int rows = 0;
    for (const Def& d : defs) rows += d.n * 2 * d.cout;
    h->ada_rows = rows;
    h->ada_w = h->take((size_t)rows * T);
    h->ada_b = h->take(rows);

    int row = 0;
    for (int s = 0; s < 8; ++s) {
        const Def& d = defs[s];
        Stage& st = h->stages[s];
        st.name = d.name;
        st.cin = d.cin;
        st.cout = d.cout;
        st.down = d.down;
        st.up = d.up;
        st.attn = d.attn;
        const long px = px1 >> (2 * d.level);  // pixels*batch at the level the residual blocks run on
        const std::string p = std::string(d.name) + ".";
        if (d.down)  // the stage's first conv runs at the resolution above (efficient_unet.py:132-136)
            st.dconv = h->conv(p + "downsample.0.weight", p + "downsample.0.bias", d.cin, d.cout, 3, px << 2, c.height >> (d.level - 1), c.width >> (d.level - 1), /*down=*/true);
        for (int i = 0; i < d.n; ++i) {
            ResLayer r;
            const std::string q = p + "residual_blocks." + std::to_string(i) + ".";
            r.cin = (i != 0 || d.down) ? d.cout : d.cin;
            r.cout = d.cout;
            r.scale = h->raw(q + "scale", 1);
            r.g1 = h->raw(q + "norm1.weight", r.cin);
            r.b1 = h->raw(q + "norm1.bias", r.cin);
            r.conv1 = h->conv(q + "conv1.weight", q + "conv1.bias", r.cin, r.cout, 3, px, c.height >> d.level, c.width >> d.level);
            r.ada_row = row;
            h->raw_at(q + "norm2.proj.1.weight", (int64_t)2 * r.cout * T, h->ada_w + (size_t)row * T);
            h->raw_at(q + "norm2.proj.1.bias", 2 * r.cout, h->ada_b + row);
            row += 2 * r.cout;
            r.conv2 = h->conv(q + "conv2.weight", q + "conv2.bias", r.cout, r.cout, 3, px, c.height >> d.level, c.width >> d.level);
            r.has_skip = r.cin != r.cout;
            if (r.has_skip) r.skip = h->conv(q + "skip.weight", q + "skip.bias", r.cin, r.cout, 1, px, c.height >> d.level, c.width >> d.level);
            st.res.push_back(r);
        }
        if (d.attn) {
            const std::string q = p + "self_attn_block.";
            st.at.C = d.cout;
            st.at.scale = h->raw(q + "scale", 1);
            st.at.gamma = h->raw(q + "norm.weight", d.cout);
            st.at.beta = h->raw(q + "norm.bias", d.cout);
            st.at.qkv = h->conv(q + "attn.in_proj_weight", q + "attn.in_proj_bias", d.cout, 3 * d.cout, 1, px, c.height >> d.level, c.width >> d.level);
            st.at.proj = h->conv(q + "attn.out_proj.weight", q + "attn.out_proj.bias", d.cout, d.cout, 1, px, c.height >> d.level, c.width >> d.level);
        }
        if (d.up)  // upsample then conv at the finer resolution (efficient_unet.py:169-173)
            st.uconv = h->conv(p + "upsample.1.weight", p + "upsample.1.bias", d.cout, d.cout, 3, px << 2, c.height >> (d.level - 1), c.width >> (d.level - 1));
    }
    h->out_conv = h->conv("out_conv.weight", "out_conv.bias", C0, c.out_channels, 3, px1);
    // a down-sampling convolution on the f16x2 path needs its input's range guarded: its producer -- the previous stage's
    // last residual block, second convolution, itself on the f16x2 path (wide epilogue) and no attention block behind it --
    // records max|output|
    for (int s = 0; s + 1 < 8; ++s) {
        Stage& a = h->stages[s];
        const Stage& b = h->stages[s + 1];
        a.out_tracked = b.down && (b.dconv.f2 || b.dconv.dg) && !a.attn && !a.up && !a.res.empty() && a.res.back().conv2.f2;
    }
    // up stages: input of stage 4 = output of stage 3; of stage 4 + k (k = 1..3) = [output of stage 3 + k | output of stage 3 - k]
    for (int s = 4; s < 8; ++s) {
        Stage& a = h->stages[s];
        if (a.res.empty() || !a.res[0].has_skip || !a.res[0].skip.p1) continue;
        a.skip_in_bounded = true;
        h->stages[s - 1].track_final = true;
        if (s > 4) h->stages[7 - s].track_final = true;
    }
    // fp16 storage of the two full-resolution levels (forward.hip Ctx::lvl16), as far as the plan decides it: the default network family (every GroupNorm of
    // levels 1 and 2 on fused statistics -- the streaming pass reads fp32 --, in_conv on the few-input kernel) and every convolution of those levels on a kernel
    // that has the second I/O type (at small batches some layers have too few tiles for conv_f16x2 and run the bf16 kernels: then nothing changes)
    auto blocks_ok = [](const Stage& st) {
        for (const ResLayer& r : st.res)
            if (!r.conv1.f2 || !r.conv2.f2 || (r.has_skip && !r.skip.p1)) return false;
        return true;
    };
    const Stage* S = h->stages;
    h->plan_fits16 = c.gn_num_groups == 8 && C0 % 64 == 0 && h->in_conv.algo == ALGO_DIRECT && h->in_conv.cout > 4 && h->out_conv.algo == ALGO_DIRECT && c.width % 4 == 0 &&
                     S[1].down && S[2].down && S[1].dconv.f2 && S[2].dconv.f2 && S[5].up && S[6].up && S[5].uconv.f2 && S[6].uconv.f2 && !S[0].attn && !S[1].attn && !S[6].attn &&
                     !S[7].attn && blocks_ok(S[0]) && blocks_ok(S[1]) && blocks_ok(S[6]) && blocks_ok(S[7]) && S[6].skip_in_bounded && S[7].skip_in_bounded;
}

int check_config(const r2dm_config& c) {
    if (c.in_channels < 1 || c.out_channels < 1 || c.height < 8 || c.width < 32) return fail(1, "bad image geometry");
    if ((c.height % 8) || (c.width % 32)) return fail(1, "height must be a multiple of 8 and width of 32 (3 FIR levels, 16-byte rows)");
    if (c.base_channels % 2 || c.base_channels < 4) return fail(1, "base_channels must be even");
    if (c.gn_num_groups < 1 || c.max_batch < 1) return fail(1, "bad gn_num_groups / max_batch");
    int Cl[5] = {c.base_channels, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        if (c.channel_multiplier[i] < 1 || c.num_residual_blocks[i] < 1) return fail(1, "bad multiplier / block count");
        Cl[i + 1] = c.base_channels * c.channel_multiplier[i];
    }
    for (int i = 0; i < 5; ++i)
        if (Cl[i] % c.gn_num_groups) return fail(1, "channels %d not divisible by %d groups", Cl[i], c.gn_num_groups);
    for (int i = 1; i <= 3; ++i)  // concat seam must fall on a group boundary: 2*C / G divides C
        if (Cl[i] % (2 * Cl[i] / c.gn_num_groups)) return fail(1, "GroupNorm group straddles the skip concat");
    // an up stage whose concatenated input has as many channels as its output would take the identity skip on a
    // two-source tensor (reference: nn.Identity on the concatenation); the fused residual reads one source only
    for (int i = 1; i <= 3; ++i)
        if (2 * Cl[i] == Cl[i - 1]) return fail(1, "channel_multiplier: 2*%d == %d makes u_block%d's first skip an identity over a concatenation (unsupported)", Cl[i], Cl[i - 1], i);
    const int N = (c.height / 8) * (c.width / 8);
    if (!attention_supported(Cl[4], c.attn_num_heads, N) || !attention_supported(Cl[3], c.attn_num_heads, N))
        return fail(1, "attention: the head size must divide the channels and be at most 128 (got C=%d/%d, heads=%d, N=%d)",
                    Cl[4], Cl[3], c.attn_num_heads, N);
    return 0;
}

}  // namespace r2dm

extern "C" uint64_t r2dm_blob_layout_hash(const r2dm_handle* h) {
    if (!h) return 0;
    uint64_t v = 1469598103934665603ull;  // FNV-1a over the plan
    auto mix = [&](uint64_t x) {
        for (int i = 0; i < 8; ++i) {
            v ^= (x >> (8 * i)) & 0xff;
            v *= 1099511628211ull;
        }
    };
    mix(h->blob_floats);
    mix(h->range_flag);
    mix(h->cmap);
    mix(h->ada_w);
    mix(h->ada_b);
    for (const Slot& s : h->slots) {
        for (char c : s.key) mix((unsigned char)c);
        mix((uint64_t)s.numel);
        mix((uint64_t)s.kind);
        mix(s.off);
        if (s.kind == SLOT_CONV) {
            const ConvLayer& L = s.conv;
            const uint64_t f[] = {(uint64_t)L.cin, (uint64_t)L.cout, (uint64_t)L.taps, (uint64_t)L.co_tile, (uint64_t)L.cin_pad, (uint64_t)L.algo, (uint64_t)L.src_cin,
                                  (uint64_t)L.src_off, L.w, L.b, (uint64_t)L.f2, (uint64_t)L.f2_cot, (uint64_t)L.f2_rows, L.w_f2, L.ws_f2, (uint64_t)L.p1, L.w_p1, L.ws_p1, (uint64_t)L.dg, L.w_dg, L.ws_dg};
            for (uint64_t x : f) mix(x);
        }
    }
    return v;
}
