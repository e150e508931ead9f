"""-m gpu: the ConvParams fields that only the engine's walk (forward.hip) fills, kernel by kernel through r2dm_conv2d_ring_ex -- the fused
GroupNorm statistics of the 3x3 / 1x1 convolutions (per (sample, group) fp64 [sum, sum of squares] slots), the max|output| record behind the
fp16 operand guard, the two-allocation input (Src::p1), the batch-broadcast residual and the descending tile walk.

No oracle here: the yardstick of the statistics is the kernel's own STORED output reduced in fp64 by torch, the yardstick of the output is
r2dm_conv2d_ring on the same inputs (held against fp64 by test_hip_kernels.py), bit for bit.

Which bar a kernel's statistics get is read from its source (u = 2^-24, the fp32 unit roundoff):
  fp64   1e-12 . sum|y| and 1e-12 . sum y^2 (the bar of the FIR and down-GEMM statistics tests): every addition is fp64 --
         conv_mfma.hip's epilogue and conv_epilogue.h's conv_epilogue + epi_stat_write (conv_bf16x3.hip on partial tiles);
  four   3 u . sum|y| and 5 u . sum y^2: FOUR adjacent pixels are summed in fp32 -- (v0 + v1) + (v2 + v3), two rounding levels;
         fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 v0))), four -- and everything beyond is fp64: conv_epilogue_wide (conv_bf16x3.hip on whole
         tiles, proj_f16x2.hip), conv_few_in_kernel and conv_f16x2.hip's two-plane (parity) instances.  ((1 + u)^2 - 1 < 3 u and
         (1 + u)^4 - 1 < 5 u bound the fp32 part; the fp64 part is five orders below.)
  f32    12 u . sum|y| and 12 u . sum y^2: conv_f16x2.hip's ONE-plane instance (the fp16 bulk mode) sums a slot's 512 values pairwise in
         fp32 (2 + 1 + 6 levels, one more for the squares; second-order terms allowed for), fp64 from the slot on.
These bars are relative to sum|y| and sum y^2 and do not see cancellation: what the classes are worth under a DC offset, where
var = E[y^2] - mean^2 multiplies the error by (mean / sigma)^2, is test_hip_gn_dc_offset.py's business.
One dropped or doubled element is far above all three at these shapes: the slots are also checked one by one where a slot is one image row
of a 64-pixel tile (64 . cpg values, 32 . 64 per half for 64-channel groups)."""
import functools
import math
import os

import pytest
import torch

from conftest import rnd
from r2dm_amd._lib import R2DMError

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("R2DM_CONV_ALGO", "").startswith("f"), reason="fp32-MFMA algorithm forced")]
DEV = "cuda"
U = 2.0 ** -24
INV_SQRT2 = 0.70710678


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


# ---- variants: name -> (pieces, R2DM_F2_CO_TILE, kernel size, (algo, co_tile, px_rows) the entry must report; None = any) ----------------
# (the single-kernel entries reach the few-input kernel through the selection bit of the storage tests' hook alone, R2DM_TEST_IO16 = 4: fp32
# tensors, plain convolutions without a scale -- its statistics are those of the value after the residual)
F32, BF16X3, DIRECT, F16X2, P1F16 = range(5)
VARIANTS = {
    "f16x2/64": (2, "64", 3, (F16X2, 64, 4)),
    "f16x2/32": (2, "32", 3, (F16X2, 32, 4)),
    "f16x2/128": (2, "128", 3, (F16X2, 128, 4)),
    "f16x2/64x8": (2, "64x8", 3, (F16X2, 64, 8)),
    "f16x2/64 one plane": (1, "64", 3, (F16X2, 64, 4)),
    "bf16x3": (3, None, 3, (BF16X3, None, 4)),
    "f32 mfma 3x3": (4, None, 3, (F32, None, 4)),
    "f32 mfma 1x1": (4, None, 1, (F32, None, 4)),
    "proj_f16x2": (2, None, 1, (P1F16, 64, 4)),
    "few-input direct": (2, None, 3, (DIRECT, None, 4)),
}
F2_VARIANTS = [v for v in VARIANTS if v.startswith("f16x2")]
PERSISTENT_TILE = {"f16x2/64": (64, 4), "f16x2/32": (32, 4), "f16x2/128": (128, 4), "f16x2/64x8": (64, 8), "f16x2/64 one plane": (64, 4)}


def supports(variant, cin, cout, h, w):
    """The *_supported functions of the launchers, for the shapes used here."""
    if variant.startswith("f16x2"):
        tile, rows = PERSISTENT_TILE[variant]
        # (the entries send a shape to conv_f16x2.hip where conv_bf16x3.hip would have taken it)
        return cin % (64 if cin <= 128 else 128) == 0 and cin <= 512 and cout % tile == 0 and h % rows == 0 and w % 64 == 0
    if variant == "bf16x3":
        return cout % 64 == 0 and cin % (64 if cin <= 128 else 128) == 0 and w % 4 == 0
    if variant == "proj_f16x2":
        return cin % 32 == 0 and cout % 64 == 0 and h % 4 == 0 and w % 64 == 0
    if variant == "few-input direct":
        return cin <= 4 and cout > 4 and cout % 8 == 0 and h % 4 == 0 and w % 4 == 0
    return cin > 4 and w % 4 == 0  # the fp32 MFMA kernel


def prologues(variant):
    """0 and 2 (GroupNorm affine + SiLU); proj_f16x2.hip has no SiLU prologue (0 and 1, the attention block's), the few-input kernel none."""
    return (0,) if variant == "few-input direct" else (0, 1) if variant == "proj_f16x2" else (0, 2)


def has_range(variant):
    return variant != "few-input direct"


def has_reverse(variant):
    return variant.startswith("f16x2") or variant == "proj_f16x2"


class selected:
    """The single-kernel entries' selection switches of one variant, restored on exit."""

    def __init__(self, H, variant):
        self.H, (self.pieces, tile, _, _) = H, VARIANTS[variant]
        self.env = {"R2DM_F2_CO_TILE": tile, "R2DM_TEST_IO16": "4" if variant == "few-input direct" else None}

    def __enter__(self):
        self.H.set_conv_pieces(self.pieces)
        self.cm = self.H.env(**self.env)
        self.cm.__enter__()

    def __exit__(self, *exc):
        self.H.set_conv_pieces(2)
        return self.cm.__exit__(*exc)


def epilogue_scale(variant):
    return None if variant == "few-input direct" else INV_SQRT2


def ran(variant, chosen):
    want = VARIANTS[variant][3]
    return all(w is None or w == c for w, c in zip(want, chosen))


@functools.lru_cache(maxsize=4)
def inputs(cin, cout, h, w, B, k):
    """x, weights scaled by 1 / sqrt(taps Cin), bias, residual and the prologue's (a, d) = (U(0.5, 1.5), 0.3 N(0, 1)), on the device."""
    g = torch.Generator().manual_seed(5)
    aff = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g) * 0.3], -1).contiguous()
    return (rnd(1, B, cin, h, w).to(DEV), (rnd(2, cout, cin, k, k) / math.sqrt(k * k * cin)).to(DEV), rnd(3, cout).to(DEV), rnd(4, B, cout, h, w).to(DEV),
            aff.to(DEV))


def stat_bars(algo, h, w, pieces=2):
    """(name, bar of the sums, bar of the squares) relative to sum|y| and sum y^2: from the kernels' sources (module docstring); pieces: the
    operand planes of the launch (VARIANTS) -- conv_f16x2.hip's one-plane instance alone keeps fp32 sums to the slot."""
    if algo == F16X2 and pieces == 1:
        return "f32", 12 * U, 12 * U
    if algo == F32 or (algo == BF16X3 and (h % 4 or w % 64)):
        return "fp64", 1e-12, 1e-12
    return "four", 3 * U, 5 * U


def slot_moments(y, cpg, split64):
    """[sum, sum |.|, sum of squares] of the stored output per statistics slot, (B, groups, slots, 3) in fp64, where a slot is one image row
    of one 4-row x 64-pixel tile -- slot (th nTw + tw) 4 + row -- and (split64) a 64-channel group puts its two 32-channel halves into the
    two halves of the grid (the 32-channel-half epilogues; conv_mfma.hip's 1 x 4-wave tile keeps the group whole, in the first half)."""
    B, C, h, w = y.shape
    hv = 2 if cpg == 64 and split64 else 1
    t = y.double().view(B, C // cpg, hv, cpg // hv, h // 4, 4, w // 64, 64)
    m = torch.stack([t.sum((3, 7)), t.abs().sum((3, 7)), (t * t).sum((3, 7))], -1)  # (B, G, hv, th, row, tw, 3)
    m = m.permute(0, 1, 2, 3, 5, 4, 6).reshape(B, C // cpg, hv, -1, 3)
    if hv == 1:
        m = torch.cat([m, torch.zeros_like(m)], 2)
    return m.reshape(B, C // cpg, -1, 3)


def check_statistics(label, y, stat, goff, cpg, chosen, pieces=2):
    """Assertions b, c and d of the issue on one launch's sink; chosen: the kernel that ran, as the entry reports it."""
    algo, co_tile, _ = chosen
    B, C, h, w = y.shape
    ng = C // cpg
    mine = stat[:, goff:goff + ng]
    assert torch.isfinite(mine).all(), f"{label}: a slot of a written group was not written"
    other = torch.ones(stat.shape[1], dtype=torch.bool)
    other[goff:goff + ng] = False
    assert torch.isnan(stat[:, other]).all(), f"{label}: a group outside [goff, goff + Cout / cpg) was written"
    if cpg < 64:
        assert (mine[:, :, mine.shape[2] // 2:] == 0).all(), f"{label}: second half of the slots not zero"
    name, bar_s, bar_q = stat_bars(algo, h, w, pieces)
    yd = y.double().reshape(B, ng, -1)
    want_s, want_a, want_q = yd.sum(-1), yd.abs().sum(-1), (yd * yd).sum(-1)
    got = mine.sum(2)
    es, eq = ((got[..., 0] - want_s).abs() / want_a).max().item(), ((got[..., 1] - want_q).abs() / want_q).max().item()
    msg = f"group sums rel {es:.2e} (bar {bar_s:.2e}), squares rel {eq:.2e} (bar {bar_q:.2e}) [{name}]"
    # (one element against the bar: the smallest |y| cannot be told from roundoff, the typical one must -- 30 bars, or the slots decide)
    n = yd.shape[-1]
    per_slot = (algo in (F16X2, BF16X3, P1F16) or (algo == F32 and co_tile == 64)) and h % 4 == 0 and w % 64 == 0
    assert per_slot or 1.0 / (n * bar_s) >= 30, f"{label}: {n} elements per group: one of them is within 30 bars"
    if per_slot:
        sm = slot_moments(y, cpg, algo != F32)
        ss = ((mine[..., 0] - sm[..., 0]).abs() / sm[..., 1].clamp_min(1e-300)).max().item()
        sq = ((mine[..., 1] - sm[..., 2]).abs() / sm[..., 2].clamp_min(1e-300)).max().item()
        msg += f"; per slot sums rel {ss:.2e}, squares rel {sq:.2e}"
    print(f"    {label}: {msg}")
    assert ((got[..., 0] - want_s).abs() <= bar_s * want_a).all(), f"{label}: {msg}"
    assert ((got[..., 1] - want_q).abs() <= bar_q * want_q).all(), f"{label}: {msg}"
    if per_slot:
        assert ((mine[..., 0] - sm[..., 0]).abs() <= bar_s * sm[..., 1]).all(), f"{label}: {msg}"
        assert ((mine[..., 1] - sm[..., 2]).abs() <= bar_q * sm[..., 2]).all(), f"{label}: {msg}"
    # d. a slot's energy bounds every element it covers: what the range guard of the GroupNorm's consumers takes as M
    assert (mine[..., 1].amax(2).sqrt() >= yd.abs().amax(-1)).all(), f"{label}: largest slot energy below max|y|^2"


def f32_bits(v):
    return torch.tensor(v, dtype=torch.float32).view(torch.int32).item()


def check_range(label, rec, y, algo, quiet=False):
    """Assertion e on a record that started as [7, 0]."""
    assert rec[0].item() == 7, f"{label}: range[0] was written"
    m = y.abs().max().cpu()  # (fp32: exact)
    r = rec[1:2].view(torch.float32)[0]
    if not quiet:
        print(f"    {label}: range {r.item():.6g}, max|y| {m.item():.6g}")
    assert m <= r, f"{label}: range record {r.item()} UNDER max|y| {m.item()}"
    if algo == F16X2:  # sqrt(largest four-pixel energy) x 1.000001, each of the four at most max|y|
        assert r.double() <= 2 * m.double() * (1 + 1e-5), f"{label}: range record {r.item()} above 2 max|y| = {2 * m.item()}"
    else:  # elementwise maximum (conv_epilogue.h, conv_mfma.hip)
        assert rec[1].item() == m.view(torch.int32).item(), f"{label}: range record {r.item()} is not max|y| {m.item()}"


def run_case(H, variant, cin, cout, h, w, B, G, goff, cpg):
    k = VARIANTS[variant][2]
    x, wt, b, res, aff = inputs(cin, cout, h, w, B, k)
    rng, rev = has_range(variant), int(has_reverse(variant))
    with selected(H, variant):
        for pro in prologues(variant):
            label = f"{variant} {cin}->{cout} {h}x{w} B{B} pro {pro}"
            kw = dict(aff=aff if pro else None, prologue=pro, residual=res, scale=epilogue_scale(variant))
            y0 = H.conv2d_ring(x, wt, b, **kw)
            ex = dict(kw, stat_groups=G, stat_goff=goff, stat_cpg=cpg)
            r1 = H.conv2d_ring_ex(x, wt, b, range_init=(7, 0) if rng else None, reverse=rev, **ex)
            print(f"{label}: chosen (algo, co_tile, px_rows) = {r1.chosen}")
            assert ran(variant, r1.chosen), (variant, r1.chosen)
            algo = r1.chosen[0]
            # a. statistics, range record and tile order leave the output alone
            assert torch.equal(r1.y, y0), f"{label}: output changed, max diff {(r1.y - y0).abs().max().item():.3e}"
            # b. same bits from a second call, and (fixed summation order, every slot written once) from the ascending walk
            r2 = H.conv2d_ring_ex(x, wt, b, range_init=(7, 0) if rng else None, reverse=rev, **ex)
            assert torch.equal(r2.y, y0)
            assert torch.equal(r1.stat.view(torch.int64), r2.stat.view(torch.int64)), f"{label}: statistics differ between two calls"
            check_statistics(label, r1.y, r1.stat, goff, cpg, r1.chosen, VARIANTS[variant][0])
            if rng:
                assert torch.equal(r1.range, r2.range), f"{label}: range record differs between two calls"
                check_range(label, r1.range, r1.y, algo)
            if rng or rev:
                # ... a RUNNING maximum: a larger record stays; and the other walk direction
                big = f32_bits(1e6)
                r3 = H.conv2d_ring_ex(x, wt, b, range_init=(7, big) if rng else None, reverse=0, **ex)
                assert r3.chosen == r1.chosen and torch.equal(r3.y, y0), f"{label}: output differs without reverse"
                assert torch.equal(r3.stat.view(torch.int64), r1.stat.view(torch.int64)), f"{label}: statistics depend on the walk direction"
                assert not rng or r3.range.tolist() == [7, big], f"{label}: a smaller maximum replaced the record: {r3.range.tolist()}"


def check_range_follows_a_spike(H, variant, cin, cout, h, w, B, positions):
    """With random data the record can only be caught under-reporting where the maximum happens to lie.  Here the residual is zero but for
    ONE element of 1000 at (sample, channel, row, column): whichever wave, quarter or deferred tile end owns that element must deliver it."""
    x, wt, b, _, aff = inputs(cin, cout, h, w, B, VARIANTS[variant][2])
    res = torch.zeros(B, cout, h, w, device=DEV)
    pro = prologues(variant)[-1]
    with selected(H, variant):
        for i, pos in enumerate(positions):
            res.zero_()
            res[pos] = 1000.0
            got = H.conv2d_ring_ex(x, wt, b, aff=aff if pro else None, prologue=pro, residual=res, scale=INV_SQRT2, range_init=(7, 0),
                                   reverse=i & 1 if has_reverse(variant) else 0)
            assert ran(variant, got.chosen), (variant, got.chosen)
            assert got.y[pos].abs() == got.y.abs().max() and got.y[pos].abs() > 600, (pos, got.y[pos].item())
            check_range(f"{variant} spike at {pos}", got.range, got.y, got.chosen[0], quiet=True)
    print(f"{variant} {cin}->{cout} {h}x{w} B{B}: range record followed a spike at {len(positions)} positions")


# (Cin, Cout, H, W, B, groups of the sink, first group, channels per group)
SHAPES = [
    (64, 64, 4, 64, 2, 8, 0, 8),      # one row tile: top and bottom halo rows in the same tile
    (64, 128, 8, 128, 2, 8, 0, 16),
    (64, 256, 8, 64, 3, 8, 0, 32),
    (64, 512, 4, 64, 3, 8, 0, 64),
    (128, 64, 12, 128, 2, 8, 0, 8),   # H a multiple of 4, not of 8
    (64, 64, 8, 64, 2, 4, 0, 16),     # 4 groups of 16
    (64, 64, 8, 64, 2, 8, 4, 16),     # an up stage's second producer: groups 4..7 of a shared sink
    (256, 512, 4, 64, 2, 8, 0, 64),   # two-level kernels (Cin > 128); conv_bf16x3's 32-channel tile: a wave holds HALF a 64-channel group
    (64, 64, 6, 96, 2, 8, 0, 8),      # partial tiles (rows and columns): the predicated epilogue, fp64 from the first addition
    (32, 128, 64, 256, 8, 8, 0, 16),  # the fp32-MFMA kernel's 128-channel tile (2 x 2 waves: two of a tile's four slots, the others zeroed)
    (2, 64, 8, 64, 2, 8, 0, 8),       # in_conv: the few-input direct kernel
]
CASES = [pytest.param(v, *s, id=f"{v.replace(' ', '_')}-{s[0]}-{s[1]}-{s[2]}x{s[3]}-B{s[4]}-G{s[5]}+{s[6]}x{s[7]}")
         for s in SHAPES for v in VARIANTS if supports(v, *s[:4]) and (s[1] != 128 or s[4] != 8 or v == "f32 mfma 3x3")]


@pytest.mark.parametrize("variant,cin,cout,h,w,B,G,goff,cpg", CASES)
def test_conv_statistics_range_and_tile_order(H, variant, cin, cout, h, w, B, G, goff, cpg):
    """Issue items a-e for every kernel and tile shape a residual block's convolutions run on, prologue 0 and 2 (0 and 1 for proj_f16x2.hip,
    which has no SiLU prologue; 0 for the few-input kernel, which has none), with residual and 1/sqrt(2) so that the statistics are those of
    the value AFTER both: output bit-identical to r2dm_conv2d_ring; every slot of the written groups written, nothing else; second half zero
    for narrow groups; moments of the stored output within the kernel's bar, per group and per slot; the largest slot energy bounds max|y|;
    the range record bounds max|y| (exactly it, outside conv_f16x2.hip) and is a running maximum; same bits from two calls and from both
    walk directions."""
    run_case(H, variant, cin, cout, h, w, B, G, goff, cpg)
    if (cin, cout, B) == (32, 128, 8):
        with selected(H, variant):  # (what the case is for)
            assert H.conv2d_ring_ex(*inputs(cin, cout, h, w, B, 3)[:3]).chosen[:2] == (F32, 128)


@pytest.mark.parametrize("variant", F2_VARIANTS)
def test_conv_statistics_persistent_blocks_take_several_tiles(H, variant):
    """conv_f16x2.hip is persistent: one block per CU walks the launch's tiles.  More tiles than CUs: blocks finish a tile's deferred
    quarters under the next tile and hand quarters to the staging waves (tile_end_share) -- the statistics and the range record of those
    code paths.  The groups have 16 x 8192 values here: the slots are checked one by one (check_statistics: 64 x 16 values each)."""
    cin, cout, h, w = 64, 128, 32, 256
    tile, rows = PERSISTENT_TILE[variant]
    per_sample = (cout // tile) * (w // 64) * (h // rows)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus // per_sample + 1
    assert B * per_sample > cus
    print(f"{variant}: {B * per_sample} tiles on {cus} CUs (batch {B})")
    run_case(H, variant, cin, cout, h, w, B, 8, 0, 16)
    # (every sample: the tiles a block takes first and the ones it takes later; all four 32-channel blocks, rows of both halves of an 8-row tile)
    check_range_follows_a_spike(H, variant, cin, cout, h, w, B, [(bb, (37 * i + 32 * bb + 5) % cout, (5 * i + bb) % h, (67 * i + 32 * bb + 9) % w) for bb in range(B) for i in range(4)])


@pytest.mark.parametrize("variant", [v for v in VARIANTS if has_range(v)])
def test_conv_range_record_sees_every_wave(H, variant):
    """Issue item e where a missed wave cannot hide: a spike in every (sample, 32-channel block, image row, 32-pixel segment) of a
    64 -> 128, 8 x 128 launch, i.e. in every wave's and every quarter's share of every tile shape, walking in both directions."""
    cin, cout, h, w, B = 64, 128, 8, 128, 2
    check_range_follows_a_spike(H, variant, cin, cout, h, w, B, [(bb, 32 * cb + 5 + 8 * (r & 3), r, 32 * sg + 7 + (cb & 3))
                                                                for bb in range(B) for cb in range(cout // 32) for r in range(h) for sg in range(w // 32)])


# ---- f. the two-allocation input ---------------------------------------------------------------------------------------------------------
SPLITS = [(v, c0, c1) for v in VARIANTS if v != "few-input direct"
          for c0, c1 in ((64, 64), (128, 64), (128, 128)) + (((48, 16),) if v.startswith("f32 mfma") else ())
          if supports(v, c0 + c1, 128, 8, 64)]


@pytest.mark.parametrize("variant,c0,c1", SPLITS, ids=[f"{v.replace(' ', '_')}-{a}|{b}" for v, a, b in SPLITS])
def test_conv_two_allocation_input(H, variant, c0, c1):
    """Src::p1 -- the up path's channel concat without a copy: x[:, :c0] and x[:, c0:] in two separate allocations, each between NaN-filled
    guard planes (a read past either end shows in y), against the one-source launch on the concatenation, bit for bit: every kernel stages
    whole channels and multiplies them in the same order wherever they come from, so no kernel gets the looser fp64 bars.  64|64, 128|64
    (Cin = 192 runs on the fp32-MFMA and proj_f16x2 kernels only: the split kernels need Cin % 64 / % 128) and 128|128; for the fp32-MFMA
    kernel also 48|16, a seam inside one of its 4 / 8 / 16-channel chunks."""
    cin, cout, h, w, B = c0 + c1, 128, 8, 64, 2
    x, wt, b, res, aff = inputs(cin, cout, h, w, B, VARIANTS[variant][2])
    guard = h * w
    keep, xa = H.guarded((B, c0, h, w), torch.float32, guard, DEV)
    keep1, xb = H.guarded((B, c1, h, w), torch.float32, guard, DEV)
    xa.copy_(x[:, :c0])
    xb.copy_(x[:, c0:])
    with selected(H, variant):
        for pro in prologues(variant):
            kw = dict(aff=aff if pro else None, prologue=pro, residual=res, scale=epilogue_scale(variant))
            one = H.conv2d_ring_ex(x, wt, b, **kw)
            two = H.conv2d_ring_ex(xa, wt, b, x1=xb, stat_groups=8, stat_cpg=cout // 8, **kw)
            print(f"{variant} {c0}|{c1} pro {pro}: chosen {two.chosen}")
            assert ran(variant, two.chosen) and two.chosen == one.chosen, (variant, one.chosen, two.chosen)
            assert torch.equal(one.y, H.conv2d_ring(x, wt, b, **kw))
            assert torch.isfinite(two.y).all(), f"{variant} {c0}|{c1} pro {pro}: a guard plane was read"
            assert torch.equal(two.y, one.y), f"{variant} {c0}|{c1} pro {pro}: max diff {(two.y - one.y).abs().max().item():.3e}"
            check_statistics(f"{variant} {c0}|{c1} pro {pro}", two.y, two.stat, 0, cout // 8, two.chosen, VARIANTS[variant][0])
    assert H.guard_intact(keep, guard) and H.guard_intact(keep1, guard)


@pytest.mark.parametrize("variant,c0,c1", [("f16x2/64", 72, 56), ("bf16x3", 72, 56), ("proj_f16x2", 68, 60), ("few-input direct", 1, 1)])
def test_conv_two_allocation_input_refused_off_the_chunk_boundary(H, variant, c0, c1):
    """launch_conv_f16x2 / launch_conv_bf16x3: a 16-channel chunk must not straddle the seam; launch_proj_f16x2: a thread's 8 channels;
    launch_conv_direct: one source only.  The entry refuses before anything is launched (the wrapper checks y and the sink)."""
    cin, cout, h, w, B = c0 + c1, 64, 8, 64, 2
    x, wt, b, _, _ = inputs(cin, cout, h, w, B, VARIANTS[variant][2])
    with selected(H, variant):
        assert ran(variant, H.conv2d_ring_ex(x, wt, b).chosen)
        with pytest.raises(R2DMError):
            H.conv2d_ring_ex(x[:, :c0].contiguous(), wt, b, x1=x[:, c0:].contiguous(), stat_groups=8, stat_cpg=8)


# ---- g. the batch-broadcast residual -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_conv_broadcast_residual(H, variant):
    """res_bs = 0 -- in_conv adds the constant coordinate map this way: one (Cout, H, W) residual for the whole batch against the same map
    expanded over the batch, bit for bit, B = 3."""
    cin, cout, h, w, B = (2 if variant == "few-input direct" else 64), 128, 8, 64, 3
    x, wt, b, res, aff = inputs(cin, cout, h, w, B, VARIANTS[variant][2])
    one = res[0].contiguous()
    with selected(H, variant):
        for pro in prologues(variant):
            kw = dict(aff=aff if pro else None, prologue=pro, scale=epilogue_scale(variant))
            want = H.conv2d_ring(x, wt, b, residual=one.expand(B, -1, -1, -1).contiguous(), **kw)
            got = H.conv2d_ring_ex(x, wt, b, residual=one, res_broadcast=True, stat_groups=8, stat_cpg=cout // 8, **kw)
            print(f"{variant} pro {pro}: chosen {got.chosen}")
            assert ran(variant, got.chosen), (variant, got.chosen)
            assert torch.equal(got.y, want), f"{variant} pro {pro}: max diff {(got.y - want).abs().max().item():.3e}"
            assert not torch.equal(got.y, H.conv2d_ring(x, wt, b, **kw))  # (the residual counts)
            check_statistics(f"{variant} broadcast residual pro {pro}", got.y, got.stat, 0, cout // 8, got.chosen, VARIANTS[variant][0])


# ---- h. refusals -------------------------------------------------------------------------------------------------------------------------
def test_conv_ex_refusals(H):
    """Everything r2dm_conv2d_ring_ex must refuse (include/r2dm_hip.h), each with a sink, an output and a range record in place: the
    wrapper asserts that all three still hold their fill after the refusal, then raises the entry's error on."""
    def refused(variant, shape, k=None, **kw):
        cin, cout, h, w, B = shape
        x, wt, b, _, _ = inputs(cin, cout, h, w, B, k or VARIANTS[variant][2])
        with selected(H, variant):
            with pytest.raises(R2DMError):
                H.conv2d_ring_ex(x, wt, b, **kw)
                pytest.fail(f"not refused: {variant} {shape} {kw}")

    sink = dict(stat_groups=8, stat_cpg=8)
    small = (64, 64, 8, 64, 2)
    # statistics from kernels that emit none: the fp32-MFMA kernel's 32-channel tile, the few-output direct kernel
    with selected(H, "f32 mfma 3x3"):
        assert H.conv2d_ring_ex(*inputs(16, 32, 8, 64, 2, 3)[:3]).chosen[:2] == (F32, 32)
        assert H.conv2d_ring_ex(*inputs(64, 4, 8, 64, 2, 3)[:3]).chosen[0] == DIRECT
    refused("f32 mfma 3x3", (16, 32, 8, 64, 2), stat_groups=4, stat_cpg=8)
    refused("f32 mfma 3x3", (64, 4, 8, 64, 2), stat_groups=1, stat_cpg=8)
    # channels per group outside {8, 16, 32, 64}; channels that do not split; groups that do not fit the sink
    for variant in ("f16x2/64", "bf16x3", "f32 mfma 3x3", "f32 mfma 1x1", "proj_f16x2"):
        for cpg in (0, 4, 24, 128):
            refused(variant, (64, 128, 8, 64, 2), stat_groups=64, stat_cpg=cpg)
        refused(variant, small, stat_groups=8, stat_goff=1, stat_cpg=8)
        refused(variant, small, stat_groups=8, stat_goff=5, stat_cpg=16)
        refused(variant, small, stat_groups=8, stat_goff=-1, stat_cpg=16)
        refused(variant, small, stat_groups=3, stat_cpg=16)
    refused("f32 mfma 3x3", (64, 96, 8, 64, 2), stat_groups=8, stat_cpg=64)
    refused("few-input direct", (2, 64, 8, 64, 2), stat_groups=8, stat_cpg=16, stat_goff=5)
    # a range record from the direct kernels; a descending walk where there is none
    refused("few-input direct", (2, 64, 8, 64, 2), range_init=(7, 0), **sink)
    refused("f32 mfma 3x3", (64, 4, 8, 64, 2), range_init=(7, 0))
    for variant in ("bf16x3", "f32 mfma 3x3", "f32 mfma 1x1", "few-input direct"):
        refused(variant, (2, 64, 8, 64, 2) if variant == "few-input direct" else small, reverse=1, **sink)
    refused("f16x2/64", small, reverse=2, **sink)
    # c1 outside [0, cin); x1 and c1 that do not go together
    x = inputs(*small, 3)[0]
    for variant in ("f16x2/64", "f32 mfma 3x3"):
        for c1 in (-1, 64, 72):
            refused(variant, small, x1=x, c1=c1, range_init=(7, 0), **sink)
        refused(variant, small, c1=16, **sink)
        refused(variant, small, x1=x, c1=0, **sink)
    # a broadcast residual without a residual
    refused("f16x2/64", small, res_broadcast=True, **sink)
