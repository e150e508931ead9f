"""-m gpu: what the fp16 range guard's producers RECORD, kernel by kernel.

r2dm_check_range compares one recorded bound per guarded tensor with 65504; a record that under-states lets non-finite samples through, one
that over-states sends a good checkpoint to the slower wide-range split for good.  The convolution epilogues' records are held by
test_hip_conv_engine_paths.py; here every other producer, through the _ex entries that take a record (hipops.py):

  gn_finalize_kernel from a statistics sink   record = range_cases.py's mirror of gn_bound with M = sqrt(largest slot energy), to 4 float32 ulp
                                              (the compiler may contract |a| M + |d|), and sound against the data: >= max|a x + d| with the
                                              kernel's own (a, d); sinks synthesized on the host in every summation class, and sinks that
                                              conv_f16x2.hip and fir_down2_stats_kernel left
  gn_partial + gn_finalize (streaming)        the same with M = the exact max|x| of the group, wherever it lies
  fir_up2_kernel / fir_up2_wide_kernel        record bits = bits of max|stored y|, whichever lane, wave, row or seam column holds it
  down_planes_kernel / down_planes_phase_kernel  record bits = bits of max|written plane value|, the same from both layouts
  the engine                                  a GroupNorm folded into conv_f16x2.hip records the bits gn_finalize records; the phase planes
                                              record the bits the nine planes record

Every record is a running maximum that leaves [0] alone, and no output changes with it."""
import os

import numpy as np
import pytest
import torch

import range_cases as RC
from conftest import rnd, synthetic_ckpt

pytestmark = pytest.mark.gpu
f16_path = pytest.mark.skipif(os.environ.get("R2DM_CONV_ALGO", "").startswith("f"), reason="fp32-MFMA algorithm forced")  # (conv_f16x2.hip and the engine's walk only)
DEV = "cuda"
G = 8
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


def as_f32(bits):
    return np.array([bits], dtype=np.int64).astype(np.int32).view(np.float32)[0]


def same_bits(a, b):
    """Bit-identical tensors (NaN fill included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b.contiguous().view(torch.int16))


# ---- GroupNorm: the mirror of one launch ---------------------------------------------------------------------------------------------------
def affine_params(seed, B, C, kind):
    """(kwargs of the entry on the device, w (B, C), sh (B, C) float32 as the kernel forms them): kind 'plain' | 'gamma' | 'ada'."""
    g = np.random.default_rng([77, seed])
    if kind == "plain":
        return {}, np.ones((B, C), np.float32), np.zeros((B, C), np.float32)
    if kind == "gamma":
        gamma, beta = (g.uniform(0.5, 2.0, C) * np.where(g.random(C) < 0.5, -1, 1)).astype(np.float32), g.standard_normal(C).astype(np.float32)
        return dict(gamma=torch.from_numpy(gamma).to(DEV), beta=torch.from_numpy(beta).to(DEV)), np.broadcast_to(gamma, (B, C)), np.broadcast_to(beta, (B, C))
    ada = np.concatenate([g.standard_normal((B, C)) * 3.0, g.standard_normal((B, C))], 1).astype(np.float32)
    return dict(ada=torch.from_numpy(ada).to(DEV)), np.float32(1) + ada[:, :C], ada[:, C:]


def check_record(label, res, bits, xg, aff):
    """One launch's record against the mirror `res` and against the data xg (B, G, n) with the kernel's own aff (B, C, 2)."""
    rec = as_f32(bits)
    print(RC.line(label, res, float(rec)))
    assert bits > 0, f"{label}: record {bits:#x}"
    B, Gn, n = xg.shape
    ad = aff.cpu().numpy().reshape(B, Gn, -1, 2)
    if np.isnan(res.record):
        assert bits > INF_BITS, f"{label}: the mirror's bound is NaN, the record {float(rec)}"
        return
    assert RC.ulps(rec, res.record) <= 4 if np.isfinite(res.record) else bits == INF_BITS, f"{label}: record {float(rec)!r}, mirror {float(res.record)!r}"
    if np.isfinite(res.record):
        applied = RC.applied_max(xg, ad[..., 0], ad[..., 1])
        assert float(rec) * (1.0 + 2.0 ** -20) >= float(applied.max()), f"{label}: record {float(rec)} UNDER max|a x + d| = {float(applied.max())}"


def run_sink(H, label, xg, slots, cpg, hw, kind="plain", seed=0):
    """r2dm_group_norm_from_stats_ex on a host-made sink (B, G, S, 2) of the data xg (B, G, n): every assertion of the issue's sink list."""
    B, Gn, n = xg.shape
    C = Gn * cpg
    assert n == cpg * hw
    kw, w, sh = affine_params(seed, B, C, kind)
    res = RC.Result(xg, w.reshape(B, Gn, cpg), sh.reshape(B, Gn, cpg), slots)
    stat = torch.from_numpy(np.ascontiguousarray(slots)).to(DEV)
    aff0, st0, none = H.group_norm_from_stats_ex(stat, C, 1, hw, RC.EPS, **kw)
    aff, st, bits = H.group_norm_from_stats_ex(stat, C, 1, hw, RC.EPS, range_init=0.0, **kw)
    assert none is None and same_bits(aff0, aff) and same_bits(st0, st), f"{label}: the record changed aff / stats"
    check_record(label, res, bits, xg, aff)
    if np.isfinite(res.record):  # a running maximum: a larger start stays, bit for bit
        start = 2.0 * float(as_f32(bits)) + 1.0
        assert H.group_norm_from_stats_ex(stat, C, 1, hw, RC.EPS, range_init=start, **kw)[2] == H.float_bits(start), label
    return res, bits


# ---- gn_finalize_kernel from a synthesized sink -----------------------------------------------------------------------------------------------
SLOT_COUNTS = (1, 3, 255, 256, 257, 2049)  # both sides of gn_finalize_kernel's 256-thread and 256 * 8 strides


@pytest.mark.parametrize("cpg", [8, 64])
@pytest.mark.parametrize("slots", SLOT_COUNTS)
def test_finalize_from_a_sink_finds_the_largest_slot_wherever_it_is(H, slots, cpg):
    """B = 2, 8 groups, unit noise; one slot of every group carries 8 x the data -- the largest slot energy, M^2 -- placed in turn in the first
    slot, the last, slots 255 / 256 and a slot of wave 3 (thread 200); the summation classes and the affine kinds take turns."""
    B, slot_len = 2, 32 if cpg == 8 else 64  # (n = cpg hw: hw = 4 slots | slots)
    n, hw = slots * slot_len, slots * slot_len // cpg
    base = rnd(200 + slots + cpg, B, G, n).numpy()
    hot = sorted({0, slots - 1, min(255, slots - 1), min(256, slots - 1), min(200, slots - 1), min(200 + 256 * 7, slots - 1)})
    for i, p in enumerate(hot):
        cls, kind = RC.CLASSES[i % 3], ("gamma", "ada", "plain")[i % 3]
        xg = base.copy()
        xg[..., p * slot_len:(p + 1) * slot_len] *= np.float32(8)
        sink = RC.slot_sums(xg, cls, slot_len)
        assert (sink[..., 1].argmax(-1) == p).all()
        res, _ = run_sink(H, f"sink {slots} slots cpg {cpg} hot slot {p} {cls} {kind}", xg, sink, cpg, hw, kind, seed=i)
        assert slots < 255 or "data" in set(res.branch.reshape(-1).tolist())  # (with many slots M decides the record)


TABLE_GRID = [(name, cls) for name in RC.TABLE for cls in RC.CLASSES]


@pytest.mark.parametrize("name,cls", TABLE_GRID, ids=[f"{n}-{c}" for n, c in TABLE_GRID])
def test_finalize_from_a_sink_over_the_case_table(H, name, cls):
    """The CPU table's cases (test_range_bound_cpu.py) through the kernel: 2 x 8 groups of 64 channels x 512 values, each group the case's data
    rolled by another offset (other slots, the same values); the non-finite element in ONE group."""
    x, w, sh = RC.TABLE[name]()
    B, finite = 2, np.where(np.isfinite(x), x, np.float32(0))
    xg = np.stack([np.stack([np.roll(x if (b, g) == (1, 5) else finite, 4099 * (b * G + g)) for g in range(G)]) for b in range(B)])
    sink = RC.slot_sums(xg, cls, RC.F32_SLOT if cls == "f32" else 512)
    C = G * RC.CPG
    if name.startswith("f-adagn"):  # (through the AdaGN operand: the kernel forms w = 1 + scale)
        scale = w - np.float32(1)
        w = np.float32(1) + scale
    wv, shv = np.broadcast_to(w, (B, G, RC.CPG)), np.broadcast_to(sh, (B, G, RC.CPG))
    res = RC.Result(xg, wv, shv, sink)
    if name.startswith("f-adagn"):
        ada = np.concatenate([np.broadcast_to(scale, (B, G, RC.CPG)).reshape(B, C), shv.reshape(B, C)], 1).astype(np.float32)
        kw = dict(ada=torch.from_numpy(ada).to(DEV))
    else:
        kw = dict(gamma=torch.from_numpy(np.ascontiguousarray(wv[0].reshape(C))).to(DEV), beta=torch.from_numpy(np.ascontiguousarray(shv[0].reshape(C))).to(DEV))
    stat = torch.from_numpy(sink).to(DEV)
    aff, st, bits = H.group_norm_from_stats_ex(stat, C, 16, 32, RC.EPS, range_init=0.0, **kw)
    aff0, st0, _ = H.group_norm_from_stats_ex(stat, C, 16, 32, RC.EPS, **kw)
    assert same_bits(aff0, aff) and same_bits(st0, st)
    check_record(f"sink {name} {cls}", res, bits, xg, aff)
    if name[0] in "gh":
        assert not as_f32(bits) < np.float32(RC.FP16_MAX)
    if name == "a-noise":
        assert float(as_f32(bits)) < 0.05 * RC.FP16_MAX
    if name.startswith("d-"):
        assert res.sound()


# ---- sinks that real kernels left ---------------------------------------------------------------------------------------------------------
def check_real_sink(H, label, y, stat, cpg):
    """Record from the producer's own sink against the mirror over the SAME sink, and against the stored output."""
    B, C, h, w = y.shape
    xg = y.cpu().numpy().reshape(B, C // cpg, -1)
    assert torch.isfinite(stat).all()
    return run_sink(H, label, xg, stat.cpu().numpy(), cpg, h * w, "gamma", seed=3)


@f16_path
@pytest.mark.parametrize("data", ["zero-dc", "d-pedestal-spike"])
def test_finalize_from_the_sink_of_conv_f16x2(H, data):
    """conv_f16x2.hip's 64-channel tile (four pixels in fp32, fp64 beyond) through r2dm_conv2d_ring_ex: tiny weights, the residual carries the
    data, scale 1 / sqrt(2) (test_hip_gn_dc_offset.py's recipe).  Case (d) is checked on the STORED output: var / mean^2 in [1.2e-6, 3e-6]."""
    import test_hip_conv_engine_paths as E

    cin, cout, h, w, B, cpg = 64, 512, 4, 64, 2, 64
    n = cpg * h * w
    x, wt, b, _, _ = E.inputs(cin, cout, h, w, B, 3)
    if data == "zero-dc":
        res = rnd(300, B, cout, h, w)
    else:
        res = torch.from_numpy(np.stack([np.stack([RC.case_pedestal_spike(10 * bb + g, n)[0] for g in range(G)]) for bb in range(B)])).reshape(B, cout, h, w)
    res = (res.double() * 2.0 ** 0.5).float().to(DEV)
    with E.selected(H, "f16x2/64"):
        got = H.conv2d_ring_ex(x, wt * 1e-6, torch.zeros_like(b), residual=res, scale=E.INV_SQRT2, stat_groups=G, stat_cpg=cpg)
    assert E.ran("f16x2/64", got.chosen), got.chosen
    if data != "zero-dc":
        yd = got.y.double().cpu().reshape(B, G, -1)
        ratio = yd.var(-1, unbiased=False) / yd.mean(-1) ** 2
        assert 1.2e-6 <= ratio.min().item() and ratio.max().item() <= 3e-6, ratio
    check_real_sink(H, f"conv_f16x2/64 sink, {data}", got.y, got.stat.contiguous(), cpg)


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_finalize_from_the_sink_of_fir_down2_stats(H, offset):
    """fir_down2_stats_kernel's sink (fp64 from the first addition), zero-mean and on a pedestal of 1000 sigma."""
    x = (rnd(301, 2, 64, 8, 128) + offset).to(DEV)
    y, stat = H.fir_down2_stats(x, G)
    check_real_sink(H, f"fir_down2_stats sink, offset {offset:g}", y, stat, 8)


# ---- the streaming pass -----------------------------------------------------------------------------------------------------------------------
STREAM_SHAPES = [(2, 16, 6, 20), (1, 64, 8, 64), (1, 64, 16, 128), (2, 16, 3, 5), (1, 8, 3, 7)]  # one split | one | four | scalar loop (n % 4 != 0), twice


def gn_splits(B, groups, n):
    """norm.hip's gn_splits, and the length of a split."""
    s = max(1, min(2048 // (B * groups), n // 4096, 256))
    ln = ((n + s - 1) // s + 3) & ~3
    return s, ln


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_streaming_pass_records_the_exact_maximum_wherever_it_lies(H, shape):
    """M = max|x| of the group: 1.25 x the largest |noise|, with either sign, placed in turn in the first and the last element of every split
    (gn_partial_kernel's vector loop; its scalar loop where n % 4 != 0) of ONE group (b, g).  That group decides the record: its channels have
    w = 1 (AdaGN scale 0), every other group's w = 0.01, all shifts 0 -- asserted on the mirror, as is that the group's bound is the data
    bound, where M enters, and that the mirror with the spiked element left out of M gives other bits: a kernel that misses the element
    cannot record what the mirror does."""
    B, C, h, w = shape
    cpg, n = C // G, C // G * h * w
    splits, ln = gn_splits(B, G, n)
    assert splits == (4 if shape == (1, 64, 16, 128) else 1)
    base = rnd(210 + n, *shape)
    where = sorted({p for s in range(splits) for p in (s * ln, min((s + 1) * ln, n) - 1)})
    for i, p in enumerate(where):
        x = base.clone()
        b, g = i % B, (3 * i + 1) % G
        grp = x.view(B, G, n)[b, g]
        grp[p] = (-1.25 if i & 1 else 1.25) * base.abs().max()
        label = f"streaming {shape} max at {p} of group ({b}, {g})"
        scale = np.full((B, G, cpg), -0.99, np.float32)
        scale[b, g] = 0.0
        ada = np.concatenate([scale.reshape(B, C), np.zeros((B, C), np.float32)], 1)
        wv, shv = np.float32(1) + scale, np.zeros((B, G, cpg), np.float32)
        kw = dict(ada=torch.from_numpy(ada).to(DEV))
        xg = x.numpy().reshape(B, G, -1)
        res = RC.Result(xg, wv, shv)
        # the mirror: group (b, g) decides, through the data bound, and M without the spiked element gives another record
        assert float(res.gmax[b, g]) == abs(float(grp[p])) and float(res.bound[b, g].max()) == float(res.record), label
        others = np.delete(res.bound.reshape(B * G, cpg), b * G + g, 0)
        assert float(others.max()) < 0.5 * float(res.record) and set(res.branch[b, g].tolist()) == {"data"}, label
        less = res.gmax.copy()
        less[b, g] = np.abs(np.delete(xg[b, g], p)).max()
        missed = RC.Result(xg, wv, shv, gmax=less)
        assert float(less[b, g]) < float(res.gmax[b, g]) and RC.ulps(missed.record, res.record) > 8, label
        xd = x.to(DEV)
        aff0, st0, none = H.group_norm_affine_ex(xd, G, RC.EPS, **kw)
        aff, st, bits = H.group_norm_affine_ex(xd, G, RC.EPS, range_init=0.0, **kw)
        assert none is None and same_bits(aff0, aff) and same_bits(st0, st), f"{label}: the record changed aff / stats"
        check_record(label, res, bits, xg, aff)
        start = 2.0 * float(as_f32(bits)) + 1.0
        assert H.group_norm_affine_ex(xd, G, RC.EPS, range_init=start, **kw)[2] == H.float_bits(start), label


@pytest.mark.parametrize("name", list(RC.TABLE))
def test_streaming_pass_over_the_case_table(H, name):
    """The case table through gn_partial + gn_finalize: (1, 512, 16, 32), 8 splits of a 32768-value group."""
    x, w, sh = RC.TABLE[name]()
    finite = np.where(np.isfinite(x), x, np.float32(0))
    xg = np.stack([np.roll(x if g == 5 else finite, 4099 * g) for g in range(G)])[None]
    C = G * RC.CPG
    xd = torch.from_numpy(xg.reshape(1, C, 16, 32)).to(DEV)
    wv, shv = np.broadcast_to(w, (1, G, RC.CPG)), np.broadcast_to(sh, (1, G, RC.CPG))
    res = RC.Result(xg, wv, shv)
    kw = dict(gamma=torch.from_numpy(np.ascontiguousarray(wv.reshape(C))).to(DEV), beta=torch.from_numpy(np.ascontiguousarray(shv.reshape(C))).to(DEV))
    aff, st, bits = H.group_norm_affine_ex(xd, G, RC.EPS, range_init=0.0, **kw)
    check_record(f"streaming {name}", res, bits, xg, aff)
    if name[0] in "gh":
        assert not as_f32(bits) < np.float32(RC.FP16_MAX)


# ---- fir_up2 ------------------------------------------------------------------------------------------------------------------------------------
UP_SHAPES = [(2, 3, 2, 4), (1, 2, 4, 6), (2, 5, 4, 24), (1, 4, 3, 256), (1, 2, 2, 512), (3, 7, 6, 40)]
UP = [(s, io) for s in UP_SHAPES for io in (0, 2, 3)]


def up_positions(shape):
    """Where the spike goes: the four image corners' rows and columns, the columns either side of a 64-lane boundary of either kernel (thread
    index 63 | 64 of a sample: 2 / 4 input columns per thread), the last element of the last sample."""
    B, C, h, w = shape
    pos = {(0, 0, 0, 0), (0, 0, h - 1, 0), (0, C - 1, 0, w - 1), (B - 1, 0, h - 1, w - 1), (B - 1, C - 1, h - 1, w - 1), (0, 0, h // 2, w // 2)}
    for per in (2, 4):
        if w % per == 0 and C * h * (w // per) > 64:
            for idx, col in ((63, per - 1), (64, 0)):
                c, rem = divmod(idx, h * (w // per))
                pos.add((B - 1, c, rem // (w // per), (rem % (w // per)) * per + col))
    return sorted(pos)


@pytest.mark.parametrize("shape,io16", UP, ids=[f"{'x'.join(map(str, s))}-io{io}" for s, io in UP])
def test_fir_up2_records_the_largest_stored_value(H, shape, io16):
    """Both kernels (R2DM_FIR_UP_WIDE = 0 | 2; the two-column one alone where W % 4 != 0), the three storage instantiations (fp32 -> fp32, fp32 -> fp16, fp16 -> fp16): noise of 0.05 and ONE
    element of +-4; the record is the bits of max|stored y|, y is the same bits with and without a record and within 1e-6 of the oracle in
    fp64 (fp16 storage: that plus the rounding of the store, 2^-11 relative), a larger start stays, and the two kernels record the same bits."""
    from oracle import r2dm_oracle as O

    base = rnd(220, *shape) * 0.05
    for i, pos in enumerate(up_positions(shape)):
        x = base.clone()
        x[pos] = -4.0 if i & 1 else 4.0
        xin = x.half().float() if io16 & 1 else x
        want = O.fir_up2(xin.double())
        records = {}
        for wide in ("0", "2") if shape[3] % 4 == 0 else ("0",):
            with H.env(R2DM_FIR_UP_WIDE=wide, R2DM_TEST_IO16=io16 or None):
                y0, none = H.fir_up2_ex(xin.to(DEV), io16)
                y, bits = H.fir_up2_ex(xin.to(DEV), io16, range_init=0.0)
                kept = H.fir_up2_ex(xin.to(DEV), io16, range_init=100.0)[1]
            label = f"fir_up2 {shape} wide {wide} io16 {io16} spike at {pos}"
            assert none is None and same_bits(y0, y), f"{label}: the record changed y"
            assert not torch.isnan(y).any(), f"{label}: an output element was not written"
            err = (y.double().cpu() - want).abs()
            assert (err <= (2.0 ** -11 * want.abs() + 1e-6 if io16 & 2 else 1e-6)).all(), f"{label}: max error {err.max().item():.3e}"
            m = y.float().abs().max()
            assert m > 2.0 and bits == m.view(torch.int32).item(), f"{label}: record {float(as_f32(bits))!r}, max|stored y| {m.item()!r}"
            assert kept == H.float_bits(100.0), label
            records[wide] = bits
        assert len(set(records.values())) == 1, f"fir_up2 {shape} io16 {io16} spike at {pos}: the two kernels recorded {records}"


@pytest.mark.parametrize("wide", ["0", "2"])
def test_fir_up2_sees_an_overflow_of_its_fp16_store(H, wide):
    """fp32 -> fp16 with a 2 x 2 plateau of 7e4 (one element alone reaches 9/16 of it): the inner corner interpolates to 7e4 > 65504, the store
    gives +inf, and so must the record -- it is the maximum of the values as STORED."""
    x = rnd(221, 2, 5, 4, 24) * 0.05
    x[1, 4, 1:3, 11:13] = 7.0e4
    with H.env(R2DM_FIR_UP_WIDE=wide, R2DM_TEST_IO16=2):
        y, bits = H.fir_up2_ex(x.to(DEV), 2, range_init=0.0)
    assert torch.isinf(y).any() and not torch.isnan(y).any()
    assert bits == INF_BITS, float(as_f32(bits))


# ---- the down-sampling GEMM's planes ---------------------------------------------------------------------------------------------------------
DOWN_SHAPES = [(1, 1, 4, 16), (2, 3, 8, 64), (1, 2, 12, 136), (1, 2, 8, 1024)]  # Ho = 2: one row pair is first and last | ... | 17 column quads | 128


@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_down_planes_record_the_largest_plane_value(H, shape):
    """down_planes_kernel and down_planes_phase_kernel: noise of 0.05 and one element of +-4 in the first and the last row, the first and the last
    column, the last channel.  Record bits = bits of max|value written| (phase layout: the buffer starts NaN-filled, what is still NaN was not
    written); both layouts record the same bits ("the maximum over the distinct planes = the maximum over all nine"); the record is at most
    max|x| (1 + 1e-6) -- the FIR's weights are non-negative and sum to at most 1 per axis; the planes do not change with the record."""
    B, C, h, w = shape
    base = rnd(230, *shape) * 0.05
    pos = sorted({(0, 0, 0, 0), (0, 0, 0, w - 1), (0, 0, h - 1, 0), (B - 1, C - 1, h - 1, w - 1), (B - 1, C - 1, 0, w // 2 + 1), (0, C - 1, h // 2, 7), (0, 0, 1, 8)})
    for i, p in enumerate(pos):
        x = base.clone()
        x[p] = -4.0 if i & 1 else 4.0
        xd = x.to(DEV)
        label = f"down planes {shape} spike at {p}"
        a0, none = H.down_planes_ex(xd)
        a, bits = H.down_planes_ex(xd, range_init=0.0)
        assert none is None and same_bits(a0, a) and not torch.isnan(a).any(), label
        m = a.abs().max()
        assert m > 0.3 and bits == m.view(torch.int32).item(), f"{label}: nine planes record {float(as_f32(bits))!r}, max {m.item()!r}"
        p0, none = H.down_phase_planes_ex(xd)
        ph, pbits = H.down_phase_planes_ex(xd, range_init=0.0)
        assert none is None and same_bits(p0, ph), label
        written = ph[~torch.isnan(ph)]
        assert written.numel() == B * C * (h + 3) * (2 * (w // 2) + 1)  # (every row's data of both phases, and float 3 of the first phase's rows)
        pm = written.abs().max()
        assert pbits == pm.view(torch.int32).item(), f"{label}: phase planes record {float(as_f32(pbits))!r}, max {pm.item()!r}"
        assert pbits == bits, f"{label}: phase planes record {float(as_f32(pbits))!r}, nine planes {float(as_f32(bits))!r}"
        assert float(as_f32(bits)) <= 4.0 * (1.0 + 1e-6)
        assert H.down_planes_ex(xd, range_init=100.0)[1] == H.float_bits(100.0) and H.down_phase_planes_ex(xd, range_init=100.0)[1] == H.float_bits(100.0)


# ---- the engine: folded against separate, phase planes against nine -----------------------------------------------------------------------------
ENGINE = [((32, 256), 2), ((32, 256), 3), ((64, 1024), 2), ((64, 1024), 3)]
ENGINE_IDS = [f"{r[0]}x{r[1]}-B{b}" for r, b in ENGINE]


def site_report(res, batch, **switches):
    """[(site, bound)] of one forward on a fresh model, under the given environment switches."""
    import r2dm_amd
    from hipops import env

    with env(**switches):
        m, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=res), device=DEV, show_info=False, max_batch=batch)
        y = m.model(rnd(240 + batch, batch, 2, *res).to(DEV), torch.linspace(-2.0, 3.0, batch).to(DEV))
        m.model.check_range()
        rep = m.model.range_report()
        del m
    return y, rep


def sites(rep, what):
    """(layer, bound) of the sites whose name holds `what`, in walk order; the layer is the name up to the site's description."""
    return [(name.split(what)[0], bound) for name, bound in rep if what in name]


@f16_path
@pytest.mark.parametrize("res,batch", ENGINE, ids=ENGINE_IDS)
def test_folded_group_norm_records_the_bits_gn_finalize_records(res, batch):
    """R2DM_GN_FOLD = 1 | 0 on the synthetic checkpoint, one forward on a fresh model each: mode 0 folds no GroupNorm into conv_f16x2.hip, mode 1
    does at 64 x 1024 with batch 2 (measured on an MI355X: 30 of 50 there; none at batch 3, where a block's tiles straddle samples, and none at
    32 x 256 -- every GroupNorm site of both walks then reads "(gn_finalize)" or "(streaming statistics)", and the pairing is asserted all the
    same); the GroupNorm sites of the two walks, paired by layer and order, hold the same bits (gn_bound is shared: gn_math.h)."""
    y1, fold = site_report(res, batch, R2DM_GN_FOLD="1")
    y0, sep = site_report(res, batch, R2DM_GN_FOLD="0")
    n_fold = sum("(folded into the convolution)" in n for n, _ in fold)
    assert n_fold >= 1 or (res, batch) != ((64, 1024), 2), (len(fold), fold[:6])
    assert not any("(folded into the convolution)" in n for n, _ in sep)
    a, b = sites(fold, "GroupNorm output bound"), sites(sep, "GroupNorm output bound")
    print(f"engine {res} batch {batch}: {len(a)} GroupNorm sites, {n_fold} folded; largest bound {max(v for _, v in a):.6g}")
    assert len(a) == len(b) > 10 and [k for k, _ in a] == [k for k, _ in b]
    diff = [(k, va, vb) for (k, va), (_, vb) in zip(a, b) if np.float32(va).view(np.int32) != np.float32(vb).view(np.int32)]
    assert not diff, diff[:4]
    assert all(0.0 < v < RC.FP16_MAX for _, v in a) and torch.equal(y1, y0)


@f16_path
@pytest.mark.parametrize("res,batch", ENGINE, ids=ENGINE_IDS)
def test_phase_planes_record_the_bits_the_nine_planes_record(res, batch):
    """R2DM_DOWN_GEMM = 9 against the default: the "max|FIR planes|" sites, paired by layer and order, where that stage runs (measured on an
    MI355X: at 64 x 1024; no down stage of the 32 x 256 walk takes the GEMM, and then neither walk may name such a site)."""
    _, phase = site_report(res, batch)
    _, nine = site_report(res, batch, R2DM_DOWN_GEMM="9")
    a, b = sites(phase, "max|FIR planes|"), sites(nine, "max|FIR planes|")
    print(f"engine {res} batch {batch}: {len(a)} FIR-plane sites of {len(phase)}: {a}")
    assert len(a) == len(b) >= (0 if res == (32, 256) else 1) and all("every distinct plane once" in n for n, _ in phase if "max|FIR planes|" in n) \
        and all("all nine" in n for n, _ in nine if "max|FIR planes|" in n)
    assert [(k, np.float32(v).view(np.int32)) for k, v in a] == [(k, np.float32(v).view(np.int32)) for k, v in b]
    assert all(v > 0 for _, v in a)
