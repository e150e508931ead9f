"""-m gpu: the conditioning chain of embed.hip kernel by kernel -- time_hidden_kernel, time_out_kernel, ada_proj_kernel -- against the
wide reference and the derived bound of embed_oracle.py, on the input sets test_embed_cpu.py shows to reject a subtly wrong kernel; the
strided AdaGN read of gn_finalize_kernel; and the chain through the engine at a batch above eight with distinct conditions.

Every stage is judged on the previous stage's values as the GPU stored them.  Lines that start with "embed:" are the record
(profiles/embed.txt): the largest error in units of the bound per stage and shape."""
import numpy as np
import pytest
import torch

import embed_oracle as E
from conftest import GOLDEN_RES, max_abs, rnd, synthetic_ckpt

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


@pytest.fixture(scope="module")
def sd():
    from oracle import r2dm_oracle as O

    return O.strip_prefix(synthetic_ckpt(resolution=GOLDEN_RES)["ema_weights"])


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in arrays]


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def run_time(H, t, fr, w):
    act, hid = H.time_embedding(*dev(t, fr, *w), return_hidden=True)
    return act, hid


# ---- the time embedding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [64, 8, 6, 520])
def test_sinusoid_alone(H, golden, base):
    """One-hot w1 (T = base, b1 = 0): hidden[b][r] = f32(silu64(emb[b][r])), within one ulp of the same with the correctly rounded sinusoid --
    the [sin | cos] order and every frequency, first to last, are columns of this comparison."""
    fr, w = E.freqs(base), E.one_hot_weights(base)
    g = golden("ops")
    for name, t in dict(E.SIN_CONDS, golden=g["sin_t"].numpy()).items():
        _, hid = run_time(H, t, fr, w)
        want = E.f32(E.silu64(E.sinusoid(t, fr)))
        u = E.ulps(host(hid), want)
        print(f"embed: sinusoid base {base} {name}: {u:.2f} ulp of f32(silu64(f32(sin64 | cos64)))")
        assert u <= 1, (base, name)
        if base == 64 and name == "golden":  # the reference's own float32 sinusoid
            assert E.ulps(host(hid), E.f32(E.silu64(g["sin_y"].numpy()))) <= 3


@pytest.mark.parametrize("base,T", E.TIME_SHAPES)
def test_time_embedding_t0_is_exact(H, base, T):
    """t = 0: emb = [0 .. 0, 1 .. 1], integer w1 and b1 -- the pre-activation is the exact integer n, whatever the order of the sum."""
    w1, b1, n = E.time_exact(base, T)
    _, _, w2, b2 = E.time_weights(base, T)
    for B in (1, 9):
        _, hid = run_time(H, np.zeros(B, np.float32), E.freqs(base), (w1, b1, w2, b2))
        want = np.broadcast_to(E.f32(E.silu64(n.astype(np.float64))), (B, T))
        assert E.ulps(host(hid), want) <= 1, (base, T, B)


@pytest.mark.parametrize("B", E.TIME_BATCHES)
@pytest.mark.parametrize("base,T", E.TIME_SHAPES)
def test_time_embedding_random(H, base, T, B):
    """hidden inside stage 1's bound; act inside stage 2's bound on the GPU's own hidden."""
    fr, w, t = E.freqs(base), E.time_weights(base, T), E.conds(B)
    act, hid = run_time(H, t, fr, w)
    _, st_h, st_a = E.time_embedding(t, fr, *w, hidden=host(hid))
    ok_h, worst_h, flips_h = E.within_bound(host(hid), st_h)
    ok_a, worst_a, flips_a = E.within_bound(host(act), st_a)
    print(f"embed: time ({base},{T}) B={B}: hidden {worst_h:.3f} of the bound, {E.ulps(host(hid), st_h.ref):.2f} ulp, {flips_h} not f32(ref); "
          f"act {worst_a:.3f} of the bound, {E.ulps(host(act), st_a.ref):.2f} ulp, {flips_a} not f32(ref)")
    assert ok_h, (base, T, B, worst_h)
    assert ok_a, (base, T, B, worst_a)


@pytest.mark.parametrize("base,T", E.TIME_SHAPES)
def test_time_embedding_rows_are_independent(H, base, T):
    """Row b of a batch of 33 distinct conditions is the B = 1 call, bit for bit; a NaN or infinite condition turns its own rows NaN and no other."""
    fr, w, t = E.freqs(base), E.time_weights(base, T), E.conds(33)
    act, hid = run_time(H, t, fr, w)
    for b in range(33):
        a1, h1 = run_time(H, t[b:b + 1], fr, w)
        assert same_bits(a1[0], act[b]) and same_bits(h1[0], hid[b]), (base, T, b)
    bad = t.copy()
    bad[3], bad[8], bad[32] = np.nan, np.inf, -np.inf
    act_b, hid_b = run_time(H, bad, fr, w)
    for b in range(33):
        if b in (3, 8, 32):
            assert bool(torch.isnan(act_b[b]).all() and torch.isnan(hid_b[b]).all()), (base, T, b)
        else:
            assert same_bits(act_b[b], act[b]) and same_bits(hid_b[b], hid[b]), (base, T, b)


def test_time_embedding_checkpoint_weights(H, golden, sd):
    """The golden checkpoint's own weights: the stage bounds, and test_time_embedding's statement against the reference's temb_y."""
    g = golden("ops")
    w = [sd[f"time_embedding.{i}.{n}"].numpy() for i in (1, 3) for n in ("weight", "bias")]
    t, fr = g["sin_t"].numpy(), E.freqs(64)
    act, hid = run_time(H, t, fr, w)
    _, st_h, st_a = E.time_embedding(t, fr, *w, hidden=host(hid))
    ok_h, worst_h, _ = E.within_bound(host(hid), st_h)
    ok_a, worst_a, _ = E.within_bound(host(act), st_a)
    print(f"embed: time checkpoint weights: hidden {worst_h:.3f}, act {worst_a:.3f} of the bound")
    assert ok_h and ok_a, (worst_h, worst_a)
    assert max_abs(act.cpu(), torch.nn.functional.silu(g["temb_y"])) < 2e-6


# ---- ada_proj ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,rows", E.ada_cases())
def test_ada_proj(H, T, B, rows):
    """Exact: integer operands that tell samples and rows apart -- bit-identical to the integer result.  Random: inside the stage bound."""
    act, w, bias, out = E.ada_exact(T, B, rows)
    got = H.ada_proj(*dev(act, w, bias))
    assert np.array_equal(host(got), out.astype(np.float32)), (T, B, rows)
    act, w, bias = E.ada_random(T, B, rows)
    got = host(H.ada_proj(*dev(act, w, bias)))
    st = E.dot_stage(w, act, bias)
    ok, worst, flips = E.within_bound(got, st)
    print(f"embed: ada_proj T={T} B={B} rows={rows}: {worst:.3f} of the bound, {E.ulps(got, st.ref):.2f} ulp, {flips} not f32(ref)")
    assert ok, (T, B, rows, worst)


def test_ada_proj_checkpoint_rows(H, sd):
    """The golden-resolution checkpoint's own packed projections on the GPU's own activations of nine distinct conditions."""
    w, bias = E.packed_ada({k: v.numpy() for k, v in sd.items()})
    tw = [sd[f"time_embedding.{i}.{n}"].numpy() for i in (1, 3) for n in ("weight", "bias")]
    act, _ = run_time(H, E.conds(9), E.freqs(64), tw)
    got = host(H.ada_proj(act, *dev(w, bias)))
    st = E.dot_stage(w, host(act), bias)
    ok, worst, flips = E.within_bound(got, st)
    print(f"embed: ada_proj checkpoint rows={w.shape[0]} B=9: {worst:.3f} of the bound, {E.ulps(got, st.ref):.2f} ulp, {flips} not f32(ref)")
    assert ok, worst


@pytest.mark.parametrize("T", [256, 100])
def test_ada_proj_rows_are_independent(H, T):
    """Row b of B = 33 is the B = 1 call bit for bit, on both load paths."""
    act, w, bias = dev(*E.ada_random(T, 33, 130))
    full = H.ada_proj(act, w, bias)
    for b in range(33):
        assert same_bits(H.ada_proj(act[b:b + 1], w, bias)[0], full[b]), (T, b)


def test_ada_proj_refusals(H):
    from r2dm_amd import _lib

    act, w, bias = dev(*E.ada_random(256, 2, 4))
    out = torch.full((2, 4), float("nan"), device=DEV)
    L = _lib.lib()
    st = _lib.stream_ptr(act.device)
    ptrs = [act.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr()]
    for i in range(4):
        assert L.r2dm_ada_proj(*[None if j == i else p for j, p in enumerate(ptrs)], 2, 256, 4, st) == 1
        assert b"null" in L.r2dm_last_error()
    for sizes in ((0, 256, 4), (2, 0, 4), (2, 256, 0), (-1, 256, 4), (2, -256, 4), (2, 256, -4)):
        assert L.r2dm_ada_proj(*ptrs, *sizes, st) == 1, sizes
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.R2DMError, match="aligned"):
        H.ada_proj(act, w, bias, w_offset=1)
    act, w, bias = dev(*E.ada_exact(100, 2, 4)[:3])  # the scalar path takes any alignment
    assert np.array_equal(host(H.ada_proj(act, w, bias, w_offset=1)), E.ada_exact(100, 2, 4)[3].astype(np.float32))


# ---- the strided AdaGN read --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 512])
def test_group_norm_reads_strided_ada_rows(H, C):
    """gn_finalize_kernel with the AdaGN rows where the engine has them -- inside a wider packed buffer -- against the contiguous (B, 2 C) call: the
    same bits, the same range record, and nothing of the NaN padding between the rows."""
    from r2dm_amd import _lib

    B, G, h, w = 3, 8, 4, 64
    y, stat = H.fir_down2_stats(rnd(90 + C, B, C, 2 * h, 2 * w).to(DEV), G)  # a sink as its producer leaves it
    ada = (0.5 * rnd(91 + C, B, 2 * C)).to(DEV)
    want = H.group_norm_from_stats_ex(stat, C, h, w, 1e-6, ada=ada, range_init=0.0)
    stride, first = 2 * C + 40, 24
    buf = torch.full((first + B * stride + 64,), float("nan"), device=DEV)
    rows = buf[first:first + B * stride].view(B, stride)
    rows[:, :2 * C] = ada
    got = H.group_norm_from_stats_strided(stat, C, h, w, 1e-6, rows, stride, range_init=0.0)
    assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    same = H.group_norm_from_stats_strided(stat, C, h, w, 1e-6, ada, 2 * C, range_init=0.0)
    assert same_bits(same[0], want[0]) and same[2] == want[2]
    with pytest.raises(_lib.R2DMError, match="ada rows"):
        H.group_norm_from_stats_strided(stat, C, h, w, 1e-6, rows, 2 * C - 1)
    # the applied affine is the oracle's AdaGN of the producer's output
    from oracle import r2dm_oracle as O

    ref = O.group_norm(y.double().cpu(), G, 1e-6, None, None) * (1 + ada[:, :C].double().cpu()[:, :, None, None]) + ada[:, C:].double().cpu()[:, :, None, None]
    assert max_abs(H.affine_act(y, got[0], False).cpu(), ref) < 5e-6


# ---- through the engine ----------------------------------------------------------------------------------------------------------------------------
def test_engine_batch_of_eleven_distinct_conditions():
    """A batch above eight (the projection launch's second group of samples) with eleven distinct conditions: bit-identical to its (4, 4, 3) splits,
    and within test_unet_golden's 2e-5 of the oracle in float64."""
    import r2dm_amd
    from oracle import r2dm_oracle as O

    ck = synthetic_ckpt(resolution=GOLDEN_RES)
    net = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=16)[0].model
    x, c = rnd(95, 11, 2, *GOLDEN_RES).to(DEV), torch.linspace(-12, 12, 11, device=DEV)
    full = net(x, c)
    parts = torch.cat([net(x[:4], c[:4]), net(x[4:8], c[4:8]), net(x[8:], c[8:])])
    assert torch.equal(full, parts)
    sd64 = {k: v.double().to(DEV) for k, v in O.strip_prefix(ck["ema_weights"]).items()}
    ref = O.unet_forward(sd64, O.UNetConfig(resolution=GOLDEN_RES), x.double(), c.double())
    err = max_abs(full.cpu(), ref.cpu())
    print(f"embed: engine B=11, 11 conditions: max |y - oracle64| = {err:.2e}")
    assert err < 2e-5
