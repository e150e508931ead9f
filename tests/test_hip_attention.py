"""-m gpu: the three attention kernels of attention.hip, every instantiation, on structured inputs (attention_cases.py: the shape table, the generators,
the references and the derivation of every bar; test_attention_cases_cpu.py proves the generators' preconditions on the fp64 reference alone).

  attention_f16x2_kernel<32 | 64, 2>   pieces 2 (default): the split fp16 pipe           8 waves x 32 queries per block
  attention_f16x2_kernel<32 | 64, 1>   pieces 1: one fp16 product per MAC
  attention_kernel<32 | 64>            pieces 3: fp32 MFMA                               4 waves x 32 queries per block
  attention_generic_kernel<32 | 64 | 128>   every other geometry, fp32 whatever the mode

Dispatch rule (launch_attention): head size 32 or 64 and N % 32 == 0 -> a matrix-pipe kernel, otherwise the generic one.  No entry reports the kernel that
ran, so the rule is asserted on the table (CPU) and its consequences here: a generic row gives the same bits in all three modes, a matrix-pipe row three
different outputs, the one-product mode an error above 1e-5 relative rms.

Every call goes through hipops.attention_padded: the output lies between two canary rows that must come back bit-unchanged, and every output element must
have been written.  Every case prints `attention-stress | group | case | pieces | kernel | err | err32 | ratio`; profiles/attention_stress.txt is that table."""
import numpy as np
import pytest
import torch

import attention_cases as A
from r2dm_amd._lib import R2DMError

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


def run(H, qkv, heads, pieces):
    H.set_conv_pieces(pieces)
    try:
        return H.attention_padded(qkv.to(DEV), heads).cpu()
    finally:
        H.set_conv_pieces(2)


_cache = {}


def cached(key, make):
    """References are computed once per case and shared by the modes' tests; nothing changes them afterwards."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def with_references(r, make_qkv):
    qkv = make_qkv()
    ref, e32 = A.references(qkv, r.heads)
    return qkv, ref, e32


def modes(r, of=A.MODES):
    """A generic row runs one kernel whatever the mode: beyond (a) it is run in the default mode alone."""
    return [p for p in r.modes if p in of]


def params(rows, *more, of=A.MODES, generic_once=True):
    out = []
    for r in rows:
        for p in ((2,) if generic_once and A.is_generic(r) else modes(r, of)):
            if not more:
                out.append(pytest.param(r, p, id=f"{A.row_id(r)}-p{p}"))
            for extra in (more[0] if more else ()):
                out.append(pytest.param(r, extra, p, id=f"{A.row_id(r)}-{extra}-p{p}"))
    return out


def record(group, case, r, pieces, err, err32):
    ratio = err / err32 if err32 > 0 else float("inf") if err > 0 else 0.0
    print(f"attention-stress | {group} | {case} | {pieces} | {A.kernel_for(r.heads, r.d, r.N, pieces)} | {err:.3e} | {err32:.3e} | {ratio:.2f}")


def one_product(r, pieces):
    return pieces == 1 and not A.is_generic(r)


def check_class(group, case, r, pieces, out, ref, e32, v_max, upper=True):
    """The (a) bar on one output: fp32 class against the fp32 expression's own error; the one-product mode on a matrix-pipe row by its own bounds
    (upper = False: the lower bound alone -- (d) span, where the kernel is pinned to the fp16-operand emulation instead)."""
    assert torch.isfinite(out).all(), f"{group} {case} pieces {pieces}: non-finite output"
    err, err32 = (out.double() - ref).abs().max().item(), e32.abs().max().item()
    record(group, case, r, pieces, err, err32)
    if one_product(r, pieces):
        e = A.rel_rms(out, ref)
        print(f"attention-stress one product | {group} | {case} | rel rms {e:.3e}")
        assert A.ONE_PRODUCT[0] < e and (e < A.ONE_PRODUCT[1] or not upper), (group, case, pieces, e)
    else:
        assert err <= A.fp32_class_bar(err32, v_max), (group, case, pieces, err, err32, v_max)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,pieces", params(A.SHAPES, generic_once=False))
def test_benign_data_at_every_shape(H, r, pieces):
    """Every instantiation (the table's `kernel` column; generic <64>, D == DMAX == 32, head counts 1 .. 12 and blocks with inactive waves behind a full one
    included) on N(0, 1) data with no spike: max error <= max(3 err32, 3e-6 max|v|) with err32 small, so a wrong instantiation (d = 64, N = 33 sent to
    <32>), a wave that `active` wrongly drops (q0 < N - 32) or a lost accumulator shows at its own size.  Pieces 1: test_attention_one_product's bounds."""
    qkv, ref, e32 = cached(("a", r), lambda: with_references(r, lambda: A.benign(r)))
    check_class("a benign", A.row_id(r), r, pieces, run(H, qkv, r.heads, pieces), ref, e32, A.vmax(qkv))


@pytest.mark.parametrize("r", A.SHAPES, ids=A.row_id)
def test_the_mode_picks_the_kernel_the_table_names(H, r):
    """Every row of the table.  What the dispatch rule implies for the bits: a generic row is one fp32 kernel in all three modes; on a matrix-pipe row the three modes are three
    kernels with three arithmetics, and the default mode is the split pipe."""
    qkv = cached(("a", r), lambda: with_references(r, lambda: A.benign(r)))[0]
    out = {p: run(H, qkv, r.heads, p) for p in A.MODES}
    default = H.attention_padded(qkv.to(DEV), r.heads).cpu()
    assert torch.equal(default, out[2])
    if A.is_generic(r):
        assert torch.equal(out[1], out[2]) and torch.equal(out[3], out[2])
    else:
        assert not torch.equal(out[1], out[2]) and not torch.equal(out[3], out[2]) and not torch.equal(out[1], out[3])


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind,pieces", params(A.ONE_HOT_SHAPES, A.PERMS, of=(2, 3)))
def test_one_hot_softmax_routes_every_key_to_its_query(H, r, kind, pieces):
    """q_n = gamma k_pi(n) on unit keys: the softmax is one-hot to 2^-30, the output must be v[:, pi(n)] -- every (query, key) pair pinned, where a flat
    softmax dilutes one value by 1 / N.  Guards the key -> value routing: the fp16-pipe kernel's permuted V order (position 16 s + 8 half + j <-> key
    16 s + (j / 4) 8 + half 4 + j % 4; swapping the two middle terms moves four keys of eight), the fp32-MFMA kernel's j = r % 4 + 8 (r / 4) + 4 hi, the generic
    kernel's key loop.  Reversal gives the low queries keys of the last tile (a late jump of the running maximum by gamma / sqrt(d) in every lane) and of
    the other half-wave.  Per element: 4 2^-24 |v| for the fp32 kernels; 2^-21 |v| for the split pipe = two operand splits of 22 bits each (f16x2.h: h +
    2^-11 l, 11 significant bits apiece); derivation in attention_cases.py."""
    qkv, pi, expected, gamma, _ = cached(("b", r, kind), lambda: A.one_hot(r, kind))
    out = run(H, qkv, r.heads, pieces)
    split = pieces == 2 and not A.is_generic(r)
    rel = ((out.double() - expected.double()).abs() / expected.double().abs())
    e32 = cached(("b32", r, kind), lambda: ((A.attention(qkv, r.heads, torch.float32).double() - expected.double()).abs() / expected.double().abs()).max().item())
    record("b one-hot (relative)", f"{A.row_id(r)} {kind} gamma {gamma}", r, pieces, rel.max().item(), e32)
    assert rel.max().item() <= (A.ONE_HOT_SPLIT if split else A.ONE_HOT_FP32), (rel.max().item(), int((rel > A.ONE_HOT_FP32).sum()))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
LATE = [(h, w) for h in A.LATE_HALVES for w in A.LATE_QUERIES]


@pytest.mark.parametrize("r,case,pieces", params(A.LATE_SHAPES, [f"{h}-{w}" for h, w in LATE]))
def test_late_maximum(H, r, case, pieces):
    """attention_f16x2_kernel<32 | 64, 1 | 2> and attention_kernel<32 | 64>, at a full block and at token counts whose last block has one active wave.  One key
    of the LAST tile -- in the low half-wave's registers (pos % 32 < 4) or the high half-wave's ([4, 8)) -- beats every earlier logit by about 60 for one query of
    wave 0, for one query of the last active wave of the last block, or for all queries: alpha = exp(-60) in a single lane (or in all) while the fp16-pipe
    kernel's `__any(alpha != 1)` decides the rescale of o and ol for the whole wave, and the running maximum moves in the last iteration.  Bar of (a); the rows of
    the queries that were not chosen must also meet it against the truth of the problem without the key (their logits are the same to the bit).  The
    one-product mode: (a)'s bounds, 1e-5 < relative rms < 3e-3."""
    half, which = case.split("-")

    def make():
        base, mod, pos, queries = A.late_maximum(r, half, which)
        rest = [n for n in range(r.N) if n not in set(queries)]
        return mod, A.references(mod, r.heads), A.references(base, r.heads), rest

    mod, (ref, e32), (ref_b, e32_b), rest = cached(("c", r, case), make)
    out = run(H, mod, r.heads, pieces)
    check_class("c late maximum", f"{A.row_id(r)} {case}", r, pieces, out, ref, e32, A.vmax(mod))
    if rest:
        check_class("c late maximum, other queries", f"{A.row_id(r)} {case}", r, pieces, out[..., rest], ref_b[..., rest], e32_b[..., rest], A.vmax(mod))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind,pieces", params(A.SHIFT_SHAPES, A.SHIFT_KINDS))
def test_shift_invariance(H, r, kind, pieces):
    """Every matrix-pipe instantiation and generic <32>, <64>, <128>.  k' = k + c: every query's logits move by a constant (spanning 160 across the queries, or all
    of them <= -100) that the online softmax must cancel through m_run.  Truth and err32 on the shifted inputs; bar of (a).  With every logit <= -100 a running
    maximum that started at 0 instead of -inf leaves p = exp(-100) = 0 in every lane and 0 / 0 in the output: finite outputs are asserted.
    attention_f16x2_kernel<32 | 64, 1>: (a)'s bounds hold in the all-negative case.  Under the span shift the upper one, 3e-3, cannot hold for any kernel of the
    mode: rounding k + c to fp16 alone costs 5.8e-3 .. 6.0e-3 (test_attention_cases_cpu.py asserts it on the emulation; measured on the kernel: 5.84e-3 ..
    6.03e-3).  In both cases the kernel is therefore pinned to the fp16-operand emulation itself (attention_cases.one_product_operands): per element
    |out - emul| <= the rigorous bound of p's fp16 rounding + max(3 err32, 3e-6 max|v|) for the fp32 accumulation -- a kernel that lost more than the format
    does (the operand error's largest element is 9 .. 13 x that bound) fails."""
    qkv, ref, e32 = cached(("d", r, kind), lambda: with_references(r, lambda: A.shifted(r, kind)))
    out = run(H, qkv, r.heads, pieces)
    assert torch.isfinite(out).all()
    check_class(f"d shift {kind}", A.row_id(r), r, pieces, out, ref, e32, A.vmax(qkv), upper=kind != "span")
    if one_product(r, pieces):
        emul, bound = cached(("d16", r, kind), lambda: A.one_product_operands(qkv, r.heads))
        diff, allowed = (out.double() - emul).abs(), bound + A.fp32_class_bar(e32.abs().max().item(), A.vmax(qkv))
        print(f"attention-stress emulation | d shift {kind} | {A.row_id(r)} | max|out - emul| {diff.max().item():.3e} | largest allowance {allowed.max().item():.3e} "
              f"| worst |out - emul| / allowance {(diff / allowed).max().item():.3f}")
        assert bool((diff <= allowed).all()), (kind, diff.max().item(), (diff / allowed).max().item())


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,R,pieces", params(A.DC_SHAPES, A.DC_LADDER, of=(2, 3)))
def test_dc_on_v(H, r, R, pieces):
    """attention_f16x2_kernel<32 | 64, 2>, attention_kernel<32 | 64> and generic <32>, <64>, <128>.  v' = v + R sigma, R = 16 and 256: the DC level must come
    through the convex combination unchanged (o / l with the same rounded p in both).  fp32 kernels: bar of (a).  Split pipe: max(3 err32, 2^-21 max|v'|) -- P
    and V each carry 22 bits (f16x2.h), so the sum of p v' is off by up to 2 x 2^-22 of its largest operand however small the AC part is.  (Measured: the
    split pipe stays at 0.8 .. 0.9 err32 and never needs the second term; the fp32-MFMA kernel reaches 2.5 err32 at R = 256.)"""
    qkv, ref, e32 = cached(("e", r, R), lambda: with_references(r, lambda: A.dc_on_v(r, R)[0]))
    out = run(H, qkv, r.heads, pieces)
    err, err32, v_max = (out.double() - ref).abs().max().item(), e32.abs().max().item(), A.vmax(qkv)
    record(f"e DC on V, R = {R}", A.row_id(r), r, pieces, err, err32)
    split = pieces == 2 and not A.is_generic(r)
    assert err <= (max(3 * err32, A.DC_SPLIT * v_max) if split else A.fp32_class_bar(err32, v_max)), (err, err32, v_max)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,pieces", [pytest.param(r, p, id=f"{A.row_id(r)}-p{p}") for r, ps in A.INDEPENDENCE for p in ps])
def test_containment_and_independence(H, r, pieces):
    """One shape per kernel (both matrix-pipe head sizes in all three modes, at a token count with a partly filled last block; generic <32>, <64>, <128>): the
    canary rows around the output survive (attention_padded), sample b alone gives row b of the batch, two calls give the same bits, and permuting the
    heads of qkv permutes the heads of the output -- blockIdx.y / blockIdx.z enter the addresses and nothing else, no state survives a launch."""
    qkv = cached(("a", r), lambda: with_references(r, lambda: A.benign(r)))[0]
    out = run(H, qkv, r.heads, pieces)
    assert torch.equal(out, run(H, qkv, r.heads, pieces))
    assert r.B == 2
    for b in range(r.B):
        assert torch.equal(run(H, qkv[b:b + 1].contiguous(), r.heads, pieces), out[b:b + 1])
    if r.heads > 1:
        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(r.heads))
        assert not torch.equal(perm, torch.arange(r.heads))
        C = r.heads * r.d
        shuffled = qkv.view(r.B, 3, r.heads, r.d, r.N)[:, :, perm].reshape(r.B, 3 * C, r.N).contiguous()
        assert torch.equal(run(H, shuffled, r.heads, pieces), out.view(r.B, r.heads, r.d, r.N)[:, perm].reshape(r.B, C, r.N))


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.REFUSALS))
def test_refusals_leave_the_output_alone(H, name):
    """r2dm_attention in all three modes: heads = 0, C % heads != 0, N = 0 and head size 129 (one past attention_generic_kernel<128>) raise R2DMError before any
    launch (attention_supported); attention_padded asserts that the whole
    canary-filled output buffer is bit-unchanged before it raises."""
    C, heads, N = A.REFUSALS[name]
    assert not A.supported(C, heads, N)
    qkv = torch.zeros(1, 3 * C, N, device=DEV)
    for pieces in A.MODES:
        H.set_conv_pieces(pieces)
        try:
            with pytest.raises(R2DMError, match="attention"):
                H.attention_padded(qkv, heads, C=C)
        finally:
            H.set_conv_pieces(2)
