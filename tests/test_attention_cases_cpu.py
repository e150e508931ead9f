"""The preconditions that tests/test_hip_attention.py relies on, asserted on the fp64 reference alone (no GPU): every row of the shape table reaches the
kernel it names, and every structured input of attention_cases.py is what its docstring says -- a softmax that is one-hot to 2^-30, a late maximum about
60 above every earlier logit for the chosen queries and none at all for the others, logit offsets that span +-80, logits that are all <= -100, a DC level
of R sigma on V."""
import math

import pytest
import torch

import attention_cases as A

ISSUE_TABLE = {  # (heads, d, N) -> kernel family, as the shapes were asked for
    "fp16-pipe / fp32-MFMA (matrix pipe)": [(8, 64, 32), (8, 32, 64), (8, 64, 256), (8, 32, 288), (4, 64, 288), (2, 32, 544), (8, 64, 160), (8, 32, 160), (1, 64, 64), (12, 32, 96)],
    "attention_generic_kernel<32>": [(8, 32, 50), (4, 8, 1), (3, 1, 64)],
    "attention_generic_kernel<64>": [(8, 64, 33), (4, 48, 64), (12, 33, 96)],
    "attention_generic_kernel<128>": [(2, 65, 32), (1, 128, 65)],
}


def test_every_row_reaches_the_kernel_it_names():
    """Dispatch rule of launch_attention: head size 32 or 64 and N % 32 == 0 -> matrix-pipe kernel (the mode picks which), otherwise generic <32> / <64> /
    <128> by head size, whatever the mode.  All three generic instantiations, D == DMAX == 32 and head counts other than 8 are in the table."""
    assert sorted(A.BY_SHAPE) == sorted(s for rows in ISSUE_TABLE.values() for s in rows) and len(A.BY_SHAPE) == len(A.SHAPES)
    for family, rows in ISSUE_TABLE.items():
        for s in rows:
            r = A.BY_SHAPE[s]
            assert A.supported(r.heads * r.d, r.heads, r.N) and r.B <= 2 and r.N <= 544
            names = {p: A.kernel_for(r.heads, r.d, r.N, p) for p in A.MODES}
            if A.is_generic(r):
                assert set(names.values()) == {family} and family == f"attention_generic_kernel<{r.kernel}>" and r.modes == A.MODES
            else:
                assert names == {1: f"attention_f16x2_kernel<{r.d}, 1>", 2: f"attention_f16x2_kernel<{r.d}, 2>", 3: f"attention_kernel<{r.d}>"}
    assert {A.kernel_for(r.heads, r.d, r.N, 2) for r in A.SHAPES} >= {f"attention_generic_kernel<{m}>" for m in (32, 64, 128)}
    assert {r.heads for r in A.SHAPES} >= {1, 2, 3, 4, 8, 12}
    for C, heads, N in A.REFUSALS.values():
        assert not A.supported(C, heads, N)


def test_partly_filled_blocks_after_the_first():
    """The rows that claim a block with inactive waves behind a full one have it, in the kernel they claim it for."""
    for s, pieces, want in (((8, 32, 288), 2, (2, 1, 8)), ((4, 64, 288), 1, (2, 1, 8)), ((2, 32, 544), 2, (3, 1, 8)), ((8, 64, 160), 3, (2, 1, 4)),
                            ((8, 32, 160), 3, (2, 1, 4)), ((8, 32, 288), 3, (3, 1, 4)), ((8, 64, 256), 2, (1, 8, 8)), ((8, 64, 32), 2, (1, 1, 8))):
        assert A.block_fill(s[2], pieces) == want and pieces in A.BY_SHAPE[s].modes


@pytest.mark.parametrize("r", A.ONE_HOT_SHAPES, ids=A.row_id)
def test_one_hot_preconditions(r):
    """Off key pi(n) the fp64 softmax of every query holds less than 2^-30, |q| < 1e3, every query kept; v is bounded away from the split's floor."""
    for kind in A.PERMS:
        qkv, pi, expected, gamma, seed = A.one_hot(r, kind)
        assert sorted(pi.tolist()) == list(range(r.N)) and expected.shape == (r.B, r.heads * r.d, r.N)
        q, k, v = A.heads_view(qkv, r.heads)
        assert q.abs().max().item() < A.Q_MAX and (k.double().norm(dim=2) - 1).abs().max().item() < 1e-6
        assert A.V_LO <= v.abs().min().item() and v.abs().max().item() < A.V_HI
        p = torch.softmax(A.logits(qkv, r.heads), -1)
        on = p.gather(-1, pi.view(1, 1, -1, 1).expand(r.B, r.heads, r.N, 1)).squeeze(-1)
        off = (p.sum(-1) - on).clamp_min(0).max().item() if r.N > 1 else 0.0
        off = max(off, (1 - on).max().item())
        print(f"one-hot {A.row_id(r)} {kind}: gamma {gamma} (seed {seed}), off mass {off:.2e}, max|q| {q.abs().max().item():.0f}")
        assert off < A.OFF_MASS
        assert torch.equal(expected, A.heads_view(qkv, r.heads)[2][..., pi].reshape(r.B, -1, r.N))
        assert (A.attention(qkv, r.heads, torch.float64) - expected.double()).abs().max().item() < 2 * A.OFF_MASS * A.V_HI
    assert kind == "random" and not torch.equal(pi, torch.arange(r.N)) and not torch.equal(pi, torch.arange(r.N - 1, -1, -1))
    assert A.permutation("reversal", r.N)[0].item() == r.N - 1


def test_one_hot_covers_what_was_asked():
    fast = [s for s, r in A.BY_SHAPE.items() if not A.is_generic(r) and r.N >= 64]
    assert len(fast) == 9 and all(A.BY_SHAPE[s] in A.ONE_HOT_SHAPES for s in fast)
    assert sorted(A.BY_SHAPE[s].kernel for s in A.ONE_HOT_GENERIC) == [32, 64, 128] and len(A.ONE_HOT_SHAPES) == 12
    assert A.ONE_HOT_SPLIT == 2 * 2.0 ** -22 and A.ONE_HOT_FP32 == 4 * 2.0 ** -24


@pytest.mark.parametrize("r", A.LATE_SHAPES, ids=A.row_id)
def test_late_maximum_preconditions(r):
    """The key sits in the last tile at the half-wave it claims; for the chosen queries its logit is 55 .. 70 above every earlier one and below 100; every
    other query's logits are those of the untouched problem, to the bit."""
    for half, which in ((h, w) for h in A.LATE_HALVES for w in A.LATE_QUERIES):
        base, mod, pos, queries = A.late_maximum(r, half, which)
        assert pos // 32 == r.N // 32 - 1 and ((pos % 32 < 4) if half == "low" else (4 <= pos % 32 < 8))
        if which == "wave0":
            assert len(queries) == 1 and queries[0] < 32
        elif which == "last_wave":
            assert len(queries) == 1 and queries[0] // 32 == r.N // 32 - 1
        else:
            assert queries == list(range(r.N))
        lb, lm = A.logits(base, r.heads), A.logits(mod, r.heads)
        assert lm.max().item() < 100 and lb.abs().max().item() < 10
        gap = lm[:, :, queries, pos] - lm[:, :, queries, :pos].amax(-1)
        assert 55 < gap.min().item() and gap.max().item() < 70
        rest = [n for n in range(r.N) if n not in set(queries)]
        assert torch.equal(lm[:, :, rest], lb[:, :, rest])
        ref_b, ref_m = A.attention(base, r.heads, torch.float64), A.attention(mod, r.heads, torch.float64)
        assert torch.equal(ref_m[..., rest], ref_b[..., rest])
        # the chosen queries' rows are the value of that key, to exp(-55) N
        v = mod[:, 2 * r.heads * r.d:, pos]
        assert (ref_m[..., queries] - v.double()[..., None]).abs().max().item() < 1e-15


@pytest.mark.parametrize("r", A.SHIFT_SHAPES, ids=A.row_id)
def test_shift_preconditions(r):
    """span: k' - k is one vector per (sample, head) and the per-query logit offsets it causes span 160 in every head, at least 45 and at most 115 to
    either side of zero; negative: every logit is <= -100 (and > -300: exp() of the differences stays in fp32's normal range).  The negative case is not a
    pure key shift: with Gaussian q no constant on k alone makes every logit negative, so q carries the opposite constant (q + a u, k - a u)."""
    plain = A.rnd(300 + r.heads + r.d + r.N, r.B, 3 * r.heads * r.d, r.N)
    qkv = A.shifted(r, "span")
    (q0, k0, v0), (q1, k1, v1) = A.heads_view(plain, r.heads), A.heads_view(qkv, r.heads)
    assert torch.equal(q0, q1) and torch.equal(v0, v1)
    c = (k1.double() - k0.double())
    assert (c - c[..., :1]).abs().max().item() <= 2.0 ** -23 * k1.abs().max().item()  # constant over the keys up to the fp32 rounding of k + c
    off = (A.logits(qkv, r.heads) - A.logits(plain, r.heads))
    assert (off - off[..., :1]).abs().max().item() < 1e-3  # one offset per query
    off = off[..., 0]
    assert ((off.amax(-1) - off.amin(-1)) - 2 * A.SHIFT_SPAN).abs().max().item() < 1e-3 and off.abs().max().item() < 115
    assert off.amax(-1).min().item() > 45 and off.amin(-1).max().item() < -45
    neg = A.logits(A.shifted(r, "negative"), r.heads)
    print(f"shift {A.row_id(r)}: offsets {off.min().item():.1f} .. {off.max().item():.1f}; all-negative logits {neg.min().item():.1f} .. {neg.max().item():.1f}")
    assert neg.max().item() <= -100 and neg.min().item() > -300
    assert torch.isfinite(A.attention(A.shifted(r, "negative"), r.heads, torch.float32)).all()


@pytest.mark.parametrize("r", A.DC_SHAPES, ids=A.row_id)
def test_dc_on_v_preconditions(r):
    """|mean| / sigma of v' is R, and the truth is the truth of the zero-DC problem + R sigma (a convex combination passes a constant through)."""
    plain = A.rnd(400 + r.heads + r.d + r.N, r.B, 3 * r.heads * r.d, r.N)
    ref0 = A.attention(plain, r.heads, torch.float64)
    for R in A.DC_LADDER:
        qkv, sigma = A.dc_on_v(r, R)
        v = A.heads_view(qkv, r.heads)[2].double()
        assert abs(v.mean().item() / v.std(unbiased=False).item() / R - 1) < 0.02 and abs(sigma - 1) < 0.05
        assert torch.equal(qkv[:, :2 * r.heads * r.d], plain[:, :2 * r.heads * r.d])
        assert (A.attention(qkv, r.heads, torch.float64) - ref0 - R * sigma).abs().max().item() < R * 2.0 ** -22


def test_one_product_emulation():
    """The fp16 operands' own error, by the emulation the one-product mode is pinned to in (d) (attention_cases.one_product_operands): on benign data and with every
    logit <= -100 it lies inside test_attention_one_product's bounds; under the span shift it is above 3e-3 -- no kernel of this mode can meet that bound there,
    which is why (d) span holds the kernel to the emulation instead.  The bound on what p's fp16 rounding adds is small against the operand error it sits next
    to (largest element: a fifth or less), so a kernel whose operand error were larger than the format's would not hide under it."""
    for s in ((8, 64, 256), (8, 32, 288), (4, 64, 288)):
        r = A.BY_SHAPE[s]
        qkv = A.benign(r)
        e = A.rel_rms(A.one_product_operands(qkv, r.heads)[0], A.attention(qkv, r.heads, torch.float64))
        assert A.ONE_PRODUCT[0] < e < A.ONE_PRODUCT[1] / 3
        for kind in A.SHIFT_KINDS:
            qkv = A.shifted(r, kind)
            ref = A.attention(qkv, r.heads, torch.float64)
            emul, bound = A.one_product_operands(qkv, r.heads)
            es = A.rel_rms(emul, ref)
            print(f"one-product emulation {A.row_id(r)}: benign {e:.2e}, shift {kind} {es:.2e}; max|emul - fp64| {(emul - ref).abs().max().item():.2e}, largest bound {bound.max().item():.2e}")
            assert (es > A.ONE_PRODUCT[1]) == (kind == "span") and e < es < 1e-2
            assert bound.min().item() > 0 and 5 * bound.max().item() < (emul - ref).abs().max().item()


def test_the_reference_is_test_attention_s_expression():
    """attention_cases.attention against the expression of tests/test_hip_kernels.py::test_attention, written out."""
    B, heads, d, N = 2, 3, 5, 7
    qkv = A.rnd(1, B, 3 * heads * d, N)
    q, k, v = qkv.double().chunk(3, dim=1)
    sp = lambda t: t.reshape(B, heads, d, N)
    att = torch.softmax(sp(q).transpose(-1, -2) @ sp(k) / math.sqrt(d), dim=-1)
    ref = (sp(v) @ att.transpose(-1, -2)).reshape(B, heads * d, N)
    assert (A.attention(qkv, heads, torch.float64) - ref).abs().max().item() < 1e-14
    ref64, e32 = A.references(qkv, heads)
    assert torch.equal(ref64, A.attention(qkv, heads, torch.float64)) and 0 < e32.abs().max().item() < 1e-5
