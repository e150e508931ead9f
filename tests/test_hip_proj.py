"""-m gpu: proj_f16x2.hip -- all 1x1 convolutions and the three down-sampling GEMMs -- in every one of its 13 instantiations (proj_cases.py: the table with
the entry that reaches each, the shapes, the generators, the fp64 references and the derivation of the exact grid; test_proj_cases_cpu.py proves the table
against the source and the generators' preconditions without a GPU).

No entry reports which instantiation ran (`chosen` is (P1F16, 64, 4) for all of them), so the dispatch rule is asserted on the table (CPU) and its
consequences here:
  (a) on exact-grid inputs every instantiation returns the fp64 result rounded once -- torch.equal, nothing can hide under a tolerance; a second exact grid
      with split weights does the same for the weights' l plane, which the first cannot see;
  (b) on N(0, 1) data the project's bars: two planes max|y - fp64| < 1e-5, one plane max|y - fp16-operand emulation| < 1e-5;
  (c) the tall shape (Cout % 256 == 0) gives the bits of Cout / 64 launches on the 64-channel slices, which run the wide shape -- output, statistics, range;
  (d) the two-allocation input with seams inside and between the 32-channel chunks gives the bits of the one-source launch, fp16 storage included;
  (e) what the fp16-storage hook must refuse is refused before anything is written.
The 1x1 launches go through hipops.conv2d_ring_ex (guard bands around y and the sink), the down-sampling GEMMs through hipops.down_gemm (guard bands
around y).  Every case prints `proj-instantiations | check | row | shape | err | err32 | ratio`; profiles/proj_instantiations.txt is that table."""
import os

import pytest
import torch

import proj_cases as P
from r2dm_amd._lib import R2DMError
from test_hip_conv_engine_paths import P1F16, check_range, check_statistics

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("R2DM_CONV_ALGO", "").startswith("f"), reason="fp32-MFMA algorithm forced")]
DEV = "cuda"
CHOSEN = (P1F16, 64, 4)


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


_cache = {}


def data(kind, c):
    """(inputs, fp64 reference, the fp32 torch expression's max error): computed once per case, shared by the tests, never changed."""
    key = (kind, c)
    if key not in _cache:
        d = {"exact": P.exact_inputs, "exact, split weights": P.exact_inputs_split_weights, "benign": P.benign_inputs}[kind](c)
        _cache[key] = (d,) + P.references(c, d)
    return _cache[key]


def dev(t):
    return None if t is None else t.to(DEV)


def run(H, c, d, x=None, x1=None, cpg=None, record=True):
    """One launch of case c on inputs d (x / x1: device tensors that replace d["x"], in two allocations).  cpg: channels per group of a statistics sink (None:
    no sink).  record: a range record starting at [7, 0] (the 1x1 entries).  Returns hipops.ConvExResult; the down-sampling entries report neither kernel
    nor range."""
    x = dev(d["x"]) if x is None else x
    if P.is_down(c):
        y, stat = H.down_gemm(x, dev(d["w"]), dev(d["b"]), groups=d["w"].shape[0] // cpg if cpg else 0, nine=c.entry == "nine")
        return H.ConvExResult(y, stat, None, CHOSEN)
    cout = d["w"].shape[0]
    H.set_conv_pieces(c.inst.nplk)
    try:
        with H.env(R2DM_TEST_IO16=c.inst.iom or None):
            r = H.conv2d_ring_ex(x, dev(d["w"]), dev(d["b"]), x1=x1, aff=dev(d["aff"]), prologue=c.inst.pro, residual=dev(d["res"]), scale=d["scale"],
                                 stat_groups=cout // cpg if cpg else 0, stat_cpg=cpg or 0, range_init=(7, 0) if record else None, io16=c.inst.iom)
    finally:
        H.set_conv_pieces(2)
    assert r.chosen == CHOSEN, r.chosen
    return r


def sink_cpg(c):
    """Eight groups, as the network's GroupNorms have; the fp16-storage launch takes no sink."""
    return None if c.inst.iom else c.cout // 8


def report(check, c, err, err32):
    ratio = err / err32 if err32 > 0 else float("inf") if err > 0 else 0.0
    print(f"proj-instantiations | {check} | {P.inst_id(c.inst)} | {c.cin}->{c.cout} {c.h}x{c.w} B{c.B} | {err:.3e} | {err32:.3e} | {ratio:.2f}")


def max_err(y, ref):
    return (y.double().cpu() - ref).abs().max().item()


def check_sink_and_record(label, c, r):
    if r.stat is not None:
        check_statistics(label, r.y, r.stat, 0, sink_cpg(c), CHOSEN, c.inst.nplk)
    if r.range is not None:
        check_range(label, r.range, r.y.float(), P1F16)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_exact_grid_inputs_are_bit_equal_to_fp64(H, c):
    """Every product, every partial sum of either accumulator and the epilogue are exactly representable (proj_cases.py), so the kernel returns the fp64
    result rounded to fp32 -- and once more to fp16 where it stores fp16 -- whatever its summation order.  The statistics sink meets the `four` bar of
    test_hip_conv_engine_paths.py against the stored output, the range record is exactly max|y|."""
    d, ref, e32 = data("exact", c)
    r = run(H, c, d, cpg=sink_cpg(c))
    y = r.y.cpu()
    report("a exact grid", c, max_err(y, ref), e32)
    want = P.stored(c, ref)
    assert y.dtype == want.dtype and torch.isfinite(y).all()
    assert torch.equal(y, want), f"{P.case_id(c)}: {(y != want).sum().item()} of {y.numel()} elements differ, max |y - fp64| {max_err(y, ref):.3e}"
    check_sink_and_record(P.case_id(c) + " exact grid", c, r)


@pytest.mark.parametrize("c", P.SPLIT_WEIGHT_CASES, ids=P.case_id)
def test_exact_grid_with_split_weights_is_bit_equal_to_fp64(H, c):
    """The exact grid has wl = 0 and cannot see the weights' l plane: without this test the wl . xh product was held by the 1e-5 bar of (b) alone.  Twelve-bit
    weights (wl != 0 in a quarter of them) against a coarse x operand are exact in the same sense (proj_cases.exact_inputs_split_weights): torch.equal with
    fp64 for every two-plane 1x1 instantiation."""
    d, ref, e32 = data("exact, split weights", c)
    r = run(H, c, d, cpg=sink_cpg(c))
    y = r.y.cpu()
    report("a exact grid, split weights", c, max_err(y, ref), e32)
    want = P.stored(c, ref)
    assert torch.equal(y, want), f"{P.case_id(c)}: {(y != want).sum().item()} of {y.numel()} elements differ, max |y - fp64| {max_err(y, ref):.3e}"
    check_sink_and_record(P.case_id(c) + " exact grid, split weights", c, r)


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------
def ulp16(v):
    """fp16's spacing at |v| (2^-24 below the normals)."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_benign_data_at_every_row(H, c):
    """N(0, 1) data, weights / sqrt(K), residual and 1 / sqrt(2) where the instantiation takes them.  Two planes: max|y - fp64| < 1e-5 (test_conv1x1's bar).
    One plane: max|y - emul| < 1e-5 against the fp64 product of the fp16-rounded x operand and the h plane of the weights
    (test_conv_one_product_is_exactly_fp16_operands' bar), and the error against fp64 shows that the reduced mode ran.  The fp16-storage launch rounds its
    output once more: its bar is 1e-5 + half an fp16 ulp per element, and it equals RNE_f16 of the fp32-storage launch bit for bit
    (test_in_out_and_skip_convolutions_fp16_storage_is_exact's contract)."""
    d, ref, e32 = data("benign", c)
    r = run(H, c, d, cpg=sink_cpg(c))
    y = r.y.cpu()
    assert torch.isfinite(y).all()
    err = max_err(y, ref)
    report("b benign", c, err, e32)
    if c.inst.nplk == 2:
        assert err < 1e-5, err
    else:
        emul = P.one_plane_emulation(c, d)
        dev_e = (y.double() - emul).abs()
        rel = ((y.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
        print(f"proj-instantiations one plane | {P.case_id(c)} | max|y - emul| {dev_e.max().item():.3e} | rel rms vs fp64 {rel:.3e}")
        if c.inst.iom & 2:
            assert (dev_e <= 1e-5 + 0.5 * ulp16(torch.maximum(emul.abs(), y.double().abs()))).all(), dev_e.max().item()
            c32 = c._replace(inst=P.dispatch(**dict(P.launch_args(c), io16=0, residual=False)))
            assert torch.equal(r.y, run(H, c32, d).y.half())
        else:
            assert dev_e.max().item() < 1e-5
        assert rel > 3e-5  # (the parity mode sits at ~2e-7)
    check_sink_and_record(P.case_id(c) + " benign", c, r)


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.TALL_CASES, ids=P.case_id)
def test_tall_shape_is_bit_identical_to_the_wide_shape(H, c):
    """proj_f16x2.hip states it and nothing pinned it: the Cout-channel launch (256-channel blocks) against Cout / 64 launches on the 64-channel slices of
    weight, bias and residual, which can only run the wide shape.  Both prologues, both plane counts, both down-sampling operands, on the benign data (every
    slice carries the layer's max|w|, hence its weight scale): outputs equal, the statistics rows of every group equal as bits, the largest of the slices'
    range records equal to the whole launch's."""
    d = data("benign", c)[0]
    cpg = c.cout // 8
    whole = run(H, c, d, cpg=cpg)
    ng, top = 64 // cpg, 0
    for s in range(c.cout // 64):
        sl = slice(64 * s, 64 * s + 64)
        ds = dict(d, w=d["w"][sl].contiguous(), b=d["b"][sl].contiguous(), res=None if d["res"] is None else d["res"][:, sl].contiguous())
        cs = c._replace(cout=64, inst=c.inst._replace(tall=0))
        assert P.dispatch(**P.launch_args(cs)) == cs.inst
        part = run(H, cs, ds, cpg=cpg)
        assert torch.equal(part.y, whole.y[:, sl]), f"{P.case_id(c)} slice {s}: max diff {(part.y - whole.y[:, sl]).abs().max().item():.3e}"
        assert torch.equal(part.stat.view(torch.int64), whole.stat[:, s * ng:(s + 1) * ng].contiguous().view(torch.int64)), f"{P.case_id(c)} slice {s}: statistics"
        if part.range is not None:
            assert part.range[0].item() == 7
            top = max(top, part.range[1].item())
    if whole.range is not None:
        assert whole.range.tolist() == [7, top]
    print(f"proj-instantiations | c tall = wide | {P.inst_id(c.inst)} | {c.cin}->{c.cout} {c.h}x{c.w} B{c.B} | {c.cout // 64} slices bit-identical")


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------------
def two_sources(H, c, x, seam):
    """x[:, :seam] and x[:, seam:] in two allocations of the launch's storage type, each between NaN-filled guard planes."""
    dt = torch.float16 if c.inst.iom & 1 else torch.float32
    guard = c.h * c.w
    keep0, xa = H.guarded((c.B, seam, c.h, c.w), dt, guard, DEV)
    keep1, xb = H.guarded((c.B, c.cin - seam, c.h, c.w), dt, guard, DEV)
    xa.copy_(x[:, :seam])
    xb.copy_(x[:, seam:])
    return xa, xb, lambda: H.guard_intact(keep0, guard) and H.guard_intact(keep1, guard)


@pytest.mark.parametrize("seam", P.SEAMS)
@pytest.mark.parametrize("mode", list(P.CONCAT_MODES))
@pytest.mark.parametrize("cout", [128, 256])
def test_two_allocation_input_with_seams_inside_the_chunks(H, cout, mode, seam):
    """Src::p1 at Cin = 96: a seam inside the first chunk, on a chunk boundary, inside the second and inside the third chunk; wide and tall, both prologues,
    both plane counts, and fp16 storage (half sources between half guard planes: the X16 loader's own seam arithmetic).  Bit-equal to the one-source
    launch -- output, statistics, range record -- on the exact grid and on the benign data; on the exact grid also bit-equal to fp64; with fp16 storage
    also RNE_f16 of the fp32-storage launch.  No guard plane is read (y finite) or written."""
    c = P.concat_case(cout, mode)
    for kind in ("exact", "benign"):
        d, ref, _ = data(kind, c)
        xa, xb, intact = two_sources(H, c, dev(d["x"]), seam)
        one = run(H, c, d, cpg=sink_cpg(c))
        two = run(H, c, d, x=xa, x1=xb, cpg=sink_cpg(c))
        label = f"{P.case_id(c)} {seam}|{c.cin - seam} {kind}"
        assert torch.isfinite(two.y).all(), f"{label}: a guard plane was read"
        assert torch.equal(two.y, one.y), f"{label}: max diff {(two.y.float() - one.y.float()).abs().max().item():.3e}"
        assert torch.equal(two.range, one.range)
        if one.stat is not None:
            assert torch.equal(two.stat.view(torch.int64), one.stat.view(torch.int64)), f"{label}: statistics"
        if c.inst.iom:
            c32 = c._replace(inst=P.dispatch(96, cout, c.h, c.w, pieces=1))
            assert torch.equal(two.y, run(H, c32, d).y.half()), label
        if kind == "exact":
            assert torch.equal(two.y.cpu(), P.stored(c, ref)), f"{label}: max |y - fp64| {max_err(two.y, ref):.3e}"
        assert intact(), f"{label}: a guard plane was written"


@pytest.mark.parametrize("mode", list(P.CONCAT_MODES))
def test_seam_inside_a_threads_eight_channels_stays_refused(H, mode):
    """c0 = 20: a staging thread's 8 channels would straddle the seam.  The entry refuses it itself (conv2d_ring_impl in kernel_abi.hip: "the concat seam
    must lie on an 8-channel boundary", the condition of launch_proj_f16x2), before the weights are packed: y, the range record, the packed buffer and --
    where the mode takes one; both shapes of the call are made -- the sink are untouched (the wrapper checks)."""
    c = P.concat_case(128, mode)
    d = data("benign", c)[0]
    x = dev(d["x"])
    if c.inst.iom & 1:
        x = x.half()
    run(H, c, d, x=x[:, :24].contiguous(), x1=x[:, 24:].contiguous())
    for cpg in {None, sink_cpg(c)}:
        with pytest.raises(R2DMError):
            run(H, c, d, x=x[:, :P.SEAM_REFUSED].contiguous(), x1=x[:, P.SEAM_REFUSED:].contiguous(), cpg=cpg)


# ---- (e) -----------------------------------------------------------------------------------------------------------------------------------
HOOK_REFUSALS = {"IO16 = 1 alone": dict(io16=1), "IO16 = 2 alone": dict(io16=2), "IO16 = 3 with a residual": dict(io16=3, residual=True),
                 "IO16 = 3 with prologue 1": dict(io16=3, prologue=1), "IO16 = 3 with a statistics sink": dict(io16=3, stat=True)}


@pytest.mark.parametrize("what", list(HOOK_REFUSALS))
@pytest.mark.parametrize("shape", [(32, 64, 4, 64, 1), (32, 256, 4, 64, 2)], ids=["Cout64", "Cout256"])
def test_fp16_storage_hook_refusals(H, shape, what):
    """A shape that runs this kernel in the one-plane mode: the storage hook with one bit alone, or with what the fp16-storage instantiation does not
    have -- residual, prologue, statistics -- is an error raised by the entry before anything is launched: y, the sink, the range record and the
    packed-weight buffer still hold their fill (the wrapper checks all four)."""
    kw = HOOK_REFUSALS[what]
    cin, cout, h, w, B = shape
    ok = P.Case(P.Inst(0, P.PRO_NONE, 1, 3, 0, 0), "ring", *shape)
    assert P.dispatch(cin, cout, h, w, pieces=1, **kw) is None and P.dispatch(cin, cout, h, w, pieces=1, io16=3) == ok.inst
    d = data("benign", ok)[0]
    run(H, ok, d)  # (the shape does run with fp16 storage)
    with_res = P.benign_inputs(P.Case(P.Inst(0, P.PRO_AFFINE, 1, 0, 0, 0), "ring", *shape))
    H.set_conv_pieces(1)
    try:
        with H.env(R2DM_TEST_IO16=kw["io16"]):
            with pytest.raises(R2DMError):
                H.conv2d_ring_ex(dev(d["x"]), dev(d["w"]), dev(d["b"]), aff=dev(with_res["aff"]) if kw.get("prologue") else None, prologue=kw.get("prologue", 0),
                                 residual=dev(with_res["res"]) if kw.get("residual") else None, stat_groups=8 if kw.get("stat") else 0,
                                 stat_cpg=cout // 8 if kw.get("stat") else 0, range_init=(7, 0), io16=kw["io16"])
                pytest.fail(f"not refused: {what}")
    finally:
        H.set_conv_pieces(2)
