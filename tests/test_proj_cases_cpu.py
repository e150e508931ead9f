"""The preconditions that tests/test_hip_proj.py relies on, asserted without a GPU: the table of proj_cases.py holds exactly the instantiations that
launch_proj_f16x2 can launch, every case reaches the instantiation it names through the mirrored dispatch rule, and the exact-grid generators deliver
what their name says -- the kernel's own arithmetic, repeated in fp32 in a random summation order, returns the fp64 result with no rounding at all."""
import pytest
import torch

import proj_cases as P


def test_the_table_is_the_set_of_instantiations_in_the_source():
    """Every launch_p1<...> inside launch_proj_f16x2: a new instantiation cannot arrive without a row (and a case) here."""
    found = P.source_instantiations()
    assert found == set(P.TABLE), (sorted(found - set(P.TABLE)), sorted(set(P.TABLE) - found))
    assert {c.inst for c in P.CASES} == set(P.TABLE)
    assert all(P.TABLE[c.inst] == c.entry for c in P.CASES)


def test_every_case_reaches_the_instantiation_it_names():
    for c in P.CASES:
        assert P.dispatch(**P.launch_args(c)) == c.inst, P.case_id(c)
        assert c.inst.tall == int(c.cout % 256 == 0) or c.inst.iom
    assert any(c.inst.iom and c.cout % 256 == 0 for c in P.CASES)  # the fp16-storage launch stays wide
    assert {P.gemm_shape(c)[0] // 32 for c in P.CASES if not P.is_down(c)} == {1, 3}  # a single K chunk, and an odd count in the steady state
    for cout in (128, 256):
        for mode, (pieces, pro, io16) in P.CONCAT_MODES.items():
            c = P.concat_case(cout, mode)
            assert c.inst is not None and c.inst.tall == int(cout == 256 and not io16) and c.inst.nplk == pieces and c.inst.pro == pro and c.inst.iom == io16
            for seam in P.SEAMS:
                assert P.dispatch(96, cout, 8, 128, pieces, pro, io16, residual=io16 == 0, seam=seam) == c.inst
            assert P.dispatch(96, cout, 8, 128, pieces, pro, io16, residual=io16 == 0, seam=P.SEAM_REFUSED) is None
    assert {s // 32 == (s - 1) // 32 for s in P.SEAMS} == {True, False} and all(s % 8 == 0 for s in P.SEAMS)  # seams inside chunks and on a boundary


def test_the_dispatch_mirror_refuses_what_the_launcher_refuses():
    one = dict(K=32, cout=64, h=4, w=64, pieces=1)
    assert P.dispatch(**one, io16=3) == P.Inst(0, 0, 1, 3, 0, 0)
    for bad in (dict(io16=1), dict(io16=2), dict(io16=3, residual=True), dict(io16=3, prologue=1), dict(io16=3, stat=True)):
        assert P.dispatch(**one, **bad) is None, bad
    assert P.dispatch(32, 64, 4, 64, pieces=2, io16=3) is None
    assert P.dispatch(288, 64, 4, 64, pieces=1, down="nine") is None and P.dispatch(288, 64, 4, 64, prologue=1, down="phase") is None
    assert P.dispatch(64, 64, 4, 64, down="phase") is None and P.dispatch(64, 64, 4, 64, down="nine") is not None
    assert P.dispatch(32, 64, 4, 64, prologue=2) is None


def test_the_mirror_agrees_with_the_engine_path_tests_conditions():
    """supports("proj_f16x2", ...) of test_hip_conv_engine_paths.py and proj_f16x2_supported as mirrored here are the same predicate."""
    from test_hip_conv_engine_paths import supports

    for cin in (8, 16, 32, 48, 64, 96, 100, 288):
        for cout in (32, 64, 96, 128, 256, 320):
            for h in (2, 4, 6, 8):
                for w in (32, 64, 96, 128):
                    assert P.supported(cin, cout, h, w) == supports("proj_f16x2", cin, cout, h, w)
                    assert (P.dispatch(cin, cout, h, w) is not None) == P.supported(cin, cout, h, w)


def on_grid(t, step):
    return bool((t.double() / step == (t.double() / step).round()).all())


@pytest.mark.parametrize("c", P.CASES + [P.concat_case(256, m) for m in P.CONCAT_MODES], ids=P.case_id)
def test_exact_grid_generators_are_exact(c):
    """The derivation of proj_cases.py's docstring on the data: the grids, no fp16 subnormal among the operands, sum_k |product| below 2^24 grid units for
    both accumulators (so every partial sum in every order is an fp32 number), wl = 0; then the kernel's arithmetic in fp32 in a random order equals the fp64
    reference rounded once; and the l plane is in use -- at least 20 % of the x operand's elements have l != 0 in the two-plane rows."""
    d = P.exact_inputs(c)
    xo = P.x_operand(c, d, torch.float64)
    assert torch.equal(P.x_operand(c, d, torch.float32).double(), xo)  # the affine and the FIR are exact in fp32 too
    assert on_grid(xo, 2.0 ** (-12 if c.inst.nplk == 2 else -9)) and xo.abs().max().item() <= 3
    if c.inst.nplk == 1:
        assert torch.equal(xo.float().half().double(), xo)  # h = v
    xh, xl = P.split_f16x2(xo.float())
    assert torch.equal((xh.double() + xl.double() / 2048), xo)
    for t in (xh, xl):
        assert not ((t != 0) & (t.abs() < 2.0 ** -14)).any()
    assert on_grid(xl, 0.5) and xl.abs().max().item() <= 2
    wm = P.weight_matrix(c, d["w"])
    assert P.weight_scale(wm) == 256 and all(wm[s:s + 64].abs().max().item() == 2 for s in range(0, c.cout, 64))
    assert torch.equal(P.f16_round_weights(wm), wm.double())
    assert on_grid(d["b"], 2.0 ** -12) and d["b"].abs().max().item() <= 1 and (d["res"] is None or (on_grid(d["res"], 2.0 ** -12) and d["res"].abs().max().item() <= 1))
    assert (d["res"] is None) == (not P.takes_residual(c)) and (d["aff"] is None) == (c.inst.pro == 0)
    ref, err32 = P.references(c, d)
    y, l_share, (hh, cross), _ = P.emulate(c, d)
    print(f"{P.case_id(c)}: l != 0 in {100 * l_share:.1f} % of the x operand; sum|products| hh 2^{torch.tensor(hh).log2().item():.1f}, cross "
          f"2^{torch.tensor(max(cross, 1.0)).log2().item():.1f} grid units; max|ref| {ref.abs().max().item():.1f}; fp32 torch error {err32:.1e}")
    assert hh < 2.0 ** 24 and cross < 2.0 ** 24
    assert torch.equal(ref.float().double(), ref) and ref.abs().max().item() < 2.0 ** 11  # the result itself is an fp32 number
    assert torch.equal(y, P.stored(c, ref))
    if c.inst.nplk == 2:
        assert l_share >= 0.20, l_share


@pytest.mark.parametrize("c", P.SPLIT_WEIGHT_CASES, ids=P.case_id)
def test_exact_grid_with_split_weights_is_exact(c):
    """The counterpart of the exact grid for the weights' l plane (exact_inputs_split_weights): twelve-bit weights at scale 2^10 with wl != 0 in at least 20 %
    of them, a coarse x operand, the same sum bound for both accumulators, and the kernel's arithmetic in a random order equal to fp64 rounded once."""
    d = P.exact_inputs_split_weights(c)
    xo = P.x_operand(c, d, torch.float64)
    assert on_grid(xo, 0.25) and xo.abs().max().item() <= 3 and torch.equal(P.x_operand(c, d, torch.float32).double(), xo)
    wm = P.weight_matrix(c, d["w"])
    assert P.weight_scale(wm) == 1024 and on_grid(wm * 1024, 0.25) and all(wm[s:s + 64].abs().max().item() == 4095 / 4096 for s in range(0, c.cout, 64))
    wh, wl = P.split_f16x2(wm * 1024)
    assert torch.equal(wh.double() + wl.double() / 2048, wm.double() * 1024) and set(wl.unique().tolist()) == {-512.0, 0.0, 512.0}
    ref, err32 = P.references(c, d)
    y, l_share, (hh, cross), wl_share = P.emulate(c, d)
    print(f"{P.case_id(c)}: wl != 0 in {100 * wl_share:.1f} % of the weights; sum|products| hh 2^{torch.tensor(hh).log2().item():.1f}, cross "
          f"2^{torch.tensor(cross).log2().item():.1f} grid units; max|ref| {ref.abs().max().item():.1f}; fp32 torch error {err32:.1e}")
    assert hh < 2.0 ** 24 and cross < 2.0 ** 24 and l_share == 0 and wl_share >= 0.20
    assert torch.equal(ref.float().double(), ref) and torch.equal(y, P.stored(c, ref))


@pytest.mark.parametrize("c", [c for c in P.CASES if c.inst.nplk == 1 and c.inst.pro], ids=P.case_id)
def test_benign_one_plane_affine_is_exact_in_fp32(c):
    """The one-plane emulation's precondition: x a + d of the benign one-plane rows is an fp32 number, so FMA contraction cannot change what is rounded to fp16."""
    d = P.benign_inputs(c)
    xo = P.x_operand(c, d, torch.float64)
    assert torch.equal(xo.float().double(), xo) and torch.equal(P.x_operand(c, d, torch.float32).double(), xo)
    assert not torch.equal(xo.float().half().double(), xo)  # ... and the rounding to fp16 is a real one
    P.one_plane_emulation(c, d)


def test_down_reference_is_the_oracles_composition():
    """proj_cases.result for a down-sampling row is Resample(down=2)(Conv3x3(x) + b) of the oracle, in fp64."""
    from oracle import r2dm_oracle as O

    c = next(c for c in P.CASES if P.is_down(c) and c.cout == 64)
    d = P.benign_inputs(c)
    want = O.fir_down2(O.conv_ring(d["x"].double(), d["w"].double(), d["b"].double()))
    assert (P.result(c, d) - want).abs().max().item() < 1e-12


def test_benign_weights_carry_the_layers_scale_in_every_slice():
    for c in P.TALL_CASES:
        wm = P.weight_matrix(c, P.benign_inputs(c)["w"])
        assert len({P.weight_scale(wm[s:s + 64]) for s in range(0, c.cout, 64)} | {P.weight_scale(wm)}) == 1
