"""CPU tests of the earth mover's distance: the oracle against itself (tests/emd_oracle.py: the exact solver against a brute force and, where
installed, scipy; weak duality for random prices; the fp32 emulation of the kernel's auction inside the bars of tests/test_hip_emd.py), the
refusal of malformed arguments by the C ABI and by the Python layer, and geometry_eval.py's flags.  (The kernel: tests/test_hip_emd.py.)"""
import math

import numpy as np
import pytest
import torch

import emd_oracle as O


@pytest.mark.parametrize("n", range(1, 8))
def test_hungarian_equals_brute_force(n):
    for seed in range(4):
        C = O.cost_matrix(O.gaussian(10 * n + seed, n), O.gaussian(100 + 10 * n + seed, n))
        s, cost = O.hungarian(C)
        assert O.is_permutation(s, n) and cost == O.cost_of(C, s)
        assert abs(cost - O.brute_force(C)) <= 1e-12 * cost
    # ties: an integer matrix with many equal entries
    C = np.random.Generator(np.random.PCG64(n)).integers(0, 3, (n, n)).astype(np.float64)
    assert O.hungarian(C)[1] == O.brute_force(C)


@pytest.mark.parametrize("n", (64, 257))
def test_hungarian_equals_scipy(n):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for a, b in ((O.gaussian(1, n), O.gaussian(2, n)), (O.rings(1, n), O.rings(2, n))):
        C = O.cost_matrix(a, b)
        s, cost = O.hungarian(C)
        r, c = lsa(C)
        assert O.is_permutation(s, n) and abs(cost - C[r, c].sum()) <= 1e-12 * cost


def test_dual_bound_is_below_the_optimum_for_any_prices():
    g = np.random.Generator(np.random.PCG64(5))
    for n in (1, 2, 7, 40):
        C = O.cost_matrix(O.gaussian(n, n), O.gaussian(n + 50, n))
        best = O.hungarian(C)[1]
        for scale in (0.0, 1.0, 30.0, 1e4):
            for prices in (g.uniform(0, 1, n) * scale, g.standard_normal(n) * scale):
                assert O.dual_bound(C, prices) <= best * (1 + 1e-12) + 1e-9 * scale
    # and tight at the optimal duals of a 2 x 2 problem by hand: c = [[1, 3], [2, 1]], optimum 2 at the identity, prices 0
    assert O.dual_bound(np.array([[1.0, 3.0], [2.0, 1.0]]), np.zeros(2)) == 2.0


def test_generators_are_seeded_and_shaped():
    a = O.rings(3, 257)
    assert a.dtype == np.float32 and a.shape == (257, 4) and np.array_equal(a, O.rings(3, 257)) and not np.array_equal(a, O.rings(4, 257))
    r = np.linalg.norm(a[:, :3].astype(np.float64), axis=1)
    assert 1.5 < r.min() and r.max() < 35 and a[:, 2].min() > -1.8  # nothing below the ground plane 1.7 m under the sensor
    g = O.gaussian(3, 65, 0.05, 70.0)
    assert g.dtype == np.float32 and g.shape == (65, 4) and abs(g.mean() - 70.0) < 0.05


@pytest.mark.parametrize("name,n,eps", (("gaussian", 7, 0.01), ("gaussian", 65, 0.01), ("rings", 257, 0.01), ("clusters", 257, 1.7e-5)))
def test_fp32_emulation_of_the_auction_stays_inside_the_bar(name, n, eps):
    """The inputs of the GPU test, checked where no GPU is: the same auction in numpy fp32 certifies ``emd - lower <= eps + rho``."""
    a, b = {"gaussian": (O.gaussian(1, n), O.gaussian(2, n)), "rings": (O.rings(1, n), O.rings(2, n)),
            "clusters": (O.gaussian(1, n, 0.05, 70.0), O.gaussian(2, n, 0.05, 70.0))}[name]
    r = O.auction_fp32(a, b, eps)
    C = O.cost_matrix(a, b)
    assert r["converged"] and O.is_permutation(r["assignment"], n) and (r["prices"] >= 0).all()
    emd, lower, best = O.cost_of(C, r["assignment"]) / n, O.dual_bound(C, r["prices"]) / n, O.hungarian(C)[1] / n
    rho = 2.0 ** -20 * (C.max() + float(r["prices"].max()))
    print(name, n, "rounds", r["rounds"], "gap / eps", (emd - lower) / eps, "to the optimum", emd - best)
    assert lower <= best * (1 + 1e-12) and best <= emd * (1 + 1e-12) and emd - lower <= eps + rho
    assert r["rounds"] < (1 << 20) / 16


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the pointers here are made-up addresses)."""
    from r2dm_amd import _lib

    L = _lib.lib()
    limit = L.r2dm_emd_max_points()
    assert limit >= 2048 and 48 * limit <= 160 * 1024  # 48 bytes of LDS per point, one workgroup per pair
    base = dict(a=4096, a_offsets=8192, a_clouds=2, a_total=100, b=12288, b_offsets=16384, b_clouds=2, b_total=100, pairs=20480, P=2, max_points=64,
                eps=0.01, max_rounds=1 << 20, assignment=None, prices=None, out=28672, scratch=24576, status=32768)

    def emd(**kw):
        return L.r2dm_emd_pairs(*{**base, **kw}.values(), None), L.r2dm_last_error().decode()

    for null in ("a_offsets", "b_offsets", "pairs", "out", "scratch", "status"):
        rc, msg = emd(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for kw in (dict(a=None), dict(b=None), dict(a_clouds=0), dict(b_clouds=-1), dict(a_total=-1)):
        rc, msg = emd(**kw)
        assert rc == 1 and "at least one cloud" in msg, kw
    rc, msg = emd(max_points=limit + 1)
    assert rc == 1 and f"up to {limit} points" in msg
    for kw in (dict(P=0), dict(P=-3), dict(P=1 << 31), dict(max_points=0), dict(max_points=-1)):
        rc, msg = emd(**kw)
        assert rc == 1 and "num_pairs must be in" in msg, kw
    for eps in (0.0, -0.01, math.nan, math.inf, 1e-46, 1e39):
        rc, msg = emd(eps=eps)
        assert rc == 1 and "eps must be finite and > 0" in msg, eps
    for rounds in (0, -1):
        rc, msg = emd(max_rounds=rounds)
        assert rc == 1 and "max_rounds must be >= 1" in msg
    for name in ("a", "b"):
        rc, msg = emd(**{name: 4096 + 8})
        assert rc == 1 and "16-byte aligned" in msg, name
    for name in ("a_offsets", "b_offsets", "pairs", "out", "scratch", "status"):
        rc, msg = emd(**{name: 8192 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    for name in ("assignment", "prices"):
        rc, msg = emd(**{name: 4096 + 2})
        assert rc == 1 and "4-byte aligned" in msg, name

    f = L.r2dm_emd_pairs_scratch_bytes
    for empty in ((0, 64), (-1, 64), (1 << 31, 64), (2, 0), (2, -1), (2, limit + 1)):
        assert f(*empty) == 0, empty
    assert f(1, 1) == f(1, limit) == 8 and f(5, 2048) == 40 and f((1 << 31) - 1, 64) == 8 * ((1 << 31) - 1)  # one code per pair


def test_python_argument_errors():
    import r2dm_amd
    from r2dm_amd import _lib, geometry

    cpu = torch.zeros(2, 3, 4)
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        r2dm_amd.pairwise_emd(cpu, [3, 3])
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        r2dm_amd.emd_pairs(torch.zeros(3, 4), [0, 3], torch.zeros(3, 4), [0, 3])
    for kw, msg in ((dict(eps=0.0), "eps must be"), (dict(eps=-1.0), "eps must be"), (dict(eps=math.nan), "eps must be"),
                    (dict(eps=math.inf), "eps must be"), (dict(max_rounds=0), "max_rounds must be")):
        with pytest.raises(ValueError, match=msg):
            geometry._emd_knobs(**{"eps": 0.01, "max_rounds": 8, **kw})
    assert geometry._emd_knobs(1, 8.0) == (1.0, 8)
    assert geometry.EMD_STATUS == ("bad_pair", "unequal_counts", "non_finite", "eps_floor", "round_cap")
    # the counters' messages (what a device refusal is turned into), on CPU tensors
    code = torch.tensor([0, 5, 0, 5])
    with pytest.raises(_lib.R2DMError, match=r"2 pairs \[11, 13\] did not converge"):
        geometry._raise_on_emd_status(torch.tensor([0, 0, 0, 0, 2]), code, 0.01, 10, False)
    geometry._raise_on_emd_status(torch.tensor([0, 0, 0, 0, 2]), code, 0.01, 10, True)
    geometry._raise_on_emd_status(torch.zeros(5, dtype=torch.int64), code, 0.01, 0, False)
    for k, msg in enumerate(("do not check out", "differ in size", "non-finite", "below 2\\^-18")):
        status = torch.zeros(5, dtype=torch.int64)
        status[k] = 1
        with pytest.raises(ValueError, match=msg):
            geometry._raise_on_emd_status(status, torch.tensor([k + 1]), 0.01, 0, True)


def test_command_line_flags():
    import geometry_eval

    p = geometry_eval.build_parser()
    a = p.parse_args(["--sample_dir", "s", "--real_dir", "r"])
    assert (a.distance, a.emd_eps, a.emd_max_rounds) == ("cd_sq", 0.01, 1 << 20)
    b = p.parse_args(["--sample_dir", "s", "--real_dir", "r", "--distance", "cd_sq"])
    assert vars(a) == vars(b)
    assert (a.points, a.limit, a.seed, a.out, a.real_scans, a.ckpt, a.batch_size, a.num_workers) == (2048, 2000, 0, "geometry.json", None, None, 64, 4)
    a = p.parse_args(["--sample_dir", "s", "--real_dir", "r", "--distance", "emd", "--emd_eps", "0.001", "--emd_max_rounds", "5000"])
    assert (a.distance, a.emd_eps, a.emd_max_rounds, a.points) == ("emd", 0.001, 5000, 2048)
    with pytest.raises(SystemExit):
        p.parse_args(["--sample_dir", "s", "--real_dir", "r", "--distance", "cd"])
