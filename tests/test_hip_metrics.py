"""-m gpu: the BEV metrics of evaluate.py (r2dm_amd.metrics, metrics.hip) against the reference's outputs
(tests/golden/bev_metrics.npz, tests/golden/make_golden_metrics.py) and fp64 oracles."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_metrics as G  # noqa: E402  (the fixture's integer-only input generators)

from r2dm_amd import metrics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "bev_metrics.npz")) as z:
        return {k: z[k] for k in z.files}


def cpu_histogram(pc, field_size=160.0, bins=100, lo=3.0, hi=70.0):
    """The histogram as the reference computes it: CPU norm, depth window, torch.histogramdd of (x, y)."""
    d = pc.norm(p=2, dim=1)
    keep = (d > lo) & (d < hi)
    b = field_size / 2
    return torch.histogramdd(pc[keep, 0:2], bins=bins, range=[-b, b, -b, b]).hist


@pytest.mark.parametrize("name", [c[0] for c in G.CLOUD_CASES])
def test_edge_case_histograms_match_reference(fx, name):
    field, bins, lo, hi = fx[f"params_{name}"]
    pc = torch.from_numpy(fx["cloud_depths" if name == "depths" else "cloud_edges"]).to(DEV)
    h = metrics.bev_histograms(pc[None], field_size=float(field), bins=int(bins), min_depth=float(lo), max_depth=float(hi))[0]
    want = fx[f"hist_{name}"].astype(np.int64)
    assert h.dtype == torch.int32 and h.shape == want.shape
    assert np.array_equal(h.cpu().numpy(), want), np.abs(h.cpu().numpy() - want).sum()
    assert want.sum() > 0
    one = metrics.point_cloud_to_histogram(pc, float(field), int(bins), float(lo), float(hi))
    assert one.dtype == torch.float32 and np.array_equal(one.cpu().numpy(), want)


def test_full_size_fixture_clouds_match_reference(fx):
    clouds = torch.stack([torch.from_numpy(G.full_cloud(s)) for s in G.FULL_SEEDS]).to(DEV)
    h, total = metrics.bev_histograms(clouds, return_sum=True)
    want = np.stack([fx[f"hist_full_{s}"].astype(np.int64) for s in G.FULL_SEEDS])
    assert np.array_equal(h.cpu().numpy(), want)
    assert total.dtype == torch.int64 and np.array_equal(total.cpu().numpy(), want.sum(0))


def test_sample_layout_matches_reference_and_cloud_path(fx):
    img = torch.from_numpy(fx["images"]).to(DEV)
    h = metrics.bev_histograms(img)
    assert np.array_equal(h.cpu().numpy(), fx["hist_images"].astype(np.int64))
    # the same after evaluate.py's masking, through the point-cloud layout
    depth = img[:, [0]]
    mask = ((depth > metrics.MIN_DEPTH) & (depth < metrics.MAX_DEPTH)).float()
    clouds = (img[:, 1:4] * mask).flatten(2).transpose(1, 2)
    assert torch.equal(metrics.bev_histograms(clouds), h)


def test_random_full_size_clouds_bit_identical_to_histogramdd():
    """1,024 clouds of 64 x 1024 points, against torch.histogramdd per cloud on the CPU (split over batches of 256)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(4):
        pcs = torch.randn(256, 64 * 1024, 3, device=DEV, generator=g) * torch.rand(256, 64 * 1024, 1, device=DEV, generator=g) * 60
        pcs[:, ::7] = 0.0
        h, total = metrics.bev_histograms(pcs, return_sum=True)
        got = h.cpu()
        for i, pc in enumerate(pcs.cpu()):
            assert torch.equal(got[i].to(torch.float32), cpu_histogram(pc)), i
        assert torch.equal(total.cpu(), got.to(torch.int64).sum(0))


def _pair(row):
    sp, sq, n_p, n_q, shift = (int(v) for v in row[:5])
    return (torch.from_numpy(G.mmd_hists(sp, n_p, 0)).to(DEV), torch.from_numpy(G.mmd_hists(sq, n_q, shift)).to(DEV))


def test_mmd_against_fp64_oracle_and_reference_error(fx):
    for row in fx["pairs"]:
        P, Q = _pair(row)
        mmd_ref, mmd_64, ref_err = row[8], row[9], row[10]
        got = metrics.compute_mmd_2d(P, Q)
        err = abs(got - mmd_64)
        assert err <= 1e-6 * abs(mmd_64) and err <= ref_err / 20, (row[:5], got, mmd_64, err, ref_err)
        # int32 counts, as bev_histograms returns them, give the same bits
        assert metrics.compute_mmd_2d(P.to(torch.int32), Q.to(torch.int32).view(-1, 100, 100)) == got


def test_jsd_against_fp64_oracle_and_reference(fx):
    for row in fx["pairs"]:
        P, Q = _pair(row)
        jsd_ref, jsd_64, ref_err = row[5], row[6], row[7]
        got = metrics.compute_jsd_2d(P, Q)
        assert isinstance(got, float)
        assert abs(got - jsd_64) <= 1e-12, (got, jsd_64)
        assert abs(got - jsd_ref) <= ref_err + 1e-12, (got, jsd_ref, ref_err)
        assert metrics.compute_jsd_2d(P.to(torch.int32), Q.to(torch.int32)) == got


def _mmd_fp64(P, Q, chunk=256):
    """Chunked fp64 MMD on the GPU: d^2 = |p|^2 + |q|^2 - 2 p.q in fp64 (relative error ~1e-13 at these magnitudes)."""
    p = P.double() / P.double().sum(1, keepdim=True)
    q = Q.double() / Q.double().sum(1, keepdim=True)

    def mean_1mk(a, b):
        s = 0.0
        nb = (b * b).sum(1)
        for i in range(0, len(a), chunk):
            x = a[i:i + chunk]
            d2 = ((x * x).sum(1)[:, None] + nb[None] - 2 * x @ b.T).clamp_min(0)
            s += (-torch.expm1(-2.0 * d2)).sum().item()
        return s / (len(a) * len(b))

    return 2 * mean_1mk(p, q) - mean_1mk(p, p) - mean_1mk(q, q)


def test_mmd_2048_x_2048_full_bins_and_determinism():
    P = torch.from_numpy(np.concatenate([G.mmd_hists(301 + i, 256, 0) for i in range(8)])).to(DEV)
    Q = torch.from_numpy(np.concatenate([G.mmd_hists(401 + i, 256, 1) for i in range(8)])).to(DEV)
    assert P.shape == Q.shape == (2048, 10_000)
    got = metrics.compute_mmd_2d(P, Q)
    want = _mmd_fp64(P, Q)
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert metrics.compute_mmd_2d(P, Q) == got  # fixed reduction order: the same bits
    assert metrics.mmd_terms(P, Q) == metrics.mmd_terms(P, Q)


def test_mmd_of_a_permutation_is_zero():
    H = torch.from_numpy(G.mmd_hists(501, 300, 0)).to(DEV)
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert abs(metrics.compute_mmd_2d(H, H[perm])) <= 1e-12


def test_all_zero_row_gives_nan():
    H = torch.from_numpy(G.mmd_hists(601, 40, 0)).to(DEV)
    Z = H.clone()
    Z[3] = 0
    assert np.isnan(metrics.compute_mmd_2d(Z, H))
    assert np.isnan(metrics.compute_mmd_2d(H[:5], Z[3:4]))  # a one-row set too (the reference's 0/0)
    assert np.isfinite(metrics.compute_mmd_2d(H[:5], H[5:]))
