"""CPU tests of the BEV metrics' host side: evaluate.py's CLI and the no-fallback rule of r2dm_amd.metrics."""
import subprocess
import sys

import pytest
import torch

from conftest import ROOT


def test_evaluate_help_lists_the_reference_options():
    r = subprocess.run([sys.executable, "evaluate.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--ckpt", "--sample_dir", "--dataset", "--batch_size", "--num_workers", "--real_set", "--real_dir"):
        assert opt in r.stdout, opt
    assert "{train,test,all}" in r.stdout


def test_metrics_refuse_cpu_tensors():
    from r2dm_amd import _lib, metrics

    h = torch.ones(4, 100, 100)
    for call in (lambda: metrics.bev_histograms(torch.zeros(2, 5, 16, 128)),
                 lambda: metrics.bev_histograms(torch.zeros(2, 64, 3)),
                 lambda: metrics.point_cloud_to_histogram(torch.zeros(64, 3)),
                 lambda: metrics.compute_jsd_2d(h, h),
                 lambda: metrics.compute_mmd_2d(h, h)):
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            call()


def test_metric_bin_edges_are_histogramdds():
    from r2dm_amd import metrics

    x = torch.zeros(1, 2)
    for field, bins in ((160.0, 100), (100.0, 64)):
        b = field / 2
        assert torch.equal(metrics.bin_edges(field, bins), torch.histogramdd(x, bins=bins, range=[-b, b, -b, b]).bin_edges[0])
