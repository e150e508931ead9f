"""-m gpu: evaluate.py (BEV part) end to end on files written by sample_and_save.py from a synthetic checkpoint."""
import json
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_RES, ROOT, synthetic_ckpt

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    r = subprocess.run([sys.executable, f"{ROOT}/evaluate.py"] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _result(sample_dir, before):
    new = sorted(set(sample_dir.parent.glob(sample_dir.name + "_*.json")) - before)
    assert len(new) == 1, new
    return json.loads(new[0].read_text())


def test_evaluate_real_dir_and_reference_cache_agree_with_api(tmp_path):
    from r2dm_amd import metrics
    from r2dm_amd.option import Config

    ckpt = tmp_path / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    gen, real = tmp_path / "gen", tmp_path / "real"
    for out, n in ((gen, 3), (real, 4)):
        subprocess.run([sys.executable, "sample_and_save.py", "--ckpt", str(ckpt), "--output_dir", str(out), "--batch_size", "2",
                        "--num_samples", str(n), "--num_steps", "2"], cwd=ROOT, check=True, timeout=600)
    # a second real set: the reference's cache pickle, under its own name in the working directory
    gen_files, real_files = sorted(gen.glob("*.pth")), sorted(real.glob("*.pth"))
    load = lambda fs: torch.stack([torch.load(f) for f in fs]).cuda()
    h_gen, h_real = metrics.bev_histograms(load(gen_files)), metrics.bev_histograms(load(real_files))
    cfg = Config(**torch.load(ckpt)["cfg"])
    H, W = GOLDEN_RES
    cache = tmp_path / f"real_set_{cfg.data.dataset}_{cfg.data.projection}_{H}x{W}_test.pkl"
    with open(cache, "wb") as f:
        pickle.dump(dict(img_feats=np.zeros((4, 8), np.float32), pts_feats=np.zeros((4, 8), np.float32),
                         bev_hists=h_real.float().cpu().numpy()), f)

    # the API on the same files, with the reference's subset order (random.Random(0) over the real set)
    import random

    perm = list(range(4))
    random.Random(0).shuffle(perm)
    want_jsd = metrics.compute_jsd_2d(h_real[perm], h_gen)
    want_mmd = metrics.compute_mmd_2d(h_real[perm], h_gen)
    assert h_gen.sum() > 0 and h_real.sum() > 0

    before = set(tmp_path.glob("gen_*.json"))
    _run(["--ckpt", str(ckpt), "--sample_dir", str(gen), "--dataset", "test", "--batch_size", "2", "--num_workers", "0",
          "--real_dir", str(real)], cwd=tmp_path)
    a = _result(gen, before)
    before |= set(tmp_path.glob("gen_*.json"))
    _run(["--ckpt", str(ckpt), "--sample_dir", str(gen), "--dataset", "test", "--batch_size", "2", "--num_workers", "0"], cwd=tmp_path)
    b = _result(gen, before)

    for r in (a, b):
        assert set(r) == {"img", "pts", "bev", "info"} and r["img"] == {} and r["pts"] == {}
        assert r["info"]["phase"] == "test" and r["info"]["directory"] == str(gen)
        assert r["info"]["#real"] == 4 and r["info"]["#fake"] == 3
        assert r["bev"]["jsd"] == want_jsd and r["bev"]["mmd"] == want_mmd
    assert a["bev"] == b["bev"]
