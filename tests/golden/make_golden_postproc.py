#!/usr/bin/env python3
"""Generate tests/golden/postproc.npz by running the REAL reference's ``kNN`` and ``CRFRNN`` (metrics/extractor/rangenet.py) on the CPU,
in fp32 and in fp64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_postproc.py /path/to/reference

torchvision, which the reference module imports for its Preprocess, is replaced by a stub.  The reference's ``kNN`` cannot run after
``.double()`` (its ``label_bins`` is created in the default dtype): its fp64 pass is built and run under
``torch.set_default_dtype(torch.float64)``.

Contents (data only):
  - kNN, for every case of ``KNN_CASES``: ``knn32_* `` / ``knn64_*`` = the reference's fp32 / fp64 labels (uint8); for the stored cases
    also the inputs ``depth_*`` / ``label_*`` (the 64 x 1024 ones are regenerated from integer draws by ``knn_scene``);
  - ``gauss_3`` / ``gauss_5``: the reference's ``dist_kernel`` (1 - Gaussian); ``kernel_gamma``: its default smoothness kernel (20,20,3,5);
  - CRF-RNN, for every case of ``CRF_CASES``: ``err_crf_*`` = [rms, max] of the reference's fp32 run against its fp64 run; for the stored
    cases the inputs ``unary_*`` / ``xyz_*`` / ``mask_*`` and the fp64 result ``q64_*``; ``crfstate_custom_*``: the reference module's
    state dict of the "custom" case;
  - ``crf_keys`` / ``crf_shapes``: the reference module's state-dict keys and shapes (20 classes, the default window);
  - ``hub``: JSON, the parameter names and defaults of the reference's five hub entries and of its two post-processor classes.
Asserted here: tests/postproc_oracle.py in fp64 equals the reference's fp64 labels on every pixel and its Q to 1e-12; the fp32 restatement
equals the reference's fp32 labels on the sure pixels, which are at least 99 %; on the theta_beta = 0.5 cases the appearance term's rms is at
least a tenth of the smoothness term's; the reference's fp32 argmax equals its fp64 argmax wherever the fp64 top-two margin exceeds 8x its
max error, and those pixels are at least 99 %."""
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "postproc.npz")

NUM_CLASSES = 20
MARGIN, MAX_EXCLUDED = 8.0, 0.01
# name, seed, shape (B,H,W), window, k, cutoff, stored, kind.  The 1 % cap on the pixels left out is a condition on the INPUTS, asserted in main: with
# the 5 x 5 window a scene lands between 0.4 % and 1.0 %, and the seeds 82 (2.75 % of 400 pixels) and 84 (1.001 %) were passed over for it.
KNN_CASES = [
    ("edge", 81, (3, 7, 70), 3, 3, 1.0, True, "scene"),
    ("win5", 182, (2, 5, 40), 5, 5, 1.0, True, "scene"),
    ("flat", 83, (1, 2, 33), 3, 3, 1.0, True, "scene"),    # H smaller than the window
    ("full3", 284, (1, 64, 1024), 3, 3, 1.0, False, "scene"),
    ("full5", 284, (1, 64, 1024), 5, 5, 1.0, False, "scene"),
    ("void", 85, (1, 4, 40), 3, 3, 1.0, True, "void"),     # an image of only -1
    # cutoff = 0: nobody is discarded.  Every depth is valid: without a cutoff two infinite distances at the k-th place are a tie between two
    # VOTES, which the reference's unsorted topk resolves as it likes and this project in favour of the lower offset
    ("nocut", 86, (3, 7, 70), 3, 3, 0.0, True, "valid"),
]
# name, seed, shape (B,N,H,W), window, iterations, stored, parameters
CRF_CASES = [
    ("default", 91, (2, 20, 6, 70), (3, 5), 3, True, "default"),
    ("custom", 91, (2, 20, 6, 70), (3, 5), 3, True, "custom"),
    ("small", 92, (1, 5, 3, 33), (3, 3), 1, True, "beta"),
    ("full", 93, (1, 20, 64, 1024), (3, 5), 3, False, "beta"),
]


def knn_scene(seed, shape, kind="scene"):
    """(depth (B,1,H,W) fp32, label (B,H,W) int64) from integer draws.  Per row, segments of 8 - 47 columns with one base depth in [2, 60)
    on a 2^-10 grid and one label; a row is the row above with probability 3/4; noise integers(-512, 512) / 2^12; 2 % of the pixels
    are -1 (kind "valid": none is); 20 % of the labels are redrawn.  (Uniformly random depths would make every vote a discard.)"""
    g = np.random.Generator(np.random.PCG64(seed))
    B, H, W = shape
    if kind == "void":
        return np.full((B, 1, H, W), -1.0, np.float32), g.integers(0, NUM_CLASSES, size=(B, H, W)).astype(np.int64)
    base = np.empty((B, H, W), np.float64)
    label = np.empty((B, H, W), np.int64)
    for b in range(B):
        for h in range(H):
            if h > 0 and g.integers(0, 4) != 0:
                base[b, h], label[b, h] = base[b, h - 1], label[b, h - 1]
                continue
            w = 0
            while w < W:
                n = int(g.integers(8, 48))
                base[b, h, w:w + n] = g.integers(2 * 2**10, 60 * 2**10) / 2**10
                label[b, h, w:w + n] = g.integers(0, NUM_CLASSES)
                w += n
    depth = base + g.integers(-512, 512, size=(B, H, W)) / 2**12
    invalid = g.integers(0, 50, size=(B, H, W)) == 0
    if kind != "valid":
        depth[invalid] = -1.0
    redraw = g.integers(0, 5, size=(B, H, W)) == 0
    label[redraw] = g.integers(0, NUM_CLASSES, size=int(redraw.sum()))
    return depth.astype(np.float32)[:, None], label


def crf_inputs(seed, shape):
    """(unary (B,N,H,W), xyz (B,3,H,W), mask (B,H,W)) fp32 from integer draws: unary integers(-2^12, 2^12) / 2^9; xyz = ring-wise depths
    (one base depth per ring in [4, 40), noise integers(-64, 64) / 2^10) along a 64-beam ray grid whose directions are rational in the
    half-angle tangents (only + - x / in fp64: the same bits everywhere); the mask is 90 % ones and xyz is multiplied by it."""
    g = np.random.Generator(np.random.PCG64(seed))
    B, N, H, W = shape
    unary = g.integers(-2**12, 2**12, size=shape) / 2**9
    beam = (np.arange(H) * 64) // H
    te = 0.03 - 0.25 * beam / 63.0                     # tan(elevation / 2): about +3 .. -25 degrees
    ta = (2.0 * np.arange(W) + 1.0 - W) / W            # tan(azimuth / 2): a half circle
    ce, se = (1 - te * te) / (1 + te * te), 2 * te / (1 + te * te)
    ca, sa = (1 - ta * ta) / (1 + ta * ta), 2 * ta / (1 + ta * ta)
    rays = np.stack([ce[:, None] * ca[None, :], ce[:, None] * sa[None, :], se[:, None] * np.ones(W)[None, :]])  # (3,H,W)
    depth = g.integers(4 * 2**8, 40 * 2**8, size=(B, H, 1)) / 2**8 + g.integers(-64, 64, size=(B, H, W)) / 2**10
    mask = (g.integers(0, 10, size=(B, H, W)) != 0).astype(np.float64)
    xyz = depth[:, None] * rays[None] * mask[:, None]
    return unary.astype(np.float32), xyz.astype(np.float32), mask.astype(np.float32)


def crf_kwargs(params, num_classes):
    """The constructor arguments of a CRF case (the same for the reference's CRFRNN and r2dm_amd.postproc.CRFRNN)."""
    if params == "default":
        return {}
    if params == "beta":
        return dict(theta_beta=0.5, init_weight_smoothness=0.2, init_weight_appearance=1.0)
    assert params == "custom"
    per_class = lambda lo, step: tuple(lo + step * c for c in range(num_classes))
    return dict(theta_beta=per_class(0.5, 1 / 128), init_weight_smoothness=0.2, init_weight_appearance=1.0,
                theta_gamma=per_class(0.75, 1 / 64), theta_alpha=per_class(1.25, -1 / 64))


def custom_compatibility(num_classes):
    """A random non-Potts compatibility matrix from integer draws, (N,N,1,1) fp32."""
    g = np.random.Generator(np.random.PCG64(99))
    return (g.integers(-2**8, 2**8, size=(num_classes, num_classes, 1, 1)) / 2**8).astype(np.float32)


def _signature(fn):
    return [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name] for p in inspect.signature(fn).parameters.values()]


def main(reference):
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))  # (only Preprocess uses it)
    sys.path.insert(0, reference)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from metrics.extractor import rangenet as ref  # (reference)

    import postproc_oracle as O

    torch.manual_seed(0)
    out = {}

    # ---- kNN ------------------------------------------------------------------------------------------------------------------
    for name, seed, shape, ks, k, cutoff, stored, kind in KNN_CASES:
        depth, label = (torch.from_numpy(a) for a in knn_scene(seed, shape, kind))
        with torch.no_grad():
            r32 = ref.kNN(NUM_CLASSES, k=k, kernel_size=ks, cutoff=cutoff)(depth.clone(), label.clone())
            torch.set_default_dtype(torch.float64)
            try:
                m64 = ref.kNN(NUM_CLASSES, k=k, kernel_size=ks, cutoff=cutoff)
                assert m64.dist_kernel.dtype == torch.float64
                r64 = m64(depth.double(), label.clone())
            finally:
                torch.set_default_dtype(torch.float32)
        w32, w64 = O.knn_weight(ks, 1.0, torch.float32), O.knn_weight(ks, 1.0, torch.float64)
        assert torch.equal(w64, m64.dist_kernel[0, 0]), "the oracle's weights differ from the reference's"
        d32, d64 = O.knn_dist(depth, w32), O.knn_dist(depth, w64)
        o32, o64 = O.knn_vote(d32, label, ks, k, cutoff, NUM_CLASSES), O.knn_vote(d64, label, ks, k, cutoff, NUM_CLASSES)
        assert torch.equal(o64, r64), f"{name}: the fp64 oracle differs from the reference's fp64 labels"
        sure, margin = O.knn_sure(d64, d32, k, cutoff)
        excluded = 1 - sure.double().mean().item()
        assert torch.equal(o32[sure], r32[sure]) and torch.equal(o32[sure], r64[sure]) and excluded <= MAX_EXCLUDED, (name, excluded)
        changed = (r64 != label).double().mean().item()
        print(f"knn {name}: {tuple(shape)} window {ks} k {k} cutoff {cutoff}: excluded {excluded:.2%} (margin {margin:.2e}); fp32 restatement "
              f"== reference fp32 on {'every pixel' if torch.equal(o32, r32) else f'{(o32 == r32).double().mean().item():.4%}'}; "
              f"labels changed by the filter {changed:.1%}, zero labels out {(r64 == 0).double().mean().item():.1%}")
        if kind != "void":
            assert 0.05 < changed < 0.6, "the scene must give the filter something to do"
        out[f"knn32_{name}"], out[f"knn64_{name}"] = r32.numpy().astype(np.uint8), r64.numpy().astype(np.uint8)
        if stored:
            out[f"depth_{name}"], out[f"label_{name}"] = depth.numpy(), label.numpy().astype(np.uint8)
    out["gauss_3"] = ref.kNN(NUM_CLASSES, kernel_size=3).dist_kernel[0, 0].numpy()
    out["gauss_5"] = ref.kNN(NUM_CLASSES, kernel_size=5).dist_kernel[0, 0].numpy()

    # ---- CRF-RNN --------------------------------------------------------------------------------------------------------------
    m = ref.CRFRNN(NUM_CLASSES)
    out["kernel_gamma"] = m.kernel_gamma.numpy()
    out["crf_keys"] = np.array(list(m.state_dict()))
    out["crf_shapes"] = np.array([",".join(str(n) for n in v.shape) for v in m.state_dict().values()])
    for name, seed, shape, ks, iters, stored, params in CRF_CASES:
        N = shape[1]
        unary, xyz, mask = (torch.from_numpy(a) for a in crf_inputs(seed, shape))
        m32 = ref.CRFRNN(N, kernel_size=ks, num_iters=iters, **crf_kwargs(params, N))
        if params == "custom":
            m32.label_compatibility.weight.data = torch.from_numpy(custom_compatibility(N))
        state = {k: v.detach().clone() for k, v in m32.state_dict().items()}
        m64 = ref.CRFRNN(N, kernel_size=ks, num_iters=iters, **crf_kwargs(params, N))
        m64.load_state_dict(state)
        m64.double()
        with torch.no_grad():
            q32, q64 = m32(unary, xyz, mask), m64(unary.double(), xyz.double(), mask.double())
            trace = []
            o64 = O.crf(unary, xyz, mask, state, ks, iters, torch.float64, trace)
            o32 = O.crf(unary, xyz, mask, state, ks, iters, torch.float32)
        rel = (o64 - q64).abs().max().item() / q64.abs().max().item()
        assert rel <= 1e-12, (name, rel)
        d = q32.double() - q64
        err = np.array([d.pow(2).mean().sqrt().item(), d.abs().max().item()])
        assert err[0] > 0
        do = o32.double() - q64
        rms = lambda t: t.pow(2).mean().sqrt().item()
        smooth, appear = trace[-1]
        if params != "default":
            assert rms(appear) >= 0.1 * rms(smooth), (name, rms(appear), rms(smooth))
        top2 = q64.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > MARGIN * err[1]
        assert torch.equal(q32.argmax(1)[sure], q64.argmax(1)[sure]) and 1 - sure.double().mean().item() <= MAX_EXCLUDED, name
        print(f"crf {name}: {tuple(shape)} window {ks} x {iters}: reference fp32 against fp64 rms {err[0]:.3e} max {err[1]:.3e}; the direct-sum fp32 "
              f"restatement rms {rms(do):.3e} max {do.abs().max().item():.3e}; smoothness rms {rms(smooth):.3e}, appearance rms {rms(appear):.3e}; "
              f"|Q - unary| rms {rms(q64 - unary.double()):.3e}; within the label margin {1 - sure.double().mean().item():.3%}")
        out[f"err_crf_{name}"] = err
        if stored:
            out[f"unary_{name}"], out[f"xyz_{name}"], out[f"mask_{name}"], out[f"q64_{name}"] = unary.numpy(), xyz.numpy(), mask.numpy(), q64.numpy()
        if params == "custom":
            for k, v in state.items():
                out[f"crfstate_custom_{k}"] = v.numpy()

    # ---- the public names -----------------------------------------------------------------------------------------------------
    sys.modules.pop("hubconf", None)
    import importlib.util

    spec = importlib.util.spec_from_file_location("reference_hubconf", os.path.join(reference, "hubconf.py"))
    hub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hub)
    sig = {n: _signature(getattr(hub, n)) for n in ("rangenet", "rangenet21", "rangenet53", "knn", "crf_rnn")}
    sig["KNN"] = _signature(ref.kNN.__init__)[1:]
    sig["CRFRNN"] = _signature(ref.CRFRNN.__init__)[1:]
    out["hub"] = np.array(json.dumps(sig))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
