"""Writes tests/golden/forward_listing.json: which kernel every layer of a forward dispatches to, as r2dm_forward_listing tells it
from the sizing walk (host only: no GPU, no weights).  tests/test_forward_listing_cpu.py regenerates every case and compares.

    python tests/golden/make_forward_listing.py          # rewrite the fixture -- only when a pull request changes dispatch ON PURPOSE
    python tests/golden/make_forward_listing.py --check  # compare, print the cases that differ

The fixture holds the full listing of the default geometry at batch 8 in the three precision modes, and for every other case the
SHA-256 of its listing, its workspace bytes, its launch count and how many convolutions run on the bf16x3 kernel.  The library reads
some switches once per process, so every case with a switch runs in a child process of its own (all of them side by side).
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "forward_listing.json")
MODES = (2, 1, 3)  # r2dm_set_conv_pieces: fp32 (default), fp16, fp32-bf16x3
DEFAULT = (64, 1024)
# (resolution, max_batch, batch)
GEOMETRIES = [(DEFAULT, 8, 1), (DEFAULT, 8, 2), (DEFAULT, 8, 4), (DEFAULT, 8, 8), (DEFAULT, 1, 1), (DEFAULT, 2, 2), (DEFAULT, 4, 4), (DEFAULT, 32, 32),
              ((128, 2048), 2, 2), ((32, 256), 3, 3)]
# every documented switch that alters the walk, at the default geometry and batch 8
SWITCHES = [("R2DM_DOWN_GEMM", "0"), ("R2DM_DOWN_GEMM", "9"), ("R2DM_GN_FOLD", "0"), ("R2DM_FP16_STORAGE", "0"), ("R2DM_FP16_STORAGE", "1"),
            ("R2DM_F2_NARROW", "0"), ("R2DM_F2_NARROW_SPLIT", "1"), ("R2DM_FIR_STATS", "0"), ("R2DM_CONV_ALGO", "f32")]
FULL = {(DEFAULT, 8, 8)}  # stored line by line


def case_name(res, max_batch, batch, mode, switch=None):
    return f"{res[0]}x{res[1]} max_batch={max_batch} B={batch} mode={mode}" + (f" {switch[0]}={switch[1]}" if switch else "")


def listings(res, max_batch, batch):
    """{mode: (listing, workspace bytes)} of one engine, in this process."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from r2dm_amd import _lib, synthetic
    from r2dm_amd.unet import _Engine

    eng = _Engine(synthetic.geometry_from_cfg(synthetic.default_cfg_dict(resolution=res)), max_batch)
    out = {}
    for mode in MODES:
        _lib.check(_lib.lib().r2dm_set_conv_pieces(eng.h, mode))
        out[mode] = (eng.listing(batch), int(_lib.lib().r2dm_workspace_bytes(eng.h, batch)))
    return out


def record(listing, ws, full):
    lines = listing.splitlines()
    r = {"sha256": hashlib.sha256(listing.encode()).hexdigest(), "workspace_bytes": ws, "launches": len(lines),
         "bf16x3": sum(" algo=BF16X3 " in ln for ln in lines)}
    if full:
        r["listing"] = lines
    return r


def cases_of(res, max_batch, batch, switch=None):
    return {case_name(res, max_batch, batch, mode, switch): record(s, ws, (res, max_batch, batch) in FULL and not switch)
            for mode, (s, ws) in listings(res, max_batch, batch).items()}


def generate():
    """Every case of the fixture: the switch cases in child processes started first, the rest here meanwhile."""
    children = []
    for sw in SWITCHES:
        env = dict(os.environ, **{sw[0]: sw[1]})
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--switch", sw[0], sw[1]], env=env, stdout=subprocess.PIPE, text=True))
    cases = {}
    for res, mb, b in GEOMETRIES:
        cases.update(cases_of(res, mb, b))
    for sw, p in zip(SWITCHES, children):
        out, _ = p.communicate(timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"the child process of {sw[0]}={sw[1]} ended with status {p.returncode}")
        cases.update(json.loads(out))
    return {"format": 1, "cases": cases}


def main(argv):
    if argv[:1] == ["--switch"]:  # (child: the switch is in the environment already)
        json.dump(cases_of(DEFAULT, 8, 8, (argv[1], argv[2])), sys.stdout)
        return 0
    got = generate()
    if argv[:1] == ["--check"]:
        want = json.load(open(FIXTURE))
        bad = sorted(k for k in set(got["cases"]) | set(want["cases"]) if got["cases"].get(k) != want["cases"].get(k))
        print("\n".join(bad) if bad else f"{len(got['cases'])} cases agree")
        return 1 if bad else 0
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}: {len(got['cases'])} cases, {os.path.getsize(FIXTURE)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
