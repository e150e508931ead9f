#!/usr/bin/env python3
"""Memory-side bytes of the six down-path launches of a step from four rocprofv3 counter passes of bench.py (config 1: 64x1024, batch 8):
--pmc FETCH_SIZE and --pmc WRITE_SIZE (one counter per pass, no tracing, --kernel-include-regex 'down_planes|proj_', --output-format csv), once with
R2DM_DOWN_GEMM=9 (all nine planes) and once with =1 (every distinct plane once).
Usage: scripts/down_gemm_pmc.py FETCH9.csv WRITE9.csv FETCH1.csv WRITE1.csv [batch]

Both counters are in KiB.  On gfx950 FETCH_SIZE tallies the 128-byte requests of a wide coalesced read at 64 bytes, so the table prints it as read and doubled
beside the bytes each launch has to move (x read once + the planes written; the planes + the packed weights read + y written); which of the two readings fits
is judged on the pre-pass's read of x, whose size is known exactly."""
import collections
import csv
import sys

B = int(sys.argv[5]) if len(sys.argv) > 5 else 8
H, W = 64, 1024
LEVELS = [("d2", 64, 128, H, W), ("d3", 128, 256, H // 2, W // 2), ("d4", 256, 512, H // 4, W // 4)]  # (name, Cin, Cout, input H, W)


def pairs(path):
    """Per level, the mean counter value (MB) of the pre-pass and of the projection launch that follows it in dispatch order."""
    per = collections.OrderedDict()  # dispatch -> [kernel name, summed value]
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"])):
        e = per.setdefault(int(r["Dispatch_Id"]), [r["Kernel_Name"], 0.0])
        e[1] += float(r["Counter_Value"])
    rows = list(per.values())
    out = []
    for i, (n, v) in enumerate(rows):
        if "down_planes" not in n:
            continue
        if i + 1 == len(rows):
            break
        if "proj_" not in rows[i + 1][0]:
            raise SystemExit(f"{path}: dispatch {i}: {n[:40]} is not followed by its GEMM but by {rows[i + 1][0][:40]}")
        out.append((v, rows[i + 1][1]))
    out = out[:len(out) - len(out) % 3]  # whole steps, counted from the first launch (level 1 of the first forward)
    mean = lambda xs: sum(xs) / len(xs) * 1024 / 1e6
    return [(mean([p for p, _ in out[k::3]]), mean([g for _, g in out[k::3]])) for k in range(3)], len(out) // 3


(f9, n9), (w9, _), (f1, n1), (w1, _) = (pairs(p) for p in sys.argv[1:5])
print(f"# rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, bench.py config 1 (64x1024, batch {B}); forwards averaged: nine {n9}, phase {n1}; MB (1e6 bytes) per launch")
print("%-4s %-10s %-6s | %10s %10s %10s | %10s %10s | %10s %10s %10s | %10s %10s" % ("", "Cin->Cout", "", "pre FETCH", "x 2", "must rd", "pre WRITE", "must wr",
                                                                        "gemm FETCH", "x 2", "must rd", "gemm WRITE", "must wr"))
tot = {}
for i, (name, ci, co, h, w) in enumerate(LEVELS):
    x = 4.0 * B * ci * h * w / 1e6
    y = 4.0 * B * co * (h // 2) * (w // 2) / 1e6
    wt = 4.0 * 9 * ci * co / 1e6  # (the packed matrix: two fp16 halves per weight)
    for tag, f, wr, planes in (("nine", f9[i], w9[i], 2.25 * x), ("phase", f1[i], w1[i], 4.0 * B * 2 * ci * (h + 3) * (w // 2 + 4) / 1e6)):
        print("%-4s %-10s %-6s | %10.1f %10.1f %10.1f | %10.1f %10.1f | %10.1f %10.1f %10.1f | %10.1f %10.1f" % (name, f"{ci}->{co}", tag, f[0], 2 * f[0], x, wr[0], planes,
                                                                                            f[1], 2 * f[1], planes + wt, wr[1], y))
        t = tot.setdefault(tag, [0.0] * 4)
        for k, v in enumerate((f[0], wr[0], f[1], wr[1])):
            t[k] += v
for tag, t in tot.items():
    print(f"per forward, {tag:5s}: pre-passes FETCH {t[0]:.1f} (x 2: {2 * t[0]:.1f}) WRITE {t[1]:.1f}; GEMMs FETCH {t[2]:.1f} (x 2: {2 * t[2]:.1f}) WRITE {t[3]:.1f}")
r = lambda k: tot["phase"][k] / tot["nine"][k]
print(f"phase / nine: pre-pass FETCH {r(0):.2f} WRITE {r(1):.2f}; GEMM FETCH {r(2):.2f} WRITE {r(3):.2f}")
