#!/usr/bin/env python3
"""Down-path table from two rocprofv3 kernel traces of bench.py (config 1: 64x1024, batch 8), one with R2DM_DOWN_GEMM=0 and one with =1:
the three down-sampling convolutions + fir_down2 launches against the three down_planes + down-sampling GEMM launches, per step, with each
new kernel's share of its floor (bytes / 8 TB/s, FLOP / 833 TF/s).  Usage: scripts/down_gemm_trace.py OFF_kernel_trace.csv ON_kernel_trace.csv [batch]
With --phase the two traces are R2DM_DOWN_GEMM=9 (all nine planes) and =1 (every distinct plane once): pre-pass and GEMM of each, the pre-pass's floor from the bytes
each layout must move.

Launch positions follow the engine's fixed order (r2dm_amd/csrc/forward.hip): conv_f16x2 launches 6, 13 and 20 of the 54 of a step are the down-sampling
convolutions with the switch off (51 launches with it on)."""
import collections
import csv
import sys

PHASE = "--phase" in sys.argv  # NINE_kernel_trace.csv PHASE_kernel_trace.csv [batch]: R2DM_DOWN_GEMM=9 against =1 (both run the pre-pass and the GEMM)
sys.argv = [a for a in sys.argv if a != "--phase"]
off_path, on_path = sys.argv[1], sys.argv[2]
B = int(sys.argv[3]) if len(sys.argv) > 3 else 8
H, W = 64, 1024
LEVELS = [("d2", 64, 128, H, W), ("d3", 128, 256, H // 2, W // 2), ("d4", 256, 512, H // 4, W // 4)]  # (name, Cin, Cout, input H, W)


def load(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]


def per_step(rows, pick, per):
    """Mean duration of launch position i (of `per` per step) of the kernels `pick` selects, whole steps counted from the end of the trace."""
    k = [d for n, d in rows if pick(n)]
    steps = len(k) // per
    k = k[len(k) - steps * per:]
    out = collections.defaultdict(list)
    for i, d in enumerate(k):
        out[i % per].append(d)
    return [sum(out[i]) / len(out[i]) for i in range(per)], steps


off, on = load(off_path), load(on_path)
is_f2 = lambda n: "conv_f16x2_kernel" in n and "pack" not in n


def pre_and_gemm(rows):
    """Per-step means of the three down_planes launches and of the projection launch that follows each in time order (the engine enqueues the pair back to back)."""
    # (the next projection launch, not the next row: the sampler's noise draw may start in between.  A pre-pass whose GEMM the trace no longer holds -- the
    # trace's last rows -- is dropped with it, so that both columns average the same launches; one with anything else in the next five rows is an error)
    pairs = []
    for i, (n, d) in enumerate(rows):
        if "down_planes" not in n:
            continue
        nxt = [r for r in rows[i + 1:i + 6] if "proj_" in r[0] or "down_planes" in r[0]]
        if not nxt and i + 6 > len(rows):
            break
        if not nxt or "proj_" not in nxt[0][0]:
            raise SystemExit(f"row {i}: {n} is not followed by its GEMM: {[r[0][:40] for r in rows[i + 1:i + 6]]}")
        pairs.append(((n, d), nxt[0]))
    pairs = pairs[:len(pairs) - len(pairs) % 3]  # whole steps, counted from the first launch (level 1 of the first forward)
    pre, _ = per_step([p for p, _ in pairs], lambda n: True, 3)
    gemm, _ = per_step([g for _, g in pairs], lambda n: True, 3)
    return pre, gemm


if PHASE:
    (p9, g9), (p1, g1) = pre_and_gemm(off), pre_and_gemm(on)
    c9, s9 = per_step(off, is_f2, 51)
    c1, s1 = per_step(on, is_f2, 51)
    print(f"# rocprofv3 --kernel-trace, bench.py config 1 (64x1024, batch {B}); steps averaged: nine {s9}, phase {s1}; us per launch")
    print("%-4s %-10s | %9s %6s %9s %6s %9s | %9s %6s %9s %6s %9s" % ("", "Cin->Cout", "planes 9", "HBM", "GEMM", "MFMA", "sum", "phase pl.", "HBM", "GEMM", "MFMA", "sum"))
    t9 = t1 = 0.0
    for i, (name, ci, co, h, w) in enumerate(LEVELS):
        x = 4.0 * B * ci * h * w
        b9 = x * (1 + 2.25)
        b1 = x + 4.0 * B * ci * (2 * (h + 3) * (w // 2) + (h + 3))  # x read once + two phases of 2 Ho + 3 rows (+ the wrapped column of phase E)
        fl = 2.0 * B * co * 9 * ci * (h // 2) * (w // 2) / 833.3e12 * 1e6
        print("%-4s %-10s | %9.1f %6.2f %9.1f %6.2f %9.1f | %9.1f %6.2f %9.1f %6.2f %9.1f" % (name, f"{ci}->{co}", p9[i], b9 / 8e12 * 1e6 / p9[i], g9[i], fl / g9[i], p9[i] + g9[i],
                                                                                   p1[i], b1 / 8e12 * 1e6 / p1[i], g1[i], fl / g1[i], p1[i] + g1[i]))
        t9 += p9[i] + g9[i]
        t1 += p1[i] + g1[i]
    print(f"per step: nine planes {t9:.1f} us -> phase planes {t1:.1f} us (saves {t9 - t1:.1f} us); pre-passes {sum(p9):.1f} -> {sum(p1):.1f}, GEMMs {sum(g9):.1f} -> {sum(g1):.1f}")
    print(f"the other 51 conv_f16x2 launches: nine {sum(c9):.1f} us, phase {sum(c1):.1f} us per step")
    sys.exit(0)
conv_off, s0 = per_step(off, is_f2, 54)
fir_off, _ = per_step(off, lambda n: "fir_down2" in n, 3)
conv_on, s1 = per_step(on, is_f2, 51)
pre_on, _ = per_step(on, lambda n: "down_planes" in n, 3)
# the GEMMs: the launch that follows each down_planes launch in time order (the engine enqueues the pair back to back)
after = [on[i + 1] for i in range(len(on) - 1) if "down_planes" in on[i][0]]
assert all("proj_" in n for n, _ in after), sorted({n for n, _ in after})
gemm_on, _ = per_step(after, lambda n: True, 3)
print(f"# rocprofv3 --kernel-trace, bench.py config 1 (64x1024, batch {B}); steps averaged: off {s0}, on {s1}; us per launch")
print("%-4s %-10s | %9s %9s %9s | %9s %6s %9s %6s %9s" % ("", "Cin->Cout", "conv3x3", "fir_down2", "old sum", "planes", "HBM", "GEMM", "MFMA", "new sum"))
tot_old = tot_new = 0.0
for i, (name, ci, co, h, w) in enumerate(LEVELS):
    c, f, p, g = conv_off[(6, 13, 20)[i]], fir_off[i], pre_on[i], gemm_on[i]
    bytes_pre = 4.0 * B * ci * h * w * (1 + 2.25)
    flop = 2.0 * B * co * 9 * ci * (h // 2) * (w // 2)
    print("%-4s %-10s | %9.1f %9.1f %9.1f | %9.1f %6.2f %9.1f %6.2f %9.1f" % (name, f"{ci}->{co}", c, f, c + f, p, bytes_pre / 8e12 * 1e6 / p, g, flop / 833.3e12 * 1e6 / g, p + g))
    tot_old += c + f
    tot_new += p + g
print(f"per step: conv + FIR {tot_old:.1f} us -> planes + GEMM {tot_new:.1f} us (saves {tot_old - tot_new:.1f} us)")
rest_off = sum(conv_off) - sum(conv_off[i] for i in (6, 13, 20))
print(f"the other 51 conv_f16x2 launches: off {rest_off:.1f} us, on {sum(conv_on):.1f} us per step")
