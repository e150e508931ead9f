#!/usr/bin/env python3
"""Down-path table from two rocprofv3 kernel traces of bench.py (config 1: 64x1024, batch 8), one with R2DM_DOWN_GEMM=0 and one with =1:
the three down-sampling convolutions + fir_down2 launches against the three down_planes + down-sampling GEMM launches, per step, with each
new kernel's share of its floor (bytes / 8 TB/s, FLOP / 833 TF/s).  Usage: scripts/down_gemm_trace.py OFF_kernel_trace.csv ON_kernel_trace.csv [batch]

Launch positions follow the engine's fixed order (r2dm_amd/csrc/forward.hip): conv_f16x2 launches 6, 13 and 20 of the 54 of a step are the down-sampling
convolutions with the switch off (51 launches with it on)."""
import collections
import csv
import sys

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
