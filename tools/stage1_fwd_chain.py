"""From a rocprofv3 kernel trace of bench.py (``--kernel-trace --output-format csv``): the forward launches of
ResNet stage 1 that rtdetr_conv1x1_block_out replaces, or the chained launches themselves
(profiles/conv_chain_fwd/stage1_fwd_*.txt).

The stem's max-pool launch opens every backbone forward; the convolution launches that follow it are, in order,
  separate launches:  a1 b1 short c1 | a2 b2 c2 | a3 b3 c3 | a(stage 2, block 1)
  chained launches:   a1 b1 out1     | b2 out2  | b3 out3
(a / b / c = branch2a / 2b / 2c, short = block 1's shortcut convolution, out_k = stage1_out_kernel).  Prints, per
position, the kernel, count, mean (min - max) us, the algorithmic HBM MB of the launch (every operand once, at
--pixels pixels) and the TB/s that makes.

    python tools/stage1_fwd_chain.py <run_kernel_trace.csv> [--pixels 471040]
"""
import argparse
import csv
import re
from collections import defaultdict

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--pixels", type=int, default=8 * 184 * 320)
a = ap.parse_args()
P = a.pixels

rows = []
with open(a.trace) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
CONV = ("conv_fwd_kernel", "conv3x3_halo_kernel", "conv_8ph_kernel", "stage1_out_kernel")
# role -> channels crossing HBM per pixel (bf16): inputs + outputs
SEP = [("a1", None), ("b1", None), ("short 64->256", 64 + 256), ("c1 64->256 +resid", 64 + 256 + 256),
       ("a2 256->64", 256 + 64), ("b2", None), ("c2 64->256 +resid", 64 + 256 + 256), ("a3 256->64", 256 + 64),
       ("b3", None), ("c3 64->256 +resid", 64 + 256 + 256), ("a(stage 2) 256->128", 256 + 128)]
CHAIN = [("a1", None), ("b1", None), ("out1: short + c1 + a2", 64 + 64 + 256 + 64), ("b2", None),
         ("out2: c2 + a3", 64 + 256 + 256 + 64), ("b3", None), ("out3: c3 + a(stage 2)", 64 + 256 + 256 + 128)]


def short(n):
    n = n.split("(")[0].replace("void ", "").replace("moe::", "")
    return re.sub(r"\s+", " ", n)


stat = defaultdict(list)
mode = None
for i, (_, _, n) in enumerate(rows):
    if "maxpool3x3s2" not in n:
        continue
    seq = []
    for s, e, k in rows[i + 1:i + 200]:
        if "maxpool3x3s2" in k:
            break
        if any(c in k for c in CONV):
            seq.append(((e - s) / 1e3, short(k)))
        if len(seq) == len(SEP):
            break
    chained = any("stage1_out_kernel" in k for _, k in seq)
    roles = CHAIN if chained else SEP
    if len(seq) < len(roles):
        continue
    mode = "chained" if chained else "separate"
    for (role, ch), (us, k) in zip(roles, seq):
        if ch is not None:
            stat[(role, k, ch)].append(us)

print(f"stage-1 forward, {mode} launches, P = {P} pixels")
print("| launch | kernel | n | us (min - max) | MB | TB/s |")
print("|---|---|---|---|---|---|")
total = 0.0
for (role, k, ch), v in stat.items():
    mean = sum(v) / len(v)
    mb = 2.0 * P * ch / 1e6
    total += mean
    print(f"| {role} | `{k}` | {len(v)} | {mean:.1f} ({min(v):.1f} - {max(v):.1f}) | {mb:.1f} | {mb / mean:.2f} |")
print(f"sum of the means: {total:.1f} us per forward")
