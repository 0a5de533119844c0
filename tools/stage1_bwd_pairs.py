"""From a rocprofv3 kernel trace of bench.py (``--kernel-trace --output-format csv``): the ResNet stage-1
1x1 backward launches (profiles/conv1x1_bwd/stage1_1x1_bwd_*.txt).
Two-launch path: every conv_wgrad_kernel<1, 2, 128, 64> / <1, 2, 64, 128> whose
predecessor on the timeline is a 1x1 conv_fwd_kernel (its data gradient);
fused path: every conv1x1_bwd_kernel.  Prints count / mean / min / max (us).

    python tools/stage1_bwd_pairs.py <run_kernel_trace.csv>
"""
import csv
import sys
from collections import defaultdict

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
pairs = defaultdict(list)
fused = defaultdict(list)
for i, (s, e, n) in enumerate(rows):
    if "conv1x1_bwd_kernel" in n:
        fused[n.split("(")[0]].append((e - s) / 1e3)
    if "conv_wgrad_kernel<1, 2, 128, 64>" in n or "conv_wgrad_kernel<1, 2, 64, 128>" in n:
        ps, pe, pn = rows[i - 1]
        if "conv_fwd_kernel<1," in pn:
            pairs[(pn.split("(")[0], n.split("(")[0])].append(((pe - ps) / 1e3, (e - s) / 1e3, (e - ps) / 1e3))


def st(v):
    return f"n={len(v)} mean={sum(v) / len(v):.1f} min={min(v):.1f} max={max(v):.1f}"


for k, v in pairs.items():
    print("PAIR", k[0], "+", k[1])
    print("   dgrad us:", st([a for a, _, _ in v]))
    print("   wgrad us:", st([b for _, b, _ in v]))
    print("   sum   us:", st([a + b for a, b, _ in v]), "| span us:", st([c for _, _, c in v]))
for k, v in fused.items():
    print("FUSED", k)
    print("   us:", st(v))
