"""Score tracker output against MOTChallenge ground truth without a model: the
CLEAR-MOT and identity metrics of src/rtdetr_moe/moteval.py for every
<sequence>.txt of --results (the mot/ directory scripts/track_detector.py
writes: frame,id,x,y,w,h,score,-1,-1,-1) against --gt (<sequence>/gt/gt.txt or
<sequence>.txt per sequence).  Prints one line per sequence and the combined
row, and writes the same as JSON with --out.  On a GPU (--device 0, the default
when there is one) every chunk of 1024 frames is one HIP launch; --device cpu
runs the reference and gives the same numbers.  --hota adds HOTA, DetA, AssA
and LocA (src/rtdetr_moe/hota.py; on a GPU one workgroup per frame).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(PKG_ROOT)) if str(PKG_ROOT) not in sys.path else None

from scripts.predict_detector import int_list, print_mot  # noqa: E402


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Score MOTChallenge result files against ground truth.")
    ap.add_argument("--gt", type=str, required=True, help="ground truth: <key>/gt/gt.txt or <key>.txt per sequence")
    ap.add_argument("--results", type=str, required=True, help="a directory of <key>.txt result files")
    ap.add_argument("--gt-classes", type=str, default=None, help="the classes scored, e.g. 1 (default: all)")
    ap.add_argument("--gt-ignore-classes", type=str, default="", help="the ignore-region classes, e.g. 2,7,8,12")
    ap.add_argument("--eval-iou", type=float, default=0.5, help="the IoU a match needs")
    ap.add_argument("--device", type=str, default=None, help="0, 1, ... or cpu (default: GPU 0 if there is one)")
    ap.add_argument("--hota", action="store_true", help="also score HOTA (DetA, AssA, LocA over 19 IoU thresholds)")
    ap.add_argument("--out", type=str, default=None, help="also write the metrics to this JSON file")
    return ap.parse_args(argv)


def score(gt, results, gt_classes=None, gt_ignore_classes=(), eval_iou=0.5, device=None, hota=False) -> dict:
    """moteval.evaluate of every <key>.txt in ``results``, the keys in sorted order."""
    import torch

    from src.rtdetr_moe import moteval

    keys = sorted(p.stem for p in Path(results).glob("*.txt"))
    if not keys:
        raise FileNotFoundError(f"no <sequence>.txt files in {results}")
    if device is None:
        device = "0" if torch.cuda.is_available() else "cpu"
    dev = torch.device("cpu") if str(device) == "cpu" else torch.device("cuda", int(device))
    truth = moteval.load_gt(gt, keys, gt_classes, gt_ignore_classes)
    return moteval.evaluate(truth, results, thr=eval_iou, device=dev, hota=hota)


def main(argv=None) -> dict:
    a = parse_args(argv)
    mot = score(a.gt, a.results, int_list(a.gt_classes) if a.gt_classes else None, int_list(a.gt_ignore_classes),
                a.eval_iou, a.device, a.hota)
    print_mot(mot)
    if a.out:
        Path(a.out).write_text(json.dumps(mot))
        print(f"Saved tracking metrics -> {a.out}")
    return mot


if __name__ == "__main__":
    main()
