"""Tune the tracker without a model: run a grid of track.TrackArgs over
detection files and score every configuration against MOTChallenge ground truth
(src/rtdetr_moe/tune.py).

--det holds <sequence>/det/det.txt or <sequence>.txt per sequence (frame,-1,x,y,
w,h,score,class,-1,-1: what scripts/predict_detector.py --save-det writes and
what MOTChallenge ships as public detections); --gt holds <sequence>/gt/gt.txt
or <sequence>.txt.  --grid is a JSON object of lists over the sweepable fields,
e.g. '{"match_iou":[0.2,0.3,0.5],"max_age":[15,30,60]}' or, to compare the two
associations, '{"assoc":["greedy","lsap"]}'; --tracker a JSON object of the
fields every configuration shares ("assoc" among them).  On a GPU (--device 0, the default
when there is one) all configurations are tracked in one HIP launch per chunk of
frames and scored by the evaluators' kernels; --device cpu runs the references
and gives the same numbers.  Prints one line per configuration, best first, then
the best as a --tracker JSON to paste, and writes tracker_sweep.json into --out;
--write-best also writes the best configuration's mot/<sequence>.txt there.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(PKG_ROOT)) if str(PKG_ROOT) not in sys.path else None

from scripts.predict_detector import int_list  # noqa: E402


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Sweep tracker arguments over detection files.")
    ap.add_argument("--det", type=str, required=True, help="detections: <key>/det/det.txt or <key>.txt per sequence")
    ap.add_argument("--gt", type=str, required=True, help="ground truth: <key>/gt/gt.txt or <key>.txt per sequence")
    ap.add_argument("--grid", type=str, required=True, help="JSON: {field: [values]} over the sweepable fields")
    ap.add_argument("--tracker", type=str, default=None, help="JSON of the track.TrackArgs fields all share")
    ap.add_argument("--gt-classes", type=str, default=None, help="the classes scored, e.g. 1 (default: all)")
    ap.add_argument("--gt-ignore-classes", type=str, default="", help="the ignore-region classes, e.g. 2,7,8,12")
    ap.add_argument("--eval-iou", type=float, default=0.5, help="the IoU a match needs")
    ap.add_argument("--hota", action="store_true", help="also score HOTA, and rank by it unless --metric says otherwise")
    ap.add_argument("--metric", type=str, default=None, choices=("HOTA", "MOTA", "IDF1"),
                    help="the COMBINED metric the configurations are ranked by (default: HOTA with --hota, else MOTA)")
    ap.add_argument("--shifts", type=str, default=None,
                    help="camera_motion.json of a run tracked with --cmc: the frames' camera shifts as the tracker's "
                         "input")
    ap.add_argument("--device", type=str, default=None, help="0, 1, ... or cpu (default: GPU 0 if there is one)")
    ap.add_argument("--out", type=str, default=None, help="the directory tracker_sweep.json is written to")
    ap.add_argument("--write-best", action="store_true",
                    help="--out: also write the best configuration's tracks as mot/<sequence>.txt")
    a = ap.parse_args(argv)
    if a.write_best and a.out is None:
        ap.error("--write-best needs --out")
    return a


def load_shifts(path) -> dict:
    """camera_motion.json ({sequence: [[frame, dx, dy, status], ...]}) -> {file key: fp32 [n, 2]}, frame f at f - 1."""
    import numpy as np

    out = {}
    for key, rows in json.loads(Path(path).read_text()).items():
        table = np.zeros((max([0, *(int(r[0]) for r in rows)]), 2), np.float32)
        for f, dx, dy, *_ in rows:
            table[int(f) - 1] = (dx, dy)
        out[key.replace("/", "_")] = table
    return out


def main(argv=None) -> dict:
    a = parse_args(argv)
    import torch

    from src.rtdetr_moe import engine, tune
    from src.rtdetr_moe.track import TrackArgs

    device = a.device if a.device is not None else ("0" if torch.cuda.is_available() else "cpu")
    base = json.loads(a.tracker) if a.tracker else None
    shifts = load_shifts(a.shifts) if a.shifts else None
    res = engine.tune_tracker(a.det, a.gt, json.loads(a.grid), device=device,
                              gt_classes=int_list(a.gt_classes) if a.gt_classes else None,
                              gt_ignore_classes=int_list(a.gt_ignore_classes), out=a.out, base=base,
                              eval_iou=a.eval_iou, hota=a.hota, metric=a.metric, shifts=shifts)
    varied = sorted(json.loads(a.grid))
    for place, g in enumerate(res["ranking"], 1):
        m = res["metrics"][g]["COMBINED"]
        hota = f" HOTA {m['HOTA']['HOTA']:.4f}" if "HOTA" in m else ""
        print(f"{place:4d}. config {g}:{hota} MOTA {m['MOTA']:.4f} IDF1 {m['IDF1']:.4f} IDSW {m['IDSW']} "
              f"FP {m['FP']} FN {m['FN']} | " + " ".join(f"{k}={res['configs'][g][k]}" for k in varied))
    best = res["configs"][res["best"]]
    print(f"best by {res['metric']}: --tracker '" +
          json.dumps({k: best[k] for k in (*tune.SWEEPABLE, *tune.SWEEPABLE_MODES, "max_tracks")}) + "'")
    if a.out:
        print(f"Saved the sweep -> {Path(a.out) / 'tracker_sweep.json'}")
    if a.write_best:
        keys = res["keys"]
        dets = tune.load_det(a.det, keys)
        cfg = TrackArgs.parse(best)
        dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", int(device))
        tracks = tune.sweep_tracks(dets, [cfg], cfg.max_tracks, dev, shifts)[0]  # one configuration: cheap to rerun
        (Path(a.out) / "mot").mkdir(parents=True, exist_ok=True)
        for key in keys:
            (Path(a.out) / "mot" / (key + ".txt")).write_text(tune.mot_text(tracks[key], dets[key]))
        print(f"Saved the best configuration's tracks -> {Path(a.out) / 'mot'}")
    return res


if __name__ == "__main__":
    main()
