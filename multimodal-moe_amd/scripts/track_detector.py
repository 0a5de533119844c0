"""Track pedestrians through image sequences with a trained RT-DETR-MoE
checkpoint (or a bare architecture spec): scripts/predict_detector.py with
--track on and --conf at the tracker's low band (0.1) unless given.  A sequence
is the images of one directory, in the source's order.  Writes predictions.json,
tracks.json (the COCO rows plus track_id and sequence) and mot/<sequence>.txt
(frame,id,x,y,w,h,score,-1,-1,-1) under RUNS_DIR/rtdetr/<run-name>_predict.
--cmc (with --cmc-radius, --cmc-gate, --cmc-rows T,B) turns on camera-motion
compensation and adds camera_motion.json.
--assoc lsap (or --tracker '{"assoc": "lsap"}') associates by the one-to-one
matching with the largest total IoU instead of greedily (track.py, step 4).
--gt DIR (with --gt-classes 1 --gt-ignore-classes 2,7,8,12 --eval-iou 0.5)
scores the tracks against MOTChallenge ground truth (DIR/<sequence>/gt/gt.txt or
DIR/<sequence>.txt): MOTA, MOTP, IDF1 and the counts per sequence and combined,
printed and written to mot_metrics.json; scripts/eval_tracks.py scores the
written mot/ directory again later, without a model.  --hota (with --gt) adds
HOTA, DetA, AssA and LocA to both.
--flip (as scripts/predict_detector.py takes it) tracks the merged result of
flip test-time augmentation: every pass also runs mirrored.
"""
from __future__ import annotations

import sys
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(PKG_ROOT)) if str(PKG_ROOT) not in sys.path else None

from scripts import predict_detector  # noqa: E402


def main(argv=None) -> None:
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--track" not in argv:
        argv.append("--track")
    if not any(a == "--conf" or a.startswith("--conf=") for a in argv):
        argv += ["--conf", "0.1"]
    predict_detector.main(argv)


if __name__ == "__main__":
    main()
