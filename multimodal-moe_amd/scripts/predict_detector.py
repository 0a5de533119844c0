"""Detect on image files with a trained RT-DETR-MoE checkpoint (or a bare
architecture spec) and write predictions.json (COCO results format) -- and,
with --save-img, overlays -- under RUNS_DIR/rtdetr/<run-name>_predict.

Same flag style as scripts/eval_detector.py.  --source is a directory, a glob,
one image file or a dataset yaml; frames may have any size.  --tiles 2x2 adds
sliced inference: every frame is also detected on a grid of crops and the passes
are merged (engine.predict).  --track links the detections of consecutive frames
(a sequence: the images of one directory) by track id and also writes tracks.json
and mot/<sequence>.txt; scripts/track_detector.py is the same thing.  --save-det
(without --track) also writes det/<sequence>.txt, the detections as MOTChallenge
text: the input of scripts/tune_tracker.py.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(PKG_ROOT)) if str(PKG_ROOT) not in sys.path else None

from src.paths import RUNS_DIR  # noqa: E402


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Predict with a detector run.")
    ap.add_argument("--weights", type=str, required=True, help="checkpoint (best.pt / last.pt) or architecture spec")
    ap.add_argument("--source", type=str, required=True, help="directory, glob, image file or dataset yaml")
    ap.add_argument("--img-h", type=int, default=704)
    ap.add_argument("--img-w", type=int, default=1248)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", type=str, default="0")
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--context", type=str, default=None,
                    help="one solar context label for every frame (default: contexts.json / COCO jsons by the source)")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--save-img", action="store_true", help="also write the frames with their boxes drawn")
    ap.add_argument("--run-name", type=str, default="rtdetr")
    ap.add_argument("--tiles", type=str, default=None,
                    help="ROWSxCOLS, e.g. 2x2: also detect on an overlapping grid of crops of every frame and merge")
    ap.add_argument("--tile-overlap", type=float, default=0.2, help="overlap of neighbouring tiles, in [0, 0.5]")
    ap.add_argument("--merge-iou", type=float, default=0.5, help="the merge's suppression threshold")
    ap.add_argument("--merge-metric", type=str, default="ios", choices=("ios", "iou"),
                    help="ios: intersection over the smaller box; iou: over the union")
    ap.add_argument("--class-agnostic", action="store_true", help="merge across labels")
    ap.add_argument("--merge", type=str, default="nms", choices=("nms", "fuse"),
                    help="nms: keep the best copy of every object; fuse (with --tiles or --flip): average it with its "
                         "other copies")
    ap.add_argument("--flip", action="store_true",
                    help="flip test-time augmentation: every pass also runs mirrored, un-mirrored boxes join the merge")
    ap.add_argument("--fuse-iou", type=float, default=0.55,
                    help="--merge fuse: how well a copy must agree with the kept box to be averaged in")
    ap.add_argument("--track", action="store_true",
                    help="link the detections across the frames of a sequence (one directory): tracks.json, mot/*.txt")
    ap.add_argument("--tracker", type=str, default=None,
                    help="--track: JSON of track.TrackArgs fields, e.g. '{\"max_age\": 15}' (default: ByteTrack's)")
    ap.add_argument("--assoc", type=str, default=None, choices=("greedy", "lsap"),
                    help="--track: the association of tracks and detections: greedy by IoU (the default), or lsap, the "
                         "one-to-one matching with the largest total IoU, solved in the tracker's kernel")
    ap.add_argument("--cmc", action="store_true",
                    help="--track: camera-motion compensation, the tracks move by each frame's global shift "
                         "(camera_motion.json)")
    ap.add_argument("--cmc-radius", type=int, default=None,
                    help="--cmc: search radius in pixels of the model's input, a multiple of 4 in [4, 64] (default 48)")
    ap.add_argument("--cmc-gate", type=float, default=None,
                    help="--cmc: a non-zero shift must beat no shift by this share (default 0.1)")
    ap.add_argument("--cmc-rows", type=str, default=None,
                    help="--cmc: T,B the fractions of the height the estimator looks at, e.g. 0,0.8 to leave the "
                         "bonnet out (default 0,1)")
    ap.add_argument("--gt", type=str, default=None,
                    help="--track: a directory of MOTChallenge ground truth (<key>/gt/gt.txt or <key>.txt per "
                         "sequence); the tracks are scored against it (mot_metrics.json)")
    ap.add_argument("--gt-classes", type=str, default=None,
                    help="--gt: the classes scored, e.g. 1 (default: all)")
    ap.add_argument("--gt-ignore-classes", type=str, default="",
                    help="--gt: the classes that are ignore regions, e.g. 2,7,8,12")
    ap.add_argument("--eval-iou", type=float, default=0.5, help="--gt: the IoU a match needs")
    ap.add_argument("--hota", action="store_true",
                    help="--gt: also score HOTA (DetA, AssA, LocA over 19 IoU thresholds)")
    ap.add_argument("--save-det", action="store_true",
                    help="also write det/<sequence>.txt, the detections as MOTChallenge text for "
                         "scripts/tune_tracker.py (not with --track)")
    a = ap.parse_args(argv)
    if a.save_det and a.track:
        ap.error("--save-det writes an untracked run's detections: not with --track")
    if a.gt is not None and not a.track:
        ap.error("--gt needs --track")
    if a.hota and a.gt is None:
        ap.error("--hota needs --gt")
    if a.tracker is not None and not a.track:
        ap.error("--tracker needs --track")
    if a.assoc is not None and not a.track:
        ap.error("--assoc needs --track")
    given = a.cmc_radius is not None or a.cmc_gate is not None or a.cmc_rows is not None
    if (a.cmc or given) and not a.track:
        ap.error("--cmc needs --track")
    if given and not a.cmc:
        ap.error("--cmc-radius, --cmc-gate and --cmc-rows need --cmc")
    return a


def tracker_args(a):
    """engine.predict's ``track`` from the command line: --tracker's JSON, --assoc and the --cmc options over it."""
    if not a.track:
        return None
    t = json.loads(a.tracker) if a.tracker else {}
    if a.assoc is not None:
        t["assoc"] = a.assoc
    if a.cmc:
        t["cmc"] = True
        if a.cmc_radius is not None:
            t["cmc_radius"] = a.cmc_radius
        if a.cmc_gate is not None:
            t["cmc_gate"] = a.cmc_gate
        if a.cmc_rows is not None:
            t["cmc_rows"] = tuple(float(v) for v in a.cmc_rows.split(","))
    return t or True


def int_list(text) -> list:
    return [int(v) for v in text.split(",") if v.strip()]


def gt_args(a) -> dict:
    """engine.predict's ground-truth arguments from the command line; nothing without --gt."""
    if a.gt is None:
        return {}
    return dict(gt=a.gt, gt_classes=int_list(a.gt_classes) if a.gt_classes else None,
                gt_ignore_classes=int_list(a.gt_ignore_classes), eval_iou=a.eval_iou,
                **({"hota": True} if a.hota else {}))


def print_mot(mot) -> None:
    """One line per sequence and the combined row."""
    cols = ("MOTA", "MOTP", "IDF1", "IDP", "IDR", "Recall", "Precision")
    ints = ("TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "GT", "removed", "frames")
    for key, m in mot.items():
        hota = "".join(f" {c} {m['HOTA'][c]:.4f}" for c in ("HOTA", "DetA", "AssA", "LocA")) if "HOTA" in m else ""
        print(f"{key}: " + " ".join(f"{c} {m[c]:.4f}" for c in cols) + " " + " ".join(f"{c} {m[c]}" for c in ints)
              + hota)


def main(argv=None) -> None:
    a = parse_args(argv)
    from src.rtdetr_moe import engine

    res = engine.predict(a.weights, a.source, imgsz=(a.img_h, a.img_w), batch=a.batch, device=a.device, conf=a.conf,
                         max_det=a.max_det, contexts=a.context, workers=a.workers, project=str(RUNS_DIR / "rtdetr"),
                         name=f"{a.run_name}_predict", save_json=True, save_img=a.save_img, tiles=a.tiles,
                         tile_overlap=a.tile_overlap, merge_iou=a.merge_iou, merge_metric=a.merge_metric,
                         class_agnostic=a.class_agnostic, merge=a.merge, fuse_iou=a.fuse_iou,
                         track=tracker_args(a), **gt_args(a), **({"save_det": True} if a.save_det else {}),
                         **({"flip": True} if a.flip else {}))
    n_det = sum(len(p.scores) for p in res.predictions)
    print(f"{len(res.predictions)} images, {n_det} detections at conf >= {a.conf}")
    if a.track:
        ids = {(p.sequence, int(t)) for p in res.predictions for t in p.track_ids}
        print(f"{len(ids)} tracks in {len({p.sequence for p in res.predictions})} sequences")
        print(f"Saved tracks -> {res.save_dir / 'tracks.json'}, {res.save_dir / 'mot'}")
        if a.cmc:
            print(f"Saved camera shifts -> {res.save_dir / 'camera_motion.json'}")
        if res.mot is not None:
            print_mot(res.mot)
            print(f"Saved tracking metrics -> {res.save_dir / 'mot_metrics.json'}")
    print("speed ms/img: " + ", ".join(f"{k} {v:.3f}" for k, v in res.speed.items()))
    print(f"Saved predictions -> {res.save_dir / 'predictions.json'}")
    if a.save_det:
        print(f"Saved detections -> {res.save_dir / 'det'}")


if __name__ == "__main__":
    main()
