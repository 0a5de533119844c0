"""predict() on synthetic ZOD-sized frames: the GPU resize against the host path.

Writes N (default 64) 3848 x 2168 JPEGs from a seed into a temporary directory,
then runs engine.predict on them with MOE_PREDICT_RESIZE=1 and =0 alternately
(default three times each, one process) and prints one JSON line per run with
``speed`` (ms per image) and a last line with the medians and spreads.
With --tiles RxC it runs, on the same files and alternately, prediction without
tiles, with tiles merged on the GPU (MOE_PREDICT_MERGE=1) and with tiles merged
on the host (MOE_PREDICT_MERGE=0), all with the GPU resize; --merge fuse makes
the tiled legs fuse the boxes (rtdetr_box_fuse / merge.fuse_reference).

  python tools/predict_bench.py [--model rtdetr-r50-moe8-top2] [--n 64] [--batch 16] [--rounds 3] [--workers 4]
  python tools/predict_bench.py --tiles 2x2 [--conf 0.25]
  python tools/predict_bench.py --flip [--tiles 2x2] [--merge fuse]
With --track it runs, on the same files (one sequence) and alternately,
prediction with the tracker on the GPU (MOE_PREDICT_TRACK=1), on the host
(MOE_PREDICT_TRACK=0) and without it, at conf 0; the random weights score every
query alike, so the tracker's bands are set at the quartiles of the distinct
scores of an untimed first run.

  python tools/predict_bench.py --track
With --track --cmc a fourth leg joins them: the tracker on the GPU with
camera-motion compensation (TrackArgs.cmc; the frames are unrelated to each
other, so the estimator runs its whole search and its gate refuses the result).

  python tools/predict_bench.py --track --cmc
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "multimodal-moe_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_frames(d: Path, n: int, seed: int = 0, hw=(2168, 3848)):
    from PIL import Image

    rng = np.random.default_rng(seed)
    h, w = hw
    for i in range(n):
        base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        im = Image.fromarray(base).resize((w, h), Image.BILINEAR)  # smooth content: JPEG sizes like a camera frame's
        im.save(d / f"{i:06d}.jpg", quality=90)


def tiles_leg(a, d: Path, engine):
    """Untiled, tiled with the merge kernel and tiled with the host merge, alternated per round."""
    legs = (("untiled", None, "1"), ("tiles_gpu_merge", a.tiles, "1"), ("tiles_host_merge", a.tiles, "0"))
    os.environ["MOE_PREDICT_RESIZE"] = "1"
    runs = {name: [] for name, _, _ in legs}
    for r in range(a.rounds):
        for name, tiles, merge in legs:
            os.environ["MOE_PREDICT_MERGE"] = merge
            torch.manual_seed(0)
            t0 = time.perf_counter()
            res = engine.predict(a.model, d, batch=a.batch, device=a.device, conf=a.conf, workers=a.workers,
                                 tiles=tiles, merge=a.merge if tiles else "nms")
            line = {"round": r, "leg": name, "images": len(res.predictions),
                    "detections": sum(len(p.scores) for p in res.predictions),
                    "wall_s": round(time.perf_counter() - t0, 2), **{k: round(v, 3) for k, v in res.speed.items()}}
            print(json.dumps(line), flush=True)
            runs[name].append(res.speed)
    os.environ.pop("MOE_PREDICT_MERGE", None)
    out = {"model": a.model, "batch": a.batch, "workers": a.workers, "tiles": a.tiles, "conf": a.conf,
           "merge": a.merge}
    for name, _, _ in legs:
        for k in ("preprocess", "inference", "postprocess"):
            v = [s[k] for s in runs[name]]
            out[f"{name}/{k}"] = [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
    print(json.dumps(out), flush=True)


def flip_leg(a, d: Path, engine):
    """Prediction without and with flip test-time augmentation (with --tiles: both tiled), alternated per round."""
    legs = (("flip_off", False), ("flip_on", True))
    os.environ["MOE_PREDICT_RESIZE"] = "1"
    runs = {name: [] for name, _ in legs}
    for r in range(a.rounds):
        for name, flip in legs:
            torch.manual_seed(0)
            t0 = time.perf_counter()
            res = engine.predict(a.model, d, batch=a.batch, device=a.device, conf=a.conf, workers=a.workers,
                                 tiles=a.tiles, merge=a.merge if a.tiles or flip else "nms", flip=flip)
            line = {"round": r, "leg": name, "images": len(res.predictions),
                    "detections": sum(len(p.scores) for p in res.predictions),
                    "wall_s": round(time.perf_counter() - t0, 2), **{k: round(v, 3) for k, v in res.speed.items()}}
            print(json.dumps(line), flush=True)
            runs[name].append(res.speed)
    out = {"model": a.model, "batch": a.batch, "workers": a.workers, "tiles": a.tiles, "conf": a.conf,
           "merge": a.merge, "flip": True}
    for name, _ in legs:
        for k in ("preprocess", "inference", "postprocess"):
            v = [s[k] for s in runs[name]]
            out[f"{name}/{k}"] = [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
    print(json.dumps(out), flush=True)


def track_leg(a, d: Path, engine):
    """Tracking on the GPU, on the host and off, alternated per round."""
    os.environ["MOE_PREDICT_RESIZE"] = "1"
    torch.manual_seed(0)
    res = engine.predict(a.model, d, batch=a.batch, device=a.device, conf=0.0, workers=a.workers)
    u = torch.unique(torch.cat([p.scores for p in res.predictions]))
    lo, hi, new = (float(u[min(len(u) * q // 4, len(u) - 1)]) for q in (1, 2, 3))
    tracker = dict(track_low=lo, track_high=hi, new_thr=new)
    legs = (("track_gpu", tracker, "1"), ("track_host", tracker, "0"), ("track_off", None, "1"))
    if a.cmc:
        legs = (("track_cmc_gpu", dict(tracker, cmc=True), "1"),) + legs
    runs = {name: [] for name, _, _ in legs}
    for r in range(a.rounds):
        for name, trk, switch in legs:
            os.environ["MOE_PREDICT_TRACK"] = switch
            torch.manual_seed(0)
            t0 = time.perf_counter()
            res = engine.predict(a.model, d, batch=a.batch, device=a.device, conf=0.0, workers=a.workers, track=trk)
            line = {"round": r, "leg": name, "images": len(res.predictions),
                    "rows": sum(len(p.scores) for p in res.predictions),
                    "wall_s": round(time.perf_counter() - t0, 2), **{k: round(v, 3) for k, v in res.speed.items()}}
            if trk is not None:
                line["tracks"] = len({int(t) for p in res.predictions for t in p.track_ids})
            if trk is not None and trk.get("cmc"):
                line["cmc_status"] = [sum(p.camera_status == v for p in res.predictions) for v in (0, 1, 2)]
            print(json.dumps(line), flush=True)
            runs[name].append(res.speed)
    os.environ.pop("MOE_PREDICT_TRACK", None)
    out = {"model": a.model, "batch": a.batch, "workers": a.workers, "tracker": tracker}
    for name, _, _ in legs:
        for k in ("preprocess", "inference", "postprocess"):
            v = [s[k] for s in runs[name]]
            out[f"{name}/{k}"] = [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="rtdetr-r50-moe8-top2")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--device", default="0")
    ap.add_argument("--tiles", default=None, help="ROWSxCOLS: time tiled prediction against the untiled run")
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--merge", default="nms", choices=("nms", "fuse"),
                    help="with --tiles: the merge of the tiled legs (fuse: rtdetr_box_fuse / fuse_reference)")
    ap.add_argument("--track", action="store_true",
                    help="time prediction with the tracker on the GPU, on the host and off (conf 0, one sequence)")
    ap.add_argument("--cmc", action="store_true", help="with --track: add a leg with camera-motion compensation")
    ap.add_argument("--flip", action="store_true",
                    help="time prediction with and without flip test-time augmentation (with --tiles: both tiled)")
    a = ap.parse_args(argv)
    if a.cmc and not a.track:
        ap.error("--cmc needs --track")
    from src.rtdetr_moe import engine

    with tempfile.TemporaryDirectory(prefix="predict_bench_") as td:
        d = Path(td)
        t0 = time.perf_counter()
        write_frames(d, a.n)
        print(json.dumps({"frames": a.n, "write_s": round(time.perf_counter() - t0, 2)}), flush=True)
        from PIL import Image

        from src.rtdetr_moe.preprocess import host_resize

        dec, rsz = [], []
        for p in sorted(d.glob("*.jpg"))[:8]:  # what one loader worker spends per frame
            t0 = time.perf_counter()
            arr = np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8)
            t1 = time.perf_counter()
            host_resize(arr, (704, 1248), (704, 1248))
            dec.append(1e3 * (t1 - t0))
            rsz.append(1e3 * (time.perf_counter() - t1))
        print(json.dumps({"jpeg_decode_ms_per_frame_one_core": round(statistics.median(dec), 2),
                          "host_resize_ms_per_frame_one_core": round(statistics.median(rsz), 2)}), flush=True)
        if a.track:
            track_leg(a, d, engine)
            return
        if a.flip:
            flip_leg(a, d, engine)
            return
        if a.tiles:
            tiles_leg(a, d, engine)
            return
        runs = {"1": [], "0": []}
        for r in range(a.rounds):
            for switch in ("1", "0"):
                os.environ["MOE_PREDICT_RESIZE"] = switch
                torch.manual_seed(0)
                t0 = time.perf_counter()
                res = engine.predict(a.model, d, batch=a.batch, device=a.device, conf=0.25, workers=a.workers)
                line = {"round": r, "MOE_PREDICT_RESIZE": switch, "images": len(res.predictions),
                        "wall_s": round(time.perf_counter() - t0, 2),
                        **{k: round(v, 3) for k, v in res.speed.items()}}
                print(json.dumps(line), flush=True)
                runs[switch].append(res.speed)
        out = {"model": a.model, "batch": a.batch, "workers": a.workers}
        for switch, name in (("1", "gpu_resize"), ("0", "host_resize")):
            for k in ("preprocess", "inference", "postprocess"):
                v = [s[k] for s in runs[switch]]
                out[f"{name}/{k}"] = [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
