"""Tuning the tracker (engine.tune_tracker, scripts/tune_tracker.py): a grid of
TrackArgs run over the same detections and scored against ground truth, the
rule stated once.

* ``SWEEPABLE`` / ``SWEEPABLE_MODES`` / ``expand_grid``: the fields a sweep may
  vary -- the numbers the tracker's kernel takes as parameters, and the modes it
  branches on per configuration (``assoc``: "greedy" / "lsap") -- and the grid's
  configurations.
  ``max_tracks`` is the state's layout and ``cmc*`` an input (``shifts``).
* ``load_det`` / ``det_lines``: detections as MOTChallenge ``det.txt`` text
  (frame,-1,x,y,w,h,score,class,-1,-1) and back, every fp32 value with the same
  bits, so the tracker runs on files without a model (predict(save_det=True)
  writes them; MOTChallenge's public det/det.txt reads the same way).
* ``track_sweep_reference``: track.track_reference stepped over every sequence
  for every configuration -> the compact report per frame and the final state.
  The HIP kernel rtdetr_track_sweep (_lib.track_sweep) gives the same bits for
  all configurations in ONE launch per chunk of frames and is tested against
  this function; it is also the tracker of the CPU device and of
  MOE_TRACK_SWEEP=0.
* ``sweep``: tracking, then every (configuration, sequence) pair as one dense
  sequence through the evaluators (moteval.run_device / hota.run_device_hota,
  unchanged: G x S sequences are just more sequences), then the ranking.

The compact report.  A track slot is reported by at most one row per frame, so
a frame reports count <= T rows: ``ids`` int32 [T], ``boxes`` fp32 [T, 4] and
``rows`` int32 [T] hold the reported rows in row order (``rows`` the row index
d), padded with -1 / zeros / -1.

What is scored.  The tracks' fp32 boxes as the tracker leaves them, unrounded
and unclipped; no MOT text is involved.  engine.track(..., gt=...) scores the
rows of its mot/ files instead -- boxes rounded to 3 decimals and clipped to the
frame -- so its numbers may differ from a sweep's in late digits.
"""
from __future__ import annotations

import itertools
import os
import time
from dataclasses import fields
from pathlib import Path

import numpy as np

from . import moteval
from .track import (TRACK_MAX_F, TRACK_MAX_G, TRACK_MAX_K, TRACK_MAX_S, TrackArgs, new_state, track_reference)

SWEEPABLE = ("track_high", "track_low", "new_thr", "match_iou", "second_iou", "max_age", "min_hits", "alpha", "beta",
             "class_agnostic")
SWEEPABLE_MODES = ("assoc",)  # chosen per configuration inside the launch (rtdetr_track_sweep_assoc)
MAX_CONFIGS = TRACK_MAX_G
MAX_OUT_BYTES = 256 << 20  # one launch's compact outputs: G * F * T * 24 bytes stay under this
METRICS = ("HOTA", "MOTA", "IDF1")


def expand_grid(grid: dict, base=None) -> list:
    """The cartesian product of ``grid`` {field: [values]} over the keys in
    sorted order, the last key fastest; every other field from ``base`` (a
    TrackArgs or a dict of its fields; None: the defaults).  A ValueError for an
    unknown key, a key outside SWEEPABLE and SWEEPABLE_MODES, an empty list, or more than 1024
    configurations; TrackArgs' own checks run per configuration."""
    base = TrackArgs() if base is None else TrackArgs.parse(base)
    if not isinstance(grid, dict):
        raise ValueError(f"the grid must be a dict of TrackArgs fields to lists, got {type(grid).__name__}")
    known = {f.name for f in fields(TrackArgs)}
    keys = sorted(grid)
    for k in keys:
        if k not in known:
            raise ValueError(f"unknown tracker argument {k!r} in the grid")
        if k not in SWEEPABLE and k not in SWEEPABLE_MODES:
            raise ValueError(f"{k!r} cannot be swept (the sweepable fields are "
                             f"{', '.join(SWEEPABLE + SWEEPABLE_MODES)})")
        if isinstance(grid[k], (str, bytes)) or not hasattr(grid[k], "__len__") or len(grid[k]) == 0:
            raise ValueError(f"the grid's {k!r} must be a non-empty list of values")
    n = 1
    for k in keys:
        n *= len(grid[k])
    if n > MAX_CONFIGS:
        raise ValueError(f"the grid has {n} configurations; a sweep takes at most {MAX_CONFIGS}")
    start = base.as_dict()
    return [TrackArgs(**{**start, **dict(zip(keys, combo))}) for combo in itertools.product(*(grid[k] for k in keys))]


def _configs(grid_or_configs, base) -> list:
    if isinstance(grid_or_configs, dict):
        return expand_grid(grid_or_configs, base)
    configs = [TrackArgs.parse(c) for c in grid_or_configs]
    if not configs:
        raise ValueError("a sweep needs at least one configuration")
    if len(configs) > MAX_CONFIGS:
        raise ValueError(f"{len(configs)} configurations; a sweep takes at most {MAX_CONFIGS}")
    if len({c.max_tracks for c in configs}) != 1:
        raise ValueError("the configurations of one sweep share max_tracks (the state's layout)")
    return configs


# ---------------------------------------------------------------------------
# detection files
# ---------------------------------------------------------------------------
def _box(x, y, w, h):
    """x, y, w, h (fp64) -> fp32 xyxy: x and y rounded to fp32, x + w and y + h summed in fp64 and rounded once."""
    x, y = (np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64) for v in (x, y))
    w, h = (np.asarray(v, dtype=np.float64) for v in (w, h))
    return np.stack([x, y, x + w, y + h], axis=-1).astype(np.float32).reshape(-1, 4)


def parse_det(text, what="detections") -> dict:
    """MOTChallenge detection text -> {frame: (boxes fp32 [k, 4] xyxy, scores fp32 [k], labels int32 [k])}
    (load_det's rules)."""
    rows = moteval._parse(text, what, (1.0, -1.0, -1.0))
    out = {}
    frames = rows[:, 0].astype(np.int64)
    for f in np.unique(frames):
        r = rows[frames == f]
        scores = r[:, 6].astype(np.float32)
        order = np.argsort(-scores, kind="stable")
        boxes = _box(r[:, 2], r[:, 3], r[:, 4], r[:, 5])
        if not np.isfinite(boxes).all():
            raise ValueError(f"{what}: a box of frame {int(f)} is not finite")
        labels = np.where(r[:, 7] < 0, 0, r[:, 7]).astype(np.int32)
        out[int(f)] = (boxes[order], scores[order], labels[order])
    return out


def load_det(root, keys) -> dict:
    """The detections of the sequences ``keys`` under ``root``:
    ``<root>/<key>/det/det.txt``, or else ``<root>/<key>.txt``.  A line is
    frame,-1,x,y,w,h,score,class,-1,-1 (frame 1-based; a missing score is 1, a
    missing class or -1 is label 0).  x and y are rounded to fp32; x + w and y +
    h are summed in fp64 and rounded to fp32 once.  Within a frame the rows are
    stable-sorted by descending score: the tracker takes its rows best first.
    -> {key: {frame: (boxes fp32 [k, 4] xyxy, scores fp32 [k], labels int32
    [k])}}; a frame without lines has no entry.  A missing file is a
    FileNotFoundError naming both paths."""
    root = Path(root)
    out = {}
    for key in keys:
        a, b = root / key / "det" / "det.txt", root / (key + ".txt")
        path = a if a.is_file() else b
        if not path.is_file():
            raise FileNotFoundError(f"no detections for sequence {key!r}: neither {a} nor {b} exists")
        out[key] = parse_det(path.read_text(), what=str(path))
    return out


def _side(lo, hi) -> str:
    """The text of hi - lo that load_det's sum turns back into hi's bits: 9 digits, 17 where those do not do."""
    d = float(hi) - float(lo)
    for fmt in ("%.9g", "%.17g"):
        text = fmt % d
        if np.float32(float(lo) + float(text)).tobytes() == np.float32(hi).tobytes():
            return text
    raise ValueError(f"det_lines: the side {float(lo)!r} .. {float(hi)!r} has no width that reproduces it")


def det_lines(frames) -> str:
    """load_det's inverse: {frame: (boxes, scores, labels)} -> text, one line
    ``frame,-1,x,y,w,h,score,class,-1,-1`` per row in row order, the values
    written with %.9g, which names every fp32 value; w and h are x2 - x and y2 -
    y, written so that load_det's sum gives x2's and y2's bits back (%.9g of
    the difference; %.17g for the rare side where 9 digits fall short, such as
    one that straddles 0).  A frame without rows writes nothing and reads back
    as a frame without an entry."""
    lines = []
    for f in sorted(frames):
        boxes, scores, labels = frames[f]
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        scores = np.asarray(scores, np.float32).reshape(-1)
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        if int(f) < 1 or not np.isfinite(boxes).all() or not np.isfinite(scores).all():
            raise ValueError(f"det_lines: frame {f}: frames are 1-based, boxes and scores finite")
        for (x1, y1, x2, y2), s, c in zip(boxes, scores, labels):
            lines.append("%d,-1,%.9g,%.9g,%s,%s,%.9g,%d,-1,-1\n" % (int(f), x1, y1, _side(x1, x2), _side(y1, y2), s,
                                                                   int(c)))
    return "".join(lines)


# ---------------------------------------------------------------------------
# tracking: the reference and the device driver, one packing for both
# ---------------------------------------------------------------------------
def _dev(device):
    if device is None:
        return None
    import torch

    return torch.device(device)


def sweep_on_gpu(dev) -> bool:
    """The sweep's tracker runs in the HIP kernel on a GPU device unless MOE_TRACK_SWEEP=0 asks for the reference."""
    return dev is not None and dev.type == "cuda" and os.environ.get("MOE_TRACK_SWEEP", "1") != "0"


def pack_sequences(dets, last=None, shifts=None):
    """Every sequence of ``dets`` (load_det's dict) as the tracker's padded
    arrays over frames 1 .. last[key] (None: the last frame with rows): [dict(
    boxes fp32 [n, K, 4], scores fp32 [n, K], labels int32 [n, K], n_valid int32
    [n], shift fp32 [n, 2] or None)] in the dict's order, and K -- the most rows
    of any frame, at least 1.  A frame without rows has n_valid 0.  ``shifts``
    {key: fp32 [n', 2]}: frame f's camera shift at index f - 1 (frames past n'
    get 0, 0); None: no shift is added anywhere.  K above 1024 is a ValueError."""
    K = max([1, *(len(fr[1]) for frames in dets.values() for fr in frames.values())])
    if K > TRACK_MAX_K:
        raise ValueError(f"a frame has {K} detections; the tracker takes at most {TRACK_MAX_K} rows per frame")
    seqs = []
    for key, frames in dets.items():
        n = max([0, *frames]) if last is None else int(last[key])
        if frames and max(frames) > n:
            raise ValueError(f"sequence {key!r} has detections after its last frame {n}")
        sq = {"boxes": np.zeros((n, K, 4), np.float32), "scores": np.zeros((n, K), np.float32),
              "labels": np.zeros((n, K), np.int32), "n_valid": np.zeros(n, np.int32), "shift": None}
        for f, (b, s, c) in frames.items():
            k = len(s)
            sq["boxes"][f - 1, :k], sq["scores"][f - 1, :k], sq["labels"][f - 1, :k] = b, s, c
            sq["n_valid"][f - 1] = k
        if shifts is not None:
            sq["shift"] = np.zeros((n, 2), np.float32)
            given = np.asarray(shifts.get(key, np.zeros((0, 2))), np.float32).reshape(-1, 2)[:n]
            sq["shift"][:len(given)] = given
        seqs.append(sq)
    return seqs, K


def _empty_report(G, n, T):
    return {"count": np.zeros((G, n), np.int32), "ids": np.full((G, n, T), -1, np.int32),
            "boxes": np.zeros((G, n, T, 4), np.float32), "rows": np.full((G, n, T), -1, np.int32)}


def _reference_tracks(seqs, configs, T):
    """-> ([per sequence: the compact report with a leading G], states [g][j]) by track_reference."""
    G = len(configs)
    reports, states = [], [[None] * len(seqs) for _ in range(G)]
    for j, sq in enumerate(seqs):
        n = len(sq["n_valid"])
        rep = _empty_report(G, n, T)
        for g, cfg in enumerate(configs):
            st = new_state(T)
            for f in range(n):
                oid, obox, cnt = track_reference(st, sq["boxes"][f], sq["scores"][f], sq["labels"][f],
                                                 sq["n_valid"][f], cfg,
                                                 shift=None if sq["shift"] is None else sq["shift"][f])
                rows = np.nonzero(oid >= 0)[0]
                rep["count"][g, f] = cnt
                rep["ids"][g, f, :cnt], rep["boxes"][g, f, :cnt], rep["rows"][g, f, :cnt] = oid[rows], obox[rows], rows
            states[g][j] = st
        reports.append(rep)
    return reports, states


def launch_chunks(seqs, G, T):
    """The launches of ``seqs`` (slot j for sequence j), as moteval.pack_chunks
    cuts them: a chunk holds the next frames of every sequence that has frames
    left, the same number of each, a sequence's frames in order -- at most 1024
    frames, and few enough that the launch's compact outputs (G * F * T * 24
    bytes) stay under 256 MiB.  -> [[(j, first frame, last frame + 1)]]."""
    budget = max(len(seqs), min(TRACK_MAX_F, MAX_OUT_BYTES // (G * T * 24)))
    done = [0] * len(seqs)
    chunks = []
    while True:
        live = [j for j, sq in enumerate(seqs) if done[j] < len(sq["n_valid"])]
        if not live:
            return chunks
        per = max(1, budget // len(live))
        picks = []
        for j in live:
            hi = min(done[j] + per, len(seqs[j]["n_valid"]))
            picks.append((j, done[j], hi))
            done[j] = hi
        chunks.append(picks)


def max_group(G, T) -> int:
    """The sequences one SweepState serves: at most 1024, and one frame of each must fit a launch's output budget."""
    return max(1, min(TRACK_MAX_S, TRACK_MAX_F, MAX_OUT_BYTES // (G * T * 24)))


def _device_tracks(seqs, configs, T, device, stats=None):
    """_reference_tracks by rtdetr_track_sweep: one launch per chunk (launch_chunks) whatever G is; only the compact
    outputs and the states come back."""
    import torch

    from ..moe import _lib
    from .track import SweepState

    G = len(configs)
    reports = [_empty_report(G, len(sq["n_valid"]), T) for sq in seqs]
    states = [[None] * len(seqs) for _ in range(G)]
    step = max_group(G, T)
    for lo in range(0, len(seqs), step):
        group = seqs[lo:lo + step]
        state = SweepState(G, len(group), T, device)
        for picks in launch_chunks(group, G, T):
            cat = lambda key: np.concatenate([group[j][key][a:b] for j, a, b in picks])  # noqa: E731
            slot = np.concatenate([np.full(b - a, j, np.int32) for j, a, b in picks])
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device)  # noqa: E731
            shift = up(cat("shift")) if group[0]["shift"] is not None else None
            out = _lib.track_sweep(state, up(cat("boxes")), up(cat("scores")), up(cat("labels")), up(cat("n_valid")),
                                   up(slot), up(np.zeros_like(slot)), configs, shift=shift)
            oid, obox, orow, cnt = (t.cpu().numpy() for t in out)
            if stats is not None:
                stats["launches"] = stats.get("launches", 0) + 1
            i = 0
            for j, a, b in picks:
                rep = reports[lo + j]
                rep["ids"][:, a:b], rep["boxes"][:, a:b] = oid[:, i:i + b - a], obox[:, i:i + b - a]
                rep["rows"][:, a:b], rep["count"][:, a:b] = orow[:, i:i + b - a], cnt[:, i:i + b - a]
                i += b - a
        exported = state.export_all()
        for g in range(G):
            states[g][lo:lo + len(group)] = exported[g]
    return reports, states


def sweep_tracks(dets, configs, T, device=None, shifts=None, last=None, stats=None):
    """The tracker under every configuration: rtdetr_track_sweep on a GPU
    ``device`` unless MOE_TRACK_SWEEP=0, else track_sweep_reference; the same
    bits either way.  -> track_sweep_reference's list."""
    seqs, _ = pack_sequences(dets, last, shifts)
    dev = _dev(device)
    if sweep_on_gpu(dev) and seqs:
        reports, states = _device_tracks(seqs, configs, T, dev, stats)
    else:
        reports, states = _reference_tracks(seqs, configs, T)
    keys = list(dets)
    return [{key: {**{k: v[g] for k, v in reports[j].items()}, "state": states[g][j]} for j, key in enumerate(keys)}
            for g in range(len(configs))]


def track_sweep_reference(dets, configs, T, shifts=None, last=None) -> list:
    """track.track_reference stepped over frames 1 .. last[key] of every
    sequence of ``dets`` for every configuration (``last`` {key: frames}, so
    that frames only the ground truth has exist; None: the last frame with
    rows).  -> per configuration {key: dict(count int32 [n], ids int32 [n, T],
    boxes fp32 [n, T, 4], rows int32 [n, T] -- the compact report, frame f at
    index f - 1 -- and state: the final track.new_state arrays)}."""
    seqs, _ = pack_sequences(dets, last, shifts)
    configs = list(configs)
    reports, states = _reference_tracks(seqs, configs, T)
    return [{key: {**{k: v[g] for k, v in reports[j].items()}, "state": states[g][j]}
             for j, key in enumerate(dets)} for g in range(len(configs))]


# ---------------------------------------------------------------------------
# scoring and ranking
# ---------------------------------------------------------------------------
def track_frames(report) -> dict:
    """One (configuration, sequence) compact report -> {frame: (boxes fp32 [c, 4], ids int64 [c])} of the frames
    that report a row: what moteval.parse_mot makes of a tracker's file."""
    out = {}
    for i in np.nonzero(report["count"] > 0)[0]:
        c = int(report["count"][i])
        out[int(i) + 1] = (report["boxes"][i, :c].copy(), report["ids"][i, :c].astype(np.int64))
    return out


def dense_sequences(tracks, gt, keys) -> list:
    """Every (configuration, key) pair as one moteval.dense_sequence, configuration-major: the one builder both
    tracking paths go through.  More than 4096 ids in one of them is a ValueError (the evaluator's NT limit)."""
    seqs = []
    for g, per_key in enumerate(tracks):
        for key in keys:
            sq = moteval.dense_sequence(gt[key], track_frames(per_key[key]))
            if sq["NT"] > moteval.MOT_MAX_NT:
                raise ValueError(f"configuration {g} reports {sq['NT']} track ids in sequence {key!r}; the evaluator "
                                 f"takes at most {moteval.MOT_MAX_NT}")
            if sq["NG"] > moteval.MOT_MAX_NG:
                raise ValueError(f"sequence {key!r} has {sq['NG']} ground-truth ids; the evaluator takes at most "
                                 f"{moteval.MOT_MAX_NG}")
            seqs.append(sq)
    return seqs


def metric_value(combined: dict, metric: str) -> float:
    return float(combined["HOTA"]["HOTA"] if metric == "HOTA" else combined[metric])


def rank(values) -> list:
    """Indices by descending value; ties to the lower index; NaN last (among themselves by index)."""
    return sorted(range(len(values)), key=lambda i: (values[i] != values[i], -values[i] if values[i] == values[i]
                                                     else 0.0, i))


def sweep(dets, gt, grid_or_configs, base=None, eval_iou=0.5, hota=False, metric=None, device=None, shifts=None,
          timing=None) -> dict:
    """Run a grid of tracker configurations over the same detections and score
    each against ground truth.  ``dets``: load_det's dict; ``gt``: moteval.
    load_gt's, with every key of ``dets``; ``grid_or_configs``: a grid for
    expand_grid (with ``base``) or a list of TrackArgs / dicts sharing
    max_tracks; ``shifts``: {key: fp32 [n, 2]} camera shifts per frame or None.
    Tracking: on a GPU ``device`` ONE HIP launch per chunk of frames for all
    configurations (rtdetr_track_sweep; rtdetr_track_sweep_assoc when one of
    them has assoc = "lsap") unless MOE_TRACK_SWEEP=0; otherwise
    track_sweep_reference.  A sequence's frames are 1 .. the last frame either
    side has.  Scoring: every (configuration, key) pair is one
    moteval.dense_sequence (tracker ids to dense indices in ascending order)
    through moteval.run_device / run_reference and, with ``hota``,
    hota.run_device_hota / run_reference_hota, chosen by moteval.eval_on_gpu:
    the tracks' fp32 boxes, unrounded and unclipped (engine.track(gt=...)
    scores its mot/ text instead, rounded to 3 decimals and clipped to the
    frame: late digits may differ).  -> {"keys", "configs": [as_dict()],
    "metrics": [{key: mot_metrics' dict (+ "HOTA"), "COMBINED": ...}],
    "metric", "ranking": configuration indices best first, "best"}.
    ``metric``: "HOTA" (needs ``hota``; the default with it), "MOTA" (the
    default without) or "IDF1", read from COMBINED; descending, ties to the
    lower index, NaN last.  The same dict on every path.  A ValueError, with
    the number: more than 1024 configurations, a frame with more than 1024
    rows, a configuration that reports more than 4096 ids in a sequence.
    ``timing``: a dict that receives the wall-clock seconds of "tracking",
    "packing" (the dense sequences) and "scoring", and the tracker's
    "launches"."""
    configs = _configs(grid_or_configs, base)
    metric = ("HOTA" if hota else "MOTA") if metric is None else metric
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {', '.join(METRICS)}, got {metric!r}")
    if metric == "HOTA" and not hota:
        raise ValueError('metric "HOTA" needs hota=True')
    thr = moteval.check_thr(eval_iou)
    keys = list(dets)
    if "COMBINED" in keys:
        raise ValueError('a sequence may not be called "COMBINED"')
    missing = [k for k in keys if k not in gt]
    if missing:
        raise ValueError(f"no ground truth for the sequences {missing}")
    T = configs[0].max_tracks
    last = {k: max([0, *dets[k], *gt[k]]) for k in keys}
    dev = _dev(device)
    t0 = time.perf_counter()
    stats = {}
    tracks = sweep_tracks(dets, configs, T, dev, shifts, last, stats)
    t1 = time.perf_counter()
    seqs = dense_sequences(tracks, gt, keys)
    t2 = time.perf_counter()
    on_gpu = moteval.eval_on_gpu(dev) and bool(seqs)
    states = moteval.run_device(seqs, thr, dev) if on_gpu else moteval.run_reference(seqs, thr)
    S = len(keys)
    metrics = []
    for g in range(len(configs)):
        m = {k: moteval.mot_metrics(states[g * S + j]) for j, k in enumerate(keys)}
        m["COMBINED"] = moteval.combine([m[k] for k in sorted(keys)])
        metrics.append(m)
    if hota:
        from . import hota as H

        hs = H.run_device_hota(seqs, thr, dev) if on_gpu else H.run_reference_hota(seqs, thr)
        for g, m in enumerate(metrics):
            for j, k in enumerate(keys):
                m[k]["HOTA"] = H.hota_metrics(hs[g * S + j])
            m["COMBINED"]["HOTA"] = H.combine_hota([m[k]["HOTA"] for k in sorted(keys)])
    t3 = time.perf_counter()
    if timing is not None:
        timing.update(tracking=t1 - t0, packing=t2 - t1, scoring=t3 - t2, launches=stats.get("launches", 0))
    ranking = rank([metric_value(m["COMBINED"], metric) for m in metrics])
    return {"keys": keys, "configs": [c.as_dict() for c in configs], "metrics": metrics, "metric": metric,
            "ranking": ranking, "best": ranking[0]}


def mot_text(report, frames) -> str:
    """One (configuration, sequence) compact report as MOTChallenge text in predictor.mot_lines' format
    (frame,id,x,y,w,h,score,-1,-1,-1; the score is the detection's at ``rows``; the boxes are not clipped: a
    detection file does not say how large its frames are)."""
    lines = []
    for i in np.nonzero(report["count"] > 0)[0]:
        c = int(report["count"][i])
        scores = frames[int(i) + 1][1]
        for t, (x1, y1, x2, y2), d in zip(report["ids"][i, :c].tolist(), report["boxes"][i, :c].tolist(),
                                          report["rows"][i, :c].tolist()):
            lines.append(f"{int(i) + 1},{int(t)},{x1:.3f},{y1:.3f},{x2 - x1:.3f},{y2 - y1:.3f},"
                         f"{float(scores[d]):.5f},-1,-1,-1\n")
    return "".join(lines)


def sequence_keys(root) -> list:
    """The sequences of a detection directory: every <key>/det/det.txt and every <key>.txt, sorted."""
    root = Path(root)
    keys = {p.parent.parent.name for p in root.glob("*/det/det.txt")} | {p.stem for p in root.glob("*.txt")}
    if not keys:
        raise FileNotFoundError(f"no <sequence>/det/det.txt or <sequence>.txt files in {root}")
    return sorted(keys)
