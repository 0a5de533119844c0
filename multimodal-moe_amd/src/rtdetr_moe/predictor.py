"""Prediction on image files behind engine.predict / engine.track: detect on
frames of any size, optionally on tiles of them (merged or fused), optionally
linked into tracks, and write the results.  ``predict`` is the batch loop; the
stages it calls are the functions above it:
  _check_args, _check_candidates   the arguments' ValueErrors
  _pad_slots, _detect              one detection pass over a chunk of slots
  _tile_candidates, _pass_windows  the tile passes, the candidates per frame
  _merge_rows, _untiled_rows       a batch's candidates -> per-frame host rows
  _Tracker                         the rows through the tracker
  _prediction, _write_files        rows -> Prediction, predictions -> files
A frame's host rows are fp32 [m, C], their columns named below (BOX ... TRACK_BOX).
engine.py imports this module and re-exports its public names.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass
from functools import partial
from pathlib import Path
from types import SimpleNamespace
from typing import TYPE_CHECKING

import torch

from ..moe import _lib
from ..moe.context import MISSING_ID
from .merge import (FUSE_MAX_DET, FUSE_MAX_N, FUSE_MAX_P, MERGE_MAX_DET, MERGE_MAX_N, METRICS, fuse_reference,
                    merge_reference, parse_tiles, tile_windows, unmirror_boxes)
from .motion import MotionState, new_motion_state, sequence_shifts
from .preprocess import mapped_sizes
from .track import TRACK_MAX_K, TrackArgs, TrackState, new_state, track_reference

if TYPE_CHECKING:
    from .engine import ModelHandle


# ---------------------------------------------------------------------------
# prediction on image files
# ---------------------------------------------------------------------------
@dataclass
class Prediction:
    """One image's detections: rows with score >= conf, at most max_det, best
    first; boxes fp32 [n, 4] xyxy in source pixels, clipped to the frame."""
    path: str
    size: tuple  # (w, h) of the source frame
    ctx: int
    boxes: torch.Tensor
    scores: torch.Tensor
    labels: torch.Tensor
    # tiled prediction: the pass each row came from, int64 [n]: 0 the full frame, 1 + t tile t; with flip, P0 = 1 +
    # tiles more passes follow, pass P0 + p the mirror of pass p; None without tiles and flip
    source: torch.Tensor | None = None
    # merge="fuse": the candidates averaged into each row's box, its own included, int64 [n] (>= 1); None otherwise
    members: torch.Tensor | None = None
    # track=...: the rows are the reported ones only; each row's track id, int64 [n] (from 1 per sequence), and the
    # track's filtered box, fp32 [n, 4], clipped to the frame; the frame's sequence key and its 1-based number in it
    track_ids: torch.Tensor | None = None
    track_boxes: torch.Tensor | None = None
    sequence: str | None = None
    frame: int | None = None
    # track with cmc: the frame's camera shift (dx, dy) against its predecessor in source pixels, fp32 values, and
    # the estimator's status (motion.py: 0 no estimate -- a sequence's first frame --, 1 estimated, 2 gated)
    camera_shift: tuple | None = None
    camera_status: int | None = None


@dataclass
class PredictResults:
    predictions: list
    speed: dict
    save_dir: Path | None
    model: ModelHandle | None
    # track with gt=...: moteval.evaluate's {sequence file key: metrics, "COMBINED": metrics}; None otherwise
    # (with hota=True every metrics dict also has a "HOTA" entry)
    mot: dict | None = None
    # with track: the tracker's arguments as the run used them (TrackArgs.as_dict(): assoc among them); None otherwise
    tracker: dict | None = None


def _image_id(path):
    stem = Path(path).stem
    return int(stem) if stem.isdigit() else stem


def coco_results(predictions) -> list:
    """COCO results rows as Ultralytics' save_json writes them: image_id (the
    stem, an int when numeric), file_name, category_id, bbox xywh in source
    pixels to 3 decimals, score to 5."""
    rows = []
    for p in predictions:
        for box, s, c in zip(p.boxes.tolist(), p.scores.tolist(), p.labels.tolist()):
            x1, y1, x2, y2 = box
            rows.append({"image_id": _image_id(p.path), "file_name": Path(p.path).name, "category_id": int(c),
                         "bbox": [round(x1, 3), round(y1, 3), round(x2 - x1, 3), round(y2 - y1, 3)],
                         "score": round(s, 5)})
    return rows


def track_results(predictions) -> list:
    """coco_results' rows (the detections' boxes) plus ``track_id`` and ``sequence``."""
    rows = coco_results(predictions)
    i = 0
    for p in predictions:
        for t in p.track_ids.tolist():
            rows[i]["track_id"] = int(t)
            rows[i]["sequence"] = p.sequence
            i += 1
    return rows


def mot_lines(predictions) -> dict:
    """{sequence: MOTChallenge text}: ``frame,id,x,y,w,h,score,-1,-1,-1`` per
    reported row, frame 1-based within its sequence, the box the track's
    filtered one."""
    out = {}
    for p in predictions:
        lines = out.setdefault(p.sequence, [])
        for t, (x1, y1, x2, y2), s in zip(p.track_ids.tolist(), p.track_boxes.tolist(), p.scores.tolist()):
            lines.append(f"{p.frame},{int(t)},{x1:.3f},{y1:.3f},{x2 - x1:.3f},{y2 - y1:.3f},{s:.5f},-1,-1,-1")
    return {k: "".join(line + "\n" for line in v) for k, v in out.items()}


def camera_motion(predictions) -> dict:
    """{sequence: [[frame, dx, dy, status], ...]} of a run tracked with cmc (camera_motion.json)."""
    out = {}
    for p in predictions:
        out.setdefault(p.sequence, []).append([p.frame, p.camera_shift[0], p.camera_shift[1], p.camera_status])
    return out


def _save_overlay(pred: Prediction, out_path: Path):
    from PIL import Image, ImageDraw

    im = Image.open(pred.path).convert("RGB")
    draw = ImageDraw.Draw(im)
    for (x1, y1, x2, y2), s, c in zip(pred.boxes.tolist(), pred.scores.tolist(), pred.labels.tolist()):
        draw.rectangle([x1, y1, max(x2, x1), max(y2, y1)], outline=(255, 64, 64), width=max(1, im.width // 640))
        draw.text((x1 + 2, y1 + 2), f"{int(c)} {s:.2f}", fill=(255, 255, 0))
    im.save(out_path)


def predict_resize_on_gpu(dev: torch.device) -> bool:
    """Whether predict resizes on the GPU (rtdetr_resize_pad_u8): on a GPU
    device unless MOE_PREDICT_RESIZE=0 asks for the loader's host path."""
    return dev.type == "cuda" and os.environ.get("MOE_PREDICT_RESIZE", "1") != "0"


def predict_merge_on_gpu(dev: torch.device) -> bool:
    """Whether tiled prediction merges its passes on the GPU (rtdetr_nms_merge;
    merge="fuse": rtdetr_box_fuse): on a GPU device unless MOE_PREDICT_MERGE=0
    asks for merge.merge_reference (fuse_reference) on the copied-back
    candidates."""
    return dev.type == "cuda" and os.environ.get("MOE_PREDICT_MERGE", "1") != "0"


def predict_track_on_gpu(dev: torch.device) -> bool:
    """Whether predict(track=...) links the detections on the GPU
    (rtdetr_track_update): on a GPU device unless MOE_PREDICT_TRACK=0 asks for
    track.track_reference on the copied-back candidates."""
    return dev.type == "cuda" and os.environ.get("MOE_PREDICT_TRACK", "1") != "0"


def default_sequence_of(path) -> str:
    """A frame's sequence: its parent directory's name."""
    return Path(path).parent.name


def frame_sequences(paths, sequence_of=None) -> list:
    """[(key, sequence index, 1-based frame number)] per path: consecutive
    frames with one key form a sequence, in the given order; a key that comes
    back after another key is a ValueError."""
    sequence_of = sequence_of or default_sequence_of
    out, seen, cur, j, f = [], set(), None, -1, 0
    for p in paths:
        key = str(sequence_of(p))
        if j < 0 or key != cur:
            if key in seen:
                raise ValueError(f"sequence {key!r} comes back at {p} after another sequence: the frames of a "
                                 f"sequence must be consecutive in the source's order")
            seen.add(key)
            cur, j, f = key, j + 1, 0
        f += 1
        out.append((key, j, f))
    return out


# ---------------------------------------------------------------------------
# the stages of predict
# ---------------------------------------------------------------------------
# A frame's rows on the host, fp32 [m, C], best first: the box, the score, the label; with tiles CAND, the row's
# number among the frame's candidates (pass * k + row; the device merge marks the rows past the kept ones < 0);
# with merge="fuse" MEMBERS; and, where the tracker ran on the device, its TRACK_COLS columns last: TRACK_ID, the
# id's int32 bits, then TRACK_BOX, the track's box; with cmc the frame's CMC_COLS columns stand before those, the
# same in every row: the camera shift in source pixels and the estimator's status.  Columns that a run does not have
# are not there: no padding.
BOX, SCORE, LABEL, CAND, MEMBERS = slice(0, 4), 4, 5, 6, 7
TRACK_COLS, TRACK_ID, TRACK_BOX = 5, -5, slice(-4, None)
CMC_COLS, CMC = 3, slice(-8, -5)


def _check_args(tiles, tile_overlap, merge, merge_iou, merge_metric, fuse_iou, track, flip=False):
    """-> (TrackArgs or None, tiles (rows, cols) or None, fuse): what can be refused before a device or a model is
    touched.  ``flip``: the run has mirrored passes, which the merge's arguments then serve as they serve tiles."""
    targs = None if track is None or track is False else TrackArgs.parse(track)
    tiles = parse_tiles(tiles)
    if merge not in ("nms", "fuse"):
        raise ValueError(f"merge must be 'nms' or 'fuse', got {merge!r}")
    fuse = merge == "fuse"
    if fuse:
        if tiles is None and not flip:
            raise ValueError("merge='fuse' fuses the passes of tiled prediction: give tiles=(rows, cols)")
        if not 0.0 <= float(fuse_iou) <= 1.0:
            raise ValueError(f"fuse_iou must be in [0, 1], got {fuse_iou}")
    if tiles is not None:
        tile_windows(2 * tiles[1], 2 * tiles[0], tiles, tile_overlap)  # the overlap's ValueError, before any work
    if tiles is not None or flip:
        if merge_metric not in METRICS:
            raise ValueError(f"merge_metric must be one of {sorted(METRICS)}, got {merge_metric!r}")
        if not 0.0 <= float(merge_iou) <= 1.0:
            raise ValueError(f"merge_iou must be in [0, 1], got {merge_iou}")
    return targs, tiles, fuse


def _check_candidates(tiles, fuse, max_det, model, flip=False) -> int:
    """-> the tiles per frame (0 without tiles), once the loaded model's candidates per frame fit the merge's
    (the fusion's) limits.  ``flip`` doubles the passes: 2 P0 k candidates and 2 P0 passes, P0 = 1 + tiles."""
    if tiles is None and not flip:
        return 0
    n_tiles = 0 if tiles is None else tiles[0] * tiles[1]
    if flip:
        grid = "no tiles" if tiles is None else f"tiles {tiles[0]}x{tiles[1]}"
        n_pass = 2 * (1 + n_tiles)
        n_cand = n_pass * min(max_det, model.decoder.num_queries * model.num_classes)
        if n_cand > MERGE_MAX_N or max_det > MERGE_MAX_DET:
            raise ValueError(f"{grid} with flip and max_det {max_det} is {n_cand} candidates per frame: the merge "
                             f"takes at most {MERGE_MAX_N} candidates and max_det {MERGE_MAX_DET}")
        if fuse and (n_cand > FUSE_MAX_N or max_det > FUSE_MAX_DET or n_pass > FUSE_MAX_P):
            raise ValueError(f"{grid} with flip and max_det {max_det} is {n_pass} passes and {n_cand} candidates "
                             f"per frame: the fusion takes at most {FUSE_MAX_P} passes, {FUSE_MAX_N} candidates "
                             f"and max_det {FUSE_MAX_DET}")
        return n_tiles
    n_cand = (1 + n_tiles) * min(max_det, model.decoder.num_queries * model.num_classes)
    if n_cand > MERGE_MAX_N or max_det > MERGE_MAX_DET:
        raise ValueError(f"tiles {tiles[0]}x{tiles[1]} with max_det {max_det} is {n_cand} candidates per frame: "
                         f"the merge takes at most {MERGE_MAX_N} candidates and max_det {MERGE_MAX_DET}")
    if fuse and (n_cand > FUSE_MAX_N or max_det > FUSE_MAX_DET or 1 + n_tiles > FUSE_MAX_P):
        raise ValueError(f"tiles {tiles[0]}x{tiles[1]} with max_det {max_det} is {1 + n_tiles} passes and "
                         f"{n_cand} candidates per frame: the fusion takes at most {FUSE_MAX_P} passes, "
                         f"{FUSE_MAX_N} candidates and max_det {FUSE_MAX_DET}")
    return n_tiles


def _pad_slots(t, slots, value=0):
    """``t`` [m, ...] with empty slots of ``value`` appended up to ``slots`` rows: the captured batch size serves a
    partial chunk."""
    fill = slots - t.shape[0]
    return torch.cat([t, t.new_full((fill,) + tuple(t.shape[1:]), value)]) if fill > 0 else t


def _detect(run, ctx, windows, src=None, desc=None, images=None, full=False, mirror=False):
    """One detection pass over a chunk of m <= batch slots.  ``ctx`` int32 [m]; ``windows`` the slots' (x0, y0, w,
    h) in source pixels; the model's input is either rows ``desc`` of the resize kernel's descriptor table into
    ``src`` (one resize launch) or the host's ``images``.  On a GPU the chunk is filled to ``batch`` with empty
    slots.  ``full``: the slots are whole frames -- ``src`` is the batch's buffer on the host and goes up here (the
    one upload; the tile passes take the device's copy), the first call captures the graph (untimed), and the boxes
    are clipped without the shift by the origin (adding a zero origin would turn a -0.0 into +0.0).  ``mirror``: a
    mirrored pass (predict(flip=True)) -- the resize launch reads the slots right to left (flip = 1 per slot, one
    device tensor kept on ``run``; rtdetr_resize_pad_u8_flip; ``images`` are the host's mirrored ones) and the
    boxes are un-mirrored in their window
    (merge.unmirror_boxes with the window's width) ahead of the shift and the clip.  -> a namespace:
    boxes [S, k, 4] in source pixels, scores, labels [S, k] and lim [S, 4], the clipping limits, of all S slots, the
    m real ones first; src, and images, the model's input, on the device; the clock at t_ready, the input standing on
    the device, and at t_done, after the forward, and t_cap, the capture's seconds before t_ready.  ``run``: the
    run's model, fwd (its EvalForward), dev, batch, max_det, out_hw and pad_hw."""
    on_gpu = run.dev.type == "cuda"
    slots = run.batch if on_gpu else len(windows)
    fill = slots - len(windows)
    ctx = _pad_slots(ctx, slots, MISSING_ID).to(run.dev)
    if desc is not None:
        src = src.to(run.dev, non_blocking=True)  # a tile pass: on the device already, nothing is copied
        flags = None
        if mirror:  # one device tensor for the run: a fill slot's descriptor is empty whatever its flag says
            if getattr(run, "flip_flags", None) is None:
                run.flip_flags = torch.ones(slots, dtype=torch.int32, device=run.dev)
            flags = run.flip_flags
        images = _lib.resize_pad(src, _pad_slots(desc, slots), run.out_hw, run.pad_hw, flip=flags)
    else:
        images = _pad_slots(images, slots).to(run.dev, non_blocking=True)
        if on_gpu:
            images = images.contiguous(memory_format=torch.channels_last)
    t_cap = 0.0
    if on_gpu:
        if full:
            tc = time.perf_counter()
            run.fwd.prepare(images, ctx)  # first batch: graph capture, untimed
            t_cap = time.perf_counter() - tc
        torch.cuda.synchronize()
    t_ready = time.perf_counter()
    out = run.fwd(images, ctx)
    if on_gpu:
        torch.cuda.synchronize()
    t_done = time.perf_counter()
    mapped = mapped_sizes([(w, h) for _, _, w, h in windows], run.out_hw, run.pad_hw) + [(1.0, 1.0)] * fill
    boxes, scores, labels = run.model.postprocess_batched(out, mapped, num_top=run.max_det)
    if mirror:
        boxes = unmirror_boxes(boxes, torch.tensor([[w] for _, _, w, _ in windows] + [[1.0]] * fill,
                                                   dtype=boxes.dtype, device=boxes.device))
    lim = torch.tensor([[x0 + w, y0 + h, x0 + w, y0 + h] for x0, y0, w, h in windows] + [[1.0] * 4] * fill,
                       dtype=boxes.dtype, device=boxes.device)
    if full:
        boxes = torch.minimum(boxes.clamp(min=0.0), lim[:, None, :])
    else:  # shifted by the window's origin, clipped to the window
        lo = torch.tensor([[x0, y0, x0, y0] for x0, y0, _, _ in windows] + [[0.0] * 4] * fill, dtype=boxes.dtype,
                          device=boxes.device)
        boxes = torch.minimum(torch.maximum(boxes + lo[:, None, :], lo[:, None, :]), lim[:, None, :])
    return SimpleNamespace(boxes=boxes, scores=scores, labels=labels, lim=lim, src=src, images=images, t_cap=t_cap,
                           t_ready=t_ready, t_done=t_done)


def _tile_candidates(run, bt, full, n_tiles, mirror=False):
    """The tile passes of a batch of n frames, whose full-frame pass gave ``full`` (_detect's): the n n_tiles tiles
    are slots, frame-major, detected in chunks of ``batch`` on the captured graph (rows of bt["tile_desc"] into the
    uploaded buffer, or bt["tile_images"]) -> the candidates per frame [n, (1 + n_tiles) k, ...], the full frame's
    k rows, then each tile's, row-major, and the passes' seconds of "preprocess" and of "inference".  ``mirror``:
    the mirrored tile passes after the mirrored full-frame pass ``full`` -- the same descriptor rows read mirrored
    (or bt["flip_tile_images"]), every crop inside its own window."""
    n, k = len(bt["paths"]), full.boxes.shape[1]
    wins = [w for frame_wins in bt["windows"] for w in frame_wins]
    slot_ctx = bt["ctx"].repeat_interleave(n_tiles)
    tb, ts, tl = [], [], []
    t_pre = t_inf = 0.0
    for s in range(0, len(wins), run.batch):
        ta = time.perf_counter()
        part = slice(s, s + run.batch)
        m = len(wins[part])
        det = _detect(run, slot_ctx[part], wins[part], full.src,
                      None if full.src is None else bt["tile_desc"][part],
                      bt["flip_tile_images" if mirror else "tile_images"][part] if full.src is None else None,
                      mirror=mirror)
        tb.append(det.boxes[:m])
        ts.append(det.scores[:m])
        tl.append(det.labels[:m])
        t_pre += det.t_ready - ta
        t_inf += det.t_done - det.t_ready
    cb = torch.cat([full.boxes[:n], torch.cat(tb).reshape(n, n_tiles * k, 4)], 1)
    cs = torch.cat([full.scores[:n], torch.cat(ts).reshape(n, n_tiles * k)], 1)
    cl = torch.cat([full.labels[:n], torch.cat(tl).reshape(n, n_tiles * k)], 1)
    return cb, cs, cl, t_pre, t_inf


def _pass_windows(sizes, windows, flip=False):
    """The passes' windows per frame for the fusion, fp32 [n, P, 4] x0 y0 x1 y1 on the host: the frame, then the
    bounds each tile's boxes were clipped with (``windows``: per frame its tiles', None without tiles).  ``flip``:
    the same rows once more -- an un-mirrored box is in source coordinates and a cut side is cut on the same edge,
    so a mirrored pass has the window of its unmirrored pass."""
    win = torch.tensor([[[0.0, 0.0, float(fw), float(fh)]]
                        + [[float(x0), float(y0), float(x0 + tw), float(y0 + th)] for x0, y0, tw, th in wins]
                        for (fw, fh), wins in zip(sizes, windows or [[]] * len(sizes))], dtype=torch.float32)
    return torch.cat([win, win], 1) if flip else win


def _merge_rows(cb, cs, cl, rule, fuse_iou, win, on_device, track_block=None, heads=None) -> list:
    """The merge of a batch's candidates [n, N, ...] (the full frame's k rows, then each tile's; with flip the
    mirrored passes' in the same order after them) -> the frames' kept
    rows on the host: BOX, SCORE, LABEL, CAND and, fused, MEMBERS.  ``rule``: (conf, merge_iou, merge_metric,
    max_det, class_agnostic); ``win`` fp32 [n, P, 4], the passes' windows: fuse with ``fuse_iou`` (None: NMS).
    ``on_device``: ONE launch (rtdetr_nms_merge / rtdetr_box_fuse) and one packed copy back, which
    ``track_block(boxes, scores, labels, counts)``'s columns join (``heads``: a list that takes every frame's first
    row as copied back, kept or not -- the frame's CMC columns); else one copy of the candidates and merge_reference
    / fuse_reference per frame."""
    n = cb.shape[0]
    if on_device:
        if win is None:
            ob, osc, ol, osrc, ocnt = _lib.nms_merge(cb, cs, cl.to(torch.int32), None, *rule)
        else:
            ob, osc, ol, osrc, ocnt, om = _lib.box_fuse(cb, cs, cl.to(torch.int32), None, *rule, fuse_iou,
                                                        win.to(cb.device))
        cols = [ob, osc[..., None], ol[..., None].to(ob.dtype), osrc[..., None].to(ob.dtype)]
        if win is not None:
            cols.append(om[..., None].to(ob.dtype))
        if track_block is not None:
            cols.append(track_block(ob, osc, ol, ocnt))
        packed = torch.cat(cols, -1).cpu()  # one copy back; CAND < 0 marks the rows past the kept ones
        if heads is not None:
            heads.extend(packed[:, 0])
        return [packed[i][packed[i][:, CAND] >= 0] for i in range(n)]
    packed = torch.cat([cb, cs[..., None], cl[..., None].to(cb.dtype)], -1).cpu()
    rows = []
    for i in range(n):
        cand = packed[i]
        if win is None:
            keep = torch.from_numpy(merge_reference(cand[:, BOX], cand[:, SCORE], cand[:, LABEL], None, *rule))
            rows.append(torch.cat([cand[keep], keep[:, None].to(cand.dtype)], -1))
        else:
            keep, fb, mem = fuse_reference(cand[:, BOX], cand[:, SCORE], cand[:, LABEL], None, *rule, fuse_iou,
                                           win[i])
            keep = torch.from_numpy(keep)
            rows.append(torch.cat([torch.from_numpy(fb).reshape(-1, 4), cand[keep][:, SCORE:CAND],
                                   keep[:, None].to(cand.dtype), torch.from_numpy(mem)[:, None].to(cand.dtype)], -1))
    return rows


def _untiled_rows(full, n, conf, track_block=None, heads=None) -> list:
    """Without tiles: the full-frame pass's rows (``full``: _detect's; its first n slots are frames) in one copy
    back -> per frame those with score >= conf (a prefix: they are best first already): BOX, SCORE, LABEL.
    ``track_block`` as in _merge_rows: the tracker on the frames' candidates where they stand, the valid rows
    counted on the device; the copy is then of the n frames only.  ``heads`` as in _merge_rows."""
    cols = [full.boxes, full.scores[..., None], full.labels[..., None].to(full.boxes.dtype)]
    if track_block is not None:
        cols = [c[:n] for c in cols] + [track_block(full.boxes[:n], full.scores[:n], full.labels[:n],
                                                    (full.scores[:n] >= conf).sum(1))]
    packed = torch.cat(cols, -1).cpu()  # one copy back
    if heads is not None:
        heads.extend(packed[:n, 0])
    return [packed[i][packed[i][:, SCORE] >= conf] for i in range(n)]


class _Tracker:
    """predict(track=...)'s state over the run: the frames' sequences, and the sequences' tracks -- sequence j's in
    slot j % batch of a TrackState on the device (``on_device``: rtdetr_track_update) or of track_reference's host
    states.  Refuses max_det above the tracker's limit and a sequence key that comes back (frame_sequences).
    With targs.cmc it also owns the camera-motion estimator's state, slot for slot beside the tracks': a
    motion.MotionState on the device (rtdetr_frame_shift) or sequence_shifts' host state, which measure every
    frame's shift on the full-frame pass's model input (``out_hw``: its content size)."""

    def __init__(self, targs, paths, sequence_of, batch, max_det, dev, on_device, out_hw):
        if max_det > TRACK_MAX_K:
            raise ValueError(f"track takes at most {TRACK_MAX_K} candidates per frame, got max_det {max_det}")
        self.seq_of = frame_sequences(paths, sequence_of)  # a returning key's ValueError, before any work
        self.targs, self.batch, self.on_device, self.out_hw = targs, batch, on_device, tuple(out_hw)
        self.state = TrackState(batch, targs.max_tracks, dev) if on_device else [None] * batch
        self.cmc = bool(targs.cmc)
        self.host_shift = {}  # the host path: frame -> (dx, dy, status), shift in source pixels
        if self.cmc:
            self.motion = MotionState(batch, *out_hw, dev) if on_device else new_motion_state(batch, *out_hw)

    def _tables(self, n_done, n):
        """frame_slot and frame_reset of the batch's n frames, int32 [2, n] on the host."""
        meta = self.seq_of[n_done:n_done + n]
        return torch.tensor([[j % self.batch for _, j, _ in meta], [int(f == 1) for _, _, f in meta]],
                            dtype=torch.int32)

    def _scale(self, sizes):
        """Input pixels -> source pixels per frame, fp32 [n, 2] on the host."""
        return torch.tensor([[w / self.out_hw[1], h / self.out_hw[0]] for w, h in sizes], dtype=torch.float32)

    def device_block(self, n_done, boxes, scores, labels, n_valid, lim, images=None, sizes=None):
        """The batch's n frames, the first of which is frame ``n_done`` of the source, through ONE
        rtdetr_track_update launch -> the TRACK_COLS columns [n, K, 5] fp32 to pack: the id's bits, the track's box
        clipped to the frame (``lim`` [n, 4]).  With cmc, before it and without a host synchronisation in between:
        rtdetr_frame_shift on the first n slots of ``images`` (the full-frame pass's model input) with the same
        tables, the int shifts to source pixels by one fp32 multiply with a host-made table (``sizes``: the source
        frames'), and rtdetr_track_update_shift; the CMC_COLS columns then stand before the tracker's."""
        n, K = boxes.shape[0], boxes.shape[1]
        tab = self._tables(n_done, n).to(boxes.device)  # frame_slot, frame_reset
        shift, cols = None, []
        if self.cmc:
            a = self.targs
            ish, info = _lib.frame_shift(self.motion, images[:n], self.out_hw, tab[0], tab[1], a.cmc_radius, a.cmc_gate,
                                         a.cmc_rows)
            shift = ish.to(torch.float32) * self._scale(sizes).to(boxes.device)
            cols = [torch.cat([shift, info[:, :1].to(torch.float32)], -1)[:, None, :].expand(n, K, CMC_COLS)]
        oid, obx, _ = _lib.track_update(self.state, boxes.contiguous(), scores.contiguous(),
                                        labels.to(torch.int32).contiguous(), n_valid.to(torch.int32).contiguous(),
                                        tab[0], tab[1], self.targs, shift=shift)
        obx = torch.minimum(obx.clamp(min=0.0), lim[:, None, :])
        return torch.cat(cols + [oid.view(torch.float32)[..., None], obx], -1)

    def host_block(self, n_done, images, sizes):
        """The host path's camera shifts of the batch's n frames: the model's input copied back (its content area,
        n out_h out_w 12 bytes a batch: slow, this is the off-switch path) through motion.sequence_shifts with the
        tracker's tables; report() hands each frame's to track_reference."""
        n = len(sizes)
        oh, ow = self.out_hw
        content = images[:n].permute(0, 2, 3, 1)[:, :oh, :ow].contiguous().cpu().numpy()
        tab = self._tables(n_done, n).numpy()
        a = self.targs
        ish, info = sequence_shifts(content, tab[0], tab[1], self.motion, a.cmc_radius, round(1000 * a.cmc_gate),
                                    a.cmc_rows)
        shift = torch.from_numpy(ish).to(torch.float32) * self._scale(sizes)
        for i in range(n):
            self.host_shift[n_done + i] = (float(shift[i, 0]), float(shift[i, 1]), int(info[i, 0]))

    def report(self, frame, row, size, head=None):
        """Frame ``frame`` of the source: its rows on the host -> (the reported rows, without the tracker's columns,
        and Prediction's track_ids, track_boxes, sequence and frame; with cmc camera_shift and camera_status).  The
        rows either carry the device's columns (``head``: the frame's first row as copied back, for the CMC columns
        of a frame without rows) or go through track_reference here."""
        key, j, f = self.seq_of[frame]
        cam = {}
        if self.on_device:
            ids = row[:, TRACK_ID].contiguous().view(torch.int32)
            tbx = row[:, TRACK_BOX]
            row = row[:, :-(TRACK_COLS + (CMC_COLS if self.cmc else 0))]
            if self.cmc:
                dx, dy, status = head[CMC].tolist()
                cam = dict(camera_shift=(dx, dy), camera_status=int(status))
        else:
            if f == 1:
                self.state[j % self.batch] = new_state(self.targs.max_tracks)
            shift = None
            if self.cmc:
                dx, dy, status = self.host_shift.pop(frame)
                shift, cam = (dx, dy), dict(camera_shift=(dx, dy), camera_status=status)
            oid, obx, _ = track_reference(self.state[j % self.batch], row[:, BOX].numpy(), row[:, SCORE].numpy(),
                                          row[:, LABEL].numpy(), None, self.targs, shift=shift)
            ids = torch.from_numpy(oid)
            lim = torch.tensor([[size[0], size[1], size[0], size[1]]], dtype=torch.float32)
            tbx = torch.minimum(torch.from_numpy(obx).reshape(-1, 4).clamp(min=0.0), lim)
        sel = ids >= 0
        return row[sel], dict(track_ids=ids[sel].to(torch.int64), track_boxes=tbx[sel].contiguous(), sequence=key,
                              frame=f, **cam)


def _prediction(path, size, ctx, row, k=None, fused=False, **tracked) -> Prediction:
    """One frame's rows -> its Prediction; ``k`` (tiles): the candidates per pass, CAND // k the row's pass."""
    return Prediction(path=path, size=tuple(size), ctx=int(ctx), boxes=row[:, BOX].contiguous(),
                      scores=row[:, SCORE].contiguous(), labels=row[:, LABEL].to(torch.int64),
                      source=None if k is None else row[:, CAND].to(torch.int64) // k,
                      members=row[:, MEMBERS].to(torch.int64) if fused else None, **tracked)


def _score_tracks(preds, truth, eval_iou, dev, hota=False) -> dict:
    """moteval.evaluate of exactly the rows mot/<sequence>.txt holds: mot_lines' text, parsed back."""
    from . import moteval

    texts = {key.replace("/", "_"): text for key, text in mot_lines(preds).items()}
    return moteval.evaluate({k: truth[k] for k in texts}, texts, thr=eval_iou, device=dev, hota=hota)


def _load_truth(gt, seq_of, gt_classes, gt_ignore_classes) -> dict:
    """The ground truth of the run's sequences (moteval.load_gt), by the key their mot/ files use."""
    from . import moteval

    keys = list(dict.fromkeys(key for key, _, _ in seq_of))
    files = [k.replace("/", "_") for k in keys]
    if len(set(files)) != len(files):
        raise ValueError(f"two sequences share one file key once '/' is '_': {sorted(keys)}")
    return moteval.load_gt(gt, files, gt_classes, gt_ignore_classes)


def det_files(preds, seq_of) -> dict:
    """{sequence file key: detection text} of an untracked run (tune.det_lines: frame,-1,x,y,w,h,score,class,-1,-1,
    every fp32 value with its bits): the input of engine.tune_tracker.  ``seq_of``: frame_sequences' list."""
    from .tune import det_lines

    frames = {}
    for p, (key, _, f) in zip(preds, seq_of):
        frames.setdefault(key.replace("/", "_"), {})[f] = (p.boxes.numpy(), p.scores.numpy(), p.labels.numpy())
    return {key: det_lines(fr) for key, fr in frames.items()}


def _write_files(save_dir, preds, save_json, tracked, save_img, cmc=False, mot=None, det=None):
    """predictions.json, with a tracker tracks.json and mot/<sequence>.txt (with cmc camera_motion.json, with gt
    mot_metrics.json), with save_det det/<sequence>.txt, and the overlays."""
    save_dir.mkdir(parents=True, exist_ok=True)
    if save_json:
        (save_dir / "predictions.json").write_text(json.dumps(coco_results(preds)))
    if det is not None:
        (save_dir / "det").mkdir(exist_ok=True)
        for key, text in det_files(preds, det).items():
            (save_dir / "det" / (key + ".txt")).write_text(text)
    if tracked:
        (save_dir / "tracks.json").write_text(json.dumps(track_results(preds)))
        (save_dir / "mot").mkdir(exist_ok=True)
        for key, text in mot_lines(preds).items():
            (save_dir / "mot" / (key.replace("/", "_") + ".txt")).write_text(text)
        if cmc:
            (save_dir / "camera_motion.json").write_text(json.dumps(camera_motion(preds)))
        if mot is not None:
            (save_dir / "mot_metrics.json").write_text(json.dumps(mot))
    if save_img:
        for p in preds:
            _save_overlay(p, save_dir / Path(p.path).name)


@torch.no_grad()
def predict(weights, source, imgsz=(704, 1248), batch=16, device="0", conf=0.25, max_det=300, contexts=None,
            workers=4, project=None, name=None, save_json=True, save_img=False, tiles=None, tile_overlap=0.2,
            merge_iou=0.5, merge_metric="ios", class_agnostic=False, merge="nms", fuse_iou=0.55, track=None,
            sequence_of=None, gt=None, gt_classes=None, gt_ignore_classes=(), eval_iou=0.5,
            hota=False, save_det=False, flip=False) -> PredictResults:
    """Detect on image files of any size.  ``source``: a directory, a glob, a
    list of paths or a dataset yaml (preprocess.FrameSource).  On a GPU each
    batch is one upload of the decoded uint8 frames and ONE HIP launch
    (rtdetr_resize_pad_u8: antialiased bilinear resize to ``imgsz``, / 255,
    padding to a multiple of 32, channels-last), the graph-replayed EvalForward
    (a partial last batch is filled with empty slots, so one graph serves the
    run), postprocess_batched with each image's size mapped to its source
    frame, and one copy back.  With device="cpu" or MOE_PREDICT_RESIZE=0 the
    frames take the datasets' host path instead (PIL resize + _padded_image).
    ``workers`` threads decode (and, on the host path, resize) ahead of the GPU
    (preprocess.iter_batches); 0 reads in the calling thread.
    ``.speed``: ms per image, wall clock as ``_evaluate`` takes it (graph
    capture excluded): "preprocess" from asking the loader for the batch to the
    model's input standing on the device (decode, upload, the resize launch, or
    the host resize), "inference" the forward, "postprocess" the boxes back on
    the host.  Files, under ``project/name`` when both are given:
    predictions.json (``save_json``; COCO results) and ``save_img`` overlays.
    ``tiles=(rows, cols)``: sliced inference.  Each frame is also detected on
    an overlapping grid of crops (merge.tile_windows at ``tile_overlap``), which
    reach the model at up to rows x cols times the full frame's resolution, and
    the passes are merged (merge.merge_reference's rule with ``conf``,
    ``merge_iou``, ``merge_metric`` "ios" / "iou", ``class_agnostic`` and
    ``max_det``).  On a GPU the tiles are further rows of the resize kernel's
    descriptor table into the buffer already uploaded -- cut into chunks of
    ``batch`` slots, each one resize launch, one replay of the same captured
    graph and one postprocess_batched, boxes shifted by the window's origin and
    clipped to the window -- and the merge of a batch's [B, (1 + rows cols) k,
    4] candidates (the full frame first, then the tiles row-major; k =
    min(max_det, queries x classes), at most 4096 in all) is ONE HIP launch
    (rtdetr_nms_merge; MOE_PREDICT_MERGE=0: merge_reference on the host) and
    one packed copy back.  On the CPU, or with MOE_PREDICT_RESIZE=0, the tiles
    are cropped and resized on the host.  ``Prediction.source`` then holds the
    pass of every row and ``.speed`` gains "passes" (1 + rows cols; the three
    timings include every pass, the merge under "postprocess").  Without
    ``tiles`` nothing of this runs.
    ``merge``: "nms" (the default) keeps the best copy of every object as it
    stands.  "fuse" (tiles only) keeps the same rows -- same scores, labels,
    order and ``source`` -- and replaces each box by the score-weighted average
    of the copies of its object: the candidates it suppressed whose box agrees
    with it where both passes could see (IoU > ``fuse_iou`` after clamping both
    into the two windows' intersection; 0.55 is the usual weighted-box-fusion
    default, not tuned here), a side cut by a tile's edge left out of the
    average (merge.fuse_reference).  The windows -- the frame, then the tiles'
    clipping bounds -- go up with the batch's other small tensors; on a GPU the
    fusion is ONE HIP launch in place of the merge's (rtdetr_box_fuse;
    MOE_PREDICT_MERGE=0 or the CPU: fuse_reference) and ``Prediction.members``
    (the candidates averaged into each row) joins the one packed copy back.
    ``track``: a track.TrackArgs or a dict of its fields (True: the defaults)
    links the detections of consecutive frames (track.track_reference's rule;
    the defaults are ByteTrack's and not tuned here).  ``sequence_of`` maps a
    path to its sequence's key (default: the parent directory's name);
    consecutive frames with one key form a sequence, in the source's order, and
    a key that comes back after another is a ValueError.  Sequence j keeps its
    tracks in state slot j % batch of a track.TrackState on the device and
    clears it at its first frame, so two sequences of one batch never share a
    slot.  The candidates are postprocess_batched's rows with n_valid = the
    rows with score >= conf (a prefix, counted on the device) or, with tiles,
    the merge's / the fusion's kept rows and its count; the tracker is ONE HIP
    launch per batch after them (rtdetr_track_update; fill slots are not
    passed) and the one packed copy back gains the id and the track's box.
    MOE_PREDICT_TRACK=0, the CPU device, or a merge that ran on the host
    (MOE_PREDICT_MERGE=0 with tiles: the candidates are on the host already)
    run track_reference on the copied-back candidates instead.  A frame's
    Prediction then holds the reported rows only -- a subset of what the same
    call without ``track`` returns, the same bits in boxes, scores and labels
    -- and gains ``track_ids``, ``track_boxes`` (the filtered boxes, clipped to
    the frame), ``sequence`` and ``frame``.  Files: tracks.json (the COCO rows
    plus track_id and sequence) and mot/<sequence>.txt (frame,id,x,y,w,h,
    score,-1,-1,-1; frame 1-based, the box the track's).  With ``track=None``
    nothing of this runs.
    ``track`` with ``cmc`` (TrackArgs.cmc, off by default): camera-motion
    compensation.  Every frame's global shift against its predecessor in the
    sequence is measured on the full-frame pass's model input (motion.py's rule:
    one translation, a coarse and a fine search of ``cmc_radius`` input pixels,
    a gate ``cmc_gate`` against frames without structure, ``cmc_rows`` to keep
    the window off the car's bonnet) and the tracks' predicted boxes move by it
    before the association.  On the device that is three more launches per batch
    (rtdetr_frame_shift) ahead of the tracker's (rtdetr_track_update_shift), the
    shifts scaled to source pixels on the device, no host synchronisation in
    between; the packed copy back gains the shift and the status.  The host
    paths above run motion.sequence_shifts instead, on the model's input copied
    back -- the off-switch path: that copy is n out_h out_w 12 bytes a batch and
    slow -- and give the same shifts and the same track bits.  Tiles and the
    fusion are unaffected.  ``Prediction.camera_shift`` (dx, dy in source
    pixels) and ``.camera_status`` are set, and camera_motion.json ({sequence:
    [[frame, dx, dy, status], ...]}) is written beside tracks.json.  Without
    ``cmc`` nothing of this runs.
    ``gt`` (with ``track``; without it a ValueError): a directory of
    MOTChallenge ground truth, ``<gt>/<key>/gt/gt.txt`` or ``<gt>/<key>.txt``
    per sequence, the key the one mot/<key>.txt uses (the sequence's with '/'
    replaced by '_'); moteval.load_gt reads it before any frame is decoded, with
    ``gt_classes`` (None: all) scored and ``gt_ignore_classes`` as ignore
    regions.  After the run the tracks are scored against it (moteval.py's
    rule: CLEAR-MOT and identity metrics at IoU ``eval_iou``): exactly the rows
    of mot_lines(predictions), parsed back from their text, so that scoring the
    written mot/ directory later (scripts/eval_tracks.py) gives the same
    numbers.  On a GPU every chunk of at most 1024 frames is ONE HIP launch
    (rtdetr_mot_eval); the CPU device or MOE_TRACK_EVAL=0 run
    moteval.mot_reference and give the same result.  It goes into
    ``PredictResults.mot`` ({key: metrics, "COMBINED": metrics}) and into
    mot_metrics.json beside tracks.json.  Without ``gt`` nothing of this
    runs.
    ``hota`` (with ``gt``; without it a ValueError): every entry of
    ``PredictResults.mot`` and of mot_metrics.json gains the key "HOTA":
    hota.hota_metrics' dict (HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA
    over 19 localisation thresholds).  On a GPU every frame is scored in a
    workgroup of its own (rtdetr_hota_*); the CPU device or MOE_TRACK_EVAL=0
    run hota.hota_reference and give the same result.  Without ``hota`` the
    entries are what they are without it.
    ``save_det`` (off by default; with ``track`` a ValueError, because a tracked
    frame holds only the reported rows): det/<sequence>.txt beside
    predictions.json, the run's rows as MOTChallenge detection text
    (tune.det_lines: frame,-1,x,y,w,h,score,class,-1,-1, every fp32 value with
    its bits), sequences and frame numbers from frame_sequences as for
    tracking -- the input of engine.tune_tracker / scripts/tune_tracker.py.
    ``flip`` (off by default): horizontal-flip test-time augmentation.  Every
    pass -- the full frame and, with ``tiles``, every tile -- runs a second
    time on its window mirrored, and the merge (the fusion) takes the
    candidates of all 2 P0 passes, P0 = 1 + rows cols: today's passes first,
    then their mirrored copies in the same order, so pass P0 + p of
    ``Prediction.source`` is the mirror of pass p and ``.speed["passes"]`` is
    2 P0 (2 without tiles).  A mirrored pass's input is the resize of the
    window's mirrored bytes (preprocess.resize_reference of a[:, ::-1]; NOT the
    mirror of the resized image: the two differ in late bits wherever the taps
    are not symmetric).  On a GPU the mirrored passes are further chunks of
    ``batch`` slots over the same descriptor rows -- the full frames', then the
    tiles' -- with flip = 1 (rtdetr_resize_pad_u8_flip: one resize launch per
    chunk, reading the buffer already on the device, no second upload), each a
    replay of the same captured graph with the slots' contexts; on the host
    path the collates add host_resize of the mirrored frame or crop.  A
    mirrored pass's boxes are un-mirrored in their window
    (merge.unmirror_boxes: x1' = w - x2, x2' = w - x1 in fp32, w the window's
    width) as postprocess_batched returns them, before the shift by the
    window's origin and the clip; everything after that is what runs for
    tiles.  For the fusion a mirrored pass has its unmirrored pass's window.
    Without ``tiles`` the candidates [n, 2 k] go through the same merge /
    fusion launch, and merge="fuse" is legal.  The limits are the kernels':
    2 P0 k <= 4096 candidates, and 2 P0 <= 64 passes for the fusion (a 2x2 grid
    with flip at max_det 300 fits, a 3x3 grid does not).  The tracker and the
    camera-motion estimate hang off the merge's output and the unmirrored
    full-frame pass's input, as with tiles.  No accuracy claim is made: the
    tree has no trained weights; validate(..., flip=True) scores the same
    two-pass ensemble against ground truth.  With ``flip`` off nothing of this
    runs."""
    # engine imports this module, and tests replace engine.EvalForward and preprocess.FrameSource: looked up per call
    from . import engine, preprocess

    flip = bool(flip)
    targs, tiles, fuse = _check_args(tiles, tile_overlap, merge, merge_iou, merge_metric, fuse_iou, track, flip)
    if save_det and targs is not None:
        raise ValueError("save_det writes an untracked run's detections: a tracked frame holds only the reported rows")
    if gt is not None:
        from .moteval import check_thr

        if targs is None:
            raise ValueError("gt scores tracks: give track=... as well")
        eval_iou = check_thr(eval_iou)
    elif hota:
        raise ValueError("hota scores tracks against ground truth: give gt=... as well")
    devices = engine.parse_device(device)
    dev = torch.device("cpu") if devices == ["cpu"] else torch.device("cuda", devices[0])
    on_gpu = dev.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(dev)
        _lib.lib()
    batch, max_det = int(batch), int(max_det)
    if batch < 1 or max_det < 1:
        raise ValueError(f"batch {batch} and max_det {max_det} must be >= 1")
    model = engine.load_model(weights, dev)
    if on_gpu:
        model = model.to(memory_format=torch.channels_last)
    was_training = model.training
    model.eval()
    out_hw, pad_hw = preprocess.padded_hw(imgsz)
    gpu_resize = predict_resize_on_gpu(dev)
    n_tiles = _check_candidates(tiles, fuse, max_det, model, flip)
    merged = tiles is not None or flip  # more than one pass per frame: the candidates go through the merge
    gpu_merge = predict_merge_on_gpu(dev)
    ds = preprocess.FrameSource(source, contexts=contexts)
    tracker = None
    if targs is not None:  # on the device unless the merge left the candidates on the host
        tracker = _Tracker(targs, ds.paths, sequence_of, batch, max_det, dev,
                           predict_track_on_gpu(dev) and (not merged or gpu_merge), out_hw)
    truth = _load_truth(gt, tracker.seq_of, gt_classes, gt_ignore_classes) if gt is not None else None
    gpu_track = tracker is not None and tracker.on_device
    cmc = tracker is not None and tracker.cmc
    if tiles is None:
        collate = preprocess.PackCollate(out_hw, pin=True) if gpu_resize \
            else preprocess.HostCollate(out_hw, pad_hw, flip)
    else:
        collate = preprocess.TilePackCollate(out_hw, tiles, tile_overlap, pin=True) if gpu_resize \
            else preprocess.TileHostCollate(out_hw, pad_hw, tiles, tile_overlap, flip)
    run = SimpleNamespace(model=model, fwd=engine.EvalForward(model), dev=dev, batch=batch, max_det=max_det,
                          out_hw=out_hw, pad_hw=pad_hw)
    clock = {"preprocess": 0.0, "inference": 0.0, "postprocess": 0.0}  # seconds, every batch's
    rule = (conf, merge_iou, merge_metric, max_det, class_agnostic)
    preds = []
    # decoding threads (no processes forked under a GPU context)
    it = preprocess.iter_batches(ds, batch, workers, collate)
    while True:
        t0 = time.perf_counter()
        try:
            bt = next(it)
        except StopIteration:
            break
        n, sizes, n_done = len(bt["paths"]), bt["sizes"], len(preds)
        full = _detect(run, bt["ctx"], [(0, 0, w, h) for w, h in sizes], bt.get("buf"), bt.get("desc"),
                       bt.get("images"), full=True)
        # the tracker's launch: after the merge's (untiled: on postprocess_batched's rows), before the copy back
        track_block = partial(tracker.device_block, n_done, lim=full.lim[:n], images=full.images,
                              sizes=sizes) if gpu_track else None
        heads = [] if cmc and gpu_track else None  # every frame's first row: its CMC columns
        if cmc and not gpu_track:
            tracker.host_block(n_done, full.images, sizes)
        t_pre = t_inf = 0.0  # of the passes after the full-frame one
        if not merged:
            rows, k = _untiled_rows(full, n, conf, track_block, heads), None
        else:
            k = full.boxes.shape[1]
            cb, cs, cl = full.boxes[:n], full.scores[:n], full.labels[:n]
            if tiles is not None:
                cb, cs, cl, t_pre, t_inf = _tile_candidates(run, bt, full, n_tiles)
            if flip:  # the mirrored passes, in the same order: the full frames' descriptor rows, then the tiles'
                ta = time.perf_counter()
                mfull = _detect(run, bt["ctx"], [(0, 0, w, h) for w, h in sizes], full.src, bt.get("desc"),
                                bt.get("flip_images"), full=True, mirror=True)
                t_pre += mfull.t_ready - ta
                t_inf += mfull.t_done - mfull.t_ready
                mb, ms, ml = mfull.boxes[:n], mfull.scores[:n], mfull.labels[:n]
                if tiles is not None:
                    mb, ms, ml, tp, ti = _tile_candidates(run, bt, mfull, n_tiles, mirror=True)
                    t_pre, t_inf = t_pre + tp, t_inf + ti
                cb, cs, cl = torch.cat([cb, mb], 1), torch.cat([cs, ms], 1), torch.cat([cl, ml], 1)
            win = _pass_windows(sizes, bt.get("windows"), flip) if fuse else None
            rows = _merge_rows(cb, cs, cl, rule, fuse_iou, win, gpu_merge, track_block, heads)
        for i, row in enumerate(rows):
            tr = {}
            if tracker is not None:
                row, tr = tracker.report(n_done + i, row, sizes[i], heads[i] if heads else None)
            preds.append(_prediction(bt["paths"][i], sizes[i], bt["ctx"][i], row, k, fuse, **tr))
        t3 = time.perf_counter()
        # from asking for the batch to the input on the device, the capture taken out; the forward; the rest: every
        # pass's postprocessing, the merge, the tracker, the copy back -- the tile passes' spans moved where they belong
        clock["preprocess"] += full.t_ready - t0 - full.t_cap + t_pre
        clock["inference"] += full.t_done - full.t_ready + t_inf
        clock["postprocess"] += t3 - full.t_done - (t_pre + t_inf)
    if was_training:
        model.train()
    speed = {key: 1e3 * t / max(len(preds), 1) for key, t in clock.items()}
    if merged:
        speed["passes"] = (1 + n_tiles) * (2 if flip else 1)
    mot = _score_tracks(preds, truth, eval_iou, dev, bool(hota)) if truth is not None else None
    save_dir = Path(project) / name if project and name else None
    if save_dir is not None:
        det = frame_sequences(ds.paths, sequence_of) if save_det else None
        _write_files(save_dir, preds, save_json, tracker is not None, save_img, cmc, mot, det)
    return PredictResults(predictions=preds, speed=speed, save_dir=save_dir, model=engine.ModelHandle(model), mot=mot,
                          tracker=None if targs is None else targs.as_dict())


def track(weights, source, imgsz=(704, 1248), batch=16, device="0", conf=0.1, tracker=None, **kw) -> PredictResults:
    """``predict`` with tracking on: ``tracker`` a track.TrackArgs or a dict of
    its fields (None: the defaults); ``conf`` defaults to the tracker's low
    band, so that low-score rows can keep a track alive.  Every other argument
    is predict's."""
    return predict(weights, source, imgsz=imgsz, batch=batch, device=device, conf=conf,
                   track=True if tracker is None else tracker, **kw)
