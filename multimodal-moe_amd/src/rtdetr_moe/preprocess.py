"""Inference inputs: image files to the model's input tensor (engine.predict).

* ``resize_reference``: the resize semantics, stated once.  The antialiased
  bilinear (triangle) filter of ``F.interpolate(..., antialias=True)``, which
  is PIL's ``resize(..., BILINEAR)`` without PIL's rounding to uint8 after each
  pass: per axis n_in -> n_out, scale = n_in / n_out, support = max(scale, 1),
  output i has centre c = scale (i + 0.5), taps j in [max(int(c - support +
  0.5), 0), min(int(c + support + 0.5), n_in)) of weight max(0, 1 - |(j - c +
  0.5) / support|) over their sum; the image filter is the outer product of the
  two axes, nothing rounded in between.  At n_in == n_out the weights are 1 and
  0 and the result is x / 255; otherwise PIL's image differs from it by at most
  one grey level (its two roundings).  The HIP kernel rtdetr_resize_pad_u8
  (_lib.resize_pad) computes this filter and is tested against this function.
* ``FrameSource``: a Dataset over image files that decodes and does nothing
  else: (uint8 HWC array, path, context id).
* ``PackCollate``: a batch of decoded frames as ONE uint8 buffer plus the
  descriptor table of rtdetr_resize_pad_u8 -- one upload per batch, a byte per
  value; the resize, / 255, padding and channels-last layout happen on the GPU.
* ``HostCollate``: the loader's host path (PIL resize + data._padded_image,
  exactly as YoloDataset / CocoDataset do it): the CPU device, and the baseline
  the kernel is measured against (MOE_PREDICT_RESIZE=0).
* ``TilePackCollate`` / ``TileHostCollate``: the same batches with the tiles of
  every frame (engine.predict(tiles=...)): further descriptor rows into the
  buffer that is uploaded anyway, or crops resized on the host.
* ``mirrored``: a frame or crop with its columns reversed.  The mirrored image
  of predict(flip=True) is the resize of the mirrored bytes (resize_reference /
  host_resize of ``mirrored(a)``), not the mirror of the resized image; on the
  GPU rtdetr_resize_pad_u8_flip reads the same descriptor rows right to left,
  and the host collates add it with ``flip``.
"""
from __future__ import annotations

import glob as _glob
import json
import math
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from ..moe.context import MISSING_ID, context_id_from_label
from .data import _IMG_EXT, _padded_image, _read_yaml

MAX_REDUCE = 8  # per-axis reduction handed to the kernel; a frame reduced further is resized on the host first


def resize_reference(hwc_uint8, out_h: int, out_w: int, pad_h: int, pad_w: int) -> torch.Tensor:
    """uint8 [h, w, 3] (array or tensor) -> fp64 [3, pad_h, pad_w]: the content
    resized to out_h x out_w top-left, / 255, zero padding."""
    x = torch.as_tensor(np.asarray(hwc_uint8)).permute(2, 0, 1)[None].double()
    y = F.interpolate(x, size=(int(out_h), int(out_w)), mode="bilinear", antialias=True, align_corners=False) / 255
    out = torch.zeros((3, int(pad_h), int(pad_w)), dtype=torch.float64)
    out[:, :out_h, :out_w] = y[0]
    return out


def padded_hw(imgsz, pad_to: int = 32):
    """((h, w), (pad_h, pad_w)) of an image size, padded as the datasets pad."""
    h, w = (imgsz, imgsz) if isinstance(imgsz, int) else (int(imgsz[0]), int(imgsz[1]))
    return (h, w), (int(math.ceil(h / pad_to) * pad_to), int(math.ceil(w / pad_to) * pad_to))


def mapped_sizes(sizes, out_hw, pad_hw):
    """The per-image (w, h) postprocess_batched scales boxes by: the model's
    boxes are normalised to the padded tensor and the content fills its
    top-left out_w x out_h, so a source of (src_w, src_h) pixels maps with
    (src_w pad_w / out_w, src_h pad_h / out_h)."""
    (h, w), (ph, pw) = out_hw, pad_hw
    return [(sw * pw / w, sh * ph / h) for sw, sh in sizes]


# ---------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------
def _coco_contexts(root: Path) -> dict:
    """{image stem: context id} of the COCO jsons under a dataset root (as
    YoloDataset._load_contexts finds them: root/*.json, root/annotations/*.json)."""
    ctx = {}
    for coco in list(root.glob("*.json")) + list((root / "annotations").glob("*.json")):
        if coco.name == "contexts.json":
            continue
        try:
            d = json.loads(coco.read_text())
            for im in d.get("images", []):
                if "solar_context_bin" in im:
                    ctx[Path(im.get("file_name", "")).stem] = context_id_from_label(im["solar_context_bin"])
        except Exception:
            continue
    return ctx


class FrameSource(torch.utils.data.Dataset):
    """Image files, decoded and nothing else.  ``source``: a directory (searched
    recursively), a glob pattern, one image file, a list of paths, or a dataset
    yaml (with ``split``).  Item: (uint8 [h, w, 3] RGB array as decoded, path,
    context id).  Context ids: ``contexts`` -- one label for every frame, or
    {image stem: label} -- else ``contexts.json`` ({stem: label}) beside the
    source, else ``images[].solar_context_bin`` of the COCO jsons of the
    source's dataset root, else MISSING_ID.  "Beside" and "root" are the
    frames' directory and its parent (a yaml: its directory and its ``path``),
    the nearer first."""

    def __init__(self, source, split: str = "val", contexts=None):
        roots = []  # where contexts.json / the COCO jsons are looked for, nearest first
        if isinstance(source, (list, tuple)):
            self.paths = [Path(p) for p in source]
            roots = [self.paths[0].parent, self.paths[0].parent.parent] if self.paths else []
        else:
            s = Path(str(source))
            if s.suffix.lower() in (".yaml", ".yml"):
                cfg = _read_yaml(s)
                root = Path(cfg.get("path", s.parent))
                if not root.is_absolute():
                    root = (s.parent / root).resolve()
                if not root.exists():
                    root = s.parent.resolve()
                rel = cfg.get(split)
                if rel is None:
                    raise KeyError(f"split {split!r} missing in {source}")
                img_dir = Path(rel) if Path(rel).is_absolute() else root / rel
                self.paths = sorted(p for p in img_dir.rglob("*") if p.suffix.lower() in _IMG_EXT)
                roots = [s.parent, root]
            elif s.is_dir():
                self.paths = sorted(p for p in s.rglob("*") if p.suffix.lower() in _IMG_EXT)
                roots = [s, s.parent]
            elif s.is_file():
                self.paths = [s]
                roots = [s.parent, s.parent.parent]
            else:
                self.paths = sorted(Path(p) for p in _glob.glob(str(source), recursive=True)
                                    if Path(p).suffix.lower() in _IMG_EXT)
                roots = [self.paths[0].parent, self.paths[0].parent.parent] if self.paths else []
        if not self.paths:
            raise FileNotFoundError(f"no image files in {source!r}")
        missing = [p for p in self.paths if not p.is_file()]
        if missing:
            raise FileNotFoundError(f"image file not found: {missing[0]}")
        self.default_ctx = MISSING_ID
        self.contexts = {}
        if contexts is not None and not isinstance(contexts, dict):
            self.default_ctx = context_id_from_label(contexts)
        elif contexts is not None:
            self.contexts = {str(k): context_id_from_label(v) for k, v in contexts.items()}
        else:
            for r in roots:
                side = r / "contexts.json"
                if side.exists():
                    self.contexts = {str(k): context_id_from_label(v) for k, v in json.loads(side.read_text()).items()}
                    break
            else:
                for r in roots:
                    self.contexts = _coco_contexts(r)
                    if self.contexts:
                        break

    def __len__(self):
        return len(self.paths)

    def context_id(self, path) -> int:
        return self.contexts.get(Path(path).stem, self.default_ctx)

    def __getitem__(self, i):
        from PIL import Image

        p = self.paths[i]
        arr = np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8)
        return arr, str(p), self.context_id(p)


# ---------------------------------------------------------------------------
# collates
# ---------------------------------------------------------------------------
def pack_frames(frames, out_hw=None, pin=False):
    """Frames (uint8 [h, w, 3] arrays) back to back in one uint8 buffer
    (page-locked with ``pin``: one asynchronous copy takes it up), and their
    descriptor table int64 [B, 4]: byte offset, height, width, row stride in
    bytes.  With ``out_hw``, a frame larger than MAX_REDUCE times the output on
    an axis is reduced to out_hw on the host first (PIL, as the loader does)
    and packed at identity scale."""
    rows, arrs, off = [], [], 0
    for a in frames:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"frame must be uint8 [h, w, 3], got {a.shape}")
        if out_hw is not None and (a.shape[0] > MAX_REDUCE * out_hw[0] or a.shape[1] > MAX_REDUCE * out_hw[1]):
            from PIL import Image

            a = np.asarray(Image.fromarray(a).resize((out_hw[1], out_hw[0]), Image.BILINEAR), dtype=np.uint8)
        h, w = a.shape[:2]
        rows.append([off, h, w, 3 * w])
        arrs.append(a.reshape(-1))
        off += 3 * h * w
    buf = torch.empty(off, dtype=torch.uint8, pin_memory=bool(pin))
    view = buf.numpy()
    for (o, h, w, _), a in zip(rows, arrs):
        view[o:o + 3 * h * w] = a
    return buf, torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)


def unpack_frame(buf, desc_row) -> np.ndarray:
    """The frame a descriptor row points at, read back from the buffer: uint8 [h, w, 3]."""
    off, h, w, stride = (int(v) for v in desc_row)
    b = buf.numpy() if isinstance(buf, torch.Tensor) else np.asarray(buf)
    return np.stack([b[off + r * stride: off + r * stride + 3 * w].reshape(w, 3) for r in range(h)]) if h > 0 \
        else np.zeros((0, w, 3), np.uint8)


class PackCollate:
    """[(frame, path, ctx)] -> {"buf": uint8 [bytes], "desc": int64 [B, 4],
    "paths", "sizes": [(w, h)] of the source frames, "ctx": int32 [B]}.  With
    ``pin`` the buffer is page-locked, so the batch goes up in one asynchronous
    copy."""

    def __init__(self, out_hw, pin=False):
        self.out_hw, self.pin = tuple(out_hw), bool(pin)

    def __call__(self, batch):
        buf, desc = pack_frames([b[0] for b in batch], self.out_hw, self.pin)
        return {"buf": buf, "desc": desc, "paths": [b[1] for b in batch],
                "sizes": [(int(b[0].shape[1]), int(b[0].shape[0])) for b in batch],
                "ctx": torch.tensor([b[2] for b in batch], dtype=torch.int32)}


def host_resize(frame: np.ndarray, out_hw, pad_hw) -> torch.Tensor:
    """The loader's image of one frame: PIL resize(BILINEAR) + data._padded_image
    (fp32 [3, pad_h, pad_w], / 255, content top-left)."""
    from PIL import Image

    im = Image.fromarray(frame).resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    return _padded_image(np.asarray(im, dtype=np.uint8), pad_hw[0], pad_hw[1], False)


def mirrored(frame: np.ndarray) -> np.ndarray:
    """A frame or a crop, uint8 [h, w, 3], with its columns reversed (a contiguous copy)."""
    return frame[:, ::-1].copy()


class HostCollate:
    """[(frame, path, ctx)] -> {"images": fp32 [B, 3, pad_h, pad_w], "paths",
    "sizes", "ctx"}: the datasets' host preprocessing.  With ``flip`` also
    "flip_images", the mirrored passes' inputs (predict(flip=True)): host_resize
    of each frame's mirrored bytes -- not the mirror of its resized image."""

    def __init__(self, out_hw, pad_hw, flip=False):
        self.out_hw, self.pad_hw, self.flip = tuple(out_hw), tuple(pad_hw), bool(flip)

    def __call__(self, batch):
        bt = {"images": torch.stack([host_resize(b[0], self.out_hw, self.pad_hw) for b in batch]),
              "paths": [b[1] for b in batch],
              "sizes": [(int(b[0].shape[1]), int(b[0].shape[0])) for b in batch],
              "ctx": torch.tensor([b[2] for b in batch], dtype=torch.int32)}
        if self.flip:
            bt["flip_images"] = torch.stack([host_resize(mirrored(b[0]), self.out_hw, self.pad_hw) for b in batch])
        return bt


# ---------------------------------------------------------------------------
# tiled prediction (engine.predict(tiles=...)): the same batches plus their tiles
# ---------------------------------------------------------------------------
class TilePackCollate(PackCollate):
    """PackCollate plus the tiles of every frame as further rows of the same
    descriptor table -- a crop of an uploaded frame is [off + y0 stride + 3 x0,
    th, tw, stride], so the tiles cost no second upload: "tile_desc" int64
    [B T, 4], frame-major, tiles row-major (merge.tile_windows on each PACKED
    frame, from its own descriptor row), and "windows": per frame its T windows
    (x0, y0, tw, th) in SOURCE pixels -- the packed window times src / packed
    per axis where pack_frames reduced the frame on the host (floats then)."""

    def __init__(self, out_hw, tiles, overlap, pin=False):
        super().__init__(out_hw, pin)
        self.tiles, self.overlap = (int(tiles[0]), int(tiles[1])), float(overlap)

    def __call__(self, batch):
        from .merge import tile_windows

        bt = super().__call__(batch)
        rows, windows = [], []
        for (off, h, w, stride), (sw, sh) in zip(bt["desc"].tolist(), bt["sizes"]):
            wins = tile_windows(w, h, self.tiles, self.overlap)
            rows += [[off + y0 * stride + 3 * x0, th, tw, stride] for x0, y0, tw, th in wins]
            if (sw, sh) != (w, h):
                sx, sy = sw / w, sh / h
                wins = [(x0 * sx, y0 * sy, tw * sx, th * sy) for x0, y0, tw, th in wins]
            windows.append(wins)
        bt["tile_desc"] = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
        bt["windows"] = windows
        return bt


class TileHostCollate(HostCollate):
    """HostCollate plus the tiles of every frame, cropped on the host (numpy
    slices of the decoded frame) and resized with host_resize: "tile_images"
    fp32 [B T, 3, pad_h, pad_w], frame-major, tiles row-major, and "windows":
    per frame its T windows (x0, y0, tw, th) in source pixels.  With ``flip``
    also "flip_tile_images": host_resize of every crop mirrored inside its own
    window."""

    def __init__(self, out_hw, pad_hw, tiles, overlap, flip=False):
        super().__init__(out_hw, pad_hw, flip)
        self.tiles, self.overlap = (int(tiles[0]), int(tiles[1])), float(overlap)

    def __call__(self, batch):
        from .merge import tile_windows

        bt = super().__call__(batch)
        imgs, flipped, windows = [], [], []
        for frame, _, _ in batch:
            wins = tile_windows(int(frame.shape[1]), int(frame.shape[0]), self.tiles, self.overlap)
            imgs += [host_resize(np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw]), self.out_hw, self.pad_hw)
                     for x0, y0, tw, th in wins]
            if self.flip:
                flipped += [host_resize(mirrored(frame[y0:y0 + th, x0:x0 + tw]), self.out_hw, self.pad_hw)
                            for x0, y0, tw, th in wins]
            windows.append(wins)
        bt["tile_images"] = torch.stack(imgs)
        if self.flip:
            bt["flip_tile_images"] = torch.stack(flipped)
        bt["windows"] = windows
        return bt


def iter_batches(ds, batch: int, workers: int, collate, ahead: int = 2):
    """collate(items) of consecutive ``batch`` items of ``ds``, in order.  With
    workers > 0 the items are read by that many THREADS (PIL decodes and
    resizes outside the interpreter lock) up to ``ahead`` batches in front of
    the consumer, and a batch is collated by one more thread while the previous
    one runs on the GPU.  Threads, not DataLoader worker processes: processes
    forked from one that holds a GPU context share its page-locked and
    GPU-mapped pages copy-on-write, and here every upload made while such
    workers were still decoding took seconds; threads also hand the decoded
    frames over without a copy through shared memory."""
    n = len(ds)
    starts = list(range(0, n, batch))
    if workers <= 0:
        for s in starts:
            yield collate([ds[i] for i in range(s, min(s + batch, n))])
        return
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(workers) as items, ThreadPoolExecutor(1) as packer:
        queue = deque()

        def submit(s):
            futs = [items.submit(ds.__getitem__, i) for i in range(s, min(s + batch, n))]
            queue.append(packer.submit(lambda: collate([f.result() for f in futs])))

        try:
            nxt = 0
            while nxt < len(starts) and nxt < ahead:
                submit(starts[nxt])
                nxt += 1
            while queue:
                out = queue.popleft().result()
                if nxt < len(starts):
                    submit(starts[nxt])
                    nxt += 1
                yield out
        finally:
            for f in queue:
                f.cancel()
