"""engine.track on the GPU: the tracker in one rtdetr_track_update launch per
batch on the candidates where postprocess_batched or the merge left them, id and
track box with the one packed copy back -- against the same call with
MOE_PREDICT_TRACK=0 (track_reference on the copied-back rows), bit for bit
(rtdetr-r18-moe4-top1, random weights; the model and the sizes of
tests/test_gpu_predict_tiles.py)."""
from __future__ import annotations

from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)
# seqA: 3 frames, seqB: 4 frames; with batch 2 the batches are [A1 A2] [A3 B1] [B2 B3] [B4 + a fill slot]: a
# sequence boundary inside a batch, and a partial last batch.  Each source frame is shown at least twice, so that
# tracks are matched (exactly) and confirmed.
LAYOUT = (("seqA", [(0, (640, 320)), (0, (640, 320)), (1, (640, 320))]),
          ("seqB", [(2, (483, 271)), (2, (483, 271)), (3, (483, 271)), (3, (483, 271))]))


def _sequences(root):
    from PIL import Image

    srcs = sorted(FRAMES.glob("*.jpg"))
    for name, frames in LAYOUT:
        (root / name).mkdir()
        for f, (i, wh) in enumerate(frames):
            Image.open(srcs[i]).convert("RGB").resize(wh, Image.BILINEAR).save(root / name / f"{f:03d}.png")


def _run(source, track=None, **kw):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)  # the spec's random weights: the same model in every run
    return engine.predict(SPEC, source, imgsz=IMGSZ, batch=2, device="0", conf=0.0, workers=0, track=track, **kw)


def _bands(plain):
    """The random weights score every query alike, on a coarse grid of values: bands at the quartiles of the
    distinct scores."""
    u = torch.unique(torch.cat([p.scores for p in plain.predictions]))
    assert len(u) >= 2, u  # after a merge few distinct values are left: the bands may share one
    lo, hi, new = (float(u[min(len(u) * q // 4, len(u) - 1)]) for q in (1, 2, 3))
    return dict(track_low=lo, track_high=hi, new_thr=new, min_hits=2)


@pytest.mark.parametrize("kw", [dict(), dict(tiles=(1, 2)), dict(tiles=(1, 2), merge="fuse")],
                         ids=["plain", "tiles", "fuse"])
def test_track_on_the_gpu_as_on_the_host(hip_lib, tmp_path, monkeypatch, kw):
    from src.moe import _lib as L

    _sequences(tmp_path)
    monkeypatch.setenv("MOE_PREDICT_TRACK", "1")
    L.launch_counts(reset=True)
    plain = _run(tmp_path, **kw)
    assert "track" not in L.launch_counts(reset=True)
    assert all(p.track_ids is None and p.track_boxes is None for p in plain.predictions)
    tracker = _bands(plain)
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_TRACK", switch)
        L.launch_counts(reset=True)
        runs[switch] = _run(tmp_path, track=tracker, **kw)
        counts[switch] = L.launch_counts(reset=True)
    assert counts["1"].get("track") == 4 and "track" not in counts["0"], (counts["1"], counts["0"])  # 7 frames, batch 2
    merge_kind = {"fuse": "box_fuse", "nms": "merge"}[kw.get("merge", "nms")] if kw else None
    if merge_kind:
        assert counts["1"].get(merge_kind) == 4 and counts["0"].get(merge_kind) == 4
    total = 0
    want = [(name, f + 1) for name, frames in LAYOUT for f in range(len(frames))]
    assert [(p.sequence, p.frame) for p in runs["1"].predictions] == want
    for a, b, q in zip(runs["1"].predictions, runs["0"].predictions, plain.predictions):
        assert a.path == b.path == q.path and (a.sequence, a.frame) == (b.sequence, b.frame)
        assert torch.equal(a.track_ids, b.track_ids), (a.path, a.track_ids.tolist(), b.track_ids.tolist())
        for x, y in ((a.boxes, b.boxes), (a.scores, b.scores), (a.track_boxes, b.track_boxes)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), a.path
        assert torch.equal(a.labels, b.labels)
        n = len(a.scores)
        total += n
        assert a.track_ids.dtype == torch.int64 and tuple(a.track_boxes.shape) == (n, 4)
        assert a.frame > 1 or n == 0
        assert len(set(a.track_ids.tolist())) == n and bool((a.track_ids >= 1).all())
        w, h = a.size
        assert bool((a.track_boxes >= 0).all() and (a.track_boxes[:, [0, 2]] <= w).all()
                    and (a.track_boxes[:, [1, 3]] <= h).all())
        # a subset of the same call without track, in its order, with the same bits
        cols = [q.boxes, q.scores[:, None], q.labels[:, None].float()]
        mine = [a.boxes, a.scores[:, None], a.labels[:, None].float()]
        if kw:
            cols.append(q.source[:, None].float())
            mine.append(a.source[:, None].float())
            assert torch.equal(a.source, b.source)
        if kw.get("merge") == "fuse":
            cols.append(q.members[:, None].float())
            mine.append(a.members[:, None].float())
            assert torch.equal(a.members, b.members)
        rows = torch.cat(cols, 1).view(torch.int32).tolist()
        pos = [rows.index(r) for r in torch.cat(mine, 1).view(torch.int32).tolist()]
        assert pos == sorted(pos) and len(set(pos)) == n
    assert total >= 20, total
    for name, _ in LAYOUT:  # ids restart at 1 with every sequence
        ids = sorted({int(t) for p in runs["1"].predictions if p.sequence == name for t in p.track_ids})
        assert ids and ids[0] == 1, (name, ids)
    if kw:
        # a merge on the host leaves the candidates there: the tracker follows them to the reference, whatever
        # MOE_PREDICT_TRACK says, and every field is the all-GPU run's
        monkeypatch.setenv("MOE_PREDICT_MERGE", "0")
        monkeypatch.setenv("MOE_PREDICT_TRACK", "1")
        L.launch_counts(reset=True)
        host = _run(tmp_path, track=tracker, **kw)
        assert "track" not in L.launch_counts(reset=True)
        assert len(host.predictions) == len(runs["1"].predictions)
        for a, b in zip(runs["1"].predictions, host.predictions):
            assert (a.path, a.size, a.ctx, a.sequence, a.frame) == (b.path, b.size, b.ctx, b.sequence, b.frame)
            for f in ("boxes", "scores", "track_boxes"):
                assert torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32)), (a.path, f)
            for f in ("labels", "source", "track_ids"):
                assert torch.equal(getattr(a, f), getattr(b, f)), (a.path, f)
            assert (a.members is None and b.members is None) if a.members is None \
                else torch.equal(a.members, b.members)


def test_predict_without_track_is_unchanged(hip_lib, tmp_path):
    from src.moe import _lib as L

    _sequences(tmp_path)
    L.launch_counts(reset=True)
    first = _run(tmp_path)
    c = L.launch_counts(reset=True)
    second = _run(tmp_path, track=None)
    assert "track" not in c and "track" not in L.launch_counts(reset=True)
    for a, b in zip(first.predictions, second.predictions):
        assert a.path == b.path and a.track_ids is None and a.sequence is None and a.frame is None
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)
        assert len(a.scores) == 300


def test_track_limits_are_refused_before_any_launch(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    _sequences(tmp_path)
    made = []
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **kw: made.append(1))
    L.launch_counts(reset=True)
    with pytest.raises(ValueError, match="max_tracks"):
        _run(tmp_path, track=dict(max_tracks=257))
    with pytest.raises(ValueError, match="candidates"):
        _run(tmp_path, track=True, max_det=1025)
    with pytest.raises(ValueError, match="comes back"):
        _run(tmp_path, track=True, sequence_of=lambda p: Path(p).stem)  # 000, 001, 002, 000, ...
    assert not made and not L.launch_counts(reset=True)
