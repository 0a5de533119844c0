"""engine.track with camera-motion compensation on the GPU: rtdetr_frame_shift on
the full-frame pass's model input and rtdetr_track_update_shift, per batch and
without a copy in between -- against the same call with MOE_PREDICT_TRACK=0
(motion.sequence_shifts and track_reference on what was copied back), bit for
bit, and against the offsets the frames were drawn at (rtdetr-r18-moe4-top1,
random weights; the sizes of tests/test_gpu_track_engine.py)."""
from __future__ import annotations

import pytest
import torch

from motion_cases import draw_frames

pytestmark = pytest.mark.gpu

SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)
# the steps in pixels of the model's input (the frames are 1280 x 640: two source pixels each).  seqA: 3 frames,
# seqB: 4 frames; with batch 2 the batches are [A1 A2] [A3 B1] [B2 B3] [B4 + a fill slot]: a sequence boundary
# inside a batch, and a partial last batch.
LAYOUT = (("seqA", [(0, 0), (12, -5), (-20, 8)]), ("seqB", [(0, 0), (33, 3), (-7, -14), (5, 0)]))


def _run(source, track=None, **kw):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)  # the spec's random weights: the same model in every run
    return engine.predict(SPEC, source, imgsz=IMGSZ, batch=2, device="0", conf=0.0, workers=0, track=track, **kw)


def _bands(plain):
    u = torch.unique(torch.cat([p.scores for p in plain.predictions]))
    assert len(u) >= 2, u
    lo, hi, new = (float(u[min(len(u) * q // 4, len(u) - 1)]) for q in (1, 2, 3))
    return dict(track_low=lo, track_high=hi, new_thr=new, min_hits=1)


@pytest.mark.parametrize("kw", [dict(), dict(tiles=(1, 2))], ids=["plain", "tiles"])
def test_cmc_on_the_gpu_as_on_the_host(hip_lib, tmp_path, monkeypatch, kw):
    from src.moe import _lib as L

    draw_frames(tmp_path, LAYOUT, IMGSZ)
    monkeypatch.setenv("MOE_PREDICT_TRACK", "1")
    plain = _run(tmp_path, **kw)
    bands = _bands(plain)
    L.launch_counts(reset=True)
    off = _run(tmp_path, track=bands, **kw)
    c_off = L.launch_counts(reset=True)
    same = _run(tmp_path, track=dict(bands, cmc=False), **kw)
    assert "motion" not in c_off and c_off.get("track") == 4 and "motion" not in L.launch_counts(reset=True)
    for a, b in zip(off.predictions, same.predictions):  # cmc off: today's call
        assert a.camera_shift is None and a.camera_status is None and b.camera_shift is None
        assert torch.equal(a.track_ids, b.track_ids) and torch.equal(a.track_boxes, b.track_boxes)
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_TRACK", switch)
        L.launch_counts(reset=True)
        runs[switch] = _run(tmp_path, track=dict(bands, cmc=True), **kw)
        counts[switch] = L.launch_counts(reset=True)
    # 7 frames, batch 2: four batches, three estimator launches and one tracker launch each
    assert counts["1"].get("motion") == 12 and counts["1"].get("track") == 4, counts["1"]
    assert "motion" not in counts["0"] and "track" not in counts["0"], counts["0"]
    steps = [s for _, seq in LAYOUT for s in seq]
    total = 0
    for a, b, (dx, dy) in zip(runs["1"].predictions, runs["0"].predictions, steps):
        assert a.path == b.path and (a.sequence, a.frame) == (b.sequence, b.frame)
        assert a.camera_shift == b.camera_shift == (2.0 * dx, 2.0 * dy), (a.path, a.camera_shift, b.camera_shift)
        assert a.camera_status == b.camera_status == int(a.frame > 1)
        assert torch.equal(a.track_ids, b.track_ids), (a.path, a.track_ids.tolist(), b.track_ids.tolist())
        for x, y in ((a.boxes, b.boxes), (a.scores, b.scores), (a.track_boxes, b.track_boxes)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), a.path
        assert torch.equal(a.labels, b.labels)
        if kw:
            assert torch.equal(a.source, b.source)
        total += len(a.scores)
    assert total >= 20, total
    # the shift reaches the tracks: the same detections, other track boxes than without it
    assert any(not torch.equal(a.track_boxes, b.track_boxes) for a, b in zip(runs["1"].predictions, off.predictions))
