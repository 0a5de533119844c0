"""The tracker's rule (track.track_reference) and engine.track on the CPU device.
No GPU: the kernel is held to this reference in tests/test_gpu_track.py."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from track_cases import check_hand_case, draw_sequence, hand_cases, identities, run_reference

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (128, 256)
# the spec's random weights score every query between 0.0127 and 0.0148: bands inside that range
TRACKER = dict(track_high=0.0142, track_low=0.0135, new_thr=0.0144, min_hits=2)


def _args(**kw):
    from src.rtdetr_moe.track import TrackArgs

    return TrackArgs(**kw)


def test_clean_sequence_one_id_per_object():
    seq = draw_sequence(12, 40, 300, seed=1)
    res = run_reference(seq, _args(), 64)
    ids, switches = identities(seq, res["out_id"])
    assert switches == 0 and sorted(v[0] for v in ids.values()) == list(range(1, 13))
    assert all(len(v) == 1 for v in ids.values())
    assert res["state"]["next_id"] == 13 and res["state"]["dropped"] == 0
    # min_hits 2: nothing reported in the first frame, everything from the second on
    assert res["count"].tolist() == [0] + [12] * 39
    # a reported box is the filtered one: on exact constant-velocity input it settles on the detection
    d = np.abs(res["out_box"][-1][:12] - seq["boxes"][-1][:12]).max()
    assert d < 0.05, d


def test_noisy_sequence_uses_every_path():
    seq = draw_sequence(20, 60, 300, seed=2, jitter=2.0, miss=0.1, low_share=0.15, fp=3)
    res = run_reference(seq, _args(), 64)
    ids, switches = identities(seq, res["out_id"])
    e = res["events"]
    assert switches == 0 and len(ids) == 20 and all(len(v) == 1 for v in ids.values())
    assert e["stage2"] >= 50 and e["refound"] >= 50 and e["tentative_freed"] >= 20, e


def test_gap_keeps_or_renews_the_id():
    a = _args(max_age=5)
    for gap, same in ((5, True), (6, False)):
        seq = draw_sequence(3, 30, 16, seed=3, gaps={1: (10, 10 + gap)})
        res = run_reference(seq, a, 8)
        ids, switches = identities(seq, res["out_id"])
        assert len(ids[0]) == 1 and len(ids[2]) == 1
        assert (len(ids[1]) == 1) == same, (gap, ids)
        assert res["events"]["expired"] == (0 if same else 1)
        if not same:
            assert ids[1][1] == 4 and switches == 1  # a new id after the three first


def test_stage_two_keeps_the_report_of_a_low_frame():
    seq = draw_sequence(1, 6, 4, seed=4)
    seq["scores"][3, 0] = 0.3  # one low frame
    on = run_reference(seq, _args(), 4)
    off = run_reference(seq, _args(track_low=0.5), 4)  # track_low == track_high: no low band
    assert on["out_id"][:, 0].tolist() == [-1, 1, 1, 1, 1, 1] and on["events"]["stage2"] == 1
    assert off["out_id"][:, 0].tolist() == [-1, 1, 1, -1, 1, 1] and off["events"]["stage2"] == 0
    assert off["events"]["refound"] == 1


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(case):
    res = run_reference(case["seq"], _args(**case["args"]), case["T"])
    check_hand_case(case, res)
    assert (res["events"]["ties"] >= 1) == (case["ties"] >= 1)
    assert res["state"]["dropped"] == case.get("dropped", 0)


def test_min_hits_one_reports_at_birth():
    seq = draw_sequence(3, 2, 8, seed=5)
    res = run_reference(seq, _args(min_hits=1), 8)
    assert res["count"].tolist() == [3, 3] and sorted(res["out_id"][0][:3].tolist()) == [1, 2, 3]
    assert np.array_equal(res["out_box"][0][:3], seq["boxes"][0][:3])


def test_four_slots_eight_objects_drop_births():
    seq = draw_sequence(8, 10, 300, seed=3)
    res = run_reference(seq, _args(), 4)
    assert res["state"]["dropped"] == res["events"]["dropped"] == 4 * 10
    assert res["state"]["next_id"] == 5 and (res["state"]["hits"] > 0).all()
    assert res["count"].tolist() == [0] + [4] * 9


def test_bad_scores_never_take_part():
    seq = draw_sequence(4, 5, 8, seed=6)
    seq["scores"][:, 1] = np.nan
    seq["scores"][:, 2] = -np.inf
    seq["scores"][:, 3] = np.inf
    res = run_reference(seq, _args(track_low=-np.inf, min_hits=1), 8, n_valid=None)
    # rows 1..3 never report; row 0 (the frame's best detection) does; the fillers are low and found nothing
    assert (res["out_id"][:, 1:4] == -1).all() and (res["out_id"][:, 0] >= 1).all()
    assert not res["out_box"][:, 1:4].any() and (res["count"] == 1).all()


def test_frame_by_frame_equals_chunks():
    from src.rtdetr_moe.track import states_equal

    seq = draw_sequence(10, 24, 64, seed=7, jitter=2.0, miss=0.15, low_share=0.15, fp=2, leave={2: 9})
    a = _args(max_age=3)
    whole = run_reference(seq, a, 16)
    parts = run_reference(seq, a, 16, chunks=[range(0, 1), range(1, 16), range(16, 24)])
    assert whole["events"]["expired"] >= 1
    for k in ("out_id", "count"):
        assert np.array_equal(whole[k], parts[k])
    assert np.array_equal(whole["out_box"].view(np.int32), parts["out_box"].view(np.int32))
    assert states_equal(whole["state"], parts["state"])


def test_track_args_are_checked():
    from src.rtdetr_moe.track import TrackArgs

    assert TrackArgs.parse(dict(max_age=3)).max_age == 3 and TrackArgs.parse(True) == TrackArgs()
    for bad in (dict(max_tracks=257), dict(max_tracks=0), dict(min_hits=0), dict(max_age=-1), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            TrackArgs(**bad)
    with pytest.raises(ValueError):
        TrackArgs.parse(dict(iou=0.3))
    with pytest.raises(ValueError):
        TrackArgs.parse("bytetrack")


def _two_sequences(root):
    """seqA (4 frames) and seqB (3 frames): tiny copies of the zod_mini frames, each shown twice or more."""
    from PIL import Image

    srcs = sorted(FRAMES.glob("*.jpg"))
    for name, idx in (("seqA", [0, 0, 1, 1]), ("seqB", [2, 2, 2])):
        (root / name).mkdir()
        for f, i in enumerate(idx):
            Image.open(srcs[i]).convert("RGB").resize((256, 128), Image.BILINEAR).save(root / name / f"{f:03d}.png")


@pytest.mark.parametrize("tiled", [dict(), dict(tiles=(2, 1)), dict(tiles=(2, 1), merge="fuse")],
                         ids=["plain", "tiles", "fuse"])
def test_engine_track_on_the_cpu(tmp_path, tiled):
    from src.rtdetr_moe import engine

    src = tmp_path / "frames"
    src.mkdir()
    _two_sequences(src)
    kw = dict(imgsz=IMGSZ, batch=2, device="cpu", conf=0.0, workers=0)
    torch.manual_seed(0)
    plain = engine.predict(SPEC, src, **kw, **tiled)
    torch.manual_seed(0)
    res = engine.track(SPEC, src, tracker=TRACKER, project=str(tmp_path), name="run", **kw, **tiled)
    assert all(p.track_ids is None and p.track_boxes is None and p.sequence is None for p in plain.predictions)
    assert [(p.sequence, p.frame) for p in res.predictions] == [("seqA", f) for f in (1, 2, 3, 4)] + \
        [("seqB", f) for f in (1, 2, 3)]
    total = 0
    for p, q in zip(res.predictions, plain.predictions):
        n = len(p.scores)
        total += n
        assert p.path == q.path and p.track_ids.dtype == torch.int64 and tuple(p.track_boxes.shape) == (n, 4)
        assert p.frame > 1 or n == 0  # min_hits 2: nothing reported in a sequence's first frame
        # the rows are a subset of predict's, in its order, with the same bits
        cols = [q.boxes, q.scores[:, None], q.labels[:, None].float()]
        mine = [p.boxes, p.scores[:, None], p.labels[:, None].float()]
        if tiled:
            cols.append(q.source[:, None].float())
            mine.append(p.source[:, None].float())
        if tiled.get("merge") == "fuse":
            cols.append(q.members[:, None].float())
            mine.append(p.members[:, None].float())
        rows = torch.cat(cols, 1).view(torch.int32).tolist()
        pos = [rows.index(r) for r in torch.cat(mine, 1).view(torch.int32).tolist()]
        assert pos == sorted(pos) and len(set(pos)) == n
        w, h = p.size
        assert bool((p.track_boxes >= 0).all() and (p.track_boxes[:, [0, 2]] <= w).all()
                    and (p.track_boxes[:, [1, 3]] <= h).all())
        assert len(set(p.track_ids.tolist())) == n and bool((p.track_ids >= 1).all())
    assert total >= 6
    if tiled:  # the full frame and both tiles have rows among the reported ones
        assert {int(v) for p in res.predictions for v in p.source} == {0, 1, 2}
    if tiled.get("merge") == "fuse":
        assert any(bool((p.members > 1).any()) for p in res.predictions)
    # ids restart at 1 per sequence
    for name in ("seqA", "seqB"):
        ids = sorted({int(t) for p in res.predictions if p.sequence == name for t in p.track_ids})
        assert ids and ids[0] == 1, (name, ids)
    # a frame shown twice: the second showing matches the first's tracks exactly where they stand
    rows = json.loads((tmp_path / "run" / "tracks.json").read_text())
    assert len(rows) == total and {"image_id", "bbox", "score", "category_id", "track_id", "sequence"} <= set(rows[0])
    assert {r["sequence"] for r in rows} == {"seqA", "seqB"}
    n_lines = 0
    for name in ("seqA", "seqB"):
        for line in (tmp_path / "run" / "mot" / f"{name}.txt").read_text().splitlines():
            f = line.split(",")
            assert len(f) == 10 and 1 <= int(f[0]) <= 4 and int(f[1]) >= 1 and f[7:] == ["-1", "-1", "-1"]
            assert all(float(v) >= 0 for v in f[2:7])
            n_lines += 1
    assert n_lines == total
    assert len(json.loads((tmp_path / "run" / "predictions.json").read_text())) == total


def test_a_sequence_key_that_returns_is_refused(tmp_path):
    from src.rtdetr_moe import engine

    _two_sequences(tmp_path)
    paths = sorted((tmp_path / "seqA").glob("*.png"))[:1] + sorted((tmp_path / "seqB").glob("*.png"))[:1] + \
        sorted((tmp_path / "seqA").glob("*.png"))[1:2]
    with pytest.raises(ValueError, match="comes back"):
        engine.track(SPEC, [str(p) for p in paths], imgsz=IMGSZ, batch=2, device="cpu", workers=0)
    # sequence_of decides: one key for all is one sequence
    torch.manual_seed(0)
    res = engine.track(SPEC, [str(p) for p in paths], imgsz=IMGSZ, batch=2, device="cpu", conf=0.0, workers=0,
                       tracker=TRACKER, sequence_of=lambda p: "all")
    assert [(p.sequence, p.frame) for p in res.predictions] == [("all", 1), ("all", 2), ("all", 3)]


def test_boundary_and_script_expose_the_tracker(tmp_path):
    from scripts import predict_detector, track_detector  # noqa: F401
    from src.models.vision import rtdetr as B
    from src.moe import _lib as L

    assert "predict_rtdetr_tracker" in B.__all__
    assert "rtdetr_track_update" in L.SIGNATURES and L.PROF_KINDS[20] == "track"
    a = predict_detector.parse_args(["--weights", SPEC, "--source", "x", "--track", "--tracker", '{"max_age": 3}'])
    assert a.track and json.loads(a.tracker) == {"max_age": 3}
    _two_sequences(tmp_path)
    torch.manual_seed(0)
    res = B.predict_rtdetr_tracker(SPEC, str(tmp_path / "seqB"), imgsz=IMGSZ, batch=2, device="cpu", conf=0.0,
                                   tracker=TRACKER)
    assert [p.frame for p in res.predictions] == [1, 2, 3] and res.predictions[0].sequence == "seqB"
    assert sum(len(p.track_ids) for p in res.predictions) >= 2
