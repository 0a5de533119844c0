"""engine.track(..., gt=...) on the GPU: the tracks scored by rtdetr_mot_eval, one
launch per chunk of frames, against the same call with MOE_TRACK_EVAL=0
(moteval.mot_reference), the written mot_metrics.json against
scripts/eval_tracks.py on the written mot/ directory, and the run without gt
untouched (the model, sizes and sequences of tests/test_gpu_track_engine.py)."""
from __future__ import annotations

import json

import pytest
import torch

from test_gpu_track_engine import LAYOUT, _bands, _run, _sequences

pytestmark = pytest.mark.gpu


def _write_gt(root, tracked):
    """Ground truth made from a tracked run: every reported row's track box moved by 1.5 px, id + 100, class 1;
    every fifth row left out (a false positive), one ignore region (class 8) on a row of seqB, one conf == 0 row.
    seqA in the <key>/gt/gt.txt layout, seqB as <key>.txt."""
    lines = {name: [] for name, _ in LAYOUT}
    n = 0
    for p in tracked.predictions:
        for t, (x1, y1, x2, y2) in zip(p.track_ids.tolist(), p.track_boxes.tolist()):
            n += 1
            if n % 5 == 0:
                continue
            cls = 8 if (p.sequence == "seqB" and n % 7 == 0) else 1
            box = f"{x1 + 1.5:.2f},{y1:.2f},{x2 - x1:.2f},{y2 - y1:.2f}"
            lines[p.sequence].append(f"{p.frame},{100 + t},{box},1,{cls},1")
    lines["seqA"].append("1,999,5,5,20,20,0,1,1")
    (root / "seqA" / "gt").mkdir(parents=True)
    (root / "seqA" / "gt" / "gt.txt").write_text("\n".join(lines["seqA"]) + "\n")
    (root / "seqB.txt").write_text("\n".join(lines["seqB"]) + "\n")
    return root


def _files(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


@pytest.mark.timeout(600)
def test_track_with_gt_on_the_gpu_as_on_the_host(hip_lib, tmp_path, monkeypatch):
    from scripts import eval_tracks
    from src.moe import _lib as L

    src = tmp_path / "src"
    src.mkdir()
    _sequences(src)
    monkeypatch.setenv("MOE_TRACK_EVAL", "1")
    tracker = _bands(_run(src))
    L.launch_counts(reset=True)
    base = _run(src, track=tracker, project=str(tmp_path), name="base")
    assert "mot_eval" not in L.launch_counts(reset=True)
    assert base.mot is None and not (tmp_path / "base" / "mot_metrics.json").exists()
    gt = _write_gt(tmp_path / "gt", base)
    kw = dict(track=tracker, gt=gt, gt_ignore_classes=(8,), project=str(tmp_path))
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_TRACK_EVAL", switch)
        L.launch_counts(reset=True)
        runs[switch] = _run(src, name="gt" + switch, **kw)
        counts[switch] = L.launch_counts(reset=True)
    assert counts["1"].get("mot_eval") == 1 and "mot_eval" not in counts["0"], (counts["1"], counts["0"])  # 7 frames
    mot = runs["1"].mot
    assert mot == runs["0"].mot and list(mot) == ["seqA", "seqB", "COMBINED"]
    c = mot["COMBINED"]
    assert c["frames"] == 7 and c["TP"] >= 10 and c["FP"] >= 2 and c["removed"] >= 1 and c["IDTP"] >= 10, c
    assert c["TP"] == mot["seqA"]["TP"] + mot["seqB"]["TP"]
    # the files: the metrics beside the tracks; everything else as without gt
    for name in ("gt1", "gt0"):
        got = _files(tmp_path / name)
        assert json.loads(got.pop("mot_metrics.json")) == mot
        assert got == _files(tmp_path / "base")
    for a, b in zip(runs["1"].predictions, base.predictions):
        assert a.path == b.path and torch.equal(a.track_ids, b.track_ids)
        assert torch.equal(a.track_boxes.view(torch.int32), b.track_boxes.view(torch.int32))
    # scoring the written directory later gives the same numbers, on either path
    out = tmp_path / "again.json"
    again = eval_tracks.main(["--gt", str(gt), "--results", str(tmp_path / "gt1" / "mot"), "--gt-ignore-classes", "8",
                              "--out", str(out)])
    assert again == mot == json.loads(out.read_text())
    assert eval_tracks.score(gt, tmp_path / "gt1" / "mot", gt_ignore_classes=[8], device="cpu") == mot


@pytest.mark.timeout(120)
def test_gt_is_refused_before_any_work(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    src = tmp_path / "src"
    src.mkdir()
    _sequences(src)
    made = []
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **kw: made.append(1))
    L.launch_counts(reset=True)
    with pytest.raises(ValueError, match="track"):
        _run(src, gt=tmp_path)
    with pytest.raises(ValueError, match="IoU"):
        _run(src, track=True, gt=tmp_path, eval_iou=0.0)
    with pytest.raises(FileNotFoundError, match="seqA"):
        _run(src, track=True, gt=tmp_path / "nothing")
    assert not made and not L.launch_counts(reset=True)
