"""engine.track(..., gt=..., hota=True) on the GPU: the tracks scored by the
frame-parallel rtdetr_hota_* kernels against the same call with
MOE_TRACK_EVAL=0 (hota.hota_reference), the written mot_metrics.json against
scripts/eval_tracks.py --hota on the written mot/ directory, and the run
without hota untouched (the model, sizes, sequences and ground truth of
tests/test_gpu_mot_eval_engine.py)."""
from __future__ import annotations

import json

import pytest

from test_gpu_mot_eval_engine import _files, _write_gt
from test_gpu_track_engine import _bands, _run, _sequences

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_track_with_hota_on_the_gpu_as_on_the_host(hip_lib, tmp_path, monkeypatch):
    from scripts import eval_tracks
    from src.moe import _lib as L

    src = tmp_path / "src"
    src.mkdir()
    _sequences(src)
    monkeypatch.setenv("MOE_TRACK_EVAL", "1")
    tracker = _bands(_run(src))
    base = _run(src, track=tracker, project=str(tmp_path), name="base")
    gt = _write_gt(tmp_path / "gt", base)
    kw = dict(track=tracker, gt=gt, gt_ignore_classes=(8,), project=str(tmp_path))
    L.launch_counts(reset=True)
    plain = _run(src, name="plain", **kw)
    plain_counts = L.launch_counts(reset=True)
    assert "hota" not in plain_counts and plain_counts.get("mot_eval") == 1
    assert all("HOTA" not in m for m in plain.mot.values())
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_TRACK_EVAL", switch)
        L.launch_counts(reset=True)
        runs[switch] = _run(src, name="hota" + switch, hota=True, **kw)
        counts[switch] = L.launch_counts(reset=True)
    assert counts["1"].get("hota") == 3 and "hota" not in counts["0"], (counts["1"], counts["0"])  # 7 frames
    assert counts["1"].get("mot_eval") == 1 and "mot_eval" not in counts["0"]
    mot = runs["1"].mot
    assert mot == runs["0"].mot and list(mot) == ["seqA", "seqB", "COMBINED"]
    assert {k: {x: v for x, v in m.items() if x != "HOTA"} for k, m in mot.items()} == plain.mot
    h = mot["COMBINED"]["HOTA"]
    assert h["arrays"]["TP"][0] >= 10 and h["arrays"]["FP"][0] >= 2 and 0.0 < h["HOTA"] <= h["HOTA(0)"] <= 1.0, h
    # the files: "HOTA" in the metrics only when asked, everything else as without it
    for name in ("hota1", "hota0"):
        got = _files(tmp_path / name)
        assert json.loads(got.pop("mot_metrics.json")) == mot
        want = _files(tmp_path / "plain")
        assert json.loads(want.pop("mot_metrics.json")) == plain.mot
        assert got == want
    out = tmp_path / "again.json"
    again = eval_tracks.main(["--gt", str(gt), "--results", str(tmp_path / "hota1" / "mot"), "--gt-ignore-classes",
                              "8", "--hota", "--out", str(out)])
    assert again == mot == json.loads(out.read_text())
    assert eval_tracks.score(gt, tmp_path / "hota1" / "mot", gt_ignore_classes=[8], device="cpu", hota=True) == mot


@pytest.mark.timeout(120)
def test_hota_without_gt_is_refused_before_any_work(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    src = tmp_path / "src"
    src.mkdir()
    _sequences(src)
    made = []
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **kw: made.append(1))
    L.launch_counts(reset=True)
    with pytest.raises(ValueError, match="gt"):
        _run(src, track=True, hota=True)
    assert not made and not L.launch_counts(reset=True)
