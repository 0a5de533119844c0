"""tune.py on the CPU: the grid, the detection files' round trip, the sweep
against a loop written here from the tracker's and the evaluators' own pieces,
and the ranking against an independent argsort."""
from __future__ import annotations

import itertools
import json
import math
from pathlib import Path

import numpy as np
import pytest

from track_cases import run_reference
from tune_cases import GRID16, KEY, case, check_distinct, reference

ROOT = Path(__file__).resolve().parents[1]


def test_expand_grid_order_and_refusals():
    from src.rtdetr_moe.track import TrackArgs
    from src.rtdetr_moe.tune import SWEEPABLE, expand_grid

    assert SWEEPABLE == ("track_high", "track_low", "new_thr", "match_iou", "second_iou", "max_age", "min_hits",
                         "alpha", "beta", "class_agnostic")
    got = expand_grid({"max_age": [1, 2, 3], "alpha": [0.25, 0.75]}, base={"min_hits": 3, "max_tracks": 8})
    # sorted keys (alpha, max_age), the last fastest; everything else the base's
    assert [(c.alpha, c.max_age) for c in got] == [(0.25, 1), (0.25, 2), (0.25, 3), (0.75, 1), (0.75, 2), (0.75, 3)]
    assert all(c.min_hits == 3 and c.max_tracks == 8 and c.match_iou == TrackArgs().match_iou for c in got)
    assert expand_grid({}) == [TrackArgs()]
    g16 = expand_grid(GRID16)
    want = list(itertools.product([0.2, 0.8], [0, 3], [1, 2], [0.5, 0.7]))
    assert [(c.match_iou, c.max_age, c.min_hits, c.track_high) for c in g16] == want
    assert len(expand_grid({"max_age": list(range(32)), "min_hits": list(range(1, 33))})) == 1024
    for bad, word in (({"nonsense": [1]}, "unknown"), ({"max_tracks": [8, 16]}, "cannot be swept"),
                      ({"cmc": [True]}, "cannot be swept"), ({"cmc_radius": [8]}, "cannot be swept"),
                      ({"max_age": []}, "non-empty"), ({"max_age": 3}, "non-empty"),
                      ({"max_age": list(range(33)), "min_hits": list(range(1, 33))}, "1056"),
                      ({"min_hits": [1, 0]}, "min_hits"), ({"alpha": [float("nan")]}, "NaN")):
        with pytest.raises(ValueError, match=word):
            expand_grid(bad)


def test_det_lines_round_trip_keeps_the_bits(tmp_path):
    from src.rtdetr_moe.tune import det_lines, load_det, parse_det

    c = case(65, 2)
    frames = dict(c["dets"][KEY])
    rng = np.random.default_rng(0)
    # awkward values: a box that straddles 0, tiny and huge coordinates, a frame without rows, labels, a tied score
    frames[30] = (np.array([[-35.123456, -0.1, 0.0012345, 17.3], [1e-7, 3e5, 1e5 + 0.0078125, 3e5 + 1],
                            [5, 5, 5, 5], [7.25, 1.5, 9.75, 3.5]], np.float32),
                  np.array([0.9, 0.5, 0.5, np.float32(1) / 3], np.float32), np.array([3, 0, 2, 1], np.int32))
    frames[31] = (rng.uniform(-50, 2000, (40, 4)).astype(np.float32), np.sort(rng.random(40).astype(np.float32))[::-1],
                  rng.integers(0, 5, 40).astype(np.int32))
    frames[33] = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    text = det_lines(frames)
    (tmp_path / KEY / "det").mkdir(parents=True)
    (tmp_path / KEY / "det" / "det.txt").write_text(text)
    (tmp_path / "flat.txt").write_text(text)
    back = load_det(tmp_path, [KEY, "flat"])
    for key in (KEY, "flat"):
        assert sorted(back[key]) == sorted(f for f in frames if len(frames[f][1]))  # the empty frame has no entry
        for f, (b, s, lab) in back[key].items():
            assert b.dtype == np.float32 and s.dtype == np.float32 and lab.dtype == np.int32
            assert b.tobytes() == frames[f][0].tobytes() and s.tobytes() == frames[f][1].tobytes(), f
            assert np.array_equal(lab, frames[f][2])
    assert det_lines(back[KEY]) == text
    assert text.splitlines()[0].count(",") == 9 and text.splitlines()[0].split(",")[1] == "-1"
    # rows are stable-sorted by descending score; a missing class or -1 is label 0; a missing score is 1
    got = parse_det("2,-1,10,10,5,5,0.25,4,-1,-1\n2,-1,20,10,5,5,0.75\n2,-1,30,10,5,5,0.25,-1,-1,-1\n"
                    "2,-1,40,10,5,5,0.75,2\n1,-1,1,2,3,4\n")
    assert got[2][0][:, 0].tolist() == [20, 40, 10, 30] and got[2][1].tolist() == [0.75, 0.75, 0.25, 0.25]
    assert got[2][2].tolist() == [0, 2, 4, 0]
    assert got[1][0].tolist() == [[1, 2, 4, 6]] and got[1][1].tolist() == [1.0] and got[1][2].tolist() == [0]
    with pytest.raises(FileNotFoundError) as e:
        load_det(tmp_path, ["absent"])
    assert str(tmp_path / "absent" / "det" / "det.txt") in str(e.value) and str(tmp_path / "absent.txt") in str(e.value)


def _own_loop(c, args, T, hota=True, thr=0.5):
    """The sweep's result for one configuration from the pieces under it; nothing of tune.py."""
    from src.rtdetr_moe import hota as H
    from src.rtdetr_moe import moteval

    res = run_reference(c["seq"], args, T, n_valid=None)
    trk = {}
    for f in range(len(res["count"])):
        rows = np.nonzero(res["out_id"][f] >= 0)[0]
        if len(rows):
            trk[f + 1] = (res["out_box"][f][rows], res["out_id"][f][rows].astype(np.int64))
    sq = moteval.dense_sequence(c["gt"][KEY], trk)
    m = moteval.mot_metrics(moteval.run_reference([sq], thr)[0])
    out = {KEY: m, "COMBINED": moteval.combine([m])}
    if hota:
        m["HOTA"] = H.hota_metrics(H.run_reference_hota([sq], thr)[0])
        out["COMBINED"]["HOTA"] = H.combine_hota([m["HOTA"]])
    return out, res


def test_one_configuration_equals_a_loop_of_the_pieces():
    from src.rtdetr_moe import tune
    from src.rtdetr_moe.track import TrackArgs, states_equal

    c = case(65, 2)
    args = TrackArgs(max_age=3)
    want, res = _own_loop(c, args, args.max_tracks)
    assert want[KEY]["TP"] >= 150 and want[KEY]["IDSW"] + want[KEY]["FP"] + want[KEY]["FN"] >= 1
    got = tune.sweep(c["dets"], c["gt"], [args], hota=True)
    assert got["metrics"] == [want]
    assert got["keys"] == [KEY] and got["configs"] == [args.as_dict()] and got["metric"] == "HOTA"
    assert got["ranking"] == [0] and got["best"] == 0
    json.dumps(got)
    assert tune.sweep(c["dets"], c["gt"], {}, base=args)["metrics"] == [_own_loop(c, args, args.max_tracks, False)[0]]
    # the compact report is the compaction of the tracker's rows, and the state its state
    ref = tune.track_sweep_reference(c["dets"], [args], args.max_tracks)[0][KEY]
    assert states_equal(ref["state"], res["state"]) and np.array_equal(ref["count"], res["count"])
    for f in range(24):
        rows = np.nonzero(res["out_id"][f] >= 0)[0]
        n = len(rows)
        assert np.array_equal(ref["rows"][f, :n], rows) and (ref["rows"][f, n:] == -1).all()
        assert np.array_equal(ref["ids"][f, :n], res["out_id"][f][rows]) and (ref["ids"][f, n:] == -1).all()
        assert ref["boxes"][f, :n].tobytes() == res["out_box"][f][rows].tobytes() and not ref["boxes"][f, n:].any()
    # ground-truth-only tail frames exist for the tracker: the state ages over them
    tail = tune.track_sweep_reference(c["dets"], [args], args.max_tracks, last={KEY: 30})[0][KEY]
    assert tail["count"].shape == (30,) and not tail["count"][24:].any() and tail["state"]["hits"].sum() == 0


def _argsort(values):
    """Descending, ties to the lower index, NaN last: written apart from tune.rank."""
    idx = list(range(len(values)))
    good = [i for i in idx if not math.isnan(values[i])]
    order = []
    while good:
        top = max(values[i] for i in good)
        first = min(i for i in good if values[i] == top)
        order.append(first)
        good.remove(first)
    return order + [i for i in idx if math.isnan(values[i])]


@pytest.fixture(scope="module")
def grid_sweep():
    from src.rtdetr_moe import tune

    c = case(65, 2)
    return tune.sweep(c["dets"], c["gt"], GRID16, base={"max_tracks": 64}, hota=True)


@pytest.mark.parametrize("metric", ["HOTA", "MOTA", "IDF1"])
def test_grid16_ranking_is_an_independent_argsort(grid_sweep, metric):
    from src.rtdetr_moe import tune

    c = case(65, 2)
    check_distinct(65, 64, 2, reference(65, 64, 2)[1])
    res = grid_sweep if metric == "HOTA" else tune.sweep(c["dets"], c["gt"], GRID16, base={"max_tracks": 64},
                                                         hota=True, metric=metric)
    assert res["metric"] == metric and len(res["metrics"]) == 16
    if metric != "HOTA":
        assert res["metrics"] == grid_sweep["metrics"]
    combined = [m["COMBINED"] for m in res["metrics"]]
    values = [m["HOTA"]["HOTA"] if metric == "HOTA" else m[metric] for m in combined]
    assert len(set(values)) >= 8  # the grid matters to the score
    assert res["ranking"] == _argsort(values) and res["best"] == res["ranking"][0]
    assert sorted(res["ranking"]) == list(range(16))


def test_ties_nan_and_refusals():
    from src.rtdetr_moe import engine, tune
    from src.rtdetr_moe.track import TrackArgs

    c = case(5, 1)
    a, b = TrackArgs(max_tracks=4, max_age=3), TrackArgs(max_tracks=4, max_age=0, match_iou=0.8)
    res = tune.sweep(c["dets"], c["gt"], [b, a, b, a])
    vals = [m["COMBINED"]["MOTA"] for m in res["metrics"]]
    assert vals[0] == vals[2] and vals[1] == vals[3] and vals[0] != vals[1] and res["metric"] == "MOTA"
    assert res["ranking"] == ([1, 3, 0, 2] if vals[1] > vals[0] else [0, 2, 1, 3])
    nan = float("nan")
    assert tune.rank([0.5, nan, 0.7, 0.5, nan, -1.0]) == [2, 0, 3, 5, 1, 4] == _argsort([0.5, nan, 0.7, 0.5, nan, -1.0])
    with pytest.raises(ValueError, match="hota=True"):
        tune.sweep(c["dets"], c["gt"], [a], metric="HOTA")
    with pytest.raises(ValueError, match="metric"):
        tune.sweep(c["dets"], c["gt"], [a], metric="MOTP")
    with pytest.raises(ValueError, match="1025"):
        tune.sweep(c["dets"], c["gt"], [a] * 1025)
    with pytest.raises(ValueError, match="max_tracks"):
        tune.sweep(c["dets"], c["gt"], [a, TrackArgs(max_tracks=8)])
    with pytest.raises(ValueError, match="ground truth"):
        tune.sweep(c["dets"], {}, [a])
    big = {KEY: {1: (np.zeros((1025, 4), np.float32), np.zeros(1025, np.float32), np.zeros(1025, np.int32))}}
    with pytest.raises(ValueError, match="1025"):
        tune.sweep(big, c["gt"], [a])
    # more than 4096 reported ids in one sequence: 5 new one-frame tracks a frame, min_hits 1
    n = 4100 // 5 + 1
    box = np.array([[100 * j, 0, 100 * j + 40, 100] for j in range(5)], np.float32)
    many = {KEY: {f: (box + (f % 2) * np.float32(50), np.full(5, 0.9, np.float32), np.zeros(5, np.int32))
                  for f in range(1, n + 1)}}
    with pytest.raises(ValueError, match=str(5 * n)):
        tune.sweep(many, {KEY: {}}, [TrackArgs(max_tracks=16, min_hits=1, max_age=0, match_iou=0.9)])
    with pytest.raises(ValueError, match="save_det"):
        engine.predict("rtdetr-r18-moe4-top1", "nowhere", device="cpu", save_det=True, track=True)


def test_save_det_writes_what_load_det_reads(tmp_path):
    import torch

    from src.rtdetr_moe import engine, tune

    frames = ROOT / "tests" / "golden" / "zod_mini" / "frames"
    torch.manual_seed(0)
    kw = dict(imgsz=(320, 640), batch=4, device="cpu", conf=0.0, max_det=20, workers=0, project=str(tmp_path))
    res = engine.predict("rtdetr-r18-moe4-top1", frames, name="det", save_det=True, **kw)
    torch.manual_seed(0)
    assert not (engine.predict("rtdetr-r18-moe4-top1", frames, name="plain", **kw).save_dir / "det").exists()
    seqs = engine.frame_sequences([p.path for p in res.predictions])
    keys = sorted({k for k, _, _ in seqs})
    assert sorted(p.stem for p in (res.save_dir / "det").glob("*.txt")) == keys == tune.sequence_keys(res.save_dir / "det")
    back = tune.load_det(res.save_dir / "det", keys)
    assert sum(len(v) for v in back.values()) == len(res.predictions) >= 2
    for p, (key, _, f) in zip(res.predictions, seqs):
        b, s, lab = back[key][f]
        assert len(s) == 20 and b.tobytes() == p.boxes.numpy().tobytes() and s.tobytes() == p.scores.numpy().tobytes()
        assert np.array_equal(lab, p.labels.numpy())
