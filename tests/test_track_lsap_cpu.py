"""TrackArgs.assoc = "lsap" on the CPU: the rule (track.track_reference, step 4
"lsap"), its optimality against a brute force, the default path's keys, the
preconditions of the drawn GPU cases, and the plumbing (TrackArgs, the sweep's
grid, engine.predict, tune.sweep, the C ABI's declarations).  No GPU: the kernel
is held to this reference in tests/test_gpu_track_lsap.py."""
from __future__ import annotations

import itertools
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import track_lsap_cases as C
from track_cases import check_hand_case
from tune_cases import KEY, case

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (128, 256)
TRACKER = dict(track_high=0.0142, track_low=0.0135, new_thr=0.0144, min_hits=2)  # test_track_cpu.py's bands


def _args(**kw):
    from src.rtdetr_moe.track import TrackArgs

    return TrackArgs(**kw)


@pytest.mark.parametrize("case_", C.lsap_hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(case_):
    c = case_
    n = int(c["seq"]["n_valid"][0])
    for assoc, want in (("lsap", c["ids"]), ("greedy", c["greedy"])):
        res = C.run(c["seq"], _args(max_tracks=c["T"], assoc=assoc, **c["args"]), c["T"],
                    state=C.state_of(c["T"], c["tracks"]))
        got = res["out_id"][0].tolist()
        assert got[:n] == want and all(v == -1 for v in got[n:]), (c["name"], assoc, got, want)
        if assoc == "lsap":
            assert res["events"]["solve_shapes"] == c["solves"] and res["events"]["ties"] == 0
            assert res["events"]["solves"] == len(c["solves"])
            assert res["events"]["solve_n_max"] == max(min(s) for s in c["solves"])
            assert res["events"]["solve_q_max"] == max(max(s) for s in c["solves"])


def test_the_worked_example_differs_between_the_modes():
    c = C.lsap_hand_cases()[0]
    assert c["name"] == "two_people" and c["ids"] == [2, 1] and c["greedy"] == [1, 3]
    orient = [s for h in C.lsap_hand_cases() for s in h["solves"]]  # every orientation among the hand cases
    assert any(a > b for a, b in orient) and any(a < b for a, b in orient) and any(a == b for a, b in orient)


@pytest.mark.parametrize("case_", C.tie_cases(), ids=lambda c: c["name"])
def test_tie_cases_under_lsap(case_):
    c = case_
    res = C.run(c["seq"], _args(max_tracks=c["T"], max_age=3, assoc="lsap", **c["args"]), c["T"])
    check_hand_case(c, res)
    assert res["events"]["ties"] == 0  # a greedy notion: not counted


def _best_total(adm, iou64):
    """The largest fp64 IoU sum over the one-to-one matchings of admissible pairs, by brute force."""
    nt, nd = adm.shape
    best = 0.0
    for k in range(1, min(nt, nd) + 1):
        for ts in itertools.combinations(range(nt), k):
            for ds in itertools.permutations(range(nd), k):
                if all(adm[t, d] for t, d in zip(ts, ds)):
                    best = max(best, float(sum(iou64[t, d] for t, d in zip(ts, ds))))
    return best


def test_optimality_against_brute_force():
    from src.rtdetr_moe.track import _associate_lsap, _iou

    rng = np.random.default_rng(0)
    solved = nontrivial = 0
    for trial in range(200):
        nt, nd = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        # 40 x 100 boxes a few pixels apart: most pairs overlap, many above the threshold
        tx, dx = rng.uniform(0, 60, nt), rng.uniform(0, 60, nd)
        box = np.stack([tx, np.zeros(nt), tx + 40, np.full(nt, 100.0)], 1).astype(np.float32)
        b = np.stack([dx, rng.uniform(-5, 5, nd), dx + 40, np.full(nd, 100.0)], 1).astype(np.float32)
        label, lab = rng.integers(0, 2, nt).astype(np.int32), rng.integers(0, 2, nd).astype(np.int32)
        agnostic = bool(trial % 2)
        thr = float(rng.choice([-1.0, 0.0, 0.2, 0.5]))
        events = {"solves": 0, "solve_n_max": 0, "solve_q_max": 0}
        got = _associate_lsap(np.arange(nt), np.arange(nd), box, label, b, lab, thr, agnostic, events)
        iou = _iou(box, b)
        adm = iou > np.float32(thr)
        if not agnostic:
            adm &= label[:, None] == lab[None, :]
        assert all(adm[t, d] for t, d in got)
        assert len({t for t, _ in got}) == len(got) == len({d for _, d in got})
        total = float(sum(np.float64(iou[t, d]) for t, d in got))
        best = _best_total(adm, iou.astype(np.float64))
        assert abs(total - best) <= 1e-9, (trial, total, best)
        assert events["solves"] == (1 if adm.any() else 0)
        solved += events["solves"]
        nontrivial += int(adm.sum() > max(adm.any(0).sum(), adm.any(1).sum()))
    assert solved >= 150 and nontrivial >= 100  # the draw does exercise the solver


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_preconditions_of_the_drawn_gpu_cases(shape):
    C.check_preconditions(shape)


def test_coverage_of_the_drawn_gpu_cases():
    C.check_coverage()


def test_default_path_keeps_its_keys():
    from src.rtdetr_moe.track import EVENTS, LSAP_EVENTS, TrackArgs

    assert TrackArgs().assoc == "greedy" and TrackArgs().as_dict()["assoc"] == "greedy"
    assert EVENTS == ("stage1", "stage2", "refound", "tentative_freed", "expired", "births", "dropped", "ties",
                      "reported")
    assert LSAP_EVENTS == ("solves", "solve_n_max", "solve_q_max")
    c = C.drawn(C.SHAPES[6])
    assert tuple(c["greedy"]["events"]) == EVENTS
    assert set(c["ref"]["events"]) == set(EVENTS + LSAP_EVENTS) | {"solve_shapes"}


def test_bad_assoc_values_are_refused():
    from src.rtdetr_moe.track import TrackArgs

    for bad in ("hungarian", "LSAP", "", None, 1, True):
        with pytest.raises(ValueError, match='"greedy" or "lsap"'):
            TrackArgs(assoc=bad)
    assert TrackArgs.parse({"assoc": "lsap"}).assoc == "lsap"


def test_expand_grid_takes_assoc():
    from src.rtdetr_moe.tune import SWEEPABLE, SWEEPABLE_MODES, expand_grid

    assert SWEEPABLE == ("track_high", "track_low", "new_thr", "match_iou", "second_iou", "max_age", "min_hits",
                         "alpha", "beta", "class_agnostic")
    assert SWEEPABLE_MODES == ("assoc",)
    got = expand_grid({"match_iou": [0.2, 0.3], "assoc": ["greedy", "lsap"]}, base={"max_tracks": 8})
    assert [(c.assoc, c.match_iou) for c in got] == [("greedy", 0.2), ("greedy", 0.3), ("lsap", 0.2), ("lsap", 0.3)]
    assert [c.assoc for c in expand_grid({"max_age": [1, 2]}, base={"assoc": "lsap"})] == ["lsap", "lsap"]
    for bad, word in (({"assoc": ["lapjv"]}, "greedy"), ({"assoc": "lsap"}, "non-empty"), ({"assoc": []}, "non-empty"),
                      ({"max_tracks": [8, 16]}, "cannot be swept"), ({"cmc": [True]}, "cannot be swept")):
        with pytest.raises(ValueError, match=word):
            expand_grid(bad)


def test_predict_on_the_cpu_tracks_with_lsap(tmp_path):
    from PIL import Image

    from src.rtdetr_moe import engine

    src = tmp_path / "seq"
    src.mkdir()
    srcs = sorted(FRAMES.glob("*.jpg"))
    for f, i in enumerate([0, 0, 1, 1]):
        Image.open(srcs[i]).convert("RGB").resize((256, 128), Image.BILINEAR).save(src / f"{f:03d}.png")
    kw = dict(imgsz=IMGSZ, batch=2, device="cpu", conf=0.0, workers=0)
    runs = {}
    for assoc in ("greedy", "lsap"):
        torch.manual_seed(0)
        runs[assoc] = engine.predict(SPEC, src, track={**TRACKER, "assoc": assoc}, project=str(tmp_path), name=assoc,
                                     save_json=True, **kw)
    res = runs["lsap"]
    assert [p.frame for p in res.predictions] == [1, 2, 3, 4]
    assert sum(len(p.track_ids) for p in res.predictions) >= 3
    # a frame shown twice: every track finds its own box again under either rule
    assert [p.track_ids.tolist() for p in res.predictions[:2]] == [p.track_ids.tolist()
                                                                   for p in runs["greedy"].predictions[:2]]
    assert res.tracker["assoc"] == "lsap" and runs["greedy"].tracker["assoc"] == "greedy"
    json.dumps(res.tracker)
    assert (tmp_path / "lsap" / "tracks.json").is_file()


def test_sweep_on_the_cpu_returns_both_modes():
    from src.rtdetr_moe import tune

    c = case(65, 2)
    res = tune.sweep(c["dets"], c["gt"], {"assoc": ["greedy", "lsap"]}, base={"max_tracks": 64, "max_age": 3}, hota=True,
                     device="cpu")
    assert [cfg["assoc"] for cfg in res["configs"]] == ["greedy", "lsap"]
    assert len(res["metrics"]) == 2 and sorted(res["ranking"]) == [0, 1]
    one = tune.sweep(c["dets"], c["gt"], [dict(max_tracks=64, max_age=3, assoc="lsap")], hota=True)
    assert one["metrics"][0] == res["metrics"][1]
    json.dumps(res["configs"])  # what tracker_sweep.json holds


def test_the_c_abi_declares_both_entries():
    from scripts import predict_detector
    from src.moe import _lib as L

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "moe_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b((?:moe|rtdetr|train)_[a-z0-9_]+)\s*\(", text))
    assert {"rtdetr_track_update_assoc", "rtdetr_track_sweep_assoc"} <= declared and set(L.SIGNATURES) == declared
    assert len(L.SIGNATURES["rtdetr_track_update_assoc"][1]) == len(L.SIGNATURES["rtdetr_track_update_shift"][1]) + 1
    assert len(L.SIGNATURES["rtdetr_track_sweep_assoc"][1]) == len(L.SIGNATURES["rtdetr_track_sweep"][1]) + 1
    a = predict_detector.parse_args(["--weights", SPEC, "--source", "x", "--track", "--assoc", "lsap"])
    assert predict_detector.tracker_args(a) == {"assoc": "lsap"}
    a = predict_detector.parse_args(["--weights", SPEC, "--source", "x", "--track", "--tracker", '{"assoc": "lsap"}'])
    assert predict_detector.tracker_args(a) == {"assoc": "lsap"}
