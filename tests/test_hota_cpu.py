"""HOTA's rule on the CPU (hota.py: hota_reference, hota_metrics, combine_hota,
moteval.evaluate(..., hota=True)): hand cases with counted answers, the rule
against a plain fp64 transcription of the published algorithm
(hota_cases.transcription), the order-freedom the GPU path rests on, and the
default path left as it was."""
from __future__ import annotations

import json

import numpy as np
import pytest

import hota_cases as hc
import mot_eval_cases as mc
from mot_eval_cases import A, B, C, frame, shifted

from src.rtdetr_moe import hota, moteval

MEANS = hota.HOTA_FIELDS


def _metrics(frames, NG, NT, **kw):
    return hota.hota_metrics(hota.hota_reference(frames, NG, NT, **kw))


def test_alpha_table():
    assert hota.ALPHA.dtype == np.float64 and len(hota.ALPHA) == 19
    assert np.array_equal(hota.ALPHA, np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps)


def test_perfect_tracking_is_one_everywhere():
    frames = [frame([(0, A, 1), (1, B, 1)], [(1, B), (0, A)]) for _ in range(6)]
    m = _metrics(frames, 2, 2)
    for k in MEANS:
        assert m[k] == 1.0, k
        assert m["arrays"][k] == [1.0] * 19, k
    assert m["HOTA(0)"] == m["LocA(0)"] == m["HOTALocA(0)"] == 1.0
    assert m["arrays"]["TP"] == [12] * 19 and m["arrays"]["FN"] == m["arrays"]["FP"] == [0] * 19
    json.dumps(m)


def test_identity_switch_halves_the_association():
    frames = [frame([(0, A, 1)], [(0 if f < 5 else 1, A)]) for f in range(10)]
    st = hota.hota_reference(frames, 1, 2)
    assert st["counts"].tolist() == [[10] * 19, [0] * 19, [0] * 19]
    assert st["mc"][:, 0].tolist() == [[5, 5]] * 19
    assert st["pot_q"].tolist() == [[5 << 32, 5 << 32]]
    m = hota.hota_metrics(st)
    assert m["DetA"] == 1.0 and m["AssA"] == 0.5 and m["HOTA"] == pytest.approx(np.sqrt(0.5), abs=1e-15)
    assert m["AssRe"] == 0.5 and m["AssPr"] == 1.0 and m["LocA"] == 1.0


def test_one_pair_at_iou_two_thirds():
    frames = [frame([(0, A, 1)], [(0, shifted(A, 8))])] * 3  # 32 / 48
    st = hota.hota_reference(frames, 1, 1)
    assert st["counts"][0].tolist() == [3] * 13 + [0] * 6
    assert st["counts"][1].tolist() == st["counts"][2].tolist() == [0] * 13 + [3] * 6
    m = hota.hota_metrics(st)
    for k in ("HOTA", "DetA", "AssA"):
        assert m[k] == pytest.approx(13 / 19, abs=1e-15), k
    iou = float(moteval._iou(np.asarray([shifted(A, 8)], np.float32), np.asarray([A], np.float32))[0, 0])
    assert m["arrays"]["LocA"] == pytest.approx([iou] * 13 + [1.0] * 6, abs=1e-15)
    assert m["arrays"]["loc_sum"][:13] == [iou + iou + iou] * 13


def test_threshold_equal_to_the_iou_counts():
    # IoU exactly 0.5 against ALPHA[9] = 0.5 - eps: counted at the ten thresholds up to 0.5
    st = hota.hota_reference([frame([(0, (0, 0, 1, 1), 1)], [(0, (0, 0, 2, 1))])], 1, 1)
    assert st["counts"][0].tolist() == [1] * 10 + [0] * 9


def test_row_on_an_ignore_region_is_no_false_positive():
    frames = [frame([(0, A, 1), (1, B, 0)], [(0, A), (1, B), (2, C)])] * 2
    st = hota.hota_reference(frames, 2, 3)
    assert st["trk_count"].tolist() == [2, 0, 2] and st["gt_count"].tolist() == [2, 0]
    assert st["counts"].tolist() == [[2] * 19, [0] * 19, [2] * 19]  # only the row on C is a false positive
    assert st["pot_q"][1].tolist() == [0, 0, 0] and st["mc"][:, :, 1].sum() == 0


def test_empty_sides_and_empty_sequences():
    m = hota.hota_metrics(hota.new_hota_state(1, 1))
    assert all(m[k] == 0.0 for k in MEANS if k != "LocA") and m["LocA"] == 1.0  # TrackEval's LocA without a pair
    m = hota.hota_metrics(hota.new_hota_state(0, 0))
    assert m["HOTA"] == 0.0 and m["arrays"]["TP"] == [0] * 19
    no_rows = _metrics([frame([(0, A, 1)], [])] * 2, 1, 1)
    assert no_rows["arrays"]["FN"] == [2] * 19 and no_rows["HOTA"] == no_rows["DetRe"] == 0.0
    no_truth = _metrics([frame([], [(0, A)])] * 2, 1, 1)
    assert no_truth["arrays"]["FP"] == [2] * 19 and no_truth["HOTA"] == no_truth["DetPr"] == 0.0
    assert hota.combine_hota([])["HOTA"] == 0.0
    out = moteval.evaluate({}, {}, hota=True)
    assert out == {"COMBINED": {**moteval.combine([]), "HOTA": hota.combine_hota([])}}
    gt = {"s": moteval.parse_gt("")}
    assert moteval.evaluate(gt, {"s": ""}, hota=True)["s"]["HOTA"]["HOTA"] == 0.0


def test_combined_row_by_hand():
    # a: the identity switch (TP 10, AssA 0.5); b: 3 perfect frames and 1 miss (TP 3, FN 1)
    # b's AssA = 3 * 3 / (4 + 3 - 3) / 3
    a = _metrics([frame([(0, A, 1)], [(0 if f < 5 else 1, A)]) for f in range(10)], 1, 2)
    b = _metrics([frame([(0, A, 1)], [(0, A)])] * 3 + [frame([(0, A, 1)], [])], 1, 1)
    assert b["DetA"] == 0.75 and b["AssA"] == 0.75
    c = hota.combine_hota([a, b])
    assert c["arrays"]["TP"] == [13] * 19 and c["arrays"]["FN"] == [1] * 19 and c["arrays"]["FP"] == [0] * 19
    assert c["DetA"] == pytest.approx(13 / 14, abs=1e-15)
    assert c["AssA"] == pytest.approx((0.5 * 10 + 0.75 * 3) / 13, abs=1e-15)
    assert c["HOTA"] == pytest.approx(np.sqrt(13 / 14 * 7.25 / 13), abs=1e-15)
    assert c["LocA"] == 1.0 and c["arrays"]["loc_sum"] == [13.0] * 19
    # evaluate combines in sorted key order whatever order gt has
    ga, ra = hc.mot_files(hc.drawn(3, 20, 6, 9, (0, 6), (0, 9), 0.2, 0.3)[0])
    gb, rb = hc.mot_files(hc.drawn(4, 20, 6, 9, (0, 6), (0, 9), 0.2, 0.3)[0])
    gt = {"b": moteval.parse_gt(gb, ignore_classes=[8]), "a": moteval.parse_gt(ga, ignore_classes=[8])}
    out = moteval.evaluate(gt, {"a": ra, "b": rb}, hota=True)
    assert out["COMBINED"]["HOTA"] == hota.combine_hota([out["a"]["HOTA"], out["b"]["HOTA"]])
    assert out["COMBINED"]["HOTA"]["arrays"]["TP"][0] > 20


@pytest.mark.parametrize("shape", range(len(hc.TRANSCRIPTION_SHAPES)))
def test_rule_equals_the_transcription(shape):
    """TP / FN / FP per threshold and the whole mc table, exactly, seeds 0..39; HOTA to 1e-12."""
    F, NG, NT, m, k, ignore, tie = hc.TRANSCRIPTION_SHAPES[shape]
    for seed in range(40):
        frames = mc.draw_frames(seed, F, NG, NT, m, k, ignore=ignore, tie=tie)
        st = hota.hota_reference(frames, NG, NT)
        want = hc.transcription(frames, NG, NT)
        for i, key in enumerate(("TP", "FN", "FP")):
            assert st["counts"][i].tolist() == want[key].tolist(), (seed, key)
        assert np.array_equal(st["mc"].astype(np.int64), want["mc"]), seed
        got = hota.hota_metrics(st)
        for key in ("HOTA", "DetA", "AssA", "LocA"):
            assert abs(got[key] - want[key]) <= 1e-12, (seed, key, got[key], want[key])
        assert want["TP"][0] > 0


def test_frames_in_any_order_and_in_chunks():
    frames, ref = hc.drawn(7, 30, 12, 16, (4, 12), (4, 16), 0.1, 0.2)
    assert ref["counts"][0, 0] > 50 and ref["loc_sum"][0] > 0
    n = len(frames)
    rng = np.random.default_rng(0)
    for order, order_b in ((range(n - 1, -1, -1), None), (rng.permutation(n), rng.permutation(n)),
                           ([*range(17, n), *range(1, 17), 0], [*range(1), *range(17, n), *range(1, 17)])):
        hc.assert_same(hota.hota_reference(frames, 12, 16, order=order, order_b=order_b), ref)
    # chunks through the frame-level functions, the partials put back in frame order
    st = hota.new_hota_state(12, 16)
    chunks = ([29, 3, 4], list(range(5, 29)), [0, 1, 2])
    for chunk in chunks:
        for f in chunk:
            hota.hota_pass_a(st, frames[f][:3], frames[f][3:])
    gas = hota.hota_gas(st)
    parts = np.zeros((n, 19))
    for chunk in reversed(chunks):
        for f in chunk:
            parts[f] = hota.hota_pass_b(st, gas, frames[f][:3], frames[f][3:])
    st["loc_sum"], st["gas"], st["loc_part"] = hota.reduce_loc(parts), gas, parts
    hc.assert_same(st, ref)
    assert hota.hota_states_equal(st, ref)


def test_sums_are_sequential_not_pairwise():
    """65 rows against 40 truths of random overlap: numpy's pairwise sum differs from the rule's order somewhere, and
    the reference follows the rule (an explicit loop)."""
    frames, ref = hc.drawn(1, 3, 40, 65, (40, 40), (65, 65), 0.0, 0.0)
    g, t, iou, _ = hota.frame_rows(frames[0][:3], frames[0][3:], 40, 65, 0.5)
    sim = iou.astype(np.float64)
    seq = np.zeros(len(t))
    for j in range(len(g)):
        seq = seq + sim[:, j]
    st = hota.new_hota_state(40, 65)
    hota.hota_pass_a(st, frames[0][:3], frames[0][3:])
    col = np.cumsum(sim, axis=0)[-1]
    den = (seq[:, None] + col[None, :]) - sim
    want = np.rint(np.where(den > np.finfo(float).eps, sim / den, 0.0) * 2.0 ** 32).astype(np.int64)
    assert np.array_equal(st["pot_q"][g[None, :], t[:, None]], want)


def test_without_hota_nothing_changes():
    frames = hc.drawn(5, 20, 6, 9, (0, 6), (0, 9), 0.2, 0.3)[0]
    g, r = hc.mot_files(frames)
    gt = {"s": moteval.parse_gt(g, ignore_classes=[8]), "t": moteval.parse_gt(g)}
    res = {"s": r, "t": r}
    plain = moteval.evaluate(gt, res)
    # the parent's evaluate, spelled out
    seqs = [moteval.dense_sequence(gt[k], moteval.parse_mot(res[k])) for k in gt]
    want = {k: moteval.mot_metrics(st) for k, st in zip(gt, moteval.run_reference(seqs, 0.5))}
    want["COMBINED"] = moteval.combine([want["s"], want["t"]])
    assert plain == want and all("HOTA" not in m for m in plain.values())
    assert plain == moteval.evaluate(gt, res, hota=False)
    with_hota = moteval.evaluate(gt, res, hota=True)
    assert list(with_hota) == list(plain)
    for k, m in with_hota.items():
        assert list(m)[-1] == "HOTA" and {x: v for x, v in m.items() if x != "HOTA"} == plain[k]
    assert with_hota["s"]["HOTA"] != with_hota["t"]["HOTA"]  # the ignore regions count
    json.dumps(with_hota)


def test_eval_tracks_hota_on_written_files(tmp_path, capsys):
    from scripts import eval_tracks

    frames = hc.drawn(5, 20, 6, 9, (0, 6), (0, 9), 0.2, 0.3)[0]
    g, r = hc.mot_files(frames)
    (tmp_path / "gt" / "seq" / "gt").mkdir(parents=True)
    (tmp_path / "gt" / "seq" / "gt" / "gt.txt").write_text(g)
    (tmp_path / "mot").mkdir()
    (tmp_path / "mot" / "seq.txt").write_text(r)
    in_run = moteval.evaluate({"seq": moteval.parse_gt(g, ignore_classes=[8])}, {"seq": r}, hota=True)
    args = ["--gt", str(tmp_path / "gt"), "--results", str(tmp_path / "mot"), "--gt-ignore-classes", "8",
            "--device", "cpu"]
    out = tmp_path / "m.json"
    again = eval_tracks.main([*args, "--hota", "--out", str(out)])
    assert again == in_run == json.loads(out.read_text())
    assert " HOTA " in capsys.readouterr().out
    plain = eval_tracks.main(args)
    assert "HOTA" not in plain["seq"] and " HOTA " not in capsys.readouterr().out
    assert plain == moteval.evaluate({"seq": moteval.parse_gt(g, ignore_classes=[8])}, {"seq": r})


def test_groups_stay_under_the_table_budget():
    seqs = [{"NG": 1024, "NT": 1024}, {"NG": 10, "NT": 10}, {"NG": 1024, "NT": 4096}, {"NG": 3, "NT": 3}]
    groups = hota.hota_groups(seqs)
    assert groups == [(0, 2), (2, 3), (3, 4)]
    assert hota.hota_groups([]) == [] and hota.hota_groups([{"NG": 0, "NT": 0}] * 3) == [(0, 3)]
    assert len(hota.hota_groups([{"NG": 1, "NT": 1}] * 1025)) == 2
