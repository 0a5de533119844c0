"""The tracking evaluator's rule on the CPU (moteval.mot_reference, mot_metrics,
load_gt, evaluate): hand cases with counted answers, exhaustive checks of both
assignments on small problems, independence from chunking, MOTChallenge file
handling, and consistency with tests/track_cases.py's identities()."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import mot_eval_cases as mc
from mot_eval_cases import A, B, C, frame, shifted

from src.rtdetr_moe import moteval

D = (700.0, 50.0, 740.0, 150.0)


def test_perfect_tracking():
    frames = [frame([(0, A, 1), (1, B, 1)], [(0, A), (1, B)]) for _ in range(5)]
    m = mc.metrics_of(frames, 2, 2)
    assert (m["TP"], m["FN"], m["FP"], m["IDSW"], m["Frag"], m["frames"]) == (10, 0, 0, 0, 0, 5)
    assert m["MOTA"] == 1.0 and m["IDF1"] == 1.0 and m["MOTP"] == 1.0 and m["MT"] == 2 and m["GT"] == 2


def test_ids_swap_half_way():
    frames = [frame([(0, A, 1), (1, B, 1)], [(0, A), (1, B)] if f < 5 else [(0, B), (1, A)]) for f in range(10)]
    m = mc.metrics_of(frames, 2, 2)
    assert (m["TP"], m["FN"], m["FP"], m["IDSW"]) == (20, 0, 0, 2)
    assert m["MOTA"] == 0.9
    assert (m["IDTP"], m["IDFN"], m["IDFP"]) == (10, 10, 10) and m["IDF1"] == 0.5


def test_continuity_keeps_the_previous_pair():
    near, nearer = shifted(A, 11.6), shifted(A, 2.0)  # IoU 0.55 and 0.905 with A
    frames = [frame([(0, A, 1)], [(0, near)]), frame([(0, A, 1)], [(1, nearer), (0, near)])]
    st = moteval.new_state(1, 2)
    assert moteval.mot_reference(st, frames[0][:3], frames[0][3:]) == [(0, 0)]
    assert moteval.mot_reference(st, frames[1][:3], frames[1][3:]) == [(0, 0)]
    m = moteval.mot_metrics(st)
    assert (m["TP"], m["FP"], m["IDSW"]) == (2, 1, 0)
    # a fresh state has nothing to keep: the better candidate wins
    assert moteval.mot_reference(moteval.new_state(1, 2), frames[1][:3], frames[1][3:]) == [(0, 1)]


def test_gap_then_the_same_id():
    frames = [frame([(0, A, 1)], [] if f in (2, 3) else [(0, A)]) for f in range(6)]
    m = mc.metrics_of(frames, 1, 1)
    assert (m["TP"], m["FN"], m["IDSW"], m["Frag"]) == (4, 2, 0, 1)


def test_gap_then_a_new_id():
    frames = [frame([(0, A, 1)], [] if f in (2, 3) else [(0 if f < 2 else 1, A)]) for f in range(6)]
    m = mc.metrics_of(frames, 1, 2)
    assert (m["TP"], m["FN"], m["IDSW"], m["Frag"]) == (4, 2, 1, 1)


def test_frag_looks_at_the_previous_present_frame():
    # the truth itself is absent in frames 2 and 3: matched before, matched after -- no fragmentation
    frames = [frame([] if f in (2, 3) else [(0, A, 1)], [(0, A)]) for f in range(6)]
    m = mc.metrics_of(frames, 1, 1)
    assert (m["TP"], m["FN"], m["FP"], m["Frag"], m["IDSW"]) == (4, 0, 2, 0, 0)


def test_mt_pt_ml_thresholds():
    boxes, n_matched = (A, B, C, D), (9, 8, 2, 1)  # of 10 frames: above 0.8, exactly 0.8, exactly 0.2, below 0.2
    frames = [frame([(g, boxes[g], 1) for g in range(4)], [(g, boxes[g]) for g in range(4) if f < n_matched[g]])
              for f in range(10)]
    m = mc.metrics_of(frames, 4, 4)
    assert (m["GT"], m["MT"], m["PT"], m["ML"]) == (4, 1, 2, 1)


def test_ignore_region_removes_the_row():
    frames = [frame([(0, A, 1), (1, B, 0)], [(0, A), (1, B)])]
    m = mc.metrics_of(frames, 2, 2)
    assert (m["TP"], m["FP"], m["FN"], m["removed"]) == (1, 0, 0, 1)
    assert (m["IDFP"], m["IDFN"], m["IDTP"]) == (0, 0, 1)
    # the same row on a scored truth that another row already holds is a false positive
    m = mc.metrics_of([frame([(0, A, 1)], [(0, A), (1, B)])], 1, 2)
    assert (m["TP"], m["FP"], m["removed"]) == (1, 1, 0)


def test_conf_zero_row_is_dropped():
    gt = moteval.parse_gt(mc.mot_text([(1, 1, *A, 1, 1, 1), (1, 2, *B, 0, 1, 1)]))
    assert list(gt[1][1]) == [1]
    out = moteval.evaluate({"s": gt}, {"s": mc.mot_text([(1, 1, *A, 0.9, -1, -1, -1), (1, 2, *B, 0.9, -1, -1, -1)])})
    assert (out["s"]["TP"], out["s"]["FP"], out["s"]["removed"]) == (1, 1, 0)


def test_empty_sides():
    frames = [frame([], [(0, A)]), frame([(0, A, 1)], []), frame([], [])]
    m = mc.metrics_of(frames, 1, 1)
    assert (m["TP"], m["FP"], m["FN"], m["frames"]) == (0, 1, 1, 3)
    assert m["MOTA"] == -1.0 and m["MOTP"] == 0.0


def test_more_truths_than_rows_and_more_rows_than_truths():
    m = mc.metrics_of([frame([(0, A, 1), (1, B, 1), (2, C, 1)], [(0, B)])], 3, 1)
    assert (m["TP"], m["FN"], m["FP"]) == (1, 2, 0)
    m = mc.metrics_of([frame([(0, B, 1)], [(0, A), (1, B), (2, C)])], 1, 3)
    assert (m["TP"], m["FN"], m["FP"]) == (1, 0, 2)


def test_empty_denominators_give_zero():
    m = moteval.mot_metrics(moteval.new_state(1, 1))
    for k in ("MOTA", "MOTP", "Recall", "Precision", "IDF1", "IDP", "IDR"):
        assert m[k] == 0.0
    assert moteval.combine([])["MOTA"] == 0.0 and moteval.combine([])["IDF1"] == 0.0
    assert moteval.evaluate({}, {}) == {"COMBINED": moteval.combine([])}


def test_combined_row_sums_the_counts():
    a = mc.metrics_of([frame([(0, A, 1)], [(0, A)])] * 3, 1, 1)
    b = mc.metrics_of([frame([(0, A, 1)], [(0, B)])], 1, 1)
    c = moteval.combine([a, b])
    assert (c["TP"], c["FN"], c["FP"], c["frames"], c["GT"]) == (3, 1, 1, 4, 2)
    assert c["MOTA"] == (3 - 1) / 4 and c["IDF1"] == 6 / 8 and c["MOTP"] == 1.0


def test_bad_input_raises_before_anything_runs():
    st = moteval.new_state(2, 2)
    before = moteval.copy_state(st)
    with pytest.raises(ValueError, match="twice"):
        moteval.mot_reference(st, *_split(frame([(0, A, 1), (0, B, 1)], [(0, A)])))
    with pytest.raises(ValueError, match="twice"):
        moteval.mot_reference(st, *_split(frame([(0, A, 1)], [(1, A), (1, B)])))
    with pytest.raises(ValueError, match="outside"):
        moteval.mot_reference(st, *_split(frame([(2, A, 1)], [])))
    with pytest.raises(ValueError, match="IoU"):
        moteval.mot_reference(st, *_split(frame([(0, A, 1)], [])), thr=0.0)
    assert moteval.states_equal(st, before)


def _split(fr):
    return fr[:3], fr[3:]


@pytest.mark.parametrize("seed", range(6))
def test_frame_matching_maximises_the_total_score(seed):
    """Every one-to-one assignment of a frame of at most 5 x 5 rows is enumerated."""
    rng = np.random.default_rng(seed)
    for fr in mc.draw_frames(seed, 40, 5, 5, (0, 5), (0, 5), tie=0.3, jitter=8.0):
        gb, gi, gf, tb, ti = fr
        st = moteval.new_state(5, 5)
        st["prev_step"][:] = rng.integers(-1, 5, 5)
        score = moteval.frame_scores(st["prev_step"], gi.astype(np.int64), ti.astype(np.int64),
                                     moteval._iou(tb, gb), 0.5).astype(np.float64)
        pairs = moteval.mot_reference(st, (gb, gi, gf), (tb, ti))
        got = sum(score[list(ti).index(t), list(gi).index(g)] for g, t in pairs)
        nt, ng = score.shape
        best = 0.0
        if nt and ng:
            small, large = (range(ng), range(nt)) if ng <= nt else (range(nt), range(ng))
            for perm in itertools.permutations(large, len(small)):
                best = max(best, sum(score[p, s] if ng <= nt else score[s, p] for s, p in zip(small, perm)))
        assert got == best
        assert len({g for g, _ in pairs}) == len(pairs) == len({t for _, t in pairs})


@pytest.mark.parametrize("seed", range(4))
def test_idtp_is_the_maximum_over_all_permutations(seed):
    rng = np.random.default_rng(100 + seed)
    NG, NT = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    st = mc.run_reference(mc.draw_frames(seed, 30, NG, NT, (0, NG), (0, NT), drift=0.4, tie=0.2), NG, NT)
    pmc = np.zeros((6, 6), np.int64)
    pmc[:NG, :NT] = st["pmc"]
    best = max(sum(pmc[g, p[g]] for g in range(6)) for p in itertools.permutations(range(6)))
    m = moteval.mot_metrics(st)
    assert m["IDTP"] == best and best > 0
    assert m["IDFN"] == int(st["gt_count"].sum()) - best and m["IDFP"] == int(st["trk_count"].sum()) - best


def test_chunking_changes_nothing():
    frames = mc.draw_frames(7, 40, 6, 9, (0, 6), (0, 9), ignore=0.2, tie=0.2)
    whole = mc.run_reference(frames, 6, 9)
    parts = mc.run_reference(frames, 6, 9, chunks=[range(0, 1), range(1, 17), range(17, 40)])
    assert moteval.states_equal(whole, parts)
    assert whole["counts"][5] == 40 and whole["counts"][4] > 0 and whole["counts"][3] > 0


def _gt_rows():
    return [(1, 7, *A, 1, 1, 1.0), (1, 9, *B, 1, 8, 0.5), (2, 7, *shifted(A, 1.5), 1, 1, 1.0), (4, 3, *C, 1, 2, 1.0),
            (4, 5, *D, 0, 1, 1.0)]


def test_load_gt_round_trips_both_layouts(tmp_path):
    text = mc.mot_text(_gt_rows())
    (tmp_path / "a" / "gt").mkdir(parents=True)
    (tmp_path / "a" / "gt" / "gt.txt").write_text(text)
    (tmp_path / "b.txt").write_text(text)
    gt = moteval.load_gt(tmp_path, ["a", "b"], classes=[1, 2], ignore_classes=[8])
    for key in ("a", "b"):
        fr = gt[key]
        assert sorted(fr) == [1, 2, 4]  # frame 3 has no lines; the conf == 0 row of frame 4 is dropped
        assert fr[1][1].tolist() == [7, 9] and fr[1][2].tolist() == [1, 0]
        assert fr[4][1].tolist() == [3]
        assert np.array_equal(fr[1][0], np.asarray([A, B], np.float32))
        assert fr[2][0].dtype == np.float32 and fr[2][0][0, 0] == np.float32(101.5)
    # class 8 neither scored nor ignored
    assert moteval.load_gt(tmp_path, ["b"], classes=[1])["b"][1][1].tolist() == [7]
    # missing trailing columns are 1,1,1
    (tmp_path / "c.txt").write_text("1,4,10,20,30,40\n")
    assert moteval.load_gt(tmp_path, ["c"], classes=[1])["c"][1][2].tolist() == [1]
    with pytest.raises(FileNotFoundError) as e:
        moteval.load_gt(tmp_path, ["zz"])
    assert str(tmp_path / "zz" / "gt" / "gt.txt") in str(e.value) and str(tmp_path / "zz.txt") in str(e.value)


def test_duplicate_id_in_a_frame_raises(tmp_path):
    (tmp_path / "d.txt").write_text(mc.mot_text([(1, 7, *A), (1, 7, *B)]))
    with pytest.raises(ValueError, match="twice"):
        moteval.load_gt(tmp_path, ["d"])
    with pytest.raises(ValueError, match="twice"):
        moteval.parse_mot(mc.mot_text([(2, 1, *A, 0.9, -1, -1, -1), (2, 1, *B, 0.9, -1, -1, -1)]))


def test_evaluate_on_text_and_on_files_agrees(tmp_path):
    gt = {"a": moteval.parse_gt(mc.mot_text(_gt_rows()), ignore_classes=[8]),
          "b": moteval.parse_gt(mc.mot_text(_gt_rows()[:3]))}
    res = {"a": mc.mot_text([(1, 1, *A, 0.9, -1, -1, -1), (1, 2, *B, 0.8, -1, -1, -1), (2, 2, *A, 0.9, -1, -1, -1),
                             (5, 1, *C, 0.7, -1, -1, -1)]),
           "b": ""}
    for key, text in res.items():
        (tmp_path / (key + ".txt")).write_text(text)
    out = moteval.evaluate(gt, res)
    assert out == moteval.evaluate(gt, tmp_path) == moteval.evaluate(gt, str(tmp_path), device="cpu")
    assert list(out) == ["a", "b", "COMBINED"]
    a = out["a"]
    assert (a["frames"], a["TP"], a["FN"], a["FP"], a["IDSW"], a["removed"]) == (5, 2, 1, 1, 1, 1)
    assert (out["b"]["frames"], out["b"]["FN"]) == (2, 3)
    assert out["COMBINED"]["FN"] == 4 and out["COMBINED"]["frames"] == 7
    with pytest.raises(ValueError, match="no results"):
        moteval.evaluate(gt, {"a": ""})


@pytest.mark.parametrize("jumps", [{}, {1: 12, 4: 20}])
def test_idsw_equals_identities_switches(jumps):
    """No false positives, no misses, objects apart: every reported row is
    matched to its own object, so the evaluator's IDSW is identities()' count."""
    import track_cases as tc

    seq, truth = mc.draw_tracked(6, 30, seed=3, jumps=jumps)
    res = tc.run_reference(seq, dict(min_hits=1), T=16)
    _, switches = tc.identities(seq, res["out_id"])
    NT = int(res["out_id"].max())
    st = moteval.new_state(6, NT)
    for f in range(30):
        rows = np.nonzero(res["out_id"][f] >= 0)[0]
        trk = (res["out_box"][f][rows], res["out_id"][f][rows] - 1)
        pairs = moteval.mot_reference(st, (truth[f], np.arange(6), np.ones(6, np.int32)), trk)
        want = sorted((int(seq["truth"][f, d]), int(res["out_id"][f, d]) - 1) for d in rows)
        assert sorted(pairs) == want
    m = moteval.mot_metrics(st)
    assert m["IDSW"] == switches == len(jumps)
    assert m["FP"] == 0 and m["FN"] == 0
