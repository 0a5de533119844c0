"""rtdetr_hota_pass_a / _gas / _pass_b (_lib.hota_*) against hota.hota_reference:
every integer array, pot_q, gas (as int32), the [F][19] loc partials and loc_sum
(as int64) after the launches, exactly.  No tolerance: the shared arrays are
added with integer atomics, the sums follow the reference's order, and the one
solve is scipy's, ties included."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import hota_cases as hc
import mot_eval_cases as mc
from mot_eval_cases import A, B, C, frame

from src.rtdetr_moe import hota, moteval

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# name: (seed, F, NG, NT, shown truths, shown rows, ignore share, tie share), test_gpu_mot_eval.py's shapes: one row
# a side; 65 rows, one past a wave's stride, as the solver's columns, as both and as its rows' partners; empty
# sides; few truths against more tracker indices than two waves; identical boxes
SHAPES = {
    "one_by_one": (0, 12, 1, 1, (0, 1), (0, 1), 0.0, 0.3),
    "rows_65_truths_40": (1, 3, 40, 65, (40, 40), (65, 65), 0.1, 0.2),
    "rows_65_truths_65": (2, 3, 65, 65, (65, 65), (65, 65), 0.1, 0.2),
    "rows_40_truths_65": (3, 3, 65, 40, (65, 65), (40, 40), 0.1, 0.2),
    "mixed_with_empty_sides": (4, 40, 12, 15, (0, 12), (0, 15), 0.2, 0.2),
    "ng_3_nt_130": (5, 10, 3, 130, (0, 3), (0, 130), 0.2, 0.2),
    "identical_boxes": (6, 16, 8, 12, (4, 8), (6, 12), 0.1, 0.9),
}


def _upload(seqs, order, slots, M=None, K=None):
    """The frames ``order`` = [(sequence number, frame)] as one batch; padding rows hold garbage."""
    picks = [seqs[q][f] for q, f in order]
    M = M or max([1, *(len(p[1]) for p in picks)])
    K = K or max([1, *(len(p[4]) for p in picks)])
    F = len(picks)
    gb, tb = np.full((F, M, 4), np.nan, np.float32), np.full((F, K, 4), np.nan, np.float32)
    gi, gf, ti = np.full((F, M), -7, np.int32), np.full((F, M), 3, np.int32), np.full((F, K), 10 ** 6, np.int32)
    ng, nt = np.zeros(F, np.int32), np.zeros(F, np.int32)
    for i, (b, g, fl, tbx, t) in enumerate(picks):
        gb[i, :len(g)], gi[i, :len(g)], gf[i, :len(g)], ng[i] = b, g, fl, len(g)
        tb[i, :len(t)], ti[i, :len(t)], nt[i] = tbx, t, len(t)
    host = dict(gt_boxes=gb, gt_idx=gi, gt_flag=gf, n_gt=ng, trk_boxes=tb, trk_idx=ti, n_trk=nt,
                frame_slot=np.asarray(slots, np.int32))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in host.items()}


def _score(L, state, seqs, launches, slot_of=None, M=None, K=None):
    """Both passes over ``launches`` = lists of (sequence number, frame) -> {sequence number: exported state}."""
    slot_of = slot_of or list(range(len(seqs)))
    batches = []
    for order in launches:
        t = _upload(seqs, order, [slot_of[q] for q, _ in order], M, K)
        keep = torch.full(t["trk_idx"].shape, 77, dtype=torch.uint8, device=DEV)
        L.hota_pass_a(state, t, keep)
        batches.append((order, t, keep))
    L.hota_gas(state)
    parts = {q: np.zeros((len(s), 19)) for q, s in enumerate(seqs)}
    for order, t, keep in reversed(batches):  # pass B in another order of launches
        loc = L.hota_pass_b(state, t, keep).cpu().numpy()
        for i, (q, f) in enumerate(order):
            parts[q][f] = loc[i]
    L.hota_check(state)
    return {q: state.export(slot_of[q], parts[q]) for q in range(len(seqs))}


def _case(name):
    seed, F, NG, NT, m, k, ignore, tie = SHAPES[name]
    frames, ref = hc.drawn(seed, F, NG, NT, m, k, ignore, tie)
    return frames, NG, NT, ref


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernels_equal_reference(hip_lib, name):
    from src.moe import _lib as L

    frames, NG, NT, ref = _case(name)
    if name == "mixed_with_empty_sides":
        assert any(len(f[1]) == 0 for f in frames) and any(len(f[4]) == 0 for f in frames)
        assert ref["counts"][0, 0] > 0 and any((f[2] == 0).any() for f in frames)
    if name == "identical_boxes":
        assert ref["counts"][0, 18] > 0 and ref["loc_sum"][18] > 0
    st = hota.HotaEvalState(1, NG, NT, DEV)
    before = L.launch_counts().get("hota", 0)
    got = _score(L, st, [frames], [[(0, f) for f in range(len(frames))]])[0]
    assert L.launch_counts().get("hota", 0) - before == 3
    hc.assert_same(got, ref)


@pytest.mark.timeout(60)
def test_every_row_removed_by_ignore_regions(hip_lib):
    from src.moe import _lib as L

    frames = [frame([(0, A, 1)], [(0, A)]),
              frame([(1, A, 0), (2, B, 0), (0, C, 1)], [(0, A), (1, B)]),  # both rows removed, the truth missed
              frame([(1, A, 0), (2, B, 0)], [(2, B), (1, A)]),              # nothing left on either side
              frame([(0, A, 1)], [(0, A)])]
    ref = hota.hota_reference(frames, 3, 3)
    assert ref["counts"][:, 0].tolist() == [2, 1, 0] and ref["trk_count"].tolist() == [2, 0, 0]
    got = _score(L, hota.HotaEvalState(1, 3, 3, DEV), [frames], [[(0, f) for f in range(4)]])[0]
    hc.assert_same(got, ref)


@pytest.mark.timeout(60)
def test_200_workgroups_on_one_cell(hip_lib):
    """One truth and one track over 200 frames in one launch: every workgroup adds to the same pot_q and mc cell."""
    from src.moe import _lib as L

    frames = [frame([(0, A, 1)], [(0, A)])] * 200
    got = _score(L, hota.HotaEvalState(1, 1, 1, DEV), [frames], [[(0, f) for f in range(200)]])[0]
    assert got["pot_q"].tolist() == [[200 << 32]] and got["mc"].reshape(-1).tolist() == [200] * 19
    assert got["counts"].tolist() == [[200] * 19, [0] * 19, [0] * 19]
    assert got["gt_count"].tolist() == [200] and got["trk_count"].tolist() == [200]
    assert got["gas"].tolist() == [[1.0]] and got["loc_sum"].tolist() == [200.0] * 19
    hc.assert_same(got, hota.hota_reference(frames, 1, 1))


@pytest.mark.timeout(60)
def test_three_sequences_in_one_launch(hip_lib):
    """Lengths 1, 7 and 40, interleaved, the slots not in sequence order; a fourth slot without frames stays empty
    and a frame of a slot outside the state is skipped."""
    from src.moe import _lib as L

    frames, NG, NT, ref = _case("mixed_with_empty_sides")
    seqs = [frames[:1], frames[10:17], frames]
    refs = [hota.hota_reference(s, NG, NT) for s in seqs[:2]] + [ref]
    order = sorted([(q, f) for q in range(3) for f in range(len(seqs[q]))], key=lambda qf: (qf[1], -qf[0]))
    st = hota.HotaEvalState(4, NG, NT, DEV)
    got = _score(L, st, seqs, [order], slot_of=[2, 0, 3])
    for q in range(3):
        hc.assert_same(got[q], refs[q])
    empty = st.export(1, np.zeros((0, 19)))
    assert not empty["pot_q"].any() and not empty["mc"].any() and not empty["counts"].any()
    t = _upload([frames], [(0, 5)], [9])
    keep = torch.zeros(t["trk_idx"].shape, dtype=torch.uint8, device=DEV)
    L.hota_pass_a(st, t, keep)
    assert L.hota_pass_b(st, t, keep).cpu().numpy().tolist() == [[0.0] * 19]
    L.hota_check(st)
    hc.assert_same(st.export(3, got[2]["loc_part"]), ref)


@pytest.mark.timeout(60)
def test_launches_of_1_16_23_equal_one_launch(hip_lib):
    from src.moe import _lib as L

    frames, NG, NT, ref = _case("mixed_with_empty_sides")
    before = L.launch_counts().get("hota", 0)
    got = _score(L, hota.HotaEvalState(1, NG, NT, DEV), [frames],
                 [[(0, f) for f in range(lo, hi)] for lo, hi in ((0, 1), (1, 17), (17, 40))])[0]
    assert L.launch_counts().get("hota", 0) - before == 7
    hc.assert_same(got, ref)


@pytest.mark.timeout(60)
def test_iou_equal_to_the_threshold(hip_lib):
    """IoU exactly 0.5 against the table's 0.5 - eps: counted at ten thresholds."""
    from src.moe import _lib as L

    frames = [frame([(0, (0, 0, 1, 1), 1)], [(0, (0, 0, 2, 1))])]
    ref = hota.hota_reference(frames, 1, 1)
    assert ref["counts"][0].tolist() == [1] * 10 + [0] * 9
    got = _score(L, hota.HotaEvalState(1, 1, 1, DEV), [frames], [[(0, 0)]])[0]
    hc.assert_same(got, ref)


@pytest.mark.timeout(120)
def test_at_the_lds_limits(hip_lib):
    """K = 1024 rows and M = 256 truths, 2 frames."""
    from src.moe import _lib as L

    frames = mc.draw_frames(11, 2, 256, 1024, (256, 256), (1024, 1024), ignore=0.1, tie=0.2)
    ref = hota.hota_reference(frames, 256, 1024)
    assert ref["counts"][0, 0] > 100 and ref["trk_count"].sum() < 2048
    got = _score(L, hota.HotaEvalState(1, 256, 1024, DEV), [frames], [[(0, 0), (0, 1)]])[0]
    hc.assert_same(got, ref)


@pytest.mark.timeout(60)
def test_evaluate_on_the_device_equals_the_host(hip_lib, monkeypatch):
    from src.moe import _lib as L

    gt, res = {}, {}
    for key, n, seed in (("a", 30, 21), ("b", 7, 22), ("c", 1, 23)):
        g, r = hc.mot_files(mc.draw_frames(seed, n, 9, 11, (0, 9), (0, 11), ignore=0.2, tie=0.2))
        gt[key], res[key] = moteval.parse_gt(g, ignore_classes=[8]), r
    L.launch_counts(reset=True)
    plain = moteval.evaluate(gt, res, device=DEV)
    assert L.launch_counts(reset=True) == {"mot_eval": 1}
    on_dev = moteval.evaluate(gt, res, device=DEV, hota=True)
    assert L.launch_counts(reset=True) == {"mot_eval": 1, "hota": 3}  # 38 frames: one chunk a pass, and gas
    monkeypatch.setenv("MOE_TRACK_EVAL", "0")
    assert on_dev == moteval.evaluate(gt, res, device=DEV, hota=True) == moteval.evaluate(gt, res, hota=True)
    assert not L.launch_counts(reset=True)
    assert {k: {x: v for x, v in m.items() if x != "HOTA"} for k, m in on_dev.items()} == plain
    assert on_dev["COMBINED"]["HOTA"]["arrays"]["TP"][0] > 50 and 0 < on_dev["COMBINED"]["HOTA"]["HOTA"] < 1
    # the states themselves
    seqs = [moteval.dense_sequence(gt[k], moteval.parse_mot(res[k])) for k in gt]
    for a, b in zip(hota.run_device_hota(seqs, 0.5, DEV), hota.run_reference_hota(seqs, 0.5)):
        hc.assert_same(a, b)


@pytest.mark.timeout(60)
def test_sequence_over_the_table_budget_goes_to_the_host(hip_lib, monkeypatch):
    from src.moe import _lib as L

    frames = mc.draw_frames(9, 6, 5, 7, (0, 5), (0, 7), ignore=0.2, tie=0.2)
    seqs = [{"NG": 5, "NT": 7, "frames": frames}] * 2
    want = hota.run_reference_hota(seqs, 0.5)
    monkeypatch.setattr(hota, "HOTA_MAX_CELLS", 34)  # one 5 x 7 table is over it
    L.launch_counts(reset=True)
    with pytest.warns(UserWarning, match="scored on the host"):
        got = hota.run_device_hota(seqs, 0.5, DEV)
    assert not L.launch_counts(reset=True)
    for a, b in zip(got, want):
        hc.assert_same(a, b)
    monkeypatch.setattr(hota, "HOTA_MAX_CELLS", 35)  # one table fits, two do not: two groups on the device
    for a, b in zip(hota.run_device_hota(seqs, 0.5, DEV), want):
        hc.assert_same(a, b)
    assert L.launch_counts(reset=True) == {"hota": 6}


@pytest.mark.timeout(60)
def test_refusals_launch_nothing(hip_lib):
    import ctypes

    from src.moe import _lib as L

    st = hota.HotaEvalState(1, 2, 2, DEV)

    def batch(F, M, K):
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)  # noqa: E731
        t = dict(gt_boxes=torch.zeros((F, M, 4), device=DEV), gt_idx=z(F, M), gt_flag=z(F, M), n_gt=z(F),
                 trk_boxes=torch.zeros((F, K, 4), device=DEV), trk_idx=z(F, K), n_trk=z(F), frame_slot=z(F))
        return t, torch.zeros((F, K), dtype=torch.uint8, device=DEV)

    L.launch_counts(reset=True)
    for F, M, K, match in ((1, 4, 1025, "K <= 1024"), (1, 257, 4, "M <= 256")):
        with pytest.raises(L.MoEKernelError, match=match):
            L.hota_pass_a(st, *batch(F, M, K))
        with pytest.raises(L.MoEKernelError, match=match):
            L.hota_pass_b(st, *batch(F, M, K))
    with pytest.raises(L.MoEKernelError, match="thr"):
        L.hota_pass_a(st, *batch(1, 1, 1), thr=float("nan"))
    L.hota_pass_a(st, *batch(0, 4, 4))  # F == 0: fine, and no launch
    assert tuple(L.hota_pass_b(st, *batch(0, 4, 4)).shape) == (0, 19)
    # a table over the budget: the state refuses it, and so does the library whatever the pointers are
    with pytest.raises(ValueError, match="S \\* NG \\* NT"):
        hota.HotaEvalState(1, 1024, 2049, DEV)
    t, keep = batch(1, 1, 1)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    ins = [p(t[k]) for k in L._HOTA_INPUTS]
    lib = L.lib()
    assert lib.rtdetr_hota_pass_a(*ins, 1, 1, 1, 1, 1024, 2049, 0.5, p(st.pot_q), p(st.gt_count), p(st.trk_count),
                                  p(keep), p(st.status), None) != 0
    assert b"budget" in lib.moe_last_error()
    assert lib.rtdetr_hota_gas(p(st.pot_q), p(st.gt_count), p(st.trk_count), 2, 1024, 1025, p(st.gas), None) != 0
    loc = torch.zeros((1, 19), dtype=torch.float64, device=DEV)
    assert lib.rtdetr_hota_pass_b(*ins, p(keep), 1, 1, 1, 1, 1024, 2049, p(st.gas), p(st.alpha), p(st.counts),
                                  p(st.mc), p(loc), p(st.status), None) != 0
    assert not L.launch_counts(reset=True)
    L.hota_check(st)
    assert not st.pot_q.any() and not st.mc.any() and not st.counts.any()
    # an index outside the state fails the call and leaves the frame out of both passes
    fr = frame([(2, A, 1)], [(0, A)])
    with pytest.raises(L.MoEKernelError, match="status 4"):
        _score(L, st, [[fr]], [[(0, 0)]])
    assert not st.pot_q.any() and not st.mc.any() and not st.counts.any() and not st.gt_count.any()
