"""rtdetr_mot_eval (_lib.mot_eval) against moteval.mot_reference: every state
array, every count, the pmc table and the fp64 sum (as bits) after the launch,
exactly.  No tolerance: the kernel restates the reference's fp32 IoU operation
by operation, solves both assignments as scipy does, ties included, and adds
the sum in the reference's order."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import mot_eval_cases as mc
from mot_eval_cases import A, B, C, frame, shifted

from src.rtdetr_moe import moteval

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# name: (NG, NT, F, shown truths (lo, hi), shown rows (lo, hi), ignore share, tie share, seed).  The smallest
# shapes at which each mechanism can go wrong: one row a side; 65 rows, one past a wave's stride, as the solver's
# columns (rows > truths), as both (equal) and as its rows' partners (truths > rows); empty sides; few truths
# against more tracker indices than two waves; identical boxes.
SHAPES = {
    "one_by_one": (1, 1, 12, (0, 1), (0, 1), 0.0, 0.3, 0),
    "rows_65_truths_40": (40, 65, 3, (40, 40), (65, 65), 0.1, 0.2, 1),
    "rows_65_truths_65": (65, 65, 3, (65, 65), (65, 65), 0.1, 0.2, 2),
    "rows_40_truths_65": (65, 40, 3, (65, 65), (40, 40), 0.1, 0.2, 3),
    "mixed_with_empty_sides": (12, 15, 40, (0, 12), (0, 15), 0.2, 0.2, 4),
    "ng_3_nt_130": (3, 130, 10, (0, 3), (0, 130), 0.2, 0.2, 5),
    "identical_boxes": (8, 12, 16, (4, 8), (6, 12), 0.1, 0.9, 6),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    NG, NT, F, m, k, ignore, tie, seed = SHAPES[name]
    frames = mc.draw_frames(seed, F, NG, NT, m, k, ignore=ignore, tie=tie)
    return frames, NG, NT, mc.run_reference(frames, NG, NT)


def _launch(L, state, seqs, order, slots, resets, thr=0.5, M=None, K=None):
    """One launch over the frames ``order`` = [(sequence number, frame)]; padding rows hold garbage."""
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
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    L.mot_eval(state, dev(gb), dev(gi), dev(gf), dev(ng), dev(tb), dev(ti), dev(nt),
               torch.tensor(slots, dtype=torch.int32, device=DEV), torch.tensor(resets, dtype=torch.int32, device=DEV),
               thr)
    L.mot_eval_check(state)


def _same(got, ref):
    for key in moteval.STATE_ARRAYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(ref[key])
        if key == "motp_sum":
            a, b = a.view(np.int64), b.view(np.int64)
        assert a.dtype == b.dtype and np.array_equal(a, b), (key, np.argwhere(a != b)[:8].tolist())
    assert moteval.states_equal(got, ref)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_reference(hip_lib, name):
    from src.moe import _lib as L

    frames, NG, NT, ref = _case(name)
    if name == "mixed_with_empty_sides":
        assert any(len(f[1]) == 0 for f in frames) and any(len(f[4]) == 0 for f in frames)
        assert ref["counts"][4] > 0 and ref["counts"][3] > 0  # removed rows and switches
    if name == "identical_boxes":
        assert ref["motp_sum"][0] > 0 and ref["counts"][0] > 0
    st = moteval.MotEvalState(1, NG, NT, DEV)
    _launch(L, st, [frames], [(0, f) for f in range(len(frames))], [0] * len(frames), [0] * len(frames))
    _same(st.export(0), ref)


@pytest.mark.timeout(60)
def test_every_row_removed_by_ignore_regions(hip_lib):
    from src.moe import _lib as L

    frames = [frame([(0, A, 1)], [(0, A)]),
              frame([(1, A, 0), (2, B, 0), (0, C, 1)], [(0, A), (1, B)]),  # both rows removed, the truth missed
              frame([(1, A, 0), (2, B, 0)], [(2, B), (1, A)]),              # nothing left on either side
              frame([(0, A, 1)], [(0, A)])]
    ref = mc.run_reference(frames, 3, 3)
    assert ref["counts"].tolist()[:6] == [2, 1, 0, 0, 4, 4]
    st = moteval.MotEvalState(1, 3, 3, DEV)
    _launch(L, st, [frames], [(0, f) for f in range(4)], [0] * 4, [0] * 4)
    _same(st.export(0), ref)


@pytest.mark.timeout(60)
def test_three_sequences_in_one_launch(hip_lib):
    """Lengths 1, 7 and 40, interleaved, the slots not in sequence order; a fourth slot without frames stays new."""
    from src.moe import _lib as L

    frames, NG, NT, ref = _case("mixed_with_empty_sides")
    seqs = [frames[:1], frames[10:17], frames]
    refs = [mc.run_reference(s, NG, NT) for s in seqs[:2]] + [ref]
    order = sorted([(q, f) for q in range(3) for f in range(len(seqs[q]))], key=lambda qf: (qf[1], -qf[0]))
    slot_of = [2, 0, 3]
    st = moteval.MotEvalState(4, NG, NT, DEV)
    _launch(L, st, seqs, order, [slot_of[q] for q, _ in order], [0] * len(order))
    for q in range(3):
        _same(st.export(slot_of[q]), refs[q])
    _same(st.export(1), moteval.new_state(NG, NT))


@pytest.mark.timeout(60)
def test_launches_of_1_16_23_keep_the_state(hip_lib):
    from src.moe import _lib as L

    frames, NG, NT, ref = _case("mixed_with_empty_sides")
    st = moteval.MotEvalState(1, NG, NT, DEV)
    before = L.launch_counts().get("mot_eval", 0)
    for lo, hi in ((0, 1), (1, 17), (17, 40)):
        _launch(L, st, [frames], [(0, f) for f in range(lo, hi)], [0] * (hi - lo), [0] * (hi - lo))
    assert L.launch_counts().get("mot_eval", 0) - before == 3
    _same(st.export(0), ref)


@pytest.mark.timeout(60)
def test_slot_reused_after_frame_reset(hip_lib):
    from src.moe import _lib as L

    frames, NG, NT, ref = _case("mixed_with_empty_sides")
    other, _, _, _ = _case("identical_boxes")  # smaller indices: fits the same state
    st = moteval.MotEvalState(1, NG, NT, DEV)
    order = [(0, f) for f in range(len(other))] + [(1, f) for f in range(len(frames))]
    resets = [0] * len(other) + [1] + [0] * (len(frames) - 1)
    _launch(L, st, [other, frames], order, [0] * len(order), resets)
    _same(st.export(0), ref)


@pytest.mark.timeout(60)
def test_thr_equal_to_a_pairs_iou(hip_lib):
    from src.moe import _lib as L

    moved = shifted(A, 13.0)
    iou = moteval._iou(np.asarray([moved], np.float32), np.asarray([A], np.float32))[0, 0]
    frames = [frame([(0, A, 1)], [(0, moved)])] * 2
    for thr, tp in ((float(iou), 2), (float(np.nextafter(iou, np.float32(1))), 0)):
        ref = mc.run_reference(frames, 1, 1, thr)
        assert ref["counts"][0] == tp and ref["pmc"][0, 0] == tp
        st = moteval.MotEvalState(1, 1, 1, DEV)
        _launch(L, st, [frames], [(0, 0), (0, 1)], [0, 0], [0, 0], thr=thr)
        _same(st.export(0), ref)


@pytest.mark.timeout(120)
def test_at_the_lds_limits(hip_lib):
    """K = 1024 rows and M = 256 truths, 2 frames: 63.8 KiB of LDS."""
    from src.moe import _lib as L

    frames = mc.draw_frames(11, 2, 256, 1024, (256, 256), (1024, 1024), ignore=0.1, tie=0.2)
    ref = mc.run_reference(frames, 256, 1024)
    assert ref["counts"][0] > 100 and ref["counts"][4] > 0
    st = moteval.MotEvalState(1, 256, 1024, DEV)
    _launch(L, st, [frames], [(0, 0), (0, 1)], [0, 0], [0, 0])
    _same(st.export(0), ref)


@pytest.mark.timeout(60)
def test_evaluate_on_the_device_equals_the_host(hip_lib, monkeypatch):
    from src.moe import _lib as L

    rng = np.random.default_rng(0)
    gt, res = {}, {}
    for key, n in (("a", 30), ("b", 7), ("c", 1)):
        rows_g, rows_t = [], []
        for f, (gb, gi, gf, tb, ti) in enumerate(mc.draw_frames(int(rng.integers(99)), n, 9, 11, (0, 9), (0, 11),
                                                                 ignore=0.2, tie=0.2), 1):
            rows_g += [(f, 10 + 3 * int(g), *np.round(b, 2).tolist(), 1, 1 if fl else 8, 1)
                       for b, g, fl in zip(gb, gi, gf)]
            rows_t += [(f, 5 + 2 * int(t), *np.round(b, 2).tolist(), 0.9, -1, -1, -1) for b, t in zip(tb, ti)]
        gt[key] = moteval.parse_gt(mc.mot_text(rows_g), ignore_classes=[8])
        res[key] = mc.mot_text(rows_t)
    before = L.launch_counts().get("mot_eval", 0)
    on_dev = moteval.evaluate(gt, res, device=DEV)
    assert L.launch_counts().get("mot_eval", 0) - before == 1  # 38 frames: one chunk
    monkeypatch.setenv("MOE_TRACK_EVAL", "0")
    assert on_dev == moteval.evaluate(gt, res, device=DEV) == moteval.evaluate(gt, res)
    assert L.launch_counts().get("mot_eval", 0) - before == 1
    assert on_dev["COMBINED"]["TP"] > 50 and on_dev["COMBINED"]["removed"] > 0


@pytest.mark.timeout(60)
def test_refusals_launch_nothing(hip_lib):
    from src.moe import _lib as L

    st = moteval.MotEvalState(1, 2, 2, DEV)

    def call(F, M, K):
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)  # noqa: E731
        L.mot_eval(st, torch.zeros((F, M, 4), device=DEV), z(F, M), z(F, M), z(F), torch.zeros((F, K, 4), device=DEV),
                   z(F, K), z(F), z(F), z(F), 0.5)

    before = L.launch_counts()
    with pytest.raises(L.MoEKernelError, match="K <= 1024"):
        call(1, 4, 1025)
    with pytest.raises(L.MoEKernelError, match="M <= 256"):
        call(1, 257, 4)
    with pytest.raises(L.MoEKernelError, match="thr"):
        L.mot_eval(st, *(torch.zeros(s, dtype=d, device=DEV) for s, d in (
            ((1, 1, 4), torch.float32), ((1, 1), torch.int32), ((1, 1), torch.int32), ((1,), torch.int32),
            ((1, 1, 4), torch.float32), ((1, 1), torch.int32), ((1,), torch.int32), ((1,), torch.int32),
            ((1,), torch.int32))), float("nan"))
    call(0, 4, 4)  # F == 0: fine, and no launch
    assert L.launch_counts() == before
    L.mot_eval_check(st)
    _same(st.export(0), moteval.new_state(2, 2))
    # an index outside the state fails the call and leaves the frame out
    fr = frame([(2, A, 1)], [(0, A)])
    with pytest.raises(L.MoEKernelError, match="status 4"):
        _launch(L, st, [[fr]], [(0, 0)], [0], [0])
    st.status.zero_()
    _same(st.export(0), moteval.new_state(2, 2))
