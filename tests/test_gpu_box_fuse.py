"""rtdetr_box_fuse (_lib.box_fuse) against merge.fuse_reference: the fused boxes,
members, kept indices, count, scores, labels and the padding, exactly (no
tolerance: the kernel restates the reference's fp32 arithmetic operation by
operation, in the reference's order, with one correctly rounded division)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import nms_merge_cases
from box_fuse_cases import draw_batch, hand_cases, reference_batch, run_hand_case

pytestmark = pytest.mark.gpu

# (P, k, max_det, metric, class_agnostic, thr, fuse_thr, conf, n_valid given): B = 3 images with n_valid = {0, N // 2,
# N} (None: the NULL pointer).  N = P k = 5, 65, 130, 260, 1500, 4095: both sides of the 64-lane chunk, the 256 /
# 1024-thread launch switch (N <= 256), the sort padding; P = 3 at N = 63 and 129; max_det 1, below a chunk, the
# default, the limit.
SIZES = [
    (5, 1, 300, "ios", False, 0.5, 0.55, 0.0, None),
    (5, 13, 7, "ios", False, 0.5, 0.55, 0.0, None),
    (5, 13, 300, "iou", True, 0.5, 0.55, 0.0, True),
    (5, 26, 1024, "ios", False, 0.5, 0.55, 0.25, True),
    (5, 52, 300, "ios", False, 0.5, 0.55, 0.0, True),
    (5, 52, 1, "ios", False, 0.5, 0.55, 0.0, True),
    (5, 300, 300, "ios", False, 0.5, 0.55, 0.25, True),
    (5, 300, 1024, "iou", True, 0.5, 0.55, 0.0, None),
    (5, 300, 7, "ios", False, 0.5, 0.55, 0.0, None),
    (5, 819, 300, "ios", False, 0.5, 0.55, 0.0, True),
    (5, 819, 1024, "ios", True, 0.5, 0.55, 0.25, None),
    (3, 21, 300, "ios", False, 0.5, 0.55, 0.0, True),
    (3, 43, 7, "iou", False, 0.5, 0.55, 0.0, None),
]
# (seed, objects) where the default draw does not meet the preconditions asserted below: few objects where max_det
# cuts the walk early, so that their copies stand among the first visited; tuned on the CPU reference
DRAWS = {(5, 1, 300): (1, 2), (5, 13, 7): (5, 3), (5, 300, 7): (5, 3), (3, 43, 7): (5, 3)}
# every combination of the options at N = 130
OPTIONS = [(5, 26, 300, m, a, t, f, c, True) for m in ("ios", "iou") for a in (False, True) for t in (0.0, 0.5)
           for f in (0.0, 0.55, 1.0) for c in (0.0, 0.25)]


def _garbage(B, max_det, dev):
    """Output buffers holding what a reused buffer might: NaN, huge values, plausible indices."""
    return (torch.full((B, max_det, 4), float("nan"), device=dev), torch.full((B, max_det), 7.5, device=dev),
            torch.full((B, max_det), 12345, dtype=torch.int32, device=dev),
            torch.full((B, max_det), 3, dtype=torch.int32, device=dev),
            torch.full((B,), 999, dtype=torch.int32, device=dev),
            torch.full((B, max_det), -77, dtype=torch.int32, device=dev))


def _launch(L, boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, agnostic, fuse_thr):
    dev = torch.device("cuda", 0)
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    win = None if windows is None else windows.to(dev)
    out = L.box_fuse(boxes.to(dev), scores.to(dev), labels.to(dev), nv, conf, thr, metric, max_det, agnostic,
                     fuse_thr, win, out=_garbage(boxes.shape[0], max_det, dev))
    return tuple(t.cpu() for t in out)


def _check(L, boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, agnostic, fuse_thr, ref):
    """One launch into garbage-filled buffers; every output element against the reference."""
    args = (boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, agnostic, fuse_thr)
    ob, osc, ol, osrc, cnt, om = _launch(L, *args)
    assert cnt.tolist() == [len(r["kept"]) for r in ref]
    for b, r in enumerate(ref):
        n = len(r["kept"])
        assert osrc[b, :n].tolist() == r["kept"]
        idx = torch.tensor(r["kept"], dtype=torch.int64)
        assert torch.equal(om[b, :n], r["members"]), (b, om[b, :n].tolist(), r["members"].tolist())
        assert torch.equal(ob[b, :n].view(torch.int32), r["fused"].view(torch.int32)), \
            (b, (ob[b, :n] != r["fused"]).nonzero().tolist()[:8])
        assert torch.equal(osc[b, :n].view(torch.int32), scores[b][idx].view(torch.int32))
        assert torch.equal(ol[b, :n], labels[b][idx])
        assert bool((osrc[b, n:] == -1).all()) and not om[b, n:].any()
        assert not ob[b, n:].view(torch.int32).any() and not osc[b, n:].view(torch.int32).any()
        assert not ol[b, n:].any()
    # the walk's outputs are rtdetr_nms_merge's on the same inputs
    dev = torch.device("cuda", 0)
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    nb, nsc, nl, nsrc, ncnt = (t.cpu() for t in L.nms_merge(boxes.to(dev), scores.to(dev), labels.to(dev), nv, conf,
                                                            thr, metric, max_det, agnostic))
    assert torch.equal(nsrc, osrc) and torch.equal(ncnt, cnt) and torch.equal(nl, ol)
    assert torch.equal(nsc.view(torch.int32), osc.view(torch.int32))
    # a relaunch gives the same bits
    again = _launch(L, *args)
    first = (ob, osc, ol, osrc, cnt, om)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, first))


def _preconditions(ref, N, max_det, thr, fuse_thr):
    """Asserted on the reference, before the GPU is touched: the comparison must not pass on nothing."""
    clusters, unfused = sum(r["clusters"] for r in ref), sum(r["unfused"] for r in ref)
    cut, repaired = sum(r["cut"] for r in ref), sum(r["repaired"] for r in ref)
    members = torch.cat([r["members"] for r in ref])
    print(f"kept {[len(r['kept']) for r in ref]} clusters {clusters} unfused {unfused} cut {cut} repaired {repaired}")
    if max_det == 1:
        # the walk stops at the first keep: nothing was visited after it, so nothing was suppressed or fused
        assert clusters == 0 and unfused == 0 and bool((members == 1).all()) and len(members) >= 2
    elif fuse_thr == 1.0:
        # inter <= min(area_i, area_j) <= (area_i + area_j) - inter in fp32 (rounding is monotone), so inter > 1 *
        # union never holds: every suppressed candidate stays unfused
        assert clusters == 0 and bool((members == 1).all()) and unfused >= 1
    elif fuse_thr == 0.0:
        # every copy lies inside its pass's window, so the overlap that suppressed it (inter > thr * den >= 0)
        # lies inside both windows' intersection V and survives the clamp: inter > 0 and everything suppressed fuses
        assert clusters >= 2 and unfused == 0
    else:
        assert clusters >= 2 and unfused >= 1
        if N >= 260:
            assert cut >= 1 and repaired >= 1


@pytest.mark.parametrize("P,k,max_det,metric,agnostic,thr,fuse_thr,conf,nv", SIZES + OPTIONS)
def test_drawn_candidates(hip_lib, P, k, max_det, metric, agnostic, thr, fuse_thr, conf, nv):
    from src.moe import _lib as L

    N = P * k
    seed, objects = DRAWS.get((P, k, max_det), (N * 31 + max_det, None))
    boxes, scores, labels, windows = draw_batch(3, P, k, seed=seed, objects=objects)
    n_valid = [0, N // 2, N] if nv else None
    ref = reference_batch(boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, agnostic, fuse_thr)
    _preconditions(ref, N, max_det, thr, fuse_thr)
    _check(L, boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, agnostic, fuse_thr, ref)


@pytest.mark.parametrize("N", [64, 257])
def test_without_windows(hip_lib, N):
    """P = 0: one pool of candidates, nothing clamped, nothing cut."""
    from src.moe import _lib as L

    boxes, scores, labels = nms_merge_cases.draw_batch(3, N, seed=N + 11)
    n_valid = [0, N // 2, N]
    ref = reference_batch(boxes, scores, labels, None, n_valid, 0.0, 0.5, "ios", 300, False, 0.55)
    assert sum(r["clusters"] for r in ref) >= 2 and sum(r["unfused"] for r in ref) >= 1
    assert sum(r["cut"] for r in ref) == 0
    _check(L, boxes, scores, labels, None, n_valid, 0.0, 0.5, "ios", 300, False, 0.55, ref)


def test_max_det_falls_in_the_middle_of_a_chunk(hip_lib):
    from src.moe import _lib as L

    P, k, max_det = 5, 52, 100
    boxes, scores, labels, windows = draw_batch(3, P, k, seed=70)
    ref = reference_batch(boxes, scores, labels, windows, None, 0.0, 0.5, "ios", max_det, False, 0.55)
    for b, r in enumerate(ref):
        order = np.argsort(-scores[b].numpy(), kind="stable")
        pos = int(np.nonzero(order == r["kept"][-1])[0][0])  # conf 0 and scores >= 0: everyone takes part
        # the cut is reached, inside a chunk of 64 with visited candidates before it and unvisited ones after it
        assert len(r["kept"]) == max_det and 8 <= pos % 64 <= 55 and pos + 8 < P * k, (b, pos)
    assert sum(r["clusters"] for r in ref) >= 2 and sum(r["unfused"] for r in ref) >= 1
    _check(L, boxes, scores, labels, windows, None, 0.0, 0.5, "ios", max_det, False, 0.55, ref)


def test_hand_made_cases(hip_lib):
    from src.moe import _lib as L

    def fuse(boxes, scores, labels, windows, conf, thr, metric, max_det, agnostic, fuse_thr):
        ob, _, _, osrc, cnt, om = _launch(L, boxes, scores, labels, windows, None, conf, thr, metric,
                                          min(max_det, 1024), agnostic, fuse_thr)
        n = int(cnt[0])
        return osrc[0, :n].tolist(), ob[0, :n], om[0, :n].tolist()

    for case in hand_cases():
        run_hand_case(case, fuse)


def test_one_box_200_times(hip_lib):
    from src.moe import _lib as L

    _, scores, _ = nms_merge_cases.draw_batch(2, 200, seed=5)
    boxes = torch.tensor([100.0, 50.0, 140.0, 150.0]).repeat(2, 200, 1)
    labels = torch.zeros((2, 200), dtype=torch.int32)
    for metric in ("ios", "iou"):
        ref = reference_batch(boxes, scores, labels, None, None, 0.0, 0.5, metric, 300, False, 0.55)
        assert [len(r["kept"]) for r in ref] == [1, 1] and [int(r["members"][0]) for r in ref] == [200, 200]
        _check(L, boxes, scores, labels, None, None, 0.0, 0.5, metric, 300, False, 0.55, ref)


def test_500_disjoint_boxes(hip_lib):
    from src.moe import _lib as L

    N = 500
    i = torch.arange(N, dtype=torch.float32)
    x, y = 30 * (i % 40), 60 * (i // 40)
    boxes = torch.stack([x, y, x + 20, y + 50], 1).repeat(2, 1, 1)  # touching neither neighbour
    _, scores, labels = nms_merge_cases.draw_batch(2, N, seed=6)
    for max_det, want in ((1024, N), (300, 300)):
        ref = reference_batch(boxes, scores, labels, None, None, 0.0, 0.0, "ios", max_det, True, 0.55)
        for b, r in enumerate(ref):
            assert len(r["kept"]) == want and bool((r["members"] == 1).all())
            # untouched: integer coordinates below 2^12 times scores m / 64 are exact products, so (s c) / s = c;
            # a score of 0 falls back to the leader's own coordinate
            assert torch.equal(r["fused"], boxes[b][torch.tensor(r["kept"])])
        _check(L, boxes, scores, labels, None, None, 0.0, 0.0, "ios", max_det, True, 0.55, ref)


def test_n_valid_is_clamped_and_empty_inputs(hip_lib):
    from src.moe import _lib as L

    boxes, scores, labels, windows = draw_batch(3, 5, 20, seed=8)
    nv = [-5, 100000, 40]
    ref = reference_batch(boxes, scores, labels, windows, nv, 0.0, 0.5, "ios", 50, False, 0.55)
    assert ref[0]["kept"] == [] and len(ref[1]["kept"]) >= 2
    _check(L, boxes, scores, labels, windows, nv, 0.0, 0.5, "ios", 50, False, 0.55, ref)
    # N == 0: succeeds, count zeroed, outputs all padding
    empty = [dict(kept=[], fused=torch.zeros((0, 4)), members=torch.zeros(0, dtype=torch.int32))] * 3
    _check(L, boxes[:, :0], scores[:, :0], labels[:, :0], windows, None, 0.0, 0.5, "ios", 9, False, 0.55, empty)
    # B == 0: succeeds without a launch
    L.launch_counts(reset=True)
    out = L.box_fuse(boxes[:0].cuda(), scores[:0].cuda(), labels[:0].cuda(), None, 0.0, 0.5, "ios", 9)
    assert tuple(out[0].shape) == (0, 9, 4) and tuple(out[5].shape) == (0, 9)
    assert not L.launch_counts(reset=True)


def test_bad_arguments_return_an_error_without_a_launch(hip_lib):
    from src.moe import _lib as L

    dev = torch.device("cuda", 0)
    boxes, scores, labels, windows = (t.to(dev) for t in draw_batch(2, 4, 16, seed=9))
    out = _garbage(2, 8, dev)
    before = [t.clone() for t in out]
    p = [t.data_ptr() for t in (boxes, scores, labels)]
    o = [t.data_ptr() for t in out]
    w = windows.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    nan = float("nan")

    def call(B=2, N=64, conf=0.0, thr=0.5, metric=1, agnostic=0, max_det=8, fuse_thr=0.55, win=w, P=4, ins=p, outs=o):
        return hip_lib.rtdetr_box_fuse(ins[0], ins[1], ins[2], None, B, N, conf, thr, metric, agnostic, max_det,
                                       fuse_thr, win, P, outs[0], outs[1], outs[2], outs[3], outs[4], outs[5], st)

    L.launch_counts(reset=True)
    bad = [dict(N=4097, P=0), dict(N=-1, P=0), dict(B=1025), dict(B=-1), dict(max_det=0), dict(max_det=1025),
           dict(metric=2), dict(metric=-1), dict(thr=nan), dict(conf=nan), dict(fuse_thr=nan), dict(P=-1),
           dict(P=65, N=65), dict(P=5), dict(win=None), dict(win=w + 4), dict(ins=[None, p[1], p[2]]),
           dict(ins=[p[0], None, p[2]]), dict(ins=[p[0], p[1], None]), dict(ins=[p[0] + 4, p[1], p[2]]),
           dict(outs=[o[0] + 4] + o[1:])]
    bad += [dict(outs=o[:j] + [None] + o[j + 1:]) for j in range(6)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_box_fuse"), kw
    torch.cuda.synchronize()
    assert not L.launch_counts()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, before))
    assert call() == 0 and call(win=None, P=0) == 0
    torch.cuda.synchronize()
    assert L.launch_counts(reset=True) == {"merge": 2}  # raw calls: the wrapper's own count is not involved
    # the typed wrapper refuses what the C entry cannot see, and counts its launches under their own name
    with pytest.raises(L.MoEKernelError):
        L.box_fuse(boxes, scores, labels.long(), None, 0.0, 0.5, "ios", 8)
    with pytest.raises(L.MoEKernelError):
        L.box_fuse(boxes, scores[:, :63], labels, None, 0.0, 0.5, "ios", 8)
    with pytest.raises(L.MoEKernelError):
        L.box_fuse(boxes, scores, labels, None, 0.0, 0.5, "giou", 8)
    with pytest.raises(L.MoEKernelError):
        L.box_fuse(boxes, scores, labels, None, 0.0, 0.5, "ios", 8, windows=windows[:1])
    with pytest.raises(L.MoEKernelError):
        L.box_fuse(boxes, scores, labels, None, 0.0, 0.5, "ios", 8, windows=windows.cpu())
    with pytest.raises(L.MoEKernelError, match="rtdetr_box_fuse"):
        L.box_fuse(boxes, scores, labels, None, 0.0, 0.5, "ios", 8, windows=windows[:, :3].contiguous())  # 64 % 3
    assert not L.launch_counts()
    L.box_fuse(boxes, scores, labels, None, 0.0, 0.5, "ios", 8, windows=windows)
    L.nms_merge(boxes, scores, labels, None, 0.0, 0.5, "ios", 8)
    assert L.launch_counts(reset=True) == {"box_fuse": 1, "merge": 1}
    assert "rtdetr_box_fuse" in L.SIGNATURES
