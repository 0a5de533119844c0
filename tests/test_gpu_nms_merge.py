"""rtdetr_nms_merge (_lib.nms_merge) against merge.merge_reference: the kept
indices, count, the gathered outputs and the padding, exactly (no tolerance:
the kernel restates the reference's fp32 arithmetic operation by operation)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from nms_merge_cases import draw_batch, reference_batch

pytestmark = pytest.mark.gpu

# (N, max_det, metric, class_agnostic, thr, conf, n_valid given): B = 3 images with n_valid = {0, N // 2, N}
# (None: the NULL pointer, every image N).  N around the 64-lane chunk, the 256 / 1024-thread launch boundary
# (N <= 256), one and many chunks, the limits; max_det 1, below a chunk, the default, the limit.
SIZES = [
    (1, 1, "ios", False, 0.5, 0.0, True),
    (63, 7, "iou", False, 0.5, 0.0, True),
    (64, 300, "ios", True, 0.5, 0.25, True),
    (65, 1, "iou", False, 0.0, 0.0, True),
    (129, 1024, "ios", False, 0.5, 0.0, True),
    (256, 300, "iou", True, 0.5, 0.25, True),
    (257, 300, "ios", False, 0.5, 0.0, True),
    (1500, 300, "ios", False, 0.5, 0.25, True),
    (1500, 300, "iou", True, 0.5, 0.0, True),
    (1500, 7, "ios", False, 0.0, 0.0, True),
    (1500, 1024, "iou", False, 0.0, 0.25, None),
    (4096, 1024, "iou", False, 0.5, 0.0, True),
    (4096, 300, "ios", True, 0.5, 0.25, None),
    (4096, 1024, "ios", False, 1.0, 0.0, True),
]
# max_det 7 of 1500 candidates: with 250 clusters the seven best are seven different objects and nothing is
# suppressed before the cut; 12 clusters put copies among the first visited
CLUSTERS = {(1500, 7): 12}
# every combination of the options at one size
OPTIONS = [(129, 300, m, a, t, c, True) for m in ("ios", "iou") for a in (False, True) for t in (0.0, 0.5, 1.0)
           for c in (0.0, 0.25)]


def _garbage(B, max_det, dev):
    """Output buffers holding what a reused buffer might: NaN, huge values, plausible indices."""
    return (torch.full((B, max_det, 4), float("nan"), device=dev), torch.full((B, max_det), 7.5, device=dev),
            torch.full((B, max_det), 12345, dtype=torch.int32, device=dev),
            torch.full((B, max_det), 3, dtype=torch.int32, device=dev),
            torch.full((B,), 999, dtype=torch.int32, device=dev))


def _check(L, boxes, scores, labels, n_valid, conf, thr, metric, max_det, agnostic, kept):
    """One launch into garbage-filled buffers; every output element against the reference's kept lists."""
    dev = torch.device("cuda", 0)
    B = boxes.shape[0]
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=dev)
    out = L.nms_merge(boxes.to(dev), scores.to(dev), labels.to(dev), nv, conf, thr, metric, max_det, agnostic,
                      out=_garbage(B, max_det, dev))
    ob, osc, ol, osrc, cnt = (t.cpu() for t in out)
    assert cnt.tolist() == [len(k) for k in kept]
    for b, k in enumerate(kept):
        n = len(k)
        assert osrc[b, :n].tolist() == k
        idx = torch.tensor(k, dtype=torch.int64)
        assert torch.equal(ob[b, :n], boxes[b][idx])
        assert torch.equal(osc[b, :n].view(torch.int32), scores[b][idx].view(torch.int32))  # the bits: -0.0, -inf
        assert torch.equal(ol[b, :n], labels[b][idx])
        assert bool((osrc[b, n:] == -1).all())
        assert not ob[b, n:].view(torch.int32).any() and not osc[b, n:].view(torch.int32).any()
        assert not ol[b, n:].any()


@pytest.mark.parametrize("N,max_det,metric,agnostic,thr,conf,nv", SIZES + OPTIONS)
def test_drawn_candidates(hip_lib, N, max_det, metric, agnostic, thr, conf, nv):
    from src.moe import _lib as L

    boxes, scores, labels = draw_batch(3, N, seed=N * 31 + max_det, clusters=CLUSTERS.get((N, max_det)))
    n_valid = [0, N // 2, N] if nv else None
    kept, suppressed = reference_batch(boxes, scores, labels, n_valid, conf, thr, metric, max_det, agnostic)
    # the comparison must not pass on nothing: asserted on the reference, before the GPU is touched
    print(f"N {N} max_det {max_det} {metric} agnostic {agnostic} thr {thr} conf {conf}: kept "
          f"{[len(k) for k in kept]}, suppressed {suppressed}")
    if thr == 1.0:
        # by the rule itself nothing can be suppressed at thr = 1: iw <= either width and ih <= either height
        # (fp32 subtraction is monotone), so inter <= min(area_i, area_j) <= den under both metrics and
        # inter > den never holds; the case is degenerate like max_det = 1: everything is kept up to the cut
        assert sum(suppressed) == 0 and max(len(k) for k in kept) >= min(2, max_det)
    elif N > 1 and max_det > 1:
        assert max(len(k) for k in kept) >= 2 and sum(suppressed) >= 2
    _check(L, boxes, scores, labels, n_valid, conf, thr, metric, max_det, agnostic, kept)


def test_all_candidates_one_box(hip_lib):
    from src.moe import _lib as L

    _, scores, _ = draw_batch(2, 200, seed=5)
    boxes = torch.tensor([100.0, 50.0, 140.0, 150.0]).repeat(2, 200, 1)
    labels = torch.zeros((2, 200), dtype=torch.int32)
    for metric in ("ios", "iou"):
        kept, _ = reference_batch(boxes, scores, labels, None, 0.0, 0.5, metric, 300, False)
        assert [len(k) for k in kept] == [1, 1]
        assert kept[0] == [int(np.argsort(-scores[0].numpy(), kind="stable")[0])]
        _check(L, boxes, scores, labels, None, 0.0, 0.5, metric, 300, False, kept)


def test_all_candidates_disjoint(hip_lib):
    from src.moe import _lib as L

    N = 500
    i = torch.arange(N, dtype=torch.float32)
    x, y = 30 * (i % 40), 60 * (i // 40)
    boxes = torch.stack([x, y, x + 20, y + 50], 1).repeat(2, 1, 1)  # touching neither neighbour
    _, scores, labels = draw_batch(2, N, seed=6)
    for max_det, want in ((1024, N), (300, 300)):
        kept, suppressed = reference_batch(boxes, scores, labels, None, 0.0, 0.0, "ios", max_det, True)
        assert [len(k) for k in kept] == [want, want] and suppressed == [0, 0]
        _check(L, boxes, scores, labels, None, 0.0, 0.0, "ios", max_det, True, kept)


def test_nan_inf_scores_and_zero_area_boxes(hip_lib):
    from src.moe import _lib as L

    N = 300
    boxes, scores, labels = draw_batch(2, N, seed=7)
    scores[:, ::7] = float("nan")
    scores[:, 3::11] = float("-inf")
    scores[:, 5::13] = float("inf")
    scores[0, 2::17] = -0.0
    scores[1, 4::17] = 0.0
    boxes[:, 1::5, 2] = boxes[:, 1::5, 0]            # zero width
    boxes[:, 2::9, 3] = boxes[:, 2::9, 1] - 4.0      # y2 < y1
    for conf in (float("-inf"), -1.0, 0.0, 0.25):
        for metric in ("ios", "iou"):
            kept, suppressed = reference_batch(boxes, scores, labels, [N, N - 50], conf, 0.5, metric, 300, False)
            flat = [i for k in kept for i in k]
            assert not any(bool(torch.isnan(scores[b, i])) for b, k in enumerate(kept) for i in k)
            assert len(flat) >= 2 and sum(suppressed) >= 2
            if conf == float("-inf"):
                assert any(scores[b, i] == float("-inf") for b, k in enumerate(kept) for i in k)
            # every zero-area candidate that takes part is kept (the cut is not reached)
            assert all(len(k) < 300 for k in kept)
            _check(L, boxes, scores, labels, [N, N - 50], conf, 0.5, metric, 300, False, kept)


def test_n_valid_is_clamped_and_empty_inputs(hip_lib):
    from src.moe import _lib as L

    boxes, scores, labels = draw_batch(3, 100, seed=8)
    kept, _ = reference_batch(boxes, scores, labels, [-5, 100000, 40], 0.0, 0.5, "ios", 50, False)
    assert kept[0] == [] and len(kept[1]) >= 2
    _check(L, boxes, scores, labels, [-5, 100000, 40], 0.0, 0.5, "ios", 50, False, kept)
    # N == 0: succeeds, count zeroed, outputs all padding
    _check(L, boxes[:, :0], scores[:, :0], labels[:, :0], None, 0.0, 0.5, "ios", 9, False, [[], [], []])
    # B == 0: succeeds
    out = L.nms_merge(boxes[:0].cuda(), scores[:0].cuda(), labels[:0].cuda(), None, 0.0, 0.5, "ios", 9)
    assert tuple(out[0].shape) == (0, 9, 4) and tuple(out[4].shape) == (0,)


def test_bad_arguments_return_an_error_without_a_launch(hip_lib):
    from src.moe import _lib as L

    dev = torch.device("cuda", 0)
    boxes, scores, labels = (t.to(dev) for t in draw_batch(2, 64, seed=9))
    out = _garbage(2, 8, dev)
    before = [t.clone() for t in out]
    p = [t.data_ptr() for t in (boxes, scores, labels)]
    o = [t.data_ptr() for t in out]
    st = torch.cuda.current_stream().cuda_stream
    nan = float("nan")

    def call(B=2, N=64, conf=0.0, thr=0.5, metric=1, agnostic=0, max_det=8, ins=p, outs=o):
        return hip_lib.rtdetr_nms_merge(ins[0], ins[1], ins[2], None, B, N, conf, thr, metric, agnostic, max_det,
                                        outs[0], outs[1], outs[2], outs[3], outs[4], st)

    L.launch_counts(reset=True)
    bad = [dict(N=4097), dict(N=-1), dict(B=1025), dict(B=-1), dict(max_det=0), dict(max_det=1025), dict(metric=2),
           dict(metric=-1), dict(thr=nan), dict(conf=nan), dict(ins=[None, p[1], p[2]]), dict(ins=[p[0], None, p[2]]),
           dict(ins=[p[0], p[1], None]), dict(ins=[p[0] + 4, p[1], p[2]]), dict(outs=[o[0] + 4] + o[1:])]
    bad += [dict(outs=o[:j] + [None] + o[j + 1:]) for j in range(5)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_nms_merge"), kw
    torch.cuda.synchronize()
    assert "merge" not in L.launch_counts()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, before))
    assert call() == 0
    torch.cuda.synchronize()
    assert L.launch_counts(reset=True).get("merge") == 1
    # the typed wrapper refuses what the C entry cannot see
    with pytest.raises(L.MoEKernelError):
        L.nms_merge(boxes, scores, labels.long(), None, 0.0, 0.5, "ios", 8)
    with pytest.raises(L.MoEKernelError):
        L.nms_merge(boxes, scores[:, :63], labels, None, 0.0, 0.5, "ios", 8)
    with pytest.raises(L.MoEKernelError):
        L.nms_merge(boxes, scores, labels, None, 0.0, 0.5, "giou", 8)
    with pytest.raises(L.MoEKernelError):
        L.nms_merge(boxes.cpu(), scores, labels, None, 0.0, 0.5, "ios", 8)
    assert "rtdetr_nms_merge" in L.SIGNATURES and L.PROF_KINDS[19] == "merge"
