"""The reference and the case table of the fused set criterion's GPU tests
(tests/criterion_cases.py), checked without a GPU: the reference IS the
project's loss (SetCriterion.forward, the scipy host path, and its autograd
gradients), cost64 is HungarianMatcher's cost, and the tables have the
properties the GPU tests rely on.  With CRITERION_REPORT=<file> every case
appends one JSON line with the error of the fp32 torch evaluation against the
float64 reference -- the reference's side of the GPU tests' tolerance."""
import numpy as np
import pytest
import torch

import criterion_cases as cc
from src.rtdetr_moe import criterion as crit_mod
from src.rtdetr_moe.criterion import SetCriterion

GENERAL_ROWS = cc.SHAPE_ROWS + [cc.SQUARE_ROW]

# fp32 on both sides, the same element-wise formulas: what differs is the
# summation tree of up to 16 K terms (pairwise: ~log2(n) 2^-24 ~ 8e-7 each side)
# and one division.  2^-17 = 128 fp32 ulp leaves room for both.
SAME_FORMULA_FP32 = 2.0 ** -17
# |cost| stays below 32 (5 L1 <= 10, 2 |focal| <= 28, 2 |GIoU| <= 4); an fp32 ulp
# there is 1.9e-6 and the cost is about ten roundings deep
COST_FP32_ABS = 2e-5


def _outputs_targets(row):
    logits, boxes, tb, tl, n_valid = cc.draw(row)
    S = logits.shape[0]
    sets = [{"pred_logits": logits[s].clone().requires_grad_(True),
             "pred_boxes": boxes[s].clone().requires_grad_(True)} for s in range(S)]
    outputs = dict(sets[0])
    if S > 1:
        outputs["aux_outputs"] = sets[1:]
    targets = [{"boxes": tb[b, :int(n)], "labels": tl[b, :int(n)]} for b, n in enumerate(n_valid)]
    return (logits, boxes, tb, tl, n_valid), sets, outputs, targets


def _scipy_assign(crit, sets, targets, M):
    indices = crit.matcher.match_many(sets, targets)
    assign = torch.full((len(sets), len(targets), M), -1, dtype=torch.int32)
    for s, per_image in enumerate(indices):
        for b, (q, m) in enumerate(per_image):
            assign[s, b, m] = q.to(torch.int32)
    return assign


@pytest.mark.parametrize("row", GENERAL_ROWS, ids=cc.row_id)
def test_reference_is_the_projects_loss(row):
    """evaluate() in fp32 at scipy's assignment, with the criterion's weights,
    gives SetCriterion.forward's losses and autograd gradients."""
    S, B, Q, C, M, nv = row
    (logits, boxes, tb, tl, n_valid), sets, outputs, targets = _outputs_targets(row)
    crit = SetCriterion(num_classes=C)
    nb = float(max(sum(nv), 1))
    assign = _scipy_assign(crit, sets, targets, M)
    assert all(int((assign[:, b] >= 0).sum()) == S * n for b, n in enumerate(nv))
    losses = crit.forward(outputs, targets, nb)
    leaves = [t for o in sets for t in (o["pred_logits"], o["pred_boxes"])]
    grads = torch.autograd.grad(sum(losses.values()), leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    suffix = [""] + [f"_aux{i}" for i in range(S - 1)]
    want = torch.stack([torch.stack([losses[k + sfx].detach() for k in ("loss_vfl", "loss_bbox", "loss_giou")])
                        for sfx in suffix])
    W = torch.tensor(cc.CRIT_W).expand(S, 3)
    comps, g_lg, g_bx = cc.evaluate(torch.float32, logits, boxes, tb, tl, n_valid, assign, nb, crit.alpha, W)
    got = {"losses": (comps * W, want), "d_logits": (g_lg, torch.stack(grads[0::2])),
           "d_boxes": (g_bx, torch.stack(grads[1::2]))}
    for k, (a, b) in got.items():
        e = cc.rel_err(a, b)
        print(cc.row_id(row), k, e)
        assert e <= SAME_FORMULA_FP32, (k, e)


@pytest.mark.parametrize("row", GENERAL_ROWS, ids=cc.row_id)
def test_cost64_is_the_matchers_cost(row, monkeypatch):
    """The matrices HungarianMatcher.match_many hands to scipy are cost64[s, b, :, :n]."""
    S, B, Q, C, M, nv = row
    (logits, boxes, tb, tl, n_valid), sets, _, targets = _outputs_targets(row)
    seen = []
    solver = crit_mod.linear_sum_assignment

    def spy(c):
        seen.append(np.array(c, np.float64))
        return solver(c)

    monkeypatch.setattr(crit_mod, "linear_sum_assignment", spy)
    SetCriterion(num_classes=C).matcher.match_many(sets, targets)
    want = cc.cost64(logits, boxes, tb, tl).numpy()
    expect = [(s, b) for s in range(S) for b in range(B) if nv[b] > 0] if sum(nv) else []
    assert len(seen) == len(expect)
    for c, (s, b) in zip(seen, expect):
        assert c.shape == (Q, nv[b])
        d = float(np.abs(c - want[s, b, :, :nv[b]]).max())
        assert d <= COST_FP32_ABS, (s, b, d)
    eps = cc.cost_eps(logits, boxes, tb, tl)
    assert 0.0 < eps <= cc.MARGIN * COST_FP32_ABS


def test_rows_fit_their_problem():
    for row in cc.MATCH_ROWS + [(cc.DN["S"], cc.DN["B"], 2 * cc.DN["M"], cc.DN["C"], cc.DN["M"], cc.DN["n_valid"])]:
        S, B, Q, C, M, nv = row
        assert len(nv) == B and all(0 <= n <= min(Q, M) for n in nv), row
        assert B * Q * C * 4 <= 64 * 1024, row
    S, B, Q, C, M, _ = cc.SHAPE_ROWS[5]
    assert B * Q * C * 4 == 65536
    assert any(r[1] * r[4] > 256 and r[4] > 64 for r in cc.SHAPE_ROWS)
    assert any(r[3] > 4 for r in cc.SHAPE_ROWS) and any(sum(r[5]) == 0 for r in cc.SHAPE_ROWS)
    for c in cc.loss_cases().values():  # a valid slot's query is matched once
        si, bi, mi, qi = cc.matched_pairs(c.n_valid, c.assign)
        key = (si * c.shape[1] + bi) * c.shape[2] + qi
        assert key.unique().numel() == key.numel(), c.name
        assert qi.numel() == 0 or int(qi.max()) < c.shape[2], c.name
    lab = cc.label_case()
    C = lab.shape[3]
    assert (lab.tgt_labels == -1).any() and (lab.tgt_labels == C).any()


def test_geometry_table_is_exact_and_clear_of_the_thresholds():
    c = cc.geometry_case()
    n = cc.N_DYADIC
    M = c.shape[4]
    assert M == n + len(cc.TINY_ROWS) and c.shape[2] == 2 * M
    src = c.boxes[:, :, 0::2][:, :, :n]
    for t in (src, c.tgt_boxes[:, :n]):  # on the 1/64 grid
        assert torch.equal(t * 64, (t * 64).round())
    # corners, differences and therefore every tie are the same numbers in fp32 and fp64
    for t in (src, c.tgt_boxes[:, :n]):
        assert torch.equal(cc._xyxy(t).double(), cc._xyxy(t.double()))
    assert torch.equal((src - c.tgt_boxes[None, :, :n]).double(), src.double() - c.tgt_boxes[None, :, :n].double())
    # every union and enclosing area is far from the 1e-9 clamp, in both precisions
    for dtype in (torch.float32, torch.float64):
        union, area = cc.geometry_parts(c, dtype)
        for name, v in (("union", union), ("area", area)):
            assert bool(((v <= 1e-10) | (v >= 1e-6)).all()), (name, dtype, v)
    u64, a64 = cc.geometry_parts(c, torch.float64)
    tiny = {r[0]: n + i for i, r in enumerate(cc.TINY_ROWS)}
    assert bool((u64[..., tiny["tiny_coincident"]] < 1e-9).all() and (a64[..., tiny["tiny_coincident"]] < 1e-9).all())
    assert bool((u64[..., tiny["tiny_apart"]] < 1e-9).all() and (a64[..., tiny["tiny_apart"]] >= 1e-6).all())
    # the rows do what their names say (image 0, set 0)
    rows = {r[0]: i for i, r in enumerate(cc.GEOMETRY_ROWS)}
    a = cc._xyxy(c.boxes[0, 0, 0::2].double())
    b = cc._xyxy(c.tgt_boxes[0].double())
    iw = torch.min(a[:, 2], b[:, 2]) - torch.max(a[:, 0], b[:, 0])
    ih = torch.min(a[:, 3], b[:, 3]) - torch.max(a[:, 1], b[:, 1])
    assert iw[rows["touch_edge"]] == 0 and ih[rows["touch_edge"]] > 0
    assert iw[rows["touch_corner"]] == 0 and ih[rows["touch_corner"]] == 0
    assert iw[rows["disjoint_x"]] < 0 and ih[rows["disjoint_x"]] > 0
    assert iw[rows["disjoint_y"]] > 0 and ih[rows["disjoint_y"]] < 0
    assert iw[rows["disjoint_xy"]] < 0 and ih[rows["disjoint_xy"]] < 0
    assert torch.equal(a[rows["identical"]], b[rows["identical"]])
    assert a[rows["shared_left_edge"], 0] == b[rows["shared_left_edge"], 0]
    assert a[rows["shared_right_top_edge"], 2] == b[rows["shared_right_top_edge"], 2]
    assert a[rows["negative_width_source"], 2] < a[rows["negative_width_source"], 0]
    assert a[rows["zero_width_source"], 2] == a[rows["zero_width_source"], 0]
    g = rows["general_overlap"]
    assert not bool((a[g] == b[g]).any()) and iw[g] > 0 and ih[g] > 0


def test_logit_table_has_finite_expected_values():
    c = cc.logit_case()
    ref, _ = cc.case_reference(c.name)
    for t in ref:
        assert bool(torch.isfinite(t).all())
    si, bi, mi, qi = cc.matched_pairs(c.n_valid, c.assign)
    iou, _ = cc._iou_giou(cc._xyxy(c.boxes.double()[si, bi, qi]), cc._xyxy(c.tgt_boxes.double()[bi, mi]))
    assert bool((iou == 0).any() and (iou == 1).any() and ((iou > 0.3) & (iou < 0.9)).any())
    matched = c.logits[si, bi, qi, c.tgt_labels[bi, mi]]
    bg = torch.ones_like(c.logits, dtype=torch.bool)
    bg[si, bi, qi, c.tgt_labels[bi, mi]] = False
    for v in cc.LOGIT_VALUES:  # every value on a matched entry at every IoU kind, and on background entries
        for kind in (iou == 0, iou == 1, (iou > 0) & (iou < 1)):
            assert bool((matched[kind] == v).any()), v
        assert bool((c.logits[bg] == v).any()), v


@pytest.mark.parametrize("name", cc.LOSS_CASE_NAMES)
def test_fp32_figures(name):
    """The reference is finite on every case; its fp32 evaluation's error is
    reported (CRITERION_REPORT) as the yardstick of the GPU tests."""
    ref, fig = cc.case_reference(name)
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    assert all(np.isfinite(v) for v in fig.values())
    cc.report({"case": name, "side": "fp32_torch", **fig, "limits": cc.limits(fig)})
    print(name, fig)
