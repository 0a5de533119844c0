"""Reference and case table of the fused set criterion's tests
(tests/test_criterion_cases_cpu.py, tests/test_gpu_criterion_edges.py).  No GPU
import: everything here runs on the CPU.

``reference`` is SetCriterion.forward_padded's loss for a GIVEN assignment,
restated in plain torch and evaluated in float64 on the (fp32) inputs widened
exactly; ``evaluate`` is the same code at any dtype, so that its fp32 run
measures what fp32 can do at all on a case (``fp32_figures``): the kernels are
allowed ``MARGIN`` times that error against the float64 reference, and never
less than ``FLOOR``.  ``cost64`` is the matcher's cost in float64.

The cases are the smallest inputs at which each branch of csrc/matcher.hip's
set_loss_kernel / set_loss_bwd_kernel / lsap_rtdetr_kernel runs: a geometry
table on a dyadic grid (ties, clamp gates, degenerate boxes), a table of
saturated logits, a table of shapes, out-of-range labels and the denoising
layout."""
from __future__ import annotations

import functools
import json
import os
from dataclasses import dataclass, replace

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0          # kernel error allowed, in units of the fp32 torch error of the same case
FLOOR = 2.0 ** -21    # four fp32 ulp: the limit where the fp32 torch error is (near) zero
ALPHA = 0.75          # SetCriterion's VFL alpha
CRIT_W = (1.0, 5.0, 2.0)  # SetCriterion's loss weights (vfl, bbox, giou)


@dataclass(frozen=True)
class Case:
    name: str
    logits: torch.Tensor      # fp32 [S, B, Q, C]
    boxes: torch.Tensor       # fp32 [S, B, Q, 4] cxcywh
    tgt_boxes: torch.Tensor   # fp32 [B, M, 4]
    tgt_labels: torch.Tensor  # int64 [B, M]
    n_valid: torch.Tensor     # int32 [B]
    assign: torch.Tensor      # int32 [S, B, M]
    num_boxes: float
    W: torch.Tensor           # fp32 [S, 3]: weight of every set's (vfl, l1, giou)
    alpha: float = ALPHA

    @property
    def shape(self):
        S, B, Q, C = self.logits.shape
        return S, B, Q, C, self.tgt_boxes.shape[1]

    def args(self):
        return (self.logits, self.boxes, self.tgt_boxes, self.tgt_labels, self.n_valid, self.assign,
                self.num_boxes, self.alpha, self.W)


# ---------------------------------------------------------------------------
# the loss, for a given assignment
# ---------------------------------------------------------------------------
def _xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _area(b):
    return (b[..., 2] - b[..., 0]).clamp(min=0) * (b[..., 3] - b[..., 1]).clamp(min=0)


def _iou_giou(a, b, parts=False):
    """IoU and GIoU of broadcast xyxy boxes, with the criterion's clamps at 0 and 1e-9."""
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = _area(a) + _area(b) - inter
    iou = inter / union.clamp(min=1e-9)
    wh2 = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area = wh2[..., 0] * wh2[..., 1]
    giou = iou - (area - union) / area.clamp(min=1e-9)
    return (iou, giou, union, area) if parts else (iou, giou)


def matched_pairs(n_valid, assign):
    """Index vectors (s, b, m, q) of the pairs the loss counts: m < n_valid[b], assign[s, b, m] >= 0."""
    S, B, M = assign.shape
    valid = (torch.arange(M)[None, :] < n_valid.long()[:, None])[None] & (assign >= 0)
    si, bi, mi = valid.nonzero(as_tuple=True)
    return si, bi, mi, assign.long()[si, bi, mi]


def evaluate(dtype, logits, boxes, tgt_boxes, tgt_labels, n_valid, assign, num_boxes, alpha, W):
    """(comps [S, 3], d logits, d boxes) in ``dtype`` on the CPU: comps = (VFL, L1,
    GIoU loss) / num_boxes per set, the gradients those of (comps * W).sum()."""
    lg = logits.detach().cpu().to(dtype).requires_grad_(True)
    bx = boxes.detach().cpu().to(dtype).requires_grad_(True)
    tb = tgt_boxes.detach().cpu().to(dtype)
    W = torch.as_tensor(W).detach().cpu().to(dtype)
    nb = torch.as_tensor(float(num_boxes)).to(dtype)
    S, B, Q, C = lg.shape
    lab = tgt_labels.cpu().long().clamp(0, C - 1)
    si, bi, mi, qi = matched_pairs(n_valid.cpu(), assign.cpu())
    src, tgt = bx[si, bi, qi], tb[bi, mi]
    iou, giou = _iou_giou(_xyxy(src), _xyxy(tgt))
    l1 = torch.zeros(S, dtype=dtype).index_add(0, si, (src - tgt).abs().sum(-1))
    lgi = torch.zeros(S, dtype=dtype).index_add(0, si, 1.0 - giou)
    score = torch.zeros((S, B, Q, C), dtype=dtype)
    onehot = torch.zeros((S, B, Q, C), dtype=dtype)
    score[si, bi, qi, lab[bi, mi]] = iou.detach()
    onehot[si, bi, qi, lab[bi, mi]] = 1.0
    pred = lg.sigmoid().detach()
    weight = alpha * pred.pow(2) * (1 - onehot) + score
    vfl = F.binary_cross_entropy_with_logits(lg, score, weight=weight, reduction="none").sum((1, 2, 3))
    comps = torch.stack([vfl, l1, lgi], 1) / nb
    g_lg, g_bx = torch.autograd.grad((comps * W).sum(), [lg, bx], allow_unused=True)
    g_lg = torch.zeros_like(lg) if g_lg is None else g_lg
    g_bx = torch.zeros_like(bx) if g_bx is None else g_bx
    return comps.detach(), g_lg, g_bx


def reference(logits, boxes, tgt_boxes, tgt_labels, n_valid, assign, num_boxes, alpha, W):
    return evaluate(torch.float64, logits, boxes, tgt_boxes, tgt_labels, n_valid, assign, num_boxes, alpha, W)


# ---------------------------------------------------------------------------
# the matcher's cost
# ---------------------------------------------------------------------------
def cost(dtype, logits, boxes, tgt_boxes, tgt_labels):
    """HungarianMatcher's cost 5 L1 + 2 (pos - neg) + 2 (-GIoU) -> [S, B, Q, M] in ``dtype``."""
    lg, bx, tb = (t.detach().cpu().to(dtype) for t in (logits, boxes, tgt_boxes))
    S, B, Q, C = lg.shape
    M = tb.shape[1]
    lab = tgt_labels.cpu().long().clamp(0, C - 1)
    p = lg.sigmoid().gather(3, lab[None, :, None, :].expand(S, B, Q, M))
    neg = (1 - 0.25) * p ** 2 * (-(1 - p + 1e-8).log())
    pos = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log())
    c_bbox = (bx[:, :, :, None, :] - tb[None, :, None, :, :]).abs().sum(-1)
    _, giou = _iou_giou(_xyxy(bx)[:, :, :, None, :], _xyxy(tb)[None, :, None, :, :])
    return 5.0 * c_bbox + 2.0 * (pos - neg) + 2.0 * (-giou)


def cost64(logits, boxes, tgt_boxes, tgt_labels):
    return cost(torch.float64, logits, boxes, tgt_boxes, tgt_labels)


def cost_eps(logits, boxes, tgt_boxes, tgt_labels):
    """MARGIN x the largest difference between the fp32 torch cost and cost64."""
    d = (cost(torch.float32, logits, boxes, tgt_boxes, tgt_labels).double()
         - cost64(logits, boxes, tgt_boxes, tgt_labels)).abs()
    return MARGIN * float(d.max())


# ---------------------------------------------------------------------------
# error measure and limits
# ---------------------------------------------------------------------------
def rel_err(got, ref):
    """max over elements of |got - ref| / (|ref| + rms(ref)); where the whole
    reference is zero, 0 if got is too and inf otherwise."""
    got = np.asarray(torch.as_tensor(got).detach().cpu().double().numpy())
    ref = np.asarray(torch.as_tensor(ref).detach().cpu().double().numpy())
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float("inf")
    den = np.abs(ref) + float(np.sqrt((ref ** 2).mean()))
    if float(den.max()) == 0.0:
        return 0.0 if float(err.max()) == 0.0 else float("inf")
    return float((err / np.where(den > 0, den, 1.0)).max())


OUTPUTS = ("comps", "d_logits", "d_boxes")


def figures(got, ref):
    return {k: rel_err(g, r) for k, g, r in zip(OUTPUTS, got, ref)}


def fp32_figures(args, ref=None):
    """Error of the fp32 torch evaluation against the float64 reference, per output."""
    ref = reference(*args) if ref is None else ref
    return figures(evaluate(torch.float32, *args), ref)


def limits(fp32_fig):
    return {k: max(MARGIN * v, FLOOR) for k, v in fp32_fig.items()}


def report(record):
    """With CRITERION_REPORT=<file>: append one JSON line per call (the figures
    of a case, for the tolerance record in test_gpu_criterion_edges.py)."""
    path = os.environ.get("CRITERION_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


# ---------------------------------------------------------------------------
# geometry table (units of 1/64): (name, source cxcywh, target cxcywh)
# ---------------------------------------------------------------------------
_T = (32, 32, 16, 16)  # x 24..40, y 24..40
GEOMETRY_ROWS = [
    ("identical", (32, 32, 16, 16), _T),
    ("shared_left_edge", (28, 30, 8, 8), _T),           # x 24..32, y 26..34
    ("shared_right_top_edge", (36, 28, 8, 8), _T),      # x 32..40, y 24..32
    ("source_inside", (32, 32, 8, 8), _T),
    ("target_inside", (32, 32, 32, 32), _T),
    ("touch_edge", (44, 32, 8, 8), _T),                 # x 40..48: iw == 0
    ("touch_corner", (44, 44, 8, 8), _T),               # iw == ih == 0
    ("disjoint_x", (52, 32, 8, 8), _T),                 # iw < 0
    ("disjoint_y", (32, 52, 8, 8), _T),
    ("disjoint_xy", (52, 52, 8, 8), _T),
    ("zero_width_source", (32, 32, 0, 8), _T),
    ("zero_area_target", (30, 30, 8, 8), (32, 32, 0, 0)),
    ("negative_width_source", (32, 32, -8, 8), _T),     # aw < 0
    ("general_overlap", (37, 35, 14, 8), _T),           # x 30..44, y 31..39: no tie, the control row
]
# the 1e-9 clamps, not on the grid: (name, source, target) in absolute units.
# The second pair is half the size of the first: at 1e-5 its union would be 2e-10,
# inside the band that the table keeps clear of the 1e-9 threshold.
TINY_ROWS = [
    ("tiny_coincident", (0.0, 0.0, 1e-5, 1e-5), (0.0, 0.0, 1e-5, 1e-5)),   # uni, area < 1e-9
    ("tiny_apart", (0.0, 0.0, 5e-6, 5e-6), (0.75, 0.75, 5e-6, 5e-6)),      # uni < 1e-9 <= area
]
N_DYADIC = len(GEOMETRY_ROWS)
GEOMETRY_NUM_BOXES = 32.0  # a power of two: W / num_boxes is exact in any order


def _swap_xy(b):
    return b[..., [1, 0, 3, 2]]


def _W(S, seed):
    """[S, 3] distinct weights, all exactly fp32 (multiples of 1/16 in [0.5, 4))."""
    rng = np.random.default_rng(1000 + seed)
    v = rng.choice(np.arange(8, 64), size=S * 3, replace=False) / 16.0
    return torch.from_numpy(v.reshape(S, 3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def geometry_case() -> Case:
    """B = 2 (image 1: x and y exchanged), S = 2 (set 1: every source reflected
    about its target's centre, which turns a shared left edge into a shared
    right edge), M = rows, Q = 2 M, assign[m] = 2 m, C = 2."""
    rng = np.random.default_rng(7)
    src = np.array([r[1] for r in GEOMETRY_ROWS], np.float64) / 64.0
    tgt = np.array([r[2] for r in GEOMETRY_ROWS], np.float64) / 64.0
    src = np.concatenate([src, np.array([r[1] for r in TINY_ROWS])])
    tgt = np.concatenate([tgt, np.array([r[2] for r in TINY_ROWS])])
    src, tgt = torch.from_numpy(src).float(), torch.from_numpy(tgt).float()
    M = src.shape[0]
    S, B, Q, C = 2, 2, 2 * M, 2
    refl = src.clone()
    refl[:, :2] = 2 * tgt[:, :2] - src[:, :2]
    tb = torch.stack([tgt, _swap_xy(tgt)])
    boxes = torch.empty(S, B, Q, 4)
    boxes[:, :, 1::2] = torch.from_numpy(rng.integers(4, 57, (S, B, M, 4)) / 64.0).float()
    for s, sb in enumerate((src, refl)):
        boxes[s, 0, 0::2] = sb
        boxes[s, 1, 0::2] = _swap_xy(sb)
    logits = torch.from_numpy(rng.integers(-32, 33, (S, B, Q, C)) / 8.0).float()
    labels = (torch.arange(M) % 2).expand(B, M).contiguous()
    assign = (2 * torch.arange(M, dtype=torch.int32)).expand(S, B, M).contiguous()
    return Case("geometry", logits, boxes, tb, labels, torch.tensor([M, M], dtype=torch.int32), assign,
                GEOMETRY_NUM_BOXES, _W(S, 1))


def geometry_parts(case: Case, dtype):
    """(union, enclosing area) [S, B, M] of the table's matched pairs in ``dtype``."""
    q = case.assign.long()
    src = case.boxes.to(dtype).gather(2, q[..., None].expand(*q.shape, 4))
    tgt = case.tgt_boxes.to(dtype)[None].expand_as(src)
    _, _, union, area = _iou_giou(_xyxy(src), _xyxy(tgt), parts=True)
    return union, area


# ---------------------------------------------------------------------------
# logit table
# ---------------------------------------------------------------------------
LOGIT_VALUES = [0.0] + [sgn * v for v in (1e-4, 5.0, 17.0, 30.0, 88.0, 89.0, 104.0, 200.0) for sgn in (1.0, -1.0)]


@functools.lru_cache(maxsize=None)
def logit_case() -> Case:
    """Every value of LOGIT_VALUES on a matched entry with IoU 0 (touching
    boxes), a mid IoU and IoU 1, on the other class of a matched query and on
    unmatched queries.  B = 1, C = 2, M = 3 x 17, Q = 2 M, assign[m] = 2 m;
    set 1 holds the same values rotated by 7."""
    rng = np.random.default_rng(8)
    V = torch.tensor(LOGIT_VALUES, dtype=torch.float32)
    n = len(LOGIT_VALUES)
    M = 3 * n
    S, B, Q, C = 2, 1, 2 * M, 2
    labels = (torch.arange(M) % 2)[None].contiguous()
    tgt = torch.tensor([0.5, 0.5, 0.25, 0.25]).expand(B, M, 4).contiguous()
    kinds = torch.tensor([[0.75, 0.5, 0.25, 0.25],      # touching at an edge: IoU exactly 0
                          [0.5625, 0.5, 0.25, 0.25],    # IoU 0.6
                          [0.5, 0.5, 0.25, 0.25]])      # IoU exactly 1
    boxes = torch.from_numpy(rng.integers(8, 49, (S, B, Q, 4)) / 64.0).float()
    boxes[:, :, 0::2] = kinds.repeat_interleave(n, 0)
    logits = torch.empty(S, B, Q, C)
    m = torch.arange(M)
    for s in range(S):
        r = 7 * s
        logits[s, 0, 2 * m, labels[0]] = V[(m + r) % n]            # the matched entry
        logits[s, 0, 2 * m, 1 - labels[0]] = V[(m + r + 5) % n]    # background on a matched query
        logits[s, 0, 2 * m + 1, 0] = V[(m + r + 3) % n]            # background queries
        logits[s, 0, 2 * m + 1, 1] = V[(m + r + 11) % n]
    assign = (2 * torch.arange(M, dtype=torch.int32)).expand(S, B, M).contiguous()
    return Case("logits", logits, boxes, tgt, labels, torch.tensor([M], dtype=torch.int32), assign, float(M),
                _W(S, 2))


# ---------------------------------------------------------------------------
# shape table: random inputs in general position, as the existing tests draw them
# ---------------------------------------------------------------------------
SHAPE_ROWS = [
    (1, 1, 1, 1, 1, (1,)),
    (1, 1, 7, 1, 8, (7,)),
    (2, 3, 65, 5, 9, (0, 9, 4)),           # C > 4: the logits side of the backward's grid is the longer
    (3, 2, 255, 8, 4, (0, 0)),             # all images empty, num_boxes = 1
    (2, 2, 300, 1, 200, (200, 131)),       # B M > 256 (strided pair loop), M > 64
    (1, 4, 256, 16, 3, (3, 0, 1, 2)),      # B Q C 4 == 65536: the largest LDS score map
    (2, 2, 64, 80, 16, (16, 5)),           # COCO's class count
]
SQUARE_ROW = (2, 2, 8, 3, 8, (8, 8))       # n == Q: the solver's non-transposed branch
INTEGRATION_ROW = SHAPE_ROWS[2]


def row_id(row):
    return "S{}B{}Q{}C{}M{}".format(*row[:5])


def draw(row, seed=0):
    """(logits, boxes, tgt_boxes, tgt_labels, n_valid) of a shape row."""
    S, B, Q, C, M, nv = row
    g = torch.Generator().manual_seed(100 + seed + 7 * S + 11 * B + 13 * Q + 17 * C + 19 * M)
    logits = torch.randn(S, B, Q, C, generator=g).clamp(-8, 8)
    boxes = torch.rand(S, B, Q, 4, generator=g) * 0.5 + 0.2
    tb = torch.rand(B, M, 4, generator=g) * 0.4 + 0.3
    tl = torch.randint(0, C, (B, M), generator=g)
    return logits, boxes, tb, tl, torch.tensor(nv, dtype=torch.int32)


def random_assign(S, B, Q, M, seed):
    """A seeded injective assignment [S, B, M] (-1 where Q < M runs out): the
    padded slots m >= n_valid[b] name queries too, which the loss must ignore."""
    g = torch.Generator().manual_seed(500 + seed)
    a = torch.full((S, B, M), -1, dtype=torch.int32)
    for s in range(S):
        for b in range(B):
            p = torch.randperm(Q, generator=g)[:M].to(torch.int32)
            a[s, b, :len(p)] = p
    return a


@functools.lru_cache(maxsize=None)
def shape_case(row) -> Case:
    S, B, Q, C, M, nv = row
    logits, boxes, tb, tl, n_valid = draw(row)
    return Case(row_id(row), logits, boxes, tb, tl, n_valid, random_assign(S, B, Q, M, Q + M),
                float(max(sum(nv), 1)), _W(S, 10 + Q))


LABEL_ROW = (2, 2, 16, 3, 6, (6, 4))


@functools.lru_cache(maxsize=None)
def label_case() -> Case:
    """Labels -1 and C among the targets: they count as 0 and C - 1."""
    c = shape_case(LABEL_ROW)
    C = LABEL_ROW[3]
    tl = torch.tensor([[-1, 0, C, 2, 1, -1], [C, C, -1, 1, 0, 2]], dtype=torch.int64)
    return replace(c, name="labels", tgt_labels=tl)


# ---------------------------------------------------------------------------
# denoising layout
# ---------------------------------------------------------------------------
DN = dict(S=2, G=3, B=2, M=5, C=3, n_valid=(5, 2))


def dn_per_group(t, G):
    """[S, B, G 2M, .] -> [S G, B, 2M, .]: every group as its own prediction set."""
    S, B, Qdn, K = t.shape
    return t.view(S, B, G, Qdn // G, K).permute(0, 2, 1, 3, 4).reshape(S * G, B, Qdn // G, K)


def dn_from_groups(t, G):
    """The inverse of dn_per_group."""
    SG, B, Q2, K = t.shape
    return t.view(SG // G, G, B, Q2, K).permute(0, 2, 1, 3, 4).reshape(SG // G, B, G * Q2, K)


@functools.lru_cache(maxsize=None)
def dn_case():
    """(case in the per-group view, coefficients [S, 3] of the returned losses):
    the test sums dn_losses' components with distinct coefficients, so the
    reference's W is coefficient x criterion weight / G on every group's set."""
    S, G, B, M, C = (DN[k] for k in "SGBMC")
    logits, boxes, tb, tl, n_valid = draw((S, B, 2 * M * G, C, M, DN["n_valid"]), seed=3)
    coef = _W(S, 3)
    W = (coef * torch.tensor(CRIT_W)).repeat_interleave(G, 0) / G
    assign = torch.arange(M, dtype=torch.int32).expand(S * G, B, M).contiguous()
    case = Case("denoising", dn_per_group(logits, G).contiguous(), dn_per_group(boxes, G).contiguous(), tb, tl,
                n_valid, assign, float(sum(DN["n_valid"])), W)
    return case, coef


def loss_cases():
    """Every case of the loss kernels' table, by name."""
    cases = [geometry_case(), logit_case()] + [shape_case(r) for r in SHAPE_ROWS] + [label_case(), dn_case()[0]]
    return {c.name: c for c in cases}


LOSS_CASE_NAMES = ["geometry", "logits"] + [row_id(r) for r in SHAPE_ROWS] + ["labels", "denoising"]
MATCH_ROWS = SHAPE_ROWS + [SQUARE_ROW, LABEL_ROW]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(float64 reference, fp32 torch figures) of a table case, computed once."""
    c = loss_cases()[name]
    ref = reference(*c.args())
    return ref, fp32_figures(c.args(), ref)


def match_inputs(row):
    """Matcher inputs of a row: the shape row's draw; the label row with its out-of-range labels."""
    if row == LABEL_ROW:
        c = label_case()
        return c.logits, c.boxes, c.tgt_boxes, c.tgt_labels, c.n_valid
    return draw(row)
