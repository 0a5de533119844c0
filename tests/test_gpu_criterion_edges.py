"""The fused set criterion (csrc/matcher.hip: lsap_rtdetr_kernel,
set_loss_kernel, set_loss_bwd_kernel) against the float64 reference of
tests/criterion_cases.py, on the tables built there: tie and clamp-gate
geometry on a dyadic grid, saturated logits, the shapes at which the kernels
change path, out-of-range labels, the denoising layout, the matcher's
optimality and its failure reports, and SetCriterion.loss_padded end to end.

Tolerance.  Per case and output, err = max |got - ref| / (|ref| + rms(ref))
against the float64 reference may be at most MARGIN = 4 times the same figure
of the fp32 torch evaluation of the same formula on the CPU (4x is assumed: a
few ulp of expf/logf and another reduction tree), and never less than
FLOOR = 2^-21 (four fp32 ulp).  The matcher's assignment may cost, in cost64,
at most 2 n eps more than scipy's optimum, eps = 4 x max |fp32 torch cost -
cost64|.

Measured on an MI355X (kernel err / limit, per output; CRITERION_REPORT=<file>
writes these lines):

  case              comps              d logits           d boxes
  geometry          3.1e-08 / 4.8e-07  1.4e-07 / 6.9e-07  2.3e-08 / 4.8e-07
  geometry, dyadic rows against their own rms             5.2e-08 / 4.8e-07
  logits            4.3e-08 / 4.8e-07  1.2e-07 / 4.8e-07  5.6e-08 / 4.8e-07
  S1B1Q1C1M1        2.3e-08 / 4.8e-07  3.6e-07 / 1.6e-06  4.5e-08 / 4.8e-07
  S1B1Q7C1M8        5.1e-08 / 4.8e-07  4.0e-07 / 1.6e-06  8.0e-08 / 4.8e-07
  S2B3Q65C5M9       1.3e-08 / 4.8e-07  2.6e-07 / 1.0e-06  1.4e-07 / 5.1e-07
  S3B2Q255C8M4      8.0e-08 / 4.8e-07  2.3e-07 / 1.0e-06  0       / 4.8e-07
  S2B2Q300C1M200    4.7e-08 / 1.0e-06  8.2e-07 / 3.4e-06  3.6e-07 / 1.4e-06
  S1B4Q256C16M3     4.1e-08 / 4.8e-07  2.6e-07 / 9.5e-07  1.7e-07 / 8.6e-07
  S2B2Q64C80M16     5.8e-08 / 4.8e-07  3.0e-07 / 1.0e-06  1.1e-07 / 4.8e-07
  labels            3.3e-08 / 4.8e-07  3.5e-07 / 1.7e-06  1.9e-07 / 4.8e-07
  denoising         5.8e-08 / 4.8e-07  2.4e-07 / 8.5e-07  1.5e-07 / 4.8e-07
  loss_padded       6.6e-08 / 4.8e-07  4.0e-07 / 2.3e-06  1.5e-07 / 4.8e-07

Every kernel figure is below the floor or below 1.2x the fp32 torch figure of
its case: nothing comes near the 4x margin.  The matcher's
assignments cost at most 3e-14 more than scipy's optimum on cost64 (allowed:
9e-7 at n = 1 to 3e-3 at n = 200).
"""
import numpy as np
import pytest
import torch

import criterion_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(case):
    return dict(tb=case.tgt_boxes.to(DEV), tl=case.tgt_labels.to(DEV), nv=case.n_valid.to(DEV),
                nb=torch.tensor(case.num_boxes, dtype=torch.float32, device=DEV), assign=case.assign.to(DEV))


def _run_loss(case, W=None, tgt_labels=None):
    """(comps, d logits, d boxes) of (comps * W).sum() through _SetLossHip with the case's assignment."""
    from src.rtdetr_moe.criterion import _SetLossHip

    d = _dev(case)
    lg = case.logits.to(DEV).requires_grad_(True)
    bx = case.boxes.to(DEV).requires_grad_(True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    tl = d["tl"] if tgt_labels is None else tgt_labels.to(DEV)
    comps, assign = _SetLossHip.apply(lg, bx, d["tb"], tl, d["nv"], d["nb"], status, case.alpha, d["assign"])
    assert torch.equal(assign, d["assign"]) and int(status.item()) == 0
    W = case.W if W is None else W
    g_lg, g_bx = torch.autograd.grad((comps * W.to(DEV)).sum(), [lg, bx])
    torch.cuda.synchronize()
    return comps.detach().cpu(), g_lg.cpu(), g_bx.cpu()


def _check(name, got, ref, fig32):
    fig = cc.figures(got, ref)
    lim = cc.limits(fig32)
    cc.report({"case": name, "side": "kernel", **fig, "limits": lim})
    print(name, "kernel", fig, "fp32 torch", fig32, "limits", lim)
    for k in cc.OUTPUTS:
        assert fig[k] <= lim[k], f"{name} {k}: {fig[k]:.3e} > {lim[k]:.3e} (fp32 torch {fig32[k]:.3e})"


def _unmatched_rows(case):
    """bool [S, B, Q]: box rows no valid slot is assigned to (the padded slots' queries among them)."""
    S, B, Q, _, _ = case.shape
    si, bi, _, qi = cc.matched_pairs(case.n_valid, case.assign)
    free = torch.ones(S, B, Q, dtype=torch.bool)
    free[si, bi, qi] = False
    return free


@pytest.mark.parametrize("name", [n for n in cc.LOSS_CASE_NAMES if n != "denoising"])
def test_loss_and_gradients_match_fp64(hip_lib, name):
    case = cc.loss_cases()[name]
    ref, fig32 = cc.case_reference(name)
    got = _run_loss(case)
    free = _unmatched_rows(case)
    S, B, _, _, M = case.shape
    padded = torch.arange(M)[None, :] >= case.n_valid.long()[:, None]  # [B, M]: slots m >= n_valid[b]
    for s in range(S):  # the queries they name are unmatched rows (the tables assign injectively)
        for b, m in padded.nonzero().tolist():
            assert case.assign[s, b, m] < 0 or free[s, b, case.assign[s, b, m]]
    assert bool((got[2][free] == 0).all()), "box gradient on an unmatched query or a padded slot's query"
    _check(name, got, ref, fig32)


def test_geometry_dyadic_rows_on_their_own_scale(hip_lib):
    """The two tiny rows' GIoU gradients (~1e4: the union clamped to 1e-9)
    dominate rms(d boxes) of the whole table; the dyadic rows' box gradients
    are judged here against their own rms, so that a wrong tie half or gate in
    an O(1) gradient cannot hide under it."""
    case = cc.geometry_case()
    n = cc.N_DYADIC
    ref = cc.reference(*case.args())
    f32 = cc.evaluate(torch.float32, *case.args())
    got = _run_loss(case)

    def dyadic(t):
        return t[:, :, 0::2][:, :, :n]

    e32, e = cc.rel_err(dyadic(f32[2]), dyadic(ref[2])), cc.rel_err(dyadic(got[2]), dyadic(ref[2]))
    lim = max(cc.MARGIN * e32, cc.FLOOR)
    cc.report({"case": "geometry_dyadic", "side": "kernel", "d_boxes": e, "fp32_torch": e32, "limit": lim})
    print("geometry_dyadic d_boxes kernel", e, "fp32 torch", e32, "limit", lim)
    assert e <= lim


def test_geometry_l1_gradient_is_exact(hip_lib):
    """On the dyadic rows dx is exact, so d L1 is sign(dx) W[s, 1] / num_boxes bit
    for bit (num_boxes a power of two), 0 where the coordinates are equal."""
    case = cc.geometry_case()
    W = case.W.clone()
    W[:, 0] = 0
    W[:, 2] = 0
    _, _, ref_bx = cc.reference(*case.args()[:-1], W)
    _, _, g_bx = _run_loss(case, W)
    n = cc.N_DYADIC
    got, want = g_bx[:, :, 0::2][:, :, :n].double(), ref_bx[:, :, 0::2][:, :, :n]
    step = (case.W[:, 1].double() / case.num_boxes)[:, None, None, None]
    assert bool(((want == 0) | (want.abs() == step)).all()) and bool((want == 0).any())
    assert torch.equal(got, want)


def test_out_of_range_labels_are_clamped(hip_lib):
    """Labels -1 and C give the bits of labels 0 and C - 1."""
    case = cc.label_case()
    C = case.shape[3]
    raw = _run_loss(case)
    clamped = _run_loss(case, tgt_labels=case.tgt_labels.clamp(0, C - 1))
    for a, b in zip(raw, clamped):
        assert torch.equal(a, b)


def test_denoising_layout_through_dn_losses(hip_lib):
    """SetCriterion.dn_losses(fused=True), every returned loss under its own coefficient."""
    from src.rtdetr_moe.criterion import SetCriterion

    case, coef = cc.dn_case()
    S, G, C = cc.DN["S"], cc.DN["G"], cc.DN["C"]
    lg_full, bx_full = cc.dn_from_groups(case.logits, G), cc.dn_from_groups(case.boxes, G)
    outs = [{"pred_logits": lg_full[s].to(DEV).requires_grad_(True),
             "pred_boxes": bx_full[s].to(DEV).requires_grad_(True)} for s in range(S)]
    crit = SetCriterion(num_classes=C)
    assert crit.dn_fused_ok(outs, cc.DN["M"]) and crit.alpha == case.alpha
    losses = crit.dn_losses(outs, case.tgt_boxes.to(DEV), case.tgt_labels.to(DEV), case.n_valid.to(DEV),
                            case.num_boxes, G, fused=True)
    keys = [[k + sfx for k in ("loss_vfl", "loss_bbox", "loss_giou")] for sfx in crit._dn_names(S)]
    assert set(losses) == {k for row in keys for k in row}
    total = sum(float(coef[s, k]) * losses[keys[s][k]] for s in range(S) for k in range(3))
    leaves = [t for o in outs for t in (o["pred_logits"], o["pred_boxes"])]
    grads = torch.autograd.grad(total, leaves)
    torch.cuda.synchronize()

    def per_layer(comps):  # per-group comps [S G, 3] -> the weighted losses dn_losses returns [S, 3]
        return comps.view(S, G, 3).sum(1) / G * torch.tensor(cc.CRIT_W, dtype=comps.dtype)

    got = (torch.stack([torch.stack([losses[k].detach() for k in row]) for row in keys]).cpu(),
           cc.dn_per_group(torch.stack(grads[0::2]).cpu(), G), cc.dn_per_group(torch.stack(grads[1::2]).cpu(), G))
    ref = cc.reference(*case.args())
    f32 = cc.evaluate(torch.float32, *case.args())
    ref = (per_layer(ref[0]), ref[1], ref[2])
    fig32 = cc.figures((per_layer(f32[0]), f32[1], f32[2]), ref)
    pad = torch.arange(cc.DN["M"])[None, :] >= case.n_valid.long()[:, None]  # [B, M]: slot m is query m of a group
    assert bool((got[2][:, :, :cc.DN["M"]][:, pad] == 0).all()) and bool((got[2][:, :, cc.DN["M"]:] == 0).all())
    _check("denoising", got, ref, fig32)


# ---------------------------------------------------------------------------
# the fused matcher
# ---------------------------------------------------------------------------
def _run_match(logits, boxes, tb, tl, nv):
    """(assign [S, B, M] on the host, status) of one rtdetr_set_criterion_match launch."""
    from src.moe import _lib as L

    S, B, Q, C = logits.shape
    M = tb.shape[1]
    lg, bx, tbd = (t.to(DEV).float().contiguous() for t in (logits, boxes, tb))
    tld, nvd = tl.to(DEV).to(torch.int32).contiguous(), nv.to(DEV).to(torch.int32).contiguous()
    assign = torch.full((S, B, M), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    L._check(L.lib().rtdetr_set_criterion_match(lg.data_ptr(), bx.data_ptr(), tbd.data_ptr(), tld.data_ptr(),
                                                nvd.data_ptr(), S, B, Q, C, M, assign.data_ptr(),
                                                status.data_ptr(), L._stream()), "rtdetr_set_criterion_match")
    torch.cuda.synchronize()
    return assign.cpu(), int(status.item())


def _assert_valid_assignment(a, n, Q):
    """One problem's row [M]: n distinct queries in [0, Q), then -1."""
    assert bool((a[n:] == -1).all()), a
    q = a[:n]
    assert bool(((q >= 0) & (q < Q)).all()) and q.unique().numel() == n, a


@pytest.mark.parametrize("row", cc.MATCH_ROWS, ids=cc.row_id)
def test_fused_matcher_is_optimal(hip_lib, row):
    from scipy.optimize import linear_sum_assignment

    S, B, Q, C, M, nv = row
    inputs = cc.match_inputs(row)
    assert float(inputs[0].abs().max()) <= 8.0
    assign, status = _run_match(*inputs)
    assert status == 0
    again, _ = _run_match(*inputs)
    assert torch.equal(assign, again)
    c64 = cc.cost64(*inputs[:4]).numpy()
    eps = cc.cost_eps(*inputs[:4])
    for s in range(S):
        for b in range(B):
            n = nv[b]
            _assert_valid_assignment(assign[s, b], n, Q)
            if n == 0:
                continue
            c = c64[s, b, :, :n]
            r, col = linear_sum_assignment(c)
            best = float(c[r, col].sum())
            got = float(c[assign[s, b, :n].numpy(), np.arange(n)].sum())
            print(cc.row_id(row), s, b, "excess", got - best, "allowed", 2 * n * eps)
            assert best - 1e-9 <= got <= best + 2 * n * eps, (s, b, got, best, eps)


def test_fused_matcher_reports_too_many_targets(hip_lib):
    """n_valid > Q in one image: status 1, that image all -1, the others matched as without it."""
    row = (2, 3, 4, 2, 8, (3, 6, 2))
    logits, boxes, tb, tl, nv = cc.draw(row)
    assign, status = _run_match(logits, boxes, tb, tl, nv)
    assert status == 1
    assert bool((assign[:, 1] == -1).all())
    clean, status0 = _run_match(logits, boxes, tb, tl, torch.tensor([3, 0, 2], dtype=torch.int32))
    assert status0 == 0 and torch.equal(assign, clean)
    for s in range(2):
        for b in (0, 2):
            _assert_valid_assignment(assign[s, b], row[5][b], row[2])


@pytest.mark.parametrize("poison", ["nan_logits", "inf_boxes"])
def test_fused_matcher_reports_non_finite_costs(hip_lib, poison):
    """One (s, b) whose costs are all NaN / +inf: status 2, every other problem as in the clean launch."""
    row = (2, 2, 8, 2, 4, (3, 4))
    logits, boxes, tb, tl, nv = cc.draw(row)
    clean, status0 = _run_match(logits, boxes, tb, tl, nv)
    assert status0 == 0
    logits, boxes = logits.clone(), boxes.clone()
    if poison == "nan_logits":
        logits[1, 0] = float("nan")
    else:
        boxes[1, 0] = float("inf")
    assign, status = _run_match(logits, boxes, tb, tl, nv)
    assert status == 2
    for s, b in ((0, 0), (0, 1), (1, 1)):
        assert torch.equal(assign[s, b], clean[s, b])


# ---------------------------------------------------------------------------
# SetCriterion.loss_padded: kernel matching, then kernel loss
# ---------------------------------------------------------------------------
def test_loss_padded_end_to_end(hip_lib, monkeypatch):
    from src.rtdetr_moe import criterion as crit_mod
    from src.rtdetr_moe.criterion import SetCriterion

    row = cc.INTEGRATION_ROW
    S, B, Q, C, M, nv = row
    logits, boxes, tb, tl, n_valid = cc.draw(row)
    sets = [{"pred_logits": logits[s].to(DEV).requires_grad_(True),
             "pred_boxes": boxes[s].to(DEV).requires_grad_(True)} for s in range(S)]
    outputs = dict(sets[0], aux_outputs=sets[1:])
    crit = SetCriterion(num_classes=C)
    assert crit.fused_ok(outputs, M)
    returned = []
    apply = crit_mod._SetLossHip.apply

    def spy(*args):
        out = apply(*args)
        returned.append(out[1])
        return out

    monkeypatch.setattr(crit_mod._SetLossHip, "apply", staticmethod(spy))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nb = float(sum(nv))
    total, parts = crit.loss_padded(outputs, tb.to(DEV), tl.to(DEV), n_valid.to(DEV),
                                    torch.tensor(nb, device=DEV), status)
    leaves = [t for o in sets for t in (o["pred_logits"], o["pred_boxes"])]
    grads = torch.autograd.grad(total, leaves)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and len(returned) == 1
    assign = returned[0].cpu()
    for s in range(S):
        for b in range(B):
            _assert_valid_assignment(assign[s, b], nv[b], Q)
    W = torch.tensor(cc.CRIT_W).expand(S, 3)
    args = (logits, boxes, tb, tl, n_valid, assign, nb, crit.alpha, W)
    ref = cc.reference(*args)
    f32 = cc.evaluate(torch.float32, *args)
    names = [k + sfx for sfx in [""] + [f"_aux{i}" for i in range(S - 1)]
             for k in ("loss_vfl", "loss_bbox", "loss_giou")]
    assert set(parts) == set(names)
    weighted = torch.stack([parts[k] for k in names]).cpu().view(S, 3)
    got = (weighted, torch.stack(grads[0::2]).cpu(), torch.stack(grads[1::2]).cpu())
    ref = (ref[0] * W.double(), ref[1], ref[2])
    fig32 = cc.figures((f32[0] * W, f32[1], f32[2]), ref)
    _check("loss_padded", got, ref, fig32)
    assert cc.rel_err(total.detach().cpu(), ref[0].sum()) <= cc.limits(fig32)["comps"]
