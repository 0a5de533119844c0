"""Contrastive denoising queries (src/rtdetr_moe/denoising.py), their decoder
path and their losses, on the CPU in fp32: shapes and index layout, the
segment ids against upstream RT-DETR's boolean attention mask, the noise
model, the spec token, decoder isolation and SetCriterion.dn_losses against
the reference loss formulation."""
from __future__ import annotations

import pytest
import torch

from src.moe.config import parse_moe_spec
from src.rtdetr_moe.criterion import PAD_BOX, SetCriterion, box_cxcywh_to_xyxy, pad_targets
from src.rtdetr_moe.denoising import DenoisingConfig, dn_index, dn_shapes, make_denoising, segments
from src.rtdetr_moe.linear import segment_mask

SPEC = "rtdetr-r18-moe4-top2-dn100"


def test_group_count_and_query_count():
    assert dn_shapes(16, 100) == (6, 192)
    assert dn_shapes(128, 100) == (1, 256)
    assert dn_shapes(32, 100) == (3, 192)


def test_index_layout_and_segments():
    G, M, Q = 3, 4, 5
    seg = segments(G, M, Q)
    assert seg.dtype == torch.int32 and seg.shape == (2 * M * G + Q,)
    seen = set()
    for g in range(G):
        for h in range(2):
            for j in range(M):
                i = dn_index(g, h, j, M)
                assert i == g * 2 * M + h * M + j
                assert int(seg[i]) == g
                seen.add(i)
    assert seen == set(range(2 * M * G))
    assert (seg[2 * M * G:] == -1).all()


def _upstream_mask(max_gt_num, num_group, num_queries):
    """RT-DETR's get_contrastive_denoising_training_group, the attention mask
    part, written out (True = the query row must NOT see the key column)."""
    num_denoising = max_gt_num * 2 * num_group
    tgt_size = num_denoising + num_queries
    attn_mask = torch.full([tgt_size, tgt_size], False, dtype=torch.bool)
    # match query cannot see the reconstruction
    attn_mask[num_denoising:, :num_denoising] = True
    # reconstruct cannot see each other
    for i in range(num_group):
        if i == 0:
            attn_mask[max_gt_num * 2 * i: max_gt_num * 2 * (i + 1), max_gt_num * 2 * (i + 1): num_denoising] = True
        if i == num_group - 1:
            attn_mask[max_gt_num * 2 * i: max_gt_num * 2 * (i + 1), :max_gt_num * i * 2] = True
        else:
            attn_mask[max_gt_num * 2 * i: max_gt_num * 2 * (i + 1), max_gt_num * 2 * (i + 1): num_denoising] = True
            attn_mask[max_gt_num * 2 * i: max_gt_num * 2 * (i + 1), :max_gt_num * 2 * i] = True
    return attn_mask


@pytest.mark.parametrize("M,G,Q", [(12, 4, 40), (16, 6, 300), (32, 1, 1)])
def test_segments_reproduce_upstream_mask(M, G, Q):
    visible = segment_mask(segments(G, M, Q))
    assert torch.equal(visible, ~_upstream_mask(M, G, Q))
    assert visible.diagonal().all()  # no fully masked row


def _targets():
    """Boxes away from the border: centre in [0.4, 0.6], size in [0.05, 0.15],
    so that corners moved by up to 2 x half a side stay inside [0, 1]."""
    g = torch.Generator().manual_seed(0)
    counts = [5, 0, 16]
    tg = [{"boxes": torch.cat([torch.rand(n, 2, generator=g) * 0.2 + 0.4,
                               torch.rand(n, 2, generator=g) * 0.1 + 0.05], -1),
           "labels": torch.randint(0, 3, (n,), generator=g)} for n in counts]
    return tg, counts


def test_make_denoising_noise_model():
    tg, counts = _targets()
    M, C = 16, 3
    G, Qdn = dn_shapes(M, 100)
    tb, tl, nv = pad_targets(tg, M)
    cfg = DenoisingConfig(label_noise_ratio=0.5, box_noise_scale=1.0)
    lab, unact = make_denoising(tb, tl, nv, C, G, cfg, torch.Generator().manual_seed(7))
    lab2, unact2 = make_denoising(tb, tl, nv, C, G, cfg, torch.Generator().manual_seed(7))
    lab3, unact3 = make_denoising(tb, tl, nv, C, G, cfg, torch.Generator().manual_seed(8))
    assert torch.equal(lab, lab2) and torch.equal(unact, unact2)  # same seed, same tensors
    assert not torch.equal(unact, unact3)
    B = len(counts)
    assert lab.shape == (B, Qdn) and lab.dtype == torch.int64
    assert unact.shape == (B, Qdn, 4) and unact.dtype == torch.float32
    assert torch.isfinite(unact).all()
    out_l = torch.empty_like(lab)
    out_u = torch.empty_like(unact)
    r = make_denoising(tb, tl, nv, C, G, cfg, torch.Generator().manual_seed(7), out=(out_l, out_u))
    assert r[0] is out_l and r[1] is out_u and torch.equal(out_l, lab) and torch.equal(out_u, unact)
    boxes = unact.sigmoid().view(B, G, 2, M, 4)
    labels = lab.view(B, G, 2, M)
    pad = torch.tensor(PAD_BOX)
    n_flipped = n_valid_slots = 0
    for b, n in enumerate(counts):
        # padded slots: class num_classes, the un-noised PAD_BOX
        assert (labels[b, :, :, n:] == C).all()
        assert torch.allclose(boxes[b, :, :, n:], pad.expand(G, 2, M - n, 4), atol=1e-6)
        if n == 0:
            continue
        gt = box_cxcywh_to_xyxy(tb[b, :n])                      # [n, 4]
        half = torch.cat([tb[b, :n, 2:], tb[b, :n, 2:]], -1) * 0.5 * cfg.box_noise_scale
        d = (box_cxcywh_to_xyxy(boxes[b, :, :, :n]) - gt).abs()  # [G, 2, n, 4]
        tol = 1e-5
        assert (d[:, 0] <= half + tol).all()                     # positives: r in [0, 1)
        # negatives: r in [1, 2).  Two corners moved towards each other by more
        # than half a side each cross, and the side is then clipped at 0 (as
        # upstream's): only sides that kept a positive length show their corners
        neg = boxes[b, :, 1, :n]
        kept = torch.stack([neg[..., 2], neg[..., 3], neg[..., 2], neg[..., 3]], -1) > 1e-4
        assert kept.float().mean() > 0.5
        assert (d[:, 1] >= half - tol)[kept].all() and (d[:, 1] <= 2 * half + tol)[kept].all()
        assert ((d[:, 1] > half + tol) & kept).any()
        assert d[:, 0].max() > 0
        assert (labels[b, :, :, :n] >= 0).all() and (labels[b, :, :, :n] < C).all()
        n_flipped += int((labels[b, :, :, :n] != tl[b, :n]).sum())
        n_valid_slots += G * 2 * n
    # redrawn with probability 1/4, 2/3 of the draws differ: ~1/6 of 252 slots
    assert 0 < n_flipped < n_valid_slots // 2
    # no noise at all: the targets themselves
    lab0, unact0 = make_denoising(tb, tl, nv, C, G, DenoisingConfig(0.0, 0.0), torch.Generator().manual_seed(1))
    assert torch.allclose(unact0.sigmoid().view(B, G, 2, M, 4)[2, 1, 0], tb[2], atol=1e-6)
    assert torch.equal(lab0.view(B, G, 2, M)[2, 3, 1], tl[2])


def test_spec_token():
    assert parse_moe_spec(SPEC).num_denoising == 100
    assert parse_moe_spec("rtdetr-r18-moe4-top2").num_denoising == 0
    assert parse_moe_spec("rtdetr-r50-dn200-moe8").num_denoising == 200


@pytest.fixture(scope="module")
def decoder_run():
    """One R18 model with denoising (capacity factor 0: no token can displace
    another), one batch, run in training mode without and with a dn pack."""
    from src.rtdetr_moe.data import SyntheticZOD
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC)
    assert model.spec.moe.capacity_factor == 0
    model.train()
    images, targets, ctx = SyntheticZOD(batch=2, img_h=128, img_w=160, seed=6).sample("cpu")
    M = 16
    G, Qdn = dn_shapes(M, 100)
    tb, tl, nv = pad_targets(targets, M)
    lab, unact = make_denoising(tb, tl, nv, 1, G, None, torch.Generator().manual_seed(3))
    plain = model(images, ctx)
    with_dn = model(images, ctx, (lab, unact, G))
    return model, plain, with_dn, (tb, tl, nv, G, Qdn, M)


def test_state_dict_keys_without_denoising():
    from src.rtdetr_moe.model import RTDETRMoE

    with_dn = RTDETRMoE(SPEC).state_dict()
    without = RTDETRMoE("rtdetr-r18-moe4-top2").state_dict()
    assert not any("denoising" in k for k in without)
    assert set(with_dn) - set(without) == {"decoder.denoising_class_embed"}
    assert with_dn["decoder.denoising_class_embed"].shape == (2, 256)
    assert (with_dn["decoder.denoising_class_embed"][1] == 0).all()


def test_matching_queries_do_not_see_denoising_queries(decoder_run):
    model, plain, with_dn, (tb, tl, nv, G, Qdn, M) = decoder_run
    assert "dn_outputs" not in plain and "dn_meta" not in plain
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)  # noqa: E731
    for k in ("pred_logits", "pred_boxes"):
        assert with_dn[k].shape == plain[k].shape
        close(with_dn[k], plain[k])
        close(with_dn["enc_outputs"][k], plain["enc_outputs"][k])
        for a, b in zip(with_dn["aux_outputs"], plain["aux_outputs"]):
            close(a[k], b[k])
    assert len(with_dn["aux_outputs"]) == len(plain["aux_outputs"])
    n_layers = len(model.decoder.layers)
    assert len(with_dn["dn_outputs"]) == n_layers
    for o in with_dn["dn_outputs"]:
        assert o["pred_logits"].shape == (2, Qdn, 1) and o["pred_boxes"].shape == (2, Qdn, 4)
    assert with_dn["dn_meta"] == {"groups": G, "slots": M}


def test_eval_mode_ignores_the_pack(decoder_run):
    model, plain, with_dn, (tb, tl, nv, G, Qdn, M) = decoder_run
    from src.rtdetr_moe.data import SyntheticZOD

    images, _, ctx = SyntheticZOD(batch=2, img_h=128, img_w=160, seed=6).sample("cpu")
    lab, unact = make_denoising(tb, tl, nv, 1, G, None, torch.Generator().manual_seed(3))
    model.eval()
    try:
        with torch.no_grad():
            a = model(images, ctx)
            b = model(images, ctx, (lab, unact, G))
    finally:
        model.train()
    assert "dn_outputs" not in b
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])


def test_dn_losses_match_reference_formulation(decoder_run):
    """dn_losses (torch formulation) = SetCriterion._losses on the denoising
    outputs with the fixed index pairs (positive query g 2M + j <-> target j)
    and num_boxes G."""
    model, plain, with_dn, (tb, tl, nv, G, Qdn, M) = decoder_run
    crit = SetCriterion(num_classes=1)
    num_boxes = 5.0
    got = crit.dn_losses(with_dn["dn_outputs"], tb, tl, nv, num_boxes, G, fused=False)
    n_layers = len(with_dn["dn_outputs"])
    names = [f"_dn_aux{i}" for i in range(n_layers - 1)] + ["_dn"]
    assert set(got) == {k + s for k in ("loss_vfl", "loss_bbox", "loss_giou") for s in names}
    targets = [{"boxes": tb[b, :int(nv[b])], "labels": tl[b, :int(nv[b])]} for b in range(tb.shape[0])]
    indices = []
    for b in range(tb.shape[0]):
        n = int(nv[b])
        src = torch.tensor([dn_index(g, 0, j, M) for g in range(G) for j in range(n)], dtype=torch.int64)
        tgt = torch.tensor([j for g in range(G) for j in range(n)], dtype=torch.int64)
        indices.append((src, tgt))
    assert sum(len(s) for s, _ in indices) > 0
    for o, suffix in zip(with_dn["dn_outputs"], names):
        ref = crit._losses(o, targets, indices, num_boxes * G)
        for k, v in ref.items():
            torch.testing.assert_close(got[k + suffix], v * crit.w[k], rtol=1e-5, atol=1e-6, msg=k + suffix)


def test_gradients_reach_embedding_and_decoder(decoder_run):
    model, plain, with_dn, (tb, tl, nv, G, Qdn, M) = decoder_run
    crit = SetCriterion(num_classes=1)
    loss = sum(crit.dn_losses(with_dn["dn_outputs"], tb, tl, nv, 5.0, G, fused=False).values())
    dec = model.decoder
    params = {"embed": dec.denoising_class_embed, "attn": dec.layers[0].self_attn.in_proj_weight,
              "score": dec.dec_score_head[-1].weight,
              "bbox": dec.dec_bbox_head[0].layers[-1].weight,  # (zero-initialised: nothing reaches the layers below)
              "expert": dec.layers[-1].ffn.w1}
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    for (name, _), g in zip(params.items(), grads):
        assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0, name
    g_embed = grads[0]
    assert (g_embed[dec.num_classes] == 0).all()  # the padded slots' row stays at zero
    assert g_embed[:dec.num_classes].abs().sum() > 0
