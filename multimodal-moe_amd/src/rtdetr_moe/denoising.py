"""Contrastive denoising queries for training (RT-DETR's
get_contrastive_denoising_training_group, restated with fixed shapes so that
the training step stays one hipGraph).

Next to the Q matching queries the decoder gets Qdn noised copies of the
ground truth: G groups, each holding a positive half (small box noise: the
decoder must recover the target) and a negative half (larger noise: it must
answer "background") of the M padded target slots.  They are supervised with
a fixed assignment (SetCriterion.dn_losses), no Hungarian matching.

Fixed shapes: M is the padded target capacity of the step (GraphedStep.M),
G = max(1, num_denoising // M) and Qdn = 2 M G whatever the batch holds
(upstream sizes the groups by the batch's largest box count).  Group g, half
h (0 = positive, 1 = negative) and target slot j are query g 2M + h M + j.
Slots j >= n_valid[b] carry the label num_classes (the zero row of the
decoder's denoising_class_embed) and the un-noised PAD_BOX (upstream: a zero
box); like upstream's they stay visible inside their group and carry no loss.

Self-attention mask as segment ids (csrc/attn.hip, rtdetr_attn_*_seg): group
g for the denoising block, -1 (shared: visible to all) for the matching
queries -- matching queries do not see denoising queries and the groups do
not see each other."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .criterion import PAD_BOX, box_cxcywh_to_xyxy


@dataclass
class DenoisingConfig:
    label_noise_ratio: float = 0.5  # a valid slot's label is redrawn with probability ratio / 2
    box_noise_scale: float = 1.0    # corner noise in units of half the box width / height
    eps: float = 1e-5               # inverse sigmoid clamp (decoder.box_refine's)


def dn_shapes(M: int, num_denoising: int) -> tuple[int, int]:
    """(G, Qdn) for a padded target capacity M and a requested query count."""
    G = max(1, int(num_denoising) // int(M))
    return G, 2 * int(M) * G


def dn_index(g: int, h: int, j: int, M: int) -> int:
    """Query index of group g, half h (0 positive, 1 negative), target slot j."""
    return g * 2 * M + h * M + j


def segments(G: int, M: int, Q: int, device=None) -> torch.Tensor:
    """int32 [2 M G + Q] segment ids: g over group g's 2M queries, then -1 for
    the Q matching queries."""
    seg = torch.full((2 * M * G + Q,), -1, dtype=torch.int32)
    seg[:2 * M * G] = torch.arange(G, dtype=torch.int32).repeat_interleave(2 * M)
    return seg.to(device) if device is not None else seg


def make_denoising(tgt_boxes, tgt_labels, n_valid, num_classes, G, cfg: DenoisingConfig | None = None,
                   generator: torch.Generator | None = None, out=None):
    """Noised targets -> (labels int64 [B, Qdn], ref_unact fp32 [B, Qdn, 4]);
    tgt_boxes [B, M, 4] cxcywh, tgt_labels [B, M], n_valid int [B] (the padded
    targets of criterion.pad_targets).  Device ops only, no host sync, fixed
    shapes; written into ``out`` = (labels, ref_unact) static buffers when
    given.  All randomness from ``generator``."""
    cfg = cfg or DenoisingConfig()
    B, M, _ = tgt_boxes.shape
    dev = tgt_boxes.device
    shape = (B, G, 2, M)
    rand = lambda *s: torch.rand(s, generator=generator, device=dev)  # noqa: E731
    valid = (torch.arange(M, device=dev)[None, :] < n_valid[:, None])[:, None, None, :].expand(shape)
    # labels: redrawn uniformly with probability label_noise_ratio / 2
    lab = tgt_labels.long()[:, None, None, :].expand(shape)
    if cfg.label_noise_ratio > 0:
        flip = rand(*shape) < cfg.label_noise_ratio * 0.5
        drawn = torch.randint(0, num_classes, shape, generator=generator, device=dev)
        lab = torch.where(flip, drawn, lab)
    lab = torch.where(valid, lab, torch.full_like(lab, num_classes))
    # boxes: every xyxy corner moves by sign * r * (w or h) / 2 * scale,
    # r in [0, 1) for the positive half and [1, 2) for the negative half
    box = tgt_boxes.float()[:, None, None, :, :].expand(*shape, 4)
    pad = torch.tensor(PAD_BOX, dtype=torch.float32, device=dev).expand(*shape, 4)
    if cfg.box_noise_scale > 0:
        half = torch.cat([box[..., 2:], box[..., 2:]], -1) * (0.5 * cfg.box_noise_scale)
        sign = torch.randint(0, 2, (*shape, 4), generator=generator, device=dev).float() * 2.0 - 1.0
        r = rand(*shape, 4) + torch.tensor([0.0, 1.0], device=dev)[None, None, :, None, None]
        xyxy = (box_cxcywh_to_xyxy(box) + sign * r * half).clamp(0.0, 1.0)
        noised = torch.cat([(xyxy[..., :2] + xyxy[..., 2:]) * 0.5, xyxy[..., 2:] - xyxy[..., :2]], -1)
        box = torch.where(valid[..., None], noised, pad)
    else:
        box = torch.where(valid[..., None], box, pad)
    box = box.clamp(0.0, 1.0)
    unact = torch.log(box.clamp(min=cfg.eps) / (1 - box).clamp(min=cfg.eps))
    lab, unact = lab.reshape(B, G * 2 * M), unact.reshape(B, G * 2 * M, 4)
    if out is not None:
        out[0].copy_(lab)
        out[1].copy_(unact)
        return out[0], out[1]
    return lab.contiguous(), unact.contiguous()
