"""Per-context routing statistics of the MoE layers (validation's context
report).

For one layer the table is int64 [n_ctx, E, 5]: for every solar-context bin c
and expert e, how many (token, slot) assignments of context c went to e, how
many tokens had e as their first choice, how many of the assignments the
capacity dropped, and the gate weight and router probability they carried --
the last two in 2^-32 fixed point, ``fix(x) = (int64) rint(x * 2^32)``, so
every sum is an integer: the table does not depend on the order of the adds
and the GPU kernel (``moe_route_stats``) equals ``route_stats_reference``
exactly.  Tokens per context need no field: they are ``top1.sum(over e)``.
"""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np
import torch

FIELDS = ("assignments", "top1", "dropped", "gate_mass", "prob_mass")
FIX_ONE = 1 << 32


def _fix(x: torch.Tensor) -> torch.Tensor:
    # torch.round is round-half-even, as np.rint and the kernel's __double2ll_rn
    return torch.round(x.double() * float(FIX_ONE)).to(torch.int64)


def route_stats_reference(idx, w, pos, probs, ctx_img, tokens_per_image, n_ctx) -> torch.Tensor:
    """The table of ``moe_route_stats`` in torch, integer accumulation only.

    idx [T, k] (any integer dtype), w [T, k], pos [T, k] or None, probs [T, E],
    ctx_img [T / tokens_per_image] or None (every token in context 0) ->
    int64 [n_ctx, E, 5] on the inputs' device.  An image whose context id is
    outside [0, n_ctx) and an expert index outside [0, E) contribute nothing.
    """
    T, k = idx.shape
    E = probs.shape[1]
    dev = idx.device
    n_ctx, tpi = int(n_ctx), int(tokens_per_image)
    if tpi < 1 or T % tpi != 0:
        raise ValueError(f"T {T} is no multiple of tokens_per_image {tpi}")
    if ctx_img is None:
        if n_ctx != 1:
            raise ValueError("without ctx_img every token is in context 0: n_ctx must be 1")
        c_tok = torch.zeros(T, dtype=torch.int64, device=dev)
    else:
        c_tok = ctx_img.to(torch.int64).reshape(-1)[:T // tpi].repeat_interleave(tpi)
    tok_ok = (c_tok >= 0) & (c_tok < n_ctx)
    flat = torch.zeros(n_ctx * E * len(FIELDS), dtype=torch.int64, device=dev)
    if T == 0:
        return flat.view(n_ctx, E, len(FIELDS))

    def add(ctx, expert, field, values, keep):
        flat.index_add_(0, ((ctx * E + expert) * len(FIELDS) + field)[keep], values[keep])

    e = idx.to(torch.int64)
    one = torch.ones_like(e)
    c_slot = c_tok[:, None].expand(T, k)
    ok = tok_ok[:, None] & (e >= 0) & (e < E)
    add(c_slot, e, 0, one, ok)
    first = torch.zeros_like(ok)
    first[:, 0] = True
    add(c_slot, e, 1, one, ok & first)
    if pos is not None:
        add(c_slot, e, 2, one, ok & (pos < 0))
    add(c_slot, e, 3, _fix(w), ok)
    ee = torch.arange(E, device=dev)[None, :].expand(T, E)
    add(c_tok[:, None].expand(T, E), ee, 4, _fix(probs), tok_ok[:, None].expand(T, E))
    return flat.view(n_ctx, E, len(FIELDS))


def record(table, idx, w, pos, probs, ctx_img, tokens_per_image):
    """ADD one layer forward's statistics to ``table`` (int64 [n_ctx, E, 5]):
    one HIP launch for GPU tensors, the reference for CPU tensors."""
    n_ctx = int(table.shape[0])
    if ctx_img is None and n_ctx != 1:
        raise ValueError("a routing table with more than one context needs the batch's context ids")
    if table.is_cuda:
        from . import _lib as L

        ci = ctx_img.to(torch.int32).contiguous() if ctx_img is not None else None
        L.route_stats(idx, w, pos, probs, ci, n_ctx, int(tokens_per_image), table)
    else:
        table += route_stats_reference(idx, w, pos, probs, ctx_img, tokens_per_image, n_ctx)


def layer_names(model) -> list:
    """``encoder.<i>`` / ``decoder.<i>`` for model.moe_layers(), in its order."""
    from .layer import MoEFFN

    names, count = [], {}
    for name, mod in model.named_modules():
        if isinstance(mod, MoEFFN):
            part = "encoder" if name.split(".")[0] == "encoder" else "decoder"
            names.append(f"{part}.{count.get(part, 0)}")
            count[part] = count.get(part, 0) + 1
    return names


def _is_ep(layer) -> bool:
    return layer.ep_size > 1 or bool(layer.cfg.expert_parallel)


class RouteStats:
    """One int64 table [n_ctx, E, 5] per MoE layer of a model, on the layer's
    device, keyed ``encoder.<i>`` / ``decoder.<i>`` in ``model.moe_layers()``
    order.  Expert-parallel layers keep no table (``skipped`` names them).

    with stats.attach(model):   # every layer forward adds to its table
        ...
    """

    def __init__(self, model, n_ctx: int | None = None):
        from .context import NUM_CONTEXTS

        self.n_ctx = int(NUM_CONTEXTS if n_ctx is None else n_ctx)
        self.layers, self.table, self.skipped, self.meta = {}, {}, {}, {}
        for name, layer in zip(layer_names(model), model.moe_layers()):
            self.meta[name] = {"experts": int(layer.cfg.num_experts), "top_k": int(layer.cfg.top_k)}
            if _is_ep(layer):
                self.skipped[name] = "expert-parallel layer: routing tables are kept for single-device layers only"
                continue
            self.layers[name] = layer
            self.table[name] = torch.zeros((self.n_ctx, layer.cfg.num_experts, len(FIELDS)), dtype=torch.int64,
                                           device=layer.wg.device)

    @contextmanager
    def attach(self, model=None):
        """Set every layer's sink for the duration (``model`` is accepted for
        symmetry; the layers were taken at construction)."""
        try:
            for name, layer in self.layers.items():
                layer.route_stats = self.table[name]
            yield self
        finally:
            for layer in self.layers.values():
                layer.route_stats = None

    def reset(self):
        for t in self.table.values():
            t.zero_()

    def snapshot(self) -> dict:
        return {name: t.clone() for name, t in self.table.items()}

    def restore(self, s: dict):
        for name, t in self.table.items():
            t.copy_(s[name])

    def tables(self) -> dict:
        """{layer name: int64 numpy [n_ctx, E, 5]} (waits for the device)."""
        return {name: t.cpu().numpy() for name, t in self.table.items()}


def mi_bits(assignments) -> float:
    """Mutual information, in bits, between context and expert over the
    assignment counts n[c, e]: sum over n > 0 of p log2(p / (p_c p_e)), p = n / N;
    0 for an empty table.  0 = the context does not decide the expert;
    log2(min(C, E)) = it decides it fully."""
    n = np.asarray(assignments, dtype=np.float64)
    N = n.sum()
    if N <= 0:
        return 0.0
    p = n / N
    pc = p.sum(1, keepdims=True)
    pe = p.sum(0, keepdims=True)
    nz = n > 0
    return float((p[nz] * np.log2(p[nz] / (pc * pe)[nz])).sum())


def routing_summary(table, k: int, labels) -> dict:
    """One layer's table as plain Python (JSON-ready): the five integer fields
    as [n_ctx][E] lists, gate / prob mass also as floats, tokens per context,
    each context's expert share of its assignments, and ``mi_bits``."""
    t = np.asarray(table).astype(np.int64)
    out = {"labels": list(labels), "top_k": int(k)}
    for f, name in enumerate(FIELDS):
        out[name] = t[:, :, f].tolist()
    out["gate_mass_float"] = (t[:, :, 3].astype(np.float64) / FIX_ONE).tolist()
    out["prob_mass_float"] = (t[:, :, 4].astype(np.float64) / FIX_ONE).tolist()
    out["tokens"] = t[:, :, 1].sum(1).tolist()
    a = t[:, :, 0].astype(np.float64)
    tot = a.sum(1, keepdims=True)
    out["expert_share"] = np.divide(a, tot, out=np.zeros_like(a), where=tot > 0).tolist()
    out["mi_bits"] = mi_bits(t[:, :, 0])
    return out
