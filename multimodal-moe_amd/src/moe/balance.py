"""Loss-free expert load balancing (Wang et al. 2024, "Auxiliary-Loss-Free
Load Balancing Strategy for Mixture-of-Experts"; used in DeepSeek-V3).

Every MoE layer built with ``MoEConfig.balance_rate > 0`` (an ``-alb`` spec
token) owns ``sel_bias``, an fp32 buffer [E] of zeros.  The router adds it to
the logits FOR THE TOP-K SELECTION ONLY (eager.route; on the GPU
moe_router_topk_fwd_sel): gates, softmax, aux losses and the whole backward
never see it, so no gradient fights the detection loss.  After every optimizer
step the bias of an expert that received less than the mean load moves up by
the rate, and that of an over-loaded expert down.

The rule (``balance_reference``), per layer l, on the load summed over the
micro-steps of one optimizer step and over the ranks::

    total = sum_e load[l, e]                         (0: bias unchanged, maxvio 0)
    s_e   = sign(total - E load[l, e])               exact in int64
    bias[l, e] = fl32(bias[l, e] + s_e fl32(rate))
    bias[l, e] = bias[l, e] - min_e bias[l, e]       recentre: the smallest becomes 0
    maxvio[l]  = float32((double)(E max_e load - total) / (double)total)
    load[l, :] = 0

The published update has no recentring.  More experts sit below the mean load
than above it, so the mean bias drifts upwards without bound; a shift common to
all experts changes no selection, so the smallest bias is pinned at 0.

``load`` is the layers' unclipped ``hist`` (assignments before capacity
drops).  Under data or expert parallelism every rank routes its own tokens
over all E experts, so the rank-summed hist is the global load and every rank
applies the same update to its replica of the bias.

On the GPU both halves are ONE ``moe_balance_step`` launch for all layers of
the model (csrc/balance.hip), outside the step graph: the graph's router
launch reads ``sel_bias`` by address, so the next replay routes with the
updated values, and the captures' warm-up passes move nothing.

Per context (``MoEConfig.balance_per_context``, an ``-albc`` spec token).  One
bias per expert sees only the mix of contexts in a step: the context bias
pushes each context's tokens to its own few experts, and a batch that holds a
single context (a driving sequence, a night shard) stays as skewed as before.
In this mode ``sel_bias`` is fp32 [C, E]; a token of an image with context c
is ranked by ``fl32(logit + sel_bias[c, e])`` (eager.route; on the GPU
moe_router_topk_fwd_selctx), and row c moves by the rule above on
``load[l, c, e]``, the (token, slot) assignments to expert e among the tokens
of images with context c -- counted before capacity drops from the layer's
``last_topk_idx`` / ``last_ctx``, summed over micro-steps and ranks; an expert
or context id outside its range counts nowhere (route_stats' convention).  A
row whose context had no tokens in the optimizer step is not touched.  On the
GPU: one ``moe_balance_step_ctx`` launch for all layers, a workgroup per
(context, layer).  The price: every context's SELECTION is flattened, so the
contexts no longer specialise in which experts they pick; they still do in the
gates, which come from the unbiased logits.
"""
from __future__ import annotations

import numpy as np
import torch

# one record of moe_balance_step's device table (csrc/balance.hip BalanceLayer)
_REC = np.dtype([("hist", np.uint64), ("bias", np.uint64)])
# ... and of moe_balance_step_ctx's (BalanceCtxLayer, 32 B)
_REC_CTX = np.dtype([("topk_idx", np.uint64), ("bias", np.uint64), ("ctx_img", np.uint64), ("T", np.int32),
                     ("tokens_per_image", np.int32)])
assert _REC.itemsize == 16 and _REC_CTX.itemsize == 32


def balance_reference(load: torch.Tensor, bias: torch.Tensor, rate: float) -> torch.Tensor:
    """The update rule in torch ops, in place on ``bias`` (fp32 [L, E]) and
    ``load`` (int64 [L, E], zeroed); returns maxvio fp32 [L].  What
    moe_balance_step(apply=1) computes bit for bit.

    The rule is per row, so the per-context update is this function on
    ``load.view(L * C, E)`` and ``bias.view(L * C, E)`` (maxvio then views as
    [L, C]): what moe_balance_step_ctx(apply=1) computes bit for bit."""
    L, E = load.shape
    r32 = torch.tensor(float(rate), dtype=torch.float32, device=bias.device)
    maxvio = torch.zeros(L, dtype=torch.float32, device=bias.device)
    for l in range(L):
        ld = load[l].to(torch.int64)
        total = ld.sum()
        if int(total) != 0:
            s = torch.sign(total - E * ld).to(torch.float32)
            b = bias[l] + s * r32
            bias[l].copy_(b - b.min())
            maxvio[l] = ((E * ld.max() - total).to(torch.float64) / total.to(torch.float64)).to(torch.float32)
        load[l].zero_()
    return maxvio


def context_counts(topk_idx: torch.Tensor, ctx_img: torch.Tensor, tokens_per_image: int, C: int,
                   E: int) -> torch.Tensor:
    """int64 [C, E]: the (token, slot) assignments to each expert among the
    tokens of the images of each context; ids outside [0, E) / [0, C) count
    nowhere.  The CPU statement of moe_balance_step_ctx's counting."""
    idx = topk_idx.to(torch.int64)
    T, k = idx.shape
    ctx_tok = ctx_img.to(torch.int64).repeat_interleave(int(tokens_per_image))[:T]
    if ctx_tok.numel() != T:
        raise ValueError(f"context_counts: {ctx_img.numel()} images of {tokens_per_image} tokens do not cover {T}")
    c = ctx_tok.unsqueeze(1).expand(T, k)
    ok = (idx >= 0) & (idx < E) & (c >= 0) & (c < C)
    return torch.bincount((c * E + idx)[ok], minlength=C * E).view(C, E)


def balanced_layers(model) -> list:
    """The model's MoE layers that carry a selection bias, in module order."""
    from .layer import MoEFFN

    return [m for m in model.modules() if isinstance(m, MoEFFN) and getattr(m, "sel_bias", None) is not None]


class LoadBalancer:
    """Owns what the update needs besides the layers' ``sel_bias`` buffers: the
    int64 load table (no part of any state dict: it is empty between optimizer
    steps), the GPU launch's address table and ``maxvio``.  Per expert
    (``sel_bias`` [E]): load [L, E], maxvio [L].  Per context (``sel_bias``
    [C, E], ``per_context``): load [L, C, E], maxvio [L, C], and a layer's
    ``last_maxvio`` is the maximum over its contexts.  A model that mixes the
    two kinds of layer is refused.

    ``add()`` after every micro-step's forward: load += each layer's
    ``last_hist`` (per context: the per-context counts of its
    ``last_topk_idx`` / ``last_ctx``).  ``apply()`` once per optimizer step: at
    world > 1 one int64 all-reduce of the whole table, then the rule.  GPU: one
    moe_balance_step (moe_balance_step_ctx) launch each; the address table is
    rebuilt when an address or a token count changes, and the tensors it names
    are held.  CPU: torch ops.

    ``pin()`` (a captured step): take the layers' current ``last_hist`` (and
    ``last_topk_idx``, ``last_ctx``) tensors -- the graph's static outputs --
    as the sources of every later ``add()``, whatever another forward (an
    evaluation) has put there since; ``add()`` then also puts them back, so
    they are the training step's after a step.  ``unpin()``: read them afresh
    again."""

    _SOURCES = ("last_hist", "last_topk_idx", "last_ctx")

    def __init__(self, model, rate: float, group=None, world: int = 1):
        self.layers = balanced_layers(model)
        if not self.layers:
            raise ValueError("LoadBalancer: the model has no MoE layer with a selection bias")
        if not float(rate) > 0.0:
            raise ValueError(f"LoadBalancer: rate {rate} must be positive")
        dims = {int(m.sel_bias.dim()) for m in self.layers}
        if len(dims) != 1:
            raise ValueError("LoadBalancer: per-expert and per-context selection biases in one model")
        self.per_context = dims.pop() == 2
        Es = {int(m.sel_bias.shape[-1]) for m in self.layers}
        if len(Es) != 1:
            raise ValueError(f"LoadBalancer: layers with different expert counts {sorted(Es)}")
        self.E = Es.pop()
        self.L = len(self.layers)
        self.rate, self.group, self.world = float(rate), group, int(world)
        dev = self.layers[0].sel_bias.device
        self.device = dev
        if self.per_context:
            Cs = {int(m.sel_bias.shape[0]) for m in self.layers}
            ks = {int(m.cfg.top_k) for m in self.layers}
            if len(Cs) != 1 or len(ks) != 1:
                raise ValueError(f"LoadBalancer: layers with different context counts {sorted(Cs)} or top-k {sorted(ks)}")
            self.C, self.k = Cs.pop(), ks.pop()
            self.load = torch.zeros((self.L, self.C, self.E), dtype=torch.int64, device=dev)
            self.maxvio = torch.zeros((self.L, self.C), dtype=torch.float32, device=dev)
            self._layer_maxvio = torch.zeros(self.L, dtype=torch.float32, device=dev)
        else:
            self.C = self.k = None
            self.load = torch.zeros((self.L, self.E), dtype=torch.int64, device=dev)
            self.maxvio = torch.zeros(self.L, dtype=torch.float32, device=dev)
            self._layer_maxvio = self.maxvio
        for i, m in enumerate(self.layers):
            m.last_maxvio = self._layer_maxvio[i]
        self._pinned = None
        self._held = None      # the tensors the device table names
        self._ptrs = None
        self._table = None
        self._table_apply = None  # source pointers NULL: apply after the all-reduce

    # -- sources ---------------------------------------------------------------
    def _names(self):
        return self._SOURCES if self.per_context else self._SOURCES[:1]

    def _read(self, what):
        srcs = [tuple(getattr(m, n) for n in self._names()) for m in self.layers]
        if any(t is None for s in srcs for t in s):
            raise RuntimeError(f"LoadBalancer.{what}: a layer has not run a forward yet")
        return srcs

    def pin(self):
        self._pinned = self._read("pin")

    def unpin(self):
        self._pinned = None

    def _sources(self):
        """Per layer (last_hist,) or (last_hist, last_topk_idx, last_ctx)."""
        if self._pinned is not None:
            for m, src in zip(self.layers, self._pinned):
                for n, t in zip(self._names(), src):
                    setattr(m, n, t)
            return self._pinned
        return self._read("add")

    def _tables(self, srcs):
        biases = [m.sel_bias for m in self.layers]
        tokens = tuple(int(s[1].shape[0]) for s in srcs) if self.per_context else ()
        ptrs = tuple(t.data_ptr() for s in srcs for t in s) + tuple(b.data_ptr() for b in biases) + tokens
        if ptrs != self._ptrs:
            for b in biases:
                if b.dtype != torch.float32 or not b.is_contiguous() or b.device != self.device:
                    raise RuntimeError("LoadBalancer: sel_bias must be a contiguous fp32 buffer on one device")
            if self.per_context:
                rec = self._ctx_records(srcs, biases)
                null = "topk_idx"
            else:
                for (h,) in srcs:
                    if h.dtype != torch.int32 or not h.is_contiguous() or h.numel() != self.E or h.device != self.device:
                        raise RuntimeError("LoadBalancer: last_hist must be a contiguous int32 [E] on the bias' device")
                rec = np.zeros(self.L, dtype=_REC)
                for i, ((h,), b) in enumerate(zip(srcs, biases)):
                    rec[i]["hist"] = h.data_ptr()
                    rec[i]["bias"] = b.data_ptr()
                null = "hist"
            self._table = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            rec[null] = 0
            self._table_apply = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            self._held, self._ptrs = (list(srcs), biases), ptrs
        return self._table, self._table_apply

    def _ctx_records(self, srcs, biases):
        """moe_balance_step_ctx's table, every bound the kernel relies on checked
        here: topk_idx int32 [T, k] and ctx_img int32 with an id for every image
        of T tokens."""
        rec = np.zeros(self.L, dtype=_REC_CTX)
        for i, (m, (_, idx, ci), b) in enumerate(zip(self.layers, srcs, biases)):
            for t, what in ((idx, "last_topk_idx"), (ci, "last_ctx")):
                if t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
                    raise RuntimeError(f"LoadBalancer: {what} must be a contiguous int32 tensor on the bias' device")
            if idx.dim() != 2 or idx.shape[1] != self.k or tuple(b.shape) != (self.C, self.E):
                raise RuntimeError(f"LoadBalancer: last_topk_idx {tuple(idx.shape)} / sel_bias {tuple(b.shape)} do "
                                   f"not match k {self.k}, C {self.C}, E {self.E}")
            T = int(idx.shape[0])
            if T == 0 or ci.numel() == 0 or T % ci.numel() != 0:
                raise RuntimeError(f"LoadBalancer: {T} tokens are not a whole number of tokens for {ci.numel()} images")
            rec[i]["topk_idx"], rec[i]["bias"], rec[i]["ctx_img"] = idx.data_ptr(), b.data_ptr(), ci.data_ptr()
            rec[i]["T"], rec[i]["tokens_per_image"] = T, T // ci.numel()
        return rec

    def _launch(self, table, apply):
        from . import _lib as L

        if self.per_context:
            L.balance_step_ctx(table, self.L, self.C, self.E, self.k, self.load, self.rate, apply, self.maxvio)
            if apply:
                torch.amax(self.maxvio, dim=1, out=self._layer_maxvio)
        else:
            L.balance_step(table, self.L, self.E, self.load, self.rate, apply, self.maxvio)

    # -- the two halves ----------------------------------------------------------
    @torch.no_grad()
    def add(self):
        srcs = self._sources()
        if self.device.type != "cuda":
            for i, src in enumerate(srcs):
                if self.per_context:
                    _, idx, ci = src
                    self.load[i] += context_counts(idx, ci, idx.shape[0] // max(1, ci.numel()), self.C, self.E)
                else:
                    self.load[i] += src[0].to(torch.int64)
            return
        self._launch(self._tables(srcs)[0], False)

    @torch.no_grad()
    def apply(self):
        if self.world > 1:
            import torch.distributed as dist

            if self.load.is_cuda and dist.get_backend(self.group) == "gloo":
                # gloo moves host memory only (ranks sharing one GPU in the multi-rank tests)
                host = self.load.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
                self.load.copy_(host)
            else:
                dist.all_reduce(self.load, op=dist.ReduceOp.SUM, group=self.group)
        if self.device.type != "cuda":
            bias = torch.stack([m.sel_bias for m in self.layers])
            mv = balance_reference(self.load.view(-1, self.E), bias.view(-1, self.E), self.rate)
            self.maxvio.copy_(mv.view_as(self.maxvio))
            if self.per_context:
                self._layer_maxvio.copy_(self.maxvio.amax(dim=1))
            for m, b in zip(self.layers, bias):
                m.sel_bias.copy_(b)
            return
        srcs = self._held[0] if self._held is not None else self._sources()
        self._launch(self._tables(srcs)[1], True)
