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
"""
from __future__ import annotations

import numpy as np
import torch

# one record of moe_balance_step's device table (csrc/balance.hip BalanceLayer)
_REC = np.dtype([("hist", np.uint64), ("bias", np.uint64)])


def balance_reference(load: torch.Tensor, bias: torch.Tensor, rate: float) -> torch.Tensor:
    """The update rule in torch ops, in place on ``bias`` (fp32 [L, E]) and
    ``load`` (int64 [L, E], zeroed); returns maxvio fp32 [L].  What
    moe_balance_step(apply=1) computes bit for bit."""
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


def balanced_layers(model) -> list:
    """The model's MoE layers that carry a selection bias, in module order."""
    from .layer import MoEFFN

    return [m for m in model.modules() if isinstance(m, MoEFFN) and getattr(m, "sel_bias", None) is not None]


class LoadBalancer:
    """Owns what the update needs besides the layers' ``sel_bias`` buffers: the
    int64 [L, E] load table (no part of any state dict: it is empty between
    optimizer steps), the GPU launch's address table and ``maxvio`` [L].

    ``add()`` after every micro-step's forward: load += each layer's
    ``last_hist``.  ``apply()`` once per optimizer step: at world > 1 one int64
    all-reduce of the table, then the rule.  GPU: one moe_balance_step launch
    each; the table of (hist, bias) addresses is rebuilt when an address
    changes, and the tensors it names are held.  CPU: torch ops.

    ``pin()`` (a captured step): take the layers' current ``last_hist`` tensors
    -- the graph's static outputs -- as the sources of every later ``add()``,
    whatever another forward (an evaluation) has put into ``last_hist`` since;
    ``add()`` then also puts them back, so ``last_hist`` is the training
    step's after a step.  ``unpin()``: read ``last_hist`` afresh again."""

    def __init__(self, model, rate: float, group=None, world: int = 1):
        self.layers = balanced_layers(model)
        if not self.layers:
            raise ValueError("LoadBalancer: the model has no MoE layer with a selection bias")
        if not float(rate) > 0.0:
            raise ValueError(f"LoadBalancer: rate {rate} must be positive")
        Es = {int(m.sel_bias.numel()) for m in self.layers}
        if len(Es) != 1:
            raise ValueError(f"LoadBalancer: layers with different expert counts {sorted(Es)}")
        self.E = Es.pop()
        self.L = len(self.layers)
        self.rate, self.group, self.world = float(rate), group, int(world)
        dev = self.layers[0].sel_bias.device
        self.device = dev
        self.load = torch.zeros((self.L, self.E), dtype=torch.int64, device=dev)
        self.maxvio = torch.zeros(self.L, dtype=torch.float32, device=dev)
        for i, m in enumerate(self.layers):
            m.last_maxvio = self.maxvio[i]
        self._pinned = None
        self._held = None      # the tensors the device table names
        self._ptrs = None
        self._table = None
        self._table_apply = None  # hist pointers NULL: apply after the all-reduce

    # -- sources ---------------------------------------------------------------
    def pin(self):
        self._pinned = [m.last_hist for m in self.layers]
        if any(h is None for h in self._pinned):
            raise RuntimeError("LoadBalancer.pin: a layer has not run a forward yet")

    def unpin(self):
        self._pinned = None

    def _hists(self):
        if self._pinned is not None:
            for m, h in zip(self.layers, self._pinned):
                m.last_hist = h
            return self._pinned
        hs = [m.last_hist for m in self.layers]
        if any(h is None for h in hs):
            raise RuntimeError("LoadBalancer.add: a layer has not run a forward yet")
        return hs

    def _tables(self, hists):
        biases = [m.sel_bias for m in self.layers]
        ptrs = tuple(h.data_ptr() for h in hists) + tuple(b.data_ptr() for b in biases)
        if ptrs != self._ptrs:
            for h in hists:
                if h.dtype != torch.int32 or not h.is_contiguous() or h.numel() != self.E or h.device != self.device:
                    raise RuntimeError("LoadBalancer: last_hist must be a contiguous int32 [E] on the bias' device")
            for b in biases:
                if b.dtype != torch.float32 or not b.is_contiguous() or b.device != self.device:
                    raise RuntimeError("LoadBalancer: sel_bias must be a contiguous fp32 buffer on one device")
            rec = np.zeros(self.L, dtype=_REC)
            for i, (h, b) in enumerate(zip(hists, biases)):
                rec[i]["hist"] = h.data_ptr()
                rec[i]["bias"] = b.data_ptr()
            self._table = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            rec["hist"] = 0
            self._table_apply = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            self._held, self._ptrs = (list(hists), biases), ptrs
        return self._table, self._table_apply

    # -- the two halves ----------------------------------------------------------
    @torch.no_grad()
    def add(self):
        hists = self._hists()
        if self.device.type != "cuda":
            for i, h in enumerate(hists):
                self.load[i] += h.to(torch.int64)
            return
        from . import _lib as L

        table, _ = self._tables(hists)
        L.balance_step(table, self.L, self.E, self.load, self.rate, False, self.maxvio)

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
            self.maxvio.copy_(balance_reference(self.load, bias, self.rate))
            for m, b in zip(self.layers, bias):
                m.sel_bias.copy_(b)
            return
        from . import _lib as L

        hists = self._held[0] if self._held is not None else self._hists()
        _, table = self._tables(hists)
        L.balance_step(table, self.L, self.E, self.load, self.rate, True, self.maxvio)
