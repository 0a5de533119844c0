"""Exponential moving average (EMA) of the model's weights in training.

The reference trains through Ultralytics' ``RTDETR.train``
(``src/models/vision/rtdetr.py:82-94``), whose trainer keeps a ModelEMA: after
every optimizer step each floating-point entry of the model's state dict
(parameters and buffers) moves towards its live value,

    ema = d_t ema + (1 - d_t) value,    d_t = decay (1 - exp(-t / tau)),

with t the number of updates so far (from 1), decay 0.9999 and tau 2000; the
trainer validates the averaged model and writes it into best.pt / last.pt.
Integer entries (BatchNorm's num_batches_tracked) are not averaged, and an
entry that training never changes (FrozenBatchNorm2d's buffers, a parameter
without a gradient) is its own average: both come from the live model.

On the GPU the parameters' average lives next to the optimizer's fp32 masters
(optim.FlatAdamW / ShardedDPAdamW ``enable_ema``: one flat buffer laid out like
the masters, so under ZeRO-1 it is sharded 1/W like them) and is blended
inside the AdamW launch (``train_adamw_ema_step``).  Every other
floating-point entry that training changes -- the BatchNorm running
statistics -- is blended into a second flat fp32 buffer by ONE ``train_ema_update`` launch
over a device table of their addresses.  On the CPU (config C1,
torch.optim.AdamW) the same blend is a pair of torch ops per tensor
(``_blend_``): the readable statement of the semantics.

The blend itself is fp32: d32 = float32(d_t), then
``ema = fma(d32, ema, (float32(1) - d32) * value)``.
"""
from __future__ import annotations

import math
from contextlib import contextmanager

import numpy as np
import torch
from torch import nn


def ema_decay_at(t: int, decay: float = 0.9999, tau: float = 2000.0) -> float:
    """Decay of update ``t`` (t = 1 for the first), on the host in double."""
    return float(decay) * (1.0 - math.exp(-float(t) / float(tau)))


def _blend_(ema: torch.Tensor, value: torch.Tensor, d: float):
    """ema = d ema + (1 - d) value in fp32, with d and 1 - d rounded as the kernels round them."""
    d32 = np.float32(d)
    omd = np.float32(1.0) - d32
    ema.mul_(float(d32)).add_(value.detach().to(torch.float32), alpha=float(omd))


def _constant_entries(model: nn.Module) -> set:
    """State-dict names that training never changes: FrozenBatchNorm2d's
    buffers and parameters without a gradient.  The average of such a value is
    the value itself; running the fp32 blend on it would only add rounding
    drift (d32 + (1 - d32) is not exactly 1 while d32 < 0.5).  So they are not
    blended, ``state_dict`` takes them from the live model, and ``applied``
    leaves them alone -- which it must: FrozenBatchNorm2d caches its scale /
    shift by the buffers' version counters, and a captured step graph reads
    that cache by address."""
    from .backbone import FrozenBatchNorm2d

    out = {n for n, p in model.named_parameters() if not p.requires_grad}
    for name, m in model.named_modules():
        if isinstance(m, FrozenBatchNorm2d):
            out |= {f"{name}.{b}" if name else b for b, _ in m.named_buffers(recurse=False)}
    return out


class ModelEMA:
    """``opt``: the step's optimizer when it is one of ours (FlatAdamW /
    ShardedDPAdamW: the GPU path), else None (torch ops; the optimizer is
    stepped by the caller before ``update``).  Build it after the optimizer has
    taken over the parameters and before the first step: the average starts at
    the initial weights, as Ultralytics' deepcopy does."""

    def __init__(self, model: nn.Module, opt=None, decay: float = 0.9999, tau: float = 2000.0):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"EMA decay {decay} outside [0, 1)")
        if not float(tau) > 0.0:
            raise ValueError(f"EMA tau {tau} must be positive")
        self.model = model
        self.decay, self.tau = float(decay), float(tau)
        self.updates = 0
        self.opt = opt if hasattr(opt, "enable_ema") else None
        self.constant = _constant_entries(model)
        entries = model.state_dict(keep_vars=True)
        if self.opt is None:
            self.shadow = {k: v.detach().clone().to(torch.float32) for k, v in entries.items()
                           if v.is_floating_point() and k not in self.constant}
            return
        from .optim import CHUNK

        self.opt.enable_ema()
        owned = {id(p) for p in self.opt.params}
        # every other floating-point entry that training changes: one flat fp32 average of their own
        self.rest = [(k, v) for k, v in entries.items()
                     if v.is_floating_point() and id(v) not in owned and k not in self.constant]
        self.rest_off, off = [], 0
        for _, v in self.rest:
            self.rest_off.append(off)
            off += (v.numel() + 7) // 8 * 8
        dev = self.opt.device
        self.rest_ema = torch.zeros(max(off, 8), dtype=torch.float32, device=dev)
        chunks = [(i, c) for i, (_, v) in enumerate(self.rest) for c in range((v.numel() + CHUNK - 1) // CHUNK)]
        self.n_chunks = len(chunks)
        self.chunks = torch.tensor(chunks if chunks else [(0, 0)], dtype=torch.int32, device=dev).reshape(-1, 2)
        self._staged = {}
        self._ptrs = None
        self._table = None
        with torch.no_grad():
            for (_, v), o in zip(self.rest, self.rest_off):
                self.rest_ema[o:o + v.numel()].copy_(self._flat(v))

    # -- schedule ------------------------------------------------------------
    def decay_at(self, t: int) -> float:
        return ema_decay_at(t, self.decay, self.tau)

    # -- update --------------------------------------------------------------
    @staticmethod
    def _flat(v):
        from .optim import _storage_flat

        return _storage_flat(v.detach())

    def _source(self, i, v):
        """The tensor the kernel reads entry ``i`` from: the live buffer, or a
        16-B aligned fp32 staging copy of it (other dtypes, odd addresses)."""
        if v.dtype in (torch.float32, torch.bfloat16) and v.data_ptr() % 16 == 0:
            return self._flat(v)
        buf = self._staged.get(i)
        if buf is None:
            buf = self._staged[i] = torch.empty(v.numel(), dtype=torch.float32, device=v.device)
        buf.copy_(self._flat(v))
        return buf

    def _build_table(self, srcs):
        from .optim import _REC

        rec = np.zeros(max(len(srcs), 1), dtype=_REC)
        for i, s in enumerate(srcs):
            rec[i]["grad"] = s.data_ptr()
            rec[i]["numel"] = s.numel()
            rec[i]["moff"] = self.rest_off[i]
            rec[i]["gdtype"] = 0 if s.dtype == torch.bfloat16 else 1
        self._table = torch.from_numpy(rec.view(np.uint8).copy()).to(self.rest_ema.device)

    @torch.no_grad()
    def update(self, grads=None, **step_kw):
        """One update, once per optimizer step.  GPU: runs the optimizer step
        itself (``opt.step(grads, ema_decay=d_t, **step_kw)``: the parameters'
        blend is part of the AdamW launch), then blends the other entries in
        one launch.  CPU: the caller has stepped the optimizer; blends every
        floating-point entry with torch ops."""
        self.updates += 1
        d = self.decay_at(self.updates)
        if self.opt is None:
            live = self.model.state_dict(keep_vars=True)
            for k, e in self.shadow.items():
                _blend_(e, live[k], d)
            return
        from ..moe import _lib as L

        self.opt.step(grads, ema_decay=d, **step_kw)
        if not self.rest:
            return
        srcs = [self._source(i, v) for i, (_, v) in enumerate(self.rest)]
        ptrs = tuple(s.data_ptr() for s in srcs)
        if ptrs != self._ptrs:
            self._build_table(srcs)
            self._ptrs = ptrs
        L._check(L.lib().train_ema_update(self._table.data_ptr(), self.chunks.data_ptr(), self.n_chunks,
                                          self.rest_ema.data_ptr(), d, L._stream()), "train_ema_update")

    # -- the averaged model ----------------------------------------------------
    def _param_averages(self):
        """{id(parameter): fp32 average in the parameter's layout} of the
        optimizer's parameters (one all-gather under the sharded optimizer)."""
        opt = self.opt
        allm = opt.gather_slices(opt.ema) if hasattr(opt, "gather_slices") else None
        out = {}
        for p in opt.params:
            seg = opt._gathered(opt.ema, p, allm) if allm is not None else opt.ema_of(p)
            out[id(p)] = seg.as_strided(p.shape, p.stride())
        return out

    @torch.no_grad()
    def state_dict(self) -> dict:
        """The model's state dict (same names and shapes) with every
        floating-point entry replaced by its fp32 average (its fp32 value for an
        entry training never changes); integer entries are the live model's.  Under the sharded optimizer a collective (every rank
        calls it); expert-parallel shards stay this rank's shards, as in
        ``model.state_dict()``."""
        live = self.model.state_dict(keep_vars=True)
        if self.opt is None:
            return {k: (self.shadow[k].clone() if k in self.shadow else self._live(v)) for k, v in live.items()}
        avg = self._param_averages()
        rest = {k: self.rest_ema[o:o + v.numel()].as_strided(v.shape, v.stride())
                for (k, v), o in zip(self.rest, self.rest_off)}
        out = {}
        for k, v in live.items():
            if id(v) in avg:
                out[k] = avg[id(v)].clone()
            elif k in rest:
                out[k] = rest[k].clone()
            else:
                out[k] = self._live(v)
        return out

    @staticmethod
    def _live(v):
        v = v.detach()
        return v.to(torch.float32, copy=True) if v.is_floating_point() else v.clone()

    @contextmanager
    def applied(self):
        """Validate the averaged model: inside the context the live parameters
        and buffers hold the averages (written in place, RNE to bf16 for bf16
        weights, so every address a captured graph reads stays valid); on exit
        every parameter, buffer, master and optimizer moment is restored bit
        for bit.  Entries that training never changes (_constant_entries) keep
        their live value, which is their average.  Enter in train mode: the evaluation's own ``model.eval()``
        then folds BatchNorm from the averaged weights (evalfold.py) and the
        next ``model.train()`` drops the fold.  Under the sharded optimizer
        entering is a collective (an all-gather of the slices' averages into
        the flat parameter spaces): every rank enters."""
        with torch.no_grad():
            undo = self._apply()
        try:
            yield self
        finally:
            with torch.no_grad():
                for dst, saved in undo:
                    dst.copy_(saved)

    def _apply(self):
        """Write the averages over the live values; returns [(tensor, its
        saved contents)] for everything overwritten."""
        undo = []

        def put(dst, src):
            undo.append((dst, dst.clone()))
            dst.copy_(src)

        if self.opt is None:
            live = self.model.state_dict(keep_vars=True)
            for k, e in self.shadow.items():
                put(live[k].detach(), e)
            return undo
        opt = self.opt
        if hasattr(opt, "PB"):
            # ZeRO-1: the replicated parameters are views of PB / PF (the masters are
            # separate): this rank's slice of the averages, all-gathered over them
            from .optim import _collective

            Sb, Sf = opt.S
            r = opt.rank
            undo += [(opt.PB, opt.PB.clone()), (opt.PF, opt.PF.clone())]
            opt.PB[r * Sb:(r + 1) * Sb].copy_(opt.ema[:Sb])
            opt.PF[r * Sf:(r + 1) * Sf].copy_(opt.ema[Sb:Sb + Sf])
            _collective("ag", opt.PB, opt.PB[r * Sb:(r + 1) * Sb], opt.group)
            _collective("ag", opt.PF, opt.PF[r * Sf:(r + 1) * Sf], opt.group)
            for i in opt.ep_idx:
                p = opt.params[i]
                put(self._flat(p), opt.ema_of(p))
        else:
            # fp32 parameters are views of their master segment: the masters are
            # saved whole and overwritten by the average; bf16 weights one by one
            undo.append((opt.master, opt.master.clone()))
            opt.master.copy_(opt.ema)
            for p in opt.params:
                if p.dtype == torch.bfloat16:
                    put(self._flat(p), opt.ema_of(p))
        for (_, v), o in zip(self.rest, self.rest_off):
            put(self._flat(v), self.rest_ema[o:o + v.numel()])
        return undo
