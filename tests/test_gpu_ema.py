"""The weight average on the GPU (csrc/optim.hip: train_adamw_ema_step,
train_ema_update; optim.FlatAdamW.enable_ema).  The reference's Ultralytics
trainer keeps ema = d_t ema + (1 - d_t) w after every optimizer step
(src/models/vision/rtdetr.py:82-94 trains through it).

Numerical reference: the fp64 recurrence over the optimizer's OWN masters
(``master_of`` after each step), with d32 = float32(d_t) and omd32 =
float32(1) - d32 computed in fp32 and widened, so AdamW's rounding never
enters.  Tolerance, derived: a step rounds one product and one fma, at most
2^-23 A of new error, and multiplies the error so far by d < 1; after n steps
|ema - ref| <= n 2^-22 A elementwise (A = the largest |master| or |ema| seen;
a factor 2 of margin)."""
from __future__ import annotations

import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

DEV = "cuda"
DECAY, TAU, STEPS = 0.9, 2.0, 4
SKIP = (2, 4)  # (step, tensor) without a gradient
# tests/test_gpu_optim.py::_params' shapes (channels-last 4-D, tails of 5 and
# 4096+7, 2 x 2049) + numel 8, 2047, 2048: every chunk- and vector-boundary
# case of a 2048-element chunk with 8-wide vectors
SHAPES = [((37, 13, 3, 3), torch.bfloat16, True), ((37,), torch.bfloat16, False), ((5,), torch.float32, False),
          ((1000, 3), torch.float32, False), ((4096 + 7,), torch.bfloat16, False), ((2, 2049), torch.float32, False),
          ((64, 16, 1, 1), torch.bfloat16, True), ((8,), torch.float32, False), ((2047,), torch.bfloat16, False),
          ((2048,), torch.float32, False)]


def make_params(seed=0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp, dt, cl in SHAPES:
        t = (torch.randn(shp, generator=g) * 0.1).to(dev)
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(torch.nn.Parameter(t.to(dt)))
    return out


def make_grads(ps, step, g):
    grads = []
    for i, p in enumerate(ps):
        gr = (torch.randn(p.shape, generator=g) * (0.3 + i)).to(p.device).to(p.dtype)  # drawn for every tensor
        if p.dim() == 4:
            gr = gr.contiguous(memory_format=torch.channels_last)
        grads.append(None if (step, i) == SKIP else gr)
    return grads


def decay32(t, decay=DECAY, tau=TAU):
    """(d32, omd32) of update t as doubles: the fp32 values the kernel blends with."""
    d32 = np.float32(decay * (1.0 - math.exp(-t / tau)))
    return float(d32), float(np.float32(1.0) - d32)


def reference_track(masters, start):
    """fp64 recurrence over per-step masters [n][tensor] from ``start``; returns
    (per-step references, A per tensor)."""
    ref = [s.double() for s in start]
    A = [float(s.abs().max()) for s in start]
    out = []
    for t, ms in enumerate(masters, 1):
        d, omd = decay32(t)
        ref = [d * r + omd * m.double() for r, m in zip(ref, ms)]
        A = [max(a, float(m.abs().max()), float(r.abs().max())) for a, m, r in zip(A, ms, ref)]
        out.append(ref)
    return out, A


@functools.lru_cache(maxsize=None)
def _run(mode):
    """Four steps of FlatAdamW over SHAPES, two lr groups; mode "off" (no
    average), "fused" (train_adamw_ema_step) or "unfused" (MOE_EMA_FUSED=0)."""
    from src.rtdetr_moe.ema import ema_decay_at
    from src.rtdetr_moe.optim import FlatAdamW, _storage_flat

    ps = make_params()
    opt = FlatAdamW([(ps[:3], 1e-3), (ps[3:], 3e-4)], weight_decay=1e-2, clip_norm=0.05)
    if mode != "off":
        opt.enable_ema()
    old = os.environ.get("MOE_EMA_FUSED")
    os.environ["MOE_EMA_FUSED"] = "0" if mode == "unfused" else "1"
    try:
        g = torch.Generator().manual_seed(1)
        res = {"start": [opt.master_of(p).clone() for p in ps], "masters": [], "emas": [], "coef": []}
        for step in range(STEPS):
            opt.step(make_grads(ps, step, g), ema_decay=None if mode == "off" else ema_decay_at(step + 1, DECAY, TAU))
            torch.cuda.synchronize()
            res["masters"].append([opt.master_of(p).clone() for p in ps])
            res["coef"].append(opt.coef.clone())
            if mode != "off":
                res["emas"].append([opt.ema_of(p).clone() for p in ps])
    finally:
        if old is None:
            os.environ.pop("MOE_EMA_FUSED")
        else:
            os.environ["MOE_EMA_FUSED"] = old
    res.update(exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), master=opt.master.clone(),
               weights=[_storage_flat(p.detach()).clone() for p in ps], tsteps=opt.tsteps.clone(),
               ema=None if opt.ema is None else opt.ema.clone())
    return res


@pytest.mark.gpu
def test_fused_ema_matches_the_recurrence(hip_lib):
    r = _run("fused")
    refs, A = reference_track(r["masters"], r["start"])
    for n, (ref, got) in enumerate(zip(refs, r["emas"]), 1):
        for i, (a, b) in enumerate(zip(ref, got)):
            A[i] = max(A[i], float(b.abs().max()))
            err = float((b.double() - a).abs().max())
            assert err <= n * 2.0 ** -22 * A[i], (n, i, err, A[i])
    assert float((r["emas"][-1][0] - r["masters"][-1][0]).abs().max()) > 1e-4  # an average, not a copy
    # the tensor without a gradient at step 2: its master stands still, its average still closes in on it
    s, i = SKIP
    m = r["masters"][s][i]
    assert torch.equal(m, r["masters"][s - 1][i])
    before, after = r["emas"][s - 1][i], r["emas"][s][i]
    assert not torch.equal(before, after)
    assert float((after - m).abs().sum()) < float((before - m).abs().sum())
    d, omd = decay32(s + 1)
    assert float((after.double() - (d * before.double() + omd * m.double())).abs().max()) <= 2.0 ** -22 * A[i]


@pytest.mark.gpu
def test_ema_does_not_perturb_the_update(hip_lib):
    a, b = _run("off"), _run("fused")
    for k in ("master", "exp_avg", "exp_avg_sq", "tsteps"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
    assert all(torch.equal(x, y) for x, y in zip(a["coef"], b["coef"]))


@pytest.mark.gpu
def test_fused_equals_unfused(hip_lib):
    a, b = _run("fused"), _run("unfused")
    assert torch.equal(a["ema"], b["ema"])
    assert torch.equal(a["master"], b["master"])


def _table(srcs, offs):
    from src.rtdetr_moe.optim import CHUNK, _REC

    rec = np.zeros(len(srcs), dtype=_REC)
    for i, (s, o) in enumerate(zip(srcs, offs)):
        rec[i]["grad"] = s.data_ptr()
        rec[i]["numel"] = s.numel()
        rec[i]["moff"] = o
        rec[i]["gdtype"] = 0 if s.dtype == torch.bfloat16 else 1
    chunks = [(i, c) for i, s in enumerate(srcs) for c in range((s.numel() + CHUNK - 1) // CHUNK)]
    return (torch.from_numpy(rec.view(np.uint8).copy()).to(DEV),
            torch.tensor(chunks, dtype=torch.int32, device=DEV).reshape(-1, 2))


@pytest.mark.gpu
def test_ema_update_on_buffers(hip_lib):
    """train_ema_update over bf16 and fp32 sources of numel 5, 8 and 2049 (a
    tail, one full vector, a second chunk with a one-element tail)."""
    from src.moe import _lib as L

    g = torch.Generator().manual_seed(5)
    sizes = [5, 8, 2049]
    offs, off = [], 0
    for n in sizes * 2:
        offs.append(off)
        off += (n + 7) // 8 * 8
    srcs = [torch.zeros(n, dtype=dt, device=DEV) for dt in (torch.bfloat16, torch.float32) for n in sizes]
    wide = [torch.zeros(n, dtype=torch.float32, device=DEV) for n in sizes]  # the bf16 sources widened
    tab, chunks = _table(srcs, offs)
    wtab, wchunks = _table(wide, offs[:3])
    ema = torch.randn(off, generator=g).to(DEV)
    ema_w = ema.clone()
    untouched = torch.ones(off, dtype=torch.bool)
    for n, o in zip(sizes * 2, offs):
        untouched[o:o + n] = False
    start = ema.clone()
    ref = [ema[o:o + n].double() for n, o in zip(sizes * 2, offs)]
    A = [float(r.abs().max()) for r in ref]
    for t in range(1, 4):
        for s in srcs:
            s.copy_(torch.randn(s.shape, generator=g).to(DEV))
        for w, s in zip(wide, srcs):
            w.copy_(s)
        d = DECAY * (1.0 - math.exp(-t / TAU))
        d32, omd = decay32(t)
        for tb, ch, e in ((tab, chunks, ema), (wtab, wchunks, ema_w)):
            L._check(hip_lib.train_ema_update(tb.data_ptr(), ch.data_ptr(), ch.shape[0], e.data_ptr(), d,
                                              L._stream()), "train_ema_update")
        torch.cuda.synchronize()
        for i, (n, o, s) in enumerate(zip(sizes * 2, offs, srcs)):
            ref[i] = d32 * ref[i] + omd * s.double()
            got = ema[o:o + n]
            A[i] = max(A[i], float(s.float().abs().max()), float(ref[i].abs().max()), float(got.abs().max()))
            assert float((got.double() - ref[i]).abs().max()) <= t * 2.0 ** -22 * A[i], (t, i)
    assert torch.equal(ema.cpu()[untouched], start.cpu()[untouched])  # padding between segments is not written
    for n, o in zip(sizes, offs):  # a bf16 source is its fp32 widening, exactly
        assert torch.equal(ema[o:o + n], ema_w[o:o + n])


def _optim_launches(lib):
    counts = (ctypes.c_longlong * 16)()
    assert lib.moe_launch_counts(counts, 16) == 0
    return counts[8]  # kind 8: optimizer


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(hip_lib):
    from src.moe import _lib as L

    n = 2049
    src = torch.randn(n, device=DEV)
    tab, chunks = _table([src], [0])
    ema = torch.zeros(2056 + 8, device=DEV)
    keep = ema.clone()
    z = torch.zeros(2056, device=DEV)
    coef = torch.ones(2, device=DEV)
    tsteps = torch.ones(1, dtype=torch.int32, device=DEV)
    lrs = (ctypes.c_float * 1)(1e-3)
    s = L._stream()

    def update(e, d):
        return hip_lib.train_ema_update(tab.data_ptr(), chunks.data_ptr(), chunks.shape[0], e, d, s)

    def adamw(e, d):
        return hip_lib.train_adamw_ema_step(tab.data_ptr(), chunks.data_ptr(), chunks.shape[0], coef.data_ptr(),
                                            z.data_ptr(), z.data_ptr(), z.data_ptr(), tsteps.data_ptr(), lrs, 1,
                                            0.0, 0.9, 0.999, 1e-8, e, d, s)

    hip_lib.moe_launch_counts_reset()
    for fn, name in ((update, "train_ema_update"), (adamw, "train_adamw_ema_step")):
        for e, d in ((ema.data_ptr(), 1.0), (ema.data_ptr(), -0.1), (None, 0.5), (ema.data_ptr() + 4, 0.5),
                     (ema.data_ptr(), float("nan"))):
            assert fn(e, d) != 0, (name, e, d)
            assert name in hip_lib.moe_last_error().decode()
    assert _optim_launches(hip_lib) == 0
    torch.cuda.synchronize()
    assert torch.equal(ema, keep) and not z.any()
    # no chunks: accepted, nothing launched; a good call launches exactly once
    assert hip_lib.train_ema_update(None, None, 0, ema.data_ptr(), 0.5, s) == 0
    assert _optim_launches(hip_lib) == 0
    assert update(ema.data_ptr(), 0.5) == 0
    assert _optim_launches(hip_lib) == 1
    torch.cuda.synchronize()
    assert torch.equal(ema[:n], 0.5 * src) and torch.equal(ema[n:], keep[n:])
