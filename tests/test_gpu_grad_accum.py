"""Gradient accumulation on the GPU (csrc/optim.hip: train_grad_accum;
optim.GradAccumulator) and the optimizer fed from it.  The reference's
Ultralytics trainer accumulates nbs / batch batches per optimizer step
(src/models/vision/rtdetr.py:82-94 trains through it).

The kernel is checked bit for bit (torch.equal) against
``acc = g1.float(); acc += g2.float(); acc += g3.float()`` in torch: one thread
owns each element and the sums happen in micro-step order, so there is no
rounding freedom.  The optimizer on the accumulated sums is bit-equal to the
same optimizer on the torch sums, and within rtol 2e-5 / atol 1e-7 of
clip_grad_norm_ + torch.optim.AdamW on the mean gradient: the project's figure
for fp32 masters against torch with a different operation order
(tests/test_gpu_optim.py)."""
from __future__ import annotations

import functools

import pytest
import torch

DEV = "cuda"
MICRO = 3
SENTINEL = 12345.0
# numel 1, 7, 8, 9: the 8-wide vector and its tail; 2047, 2048, 2049: the edge of a 2048-element
# chunk; 4096 + 7: several chunks and a tail; a channels-last 4-D tensor (storage order);
# SKIP2 has no gradient in the second micro-step only, NEVER in none
SHAPES = [((1,), torch.float32, False), ((7,), torch.bfloat16, False), ((8,), torch.float32, False),
          ((9,), torch.bfloat16, False), ((2047,), torch.bfloat16, False), ((2048,), torch.float32, False),
          ((2049,), torch.float32, False), ((4096 + 7,), torch.bfloat16, False),
          ((6, 5, 3, 3), torch.bfloat16, True), ((33,), torch.float32, False), ((19,), torch.bfloat16, False)]
CL, SKIP2, NEVER = 8, 9, 10
FP32_GRAD = (2, 3)  # (micro-step, tensor): an fp32 gradient of a bf16 parameter


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp, dt, cl in SHAPES:
        t = (torch.randn(shp, generator=g) * 0.1).to(DEV)
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(torch.nn.Parameter(t.to(dt)))
    return out


def _grads(ps, seed=1):
    """[micro-step][tensor]: the parameter's dtype and layout, except one fp32
    gradient of a bf16 parameter and, in the second micro-step, the
    channels-last tensor's gradient in the contiguous layout (staged)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for m in range(MICRO):
        row = []
        for i, p in enumerate(ps):
            gr = (torch.randn(p.shape, generator=g) * (0.3 + i)).to(DEV)  # drawn for every tensor
            gr = gr if (m, i) == FP32_GRAD else gr.to(p.dtype)
            if p.dim() == 4:
                gr = gr.contiguous(memory_format=torch.contiguous_format if m == 1 else torch.channels_last)
            row.append(None if i == NEVER or (i == SKIP2 and m == 1) else gr)
        out.append(row)
    return out


def _torch_sums(ps, grads):
    """acc = g1.float(); acc += g2.float(); ... in the parameter's layout; None without any gradient."""
    sums = []
    for i, p in enumerate(ps):
        acc = None
        for row in grads:
            g = row[i]
            if g is None:
                continue
            g32 = torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=p.device).copy_(g.float())
            if acc is None:
                acc = g32
            else:
                acc += g32
        sums.append(acc)
    return sums


def _gaps(acc):
    """[(start, end)] of the alignment gaps behind the segments of the flat buffer."""
    ends = acc.offsets[1:] + [acc.flat.numel()]
    return [(o + p.numel(), e) for p, o, e in zip(acc.params, acc.offsets, ends) if o + p.numel() < e]


@functools.lru_cache(maxsize=None)
def _accumulated():
    from src.rtdetr_moe.optim import GradAccumulator, _storage_flat

    ps = _params()
    grads = _grads(ps)
    acc = GradAccumulator(ps)
    acc.flat.fill_(float("nan"))
    gaps = _gaps(acc)
    for a, b in gaps:
        acc.flat[a:b] = SENTINEL
    for m in range(MICRO):
        acc.add(grads[m])
    torch.cuda.synchronize()
    flat = acc.flat.clone()
    counts = (acc.count,)
    taken, count = acc.take()
    got = [None if t is None else _storage_flat(t).clone() for t in taken]
    want = [None if s is None else _storage_flat(s) for s in _torch_sums(ps, grads)]
    return dict(flat=flat, gaps=gaps, got=got, want=want, count=count, counts=counts + (acc.count,),
                offsets=list(acc.offsets), numels=[p.numel() for p in ps])


@pytest.mark.gpu
def test_kernel_equals_torch_sums(hip_lib):
    r = _accumulated()
    assert r["count"] == MICRO and r["counts"] == (MICRO, 0)
    for i, (got, want) in enumerate(zip(r["got"], r["want"])):
        if i == NEVER:
            continue
        assert got.dtype == torch.float32 and torch.equal(got, want), i
        seg = r["flat"][r["offsets"][i]:r["offsets"][i] + r["numels"][i]]
        assert torch.equal(seg, want), i  # take() hands out views of the flat buffer
    assert not torch.isnan(r["flat"]).any()  # the first launch overwrote every element of every segment


@pytest.mark.gpu
def test_gaps_and_missing_gradients(hip_lib):
    r = _accumulated()
    assert len(r["gaps"]) >= 6
    for a, b in r["gaps"]:
        assert bool((r["flat"][a:b] == SENTINEL).all()), (a, b)  # nothing written outside a tensor
    assert r["got"][NEVER] is None and r["want"][NEVER] is None
    o = r["offsets"][NEVER]
    assert bool((r["flat"][o:o + r["numels"][NEVER]] == 0).all())  # zeros from the first launch
    assert r["got"][SKIP2] is not None  # a gradient in two of the three micro-steps: their sum


@pytest.mark.gpu
def test_table_is_kept_while_addresses_stand(hip_lib):
    from src.rtdetr_moe.optim import GradAccumulator

    ps = _params()
    grads = _grads(ps)[0]
    acc = GradAccumulator(ps)
    acc.add(grads)
    table = acc._table
    acc.add(grads)
    assert acc._table is table
    taken, count = acc.take()
    torch.cuda.synchronize()
    assert count == 2 and torch.equal(taken[1], grads[1].float() + grads[1].float())
    acc.add(grads)  # a new cycle overwrites: no trace of the last one
    assert acc._table is table
    torch.cuda.synchronize()
    assert torch.equal(acc.take()[0][1], grads[1].float())
    with pytest.raises(RuntimeError):
        acc.take()


@pytest.mark.gpu
def test_argument_checks(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.optim import GradAccumulator

    ps = _params()
    acc = GradAccumulator(ps)
    acc.add(_grads(ps)[0])
    torch.cuda.synchronize()
    before = acc.flat.clone()
    s = L._stream()
    tab, ch, n, flat = acc._table.data_ptr(), acc.chunks.data_ptr(), acc.n_chunks, acc.flat.data_ptr()
    assert hip_lib.train_grad_accum(tab, ch, n, flat + 4, 0, s) != 0      # misaligned accumulator
    assert b"16-B aligned" in hip_lib.moe_last_error()
    assert hip_lib.train_grad_accum(tab, ch, n, None, 0, s) != 0
    assert hip_lib.train_grad_accum(None, ch, n, flat, 0, s) != 0
    assert hip_lib.train_grad_accum(tab, None, n, flat, 1, s) != 0
    assert hip_lib.train_grad_accum(tab, ch, -1, flat, 0, s) != 0
    assert hip_lib.train_grad_accum(None, None, 0, flat, 1, s) == 0        # nothing to do: no launch
    torch.cuda.synchronize()
    assert torch.equal(acc.flat, before)  # a refused call launches nothing


@pytest.mark.gpu
def test_reducer_takes_accumulated_gradients(hip_lib):
    """The MOE_ZERO=0 data-parallel path packs an accumulation cycle's fp32
    sums (of bf16 parameters too) as it packs the gradients themselves."""
    from src.rtdetr_moe.optim import DPGradReducer, GradAccumulator

    ps = _params()
    grads = _grads(ps)
    acc = GradAccumulator(ps)
    for row in grads:
        acc.add(row)
    taken, _ = acc.take()
    out = DPGradReducer(ps)(taken)  # one process: the pack, no all-reduce
    torch.cuda.synchronize()
    for i, (o, t) in enumerate(zip(out, taken)):
        if i == NEVER:
            assert o is None and t is None
        else:
            assert o.dtype == torch.float32 and o.stride() == ps[i].stride() and torch.equal(o, t), i


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 0.05])
def test_optimizer_on_accumulated_gradients(hip_lib, clip):
    from src.rtdetr_moe.optim import FlatAdamW, GradAccumulator, _storage_flat

    inv = 1.0 / MICRO
    kw = dict(weight_decay=1e-2, clip_norm=clip)
    ps, twin_ps = _params(), _params()
    ref = [torch.nn.Parameter(p.detach().float().clone()) for p in ps]  # torch's fp32 masters (same strides)
    grads = _grads(ps)
    sums = _torch_sums(ps, grads)
    opt = FlatAdamW([(ps[:3], 1e-3), (ps[3:], 3e-4)], **kw)
    twin = FlatAdamW([(twin_ps[:3], 1e-3), (twin_ps[3:], 3e-4)], **kw)
    topt = torch.optim.AdamW([{"params": ref[:3], "lr": 1e-3}, {"params": ref[3:], "lr": 3e-4}], lr=1e-3,
                             weight_decay=1e-2, foreach=False)
    acc = GradAccumulator(opt.params)
    for m in range(MICRO):
        acc.add(grads[m])
    taken, count = acc.take()
    assert count == MICRO and taken[NEVER] is None
    opt.step(taken, inv_world=1.0 / count)
    twin.step(sums, inv_world=inv)
    for r, s in zip(ref, sums):
        r.grad = None if s is None else s * inv  # the mean gradient
    if clip > 0:
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], clip, foreach=False)
    topt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt.master, twin.master) and torch.equal(opt.exp_avg, twin.exp_avg)
    assert torch.equal(opt.exp_avg_sq, twin.exp_avg_sq) and torch.equal(opt.coef, twin.coef)
    for i, (p, r) in enumerate(zip(ps, ref)):
        m = opt.master_of(p)
        torch.testing.assert_close(m, _storage_flat(r.detach()), rtol=2e-5, atol=1e-7)
        if p.dtype == torch.bfloat16:
            assert torch.equal(_storage_flat(p.detach()), m.to(torch.bfloat16)), i  # RNE of the master
        else:
            assert torch.equal(_storage_flat(p.detach()), m), i
    assert torch.equal(opt.master_of(ps[NEVER]), _storage_flat(ref[NEVER].detach()))  # skipped by both
    # the norm is that of the mean gradient
    tn = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(s * inv) for s in sums if s is not None]))
    assert abs(float(opt.grad_norm()) - float(tn)) <= 1e-4 * float(tn)
