"""One RT-DETR-MoE training step (TrainStep), in one of three modes.

Whole-step graph (GPU, graphs=True with targets=; GraphedStep): the model's
forward through the project's HIP kernels, the set criterion with the GPU
Hungarian matcher (fused: matching + losses in three HIP launches), the
denoising losses and the backward to every parameter are ONE hipGraph.  Its
inputs -- images, context ids, padded targets, box count, the denoising pack
-- live in static buffers refreshed by device copies before each replay; no
host round trip inside the step.  Issued eagerly from Python and the autograd
engine the same launches take the host longer to enqueue than the GPU takes to
run them.  This is what bench.py times and engine.train drives.

Graph pair (GPU, graphs=True without targets; GraphedModel): the forward and
the backward are one replay each; between them the batched set criterion runs
eagerly on the list of targets, with the Hungarian matching on the host (one
device->host copy of all cost matrices).  The backward graph computes
torch.autograd.grad of the forward outputs w.r.t. every trainable parameter.
The captured forward keeps the MoE aux losses as an explicit graph output so
their gradients reach the router through the captured backward.

Eager (GPU with graphs=False or after use_eager(); CPU): forward, criterion
and loss.backward() issued from Python; on the CPU in fp32 with
torch.optim.AdamW, at world > 1 under DDP.

In both graph modes the gradients land in static buffers that the optimizer
reads directly (no per-parameter AccumulateGrad copies).  Every capture goes
through one skeleton, _capture_session: warm-up and capture on the same side
stream, which keeps the captured graph a single chain.

What stays outside every graph:
- the optimizer (optim.FlatAdamW: gradient clip + AdamW + bf16 weight refresh
  in three HIP launches; at world > 1 optim.ShardedDPAdamW: one fp32
  reduce-scatter over RCCL, AdamW on this rank's slice, one all-gather of the
  weights), and inside its AdamW launch the weight average (ema.ModelEMA);
- batch augmentation (an -aug model spec, augment.BatchAugment), in front of
  the step: with the whole-step graph its two HIP launches write the graph's
  static images, padded targets and box count directly.  With mosaic (a
  -mosaic spec, TrainStep(mosaic=p)) an image carries the boxes of up to four,
  so the padding M is reserved from the augmenter's host bound
  (BatchAugment.need) before the launches;
- the denoising queries' noise (a -dn<N> spec, DenoisingState.pack), drawn
  into the graph's static pack next to the targets;
- gradient accumulation (an -nbs<N> spec, TrainStep(accumulate=K)): a replay
  overwrites the static gradient buffers, so after each one a HIP launch adds
  them to an fp32 sum (optim.GradAccumulator); every K-th call runs the
  data-parallel exchange and the optimizer once, on the mean gradient;
- loss-free load balancing (an -alb spec, moe.balance.LoadBalancer): one HIP
  launch after each replay adds every MoE layer's expert histogram to an int64
  load table, and one ahead of the optimizer step moves the layers' selection
  biases, which the captured router launches read by address.
"""
from __future__ import annotations

import os
import time
from contextlib import contextmanager

import torch
import torch.distributed as dist
from torch import nn

from .augment import targets_from_padded
from .conv import check_grad_slots
from .criterion import pad_capacity, pad_targets
from .denoising import DenoisingConfig, dn_shapes, make_denoising
from .linear import TokenSelfAttention, deferred_weight_grads, merge_deferred
from .model import RTDETRMoE
from .schedule import accumulate_count

_FUSED_CRIT = os.environ.get("MOE_FUSED_CRITERION", "1") != "0"  # A/B switch
# MOE_ZERO=0: GPU data parallelism through the flat fp32 all-reduce + replicated
# FlatAdamW (optim.DPGradReducer) instead of the sharded optimizer (A/B switch)
_ZERO = os.environ.get("MOE_ZERO", "1") != "0"

# Stream-capture mode of every hipGraph capture (step graphs, the evaluation
# forward): "thread_local", so that only the capturing thread is restricted.
# It is NOT what keeps a capture that holds RCCL collectives (the C4
# expert-parallel all-to-alls) alive -- quiesce_collectives is: the process
# group's watchdog thread polls the end events of recent eager collectives,
# and a poll that lands while the capture is open, with the RCCL stream joined
# into it, fails with hipErrorCapturedEvent and terminates the process (in
# either mode: tools/rccl_capture_probe.py, gpurun_out/r6b global, r6p
# thread_local; with the drain: r6c).
CAPTURE_MODE = "thread_local"
# Seconds to let the RCCL watchdog retire the warm-up's eager collectives
# before a capture opens (quiesce_collectives; its poll period is ~100 ms).
_DRAIN_S = float(os.environ.get("MOE_CAPTURE_DRAIN_S", "0.5"))


def rccl_env():
    """Call before every ``init_process_group("nccl")``: one CUDA event per
    collective instead of torch's recycled event cache, so that no event a
    capture recorded (captured collectives' end events) is ever handed to an
    eager collective that the watchdog then polls.  Together with
    quiesce_collectives this leaves the watchdog only eagerly recorded,
    completed events to look at."""
    os.environ.setdefault("TORCH_NCCL_CUDA_EVENT_CACHE", "0")


def quiesce_collectives():
    """Before opening a capture while an RCCL group is live: drain the device,
    then give the group's watchdog time to retire every completed eager
    collective, so that none of their events is polled while the capture is
    open (see CAPTURE_MODE).  No eager collective may be issued between this
    call and the end of the capture."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    if "nccl" not in str(dist.get_backend()).lower():
        return
    torch.cuda.synchronize()
    if _DRAIN_S > 0:
        time.sleep(_DRAIN_S)


def _drop_autograd_graphs(model=None):
    """Release the autograd graphs of the warm-up / capture passes now.  Two
    things keep such a graph -- and the parameters' AccumulateGrad nodes in
    it, which remember the side stream they were created on -- alive past the
    capture: the MoE layers' cached aux-loss tensors (``last_aux``,
    ``last_aux_weighted``: differentiable, they reach every parameter upstream
    of the router) and the custom Functions' ctx reference cycles.  A later
    pass on another stream (the re-capture's new side stream, bench.py's eager
    profile steps) would then re-use the stale nodes and synchronise across
    streams in every step (torch's "AccumulateGrad node's stream does not
    match" warning).  The cached tensors are detached (same storage: their
    values still follow graph replays) and the cycles collected."""
    import gc

    from ..moe.layer import MoEFFN

    if model is not None:
        for m in model.modules():
            if isinstance(m, MoEFFN):
                if m.last_aux is not None:
                    m.last_aux = tuple(t.detach() if torch.is_tensor(t) else t for t in m.last_aux)
                for name in ("last_aux_weighted", "ep_aux_weighted"):
                    t = getattr(m, name, None)
                    if torch.is_tensor(t):
                        setattr(m, name, t.detach())
    gc.collect()


def release_graphs():
    """Before ``dist.destroy_process_group()``: free every unreachable captured
    graph (their captured RCCL kernels keep the communicator busy: the destroy
    then hangs, gpurun_out/r6c) and drain the device."""
    import gc

    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


@contextmanager
def _capture_session(warm, warmup, fn):
    """The skeleton of every step capture (GraphedModel's pair, GraphedStep's
    one graph).  Before the body: ``warmup`` calls of ``warm()`` (one forward +
    backward each) on a new side stream, the streams joined, the device
    drained and quiesce_collectives.  The body gets ``(pool, capture)``:
    ``with capture(graph):`` captures ``graph`` into the session's pool ON THE
    WARM-UP STREAM -- the autograd nodes the warm-up created (AccumulateGrad
    keeps the stream it was made on) then match the capture stream, so the
    backward needs no cross-stream syncs: a single chain, no fork/join branches
    for the HIP runtime to spread over parallel streams.  The body drops its
    own references to the captured passes' tensors; after it the autograd
    graphs of ``fn`` (when a Module) are released and the device drained."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: convolution search, library attributes, allocator
        for _ in range(warmup):
            warm()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    quiesce_collectives()
    pool = torch.cuda.graph_pool_handle()
    yield pool, lambda graph: torch.cuda.graph(graph, pool=pool, stream=side, capture_error_mode=CAPTURE_MODE)
    _drop_autograd_graphs(fn if isinstance(fn, nn.Module) else None)
    torch.cuda.synchronize()


def _most_boxes(targets):
    """The largest box count of one image in a batch of targets."""
    return max((len(t["boxes"]) for t in targets), default=0)


def _dense_grads(grads, params):
    """A capture's gradient outputs as the static buffers the optimizer reads:
    zeros where autograd found no path to a parameter."""
    return [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]


class FlatOutputs(nn.Module):
    """Model wrapper whose forward returns a flat tuple of tensors (a graph
    output signature): final, auxiliary and encoder logits/boxes, then -- with
    a denoising pack ``dn`` (denoising.make_denoising) -- the denoising
    logits/boxes of every decoder layer, + MoE aux loss."""

    def __init__(self, model: RTDETRMoE):
        super().__init__()
        self.model = model

    def forward(self, images, ctx, dn=None):
        out = self.model(images, ctx) if dn is None else self.model(images, ctx, dn)
        sets = [out] + list(out["aux_outputs"]) + [out["enc_outputs"]] + list(out.get("dn_outputs", []))
        flat = []
        for s in sets:
            flat += [s["pred_logits"], s["pred_boxes"]]
        aux = self.model.moe_aux_loss()
        flat.append(aux if aux is not None else out["pred_boxes"].sum() * 0.0)
        return tuple(flat)

    @staticmethod
    def unflatten(flat, n_dn=0):
        """n_dn: how many denoising pairs follow the encoder pair (0, or one per
        decoder layer)."""
        pairs = [{"pred_logits": flat[i], "pred_boxes": flat[i + 1]} for i in range(0, len(flat) - 1, 2)]
        dn_pairs = pairs[len(pairs) - n_dn:] if n_dn else []
        pairs = pairs[:len(pairs) - n_dn] if n_dn else pairs
        out = dict(pairs[0])
        out["aux_outputs"] = pairs[1:-1]
        out["enc_outputs"] = pairs[-1]
        if n_dn:
            out["dn_outputs"] = dn_pairs
        return out, flat[-1]


class _ReplayFn(torch.autograd.Function):
    """Forward = replay of the captured forward graph; backward = copy the
    incoming output gradients into the static buffers and replay the captured
    backward graph (parameter grads land in the runner's static buffers)."""

    @staticmethod
    def forward(ctx, runner, anchor):
        runner.g_fwd.replay()
        ctx.runner = runner
        return tuple(o.detach() for o in runner.static_out)

    @staticmethod
    def backward(ctx, *grads):
        r = ctx.runner
        for buf, g in zip(r.static_gout, grads):
            if g is None:
                buf.zero_()
            else:
                buf.copy_(g)
        r.g_bwd.replay()
        return None, None


class GraphedModel:
    """Capture ``fn(images, ctx) -> tuple of tensors`` forward and backward as
    two hipGraphs (see the module docstring).  After ``loss.backward()`` the
    parameter gradients are in ``static_grads`` (one per ``params`` entry)."""

    def __init__(self, fn, params, images, ctx, warmup=3, autocast=False):
        self.fn = fn
        self.params = params
        self.autocast = autocast
        self.static_images = images.clone()
        self.static_ctx = ctx.clone()
        with _capture_session(self._warm, warmup, fn) as (self.pool, capture):
            self.g_fwd = torch.cuda.CUDAGraph()
            with capture(self.g_fwd):
                out = self._run()
            self.static_out = out
            self.diff = [i for i, o in enumerate(out) if o.requires_grad]
            self.static_gout = [torch.zeros_like(o) for o in out]
            self.g_bwd = torch.cuda.CUDAGraph()
            with capture(self.g_bwd):
                grads = torch.autograd.grad([out[i] for i in self.diff], params,
                                            [self.static_gout[i] for i in self.diff], allow_unused=True)
                check_grad_slots()
            self.static_grads = _dense_grads(grads, params)
            self.anchor = torch.zeros((), device=images.device, requires_grad=True)
            del grads

    def _warm(self):
        out = self._run()
        diff = [o for o in out if o.requires_grad]
        torch.autograd.grad(diff, self.params, [torch.ones_like(o) for o in diff], allow_unused=True)
        check_grad_slots()

    def _run(self):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast, cache_enabled=False):
            return self.fn(self.static_images, self.static_ctx)

    def __call__(self, images, ctx):
        if images.data_ptr() != self.static_images.data_ptr():
            self.static_images.copy_(images)
        if ctx.data_ptr() != self.static_ctx.data_ptr():
            self.static_ctx.copy_(ctx)
        return _ReplayFn.apply(self, self.anchor)


class DenoisingState:
    """What a step needs to make denoising queries for a model built with a
    -dn<N> spec: the query count, the decoder's class / layer counts, the
    noise configuration and ONE device generator, created once per TrainStep
    and seeded from the run's seed and the rank."""

    def __init__(self, model: RTDETRMoE, device, seed=0, cfg=None):
        self.num_denoising = model.decoder.num_denoising
        self.num_classes = model.decoder.num_classes
        self.num_layers = len(model.decoder.layers)
        self.cfg = cfg or DenoisingConfig()
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.generator = torch.Generator(device=device)
        self.generator.manual_seed(int(seed) * 1000 + rank)

    def pack(self, tgt_boxes, tgt_labels, n_valid, M, out=None):
        """The denoising pack ``(labels [B, Qdn], boxes [B, Qdn, 4], G)`` of
        targets padded to M (G and Qdn follow M: denoising.dn_shapes), drawn
        from the generator into new tensors, or into ``out`` (an earlier pack
        for the same M: a graphed step's static buffers), which is returned."""
        G, _ = dn_shapes(M, self.num_denoising)
        labels, boxes = make_denoising(tgt_boxes, tgt_labels, n_valid, self.num_classes, G, self.cfg,
                                       self.generator, None if out is None else out[:2])
        return labels, boxes, G


class GraphedStep:
    """The whole differentiable step -- model forward, set criterion with the
    GPU Hungarian matcher (``SetCriterion.forward_padded``), backward to every
    parameter -- captured as ONE hipGraph.  Inputs (images, context ids,
    padded targets, box count) live in static buffers refreshed by device
    copies before each replay; gradients land in ``static_grads``.  No host
    round trip inside the step: the host only refreshes inputs, replays, and
    launches the optimizer.  Targets are padded to ``max_boxes`` per image;
    a batch with more boxes re-captures at the next multiple of 16; the new
    capture allocates new gradient buffers, announced through ``on_capture``
    (TrainStep re-points ``p.grad`` and drops its flat all-reduce views).
    ``dn`` (a DenoisingState, for a model with denoising queries): the noised
    labels and reference boxes live in static buffers sized from M, refreshed
    by denoising.make_denoising next to the targets before each replay; their
    losses (SetCriterion.dn_losses) are part of the captured loss."""

    def __init__(self, fn, criterion, params, images, ctx, targets, num_boxes, *, warmup=3, autocast=False,
                 max_boxes=None, on_capture=None, dn=None):
        self.fn, self.criterion, self.params, self.autocast = fn, criterion, params, autocast
        self.dn = dn
        self.on_capture = on_capture  # called with static_grads after every (re-)capture
        self.captures = 0
        dev = images.device
        self.static_images = images.clone()
        self.static_ctx = ctx.clone()
        self.M = max_boxes or pad_capacity(_most_boxes(targets))
        self.tb, self.tl, self.nv = pad_targets(targets, self.M)
        self.nb = torch.full((), float(num_boxes), dtype=torch.float32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.warmup = warmup
        self._dn_alloc()
        self._capture()

    def _dn_alloc(self):
        """The static denoising pack for the current M, drawn once for the
        warm-up and the capture without advancing the generator: the first
        replay draws what an eager first step draws."""
        self.dn_pack = None
        if self.dn is not None:
            state = self.dn.generator.get_state()
            self.dn_pack = self.dn.pack(self.tb, self.tl, self.nv, self.M)
            self.dn.generator.set_state(state)

    def _dn_refresh(self):
        if self.dn_pack is not None:
            self.dn.pack(self.tb, self.tl, self.nv, self.M, out=self.dn_pack)

    def _loss(self):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast, cache_enabled=False):
            if self.dn_pack is None:
                flat = self.fn(self.static_images, self.static_ctx)
            else:
                flat = self.fn(self.static_images, self.static_ctx, self.dn_pack)
        n_dn = 0 if self.dn_pack is None else self.dn.num_layers
        out, aux = FlatOutputs.unflatten(flat, n_dn)
        if _FUSED_CRIT and self.criterion.fused_ok(out, self.M):  # matching + losses in 3 HIP launches
            total, losses = self.criterion.loss_padded(out, self.tb, self.tl, self.nv, self.nb, self.status)
            total = total + aux
        else:
            losses = self.criterion.forward_padded(out, self.tb, self.tl, self.nv, self.nb, self.status)
            total = sum(losses.values()) + aux
        if n_dn:  # fixed assignment, no matching
            dnl = self.criterion.dn_losses(out["dn_outputs"], self.tb, self.tl, self.nv, self.nb, self.dn_pack[2],
                                           fused=None if _FUSED_CRIT else False)
            total = total + sum(dnl.values())
            losses = {**losses, **dnl}
        return total, losses

    def _grads(self, loss):
        """Gradients of every parameter: autograd for most, the conforming dense
        layers' weight + bias gradients batched after it (linear.DeferredWgrad)."""
        from .conv import batched_flips, deferred_wgrads
        from contextlib import nullcontext

        # bf16 weights live at fixed addresses: the convolutions' flipped weights in one launch
        # (conv.batched_flips); autocast's per-step weight casts would not.  The convolutions'
        # weight-gradient slice sums batched at the end of the backward (conv.deferred_wgrads;
        # under autocast the weight casts' backward reads each gradient at once)
        flips = nullcontext() if self.autocast else batched_flips(loss.device)
        with deferred_weight_grads() as deferred, flips, deferred_wgrads(enabled=not self.autocast):
            grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        check_grad_slots()
        self.deferred_layers = 0 if deferred is None else len(deferred.items)
        return merge_deferred(self.params, grads, deferred)

    def _warm(self):
        loss, _ = self._loss()
        self._grads(loss)

    def _capture(self):
        with _capture_session(self._warm, self.warmup, self.fn) as (self.pool, capture):
            self.graph = torch.cuda.CUDAGraph()
            with capture(self.graph):
                loss, losses = self._loss()
                grads = self._grads(loss)
                self.static_loss = loss.detach()
                self.static_losses = {k: v.detach() for k, v in losses.items()}
            self.static_grads = _dense_grads(grads, self.params)
            del loss, losses, grads
        self.captures += 1
        if self.on_capture is not None:
            self.on_capture(self.static_grads)

    def reserve(self, targets, need=None):
        """Make room for this batch's targets: a batch with more boxes than the
        captured padding re-captures at the next multiple of 16 (rare).
        ``need``: the boxes an image may hold when that is not the batch's
        largest count (mosaic: BatchAugment.need)."""
        if need is None:
            need = _most_boxes(targets)
        if need > self.M:
            self.M = pad_capacity(need)
            self.tb, self.tl, self.nv = pad_targets(targets, self.M)
            self.graph = None
            self._dn_alloc()  # G and Qdn follow M
            self._capture()

    def __call__(self, images, ctx, targets, num_boxes, in_place=False):
        """in_place: the caller (TrainStep with batch augmentation) has already
        called ``reserve`` and written this step's images, padded targets and
        box count into ``static_images``, ``tb`` / ``tl`` / ``nv`` and ``nb``;
        nothing but the context ids is copied."""
        if not in_place:
            self.reserve(targets)
            if images.data_ptr() != self.static_images.data_ptr():
                self.static_images.copy_(images)
            pad_targets(targets, self.M, self.tb, self.tl, self.nv)
            if torch.is_tensor(num_boxes):  # device scalar (e.g. all-reduced box count): no host sync
                self.nb.copy_(num_boxes.reshape(()))
            else:
                self.nb.fill_(float(num_boxes))
        if ctx.data_ptr() != self.static_ctx.data_ptr():
            self.static_ctx.copy_(ctx)
        self._dn_refresh()
        self.graph.replay()
        return self.static_loss


def _ep_group(model: nn.Module):
    """The process group the expert-parallel layers shard their experts over
    (None = the default group; every EP layer uses the same one)."""
    from ..moe.layer import MoEFFN

    groups = {id(m.ep_group): m.ep_group for m in model.modules() if isinstance(m, MoEFFN) and m.ep_size > 1}
    if len(groups) > 1:
        raise ValueError("expert-parallel layers over different process groups are not supported")
    return next(iter(groups.values()), None)


@torch.no_grad()
def clip_grad_norm_sharded(rep_params, shard_params, max_norm, shard_group=None):
    """torch.nn.utils.clip_grad_norm_ over a model whose ``shard_params`` are
    sharded across ``shard_group`` (expert parallelism): the global norm is
    sqrt(|g_rep|^2 + sum over ranks |g_shard|^2), identical on every rank, so
    the clip coefficient -- and hence the replicated weights -- stay in lockstep.
    Returns the total norm."""
    rep = [p.grad for p in rep_params if p.grad is not None]
    shard = [p.grad for p in shard_params if p.grad is not None]
    dev = (rep or shard)[0].device if (rep or shard) else torch.device("cpu")
    sq_rep = torch.stack([g.float().pow(2).sum() for g in rep]).sum() if rep else torch.zeros((), device=dev)
    sq_sh = torch.stack([g.float().pow(2).sum() for g in shard]).sum() if shard else torch.zeros((), device=dev)
    if shard_params and dist.is_available() and dist.is_initialized() and dist.get_world_size(shard_group) > 1:
        sq_sh = sq_sh.reshape(1)
        dist.all_reduce(sq_sh, group=shard_group)
        sq_sh = sq_sh.reshape(())
    total = (sq_rep + sq_sh).sqrt()
    coef = (max_norm / (total + 1e-6)).clamp(max=1.0)
    for g in rep + shard:
        g.mul_(coef.to(g.dtype))
    return total


def gemm_params(model: nn.Module):
    """Parameters that are GEMM / convolution operands: weights and biases of
    Linear, Conv2d and MultiheadAttention layers and the MoE expert weights,
    plus LayerNorm affines (the HIP layer_norm kernel wants them in the input
    dtype).  These are held in bf16 (TrainStep precision "bf16"); BatchNorm
    (mixed bf16-input / fp32-affine kernels), the MoE router and everything
    else stay fp32."""
    from ..moe.layer import MoEFFN

    out, seen = [], set()
    for mod in model.modules():
        if isinstance(mod, (nn.Linear, nn.Conv2d, nn.LayerNorm)):  # layer_norm on HIP needs weight dtype == input
            ps = [mod.weight, mod.bias]
        elif isinstance(mod, (nn.MultiheadAttention, TokenSelfAttention)):
            ps = [mod.in_proj_weight, mod.in_proj_bias]
        elif isinstance(mod, MoEFFN):
            ps = [mod.w1, mod.b1, mod.w2, mod.b2]
        else:
            continue
        for p in ps:
            if p is not None and id(p) not in seen:
                seen.add(id(p))
                out.append(p)
    return out


class TrainStep:
    """precision (GPU):
      "bf16" (default) -- GEMM/conv operands (gemm_params) held in bf16, fp32
             master copies in the optimizer, no autocast: no per-layer weight
             casts in the forward nor grad casts in the backward (about 1,700
             cast ops per C2 step under autocast, most of the host time of an
             eager step); the optimizer (optim.FlatAdamW: gradient clip +
             AdamW in three HIP launches) reads the bf16 grads, updates the
             flat fp32 masters and rewrites the bf16 weights;
      "amp"  -- fp32 parameters under bf16 autocast (same optimizer).
    On CPU the model runs in fp32 with torch.optim.AdamW and
    clip_grad_norm_ (the semantics FlatAdamW restates).

    accumulate: micro-steps (calls) per optimizer step, K.  None takes
    the model spec's nominal batch size (-nbs<N>): K = max(1, round(nbs /
    (batch * world))), 1 without the token.  With K = 1 the step is
    unchanged (no accumulator, the same launches).  With K > 1 every call
    adds its gradients to an fp32 sum on the device (optim.GradAccumulator,
    one HIP launch after the graph replay) and the K-th call runs the
    data-parallel exchange, the clip and AdamW (and the weight average)
    once on the mean gradient over micro-steps and ranks; every call
    returns its own loss.  ``self.accumulate`` may be changed between calls
    (the engine's warm-up ramp); ``micro_steps`` / ``opt_steps`` count the
    calls and the optimizer steps.  ``set_lr_scale`` scales the learning
    rates given here (the engine's schedule).
    seed: the run's seed (the denoising queries' noise generator, the
    augmentation parameters' generator).
    augment: batch augmentation (augment.BatchAugment: scale / translate
    jitter, flip, HSV jitter of images and boxes, on the GPU two HIP
    launches in front of the step graph); None takes the model spec's
    -aug token, False leaves the step unchanged (``self.aug`` is None).
    With it the step takes uint8 or fp32 images in any layout.  With
    graphs=True it needs targets= (the whole-step graph, whose static
    inputs the kernels write; the forward / backward graph pair without
    targets is refused with a ValueError).  The eager / CPU step takes any
    batch size up to the first batch's.
    mosaic: the probability that a training image becomes a four-image
    mosaic of its batch (augment.py); None takes the model spec's -mosaic
    token; a positive value implies ``augment`` unless that is False.
    ``self.aug.mosaic`` may be changed between steps (the engine's
    close_mosaic).  With graphs=True the first capture pads the targets to
    max(16, 4 x the example batch's largest count rounded up to 16) -- a
    heuristic start that spares re-captures, not a bound: every step
    reserves the augmenter's bound and re-captures when it is larger.
    content_hw: the (h, w) of the image content inside the padded tensor
    (the augmentation's frame; default: the whole tensor).
    ema_decay / ema_tau: the weight average (ema.ModelEMA: updated once per
    optimizer step, on the GPU inside the AdamW launch); None takes the
    model spec's values (-ema / -ematau<N> tokens), a decay of 0 is off
    (``self.ema`` is None and the step is unchanged).
    zero: the ZeRO-1 optimizer (optim.ShardedDPAdamW) -- default: at
    world > 1 unless MOE_ZERO=0; True also at world 1 (a world-1 process
    group: the RCCL reduce-scatter / all-gather branch on one GPU, tests)."""

    def __init__(self, model: RTDETRMoE, criterion, images, ctx, *, lr=1e-4, lr_backbone=1e-5,
                 weight_decay=1e-4, clip_norm=0.1, graphs=True, ddp_local=None, world=1, precision="bf16",
                 targets=None, num_boxes=1.0, zero=None, seed=0, ema_decay=None, ema_tau=None, augment=None,
                 content_hw=None, mosaic=None, accumulate=None):
        """The stages run in this order, and the order is the contract:
          1. bf16 cast of gemm_params (precision "bf16")
          2. broadcast from rank 0 (the flat A/B path only)   } _build_optimizer
          3. the optimizer takes over the parameters: fp32    }
             ones become views of its flat spaces
          4. the accumulator, when accumulate > 1 (GPU)
          5. ep_grad_scale = 1.0 on expert-parallel MoE layers, then the load
             balancer (an -alb spec)                              _build_balancer
          6. augmenter, image conversion and _cast_in           _build_augmenter
          7. DenoisingState (its generator)
          8. warm-up and capture                                _build_runner
          9. EMA                                                _build_ema
        3 to 7 precede the capture because the graph bakes in their addresses
        and values.  The EMA comes last because it starts from the state the
        first step sees: after the optimizer took over the parameters and after
        the captures' warm-up passes (they move the BatchNorm statistics, not
        the weights)."""
        self.model = model
        self.criterion = criterion
        self.clip_norm = clip_norm
        self.phases = None  # list to enable per-phase event marks (phase_summary)
        self.world = world
        self.graphs = graphs
        self.precision = precision if images.is_cuda else "fp32"
        spec = getattr(model, "spec", None)
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        self.params = [p for _, p in named]
        if self.precision == "bf16":
            for p in gemm_params(model):
                p.data = p.data.to(torch.bfloat16)
        self.ep_params = [p for p in self.params if getattr(p, "expert_parallel", False)]
        self.dp_params = [p for p in self.params if not getattr(p, "expert_parallel", False)]
        self.ep_group = _ep_group(model)
        self.opt, self.opt_params, self.reducer = self._build_optimizer(named, images.is_cuda, lr, lr_backbone,
                                                                        weight_decay, zero)
        self.flat = FlatOutputs(model)
        self.base_lrs = [float(lr_backbone), float(lr)]  # per LR group (backbone, rest): set_lr_scale scales these
        self.accumulate = self._resolve_accumulate(accumulate, spec, images.shape[0])
        self.micro_steps = 0  # calls
        self.opt_steps = 0    # optimizer steps
        self.acc = None       # optim.GradAccumulator (GPU), allocated when a cycle of more than one micro-step starts
        self._pending = 0     # CPU: backward passes summed in .grad since the last optimizer step
        if self.accumulate > 1 and self.opt_params is None:
            self._accumulator()
        if world > 1 and images.is_cuda:
            self._unscale_expert_parallel()
        # loss-free load balancing (an -alb spec): None when no layer has a selection bias, and the
        # step is unchanged.  Built before the capture: _bind_grads pins it to each capture's hist
        self.balancer = self._build_balancer()
        self._m_in = 16  # the mosaic path's raw-target padding: grows with the batches' counts
        self.aug, images, max_boxes = self._build_augmenter(spec, augment, mosaic, images, targets, content_hw, seed)
        images = self._cast_in(images)
        # contrastive denoising queries (a -dn<N> spec): one generator per TrainStep
        self.dn = DenoisingState(model, images.device, seed) if model.decoder.num_denoising > 0 else None
        self.last_losses = None  # {component: detached value} of the last step (criterion sets, _dn sets)
        self.stepper, self.runner, self.fn, self.ddp = self._build_runner(images, ctx, targets, num_boxes, max_boxes,
                                                                           ddp_local)
        self.ema = self._build_ema(spec, ema_decay, ema_tau)

    def _build_optimizer(self, named, on_gpu, lr, lr_backbone, weight_decay, zero):
        """-> (opt, opt_params, reducer).  GPU: flat fp32 masters + moments,
        clip + AdamW + bf16 weight refresh in three HIP launches (optim.py);
        fp32 parameters become views of their master segment.  Expert-parallel
        shards enter the clip norm through a sum over the EP group (the same
        global norm on every rank).  ``opt_params`` is None on the GPU, the
        optimizer's parameter list on the CPU (torch.optim.AdamW); ``reducer``
        is the flat A/B path's all-reduce, None everywhere else."""
        bb = [p for n, p in named if n.startswith("backbone.")]
        rest = [p for n, p in named if not n.startswith("backbone.")]
        if not on_gpu:
            opt = torch.optim.AdamW([{"params": bb, "lr": lr_backbone}, {"params": rest, "lr": lr}], lr=lr,
                                    weight_decay=weight_decay)
            return opt, bb + rest, None
        from .optim import DPGradReducer, FlatAdamW, ShardedDPAdamW

        use_zero = (self.world > 1 and _ZERO) if zero is None else bool(zero)
        if use_zero:
            # C3 data parallelism: reduce-scatter of the fp32 gradients, AdamW on this rank's 1/world
            # slice, all-gather of the weights; the replicated parameters become views of its flat spaces
            opt = ShardedDPAdamW([(bb, lr_backbone), (rest, lr)], weight_decay=weight_decay,
                                 clip_norm=self.clip_norm, sharded=self.ep_params)
            return opt, None, None
        reducer = None
        if self.world > 1:
            # (A/B flat path) every replica starts from rank 0's weights, as DDP does, before
            # FlatAdamW copies its masters
            reducer = DPGradReducer(self.dp_params)
            reducer.broadcast_params()
        opt = FlatAdamW([(bb, lr_backbone), (rest, lr)], weight_decay=weight_decay, clip_norm=self.clip_norm,
                        sharded=self.ep_params, shard_group=self.ep_group)
        return opt, None, reducer

    def _resolve_accumulate(self, accumulate, spec, batch):
        if accumulate is None:
            accumulate = accumulate_count(int(getattr(spec, "nbs", 0)), batch, self.world)
        if int(accumulate) < 1:
            raise ValueError(f"accumulate must be >= 1, got {accumulate}")
        return int(accumulate)

    def _unscale_expert_parallel(self):
        """Expert-parallel weights are not reduced (their gradients already
        hold every rank's tokens), so their layers must not pre-scale by
        1/world: the optimizer applies 1/world to every gradient."""
        from ..moe.layer import MoEFFN

        for m in self.model.modules():
            if isinstance(m, MoEFFN) and m.ep_size > 1:
                m.ep_grad_scale = 1.0

    def _build_balancer(self):
        """-> moe.balance.LoadBalancer or None.  Its two launches stay outside
        every graph: add() after each micro-step's forward, apply() where the
        optimizer steps; the captures' warm-up passes therefore move neither
        the biases nor the load, and the captured router launch reads the
        biases by address."""
        from ..moe.balance import LoadBalancer, balanced_layers

        layers = balanced_layers(self.model)
        if not layers:
            return None
        return LoadBalancer(self.model, layers[0].cfg.balance_rate, group=None, world=self.world)

    def _build_augmenter(self, spec, augment, mosaic, images, targets, content_hw, seed):
        """-> (aug or None, the images as the step's example input, the first
        capture's padding or None).  With an augmenter the images become what
        its kernels read and the static buffer holds: float, channels_last."""
        mosaic = float(getattr(spec, "mosaic", 0.0) if mosaic is None else mosaic)
        if not ((bool(getattr(spec, "augment", False)) or mosaic > 0) if augment is None else bool(augment)):
            return None, images, None
        from .augment import BatchAugment

        if self.graphs and targets is None:
            raise ValueError("batch augmentation needs targets= for graphs=True (the whole-step graph)")
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        padded_hw = tuple(images.shape[-2:])
        aug = BatchAugment(images.shape[0], content_hw or padded_hw, padded_hw, images.device, seed=seed, rank=rank,
                           out_dtype=torch.bfloat16 if self.precision == "bf16" else torch.float32, mosaic=mosaic)
        max_boxes = None
        if aug.mosaic_path and targets is not None:
            max_boxes = pad_capacity(4 * _most_boxes(targets))  # a starting point, see ``mosaic`` (class docstring)
        if images.dtype == torch.uint8:
            images = images.float() / 255.0
        if images.is_cuda:
            images = images.contiguous(memory_format=torch.channels_last)
        return aug, images, max_boxes

    def _build_runner(self, images, ctx, targets, num_boxes, max_boxes, ddp_local):
        """Warm-up and capture -> (stepper, runner, fn, ddp): the whole-step
        graph, or the graph pair (``fn`` is the runner), or the eager callable
        ``fn`` (on the CPU at world > 1 under DDP)."""
        autocast = self.precision == "amp"
        if self.graphs and targets is not None:  # whole step as one graph (GPU matcher)
            stepper = GraphedStep(self.flat, self.criterion, self.params, images, ctx, targets, num_boxes,
                                  autocast=autocast, on_capture=self._bind_grads, dn=self.dn, max_boxes=max_boxes)
            return stepper, None, None, None
        if self.graphs:
            if self.dn is not None:
                raise ValueError("a model with denoising queries needs targets= for graphs=True "
                                 "(the whole-step graph)")
            runner = GraphedModel(self.flat, self.params, images, ctx, autocast=autocast)
            self._bind_grads(runner.static_grads)  # the optimizer reads the backward graph's static buffers
            return None, runner, runner, None
        if self.world > 1 and not images.is_cuda:  # CPU (gloo): DDP buckets overlapped with the backward
            from .engine import wrap_ddp

            ddp = wrap_ddp(self.flat, ddp_local)
            return None, None, ddp, ddp
        return None, None, self.flat, None

    def _build_ema(self, spec, ema_decay, ema_tau):
        """-> ema.ModelEMA or None (a decay of 0); allocates, moves nothing."""
        ema_decay = float(getattr(spec, "ema_decay", 0.0) if ema_decay is None else ema_decay)
        ema_tau = float(getattr(spec, "ema_tau", 2000.0) if ema_tau is None else ema_tau)
        if not ema_decay > 0.0:
            return None
        from .ema import ModelEMA

        return ModelEMA(self.model, self.opt, decay=ema_decay, tau=ema_tau)

    def _bind_grads(self, static_grads):
        """Point every parameter's .grad at the (new) static gradient buffers of
        a capture (the reducer rebuilds its table when the addresses change)."""
        for p, g in zip(self.params, static_grads):
            p.grad = g
        if self.balancer is not None:  # the new capture's static hist tensors are what every replay writes
            self.balancer.pin()

    def _augment_in_place(self, images, targets):
        """Graphed step: pad the incoming targets into the augmenter's raw
        buffers, then let its kernels write the step graph's static inputs --
        images, padded targets, counts -- and the box count (the batch sum of
        the surviving boxes; at world > 1 its mean over the ranks, clamped at
        1, as the engine forms the host count), all on the device."""
        st = self.stepper
        counts = [len(t["boxes"]) for t in targets]
        # reserve the host bound for this step's table: on the mosaic path an image holds the boxes of up
        # to four (a plain table's bound is the batch's largest count)
        table = self.aug.draw(len(targets))
        st.reserve(targets, need=self.aug.need(counts, table))
        if self.aug.mosaic_path:
            # compact from raw buffers of the batch's own padding (M_in) into the graph's (M_out = st.M)
            self._m_in = max(self._m_in, pad_capacity(max(counts, default=0)))
        m_in = self._m_in if self.aug.mosaic_path else st.M  # the plain kernels keep the inputs' M
        raw = self.aug.raw_targets(m_in)
        pad_targets(targets, m_in, *raw)
        _, _, _, _, total = self.aug(images, *raw, out_images=st.static_images, out_targets=(st.tb, st.tl, st.nv),
                                     table=table)
        self._box_count(total, st.nb)

    def _box_count(self, total, out):
        if self.world > 1 and dist.is_available() and dist.is_initialized():
            total = total.reshape(1).clone()
            dist.all_reduce(total)
            total = total.reshape(()) / self.world
        torch.clamp(total, min=1.0, out=out)
        return out

    def _augment_eager(self, images, targets):
        """Eager / CPU step: augment, then back to the list of dicts the eager
        criterion takes (one host read of the counts)."""
        M = pad_capacity(_most_boxes(targets))
        raw = self.aug.raw_targets(M, len(targets))  # a shorter batch (an epoch's last) uses the leading slots
        pad_targets(targets, M, *raw)
        table, M_out = self.aug.draw(len(targets)), None
        if self.aug.mosaic_path:  # the output capacity from the same host bound as the graphed step's
            M_out = pad_capacity(self.aug.need([len(t["boxes"]) for t in targets], table))
        img, tb, tl, nv, total = self.aug(images, *raw, table=table, M_out=M_out)
        nb = self._box_count(total, torch.empty_like(total))
        return img, targets_from_padded(tb, tl, nv), nb if img.is_cuda else float(nb)

    def _cast_in(self, images):
        return images.to(torch.bfloat16) if self.precision == "bf16" else images

    def use_eager(self):
        """Leave graph mode (bench.py's kernel-profiling steps): later steps run
        the model eagerly; parameter grads go back to autograd allocation."""
        if self.runner is not None or self.stepper is not None:
            self.runner = None
            self.stepper = None
            self.fn = self.flat
            self.graphs = False
            for p in self.params:
                p.grad = None
            if self.balancer is not None:
                self.balancer.unpin()
            _drop_autograd_graphs(self.model)  # the captures' AccumulateGrad nodes (side stream) go too

    def _allreduce_grads(self, grads=None):
        """Data-parallel gradient sum (GPU, world > 1): the replicated
        parameters' gradients summed in fp32 by one all-reduce
        (optim.DPGradReducer).  Returns the gradient list in the optimizer's
        parameter order: the summed fp32 views for replicated parameters, the
        local gradients for expert-parallel ones; the optimizer divides by the
        world size inside its kernels.  ``grads``: the local gradients in the
        optimizer's parameter order (an accumulation cycle's fp32 sums);
        default: each parameter's ``.grad``."""
        if grads is None:
            grads = [p.grad for p in self.opt.params]
        local = {id(p): g for p, g in zip(self.opt.params, grads)}
        red = {id(p): v for p, v in zip(self.dp_params, self.reducer([local[id(p)] for p in self.dp_params]))}
        return [red.get(id(p), local[id(p)]) for p in self.opt.params]

    def _mark(self, name):
        if self.phases is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.phases.append((name, e, time.perf_counter()))

    def __call__(self, images, ctx, targets, num_boxes):
        self._mark("start")
        if self.stepper is not None:
            return self._step_graphed(images, ctx, targets, num_boxes)
        return self._step_eager(images, ctx, targets, num_boxes)

    def _step_graphed(self, images, ctx, targets, num_boxes):
        """The whole-step graph: refresh its static inputs, replay, optimizer."""
        if self.aug is not None:  # the kernels write the graph's static inputs
            self._augment_in_place(images, targets)
            self._mark("augment")
            loss = self.stepper(None, ctx, targets, None, in_place=True)
        else:
            loss = self.stepper(self._cast_in(images), ctx, targets, num_boxes)
        self.last_losses = self.stepper.static_losses
        self._mark("step_graph")
        self._optimizer_step()
        self._mark("optimizer")
        return loss

    def _step_eager(self, images, ctx, targets, num_boxes):
        """Forward, host criterion, backward, optimizer: ``self.fn`` is the
        graph pair (``self.runner``: its two replays), or the eager model on
        the GPU or the CPU (there under DDP at world > 1)."""
        if self.aug is not None:
            images, targets, num_boxes = self._augment_eager(images, targets)
            self._mark("augment")
        autograd_grads = self.runner is None  # the graph pair's gradients land in its static buffers
        if autograd_grads and self._pending == 0:  # (CPU, inside a cycle: autograd accumulates in .grad)
            for p in self.params:
                p.grad = None
        dn_pack = None
        if self.dn is not None:  # as GraphedStep, without static buffers
            M = pad_capacity(_most_boxes(targets))
            tb, tl, nv = pad_targets(targets, M)
            dn_pack = self.dn.pack(tb, tl, nv, M)
        inputs = (self._cast_in(images), ctx) if dn_pack is None else (self._cast_in(images), ctx, dn_pack)
        with torch.autocast(images.device.type, dtype=torch.bfloat16, enabled=self.precision == "amp"):
            flat = self.fn(*inputs)
        self._mark("forward")
        out, aux = FlatOutputs.unflatten(flat, 0 if dn_pack is None else self.dn.num_layers)
        losses = self.criterion(out, targets, num_boxes)
        if dn_pack is not None:
            losses.update(self.criterion.dn_losses(out["dn_outputs"], tb, tl, nv, num_boxes, dn_pack[2],
                                                   fused=None if _FUSED_CRIT else False))
        self.last_losses = {k: v.detach() for k, v in losses.items()}
        loss = sum(losses.values()) + aux
        self._mark("criterion")
        if autograd_grads and self.ddp is None and images.is_cuda:
            # dense weight gradients batched after the backward (DDP's reducer
            # needs every gradient during the backward, so not under DDP)
            with deferred_weight_grads() as deferred:
                loss.backward()
            if deferred is not None:
                grads = merge_deferred(self.params, [p.grad for p in self.params], deferred)
                for p, g in zip(self.params, grads):
                    p.grad = g
        else:
            loss.backward()
        check_grad_slots()
        self._mark("backward")
        self._optimizer_step()
        self._mark("optimizer")
        return loss.detach()

    def _accumulator(self):
        if self.acc is None:
            from .optim import GradAccumulator

            self.acc = GradAccumulator(self.opt.params)
        return self.acc

    def set_lr_scale(self, scales):
        """Learning rates = the construction's (backbone, rest) times ``scales``
        (one factor per LR group); they reach the next optimizer launch by value."""
        if len(scales) != len(self.base_lrs):
            raise ValueError(f"set_lr_scale: {len(self.base_lrs)} LR groups, got {len(scales)} factors")
        lrs = [b * float(s) for b, s in zip(self.base_lrs, scales)]
        if self.opt_params is None:
            self.opt.lrs = lrs
        else:
            for g, v in zip(self.opt.param_groups, lrs):
                g["lr"] = v

    def lrs(self):
        """The current learning rate of every LR group (backbone, rest)."""
        return list(self.opt.lrs) if self.opt_params is None else [g["lr"] for g in self.opt.param_groups]

    def _optimizer_step(self):
        """One micro-step done: the optimizer runs on the last one of a cycle."""
        self.micro_steps += 1
        if self.opt_params is None:
            self._optimizer_step_gpu()
        else:
            self._optimizer_step_cpu()

    def _optimizer_step_gpu(self):
        """FlatAdamW / ShardedDPAdamW (reduction + clip inside)."""
        # with a weight average, ModelEMA.update runs the optimizer step with this update's decay
        opt_step = self.opt.step if self.ema is None else self.ema.update
        if self.balancer is not None:  # this micro-step's expert loads; applied with the optimizer step below
            self.balancer.add()
        if self.accumulate <= 1 and (self.acc is None or self.acc.count == 0):
            self._balance_apply()
            if self.reducer is not None:
                opt_step(self._allreduce_grads(), inv_world=1.0 / self.world)
            else:
                opt_step()
            self.opt_steps += 1
            return
        # accumulation: this micro-step's gradients into the fp32 sum; on the last one of the
        # cycle the exchange + clip + AdamW once, on the mean over micro-steps and ranks
        acc = self._accumulator()
        acc.add([p.grad for p in self.opt.params])
        if acc.count < self.accumulate:
            return
        grads, count = acc.take()
        self._balance_apply()
        if self.reducer is not None:
            grads = self._allreduce_grads(grads)
        opt_step(grads, inv_world=1.0 / (self.world * count))
        self.opt_steps += 1

    def _balance_apply(self):
        """Once per optimizer step, ahead of it: the selection biases move by
        the load summed since the last one (over the ranks at world > 1), so a
        weight average taken in the optimizer step blends the new biases."""
        if self.balancer is not None:
            self.balancer.apply()

    def _optimizer_step_cpu(self):
        """torch.optim.AdamW on the gradients autograd summed in ``.grad``."""
        self._pending += 1
        if self.balancer is not None:
            self.balancer.add()
        if self._pending < self.accumulate:
            return
        self._balance_apply()
        if self._pending > 1:  # autograd summed the cycle's backward passes: the mean
            with torch.no_grad():
                for p in self.opt_params:
                    if p.grad is not None:
                        p.grad.div_(self._pending)
        self._pending = 0
        if self.clip_norm > 0:
            clip_grad_norm_sharded(self.dp_params, self.ep_params, self.clip_norm, self.ep_group)
        self.opt.step()
        if self.ema is not None:
            self.ema.update()
        self.opt_steps += 1

    def phase_summary(self):
        """{phase: (gpu ms, host ms)} averaged over the marked steps (syncs)."""
        torch.cuda.synchronize()
        acc, n = {}, 0
        ph = self.phases or []
        for i in range(1, len(ph)):
            name, e, t = ph[i]
            if name == "start":
                n += 1
                continue
            pe, pt = ph[i - 1][1], ph[i - 1][2]
            g, h = acc.get(name, (0.0, 0.0))
            acc[name] = (g + pe.elapsed_time(e), h + 1e3 * (t - pt))
        n = max(n + 1, 1)
        return {k: (round(g / n, 3), round(h / n, 3)) for k, (g, h) in acc.items()}
