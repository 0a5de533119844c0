"""Training / validation engine behind src/models/vision/rtdetr.py.

Replaces what the reference delegates to Ultralytics (``RTDETR(cfg.model)
.train(...)`` / ``.val(...)``, src/models/vision/rtdetr.py:82-94, :112-127):
  * ``train(...)``    -> TrainResults  (.results_dict, .model, .save_dir, .best, .last)
  * ``validate(...)`` -> DetMetrics    (.results_dict, .box, .speed, .model)
Devices follow the reference's ``device`` string ("cpu", "0", "0,1,2,3"):
one process per GPU; a multi-GPU string launches that many local workers
(torch.multiprocessing) unless the caller is already under torchrun.  Every
training batch is one ``step.TrainStep`` -- the same step bench.py times: on
the GPU a whole-step hipGraph with bf16 weights + fp32 masters and the flat
RCCL gradient all-reduce; fp32 eager on CPU (config C1).
"""
from __future__ import annotations

import contextlib
import csv
import json
import math
import os
import random
import time
from dataclasses import asdict, dataclass, field
from datetime import timedelta
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel as DDP

from ..moe.config import parse_moe_spec
from .criterion import SetCriterion
from .data import CocoDataset, SyntheticZOD, YoloDataset, collate
from .metrics import BoxMetrics, DetectionEvaluator, DeviceDetectionEvaluator, gt_xyxy_pixels, named_bands
from .model import RTDETRMoE
# prediction on image files lives in predictor.py; its names stay reachable as engine.predict, engine.Prediction, ...
from .predictor import (Prediction, PredictResults, camera_motion, coco_results, default_sequence_of,  # noqa: F401
                        frame_sequences,
                        mot_lines, predict, predict_merge_on_gpu, predict_resize_on_gpu, predict_track_on_gpu, track,
                        track_results)
from .schedule import accumulate_count, schedule_at, warmup_iters


# ---------------------------------------------------------------------------
# distributed helpers
# ---------------------------------------------------------------------------
def wrap_ddp(model: torch.nn.Module, local_rank: int | None, bucket_cap_mb: int = 64) -> DDP:
    """Data-parallel wrapper over RCCL.  Expert weights
    that are sharded over an expert-parallel group (C4) are excluded from the
    gradient all-reduce."""
    ignore = [n for n, p in model.named_parameters() if getattr(p, "expert_parallel", False)]
    if ignore:
        DDP._set_params_and_buffers_to_ignore_for_model(model, ignore)
    kw = dict(device_ids=[local_rank], output_device=local_rank) if local_rank is not None else {}
    return DDP(model, broadcast_buffers=False, gradient_as_bucket_view=True, bucket_cap_mb=bucket_cap_mb, **kw)


def parse_device(device: str | int | None) -> list:
    """"cpu" -> ["cpu"]; "0" -> [0]; "0,1" -> [0, 1]; "" / None -> [0] if a GPU else ["cpu"]."""
    s = "" if device is None else str(device).strip().lower()
    if s in ("", "auto"):
        return [0] if torch.cuda.is_available() else ["cpu"]
    if s == "cpu":
        return ["cpu"]
    s = s.replace("cuda:", "")
    return [int(v) for v in s.split(",") if v.strip() != ""]


def _dist_ctx():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


# ---------------------------------------------------------------------------
# model handle / results objects (the attributes the reference reads)
# ---------------------------------------------------------------------------
class ModelHandle:
    """``.model`` is the nn.Module (yolo.py:108-114 reads .model.parameters()
    and .model.flops/.GFLOPs)."""

    def __init__(self, module: RTDETRMoE):
        self.model = module

    def __repr__(self):
        return f"ModelHandle({self.model.spec.raw})"


@dataclass
class TrainResults:
    results_dict: dict
    model: ModelHandle | None
    save_dir: Path
    best: Path | None
    last: Path | None
    epochs_run: int = 0
    moe: dict = field(default_factory=dict)


@dataclass
class DetMetrics:
    results_dict: dict
    box: BoxMetrics
    speed: dict
    model: ModelHandle | None
    save_dir: Path | None = None
    moe: dict = field(default_factory=dict)
    context: dict | None = None  # the per-context report (validate(context_report=True)), else None
    size: dict | None = None  # the size report (validate(size_report=True)), else None


def _results_dict(box: BoxMetrics) -> dict:
    return {"metrics/precision(B)": box.mp, "metrics/recall(B)": box.mr, "metrics/mAP50(B)": box.map50,
            "metrics/mAP50-95(B)": box.map, "fitness": 0.1 * box.map50 + 0.9 * box.map}


# ---------------------------------------------------------------------------
# checkpoints: plain dicts of tensors / primitives (torch.load weights_only=True)
# ---------------------------------------------------------------------------
def _expert_shard_names(model: RTDETRMoE) -> dict:
    """{state-dict key: (MoEFFN, attribute)} of the expert weights that an
    expert-parallel model holds as [E/W, ...] shards."""
    from ..moe.layer import MoEFFN

    out = {}
    for name, mod in model.named_modules():
        if isinstance(mod, MoEFFN) and mod.ep_size > 1:
            for a in ("w1", "b1", "w2", "b2"):
                out[f"{name}.{a}" if name else a] = (mod, a)
    return out


def gather_expert_shards(model: RTDETRMoE, sd: dict) -> dict:
    """Collective over the expert-parallel group (every rank must call it):
    replace each [E/W, ...] expert shard in ``sd`` by the stacked [E, ...]
    tensor of all ranks (expert weights are saved stacked so EP
    shards re-assemble).  Identity for a model without EP layers."""
    names = _expert_shard_names(model)
    if not names:
        return sd
    out = dict(sd)
    for key, (mod, _) in names.items():
        t = sd[key].detach().contiguous()
        W = mod.ep_size
        parts = [torch.empty_like(t) for _ in range(W)]
        dist.all_gather(parts, t, group=mod.ep_group)
        out[key] = torch.cat(parts, 0)
    return out


def shard_expert_state(model: RTDETRMoE, sd: dict) -> dict:
    """Inverse of gather_expert_shards for loading: stacked [E, ...] expert
    tensors are cut to this rank's [r E/W, (r+1) E/W) slice when the model is
    expert-parallel."""
    names = _expert_shard_names(model)
    if not names:
        return sd
    out = dict(sd)
    for key, (mod, attr) in names.items():
        full = sd.get(key)
        local = getattr(mod, attr)
        if full is None or full.shape[0] == local.shape[0]:
            continue
        El = local.shape[0]
        r = dist.get_rank(mod.ep_group)
        out[key] = full[r * El:(r + 1) * El]
    return out


def resolve_spec(raw: str):
    """Parse a model spec for THIS process: an expert-parallel spec (-ep<W>)
    outside a process group of W ranks builds the same model with all experts
    local (e.g. single-process evaluation of an EP-trained checkpoint)."""
    spec = parse_moe_spec(raw)
    m = spec.moe
    if m is not None and m.ep_size > 1:
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if world != m.ep_size:
            m.ep_size = 1
            m.expert_parallel = False
    return spec


def save_checkpoint(path: Path, model: RTDETRMoE, epoch: int, fitness: float, optimizer=None, state_dict=None,
                    ema=None):
    """ema: {"decay", "tau", "updates"} when ``state_dict`` holds the averaged
    weights of a run with a weight average (ema.ModelEMA); the key is absent otherwise."""
    path.parent.mkdir(parents=True, exist_ok=True)
    sd = model.state_dict() if state_dict is None else state_dict
    ck = {"spec": model.spec.raw, "num_classes": model.num_classes, "epoch": int(epoch),
          "fitness": float(fitness), "state_dict": {k: v.detach().float().cpu() if v.is_floating_point() else
                                                    v.detach().cpu() for k, v in sd.items()}}
    if model.spec.moe is not None:
        ck["moe_cfg"] = {k: v for k, v in asdict(model.spec.moe).items()}
    if optimizer is not None:
        ck["optimizer"] = optimizer.state_dict()
    if ema is not None:
        ck["ema"] = dict(ema)
    torch.save(ck, path)


def load_model(weights: str | Path, device="cpu", num_classes: int = 1) -> RTDETRMoE:
    """A checkpoint written by save_checkpoint, or a bare architecture spec
    (``num_classes`` applies to the spec only; a checkpoint carries its own)."""
    p = Path(str(weights))
    if p.exists():
        ck = torch.load(p, map_location="cpu", weights_only=True)
        model = RTDETRMoE(resolve_spec(ck["spec"]), num_classes=int(ck.get("num_classes", 1)))
        model.load_state_dict(shard_expert_state(model, ck["state_dict"]))
        return model.to(device)
    if str(weights).endswith((".pt", ".pth")):
        raise FileNotFoundError(f"weights file not found: {weights}")
    return RTDETRMoE(resolve_spec(str(weights)), num_classes=num_classes).to(device)


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def _is_synthetic(data) -> bool:
    return str(data).startswith("synthetic")


def _synthetic_steps(data, default=4) -> int:
    s = str(data)
    return int(s.split(":", 1)[1]) if ":" in s else default


def _hw(imgsz):
    return (imgsz, imgsz) if isinstance(imgsz, int) else (int(imgsz[0]), int(imgsz[1]))


def _batches(data, split, imgsz, batch, workers, seed, rank, world, epoch, drop_last=False, as_uint8=False):
    """as_uint8: the file datasets yield the padded uint8 tensor (a quarter of
    the host-to-device copy; the augmentation kernel scales it by 1/255)."""
    h, w = _hw(imgsz)
    if _is_synthetic(data):
        gen = SyntheticZOD(batch=batch, img_h=h, img_w=w, seed=seed * 1000 + rank + (0 if split == "train" else 777)
                           + epoch * 7919)
        for _ in range(_synthetic_steps(data)):
            yield gen.sample()
        return
    if isinstance(data, dict):  # COCO export: {"train"/"val": {"img_folder", "ann_file"}}
        ds = CocoDataset(data[split]["img_folder"], data[split]["ann_file"], imgsz=(h, w), as_uint8=as_uint8)
    else:
        ds = YoloDataset(data, split=split, imgsz=(h, w), as_uint8=as_uint8)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=split == "train",
                                                              seed=seed) if world > 1 else None
    if sampler is not None:
        sampler.set_epoch(epoch)
    g = torch.Generator().manual_seed(seed + epoch)
    dl = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=(split == "train" and sampler is None),
                                     sampler=sampler, num_workers=workers, collate_fn=collate,
                                     generator=g, drop_last=drop_last and len(ds) >= batch * world,
                                     persistent_workers=False)
    yield from dl


def _num_batches(data, split, imgsz, batch, world, drop_last=False) -> int:
    """How many batches ``_batches`` yields per epoch on one rank (the
    schedule's warm-up length is a number of iterations)."""
    if _is_synthetic(data):
        return _synthetic_steps(data)
    h, w = _hw(imgsz)
    if isinstance(data, dict):
        n = len(CocoDataset(data[split]["img_folder"], data[split]["ann_file"], imgsz=(h, w)))
    else:
        n = len(YoloDataset(data, split=split, imgsz=(h, w)))
    drop = drop_last and n >= batch * world
    if world > 1:  # DistributedSampler pads every rank to the same length
        n = math.ceil(n / world)
    return n // batch if drop else math.ceil(n / batch)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
@dataclass
class TrainArgs:
    model: str
    data: str
    imgsz: object = (704, 1248)
    epochs: int = 50
    patience: int = 100
    batch: int = 16
    device: str = "0"
    project: str = "outputs/runs/rtdetr"
    name: str = "baseline"
    seed: int = 0
    workers: int = 8
    lr: float = 1e-4
    lr_backbone: float = 1e-5
    weight_decay: float = 1e-4
    clip_norm: float = 0.1
    num_classes: int = 1
    ema_decay: float | None = None  # weight average (ema.ModelEMA); None: the model spec's -ema token (0 = off)
    ema_tau: float | None = None
    augment: bool | None = None  # GPU batch augmentation (augment.BatchAugment); None: the model spec's -aug token
    mosaic: float | None = None  # mosaic probability per image (implies augment); None: the spec's -mosaic token
    close_mosaic: int = 10       # the last close_mosaic epochs run without mosaic (Ultralytics' close_mosaic)
    # gradient accumulation and the learning-rate schedule (schedule.py); None: the model spec's token
    nbs: int | None = None              # nominal batch size (-nbs<N>): round(nbs / (batch world)) batches per step
    warmup_epochs: float | None = None  # LR / accumulation warm-up (-warm[<E>]); 0 = off
    lrf: float | None = None            # final LR factor of the decay (-lrf<f>); 1 = constant
    cos_lr: bool | None = None          # cosine decay (-cos)
    # per-context validation report (mAP and expert routing per solar bin); None: MOE_CONTEXT_REPORT=1
    context_report: bool | None = None


def _seed_all(seed: int):
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)


def _master_state_dict(core: RTDETRMoE, step) -> dict:
    """The model's state dict with every bf16 GEMM/conv weight replaced by its
    fp32 master from the optimizer (TrainStep precision "bf16"), so a
    checkpoint carries the exact training state."""
    sd = core.state_dict()
    opt = getattr(step, "opt", None)
    if opt is None or not hasattr(opt, "master_of"):
        return sd
    names = {id(p): n for n, p in core.named_parameters()}
    for p in opt.params:
        if p.dtype == torch.bfloat16 and id(p) in names:
            sd[names[id(p)]] = opt.master_of(p).as_strided(p.shape, p.stride()).detach()
    return sd


def _train_worker(a: TrainArgs, rank: int, world: int, local: int | str) -> TrainResults | None:
    """One rank's training loop.  Each batch is one ``TrainStep`` -- the step
    bench.py measures: on the GPU bf16 GEMM/conv weights with fp32 masters, the
    whole differentiable step (forward, set criterion with the GPU Hungarian
    matcher, backward) replayed as ONE hipGraph, the flat gradient all-reduce
    over RCCL when world > 1, and the fused clip + AdamW (FlatAdamW); on the
    CPU (config C1) fp32 eager with torch.optim.AdamW + clip_grad_norm_ (DDP
    over gloo when world > 1).  The graph has static shapes, so on the GPU the
    train loader drops a last partial batch (every step sees ``batch`` images);
    the loss is accumulated on the device and read once per epoch.
    With a weight average (an -ema spec token or ``ema_decay``; ema.ModelEMA)
    the validation runs on the averaged weights (``step.ema.applied()``), so
    the fitness is the averaged model's, and the checkpoints carry the averaged
    state dict plus an "ema" entry -- what Ultralytics' trainer validates and
    saves.
    With batch augmentation (an -aug spec token or ``augment``) the training
    batches -- never the validation ones -- go through augment.BatchAugment
    inside the step; on the GPU the file datasets then hand over uint8 images,
    in the loader's layout (the kernel reads through strides).
    With mosaic (a -mosaic spec token or ``mosaic``) the probability is set to
    0 from epoch ``epochs - close_mosaic`` on: the augmenter then draws
    degenerate rows for the same kernels, so nothing is re-captured.
    With a nominal batch size or a learning-rate schedule (-nbs / -warm / -lrf /
    -cos spec tokens or the TrainArgs of the same names; schedule.py) the loop
    counts micro-batches and sets the step's learning-rate factor and
    accumulation count before every call; accumulation cycles carry across
    epoch boundaries (no flush), so validation sees the weights of the last
    completed optimizer step, and results.csv gains the columns lr/pg0, lr/pg1,
    train/accumulate and train/opt_steps."""
    from .step import TrainStep

    on_gpu = local != "cpu"
    device = torch.device("cuda", local) if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(local)
        from ..moe import _lib

        _lib.lib()  # the GPU path has no fallback: fail now if libmoe_hip.so is missing
        # MIOpen picks convolution kernels by a (fast-mode) search per shape
        # instead of its immediate-mode heuristic: ~17% shorter C2 steps
        os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
        torch.backends.cudnn.benchmark = True
    _seed_all(a.seed)
    model = load_model(a.model, device, a.num_classes)
    if on_gpu:
        model = model.to(memory_format=torch.channels_last)
    core = model
    ep = bool(_expert_shard_names(core))
    crit = SetCriterion(num_classes=core.num_classes)
    save_dir = Path(a.project) / a.name
    wdir = save_dir / "weights"
    if rank == 0:
        wdir.mkdir(parents=True, exist_ok=True)
    best_fit, best_epoch = -1.0, -1
    last_metrics = BoxMetrics()
    mosaic = float(getattr(getattr(core, "spec", None), "mosaic", 0.0) if a.mosaic is None else a.mosaic)
    augment = (bool(getattr(getattr(core, "spec", None), "augment", False)) or mosaic > 0) if a.augment is None \
        else bool(a.augment)
    # gradient accumulation and the learning-rate schedule (schedule.py): off unless a token / argument asks
    spec = getattr(core, "spec", None)
    nbs = int(getattr(spec, "nbs", 0) if a.nbs is None else a.nbs)
    warmup_epochs = float(getattr(spec, "warmup_epochs", 0.0) if a.warmup_epochs is None else a.warmup_epochs)
    lrf = float(getattr(spec, "lrf", 1.0) if a.lrf is None else a.lrf)
    cos_lr = bool(getattr(spec, "cos_lr", False) if a.cos_lr is None else a.cos_lr)
    if nbs < 0 or warmup_epochs < 0 or not 0.0 < lrf <= 1.0:
        raise ValueError(f"nbs {nbs} / warmup_epochs {warmup_epochs} must be >= 0 and lrf {lrf} in (0, 1]")
    scheduled = nbs > 0 or warmup_epochs > 0 or lrf != 1.0 or cos_lr
    nw = -1
    if warmup_epochs > 0:
        nw = warmup_iters(warmup_epochs, _num_batches(a.data, "train", a.imgsz, a.batch, world, drop_last=on_gpu))
    ni = 0  # micro-batches since the start of the run
    csv_rows = []
    want_report = _context_report_on(a.context_report)
    epoch = 0
    step = None
    shape = None
    for epoch in range(a.epochs):
        core.train()
        t_ep = time.perf_counter()
        tot = torch.zeros((), dtype=torch.float64, device=device)
        n = 0
        for images, targets, ctx in _batches(a.data, "train", a.imgsz, a.batch, a.workers, a.seed, rank, world,
                                             epoch, drop_last=on_gpu, as_uint8=augment and on_gpu):
            images = images.to(device, non_blocking=True)
            if on_gpu and not augment:
                images = images.contiguous(memory_format=torch.channels_last)
            ctx = ctx.to(device)
            tg = [{"boxes": t["boxes"].to(device), "labels": t["labels"].to(device)} for t in targets]
            if augment and on_gpu and step is not None:
                num_boxes = None  # the step counts the surviving boxes itself, on the device (all-reduced there)
            else:
                nb = torch.tensor([float(sum(len(t["boxes"]) for t in targets))], device=device)
                if world > 1:
                    dist.all_reduce(nb)
                num_boxes = (nb / world).clamp_(min=1.0).reshape(())
            if step is None:
                step = TrainStep(core, crit, images, ctx, lr=a.lr, lr_backbone=a.lr_backbone,
                                 weight_decay=a.weight_decay, clip_norm=a.clip_norm, graphs=on_gpu, world=world,
                                 precision="bf16" if on_gpu else "fp32",
                                 ddp_local=None, targets=tg if on_gpu else None,
                                 num_boxes=float(num_boxes), seed=a.seed, ema_decay=a.ema_decay,
                                 ema_tau=a.ema_tau, augment=augment, content_hw=_hw(a.imgsz), mosaic=mosaic,
                                 accumulate=accumulate_count(nbs, a.batch, world))
                shape = tuple(images.shape)
            if scheduled:
                f, step.accumulate = schedule_at(ni, epoch, nw=nw, epochs=a.epochs, lrf=lrf, cos=cos_lr, nbs=nbs,
                                                 batch=a.batch, world=world)
                step.set_lr_scale([f, f])
            ni += 1
            if mosaic > 0 and step.aug is not None:
                step.aug.mosaic = 0.0 if epoch >= a.epochs - a.close_mosaic else mosaic
            if on_gpu and tuple(images.shape) != shape:
                raise RuntimeError(f"batch shape {tuple(images.shape)} differs from the captured {shape}")
            loss = step(images, ctx, tg, num_boxes if on_gpu else float(num_boxes))
            tot += loss.detach().double()
            n += 1
        # validation: rank 0 evaluates the unwrapped model; an expert-parallel
        # model's forward holds all-to-alls, so every rank runs the same
        # validation batches in lockstep (rank 0 keeps the metrics)
        metrics = None
        report = {} if want_report else None
        ema = getattr(step, "ema", None)
        sharded = getattr(getattr(step, "opt", None), "W", 1) > 1
        # with a weight average the averaged model is validated; entering is a
        # collective under the sharded optimizer (every rank enters, rank 0 evaluates)
        if ema is not None and (rank == 0 or ep or sharded):
            with ema.applied():
                if rank == 0 or ep:
                    metrics = _evaluate(core, a.data, "val", a.imgsz, a.batch, device, a.workers, a.seed,
                                        report=report)
        elif rank == 0 or ep:
            metrics = _evaluate(core, a.data, "val", a.imgsz, a.batch, device, a.workers, a.seed, report=report)
        # checkpoint state: fp32 masters (the fp32 averages with a weight average); expert
        # shards gathered to [E, ...] (collective)
        # (a sharded data-parallel optimizer gathers masters collectively: every rank joins)
        collective = ep or sharded
        sd = None
        if rank == 0 or collective:
            sd = gather_expert_shards(core, _master_state_dict(core, step) if ema is None else ema.state_dict())
        ema_info = None if ema is None else {"decay": ema.decay, "tau": ema.tau, "updates": ema.updates}
        if rank == 0:
            last_metrics = metrics
            fit = _results_dict(metrics)["fitness"]
            save_checkpoint(wdir / "last.pt", core, epoch, fit, state_dict=sd, ema=ema_info)
            if fit > best_fit:
                best_fit, best_epoch = fit, epoch
                save_checkpoint(wdir / "best.pt", core, epoch, fit, state_dict=sd, ema=ema_info)
            row = {"epoch": epoch + 1, "train/loss": float(tot) / max(n, 1), "time_s": time.perf_counter() - t_ep,
                   **_results_dict(metrics)}
            if scheduled:  # the values of the epoch's last micro-batch
                pg = step.lrs()
                row.update({"lr/pg0": pg[0], "lr/pg1": pg[1], "train/accumulate": step.accumulate,
                            "train/opt_steps": step.opt_steps})
            row.update(_moe_stats(core))
            if report is not None:
                row.update(_context_columns(report))
            csv_rows.append(row)
        stop = torch.tensor([0.0], device=device)
        if rank == 0 and epoch - best_epoch >= a.patience:
            stop[0] = 1.0
        if world > 1:
            dist.broadcast(stop, 0)
        if float(stop.item()) > 0:
            break
    if rank != 0:
        return None
    with open(save_dir / "results.csv", "w", newline="") as f:
        if csv_rows:
            wr = csv.DictWriter(f, fieldnames=list(csv_rows[0].keys()))
            wr.writeheader()
            wr.writerows(csv_rows)
    return TrainResults(results_dict=_results_dict(last_metrics), model=ModelHandle(core), save_dir=save_dir,
                        best=wdir / "best.pt", last=wdir / "last.pt", epochs_run=epoch + 1, moe=_moe_stats(core))


def _moe_stats(model: RTDETRMoE) -> dict:
    out = {}
    layers = model.moe_layers()
    for i, m in enumerate(layers):
        if m.last_hist is not None:
            h = m.last_hist.detach().float().cpu()
            out[f"moe/l{i}_load_cv"] = float(h.std() / h.mean().clamp(min=1e-9))
        if getattr(m, "last_maxvio", None) is not None:  # load balancing on: max load / mean - 1 of the last step
            out[f"moe/l{i}_maxvio"] = float(m.last_maxvio.detach())
        if getattr(m, "last_ep_overflow", None) is not None:
            out[f"moe/l{i}_ep_overflow"] = int(m.last_ep_overflow)
        if m.last_aux is not None:
            out[f"moe/l{i}_lb"] = float(m.last_aux[0].detach())
            out[f"moe/l{i}_z"] = float(m.last_aux[1].detach())
    return out


def _context_report_on(flag: bool | None) -> bool:
    """The context-report switch: an explicit argument, else MOE_CONTEXT_REPORT=1."""
    return os.environ.get("MOE_CONTEXT_REPORT") == "1" if flag is None else bool(flag)


def _size_report_on(flag: bool | None) -> bool:
    """The size-report switch: an explicit argument, else MOE_SIZE_REPORT=1."""
    return os.environ.get("MOE_SIZE_REPORT") == "1" if flag is None else bool(flag)


def _context_columns(report: dict) -> dict:
    """results.csv columns of one epoch's context report: mAP50-95 per solar
    bin (an empty cell for a bin without targets) and, per MoE layer, the mutual
    information between context and expert (empty for an expert-parallel layer)."""
    out = {}
    for label in report["bins"]:
        d = report["detection"].get(label)
        out[f"metrics/mAP50-95(B)/{label}"] = d["mAP50-95"] if d is not None and d["targets"] > 0 else ""
    for i, r in enumerate(report["routing"]):
        out[f"moe/l{i}_ctx_mi"] = r["mi_bits"] if "mi_bits" in r else ""
    return out


def _mp_entry(local_idx, a, devices, port, out_file):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(local_idx),
                       "WORLD_SIZE": str(len(devices)), "LOCAL_RANK": str(local_idx)})
    dev = devices[local_idx]
    torch.cuda.set_device(dev)
    from .step import rccl_env

    rccl_env()
    # collective timeout: a dead rank fails the run instead of hanging it
    dist.init_process_group("nccl", device_id=torch.device("cuda", dev),
                            timeout=timedelta(seconds=float(os.environ.get("MOE_DIST_TIMEOUT_S", "1800"))))
    try:
        res = _train_worker(a, local_idx, len(devices), dev)
        if local_idx == 0 and res is not None:
            Path(out_file).write_text(json.dumps({"results_dict": res.results_dict, "epochs_run": res.epochs_run,
                                                  "moe": res.moe}))
    finally:
        from .step import release_graphs

        release_graphs()  # the rank's step / evaluation graphs, before the communicator goes
        dist.destroy_process_group()


def train(a: TrainArgs) -> TrainResults:
    devices = parse_device(a.device)
    if dist.is_available() and dist.is_initialized():  # already under torchrun
        rank, world = dist.get_rank(), dist.get_world_size()
        local = int(os.environ.get("LOCAL_RANK", rank)) if devices != ["cpu"] else "cpu"
        return _train_worker(a, rank, world, local)
    if devices == ["cpu"] or len(devices) == 1:
        return _train_worker(a, 0, 1, devices[0])
    import socket
    import tempfile

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_file = Path(tempfile.mkdtemp()) / "rank0.json"
    mp.spawn(_mp_entry, args=(a, devices, port, str(out_file)), nprocs=len(devices), join=True)
    d = json.loads(out_file.read_text())
    save_dir = Path(a.project) / a.name
    model = load_model(save_dir / "weights" / "last.pt", "cpu")
    return TrainResults(results_dict=d["results_dict"], model=ModelHandle(model), save_dir=save_dir,
                        best=save_dir / "weights" / "best.pt", last=save_dir / "weights" / "last.pt",
                        epochs_run=d["epochs_run"], moe=d.get("moe", {}))


# ---------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------
class EvalForward:
    """The inference forward of ``_evaluate`` (no_grad, bf16 autocast on the
    GPU).  On the GPU each input shape is captured once as a hipGraph and
    replayed (static input buffers refreshed by device copies; the outputs are
    the graph's static tensors, valid until the next call) -- the eval forward
    is ~400 kernel launches, which eager PyTorch issues slower than the GPU
    runs them.  MOE_EVAL_GRAPHS=0 keeps it eager; at most ``max_shapes``
    shapes are captured (later ones run eagerly)."""

    def __init__(self, model: RTDETRMoE, max_shapes: int = 2):
        self.model = model
        self.graphs = {}
        self.max_shapes = max_shapes
        self.enabled = os.environ.get("MOE_EVAL_GRAPHS", "1") != "0"
        # stats.RouteStats attached to the model, if any: the warm-ups and prepare()'s replay run the
        # layers' route_stats launches too, so its tables are put back after them -- a batch then adds
        # to them exactly once, by the replay (or the eager run) that produces its outputs
        self.route_stats = None

    def _run(self, images, ctx):
        with torch.autocast(images.device.type, dtype=torch.bfloat16, enabled=images.is_cuda, cache_enabled=False):
            return self.model(images, ctx)

    @staticmethod
    def _key(images, ctx):
        return (tuple(images.shape), images.dtype, tuple(images.stride()), tuple(ctx.shape), ctx.dtype)

    @torch.no_grad()
    def prepare(self, images, ctx):
        """Capture the graph for this input shape now (outside any timed span)."""
        if images.is_cuda and self.enabled and self._key(images, ctx) not in self.graphs \
                and len(self.graphs) < self.max_shapes:
            snap = self.route_stats.snapshot() if self.route_stats is not None else None
            self(images, ctx)
            if snap is not None:
                self.route_stats.restore(snap)

    @torch.no_grad()
    def __call__(self, images, ctx):
        if not (images.is_cuda and self.enabled):
            return self._run(images, ctx)
        key = self._key(images, ctx)
        ent = self.graphs.get(key)
        if ent is None:
            if len(self.graphs) >= self.max_shapes:
                return self._run(images, ctx)
            si, sc = images.clone(), ctx.clone()
            snap = self.route_stats.snapshot() if self.route_stats is not None else None
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up: convolution search, lazy library state, allocator
                for _ in range(2):
                    self._run(si, sc)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            from .step import CAPTURE_MODE, quiesce_collectives

            quiesce_collectives()  # training's eager collectives retired before the capture opens
            g = torch.cuda.CUDAGraph()

            with torch.cuda.graph(g, stream=side, capture_error_mode=CAPTURE_MODE):
                out = self._run(si, sc)
            torch.cuda.synchronize()
            if snap is not None:  # the two warm-ups added to the tables; the capture itself ran nothing
                self.route_stats.restore(snap)
            ent = self.graphs[key] = (g, si, sc, out)
        g, si, sc, out = ent
        si.copy_(images)
        sc.copy_(ctx)
        g.replay()
        return out


@torch.no_grad()
def _evaluate(model: RTDETRMoE, data, split, imgsz, batch, device, workers, seed, speed: dict | None = None,
              ev_out: list | None = None, report: dict | None = None, size_report: dict | None = None,
              size_bands=None, flip=False, merge="nms", merge_iou=0.5, merge_metric="ios", fuse_iou=0.55):
    """report: a dict to fill with the per-context report (``_fill_report``):
    detection metrics per solar bin and each MoE layer's routing table, summed
    over the split by one more HIP launch per layer forward.  None: the pass
    launches and returns exactly what it does without the feature.

    size_report: a dict to fill with the size report (``_fill_size_report``):
    AP, recall and log-average miss rate per pedestrian-height band of
    size_bands (``metrics.named_bands``; heights in source-frame pixels, an
    image's scale its target's ``src_size`` height over the content height, 1.0
    without one), matched by one more HIP launch per batch.  None: as above.

    flip: score the two-pass ensemble of predict(flip=True) (``_flip_rows``): a second forward per batch on the
    mirrored content, its boxes un-mirrored, both passes' rows merged (fused) to the K rows a pass has.  The
    context report's routing tables count the unmirrored pass only: a replayed graph carries its sink with it, so
    the tables are put back after the second forward instead of the sink being taken off (the same tables either
    way).  ``speed`` includes both passes.  False: the pass launches and returns exactly what it does without."""
    content_w = _hw(imgsz)[1]
    rule = (merge == "fuse", float(merge_iou), merge_metric, float(fuse_iou))
    model.eval()
    names = bands = None
    if size_report is not None:
        names, bands = named_bands(size_bands)
    content_h = _hw(imgsz)[0]
    on_gpu = device.type == "cuda"
    fwd = EvalForward(model)
    stats = None
    if report is not None:
        from ..moe.stats import RouteStats

        stats = fwd.route_stats = RouteStats(model)
    # on the GPU the per-image matching is one HIP launch per batch (MOE_EVAL_MATCH=0: the host loop)
    ev = DeviceDetectionEvaluator() if on_gpu else DetectionEvaluator()
    if ev_out is not None:
        ev_out.append(ev)
    t_pre = t_inf = t_post = 0.0
    n_img = 0
    with stats.attach(model) if stats is not None else contextlib.nullcontext():
        for images, targets, ctx in _batches(data, split, imgsz, batch, workers, seed, 0, 1, 0):
            t0 = time.perf_counter()
            ids = [int(c) for c in ctx.tolist()] if report is not None else None  # on the host, before the upload
            scales = None
            if bands is not None:
                scales = [t["src_size"][1] / content_h if "src_size" in t else 1.0 for t in targets]
            images = images.to(device, non_blocking=True)
            ctx = ctx.to(device)
            t_cap = 0.0
            if on_gpu:
                images = images.contiguous(memory_format=torch.channels_last)
                tc = time.perf_counter()
                fwd.prepare(images, ctx)  # first batch of a shape: graph capture, untimed
                t_cap = time.perf_counter() - tc
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = fwd(images, ctx)
            if on_gpu:
                torch.cuda.synchronize()
            t2 = time.perf_counter()
            H, W = images.shape[-2:]
            rows, t_second = None, 0.0
            if flip:  # the graph's outputs are valid until the next call: the first pass's rows before the second
                first = model.postprocess_batched(out, [(W, H)] * images.shape[0])
                snap = stats.snapshot() if stats is not None else None
                mirrored = _mirror_content(images, content_w)
                if on_gpu:
                    torch.cuda.synchronize()
                tm = time.perf_counter()
                out = fwd(mirrored, ctx)
                if on_gpu:
                    torch.cuda.synchronize()
                t_second = time.perf_counter() - tm  # "inference" has both forwards, "postprocess" the rest
                if snap is not None:
                    stats.restore(snap)
                rows = _flip_rows(first, model.postprocess_batched(out, [(W, H)] * images.shape[0]), content_w,
                                  content_h, rule, on_gpu)
            if on_gpu:
                ev.update_batch(*(rows or model.postprocess_batched(out, [(W, H)] * images.shape[0])), targets,
                                size=(W, H), ctx=ids, bands=bands, scales=scales)
                torch.cuda.synchronize()
            else:
                dets = [{"boxes": b, "scores": sc, "labels": lb} for b, sc, lb in zip(*rows)] if flip \
                    else model.postprocess(out, [(W, H)] * images.shape[0])
                for i, (det, t) in enumerate(zip(dets, targets)):
                    gt_xyxy = gt_xyxy_pixels(t["boxes"].numpy().astype(np.float64), W, H)
                    ev.update(det["boxes"].float().cpu().numpy(), det["scores"].float().cpu().numpy(),
                              det["labels"].cpu().numpy(), gt_xyxy, t["labels"].numpy(),
                              ctx=ids[i] if ids is not None else None, bands=bands,
                              scale=1.0 if scales is None else scales[i])
            t3 = time.perf_counter()
            t_pre += t1 - t0 - t_cap
            t_inf += t2 - t1 + t_second
            t_post += t3 - t2 - t_second
            n_img += images.shape[0]
    model.train()
    if speed is not None and n_img:
        speed.update({"preprocess": 1e3 * t_pre / n_img, "inference": 1e3 * t_inf / n_img,
                      "loss": 0.0, "postprocess": 1e3 * t_post / n_img})
    if report is not None:
        _fill_report(report, model, ev, stats)
    if size_report is not None:
        _fill_size_report(size_report, ev, names, bands, n_img)
    return ev.compute()


def _mirror_content(images, content_w: int):
    """The batch with its content region mirrored: columns [0, content_w) reversed, the padding left where it is,
    the layout (channels-last on the GPU) kept."""
    out = images.clone()
    out[..., :content_w] = images[..., :content_w].flip(-1)
    return out


def _flip_rows(first, second, content_w, content_h, rule, on_gpu):
    """validate(flip=True): the two passes' rows -> the merged rows to score.  ``first`` / ``second``:
    postprocess_batched's (boxes [B, K, 4], scores, labels) of the batch and of its mirrored copy, in pixels of the
    padded tensor, whose content starts at x = 0: the second pass's boxes are un-mirrored with
    merge.unmirror_boxes(., content_w), the rows concatenated [B, 2 K] and merged to max_det = K at conf 0 by the
    call predict uses -- ``rule``: (fuse, merge_iou, merge_metric, fuse_iou); fused, both passes have the content
    region (0, 0, content_w, content_h) as their window (validation clips no box, so no side is ever cut by it).
    K is postprocess_batched's, at most 300, so the 2 K candidates always fit the merge's limits.  On a GPU: ONE
    launch (_lib.nms_merge / _lib.box_fuse) -> (boxes [B, K, 4], scores,
    labels [B, K]) with the merge's zero-score tail as it stands: update_batch takes no per-image count, and it
    drops rows scored under its conf_thres (0.001) before they reach any list, so the tail is neutral for AP.  On
    the CPU: merge_reference / fuse_reference per image -> three lists of the kept rows."""
    from .merge import fuse_reference, merge_reference, unmirror_boxes

    fuse, merge_iou, merge_metric, fuse_iou = rule
    (b1, s1, l1), (b2, s2, l2) = first, second
    B, K = int(s1.shape[0]), int(s1.shape[1])
    cb = torch.cat([b1, unmirror_boxes(b2, float(content_w))], 1)
    cs, cl = torch.cat([s1, s2], 1), torch.cat([l1, l2], 1)
    win = torch.tensor([[[0.0, 0.0, float(content_w), float(content_h)]] * 2] * B,
                       dtype=torch.float32) if fuse else None
    if on_gpu:
        from ..moe import _lib

        args = (cb.contiguous(), cs.contiguous(), cl.to(torch.int32).contiguous(), None, 0.0, merge_iou, merge_metric,
                K, False)
        got = _lib.box_fuse(*args, fuse_iou, win.to(cb.device)) if fuse else _lib.nms_merge(*args)
        return got[0], got[1], got[2].to(l1.dtype)
    boxes, scores, labels = [], [], []
    for i in range(B):
        if fuse:
            keep, fb, _ = fuse_reference(cb[i], cs[i], cl[i], None, 0.0, merge_iou, merge_metric, K, False, fuse_iou,
                                         win[i])
            boxes.append(torch.from_numpy(fb).reshape(-1, 4))
        else:
            keep = merge_reference(cb[i], cs[i], cl[i], None, 0.0, merge_iou, merge_metric, K, False)
            boxes.append(cb[i][torch.from_numpy(keep)])
        keep = torch.from_numpy(keep)
        scores.append(cs[i][keep])
        labels.append(cl[i][keep])
    return boxes, scores, labels


def _fill_size_report(report: dict, ev: DetectionEvaluator, names, bands, images: int) -> None:
    """The size report of one validation pass (size_report.json): {"unit":
    "source px", "bands": [{"name", "lo", "hi"}] (hi null for an open band),
    "images", "detection": {band name or "all": targets, AP50, AP50-95, recall,
    LAMR}} (``DetectionEvaluator.compute_by_size``; null metrics for a band
    without in-band truths)."""
    report["unit"] = "source px"
    report["bands"] = [{"name": n, "lo": float(lo), "hi": float(hi) if np.isfinite(hi) else None}
                       for n, (lo, hi) in zip(names, bands)]
    report["images"] = int(images)
    empty = {"targets": 0, "AP50": None, "AP50-95": None, "recall": None, "LAMR": None}
    report["detection"] = ev.compute_by_size(names) if images else {n: dict(empty) for n in [*names, "all"]}


def _fill_report(report: dict, model: RTDETRMoE, ev: DetectionEvaluator, stats) -> None:
    """The per-context report of one validation pass (context_report.json):
    {"bins": the context labels, "detection": {bin: images, targets, precision,
    recall, mAP50, mAP50-95} for the bins that had images, "routing": per MoE
    layer its stats.routing_summary, or "routing": null for a layer without a
    table}."""
    from ..moe.context import CONTEXT_LABELS
    from ..moe.stats import layer_names, routing_summary

    report["bins"] = list(CONTEXT_LABELS)
    report["detection"] = {
        label: {"images": d["images"], "targets": d["targets"], "precision": d["box"].mp, "recall": d["box"].mr,
                "mAP50": d["box"].map50, "mAP50-95": d["box"].map}
        for label, d in ev.compute_by_context(CONTEXT_LABELS).items()}
    tables = stats.tables()
    report["routing"] = []
    for name in layer_names(model):
        if name in tables:
            meta = stats.meta[name]
            report["routing"].append({"layer": name, "experts": meta["experts"],
                                      **routing_summary(tables[name], meta["top_k"], CONTEXT_LABELS)})
        else:
            report["routing"].append({"layer": name, "routing": None, "why": stats.skipped[name]})


def validate(weights, data, split="val", imgsz=(704, 1248), batch=16, device="0", project=None, name=None,
             workers=4, seed=0, context_report: bool | None = None, size_report: bool | None = None,
             size_bands=None, flip=False, merge="nms", merge_iou=0.5, merge_metric="ios",
             fuse_iou=0.55) -> DetMetrics:
    """context_report: also build the per-context report (``DetMetrics.context``
    and, with a save directory, context_report.json there); None reads
    MOE_CONTEXT_REPORT=1.  Off by default.

    size_report: also build the size report (``DetMetrics.size`` and, with a
    save directory, size_report.json there): AP, recall and log-average miss
    rate per pedestrian-height band; None reads MOE_SIZE_REPORT=1.  Off by
    default.  size_bands: (name, lo, hi) triples in source-frame pixels, lo
    inclusive, hi exclusive, hi None for an open band (default far [0, 40),
    medium [40, 100), near [100, inf)).

    flip (off by default): score predict(flip=True)'s two-pass ensemble against
    the ground truth -- per batch a second forward on the images with their
    content mirrored, its boxes un-mirrored (merge.unmirror_boxes), the two
    passes' rows [B, 2 K] merged to K rows at conf 0 by predict's own merge
    (``merge`` "nms" or "fuse" with ``merge_iou``, ``merge_metric`` and
    ``fuse_iou`` as predict takes them; one rtdetr_nms_merge / rtdetr_box_fuse
    launch on a GPU, merge_reference / fuse_reference per image on the CPU).
    Every metric and both reports then describe the merged rows; the context
    report's routing tables count the unmirrored pass only, and ``speed``
    includes both passes.  Without ``flip`` the merge arguments are not looked
    at and validation launches and returns what it always did."""
    if size_bands is not None:
        named_bands(size_bands)  # a bad table fails before the model loads
    if flip:
        from .predictor import _check_args

        _check_args(None, 0.2, merge, merge_iou, merge_metric, fuse_iou, None, True)  # before the model loads
    devices = parse_device(device)
    dev = torch.device("cpu") if devices == ["cpu"] else torch.device("cuda", devices[0])
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
        from ..moe import _lib

        _lib.lib()
    model = load_model(weights, dev)
    if dev.type == "cuda":
        model = model.to(memory_format=torch.channels_last)
    speed = {}
    report = {} if _context_report_on(context_report) else None
    sizes = {} if _size_report_on(size_report) else None
    box = _evaluate(model, data, split, imgsz, batch, dev, workers, seed, speed, report=report, size_report=sizes,
                    size_bands=size_bands, flip=bool(flip), merge=merge, merge_iou=merge_iou,
                    merge_metric=merge_metric, fuse_iou=fuse_iou)
    save_dir = Path(project) / name if project and name else None
    if save_dir is not None:
        save_dir.mkdir(parents=True, exist_ok=True)
        if report is not None:
            (save_dir / "context_report.json").write_text(json.dumps(report, indent=1))
        if sizes is not None:
            (save_dir / "size_report.json").write_text(json.dumps(sizes, indent=1))
    return DetMetrics(results_dict=_results_dict(box), box=box, speed=speed, model=ModelHandle(model),
                      save_dir=save_dir, moe=_moe_stats(model), context=report, size=sizes)



# ---------------------------------------------------------------------------
# tracker tuning
# ---------------------------------------------------------------------------
def tune_tracker(det, gt, grid, device="0", gt_classes=None, gt_ignore_classes=(), out=None, **kw) -> dict:
    """Sweep a grid of tracker arguments over detection files and score every
    configuration against ground truth (tune.sweep).  ``det``: a directory of
    ``<key>/det/det.txt`` or ``<key>.txt`` files (tune.load_det;
    predict(save_det=True) writes them, MOTChallenge's public detections read
    the same way); ``gt``: MOTChallenge ground truth for the same keys
    (moteval.load_gt with ``gt_classes`` / ``gt_ignore_classes``); ``grid``:
    {field: [values]} over tune.SWEEPABLE and tune.SWEEPABLE_MODES ("assoc":
    ["greedy", "lsap"]), or a list of configurations.  On a
    GPU ``device`` all configurations are tracked in ONE HIP launch per chunk of
    frames (rtdetr_track_sweep) and scored by the evaluators' kernels; "cpu"
    runs the references and gives the same dict.  ``out``: a directory that
    receives tracker_sweep.json.  Every other argument is tune.sweep's (base,
    eval_iou, hota, metric, shifts)."""
    from . import moteval, tune

    devices = parse_device(device)
    dev = torch.device("cpu") if devices == ["cpu"] else torch.device("cuda", devices[0])
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
        from ..moe import _lib

        _lib.lib()
    keys = tune.sequence_keys(det)
    dets = tune.load_det(det, keys)
    truth = moteval.load_gt(gt, keys, gt_classes, gt_ignore_classes)
    res = tune.sweep(dets, truth, grid, device=dev, **kw)
    if out is not None:
        Path(out).mkdir(parents=True, exist_ok=True)
        (Path(out) / "tracker_sweep.json").write_text(json.dumps(res))
    return res
