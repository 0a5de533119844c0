"""Learning-rate schedule and gradient-accumulation count of a training run.

Pure host arithmetic restating Ultralytics' trainer, which the reference
trains through (``RTDETR.train``, src/models/vision/rtdetr.py:82-94):

  * the learning rate of epoch ``x`` is ``base * lr_factor(x)``: linear from 1
    down to ``lrf`` over ``epochs``, or (``cos``) half a cosine between them;
  * the first ``nw = warmup_iters(warmup_epochs, nb)`` iterations (micro-
    batches; ``nb`` per epoch) ramp the learning rate from 0 to the epoch's
    value and the accumulation count from 1 to ``K``, recomputed every
    iteration while ``ni <= nw``;
  * ``K = accumulate_count(nbs, batch, world)``: the micro-batches per
    optimizer step that make up the nominal batch size ``nbs``.

The step applies the results: ``TrainStep.set_lr_scale`` (the factor reaches
the optimizer launch by value) and ``TrainStep.accumulate``.  Not restated:
Ultralytics' weight-decay rescaling by batch * accumulate / nbs, its
bias-group warm-up learning rate and its momentum warm-up.
"""
from __future__ import annotations

import math

import numpy as np


def lr_factor(epoch: int, epochs: int, lrf: float = 1.0, cos: bool = False) -> float:
    """The learning-rate factor of ``epoch`` (0-based) in a run of ``epochs``."""
    if cos:
        return ((1.0 - math.cos(epoch * math.pi / epochs)) / 2.0) * (lrf - 1.0) + 1.0
    return max(1.0 - epoch / epochs, 0.0) * (1.0 - lrf) + lrf


def warmup_iters(warmup_epochs: float, nb: int) -> int:
    """Warm-up length in iterations: at least 100, or -1 when warm-up is off."""
    return max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1


def accumulate_count(nbs: int, batch: int, world: int = 1) -> int:
    """Micro-batches per optimizer step for a nominal batch size ``nbs`` (0 = off: 1)."""
    return max(1, round(nbs / (batch * world))) if nbs > 0 else 1


def warmup_lr_factor(ni: int, nw: int, factor: float) -> float:
    """The factor at iteration ``ni <= nw`` of the warm-up: from 0 to the epoch's ``factor``."""
    return float(np.interp(ni, [0, nw], [0.0, factor]))


def warmup_accumulate(ni: int, nw: int, nbs: int, batch: int, world: int = 1) -> int:
    """The accumulation count at iteration ``ni <= nw`` of the warm-up: from 1 to nbs / (batch * world)."""
    if nbs <= 0:
        return 1
    return max(1, int(np.interp(ni, [0, nw], [1, nbs / (batch * world)]).round()))


def schedule_at(ni: int, epoch: int, *, nw: int, epochs: int, lrf: float = 1.0, cos: bool = False, nbs: int = 0,
                batch: int = 1, world: int = 1):
    """(learning-rate factor, accumulation count) of iteration ``ni`` (counted
    in micro-batches from the start of the run) in ``epoch``."""
    f = lr_factor(epoch, epochs, lrf, cos)
    if ni <= nw:
        return warmup_lr_factor(ni, nw, f), warmup_accumulate(ni, nw, nbs, batch, world)
    return f, accumulate_count(nbs, batch, world)
