"""The learning-rate schedule and the accumulation count (src/rtdetr_moe/
schedule.py, host arithmetic restating Ultralytics' trainer, which the
reference trains through: src/models/vision/rtdetr.py:82-94) and their model
spec tokens.  Known answers worked out by hand from the formulas."""
from __future__ import annotations

import math

import pytest

from src.moe.config import parse_moe_spec
from src.rtdetr_moe import schedule as S


def test_lr_factor_linear():
    # max(1 - x / epochs, 0) (1 - lrf) + lrf
    assert S.lr_factor(0, 10, 0.1) == 1.0
    assert S.lr_factor(5, 10, 0.1) == pytest.approx(0.55, abs=1e-15)
    assert S.lr_factor(9, 10, 0.1) == pytest.approx(0.1 * 0.9 + 0.1, abs=1e-15)
    assert S.lr_factor(10, 10, 0.1) == pytest.approx(0.1, abs=1e-15)
    assert S.lr_factor(12, 10, 0.1) == pytest.approx(0.1, abs=1e-15)  # clamped past the end
    assert all(S.lr_factor(e, 10, 1.0) == 1.0 for e in range(11))     # lrf 1: a constant rate


def test_lr_factor_cosine():
    # ((1 - cos(x pi / epochs)) / 2) (lrf - 1) + 1
    assert S.lr_factor(0, 10, 0.1, cos=True) == 1.0
    assert S.lr_factor(5, 10, 0.1, cos=True) == pytest.approx(0.55, abs=1e-15)
    assert S.lr_factor(9, 10, 0.1, cos=True) == pytest.approx((1 - math.cos(0.9 * math.pi)) / 2 * -0.9 + 1, abs=1e-15)
    assert S.lr_factor(10, 10, 0.1, cos=True) == pytest.approx(0.1, abs=1e-15)
    # between the ends the cosine lies above the line in the first half, below it in the second
    assert S.lr_factor(2, 10, 0.1, cos=True) > S.lr_factor(2, 10, 0.1)
    assert S.lr_factor(8, 10, 0.1, cos=True) < S.lr_factor(8, 10, 0.1)


def test_warmup_iters_has_a_floor_of_100():
    assert S.warmup_iters(3, 10) == 100
    assert S.warmup_iters(3, 1000) == 3000
    assert S.warmup_iters(0.5, 301) == 150   # round(150.5) = 150 (round half to even, as Python's round)
    assert S.warmup_iters(0, 1000) == -1
    assert S.warmup_iters(0.0, 5) == -1


def test_accumulate_count():
    assert S.accumulate_count(64, 16, 1) == 4
    assert S.accumulate_count(64, 8, 1) == 8
    assert S.accumulate_count(64, 16, 8) == 1   # round(0.5) = 0 -> clamped to 1
    assert S.accumulate_count(64, 4, 2) == 8
    assert S.accumulate_count(32, 8, 1) == 4
    assert S.accumulate_count(0, 16, 1) == 1    # off
    assert S.accumulate_count(100, 16, 1) == 6  # round(6.25)


def test_warmup_interpolation():
    nw, f = 100, 0.55
    assert S.warmup_lr_factor(0, nw, f) == 0.0
    assert S.warmup_lr_factor(nw // 2, nw, f) == pytest.approx(0.275, abs=1e-15)
    assert S.warmup_lr_factor(nw, nw, f) == pytest.approx(f, abs=1e-15)
    # accumulate: 1 -> nbs / (batch world) = 4
    assert S.warmup_accumulate(0, nw, 64, 16) == 1
    assert S.warmup_accumulate(nw // 2, nw, 64, 16) == 2   # 2.5 rounds to even
    assert S.warmup_accumulate(60, nw, 64, 16) == 3        # 2.8
    assert S.warmup_accumulate(nw, nw, 64, 16) == 4
    assert S.warmup_accumulate(nw, nw, 64, 16, world=2) == 2
    assert S.warmup_accumulate(50, nw, 0, 16) == 1         # no nominal batch size: no accumulation


def test_schedule_at():
    kw = dict(nw=100, epochs=10, lrf=0.1, nbs=64, batch=16, world=1)
    assert S.schedule_at(0, 0, **kw) == (0.0, 1)
    f, k = S.schedule_at(50, 0, **kw)
    assert f == pytest.approx(0.5, abs=1e-15) and k == 2
    f, k = S.schedule_at(100, 1, **kw)  # ni == nw is still the warm-up's last iteration: the epoch's value
    assert f == pytest.approx(S.lr_factor(1, 10, 0.1), abs=1e-15) and k == 4
    assert S.schedule_at(101, 1, **kw) == (S.lr_factor(1, 10, 0.1), 4)
    # warm-up off (nw = -1): the epoch's value from the first iteration
    assert S.schedule_at(0, 0, nw=-1, epochs=10, lrf=0.1, nbs=64, batch=16) == (1.0, 4)
    assert S.schedule_at(7, 5, nw=-1, epochs=10) == (1.0, 1)


def test_spec_tokens():
    s = parse_moe_spec("rtdetr-r18-moe4-top2-dec2-nbs64-warm-lrf0.01-cos")
    assert (s.nbs, s.warmup_epochs, s.lrf, s.cos_lr) == (64, 3.0, 0.01, True)
    assert s.moe.num_experts == 4 and s.moe.top_k == 2 and s.num_decoder_layers == 2  # the others still parse
    assert parse_moe_spec("rtdetr-r50-warm1.5").warmup_epochs == 1.5
    assert parse_moe_spec("rtdetr-r50-warm0").warmup_epochs == 0.0
    assert parse_moe_spec("rtdetr-r50-lrf1").lrf == 1.0
    assert parse_moe_spec("rtdetr-r50-nbs0").nbs == 0
    s = parse_moe_spec("rtdetr-r50-cos")
    assert s.cos_lr and s.moe is None  # "cos" is not a "cf" (capacity factor) token
    # next to tokens with a shared first letter: -noctx / -nbs, -cf / -cos, -mosaic / -moe
    s = parse_moe_spec("rtdetr-r50-moe8-top2-cf1.25-noctx-mosaic0.5-nbs32-cos")
    assert s.nbs == 32 and s.cos_lr and s.moe.capacity_factor == 1.25 and not s.moe.use_context and s.mosaic == 0.5


@pytest.mark.parametrize("bad", ["-lrf0", "-lrf1.5", "-nbs-1", "-lrf", "-nbsx", "-warmx", "-lrfx"])
def test_spec_tokens_refuse_bad_values(bad):
    with pytest.raises(ValueError):
        parse_moe_spec("rtdetr-r18-moe4-top2" + bad)


def test_spec_defaults():
    s = parse_moe_spec("rtdetr-r50-moe8-top2")
    assert (s.nbs, s.warmup_epochs, s.lrf, s.cos_lr) == (0, 0.0, 1.0, False)
    # all off: one micro-batch per step and a factor of exactly 1 at every iteration
    assert S.accumulate_count(s.nbs, 16, 1) == 1
    nw = S.warmup_iters(s.warmup_epochs, 50)
    assert all(S.schedule_at(ni, ni // 50, nw=nw, epochs=4, lrf=s.lrf, cos=s.cos_lr, nbs=s.nbs, batch=16) == (1.0, 1)
               for ni in range(200))
