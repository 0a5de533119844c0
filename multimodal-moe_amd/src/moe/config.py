"""MoE knobs and the ``--model`` spec grammar.

The reference's ``--model`` flag names an Ultralytics hub weight
(scripts/train_rtdetr.py:40, src/models/vision/rtdetr.py:39).  Here it names a
local architecture spec (no network fetch), e.g.::

    rtdetr-r50-moe8-top2          C2/C3: R50, 8 experts, top-2, bf16
    rtdetr-r18-moe4-top1          C1: R18, 4 experts, top-1 (CPU plumbing)
    rtdetr-r50-moe16-top2-ep8     C4: 16 experts sharded over 8 ranks (slots sized per layer, below)
    rtdetr-r50-moe16-top2-ep8-epcf0    same, every layer lossless (T slots per source and expert)
    rtdetr-r50-moe16-top2-ep8-epmb0    same, every layer at ep_capacity_factor (no lossless budget)
    rtdetr-r50-moe32-top4-cf1.25-fp8   C5: capacity factor 1.25, fp8 experts
    rtdetr-r50                    dense FFN (no MoE)
    rtdetr-r50-moe8-top2-dn100    C2 trained with ~100 contrastive denoising queries per image
                                  (-dn<N>: src/rtdetr_moe/denoising.py; default 0 = none)
    rtdetr-r50-moe8-top2-ema      C2 trained with an exponential moving average of the weights
                                  (src/rtdetr_moe/ema.py; Ultralytics' decay 0.9999, tau 2000), which
                                  is what gets validated and checkpointed.  -ema<d> sets the decay
                                  (-ema0.999), -ematau<N> the warm-up constant; default: no average
    rtdetr-r50-moe8-top2-aug      C2 trained with GPU batch augmentation (src/rtdetr_moe/augment.py):
                                  scale / translate jitter, horizontal flip and HSV jitter at Ultralytics'
                                  default magnitudes, images and boxes on the device.  The token takes no
                                  value (magnitudes: augment.AugmentParams); default: no augmentation
    rtdetr-r50-moe8-top2-mosaic   the same with mosaic in front: four images of the batch per training
                                  frame (Ultralytics' mosaic=1.0).  -mosaic<p> sets the probability per
                                  image (-mosaic0.5), p in [0, 1]; the token implies -aug; the engine
                                  turns it off for the last TrainArgs.close_mosaic epochs; default: none
    rtdetr-r50-moe8-top2-nbs64    C2 trained at a nominal batch size of 64: the optimizer steps on the mean
                                  gradient of round(64 / (batch x world)) micro-batches (TrainStep accumulate;
                                  Ultralytics' nbs).  Default 0 = a step on every batch
    rtdetr-r50-moe8-top2-warm-lrf0.01-cos   learning-rate schedule (src/rtdetr_moe/schedule.py, Ultralytics'):
                                  -warm[<E>] ramps the rate from 0 (and the accumulation count from 1) over
                                  the first E epochs, bare = 3, at least 100 iterations; -lrf<f> decays the
                                  rate linearly to f x lr over the run, f in (0, 1]; -cos makes the decay
                                  half a cosine.  Default: constant rate, no warm-up
    rtdetr-r50-moe8-top2-alb      C2 with loss-free expert load balancing (src/moe/balance.py; Wang et al.
                                  2024): a per-expert bias added to the router logits for the top-k
                                  selection only, moved by a fixed rate after every optimizer step, up for
                                  an under-loaded expert and down for an over-loaded one.  Bare = 1e-3 (the
                                  paper's value, not tuned here), -alb<u> sets the rate (-alb0.01), u > 0;
                                  the token implies a MoE config.  Default: no bias (balance_rate 0)
    rtdetr-r50-moe8-top2-alb-lb0  the same without the auxiliary load-balance loss: -lb<c> sets lb_coef,
                                  c >= 0 (default 1e-2)
    rtdetr-r50-moe8-top2-albc     the same rule with a bias per (context, expert): a token is ranked with the
                                  row of its image's context, and a row moves by the load its context's tokens
                                  put on the experts, so a batch that holds one context is flattened too.
                                  The contexts then no longer differ in WHICH experts they select, only in the
                                  gates.  -albc<u> sets the rate (-albc0.01), bare = 1e-3; needs the context
                                  (-albc-noctx is refused).  Default: off (balance_per_context False)
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass, field


@dataclass
class MoEConfig:
    num_experts: int = 8
    top_k: int = 2
    hidden: int = 1024            # expert FFN width (RT-DETR dim_feedforward)
    capacity_factor: float = 0.0  # 0 -> no capacity limit (no drops)
    normalize: bool = True        # renormalise top-k gates to sum 1 (k > 1)
    expert_dtype: str = "bf16"    # "bf16" | "fp8"
    lb_coef: float = 1e-2         # load-balance loss coefficient
    z_coef: float = 1e-3          # router z-loss coefficient
    num_contexts: int = 6         # solar bins + missing
    use_context: bool = True
    ep_size: int = 1              # expert-parallel group size (C4)
    expert_parallel: bool = False  # route through ep.py (set by an -ep<n> spec token, n >= 1)
    # rows each rank may send to one expert in the fixed-capacity all-to-all
    # (layers with capacity_factor > 0 use their own capacity instead), sized
    # PER LAYER from its token count T:
    #  * lossless (S = T, the worst case: the EP layer equals the single-process
    #    layer) when that exchange buffer, E T d 2 bytes, fits ep_lossless_mb
    #    (default 32 MB: every C4 decoder layer, 16 x 2,400 x 512 B = 19.7 MB,
    #    where single-context batches skew the experts most -- round 4 measured
    #    22.7 % drops there at 2x the mean);
    #  * else ceil(ep_capacity_factor T k / E) (default 2.0, SURVEY 8(e)'s
    #    budget: the C4 encoder, 60 MB lossless -> 15 MB); assignments beyond it
    #    are dropped like capacity drops and counted (MoEFFN.last_ep_overflow,
    #    bench ep_overflow).
    # Spec tokens: -epcf<f> sets the factor (-epcf0: every layer lossless),
    # -epmb<MB> the lossless budget (-epmb0: every layer at the factor).
    ep_capacity_factor: float = 2.0
    ep_lossless_mb: float = 32.0
    router_init_std: float = 0.02
    ctx_init_scale: float = 0.5
    # loss-free load balancing (balance.py): the selection bias' step per optimizer step; 0 = off (no
    # bias buffer, the plain router).  Spec token -alb[<u>]
    balance_rate: float = 0.0
    # the selection bias is fp32 [num_contexts, E], indexed by the image's context and moved by that context's
    # load, instead of [E].  Spec token -albc[<u>] (sets balance_rate too); needs use_context
    balance_per_context: bool = False

    def capacity(self, tokens: int) -> int:
        if self.capacity_factor <= 0:
            return 0
        return int(math.ceil(self.capacity_factor * tokens * self.top_k / self.num_experts))

    def ep_slot_rows(self, tokens: int, d_model: int = 256) -> int:
        """Rows per (source rank, expert) of the expert-parallel exchange: the
        layer capacity when it has one; T (lossless) when the factor is 0, or
        when the lossless buffer E T d 2 bytes fits ep_lossless_mb; else
        ceil(ep_capacity_factor T k / E) -- never more than T (a token sends at
        most one row to an expert)."""
        cap = self.capacity(tokens)
        if cap > 0:
            return cap
        f = self.ep_capacity_factor
        lossless_bytes = self.num_experts * tokens * d_model * 2
        if f <= 0 or f * self.top_k >= self.num_experts or lossless_bytes <= self.ep_lossless_mb * 1e6:
            return max(1, tokens)
        return max(1, min(tokens, int(math.ceil(f * tokens * self.top_k / self.num_experts))))


@dataclass
class ModelSpec:
    backbone: str = "r50"          # r18 | r34 | r50 | r101
    moe: MoEConfig | None = field(default_factory=MoEConfig)
    num_decoder_layers: int | None = None  # default by backbone (6 for r50, 3 for r18)
    num_denoising: int = 0         # contrastive denoising queries per image in training (-dn<N>; 0 = off)
    ema_decay: float = 0.0         # EMA of the weights in training (-ema = 0.9999, -ema<d>; 0 = off)
    ema_tau: float = 2000.0        # EMA warm-up: d_t = ema_decay (1 - exp(-t / ema_tau)) (-ematau<N>)
    augment: bool = False          # GPU batch augmentation in training (-aug; rtdetr_moe/augment.py)
    mosaic: float = 0.0            # mosaic probability per image (-mosaic = 1.0, -mosaic<p>; implies augment)
    nbs: int = 0                   # nominal batch size: accumulate round(nbs / (batch world)) micro-batches (-nbs<N>; 0 = off)
    warmup_epochs: float = 0.0     # LR / accumulation warm-up in epochs, at least 100 iterations (-warm = 3, -warm<E>; 0 = off)
    lrf: float = 1.0               # final learning-rate factor of the decay, in (0, 1] (-lrf<f>; 1 = constant)
    cos_lr: bool = False           # cosine instead of linear decay (-cos)
    raw: str = ""


_SPEC_RE = re.compile(r"^rtdetr-(r18|r34|r50|r101)((?:-[a-z0-9.]+)*)$")


def parse_moe_spec(spec: str) -> ModelSpec:
    """Parse ``rtdetr-<backbone>[-moe<E>][-top<k>][-cf<f>][-fp8][-ep<n>][-epcf<f>][-dec<L>][-dn<N>][-ema[<d>]][-ematau<N>][-aug][-mosaic[<p>]][-nbs<N>][-warm[<E>]][-lrf<f>][-cos][-alb[<u>]][-albc[<u>]][-lb<c>]``
    (``-aug``: training batch augmentation, no value; ``-mosaic[<p>]``: four-image mosaic with
    probability p, default 1.0, implies ``-aug``; ``-nbs<N>``: nominal batch size for gradient
    accumulation; ``-warm[<E>]`` / ``-lrf<f>`` / ``-cos``: the learning-rate schedule;
    ``-alb[<u>]``: loss-free load balancing at rate u > 0, default 1e-3, implies a MoE config;
    ``-albc[<u>]``: the same with a bias per (context, expert), not with ``-noctx``;
    ``-lb<c>``: the load-balance loss coefficient, c >= 0)."""
    s = spec.strip().lower()
    if s.endswith(".pt") or s.endswith(".pth"):
        raise ValueError(f"{spec!r} is a weights file, not an architecture spec")
    m = _SPEC_RE.match(s)
    if not m:
        raise ValueError(
            f"unknown model spec {spec!r}; expected e.g. 'rtdetr-r50-moe8-top2' "
            "(hub weight names such as 'rtdetr-l.pt' need a network fetch and are not supported)")
    out = ModelSpec(backbone=m.group(1), moe=None, raw=spec)
    moe = None
    for tok in [t for t in m.group(2).split("-") if t]:
        if tok == "aug":  # exact, ahead of every prefix match
            out.augment = True
        elif tok.startswith("mosaic"):  # ahead of the "moe" prefix
            try:
                out.mosaic = float(tok[6:]) if tok[6:] else 1.0
            except ValueError:
                raise ValueError(f"bad mosaic probability {tok[6:]!r} in model spec {spec!r}") from None
            if not 0.0 <= out.mosaic <= 1.0:
                raise ValueError(f"mosaic probability outside [0, 1] in model spec {spec!r}")
            out.augment = True
        elif tok == "cos":  # exact, ahead of every prefix match
            out.cos_lr = True
        elif tok.startswith("nbs"):
            try:
                out.nbs = int(tok[3:])
            except ValueError:
                raise ValueError(f"bad nominal batch size {tok[3:]!r} in model spec {spec!r}") from None
            if out.nbs < 0:
                raise ValueError(f"negative nominal batch size in model spec {spec!r}")
        elif tok.startswith("warm"):
            try:
                out.warmup_epochs = float(tok[4:]) if tok[4:] else 3.0
            except ValueError:
                raise ValueError(f"bad warm-up length {tok[4:]!r} in model spec {spec!r}") from None
            if not out.warmup_epochs >= 0.0:
                raise ValueError(f"negative warm-up length in model spec {spec!r}")
        elif tok.startswith("lrf"):
            try:
                out.lrf = float(tok[3:])
            except ValueError:
                raise ValueError(f"bad final learning-rate factor {tok[3:]!r} in model spec {spec!r}") from None
            if not 0.0 < out.lrf <= 1.0:
                raise ValueError(f"final learning-rate factor outside (0, 1] in model spec {spec!r}")
        elif tok.startswith("alb"):  # -albc[<u>] ahead of -alb[<u>]: the later token of the two decides the mode
            moe = moe or MoEConfig()
            moe.balance_per_context = tok.startswith("albc")
            val = tok[4:] if moe.balance_per_context else tok[3:]
            try:
                moe.balance_rate = float(val) if val else 1e-3
            except ValueError:
                raise ValueError(f"bad balance rate {val!r} in model spec {spec!r}") from None
            if not (moe.balance_rate > 0.0 and math.isfinite(moe.balance_rate)):
                raise ValueError(f"balance rate must be positive in model spec {spec!r}")
        elif tok.startswith("lb"):
            moe = moe or MoEConfig()
            try:
                moe.lb_coef = float(tok[2:])
            except ValueError:
                raise ValueError(f"bad load-balance coefficient {tok[2:]!r} in model spec {spec!r}") from None
            if not (moe.lb_coef >= 0.0 and math.isfinite(moe.lb_coef)):
                raise ValueError(f"negative load-balance coefficient in model spec {spec!r}")
        elif tok.startswith("moe"):
            moe = moe or MoEConfig()
            moe.num_experts = int(tok[3:])
        elif tok.startswith("top"):
            moe = moe or MoEConfig()
            moe.top_k = int(tok[3:])
        elif tok.startswith("cf"):
            moe = moe or MoEConfig()
            moe.capacity_factor = float(tok[2:])
        elif tok == "fp8":
            moe = moe or MoEConfig()
            moe.expert_dtype = "fp8"
        elif tok == "noctx":
            moe = moe or MoEConfig()
            moe.use_context = False
        elif tok.startswith("epcf"):
            moe = moe or MoEConfig()
            moe.ep_capacity_factor = float(tok[4:])
        elif tok.startswith("epmb"):
            moe = moe or MoEConfig()
            moe.ep_lossless_mb = float(tok[4:])
        elif tok.startswith("ematau"):  # before "ema"
            out.ema_tau = float(tok[6:])
            if not out.ema_tau > 0:
                raise ValueError(f"EMA tau must be positive in model spec {spec!r}")
        elif tok.startswith("ema"):
            out.ema_decay = float(tok[3:]) if tok[3:] else 0.9999
            if not 0.0 <= out.ema_decay < 1.0:
                raise ValueError(f"EMA decay outside [0, 1) in model spec {spec!r}")
        elif tok.startswith("ep"):
            moe = moe or MoEConfig()
            moe.ep_size = int(tok[2:])
            moe.expert_parallel = True
        elif tok.startswith("dec"):
            out.num_decoder_layers = int(tok[3:])
        elif tok.startswith("dn"):
            out.num_denoising = int(tok[2:])
            if out.num_denoising < 0:
                raise ValueError(f"negative denoising query count in model spec {spec!r}")
        else:
            raise ValueError(f"unknown token {tok!r} in model spec {spec!r}")
    if moe is not None:
        if moe.top_k > moe.num_experts:
            raise ValueError("top_k must be <= num_experts")
        if moe.num_experts % moe.ep_size:
            raise ValueError("num_experts must be divisible by ep_size")
        if moe.balance_per_context and not moe.use_context:
            raise ValueError(f"-albc needs the image context, which -noctx removes, in model spec {spec!r}")
    out.moe = moe
    return out
