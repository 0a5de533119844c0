"""moe_route_stats on the GPU: the kernel against
stats.route_stats_reference on the same device tensors, its accumulate /
range contract, real router outputs, the MoEFFN sink on the bf16 and the MXFP8
route, and the engine's context report under hipGraph replay.  Every
comparison is an integer ``torch.equal`` or ``==``: the tables are sums of
integers, so no tolerance applies."""
from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

from test_context_report import IMGSZ, MODEL, check_report_tokens, zod_mini_data

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SHAPES = [(5, 37, 4, 2), (1, 1, 1, 1), (3, 130, 8, 2), (2, 64, 33, 8), (16, 920, 8, 2), (7, 300, 64, 4)]


def make_inputs(B, tpi, E, k, seed, drop=True):
    """Random router outputs: idx distinct per token, w and probs from a softmax."""
    g = torch.Generator().manual_seed(seed)
    T = B * tpi
    probs = torch.softmax(2.0 * torch.randn((T, E), generator=g), -1)
    idx = torch.rand((T, E), generator=g).argsort(1)[:, :k].to(torch.int32).contiguous()
    w = torch.softmax(torch.randn((T, k), generator=g), -1)
    pos = torch.arange(T * k, dtype=torch.int32).view(T, k).clone()
    if drop:
        pos[torch.rand((T, k), generator=g) < 0.25] = -1
    return tuple(t.to(DEV) for t in (idx, w, pos, probs))


def contexts(B, n_ctx, seed, absent=(1, 4)):
    ok = [c for c in range(n_ctx) if c not in absent]
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(ok, dtype=torch.int32)[torch.randint(len(ok), (B,), generator=g)].to(DEV)


@pytest.mark.parametrize("B,tpi,E,k", SHAPES)
def test_kernel_equals_the_reference(hip_lib, B, tpi, E, k):
    from src.moe import _lib as L
    from src.moe.stats import route_stats_reference

    idx, w, pos, probs = make_inputs(B, tpi, E, k, seed=B * 1000 + E)
    ci = contexts(B, 6, seed=E)
    for p in (pos, None):
        for c, n_ctx in ((None, 1), (ci, 6)):
            got = torch.zeros((n_ctx, E, 5), dtype=torch.int64, device=DEV)
            L.route_stats(idx, w, p, probs, c, n_ctx, tpi, got)
            want = route_stats_reference(idx, w, p, probs, c, tpi, n_ctx)
            assert torch.equal(got, want), (p is None, n_ctx)
            assert int(got[:, :, 1].sum()) == B * tpi and int(got[:, :, 0].sum()) == B * tpi * k
            if n_ctx == 6:
                assert int(got[[1, 4]].abs().sum()) == 0  # the two absent contexts
            if p is not None and B * tpi * k >= 64:
                assert int(got[:, :, 2].sum()) == int((pos < 0).sum()) > 0


def test_calls_accumulate(hip_lib):
    from src.moe import _lib as L

    B, tpi, E, k = 3, 130, 8, 2
    idx, w, pos, probs = make_inputs(B, tpi, E, k, seed=11)
    ci = contexts(B, 6, seed=3, absent=())
    single = torch.zeros((6, E, 5), dtype=torch.int64, device=DEV)
    L.route_stats(idx, w, pos, probs, ci, 6, tpi, single)
    twice = torch.zeros_like(single)
    for _ in range(2):
        L.route_stats(idx, w, pos, probs, ci, 6, tpi, twice)
    assert torch.equal(twice, 2 * single)
    pattern = (torch.arange(6 * E * 5, dtype=torch.int64, device=DEV).view(6, E, 5) * 1_000_003 - 77)
    filled = pattern.clone()
    L.route_stats(idx, w, pos, probs, ci, 6, tpi, filled)
    assert torch.equal(filled, pattern + single)
    # T == 0: success, no launch
    L.launch_counts(reset=True)
    L.route_stats(idx[:0], w[:0], pos[:0], probs[:0], None, 1, tpi, torch.zeros((1, E, 5), dtype=torch.int64,
                                                                               device=DEV))
    assert "route_stats" not in L.launch_counts()


def test_bad_arguments_are_refused(hip_lib):
    from src.moe import _lib as L

    idx, w, pos, probs = make_inputs(2, 6, 4, 2, seed=1)
    ci = contexts(2, 6, seed=1)
    st = torch.zeros((6, 4, 5), dtype=torch.int64, device=DEV)
    st1 = torch.zeros((1, 4, 5), dtype=torch.int64, device=DEV)
    L.launch_counts(reset=True)
    with pytest.raises(L.MoEKernelError, match="tokens_per_image"):
        L.route_stats(idx, w, pos, probs, None, 1, 5, st1)  # T % tokens_per_image != 0
    with pytest.raises(L.MoEKernelError, match="n_ctx"):
        L.route_stats(idx, w, pos, probs, None, 6, 6, st)  # NULL ctx_img with n_ctx != 1
    with pytest.raises(L.MoEKernelError, match="n_ctx"):
        L.route_stats(idx, w, pos, probs, ci, 0, 6, st[:0])
    pr1 = make_inputs(2, 6, 1, 1, seed=2)[3]
    with pytest.raises(L.MoEKernelError, match="<=E"):  # k > E
        L.route_stats(idx, w, pos, pr1, ci, 6, 6, torch.zeros((6, 1, 5), dtype=torch.int64, device=DEV))
    i65 = torch.zeros((12, 1), dtype=torch.int32, device=DEV)
    with pytest.raises(L.MoEKernelError, match="<=E"):  # E > 64
        L.route_stats(i65, torch.ones((12, 1), device=DEV), None, torch.zeros((12, 65), device=DEV), ci, 6, 6,
                      torch.zeros((6, 65, 5), dtype=torch.int64, device=DEV))
    with pytest.raises(L.MoEKernelError, match="int64"):
        L.route_stats(idx, w, pos, probs, ci, 6, 6, st.int())
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        L.route_stats(idx.cpu(), w, pos, probs, ci, 6, 6, st)
    assert "route_stats" not in L.launch_counts() and int(st.abs().sum()) == 0


def test_out_of_range_ids_stay_in_bounds(hip_lib):
    """Context ids -1 and n_ctx, expert indices -1 and E: valid calls whose
    out-of-range rows contribute nothing and write nothing, here next to
    guard words on both sides of the table."""
    from src.moe import _lib as L
    from src.moe.stats import route_stats_reference

    B, tpi, E, k, n_ctx = 8, 70, 8, 2, 6
    idx, w, pos, probs = make_inputs(B, tpi, E, k, seed=21)
    ci = contexts(B, n_ctx, seed=5, absent=())
    ci[1], ci[6] = -1, n_ctx
    idx[3, 0], idx[tpi + 2, 1], idx[5 * tpi, 0], idx[-1, 1] = -1, E, E, -1
    n, guard = n_ctx * E * 5, 512
    buf = torch.full((guard + n + guard,), -0x0123456789ABCDEF, dtype=torch.int64, device=DEV)
    st = buf[guard:guard + n].view(n_ctx, E, 5)
    st.zero_()
    L.route_stats(idx, w, pos, probs, ci, n_ctx, tpi, st)
    assert torch.equal(st, route_stats_reference(idx, w, pos, probs, ci, tpi, n_ctx))
    assert int(st[:, :, 1].sum()) == 6 * tpi - 2  # two images and two first choices are nowhere
    assert bool((buf[:guard] == -0x0123456789ABCDEF).all()) and bool((buf[guard + n:] == -0x0123456789ABCDEF).all())


def test_real_router_outputs(hip_lib):
    from src.moe import _lib as L
    from src.moe.stats import route_stats_reference

    d, E, k, B, tpi = 128, 4, 2, 3, 37
    T = B * tpi
    g = torch.Generator().manual_seed(4)
    x = torch.randn((T, d), generator=g).to(torch.bfloat16).to(DEV)
    wg = (0.3 * torch.randn((E, d), generator=g)).to(DEV)
    cb = torch.randn((6, E), generator=g).to(DEV)
    ci = torch.tensor([2, 5, 2], dtype=torch.int32, device=DEV)
    cap = int(math.ceil(0.5 * T * k / E))
    idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True)
    rows = min(T * k, E * cap)
    pos, tok, hist, offsets, _, _, _ = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, cap, rows)
    st = torch.zeros((6, E, 5), dtype=torch.int64, device=DEV)
    L.route_stats(idx, w, pos, probs, ci, 6, tpi, st)
    assert torch.equal(st, route_stats_reference(idx, w, pos, probs, ci, tpi, 6))
    assert torch.equal(st[:, :, 0].sum(0), hist.long())
    dropped = (hist.long() - cap).clamp(min=0)
    assert torch.equal(st[:, :, 2].sum(0), dropped) and int(dropped.sum()) > 0
    assert st[:, :, 1].sum(1).tolist() == [0, 0, 2 * tpi, 0, 0, tpi]


@pytest.mark.parametrize("expert_dtype", ["bf16", "fp8"])
def test_layer_sink(hip_lib, expert_dtype):
    from src.moe import _lib as L
    from src.moe.config import MoEConfig
    from src.moe.layer import MoEFFN

    torch.manual_seed(0)
    E, k, B, tpi, d = 8, 2, 4, 150, 256
    layer = MoEFFN(d, MoEConfig(num_experts=E, top_k=k, capacity_factor=1.0, expert_dtype=expert_dtype)).to(DEV)
    x = torch.randn((B, tpi, d), device=DEV).to(torch.bfloat16)
    ci = torch.tensor([0, 3, 3, 5], device=DEV)
    assert layer.route_stats is None
    with torch.no_grad():
        torch.cuda.synchronize()
        L.launch_counts(reset=True)
        y0 = layer(x, ci, residual=True)
        torch.cuda.synchronize()
        plain = L.launch_counts(reset=True)
        assert "route_stats" not in plain and plain.get("router", 0) >= 1
        layer.route_stats = torch.zeros((6, E, 5), dtype=torch.int64, device=DEV)
        y1 = layer(x, ci, residual=True)
        torch.cuda.synchronize()
        sunk = L.launch_counts(reset=True)
    assert sunk.pop("route_stats") == 1 and sunk == plain  # one more launch, nothing else changes
    assert torch.equal(y0, y1)
    st = layer.route_stats
    assert torch.equal(st[:, :, 0].sum(0), layer.last_hist.long())
    assert int(st[:, :, 1].sum()) == B * tpi
    assert st[:, :, 1].sum(1).tolist() == [tpi, 0, 0, 2 * tpi, 0, tpi]
    assert torch.equal(st[:, :, 2].sum(0), (layer.last_hist.long() - layer.cfg.capacity(B * tpi)).clamp(min=0))
    # a table with several contexts needs the ids
    with torch.no_grad(), pytest.raises(ValueError, match="context"):
        layer(x, None)


@pytest.fixture(scope="module")
def engine_runs(hip_lib):
    """_evaluate on zod_mini (4 frames, batch 3: shapes of 3 images, then 1)
    with one model: report + eager, report + graphs, no report + graphs (the
    two graph runs follow the eager one, so neither holds first-use launches)."""
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    torch.manual_seed(0)
    model = engine.load_model(MODEL, DEV).to(memory_format=torch.channels_last)
    runs = {}
    old = os.environ.get("MOE_EVAL_GRAPHS")
    try:
        for name, graphs, on in (("eager", "0", True), ("graph", "1", True), ("off", "1", False)):
            os.environ["MOE_EVAL_GRAPHS"] = graphs
            report, evs = ({} if on else None), []
            torch.cuda.synchronize()
            L.launch_counts(reset=True)
            box = engine._evaluate(model, zod_mini_data(), "val", IMGSZ, 3, DEV, 0, 0, ev_out=evs, report=report)
            torch.cuda.synchronize()
            runs[name] = dict(box=box, ev=evs[0], report=report, counts=L.launch_counts(reset=True))
    finally:
        if old is None:
            os.environ.pop("MOE_EVAL_GRAPHS", None)
        else:
            os.environ["MOE_EVAL_GRAPHS"] = old
    runs["model"] = model
    return runs


def test_engine_report_under_graph_replay(engine_runs):
    r, model = engine_runs, engine_runs["model"]
    layers = len(model.moe_layers())
    # per captured shape two eager warm-ups and the capture (a captured launch counts once; replays do
    # not): layers x (2 batches + 4 warm-ups); eager: one launch per layer and batch
    assert r["graph"]["counts"]["route_stats"] == layers * (2 + 4)
    assert r["eager"]["counts"]["route_stats"] == layers * 2
    check_report_tokens(r["graph"]["report"], model)
    # the warm-ups and prepare()'s replay do not leak into the tables: replay == eager, exactly
    assert r["graph"]["report"]["routing"] == r["eager"]["report"]["routing"]
    assert r["graph"]["report"]["detection"] == r["eager"]["report"]["detection"]
    assert all(layer.route_stats is None for layer in model.moe_layers())


def test_engine_without_the_report_is_unchanged(engine_runs):
    from src.rtdetr_moe.engine import _results_dict

    on, off = engine_runs["graph"], engine_runs["off"]
    assert off["report"] is None and "route_stats" not in off["counts"]
    counts = dict(on["counts"])
    counts.pop("route_stats")
    assert counts == off["counts"]
    assert _results_dict(on["box"]) == _results_dict(off["box"])
    a, b = on["box"], off["box"]
    assert (a.mp, a.mr, a.map50, a.map) == (b.mp, b.mr, b.map50, b.map)
    for name in ("tp", "conf", "pred_cls", "target_cls"):
        xs, ys = getattr(on["ev"], name), getattr(off["ev"], name)
        assert len(xs) == len(ys) == 4 and all(np.array_equal(x, y) for x, y in zip(xs, ys)), name
    assert on["ev"].image_ctx == [0, 3, 4, 5] and off["ev"].image_ctx == [None] * 4


def test_synthetic_report(hip_lib):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)
    model = engine.load_model(MODEL, DEV).to(memory_format=torch.channels_last)
    report = {}
    on = engine._evaluate(model, "synthetic:2", "val", (256, 256), 2, DEV, 0, 0, report=report)
    off = engine._evaluate(model, "synthetic:2", "val", (256, 256), 2, DEV, 0, 0)
    assert sum(d["images"] for d in report["detection"].values()) == 4
    assert (on.mp, on.mr, on.map50, on.map) == (off.mp, off.mr, off.map50, off.map)
    for r in report["routing"]:
        assert sum(r["tokens"]) == 4 * (64 if r["layer"].startswith("encoder.") else 300)
