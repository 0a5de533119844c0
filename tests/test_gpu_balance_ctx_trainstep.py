"""Per-context loss-free load balancing through the training step on the GPU
(step.TrainStep on an -albc spec, the whole step as one hipGraph): every
layer's [C, E] selection bias moves once per optimizer step, by
src/moe/balance.py's rule on the per-context counts of the layer's
last_topk_idx / last_ctx, outside the graph; the graph's router launches read
the table by address.  Model, data and construction follow
tests/test_gpu_balance_trainstep.py, with two images of different contexts
per batch."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SPEC = "rtdetr-r18-moe4-top2-dec2"
RATE = 0.25
NB = 2.0
MIXED = (11, 12, 15)  # SyntheticZOD(batch=2) seeds whose two images have different contexts: [2, 0], [3, 4], [3, 4]


def _data(dev, seed):
    from src.rtdetr_moe.data import SyntheticZOD

    images, targets, ctx = SyntheticZOD(batch=2, img_h=256, img_w=256, seed=seed).sample(dev)
    images = images.contiguous(memory_format=torch.channels_last)
    return images, ctx, [{k: v.to(dev) for k, v in t.items()} for t in targets], NB


def _step(spec, **kw):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    dev = torch.device("cuda", 0)
    b1 = _data(dev, MIXED[0])
    torch.manual_seed(0)
    model = RTDETRMoE(spec).to(dev).to(memory_format=torch.channels_last)
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[1], graphs=True, lr=1e-3, targets=b1[2],
                     num_boxes=NB, **kw)
    assert step.stepper is not None
    return model, step


def _biases(step):
    torch.cuda.synchronize()
    return torch.stack([m.sel_bias.detach().clone() for m in step.balancer.layers]).cpu()


def _hists(step):
    torch.cuda.synchronize()
    return torch.stack([m.last_hist.detach().clone() for m in step.balancer.layers]).cpu().long()


def _counts(step):
    """int64 [L, C, E] from the layers' last_topk_idx / last_ctx, on the CPU."""
    from src.moe.balance import context_counts

    torch.cuda.synchronize()
    out = []
    for m in step.balancer.layers:
        idx, ci = m.last_topk_idx.cpu(), m.last_ctx.cpu()
        C, E = m.sel_bias.shape
        out.append(context_counts(idx, ci, idx.shape[0] // ci.numel(), C, E))
    return torch.stack(out)


def _replay(want, counts):
    """The reference rule on the [L * C, E] rows, in place on ``want``; -> maxvio [L, C]."""
    from src.moe.balance import balance_reference

    L, C, E = want.shape
    return balance_reference(counts.clone().view(-1, E), want.view(-1, E), RATE).view(L, C)


@functools.lru_cache(maxsize=None)
def _scenario():
    dev = torch.device("cuda", 0)
    model, step = _step(f"{SPEC}-albc{RATE}")
    bal = step.balancer
    r = {"L": bal.L, "shape": tuple(bal.load.shape), "bias0": _biases(step), "load0": bal.load.cpu().clone(),
         "got": [], "want": [], "cnt": [], "hist": [], "maxvio": [], "ctx": []}
    want = r["bias0"].clone()
    for seed in MIXED:
        b = _data(dev, seed)
        step(*b)
        cnt = _counts(step)
        mv = _replay(want, cnt)
        r["got"].append(_biases(step))
        r["want"].append(want.clone())
        r["cnt"].append(cnt)
        r["hist"].append(_hists(step))
        r["maxvio"].append((bal.maxvio.cpu().clone(), mv, torch.stack([m.last_maxvio for m in bal.layers]).cpu()))
        r["ctx"].append(b[1].cpu().tolist())
    r["counters"] = (step.micro_steps, step.opt_steps)
    r["ptrs"] = [(m.last_topk_idx.data_ptr(), m.last_ctx.data_ptr(), m.last_hist.data_ptr()) for m in bal.layers]
    # two no_grad evaluation forwards on a [3, 4] batch, the second with 1000 written into row 3 of one layer's
    # table, at the expert e that layer used least in the first: image 0 (context 3) goes to e, image 1 (context
    # 4) selects as before
    model.eval()
    b = _data(dev, MIXED[2])
    layer = bal.layers[1]
    r["eval_ctx"] = b[1].cpu().tolist()
    ev = []
    for poke in (False, True):
        if poke:
            r["e"] = int(torch.bincount(ev[0][1].reshape(-1).long(), minlength=4).argmin())
            with torch.no_grad():
                layer.sel_bias[3, r["e"]] = 1000.0
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            model(b[0], b[1])
        torch.cuda.synchronize()
        ev.append([m.last_topk_idx.cpu().clone() for m in bal.layers])
    model.train()
    r["eval_idx"] = ev
    r["eval_moved_ptrs"] = [m.last_topk_idx.data_ptr() for m in bal.layers]
    r["bias_eval"], r["load_eval"] = _biases(step), bal.load.cpu().clone()
    # the next replay reads the poked table by address, and add() counts the capture's tensors, not the evaluation's
    want = r["bias_eval"].clone()
    b = _data(dev, MIXED[1])
    step(*b)
    cnt = _counts(step)
    r["poked"] = dict(cnt=cnt, hist=_hists(step), got=_biases(step), maxvio=(bal.maxvio.cpu().clone(), _replay(want, cnt)),
                      want=want, ctx=b[1].cpu().tolist(), tokens=layer.last_tokens,
                      ptrs=[(m.last_topk_idx.data_ptr(), m.last_ctx.data_ptr(), m.last_hist.data_ptr())
                            for m in bal.layers])
    r["keys"] = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.endswith("sel_bias")}
    return r


def test_capture_leaves_the_table_alone(hip_lib):
    r = _scenario()
    assert r["L"] == 3 and r["shape"] == (3, 6, 4)  # AIFI + two decoder layers, 6 contexts, 4 experts
    assert tuple(r["bias0"].shape) == (3, 6, 4)
    assert float(r["bias0"].abs().sum()) == 0.0 and int(r["load0"].abs().sum()) == 0
    assert len(r["keys"]) == 3 and set(r["keys"].values()) == {(6, 4)}


def test_each_step_applies_the_reference_rule_per_context(hip_lib):
    r = _scenario()
    assert r["counters"] == (3, 3)
    for i in range(3):
        assert len(set(r["ctx"][i])) == 2  # a batch of mixed contexts
        assert torch.equal(r["got"][i], r["want"][i]), f"step {i}"
        got, ref, per_layer = r["maxvio"][i]
        assert torch.equal(got, ref) and torch.equal(per_layer, ref.amax(1)), f"step {i}"
        assert torch.equal(r["cnt"][i].sum(1), r["hist"][i]) and int(r["hist"][i].sum()) > 0  # over contexts: hist
        present = sorted(set(r["ctx"][i]))
        absent = [c for c in range(6) if c not in present]
        assert int(r["cnt"][i][:, absent].sum()) == 0 and all(int(r["cnt"][i][:, c].sum()) > 0 for c in present)
        before = r["bias0"] if i == 0 else r["got"][i - 1]
        assert torch.equal(r["got"][i][:, absent], before[:, absent])  # rows of absent contexts are not touched
    assert not torch.equal(r["got"][0], r["bias0"]) and not torch.equal(r["got"][1], r["got"][0])


def test_evaluation_uses_the_table_and_moves_nothing(hip_lib):
    r = _scenario()
    want = r["got"][2].clone()
    want[1, 3, r["e"]] = 1000.0  # the poke, nothing else
    assert torch.equal(r["bias_eval"], want) and int(r["load_eval"].abs().sum()) == 0
    assert r["eval_ctx"] == [3, 4]
    plain, poked = r["eval_idx"]
    T = plain[1].shape[0]
    img0 = torch.arange(T) < T // 2
    assert bool((poked[1][img0] == r["e"]).any(1).all())      # context 3's image: every token takes expert e
    assert not bool((plain[1][img0] == r["e"]).any(1).all())
    for a, b in zip(plain, poked):                            # context 4's image selects as before, in every layer
        n = a.shape[0] // 2
        assert torch.equal(a[n:], b[n:])


def test_replay_reads_the_table_by_address_and_add_counts_the_capture(hip_lib):
    r = _scenario()
    p = r["poked"]
    assert p["ctx"] == [3, 4]
    cnt = p["cnt"][1]  # the poked layer
    per_image = p["tokens"] // 2
    e = r["e"]
    assert int(cnt[3, e]) == per_image and int(cnt[3].sum()) == 2 * per_image  # every token of context 3's image
    assert int(cnt[4, e]) < per_image and int(cnt[4].sum()) == 2 * per_image   # the other image: not so
    # the evaluation re-pointed the layers' tensors; the step put the capture's back and counted those
    assert all(a != b[0] for a, b in zip(r["eval_moved_ptrs"], r["ptrs"]))
    assert p["ptrs"] == r["ptrs"]
    assert torch.equal(p["cnt"].sum(1), p["hist"])
    assert torch.equal(p["got"], p["want"]) and torch.equal(*p["maxvio"])


def test_accumulation_applies_once_per_cycle(hip_lib):
    dev = torch.device("cuda", 0)
    model, step = _step(f"{SPEC}-albc{RATE}", accumulate=2)
    b0 = _biases(step)
    step(*_data(dev, MIXED[0]))
    c1, h1, b1 = _counts(step), _hists(step), _biases(step)
    assert torch.equal(b1, b0) and torch.equal(step.balancer.load.cpu(), c1) and step.opt_steps == 0
    assert torch.equal(c1.sum(1), h1)
    step(*_data(dev, MIXED[1]))
    c2, h2, b2 = _counts(step), _hists(step), _biases(step)
    want = b0.clone()
    _replay(want, c1 + c2)
    assert step.opt_steps == 1 and torch.equal(b2, want) and not torch.equal(b2, b0)
    assert torch.equal(c2.sum(1), h2) and not torch.equal(c1, c2) and int(step.balancer.load.abs().sum()) == 0
