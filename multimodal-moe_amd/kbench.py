"""Kernel microbenchmark for the MoE HIP kernels at the C2 shapes.

Times every kernel of one MoE layer (encoder T = 8*920, decoder T = 8*300;
E = 8, k = 2, d = 256, F = 1024) back to back on one stream, interleaving the
tuning variants in one process (median of rounds), and prints one JSON line
per (kernel, shape, variant) with us / TFLOP/s / GB/s.

  python multimodal-moe_amd/kbench.py [--reps 50] [--rounds 5] [--variants 1,2] [--stages 3,4]
  python multimodal-moe_amd/kbench.py --augment     the batch-augmentation kernels at C2's batch
  python multimodal-moe_amd/kbench.py --eval-match  the validation matcher against the host loop
  python multimodal-moe_amd/kbench.py --eval-match-bands  the size-stratified matcher, the plain one and the host loop
  python multimodal-moe_amd/kbench.py --route-stats the routing-statistics kernel against its torch reference
  python multimodal-moe_amd/kbench.py --resize      the inference resize kernel against the host resize it replaces
  python multimodal-moe_amd/kbench.py --resize-flip the mirrored resize launch against the unmirrored one and the old entry
  python multimodal-moe_amd/kbench.py --nms-merge   tiled prediction's merge kernel against the host reference
  python multimodal-moe_amd/kbench.py --box-fuse    tiled prediction's box-fusion kernel against the merge kernel
  python multimodal-moe_amd/kbench.py --track       the tracker's kernel against the host loop and a forward replay
  python multimodal-moe_amd/kbench.py --track-sweep the parameter sweep's kernel against G launches of the tracker's
  python multimodal-moe_amd/kbench.py --track-lsap  assoc = lsap against the greedy kernel, the host and a forward replay
  python multimodal-moe_amd/kbench.py --frame-shift the camera-motion estimator against the host and a forward replay
  python multimodal-moe_amd/kbench.py --mot-eval    the tracking evaluator against the host and a forward replay
  python multimodal-moe_amd/kbench.py --hota        the frame-parallel HOTA kernels against the host and rtdetr_mot_eval
  python multimodal-moe_amd/kbench.py --grad-accum [--cold]  the gradient-accumulation kernel over C2's parameters
  python multimodal-moe_amd/kbench.py --balance [--cold]  loss-free load balancing: the biased router and the balance launch
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch  # noqa: E402

from src.moe import _lib as L  # noqa: E402


_FLUSH = None


def timed(fn, reps):
    """Median kernel execution time (us) of `fn` over `reps` calls (the sum of
    its launches when it makes several), from the dispatch-stamped event pairs
    of libmoe_hip's profiler (hipExtLaunchKernel): no host overhead or
    inter-launch gaps included.  With --cold every call is preceded by a read
    of a buffer larger than the Infinity Cache (operands start in HBM, as in a
    training step where ~GBs pass between a layer's uses of its weights)."""
    fn()
    torch.cuda.synchronize()
    L.lib().moe_profile_enable(1)
    try:
        if _FLUSH is not None:
            _FLUSH.sum()
        fn()
        per = max(1, len(L.profile_records()))
        for _ in range(reps):
            if _FLUSH is not None:
                _FLUSH.sum()
            fn()
        recs = L.profile_records()
    finally:
        L.lib().moe_profile_enable(0)
    ms = [r[1] for r in recs]
    return 1e3 * statistics.median(sum(ms[i:i + per]) for i in range(0, len(ms) - per + 1, per))


SKEW = [0.0]


def setup(T, E, k, d, F, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((T, d), device="cuda", generator=g).to(torch.bfloat16)
    wg = (torch.randn((E, d), device="cuda", generator=g) * 0.3).float()
    cb = torch.randn((6, E), device="cuda", generator=g).float() * 0.5
    # --skew: an expert preference in the context bias, so the routed counts
    # differ between experts as in a real model (C2 layers: max/mean 1.9-3.2x)
    cb += SKEW[0] * torch.linspace(0.0, 1.0, E, device="cuda")
    ci = torch.randint(0, 6, (T // 920 if T % 920 == 0 else T // 300,), device="cuda", generator=g).int()
    tpi = 920 if T % 920 == 0 else 300
    w1 = (torch.randn((E, F, d), device="cuda", generator=g) / 16).to(torch.bfloat16)
    w2 = (torch.randn((E, d, F), device="cuda", generator=g) / 32).to(torch.bfloat16)
    b1 = torch.zeros((E, F), device="cuda")
    b2 = torch.zeros((E, d), device="cuda")
    idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True)
    rank_base, hist, offsets = L.route_scan(bcnt, 0)
    rows = T * k
    xp, pos = L.permute_fwd(x, idx, lrank, rank_base, offsets, E, 0, rows)
    _, tok = L.route_index(idx, lrank, rank_base, offsets, E, 0, rows)
    _, _, _, _, gate, _, _ = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, 0, rows, 1e-2, 1e-3, row_gate=True)
    h = L.grouped_gemm(xp, w1, offsets, E, rows, F, d, 1, L.EPI_BIAS_RELU, bias=b1)
    yp = L.grouped_gemm(h, w2, offsets, E, rows, d, F, 1, L.EPI_BIAS, bias=b2)
    dy = torch.randn((T, d), device="cuda", generator=g).to(torch.bfloat16)
    dyp, dw = L.combine_bwd(dy, yp, pos, w)
    dh = L.grouped_gemm(dyp, w2, offsets, E, rows, F, d, 0, L.EPI_RELU_MASK, aux=h)
    dxp = L.grouped_gemm(dh, w1, offsets, E, rows, d, F, 0, L.EPI_NONE)
    # MXFP8 expert path (C5 kernels) on the same routing
    xq, xs, _ = L.permute_fwd_mx(x, idx, lrank, rank_base, offsets, E, 0, rows)
    w1q, w1s = L.quantize_mx(w1)
    w2q, w2s = L.quantize_mx(w2)
    hq, hs = L.grouped_gemm_mx(xq, xs, w1q, w1s, offsets, E, rows, F, d, L.EPI_BIAS_RELU, bias=b1, out_mx=True)
    _, dlogits = L.token_bwd(dxp, pos, probs, idx, w, dw, lse, None, None, wg, True)
    return dict(dlogits=dlogits, T=T, E=E, k=k, d=d, F=F, x=x, gate=gate, wg=wg, cb=cb, ci=ci, tpi=tpi, w1=w1, w2=w2, b1=b1, b2=b2, idx=idx,
                auxp=auxp,
                w=w, probs=probs, lse=lse, lrank=lrank, bcnt=bcnt, rank_base=rank_base, offsets=offsets, rows=rows,
                xp=xp, pos=pos, tok=tok, h=h, yp=yp, dy=dy, dyp=dyp, dw=dw, dh=dh, dxp=dxp,
                xq=xq, xs=xs, w1q=w1q, w1s=w1s, w2q=w2q, w2s=w2s, hq=hq, hs=hs)


def layer_fwd_bwd(c):
    """One MoE layer forward + backward through ops._MoELayer (all its HIP launches)."""
    from src.moe.ops import moe_layer_hip

    x = c["x"].detach().requires_grad_(True)
    y, aux, raw, hist = moe_layer_hip(x, c["wg"], c["cb"], c["w1"], c["b1"], c["w2"], c["b2"], c["ci"], c["tpi"],
                                      c["k"], True, 0, aux_coefs=(1e-2, 1e-3))
    torch.autograd.backward([y, aux], [c["dy"], torch.ones_like(aux)])


def kernels(c):
    T, E, k, d, F, rows = c["T"], c["E"], c["k"], c["d"], c["F"], c["rows"]
    A = rows
    out = [
        ("router", lambda: L.router_topk_fwd(c["x"], c["wg"], c["cb"], c["ci"], c["tpi"], k, True), 0,
         512 * T + T * (4 * (E + 1) + 16 * k)),
        ("route_scan", lambda: L.route_scan(c["bcnt"], 0), 0, 8 * c["bcnt"].numel()),
        ("permute", lambda: L.permute_fwd(c["x"], c["idx"], c["lrank"], c["rank_base"], c["offsets"], E, 0, rows),
         0, 512 * (T + A) + 12 * A),
        ("gemm1_fwd", lambda: L.grouped_gemm(c["xp"], c["w1"], c["offsets"], E, rows, F, d, 1, L.EPI_BIAS_RELU,
                                             bias=c["b1"]), 2.0 * A * F * d, 0),
        ("gemm2_fwd", lambda: L.grouped_gemm(c["h"], c["w2"], c["offsets"], E, rows, d, F, 1, L.EPI_BIAS,
                                             bias=c["b2"]), 2.0 * A * F * d, 0),
        ("ffn_fwd_fused", lambda: L.expert_ffn_fwd(c["x"], c["tok"], c["w1"], c["b1"], c["w2"], c["b2"], c["offsets"],
                                                   E, rows), 4.0 * A * F * d, 0),
        ("route_index", lambda: L.route_index(c["idx"], c["lrank"], c["rank_base"], c["offsets"], E, 0, rows), 0,
         16 * A + 4 * A),
        ("gemm1_fwd_gather", lambda: L.grouped_gemm_gather(c["x"], c["tok"], c["w1"], c["offsets"], E, rows, F, d, 1,
                                                           L.EPI_BIAS_RELU, bias=c["b1"]), 2.0 * A * F * d, 0),
        # as the layer's backward runs it: dY rows gathered by token and scaled by the gate in both halves
        ("gemm_pair2", lambda: L.grouped_gemm_bwd_pair(c["dy"], c["w2"], c["offsets"], E, rows, F, d, L.EPI_RELU_MASK,
                                                       c["h"], c["dy"], c["h"], a_gather=c["tok"], row_scale=c["gate"],
                                                       wx_gather=c["tok"], wx_scale=c["gate"]), 4.0 * A * F * d, 0),
        ("gemm_pair1", lambda: L.grouped_gemm_bwd_pair(c["dh"], c["w1"], c["offsets"], E, rows, d, F, L.EPI_NONE,
                                                       None, c["dh"], c["x"], c["tok"]), 4.0 * A * F * d, 0),
        # the layer's backward since round 5: dH, then {dXp, dW2, dW1} in one grid (moe_expert_ffn_bwd)
        ("ffn_bwd2", lambda: L.expert_ffn_bwd(c["dy"], c["tok"], c["gate"], c["x"], c["h"], c["w1"], c["w2"],
                                              c["offsets"], E, rows), 8.0 * A * F * d, 0),
        ("route_dispatch", lambda: L.route_dispatch(c["bcnt"], c["idx"], c["lrank"], c["w"], c["auxp"], T, E, 0,
                                                    rows, 1e-2, 1e-3, row_gate=True), 0, 24 * A),
        ("moe_layer_fwd_bwd", lambda: layer_fwd_bwd(c), 6.0 * A * F * d, 0),
        ("combine", lambda: L.combine_fwd(c["yp"], c["pos"], c["w"], T), 0, 512 * (A + T) + 8 * A),
        ("combine_bwd", lambda: L.combine_bwd(c["dy"], c["yp"], c["pos"], c["w"]), 0, 512 * (T + 2 * A) + 12 * A),
        ("gemm_dgrad2", lambda: L.grouped_gemm(c["dyp"], c["w2"], c["offsets"], E, rows, F, d, 0, L.EPI_RELU_MASK,
                                               aux=c["h"]), 2.0 * A * F * d, 0),
        ("gemm_wgrad2", lambda: L.grouped_gemm_wgrad(c["dyp"], c["h"], c["offsets"], E), 2.0 * A * F * d, 0),
        ("gemm_dgrad1", lambda: L.grouped_gemm(c["dh"], c["w1"], c["offsets"], E, rows, d, F, 0, L.EPI_NONE),
         2.0 * A * F * d, 0),
        ("gemm_wgrad1", lambda: L.grouped_gemm_wgrad(c["dh"], c["xp"], c["offsets"], E), 2.0 * A * F * d, 0),
        # MXFP8 (C5) variants: bytes are the algorithmic ones of the fp8 operands
        ("permute_mx", lambda: L.permute_fwd_mx(c["x"], c["idx"], c["lrank"], c["rank_base"], c["offsets"], E, 0,
                                                rows), 0, 512 * T + (256 + 8) * A + 12 * A),
        ("quantize_w1_mx", lambda: L.quantize_mx(c["w1"]), 0, E * F * d * (2 + 1 + 1 / 32)),
        ("gemm1_fwd_mx", lambda: L.grouped_gemm_mx(c["xq"], c["xs"], c["w1q"], c["w1s"], c["offsets"], E, rows, F, d,
                                                   L.EPI_BIAS_RELU, bias=c["b1"], out_mx=True), 2.0 * A * F * d, 0),
        ("gemm2_fwd_mx", lambda: L.grouped_gemm_mx(c["hq"], c["hs"], c["w2q"], c["w2s"], c["offsets"], E, rows, d, F,
                                                   L.EPI_BIAS, bias=c["b2"]), 2.0 * A * F * d, 0),
        ("gemm_dgrad2_mx", lambda: L.grouped_gemm(c["dyp"], c["w2"], c["offsets"], E, rows, F, d, 0,
                                                  L.EPI_RELU_MASK_MX, aux=c["hq"]), 2.0 * A * F * d, 0),
        ("gemm_wgrad2_mx", lambda: L.grouped_gemm_wgrad_mx(c["dyp"], c["hq"], c["hs"], c["offsets"], E),
         2.0 * A * F * d, 0),
        ("gemm_wgrad1_mx", lambda: L.grouped_gemm_wgrad_mx(c["dh"], c["xq"], c["xs"], c["offsets"], E),
         2.0 * A * F * d, 0),
        ("router_wgrad", lambda: L.router_wgrad(c["dlogits"], c["x"], c["ci"], c["tpi"], 6), 0,
         4 * T * E + 512 * T + 4 * (E * d + 6 * E)),
        ("token_bwd", lambda: L.token_bwd(c["dxp"], c["pos"], c["probs"], c["idx"], c["w"], c["dw"], c["lse"],
                                          None, None, c["wg"], True), 0, 512 * (A + T) + 4 * (2 * E + 3 * k) * T),
    ]
    return out


def augment_leg(reps, rounds):
    """The augmentation kernels at C2's batch (B 8, 3x736x1280 with 720 content
    rows, M 16): us and GB/s of algorithmic bytes (the source content once +
    the destination; boxes: the padded targets in and out), median over
    rounds, next to the same work done by augment_reference on GPU tensors
    (the torch-composition baseline, timed with events around the whole call,
    its cast to bf16 channels_last included).  The mosaic kernels run on the
    same batch in the same process, each leg right after its plain
    counterpart in every round (a [B, 24] table with mosaic on every row,
    boxes compacted from M 16 into M_out 64)."""
    from src.rtdetr_moe import augment as A
    from src.rtdetr_moe.criterion import pad_targets

    B, hw, phw, M = 8, (720, 1280), (736, 1280), 16
    g = torch.Generator().manual_seed(0)
    table = A.draw_params(g, B, hw, phw).cuda()
    mtable = A.draw_mosaic_params(torch.Generator().manual_seed(0), B, hw, phw, 1.0).cuda()
    Mo = 64
    u8 = torch.zeros((B, 3, *phw), dtype=torch.uint8)
    u8[:, :, :hw[0]] = torch.randint(0, 256, (B, 3, *hw), generator=g, dtype=torch.uint8)
    u8 = u8.cuda()
    f32 = (u8.float() / 255.0).contiguous(memory_format=torch.channels_last)
    targets = [{"boxes": torch.rand((n, 4), generator=g).cuda() * 0.2 + 0.3,
                "labels": torch.zeros(n, dtype=torch.int64, device="cuda")} for n in (3, 0, 16, 5, 1, 7, 2, 4)]
    tb, tl, nv = pad_targets(targets, M)
    outs = {dt: torch.empty((B, 3, *phw), dtype=dt, device="cuda", memory_format=torch.channels_last)
            for dt in (torch.bfloat16, torch.float32)}
    box_out = (torch.empty_like(tb), torch.empty_like(tl), torch.empty_like(nv),
               torch.empty((), dtype=torch.float32, device="cuda"))
    mbox_out = (torch.empty((B, Mo, 4), device="cuda"), torch.empty((B, Mo), dtype=torch.int64, device="cuda"),
                torch.empty_like(nv), torch.empty((), dtype=torch.float32, device="cuda"))
    px_src, px_dst = B * 3 * hw[0] * hw[1], B * 3 * phw[0] * phw[1]
    legs = [("augment_images u8_nchw->bf16", lambda: A.augment_images_hip(u8, table, outs[torch.bfloat16], hw),
             px_src + 2 * px_dst),
            ("mosaic_images u8_nchw->bf16", lambda: A.mosaic_images_hip(u8, mtable, outs[torch.bfloat16], hw),
             px_src + 2 * px_dst),
            ("augment_images f32_nhwc->bf16", lambda: A.augment_images_hip(f32, table, outs[torch.bfloat16], hw),
             4 * px_src + 2 * px_dst),
            ("mosaic_images f32_nhwc->bf16", lambda: A.mosaic_images_hip(f32, mtable, outs[torch.bfloat16], hw),
             4 * px_src + 2 * px_dst),
            ("augment_images f32_nhwc->f32", lambda: A.augment_images_hip(f32, table, outs[torch.float32], hw),
             4 * px_src + 4 * px_dst),
            ("augment_boxes (2 launches)", lambda: A.augment_boxes_hip(tb, tl, nv, table, hw, phw, out=box_out),
             B * (M * 48 + 8 + 64) + 4 * B + 4),
            ("mosaic_boxes (2 launches)", lambda: A.mosaic_boxes_hip(tb, tl, nv, mtable, hw, phw, out=mbox_out),
             B * (4 * M * 24 + Mo * 24 + 8 + 96) + 4 * B + 4)]

    def torch_ref():
        img, *_ = A.augment_reference(f32, tb, tl, nv, table, hw)
        return img.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def event_timed(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    res = {}
    for _ in range(rounds):
        for name, fn, byts in legs:
            res.setdefault((name, byts), []).append(timed(fn, reps))
        res.setdefault(("augment_reference torch f32_nhwc->bf16 (events, whole call)", 4 * px_src + 2 * px_dst),
                       []).append(event_timed(torch_ref, max(3, reps // 10)))
    for (name, byts), us in res.items():
        med = statistics.median(us)
        print(json.dumps({"kernel": name, "shape": f"B{B} 3x{phw[0]}x{phw[1]} content {hw[0]}x{hw[1]} M{M}",
                          "us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                          "GBs": round(byts / med * 1e-3, 1), "bytes": byts}), flush=True)


def _eval_match_inputs(rng, B, K, M):
    """One batch of the eval-match legs: M truths per image, K predictions of
    which half are jittered truths and half noise, one class.  Returns the host
    arrays (boxes, scores, labels, gt, gl) and rtdetr_eval_match's device operands."""
    import numpy as np

    from src.rtdetr_moe import metrics as MT

    xy = rng.uniform(0, 1100, (B, M, 2))
    gt = np.concatenate([xy, xy + rng.uniform(15, 120, (B, M, 2))], 2)
    src = rng.integers(0, M, (B, K))
    boxes = np.take_along_axis(gt, src[..., None], 1) + rng.uniform(-6, 6, (B, K, 4))
    noise = rng.random((B, K)) < 0.5
    p = rng.uniform(0, 1100, (int(noise.sum()), 2))
    boxes[noise] = np.concatenate([p, p + rng.uniform(5, 120, p.shape)], 1)  # half the predictions: noise
    boxes = boxes.astype(np.float32)
    scores = rng.random((B, K)).astype(np.float32)
    labels = np.zeros((B, K), np.int64)
    gl = np.zeros((B, M), np.int64)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = (cu(boxes), cu(scores), cu(labels.astype(np.int32)), cu(gt), cu(gl.astype(np.int32)),
         torch.full((B,), M, dtype=torch.int32, device="cuda"), cu(np.asarray(MT.IOU_THRESHOLDS, np.float64)))
    return boxes, scores, labels, gt, gl, d


def eval_match_bands_leg(reps, rounds):
    """The size-stratified matcher at the eval-match leg's shapes (B 16, K 300,
    M 20 or 64, one class) with the three default bands, every other image at
    the scale of a 3848 x 2168 frame evaluated at 1248 x 704: us per batch of
    rtdetr_eval_match_bands and of rtdetr_eval_match on the same inputs
    (dispatch-stamped kernel time), next to ms per batch of the host's
    metrics.match_predictions_banded (wall clock, 16 images).  Refuses to time
    unless the codes equal the reference.  Median, min and max over the rounds,
    the sides interleaved in each round."""
    import time

    import numpy as np

    from src.rtdetr_moe import metrics as MT

    B, K = 16, 300
    names, bands = MT.named_bands()
    scale = np.where(np.arange(B) % 2 == 0, 1.0, 2168 / 704)
    rng = np.random.default_rng(0)
    for M in (20, 64):
        boxes, scores, labels, gt, gl, d = _eval_match_inputs(rng, B, K, M)
        db = (*d, torch.from_numpy(scale).cuda(), torch.from_numpy(bands).cuda())

        def host_path():
            return np.stack([MT.match_predictions_banded(boxes[b], scores[b], labels[b], gt[b], gl[b], bands, scale[b])
                             for b in range(B)])

        want = host_path()
        if not np.array_equal(L.eval_match_bands(*db).cpu().numpy(), want):
            raise SystemExit("eval_match_bands differs from match_predictions_banded")
        res = {"bands_kernel_us": [], "eval_match_kernel_us": [], "host_match_ms": []}
        for _ in range(rounds):
            res["bands_kernel_us"].append(timed(lambda: L.eval_match_bands(*db), reps))
            res["eval_match_kernel_us"].append(timed(lambda: L.eval_match(*d), reps))
            t0 = time.perf_counter()
            host_path()
            res["host_match_ms"].append(1e3 * (time.perf_counter() - t0))
        out = {"kernel": "rtdetr_eval_match_bands",
               "shape": f"B{B} K{K} M{M} T{len(MT.IOU_THRESHOLDS)} R{len(bands)}", "bands": names,
               "codes_at_0.5": {n: [int((want[:, r, :, 0] == c).sum()) for c in (0, 1, 2)] for r, n in enumerate(names)}}
        for k, v in res.items():
            out[k] = round(statistics.median(v), 3)
            out[k + "_min"] = round(min(v), 3)
            out[k + "_max"] = round(max(v), 3)
        print(json.dumps(out), flush=True)


def eval_match_leg(reps, rounds):
    """The validation matcher at the eval leg's shape (B 16, K 300 predictions,
    M 20 or 64 truths per image, one class): us per batch of rtdetr_eval_match
    (dispatch-stamped kernel time) next to ms per batch of the host's
    metrics.match_predictions on the same inputs (wall clock, 16 images), and
    ms per batch of the whole device path of the evaluator (upload, launch, one
    packed copy back; wall clock ending in that copy).  Median, min and max
    over the rounds, the two sides interleaved in each round."""
    import time

    import numpy as np

    from src.rtdetr_moe import metrics as MT

    B, K = 16, 300
    rng = np.random.default_rng(0)
    for M in (20, 64):
        boxes, scores, labels, gt, gl, d = _eval_match_inputs(rng, B, K, M)
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        tp = L.eval_match(*d).cpu().numpy().astype(bool)
        want = np.stack([MT.match_predictions(boxes[b], scores[b], labels[b], gt[b], gl[b]) for b in range(B)])
        if not np.array_equal(tp, want):
            raise SystemExit("eval_match differs from match_predictions")
        # the evaluator's device path end to end, on normalised cxcywh targets of a 1280 x 736 image
        W, H = 1280, 736
        tg = [{"boxes": torch.from_numpy(np.stack([(gt[b, :, 0] + gt[b, :, 2]) / 2 / W,
                                                   (gt[b, :, 1] + gt[b, :, 3]) / 2 / H,
                                                   (gt[b, :, 2] - gt[b, :, 0]) / W,
                                                   (gt[b, :, 3] - gt[b, :, 1]) / H], 1).astype(np.float32)),
               "labels": torch.zeros(M, dtype=torch.int64)} for b in range(B)]
        db, ds, dl = d[0], d[1], cu(labels)

        def device_path():
            MT.DeviceDetectionEvaluator().update_batch(db, ds, dl, tg, size=(W, H))

        def wall(fn, n):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            return statistics.median(ts)

        def host_path():
            for b in range(B):
                MT.match_predictions(boxes[b], scores[b], labels[b], gt[b], gl[b])

        res = {"kernel_us": [], "device_path_ms": [], "host_match_ms": []}
        for _ in range(rounds):
            res["kernel_us"].append(timed(lambda: L.eval_match(*d), reps))
            res["device_path_ms"].append(wall(device_path, max(3, reps // 5)))
            res["host_match_ms"].append(wall(host_path, 3))
        out = {"kernel": "rtdetr_eval_match", "shape": f"B{B} K{K} M{M} T{len(MT.IOU_THRESHOLDS)}",
               "true_positives_at_0.5": int(want[..., 0].sum())}
        for k, v in res.items():
            out[k] = round(statistics.median(v), 3)
            out[k + "_min"] = round(min(v), 3)
            out[k + "_max"] = round(max(v), 3)
        print(json.dumps(out), flush=True)


def route_stats_leg(reps, rounds):
    """moe_route_stats at C2's eval shapes (batch 16: encoder T = 16 x 920,
    decoder T = 16 x 300; E 8, k 2, 6 contexts) against
    stats.route_stats_reference on the same device tensors (checked equal
    first).  kernel_us: the kernel's dispatch-stamped execution time.
    kernel_stream_us / reference_stream_us: stream time per call, from one
    event pair around ``reps`` back-to-back calls (launch gaps included: what
    the torch form's dozen launches cost in an eager pass).  Median, min and max
    over the rounds, the two sides interleaved in each round."""
    from src.moe.stats import route_stats_reference

    B, E, k, n_ctx = 16, 8, 2, 6
    g = torch.Generator().manual_seed(0)
    for name, tpi in (("encoder", 920), ("decoder", 300)):
        T = B * tpi
        probs = torch.softmax(2.0 * torch.randn((T, E), generator=g), -1).cuda()
        idx = torch.rand((T, E), generator=g).argsort(1)[:, :k].to(torch.int32).contiguous().cuda()
        w = torch.softmax(torch.randn((T, k), generator=g), -1).cuda()
        pos = torch.arange(T * k, dtype=torch.int32).view(T, k).clone()
        pos[torch.rand((T, k), generator=g) < 0.1] = -1
        pos = pos.cuda()
        ci = torch.randint(n_ctx, (B,), generator=g).to(torch.int32).cuda()
        table = torch.zeros((n_ctx, E, 5), dtype=torch.int64, device="cuda")
        L.route_stats(idx, w, pos, probs, ci, n_ctx, tpi, table)
        if not torch.equal(table, route_stats_reference(idx, w, pos, probs, ci, tpi, n_ctx)):
            raise SystemExit("route_stats differs from route_stats_reference")

        def kernel():
            L.route_stats(idx, w, pos, probs, ci, n_ctx, tpi, table)

        def reference():
            table.add_(route_stats_reference(idx, w, pos, probs, ci, tpi, n_ctx))

        def stream_us(fn, n):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / n

        res = {"kernel_us": [], "kernel_stream_us": [], "reference_stream_us": []}
        for _ in range(rounds):
            res["kernel_us"].append(timed(kernel, reps))
            res["kernel_stream_us"].append(stream_us(kernel, reps))
            res["reference_stream_us"].append(stream_us(reference, reps))
        out = {"kernel": "moe_route_stats", "shape": f"{name} T{T} E{E} k{k} C{n_ctx}"}
        for key, v in res.items():
            out[key] = round(statistics.median(v), 2)
            out[key + "_min"] = round(min(v), 2)
            out[key + "_max"] = round(max(v), 2)
        print(json.dumps(out), flush=True)


def balance_leg(reps, rounds, steps=3000):
    """Loss-free load balancing (src/moe/balance.py).  Checks the biased router
    against eager.route and moe_balance_step against balance_reference; times
    the router with and without a selection bias, alternated in every round,
    at the shapes of the ``router`` line (C2 encoder / decoder), and the
    balance launch for C2's 7 MoE layers; then runs the update rule on the
    kernels: a frozen router at the project's init scales (E 8, top-2, d 256,
    6 contexts, router_init_std 0.02, ctx_init_scale 0.5), 8 images x 300
    unit-normal decoder tokens per step, ``steps`` steps, contexts mixed per
    image or one per batch, rate 0 and 1e-3.  Prints the max violation (max
    load / mean - 1) and the share of assignments a capacity factor of 1.25
    would drop, each as the mean over the first and over the last 100 steps.
    The per-context form (-albc: moe_router_topk_fwd_selctx,
    moe_balance_step_ctx) has the same legs: checks against eager.route with a
    [C, E] table and against context_counts + balance_reference on the rows;
    the three routers alternated; the balance launch with mixed contexts and
    with all images in one (the worst case: one workgroup per layer counts
    everything) at C2's and C5's shapes; the simulation with a [C, E] table at
    rates 1e-3 and 1e-2 (max violation and drops of the whole batch, as in the
    other rows).  Synthetic inputs and frozen weights: not a statement about
    accuracy."""
    import math

    import numpy as np

    from src.moe.balance import _REC, _REC_CTX, balance_reference, context_counts
    from src.moe.eager import route

    # -- checks ----------------------------------------------------------------
    g = torch.Generator().manual_seed(0)
    T, d, E, k, tpi, C = 2400, 256, 8, 2, 300, 6
    x = (torch.randint(-8, 9, (T, d), generator=g).float() / 8)
    wg = torch.randint(-4, 5, (E, d), generator=g).float() / 16
    cb = torch.randint(-64, 65, (C, E), generator=g).float() / 64
    sb = torch.randint(-256, 257, (E,), generator=g).float() / 128
    ci = torch.randint(0, C, (T // tpi,), generator=g).int()
    probs_r, lse_r, idx_r, w_r = route(x, wg, cb, ci, tpi, k, True, sb)
    idx, w, probs, lse, *_ = L.router_topk_fwd(x.to(torch.bfloat16).cuda(), wg.cuda(), cb.cuda(), ci.cuda(), tpi, k,
                                               True, sel_bias=sb.cuda())
    if not torch.equal(idx.cpu().long(), idx_r):
        raise SystemExit("the biased router's selection differs from eager.route")
    err = max(float((probs.cpu() - probs_r).abs().max()), float((w.cpu() - w_r).abs().max()))
    if err > 2e-6:
        raise SystemExit(f"the biased router's probs / gates are {err:.2e} from eager.route")

    def table(hists, biases):
        rec = np.zeros(len(biases), dtype=_REC)
        for i, b in enumerate(biases):
            rec[i]["hist"] = 0 if hists is None else hists[i].data_ptr()
            rec[i]["bias"] = b.data_ptr()
        return torch.from_numpy(rec.view(np.uint8).copy()).cuda()

    Lc = 7
    hist = torch.randint(0, 1000, (Lc, E), generator=g).int()
    bias = torch.randint(-256, 257, (Lc, E), generator=g).float() / 128
    load_r, bias_r = hist.long(), bias.clone()
    maxvio_r = balance_reference(load_r, bias_r, 1e-3)
    hist_g, bias_g = hist.cuda(), bias.cuda()
    load_g = torch.zeros((Lc, E), dtype=torch.int64, device="cuda")
    maxvio = torch.zeros(Lc, device="cuda")
    tab = table([hist_g[l] for l in range(Lc)], [bias_g[l] for l in range(Lc)])
    L.balance_step(tab, Lc, E, load_g, 1e-3, True, maxvio)
    if not (torch.equal(bias_g.cpu(), bias_r) and torch.equal(maxvio.cpu(), maxvio_r) and int(load_g.abs().sum()) == 0):
        raise SystemExit("moe_balance_step differs from balance_reference")
    print(json.dumps({"check": "balance", "router_idx_equal": True, "router_max_abs_err": err,
                      "balance_step_bitwise": True}), flush=True)

    # the per-context form
    sbc = torch.randint(-256, 257, (C, E), generator=g).float() / 128
    probs_r, lse_r, idx_r, w_r = route(x, wg, cb, ci, tpi, k, True, sbc)
    idx, w, probs, lse, *_ = L.router_topk_fwd(x.to(torch.bfloat16).cuda(), wg.cuda(), cb.cuda(), ci.cuda(), tpi, k,
                                               True, sel_bias=sbc.cuda())
    if not torch.equal(idx.cpu().long(), idx_r):
        raise SystemExit("the per-context router's selection differs from eager.route")
    errc = max(float((probs.cpu() - probs_r).abs().max()), float((w.cpu() - w_r).abs().max()))
    if errc > 2e-6:
        raise SystemExit(f"the per-context router's probs / gates are {errc:.2e} from eager.route")

    def ctx_table(idxs, biases, ctxs, tpis):
        rec = np.zeros(len(biases), dtype=_REC_CTX)
        for i, b in enumerate(biases):
            rec[i]["topk_idx"] = 0 if idxs is None else idxs[i].data_ptr()
            rec[i]["bias"], rec[i]["ctx_img"] = b.data_ptr(), ctxs[i].data_ptr()
            rec[i]["T"], rec[i]["tokens_per_image"] = ctxs[i].numel() * tpis[i], tpis[i]
        return torch.from_numpy(rec.view(np.uint8).copy()).cuda()

    def ctx_case(Ec, kc, Bc, single):
        """C2 / C5-like: one encoder layer (920 tokens per image) and six decoder layers (300)."""
        tp = [920] + [300] * (Lc - 1)
        ids = [torch.rand((Bc * t, Ec), generator=g).argsort(1)[:, :kc].int().contiguous() for t in tp]
        cs = [torch.randint(0, C, (Bc,), generator=g).int() for _ in tp]
        if single:
            cs = [c[:1].expand(Bc).contiguous() for c in cs]
        return tp, ids, cs

    tp, ids, cs = ctx_case(E, k, 8, False)
    biasc = torch.randint(-256, 257, (Lc, C, E), generator=g).float() / 128
    loadc_r = torch.stack([context_counts(i, c, t, C, E) for i, c, t in zip(ids, cs, tp)])
    biasc_r = biasc.clone()
    mvc_r = balance_reference(loadc_r.view(-1, E), biasc_r.view(-1, E), 1e-3).view(Lc, C)
    ids_g, cs_g, biasc_g = [i.cuda() for i in ids], [c.cuda() for c in cs], biasc.cuda()
    loadc_g = torch.zeros((Lc, C, E), dtype=torch.int64, device="cuda")
    mvc = torch.zeros((Lc, C), device="cuda")
    tabc = ctx_table(ids_g, [biasc_g[l] for l in range(Lc)], cs_g, tp)
    L.balance_step_ctx(tabc, Lc, C, E, k, loadc_g, 1e-3, True, mvc)
    if not (torch.equal(biasc_g.cpu(), biasc_r) and torch.equal(mvc.cpu(), mvc_r) and int(loadc_g.abs().sum()) == 0):
        raise SystemExit("moe_balance_step_ctx differs from context_counts + balance_reference")
    print(json.dumps({"check": "balance per context", "router_idx_equal": True, "router_max_abs_err": errc,
                      "balance_step_ctx_bitwise": True}), flush=True)

    # -- timing ----------------------------------------------------------------
    shapes = {"enc": setup(8 * 920, 8, 2, 256, 1024), "dec": setup(8 * 300, 8, 2, 256, 1024, seed=1)}
    for sname, c in shapes.items():
        sel = torch.randn(c["E"], device="cuda") * 0.1
        selc = torch.randn((6, c["E"]), device="cuda") * 0.1
        res = {"plain": [], "sel": [], "selctx": []}
        for _ in range(rounds):
            res["plain"].append(timed(lambda: L.router_topk_fwd(c["x"], c["wg"], c["cb"], c["ci"], c["tpi"], c["k"],
                                                                True), reps))
            res["sel"].append(timed(lambda: L.router_topk_fwd(c["x"], c["wg"], c["cb"], c["ci"], c["tpi"], c["k"],
                                                              True, sel_bias=sel), reps))
            res["selctx"].append(timed(lambda: L.router_topk_fwd(c["x"], c["wg"], c["cb"], c["ci"], c["tpi"], c["k"],
                                                                 True, sel_bias=selc), reps))
        out = {"kernel": "router", "shape": sname, "cold": _FLUSH is not None}
        for key, v in res.items():
            out[key + "_us"] = round(statistics.median(v), 2)
            out[key + "_us_min"] = round(min(v), 2)
            out[key + "_us_max"] = round(max(v), 2)
        out["sel_over_plain"] = round(out["sel_us"] / out["plain_us"], 4)
        out["selctx_over_plain"] = round(out["selctx_us"] / out["plain_us"], 4)
        out["selctx_over_sel"] = round(out["selctx_us"] / out["sel_us"], 4)
        print(json.dumps(out), flush=True)
    res = {"add": [], "apply": []}
    for _ in range(rounds):
        res["add"].append(timed(lambda: L.balance_step(tab, Lc, E, load_g, 1e-3, False, maxvio), reps))
        res["apply"].append(timed(lambda: L.balance_step(tab, Lc, E, load_g, 1e-3, True, maxvio), reps))
    out = {"kernel": "moe_balance_step", "shape": f"L{Lc} E{E}"}
    for key, v in res.items():
        out[key + "_us"] = round(statistics.median(v), 2)
        out[key + "_us_min"] = round(min(v), 2)
        out[key + "_us_max"] = round(max(v), 2)
    print(json.dumps(out), flush=True)
    for Ec, kc, Bc in ((8, 2, 8), (32, 4, 16)):  # C2's and C5's MoE layers
        for single in (False, True):
            tp, ids, cs = ctx_case(Ec, kc, Bc, single)
            ids_g, cs_g = [i.cuda() for i in ids], [c.cuda() for c in cs]
            bg = torch.zeros((Lc, C, Ec), device="cuda")
            lg = torch.zeros((Lc, C, Ec), dtype=torch.int64, device="cuda")
            mg = torch.zeros((Lc, C), device="cuda")
            tb = ctx_table(ids_g, [bg[l] for l in range(Lc)], cs_g, tp)
            res = {"add": [], "apply": []}
            for _ in range(rounds):
                res["add"].append(timed(lambda: L.balance_step_ctx(tb, Lc, C, Ec, kc, lg, 1e-3, False, mg), reps))
                res["apply"].append(timed(lambda: L.balance_step_ctx(tb, Lc, C, Ec, kc, lg, 1e-3, True, mg), reps))
            out = {"kernel": "moe_balance_step_ctx", "shape": f"L{Lc} C{C} E{Ec} k{kc} batch {Bc}",
                   "contexts": "one per batch" if single else "mixed"}
            for key, v in res.items():
                out[key + "_us"] = round(statistics.median(v), 2)
                out[key + "_us_min"] = round(min(v), 2)
                out[key + "_us_max"] = round(max(v), 2)
            print(json.dumps(out), flush=True)

    # -- the rule on the kernels -------------------------------------------------
    B = T // tpi
    cap = int(math.ceil(1.25 * T * k / E))
    for batches in ("mixed contexts", "one context per batch"):
        for rate, per_ctx in ((0.0, False), (1e-3, False), (1e-3, True), (1e-2, True)):
            gg = torch.Generator(device="cuda").manual_seed(1)
            wgs = (torch.randn((E, d), device="cuda", generator=gg) * 0.02).float()
            cbs = (torch.randn((C, E), device="cuda", generator=gg) * 0.5).float()
            sbias = torch.zeros((C, E) if per_ctx else E, device="cuda")
            load = torch.zeros((1, C, E) if per_ctx else (1, E), dtype=torch.int64, device="cuda")
            mv = torch.zeros(C if per_ctx else 1, device="cuda")
            vio = torch.zeros(steps, device="cuda")
            drop = torch.zeros(steps, device="cuda")
            keep = []  # every step's hist and table stay alive until the final synchronize
            for s in range(steps):
                xs = torch.randn((T, d), device="cuda", generator=gg).to(torch.bfloat16)
                cis = torch.randint(0, C, (B,), device="cuda", generator=gg).int()
                if batches != "mixed contexts":
                    cis = cis[:1].expand(B).contiguous()
                idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(xs, wgs, cbs, cis, tpi, k, True,
                                                                           sel_bias=sbias)
                h = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, 0, T * k)[2]
                if per_ctx:  # the rows move by their contexts' loads; the violation reported is the batch's
                    tb = ctx_table([idx], [sbias], [cis], [tpi])
                    L.balance_step_ctx(tb, 1, C, E, k, load, rate, True, mv)
                    vio[s] = (E * h.max() - h.sum()) / h.sum()
                else:
                    tb = table([h], [sbias])
                    L.balance_step(tb, 1, E, load, rate, True, mv)
                    vio[s] = mv[0]
                drop[s] = (h - cap).clamp(min=0).sum() / float(T * k)
                keep.append((h, tb, idx, cis))
                if len(keep) >= 256:
                    torch.cuda.synchronize()
                    keep.clear()
            torch.cuda.synchronize()
            n = min(100, steps)
            print(json.dumps({"simulation": batches, "bias": "per context" if per_ctx else "per expert",
                              "rate": rate, "steps": steps, "cap_factor": 1.25,
                              "maxvio_first": round(float(vio[:n].mean()), 3),
                              "maxvio_last": round(float(vio[-n:].mean()), 3),
                              "dropped_first": round(float(drop[:n].mean()), 3),
                              "dropped_last": round(float(drop[-n:].mean()), 3),
                              "bias_final": [round(float(v), 4) for v in sbias.cpu().reshape(-1)]}), flush=True)


def resize_leg(reps, rounds):
    """rtdetr_resize_pad_u8 on a batch of 16 frames: ZOD's 3848 x 2168 ->
    1248 x 704, and 1280 x 720 at identity scale padded to 736.  kernel_us: the
    kernel's dispatch-stamped execution time; GBs: (source bytes + 12 pad_h
    pad_w B) over it, and its share of the HBM peak.  device_path_ms: upload of
    the packed uint8 batch + the launch, wall clock.  host_path_ms: what it
    replaces, on this machine's CPU in this process -- PIL resize +
    _padded_image per frame, the fp32 upload and the channels-last copy, wall
    clock.  Median, min and max over the rounds, the sides interleaved in each
    round; the kernel's output is checked against resize_reference first."""
    import time

    import numpy as np

    from src.rtdetr_moe.preprocess import HostCollate, PackCollate, padded_hw, resize_reference

    B = 16
    rng = np.random.default_rng(0)
    for name, (sh, sw), imgsz in (("zod", (2168, 3848), (704, 1248)), ("identity", (720, 1280), (720, 1280))):
        out_hw, pad_hw = padded_hw(imgsz)
        # smooth content plus noise, one frame per slot
        frames = []
        for _ in range(B):
            base = rng.integers(0, 256, (sh // 8 + 1, sw // 8 + 1, 3)).astype(np.float32)
            up = np.kron(base, np.ones((8, 8, 1), np.float32))[:sh, :sw]
            frames.append(np.clip(up + rng.normal(0, 8, (sh, sw, 3)), 0, 255).astype(np.uint8))
        items = [(f, f"{i}.png", 0) for i, f in enumerate(frames)]
        packed = PackCollate(out_hw)(items)
        buf, desc = packed["buf"].pin_memory(), packed["desc"]
        dbuf = buf.cuda()
        out = L.resize_pad(dbuf, desc, out_hw, pad_hw)
        ref = resize_reference(frames[0], *out_hw, *pad_hw)
        err = float((out[0].cpu().double() - ref).abs().max())
        if err > 5e-6:
            raise SystemExit(f"resize_pad differs from resize_reference by {err:.3e}")
        ddesc = desc.cuda()
        host = HostCollate(out_hw, pad_hw)

        def kernel():
            L.resize_pad(dbuf, None, out_hw, pad_hw, out=out, desc_dev=ddesc)

        def device_path():
            L.resize_pad(buf.cuda(non_blocking=True), desc, out_hw, pad_hw, out=out)

        def host_path():
            host(items)["images"].cuda(non_blocking=True).contiguous(memory_format=torch.channels_last)

        def wall(fn, n):
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            return statistics.median(ts)

        res = {"kernel_us": [], "device_path_ms": [], "host_path_ms": []}
        for _ in range(rounds):
            res["kernel_us"].append(timed(kernel, reps))
            res["device_path_ms"].append(wall(device_path, 5))
            res["host_path_ms"].append(wall(host_path, 1))
        byts = int(buf.numel()) + 12 * pad_hw[0] * pad_hw[1] * B
        line = {"kernel": "rtdetr_resize_pad_u8", "shape": f"{name} B{B} {sh}x{sw} -> {out_hw[0]}x{out_hw[1]} "
                f"(pad {pad_hw[0]}x{pad_hw[1]})", "max_err_vs_reference": err, "bytes": byts}
        for k, v in res.items():
            line[k] = round(statistics.median(v), 3)
            line[k + "_min"] = round(min(v), 3)
            line[k + "_max"] = round(max(v), 3)
        line["GBs"] = round(byts / line["kernel_us"] * 1e-3, 1)
        line["hbm_peak_share"] = round(line["GBs"] / L.PEAK_HBM_GBS, 3)
        line["host_over_device_path"] = round(line["host_path_ms"] / line["device_path_ms"], 1)
        print(json.dumps(line), flush=True)


def resize_flip_leg(reps, rounds):
    """rtdetr_resize_pad_u8_flip at --resize's shape (16 frames of 3848 x 2168
    -> 1248 x 704).  First equality: all flags 1 against rtdetr_resize_pad_u8 on
    host-mirrored frames, all flags 0 against it on the frames as they are
    (torch.equal, or the run stops).  Then three launches timed, interleaved in
    each round: all flags 0, all flags 1, and rtdetr_resize_pad_u8.  kernel_us:
    the dispatch-stamped execution time; median, min and max over the rounds."""
    import numpy as np

    from src.rtdetr_moe.preprocess import PackCollate, mirrored, padded_hw

    B, (sh, sw) = 16, (2168, 3848)
    out_hw, pad_hw = padded_hw((704, 1248))
    rng = np.random.default_rng(0)
    frames = []
    for _ in range(B):  # smooth content plus noise, one frame per slot (resize_leg's)
        base = rng.integers(0, 256, (sh // 8 + 1, sw // 8 + 1, 3)).astype(np.float32)
        up = np.kron(base, np.ones((8, 8, 1), np.float32))[:sh, :sw]
        frames.append(np.clip(up + rng.normal(0, 8, (sh, sw, 3)), 0, 255).astype(np.uint8))
    pack = PackCollate(out_hw)
    packed = pack([(f, f"{i}.png", 0) for i, f in enumerate(frames)])
    dbuf, desc = packed["buf"].cuda(), packed["desc"]
    L.check_resize_desc(desc, dbuf.numel())
    ddesc = desc.cuda()
    zeros, ones = (torch.full((B,), v, dtype=torch.int32, device="cuda") for v in (0, 1))
    plain = L.resize_pad(dbuf, None, out_hw, pad_hw, desc_dev=ddesc)
    if not torch.equal(L.resize_pad(dbuf, None, out_hw, pad_hw, desc_dev=ddesc, flip=zeros), plain):
        raise SystemExit("rtdetr_resize_pad_u8_flip with flags 0 differs from rtdetr_resize_pad_u8")
    mbuf = pack([(mirrored(f), f"{i}.png", 0) for i, f in enumerate(frames)])["buf"].cuda()
    want = L.resize_pad(mbuf, None, out_hw, pad_hw, desc_dev=ddesc)
    del mbuf
    out = L.resize_pad(dbuf, None, out_hw, pad_hw, desc_dev=ddesc, flip=ones)
    if not torch.equal(out, want):
        raise SystemExit("rtdetr_resize_pad_u8_flip with flags 1 differs from rtdetr_resize_pad_u8 on mirrored frames")
    if torch.equal(out, plain):
        raise SystemExit("the mirrored launch wrote the unmirrored image")
    del want, plain
    legs = {"flip_all_0": lambda: L.resize_pad(dbuf, None, out_hw, pad_hw, out=out, desc_dev=ddesc, flip=zeros),
            "flip_all_1": lambda: L.resize_pad(dbuf, None, out_hw, pad_hw, out=out, desc_dev=ddesc, flip=ones),
            "rtdetr_resize_pad_u8": lambda: L.resize_pad(dbuf, None, out_hw, pad_hw, out=out, desc_dev=ddesc)}
    res = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(timed(fn, reps))
    byts = int(dbuf.numel()) + 12 * pad_hw[0] * pad_hw[1] * B
    line = {"kernel": "rtdetr_resize_pad_u8_flip", "shape": f"B{B} {sh}x{sw} -> {out_hw[0]}x{out_hw[1]} "
            f"(pad {pad_hw[0]}x{pad_hw[1]})", "equal_to_host_mirrored": True, "rounds": rounds, "bytes": byts}
    for k, v in res.items():
        line[k + "_us"] = round(statistics.median(v), 3)
        line[k + "_us_min"] = round(min(v), 3)
        line[k + "_us_max"] = round(max(v), 3)
    line["mirrored_over_unmirrored"] = round(line["flip_all_1_us"] / line["flip_all_0_us"], 3)
    print(json.dumps(line), flush=True)


def nms_merge_leg(reps, rounds):
    """rtdetr_nms_merge at tiled prediction's shape (B 16 frames, N 1500
    candidates: the full frame and a 2 x 2 grid at k 300; max_det 300; "ios" and
    "iou" at 0.5, conf 0.25) against merge.merge_reference on the host, same
    process, same candidates (checked equal first).  The candidates are
    clustered: N // 6 objects per frame, each several times, boxes of
    pedestrian shape jittered by a few pixels, scores on a 1/64 grid, two
    labels.  kernel_us: the kernel's dispatch-stamped execution time per launch;
    device_path_ms: launch + one packed copy back, wall clock; host_merge_ms:
    the reference loop over the 16 frames on arrays already on the host, wall
    clock.  forward_replay_us: one EvalForward graph replay at batch 16
    (rtdetr-r50-moe8-top2, 704 x 1248; event pair around the replay).  Median,
    min and max over the rounds, the sides interleaved in each round."""
    import time

    import numpy as np

    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference
    from src.rtdetr_moe.model import RTDETRMoE

    B, N, max_det, conf, thr = 16, 1500, 300, 0.25, 0.5
    rng = np.random.default_rng(0)
    M = N // 6
    cx, cy = rng.uniform(100, 3748, (B, M)), rng.uniform(120, 2048, (B, M))
    h = rng.uniform(40, 200, (B, M))
    which = rng.integers(0, M, (B, N))
    take = lambda a: np.take_along_axis(a, which, 1)  # noqa: E731
    jit = rng.normal(0.0, 3.0, (B, N, 4))
    x1, y1 = take(cx) - 0.2 * take(h) + jit[..., 0], take(cy) - 0.5 * take(h) + jit[..., 1]
    x2, y2 = take(cx) + 0.2 * take(h) + jit[..., 2], y1 + take(h) * rng.uniform(0.6, 1.0, (B, N)) + jit[..., 3]
    boxes = np.stack([x1, y1, x2, y2], -1).astype(np.float32)
    scores = (rng.integers(0, 64, (B, N)) / 64.0).astype(np.float32)
    labels = rng.integers(0, 2, (B, N)).astype(np.int32)
    db, ds, dl = (torch.from_numpy(a).cuda() for a in (boxes, scores, labels))

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    for metric in ("ios", "iou"):
        out = tuple(t.cpu() for t in L.nms_merge(db, ds, dl, None, conf, thr, metric, max_det))
        want = [merge_reference(boxes[b], scores[b], labels[b], None, conf, thr, metric, max_det) for b in range(B)]
        for b, k in enumerate(want):
            if int(out[4][b]) != len(k) or out[3][b, :len(k)].tolist() != k.tolist():
                raise SystemExit(f"nms_merge differs from merge_reference ({metric}, image {b})")

        def device_path():
            ob, osc, ol, osrc, _ = L.nms_merge(db, ds, dl, None, conf, thr, metric, max_det)
            torch.cat([ob, osc[..., None], ol[..., None].float(), osrc[..., None].float()], -1).cpu()

        def host_path():
            for b in range(B):
                merge_reference(boxes[b], scores[b], labels[b], None, conf, thr, metric, max_det)

        res = {"kernel_us": [], "device_path_ms": [], "host_merge_ms": [], "forward_replay_us": []}
        for _ in range(rounds):
            res["kernel_us"].append(timed(lambda: L.nms_merge(db, ds, dl, None, conf, thr, metric, max_det), reps))
            res["device_path_ms"].append(wall(device_path, max(3, reps // 5)))
            res["host_merge_ms"].append(wall(host_path, 3))
            res["forward_replay_us"].append(replay_us())
        line = {"kernel": "rtdetr_nms_merge", "shape": f"B{B} N{N} max_det{max_det} {metric} thr{thr} conf{conf}",
                "take_part": int((scores >= conf).sum()), "kept": int(sum(len(k) for k in want))}
        for k, v in res.items():
            line[k] = round(statistics.median(v), 3)
            line[k + "_min"] = round(min(v), 3)
            line[k + "_max"] = round(max(v), 3)
        line["host_over_kernel"] = round(1e3 * line["host_merge_ms"] / line["kernel_us"], 1)
        line["kernel_share_of_forward"] = round(line["kernel_us"] / line["forward_replay_us"], 4)
        print(json.dumps(line), flush=True)


def box_fuse_leg(reps, rounds):
    """rtdetr_box_fuse on the candidates of --nms-merge (B 16, N 1500, max_det
    300, "ios" 0.5, conf 0.25), laid out as 5 passes of k 300 with the 2 x 2
    windows of a 3848 x 2168 frame, fuse_thr 0.55: checked equal to
    merge.fuse_reference first, then fuse_kernel_us and nms_kernel_us
    (rtdetr_nms_merge on the same inputs; dispatch-stamped kernel time per
    launch) and forward_replay_us (one EvalForward graph replay at batch 16,
    rtdetr-r50-moe8-top2, 704 x 1248), alternated in each round; median, min
    and max over the rounds."""
    import numpy as np

    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import fuse_reference, tile_windows
    from src.rtdetr_moe.model import RTDETRMoE

    B, N, max_det, conf, thr, metric, fuse_thr = 16, 1500, 300, 0.25, 0.5, "ios", 0.55
    rng = np.random.default_rng(0)  # nms_merge_leg's draw
    M = N // 6
    cx, cy = rng.uniform(100, 3748, (B, M)), rng.uniform(120, 2048, (B, M))
    h = rng.uniform(40, 200, (B, M))
    which = rng.integers(0, M, (B, N))
    take = lambda a: np.take_along_axis(a, which, 1)  # noqa: E731
    jit = rng.normal(0.0, 3.0, (B, N, 4))
    x1, y1 = take(cx) - 0.2 * take(h) + jit[..., 0], take(cy) - 0.5 * take(h) + jit[..., 1]
    x2, y2 = take(cx) + 0.2 * take(h) + jit[..., 2], y1 + take(h) * rng.uniform(0.6, 1.0, (B, N)) + jit[..., 3]
    boxes = np.stack([x1, y1, x2, y2], -1).astype(np.float32)
    scores = (rng.integers(0, 64, (B, N)) / 64.0).astype(np.float32)
    labels = rng.integers(0, 2, (B, N)).astype(np.int32)
    win = np.asarray([(0, 0, 3848, 2168)] + [(x0, y0, x0 + tw, y0 + th)
                                             for x0, y0, tw, th in tile_windows(3848, 2168, (2, 2), 0.2)], np.float32)
    windows = np.broadcast_to(win, (B, 5, 4)).copy()
    db, ds, dl, dw = (torch.from_numpy(a).cuda() for a in (boxes, scores, labels, windows))

    out = tuple(t.cpu() for t in L.box_fuse(db, ds, dl, None, conf, thr, metric, max_det, False, fuse_thr, dw))
    members = 0
    for b in range(B):
        kept, fused, mem = fuse_reference(boxes[b], scores[b], labels[b], None, conf, thr, metric, max_det, False,
                                          fuse_thr, win)
        n = len(kept)
        if (int(out[4][b]) != n or out[3][b, :n].tolist() != kept.tolist()
                or not np.array_equal(out[0][b, :n].numpy().view(np.int32), fused.view(np.int32))
                or out[5][b, :n].tolist() != mem.tolist()):
            raise SystemExit(f"box_fuse differs from fuse_reference (image {b})")
        members += int(mem.sum())

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    res = {"fuse_kernel_us": [], "nms_kernel_us": [], "forward_replay_us": []}
    for _ in range(rounds):
        res["fuse_kernel_us"].append(timed(
            lambda: L.box_fuse(db, ds, dl, None, conf, thr, metric, max_det, False, fuse_thr, dw), reps))
        res["nms_kernel_us"].append(timed(lambda: L.nms_merge(db, ds, dl, None, conf, thr, metric, max_det), reps))
        res["forward_replay_us"].append(replay_us())
    line = {"kernel": "rtdetr_box_fuse",
            "shape": f"B{B} N{N} P5 max_det{max_det} {metric} thr{thr} fuse_thr{fuse_thr} conf{conf}",
            "take_part": int((scores >= conf).sum()), "kept": int(out[4].sum()), "members": members}
    for k, v in res.items():
        line[k] = round(statistics.median(v), 3)
        line[k + "_min"] = round(min(v), 3)
        line[k + "_max"] = round(max(v), 3)
    line["fuse_over_nms"] = round(line["fuse_kernel_us"] / line["nms_kernel_us"], 2)
    line["fuse_share_of_forward"] = round(line["fuse_kernel_us"] / line["forward_replay_us"], 4)
    print(json.dumps(line), flush=True)


def track_sequence(n_obj, F, K, seed=0, first=0):
    """A synthetic pedestrian sequence as a detector reports it: n_obj
    constant-velocity objects with 2 px of jitter per side, 10 % of them missed
    and 15 % scored low per frame, 3 false positives, fillers below the low band
    up to K rows, best first.  -> boxes fp32 [F, K, 4], scores fp32 [F, K],
    labels int32 [F, K], n_valid int32 [F] (the rows with score >= 0.1), truth
    int64 [F, K] (the object of a row, -1 for none).  Frames first..first+F-1."""
    import numpy as np

    rng = np.random.default_rng(seed)
    i = np.arange(n_obj)
    w, h = rng.uniform(30, 50, n_obj), rng.uniform(80, 120, n_obj)
    x0, y0 = 40.0 + (i % 10) * 110.0, 60.0 + (i // 10) * 150.0
    vx, vy = rng.uniform(-0.8, 0.8, n_obj), rng.uniform(-0.3, 0.3, n_obj)
    boxes, scores = np.zeros((F, K, 4), np.float32), np.zeros((F, K), np.float32)
    n_valid, truth = np.zeros(F, np.int32), np.full((F, K), -1, np.int64)
    for f in range(F):
        t = first + f
        rows = []
        for o in range(n_obj):
            if t > 0 and rng.random() < 0.1:
                continue
            sc = rng.uniform(0.15, 0.45) if t > 1 and rng.random() < 0.15 else rng.uniform(0.65, 0.95)
            x, y = x0[o] + vx[o] * t, y0[o] + vy[o] * t
            rows.append((sc, np.array([x, y, x + w[o], y + h[o]]) + rng.normal(0, 2.0, 4), o))
        for _ in range(3):
            x, y, ww = rng.uniform(0, 1188), rng.uniform(0, 574), rng.uniform(25, 55)
            rows.append((rng.uniform(0.1, 0.9), np.array([x, y, x + ww, y + 2.4 * ww]), -1))
        rows.sort(key=lambda r: -r[0])
        rows = rows[:K]
        n = len(rows)
        for d, (sc, b, o) in enumerate(rows):
            boxes[f, d], scores[f, d], truth[f, d] = b, sc, o
        fx, fy = rng.uniform(0, 1188, K - n), rng.uniform(0, 574, K - n)
        boxes[f, n:] = np.stack([fx, fy, fx + 40, fy + 100], 1)
        scores[f, n:] = np.sort(rng.uniform(0.001, 0.05, K - n))[::-1]
        n_valid[f] = n
    return boxes, scores, np.zeros((F, K), np.int32), n_valid, truth


def track_leg(reps, rounds):
    """rtdetr_track_update at predict's shape (F 16 frames of one sequence, K 300
    rows, 40 objects: about 40 live tracks, the defaults of track.TrackArgs)
    against track.track_reference on the host, same process, same candidates
    (outputs and state checked equal first, bit for bit).  The state before the
    timed batch is the one 16 earlier frames of the sequence leave; every timed
    launch starts from a copy of it.  kernel_us: the kernel's dispatch-stamped
    execution time per launch; device_path_ms: launch + one packed copy back,
    wall clock; host_track_ms: one copy back of the candidates + the reference
    loop over the 16 frames, wall clock.  forward_replay_us: one EvalForward
    graph replay at batch 16 (rtdetr-r50-moe8-top2, 704 x 1248).  Median, min
    and max over the rounds, the sides interleaved in each round.  Also the
    reference's ids per object and id switches over the 32 frames (no accuracy
    claim: synthetic constant-velocity input)."""
    import time

    import numpy as np

    from src.rtdetr_moe import engine
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.track import TrackArgs, TrackState, copy_state, new_state, states_equal, track_reference

    F, K, n_obj = 16, 300, 40
    args = TrackArgs()
    boxes, scores, labels, n_valid, truth = track_sequence(n_obj, 2 * F, K)
    state = TrackState(1, args.max_tracks, "cuda")
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    zeros = torch.zeros(F, dtype=torch.int32, device="cuda")
    ref = new_state(args.max_tracks)
    ids, switches, events, want = {}, 0, {}, []
    for f in range(2 * F):
        oid, obox, cnt = track_reference(ref, boxes[f], scores[f], labels[f], n_valid[f], args, events)
        want.append((oid, obox, cnt))
        for d in np.nonzero((truth[f] >= 0) & (oid >= 0))[0]:
            seen = ids.setdefault(int(truth[f, d]), [])
            if seen and seen[-1] != oid[d]:
                switches += 1
            if not seen or seen[-1] != oid[d]:
                seen.append(int(oid[d]))
        if f == F - 1:
            warm = copy_state(ref)
    L.track_update(state, dev(boxes[:F]), dev(scores[:F]), dev(labels[:F]), dev(n_valid[:F]), zeros, zeros, args)
    if not states_equal(state.export(0), warm):
        raise SystemExit("track_update's state differs from track_reference's (frames 0..15)")
    snap = state.snapshot()
    db, ds, dl, dn = dev(boxes[F:]), dev(scores[F:]), dev(labels[F:]), dev(n_valid[F:])
    out = tuple(t.cpu().numpy() for t in L.track_update(state, db, ds, dl, dn, zeros, zeros, args))
    for f in range(F):
        oid, obox, cnt = want[F + f]
        if (int(out[2][f]) != cnt or not np.array_equal(out[0][f], oid)
                or not np.array_equal(out[1][f].view(np.int32), obox.view(np.int32))):
            raise SystemExit(f"track_update differs from track_reference (frame {F + f})")
    if not states_equal(state.export(0), ref):
        raise SystemExit("track_update's state differs from track_reference's (frames 16..31)")

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    def kernel():
        state.restore(snap)  # torch copies: not among the library's profiled launches
        return L.track_update(state, db, ds, dl, dn, zeros, zeros, args)

    def device_path():
        oid, obx, _ = kernel()
        torch.cat([db, ds[..., None], dl[..., None].float(), oid.view(torch.float32)[..., None], obx], -1).cpu()

    def host_path():
        packed = torch.cat([db, ds[..., None], dl[..., None].float()], -1).cpu().numpy()
        st = copy_state(warm)
        for f in range(F):
            track_reference(st, packed[f, :, :4], packed[f, :, 4], packed[f, :, 5], n_valid[F + f], args)

    res = {"kernel_us": [], "device_path_ms": [], "host_track_ms": [], "forward_replay_us": []}
    for _ in range(rounds):
        res["kernel_us"].append(timed(kernel, reps))
        res["device_path_ms"].append(wall(device_path, max(3, reps // 5)))
        res["host_track_ms"].append(wall(host_path, 3))
        res["forward_replay_us"].append(replay_us())
    live = int((warm["hits"] > 0).sum())
    line = {"kernel": "rtdetr_track_update", "shape": f"F{F} K{K} T{args.max_tracks} S1 objects{n_obj}",
            "live_tracks": live, "reported": int(out[2].sum()),
            "reference_32_frames": {"objects_tracked": len(ids), "ids_per_object_max": max(len(v) for v in ids.values()),
                                    "switches": switches, "stage2": events["stage2"], "refound": events["refound"],
                                    "tentative_freed": events["tentative_freed"]}}
    for k, v in res.items():
        line[k] = round(statistics.median(v), 3)
        line[k + "_min"] = round(min(v), 3)
        line[k + "_max"] = round(max(v), 3)
    line["host_over_kernel"] = round(1e3 * line["host_track_ms"] / line["kernel_us"], 1)
    line["kernel_share_of_forward"] = round(line["kernel_us"] / line["forward_replay_us"], 4)
    print(json.dumps(line), flush=True)


def track_sweep_leg(reps, rounds):
    """rtdetr_track_sweep at about MOT17's training split (8 sequences of 600
    frames, --track's 300 candidate rows a frame of 40 objects, T 64) with G =
    1, 16 and 64 configurations, one JSON line per G.  First the kernel's
    compact report and states at G 16, all 4800 frames, are checked equal to
    tune.track_sweep_reference's, bit for bit.  sweep_kernel_us: the launches of
    one sweep (tune.launch_chunks: 1024 frames each), dispatch-stamped, summed;
    update_x_g_kernel_us: rtdetr_track_update launched G times over the same
    chunks, one configuration each -- what there was before -- likewise;
    host_reference_ms: tune.track_sweep_reference for ONE configuration, wall
    clock (G of them cost G times that: a loop); forward_replay_us: one
    EvalForward graph replay at batch 16 (rtdetr-r50-moe8-top2, 704 x 1248);
    sweep_wall_ms: tune.sweep(hota=True) on the GPU, wall clock, split into
    tracking (packing the detections, the launches, the copies back), packing
    (the G x 8 dense sequences on the host) and scoring (rtdetr_mot_eval and
    rtdetr_hota_*, their own host packing included).  Median, min and max over
    the rounds."""
    import time

    import numpy as np

    from src.rtdetr_moe import engine, tune
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.track import SweepState, TrackArgs, TrackState, states_equal

    S, F, K, T, n_obj = 8, 600, 300, 64, 40
    grids = {1: {}, 16: {"match_iou": [0.2, 0.3, 0.4, 0.5], "max_age": [5, 15, 30, 60]},
             64: {"match_iou": [0.2, 0.3, 0.4, 0.5], "max_age": [5, 15, 30, 60], "min_hits": [1, 2],
                  "track_high": [0.5, 0.6]}}
    dets, gt = {}, {}
    for q in range(S):
        boxes, scores, labels, _, _ = track_sequence(n_obj, F, K, seed=q)
        key = f"seq{q}"
        dets[key] = {f + 1: (boxes[f], scores[f], labels[f]) for f in range(F)}
        rng = np.random.default_rng(q)  # track_sequence's first draws: the objects' clean boxes
        i = np.arange(n_obj)
        w, h = rng.uniform(30, 50, n_obj), rng.uniform(80, 120, n_obj)
        x0, y0 = 40.0 + (i % 10) * 110.0, 60.0 + (i // 10) * 150.0
        vx, vy = rng.uniform(-0.8, 0.8, n_obj), rng.uniform(-0.3, 0.3, n_obj)
        gt[key] = {f + 1: (np.stack([x0 + vx * f, y0 + vy * f, x0 + vx * f + w, y0 + vy * f + h], 1).astype(np.float32),
                           i + 1, np.ones(n_obj, np.int32)) for f in range(F)}
    seqs, _ = tune.pack_sequences(dets)
    base = TrackArgs(max_tracks=T)
    dev = torch.device("cuda")

    cfg16 = tune.expand_grid(grids[16], base)
    t0 = time.perf_counter()
    want = tune.track_sweep_reference(dets, cfg16, T)
    ref_s = time.perf_counter() - t0
    got = tune.sweep_tracks(dets, cfg16, T, dev)
    for g in range(16):
        for key in dets:
            a, b = got[g][key], want[g][key]
            if not (np.array_equal(a["count"], b["count"]) and np.array_equal(a["ids"], b["ids"])
                    and np.array_equal(a["rows"], b["rows"]) and a["boxes"].tobytes() == b["boxes"].tobytes()
                    and states_equal(a["state"], b["state"])):
                raise SystemExit(f"track_sweep differs from track_sweep_reference (configuration {g}, {key})")
    reported = [int(sum(want[g][k]["count"].sum() for k in dets)) for g in range(16)]

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    for G, grid in grids.items():
        configs = tune.expand_grid(grid, base)
        chunks = []
        for picks in tune.launch_chunks(seqs, G, T):
            cat = lambda key: up(np.concatenate([seqs[j][key][a:b] for j, a, b in picks]))  # noqa: E731
            slot = np.concatenate([np.full(b - a, j, np.int32) for j, a, b in picks])
            reset = np.concatenate([(np.arange(a, b) == 0).astype(np.int32) for j, a, b in picks])
            chunks.append((cat("boxes"), cat("scores"), cat("labels"), cat("n_valid"), up(slot), up(reset)))
        sweep_state, one_state = SweepState(G, S, T, dev), TrackState(S, T, dev)
        outs = [tuple(torch.empty(sh, dtype=dt, device=dev) for sh, dt in
                      (((G, len(c[4]), T), torch.int32), ((G, len(c[4]), T, 4), torch.float32),
                       ((G, len(c[4]), T), torch.int32), ((G, len(c[4])), torch.int32))) for c in chunks]

        def sweep_kernel():
            for c, o in zip(chunks, outs):
                L.track_sweep(sweep_state, *c, configs, out=o)

        def update_x_g():
            for cfg in configs:
                for c in chunks:
                    L.track_update(one_state, *c, cfg)

        def host_one():
            tune.track_sweep_reference(dets, configs[:1], T)

        res = {"sweep_kernel_us": [], "update_x_g_kernel_us": [], "host_reference_ms": [], "forward_replay_us": [],
               "sweep_wall_ms": [], "tracking_ms": [], "packing_ms": [], "scoring_ms": []}
        best = None
        for r in range(rounds):
            res["sweep_kernel_us"].append(timed(sweep_kernel, max(2, reps // 10)))
            res["update_x_g_kernel_us"].append(timed(update_x_g, 1 if G > 1 else max(2, reps // 10)))
            res["forward_replay_us"].append(replay_us())
            if G == 1:
                t0 = time.perf_counter()
                host_one()
                res["host_reference_ms"].append(1e3 * (time.perf_counter() - t0))
            if G < 64 or r < 3:  # the largest sweep's wall clock: three rounds
                tm = {}
                t0 = time.perf_counter()
                out = tune.sweep(dets, gt, configs, hota=True, device=dev, timing=tm)
                res["sweep_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                for k in ("tracking", "packing", "scoring"):
                    res[k + "_ms"].append(1e3 * tm[k])
                best = (out["best"], round(out["metrics"][out["best"]]["COMBINED"]["HOTA"]["HOTA"], 4), tm["launches"])
        line = {"kernel": "rtdetr_track_sweep", "shape": f"S{S} F{F} K{K} T{T} G{G} objects{n_obj}",
                "launches": len(chunks), "workgroups": S * G, "update_launches": G * len(chunks),
                "checked_bit_for_bit_at": "G16, 4800 frames", "reference_g16_s": round(ref_s, 1),
                "reported_rows_g16_min_max": [min(reported), max(reported)],
                "best_config_hota_launches": best, "wall_rounds": len(res["sweep_wall_ms"])}
        for k, v in res.items():
            if v:
                line[k] = round(statistics.median(v), 3)
                line[k + "_min"] = round(min(v), 3)
                line[k + "_max"] = round(max(v), 3)
        line["update_x_g_over_sweep"] = round(line["update_x_g_kernel_us"] / line["sweep_kernel_us"], 2)
        line["sweep_kernel_over_forward"] = round(line["sweep_kernel_us"] / line["forward_replay_us"], 3)
        print(json.dumps(line), flush=True)


def crowd_sequence(n_obj, F, K, seed=0, spacing=18.0, speed=3.0):
    """track_sequence for a crowd: 40 x 100 px pedestrians ``spacing`` px apart
    (closer than their width: neighbours overlap at an IoU of about 0.38) in
    rows 120 px apart, walking at up to ``speed`` px a frame in alternating
    directions, so that neighbours cross; 1.5 px of jitter per side, 10 %
    missed, 20 % scored low, 2 false positives.  -> track_sequence's tuple and
    clean fp32 [F, n_obj, 4], the objects' true boxes (the ground truth)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    per_row = int(1148 // spacing)
    i = np.arange(n_obj)
    x0, y0 = 30.0 + spacing * (i % per_row), 20.0 + 120.0 * (i // per_row)
    vx = np.where(i % 2 == 0, speed, -speed) * rng.uniform(0.6, 1.0, n_obj)
    boxes, scores = np.zeros((F, K, 4), np.float32), np.zeros((F, K), np.float32)
    n_valid, truth = np.zeros(F, np.int32), np.full((F, K), -1, np.int64)
    clean = np.zeros((F, n_obj, 4), np.float32)
    for f in range(F):
        x = x0 + vx * f
        clean[f] = np.stack([x, y0, x + 40.0, y0 + 100.0], 1)
        rows = []
        for o in range(n_obj):
            if f > 0 and rng.random() < 0.1:
                continue
            sc = rng.uniform(0.15, 0.45) if f > 1 and rng.random() < 0.2 else rng.uniform(0.65, 0.95)
            rows.append((sc, clean[f, o].astype(np.float64) + rng.normal(0, 1.5, 4), o))
        for _ in range(2):
            fx, fy = rng.uniform(0, 1188), rng.uniform(0, 574)
            rows.append((rng.uniform(0.1, 0.9), np.array([fx, fy, fx + 40.0, fy + 100.0]), -1))
        rows.sort(key=lambda r: -r[0])
        rows = rows[:K]
        n = len(rows)
        for d, (sc, b, o) in enumerate(rows):
            boxes[f, d], scores[f, d], truth[f, d] = b, sc, o
        fx, fy = rng.uniform(0, 1188, K - n), rng.uniform(0, 574, K - n)
        boxes[f, n:] = np.stack([fx, fy, fx + 40, fy + 100], 1)
        scores[f, n:] = np.sort(rng.uniform(0.001, 0.05, K - n))[::-1]
        n_valid[f] = n
    return boxes, scores, np.zeros((F, K), np.int32), n_valid, truth, clean


def track_lsap_leg(reps, rounds):
    """TrackArgs.assoc: rtdetr_track_update_assoc with assoc = lsap against the
    greedy kernel, one JSON line per shape: --track's (F 16, K 300, 40 objects, T
    64) and a crowd (F 16, K 300, 200 overlapping objects that cross, T 256: the
    solved problems are as large as the crowd).  Per shape and mode the kernel's
    outputs and state over frames 16..31 are first checked equal to
    track.track_reference's, bit for bit (the state before them is the one 16
    earlier frames leave).  kernel_us: dispatch-stamped execution time of one
    launch; host_reference_ms: the reference loop over the 16 frames, wall
    clock; forward_replay_us: one EvalForward graph replay at batch 16
    (rtdetr-r50-moe8-top2, 704 x 1248); solves / solve_n_max / solve_q_max: the
    reference's events over the 16 timed frames.  Median, min and max over the
    rounds, the modes interleaved in each round.  Then the accuracy line: 4
    crowd sequences of 200 frames (60 objects) scored against the objects' clean
    boxes by tune.sweep(hota=True) over {"assoc": ["greedy", "lsap"]} in one
    launch per chunk: HOTA, IDF1, IDSW per mode.  Synthetic numbers only: no
    claim is made beyond them."""
    import time

    import numpy as np

    from src.rtdetr_moe import engine, tune
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.track import TrackArgs, TrackState, copy_state, new_state, states_equal, track_reference

    F, K = 16, 300
    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    zeros = torch.zeros(F, dtype=torch.int32, device="cuda")
    shapes = {"track": (track_sequence(40, 2 * F, K)[:4], 64, 40), "crowd": (crowd_sequence(200, 2 * F, K)[:4], 256, 200)}
    for name, ((boxes, scores, labels, n_valid), T, n_obj) in shapes.items():
        db, ds, dl, dn = dev(boxes[F:]), dev(scores[F:]), dev(labels[F:]), dev(n_valid[F:])
        modes = {}
        for assoc in ("greedy", "lsap"):
            args = TrackArgs(max_tracks=T, assoc=assoc)
            ref, events, want = new_state(T), {}, []
            for f in range(2 * F):
                if f == F:
                    warm, events = copy_state(ref), {}
                want.append(track_reference(ref, boxes[f], scores[f], labels[f], n_valid[f], args, events))
            state = TrackState(1, T, "cuda")
            state.load(0, warm)
            snap = state.snapshot()
            out = tuple(t.cpu().numpy() for t in L.track_update(state, db, ds, dl, dn, zeros, zeros, args))
            for f in range(F):
                oid, obox, cnt = want[F + f]
                if (int(out[2][f]) != cnt or not np.array_equal(out[0][f], oid)
                        or not np.array_equal(out[1][f].view(np.int32), obox.view(np.int32))):
                    raise SystemExit(f"track_update ({assoc}, {name}) differs from track_reference (frame {F + f})")
            if not states_equal(state.export(0), ref):
                raise SystemExit(f"track_update's state ({assoc}, {name}) differs from track_reference's")
            modes[assoc] = dict(args=args, state=state, snap=snap, warm=warm, events=events,
                                live=int((warm["hits"] > 0).sum()), reported=int(out[2].sum()))

        def kernel(m):
            m["state"].restore(m["snap"])
            return L.track_update(m["state"], db, ds, dl, dn, zeros, zeros, m["args"])

        def host(m):
            st = copy_state(m["warm"])
            t0 = time.perf_counter()
            for f in range(F):
                track_reference(st, boxes[F + f], scores[F + f], labels[F + f], n_valid[F + f], m["args"])
            return 1e3 * (time.perf_counter() - t0)

        res = {f"{k}_{a}": [] for k in ("kernel_us", "host_reference_ms") for a in modes}
        res["forward_replay_us"] = []
        for _ in range(rounds):
            for a, m in modes.items():
                res[f"kernel_us_{a}"].append(timed(lambda: kernel(m), reps))
                res[f"host_reference_ms_{a}"].append(host(m))
            res["forward_replay_us"].append(replay_us())
        e = modes["lsap"]["events"]
        line = {"kernel": "rtdetr_track_update_assoc", "shape": f"{name}: F{F} K{K} T{T} S1 objects{n_obj}",
                "live_tracks": modes["lsap"]["live"], "reported_greedy": modes["greedy"]["reported"],
                "reported_lsap": modes["lsap"]["reported"], "solves": e["solves"], "solve_n_max": e["solve_n_max"],
                "solve_q_max": e["solve_q_max"], "checked_bit_for_bit": "both modes, frames 16..31"}
        for k, v in res.items():
            line[k] = round(statistics.median(v), 3)
            line[k + "_min"] = round(min(v), 3)
            line[k + "_max"] = round(max(v), 3)
        line["lsap_over_greedy"] = round(line["kernel_us_lsap"] / line["kernel_us_greedy"], 2)
        line["host_over_kernel_lsap"] = round(1e3 * line["host_reference_ms_lsap"] / line["kernel_us_lsap"], 1)
        line["lsap_share_of_forward"] = round(line["kernel_us_lsap"] / line["forward_replay_us"], 4)
        print(json.dumps(line), flush=True)

    S, FA, n_obj = 4, 200, 60
    dets, gt = {}, {}
    for q in range(S):
        boxes, scores, labels, _, _, clean = crowd_sequence(n_obj, FA, K, seed=100 + q)
        key = f"crowd{q}"
        dets[key] = {f + 1: (boxes[f], scores[f], labels[f]) for f in range(FA)}
        gt[key] = {f + 1: (clean[f], np.arange(n_obj) + 1, np.ones(n_obj, np.int32)) for f in range(FA)}
    tm = {}
    out = tune.sweep(dets, gt, {"assoc": ["greedy", "lsap"]}, base=TrackArgs(max_tracks=128), hota=True,
                     device=torch.device("cuda"), timing=tm)
    line = {"kernel": "rtdetr_track_sweep_assoc", "shape": f"S{S} F{FA} K{K} T128 G2 objects{n_obj} (crowd, synthetic)",
            "launches": tm["launches"], "tracking_ms": round(1e3 * tm["tracking"], 1)}
    for cfg, m in zip(out["configs"], out["metrics"]):
        c = m["COMBINED"]
        line[cfg["assoc"]] = {"HOTA": round(c["HOTA"]["HOTA"], 4), "AssA": round(c["HOTA"]["AssA"], 4),
                              "IDF1": round(c["IDF1"], 4), "MOTA": round(c["MOTA"], 4), "IDSW": int(c["IDSW"])}
    print(json.dumps(line), flush=True)


def frame_shift_leg(reps, rounds):
    """rtdetr_frame_shift at predict's shape (F 16 frames of one sequence, 704 x
    1248, the defaults of track.TrackArgs: radius 48, gate 0.1) against
    motion.sequence_shifts on the host, same process, same frames (shifts, SADs
    and state checked equal first).  The frames are views of a scene of 8 x 8
    blocks plus noise, panning by up to 45 px a frame; the checked launch starts
    from the state 16 earlier frames leave, a timed one from the state the
    batch itself left (its first frame then measures against its last, the
    other 15 as checked).  kernel_us: the three
    launches' dispatch-stamped execution time per batch, and each launch's
    (grey, coarse, fine); host_ms: sequence_shifts on the 16 frames already on
    the host (the copy back of the model's input is not in it), wall clock.
    forward_replay_us: one EvalForward graph replay at batch 16
    (rtdetr-r50-moe8-top2, 704 x 1248).  Median, min and max over the rounds,
    the sides interleaved in each round."""
    import time

    import numpy as np

    from src.rtdetr_moe import engine, motion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.track import TrackArgs

    F, h, w, m = 16, 704, 1248, 64
    args = TrackArgs()
    rng = np.random.default_rng(0)
    small = rng.random(((h + 2 * m) // 8 + 1, (w + 2 * m) // 8 + 1, 3)).astype(np.float32)
    scene = np.repeat(np.repeat(small, 8, 0), 8, 1)
    steps = rng.integers(-45, 46, (2 * F, 2))
    steps[::5] = 0
    pos = np.clip(np.cumsum(steps, 0), -m, m)  # the views stay inside the scene
    frames = np.stack([scene[m - y:m - y + h, m - x:m - x + w] + rng.normal(0, 0.02, (h, w, 3)).astype(np.float32)
                       for x, y in pos]).astype(np.float32)
    gate = round(1000 * args.cmc_gate)
    ref = motion.new_motion_state(1, h, w)
    zeros = np.zeros(F, np.int32)
    motion.sequence_shifts(frames[:F], zeros, zeros, ref, args.cmc_radius, gate, args.cmc_rows)
    warm = {k: v.copy() for k, v in ref.items()}
    want = motion.sequence_shifts(frames[F:], zeros, zeros, ref, args.cmc_radius, gate, args.cmc_rows)
    true = np.diff(pos, axis=0)[F - 1:]
    state = motion.MotionState(1, h, w, "cuda", frames=F)
    up = lambda a: torch.from_numpy(a).cuda().permute(0, 3, 1, 2)  # noqa: E731
    tab = torch.zeros(F, dtype=torch.int32, device="cuda")
    x = up(frames[F:])
    L.frame_shift(state, up(frames[:F]), (h, w), tab, tab, args.cmc_radius, args.cmc_gate, args.cmc_rows)
    got = L.frame_shift(state, x, (h, w), tab, tab, args.cmc_radius, args.cmc_gate, args.cmc_rows)
    exp = state.export()
    if not (np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
            and np.array_equal(exp["grey"], ref["grey"]) and np.array_equal(exp["valid"], ref["valid"])):
        raise SystemExit("frame_shift differs from sequence_shifts")
    def kernel():  # the state after it is the same every time: the slot's image is the batch's last frame
        return L.frame_shift(state, x, (h, w), tab, tab, args.cmc_radius, args.cmc_gate, args.cmc_rows)

    def parts(n):
        kernel()
        torch.cuda.synchronize()
        L.lib().moe_profile_enable(1)
        try:
            for _ in range(n):
                kernel()
            ms = [r[1] for r in L.profile_records()]
        finally:
            L.lib().moe_profile_enable(0)
        return [1e3 * statistics.median(ms[i::3]) for i in range(3)]

    def host_ms():
        st = {k: v.copy() for k, v in warm.items()}
        t0 = time.perf_counter()
        motion.sequence_shifts(frames[F:], zeros, zeros, st, args.cmc_radius, gate, args.cmc_rows)
        return 1e3 * (time.perf_counter() - t0)

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    xin = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(xin, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(xin, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    res = {"kernel_us": [], "grey_us": [], "coarse_us": [], "fine_us": [], "host_ms": [], "forward_replay_us": []}
    for _ in range(rounds):
        res["kernel_us"].append(timed(kernel, reps))
        for k, v in zip(("grey_us", "coarse_us", "fine_us"), parts(reps)):
            res[k].append(v)
        res["host_ms"].append(host_ms())
        res["forward_replay_us"].append(replay_us())
    line = {"kernel": "rtdetr_frame_shift", "shape": f"F{F} {h}x{w} S1 radius{args.cmc_radius} gate{gate}",
            "status": want[1][:, 0].tolist(), "shifts_found": int((want[0] == true).all(1).sum())}
    for k, v in res.items():
        line[k] = round(statistics.median(v), 3)
        line[k + "_min"] = round(min(v), 3)
        line[k + "_max"] = round(max(v), 3)
    line["host_over_kernel"] = round(1e3 * line["host_ms"] / line["kernel_us"], 1)
    line["kernel_share_of_forward"] = round(line["kernel_us"] / line["forward_replay_us"], 4)
    print(json.dumps(line), flush=True)


def mot_sequence(seed, F, n_gt, n_trk):
    """A sequence for the tracking evaluator with dense indices: n_gt
    constant-velocity pedestrians, every one a ground-truth row in every frame;
    tracker index t < n_gt follows one of them with 2 px of jitter per side
    (every 40 frames or so two tracker indices swap their objects: identity
    switches), the other n_trk - n_gt rows are random false positives.  -> the
    frames as moteval.mot_reference takes them."""
    import numpy as np

    rng = np.random.default_rng(seed)
    i = np.arange(n_gt)
    wh = np.stack([rng.uniform(30, 50, n_gt), rng.uniform(80, 120, n_gt)], 1)
    xy0 = np.stack([40.0 + (i % 10) * 110.0, 60.0 + (i // 10) * 150.0], 1)
    v = np.stack([rng.uniform(-0.8, 0.8, n_gt), rng.uniform(-0.3, 0.3, n_gt)], 1)
    follows = np.arange(n_gt)
    gi, ti, flags = np.arange(n_gt, dtype=np.int32), np.arange(n_trk, dtype=np.int32), np.ones(n_gt, np.int32)
    frames = []
    for f in range(F):
        if rng.random() < 1 / 40:
            a, b = rng.choice(n_gt, 2, replace=False)
            follows[a], follows[b] = follows[b], follows[a]
        xy = xy0 + v * f
        gb = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        fx, fy = rng.uniform(0, 1188, n_trk - n_gt), rng.uniform(0, 574, n_trk - n_gt)
        tb = np.concatenate([gb[follows] + rng.normal(0, 2.0, (n_gt, 4)), np.stack([fx, fy, fx + 40, fy + 100], 1)])
        frames.append((gb, gi, flags, tb.astype(np.float32), ti))
    return frames


def pan_frames():
    """The synthetic pedestrians of --track seen through the camera pan of
    --frame-shift (every box of frame f moved by the pan's position; the
    tracker's shift is the pan's step), tracked by track.track_reference with
    cmc off and on -> {"cmc_off" / "cmc_on": [(truth boxes fp32, g, flags,
    tracker boxes, t)]}, the evaluators' frames (NG 40, NT up to 4096)."""
    import numpy as np

    from src.rtdetr_moe.track import TrackArgs, new_state, track_reference

    Fp, Kp, n_obj = 32, 300, 40
    boxes, scores, labels, n_valid, _ = track_sequence(n_obj, Fp, Kp)
    rng = np.random.default_rng(0)  # track_sequence's first draws: the objects' clean boxes
    i = np.arange(n_obj)
    w, h = rng.uniform(30, 50, n_obj), rng.uniform(80, 120, n_obj)
    x0, y0 = 40.0 + (i % 10) * 110.0, 60.0 + (i // 10) * 150.0
    vx, vy = rng.uniform(-0.8, 0.8, n_obj), rng.uniform(-0.3, 0.3, n_obj)
    steps = np.random.default_rng(0).integers(-45, 46, (Fp, 2))
    steps[::5] = 0
    pos = np.clip(np.cumsum(steps, 0), -64, 64).astype(np.float32)
    shift = np.diff(pos, axis=0, prepend=pos[:1])
    out = {}
    for cmc in (False, True):
        st, frames = new_state(TrackArgs().max_tracks), []
        for f in range(Fp):
            move = np.tile(pos[f], 2)
            oid, obox, _ = track_reference(st, boxes[f] + move, scores[f], labels[f], n_valid[f], TrackArgs(),
                                           shift=shift[f] if cmc else None)
            rows = np.nonzero(oid >= 0)[0]
            truth = np.stack([x0 + vx * f, y0 + vy * f, x0 + vx * f + w, y0 + vy * f + h], 1) + move
            frames.append((truth.astype(np.float32), i, np.ones(n_obj, np.int32), obox[rows], oid[rows] - 1))
        out["cmc_on" if cmc else "cmc_off"] = frames
    return out


def mot_eval_leg(reps, rounds):
    """rtdetr_mot_eval at about MOT17's training split (8 sequences of 600
    frames, 30 truths and 35 tracker rows a frame) against moteval.mot_reference
    on the host, same process, same rows (every state array checked equal
    first, bit for bit).  The 4800 frames are 5 launches (moteval.pack_chunks:
    128 frames of each sequence a launch, one 64-lane workgroup per sequence --
    the kernel is latency bound by construction: the frames of a sequence are
    serial).  kernel_us: the 5 launches' dispatch-stamped execution time;
    device_path_ms: new state, the launches, the state copied back and
    mot_metrics, wall clock, the rows already on the device; host_ms: the
    reference loop over the 4800 frames and mot_metrics, wall clock.
    forward_replay_us: one EvalForward graph replay at batch 16
    (rtdetr-r50-moe8-top2, 704 x 1248).  Median, min and max over the rounds,
    the sides interleaved in each round.
    Also, on the synthetic pedestrians of --track seen through the camera pan of
    --frame-shift (every box of frame f moved by the pan's position; the
    tracker's shift is the pan's step, which --frame-shift checks the estimator
    finds): MOTA, IDF1 and IDSW of track.track_reference's output against the
    clean boxes, with cmc off and on.  Synthetic input: no accuracy claim beyond
    it."""
    import time

    from src.rtdetr_moe import engine, moteval
    from src.rtdetr_moe.model import RTDETRMoE

    S, F, n_gt, n_trk, thr = 8, 600, 30, 35, 0.5
    seqs = [{"NG": n_gt, "NT": n_trk, "frames": mot_sequence(s, F, n_gt, n_trk)} for s in range(S)]
    chunks, M, K = moteval.pack_chunks(seqs)
    dev_chunks = [{k: torch.from_numpy(v).cuda() for k, v in c.items()} for c in chunks]
    order = ("gt_boxes", "gt_idx", "gt_flag", "n_gt", "trk_boxes", "trk_idx", "n_trk", "frame_slot", "frame_reset")
    made = []

    def kernel():
        st = moteval.MotEvalState(S, n_gt, n_trk, "cuda")  # torch fills: not among the library's profiled launches
        for c in dev_chunks:
            L.mot_eval(st, *(c[k] for k in order), thr)
        made[:] = [st]

    def device_path():
        kernel()
        L.mot_eval_check(made[0])
        return [moteval.mot_metrics(made[0].export(s)) for s in range(S)]

    def host_path():
        return [moteval.mot_metrics(st) for st in moteval.run_reference(seqs, thr)]

    want = moteval.run_reference(seqs, thr)
    kernel()
    L.mot_eval_check(made[0])
    for s in range(S):
        if not moteval.states_equal(made[0].export(s), want[s]):
            raise SystemExit(f"mot_eval's state differs from mot_reference's (sequence {s})")
    combined = moteval.combine(device_path())

    pan = {}
    for cmc, frames in pan_frames().items():
        ev = moteval.new_state(40, 4096)
        for truth, i, flags, obox, oid in frames:
            moteval.mot_reference(ev, (truth, i, flags), (obox, oid), thr)
        m = moteval.mot_metrics(ev)
        pan[cmc] = {"MOTA": round(m["MOTA"], 4), "IDF1": round(m["IDF1"], 4),
                    "IDSW": m["IDSW"], "FN": m["FN"], "FP": m["FP"]}

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    def wall(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    res = {"kernel_us": [], "device_path_ms": [], "host_ms": [], "forward_replay_us": []}
    for _ in range(rounds):
        res["kernel_us"].append(timed(kernel, max(3, reps // 10)))
        res["device_path_ms"].append(wall(device_path, 3))
        res["host_ms"].append(wall(host_path, 1))
        res["forward_replay_us"].append(replay_us())
    line = {"kernel": "rtdetr_mot_eval", "shape": f"S{S} F{F} M{M} K{K} NG{n_gt} NT{n_trk}", "launches": len(chunks),
            "combined": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in combined.items()
                         if k in ("MOTA", "MOTP", "IDF1", "IDSW", "TP", "FN", "FP", "Frag")},
            "pan_32_frames": pan}
    for k, v in res.items():
        line[k] = round(statistics.median(v), 3)
        line[k + "_min"] = round(min(v), 3)
        line[k + "_max"] = round(max(v), 3)
    line["host_over_kernel"] = round(1e3 * line["host_ms"] / line["kernel_us"], 1)
    line["host_over_device_path"] = round(line["host_ms"] / line["device_path_ms"], 1)
    line["kernel_over_forward"] = round(line["kernel_us"] / line["forward_replay_us"], 3)
    print(json.dumps(line), flush=True)


def hota_leg(reps, rounds):
    """The frame-parallel HOTA kernels (rtdetr_hota_pass_a / _gas / _pass_b) at
    --mot-eval's shape (8 sequences of 600 frames, 30 truths and 35 tracker rows
    a frame) against hota.hota_reference on the host, same process, same rows:
    every state array, gas and the loc partials checked equal first, bit for
    bit.  The 4800 frames are one launch of 4800 workgroups per pass
    (moteval.pack_chunks at hota.HOTA_MAX_F), against rtdetr_mot_eval's 5
    launches of 8.  hota_kernels_us: pass A, gas and pass B, dispatch-stamped,
    the rows on the device; mot_eval_kernel_us: rtdetr_mot_eval's 5 launches,
    likewise; device_path_ms: hota.run_device_hota (pack, upload, new state, the
    launches, the state and the partials copied back, the reduction in frame
    order) and hota_metrics, wall clock; host_ms: hota.run_reference_hota and
    hota_metrics, wall clock; forward_replay_us: one EvalForward graph replay at
    batch 16.  Median, min and max over the rounds, the sides interleaved in
    each round.  Also HOTA / DetA / AssA of the synthetic pan (pan_frames) with
    cmc off and on: synthetic input, no accuracy claim beyond it."""
    import time

    from src.rtdetr_moe import engine, hota, moteval
    from src.rtdetr_moe.model import RTDETRMoE

    S, F, n_gt, n_trk, thr = 8, 600, 30, 35, 0.5
    seqs = [{"NG": n_gt, "NT": n_trk, "frames": mot_sequence(s, F, n_gt, n_trk)} for s in range(S)]
    chunks, M, K = moteval.pack_chunks(seqs, hota.HOTA_MAX_F)
    dev_chunks = [{k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "frame_reset"} for c in chunks]
    keeps = [torch.empty(c["trk_idx"].shape, dtype=torch.uint8, device="cuda") for c in dev_chunks]
    mot_chunks = [{k: torch.from_numpy(v).cuda() for k, v in c.items()} for c in moteval.pack_chunks(seqs)[0]]
    order = ("gt_boxes", "gt_idx", "gt_flag", "n_gt", "trk_boxes", "trk_idx", "n_trk", "frame_slot", "frame_reset")

    def kernels():
        st = hota.HotaEvalState(S, n_gt, n_trk, "cuda")  # torch fills: not among the library's profiled launches
        for c, keep in zip(dev_chunks, keeps):
            L.hota_pass_a(st, c, keep, thr)
        L.hota_gas(st)
        for c, keep in zip(dev_chunks, keeps):
            L.hota_pass_b(st, c, keep)

    def mot_kernel():
        st = moteval.MotEvalState(S, n_gt, n_trk, "cuda")
        for c in mot_chunks:
            L.mot_eval(st, *(c[k] for k in order), thr)

    def device_path():
        return [hota.hota_metrics(st) for st in hota.run_device_hota(seqs, thr, torch.device("cuda"))]

    def host_path():
        return [hota.hota_metrics(st) for st in hota.run_reference_hota(seqs, thr)]

    want = hota.run_reference_hota(seqs, thr)
    for s, (got, ref) in enumerate(zip(hota.run_device_hota(seqs, thr, torch.device("cuda")), want)):
        if not hota.hota_states_equal(got, ref) or got["gas"].tobytes() != ref["gas"].tobytes() or \
                got["loc_part"].tobytes() != ref["loc_part"].tobytes():
            raise SystemExit(f"the HOTA kernels' state differs from hota_reference's (sequence {s})")
    combined = hota.combine_hota(device_path())
    if combined != hota.combine_hota([hota.hota_metrics(st) for st in want]):
        raise SystemExit("the device path's combined HOTA differs from the host's")
    pan = {}
    for cmc, frames in pan_frames().items():
        m = hota.hota_metrics(hota.hota_reference(frames, 40, 4096, thr))
        pan[cmc] = {k: round(m[k], 4) for k in ("HOTA", "DetA", "AssA", "LocA")}

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last).eval()
    fwd = engine.EvalForward(model)
    x = torch.rand((16, 3, 704, 1248), device="cuda").contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(16, dtype=torch.int32, device="cuda")
    fwd.prepare(x, ctx)

    def replay_us(n=10):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd(x, ctx)
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts)

    def wall(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    res = {"hota_kernels_us": [], "mot_eval_kernel_us": [], "device_path_ms": [], "host_ms": [],
           "forward_replay_us": []}
    for _ in range(rounds):
        res["hota_kernels_us"].append(timed(kernels, max(3, reps // 10)))
        res["mot_eval_kernel_us"].append(timed(mot_kernel, max(3, reps // 10)))
        res["device_path_ms"].append(wall(device_path, 3))
        res["host_ms"].append(wall(host_path, 1))
        res["forward_replay_us"].append(replay_us())
    line = {"kernel": "rtdetr_hota", "shape": f"S{S} F{F} M{M} K{K} NG{n_gt} NT{n_trk}",
            "launches": 2 * len(chunks) + 1, "workgroups_per_pass": S * F, "mot_eval_launches": len(mot_chunks),
            "combined": {k: round(combined[k], 4) for k in ("HOTA", "DetA", "AssA", "LocA")}, "pan_32_frames": pan}
    for k, v in res.items():
        line[k] = round(statistics.median(v), 3)
        line[k + "_min"] = round(min(v), 3)
        line[k + "_max"] = round(max(v), 3)
    line["mot_eval_over_hota_kernels"] = round(line["mot_eval_kernel_us"] / line["hota_kernels_us"], 2)
    line["host_over_device_path"] = round(line["host_ms"] / line["device_path_ms"], 1)
    line["hota_kernels_over_forward"] = round(line["hota_kernels_us"] / line["forward_replay_us"], 3)
    print(json.dumps(line), flush=True)


def grad_accum_leg(reps, rounds):
    """train_grad_accum over C2's parameter list (rtdetr-r50-moe8-top2, GEMM /
    convolution operands in bf16 as in the training step): us per launch
    (dispatch-stamped kernel time) and GB/s of the bytes it must move -- the
    gradient read, the accumulator written, and in add mode the accumulator
    read -- in ``first`` and add mode, interleaved in each round.  With --cold
    every launch starts from HBM, as after a step's forward and backward."""
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.optim import GradAccumulator
    from src.rtdetr_moe.step import gemm_params

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r50-moe8-top2").cuda().to(memory_format=torch.channels_last)
    for p in gemm_params(model):
        p.data = p.data.to(torch.bfloat16)
    params = [p for p in model.parameters() if p.requires_grad]
    grads = [torch.randn_like(p) for p in params]
    acc = GradAccumulator(params)
    n = sum(p.numel() for p in params)
    gbytes = sum(g.numel() * g.element_size() for g in grads)
    byts = {"first": gbytes + 4 * n, "add": gbytes + 8 * n}

    def launch(first):
        acc.count = 0 if first else 1
        acc.add(grads)

    res = {"first": [], "add": []}
    for _ in range(rounds):
        for mode in res:
            res[mode].append(timed(lambda: launch(mode == "first"), reps))
    for mode, v in res.items():
        us = statistics.median(v)
        print(json.dumps({"kernel": "train_grad_accum", "mode": mode, "shape": f"C2 {len(params)} tensors {n} elements "
                          f"{acc.n_chunks} chunks", "cold": _FLUSH is not None, "us": round(us, 2),
                          "us_min": round(min(v), 2), "us_max": round(max(v), 2), "MB": round(byts[mode] / 1e6, 1),
                          "GBs": round(byts[mode] / us / 1e3, 1),
                          "hbm_peak_share": round(byts[mode] / us / 1e3 / L.PEAK_HBM_GBS, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grad-accum", action="store_true",
                    help="time the gradient-accumulation kernel over C2's parameter list (first / add mode) and exit")
    ap.add_argument("--augment", action="store_true", help="time the batch-augmentation kernels (C2's batch) and exit")
    ap.add_argument("--eval-match", action="store_true",
                    help="time the validation matcher (B 16, K 300, M 20 / 64) against the host loop and exit")
    ap.add_argument("--eval-match-bands", action="store_true",
                    help="time the size-stratified matcher (B 16, K 300, M 20 / 64, R 3) against the plain matcher "
                         "and the host loop and exit")
    ap.add_argument("--route-stats", action="store_true",
                    help="time moe_route_stats (C2's eval shapes, batch 16) against its torch reference and exit")
    ap.add_argument("--balance", action="store_true",
                    help="check the biased router and moe_balance_step against their CPU statements, time the router "
                         "with and without a selection bias and the balance launch, run the update rule for "
                         "--balance-steps steps on a frozen synthetic router, and exit")
    ap.add_argument("--balance-steps", type=int, default=3000)
    ap.add_argument("--resize", action="store_true",
                    help="time rtdetr_resize_pad_u8 (16 ZOD-sized frames, and identity scale) against the host "
                         "resize it replaces and exit")
    ap.add_argument("--nms-merge", action="store_true",
                    help="time rtdetr_nms_merge (B 16, N 1500, max_det 300) against merge.merge_reference on the host "
                         "and one EvalForward replay, and exit")
    ap.add_argument("--resize-flip", action="store_true",
                    help="check rtdetr_resize_pad_u8_flip against rtdetr_resize_pad_u8 on host-mirrored frames, time "
                         "it with all flags 0 and all flags 1 against the old entry (--resize's shape), and exit")
    ap.add_argument("--box-fuse", action="store_true",
                    help="time rtdetr_box_fuse (B 16, 5 passes of 300, max_det 300) against rtdetr_nms_merge on the "
                         "same inputs and one EvalForward replay, after checking it against merge.fuse_reference")
    ap.add_argument("--track", action="store_true",
                    help="time rtdetr_track_update (16 frames of one sequence, K 300, about 40 live tracks) against "
                         "track_reference on the host and one forward replay, and exit")
    ap.add_argument("--track-sweep", action="store_true",
                    help="check rtdetr_track_sweep against tune.track_sweep_reference (8 sequences of 600 frames, K "
                         "300), time it at G 1 / 16 / 64 against rtdetr_track_update launched G times, the host "
                         "reference and one forward replay, time tune.sweep's stages, and exit")
    ap.add_argument("--track-lsap", action="store_true",
                    help="check rtdetr_track_update_assoc (assoc = lsap) against track_reference, time it against the "
                         "greedy kernel at --track's shape and at a crowd shape, the host reference and one forward "
                         "replay, print HOTA / IDF1 / IDSW of both modes on synthetic crowds, and exit")
    ap.add_argument("--frame-shift", action="store_true",
                    help="check rtdetr_frame_shift against motion.sequence_shifts, then time it against the host and "
                         "a forward replay, and exit")
    ap.add_argument("--mot-eval", action="store_true",
                    help="check rtdetr_mot_eval against moteval.mot_reference (8 sequences of 600 frames), time it "
                         "against the host reference and a forward replay, print MOTA / IDF1 / IDSW on the synthetic "
                         "pan with cmc off and on, and exit")
    ap.add_argument("--hota", action="store_true",
                    help="check the frame-parallel HOTA kernels against hota.hota_reference at --mot-eval's shape, "
                         "time them against the host reference, rtdetr_mot_eval and a forward replay, print HOTA / "
                         "DetA / AssA on the synthetic pan with cmc off and on, and exit")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="0")
    ap.add_argument("--stages", default="0")
    ap.add_argument("--only", default="")
    ap.add_argument("--tune", action="append", default=[], help="key=value for moe_set_tuning (repeatable)")
    ap.add_argument("--config", choices=["c2", "c5"], default="c2", help="layer shapes (C2: E8 k2 bs8; C5: E32 k4 bs16)")
    ap.add_argument("--debug", default="0", help="comma list of gemm_debug modes (1 no C stores, 2 no main loop)")
    ap.add_argument("--bm", default="0", help="comma list of forced row-tile heights (0 = auto) for rows and wgrad")
    ap.add_argument("--xcd", default="0", help="comma list of ROWS tile->XCD maps (0 auto, 1 round-robin, 2 contiguous)")
    ap.add_argument("--ksplit", default="0", help="comma list of split-K factors (0 auto, 1 off, 2..8 forced)")
    ap.add_argument("--pair", default="1", help="comma list of gemm_pair modes (1 one launch, 0 two launches)")
    ap.add_argument("--wg", default="0:0", help="comma list of gathered-wgrad bodies dma:stages (dma 0 auto / 1 "
                                                "register-staged; stages 0 auto, 2, 3)")
    ap.add_argument("--skew", type=float, default=0.0, help="expert preference added to the context bias")
    ap.add_argument("--cold", action="store_true", help="flush the Infinity Cache (512 MiB read) before every call")
    ap.add_argument("--sweep", action="append", default=[],
                    help="key=v1,v2,... moe_set_tuning values interleaved per round (one knob; repeat the flag "
                         "for a cross product)")
    a = ap.parse_args()
    SKEW[0] = a.skew
    L.lib()
    if a.augment:
        augment_leg(a.reps, a.rounds)
        return
    if a.eval_match:
        eval_match_leg(a.reps, a.rounds)
        return
    if a.eval_match_bands:
        eval_match_bands_leg(a.reps, a.rounds)
        return
    if a.route_stats:
        route_stats_leg(a.reps, a.rounds)
        return
    if a.resize_flip:
        resize_flip_leg(a.reps, a.rounds)
        return
    if a.resize:
        resize_leg(a.reps, a.rounds)
        return
    if a.nms_merge:
        nms_merge_leg(a.reps, a.rounds)
        return
    if a.track:
        track_leg(a.reps, a.rounds)
        return
    if a.track_sweep:
        track_sweep_leg(a.reps, a.rounds)
        return
    if a.track_lsap:
        track_lsap_leg(a.reps, a.rounds)
        return
    if a.box_fuse:
        box_fuse_leg(a.reps, a.rounds)
        return
    if a.frame_shift:
        frame_shift_leg(a.reps, a.rounds)
        return
    if a.mot_eval:
        mot_eval_leg(a.reps, a.rounds)
        return
    if a.hota:
        hota_leg(a.reps, a.rounds)
        return
    if a.cold:
        global _FLUSH
        _FLUSH = torch.zeros(128 << 20, device="cuda", dtype=torch.float32)
    if a.grad_accum:
        grad_accum_leg(a.reps, a.rounds)
        return
    if a.balance:
        balance_leg(a.reps, a.rounds, a.balance_steps)
        return
    for kv in a.tune:
        key, val = kv.split("=", 1)
        L.set_tuning(key, int(val))
    configs = [(v, s, dbg, bm, xm, ks, pr, wg) for v in map(int, a.variants.split(",")) for s in map(int, a.stages.split(","))
               for dbg in map(int, a.debug.split(",")) for bm in map(int, a.bm.split(","))
               for xm in map(int, a.xcd.split(",")) for ks in map(int, a.ksplit.split(","))
               for pr in map(int, a.pair.split(",")) for wg in a.wg.split(",")
               if not (v == 1 and s != int(a.stages.split(",")[0]))]
    if a.config == "c5":  # 32 experts, top-4, bs 16 (no capacity drops here: cf only trims the tail)
        shapes = {"enc": setup(16 * 920, 32, 4, 256, 1024), "dec": setup(16 * 300, 32, 4, 256, 1024, seed=1)}
    else:
        shapes = {"enc": setup(8 * 920, 8, 2, 256, 1024), "dec": setup(8 * 300, 8, 2, 256, 1024, seed=1)}
    sweeps = [[]]
    for sw in a.sweep:
        key, vals = sw.split("=", 1)
        sweeps = [prev + [(key, int(v))] for prev in sweeps for v in vals.split(",")]
    res = {}
    for _ in range(a.rounds):
      for swv in sweeps:
        for key, val in swv:
            L.set_tuning(key, val)
        tag = ",".join(f"{k}={v}" for k, v in swv)
        for (v, s, dbg, bm, xm, ks, pr, wg) in configs:
            wd, ws = (int(u) for u in wg.split(":"))
            L.set_tuning("wgrad_dma", wd)
            L.set_tuning("wgrad_stages", ws)
            L.set_tuning("gemm_pair", pr)
            L.set_tuning("ksplit", ks)
            L.set_tuning("xcd_map", xm)
            L.set_tuning("rows_bm", bm)
            L.set_tuning("wgrad_bm", bm)
            L.set_tuning("gemm_variant", v)
            L.set_tuning("gemm_stages", s)
            L.set_tuning("gemm_debug", dbg)
            for sname, c in shapes.items():
                for name, fn, flops, byts in kernels(c):
                    if a.only and a.only not in name:
                        continue
                    if not name.startswith("gemm") and (v, s, dbg, bm, xm, ks, pr, wg) != configs[0]:
                        continue
                    if pr != 1 and "pair" not in name:
                        continue
                    res.setdefault((name, sname, v, s, dbg, bm, xm, ks, pr, wg, flops, byts, tag), []).append(
                        timed(fn, a.reps))
        for key, _ in swv:
            L.set_tuning(key, 0)
    L.set_tuning("ksplit", 0)
    L.set_tuning("gemm_pair", 1)
    L.set_tuning("gemm_debug", 0)
    L.set_tuning("rows_bm", 0)
    L.set_tuning("wgrad_bm", 0)
    L.set_tuning("xcd_map", 0)
    L.set_tuning("wgrad_dma", 0)
    L.set_tuning("wgrad_stages", 0)
    for (name, sname, v, s, dbg, bm, xm, ks, pr, wg, flops, byts, tag), ts in res.items():
        us = statistics.median(ts)
        d = {"kernel": name, "config": a.config, "shape": sname, "sweep": tag, "variant": v, "stages": s, "debug": dbg,
             "bm": bm,
             "xcd": xm, "ksplit": ks, "pair": pr, "wg": wg, "skew": a.skew, "cold": a.cold, "us": round(us, 2),
             "min_us": round(min(ts), 2)}
        if flops:
            d["tflops"] = round(flops / us / 1e6, 1)
            d["frac_bf16_peak"] = round(flops / us / 1e6 / 2500.0, 4)
        if byts:
            d["gbs"] = round(byts / us / 1e3, 1)
            d["frac_hbm_peak"] = round(byts / us / 1e3 / 8000.0, 4)
        print(json.dumps(d))


if __name__ == "__main__":
    main()
