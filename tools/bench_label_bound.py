#!/usr/bin/env python3
"""Times the two launches of the label bound (DenoisingModel.label_bound: ccdm_bound_noise + ccdm_bound_terms) against the shipped
unfused training-time chain on the same x0, and both against the network pass they sit behind, at two shapes of 64 engine rows:

    lidc         K = 2, 128x128, one image channel        (all 250 levels of one LIDC label are four such passes)
    cityscapes   K = 20, 128x256, three image channels    (the LIDC-width network at the Cityscapes shape: the real Cityscapes network
                                                           is wider, so the bound's share of a pass there is smaller than printed)

    fused    ccdm_bound_noise (labels -> x_t) + ccdm_bound_terms (x0 [N,HW,K], x_t uint8 -> per-row float64 sums), `fused_terms` alone too
    chain    from the same x0 and the same x_t: the BCHW copy of x0 (permute + contiguous), one_hot(x_t) and one_hot(y) in fp32,
             DiffusionModel.theta_post, theta_post_prob, kl_clamped, the sum over classes and the sum over pixels — without the draw
             of x_t (q_xt_given_x0 and a categorical sample on top), so the chain's side is the smaller of the two it could be
    network  one engine pass to x0 (STEP_SOFTMAX_ONLY) with per-row timesteps, eager launches

Protocol: every variant is warmed up; inside each of `--reps` (>= 3) repetitions the variants run one after the other, each for a
window of back-to-back iterations long enough for `--window` seconds (default 0.5) between two device events; median and spread
(min, max) over the repetitions.  Both paths' per-row sums are compared first (absolutely, per pixel: both round in fp32).  Next to the times: the bytes each variant must move,
from the shapes (fused 4 K + 4 per pixel and row; the chain 56 K + 18 at its least).  Prints one JSON line per shape.

    python tools/bench_label_bound.py [--reps 3] [--window 0.5] [--shapes lidc,cityscapes] [--no-network]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict  # noqa: E402
from ccdm_stochastic_segmentation_amd.models import bound_rows  # noqa: E402

SHAPES = {"lidc": dict(K=2, H=128, W=128, C=1), "cityscapes": dict(K=20, H=128, W=256, C=3)}
ROWS, T, LABELS = 64, 250, 4


def window(fn, seconds, dev):
    """us per iteration over a window of back-to-back iterations that lasts about `seconds`, between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    e1.synchronize()
    iters = max(5, int(np.ceil(seconds / max(e0.elapsed_time(e1) / 5 * 1e-3, 1e-7))))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, iters


def bench_shape(name, cfg, reps, seconds, with_network, dev):
    K, H, W, Cimg = cfg["K"], cfg["H"], cfg["W"], cfg["C"]
    HW, N = H * W, ROWS
    bp = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
    model = build_model(T, "cosine", {"s": 0.008}, [(Cimg, H, W), (K, H, W)], (Cimg, H, W), "unet_openai", bp, "datasets.lidc", "confidence", None)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}, strict=True)
    model = model.to(dev).eval()
    dm = model.diffusion
    lib = hip.load()
    rng = np.random.default_rng(0)
    labels = torch.from_numpy(rng.integers(0, K, (LABELS, HW)).astype(np.uint8)).to(dev)
    ts = np.linspace(1, T, N // LABELS).round().astype(np.int64)[None].repeat(LABELS, 0)              # 16 levels of each of 4 labels
    table_np, slot = bound_rows(ts, 1, N, K, [float(v) for v in dm.cumalphas.double()], dm.posterior_coeffs, LABELS)[0]
    table = torch.from_numpy(table_np.view(np.int32).reshape(N, 8)).to(dev)
    t_rows = torch.from_numpy(table_np["t"].astype(np.int64)).to(dev)
    label_rows = torch.from_numpy(table_np["label_row"].astype(np.int64)).to(dev)
    x0 = torch.softmax(torch.from_numpy(rng.normal(0, 2, (N, HW, K)).astype(np.float32)).to(dev), dim=-1).contiguous()
    xt = torch.zeros((N, HW), dtype=torch.uint8, device=dev)
    ws = torch.zeros((lib.ccdm_bound_terms_workspace_bytes(N, HW, K) // 8,), dtype=torch.float64, device=dev)
    row_sum, row_weight = (torch.zeros((N,), dtype=torch.float64, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def noise():
        hip.check(lib.ccdm_bound_noise(labels.data_ptr(), table.data_ptr(), N, LABELS, HW, K, 1, xt.data_ptr(), stream), "bound_noise")

    def terms():
        hip.check(lib.ccdm_bound_terms(x0.data_ptr(), xt.data_ptr(), labels.data_ptr(), table.data_ptr(), None, N, LABELS, HW, K, 1e-12,
                                       ws.data_ptr(), row_sum.data_ptr(), row_weight.data_ptr(), None, stream), "bound_terms")

    def fused():
        noise()
        terms()

    def chain():
        theta = x0.reshape(N, H, W, K).permute(0, 3, 1, 2).contiguous()
        xt_oh = torch.nn.functional.one_hot(xt.long(), K).reshape(N, H, W, K).permute(0, 3, 1, 2).float().contiguous()
        y_oh = torch.nn.functional.one_hot(labels.long()[label_rows], K).reshape(N, H, W, K).permute(0, 3, 1, 2).float().contiguous()
        kl = dm.kl_clamped(dm.theta_post(xt_oh, y_oh, t_rows), dm.theta_post_prob(xt_oh, theta, t_rows))
        return kl.sum(dim=1).double().sum(dim=(1, 2))

    fused()
    got, want = row_sum.clone(), chain()
    torch.cuda.synchronize(dev)
    # both are fp32 per pixel; at t = T a pixel's term is about 1e-7, the size of its rounding: the comparison is absolute, per pixel
    diff = float((got - want).abs().max()) / HW
    assert diff <= 2 * (K + 256) * 2.0 ** -24, f"fused and chain per-row sums differ by {diff} per pixel"
    variants = {"fused": fused, "fused_terms": terms, "chain": chain}
    if with_network:
        image = torch.from_numpy(rng.uniform(-1, 1, (N, Cimg, H, W)).astype(np.float32)).to(dev)
        eng = model._engine(torch.empty((N, K, H, W), device="meta"), image, None)
        ctx = eng.enter()
        ctx.__enter__()
        eng.set_inputs(xt.reshape(N, H, W), image)
        eng.set_tables([float(v) for v in table_np["t"]], [(0.0, 1.0, hip.STEP_SOFTMAX_ONLY)] * N, per_sample=True)
        variants["network"] = lambda: eng.run(1, with_epilogue=True, use_graph=False)
        stream = eng.stream.cuda_stream                              # everything is timed on the engine's stream
    for fn in variants.values():                                     # untimed: code objects, allocator, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    us = {k: [] for k in variants}
    iters = {}
    for _ in range(reps):
        for k, fn in variants.items():
            v, iters[k] = window(fn, seconds, dev)
            us[k].append(v)
    if with_network:
        ctx.__exit__(None, None, None)
        eng.leave()
    med = {k: float(np.median(v)) for k, v in us.items()}
    px = N * HW
    bytes_moved = {"fused": px * (4 * K + 4), "fused_terms": px * (4 * K + 2),
                   # BCHW copy 8K; one_hot(x_t): 1 in, 8K int64 out, then 8K in, 4K out (likewise y); theta_post 12K; theta_post_prob 12K;
                   # kl 12K; class sum 4K + 4; pixel sum 4 + 8 — counted at their least: fp32 one-hots written once
                   "chain": px * (8 * K + 2 * (1 + 4 * K) + 12 * K + 12 * K + 12 * K + 4 * K + 4 + 12)}
    res = {"shape": name, "N": N, "K": K, "size": [H, W], "reps": reps, "window_s": seconds, "iterations_per_window": iters,
           "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in us.items()},
           "bytes_moved": bytes_moved, "GBps": {k: round(bytes_moved[k] / med[k] / 1e3, 1) for k in bytes_moved},
           "chain_over_fused": round(med["chain"] / med["fused"], 2),
           "chain_over_fused_range": [round(min(us["chain"]) / max(us["fused"]), 2), round(max(us["chain"]) / min(us["fused"]), 2)],
           "max_row_sum_diff_per_pixel": diff}
    if with_network:
        res["share_of_pass"] = {k: round(med[k] / (med["network"] + med[k]), 4) for k in ("fused", "chain")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="lidc,cityscapes")
    ap.add_argument("--no-network", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_bound: needs a GPU (there is no CPU path to time)")
    if a.reps < 3:
        raise SystemExit("bench_label_bound: --reps must be at least 3")
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        print(json.dumps(bench_shape(name, SHAPES[name], a.reps, a.window, not a.no_network, dev)), flush=True)


if __name__ == "__main__":
    main()
