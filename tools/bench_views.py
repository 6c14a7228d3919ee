#!/usr/bin/env python3
"""Times flip-averaged sampling (DenoisingModel(..., views=)) in one run, at V = 2 (hflip) and V = 4 (hflip, vflip, hvflip).

    views_kernel      ccdm_views_step alone at 64 x 128x128, K = 2 (one thread per pixel, no xin) and at 4 x 128x256, K = 20 with xin
                      (the staged kernel), in STEP_SAMPLE at neutral shaping without evidence, beside ccdm_shaped_step on the same N
                      and K — the yardstick: the views launch reads V times its x0 bytes and writes V times its xt (and xin) bytes.
                      Device events around `--launches` back-to-back launches (so a launch's share of the queue, not a kernel trace),
                      rounds interleaved in rotating order.  Cases: shaped, views_v1 (V = 1: the same bytes through the views kernel),
                      views_v2, views_v4, and views_v2_vflip (V = 2 mirrored in y only: the source runs are forward runs).
    step              the LIDC network — 128x128, K = 2, synthetic weights — at batch `--batch`, cases interleaved round by round:
                        plain_static      the plain call pinned to the static execution mode a call with views takes
                        views_v2, views_v4  the call with views: V network passes per step on an engine of V * batch rows, one
                                          ccdm_views_step launch behind them
                        plain_rows_v2, plain_rows_v4  the plain call at V * batch samples: the same engine rows without the views launch
                      Host clock around calls that end in a device synchronise, after one untimed call per case; ms per denoise step =
                      call time / steps.  Reported: a views step over V plain steps, and over the plain step of the same rows.

Prints one JSON line.

    python tools/bench_views.py [--rounds 3] [--batch 16] [--steps 50] [--launches 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict  # noqa: E402

HFLIP, VFLIP, HVFLIP = 1, 2, 3


def bench_kernel(dev, launches, rounds):
    lib = hip.load()
    rng = np.random.default_rng(1)
    out = {}
    for name, (N, H, W, K, stride) in {"64x128x128 K=2": (64, 128, 128, 2, 0), "4x128x256 K=20 xin": (4, 128, 256, 20, 23)}.items():
        HW, VMAX = H * W, 4
        r = (rng.random((VMAX * N, HW, K)) + 0.5).astype(np.float32)
        x0 = torch.from_numpy(r / r.sum(-1, keepdims=True)).to(dev)
        xt = torch.from_numpy(rng.integers(0, K, (VMAX * N, HW)).astype(np.uint8)).to(dev)
        xin = torch.zeros((VMAX * N, HW, stride), device=dev) if stride else None
        xp = None if xin is None else xin.data_ptr()
        a, c = 0.98, 0.6
        stream = torch.cuda.current_stream(dev).cuda_stream

        def shaped(i):
            hip.check(lib.ccdm_shaped_step(x0.data_ptr(), None, N, HW, K, 1.0, 1.0, a, c, hip.STEP_SAMPLE, i % 250, 1, 0, xt.data_ptr(), xp, stride,
                                           None, None, stream), "shaped_step")

        def views(flips):
            code = sum(f << (2 * v) for v, f in enumerate(flips, 1))

            def launch(i):
                hip.check(lib.ccdm_views_step(x0.data_ptr(), None, N, H, W, K, 1 + len(flips), code, 1.0, 1.0, a, c, hip.STEP_SAMPLE, i % 250, 1, 0,
                                              xt.data_ptr(), xp, stride, None, None, stream), "views_step")
            return launch
        fns = {"shaped": shaped, "views_v1": views(()), "views_v2": views((HFLIP,)), "views_v4": views((HFLIP, VFLIP, HVFLIP)),
               "views_v2_vflip": views((VFLIP,))}
        us = {k: [] for k in fns}
        for fn in fns.values():                              # untimed: code objects, caches, clocks
            for i in range(launches // 4):
                fn(i)
        torch.cuda.synchronize(dev)
        order = list(fns)
        for _ in range(rounds):
            for key in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(launches):
                    fns[key](i)
                e1.record()
                e1.synchronize()
                us[key].append(e0.elapsed_time(e1) / launches * 1e3)
            order = order[1:] + order[:1]                    # (the first window of a round starts on an idle device)
        med = {k: float(np.median(v)) for k, v in us.items()}
        out[name] = {"us_per_launch": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in us.items()},
                     "over_shaped": {k: round(med[k] / med["shaped"], 3) for k in fns if k != "shaped"}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--launches", type=int, default=2000, help="back-to-back launches per timed round of the kernel (0 = skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_views: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    N, K, H, W, T = a.batch, 2, 128, 128, 250
    bp = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
    model = build_model(T, "cosine", {"s": 0.008}, [(1, H, W), (K, H, W)], (1, H, W), "unet_openai", bp, "datasets.lidc", "confidence", None)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}, strict=True)
    model = model.to(dev).eval()
    model.philox_seed, model.philox_advance, model.calibrate_mode = 1, False, False
    rng = np.random.default_rng(0)
    image = torch.from_numpy(rng.uniform(-1, 1, (4 * N, 1, H, W)).astype(np.float32)).to(dev)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (4 * N, H, W))), K).permute(0, 3, 1, 2).float().to(dev)
    t = torch.as_tensor(10000 + a.steps) if a.steps < T else None
    kw = {} if t is None else {"t": t}
    cases = {"plain_static": (N, {}), "views_v2": (N, dict(views=("hflip",))), "views_v4": (N, dict(views=("hflip", "vflip", "hvflip"))),
             "plain_rows_v2": (2 * N, {}), "plain_rows_v4": (4 * N, {})}

    def call(n, extra):
        out = model(x[:n], image[:n], **kw, **extra)["diffusion_out"]
        torch.cuda.synchronize(dev)
        return out

    outs, modes = {}, {}
    for name, (n, extra) in cases.items():                   # untimed: engines, graph capture
        outs[name] = call(n, extra)
        modes[name] = list(model.last_mode)
    assert not torch.equal(outs["plain_static"], outs["views_v2"]) and outs["views_v4"].shape == outs["plain_static"].shape
    ms = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, (n, extra) in cases.items():
            t0 = time.perf_counter()
            call(n, extra)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    med = {n: float(np.median(v)) for n, v in ms.items()}
    res = {"shape": {"N": N, "K": K, "size": [H, W], "steps": a.steps}, "rounds": a.rounds, "mode_streams_graph": modes,
           "ms_per_denoise_step": {n: {"median": round(med[n], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()},
           "views_step_over_V_plain_steps": {f"v{V}": round(med[f"views_v{V}"] / (V * med["plain_static"]), 4) for V in (2, 4)},
           "views_step_over_plain_step_of_the_same_rows": {f"v{V}": round(med[f"views_v{V}"] / med[f"plain_rows_v{V}"], 4) for V in (2, 4)}}
    if a.launches > 0:
        res["views_kernel"] = bench_kernel(dev, a.launches, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
