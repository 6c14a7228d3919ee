#!/usr/bin/env python3
"""Times what sampling with known labels (DenoisingModel(..., known_labels=)) adds to a denoise step at the C2 shape — LIDC network,
128x128, K = 2, batch 64, the full T = 250 walk, synthetic weights — in one run, the cases interleaved round by round:

    unconditioned         the plain call as it ships (substreams = 0: the execution mode is measured once, before the timed rounds)
    unconditioned_static  the plain call pinned to the static execution mode a conditioned call takes (calibrate_mode off)
    all_free              known_labels with every pixel free: the per-step stepping and the clamp launch, no pixel rewritten
    mask                  known_labels with a `--share` of the pixels known (default 0.1), drawn at random

A conditioned call walks every engine one step at a time and launches ccdm_known_labels_step behind each step: one more launch per
step and sub-batch, and a host round per step where the plain call hands a whole walk to ccdm_engine_run.  Host clock around calls
that end in a device synchronise, after one untimed call per case; ms per denoise step = call time / steps.

Resampling jumps (resample=(jump_length, resamples)), in the same run:

    renoise_kernel        ccdm_renoise_step alone at the C2 shape (64 x 128x128, K = 2, no xin: the 4-pixel kernel) and at 4 x 128x256,
                          K = 20 with xin, next to ccdm_known_labels_step over an all-known map of the same shape and, without xin, the
                          one-pixel-per-thread kernel (an xt that is not 4-byte aligned takes it): device events around `--launches`
                          back-to-back launches (so a launch's share of the queue, not a kernel trace), rounds interleaved in rotating order;
                          with the bytes the kernel moves and the share of 8 TB/s they imply at the measured time
    resampled             the `mask` call with resample = `--resample` (default 10,10: 2320 rows at T = 250 against 250), against
                          the plain conditioned call: ms per call and per row walked

Prints one JSON line.

    python tools/bench_known_labels.py [--rounds 5] [--batch 64] [--steps 250] [--share 0.1] [--resample 10,10] [--resample-rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict  # noqa: E402
from ccdm_stochastic_segmentation_amd.models import resample_walk, step_values  # noqa: E402

HBM_BYTES_PER_S = 8e12


def bench_renoise_kernel(dev, launches, rounds):
    """ccdm_renoise_step and, over an all-known map equal to xt, ccdm_known_labels_step: us per launch, back to back on one stream."""
    lib = hip.load()
    rng = np.random.default_rng(1)
    out = {}
    for name, (N, HW, K, stride) in {"C2 64x128x128 K=2": (64, 128 * 128, 2, 0), "4x128x256 K=20 xin": (4, 128 * 256, 20, 23)}.items():
        buf = torch.zeros(N * HW + 4, dtype=torch.uint8, device=dev)        # (xt, and one byte further on, the same map unaligned)
        xt, xt_odd = buf[:N * HW], buf[1:1 + N * HW]
        xt.copy_(torch.from_numpy(rng.integers(0, K, N * HW).astype(np.uint8)))
        known = xt.clone()
        xin = torch.zeros((N, HW, stride), device=dev) if stride else None
        xp = None if xin is None else xin.data_ptr()
        r = 0.9
        p_move = (1.0 - r) / K
        p_stay, p_move = float(np.float32(r + p_move)), float(np.float32(p_move))
        stream = torch.cuda.current_stream(dev).cuda_stream

        def renoise(i, ptr=xt.data_ptr()):
            hip.check(lib.ccdm_renoise_step(N, HW, K, p_stay, p_move, i % 250, 1, 0, ptr, xp, stride, stream), "renoise_step")

        def clamp(i):
            hip.check(lib.ccdm_known_labels_step(known.data_ptr(), N, HW, K, p_stay, p_move, hip.STEP_SAMPLE, i % 250, 1, 0, xt.data_ptr(), xp,
                                                 stride, None, None, stream), "known_labels_step")
        fns = {"renoise": renoise, "clamp_all_known": clamp}
        if not stride:                                       # an xt that is not 4-byte aligned takes the one-pixel-per-thread kernel
            fns["renoise_per_byte"] = lambda i: renoise(i, xt_odd.data_ptr())
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
        moved = N * HW * (2 + 4 * K * (1 if stride else 0))         # 1 byte read, 1 byte (+ K floats of xin) written per pixel
        med = {k: float(np.median(v)) for k, v in us.items()}
        out[name] = {"us_per_launch": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in us.items()},
                     "bytes_moved": moved, "share_of_8TBps": round(moved / HBM_BYTES_PER_S / (med["renoise"] * 1e-6), 4),
                     "renoise_over_clamp": round(med["renoise"] / med["clamp_all_known"], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--resample", default="10,10", help="jump_length,resamples of the resampled call ('' = skip it)")
    ap.add_argument("--resample-rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5000, help="back-to-back launches per timed round of the renoise kernel (0 = skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_known_labels: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    N, K, H, W, T = a.batch, 2, 128, 128, 250
    bp = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
    model = build_model(T, "cosine", {"s": 0.008}, [(1, H, W), (K, H, W)], (1, H, W), "unet_openai", bp, "datasets.lidc", "confidence", None)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}, strict=True)
    model = model.to(dev).eval()
    model.philox_seed, model.philox_advance = 1, False
    rng = np.random.default_rng(0)
    image = torch.from_numpy(rng.uniform(-1, 1, (N, 1, H, W)).astype(np.float32)).to(dev)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (N, H, W))), K).permute(0, 3, 1, 2).float().to(dev)
    free = torch.full((N, H, W), 255, dtype=torch.uint8)
    labels = torch.from_numpy(rng.integers(0, K, (N, H, W)).astype(np.uint8))
    mask = torch.where(torch.from_numpy(rng.random((N, H, W)) < a.share), labels, free)
    t = torch.as_tensor(10000 + a.steps) if a.steps < T else None
    kw = {} if t is None else {"t": t}

    def call(calibrate, known):
        model.calibrate_mode = calibrate
        extra = {} if known is None else {"known_labels": known}
        out = model(x, image, **kw, **extra)["diffusion_out"]
        torch.cuda.synchronize(dev)
        return out

    cases = {"unconditioned": (True, None), "unconditioned_static": (False, None), "all_free": (False, free), "mask": (False, mask)}
    outs, modes = {}, {}
    for name, (cal, known) in cases.items():                 # untimed: engines, graph capture, the execution-mode measurement
        outs[name] = call(cal, known)
        modes[name] = list(model.last_mode)
    assert torch.equal(outs["unconditioned"], outs["unconditioned_static"]) and torch.equal(outs["unconditioned"], outs["all_free"])
    ms = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, (cal, known) in cases.items():
            t0 = time.perf_counter()
            call(cal, known)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    res = {"shape": {"N": N, "K": K, "size": [H, W], "steps": a.steps}, "rounds": a.rounds, "share_known": float((mask != 255).float().mean()),
           "mode_streams_graph": modes,
           "ms_per_denoise_step": {n: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()}}
    base = float(np.median(ms["unconditioned_static"]))
    res["over_unconditioned_static"] = {n: round(float(np.median(ms[n])) / base, 4) for n in ("all_free", "mask")}
    if a.launches > 0:
        res["renoise_kernel"] = bench_renoise_kernel(dev, a.launches, a.rounds)
    if a.resample:
        pair = tuple(int(v) for v in a.resample.split(","))
        rows = len(resample_walk(len(step_values(T, None if t is None else int(t))), *pair))
        jumps = (rows - a.steps) // max(pair[0], 1)

        def resampled():
            model.calibrate_mode = False
            out = model(x, image, **kw, known_labels=mask, resample=pair)["diffusion_out"]
            torch.cuda.synchronize(dev)
            return out
        keep = mask != 255
        got = resampled().cpu()                                # untimed; the known pixels still come back as their labels
        assert torch.equal(got.argmax(1)[keep], mask[keep].long())
        call_ms = {"conditioned": [], "resampled": []}
        for _ in range(a.resample_rounds):
            for name, fn in (("conditioned", lambda: call(False, mask)), ("resampled", resampled)):
                t0 = time.perf_counter()
                fn()
                call_ms[name].append((time.perf_counter() - t0) * 1e3)
        cm, rm = float(np.median(call_ms["conditioned"])), float(np.median(call_ms["resampled"]))
        res["resampled"] = {"resample": list(pair), "rows": rows, "plain_rows": a.steps, "renoise_launches_per_sub_batch": jumps,
                            "rounds": a.resample_rounds, "ms_per_call": {n: [round(v, 1) for v in vs] for n, vs in call_ms.items()},
                            "ms_per_row": {"conditioned": round(cm / a.steps, 4), "resampled": round(rm / rows, 4)},
                            "call_over_conditioned": round(rm / cm, 4), "rows_over_plain_rows": round(rows / a.steps, 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
