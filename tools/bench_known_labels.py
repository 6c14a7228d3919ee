#!/usr/bin/env python3
"""Times what sampling with known labels (DenoisingModel(..., known_labels=)) adds to a denoise step at the C2 shape — LIDC network,
128x128, K = 2, batch 64, the full T = 250 walk, synthetic weights — in one run, the cases interleaved round by round:

    unconditioned         the plain call as it ships (substreams = 0: the execution mode is measured once, before the timed rounds)
    unconditioned_static  the plain call pinned to the static execution mode a conditioned call takes (calibrate_mode off)
    all_free              known_labels with every pixel free: the per-step stepping and the clamp launch, no pixel rewritten
    mask                  known_labels with a `--share` of the pixels known (default 0.1), drawn at random

A conditioned call walks every engine one step at a time and launches ccdm_known_labels_step behind each step: one more launch per
step and sub-batch, and a host round per step where the plain call hands a whole walk to ccdm_engine_run.  Host clock around calls
that end in a device synchronise, after one untimed call per case; ms per denoise step = call time / steps.  Prints one JSON line.

    python tools/bench_known_labels.py [--rounds 5] [--batch 64] [--steps 250] [--share 0.1]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--share", type=float, default=0.1)
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
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
