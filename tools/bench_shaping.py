#!/usr/bin/env python3
"""Times temperature and truncation sampling (DenoisingModel(..., temperature=, truncation=)) in one run.

    shaped_kernel     ccdm_shaped_step alone at 64 x 128x128, K = 2 (one thread per pixel, no xin) and at 4 x 128x256, K = 20 with xin
                      (the staged kernel), in STEP_SAMPLE.  The yardstick is the kernel itself at (tau, r) = (1, 1), where both parts
                      are skipped: the same bytes moved, without the selection.  Device events around `--launches` back-to-back
                      launches (so a launch's share of the queue, not a kernel trace), rounds interleaved in rotating order.  Cases,
                      all with evidence unless named otherwise:
                        evidence_entry      ccdm_evidence_step: the same kernel at (1, 1) through the entry that takes no shaping
                        neutral             (tau, r) = (1, 1) through ccdm_shaped_step
                        truncate            r = 0.9 on flat rows (every entry within a factor 3 of the others: at K = 20 a pixel scans
                                            about 18 times before its mass reaches r)
                        truncate_peaked     r = 0.9 on rows that are softmax of 4 N(0,1) logits (one to three scans), mixed pixel by
                                            pixel with flat rows: lanes of a wave leave the loop at different times
                        temper              tau = 0.7, r = 1: a division, a logarithm and an exponential per class
                        temper_truncate     tau = 0.7, r = 0.9 on flat rows
                        truncate_no_evidence  r = 0.9 without the evidence operand (half the floats read)
    step              the C2 shape — LIDC network, 128x128, K = 2, batch 64, synthetic weights — cases interleaved round by round:
                        unguided_static   the plain call pinned to the static execution mode a guided call takes (calibrate_mode off)
                        neutral           temperature = truncation = 1.0: the per-step stepping, the head stopping at x0 and the shaped
                                          launch; the samples are the unguided call's, bit for bit (asserted)
                        shaped            temperature = 0.7, truncation = 0.9
                        evidence          random weights in [0.05, 1] (the evidence-guided step)
                        shaped_evidence   both: still one launch behind the network
                      Host clock around calls that end in a device synchronise, after one untimed call per case; ms per denoise step =
                      call time / steps.

Prints one JSON line.

    python tools/bench_shaping.py [--rounds 5] [--batch 64] [--steps 250] [--launches 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict  # noqa: E402


def bench_kernel(dev, launches, rounds):
    lib = hip.load()
    rng = np.random.default_rng(1)
    out = {}
    inv_tau = float(np.float32(1.0 / 0.7))
    for name, (N, HW, K, stride) in {"64x128x128 K=2": (64, 128 * 128, 2, 0), "4x128x256 K=20 xin": (4, 128 * 256, 20, 23)}.items():
        r = (rng.random((N, HW, K)) + 0.5).astype(np.float32)
        flat = r / r.sum(-1, keepdims=True)
        logits = 4.0 * rng.standard_normal((N, HW, K))
        p = np.exp(logits - logits.max(-1, keepdims=True))
        peaked = flat.copy()
        peaked[:, 1::2] = np.maximum(p / p.sum(-1, keepdims=True), 1e-6).astype(np.float32)[:, 1::2]
        rows = {"flat": torch.from_numpy(flat).to(dev), "peaked": torch.from_numpy(peaked).to(dev)}
        ev = torch.from_numpy(rng.uniform(0.05, 1.0, (N, HW, K)).astype(np.float32)).to(dev)
        xt = torch.from_numpy(rng.integers(0, K, (N, HW)).astype(np.uint8)).to(dev)
        xin = torch.zeros((N, HW, stride), device=dev) if stride else None
        xp = None if xin is None else xin.data_ptr()
        a, c = 0.98, 0.6
        stream = torch.cuda.current_stream(dev).cuda_stream

        def evidence(i):
            hip.check(lib.ccdm_evidence_step(rows["flat"].data_ptr(), ev.data_ptr(), N, HW, K, a, c, hip.STEP_SAMPLE, i % 250, 1, 0, xt.data_ptr(),
                                             xp, stride, None, None, stream), "evidence_step")

        def shaped(kind, with_ev, inv, top_r):
            x0p, evp = rows[kind].data_ptr(), ev.data_ptr() if with_ev else None

            def launch(i):
                hip.check(lib.ccdm_shaped_step(x0p, evp, N, HW, K, inv, top_r, a, c, hip.STEP_SAMPLE, i % 250, 1, 0, xt.data_ptr(), xp, stride,
                                               None, None, stream), "shaped_step")
            return launch
        fns = {"evidence_entry": evidence, "neutral": shaped("flat", True, 1.0, 1.0), "truncate": shaped("flat", True, 1.0, 0.9),
               "truncate_peaked": shaped("peaked", True, 1.0, 0.9), "temper": shaped("flat", True, inv_tau, 1.0),
               "temper_truncate": shaped("flat", True, inv_tau, 0.9), "truncate_no_evidence": shaped("flat", False, 1.0, 0.9)}
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
                     "over_neutral": {k: round(med[k] / med["neutral"], 3) for k in fns if k != "neutral"}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--launches", type=int, default=2000, help="back-to-back launches per timed round of the kernel (0 = skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shaping: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    N, K, H, W, T = a.batch, 2, 128, 128, 250
    bp = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
    model = build_model(T, "cosine", {"s": 0.008}, [(1, H, W), (K, H, W)], (1, H, W), "unet_openai", bp, "datasets.lidc", "confidence", None)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}, strict=True)
    model = model.to(dev).eval()
    model.philox_seed, model.philox_advance, model.calibrate_mode = 1, False, False
    rng = np.random.default_rng(0)
    image = torch.from_numpy(rng.uniform(-1, 1, (N, 1, H, W)).astype(np.float32)).to(dev)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (N, H, W))), K).permute(0, 3, 1, 2).float().to(dev)
    t = torch.as_tensor(10000 + a.steps) if a.steps < T else None
    kw = {} if t is None else {"t": t}
    soft = torch.from_numpy(rng.uniform(0.05, 1.0, (N, K, H, W)).astype(np.float32))
    cases = {"unguided_static": {}, "neutral": dict(temperature=1.0, truncation=1.0), "shaped": dict(temperature=0.7, truncation=0.9),
             "evidence": dict(evidence=soft), "shaped_evidence": dict(evidence=soft, temperature=0.7, truncation=0.9)}

    def call(extra):
        out = model(x, image, **kw, **extra)["diffusion_out"]
        torch.cuda.synchronize(dev)
        return out

    outs, modes = {}, {}
    for name, extra in cases.items():                        # untimed: engines, graph capture
        outs[name] = call(extra)
        modes[name] = list(model.last_mode)
    assert torch.equal(outs["unguided_static"], outs["neutral"]) and not torch.equal(outs["unguided_static"], outs["shaped"])
    ms = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, extra in cases.items():
            t0 = time.perf_counter()
            call(extra)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    res = {"shape": {"N": N, "K": K, "size": [H, W], "steps": a.steps}, "rounds": a.rounds, "mode_streams_graph": modes,
           "ms_per_denoise_step": {n: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()}}
    base = float(np.median(ms["unguided_static"]))
    res["over_unguided_static"] = {n: round(float(np.median(ms[n])) / base, 4) for n in cases if n != "unguided_static"}
    res["shaped_over_evidence"] = round(float(np.median(ms["shaped"])) / float(np.median(ms["evidence"])), 4)
    if a.launches > 0:
        res["shaped_kernel"] = bench_kernel(dev, a.launches, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
