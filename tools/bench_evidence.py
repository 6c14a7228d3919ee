#!/usr/bin/env python3
"""Times sampling under per-pixel soft evidence (DenoisingModel(..., evidence=)) in one run.

    evidence_kernel   ccdm_evidence_step alone at 64 x 128x128, K = 2 (one thread per pixel, no xin) and at 4 x 128x256, K = 20 with xin
                      (the staged kernel), in STEP_SAMPLE: device events around `--launches` back-to-back launches (so a launch's share
                      of the queue, not a kernel trace), rounds interleaved in rotating order; with the bytes the launch moves —
                      8 K + 1 in, 1 out, + 4 K where xin is written — and the share of 8 TB/s they imply at the measured time.  Next
                      to it ccdm_posterior_sample on the same probabilities (softmax = 0): the unguided step's own draw kernel, which
                      reads half the floats.
    step              the C2 shape — LIDC network, 128x128, K = 2, batch 64, synthetic weights — cases interleaved round by round:
                        unguided_static   the plain call pinned to the static execution mode a guided call takes (calibrate_mode off):
                                          the step of the code as it was before the keyword existed, which a call without it still takes
                        all_ones          evidence of all ones: the per-step stepping, the head stopping at x0 and the evidence launch;
                                          the samples are the unguided call's, bit for bit (asserted)
                        soft              random weights in [0.05, 1]
                      Host clock around calls that end in a device synchronise, after one untimed call per case; ms per denoise step =
                      call time / steps.

Prints one JSON line.

    python tools/bench_evidence.py [--rounds 5] [--batch 64] [--steps 250] [--launches 5000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict  # noqa: E402

HBM_BYTES_PER_S = 8e12


def bench_kernel(dev, launches, rounds):
    lib = hip.load()
    rng = np.random.default_rng(1)
    out = {}
    for name, (N, HW, K, stride) in {"64x128x128 K=2": (64, 128 * 128, 2, 0), "4x128x256 K=20 xin": (4, 128 * 256, 20, 23)}.items():
        r = (rng.random((N, HW, K)) + 0.5).astype(np.float32)
        x0 = torch.from_numpy(r / r.sum(-1, keepdims=True)).to(dev)
        ev = torch.from_numpy(rng.uniform(0.05, 1.0, (N, HW, K)).astype(np.float32)).to(dev)
        xt = torch.from_numpy(rng.integers(0, K, (N, HW)).astype(np.uint8)).to(dev)
        xin = torch.zeros((N, HW, stride), device=dev) if stride else None
        xp = None if xin is None else xin.data_ptr()
        a, c = 0.98, 0.6
        table = torch.tensor([[a, c, float(hip.STEP_SAMPLE), 0.0]] * 250, dtype=torch.float32, device=dev)
        steps = torch.arange(250, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        post = hip.PostArgs()
        post.head, post.softmax, post.head_stride = x0.data_ptr(), 0, K
        post.xt, post.N, post.HW, post.K = xt.data_ptr(), N, HW, K
        post.step_table = table.data_ptr()
        post.philox_seed, post.sample_offset = 1, 0
        post.xt_next = xt.data_ptr()
        post.xin, post.xin_stride = (0 if xin is None else xp), stride

        def evidence(i):
            hip.check(lib.ccdm_evidence_step(x0.data_ptr(), ev.data_ptr(), N, HW, K, a, c, hip.STEP_SAMPLE, i % 250, 1, 0, xt.data_ptr(), xp,
                                             stride, None, None, stream), "evidence_step")

        def unguided(i):
            post.step_ptr = steps.data_ptr() + 4 * (i % 250)
            hip.check(lib.ccdm_posterior_sample(C.byref(post), stream), "posterior_sample")
        fns = {"evidence": evidence, "unguided_draw": unguided}
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
        moved = N * HW * (8 * K + 2 + 4 * K * (1 if stride else 0))
        med = {k: float(np.median(v)) for k, v in us.items()}
        out[name] = {"us_per_launch": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in us.items()},
                     "bytes_moved": moved, "share_of_8TBps": round(moved / HBM_BYTES_PER_S / (med["evidence"] * 1e-6), 4),
                     "evidence_over_unguided_draw": round(med["evidence"] / med["unguided_draw"], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--launches", type=int, default=5000, help="back-to-back launches per timed round of the kernel (0 = skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evidence: needs a GPU (there is no CPU path to time)")
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
    cases = {"unguided_static": None, "all_ones": torch.ones((N, K, H, W)),
             "soft": torch.from_numpy(rng.uniform(0.05, 1.0, (N, K, H, W)).astype(np.float32))}

    def call(ev):
        out = model(x, image, **kw, **({} if ev is None else {"evidence": ev}))["diffusion_out"]
        torch.cuda.synchronize(dev)
        return out

    outs, modes = {}, {}
    for name, ev in cases.items():                           # untimed: engines, graph capture
        outs[name] = call(ev)
        modes[name] = list(model.last_mode)
    assert torch.equal(outs["unguided_static"], outs["all_ones"]) and not torch.equal(outs["unguided_static"], outs["soft"])
    ms = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, ev in cases.items():
            t0 = time.perf_counter()
            call(ev)
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    res = {"shape": {"N": N, "K": K, "size": [H, W], "steps": a.steps}, "rounds": a.rounds, "mode_streams_graph": modes,
           "ms_per_denoise_step": {n: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for n, v in ms.items()}}
    base = float(np.median(ms["unguided_static"]))
    res["over_unguided_static"] = {n: round(float(np.median(ms[n])) / base, 4) for n in ("all_ones", "soft")}
    if a.launches > 0:
        res["evidence_kernel"] = bench_kernel(dev, a.launches, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
