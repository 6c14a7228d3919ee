#!/usr/bin/env python3
"""Times ccdm_lidcscore (the launch metrics.vote_joint_counts makes, the clearing of the outputs included) against a torch device
path of the same counts (one-hot sums over the stacks + bincount) at the LIDC shape: B = 16 images, S = 100 samples, L = 4
raters, 128 x 128, K = 2.  Maps like LIDC's: mostly background, a disc the samples and raters disagree about.  Device events
after warm-up; both paths are held against each other first.  Prints one JSON line.

    python tools/bench_lidcscore.py [--iters 50] [--warmup 5] [--batch 16] [--samples 100]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from bench_segeval import peak_above, timed  # noqa: E402


def inputs(B, S, L, R, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:R, 0:R]
    cy, cx, rad = rng.uniform(40, 88, (B, 1, 1, 1)), rng.uniform(40, 88, (B, 1, 1, 1)), rng.uniform(6, 20, (B, 1, 1, 1))
    d2 = (yy - cy) ** 2 + (xx - cx) ** 2
    samples = (d2 <= (rad * rng.uniform(0.6, 1.3, (B, S, 1, 1))) ** 2).astype(np.uint8).reshape(B, S, R * R)
    raters = (d2 <= (rad * rng.uniform(0.6, 1.3, (B, L, 1, 1))) ** 2).astype(np.uint8).reshape(B, L, R * R)
    return torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda()


def torch_path(samples, raters, K):
    B, S, HW = samples.shape
    L = raters.shape[1]
    ks = torch.arange(K, device=samples.device, dtype=torch.uint8)[None, None, :, None]
    n = (samples[:, :, None, :] == ks).sum(1)              # [B,K,HW]
    m = (raters[:, :, None, :] == ks).sum(1)
    bk = torch.arange(B * K, device=samples.device).reshape(B, K, 1)
    joint = torch.bincount(((bk * (S + 1) + n) * (L + 1) + m).flatten(), minlength=B * K * (S + 1) * (L + 1)).reshape(B, K, S + 1, L + 1)
    u, v = S * S - (n * n).sum(1), L * L - (m * m).sum(1)
    return joint, torch.stack([u.sum(1), v.sum(1), (u * u).sum(1), (v * v).sum(1), (u * v).sum(1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=100)
    a = ap.parse_args()
    B, S, L, R, K = a.batch, a.samples, 4, 128, 2
    samples, raters = inputs(B, S, L, R)
    lib = hip.load()
    joint = torch.empty((B, K, S + 1, L + 1), dtype=torch.int32, device="cuda")
    moments = torch.empty((B, 5), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        hip.check(lib.ccdm_lidcscore(samples.data_ptr(), raters.data_ptr(), B, S, L, R * R, K, joint.data_ptr(), moments.data_ptr(), stream),
                  "lidcscore")
    kernel()
    tj, tm = torch_path(samples, raters, K)
    assert torch.equal(joint.long(), tj) and torch.equal(moments, tm), "the two paths disagree"
    nbytes = samples.numel() + raters.numel()
    res = {"B": B, "S": S, "L": L, "HW": R * R, "K": K, "bytes_moved_MB": nbytes / 2 ** 20}
    res["kernel_us_median"], res["kernel_us_min"] = timed(kernel, a.iters, a.warmup)
    res["kernel_GBps"] = nbytes / (res["kernel_us_median"] * 1e-6) / 1e9
    tp = lambda: torch_path(samples, raters, K)         # noqa: E731
    res["torch_us_median"], res["torch_us_min"] = timed(tp, max(3, a.iters // 5), 2)
    res["torch_peak_MB"] = peak_above(tp) / 2 ** 20
    res["background_share"] = float((samples == 0).float().mean())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
