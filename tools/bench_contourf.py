#!/usr/bin/env python3
"""Times ccdm_contourf (one of the launches SegmentationContourF.update makes: the boundary F-score counts at one tolerance) against
ccdm_segboundary at d = 46 on the same two class maps in the same run (the yardstick: it reads and writes the same bytes, one
byte per pixel and map in, one 16-bit word per pixel through the workspace) at B = 4, 1024x2048, K = 20, theta = 17 (bfscore's
0.75 % of the diagonal there).  The labels are blocks of 32 pixels with ignored blocks; the prediction is the labels `--shift`
pixels off with a `--salt` share of the pixels redrawn, so most contour pixels match within a few rows and the salt away from
the edges searches its whole disc.  Device events after warm-up.  Prints one JSON line.

    python tools/bench_contourf.py [--iters 20] [--warmup 3] [--theta 17] [--shift 5 7] [--salt 0.01]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from bench_segeval import inputs, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--theta", type=int, default=17)
    ap.add_argument("--shift", type=int, nargs=2, default=[5, 7])
    ap.add_argument("--salt", type=float, default=0.01)
    a = ap.parse_args()
    B, H, W, K, D = 4, 1024, 2048, 20, 46
    C = K - 1
    _, lab = inputs(B, 8, 8, H, W)
    g = torch.Generator(device="cuda").manual_seed(2)
    pred = torch.roll(lab, tuple(a.shift), dims=(1, 2))
    pred = torch.where(pred < C, pred, torch.zeros_like(pred))
    salt = torch.rand((B, H, W), generator=g, device="cuda") < a.salt
    pred = torch.where(salt, torch.randint(0, C, (B, H, W), generator=g, device="cuda").to(torch.uint8), pred).contiguous()
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(max(lib.ccdm_contourf_workspace_bytes(B, H, W), lib.ccdm_segboundary_workspace_bytes(B, H, W)), dtype=torch.uint8,
                     device="cuda")
    counts = torch.zeros((B, C, 4), dtype=torch.int64, device="cuda")
    bc = torch.zeros((C, 3), dtype=torch.int64, device="cuda")
    tm = torch.zeros((C, C), dtype=torch.int64, device="cuda")

    def contourf():
        hip.check(lib.ccdm_contourf(pred.data_ptr(), lab.data_ptr(), B, H, W, K, a.theta, counts.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                  "contourf")

    def boundary():
        hip.check(lib.ccdm_segboundary(pred.data_ptr(), lab.data_ptr(), B, H, W, K, D, bc.data_ptr(), tm.data_ptr(), ws.data_ptr(), ws.numel(),
                                       stream), "segboundary")

    contourf()
    torch.cuda.synchronize()
    once = counts.sum((0, 1)).tolist()
    res = {"B": B, "size": [H, W], "K": K, "theta": a.theta, "boundary_d": D, "shift": a.shift, "salt": a.salt,
           "contour_pixels": {"nP": once[0], "mP": once[1], "nG": once[2], "mG": once[3]}}
    res["contourf_us_median"], res["contourf_us_min"] = timed(contourf, a.iters, a.warmup)
    res["segboundary_us_median"], res["segboundary_us_min"] = timed(boundary, a.iters, a.warmup)
    res["contourf_over_segboundary"] = res["contourf_us_median"] / res["segboundary_us_median"]
    res["bytes_moved_MB"] = (2 * pred.numel() + 2 * 2 * pred.numel()) / 2 ** 20      # both maps in, the workspace written and read
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
