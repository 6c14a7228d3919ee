#!/usr/bin/env python3
"""Times ccdm_uncscore (the launch SegmentationUncertainty.update makes) against ccdm_segcalib on the same probabilities and labels
in the same run (the yardstick: it reads the same bytes minus the small maps, with the same interpolation and argmax) at B = 4,
128x256 -> 1024x2048, K = 20, U = 2 maps, M = 256 bins, P = 8.  The maps are 0 on `--zero` of the pixels (the share of an image
on which the samples agree) and uniform on [0, ln K) elsewhere; `--zero 0` is the worst case for the per-wave grouping (every lane
its own bin).  Device events after warm-up.  Prints one JSON line per zero share.

    python tools/bench_uncscore.py [--iters 20] [--warmup 3] [--bins 256] [--patch 8] [--zero 0.9 0.0]"""
import argparse
import ctypes
import json
import math
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
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--patch", type=int, default=8)
    ap.add_argument("--zero", type=float, nargs="+", default=[0.9, 0.0])
    a = ap.parse_args()
    B, h, w, H, W, K, U, M, P, MC = 4, 128, 256, 1024, 2048, 20, 2, a.bins, a.patch, 15
    C = K - 1
    pred, lab = inputs(B, h, w, H, W)
    lib = hip.load()
    probs = pred.permute(0, 2, 3, 1)              # the channels-last memory the BCHW view shows
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.ccdm_segcalib_workspace_bytes(B, H, W, K, MC), dtype=torch.uint8, device="cuda")
    bins = torch.zeros((C, MC, 2), dtype=torch.int64, device="cuda")
    out = torch.empty(C * MC + 3, dtype=torch.float64, device="cuda")
    pix = torch.zeros((U, M, 2), dtype=torch.int64, device="cuda")
    patch = torch.zeros((U, M, 2), dtype=torch.int64, device="cuda")
    ranges = (ctypes.c_float * U)(*([math.log(K)] * U))

    def calib():
        hip.check(lib.ccdm_segcalib(probs.data_ptr(), K, None, lab.data_ptr(), B, h, w, H, W, K, MC, bins.data_ptr(), out.data_ptr(),
                                    out.data_ptr() + 8 * C * MC, ws.data_ptr(), ws.numel(), stream), "segcalib")

    calib_us = timed(calib, a.iters, a.warmup)
    g = torch.Generator(device="cuda").manual_seed(1)
    for zero in a.zero:
        maps = torch.rand((U, B, h, w), generator=g, device="cuda") * math.log(K)
        maps = torch.where(torch.rand((U, B, h, w), generator=g, device="cuda") < zero, torch.zeros_like(maps), maps).contiguous()

        def unc():
            hip.check(lib.ccdm_uncscore(probs.data_ptr(), K, None, lab.data_ptr(), maps.data_ptr(), ranges, B, h, w, H, W, K, U, M, P,
                                        pix.data_ptr(), patch.data_ptr(), None, 0, stream), "uncscore")

        res = {"B": B, "in": [h, w], "out": [H, W], "K": K, "U": U, "bins": M, "patch": P, "zero_share": zero}
        res["uncscore_us_median"], res["uncscore_us_min"] = timed(unc, a.iters, a.warmup)
        res["segcalib_us_median"], res["segcalib_us_min"] = calib_us
        res["uncscore_over_segcalib"] = res["uncscore_us_median"] / res["segcalib_us_median"]
        res["bytes_moved_MB"] = (probs.numel() * 4 + lab.numel() + maps.numel() * 4) / 2 ** 20
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
