#!/usr/bin/env python3
"""Times ccdm_segcalib (the launches SegmentationCalibration.update makes) against ccdm_seg_confusion on the same inputs in the
same run (the yardstick: the same interpolation and argmax) and against a torch device path of the same scores (F.interpolate
bilinear + renormalise + max + bucketing + bincount + log + Brier) at the Cityscapes shapes: C4 (B = 16, 256x512 -> 1024x2048)
and a C5 shard (B = 4, 512x1024 -> 1024x2048), K = 20, 15 bins.  Device events after warm-up; peak device memory of one call
above the inputs; the bytes a call has to move (prediction and labels once).  Prints one JSON line per shape.

    python tools/bench_segcalib.py [--iters 20] [--warmup 3] [--bins 15]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from bench_segeval import SHAPES, inputs, peak_above, timed  # noqa: E402


def torch_path(pred, lab, C, M):
    up = F.interpolate(pred, tuple(lab.shape[1:]), mode="bilinear")[:, :C]
    s = up.sum(1, keepdim=True)
    q = torch.where(s > 0, up / s, torch.full_like(up, 1.0 / C))
    conf, cls = q.max(1)
    t = lab.long()
    m = t < C
    tc = torch.where(m, t, torch.zeros_like(t))
    qt = q.gather(1, tc[:, None])[:, 0]
    cell = (cls * M + (conf * M).long().clamp(max=M - 1))[m]
    right = (cls == t)[m]
    bins = torch.stack([torch.bincount(cell, minlength=C * M), torch.bincount(cell[right], minlength=C * M)], 1)
    conf_sum = torch.bincount(cell, weights=conf[m].double(), minlength=C * M)
    brier = (q * q).sum(1) - 2 * qt + 1
    sums = torch.stack([-(qt[m].double().clamp_min(1e-12).log()).sum(), brier[m].double().sum(), qt[m].double().sum()])
    return bins, conf_sum, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bins", type=int, default=15)
    a = ap.parse_args()
    for name, (B, h, w, H, W) in SHAPES.items():
        pred, lab = inputs(B, h, w, H, W)
        lib, K, C, M = hip.load(), 20, 19, a.bins
        probs = pred.permute(0, 2, 3, 1)              # the channels-last memory the BCHW view shows
        ws = torch.empty(lib.ccdm_segcalib_workspace_bytes(B, H, W, K, M), dtype=torch.uint8, device="cuda")
        bins = torch.zeros((C, M, 2), dtype=torch.int64, device="cuda")
        out = torch.empty(C * M + 3, dtype=torch.float64, device="cuda")
        ws_cm = torch.empty(lib.ccdm_seg_confusion_workspace_bytes(B, H, W, K), dtype=torch.uint8, device="cuda")
        hard = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        soft = torch.empty((C, C), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def calib():
            hip.check(lib.ccdm_segcalib(probs.data_ptr(), K, None, lab.data_ptr(), B, h, w, H, W, K, M, bins.data_ptr(), out.data_ptr(),
                                        out.data_ptr() + 8 * C * M, ws.data_ptr(), ws.numel(), stream), "segcalib")

        def confusion():
            hip.check(lib.ccdm_seg_confusion(probs.data_ptr(), K, None, lab.data_ptr(), B, h, w, H, W, K, hard.data_ptr(), soft.data_ptr(),
                                             ws_cm.data_ptr(), ws_cm.numel(), stream), "seg_confusion")
        res = {"shape": name, "B": B, "in": [h, w], "out": [H, W], "K": K, "bins": M}
        res["confusion_us_median"], res["confusion_us_min"] = timed(confusion, a.iters, a.warmup)
        res["calib_us_median"], res["calib_us_min"] = timed(calib, a.iters, a.warmup)
        res["calib_over_confusion"] = res["calib_us_median"] / res["confusion_us_median"]
        res["bytes_moved_MB"] = (probs.numel() * 4 + lab.numel()) / 2 ** 20
        res["calib_GBps"] = (probs.numel() * 4 + lab.numel()) / (res["calib_us_median"] * 1e-6) / 1e9
        res["calib_peak_MB"] = (peak_above(calib) + ws.numel()) / 2 ** 20      # + the workspace, allocated above
        tp = lambda: torch_path(pred, lab, C, M)         # noqa: E731
        res["torch_us_median"], res["torch_us_min"] = timed(tp, max(3, a.iters // 4), 1)
        res["torch_peak_MB"] = peak_above(tp) / 2 ** 20
        print(json.dumps(res), flush=True)
        del pred, lab, ws, ws_cm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
