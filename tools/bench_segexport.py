#!/usr/bin/env python3
"""Times ccdm_segexport (the launch export_predictions makes, all three outputs) against the torch path (F.interpolate bilinear +
argmax over the first K-1 channels + two table gathers) at the Cityscapes shapes of tools/bench_segeval.py: C4 (B = 16,
256x512 -> 1024x2048) and a C5 shard (B = 4, 512x1024 -> 1024x2048), K = 20.  Device events after warm-up; peak device memory of
one call above the inputs and the outputs.  Prints one JSON line per shape, with the kernel's achieved output bytes/s (5 bytes
per pixel: train id, label id, colour) to set against the HBM write rate.

    python tools/bench_segexport.py [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip, segmentation as SEG  # noqa: E402
from tools.bench_segeval import SHAPES, inputs, peak_above, timed  # noqa: E402


def torch_path(pred, size, C, idt, colt):
    t = F.interpolate(pred, size, mode="bilinear")[:, :C].argmax(1)
    return t.to(torch.uint8), idt[t], colt[t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lib, K, C = hip.load(), 20, 19
    idt = torch.tensor(SEG.TRAIN_ID_TO_ID, dtype=torch.uint8, device="cuda")
    colt = torch.tensor(SEG.TRAIN_ID_TO_COLOR, dtype=torch.uint8, device="cuda")
    for name, (B, h, w, H, W) in SHAPES.items():
        pred, _ = inputs(B, h, w, H, W)
        probs = pred.permute(0, 2, 3, 1)              # the channels-last memory the BCHW view shows
        train = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        ids = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        color = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def kernel():
            hip.check(lib.ccdm_segexport(probs.data_ptr(), K, None, B, h, w, H, W, K, C, idt.data_ptr(), colt.data_ptr(), train.data_ptr(),
                                         ids.data_ptr(), color.data_ptr(), stream), "segexport")
        out_bytes = B * H * W * 5
        res = {"shape": name, "B": B, "in": [h, w], "out": [H, W], "K": K, "out_bytes": out_bytes}
        res["kernel_us_median"], res["kernel_us_min"] = timed(kernel, a.iters, a.warmup)
        res["kernel_out_GBps"] = out_bytes / res["kernel_us_median"] * 1e-3
        res["kernel_peak_MB"] = peak_above(kernel) / 2 ** 20            # above the inputs and the preallocated outputs
        tp = lambda: torch_path(pred, (H, W), C, idt, colt)         # noqa: E731
        res["torch_us_median"], res["torch_us_min"] = timed(tp, max(3, a.iters // 4), 1)
        res["torch_peak_MB"] = (peak_above(tp) - out_bytes) / 2 ** 20
        want = tp()
        kernel()
        torch.cuda.synchronize()
        res["train_id_mismatches_vs_torch"] = int((want[0] != train).sum())     # near-ties only (fp32 expression order)
        print(json.dumps(res), flush=True)
        del pred, probs, train, ids, color, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
