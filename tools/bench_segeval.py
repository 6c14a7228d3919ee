#!/usr/bin/env python3
"""Times ccdm_seg_confusion (the launch pair SegmentationConfusion.update makes) against the torch path of the reference's evaluator
(F.interpolate bilinear + argmax + bincount for the hard matrix + the [C,NHW] x [NHW,C] matmul of update_cm) at the
Cityscapes shapes: C4 (B = 16, 256x512 -> 1024x2048) and a C5 shard (B = 4, 512x1024 -> 1024x2048), K = 20.
Device events after warm-up; peak device memory of one call above the inputs.  Prints one JSON line per shape.

    python tools/bench_segeval.py [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402

SHAPES = {"C4": (16, 256, 512, 1024, 2048), "C5_shard": (4, 512, 1024, 1024, 2048)}


def inputs(B, h, w, H, W, K=20, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.rand((B, h, w, K), generator=g, device="cuda") ** 4
    p = p / p.sum(-1, keepdim=True)
    coarse = torch.randint(0, 21, (B, H // 32, W // 32), generator=g, device="cuda")
    lab = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)
    lab = torch.where(lab == 20, torch.full_like(lab, 255), lab).to(torch.uint8)
    return p.permute(0, 3, 1, 2), lab


def torch_path(pred, lab, C):
    up = F.interpolate(pred, tuple(lab.shape[1:]), mode="bilinear")[:, :C]
    t = lab.reshape(-1).long()
    m = t < C
    hard = torch.bincount(t[m] * C + up.argmax(1).reshape(-1)[m], minlength=C * C).reshape(C, C)
    p = up.transpose(1, 0).reshape(C, -1)
    oh = F.one_hot(torch.where(m, t, torch.full_like(t, C)), C + 1)[:, :C].float()
    soft = (p @ oh).to(torch.int)
    return hard, soft


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0]


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for name, (B, h, w, H, W) in SHAPES.items():
        pred, lab = inputs(B, h, w, H, W)
        lib, K, C = hip.load(), 20, 19
        probs = pred.permute(0, 2, 3, 1)              # the channels-last memory the BCHW view shows
        ws = torch.empty(lib.ccdm_seg_confusion_workspace_bytes(B, H, W, K), dtype=torch.uint8, device="cuda")
        hard = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        soft = torch.empty((C, C), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def kernel():
            hip.check(lib.ccdm_seg_confusion(probs.data_ptr(), K, None, lab.data_ptr(), B, h, w, H, W, K, hard.data_ptr(), soft.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream), "seg_confusion")
        res = {"shape": name, "B": B, "in": [h, w], "out": [H, W], "K": 20}
        res["kernel_us_median"], res["kernel_us_min"] = timed(kernel, a.iters, a.warmup)
        res["kernel_peak_MB"] = (peak_above(kernel) + ws.numel()) / 2 ** 20      # + the workspace, allocated above
        tp = lambda: torch_path(pred, lab, 19)         # noqa: E731
        res["torch_us_median"], res["torch_us_min"] = timed(tp, max(3, a.iters // 4), 1)
        res["torch_peak_MB"] = peak_above(tp) / 2 ** 20
        print(json.dumps(res), flush=True)
        del pred, lab, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
