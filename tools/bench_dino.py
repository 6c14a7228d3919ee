#!/usr/bin/env python3
"""Timing of the DINO ViT key-feature extractor on synthetic weights: ms per batch and per image and achieved
TFLOP/s (2 flops per multiply-add of the linear layers and the attention products of blocks 0..10 plus block 11's norm1/qkv).
--model picks the ViT (dino_vits8, dino_vits16, dino_vitb8, dino_vitb16), --stride the patch stride (default: the patch size;
any divisor of it gives overlapping patches), --sizes the N x H x W cases."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ccdm_stochastic_segmentation_amd.dino import VIT_CONFIGS, DinoViT, make_synthetic_vit_state_dict, token_grid

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="dino_vits8", choices=sorted(VIT_CONFIGS))
ap.add_argument("--stride", type=int, default=None)
ap.add_argument("--sizes", default="8x256x512,64x128x128,1x256x512", help="comma-separated NxHxW")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--no-breakdown", action="store_true", help="skip the per-kind breakdown of the first size")
args = ap.parse_args()
cfg = VIT_CONFIGS[args.model]
stride = args.stride or cfg["patch"]
sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]

DEV = torch.device("cuda:0")
enc = DinoViT(args.model, False, "concat_pixels_concat_features", stride=stride, state_dict=make_synthetic_vit_state_dict(args.model, 0))


def macs_per_token(T: int) -> float:
    d, p, r, depth = cfg["dim"], cfg["patch"], cfg["mlp_ratio"], cfg["depth"]
    lin = (depth - 1) * (d * 3 * d + d * d + 2 * d * r * d) + d * 3 * d + 3 * p * p * d
    att = (depth - 1) * 2 * T * d                                             # QK^T and PV
    return lin + att


for (N, H, W) in sizes:
    x = torch.randn((N, 3, H, W), device=DEV)
    for _ in range(2):
        enc(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        enc(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.iters
    h0, w0 = token_grid(H, W, cfg["patch"], stride)
    T = 1 + h0 * w0
    flops = 2.0 * N * T * macs_per_token(T)
    print(f"{args.model} stride {stride} N={N} {H}x{W} (T={T}): {ms:8.2f} ms per batch, {ms / N:7.2f} ms per image, "
          f"{flops / ms / 1e9:7.1f} TFLOP/s")

if args.no_breakdown:
    sys.exit(0)

# where the time goes (the first size): rocprofv3-free breakdown with events around each kind of launch
import collections
acc = collections.defaultdict(float)
ext = enc.extractor
orig = {k: getattr(ext, k) for k in ("_linear", "_layernorm", "_gelu", "_attention")}


def timed(name):
    def f(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = orig[name](*a, **k)
        e1.record()
        torch.cuda.synchronize()
        acc[name] += e0.elapsed_time(e1)
        return r
    return f


for k in orig:
    setattr(ext, k, timed(k))
N, H, W = sizes[0]
enc(torch.randn((N, 3, H, W), device=DEV))
print(f"breakdown, {N} x {H}x{W} (ms):", {k: round(v, 2) for k, v in acc.items()})
