#!/usr/bin/env python3
"""Times ccdm_lesions (the call metrics.lesion_stats makes: the labelling kernel and the pair kernel) at the LIDC shape: B = 4
images, S = 100 samples, L = 4 raters, 128 x 128, K = 2, connectivity 8, overlaps 0 and 1/2, and in the same run ccdm_surfdist on
the same maps as the yardstick.  The maps are those of tools/bench_surfdist.py (mostly background, a disc the samples and raters
disagree about) with a few specks per sample map, so that a map has several lesions.  The labels of a few maps are held against
scipy.ndimage.label first.  Device events after warm-up.  Prints one JSON line.

    python tools/bench_lesions.py [--iters 50] [--warmup 10] [--batch 4] [--samples 100]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=100)
    a = ap.parse_args()
    from bench_surfdist import inputs
    B, S, L, R, K = a.batch, a.samples, 4, 128, 2
    samples, raters = inputs(B, S, L, R)
    rng = np.random.default_rng(1)
    for b in range(B):
        for i in range(S):
            for _ in range(int(rng.integers(0, 4))):              # specks of 1 to 9 pixels: false-positive lesions
                y, x, h, w = (int(v) for v in (rng.integers(0, R - 3), rng.integers(0, R - 3), rng.integers(1, 4), rng.integers(1, 4)))
                samples[b, i, y:y + h, x:x + w] = 1

    import torch
    from scipy import ndimage
    from ccdm_stochastic_segmentation_amd import hip
    from bench_segeval import timed
    s_dev, r_dev = torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda()
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    ov = np.array([[0, 1], [1, 2]], dtype=np.int32)
    stats = torch.empty((B, S, L, 1, 6), dtype=torch.int32, device="cuda")
    need = int(lib.ccdm_lesions_workspace_bytes(B, S, L, R, R, K))
    ws = torch.empty(need // 4, dtype=torch.int32, device="cuda")

    def lesions():
        hip.check(lib.ccdm_lesions(s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, R, R, K, 8, ov.ctypes.data, 2, stats.data_ptr(), ws.data_ptr(),
                                   need, stream), "lesions")
    sd_stats = torch.empty((B, S, L, 1, 5), dtype=torch.int32, device="cuda")
    sd_sums = torch.empty((B, S, L, 1, 2), dtype=torch.float64, device="cuda")
    sd_need = int(lib.ccdm_surfdist_workspace_bytes(B, S, L, R, R, K))
    sd_ws = torch.empty(sd_need // 4, dtype=torch.int32, device="cuda")

    def surfdist():
        hip.check(lib.ccdm_surfdist(s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, R, R, K, 95, 100, sd_stats.data_ptr(), sd_sums.data_ptr(),
                                    sd_ws.data_ptr(), sd_need, stream), "surfdist")
    lesions()
    torch.cuda.synchronize()
    planes = ws[:B * (S + L) * R * R].reshape(B * (S + L), R, R).cpu().numpy()
    maps = np.concatenate([samples.reshape(-1, R, R), raters.reshape(-1, R, R)])
    for m in list(range(0, B * S, 37)) + list(range(B * S, B * (S + L))):
        want, _ = ndimage.label(maps[m] == 1, structure=np.ones((3, 3)))
        assert np.array_equal(planes[m], want), f"the labels of map {m} disagree with scipy"
    st = stats.cpu().numpy()
    res = {"B": B, "S": S, "L": L, "H": R, "W": R, "K": K, "connectivity": 8, "overlaps": ov.tolist(), "cells": B * S * L,
           "lesions_per_sample_map": float(st[..., 0].mean()), "lesions_per_rater_map": float(st[..., 1].mean()),
           "workspace_MB": need / 2 ** 20, "background_share": float((samples == 0).mean())}
    res["lesions_us_median"], res["lesions_us_min"] = timed(lesions, a.iters, a.warmup)
    res["surfdist_us_median"], res["surfdist_us_min"] = timed(surfdist, a.iters, a.warmup)
    res["lesions_us_median_again"], _ = timed(lesions, a.iters, a.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
