#!/usr/bin/env python3
"""Times ccdm_surfdist (the call metrics.surface_distance_stats makes: both transform kernels and the pair kernel) at the LIDC
shape: B = 4 images, S = 100 samples, L = 4 raters, 128 x 128, K = 2, against the host path a user would otherwise take for the
same cells: per (sample, rater) pair two scipy.ndimage.distance_transform_edt calls on the surfaces (as MedPy's hd95 / assd do),
spread over a pool of worker processes.  Maps like LIDC's: mostly background, a disc the samples and raters disagree about.  The
host path runs first, before the GPU is opened; a sample of its cells is held against the kernel's.  Device events after warm-up.
Prints one JSON line.

    python tools/bench_surfdist.py [--iters 30] [--warmup 5] [--batch 4] [--samples 100] [--workers 16]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(B, S, L, R, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:R, 0:R]
    cy, cx, rad = rng.uniform(40, 88, (B, 1, 1, 1)), rng.uniform(40, 88, (B, 1, 1, 1)), rng.uniform(6, 20, (B, 1, 1, 1))
    d2 = (yy - cy + rng.uniform(-3, 3, (B, S, 1, 1))) ** 2 + (xx - cx) ** 2
    samples = (d2 <= (rad * rng.uniform(0.6, 1.3, (B, S, 1, 1))) ** 2).astype(np.uint8)
    raters = (d2[:, :L] <= (rad * rng.uniform(0.6, 1.3, (B, L, 1, 1))) ** 2).astype(np.uint8)
    return samples, raters


def host_image(args):
    """the cells of one (image, sample) row on the host: [L][7] = n_ar, n_ra, d2_max, hd95, sum_ar, sum_ra, defined"""
    from scipy import ndimage
    a, raters = args
    out = np.zeros((raters.shape[0], 7))
    for j, r in enumerate(raters):
        ma, mr = a == 1, r == 1
        sa, sr = ma & ~ndimage.binary_erosion(ma), mr & ~ndimage.binary_erosion(mr)
        if not sa.any() or not sr.any():
            out[j, :2] = sa.sum(), sr.sum()
            continue
        d_ar, d_ra = ndimage.distance_transform_edt(~sr)[sa], ndimage.distance_transform_edt(~sa)[sr]
        pooled = np.concatenate([d_ar, d_ra])
        out[j] = d_ar.size, d_ra.size, round(float(pooled.max()) ** 2), np.percentile(pooled, 95), d_ar.sum(), d_ra.sum(), 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    B, S, L, R, K = a.batch, a.samples, 4, 128, 2
    samples, raters = inputs(B, S, L, R)
    res = {"B": B, "S": S, "L": L, "H": R, "W": R, "K": K, "cells": B * S * L, "host_workers": a.workers}

    jobs = [(samples[b, i], raters[b]) for b in range(B) for i in range(S)]
    with ProcessPoolExecutor(max_workers=a.workers) as pool:
        list(pool.map(host_image, jobs[:a.workers]))                 # the workers are up and scipy is imported
        t0 = time.perf_counter()
        host = np.stack(list(pool.map(host_image, jobs, chunksize=max(1, len(jobs) // (4 * a.workers))))).reshape(B, S, L, 7)
        res["host_scipy_ms"] = (time.perf_counter() - t0) * 1e3

    import torch
    from ccdm_stochastic_segmentation_amd import hip
    from ccdm_stochastic_segmentation_amd import metrics as M
    from bench_segeval import timed
    s_dev, r_dev = torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda()
    lib = hip.load()
    stats = torch.empty((B, S, L, 1, 5), dtype=torch.int32, device="cuda")
    sums = torch.empty((B, S, L, 1, 2), dtype=torch.float64, device="cuda")
    need = int(lib.ccdm_surfdist_workspace_bytes(B, S, L, R, R, K))
    ws = torch.empty(need // 4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        hip.check(lib.ccdm_surfdist(s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, R, R, K, 95, 100, stats.data_ptr(), sums.data_ptr(),
                                    ws.data_ptr(), need, stream), "surfdist")
    kernel()
    got = M.surface_distance_stats(s_dev, r_dev, K)
    defined = host[..., 6] > 0
    assert np.array_equal(got["n_ar"][..., 0], host[..., 0]) and np.array_equal(got["n_ra"][..., 0], host[..., 1]), "surface sizes disagree"
    assert np.array_equal(got["d2_max"][..., 0], host[..., 2]), "the maxima disagree"
    t = 95 * (got["n_ar"] + got["n_ra"] - 1)
    hd95 = (np.sqrt(got["d2_lo"]) + (t % 100) / 100 * (np.sqrt(got["d2_hi"]) - np.sqrt(got["d2_lo"])))[..., 0]
    assert np.allclose(hd95[defined], host[..., 3][defined], rtol=1e-12, atol=0), "HD95 disagrees"
    assert np.allclose(got["sum_ar"][..., 0], host[..., 4], rtol=1e-12) and np.allclose(got["sum_ra"][..., 0], host[..., 5], rtol=1e-12)
    res["cells_defined"] = int(defined.sum())
    res["workspace_MB"] = need / 2 ** 20
    res["kernel_us_median"], res["kernel_us_min"] = timed(kernel, a.iters, a.warmup)
    res["host_over_kernel"] = res["host_scipy_ms"] * 1e3 / res["kernel_us_median"]
    res["background_share"] = float((samples == 0).mean())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
