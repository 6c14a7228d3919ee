#!/usr/bin/env python3
"""Launches ccdm_tiled_step beside ccdm_views_step at V = 4 on the same number of engine-row pixels, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <out> -- python tools/bench_tiles.py [--launches 200]

    tiled   4 canvases of 256x256, tiles 128x128 at strides (64, 64): R = 9, 36 engine rows of 128x128; c is 1, 2 or 4
    views   9 samples of 128x128, V = 4: 36 engine rows of 128x128

each at K = 2 (one thread per pixel, no xin) and at K = 20 with xin (the staged kernel), in STEP_SAMPLE at neutral shaping without
evidence.  The times are the trace's (k_tiled / k_tiled_staged against k_guided / k_guided_staged with VIEWS = true); this script only
prints what it launched, as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiles: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    lib = hip.load()
    rng = np.random.default_rng(1)
    h = w = 128
    Nt, Hc, Wc, sy, sx, R = 4, 256, 256, 64, 64, 9
    Nv, V = 9, 4
    rows = R * Nt
    assert rows == V * Nv
    stream = torch.cuda.current_stream(dev).cuda_stream
    al, cu = 0.98, 0.6
    for K, stride in ((2, 0), (20, 23)):
        r = (rng.random((rows, h * w, K)) + 0.5).astype(np.float32)
        x0 = torch.from_numpy(r / r.sum(-1, keepdims=True)).to(dev)
        xt = torch.from_numpy(rng.integers(0, K, (rows, h * w)).astype(np.uint8)).to(dev)
        cxt = torch.from_numpy(rng.integers(0, K, (Nt, Hc * Wc)).astype(np.uint8)).to(dev)
        xin = torch.zeros((rows, h * w, stride), device=dev) if stride else None
        xp = None if xin is None else xin.data_ptr()
        for i in range(a.launches):
            hip.check(lib.ccdm_tiled_step(x0.data_ptr(), None, Nt, Hc, Wc, h, w, sy, sx, K, 1.0, 1.0, al, cu, hip.STEP_SAMPLE, i % 250, 1, 0,
                                          cxt.data_ptr(), xt.data_ptr(), xp, stride, None, None, stream), "tiled_step")
            hip.check(lib.ccdm_views_step(x0.data_ptr(), None, Nv, h, w, K, V, (1 << 2) | (2 << 4) | (3 << 6), 1.0, 1.0, al, cu, hip.STEP_SAMPLE,
                                          i % 250, 1, 0, xt.data_ptr(), xp, stride, None, None, stream), "views_step")
        torch.cuda.synchronize(dev)
    print(json.dumps({"engine_rows": rows, "row": [h, w], "tiled": {"N": Nt, "canvas": [Hc, Wc], "strides": [sy, sx], "R": R},
                      "views": {"N": Nv, "V": V}, "launches_per_kernel_and_K": a.launches}), flush=True)


if __name__ == "__main__":
    main()
