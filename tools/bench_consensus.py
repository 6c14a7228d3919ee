#!/usr/bin/env python3
"""Times the two entry points behind metrics.sample_consensus, ccdm_consensus (counting, histogram and selection kernels) and
ccdm_consensus_maps (mask and label), at two shapes: the LIDC shape B = 2 images, S = 100 samples, 128 x 128, K = 2 (mostly background,
a disc the samples disagree about, a share of empty samples per image) and a Cityscapes-like one, B = 4, S = 16, 128 x 256, K = 20
(noisy copies of three random block maps per image).  In the same process ccdm_modes_distance on the same stack is the yardstick: the
other summary of the sample set, O(S^2 HW) where the consensus is O(S HW).  The frequency planes are held against numpy first.  The three
calls alternate over `--rounds` rounds of `--iters` timed calls each (device events after warm-up); per call the median, the minimum and
the 10th and 90th percentile over all rounds.  Prints one JSON line per shape.

    python tools/bench_consensus.py [--iters 50] [--warmup 10] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lidc_stack(B, S, H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        empty = (0.1, 0.5)[b % 2]
        cy, cx, r0 = rng.uniform(H / 4, 3 * H / 4), rng.uniform(W / 4, 3 * W / 4), rng.uniform(H / 16, H / 6)
        for s in range(S):
            if rng.random() >= empty:
                r = r0 * rng.uniform(0.5, 1.6)
                out[b, s] = (yy - cy - rng.normal(0, 2)) ** 2 + (xx - cx - rng.normal(0, 2)) ** 2 <= r * r
    return out


def block_stack(B, S, H, W, K, seed=0):
    rng = np.random.default_rng(seed)
    out = np.empty((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        bases = np.kron(rng.integers(0, K, (3, H // 16, W // 16)), np.ones((16, 16), dtype=np.int64))
        for s in range(S):
            m = bases[rng.integers(0, 3)].copy()
            noise = rng.random((H, W)) < 0.1
            m[noise] = rng.integers(0, K, int(noise.sum()))
            out[b, s] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import torch
    from ccdm_stochastic_segmentation_amd import hip
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]

    for name, samples, K in (("lidc", lidc_stack(2, 100, 128, 128), 2), ("cityscapes_like", block_stack(4, 16, 128, 256, 20), 20)):
        B, S, H, W = samples.shape
        HW, C = H * W, K - 1
        dev = torch.from_numpy(samples).cuda().reshape(B, S, HW)
        freq = torch.empty((B, C, HW), dtype=torch.uint8, device="cuda")
        curve = torch.empty((B, C, 2, S + 1), dtype=torch.int64, device="cuda")
        best = torch.empty((B, C, 2), dtype=torch.int32, device="cuda")
        mask = torch.empty((B, C, HW), dtype=torch.uint8, device="cuda")
        label = torch.empty((B, HW), dtype=torch.uint8, device="cuda")
        need = int(lib.ccdm_consensus_workspace_bytes(B, S, HW, K))
        ws = torch.empty(need // 4, dtype=torch.int32, device="cuda")
        modes_ws = torch.empty((B, S, S, K), dtype=torch.int32, device="cuda")
        Q = torch.empty((B, S, S), dtype=torch.int32, device="cuda")

        def consensus():
            hip.check(lib.ccdm_consensus(dev.data_ptr(), B, S, HW, K, freq.data_ptr(), curve.data_ptr(), best.data_ptr(), ws.data_ptr(), need,
                                         stream), "consensus")

        def maps():
            hip.check(lib.ccdm_consensus_maps(freq.data_ptr(), best.data_ptr(), B, S, HW, K, 0, mask.data_ptr(), label.data_ptr(), stream),
                      "consensus_maps")

        def modes_distance():
            hip.check(lib.ccdm_modes_distance(dev.data_ptr(), B, S, HW, K, modes_ws.data_ptr(), Q.data_ptr(), stream), "modes_distance")
        consensus()
        maps()
        torch.cuda.synchronize()
        want = np.stack([(samples == k).sum(axis=1) for k in range(1, K)], axis=1).reshape(B, C, HW)
        assert np.array_equal(freq.cpu().numpy(), want), "the frequency planes disagree with numpy"
        thr = best[:, :, 0].cpu().numpy()
        assert np.array_equal(mask.cpu().numpy(), (want >= thr[:, :, None]).astype(np.uint8)), "the masks disagree with numpy"
        times = {"consensus": [], "consensus_maps": [], "modes_distance": []}
        for _ in range(a.rounds):                                 # alternating: all see the same neighbours on the machine
            times["consensus"] += timed(consensus)
            times["consensus_maps"] += timed(maps)
            times["modes_distance"] += timed(modes_distance)
        res = {"shape": name, "B": B, "S": S, "H": H, "W": W, "K": K, "stack_MB": samples.size / 2 ** 20, "workspace_MB": need / 2 ** 20,
               "iou_thresholds_over_S": [round(float(v), 3) for v in (thr.astype(np.float64) / S).mean(axis=1)],
               "majority_over_S": (S // 2 + 1) / S, "timed_calls": a.rounds * a.iters}
        for key, t in times.items():
            t = sorted(t)
            res.update({f"{key}_us_median": t[len(t) // 2], f"{key}_us_min": t[0], f"{key}_us_p10": t[len(t) // 10],
                        f"{key}_us_p90": t[(9 * len(t)) // 10]})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
