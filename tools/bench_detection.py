#!/usr/bin/env python3
"""Times ccdm_findings (the call metrics.sample_findings makes: the counting, labelling, bit and table kernels) at the LIDC shape: B = 16
images, S = 100 samples, L = 4 raters, 128 x 128, K = 2, connectivity 8, n_min = 10, m_min = 3, cap 64, with the confidence map, and
in the same process ccdm_lesions on the same stacks as the yardstick (it labels the same maps, once per sample and rater instead of
once per image).  The maps are those of tools/bench_lesions.py: mostly background, a disc the samples and raters disagree about, a few
specks per sample map.  The candidate labels of every image are held against scipy.ndimage.label first.  The two calls alternate over
`--rounds` rounds of `--iters` timed calls each (device events after warm-up); per call the median, the minimum and the 10th and 90th
percentile over all rounds.  Prints one JSON line.

    python tools/bench_detection.py [--iters 30] [--warmup 10] [--rounds 3] [--batch 16] [--samples 100]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=100)
    a = ap.parse_args()
    from bench_surfdist import inputs
    B, S, L, R, K, cap = a.batch, a.samples, 4, 128, 2, 64
    n_min, m_min = max(1, -(-S // 10)), L // 2 + 1
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
    s_dev, r_dev = torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda()
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    counts = torch.empty((B, 1, 2), dtype=torch.int32, device="cuda")
    cand = torch.empty((B, 1, cap, 12), dtype=torch.int32, device="cuda")
    ref = torch.empty((B, 1, cap, 4), dtype=torch.int32, device="cuda")
    conf = torch.empty((B, 1, R, R), dtype=torch.uint8, device="cuda")
    need = int(lib.ccdm_findings_workspace_bytes(B, S, L, R, R, K, cap))
    ws = torch.empty(need // 4, dtype=torch.int32, device="cuda")

    def findings():
        hip.check(lib.ccdm_findings(s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, R, R, K, 8, n_min, m_min, cap, counts.data_ptr(), cand.data_ptr(),
                                    ref.data_ptr(), conf.data_ptr(), ws.data_ptr(), need, stream), "findings")
    ov = np.array([[0, 1], [1, 2]], dtype=np.int32)
    les_stats = torch.empty((B, S, L, 1, 6), dtype=torch.int32, device="cuda")
    les_need = int(lib.ccdm_lesions_workspace_bytes(B, S, L, R, R, K))
    les_ws = torch.empty(les_need // 4, dtype=torch.int32, device="cuda")

    def lesions():
        hip.check(lib.ccdm_lesions(s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, R, R, K, 8, ov.ctypes.data, 2, les_stats.data_ptr(),
                                   les_ws.data_ptr(), les_need, stream), "lesions")
    findings()
    torch.cuda.synchronize()
    labels = ws[:B * 2 * R * R].reshape(B, 2, R, R).cpu().numpy()
    n = counts.cpu().numpy()
    for b in range(B):
        want, want_n = ndimage.label((samples[b] == 1).sum(axis=0) >= n_min, structure=np.ones((3, 3)))
        assert np.array_equal(labels[b, 0], want) and n[b, 0, 0] == want_n, f"the candidate labels of image {b} disagree with scipy"
    assert int(n.max()) <= cap, f"{int(n.max())} records, cap {cap}"

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
    times = {"findings": [], "lesions": []}
    for _ in range(a.rounds):                                     # alternating: both see the same neighbours on the machine
        times["findings"] += timed(findings)
        times["lesions"] += timed(lesions)
    res = {"B": B, "S": S, "L": L, "H": R, "W": R, "K": K, "connectivity": 8, "n_min": n_min, "m_min": m_min, "cap": cap,
           "candidates_per_image": float(n[..., 0].mean()), "reference_lesions_per_image": float(n[..., 1].mean()),
           "stack_MB": B * (S + L) * R * R / 2 ** 20, "workspace_MB": need / 2 ** 20, "lesions_workspace_MB": les_need / 2 ** 20,
           "timed_calls": a.rounds * a.iters}
    for name, t in times.items():
        t = sorted(t)
        res.update({f"{name}_us_median": t[len(t) // 2], f"{name}_us_min": t[0], f"{name}_us_p10": t[len(t) // 10],
                    f"{name}_us_p90": t[(9 * len(t)) // 10]})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
