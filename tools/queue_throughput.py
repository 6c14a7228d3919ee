#!/usr/bin/env python3
"""What continuous batching buys a service that gets small requests: samples/s of a stream of 8-sample requests through a
serving.SamplingQueue against the same requests as closed calls, in one run.  LIDC network, 128x128, K = 2, T = 250, synthetic weights.

    queue             (a) `--requests` requests of `--request-size` samples, all submitted up front to a queue of capacity `--capacity`
                          (the slots stay full: a walk that ends is replaced the next tick), run until idle, every result waited for
    solo_throughput   (b) the same requests as sequential model(x, image) calls at batch 8, slicing = "throughput" (the default) ...
    solo_latency          ... and slicing = "latency" (more, shorter workgroups per sample: the mode made for small batches)
    guided_64         (c) the same number of samples as model(x, image, temperature=1.0) calls at batch `--capacity`: per step the
                          launch sequence of a queue tick — the network to x0, then one step launch
    guided_64_one_stream  (c) pinned to one stream (substreams = 1), as the queue runs: what is left of the gap between (a) and this one is
                          the queue's own (the uploads, the per-slot parameters), the rest of (a) against (c) is the second stream
    plain_64          (d) the plain call at batch `--capacity`: the fused head, and the execution mode the model picks for it

Host clock around windows that end in a device synchronise, after one untimed window per variant; the variants alternate inside every
repetition, in rotating order.  Per variant: samples/s of every repetition, their median and spread ((max - min) / median).  Acceptance:
(a) exceeds both forms of (b) by more than the larger of their spreads.  The gap between (a) and (c) is the price of the table upload and
the per-slot parameters (and of one stream where the guided call takes two sub-batch streams); the gap between (c) and (d) is the price
of the unfused step that every guided call already pays.

`--guided`: the annotator-in-the-loop form of the same question, on the same windows.  Every request carries an evidence map, a
known-label map that covers a quarter of the pixels and temperature = 0.7:
    guided_queue      the requests through a queue built with guided=True (every tick's step is ccdm_slots_guided_step)
    guided_solo       the same requests as closed calls model(x, image, evidence=, known_labels=, temperature=0.7) at batch 8
    guided_solo_64    the same samples and guidance as closed calls at batch `--capacity`: per step the launches a guided tick fuses —
                      the network to x0, the shaped step (k_guided), the clamp (k_known_labels_step) — at the queue's batch
    guided_solo_64_one_stream   the same pinned to one stream (substreams = 1), as the queue runs: its two step kernels run on all
                      `--capacity` rows at once, the launches to hold ccdm_slots_guided_step's time against in a kernel trace
    queue             the plain queue on the same images without the guidance, in the same run: what the guidance costs a queue
Acceptance there: guided_queue exceeds guided_solo by more than the latter's spread.

Prints one JSON line.

`--only a,b` runs those variants alone (a kernel trace of one variant: rocprofv3 --kernel-trace --stats -- python tools/queue_throughput.py
--only queue --requests 8 --steps 50, then tools/trace_gaps.py on its output); the comparisons that need a missing variant are left out.

    python tools/queue_throughput.py [--requests 16] [--request-size 8] [--capacity 64] [--reps 3] [--steps 250] [--only queue,guided_64] [--guided]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=16)
    ap.add_argument("--request-size", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=250, help="rows of every walk (< T: strided)")
    ap.add_argument("--only", default="", help="comma-separated variants to run (default: all)")
    ap.add_argument("--guided", action="store_true", help="guided requests: guided_queue against guided_solo and the plain queue")
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("queue_throughput: at least three repetitions (a variant's own spread has to be known)")
    if (a.requests * a.request_size) % a.capacity:
        raise SystemExit("queue_throughput: requests * request-size must be a multiple of the capacity (the batch-64 variants draw as many samples)")
    if not torch.cuda.is_available():
        raise SystemExit("queue_throughput: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    K, H, W, T = 2, 128, 128, 250
    bp = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
    model = build_model(T, "cosine", {"s": 0.008}, [(1, H, W), (K, H, W)], (1, H, W), "unet_openai", bp, "datasets.lidc", "majority", None)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}, strict=True)
    model = model.to(dev).eval()
    model.philox_seed = 1
    rng = np.random.default_rng(0)
    total = a.requests * a.request_size
    image = torch.from_numpy(rng.uniform(-1, 1, (total, 1, H, W)).astype(np.float32)).to(dev)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (total, H, W))), K).permute(0, 3, 1, 2).float().contiguous().to(dev)
    t = 10000 + a.steps if a.steps < T else None
    tt = None if t is None else torch.as_tensor(t)
    n, cap = a.request_size, a.capacity
    queue = model.sampling_queue(cap, (1, H, W))

    def run_queue():
        rs = [queue.submit(image[i:i + n], x=x[i:i + n], t=t) for i in range(0, total, n)]
        queue.run_until_idle()
        return [r.result()["diffusion_out"] for r in rs]

    def run_solo(slicing):
        def run():
            model.slicing = slicing
            try:
                return [model(x[i:i + n], image[i:i + n], t=tt)["diffusion_out"] for i in range(0, total, n)]
            finally:
                model.slicing = "throughput"
        return run

    def run_batch(substreams=0, **kw):
        def run():
            model.substreams = substreams
            try:
                return [model(x[i:i + cap], image[i:i + cap], t=tt, **kw)["diffusion_out"] for i in range(0, total, cap)]
            finally:
                model.substreams = 0
        return run

    # --guided: per sample an evidence map (weights in [0.05, 1]) and a known-label map that covers a quarter of the pixels; host tensors,
    # as a caller has them (the model's checks read them on the host either way)
    if a.guided:
        evidence = torch.from_numpy(rng.uniform(0.05, 1.0, (total, K, H, W)).astype(np.float32))
        labels = torch.from_numpy(rng.integers(0, K, (total, H, W)))
        known = torch.where(torch.from_numpy(rng.random((total, H, W)) < 0.25), labels, torch.full_like(labels, 255))
        guided_queue = model.sampling_queue(cap, (1, H, W), guided=True)

    def guidance(i, size=None):
        size = size or n
        return dict(evidence=evidence[i:i + size], known_labels=known[i:i + size], temperature=0.7)

    def run_guided_queue():
        rs = [guided_queue.submit(image[i:i + n], x=x[i:i + n], t=t, **guidance(i)) for i in range(0, total, n)]
        guided_queue.run_until_idle()
        return [r.result()["diffusion_out"] for r in rs]

    def run_guided_solo():
        return [model(x[i:i + n], image[i:i + n], t=tt, **guidance(i))["diffusion_out"] for i in range(0, total, n)]

    def run_guided_solo_64(substreams=0):
        def run():
            model.substreams = substreams
            try:
                return [model(x[i:i + cap], image[i:i + cap], t=tt, **guidance(i, cap))["diffusion_out"] for i in range(0, total, cap)]
            finally:
                model.substreams = 0
        return run

    variants = {"queue": run_queue, "solo_throughput": run_solo("throughput"), "solo_latency": run_solo("latency"),
                "guided_64": run_batch(temperature=1.0), "guided_64_one_stream": run_batch(1, temperature=1.0), "plain_64": run_batch()}
    if a.guided:
        variants = {"guided_queue": run_guided_queue, "guided_solo": run_guided_solo, "guided_solo_64": run_guided_solo_64(),
                    "guided_solo_64_one_stream": run_guided_solo_64(1), "queue": run_queue}
    if a.only:
        unknown = [v for v in a.only.split(",") if v not in variants]
        if unknown:
            raise SystemExit(f"queue_throughput: unknown variant(s) {unknown}; known: {list(variants)}")
        variants = {k: v for k, v in variants.items() if k in a.only.split(",")}
    modes = {}
    for name, fn in variants.items():                        # untimed: engines, graph capture, the plain call's mode calibration
        fn()
        torch.cuda.synchronize(dev)
        modes[name] = None if name in ("queue", "guided_queue") else list(model.last_mode)
    rate = {name: [] for name in variants}
    order = list(variants)
    for _ in range(a.reps):
        for name in order:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            variants[name]()
            torch.cuda.synchronize(dev)
            rate[name].append(total / (time.perf_counter() - t0))
        order = order[1:] + order[:1]
    med = {k: float(np.median(v)) for k, v in rate.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in rate.items()}
    res = {"shape": {"K": K, "size": [H, W], "steps": a.steps, "requests": a.requests, "request_size": n, "capacity": cap},
           "reps": a.reps, "mode_streams_graph": modes, "queue_stats": dict(queue.stats),
           **({"guided_queue_stats": dict(guided_queue.stats)} if a.guided else {}),
           "samples_per_s": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2), "spread": round(spread[k], 4),
                                 "all": [round(r, 2) for r in v]} for k, v in rate.items()}}
    for num, den in (("queue", "solo_throughput"), ("queue", "solo_latency"), ("queue", "guided_64"), ("queue", "guided_64_one_stream"),
                     ("guided_64", "plain_64"), ("guided_queue", "guided_solo"), ("guided_queue", "guided_solo_64"),
                     ("guided_queue", "guided_solo_64_one_stream"),
                     ("guided_queue", "queue")):
        if num in med and den in med:
            res[f"{num}_over_{den}"] = round(med[num] / med[den], 4)
    if all(k in med for k in ("queue", "solo_throughput", "solo_latency")):
        b_best = max(med["solo_throughput"], med["solo_latency"])
        b_spread = max(spread["solo_throughput"], spread["solo_latency"])
        res["accepted"] = bool(med["queue"] > b_best * (1.0 + b_spread))
    if "guided_queue" in med and "guided_solo" in med:
        res["accepted"] = bool(med["guided_queue"] > med["guided_solo"] * (1.0 + spread["guided_solo"]))
    if "queue" in med and "guided_64" in med:
        res["queue_short_of_guided_64_by_more_than_its_spread"] = bool(med["queue"] < med["guided_64"] * (1.0 - spread["guided_64"]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
