#!/usr/bin/env python3
"""Times ccdm_csscore (the launch CityscapesScores.update makes) at the Cityscapes shapes of tools/bench_segeval.py, K = 20:
  csscore_us / csscore_inst_us   the fused call without and with instance ids (the clearing of its outputs included);
  ids_inst_us                    ccdm_csscore_ids with instance ids on the exported id image (no upsampling, no argmax);
  seg_confusion_us               ccdm_seg_confusion on the same shape: the yardstick for "one more pass of the same walk";
  torch_us / torch_inst_us       a torch device path: F.interpolate + argmax + table gather + bincount, and unique plus one mask
                                 per instance for the instance counts (what the script does, on the device);
  host_image_s                   the host restatement of the script's counting on ONE image on the CPU (np.unique over the encoded
                                 pair, one full-image mask per instance): the factor over the script's way.
Device events after warm-up, median and minimum; peak device memory of one call above the inputs.  One JSON line per shape.

    python tools/bench_csscore.py [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import cityscapes_scores as CS  # noqa: E402
from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from ccdm_stochastic_segmentation_amd import segmentation as SEG  # noqa: E402
from tools.bench_segeval import SHAPES, inputs, peak_above, timed  # noqa: E402

L = CS.NUM_LABELS


def targets(lab, seed=0):
    """Label ids and an instance image from bench_segeval's train-id labels (32 x 32 cells): a cell of a thing class is one
    instance with probability 3/4, numbered by its place in the image."""
    ids = torch.tensor(SEG.TRAIN_ID_TO_ID + (0,) * 236, dtype=torch.int32, device=lab.device)
    gt = ids[lab.long()]
    B, H, W = lab.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    cells = torch.arange((H // 32) * (W // 32), device=lab.device).reshape(H // 32, W // 32) % 997 + 1
    keep = torch.rand((B, H // 32, W // 32), generator=g, device=lab.device) < 0.75
    num = (cells[None] * keep).repeat_interleave(32, 1).repeat_interleave(32, 2)
    inst = torch.where((gt >= 24) & (num > 0), gt * 1000 + num, gt)
    return gt.to(torch.uint8).contiguous(), torch.where(inst > 32767, inst - 65536, inst).to(torch.int16).contiguous(), inst


def torch_path(pred, gt, inst, idt, C):
    up = F.interpolate(pred, tuple(gt.shape[1:]), mode="bilinear")[:, :C]
    pid = idt[up.argmax(1)]
    conf = torch.bincount(gt.reshape(-1).long() * L + pid.reshape(-1), minlength=L * L).reshape(L, L)
    out = []
    if inst is not None:
        for b in range(gt.shape[0]):
            for i in torch.unique(inst[b][inst[b] > 1000]).tolist():
                m = inst[b] == i
                out.append((m.sum(), (pid[b][m] == i // 1000).sum()))
        out = torch.tensor(out).cpu() if out else out
    return conf, out


def host_image(pid, gt, inst):
    """the script's counting of one image, restated: np.unique over the encoded pair, one mask per instance"""
    t0 = time.perf_counter()
    enc = gt.astype(np.int32) * 256 + pid
    values, cnt = np.unique(enc, return_counts=True)
    conf = np.zeros((L, L), np.int64)
    for v, c in zip(values, cnt):
        conf[v // 256, v % 256] += c
    n = 0
    for i in np.unique(inst[inst > 1000]):
        m = inst == i
        n += np.count_nonzero(m) + np.count_nonzero(pid[m] == i // 1000)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lib, K, C = hip.load(), 20, 19
    _, ign, cat, has, _ = CS.label_tables()
    idt, ign, cat, has = (torch.as_tensor(np.asarray(t, np.uint8)).cuda() for t in (SEG.TRAIN_ID_TO_ID, ign, cat, has))
    for name, (B, h, w, H, W) in SHAPES.items():
        pred, lab = inputs(B, h, w, H, W)
        gt, inst16, inst = targets(lab)
        probs = pred.permute(0, 2, 3, 1)              # the channels-last memory the BCHW view shows
        conf = torch.zeros((L, L), dtype=torch.int64, device="cuda")
        per_image = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        instances = torch.zeros((B, CS.INSTANCE_SLOTS, 3), dtype=torch.int32, device="cuda")
        unknown = torch.zeros(2, dtype=torch.int32, device="cuda")
        label_id = SEG.export_predictions(pred, (H, W), outputs=("label_id",))["label_id"]
        ws = torch.empty(lib.ccdm_seg_confusion_workspace_bytes(B, H, W, K), dtype=torch.uint8, device="cuda")
        hard = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        soft = torch.empty((C, C), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        tail = (L, ign.data_ptr(), cat.data_ptr(), has.data_ptr(), CS.INSTANCE_BASE, CS.INSTANCE_SLOTS, conf.data_ptr(), per_image.data_ptr(),
                instances.data_ptr(), unknown.data_ptr(), stream)

        def fused(i):
            return lambda: hip.check(lib.ccdm_csscore(probs.data_ptr(), K, None, B, h, w, H, W, K, idt.data_ptr(), gt.data_ptr(), i, *tail),
                                     "csscore")

        def ids():
            hip.check(lib.ccdm_csscore_ids(label_id.data_ptr(), B, H, W, gt.data_ptr(), inst16.data_ptr(), *tail), "csscore_ids")

        def confusion():
            hip.check(lib.ccdm_seg_confusion(probs.data_ptr(), K, None, lab.data_ptr(), B, h, w, H, W, K, hard.data_ptr(), soft.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream), "seg_confusion")
        res = {"shape": name, "B": B, "in": [h, w], "out": [H, W], "K": K}
        res["csscore_us_median"], res["csscore_us_min"] = timed(fused(None), a.iters, a.warmup)
        res["csscore_inst_us_median"], res["csscore_inst_us_min"] = timed(fused(inst16.data_ptr()), a.iters, a.warmup)
        res["ids_inst_us_median"], res["ids_inst_us_min"] = timed(ids, a.iters, a.warmup)
        res["seg_confusion_us_median"], res["seg_confusion_us_min"] = timed(confusion, a.iters, a.warmup)
        assert unknown.tolist() == [0, 0]
        res["instances"] = int((instances[:, :, 0] > 0).sum())
        res["csscore_peak_MB"] = (peak_above(fused(inst16.data_ptr())) + instances.numel() * 4) / 2 ** 20     # + the instance table, allocated above
        # bytes the pass must move per output pixel: ground truth 1, instance id 2, and the low-resolution prediction once
        res["bytes_per_pixel"] = 1 + 2 + 4 * K * (h * w) / (H * W)
        res["GBps_inst"] = res["bytes_per_pixel"] * B * H * W / (res["csscore_inst_us_median"] * 1e-6) / 1e9
        idl = idt.long()
        res["torch_us_median"], res["torch_us_min"] = timed(lambda: torch_path(pred, gt, None, idl, C), max(3, a.iters // 4), 1)
        res["torch_peak_MB"] = peak_above(lambda: torch_path(pred, gt, None, idl, C)) / 2 ** 20
        res["torch_inst_us_median"], res["torch_inst_us_min"] = timed(lambda: torch_path(pred[:1], gt[:1], inst[:1], idl, C), 3, 1)
        res["torch_inst_images"] = 1                    # the instance loop is timed on one image: it is per image
        res["host_image_s"] = host_image(label_id[0].cpu().numpy(), gt[0].cpu().numpy(), inst[0].cpu().numpy())
        print(json.dumps(res), flush=True)
        del pred, lab, ws, instances, label_id
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
