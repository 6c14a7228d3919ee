#!/usr/bin/env python3
"""Golden: what the reference's vendored official Cityscapes script (`evaluation/cs_eval.py`: `evaluateImgLists`) returns on a
small fixed-seed set of (prediction, ground truth, instance) images, in the reference's setting (evalInstLevelScore off) and with
instance-level scoring on, written as data only:
  tests/golden/cs_script_inputs.npz     pred_ids_<g>, gt_ids_<g> uint8 [B,H,W] and inst_ids_<g> uint16 [B,H,W] per group g of
                                        equally sized images; the script sees the images of all groups in order;
  tests/golden/cs_script_results.json   {"pixel": ..., "instance": ...}: both result dictionaries (NaN as null, perImageScores
                                        keyed by the image number), and "labels" / "categories" / "avgClassSize": the tables the
                                        script works from (the reference's evaluation/labels.py and the script's args).
tests/test_cityscapes_scores.py checks cityscapes_scores (tables and formulas written from the public label definition) and the
ccdm_csscore kernel against them.

    python tools/gen_goldens_cs_script.py <reference checkout>

The script imports `cityscapesscripts`, which need not be installed: stand-in modules are registered before it is loaded by path
(helpers.labels is the reference's own evaluation/labels.py, helpers.annotation a dummy, evaluation an empty module, so the script
takes its Python path).  Needs numpy, PIL and torch (the reference's transform is torch.as_tensor)."""
import importlib.util
import json
import math
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {"a": (2, 72, 96), "b": (1, 70, 90)}        # b: W % 4 != 0, H not a multiple of the kernel's 64-row tile


def load_script(ref):
    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    for name in ("cityscapesscripts", "cityscapesscripts.helpers", "cityscapesscripts.evaluation", "cityscapesscripts.helpers.annotation"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["cityscapesscripts.helpers.annotation"].Annotation = type("Annotation", (), {})
    labels = by_path("cityscapesscripts.helpers.labels", os.path.join(ref, "evaluation", "labels.py"))
    return by_path("cs_eval_reference", os.path.join(ref, "evaluation", "cs_eval.py")), labels


def make_images(labels):
    """Per group (pred_ids, gt_ids, inst_ids).  Ground truth: a grid of cells cycling through the evaluated labels, an ignored band
    (id 0) and an ignored patch (id 4), then thing instances as rectangles.  Prediction: the ground truth with rectangles of other
    evaluated labels painted over it, evaluated ids only."""
    rng = np.random.default_rng(20240917)
    evaluated = [l.id for l in labels.labels if l.id >= 0 and not l.ignoreInEval]
    no_instance = (31, 32)               # train, motorcycle: present as plain pixels, never as instances
    out = {}
    for g, (B, H, W) in GROUPS.items():
        gt = np.zeros((B, H, W), np.uint8)
        inst = np.zeros((B, H, W), np.uint16)
        pred = np.zeros((B, H, W), np.uint8)
        for b in range(B):
            cell = evaluated[b:] + evaluated[:b]
            for n in range(20):                                     # 5 x 4 cells, 19 labels and one repeated
                y0, x0 = (n // 5) * (H // 4), (n % 5) * (W // 5)
                y1, x1 = (H if n // 5 == 3 else y0 + H // 4), (W if n % 5 == 4 else x0 + W // 5)
                gt[b, y0:y1, x0:x1] = cell[n % 19]
            gt[b, :3, :] = 0                                        # ignored: unlabeled
            gt[b, H // 2:H // 2 + 5, 4:17] = 4                      # ignored: static
            inst[b] = gt[b]                                         # no instance: the instance image holds the label id
            things = [(24001, 5, 5, 12, 9), (24002, 30, 40, 9, 14), (25001, 50, 10, 10, 10), (26001, 8, 60, 15, 20),
                      (26002, 40, 70, 12, 12), (27001, 22, 20, 8, 16), (28001, 55, 45, 10, 18), (33001, 36, 3, 9, 9)]
            if g == "a" and b == 1:
                things = [(26001, 10, 10, 20, 25), (24001, 45, 50, 14, 10), (29001, 20, 60, 12, 16), (33002, 50, 5, 8, 8),
                          (25003, 5, 50, 7, 30), (25003, 60, 80, 8, 12)]        # 25003: two disjoint regions; 29001: caravan, ignored
            for iid, y0, x0, hh, ww in things:
                assert iid // 1000 not in no_instance
                gt[b, y0:y0 + hh, x0:x0 + ww] = iid // 1000
                inst[b, y0:y0 + hh, x0:x0 + ww] = iid
            p = gt[b].copy()
            p[np.isin(p, evaluated, invert=True)] = 7               # ignored ground truth is predicted as something evaluated
            paint = [l for l in evaluated if l != 31]                # train gets no false positive: its instance score is NaN
            for _ in range(14):
                y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
                p[y0:y0 + rng.integers(4, 16), x0:x0 + rng.integers(4, 24)] = paint[rng.integers(0, len(paint))]
            p[H - 6:H - 2, W - 20:W - 4] = 32                       # motorcycle does: its instance score is 0
            missed = things[1][0]                                   # one instance predicted as vegetation everywhere
            p[inst[b] == missed] = 21
            pred[b] = p
        out[g] = (pred, gt, inst)
    return out, evaluated, no_instance


def check_inputs(images, labels, evaluated, no_instance):
    ignored = [l.id for l in labels.labels if l.id >= 0 and l.ignoreInEval]
    all_gt = np.concatenate([v[1].ravel() for v in images.values()])
    all_pred = np.concatenate([v[0].ravel() for v in images.values()])
    assert set(evaluated) <= set(all_gt.tolist()), "every evaluated label in ground truth"
    assert (all_gt == 0).any() and np.isin(all_gt, [i for i in ignored if i]).any(), "ignored ground truth"
    assert set(all_pred.tolist()) <= set(evaluated), "predictions hold evaluated ids only"
    seen = {}
    missed = ignored_inst = split = False
    for g, (pred, gt, inst) in images.items():
        for b in range(pred.shape[0]):
            for iid in np.unique(inst[b][inst[b] > 1000]):
                m = inst[b] == iid
                seen.setdefault(int(iid), []).append((g, b))
                missed |= not (pred[b][m] == iid // 1000).any()
                ignored_inst |= int(iid) // 1000 in ignored
                rows = np.flatnonzero(m.any(1))
                split |= bool((np.diff(rows) > 1).any())
    assert missed and ignored_inst and split, (missed, ignored_inst, split)
    assert any(len(v) > 1 for v in seen.values()), "one instance id in two images"
    assert all(i // 1000 not in no_instance for i in seen) and set(no_instance) <= set(all_gt.tolist())
    B, H, W = GROUPS["b"]
    assert W % 4 != 0 and H % 64 != 0


def clean(x):
    if isinstance(x, dict):
        return {k: clean(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [clean(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return None if math.isnan(x) else float(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    return x


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    import torch
    from PIL import Image
    cs, labels = load_script(argv[1])
    images, evaluated, no_instance = make_images(labels)
    check_inputs(images, labels, evaluated, no_instance)
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        preds, gts = [], []
        for g, (pred, gt, inst) in images.items():
            for b in range(pred.shape[0]):
                stem = os.path.join(tmp, f"golden_{len(preds):06d}_000019")
                Image.fromarray(pred[b]).save(stem + "_pred.png")
                Image.fromarray(gt[b]).save(stem + "_gtFine_labelIds.png")
                Image.fromarray(inst[b]).save(stem + "_gtFine_instanceIds.png")          # uint16 -> a 16-bit PNG
                with Image.open(stem + "_gtFine_instanceIds.png") as im:
                    assert np.array_equal(np.array(im), inst[b])
                preds.append(stem + "_pred.png")
                gts.append(stem + "_gtFine_labelIds.png")
        for key, inst_level in (("pixel", False), ("instance", True)):
            a = cs.args
            a.evalInstLevelScore, a.evalPixelAccuracy, a.JSONOutput, a.quiet = inst_level, True, False, True
            res = cs.evaluateImgLists(preds, gts, a, lambda x: torch.as_tensor(x))
            res["perImageScores"] = {str(preds.index(k)): v for k, v in res["perImageScores"].items()}
            results[key] = clean(res)
    inst_scores = results["instance"]["classInstScores"]
    things = [l.name for l in labels.labels if l.hasInstances and not l.ignoreInEval]
    assert any(inst_scores[n] is None for n in things) and any(inst_scores[n] == 0.0 for n in things), inst_scores
    results["labels"] = [[l.name, l.id, l.trainId, l.category, bool(l.hasInstances), bool(l.ignoreInEval)] for l in labels.labels]
    results["categories"] = list(labels.category2labels.keys())
    results["avgClassSize"] = dict(cs.args.avgClassSize)
    results["source"] = "evaluation/cs_eval.py: evaluateImgLists (evalPixelAccuracy on; pixel: evalInstLevelScore off, instance: on)"
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "cs_script_inputs.npz"),
                        **{f"{n}_{g}": v for g, t in images.items() for n, v in zip(("pred_ids", "gt_ids", "inst_ids"), t)})
    with open(os.path.join(gold, "cs_script_results.json"), "w") as f:
        json.dump(results, f, indent=None, separators=(",", ":"), allow_nan=False)
        f.write("\n")
    print("wrote", [(n, os.path.getsize(os.path.join(gold, n))) for n in ("cs_script_inputs.npz", "cs_script_results.json")])


if __name__ == "__main__":
    main(sys.argv)
