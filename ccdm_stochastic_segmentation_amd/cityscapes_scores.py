"""The scores of the official Cityscapes pixel-level evaluation script — what the reference's `run_inference` gets from its vendored
copy (`evaluation/cs_eval.py`: `evaluateImgLists`) and writes as `cs_script_results.json` — from counts made on the device.

    CityscapesScores(num_classes, device)   the accumulator: update() makes one HIP launch per batch (ccdm_csscore: label-id
                                            confusion matrix, per-image pixel counts, per-instance counts; no full-resolution
                                            tensor), result() is the script's result dictionary
    scores_from_counts(...)                 the float part: a plain fp64 restatement of the script's IoU, instance-weighted IoU
                                            (iIoU), prior and average formulas on exact integer counts

The label, category and average-instance-size tables below are the public Cityscapes label definition (cityscapesScripts,
helpers/labels.py and evaluation/evalPixelLevelSemanticLabeling.py); tests/golden/cs_script_results.json pins them."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .segmentation import (CITYSCAPES_LABELS, NUM_CLASSES, TRAIN_ID_TO_ID, _check_num_classes, _cuda_device, _labels_u8,
                           prediction_args, prediction_form)

# ------------------------------------------------------------------------------------------------ label definition
# The category column of the public definition, one per row of segmentation.CITYSCAPES_LABELS, in the order the categories first
# appear (the order of the script's category2labels).
CATEGORIES: Tuple[str, ...] = ("void", "flat", "construction", "object", "nature", "sky", "human", "vehicle")
_CATEGORY_OF_ROW = (0,) * 7 + (1,) * 4 + (2,) * 6 + (3,) * 4 + (4,) * 2 + (5,) + (6,) * 2 + (7,) * 9
assert len(_CATEGORY_OF_ROW) == len(CITYSCAPES_LABELS)
_THINGS = ("person", "rider", "car", "truck", "bus", "caravan", "trailer", "train", "motorcycle", "bicycle")      # hasInstances
# (name, id, train id, category, hasInstances, ignoreInEval): a label is ignored in evaluation exactly when it has no train id
CS_LABELS: Tuple[Tuple[str, int, int, str, bool, bool], ...] = tuple(
    (n, i, t, CATEGORIES[c], n in _THINGS, t == 255) for (n, i, t), c in zip(CITYSCAPES_LABELS, _CATEGORY_OF_ROW))
# mean instance size in pixels per class over the training set (the script's args.avgClassSize)
AVG_CLASS_SIZE: Dict[str, float] = {
    "bicycle": 4672.3249222261, "caravan": 36771.8241758242, "motorcycle": 6298.7200839748, "rider": 3930.4788056518,
    "bus": 35732.1511111111, "train": 67583.7075812274, "car": 12794.0202738185, "person": 3462.4756337644,
    "truck": 27855.1264367816, "trailer": 16926.9763313609,
}
NUM_LABELS = 34                 # label ids 0..33 (license plate has id -1 and never appears in an image)
INSTANCE_BASE = 24000           # instance ids are label id * 1000 + running number; labels 24..33 have instances:
INSTANCE_SLOTS = 10000          # instance id i of an image lives in slot i - INSTANCE_BASE, 24000 <= i < 34000
PER_IMAGE_FIELDS = ("nbNotIgnoredPixels", "nbCorrectPixels", "nbEvaluatedPixels", "nbEvaluatedCorrectPixels")


def label_tables(labels: Sequence[Tuple] = CS_LABELS):
    """(names [L], ignore_in_eval uint8 [L], category uint8 [L], has_instances uint8 [L], category names) for the label ids
    0..L-1 of `labels` (rows with a negative id have no place in an image and are left out)."""
    rows = sorted((r for r in labels if r[1] >= 0), key=lambda r: r[1])
    if [r[1] for r in rows] != list(range(len(rows))):
        raise ValueError("label ids must be 0..L-1 without gaps")
    cats: List[str] = []
    for r in labels:                    # order of first appearance, rows without an id included (the script's category2labels)
        if r[3] not in cats:
            cats.append(r[3])
    return ([r[0] for r in rows], np.array([r[5] for r in rows], np.uint8), np.array([cats.index(r[3]) for r in rows], np.uint8),
            np.array([r[4] for r in rows], np.uint8), cats)


# ------------------------------------------------------------------------------------------------ the script's formulas
def _ratio(tp, fp, fn) -> float:
    denom = tp + fp + fn            # the script's order: (tp + fp) + fn, which matters for the weighted (float) form
    return float("nan") if denom == 0 else float(tp) / denom


def _average(scores: Dict[str, float]) -> float:
    valid = [v for v in scores.values() if not math.isnan(v)]
    total = 0.0
    for v in valid:
        total += v
    return total / len(valid) if valid else float("nan")


def scores_from_counts(conf, per_image: Sequence[Sequence[int]], instances: Sequence[Tuple[int, int, int, int, int]],
                       names: Optional[Sequence] = None, labels: Sequence[Tuple] = CS_LABELS,
                       avg_class_size: Optional[Dict[str, float]] = None) -> Dict[str, object]:
    """The script's result dictionary (`createResultDict`) from exact counts, in fp64:
      conf        [L][L] integers, rows = ground-truth label id, columns = predicted label id, every pixel counted;
      per_image   per image the four counts of PER_IMAGE_FIELDS;
      instances   (image, instance id, size, pixels predicted as the instance's label, pixels predicted as a label of its
                  category) per ground-truth instance, in the script's order: images in order, instance ids ascending.
                  Instances of labels ignored in evaluation are left out here if the caller has not done so.
      names       the key of each image in perImageScores (the script uses the prediction's file name), default its number.
    classScores: tp / (tp + fp + fn) per label with fp counted over evaluated ground truth only, NaN for ignored labels and for
    labels without a pixel in either role; categoryScores: the same over the evaluated labels of a category; class/categoryInstScores
    (iIoU): tp and fn replaced by sums over the instances of tp * (avgClassSize / size), added in the script's order; priors; the
    four averages over the non-NaN entries.  With no instances at all this is what the script returns with evalInstLevelScore
    off: it still runs the instance formulas on zero statistics, so such a score is 0 where the label has false positives and
    NaN where it has none.
    perImageScores: "nbNotIgnoredPixels" and "nbCorrectPixels" reproduce the script, whose np.in1d(..., invert=True) makes them
    the pixels with IGNORED ground truth and the MISMATCHES among those; "nbEvaluatedPixels" and "nbEvaluatedCorrectPixels" are
    what the names promise: pixels with evaluated ground truth, and the correctly predicted ones among them."""
    avg = AVG_CLASS_SIZE if avg_class_size is None else avg_class_size
    lab_names, ign, _, has, cats = label_tables(labels)
    L = len(lab_names)
    conf = np.asarray(conf)
    if conf.shape != (L, L):
        raise ValueError(f"conf: expected [{L},{L}], got {conf.shape}")
    M = [[int(v) for v in row] for row in conf.tolist()]
    ids = list(range(L))
    evaluated = [l for l in ids if not ign[l]]
    cat_of = {r[1]: r[3] for r in labels}
    rowsum = [sum(M[l]) for l in ids]
    total = sum(rowsum)

    def block(rows, cols):
        return sum(M[r][c] for r in rows for c in cols)

    # instance statistics: tp and fn of every instance weighted by avgClassSize / size, per class and per category
    cls_stats = {n: [0.0, 0.0] for n, l in zip(lab_names, ids) if has[l] and not ign[l]}
    cat_stats: Dict[str, list] = {}
    for cat in cats:
        members = [r for r in labels if r[3] == cat and r[1] >= 0]
        if all(r[4] for r in members):
            cat_stats[cat] = [0.0, 0.0, [r[1] for r in members]]
    for _, inst_id, size, tp, cat_tp in instances:
        l = int(inst_id) // 1000
        if l >= L or not has[l]:
            raise ValueError(f"instance id {inst_id}: label {l} has no instances")
        if ign[l]:
            continue
        name = lab_names[l]
        weight = avg[name] / float(size)
        cls_stats[name][0] += float(tp) * weight
        cls_stats[name][1] += float(size - tp) * weight
        if cat_of[l] in cat_stats:
            cat_stats[cat_of[l]][0] += float(cat_tp) * weight
            cat_stats[cat_of[l]][1] += float(size - cat_tp) * weight

    class_scores, class_inst = {}, {}
    for l, name in zip(ids, lab_names):
        others = [o for o in evaluated if o != l]
        fp = block(others, [l])
        class_scores[name] = float("nan") if ign[l] else _ratio(M[l][l], fp, rowsum[l] - M[l][l])
        class_inst[name] = _ratio(cls_stats[name][0], fp, cls_stats[name][1]) if name in cls_stats else float("nan")
    cat_scores, cat_inst = {}, {}
    for cat in cats:
        mine = [r[1] for r in labels if r[3] == cat and r[1] >= 0 and not r[5]]
        outside = [o for o in evaluated if cat_of[o] != cat]
        if mine:
            tp = block(mine, mine)
            cat_scores[cat] = _ratio(tp, block(outside, mine), sum(rowsum[l] for l in mine) - tp)
        else:
            cat_scores[cat] = float("nan")
        if cat in cat_stats:
            cat_inst[cat] = _ratio(cat_stats[cat][0], block(outside, cat_stats[cat][2]), cat_stats[cat][1])
        else:
            cat_inst[cat] = float("nan")

    res: Dict[str, object] = {
        "confMatrix": M,
        "priors": {n: (float(rowsum[l]) / total if total else float("nan")) for l, n in zip(ids, lab_names)},
        "labels": {n: l for l, n in zip(ids, lab_names)},
        "classScores": class_scores, "classInstScores": class_inst, "categoryScores": cat_scores, "categoryInstScores": cat_inst,
        "averageScoreClasses": _average(class_scores), "averageScoreInstClasses": _average(class_inst),
        "averageScoreCategories": _average(cat_scores), "averageScoreInstCategories": _average(cat_inst),
    }
    if len(per_image):
        keys = list(names) if names is not None else list(range(len(per_image)))
        if len(keys) != len(per_image):
            raise ValueError(f"{len(keys)} names for {len(per_image)} images")
        res["perImageScores"] = {k: {f: int(v) for f, v in zip(PER_IMAGE_FIELDS, row)} for k, row in zip(keys, per_image)}
    return res


# ------------------------------------------------------------------------------------------------ the accumulator
class CityscapesScores:
    """Accumulates what the official script counts over image pairs, beside SegmentationConfusion: one HIP launch per update
    (ccdm_csscore), counts only, floats on the host in result().

    update(prediction, gt_ids, inst_ids=None, names=None)
      prediction  every form SegmentationConfusion.update takes ([B,K,h,w] float, integer or bool one-hot, or a class map [B,h,w]);
                  it is upsampled to the ground truth's (H, W), classified over the first K-1 channels and mapped through
                  id_table exactly as export_predictions does: the counts are those of the script run on the PNGs that
                  PredictionWriter writes.  Never builds a full-resolution tensor or an id image;
      gt_ids      [B,H,W] ground truth in label ids;
      inst_ids    [B,H,W] the values of *_gtFine_instanceIds.png, or None.  All updates of one accumulator give them or none does:
                  without them result() is the script's with evalInstLevelScore off;
      names       the keys of these images in perImageScores (the script uses the prediction file names), default their numbers.
    update_ids(pred_ids, gt_ids, ...) takes the prediction as label ids at the ground truth's size (ccdm_csscore_ids): what the
    script reads from the PNGs.
    A ground-truth or predicted id outside the label definition, and an instance id above 1000 that belongs to no label with
    instances, raise ValueError (where the script stops with "Unknown label" or a KeyError); the accumulator keeps its state from
    before that update."""

    def __init__(self, num_classes: int = NUM_CLASSES, device=None, id_table=None):
        self.num_classes = _check_num_classes(num_classes)
        if id_table is None:
            if self.num_classes != NUM_CLASSES:
                raise ValueError(f"{num_classes} classes: the default id table is Cityscapes' ({NUM_CLASSES} classes), pass id_table")
            id_table = TRAIN_ID_TO_ID
        if len(id_table) != self.num_classes:
            raise ValueError(f"id_table: expected {self.num_classes} entries, got {len(id_table)}")
        self.device = _cuda_device(device, "CityscapesScores")
        self.label_names, ign, cat, has, _ = label_tables()
        self.L = len(self.label_names)
        self._tables = [torch.as_tensor(np.asarray(t, np.uint8)).to(self.device) for t in (id_table, ign, cat, has)]
        self._conf = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        self.per_image: List[List[int]] = []
        self.instances: List[Tuple[int, int, int, int, int]] = []       # (image, instance id, size, tp, category tp)
        self.names: List = []
        self._with_instances: Optional[bool] = None

    @property
    def conf(self) -> torch.Tensor:
        return self._conf.cpu()

    def _targets(self, gt_ids, inst_ids, B):
        if gt_ids.ndim != 3 or gt_ids.shape[0] != B:
            raise ValueError(f"gt_ids: expected [B,H,W] with B = {B}, got {tuple(gt_ids.shape)}")
        gt = _labels_u8(torch.as_tensor(gt_ids), self.device)      # outside [0, 255] is outside the label definition: 255 stands for it
        inst = None
        if inst_ids is not None:
            inst = torch.as_tensor(inst_ids)
            if tuple(inst.shape) != tuple(gt.shape):
                raise ValueError(f"inst_ids: expected {tuple(gt.shape)}, got {tuple(inst.shape)}")
            inst = inst.to(self.device).to(torch.int32)
            if inst.numel() and (int(inst.min()) < 0 or int(inst.max()) > 65535):
                raise ValueError("inst_ids: values outside [0, 65535] (a 16-bit instance image)")
            inst = torch.where(inst > 32767, inst - 65536, inst).to(torch.int16).contiguous()      # the 16 bits of the value
        with_inst = inst is not None
        if self._with_instances is not None and self._with_instances != with_inst and B > 0:
            raise ValueError("inst_ids: every update of one CityscapesScores gives instance ids, or none does")
        return gt, inst

    def _finish(self, B, conf, per_image, instances, unknown, names):
        unk = unknown.cpu().tolist()
        if unk[0]:
            raise ValueError(f"{unk[0]} pixels with a ground-truth or predicted label id outside [0, {self.L}) (unknown label)")
        if unk[1]:
            raise ValueError(f"{unk[1]} pixels of instance ids above 1000 that belong to no label with instances "
                             f"(ids in [{INSTANCE_BASE}, {INSTANCE_BASE + INSTANCE_SLOTS}) are known)")
        if names is not None and len(names) != B:
            raise ValueError(f"names: {len(names)} for {B} images")
        first = len(self.per_image)
        if instances is not None:
            self._with_instances = True
            at = (instances[:, :, 0] > 0).nonzero()              # rows in (image, slot) order: the script's order
            rows = torch.cat([at, instances[at[:, 0], at[:, 1]].to(torch.int64)], dim=1).cpu().tolist()
            self.instances += [(first + b, INSTANCE_BASE + s, n, tp, ct) for b, s, n, tp, ct in rows]
        elif B > 0:
            self._with_instances = False
        self._conf += conf
        self.per_image += per_image.cpu().tolist()
        self.names += list(names) if names is not None else list(range(first, first + B))

    def _outputs(self, B, with_inst):
        conf = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        per_image = torch.zeros((B, 4), dtype=torch.int64, device=self.device)
        unknown = torch.zeros(2, dtype=torch.int32, device=self.device)
        instances = torch.empty((B, INSTANCE_SLOTS, 3), dtype=torch.int32, device=self.device) if with_inst else None
        return conf, per_image, instances, unknown

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, gt_ids, inst_ids=None, names: Optional[Sequence] = None) -> None:
        B = int(prediction.shape[0])
        gt, inst = self._targets(gt_ids, inst_ids, B)
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        H, W = int(gt.shape[1]), int(gt.shape[2])
        conf, per_image, instances, unknown = self._outputs(B, inst is not None)
        idt, ign, cat, has = self._tables
        hip.check(hip.load().ccdm_csscore(*prediction_args(probs, ps, cls), B, h, w, H, W, self.num_classes, idt.data_ptr(), gt.data_ptr(),
                                          inst.data_ptr() if inst is not None else None, self.L, ign.data_ptr(), cat.data_ptr(),
                                          has.data_ptr(), INSTANCE_BASE, INSTANCE_SLOTS, conf.data_ptr(), per_image.data_ptr(),
                                          instances.data_ptr() if instances is not None else None, unknown.data_ptr(),
                                          torch.cuda.current_stream(self.device).cuda_stream), "csscore")
        self._finish(B, conf, per_image, instances, unknown, names)

    @torch.no_grad()
    def update_ids(self, pred_ids, gt_ids, inst_ids=None, names: Optional[Sequence] = None) -> None:
        pred = torch.as_tensor(pred_ids)
        B = int(pred.shape[0])
        gt, inst = self._targets(gt_ids, inst_ids, B)
        if tuple(pred.shape) != tuple(gt.shape):
            raise ValueError(f"pred_ids: expected {tuple(gt.shape)}, got {tuple(pred.shape)}")
        pred = _labels_u8(pred, self.device)
        H, W = int(gt.shape[1]), int(gt.shape[2])
        conf, per_image, instances, unknown = self._outputs(B, inst is not None)
        _, ign, cat, has = self._tables
        hip.check(hip.load().ccdm_csscore_ids(pred.data_ptr(), B, H, W, gt.data_ptr(), inst.data_ptr() if inst is not None else None,
                                              self.L, ign.data_ptr(), cat.data_ptr(), has.data_ptr(), INSTANCE_BASE, INSTANCE_SLOTS,
                                              conf.data_ptr(), per_image.data_ptr(),
                                              instances.data_ptr() if instances is not None else None, unknown.data_ptr(),
                                              torch.cuda.current_stream(self.device).cuda_stream), "csscore_ids")
        self._finish(B, conf, per_image, instances, unknown, names)

    def result(self) -> Dict[str, object]:
        """The script's result dictionary over everything updated so far (scores_from_counts)."""
        return scores_from_counts(self.conf.numpy(), self.per_image, self.instances, self.names)
