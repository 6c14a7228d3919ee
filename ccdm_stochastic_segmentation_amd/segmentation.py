"""Cityscapes-type segmentation evaluation: mIoU of a sampled prediction against the labels, at the dataloader resolution or
against the original full-resolution labels — the reference's `evaluation/eval_cdm.py` (`Evaluator.infer_step`, `update_cm`,
`get_miou_and_ious`, `run_inference`), which is broken on its main branch (it calls the undefined
`predict_condition`, reads the absent key `cdm_only`, and scores raw Cityscapes label ids).

    SegmentationConfusion(num_classes, device)   ignite's ConfusionMatrix / IoU / mIoU and the reference's "soft" matrix, built by
                                                 one HIP kernel (ccdm_seg_confusion) that upsamples, classifies and counts without
                                                 a full-resolution probability tensor
    export_predictions / export_labels           the full-resolution class map as label ids and colours (the images of the
                                                 reference's `save_preds`), by one HIP kernel (ccdm_segexport) that shares the
                                                 confusion kernel's arithmetic
    SegmentationCalibration(num_classes, ...)    ECE / MCE, NLL, Brier score, reliability diagram and error-detection AUROC of the
                                                 probabilities (beyond the reference), from the counts of one HIP kernel
                                                 (ccdm_segcalib) on the same walk; calibration_from_counts is the host formula
    SegmentationBoundary(num_classes, ...)       Boundary IoU and the trimap IoU curve (beyond the reference) at band widths in
                                                 pixels or as a ratio of the image diagonal, from the counts of one HIP kernel pair
                                                 (ccdm_segboundary) on the class map ccdm_segexport writes; boundary_from_counts is
                                                 the host formula, resolve_boundary_widths the width rule
    SegmentationContourF(num_classes, ...)       the boundary F-score (BF score, beyond the reference) per class and image at
                                                 tolerances in pixels or as a ratio of the image diagonal, from the counts of one
                                                 HIP kernel pair (ccdm_contourf: a disc search around every contour pixel) on the
                                                 class map ccdm_segexport writes; contour_f_from_counts is the host formula,
                                                 resolve_contour_tolerances the tolerance rule
    SegmentationUncertainty(num_classes, ...)    does the spread of a multi-sample prediction mark its wrong pixels (beyond the
                                                 reference): error-detection AUROC / AUPR, sparsification (AUSE, AURG) and PAvPU of
                                                 the entropy and mutual-information maps, from the counts of one HIP kernel
                                                 (ccdm_uncscore) on the same walk; uncertainty_from_counts is the host formula
    PredictionWriter(directory, split)           writes them as PNGs under outputs/<split>/{submit,debug,label}
    eval_segmentation(params, ...)               the evaluation loop (no ignite), built like evaluation.eval_lidc_uncertainty; with
                                                 evaluation.cityscapes_script also the official script's scores
                                                 (cityscapes_scores.CityscapesScores, one more HIP launch per batch: ccdm_csscore)
    CityscapesVal(root, ...)                     the validation split, re-stated with PIL and numpy (no torchvision)
    SyntheticCityscapes(...)                     a deterministic stand-in so the entry point runs without the data
"""
from __future__ import annotations

import glob
import logging
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip

LOGGER = logging.getLogger(__name__)

# ------------------------------------------------------------------------------------------------ label definition
# (name, label id, train id) of the public Cityscapes label definition (cityscapesScripts, helpers/labels.py); train id 255 =
# not evaluated.  tests/golden/cityscapes_train_ids.json pins it.
CITYSCAPES_LABELS: Tuple[Tuple[str, int, int], ...] = (
    ("unlabeled", 0, 255), ("ego vehicle", 1, 255), ("rectification border", 2, 255), ("out of roi", 3, 255), ("static", 4, 255),
    ("dynamic", 5, 255), ("ground", 6, 255), ("road", 7, 0), ("sidewalk", 8, 1), ("parking", 9, 255), ("rail track", 10, 255),
    ("building", 11, 2), ("wall", 12, 3), ("fence", 13, 4), ("guard rail", 14, 255), ("bridge", 15, 255), ("tunnel", 16, 255),
    ("pole", 17, 5), ("polegroup", 18, 255), ("traffic light", 19, 6), ("traffic sign", 20, 7), ("vegetation", 21, 8),
    ("terrain", 22, 9), ("sky", 23, 10), ("person", 24, 11), ("rider", 25, 12), ("car", 26, 13), ("truck", 27, 14),
    ("bus", 28, 15), ("caravan", 29, 255), ("trailer", 30, 255), ("train", 31, 16), ("motorcycle", 32, 17), ("bicycle", 33, 18),
    ("license plate", -1, 255),
)
NUM_CLASSES = 20            # 19 evaluated train ids + the ignore class
IGNORE_CLASS = 19           # the model's ignore channel / label value (datasets/cityscapes.py: BACKGROUND_CLASS)
TRAIN_ID_NAMES: Tuple[str, ...] = tuple(n for n, _, t in sorted(CITYSCAPES_LABELS, key=lambda r: r[2]) if t != 255)
# The colour column of the same public definition, one (R, G, B) per row of CITYSCAPES_LABELS (kept beside it: the rows above are
# pinned as triples by tests/golden/cityscapes_train_ids.json).
CITYSCAPES_COLORS: Tuple[Tuple[int, int, int], ...] = (
    (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
    (111, 74, 0), (81, 0, 81), (128, 64, 128), (244, 35, 232), (250, 170, 160), (230, 150, 140),
    (70, 70, 70), (102, 102, 156), (190, 153, 153), (180, 165, 180), (150, 100, 100), (150, 120, 90),
    (153, 153, 153), (153, 153, 153), (250, 170, 30), (220, 220, 0), (107, 142, 35),
    (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
    (0, 60, 100), (0, 0, 90), (0, 0, 110), (0, 80, 100), (0, 0, 230), (119, 11, 32),
    (0, 0, 142),
)
assert len(CITYSCAPES_COLORS) == len(CITYSCAPES_LABELS)
# train id -> label id / colour, 20 entries: the 19 evaluated classes in train-id order, then the ignore class as id 0 (unlabeled),
# black — the reference's train_id_to_id / train_id_to_color.  tests/golden/cityscapes_export_tables.json pins them.
_BY_TRAIN_ID = sorted((t, i, c) for (_, i, t), c in zip(CITYSCAPES_LABELS, CITYSCAPES_COLORS) if t != 255)
TRAIN_ID_TO_ID: Tuple[int, ...] = tuple(i for _, i, _ in _BY_TRAIN_ID) + (0,)
TRAIN_ID_TO_COLOR: Tuple[Tuple[int, int, int], ...] = tuple(c for _, _, c in _BY_TRAIN_ID) + ((0, 0, 0),)


def id_to_train_id_lut() -> np.ndarray:
    """uint8 [256]: Cityscapes label id -> train id, every id that is not evaluated (and every id the definition lacks) -> 19."""
    lut = np.full(256, IGNORE_CLASS, dtype=np.uint8)
    for _, i, t in CITYSCAPES_LABELS:
        if i >= 0 and t != 255:
            lut[i] = t
    return lut


# ------------------------------------------------------------------------------------------------ metrics
def iou_from_confusion(cm) -> torch.Tensor:
    """ignite's IoU on a [C,C] confusion matrix (rows = target): diag / (rowsum + colsum - diag + 1e-15) in float64.
    A class without pixels in either role gives 0."""
    cm = torch.as_tensor(cm).double()
    return cm.diag() / (cm.sum(dim=1) + cm.sum(dim=0) - cm.diag() + 1e-15)


def iou_soft_from_confusion(cm) -> torch.Tensor:
    """The reference's get_miou_and_ious (eval_cdm.py) on its soft matrix (rows = prediction): diag / (colsum + rowsum - diag),
    NaN -> 0.  In float64 (the reference's float32 sums lose integers past 2^24)."""
    cm = torch.as_tensor(cm).double()
    diag = cm.diag()
    iou = diag / (cm.sum(dim=0) + cm.sum(dim=1) - diag)
    iou[iou != iou] = 0
    return iou


def prediction_form(prediction: torch.Tensor, num_classes: int, device):
    """The form of a prediction the segmentation kernels read -> (fp32 channels-last tensor or None, pixel stride, uint8 class map
    or None, h, w): a float [B,K,h,w] that is a view of channels-last memory is read in place (any other layout is copied once at
    the low resolution), an integer or bool one-hot [B,K,h,w] and a class map [B,h,w] become a uint8 class map."""
    K = int(num_classes)
    prediction = prediction.to(device)
    if prediction.ndim == 3:
        return None, 0, prediction.to(torch.uint8).contiguous(), int(prediction.shape[1]), int(prediction.shape[2])
    if prediction.ndim != 4 or prediction.shape[1] != K:
        raise ValueError(f"prediction: expected [B,{K},h,w] or a class map [B,h,w], got {tuple(prediction.shape)}")
    h, w = int(prediction.shape[2]), int(prediction.shape[3])
    if not prediction.is_floating_point():
        return None, 0, prediction.argmax(dim=1).to(torch.uint8).contiguous(), h, w
    p = prediction.to(torch.float32).permute(0, 2, 3, 1)
    ps = p.stride(2)
    if not (p.stride(3) == 1 and ps >= K and p.stride(1) == w * ps and p.stride(0) == h * w * ps):
        p, ps = p.contiguous(), K
    return p, ps, None, h, w


def prediction_args(probs, ps, cls):
    """The three leading arguments of every segmentation kernel (probs, pixel_stride, cls) from prediction_form's first three."""
    return (probs.data_ptr() if probs is not None else None, ps, cls.data_ptr() if cls is not None else None)


def _cuda_device(device, what: str) -> torch.device:
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise hip.CcdmHipError(f"{what} runs on the GPU (no CPU path)")
    return device


def _check_num_classes(num_classes) -> int:
    if not 2 <= int(num_classes) <= 32:
        raise ValueError(f"num_classes: {num_classes} (the kernel takes 2..32 channels, the last one the ignore class)")
    return int(num_classes)


def _grown(ws: Optional[torch.Tensor], need: int, device) -> Optional[torch.Tensor]:      # the grow-only workspace
    return ws if need == 0 or (ws is not None and ws.numel() >= need) else torch.empty(need, dtype=torch.uint8, device=device)


def _write_json(output_path: str, name: str, obj) -> str:
    """obj as <output_path>/<name>.json; returns the path."""
    import json
    os.makedirs(output_path, exist_ok=True)
    path = os.path.join(output_path, name + ".json")
    with open(path, "w") as f:
        json.dump(obj, f, indent=2, sort_keys=True)
    return path


def _labels_u8(labels: torch.Tensor, device) -> torch.Tensor:
    """Labels [B,H,W] as the contiguous uint8 tensor the kernels read: anything outside [0, 255] is not counted either way, 255
    stands for it."""
    lab = labels.to(device)
    if lab.dtype != torch.uint8:
        lab = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab).to(torch.uint8)
    return lab.contiguous()


class SegmentationConfusion:
    """The two confusion matrices of the reference's Cityscapes evaluator over `num_classes` = K model channels, of which the
    first C = K - 1 are scored (the last is the ignore class, dropped as `prediction_onehot[:, 0:K-1]` drops it):
      confusion  int64 [C,C], rows = target, columns = argmax class: ignite's ConfusionMatrix(num_classes=C), accumulated;
      soft       int64 [C,C], rows = class, columns = target: the reference's update_cm, sum of the class probabilities per
                 target, truncated toward zero per update (its `.to(torch.int)`); soft_exact keeps the untruncated float64 sums.
    Pixels whose label is not in [0, C) are not counted (19, 255, ...).

    update(prediction, labels): prediction is [B,K,h,w] float (a view of channels-last memory — diffusion_out and the mean of
    predict_multiple — is read in place, any other layout is copied once at the low resolution), an integer or bool one-hot
    [B,K,h,w] (a "majority" diffusion_out) or a class map [B,h,w]; labels are [B,H,W] integers.  When (H,W) differs from (h,w)
    the prediction is upsampled bilinearly exactly as F.interpolate(mode="bilinear", align_corners=False) computes it in fp32.
    A one-hot or class map goes through the same arithmetic as the float32 of its one-hot, bit for bit; the reference cannot
    score those at resolution "original" (F.interpolate raises on the int64 one-hot).  Never builds a full-resolution tensor."""

    def __init__(self, num_classes: int, device=None):
        self.num_classes = _check_num_classes(num_classes)
        self.C = self.num_classes - 1
        self.device = _cuda_device(device, "SegmentationConfusion")
        self._hard = torch.zeros((self.C, self.C), dtype=torch.int64, device=self.device)
        self.soft = torch.zeros((self.C, self.C), dtype=torch.int64)
        self.soft_exact = torch.zeros((self.C, self.C), dtype=torch.float64)
        self._ws: Optional[torch.Tensor] = None

    @property
    def confusion(self) -> torch.Tensor:
        return self._hard.cpu()

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, labels: torch.Tensor) -> None:
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        lab = _labels_u8(labels, self.device)
        B, H, W = (int(s) for s in lab.shape)
        lib = hip.load()
        need = int(lib.ccdm_seg_confusion_workspace_bytes(B, H, W, self.num_classes)) if B > 0 else 0
        self._ws = _grown(self._ws, need, self.device)
        soft = torch.empty((self.C, self.C), dtype=torch.float64, device=self.device)
        ws = self._ws.data_ptr() if need else None
        hip.check(lib.ccdm_seg_confusion(*prediction_args(probs, ps, cls), lab.data_ptr(), B, h, w, H, W, self.num_classes,
                                         self._hard.data_ptr(), soft.data_ptr(), ws, need,
                                         torch.cuda.current_stream(self.device).cuda_stream), "seg_confusion")
        soft = soft.cpu()
        self.soft_exact += soft
        self.soft += soft.trunc().to(torch.int64)

    def iou(self) -> torch.Tensor:
        return iou_from_confusion(self.confusion)

    def miou(self) -> float:
        return float(self.iou().mean())

    def iou_soft(self) -> torch.Tensor:
        return iou_soft_from_confusion(self.soft)

    def miou_soft(self) -> float:
        return float(self.iou_soft().mean())


# ------------------------------------------------------------------------------------------------ calibration
def calibration_from_counts(bins, conf_sum, sums, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The calibration scores behind the counts of ccdm_segcalib, in float64 numpy (no GPU):
      bins      [C,M,2] by (predicted class, confidence bin): {pixels, correct pixels};
      conf_sum  [C,M]   by (predicted class, confidence bin): the sum of the confidence (the renormalised probability of the
                        predicted class);
      sums      [3]     {sum of -log q_t, sum of the Brier score, sum of q_t} over the counted pixels.
    Returns a dict of plain Python values (JSON as it stands):
      pixels, accuracy, mean_confidence, nll, brier, mean_true_class_probability    totals and means over the counted pixels;
      ece       sum over the bins b of n_b / n * |acc_b - conf_b| (top label, the class axis summed out);  mce: the largest
                |acc_b - conf_b| of a non-empty bin;
      reliability            {"count", "accuracy", "confidence"}, one entry per bin, accuracy / confidence None in an empty bin;
      ece_per_class          the same ECE over the pixels predicted as class p (a list, or a dict keyed by class_names); None for
                             a class never predicted;
      auroc_error_detection  the confidence as the score that separates correct from wrong pixels: P(conf of a correct pixel >
                             conf of a wrong one) + P(same bin) / 2 from the [M,2] histogram, exact for the binned score; None
                             when there is no correct or no wrong pixel;
      bins      M.
    Without counted pixels every score is None."""
    bins = np.asarray(bins, dtype=np.float64)
    conf_sum = np.asarray(conf_sum, dtype=np.float64)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1)
    if bins.ndim != 3 or bins.shape[2] != 2 or conf_sum.shape != bins.shape[:2] or sums.shape != (3,):
        raise ValueError(f"expected bins [C,M,2], conf_sum [C,M], sums [3], got {bins.shape}, {conf_sum.shape}, {sums.shape}")
    C, M = bins.shape[:2]
    if class_names is not None and len(class_names) != C:
        raise ValueError(f"class_names: {len(class_names)} names for {C} classes")

    def ece_mce(count, right, csum):
        """(ece, mce, accuracy per bin, confidence per bin) of one [M] histogram with at least one pixel"""
        acc = [right[b] / count[b] if count[b] else None for b in range(M)]
        conf = [csum[b] / count[b] if count[b] else None for b in range(M)]
        gaps = [abs(acc[b] - conf[b]) for b in range(M) if count[b]]
        ece = sum(count[b] / count.sum() * abs(acc[b] - conf[b]) for b in range(M) if count[b])
        return float(ece), float(max(gaps)), acc, conf

    count, right, csum = bins[:, :, 0].sum(0), bins[:, :, 1].sum(0), conf_sum.sum(0)
    n = count.sum()
    res: Dict[str, object] = {"pixels": int(n), "bins": int(M)}
    per_class = [ece_mce(bins[p, :, 0], bins[p, :, 1], conf_sum[p])[0] if bins[p, :, 0].sum() else None for p in range(C)]
    res["ece_per_class"] = per_class if class_names is None else dict(zip(class_names, per_class))
    if n == 0:
        res.update(accuracy=None, mean_confidence=None, ece=None, mce=None, nll=None, brier=None, mean_true_class_probability=None,
                   auroc_error_detection=None,
                   reliability={"count": [0] * M, "accuracy": [None] * M, "confidence": [None] * M})
        return res
    ece, mce, acc, conf = ece_mce(count, right, csum)
    wrong = count - right
    n_right, n_wrong = right.sum(), wrong.sum()
    auroc = None
    if n_right and n_wrong:
        below = np.concatenate([[0.0], np.cumsum(wrong)[:-1]])          # wrong pixels in the lower bins
        auroc = float((right * (below + 0.5 * wrong)).sum() / (n_right * n_wrong))
    res.update(accuracy=float(n_right / n), mean_confidence=float(csum.sum() / n), ece=ece, mce=mce, nll=float(sums[0] / n),
               brier=float(sums[1] / n), mean_true_class_probability=float(sums[2] / n), auroc_error_detection=auroc,
               reliability={"count": [int(c) for c in count], "accuracy": [None if a is None else float(a) for a in acc],
                            "confidence": [None if c is None else float(c) for c in conf]})
    return res


class SegmentationCalibration:
    """Calibration of a segmentation prediction against the labels (beyond the reference, whose scores are all hard): over the
    pixels SegmentationConfusion counts, with the class it counts, the confidence is the probability of that class renormalised
    over the C = K - 1 scored channels; one HIP kernel (ccdm_segcalib) upsamples, classifies, bins and sums without a
    full-resolution probability tensor.  `bins` equal-width confidence bins, 2..64.
      bins_count  int64 [C,bins,2] by (predicted class, bin): {pixels, correct pixels}, accumulated on the device;
      conf_sum    float64 [C,bins], sums float64 [3] ({-log q_t, Brier, q_t}): per update from the device, added on the host.
    update(prediction, labels) takes what SegmentationConfusion.update takes; a one-hot or class map has confidence 1 wherever
    the upsampled map is not mixed (class_map_updates counts such updates).  result() is calibration_from_counts."""

    def __init__(self, num_classes: int, device=None, bins: int = 15):
        self.num_classes = _check_num_classes(num_classes)
        if not 2 <= int(bins) <= 64:
            raise ValueError(f"bins: {bins} (the kernel takes 2..64 confidence bins)")
        self.bins = int(bins)
        self.C = self.num_classes - 1
        self.device = _cuda_device(device, "SegmentationCalibration")
        self._bins = torch.zeros((self.C, self.bins, 2), dtype=torch.int64, device=self.device)
        self.conf_sum = torch.zeros((self.C, self.bins), dtype=torch.float64)
        self.sums = torch.zeros(3, dtype=torch.float64)
        self.class_map_updates = 0
        self._ws: Optional[torch.Tensor] = None

    @property
    def bins_count(self) -> torch.Tensor:
        return self._bins.cpu()

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, labels: torch.Tensor) -> None:
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        lab = _labels_u8(labels, self.device)
        B, H, W = (int(s) for s in lab.shape)
        self.class_map_updates += int(cls is not None)
        if B == 0:
            return
        lib = hip.load()
        need = int(lib.ccdm_segcalib_workspace_bytes(B, H, W, self.num_classes, self.bins))
        self._ws = _grown(self._ws, need, self.device)
        out = torch.empty(self.C * self.bins + 3, dtype=torch.float64, device=self.device)      # conf_sum, then sums
        hip.check(lib.ccdm_segcalib(*prediction_args(probs, ps, cls), lab.data_ptr(), B, h, w, H, W, self.num_classes, self.bins,
                                    self._bins.data_ptr(), out.data_ptr(),
                                    out.data_ptr() + 8 * self.C * self.bins, self._ws.data_ptr(), need,
                                    torch.cuda.current_stream(self.device).cuda_stream), "segcalib")
        out = out.cpu()
        self.conf_sum += out[:-3].reshape(self.C, self.bins)
        self.sums += out[-3:]

    def result(self, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
        return calibration_from_counts(self.bins_count.numpy(), self.conf_sum.numpy(), self.sums.numpy(), class_names)


# ------------------------------------------------------------------------------------------------ boundary scores
BOUNDARY_MAX_WIDTH = 64             # the widest band ccdm_segboundary takes, in pixels
BOUNDARY_DEFAULT_WIDTHS = ("ratio:0.02",)       # the Boundary IoU paper's 2 % of the image diagonal: 46 px at 1024 x 2048


def _px_entry(entry, what: str, limit: int):
    """One entry of a list of pixel sizes -> ("px", int) or ("ratio", float); ValueError for anything else."""
    if isinstance(entry, (int, np.integer)) and not isinstance(entry, bool):
        if not 1 <= int(entry) <= limit:
            raise ValueError(f"{what} {entry!r}: a value in pixels lies in [1, {limit}]")
        return "px", int(entry)
    if isinstance(entry, str) and entry.startswith("ratio:"):
        try:
            ratio = float(entry[len("ratio:"):])
        except ValueError:
            ratio = float("nan")
        if not (0.0 < ratio < float("inf")):
            raise ValueError(f"{what} {entry!r}: expected 'ratio:R' with a number R > 0")
        return "ratio", ratio
    raise ValueError(f"{what} {entry!r}: expected an int in [1, {limit}] (pixels) or the string 'ratio:R'")


def _resolve_px_list(entries, size: Optional[Sequence[int]], what: str, limit: int) -> List[int]:
    """The rule the boundary widths and the contour tolerances share: a non-empty list without repeats of ints in [1, limit]
    (pixels) and "ratio:R" strings, which stand for max(1, round(R * sqrt(H^2 + W^2))) pixels at size = (H, W) and must not exceed
    `limit` there.  Without `size` the entries are only checked and a ratio entry gives 0."""
    if isinstance(entries, (str, bytes)) or not isinstance(entries, (list, tuple)) or len(entries) == 0:
        raise ValueError(f"{what}s {entries!r}: expected a non-empty list of ints (pixels) and 'ratio:R' strings")
    if len({str(e) for e in entries}) != len(entries):
        raise ValueError(f"{what}s {list(entries)!r}: an entry is repeated")
    out = []
    for entry in entries:
        kind, v = _px_entry(entry, what, limit)
        if kind == "ratio":
            if size is None:
                v = 0
            else:
                H, W = int(size[0]), int(size[1])
                v = max(1, int(round(v * float(np.sqrt(float(H * H + W * W))))))
                if v > limit:
                    raise ValueError(f"{what} {entry!r} is {v} pixels at {H} x {W}: the limit is {limit} pixels")
        out.append(v)
    return out


def resolve_boundary_widths(widths, size: Optional[Sequence[int]] = None) -> List[int]:
    """The width rule of the boundary scores.  `widths` is a non-empty list without repeats whose entries are an int >= 1 (pixels) or
    the string "ratio:R", which stands for max(1, round(R * sqrt(H^2 + W^2))) pixels at the scored size (H, W) (Python's round, as
    the published Boundary IoU code).  Returns the widths in pixels, one per entry; without `size` the entries are only checked
    and a ratio entry gives 0.  An entry that is neither, or a width outside [1, 64], is a ValueError that names the limit."""
    return _resolve_px_list(widths, size, "boundary width", BOUNDARY_MAX_WIDTH)


def boundary_from_counts(bcounts, trimap, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The boundary scores behind the counts of ccdm_segboundary at one width, on the host (no GPU):
      bcounts  [C,3] per class {|band_G|, |band_P|, |band_G & band_P|} (band: the pixels of the class within the width of its border);
      trimap   [C,C] rows = target, columns = prediction: the hard confusion matrix over the counted pixels in the band of their
               own target class.
    Returns a dict of plain Python values (JSON as it stands):
      boundary_iou       per class inter / (g + p - inter) (Boundary IoU, Cheng et al. 2021), None for a class whose two bands are
                         both empty; a list, or a dict keyed by class_names;
      mean_boundary_iou  the mean over the classes that have a value, None when there is none;
      trimap_iou, trimap_miou   iou_from_confusion of `trimap` and its mean over all C classes (as mIoU: an absent class gives 0);
      trimap_pixels      the pixels in `trimap`;
      bcounts, trimap    the counts themselves."""
    bc = np.asarray(bcounts, dtype=np.int64)
    tm = np.asarray(trimap, dtype=np.int64)
    if bc.ndim != 2 or bc.shape[1] != 3 or tm.shape != (bc.shape[0], bc.shape[0]):
        raise ValueError(f"expected bcounts [C,3] and trimap [C,C], got {bc.shape} and {tm.shape}")
    C = bc.shape[0]
    if class_names is not None and len(class_names) != C:
        raise ValueError(f"class_names: {len(class_names)} names for {C} classes")
    union = bc[:, 0] + bc[:, 1] - bc[:, 2]
    biou = [float(bc[c, 2]) / float(union[c]) if union[c] > 0 else None for c in range(C)]
    have = [v for v in biou if v is not None]
    tiou = iou_from_confusion(torch.from_numpy(tm))
    named = (lambda v: list(v)) if class_names is None else (lambda v: dict(zip(class_names, v)))
    return {"boundary_iou": named(biou), "mean_boundary_iou": float(np.mean(have)) if have else None,
            "trimap_iou": named(tiou.tolist()), "trimap_miou": float(tiou.mean()), "trimap_pixels": int(tm.sum()),
            "bcounts": bc.tolist(), "trimap": tm.tolist()}


class SegmentationBoundary:
    """Contour scores of a segmentation prediction against the labels (beyond the reference): Boundary IoU and the trimap confusion
    matrix at every width of `widths` (resolve_boundary_widths; default the Boundary IoU paper's 2 % of the image diagonal), over
    the pixels SegmentationConfusion counts, with the class it counts.  update(prediction, labels) takes what
    SegmentationConfusion.update takes: one ccdm_segexport launch turns the prediction (probabilities or a class map, at any
    size) into the class map at the labels' size, then one ccdm_segboundary launch per width counts:
      bcounts  int64 [widths,C,3], trimap int64 [widths,C,C], accumulated on the device (the contract of include/ccdm_hip.h).
    A ratio entry is resolved again at every update, at that update's (H, W), and its counts add up over the updates: an image is
    scored at the width its own diagonal gives, as Boundary IoU prescribes for a data set of mixed sizes.  `pixels` keeps, per
    entry, the distinct pixel widths used so far (one value for Cityscapes, whose images share one size).
    result() is boundary_from_counts per entry."""

    def __init__(self, num_classes: int, device=None, widths: Sequence = BOUNDARY_DEFAULT_WIDTHS):
        self.num_classes = _check_num_classes(num_classes)
        self.widths = list(widths) if isinstance(widths, (list, tuple)) else widths
        resolve_boundary_widths(self.widths)
        self.widths = [e if isinstance(e, str) else int(e) for e in self.widths]
        self.C = self.num_classes - 1
        self.device = _cuda_device(device, "SegmentationBoundary")
        n = len(self.widths)
        self._bc = torch.zeros((n, self.C, 3), dtype=torch.int64, device=self.device)
        self._tm = torch.zeros((n, self.C, self.C), dtype=torch.int64, device=self.device)
        self.pixels: List[List[int]] = [[] for _ in range(n)]
        # ccdm_segexport wants both tables although only train_id is written
        self._tables = torch.zeros(4 * self.num_classes, dtype=torch.uint8, device=self.device)
        self._ws: Optional[torch.Tensor] = None

    @property
    def bcounts(self) -> torch.Tensor:
        return self._bc.cpu()

    @property
    def trimap(self) -> torch.Tensor:
        return self._tm.cpu()

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, labels: torch.Tensor) -> None:
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        lab = _labels_u8(labels, self.device)
        B, H, W = (int(s) for s in lab.shape)
        px = resolve_boundary_widths(self.widths, (H, W))
        if B == 0:
            return
        lib = hip.load()
        K, stream = self.num_classes, torch.cuda.current_stream(self.device).cuda_stream
        train_id = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        hip.check(lib.ccdm_segexport(*prediction_args(probs, ps, cls), B, h, w, H, W, K, K - 1, self._tables.data_ptr(),
                                     self._tables.data_ptr() + K, train_id.data_ptr(), None, None, stream), "segexport")
        need = int(lib.ccdm_segboundary_workspace_bytes(B, H, W))
        self._ws = _grown(self._ws, need, self.device)
        for i, d in enumerate(px):
            hip.check(lib.ccdm_segboundary(train_id.data_ptr(), lab.data_ptr(), B, H, W, K, d, self._bc[i].data_ptr(), self._tm[i].data_ptr(),
                                           self._ws.data_ptr(), need, stream), "segboundary")
            if d not in self.pixels[i]:
                self.pixels[i].append(d)

    def result(self, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
        """{"widths": [{"entry", "pixels"} per entry], "by_width": {str(entry): boundary_from_counts(...)}}"""
        bc, tm = self.bcounts.numpy(), self.trimap.numpy()
        return {"widths": [{"entry": e, "pixels": list(p)} for e, p in zip(self.widths, self.pixels)],
                "by_width": {str(e): boundary_from_counts(bc[i], tm[i], class_names) for i, e in enumerate(self.widths)}}


# ------------------------------------------------------------------------------------------------ boundary F-score
CONTOUR_MAX_TOLERANCE = 32          # the widest disc ccdm_contourf searches, in pixels
CONTOUR_DEFAULT_TOLERANCES = ("ratio:0.0075",)      # bfscore's 0.75 % of the image diagonal: 17 px at 1024 x 2048


def resolve_contour_tolerances(tolerances, size: Optional[Sequence[int]] = None) -> List[int]:
    """The tolerance rule of the boundary F-score: the rule of resolve_boundary_widths (a non-empty list without repeats of ints,
    pixels, and "ratio:R" strings, R times the diagonal of the scored size (H, W), rounded, at least 1) with the limit
    [1, 32].  Returns the tolerances in pixels, one per entry; without `size` the entries are only checked and a ratio entry
    gives 0.  A bad entry, or a ratio beyond 32 pixels at `size`, is a ValueError that names the limit."""
    return _resolve_px_list(tolerances, size, "contour tolerance", CONTOUR_MAX_TOLERANCE)


def contour_f_from_counts(counts, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The boundary F-scores behind the counts of ccdm_contourf at one tolerance, in float64 on the host (no GPU):
      counts  [N,C,4] per image and class {nP, mP, nG, mG}: the contour pixels of the prediction, those of them matched in the
              labels, the contour pixels of the labels, those of them matched in the prediction.
    A cell (image, class) is scored when nG > 0: precision = mP / nP (0 when nP = 0), recall = mG / nG, F = 2PR / (P + R) (0 when
    P + R = 0).  Returns a dict of plain Python values (JSON as it stands); per class a list, or a dict keyed by class_names:
      bf_score, precision, recall   the mean over the class's scored images, None when it has none;
      images      the scored cells of the class;  pred_only: its cells with nG = 0 < nP, reported and not averaged;
      mean_bf_score   the mean of bf_score over the classes that have a value, None when there is none;
      pooled      {"bf_score", "precision", "recall"} per class from the sums of the four counts over all images (None for a
                  class whose summed nG is 0), with their class means "mean_bf_score", "mean_precision", "mean_recall";
      counts      those sums, [C][4]."""
    ct = np.asarray(counts)
    if ct.ndim != 3 or ct.shape[2] != 4:
        raise ValueError(f"expected counts [N,C,4], got {ct.shape}")
    ct = ct.astype(np.int64)
    N, C = ct.shape[:2]
    if class_names is not None and len(class_names) != C:
        raise ValueError(f"class_names: {len(class_names)} names for {C} classes")

    def prf(nP, mP, nG, mG):
        """(precision, recall, F) of a scored cell, nG > 0"""
        P = float(mP) / float(nP) if nP > 0 else 0.0
        R = float(mG) / float(nG)
        return P, R, (2.0 * P * R / (P + R) if P + R > 0 else 0.0)

    def mean(values):
        have = [v for v in values if v is not None]
        return float(np.mean(have)) if have else None
    named = (lambda v: list(v)) if class_names is None else (lambda v: dict(zip(class_names, v)))
    per_image = [[prf(*ct[n, c]) for n in range(N) if ct[n, c, 2] > 0] for c in range(C)]
    col = lambda k: [float(np.mean([t[k] for t in cells])) if cells else None for cells in per_image]
    total = ct.sum(axis=0)
    pooled = [prf(*total[c]) if total[c, 2] > 0 else (None, None, None) for c in range(C)]
    pcol = lambda k: [t[k] for t in pooled]
    return {"bf_score": named(col(2)), "precision": named(col(0)), "recall": named(col(1)),
            "images": named([len(cells) for cells in per_image]),
            "pred_only": named([int(((ct[:, c, 2] == 0) & (ct[:, c, 0] > 0)).sum()) for c in range(C)]),
            "mean_bf_score": mean(col(2)),
            "pooled": {"bf_score": named(pcol(2)), "precision": named(pcol(0)), "recall": named(pcol(1)),
                       "mean_bf_score": mean(pcol(2)), "mean_precision": mean(pcol(0)), "mean_recall": mean(pcol(1))},
            "counts": total.tolist()}


class SegmentationContourF:
    """The boundary F-score of a segmentation prediction against the labels (beyond the reference; Csurka et al.'s BF score,
    MATLAB's bfscore, the DAVIS F-measure): how much of the predicted contour of a class lies within a tolerance of the true
    one, and how much of the true contour was found, per class and per image, at every tolerance of `tolerances`
    (resolve_contour_tolerances; default bfscore's 0.75 % of the image diagonal), over the pixels SegmentationConfusion counts,
    with the class it counts.  update(prediction, labels) takes what SegmentationConfusion.update takes: one ccdm_segexport launch
    turns the prediction into the class map at the labels' size, then one ccdm_contourf launch per tolerance counts
      counts  int64 [tolerances, images, C, 4]: {nP, mP, nG, mG} per image and class (the contract of include/ccdm_hip.h); the
              tables of the updates are kept on the device and concatenated.
    A ratio entry is resolved again at every update, at that update's (H, W); `pixels` keeps, per entry, the distinct pixel
    tolerances used so far.  result() is contour_f_from_counts per entry."""

    def __init__(self, num_classes: int, device=None, tolerances: Sequence = CONTOUR_DEFAULT_TOLERANCES):
        self.num_classes = _check_num_classes(num_classes)
        self.tolerances = list(tolerances) if isinstance(tolerances, (list, tuple)) else tolerances
        resolve_contour_tolerances(self.tolerances)
        self.tolerances = [e if isinstance(e, str) else int(e) for e in self.tolerances]
        self.C = self.num_classes - 1
        self.device = _cuda_device(device, "SegmentationContourF")
        self._tables: List[torch.Tensor] = []               # one [tolerances, B, C, 4] per update
        self.pixels: List[List[int]] = [[] for _ in self.tolerances]
        # ccdm_segexport wants both tables although only train_id is written
        self._export_tables = torch.zeros(4 * self.num_classes, dtype=torch.uint8, device=self.device)
        self._ws: Optional[torch.Tensor] = None

    @property
    def counts(self) -> torch.Tensor:
        if not self._tables:
            return torch.zeros((len(self.tolerances), 0, self.C, 4), dtype=torch.int64)
        return torch.cat(self._tables, dim=1).cpu()

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, labels: torch.Tensor) -> None:
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        lab = _labels_u8(labels, self.device)
        B, H, W = (int(s) for s in lab.shape)
        px = resolve_contour_tolerances(self.tolerances, (H, W))
        if B == 0:
            return
        lib = hip.load()
        K, stream = self.num_classes, torch.cuda.current_stream(self.device).cuda_stream
        train_id = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        hip.check(lib.ccdm_segexport(*prediction_args(probs, ps, cls), B, h, w, H, W, K, K - 1, self._export_tables.data_ptr(),
                                     self._export_tables.data_ptr() + K, train_id.data_ptr(), None, None, stream), "segexport")
        need = int(lib.ccdm_contourf_workspace_bytes(B, H, W))
        self._ws = _grown(self._ws, need, self.device)
        table = torch.zeros((len(px), B, self.C, 4), dtype=torch.int64, device=self.device)
        for i, theta in enumerate(px):
            hip.check(lib.ccdm_contourf(train_id.data_ptr(), lab.data_ptr(), B, H, W, K, theta, table[i].data_ptr(), self._ws.data_ptr(), need,
                                        stream), "contourf")
            if theta not in self.pixels[i]:
                self.pixels[i].append(theta)
        self._tables.append(table)

    def result(self, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
        """{"tolerances": [{"entry", "pixels"} per entry], "by_tolerance": {str(entry): contour_f_from_counts(...)}}"""
        ct = self.counts.numpy()
        return {"tolerances": [{"entry": e, "pixels": list(p)} for e, p in zip(self.tolerances, self.pixels)],
                "by_tolerance": {str(e): contour_f_from_counts(ct[i], class_names) for i, e in enumerate(self.tolerances)}}


# ------------------------------------------------------------------------------------------------ uncertainty quality
UNCERTAINTY_MEASURES = ("entropy", "mutual_info")       # the per-pixel maps of DenoisingModel.predict_multiple that are scored
UNCERTAINTY_PATCHES = (2, 4, 8, 16)                     # the patch sizes ccdm_uncscore takes
UNCERTAINTY_MAX_BINS = 512


def check_uncertainty_settings(bins, patch, measures, key: str = "") -> Tuple[int, int, Tuple[str, ...]]:
    """(bins, patch, measures) of the uncertainty scores, checked on the host; `key` prefixes the name a ValueError gives."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= UNCERTAINTY_MAX_BINS:
        raise ValueError(f"{key}bins: {bins!r} (the kernel takes 2..{UNCERTAINTY_MAX_BINS} uncertainty bins)")
    if isinstance(patch, bool) or not isinstance(patch, (int, np.integer)) or int(patch) not in UNCERTAINTY_PATCHES:
        raise ValueError(f"{key}patch: {patch!r} is not in {list(UNCERTAINTY_PATCHES)}")
    if isinstance(measures, str) or not isinstance(measures, (list, tuple)) or not measures or len(set(measures)) != len(measures) \
            or any(m not in UNCERTAINTY_MEASURES for m in measures):
        raise ValueError(f"{key}measures: {measures!r} (expected a non-empty list without repeats from {list(UNCERTAINTY_MEASURES)})")
    return int(bins), int(patch), tuple(measures)


def uncertainty_from_counts(pix, patch) -> Dict[str, object]:
    """The uncertainty-quality scores of one measure behind the counts of ccdm_uncscore, in float64 numpy (no GPU):
      pix    [M,2] by uncertainty bin (bin b holds the values in [b/M, (b+1)/M) of the scale): {pixels, wrong pixels};
      patch  [M,2] by bin of the patch's mean uncertainty: {patches, inaccurate patches}.
    Returns a dict of plain Python values (JSON as it stands); with e the error rate:
      pixels, bins, error_rate;
      auroc_error_detection  the uncertainty as the detector of wrong pixels: P(u of a wrong pixel > u of a right one) +
                             P(same bin) / 2, the trapezoid over the bins = the Mann-Whitney statistic of the binned values; None
                             without a wrong or without a right pixel;
      aupr_error             the wrong pixels as positives: the step-wise average precision, sum of (recall step) * precision
                             over the non-empty bins from the most to the least uncertain; None without a wrong pixel;
      sparsification         {"fraction_removed", "error", "ideal"} at the M + 1 bin edges: entry k removes the k most uncertain
                             bins; error = wrong / kept among the kept pixels, ideal = max(e - f, 0) / (1 - f) at the removed
                             fraction f (the wrong pixels removed first; formed as max(wrong - removed, 0) / kept from the
                             integers); None where nothing is kept;
      ause                   the area between error / e and ideal / e, trapezoids over fraction_removed on the entries that keep
                             a pixel (the curve ends where only the lowest non-empty bin is left: a bin cannot be split);
      aurg                   the area between the random baseline (constant e) and the curve, (1 - error / e), likewise;
                             ause and aurg are None when e is 0;
      patches, thresholds    the patches counted; k / M for k = 0 .. M: a patch whose bin is >= k is uncertain at threshold k / M;
      p_accurate_given_certain, p_uncertain_given_inaccurate, pavpu   per threshold (Mukhoti & Gal 2018): n_ac / (n_ac + n_ic),
                             n_iu / (n_ic + n_iu), (n_ac + n_iu) / patches; None on an empty denominator;
      pavpu_max, pavpu_max_threshold, pavpu_mean   the largest pavpu, the first threshold that reaches it, the mean over the
                             thresholds; None without patches."""
    pix, patch = np.asarray(pix), np.asarray(patch)
    if pix.ndim != 2 or pix.shape[1] != 2 or patch.shape != pix.shape:
        raise ValueError(f"expected pix [M,2] and patch [M,2], got {pix.shape} and {patch.shape}")
    M = int(pix.shape[0])
    n, wrong = pix[:, 0].astype(np.float64), pix[:, 1].astype(np.float64)
    right = n - wrong
    N, n_wrong, n_right = n.sum(), wrong.sum(), right.sum()
    res: Dict[str, object] = {"pixels": int(pix[:, 0].sum()), "bins": M, "error_rate": float(n_wrong / N) if N else None}

    auroc = None
    if n_wrong and n_right:
        below = np.concatenate([[0.0], np.cumsum(right)[:-1]])          # right pixels in the lower bins
        auroc = float((wrong * (below + 0.5 * right)).sum() / (n_wrong * n_right))
    res["auroc_error_detection"] = auroc

    aupr = None
    if n_wrong:
        has = n[::-1] > 0
        precision = np.cumsum(wrong[::-1])[has] / np.cumsum(n[::-1])[has]
        aupr = float((wrong[::-1][has] / n_wrong * precision).sum())
    res["aupr_error"] = aupr

    removed = np.concatenate([[0.0], np.cumsum(n[::-1])])               # entry k: the k most uncertain bins
    kept = N - removed
    kept_wrong = n_wrong - np.concatenate([[0.0], np.cumsum(wrong[::-1])])
    some = kept > 0
    error = kept_wrong[some] / kept[some]
    ideal = np.maximum(n_wrong - removed[some], 0.0) / kept[some]
    frac = removed[some] / N if N else removed[some]
    pad = [None] * int((~some).sum())
    res["sparsification"] = {"fraction_removed": [float(f) for f in removed / N] if N else [None] * (M + 1),
                             "error": [float(v) for v in error] + pad, "ideal": [float(v) for v in ideal] + pad}
    ause = aurg = None
    if n_wrong:
        e = n_wrong / N
        step = np.diff(frac)

        def area(d):
            return float((step * 0.5 * (d[1:] + d[:-1])).sum())
        ause, aurg = area((error - ideal) / e), area(1.0 - error / e)
    res["ause"], res["aurg"] = ause, aurg

    count, bad = patch[:, 0].astype(np.float64), patch[:, 1].astype(np.float64)
    good = count - bad
    total = count.sum()
    n_ac = np.concatenate([[0.0], np.cumsum(good)])                     # entry k: the accurate patches in the bins below k
    n_ic = np.concatenate([[0.0], np.cumsum(bad)])
    n_iu = bad.sum() - n_ic

    def ratio(a, b):
        return [float(x / y) if y else None for x, y in zip(a, b)]
    res["patches"] = int(patch[:, 0].sum())
    res["thresholds"] = [k / M for k in range(M + 1)]
    res["p_accurate_given_certain"] = ratio(n_ac, n_ac + n_ic)
    res["p_uncertain_given_inaccurate"] = ratio(n_iu, n_ic + n_iu)
    res["pavpu"] = pavpu = ratio(n_ac + n_iu, np.full(M + 1, total))
    if total:
        best = int(np.argmax(pavpu))
        res.update(pavpu_max=pavpu[best], pavpu_max_threshold=best / M, pavpu_mean=float(np.mean(pavpu)))
    else:
        res.update(pavpu_max=None, pavpu_max_threshold=None, pavpu_mean=None)
    return res


class SegmentationUncertainty:
    """Does the uncertainty of a multi-sample prediction mark the pixels it gets wrong?  (Beyond the reference, which never scores
    its samples' spread.)  Over the pixels SegmentationConfusion counts, with the class it counts, every measure of `measures` —
    the per-pixel maps of DenoisingModel.predict_multiple, at the prediction's resolution — is upsampled as the prediction is,
    put on the scale [0, ln K] and counted into `bins` equal-width bins, per pixel and per aligned `patch` x `patch` patch, split
    by wrong / right: one HIP kernel (ccdm_uncscore) without a full-resolution tensor.  The scale: both measures are at most
    the entropy of the mean over the K channels, which is at most ln K; ranges[m] = float32(ln K) for both, and a value beyond
    it lands in the last bin.
      pix_count, patch_count   int64 [len(measures), bins, 2]: {pixels, wrong pixels}, {patches, inaccurate patches}, accumulated
                               on the device.
    update(prediction, maps, labels): prediction and labels as SegmentationConfusion.update takes them, maps a dict with an fp32
    [B,h,w] tensor per measure.  result(names) is {"pixels", "bins", "patch", "range", "measures": {name:
    uncertainty_from_counts(...)}} for the measures `names` (default: all)."""

    def __init__(self, num_classes: int, device=None, bins: int = 256, patch: int = 8, measures: Sequence[str] = UNCERTAINTY_MEASURES):
        self.num_classes = _check_num_classes(num_classes)
        self.bins, self.patch, self.measures = check_uncertainty_settings(bins, patch, measures)
        self.C = self.num_classes - 1
        self.range = float(np.float32(np.log(self.num_classes)))
        self.device = _cuda_device(device, "SegmentationUncertainty")
        self._pix = torch.zeros((len(self.measures), self.bins, 2), dtype=torch.int64, device=self.device)
        self._patch = torch.zeros((len(self.measures), self.bins, 2), dtype=torch.int64, device=self.device)

    @property
    def pix_count(self) -> torch.Tensor:
        return self._pix.cpu()

    @property
    def patch_count(self) -> torch.Tensor:
        return self._patch.cpu()

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, maps: Dict[str, torch.Tensor], labels: torch.Tensor) -> None:
        import ctypes
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        missing = [m for m in self.measures if m not in maps]
        if missing:
            raise ValueError(f"maps: no map for {missing} (got {sorted(maps)})")
        probs, ps, cls, h, w = prediction_form(prediction, self.num_classes, self.device)
        lab = _labels_u8(labels, self.device)
        B, H, W = (int(s) for s in lab.shape)
        for m in self.measures:
            if tuple(maps[m].shape) != (B, h, w):
                raise ValueError(f"maps[{m!r}]: expected {(B, h, w)} = [B,h,w] of the prediction, got {tuple(maps[m].shape)}")
        if B == 0:
            return
        stack = torch.stack([maps[m].to(self.device, torch.float32) for m in self.measures]).contiguous()
        U = len(self.measures)
        ranges = (ctypes.c_float * U)(*([self.range] * U))
        hip.check(hip.load().ccdm_uncscore(*prediction_args(probs, ps, cls), lab.data_ptr(), stack.data_ptr(), ranges, B, h, w, H, W,
                                           self.num_classes, U, self.bins, self.patch, self._pix.data_ptr(), self._patch.data_ptr(),
                                           None, 0, torch.cuda.current_stream(self.device).cuda_stream), "uncscore")

    def result(self, names: Optional[Sequence[str]] = None) -> Dict[str, object]:
        names = self.measures if names is None else tuple(names)
        unknown = [m for m in names if m not in self.measures]
        if unknown:
            raise ValueError(f"names: {unknown} not among the measures {list(self.measures)}")
        pix, patch = self.pix_count.numpy(), self.patch_count.numpy()
        scores = {m: uncertainty_from_counts(pix[self.measures.index(m)], patch[self.measures.index(m)]) for m in names}
        return {"pixels": int(pix[0, :, 0].sum()), "bins": self.bins, "patch": self.patch, "range": self.range, "measures": scores}


# ------------------------------------------------------------------------------------------------ prediction export
EXPORT_OUTPUTS = ("train_id", "label_id", "color")


def _export(probs, ps, cls, B, h, w, H, W, K, scored, outputs, id_table, color_table, device) -> Dict[str, torch.Tensor]:
    outputs = tuple(outputs)
    if not outputs or any(o not in EXPORT_OUTPUTS for o in outputs):
        raise ValueError(f"outputs: {outputs!r} (a non-empty subset of {list(EXPORT_OUTPUTS)})")
    if not 2 <= K <= 32:
        raise ValueError(f"{K} classes (the kernel takes 2..32 channels, the last one the ignore class)")
    if id_table is None or color_table is None:
        if K != NUM_CLASSES:
            raise ValueError(f"{K} classes: the default tables are Cityscapes' ({NUM_CLASSES} classes), pass id_table and color_table")
        id_table = TRAIN_ID_TO_ID if id_table is None else id_table
        color_table = TRAIN_ID_TO_COLOR if color_table is None else color_table
    idt = torch.as_tensor(np.asarray(id_table, dtype=np.uint8)).reshape(-1).to(device)
    colt = torch.as_tensor(np.asarray(color_table, dtype=np.uint8)).reshape(-1).to(device)
    if idt.numel() != K or colt.numel() != 3 * K:
        raise ValueError(f"id_table / color_table: expected [{K}] and [{K},3], got {idt.numel()} and {colt.numel()} values")
    out = {o: torch.empty((B, H, W, 3) if o == "color" else (B, H, W), dtype=torch.uint8, device=device) for o in outputs}
    ptr = {o: out[o].data_ptr() if o in out and B > 0 else None for o in EXPORT_OUTPUTS}
    if B > 0:
        hip.check(hip.load().ccdm_segexport(*prediction_args(probs, ps, cls), B, h, w, H, W, K, scored, idt.data_ptr(), colt.data_ptr(),
                                            ptr["train_id"], ptr["label_id"], ptr["color"],
                                            torch.cuda.current_stream(device).cuda_stream), "segexport")
    return out


@torch.no_grad()
def export_predictions(prediction: torch.Tensor, size: Sequence[int], *, outputs: Sequence[str] = ("label_id", "color"), id_table=None,
                       color_table=None, num_classes: Optional[int] = None, device=None) -> Dict[str, torch.Tensor]:
    """The class map of `prediction` at `size` = (H, W) as uint8 GPU tensors, a dict with the requested `outputs`:
      "train_id" [B,H,W]    the argmax over the first K-1 channels (the ignore channel is dropped) of the prediction upsampled
                            bilinearly to (H, W): the class SegmentationConfusion counts for that pixel, bit for bit;
      "label_id" [B,H,W]    id_table[train_id] (the reference's submit/<n>_id.png);
      "color"    [B,H,W,3]  color_table[train_id] (its debug/<n>_rgb.png).
    prediction: every form SegmentationConfusion.update takes ([B,K,h,w] float, integer or bool one-hot, or a class map [B,h,w],
    whose K is `num_classes`, default 20).  id_table [K] / color_table [K,3]: default Cityscapes' (K = 20 only).  One HIP kernel
    (ccdm_segexport); never builds a full-resolution probability tensor."""
    device = _cuda_device(device if device is not None else (prediction.device if prediction.is_cuda else None), "the prediction export")
    if prediction.ndim == 4:
        K = int(prediction.shape[1])
        if num_classes is not None and int(num_classes) != K:
            raise ValueError(f"prediction has {K} channels, num_classes = {num_classes}")
    else:
        K = int(num_classes) if num_classes is not None else (len(id_table) if id_table is not None else NUM_CLASSES)
    probs, ps, cls, h, w = prediction_form(prediction, K, device)
    H, W = int(size[0]), int(size[1])
    return _export(probs, ps, cls, int(prediction.shape[0]), h, w, H, W, K, K - 1, outputs, id_table, color_table, device)


@torch.no_grad()
def export_labels(labels: torch.Tensor, *, outputs: Sequence[str] = ("label_id",), id_table=None, color_table=None,
                  num_classes: int = NUM_CLASSES, device=None) -> Dict[str, torch.Tensor]:
    """Labels [B,H,W] in train ids as the same uint8 images (the reference's label/<n>_label.png is "label_id"): values 0..K-1 go
    through the tables, anything else (255, negative, ...) counts as the ignore class K-1.  The same kernel as
    export_predictions, on the labels as a class map at their own resolution, with all K classes scored."""
    if labels.ndim != 3:
        raise ValueError(f"labels: expected [B,H,W], got {tuple(labels.shape)}")
    device = _cuda_device(device if device is not None else (labels.device if labels.is_cuda else None), "the prediction export")
    K = int(num_classes)
    lab = labels.to(device)
    if lab.dtype == torch.bool:
        lab = lab.to(torch.uint8)
    lab = torch.where((lab < 0) | (lab > K - 1), torch.full_like(lab, K - 1), lab).to(torch.uint8).contiguous()
    B, H, W = (int(v) for v in lab.shape)
    return _export(None, 0, lab, B, H, W, H, W, K, K, outputs, id_table, color_table, device)


class PredictionWriter:
    """The reference Evaluator's `save_preds`: per image three PNGs under <directory>/outputs/<split>/
      submit/<n>_id.png     the prediction in label ids (mode L): what the official evaluation script and the benchmark server read;
      debug/<n>_rgb.png     the prediction in class colours (mode RGB);
      label/<n>_label.png   the labels in label ids (mode L);
    n counts the images from 1 across write() calls.  pred_list / label_list keep the submit and label paths in order (what the
    official script takes).  The maps come from export_predictions / export_labels; PNG encoding is host work (PIL)."""

    def __init__(self, directory: str, split: str = "val", id_table=None, color_table=None):
        base = os.path.join(directory, "outputs", split)
        self.path_submit, self.path_debug, self.path_label = (os.path.join(base, d) for d in ("submit", "debug", "label"))
        for d in (self.path_submit, self.path_debug, self.path_label):
            os.makedirs(d, exist_ok=True)
        self.id_table, self.color_table = id_table, color_table
        self.images_cnt = 0
        self.pred_list: List[str] = []
        self.label_list: List[str] = []

    def write(self, prediction: torch.Tensor, labels: torch.Tensor, size: Optional[Sequence[int]] = None) -> None:
        """prediction: any form export_predictions takes; labels: [B,H,W] train ids; size: (H, W) of the images, default the labels'."""
        from PIL import Image
        size = tuple(int(v) for v in (size if size is not None else labels.shape[1:]))
        K = int(prediction.shape[1]) if prediction.ndim == 4 else NUM_CLASSES
        pred = export_predictions(prediction, size, outputs=("label_id", "color"), id_table=self.id_table, color_table=self.color_table,
                                  num_classes=K)
        lab = export_labels(labels, outputs=("label_id",), id_table=self.id_table, color_table=self.color_table, num_classes=K)
        ids, rgb, lids = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in (pred["label_id"], pred["color"], lab["label_id"]))
        for i in range(ids.shape[0]):
            n = self.images_cnt + i + 1
            f_id, f_rgb, f_lab = (os.path.join(self.path_submit, f"{n}_id.png"), os.path.join(self.path_debug, f"{n}_rgb.png"),
                                  os.path.join(self.path_label, f"{n}_label.png"))
            Image.fromarray(np.ascontiguousarray(ids[i], dtype=np.uint8)).save(f_id)
            Image.fromarray(np.ascontiguousarray(rgb[i], dtype=np.uint8)).save(f_rgb)
            Image.fromarray(np.ascontiguousarray(lids[i], dtype=np.uint8)).save(f_lab)
            self.pred_list.append(f_id)
            self.label_list.append(f_lab)
        self.images_cnt += int(ids.shape[0])


# ------------------------------------------------------------------------------------------------ data
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class CityscapesVal(torch.utils.data.Dataset):
    """The Cityscapes split the reference's `datasets.cityscapes.validation_dataset` reads with a "resize" pipeline, re-stated
    with PIL and numpy.  Items are (image [3,H,W] fp32, one-hot labels [20,H,W] fp32, original labels [H0,W0] int64):
      pairs   leftImg8bit/<split>/<city>/*_leftImg8bit.png with gtFine/<split>/<city>/*_gtFine_labelIds.png, sorted by city and
              file name (torchvision walks `os.listdir`, whose order depends on the filesystem);
      image   PIL resize to target_size = (H, W) with BILINEAR, /255, normalised with the ImageNet mean and std;
      labels  PIL resize with NEAREST, label id -> train id (not evaluated -> 19), one-hot over 20 classes;
      original labels: the full-resolution train ids.  The reference hands `infer_step` the raw label ids here, which do not
              compare with train-id predictions; this is what its evaluator needs.
    max_size: the subset random_split(dataset, [max_size, n - max_size], generator=Generator().manual_seed(1)) keeps, in its order.
    return_instances: items get a fourth entry, the values of *_gtFine_instanceIds.png [H0,W0] int32 (what the official script's
    instance-level scores read).
    root defaults to ${TMPDIR}/cityscapes/ (the reference's BASE_PATH)."""

    def __init__(self, root: Optional[str] = None, split: str = "val", target_size: Sequence[int] = (256, 512),
                 max_size: Optional[int] = None, return_instances: bool = False):
        self.return_instances = bool(return_instances)
        self.root = os.path.expandvars(root if root else "${TMPDIR}/cityscapes/")
        self.split = split
        self.target_size = (int(target_size[0]), int(target_size[1]))
        img_dir = os.path.join(self.root, "leftImg8bit", split)
        if not os.path.isdir(img_dir):
            raise FileNotFoundError(f"{img_dir}: no Cityscapes images (set dataset_path to the directory holding leftImg8bit/ and gtFine/)")
        self.pairs: List[Tuple[str, str]] = []
        for city in sorted(os.listdir(img_dir)):
            for img in sorted(glob.glob(os.path.join(img_dir, city, "*_leftImg8bit.png"))):
                lbl = os.path.join(self.root, "gtFine", split, city,
                                   os.path.basename(img)[:-len("_leftImg8bit.png")] + "_gtFine_labelIds.png")
                if not os.path.exists(lbl):
                    raise FileNotFoundError(f"{lbl}: the label of {img} is missing")
                if self.return_instances and not os.path.exists(lbl.replace("labelIds", "instanceIds")):
                    raise FileNotFoundError(f"{lbl.replace('labelIds', 'instanceIds')}: the instance image of {img} is missing")
                self.pairs.append((img, lbl))
        self.indices = list(range(len(self.pairs)))
        if max_size:
            n = len(self.pairs)
            if max_size > n:
                raise ValueError(f"dataset_val_max_size = {max_size} > {n} images in {img_dir}")
            self.indices = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:max_size].tolist()
        self.lut = id_to_train_id_lut()

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        from PIL import Image
        img_path, lbl_path = self.pairs[self.indices[i]]
        H, W = self.target_size
        with Image.open(img_path) as im:
            img = np.asarray(im.convert("RGB").resize((W, H), Image.BILINEAR))
        with Image.open(lbl_path) as lb:
            ids = np.asarray(lb)
            small = np.asarray(lb.resize((W, H), Image.NEAREST))
        image = torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255)
        image = image.sub(torch.tensor(IMAGENET_MEAN)[:, None, None]).div(torch.tensor(IMAGENET_STD)[:, None, None])
        train = torch.from_numpy(self.lut[small.astype(np.int64) & 255].astype(np.int64))
        onehot = torch.nn.functional.one_hot(train, NUM_CLASSES).permute(2, 0, 1).float()
        original = torch.from_numpy(self.lut[ids.astype(np.int64) & 255].astype(np.int64))
        if self.return_instances:
            with Image.open(lbl_path.replace("labelIds", "instanceIds")) as im:
                inst = np.array(im).astype(np.int32)
            if inst.shape != ids.shape:
                raise ValueError(f"{lbl_path}: the instance image is {inst.shape}, the labels are {ids.shape}")
            return image, onehot, original, torch.from_numpy(inst)
        return image, onehot, original


class SyntheticCityscapes(torch.utils.data.Dataset):
    """Cityscapes-shaped stand-in: image [3,h,w], one-hot labels [20,h,w] and original train-id labels at `original_size`:
    a few class blobs over a background class, with ignore pixels (19 and 255) sprinkled in.  Deterministic per (seed, item).
    instances: items get a fourth entry, an instance image [H0,W0] int32 as Cityscapes writes it: blob number j of a class with
    instances (person .. bicycle) is the instance label id * 1000 + j on the pixels it still owns, every other pixel holds its
    label id (0 where the label is ignored).  The first three entries do not depend on it."""

    def __init__(self, size: int = 4, resolution: Sequence[int] = (32, 32), original_size: Sequence[int] = (64, 96), seed: int = 0,
                 instances: bool = False):
        self.instances = bool(instances)
        self.size, self.seed = int(size), int(seed)
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.original_size = (int(original_size[0]), int(original_size[1]))

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed * 100003 + i)
        H0, W0 = self.original_size
        yy, xx = np.mgrid[0:H0, 0:W0] / np.array([H0, W0])[:, None, None]
        lab = np.full((H0, W0), rng.integers(0, 19), dtype=np.int64)
        blobs = []
        for _ in range(4):
            cy, cx, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.3)
            blobs.append(((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, int(rng.integers(0, 19))))
            lab[blobs[-1][0]] = blobs[-1][1]
        lab[rng.random((H0, W0)) < 0.03] = IGNORE_CLASS
        lab[rng.random((H0, W0)) < 0.01] = 255
        h, w = self.resolution
        ry = np.minimum((np.arange(h) * H0) // h, H0 - 1)
        rx = np.minimum((np.arange(w) * W0) // w, W0 - 1)
        small = lab[ry][:, rx]
        small = np.where(small == 255, IGNORE_CLASS, small)
        onehot = torch.nn.functional.one_hot(torch.from_numpy(small), NUM_CLASSES).permute(2, 0, 1).float()
        colour = rng.uniform(-1, 1, (NUM_CLASSES, 3)).astype(np.float32)
        image = colour[small].transpose(2, 0, 1) + 0.2 * rng.standard_normal((3, h, w)).astype(np.float32)
        item = (torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)), onehot, torch.from_numpy(lab))
        if not self.instances:
            return item
        ids = np.asarray(TRAIN_ID_TO_ID, dtype=np.int32)
        inst = ids[np.where((lab < 0) | (lab > IGNORE_CLASS), IGNORE_CLASS, lab)]
        for j, (mask, c) in enumerate(blobs, start=1):            # a later blob owns the pixels it painted over
            if ids[c] >= 24:                                        # the labels with instances: person (24) .. bicycle (33)
                inst[mask & (lab == c)] = ids[c] * 1000 + j
        return item + (torch.from_numpy(inst),)


def make_segmentation_dataset(params: dict):
    """`dataset_file` "...synthetic..." -> SyntheticCityscapes, else CityscapesVal at dataset_path (default ${TMPDIR}/cityscapes/).
    The size comes from dataset_pipeline_val_settings.target_size (the reference's "resize" setting), the subset from
    dataset_val_max_size; the stand-in's original label size from the build-owned key `original_size`.  With
    evaluation.cityscapes_script_instances the items carry the instance image as a fourth entry."""
    settings = params.get("dataset_pipeline_val_settings") or {}
    max_size = params.get("dataset_val_max_size", None)
    instances = bool((params.get("evaluation") or {}).get("cityscapes_script_instances", False))
    if "synthetic" in params["dataset_file"]:
        return SyntheticCityscapes(size=max_size or 4, resolution=settings.get("target_size", (32, 32)),
                                   original_size=params.get("original_size", (64, 96)), instances=instances)
    return CityscapesVal(params.get("dataset_path") or None, "val", settings.get("target_size", (256, 512)), max_size,
                         return_instances=instances)


# ------------------------------------------------------------------------------------------------ evaluation
RESOLUTIONS = ("original", "dataloader")


def _feature_encoder(params: dict, synthetic_weights_seed: Optional[int], device):
    fce = params.get("feature_cond_encoder") or {"type": "none"}
    if fce.get("type", "none") == "none":
        return None
    if "dino" not in fce["type"]:
        raise ValueError(f"feature_cond_encoder.type: {fce['type']!r} (expected 'none' or 'dino')")
    from .dino import DinoViT, make_synthetic_vit_state_dict
    model_type = fce.get("model", "dino_vits8")
    path = fce.get("weights")
    if path:
        path = os.path.expanduser(os.path.expandvars(path))
        if not os.path.exists(path):
            raise FileNotFoundError(f"feature_cond_encoder.weights: {path} does not exist (the {model_type} checkpoint's state_dict)")
        sd = torch.load(path, map_location="cpu", weights_only=True)
    elif synthetic_weights_seed is not None:
        sd = make_synthetic_vit_state_dict(model_type, synthetic_weights_seed)
    else:
        raise ValueError("feature_cond_encoder.type is 'dino' but feature_cond_encoder.weights names no checkpoint: set it to the "
                         f"{model_type} weights file (there is no hub download)")
    return DinoViT(model_type, bool(fce.get("train", False)), fce.get("conditioning", "concat_pixels_concat_features"),
                   stride=int(fce.get("output_stride", 8)), state_dict=sd, device=str(device))


@torch.no_grad()
def eval_segmentation(params: dict, dataset=None, device=None, model=None, synthetic_weights_seed: Optional[int] = None) -> Dict[str, object]:
    """The reference Evaluator's inference loop (eval_cdm.py: `infer_step` over the validation loader, ignite's IoU / mIoU and its
    own soft mIoU), without ignite.  Per batch: feature condition (DinoViT when feature_cond_encoder.type is dino), prediction
    through evaluation.predict_multiple (`evaluations`, `evaluation_vote_strategy`, the `evaluation:` section), the labels of
    `evaluation.resolution` ("original": the full-resolution labels, "dataloader" (default): the argmax of the one-hot labels),
    and both confusion matrices (SegmentationConfusion).  The checkpoint is `load_from`'s "average_model".
    `evaluation.save_predictions` (default off): also write every prediction and its labels as PNGs at the scored resolution under
    `output_path` (PredictionWriter); the result then holds "pred_list" / "label_list".
    `evaluation.cityscapes_script` (default off): also score every batch as the official Cityscapes script scores the written PNGs
    (cityscapes_scores.CityscapesScores: the prediction's label ids against id_table[labels], the label ids PredictionWriter
    writes, every ignored label as id 0; what the reference's `run_inference` hands its vendored cs_eval.py).  The result then
    holds "cs_script", the script's result dictionary, also written to <output_path>/cs_script_results.json; perImageScores is
    keyed by the written submit/<n>_id.png paths when save_predictions is on, else by the image number.
    `evaluation.cityscapes_script_instances` (default off): the instance-weighted scores (iIoU) too, from the dataset's instance
    images; needs `resolution: original` (resized labels have no instance image).
    `evaluation.calibration` (default off): also score how well the probabilities are calibrated (SegmentationCalibration, one
    more HIP launch pair per batch on the tensor and labels the confusion matrices get; `evaluation.calibration_bins`, default
    15).  The result then holds "calibration" (calibration_from_counts), also written to <output_path>/calibration.json.  A
    one-hot prediction (`step_T_sample: majority` with one evaluation) is scored too: its confidence is 1 wherever the
    upsampled map is not mixed, which the log says.
    `evaluation.boundary` (default off): also score the contours (SegmentationBoundary: one ccdm_segexport launch and one
    ccdm_segboundary launch per width per batch, on the tensor and labels the confusion matrices get).
    `evaluation.boundary_widths` (default ["ratio:0.02"]) lists the band widths, each an int (pixels, 1..64) or "ratio:R" (R times
    the diagonal of the scored size); a bad list raises before anything is sampled.  The result then holds "boundary"
    (SegmentationBoundary.result: Boundary IoU and trimap IoU per width), also written to <output_path>/boundary.json.
    `evaluation.contour_f` (default off): also score the boundary F-score (SegmentationContourF: one ccdm_segexport launch and one
    ccdm_contourf launch per tolerance per batch, on the tensor and labels the confusion matrices get).
    `evaluation.contour_tolerances` (default ["ratio:0.0075"]) lists the tolerances, each an int (pixels, 1..32) or "ratio:R" (R
    times the diagonal of the scored size); a bad list raises before anything is sampled.  The result then holds "contour_f"
    (SegmentationContourF.result: the BF score per class, per image and pooled, per tolerance), also written to
    <output_path>/contour_f.json.
    `evaluation.uncertainty` (default off): also score whether the samples' spread marks the wrong pixels (SegmentationUncertainty,
    one more HIP launch per batch).  Needs `evaluations` >= 2: the batch's prediction then comes from model.predict_multiple with
    maps ("mean", "entropy", "mutual_info") — the same passes, mean and Philox calls as without the key — and "mean" feeds every
    other scorer.  `evaluation.uncertainty_bins` (default 256, 2..512), `evaluation.uncertainty_patch` (default 8; 2, 4, 8 or 16)
    and `evaluation.uncertainty_measures` (default both maps); a bad value, or one evaluation, raises before anything is sampled.
    Under the majority vote mutual_info equals entropy by construction, so only entropy is scored there.  The result then holds
    "uncertainty" (SegmentationUncertainty.result), also written to <output_path>/uncertainty.json.
    The params key `sampling: {temperature: ..., truncation: ..., views: [...], tiles: [...]}` (evaluation.sampling_keywords; each optional) is handed
    to every sampling call and to predict_multiple and echoed as "sampling" in the result; an unknown key under it raises before
    anything is sampled; without the key nothing changes.  With `views` the feature encoder, where there is one, runs once per view on
    the mirrored image (evaluation.view_features); with `tiles`, once per tile on the cropped image (evaluation.tile_features).
    `model`: a ready DenoisingModel-like callable (tests inject one); default: built from `params`."""
    from . import evaluation as E
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1:
        raise NotImplementedError(f"eval_segmentation runs on one rank: sharding the evaluation over WORLD_SIZE = {world} ranks is not "
                                  "built yet (launch it without torchrun)")
    device = torch.device(device if device is not None else "cuda")
    section = params.get("evaluation") or {}
    resolution = section.get("resolution", "dataloader")
    sampling = E.sampling_keywords(params)
    script, script_instances = bool(section.get("cityscapes_script", False)), bool(section.get("cityscapes_script_instances", False))
    if script_instances and not script:
        raise ValueError("evaluation.cityscapes_script_instances needs evaluation.cityscapes_script")
    if script_instances and resolution != "original":
        raise ValueError(f"evaluation.cityscapes_script_instances needs evaluation.resolution: original (got {resolution!r}): "
                         "resized labels have no instance image")
    boundary_widths = None
    if section.get("boundary", False):
        boundary_widths = section.get("boundary_widths", list(BOUNDARY_DEFAULT_WIDTHS))
        resolve_boundary_widths(boundary_widths)
    contour_tolerances = None
    if section.get("contour_f", False):
        contour_tolerances = section.get("contour_tolerances", list(CONTOUR_DEFAULT_TOLERANCES))
        resolve_contour_tolerances(contour_tolerances)
    unc_settings = None
    if section.get("uncertainty", False):
        unc_settings = check_uncertainty_settings(section.get("uncertainty_bins", 256), section.get("uncertainty_patch", 8),
                                                  section.get("uncertainty_measures", list(UNCERTAINTY_MEASURES)), "evaluation.uncertainty_")
        n_eval, strategy = E.vote_settings(params)
        if n_eval < 2:
            raise ValueError(f"evaluation.uncertainty needs evaluation.evaluations >= 2 (got {n_eval}): a single pass has no sample spread")
        if strategy == "majority":      # one-hot passes: every H(p_s) is 0, mutual_info is the entropy map again
            scored = tuple(m for m in unc_settings[2] if m != "mutual_info")
            if not scored:
                raise ValueError("evaluation.uncertainty_measures: under evaluation_vote_strategy majority mutual_info equals entropy "
                                 "by construction and only entropy is scored; list entropy")
            if scored != unc_settings[2]:
                LOGGER.info("uncertainty: under the majority vote mutual_info equals entropy by construction; only entropy is scored")
            unc_settings = unc_settings[:2] + (scored,)
    dataset = dataset if dataset is not None else make_segmentation_dataset(params)
    LOGGER.info("%d images in validation dataset '%s'", len(dataset), params["dataset_file"])
    if resolution not in RESOLUTIONS:
        raise ValueError(f"evaluation.resolution: {resolution!r} is not in {list(RESOLUTIONS)}")
    evaluations, vote = E.vote_settings(params)
    loader = torch.utils.data.DataLoader(dataset, batch_size=params["batch_size"], shuffle=False, num_workers=params.get("mp_loaders", 0))
    image0, labels0 = dataset[0][:2]
    if script_instances and len(dataset[0]) < 4:
        raise ValueError("evaluation.cityscapes_script_instances: the dataset's items carry no instance image (return_instances / instances)")
    input_shapes = [tuple(image0.shape), tuple(labels0.shape)]
    num_classes = input_shapes[1][0]
    if boundary_widths is not None:            # a ratio that is too wide at the scored size, before anything is sampled
        resolve_boundary_widths(boundary_widths, dataset[0][2].shape[-2:] if resolution == "original" else labels0.shape[-2:])
    if contour_tolerances is not None:
        resolve_contour_tolerances(contour_tolerances, dataset[0][2].shape[-2:] if resolution == "original" else labels0.shape[-2:])
    encoder = _feature_encoder(params, synthetic_weights_seed, device)
    if model is None:
        model = E.build_from_params(params, input_shapes, device)
        if params.get("load_from"):
            E.load_checkpoint(model, E.expanduservars(params["load_from"]), key="average_model")
        elif synthetic_weights_seed is not None:
            from .unet_spec import make_synthetic_state_dict
            model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, synthetic_weights_seed).items()})
        E.apply_sampler_options(model, params)
    conf = SegmentationConfusion(num_classes, device)
    writer = PredictionWriter(E.expanduservars(params["output_path"])) if section.get("save_predictions", False) else None
    scores = None
    if script:
        from .cityscapes_scores import CityscapesScores
        scores = CityscapesScores(num_classes, device)
    calib = SegmentationCalibration(num_classes, device, int(section.get("calibration_bins", 15))) if section.get("calibration", False) else None
    boundary = SegmentationBoundary(num_classes, device, boundary_widths) if boundary_widths is not None else None
    contour = SegmentationContourF(num_classes, device, contour_tolerances) if contour_tolerances is not None else None
    unc = SegmentationUncertainty(num_classes, device, *unc_settings) if unc_settings is not None else None
    n_img = 0
    for image, labels, labels_orig, *rest in loader:
        image = image.to(device)
        if encoder is not None and sampling.get("views"):
            feature_condition = E.view_features(encoder, image, sampling["views"])
        elif encoder is not None and sampling.get("tiles"):
            feature_condition = E.tile_features(encoder, image, sampling["tiles"])
        else:
            feature_condition = encoder(image) if encoder is not None else None
        if unc is None:
            prediction = E.predict_multiple(model, image, params, feature_condition)
        else:           # the same passes as E.predict_multiple (evaluations >= 2), with the two uncertainty maps folded alongside the mean
            multi = model.predict_multiple(image, feature_condition, num_evaluations=evaluations, voting=vote,
                                           maps=("mean", "entropy", "mutual_info"), **sampling)
            prediction = multi["mean"]
        target = labels_orig if resolution == "original" else labels.argmax(dim=1)
        target = target.to(device)
        conf.update(prediction, target)
        if unc is not None:
            unc.update(prediction, multi, target)
        if calib is not None:
            calib.update(prediction, target)
        if boundary is not None:
            boundary.update(prediction, target)
        if contour is not None:
            contour.update(prediction, target)
        if writer is not None:
            writer.write(prediction, target, tuple(target.shape[1:]))
        if scores is not None:
            gt_ids = export_labels(target, outputs=("label_id",), num_classes=num_classes)["label_id"]
            scores.update(prediction, gt_ids, rest[0] if script_instances else None,
                          writer.pred_list[-image.shape[0]:] if writer is not None else None)
        n_img += image.shape[0]
    iou, iou_soft = conf.iou(), conf.iou_soft()
    names = TRAIN_ID_NAMES if conf.C == len(TRAIN_ID_NAMES) else tuple(str(c) for c in range(conf.C))
    for name, a, b in zip(names, iou.tolist(), iou_soft.tolist()):
        LOGGER.info("IoU %-14s %.4f  (soft %.4f)", name, a, b)
    res = {"mIoU": float(iou.mean()), "IoU": iou.tolist(), "mIoU_soft": float(iou_soft.mean()), "IoU_soft": iou_soft.tolist(),
           "confusion": conf.confusion.tolist(), "images": n_img, "resolution": resolution, "evaluations": evaluations, "vote": vote}
    if params.get("sampling") is not None:
        res["sampling"] = dict(sampling)
    if writer is not None:
        res["pred_list"], res["label_list"] = list(writer.pred_list), list(writer.label_list)
        LOGGER.info("%d predictions written under %s", len(writer.pred_list), os.path.dirname(writer.path_submit))
    if scores is not None:
        res["cs_script"] = scores.result()
        path = _write_json(E.expanduservars(params["output_path"]), "cs_script_results", res["cs_script"])
        LOGGER.info("Cityscapes script: IoU classes %.4f  iIoU classes %.4f  IoU categories %.4f  iIoU categories %.4f (%s)",
                    *(res["cs_script"][k] for k in ("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories",
                                                    "averageScoreInstCategories")), path)
    if calib is not None:
        res["calibration"] = cal = calib.result(names)
        path = _write_json(E.expanduservars(params["output_path"]), "calibration", cal)
        if calib.class_map_updates:
            LOGGER.info("calibration: the prediction is a one-hot map (confidence 1 wherever the upsampled map is not mixed): "
                        "the scores below are degenerate")
        LOGGER.info("calibration over %d pixels, %d bins: ECE %s  NLL %s  Brier %s  AUROC (error detection) %s (%s)", cal["pixels"],
                    cal["bins"], *("n/a" if cal[k] is None else f"{cal[k]:.4f}" for k in ("ece", "nll", "brier", "auroc_error_detection")),
                    path)
    if boundary is not None:
        res["boundary"] = bnd = boundary.result(names)
        path = _write_json(E.expanduservars(params["output_path"]), "boundary", bnd)
        for w in bnd["widths"]:
            s = bnd["by_width"][str(w["entry"])]
            LOGGER.info("boundary width %s (%s px): Boundary mIoU %s  trimap mIoU %.4f over %d pixels (%s)", w["entry"],
                        ", ".join(str(p) for p in w["pixels"]), "n/a" if s["mean_boundary_iou"] is None else f"{s['mean_boundary_iou']:.4f}",
                        s["trimap_miou"], s["trimap_pixels"], path)
    if contour is not None:
        res["contour_f"] = ctf = contour.result(names)
        path = _write_json(E.expanduservars(params["output_path"]), "contour_f", ctf)
        for t in ctf["tolerances"]:
            s = ctf["by_tolerance"][str(t["entry"])]
            LOGGER.info("contour tolerance %s (%s px): mean BF score %s  pooled %s over %d scored cells (%s)", t["entry"],
                        ", ".join(str(p) for p in t["pixels"]),
                        *("n/a" if v is None else f"{v:.4f}" for v in (s["mean_bf_score"], s["pooled"]["mean_bf_score"])),
                        sum(s["images"].values()), path)
    if unc is not None:
        res["uncertainty"] = u = unc.result()
        path = _write_json(E.expanduservars(params["output_path"]), "uncertainty", u)
        for m, s in u["measures"].items():
            LOGGER.info("uncertainty %s over %d pixels, %d bins, %d x %d patches: AUROC (error detection) %s  AUSE %s  PAvPU max %s (%s)", m,
                        s["pixels"], u["bins"], u["patch"], u["patch"],
                        *("n/a" if s[k] is None else f"{s[k]:.4f}" for k in ("auroc_error_detection", "ause", "pavpu_max")), path)
    LOGGER.info("mIoU %.4f  soft mIoU %.4f over %d images (resolution %s, %d evaluation(s), %s)", res["mIoU"], res["mIoU_soft"], n_img,
                resolution, evaluations, vote)
    return res
