"""LIDC uncertainty metrics: generalised energy distance, sample/expert diversity and
Hungarian-matched IoU, as the reference computes them
(/root/reference/evaluation/evaluate_lidc_uncertainty.py:27-73; duplicates in ddpm/utils.py:129-174).

The O(B*S*S'*HW*K) part — per-class intersection/union counts of every pair of label maps — runs in a HIP
kernel (ccdm_pairwise_class_counts); the host only divides integers and solves the <= 100x100 assignment
problems with scipy, exactly as the reference does, so results are bit-identical to the reference's numpy.

Beyond the reference: the soft-label scores.  What the S samples imply at a pixel, p_k = (samples saying k) / S, against the
raters' soft label there, q_k = (raters saying k) / L: `vote_joint_counts` (HIP kernel ccdm_lidcscore) counts the pixels of
every image by (class, samples saying it, raters saying it), `soft_label_scores_from_counts` derives calibration, Brier score,
cross-entropy, thresholded soft Dice and the uncertainty correlation (NCC) from those integers on the host.

Also beyond the reference: the surface distances of every sample against every rater.  `surface_distance_stats` (HIP kernel
ccdm_surfdist: an exact squared distance transform per map and class, then counts, maximum, two order statistics and two fp64 sums
per (image, sample, rater, class)), `surface_scores_from_stats` derives HD95, ASSD and the Hausdorff distance on the host.

And the lesion-level scores: `lesion_stats` (HIP kernel ccdm_lesions: connected-component labels per map and class, then per
(image, sample, rater, class) the lesions of each side and how many the other side's mask covers to each overlap threshold),
`lesion_scores_from_stats` derives lesion-wise recall, precision, F1 and the agreement on the number of lesions on the host.
`lesion_match_stats` pairs the lesions of the two maps one to one by IoU (HIP kernel ccdm_lesion_match on the same workspace: matched
pairs and the fixed-point sum of their IoUs per threshold), `lesion_match_scores_from_stats` derives panoptic, segmentation and
recognition quality on the host.

And the lesion findings of the sample SET: `sample_findings` (HIP kernel ccdm_findings: per image and class the connected components of
the pixels enough samples mark, each with the number of samples that draw it, and the components the raters agree on),
`detection_scores_from_findings` derives FROC, the sensitivity at fixed false positives per image (CPM) and average precision on the host.

And the mode summary of the samples themselves: `sample_modes` (HIP kernels ccdm_modes_distance, ccdm_modes_pam, ccdm_modes_maps:
the pairwise fixed-point distance among the S samples of an image, k-medoids on it, per-mode vote and entropy maps) says which
distinct segmentations the samples propose and which share of the samples each holds; everything stays on the device.

And the single map to report: `sample_consensus` (HIP kernels ccdm_consensus, ccdm_consensus_maps: among the S + 1 thresholded frequency
maps of an image and class the one with the largest expected IoU or Dice under the samples, in exact integers; `threshold_maps` for
the maps of given thresholds)."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip


# ------------------------------------------------------------------------------------------------ shared launch prologue and host checks
def _class_map_stacks(name: str, a_idx: torch.Tensor, b_idx: Optional[torch.Tensor], flat: bool = False,
                      expected: str = "[B,S,H,W] and [B,L,H,W]"):
    """What every launch over a sample stack a_idx [B,S,...] and a rater stack b_idx [B,L,...] (None: no raters, L = 0) starts with: both
    on the GPU, of one image count and one map size -> (a8, b8, dims), the stacks as contiguous uint8 on a_idx's device.  dims is
    (B, S, L, H, W) of the [B,S,H,W] / [B,L,H,W] maps, or with `flat` (B, S, L, HW) of trailing dimensions of any rank, flattened."""
    if a_idx.device.type != "cuda" or (b_idx is not None and b_idx.device.type != "cuda"):
        raise hip.CcdmHipError(f"{name} needs GPU tensors (no CPU path)")
    if flat:
        B, S = a_idx.shape[:2]
        a8 = a_idx.reshape(B, S, -1).to(torch.uint8).contiguous()
        b8 = b_idx.reshape(B, b_idx.shape[1], -1).to(device=a8.device, dtype=torch.uint8).contiguous()
        assert b8.shape[2] == a8.shape[2] and b8.shape[0] == B
        return a8, b8, (B, S, b8.shape[1], a8.shape[2])
    if a_idx.dim() != 4 or (b_idx is not None and (b_idx.dim() != 4 or b_idx.shape[0] != a_idx.shape[0] or b_idx.shape[2:] != a_idx.shape[2:])):
        raise ValueError(f"{name}: {tuple(a_idx.shape)} / {None if b_idx is None else tuple(b_idx.shape)} (expected {expected})")
    a8 = a_idx.to(torch.uint8).contiguous()
    b8 = None if b_idx is None else b_idx.to(device=a8.device, dtype=torch.uint8).contiguous()
    B, S, H, W = (int(v) for v in a_idx.shape)
    return a8, b8, (B, S, 0 if b8 is None else int(b8.shape[1]), H, W)


def _sample_stack(samples_idx, max_samples: int) -> Tuple[int, int, int, int]:
    """(B, S, H, W) of samples_idx, which has to be integer class maps [B,S,H,W] with 1 <= S <= max_samples and a pixel to score."""
    if not isinstance(samples_idx, torch.Tensor) or samples_idx.dim() != 4 or samples_idx.dtype.is_floating_point or samples_idx.dtype.is_complex \
            or samples_idx.dtype == torch.bool:
        raise ValueError(f"samples_idx: expected integer class maps [B,S,H,W], got {getattr(samples_idx, 'dtype', type(samples_idx).__name__)} "
                         f"{tuple(getattr(samples_idx, 'shape', ()))}")
    B, S, H, W = (int(v) for v in samples_idx.shape)
    if not 1 <= S <= max_samples:
        raise ValueError(f"samples_idx: S={S} samples per image (expected 1 to {max_samples})")
    if H * W < 1:
        raise ValueError(f"samples_idx: empty maps {H}x{W}")
    return B, S, H, W


def _scored_classes(num_classes: int) -> List[int]:
    """The classes a score is taken over: 1..K-1 (the reference's distance drops class 0), class 0 when K == 1."""
    return list(range(1, num_classes)) if num_classes > 1 else [0]


def _workspace(nbytes: int, device) -> torch.Tensor:
    """A kernel's workspace of at least `nbytes` bytes (and never empty), as int32."""
    return torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.int32, device=device)


def _mean_of_image_means(values, mask):
    """The mean over the images of the mean over an image's cells under `mask`; an image without one is left out, None: every image is."""
    per_image = [float(values[b][mask[b]].mean()) for b in range(len(values)) if mask[b].any()]
    return float(np.mean(per_image)) if per_image else None


def _check_cells(stats: Dict[str, object], first: str, second: str, class_names, need_image: Optional[str] = None):
    """The per-cell arrays stats[first], stats[second] as int64 [B,S,L,C] and the scored classes, C of them like `class_names` if given;
    need_image: the name of a caller that scores at least one image."""
    a, b = np.asarray(stats[first]).astype(np.int64), np.asarray(stats[second]).astype(np.int64)
    if a.ndim != 4 or b.shape != a.shape:
        raise ValueError(f"{first} {a.shape} / {second} {b.shape}: expected [B,S,L,C]")
    classes = [int(c) for c in stats["classes"]]
    if len(classes) != a.shape[3]:
        raise ValueError(f"classes: {len(classes)} entries for {a.shape[3]} scored classes")
    if class_names is not None and len(class_names) != a.shape[3]:
        raise ValueError(f"class_names: {len(class_names)} names for {a.shape[3]} scored classes")
    if need_image is not None and a.shape[0] < 1:
        raise ValueError(f"{need_image}: the stats hold no image")
    return a, b, classes


def _concat_stats(parts: Sequence[Dict[str, object]], fields: Sequence[str], settings: Sequence[str]) -> Dict[str, object]:
    """The stats of several batches as one: `fields` concatenated along the images, `settings` as the first part has them."""
    plain = lambda v: [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    out: Dict[str, object] = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in fields}
    out.update({k: plain(parts[0][k]) for k in settings})
    return out


def pairwise_class_counts(a_idx: torch.Tensor, b_idx: torch.Tensor, num_classes: int) -> np.ndarray:
    """a_idx [B,S,...] / b_idx [B,L,...] integer class maps on the GPU -> int32 [B,S,L,K,2] (intersection, union)."""
    lib = hip.load()
    a8, b8, (B, S, L, HW) = _class_map_stacks("pairwise_class_counts", a_idx, b_idx, flat=True)
    out = torch.empty((B, S, L, num_classes, 2), dtype=torch.int32, device=a8.device)
    hip.check(lib.ccdm_pairwise_class_counts(a8.data_ptr(), b8.data_ptr(), B, S, L, HW, num_classes, out.data_ptr(),
                                             torch.cuda.current_stream(a8.device).cuda_stream), "pairwise_class_counts")
    return out.cpu().numpy()


def _distance_from_counts(counts: np.ndarray) -> np.ndarray:
    """1 - mean IoU over the non-background classes; an empty union counts as IoU 1 (iou(): nan -> 1)."""
    inter, uni = counts[..., 0].astype(np.int64), counts[..., 1].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / uni
    iou[np.isnan(iou)] = 1.0
    return 1 - iou[..., 1:].mean(-1)


def batched_distance(x_idx: torch.Tensor, y_idx: torch.Tensor, num_classes: int) -> np.ndarray:
    """[B,S,...], [B,L,...] -> [B,S,L] distances (reference `batched_distance`, :33-39)."""
    return _distance_from_counts(pairwise_class_counts(x_idx, y_idx, num_classes))


def calc_batched_generalised_energy_distance(samples_dist_0: torch.Tensor, samples_dist_1: torch.Tensor,
                                             num_classes: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """GED, diversity of dist_0, diversity of dist_1 — per image (reference :42-54)."""
    cross = np.mean(batched_distance(samples_dist_0, samples_dist_1, num_classes), axis=(1, 2))
    diversity_0 = np.mean(batched_distance(samples_dist_0, samples_dist_0, num_classes), axis=(1, 2))
    diversity_1 = np.mean(batched_distance(samples_dist_1, samples_dist_1, num_classes), axis=(1, 2))
    return 2 * cross - diversity_0 - diversity_1, diversity_0, diversity_1


def batched_hungarian_matching(samples_dist_0: torch.Tensor, samples_dist_1: torch.Tensor, num_classes: int) -> List[float]:
    """Hungarian-matched IoU per image (reference :57-73)."""
    from scipy.optimize import linear_sum_assignment
    cost = batched_distance(samples_dist_0, samples_dist_1, num_classes)
    return [float((1 - cost[i])[linear_sum_assignment(cost[i])].mean()) for i in range(cost.shape[0])]


# ------------------------------------------------------------------------------------------------ soft-label scores
def vote_joint_counts(samples_idx: torch.Tensor, raters_idx: torch.Tensor, num_classes: int) -> Tuple[np.ndarray, np.ndarray]:
    """samples_idx [B,S,...] / raters_idx [B,L,...] integer class maps on the GPU -> (joint int64 [B,K,S+1,L+1], moments int64 [B,5]):
    joint[b,k,n,m] = the pixels of image b where n samples and m raters say class k; moments[b] = {sum u, sum v, sum u^2, sum v^2,
    sum u*v} of the integer Gini impurities u = S^2 - sum_k n_k^2, v = L^2 - sum_k m_k^2 (include/ccdm_hip.h, ccdm_lidcscore)."""
    lib = hip.load()
    s8, r8, (B, S, L, HW) = _class_map_stacks("vote_joint_counts", samples_idx, raters_idx, flat=True)
    joint = torch.zeros((B, num_classes, S + 1, L + 1), dtype=torch.int32, device=s8.device)
    moments = torch.zeros((B, 5), dtype=torch.int64, device=s8.device)
    hip.check(lib.ccdm_lidcscore(s8.data_ptr(), r8.data_ptr(), B, S, L, HW, num_classes, joint.data_ptr(), moments.data_ptr(),
                                 torch.cuda.current_stream(s8.device).cuda_stream), "lidcscore")
    return joint.cpu().numpy().astype(np.int64), moments.cpu().numpy()


SOFT_LABEL_THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
SOFT_LABEL_LOG_FLOOR = 1e-12            # the floor of ccdm_kl_clamped and ccdm_segcalib


def _ceil_fraction(tau, n: int) -> int:
    """ceil(tau * n) with tau read as the decimal it is written as: 0.3 * 10 is 3, not 4"""
    return math.ceil(Fraction(str(tau)) * n)


def soft_label_scores_from_counts(joint, moments, *, bins: int = 10, thresholds: Sequence[float] = SOFT_LABEL_THRESHOLDS,
                                  class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The soft-label scores behind the counts of `vote_joint_counts` (several batches: concatenated along the images), on the host
    in float64 (no GPU).  p = n/S is the sample frequency of a class at a pixel, q = m/L the rater frequency; N = all pixels.
      reliability[k]        per level bin (level n of class k is in bin min(n*bins // S, bins-1)): count, mean_p, mean_q (None: empty bin)
      ece_soft_per_class[k] sum over bins of count/N * |mean_p - mean_q|;  ece_soft: its mean over the classes 1..K-1 (the
                            reference's distance drops class 0 the same way; K == 1: class 0)
      brier_soft            1/N sum_k sum joint * (p - q)^2
      cross_entropy_soft    -1/N sum_k sum joint * q * log(max(p, 1e-12))
      dice_soft             per image, class k >= 1 (K == 1: class 0) and threshold t: P = {n >= ceil(t*S)}, Q = {m >= ceil(t*L)}
                            (ceilings in exact rational arithmetic), Dice = 2|P & Q| / (|P| + |Q|), 1 when both are empty (the
                            reference's nan -> 1); the mean over thresholds, classes and images.  dice_soft_per_threshold: per t
      ncc                   mean over images of the Pearson correlation of u and v from `moments` (variances and covariance as
                            exact integers HW*sum(x*y) - sum(x)*sum(y)); an image where either variance is 0 is left out;
                            ncc_images: the images included; None when there is none.
    The result holds lists, numbers and None only: it survives a JSON round trip."""
    joint = np.asarray(joint)
    moments = np.asarray(moments)
    if joint.ndim != 4 or moments.shape != (joint.shape[0], 5):
        raise ValueError(f"joint {joint.shape} / moments {moments.shape}: expected [B,K,S+1,L+1] and [B,5]")
    joint = joint.astype(np.int64)
    B, K, S, L = joint.shape[0], joint.shape[1], joint.shape[2] - 1, joint.shape[3] - 1
    bins = int(bins)
    if S < 1 or L < 1 or bins < 1:
        raise ValueError(f"S={S}, L={L}, bins={bins}: each must be at least 1")
    thresholds = [float(t) for t in thresholds]
    if not thresholds or any(not 0.0 < t <= 1.0 for t in thresholds):
        raise ValueError(f"thresholds: {thresholds!r} (expected values in (0, 1])")
    if class_names is not None and len(class_names) != K:
        raise ValueError(f"class_names: {len(class_names)} names for {K} classes")
    N = int(joint[:, 0].sum())
    if N <= 0:
        raise ValueError("soft_label_scores_from_counts: the counts hold no pixel")
    p = (np.arange(S + 1, dtype=np.float64) / S)[:, None]            # [S+1,1]
    q = (np.arange(L + 1, dtype=np.float64) / L)[None, :]            # [1,L+1]
    total = joint.sum(axis=0).astype(np.float64)                     # [K,S+1,L+1]
    scored = _scored_classes(K)

    level_bin = np.minimum(np.arange(S + 1) * bins // S, bins - 1)
    reliability, ece_k = [], []
    for k in range(K):
        cnt = np.bincount(level_bin, weights=total[k].sum(axis=1), minlength=bins)
        sp = np.bincount(level_bin, weights=(total[k] * p).sum(axis=1), minlength=bins)
        sq = np.bincount(level_bin, weights=(total[k] * q).sum(axis=1), minlength=bins)
        filled = cnt > 0
        mp, mq = sp[filled] / cnt[filled], sq[filled] / cnt[filled]
        ece_k.append(float(np.sum(cnt[filled] / N * np.abs(mp - mq))))
        mean_p, mean_q = [None] * bins, [None] * bins
        for i, a, b in zip(np.flatnonzero(filled), mp, mq):
            mean_p[i], mean_q[i] = float(a), float(b)
        reliability.append({"count": [int(c) for c in cnt], "mean_p": mean_p, "mean_q": mean_q})

    brier = float((total * (p - q) ** 2).sum() / N)
    cross_entropy = float(-(total * q * np.log(np.maximum(p, SOFT_LABEL_LOG_FLOOR))).sum() / N)

    dice = np.empty((len(thresholds), len(scored), B), dtype=np.float64)
    for ti, t in enumerate(thresholds):
        tn, tm = _ceil_fraction(t, S), _ceil_fraction(t, L)
        for ci, k in enumerate(scored):
            P = joint[:, k, tn:, :].sum(axis=(1, 2)).astype(np.float64)
            Q = joint[:, k, :, tm:].sum(axis=(1, 2)).astype(np.float64)
            PQ = joint[:, k, tn:, tm:].sum(axis=(1, 2)).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = 2.0 * PQ / (P + Q)
            d[(P + Q) == 0] = 1.0
            dice[ti, ci] = d

    hw = joint[:, 0].sum(axis=(1, 2))
    corr = []
    for b in range(B):
        n = int(hw[b])
        su, sv, suu, svv, suv = (int(x) for x in moments[b])
        var_u, var_v, cov = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv           # exact (Python integers)
        if var_u > 0 and var_v > 0:
            corr.append(float(cov) / (math.sqrt(float(var_u)) * math.sqrt(float(var_v))))

    res: Dict[str, object] = {
        "pixels": N, "images": int(B), "samples": int(S), "raters": int(L), "classes": int(K), "bins": bins, "thresholds": thresholds,
        "ece_soft": float(np.mean([ece_k[k] for k in scored])), "ece_soft_per_class": ece_k, "brier_soft": brier,
        "cross_entropy_soft": cross_entropy, "dice_soft": float(dice.mean()),
        "dice_soft_per_threshold": [float(x) for x in dice.mean(axis=(1, 2))],
        "ncc": float(np.mean(corr)) if corr else None, "ncc_images": len(corr), "reliability": reliability}
    if class_names is not None:
        res["class_names"] = [str(c) for c in class_names]
    return res


# ------------------------------------------------------------------------------------------------ surface distances
SURFACE_STAT_FIELDS = ("n_ar", "n_ra", "d2_max", "d2_lo", "d2_hi")


def surface_distance_stats(a_idx: torch.Tensor, b_idx: torch.Tensor, num_classes: int, q: Tuple[int, int] = (95, 100)) -> Dict[str, object]:
    """a_idx [B,S,H,W] / b_idx [B,L,H,W] integer class maps on the GPU -> the per-cell arrays of ccdm_surfdist (include/ccdm_hip.h),
    each of shape [B,S,L,C] over the scored classes C (1..K-1; class 0 when K == 1): int64 n_ar, n_ra (the sizes of the two
    surfaces; a cell is defined iff both are > 0), d2_max, d2_lo, d2_hi (the maximum and the order statistics at the ranks
    floor(pos), ceil(pos), pos = q[0]*(n-1)/q[1], of the pooled squared surface distances; 0 in an undefined cell) and float64
    sum_ar, sum_ra (the sums of the distances of each direction); plus "q": [q[0], q[1]] and "classes": the scored classes."""
    lib = hip.load()
    a8, b8, (B, S, L, H, W) = _class_map_stacks("surface_distance_stats", a_idx, b_idx)
    q_num, q_den = int(q[0]), int(q[1])
    classes = _scored_classes(num_classes)
    Cn = len(classes)
    stats = torch.zeros((B, S, L, Cn, 5), dtype=torch.int32, device=a8.device)
    sums = torch.zeros((B, S, L, Cn, 2), dtype=torch.float64, device=a8.device)
    need = int(lib.ccdm_surfdist_workspace_bytes(B, S, L, H, W, num_classes))
    ws = _workspace(need, a8.device)
    hip.check(lib.ccdm_surfdist(a8.data_ptr(), b8.data_ptr(), B, S, L, H, W, num_classes, q_num, q_den, stats.data_ptr(), sums.data_ptr(),
                                ws.data_ptr(), need, torch.cuda.current_stream(a8.device).cuda_stream), "surfdist")
    st, sm = stats.cpu().numpy().astype(np.int64), sums.cpu().numpy()
    out: Dict[str, object] = {name: st[..., f] for f, name in enumerate(SURFACE_STAT_FIELDS)}
    out.update(sum_ar=sm[..., 0], sum_ra=sm[..., 1], q=[q_num, q_den], classes=classes)
    return out


def concat_surface_stats(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The stats of several batches as one (concatenated along the images)."""
    return _concat_stats(parts, SURFACE_STAT_FIELDS + ("sum_ar", "sum_ra"), ("q", "classes"))


def surface_scores_from_stats(stats: Dict[str, object], *, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The surface-distance scores behind the per-cell arrays of `surface_distance_stats`, on the host in float64 (no GPU).  Per
    defined cell (both surfaces non-empty), with n = n_ar + n_ra and pos = q_num*(n-1)/q_den taken in exact integer arithmetic:
      hd             sqrt(d2_max), the Hausdorff distance
      hd_percentile  sqrt(d2_lo) + frac(pos) * (sqrt(d2_hi) - sqrt(d2_lo)): numpy's linear-interpolation percentile of the pooled
                     distances (HD95 at q = 95/100, as MedPy's hd95)
      assd           (sum_ar/n_ar + sum_ra/n_ra) / 2 (MedPy's assd)
    Each score is the mean over images of the mean over the image's defined cells (samples x raters x classes); an image
    without a defined cell is left out; `*_per_class`: the same over one class's cells.  Undefined cells are counted
    (cells_undefined, of which cells_both_empty have neither surface) and never folded into a mean; a score with no defined
    cell is None.  The result holds lists, numbers and None only: it survives a JSON round trip."""
    n_ar, n_ra, classes = _check_cells(stats, "n_ar", "n_ra", class_names)
    B, S, L, Cn = n_ar.shape
    q_num, q_den = (int(x) for x in stats["q"])
    if not 0 < q_num <= q_den:
        raise ValueError(f"q: {q_num}/{q_den} (expected 0 < q_num <= q_den)")
    defined = (n_ar > 0) & (n_ra > 0)
    safe_ar, safe_ra = np.where(defined, n_ar, 1), np.where(defined, n_ra, 1)
    t = q_num * (n_ar + n_ra - 1)                                    # pos = t / q_den, exact
    frac = (t % q_den).astype(np.float64) / q_den
    lo, hi = np.sqrt(np.asarray(stats["d2_lo"], dtype=np.float64)), np.sqrt(np.asarray(stats["d2_hi"], dtype=np.float64))
    cell = {"hd": np.sqrt(np.asarray(stats["d2_max"], dtype=np.float64)), "hd_percentile": lo + frac * (hi - lo),
            "assd": (np.asarray(stats["sum_ar"], dtype=np.float64) / safe_ar + np.asarray(stats["sum_ra"], dtype=np.float64) / safe_ra) / 2.0}

    res: Dict[str, object] = {"images": int(B), "samples": int(S), "raters": int(L), "classes": classes, "q": [q_num, q_den],
                              "percentile": 100.0 * q_num / q_den, "cells_defined": int(defined.sum()),
                              "cells_undefined": int((~defined).sum()), "cells_both_empty": int(((n_ar == 0) & (n_ra == 0)).sum()),
                              "images_scored": int(defined.reshape(B, -1).any(axis=1).sum())}
    for key, values in cell.items():
        res[key] = _mean_of_image_means(values, defined)
        res[key + "_per_class"] = [_mean_of_image_means(values[..., c], defined[..., c]) for c in range(Cn)]
    res["cells_defined_per_class"] = [int(defined[..., c].sum()) for c in range(Cn)]
    if class_names is not None:
        res["class_names"] = [str(c) for c in class_names]
    return res


# ------------------------------------------------------------------------------------------------ lesion-level scores
LESION_STAT_FIELDS = ("n_a", "n_r", "hit_a", "hit_r")
LESION_OVERLAPS = ((0, 1), (1, 2))


def lesion_stats(a_idx: torch.Tensor, b_idx: torch.Tensor, num_classes: int, connectivity: int = 8,
                 overlaps: Sequence[Tuple[int, int]] = LESION_OVERLAPS) -> Dict[str, object]:
    """a_idx [B,S,H,W] / b_idx [B,L,H,W] integer class maps on the GPU -> the per-cell arrays of ccdm_lesions (include/ccdm_hip.h)
    over the scored classes C (1..K-1; class 0 when K == 1), all int64: n_a, n_r [B,S,L,C] (the lesions, i.e. connected components
    under `connectivity`, of the sample map and of the rater map) and hit_a, hit_r [B,S,L,C,T] (how many of them the other map's
    mask covers to overlaps[t] = (num, den): cov >= 1 and cov*den >= num*size); plus "overlaps": [[num, den], ...],
    "connectivity" and "classes": the scored classes."""
    lib = hip.load()
    a8, b8, (B, S, L, H, W) = _class_map_stacks("lesion_stats", a_idx, b_idx)
    ov = np.ascontiguousarray([[int(n), int(d)] for n, d in overlaps], dtype=np.int32).reshape(-1, 2)
    T = int(ov.shape[0])
    classes = _scored_classes(num_classes)
    Cn = len(classes)
    stats = torch.zeros((B, S, L, Cn, 2 + 2 * T), dtype=torch.int32, device=a8.device)
    need = int(lib.ccdm_lesions_workspace_bytes(B, S, L, H, W, num_classes))
    ws = _workspace(need, a8.device)
    hip.check(lib.ccdm_lesions(a8.data_ptr(), b8.data_ptr(), B, S, L, H, W, num_classes, int(connectivity), ov.ctypes.data, T,
                               stats.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(a8.device).cuda_stream), "lesions")
    st = stats.cpu().numpy().astype(np.int64)
    return {"n_a": st[..., 0], "n_r": st[..., 1], "hit_a": st[..., 2:2 + T], "hit_r": st[..., 2 + T:], "overlaps": ov.tolist(),
            "connectivity": int(connectivity), "classes": classes}


def concat_lesion_stats(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The stats of several batches as one (concatenated along the images)."""
    return _concat_stats(parts, LESION_STAT_FIELDS, ("overlaps", "connectivity", "classes"))


def lesion_scores_from_stats(stats: Dict[str, object], *, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The lesion-level scores behind the per-cell arrays of `lesion_stats`, on the host in float64 (no GPU).  Per cell (sample x
    rater x class of an image) and threshold:
      recall     hit_r / n_r, defined iff n_r > 0: the share of the rater's lesions the sample finds
      precision  hit_a / n_a, defined iff n_a > 0: the share of the sample's lesions the rater confirms
      f1         (hit_a + hit_r) / (n_a + n_r), defined iff n_a + n_r > 0: the share of all lesions of both maps that the other map
                 hits (2*TP / (n_a + n_r) where both sides agree on TP; 0 when one side has no lesion)
    Each score is a list over the thresholds of the mean over images of the mean over the image's defined cells; an image without a
    defined cell is left out; a score with no defined cell anywhere is None; `*_per_class`: the same over one class's cells.  Never
    folded into a mean: cells, cells_both_empty (n_a == n_r == 0), cells_sample_empty (n_a == 0), cells_rater_empty (n_r == 0),
    images_scored (images with a cell that has a lesion).  Over all cells: count_error = mean |n_a - n_r|, count_exact = the share
    with n_a == n_r, lesions_per_sample_map / lesions_per_rater_map = mean n_a / mean n_r.  The result holds lists, numbers and None
    only: it survives a JSON round trip."""
    n_a, n_r, classes = _check_cells(stats, "n_a", "n_r", class_names, need_image="lesion_scores_from_stats")
    B, S, L, Cn = n_a.shape
    overlaps = [[int(n), int(d)] for n, d in stats["overlaps"]]
    T = len(overlaps)
    if T < 1 or any(not (d >= 1 and 0 <= n <= d) for n, d in overlaps):
        raise ValueError(f"overlaps: {overlaps!r} (expected at least one num/den with 0 <= num <= den, den >= 1)")
    hit_a, hit_r = np.asarray(stats["hit_a"]).astype(np.int64), np.asarray(stats["hit_r"]).astype(np.int64)
    if hit_a.shape != n_a.shape + (T,) or hit_r.shape != hit_a.shape:
        raise ValueError(f"hit_a {hit_a.shape} / hit_r {hit_r.shape}: expected {n_a.shape + (T,)}")
    connectivity = int(stats["connectivity"])
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity: {connectivity} (expected 4 or 8)")
    cell = {"recall": (hit_r, n_r[..., None], n_r > 0), "precision": (hit_a, n_a[..., None], n_a > 0),
            "f1": (hit_a + hit_r, (n_a + n_r)[..., None], (n_a + n_r) > 0)}

    res: Dict[str, object] = {
        "images": int(B), "samples": int(S), "raters": int(L), "classes": classes, "connectivity": connectivity, "overlaps": overlaps,
        "thresholds": [n / d for n, d in overlaps], "cells": int(n_a.size), "cells_both_empty": int(((n_a == 0) & (n_r == 0)).sum()),
        "cells_sample_empty": int((n_a == 0).sum()), "cells_rater_empty": int((n_r == 0).sum()),
        "images_scored": int(((n_a + n_r) > 0).reshape(B, -1).any(axis=1).sum())}
    for key, (num, den, defined) in cell.items():
        values = num.astype(np.float64) / np.where(defined[..., None], den, 1).astype(np.float64)          # [B,S,L,C,T]
        res[key] = [_mean_of_image_means(values[..., t], defined) for t in range(T)]
        res[key + "_per_class"] = [[_mean_of_image_means(values[..., c, t], defined[..., c]) for t in range(T)] for c in range(Cn)]
    res.update(count_error=float(np.abs(n_a - n_r).mean()), count_exact=float((n_a == n_r).mean()),
               lesions_per_sample_map=float(n_a.mean()), lesions_per_rater_map=float(n_r.mean()))
    if class_names is not None:
        res["class_names"] = [str(c) for c in class_names]
    return res


# ------------------------------------------------------------------------------------------------ matched-lesion scores
LESION_MATCH_STAT_FIELDS = ("n_a", "n_r", "tp", "iou_sum")
LESION_MATCH_THRESHOLDS = ((1, 2), (3, 4))
LESION_IOU_ONE = 1 << 32                  # iou_sum is a sum of floor(inter * 2^32 / union)


def lesion_match_stats(a_idx: torch.Tensor, b_idx: torch.Tensor, num_classes: int, connectivity: int = 8,
                       thresholds: Sequence[Tuple[int, int]] = LESION_MATCH_THRESHOLDS, min_size: int = 1) -> Dict[str, object]:
    """a_idx [B,S,H,W] / b_idx [B,L,H,W] integer class maps on the GPU -> the per-cell arrays of ccdm_lesion_match
    (include/ccdm_hip.h) over the scored classes C (1..K-1; class 0 when K == 1), all int64: n_a, n_r [B,S,L,C] (the lesions of at
    least `min_size` pixels of the sample map and of the rater map) and tp, iou_sum [B,S,L,C,T] (the pairs of them with
    inter*den > num*union at thresholds[t] = (num, den) in [1/2, 1): at most one partner per lesion; and the sum of
    floor(inter * 2^32 / union) over those pairs); plus "thresholds": [[num, den], ...], "connectivity", "min_size" and "classes".
    ccdm_lesions labels the maps, ccdm_lesion_match reads its workspace: one buffer, one stream."""
    lib = hip.load()
    a8, b8, (B, S, L, H, W) = _class_map_stacks("lesion_match_stats", a_idx, b_idx)
    th = np.ascontiguousarray([[int(n), int(d)] for n, d in thresholds], dtype=np.int32).reshape(-1, 2)
    T = int(th.shape[0])
    classes = _scored_classes(num_classes)
    Cn = len(classes)
    any_overlap = np.array([[0, 1]], dtype=np.int32)              # ccdm_lesions' own counts are not used here
    hits = torch.zeros((B, S, L, Cn, 4), dtype=torch.int32, device=a8.device)
    stats = torch.zeros((B, S, L, Cn, 2 + T), dtype=torch.int32, device=a8.device)
    iou = torch.zeros((B, S, L, Cn, T), dtype=torch.int64, device=a8.device)
    need = int(lib.ccdm_lesion_match_workspace_bytes(B, S, L, H, W, num_classes))
    ws = _workspace(need, a8.device)
    stream = torch.cuda.current_stream(a8.device).cuda_stream
    hip.check(lib.ccdm_lesions(a8.data_ptr(), b8.data_ptr(), B, S, L, H, W, num_classes, int(connectivity), any_overlap.ctypes.data, 1,
                               hits.data_ptr(), ws.data_ptr(), need, stream), "lesions")
    hip.check(lib.ccdm_lesion_match(B, S, L, H, W, num_classes, th.ctypes.data, T, int(min_size), stats.data_ptr(), iou.data_ptr(),
                                    ws.data_ptr(), need, stream), "lesion_match")
    st = stats.cpu().numpy().astype(np.int64)
    return {"n_a": st[..., 0], "n_r": st[..., 1], "tp": st[..., 2:], "iou_sum": iou.cpu().numpy(), "thresholds": th.tolist(),
            "connectivity": int(connectivity), "min_size": int(min_size), "classes": classes}


def concat_lesion_match_stats(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The stats of several batches as one (concatenated along the images)."""
    return _concat_stats(parts, LESION_MATCH_STAT_FIELDS, ("thresholds", "connectivity", "min_size", "classes"))


def lesion_match_scores_from_stats(stats: Dict[str, object], *, class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """Panoptic quality over lesions from the per-cell arrays of `lesion_match_stats`, on the host in float64 (no GPU).  Per cell
    (sample x rater x class of an image) and threshold, with fp = n_a - tp, fn = n_r - tp and q = iou_sum / 2^32 (the summed IoU of
    the matched pairs):
      rq   2*tp / (n_a + n_r) = tp / (tp + fp/2 + fn/2), defined iff n_a + n_r > 0: recognition quality, the F1 of the matching
      sq   q / tp, defined iff tp > 0: segmentation quality, the mean IoU of the matched pairs
      pq   2*q / (n_a + n_r), defined iff n_a + n_r > 0: panoptic quality, sq * rq where both are defined, 0 where nothing matches
    Each score is a list over the thresholds of the mean over images of the mean over the image's defined cells; an image without a
    defined cell is left out; a score with no defined cell anywhere is None; `*_per_class`: the same over one class's cells.  The
    pooled form of the panoptic paper over all cells: pq_pooled = sum q / (sum tp + sum fp / 2 + sum fn / 2), sq_pooled = sum q /
    sum tp, rq_pooled = sum tp / (sum tp + sum fp / 2 + sum fn / 2), with tp_total, fp_total, fn_total per threshold beside them.
    Never folded into a mean: cells, cells_both_empty (n_a == n_r == 0), cells_matched per threshold (tp > 0), images_scored
    (images with a cell that has a lesion).  The result holds lists, numbers and None only: it survives a JSON round trip."""
    n_a, n_r, classes = _check_cells(stats, "n_a", "n_r", class_names, need_image="lesion_match_scores_from_stats")
    B, S, L, Cn = n_a.shape
    thresholds = [[int(n), int(d)] for n, d in stats["thresholds"]]
    T = len(thresholds)
    if T < 1 or any(not (d <= 2 * n and n < d) for n, d in thresholds):
        raise ValueError(f"thresholds: {thresholds!r} (expected at least one num/den with 1/2 <= num/den < 1)")
    tp, iou_sum = np.asarray(stats["tp"]).astype(np.int64), np.asarray(stats["iou_sum"]).astype(np.int64)
    if tp.shape != n_a.shape + (T,) or iou_sum.shape != tp.shape:
        raise ValueError(f"tp {tp.shape} / iou_sum {iou_sum.shape}: expected {n_a.shape + (T,)}")
    connectivity, min_size = int(stats["connectivity"]), int(stats["min_size"])
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity: {connectivity} (expected 4 or 8)")
    if min_size < 1:
        raise ValueError(f"min_size: {min_size} (expected at least 1)")
    q = iou_sum.astype(np.float64) / float(LESION_IOU_ONE)                                                # [B,S,L,C,T]
    both = (n_a + n_r)[..., None]
    some = np.broadcast_to(both > 0, tp.shape)
    cell = {"rq": (2.0 * tp, both, some), "sq": (q, tp, tp > 0), "pq": (2.0 * q, both, some)}

    res: Dict[str, object] = {
        "images": int(B), "samples": int(S), "raters": int(L), "classes": classes, "connectivity": connectivity, "min_size": min_size,
        "thresholds": thresholds, "ious": [n / d for n, d in thresholds], "cells": int(n_a.size),
        "cells_both_empty": int(((n_a == 0) & (n_r == 0)).sum()), "cells_matched": [int((tp[..., t] > 0).sum()) for t in range(T)],
        "images_scored": int(((n_a + n_r) > 0).reshape(B, -1).any(axis=1).sum())}
    for key, (num, den, defined) in cell.items():
        values = np.asarray(num, dtype=np.float64) / np.where(defined, den, 1).astype(np.float64)          # [B,S,L,C,T]
        res[key] = [_mean_of_image_means(values[..., t], defined[..., t]) for t in range(T)]
        res[key + "_per_class"] = [[_mean_of_image_means(values[..., c, t], defined[..., c, t]) for t in range(T)] for c in range(Cn)]
    tp_total = [int(tp[..., t].sum()) for t in range(T)]
    fp_total = [int(n_a.sum()) - n for n in tp_total]
    fn_total = [int(n_r.sum()) - n for n in tp_total]
    q_total = [int(iou_sum[..., t].sum()) / LESION_IOU_ONE for t in range(T)]
    weight = [n + 0.5 * p + 0.5 * m for n, p, m in zip(tp_total, fp_total, fn_total)]
    res.update(tp_total=tp_total, fp_total=fp_total, fn_total=fn_total,
               pq_pooled=[s / w if w > 0 else None for s, w in zip(q_total, weight)],
               sq_pooled=[s / n if n > 0 else None for s, n in zip(q_total, tp_total)],
               rq_pooled=[n / w if w > 0 else None for n, w in zip(tp_total, weight)])
    if class_names is not None:
        res["class_names"] = [str(c) for c in class_names]
    return res


# ------------------------------------------------------------------------------------------------ findings of the sample set
FINDING_CANDIDATE_FIELDS = ("size", "support", "peak", "mass", "ref_cov", "rater_hits", "ymin", "xmin", "ymax", "xmax", "sum_y", "sum_x")
FINDING_REFERENCE_FIELDS = ("size", "cov", "best_support", "best_peak")
FINDING_ARRAYS = ("counts", "candidates", "references")
FINDING_SETTINGS = ("samples", "raters", "n_min", "m_min", "connectivity", "classes", "max_candidates")
FINDINGS_MAX_CANDIDATES = 1024            # ccdm_findings' cap: what one workgroup's LDS tables hold
DETECTION_SCORES = ("support", "peak")
DETECTION_FP_RATES = (1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8)      # false positives per image of the LUNA16 score


def sample_findings(samples_idx: torch.Tensor, raters_idx: Optional[torch.Tensor], num_classes: int, *, n_min: int, m_min: Optional[int] = None,
                    connectivity: int = 8, max_candidates: int = 64, return_map: bool = False) -> Dict[str, object]:
    """The lesions the S samples of an image propose TOGETHER, and how sure the set is of each (HIP kernel ccdm_findings; the
    definition is in include/ccdm_hip.h).  samples_idx [B,S,H,W], raters_idx [B,L,H,W] or None: integer class maps on the GPU.  Per
    image and scored class (1..K-1; class 0 when K == 1: C of them) the candidates are the connected components, under `connectivity`,
    of the pixels that at least `n_min` samples give the class; the reference lesions those of the pixels at least `m_min` raters give
    it (default: a majority, L // 2 + 1).  Both are numbered in raster order of their first pixel.  Returns, on the host as int64:
      counts      [B,C,2]    the candidates and the reference lesions
      candidates  [B,C,max_candidates,12]  per candidate FINDING_CANDIDATE_FIELDS: size; support (the samples with a pixel of the
                             class inside it); peak, mass (the maximum and the sum of the per-pixel sample counts); ref_cov (its pixels
                             inside a reference lesion); rater_hits (the raters with a pixel of the class inside it); the bounding
                             box; the coordinate sums (centroid = sum / size).  Rows from the count on are zero.
      references  [B,C,max_candidates,4]   per reference lesion FINDING_REFERENCE_FIELDS: size; cov (its pixels inside a candidate);
                             best_support, best_peak (the maxima over the candidates that touch it, 0: none does)
    and the settings "samples", "raters", "n_min", "m_min" (None without raters), "connectivity", "classes", "max_candidates".
    return_map: also "confidence_map", uint8 [B,C,H,W] ON THE DEVICE: the support of the candidate that holds the pixel, 0 outside.
    An (image, class) with more candidates or reference lesions than `max_candidates` (at most 1024) raises, naming the value needed."""
    if not isinstance(samples_idx, torch.Tensor) or (raters_idx is not None and not isinstance(raters_idx, torch.Tensor)):
        raise ValueError("sample_findings: expected tensors [B,S,H,W] and [B,L,H,W] (or None)")
    s8, r8, (B, S, L, H, W) = _class_map_stacks("sample_findings", samples_idx, raters_idx, expected="[B,S,H,W] and [B,L,H,W] or None")
    if raters_idx is not None and L == 0:
        raise ValueError("sample_findings: raters_idx holds no rater (pass None)")
    n_min = whole_number(n_min, "n_min", 1, None, "expected a whole number of samples, at least 1")
    if L == 0:
        m_min = None
    else:
        m_min = L // 2 + 1 if m_min is None else whole_number(m_min, "m_min", 1, None, "expected a whole number of raters, at least 1")
    cap = whole_number(max_candidates, "max_candidates", 1, None, "expected a whole number, at least 1")
    lib = hip.load()
    classes = _scored_classes(num_classes)
    Cn = len(classes)
    dev = s8.device
    counts = torch.zeros((B, Cn, 2), dtype=torch.int32, device=dev)
    cand = torch.zeros((B, Cn, cap, len(FINDING_CANDIDATE_FIELDS)), dtype=torch.int32, device=dev)
    ref = torch.zeros((B, Cn, cap, len(FINDING_REFERENCE_FIELDS)), dtype=torch.int32, device=dev)
    conf = torch.zeros((B, Cn, H, W), dtype=torch.uint8, device=dev) if return_map else None
    need = int(lib.ccdm_findings_workspace_bytes(B, S, L, H, W, num_classes, cap))
    ws = _workspace(need, dev)
    hip.check(lib.ccdm_findings(s8.data_ptr(), None if r8 is None else r8.data_ptr(), B, S, L, H, W, num_classes, int(connectivity), n_min,
                                0 if m_min is None else m_min, cap, counts.data_ptr(), cand.data_ptr(), ref.data_ptr(),
                                None if conf is None else conf.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
              "findings")
    n = counts.cpu().numpy().astype(np.int64)
    if n.size and int(n.max()) > cap:
        b, ci, side = (int(v) for v in np.unravel_index(int(n.argmax()), n.shape))
        raise hip.CcdmHipError(f"sample_findings: image {b}, class {classes[ci]} has {int(n[b, ci, side])} "
                               f"{'candidates' if side == 0 else 'reference lesions'}, max_candidates={cap} holds {cap}: "
                               f"max_candidates={int(n.max())} needed")
    out: Dict[str, object] = {"counts": n, "candidates": cand.cpu().numpy().astype(np.int64), "references": ref.cpu().numpy().astype(np.int64),
                              "samples": S, "raters": L, "n_min": n_min, "m_min": m_min, "connectivity": int(connectivity), "classes": classes,
                              "max_candidates": cap}
    if conf is not None:
        out["confidence_map"] = conf
    return out


def concat_findings(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The findings of several batches as one (concatenated along the images); the settings have to agree.  No confidence map."""
    if not parts:
        raise ValueError("concat_findings: no part")
    for p in parts[1:]:
        differ = [k for k in FINDING_SETTINGS if p[k] != parts[0][k]]
        if differ:
            raise ValueError(f"concat_findings: the parts differ in {differ}")
    return _concat_stats(parts, FINDING_ARRAYS, FINDING_SETTINGS)


def detection_scores_from_findings(findings: Dict[str, object], *, score: str = "support", fp_rates: Sequence[float] = DETECTION_FP_RATES,
                                   class_names: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """FROC, the sensitivity at fixed false positives per image and the average precision of the sample set as a lesion detector, from
    the records of `sample_findings` (with raters), on the host in Python integers and Fractions until the last division (no GPU).
    Per scored class, pooled over the images: a candidate's confidence is its `score` (support or peak), it is TRUE iff ref_cov >= 1;
    a reference lesion is detected at a threshold iff its best_<score> reaches it.  With theta = S, S-1, ..., n_min:
      FP(theta), TPc(theta)  the false / true candidates with score >= theta;  det(theta) the reference lesions with best >= theta
      sensitivity = det / N_ref (None when the class has no reference lesion), fp_per_image = FP / images,
      precision = TPc / (TPc + FP) (None where no candidate reaches theta)
    per class ("per_class", one dict each):
      froc               {"thresholds", "fp_per_image", "sensitivity", "precision"}: the curve, one entry per theta
      sensitivity_at_fp  per entry of fp_rates the largest sensitivity among the thresholds with fp_per_image <= the rate (no
                         interpolation; the empty threshold above S always qualifies, with 0);  cpm: their mean (the LUNA16 score)
      average_precision  sum over descending theta of (R_i - R_(i-1)) * P_i with the lesion recall R = sensitivity, R_0 = 0
      candidates, true_candidates, reference_lesions, images_without_reference
    and over the classes that have a reference lesion the means "cpm" and "average_precision" (None: no class has one).  The result
    holds lists, numbers, strings and None only: it survives a JSON round trip."""
    if score not in DETECTION_SCORES:
        raise ValueError(f"score: {score!r} (expected one of {DETECTION_SCORES})")
    counts, cand, ref = (np.asarray(findings[k]).astype(np.int64) for k in FINDING_ARRAYS)
    if counts.ndim != 3 or counts.shape[2] != 2:
        raise ValueError(f"counts {counts.shape}: expected [B,C,2]")
    B, Cn = int(counts.shape[0]), int(counts.shape[1])
    if cand.ndim != 4 or cand.shape[:2] != (B, Cn) or cand.shape[3] != len(FINDING_CANDIDATE_FIELDS):
        raise ValueError(f"candidates {cand.shape}: expected [{B},{Cn},cap,{len(FINDING_CANDIDATE_FIELDS)}]")
    if ref.ndim != 4 or ref.shape[:2] != (B, Cn) or ref.shape[3] != len(FINDING_REFERENCE_FIELDS):
        raise ValueError(f"references {ref.shape}: expected [{B},{Cn},cap,{len(FINDING_REFERENCE_FIELDS)}]")
    if B < 1:
        raise ValueError("detection_scores_from_findings: the findings hold no image")
    if int(counts[..., 0].max()) > cand.shape[2] or int(counts[..., 1].max()) > ref.shape[2]:
        raise ValueError(f"counts: up to {int(counts.max())} records, the arrays hold {cand.shape[2]} / {ref.shape[2]}")
    S, L, n_min = int(findings["samples"]), int(findings["raters"]), int(findings["n_min"])
    if L < 1:
        raise ValueError("detection_scores_from_findings: findings without raters have no reference lesions to score against")
    if not 1 <= n_min <= S:
        raise ValueError(f"n_min: {n_min} outside [1, samples={S}]")
    classes = [int(c) for c in findings["classes"]]
    if len(classes) != Cn:
        raise ValueError(f"classes: {len(classes)} entries for {Cn} scored classes")
    if class_names is not None and len(class_names) != Cn:
        raise ValueError(f"class_names: {len(class_names)} names for {Cn} scored classes")
    try:
        rates = [Fraction(str(r)) for r in fp_rates]
    except (ValueError, ZeroDivisionError, TypeError):
        rates = []
    if not rates or any(isinstance(r, bool) for r in fp_rates) or any(r < 0 for r in rates):
        raise ValueError(f"fp_rates: {fp_rates!r} (expected at least one rate of false positives per image, none negative)")
    cand_field = FINDING_CANDIDATE_FIELDS.index(score)
    ref_field = FINDING_REFERENCE_FIELDS.index("best_" + score)
    ref_cov = FINDING_CANDIDATE_FIELDS.index("ref_cov")
    thresholds = list(range(S, n_min - 1, -1))
    ratio = lambda f: None if f is None else float(f)
    per_class = []
    for ci in range(Cn):
        true_scores, false_scores, best = [], [], []
        for b in range(B):
            for rec in cand[b, ci, :int(counts[b, ci, 0])].tolist():
                (true_scores if rec[ref_cov] >= 1 else false_scores).append(rec[cand_field])
            best += [rec[ref_field] for rec in ref[b, ci, :int(counts[b, ci, 1])].tolist()]
        n_ref = len(best)
        fp = [sum(1 for v in false_scores if v >= t) for t in thresholds]
        tp = [sum(1 for v in true_scores if v >= t) for t in thresholds]
        det = [sum(1 for v in best if v >= t) for t in thresholds]
        sens = [Fraction(d, n_ref) if n_ref else None for d in det]
        prec = [Fraction(t, t + f) if t + f else None for t, f in zip(tp, fp)]
        at_rate, ap = None, None
        if n_ref:
            at_rate = [max([Fraction(0)] + [s for s, f in zip(sens, fp) if Fraction(f, B) <= r]) for r in rates]
            ap, before = Fraction(0), Fraction(0)
            for s, p in zip(sens, prec):
                if s > before:                                        # a lesion found at this threshold: a true candidate reaches it
                    ap += (s - before) * p
                before = s
        per_class.append({"class": classes[ci], "candidates": len(true_scores) + len(false_scores), "true_candidates": len(true_scores),
                          "reference_lesions": n_ref, "images_without_reference": int((counts[:, ci, 1] == 0).sum()),
                          "froc": {"thresholds": thresholds, "fp_per_image": [float(Fraction(f, B)) for f in fp],
                                   "sensitivity": [ratio(s) for s in sens], "precision": [ratio(p) for p in prec]},
                          "sensitivity_at_fp": None if at_rate is None else [float(s) for s in at_rate],
                          "cpm": None if at_rate is None else float(sum(at_rate) / len(at_rate)), "average_precision": ratio(ap)})
    defined = [r for r in per_class if r["reference_lesions"]]
    res: Dict[str, object] = {"images": B, "samples": S, "raters": L, "n_min": n_min, "m_min": findings["m_min"],
                              "connectivity": int(findings["connectivity"]), "classes": classes, "score": score,
                              "fp_rates": [float(r) for r in rates], "per_class": per_class,
                              "cpm": float(np.mean([r["cpm"] for r in defined])) if defined else None,
                              "average_precision": float(np.mean([r["average_precision"] for r in defined])) if defined else None}
    if class_names is not None:
        res["class_names"] = [str(c) for c in class_names]
    return res


# ------------------------------------------------------------------------------------------------ mode summary
MODE_MAPS =("vote", "entropy", "counts")
MODES_MAX_CLASSES, MODES_MAX_SAMPLES, MODES_MAX_MODES = 32, 256, 16
MODE_DISTANCE_ONE = 1 << 20               # Q counts the Jaccard distance of a class in units of 2^-20
MODE_UNUSED = 255                         # mode_map / mode_vote of a mode that does not exist


def whole_number(value, name: str, lo: int, hi: Optional[int], what: str) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name}: {value!r} ({what})")
    return int(value)


def sample_modes(samples_idx: torch.Tensor, num_classes: int, modes: int, max_swaps: int = 64, maps: Sequence[str] = ("vote", "entropy"),
                 return_distance: bool = False) -> Dict[str, torch.Tensor]:
    """The modes of S samples per image: samples_idx [B,S,H,W] integer class maps on the GPU -> k-medoids (PAM: BUILD, then
    best-improvement SWAP) with M = `modes` clusters per image under the distance of the LIDC scores, 1 - mean foreground IoU, held as
    the int32 fixed-point Q = sum over the classes 1..K-1 of the Jaccard distance in units of 2^-20 (include/ccdm_hip.h has the
    definition, with every tie rule; all sums are integers, so the result does not depend on a reduction order).  2 <= num_classes
    <= 32, 1 <= S <= 256, 1 <= modes <= 16.  Modes are ordered by size, the largest first; when the samples hold fewer than M distinct
    foreground maps the remaining modes are unused.  Device tensors, nothing is copied to the host:
      medoid     int32 [B,M]   the sample that stands for the mode; -1: unused
      assign     int32 [B,S]   the mode of every sample
      size       int32 [B,M];  share fp32 [B,M] = size / S: how likely the mode is under the samples
      spread     int64 [B,M]   the sum of Q from the medoid to the mode's members (divide by size * (K-1) * 2^20 for the mean distance)
      cost       int64 [B]     the sum of the spreads;  swaps int32 [B]: swaps applied (at most max_swaps);  converged int32 [B]: 1 when
                               no single swap lowers the cost any further
      mode_map   uint8 [B,M,H,W]   the medoid sample itself; 255 where the mode is unused
      mode_vote  uint8 [B,M,H,W]   ("vote" in maps) the majority class over the mode's members, lowest class on ties; 255: unused
      mode_entropy fp32 [B,M,H,W]  ("entropy") the entropy in nats of the members' class frequencies: where the mode is unsure; 0: unused
      mode_counts int32 [B,M,H,W,K]  ("counts") the members saying each class
      distance   int32 [B,S,S]     (return_distance) Q; Q / ((K-1) * 2^20) is within 2^-21 of `batched_distance`."""
    B, S, H, W = _sample_stack(samples_idx, MODES_MAX_SAMPLES)
    K = whole_number(num_classes, "num_classes", 2, MODES_MAX_CLASSES, f"expected a whole number in [2, {MODES_MAX_CLASSES}]")
    M = whole_number(modes, "modes", 1, MODES_MAX_MODES, f"expected a whole number in [1, {MODES_MAX_MODES}]")
    max_swaps = whole_number(max_swaps, "max_swaps", 0, 2 ** 31 - 1, "expected a whole number, at least 0")
    maps = tuple(maps)
    bad = [m for m in maps if m not in MODE_MAPS]
    if bad:
        raise ValueError(f"maps: {bad} not available (choose from {MODE_MAPS})")
    if samples_idx.device.type != "cuda":
        raise hip.CcdmHipError("sample_modes needs GPU tensors (no CPU path)")
    lib = hip.load()
    dev, HW = samples_idx.device, H * W
    a8 = samples_idx.reshape(B, S, HW).to(torch.uint8).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty((B, S, S, K), dtype=torch.int32, device=dev)
    Q = torch.empty((B, S, S), dtype=torch.int32, device=dev)
    hip.check(lib.ccdm_modes_distance(a8.data_ptr(), B, S, HW, K, ws.data_ptr(), Q.data_ptr(), stream), "modes_distance")
    out = {"medoid": torch.empty((B, M), dtype=torch.int32, device=dev), "assign": torch.empty((B, S), dtype=torch.int32, device=dev),
           "size": torch.empty((B, M), dtype=torch.int32, device=dev), "spread": torch.empty((B, M), dtype=torch.int64, device=dev),
           "cost": torch.empty((B,), dtype=torch.int64, device=dev), "swaps": torch.empty((B,), dtype=torch.int32, device=dev),
           "converged": torch.empty((B,), dtype=torch.int32, device=dev)}
    hip.check(lib.ccdm_modes_pam(Q.data_ptr(), B, S, M, max_swaps, out["medoid"].data_ptr(), out["assign"].data_ptr(), out["size"].data_ptr(),
                                 out["spread"].data_ptr(), out["cost"].data_ptr(), out["swaps"].data_ptr(), out["converged"].data_ptr(),
                                 stream), "modes_pam")
    # (through float64: the device divides by a scalar as a multiplication by its reciprocal, which in fp32 is not the rounded quotient)
    out["share"] = (out["size"].to(torch.float64) / float(S)).to(torch.float32)
    used = out["medoid"] >= 0                                                                     # [B,M]
    picked = torch.gather(a8, 1, out["medoid"].clamp(min=0).long()[:, :, None].expand(B, M, HW))     # the medoid samples themselves
    out["mode_map"] = torch.where(used[:, :, None], picked, torch.full_like(picked, MODE_UNUSED)).reshape(B, M, H, W)
    if maps:
        vote = torch.empty((B, M, HW), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, M, HW, K), dtype=torch.int32, device=dev) if "counts" in maps else None
        entropy = torch.empty((B, M, HW), dtype=torch.float32, device=dev) if "entropy" in maps else None
        hip.check(lib.ccdm_modes_maps(a8.data_ptr(), out["assign"].data_ptr(), out["size"].data_ptr(), B, S, M, HW, K, vote.data_ptr(),
                                      None if counts is None else counts.data_ptr(), None if entropy is None else entropy.data_ptr(),
                                      stream), "modes_maps")
        if "vote" in maps:
            out["mode_vote"] = vote.reshape(B, M, H, W)
        if counts is not None:
            out["mode_counts"] = counts.reshape(B, M, H, W, K)
        if entropy is not None:
            out["mode_entropy"] = entropy.reshape(B, M, H, W)
    if return_distance:
        out["distance"] = Q
    return out


# ------------------------------------------------------------------------------------------------ metric-optimal consensus
CONSENSUS_METRICS = ("iou", "dice")
CONSENSUS_MAPS = ("label", "mask")
CONSENSUS_ONE = 1 << 20                   # a curve value counts the score against one sample in units of 2^-20
CONSENSUS_MAX_SAMPLES = 255               # the frequency planes are bytes


def threshold_maps(frequency: torch.Tensor, thresholds: torch.Tensor, num_samples: int, metric: str = "iou",
                   maps: Sequence[str] = ("label",)) -> Dict[str, torch.Tensor]:
    """The maps of given thresholds (HIP kernel ccdm_consensus_maps): frequency uint8 [B,C,H,W] and thresholds int32 [B,C,2] on the GPU
    as sample_consensus returns them (or any thresholds j >= 1: S // 2 + 1 is the majority vote's), `metric` picking the column ->
    `mask` uint8 [B,C,H,W] = frequency >= threshold and / or `label` uint8 [B,H,W]: the scored class with the largest frequency among
    the masks that hold the pixel, the lowest on ties, class 0 where none does."""
    if metric not in CONSENSUS_METRICS:
        raise ValueError(f"metric: {metric!r} (choose from {CONSENSUS_METRICS})")
    maps = tuple(maps)
    bad = [m for m in maps if m not in CONSENSUS_MAPS]
    if bad or not maps:
        raise ValueError(f"maps: {list(maps) if not maps else bad} not available (choose from {CONSENSUS_MAPS})")
    if frequency.device.type != "cuda":
        raise hip.CcdmHipError("threshold_maps needs GPU tensors (no CPU path)")
    B, C, H, W = (int(v) for v in frequency.shape)
    if frequency.dtype != torch.uint8 or thresholds.dtype != torch.int32 or tuple(thresholds.shape) != (B, C, 2):
        raise ValueError(f"thresholds: expected int32 [{B},{C},2] beside frequency uint8 [B,C,H,W], got {thresholds.dtype} {tuple(thresholds.shape)} "
                         f"beside {frequency.dtype}")
    lib = hip.load()
    dev = frequency.device
    freq, best = frequency.contiguous(), thresholds.to(dev).contiguous()
    mask = torch.empty((B, C, H, W), dtype=torch.uint8, device=dev) if "mask" in maps else None
    label = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if "label" in maps else None
    hip.check(lib.ccdm_consensus_maps(freq.data_ptr(), best.data_ptr(), B, int(num_samples), H * W, C + 1, CONSENSUS_METRICS.index(metric),
                                      None if mask is None else mask.data_ptr(), None if label is None else label.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), "consensus_maps")
    out = {}
    if label is not None:
        out["label"] = label
    if mask is not None:
        out["mask"] = mask
    return out


def sample_consensus(samples_idx: torch.Tensor, num_classes: int, metric: str = "iou", maps: Sequence[str] = ("label",)) -> Dict[str, torch.Tensor]:
    """The single map to report for S samples per image: samples_idx [B,S,H,W] integer class maps on the GPU -> per image and scored
    class k = 1..K-1 the threshold j on the sample frequency n[p] whose mask {n >= j} has the largest expected `metric` ("iou" or
    "dice") under the samples themselves, among j = 1..S+1 (S + 1: the empty map; S // 2 + 1: the majority vote against class 0).  Held
    in exact integers, a score against one sample in units of 2^-20 (include/ccdm_hip.h has the definition, with every tie rule).
    2 <= num_classes <= 32, 1 <= S <= 255.  O(S HW) work per image and class.  Device tensors, nothing is copied to the host:
      threshold   int32 [B,C]        the best j of `metric`;  thresholds int32 [B,C,2]: of IoU and of Dice
      curve       int64 [B,C,2,S+1]  the sum over the samples of the fixed-point score of every j, for IoU and for Dice
      expected    float64 [B,C]      curve at the best j / (S * 2^20): the expected `metric` of the consensus
      expected_majority float64 [B,C]  the same at j = S // 2 + 1
      frequency   uint8 [B,C,H,W]    n
      label       uint8 [B,H,W]      ("label" in maps) the consensus map: the class whose mask holds the pixel, by the largest n and then
                                     the lowest class where several do, class 0 where none does
      mask        uint8 [B,C,H,W]    ("mask") n >= threshold, 0 / 1."""
    B, S, H, W = _sample_stack(samples_idx, CONSENSUS_MAX_SAMPLES)
    K = whole_number(num_classes, "num_classes", 2, MODES_MAX_CLASSES, f"expected a whole number in [2, {MODES_MAX_CLASSES}]")
    if metric not in CONSENSUS_METRICS:
        raise ValueError(f"metric: {metric!r} (choose from {CONSENSUS_METRICS})")
    maps = tuple(maps)
    bad = [m for m in maps if m not in CONSENSUS_MAPS]
    if bad:
        raise ValueError(f"maps: {bad} not available (choose from {CONSENSUS_MAPS})")
    if samples_idx.device.type != "cuda":
        raise hip.CcdmHipError("sample_consensus needs GPU tensors (no CPU path)")
    lib = hip.load()
    dev, HW, C, m = samples_idx.device, H * W, K - 1, CONSENSUS_METRICS.index(metric)
    a8 = samples_idx.reshape(B, S, HW).to(torch.uint8).contiguous()
    freq = torch.empty((B, C, H, W), dtype=torch.uint8, device=dev)
    curve = torch.empty((B, C, 2, S + 1), dtype=torch.int64, device=dev)
    best = torch.empty((B, C, 2), dtype=torch.int32, device=dev)
    nbytes = int(lib.ccdm_consensus_workspace_bytes(B, S, HW, K))
    ws = _workspace(nbytes, dev)
    hip.check(lib.ccdm_consensus(a8.data_ptr(), B, S, HW, K, freq.data_ptr(), curve.data_ptr(), best.data_ptr(), ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream(dev).cuda_stream), "consensus")
    # (divided by a device tensor: by a host scalar the device multiplies by the reciprocal, which is not the rounded quotient)
    denom = torch.full((), float(S * CONSENSUS_ONE), dtype=torch.float64, device=dev)
    of_metric = curve[:, :, m]                                                                    # [B,C,S+1]
    out = {"threshold": best[:, :, m].contiguous(), "thresholds": best, "curve": curve,
           "expected": torch.gather(of_metric, 2, (best[:, :, m].long() - 1)[:, :, None])[:, :, 0].to(torch.float64) / denom,
           "expected_majority": of_metric[:, :, S // 2].to(torch.float64) / denom, "frequency": freq}
    if maps:
        out.update(threshold_maps(freq, best, S, metric, maps))
    return out
