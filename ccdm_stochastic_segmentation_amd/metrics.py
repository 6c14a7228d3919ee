"""LIDC uncertainty metrics: generalised energy distance, sample/expert diversity and
Hungarian-matched IoU, as the reference computes them
(/root/reference/evaluation/evaluate_lidc_uncertainty.py:27-73; duplicates in ddpm/utils.py:129-174).

The O(B*S*S'*HW*K) part — per-class intersection/union counts of every pair of label maps — runs in a HIP
kernel (ccdm_pairwise_class_counts); the host only divides integers and solves the <= 100x100 assignment
problems with scipy, exactly as the reference does, so results are bit-identical to the reference's numpy.

Beyond the reference: the soft-label scores.  What the S samples imply at a pixel, p_k = (samples saying k) / S, against the
raters' soft label there, q_k = (raters saying k) / L: `vote_joint_counts` (HIP kernel ccdm_lidcscore) counts the pixels of
every image by (class, samples saying it, raters saying it), `soft_label_scores_from_counts` derives calibration, Brier score,
cross-entropy, thresholded soft Dice and the uncertainty correlation (NCC) from those integers on the host."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip


def pairwise_class_counts(a_idx: torch.Tensor, b_idx: torch.Tensor, num_classes: int) -> np.ndarray:
    """a_idx [B,S,...] / b_idx [B,L,...] integer class maps on the GPU -> int32 [B,S,L,K,2] (intersection, union)."""
    lib = hip.load()
    if a_idx.device.type != "cuda":
        raise hip.CcdmHipError("pairwise_class_counts needs GPU tensors (no CPU path)")
    B, S = a_idx.shape[:2]
    L = b_idx.shape[1]
    a8 = a_idx.reshape(B, S, -1).to(torch.uint8).contiguous()
    b8 = b_idx.reshape(B, L, -1).to(device=a8.device, dtype=torch.uint8).contiguous()
    HW = a8.shape[2]
    assert b8.shape[2] == HW and b8.shape[0] == B
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
    if samples_idx.device.type != "cuda" or raters_idx.device.type != "cuda":
        raise hip.CcdmHipError("vote_joint_counts needs GPU tensors (no CPU path)")
    B, S = samples_idx.shape[:2]
    L = raters_idx.shape[1]
    s8 = samples_idx.reshape(B, S, -1).to(torch.uint8).contiguous()
    r8 = raters_idx.reshape(B, L, -1).to(device=s8.device, dtype=torch.uint8).contiguous()
    HW = s8.shape[2]
    assert r8.shape[2] == HW and r8.shape[0] == B
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
    scored = list(range(1, K)) if K > 1 else [0]

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
