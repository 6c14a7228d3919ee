"""What the lesion-detection tests (test_lidc_detection) share: the numpy restatement of ccdm_findings' definition (include/ccdm_hip.h),
written with one boolean mask per lesion and a flood fill of its own, a brute-force restatement of the detection scores, the
lesion-like generator of sample and rater stacks, and the hand-made maps.  A plain module: no fixture, no pytest setting."""
import functools
from fractions import Fraction

import numpy as np

CAND_FIELDS = ("size", "support", "peak", "mass", "ref_cov", "rater_hits", "ymin", "xmin", "ymax", "xmax", "sum_y", "sum_x")
REF_FIELDS = ("size", "cov", "best_support", "best_peak")


def scored_classes(K: int):
    return list(range(1, K)) if K > 1 else [0]


def flood_labels(mask: np.ndarray, connectivity: int):
    """breadth-first fill from every unlabelled mask pixel in raster order -> (int32 labels [H,W], number of components)"""
    H, W = mask.shape
    lab = np.zeros((H, W), dtype=np.int32)
    near = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (connectivity == 8 or not (dy and dx))]
    n = 0
    for y in range(H):
        for x in range(W):
            if not mask[y, x] or lab[y, x]:
                continue
            n += 1
            lab[y, x] = n
            front = [(y, x)]
            while front:
                nxt = []
                for cy, cx in front:
                    for dy, dx in near:
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] and not lab[ny, nx]:
                            lab[ny, nx] = n
                            nxt.append((ny, nx))
                front = nxt
    return lab, n


def scipy_labels(mask: np.ndarray, connectivity: int):
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    return lab.astype(np.int32), int(n)


def findings_restatement(samples: np.ndarray, raters, K: int, n_min: int, m_min, connectivity: int = 8, cap: int = 64, label=flood_labels):
    """samples [B,S,H,W] uint8, raters [B,L,H,W] uint8 or None -> the dict metrics.sample_findings returns, by the definition, plus
    "confidence_map" (numpy uint8 [B,C,H,W]) and "labels" (int32 [B,C,2,H,W]: candidates, reference lesions).  A cell with more
    records than `cap` keeps the first `cap` (the kernel's are not defined there: compare the counts only)."""
    B, S, H, W = samples.shape
    L = 0 if raters is None else raters.shape[1]
    classes = scored_classes(K)
    counts = np.zeros((B, len(classes), 2), dtype=np.int64)
    cand = np.zeros((B, len(classes), cap, len(CAND_FIELDS)), dtype=np.int64)
    ref = np.zeros((B, len(classes), cap, len(REF_FIELDS)), dtype=np.int64)
    conf = np.zeros((B, len(classes), H, W), dtype=np.uint8)
    labels = np.zeros((B, len(classes), 2, H, W), dtype=np.int32)
    for b in range(B):
        for ci, c in enumerate(classes):
            says = samples[b] == c                                                # [S,H,W]
            rater_says = raters[b] == c if L else np.zeros((0, H, W), dtype=bool)
            n = says.sum(axis=0)
            A = n >= n_min
            R = rater_says.sum(axis=0) >= m_min if L else np.zeros((H, W), dtype=bool)
            la, nc = label(A, connectivity)
            lr, nr = label(R, connectivity)
            counts[b, ci] = nc, nr
            labels[b, ci] = la, lr
            records = []
            for i in range(1, nc + 1):
                own = la == i
                ys, xs = np.nonzero(own)
                records.append([int(own.sum()), sum(int((says[s] & own).any()) for s in range(S)), int(n[own].max()), int(n[own].sum()),
                                int((own & R).sum()), sum(int((rater_says[j] & own).any()) for j in range(L)), int(ys.min()), int(xs.min()),
                                int(ys.max()), int(xs.max()), int(ys.sum()), int(xs.sum())])
                conf[b, ci][own] = records[-1][1]
            for i, rec in enumerate(records[:cap]):
                cand[b, ci, i] = rec
            for j in range(1, min(nr, cap) + 1):
                own = lr == j
                touching = [records[i - 1] for i in sorted(set(la[own].tolist()) - {0})]
                ref[b, ci, j - 1] = [int(own.sum()), int((own & A).sum()), max([t[1] for t in touching], default=0),
                                     max([t[2] for t in touching], default=0)]
    return {"counts": counts, "candidates": cand, "references": ref, "samples": S, "raters": L, "n_min": int(n_min),
            "m_min": None if L == 0 else int(m_min), "connectivity": int(connectivity), "classes": classes, "max_candidates": cap,
            "confidence_map": conf, "labels": labels}


def scores_restatement(findings, score="support", fp_rates=(1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8)):
    """the detection scores by a loop over the thresholds, per class -> a list of dicts with Fractions (None where undefined)"""
    counts, cand, ref = findings["counts"], findings["candidates"], findings["references"]
    B, Cn = counts.shape[:2]
    S, n_min = findings["samples"], findings["n_min"]
    f_c, f_r, f_cov = CAND_FIELDS.index(score), REF_FIELDS.index("best_" + score), CAND_FIELDS.index("ref_cov")
    out = []
    for ci in range(Cn):
        n_ref = int(counts[:, ci, 1].sum())
        curve = []                                                                 # (theta, FP, TPc, det), theta descending
        for theta in range(S, n_min - 1, -1):
            fp = tp = det = 0
            for b in range(B):
                for i in range(int(counts[b, ci, 0])):
                    if cand[b, ci, i, f_c] >= theta:
                        if cand[b, ci, i, f_cov] >= 1:
                            tp += 1
                        else:
                            fp += 1
                for j in range(int(counts[b, ci, 1])):
                    det += int(ref[b, ci, j, f_r] >= theta)
            curve.append((theta, fp, tp, det))
        at_rate = cpm = ap = None
        if n_ref:
            at_rate = []
            for rate in fp_rates:
                best = Fraction(0)                                                 # the empty threshold above S
                for _, fp, _, det in curve:
                    if Fraction(fp, B) <= Fraction(str(rate)):
                        best = max(best, Fraction(det, n_ref))
                at_rate.append(best)
            cpm = sum(at_rate) / len(at_rate)
            ap, before = Fraction(0), Fraction(0)
            for _, fp, tp, det in curve:
                recall = Fraction(det, n_ref)
                if recall != before:
                    ap += (recall - before) * Fraction(tp, tp + fp)
                before = recall
        out.append({"reference_lesions": n_ref, "candidates": int(counts[:, ci, 0].sum()), "curve": curve, "sensitivity_at_fp": at_rate,
                    "cpm": cpm, "average_precision": ap, "images_without_reference": int((counts[:, ci, 1] == 0).sum())})
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


EXISTENCE = (0.15, 0.4, 0.7, 1.0)


@functools.lru_cache(maxsize=None)
def lesion_like_case(B, S, L, H, W, K, seed=0):
    """Lesion-like stacks (independent noise would fuse into one candidate): per image a few disc centres, each with a scored class, a
    radius and an existence probability from EXISTENCE; every sample and every rater includes each disc with that probability, its
    radius jittered by -1, 0 or +1; a sample also draws, two times in five, a spurious disc of radius 1 somewhere.  The background byte is
    0, or K (no class) when K == 1 scores class 0.  -> (samples uint8 [B,S,H,W], raters uint8 [B,L,H,W] or None), read-only."""
    rng = np.random.default_rng(4100 + 977 * seed + 131 * H + 17 * W + 5 * K + S)
    classes = scored_classes(K)
    background = K if K == 1 else 0
    samples = np.full((B, S, H, W), background, dtype=np.uint8)
    raters = np.full((B, L, H, W), background, dtype=np.uint8) if L else None
    r_max = max(1, min(H, W) // 8)
    for b in range(B):
        discs = [(int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, r_max + 1)), classes[int(rng.integers(0, len(classes)))],
                  EXISTENCE[int(rng.integers(0, 4))]) for _ in range(int(rng.integers(2, 5)))]
        for stack, count, spurious in ((samples, S, True), (raters, L, False)):
            for i in range(count):
                for cy, cx, r, c, p in discs:
                    if rng.random() < p:
                        stack[b, i][_disc(H, W, cy, cx, max(0, r + int(rng.integers(-1, 2))))] = c
                if spurious and rng.random() < 0.4:
                    stack[b, i][_disc(H, W, int(rng.integers(0, H)), int(rng.integers(0, W)), 1)] = classes[int(rng.integers(0, len(classes)))]
    samples.setflags(write=False)
    if raters is not None:
        raters.setflags(write=False)
    return samples, raters


def default_thresholds(S, L):
    """(n_min, m_min) the tests use: a tenth of the samples, a majority of the raters"""
    return max(1, -(-S // 10)), (L // 2 + 1 if L else 0)


@functools.lru_cache(maxsize=None)
def lesion_like_findings(shape, connectivity, cap=8, seed=0):
    samples, raters = lesion_like_case(*shape, seed=seed)
    n_min, m_min = default_thresholds(shape[1], shape[2])
    return findings_restatement(samples, raters, shape[5], n_min, m_min, connectivity, cap)


def hand_map(name: str, H: int = 16, W: int = 16) -> np.ndarray:
    """a binary map [H,W] uint8 (class 1 of K = 2)"""
    m = np.zeros((H, W), dtype=np.uint8)
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "checkerboard":
        yy, xx = np.mgrid[0:H, 0:W]
        m[(yy + xx) % 2 == 0] = 1
    elif name == "spiral":                                     # a one-pixel-wide rectangular spiral with one-pixel gaps, inwards
        top, left, bottom, right = 0, 0, H - 1, W - 1
        m[top, left:right + 1] = 1
        while True:
            m[top:bottom + 1, right] = 1
            m[bottom, left:right + 1] = 1
            if bottom - top < 4 or right - left < 4:
                break
            m[top + 2:bottom + 1, left] = 1
            m[top + 2, left:right - 1] = 1
            top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
            if bottom - top < 2 or right - left < 2:
                break
    elif name == "u_last_row":                                 # arms from row 0 that only the last row joins: the unions come late
        m[:, 1] = 1; m[:, 7] = 1; m[:, 12] = 1; m[H - 1, 1:13] = 1; m[0, 4] = 1
    elif name == "diagonal":                                   # two squares that touch at a corner only
        m[2:5, 2:5] = 1; m[5:8, 5:8] = 1; m[10, 3] = 1; m[11, 4] = 1; m[12, 3] = 1
    else:
        raise KeyError(name)
    return m


HAND_MAPS = ("empty", "full", "checkerboard", "spiral", "u_last_row", "diagonal")


def hand_case(name: str):
    """-> (samples [1,3,16,16], raters [1,2,16,16]): the map in every sample but the last, which holds it shifted down by one row; the
    raters hold the map and the map shifted right by two columns"""
    m = hand_map(name)
    samples = np.stack([m, m, np.roll(m, 1, axis=0)])[None]
    raters = np.stack([m, np.roll(m, 2, axis=1)])[None]
    return np.ascontiguousarray(samples), np.ascontiguousarray(raters)
