"""What the consensus tests (test_sample_consensus) share: the numpy / int64 restatement of the definition in include/ccdm_hip.h (the
frequency planes, the curves of the S + 1 thresholded maps in units of 2^-20, the best thresholds with their tie rule, mask and label),
a brute-force version that builds every candidate mask, and the seeded inputs.  The restatement is written from the definition, not
from the kernels: per sample a bincount of n over the sample's class-k pixels, reversed cumulative sums, Python-int division.  A
plain module: no fixture, no pytest setting."""
import functools

import numpy as np

ONE = 1 << 20


# ------------------------------------------------------------------------------------------------ restatement
def term(num: int, den: int) -> int:
    """num / den in units of 2^-20, round half up, in Python integers; 2^20 where den == 0"""
    return ONE if den == 0 else (2 * num * ONE + den) // (2 * den)


def curves_restatement(a: np.ndarray, k: int):
    """a [S,HW] class maps, class k -> (n uint8 [HW], curve int64 [2,S+1])"""
    S = a.shape[0]
    is_k = a == k
    n = is_k.sum(axis=0)
    A = np.bincount(n, minlength=S + 2)[::-1].cumsum()[::-1]                         # A[j] = #{p : n[p] >= j}, j = 0 .. S+1
    curve = np.zeros((2, S + 1), dtype=np.int64)
    for s in range(S):
        I = np.bincount(n[is_k[s]], minlength=S + 2)[::-1].cumsum()[::-1]            # I[j] = #{p : a_s[p] == k and n[p] >= j}
        n_s = int(is_k[s].sum())
        for j in range(1, S + 2):
            i, aj = int(I[j]), int(A[j])
            curve[0, j - 1] += term(i, aj + n_s - i)
            curve[1, j - 1] += term(2 * i, aj + n_s)
    return n.astype(np.uint8), curve


def curves_brute_force(a: np.ndarray, k: int) -> np.ndarray:
    """the same curve with every P_j built and I, U, D counted per (j, s)"""
    S = a.shape[0]
    is_k = a == k
    n = is_k.sum(axis=0)
    curve = np.zeros((2, S + 1), dtype=np.int64)
    for j in range(1, S + 2):
        P = n >= j
        for s in range(S):
            I, U, D = int((P & is_k[s]).sum()), int((P | is_k[s]).sum()), int(P.sum()) + int(is_k[s].sum())
            curve[0, j - 1] += term(I, U)
            curve[1, j - 1] += term(2 * I, D)
    return curve


def maps_restatement(freq: np.ndarray, best: np.ndarray):
    """freq [C,HW], best [C] (the thresholds of one metric) -> (mask uint8 [C,HW], label uint8 [HW])"""
    mask = freq.astype(np.int64) >= best[:, None]
    held = np.where(mask, freq.astype(np.int64), -1)                                 # the n of the masks that hold the pixel
    label = np.where(mask.any(axis=0), np.argmax(held, axis=0) + 1, 0)               # (argmax: the first, i.e. the lowest class)
    return mask.astype(np.uint8), label.astype(np.uint8)


def consensus_restatement(samples: np.ndarray, K: int):
    """samples [B,S,H,W] -> freq uint8 [B,C,H,W], curve int64 [B,C,2,S+1], best int64 [B,C,2] and, per metric m, mask[m] uint8 [B,C,H,W]
    and label[m] uint8 [B,H,W]"""
    B, S, H, W = samples.shape
    flat = samples.reshape(B, S, H * W)
    C = K - 1
    freq = np.zeros((B, C, H * W), dtype=np.uint8)
    curve = np.zeros((B, C, 2, S + 1), dtype=np.int64)
    for b in range(B):
        for c in range(C):
            freq[b, c], curve[b, c] = curves_restatement(flat[b], c + 1)
    best = np.argmax(curve, axis=-1) + 1                                             # (argmax: the first, i.e. the lowest j)
    mask = np.zeros((2, B, C, H * W), dtype=np.uint8)
    label = np.zeros((2, B, H * W), dtype=np.uint8)
    for m in range(2):
        for b in range(B):
            mask[m, b], label[m, b] = maps_restatement(freq[b], best[b, :, m])
    return {"freq": freq.reshape(B, C, H, W), "curve": curve, "best": best, "mask": mask.reshape(2, B, C, H, W), "label": label.reshape(2, B, H, W)}


def rater_scores(label: np.ndarray, raters: np.ndarray, K: int):
    """label [B,H,W], raters [B,L,H,W] -> (IoU, Dice) float64 [B]: mean over the raters of the mean over the classes 1..K-1, 0/0 = 1"""
    B, L = raters.shape[:2]
    iou, dice = np.zeros((B, L, K - 1)), np.zeros((B, L, K - 1))
    for b in range(B):
        for l in range(L):
            for k in range(1, K):
                x, y = label[b] == k, raters[b, l] == k
                i, u, d = int((x & y).sum()), int((x | y).sum()), int(x.sum()) + int(y.sum())
                iou[b, l, k - 1] = i / u if u else 1.0
                dice[b, l, k - 1] = 2 * i / d if d else 1.0
    return iou.mean(axis=-1).mean(axis=-1), dice.mean(axis=-1).mean(axis=-1)


# ------------------------------------------------------------------------------------------------ inputs
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lidc_like(seed, B, S, H, W):
    """K = 2: per image a share of empty samples, the others a disc of varying centre and radius around one lesion"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        empty = rng.choice([0.0, 0.3, 0.6])
        cy, cx, r0 = rng.uniform(2, H - 2), rng.uniform(2, W - 2), rng.uniform(1.0, min(H, W) / 3)
        for s in range(S):
            if rng.random() < empty:
                continue
            r = r0 * rng.uniform(0.5, 1.6)
            out[b, s] = (yy - cy - rng.normal(0, 1)) ** 2 + (xx - cx - rng.normal(0, 1)) ** 2 <= r * r
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def random_case(seed, B, S, H, W, K, foreign=0):
    """noisy copies of a few random maps per image, background-heavy; `foreign` bytes of the stack set to 255 (no class)"""
    rng = np.random.default_rng(seed)
    out = np.empty((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        bases = rng.integers(0, K, (3, H, W)) * (rng.random((3, H, W)) < 0.6)
        for s in range(S):
            m = bases[rng.integers(0, 3)].copy()
            noise = rng.random((H, W)) < rng.choice([0.02, 0.1, 0.3])
            m[noise] = rng.integers(0, K, int(noise.sum()))
            out[b, s] = m
    if foreign:
        out.reshape(-1)[rng.choice(out.size, foreign, replace=False)] = 255
    return _frozen(out)


def empty_wins_case():
    """S = 8, K = 2, 3x4: four samples empty, four with one distinct pixel each"""
    a = np.zeros((1, 8, 3, 4), dtype=np.uint8)
    for s in range(4):
        a[0, 4 + s].reshape(-1)[2 * s + 1] = 1
    return _frozen(a)


def label_rule_case():
    """K = 3, S = 4, 1x4.  Pixel 0: classes 1 and 2 twice each (equal n: the lowest class wins where both masks hold it); pixel 1: class
    2 three times and class 1 once; pixel 2: class 1 in every sample; pixel 3: class 2 once (below class 2's threshold wherever that is
    above 1) -> samples [1,4,1,4]"""
    a = np.array([[1, 2, 1, 0], [1, 2, 1, 0], [2, 2, 1, 0], [2, 1, 1, 2]], dtype=np.uint8)
    return _frozen(a.reshape(1, 4, 1, 4))
