"""LIDC surface-distance scores: the transform and pair kernels (ccdm_surfdist), metrics.surface_distance_stats,
metrics.surface_scores_from_stats and the `evaluation.surface_distances` keys of eval_lidc_uncertainty.  Nothing in the reference
computes these.  The kernel's integer outputs are exact, so every kernel test asks for equality with a numpy restatement of the
definition in include/ccdm_hip.h (surface by neighbour comparison, brute-force integer d2 by broadcasting); the restatement is held
against scipy (binary_erosion, distance_transform_edt), the host scores against numpy.percentile, max and the two means.

A defined cell pools at least two distances (both surfaces are non-empty), so "n = 1" below is one surface pixel per direction
(pooled n = 2); a pooled multiset of one element only exists in an undefined cell, which the host must count and leave out."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ccdm_surfdist", "ccdm_surfdist_workspace_bytes"}
INT_FIELDS = ("n_ar", "n_ra", "d2_max", "d2_lo", "d2_hi")


# ------------------------------------------------------------------------------------------------ restatement
def scored_classes(K: int):
    return list(range(1, K)) if K > 1 else [0]


def surface_restatement(m: np.ndarray, c: int) -> np.ndarray:
    """the mask pixels of class c with one of their four neighbours outside the mask; outside the image is outside the mask"""
    mask = np.asarray(m) == c
    p = np.pad(mask, 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return mask & ~inner


def d2_restatement(surf: np.ndarray):
    """int64 [H,W]: the smallest squared Euclidean distance of every pixel to a pixel of `surf`, by brute force; None: empty set"""
    ys, xs = np.nonzero(surf)
    if ys.size == 0:
        return None
    H, W = surf.shape
    gy, gx = np.mgrid[0:H, 0:W]
    out = np.empty(H * W, dtype=np.int64)
    gy, gx = gy.reshape(-1, 1), gx.reshape(-1, 1)
    step = max(1, (1 << 22) // ys.size)
    for at in range(0, H * W, step):
        out[at:at + step] = ((gy[at:at + step] - ys[None, :]) ** 2 + (gx[at:at + step] - xs[None, :]) ** 2).min(axis=1)
    return out.reshape(H, W)


def ranks(n: int, q):
    """(floor(pos), ceil(pos), numerator of frac(pos)) for pos = q[0]*(n-1)/q[1], in integers"""
    t = q[0] * (n - 1)
    return t // q[1], t // q[1] + (1 if t % q[1] else 0), t % q[1]


def cell_from_multisets(d_ar: np.ndarray, d_ra: np.ndarray, q):
    """the kernel's outputs of one cell from the two directions' squared distances (any order): 5 integers and 2 float64 sums"""
    n_ar, n_ra = int(d_ar.size), int(d_ra.size)
    if n_ar == 0 or n_ra == 0:
        return (n_ar, n_ra, 0, 0, 0), (0.0, 0.0), np.zeros(0, dtype=np.int64)
    D = np.sort(np.concatenate([d_ar, d_ra]).astype(np.int64))
    lo, hi, _ = ranks(D.size, q)
    return (n_ar, n_ra, int(D[-1]), int(D[lo]), int(D[hi])), (float(np.sqrt(d_ar.astype(np.float64)).sum()),
                                                                float(np.sqrt(d_ra.astype(np.float64)).sum())), D


def pooled(a: np.ndarray, r: np.ndarray, c: int):
    """the two directions' squared distances of map a against map r for class c"""
    sa, sr = surface_restatement(a, c), surface_restatement(r, c)
    ta, tr = d2_restatement(sa), d2_restatement(sr)
    if ta is None or tr is None:
        return np.zeros(int(sa.sum()), dtype=np.int64), np.zeros(int(sr.sum()), dtype=np.int64), not (sa.any() or sr.any())
    return tr[sa], ta[sr], False


def stats_restatement(samples: np.ndarray, raters: np.ndarray, K: int, q=(95, 100)):
    """samples [B,S,H,W], raters [B,L,H,W] -> the dict metrics.surface_distance_stats returns, by the definition"""
    B, S = samples.shape[:2]
    L = raters.shape[1]
    classes = scored_classes(K)
    ints = np.zeros((B, S, L, len(classes), 5), dtype=np.int64)
    sums = np.zeros((B, S, L, len(classes), 2), dtype=np.float64)
    for ci, c in enumerate(classes):
        for b in range(B):
            sa = [surface_restatement(samples[b, i], c) for i in range(S)]
            sr = [surface_restatement(raters[b, j], c) for j in range(L)]
            ta, tr = [d2_restatement(s) for s in sa], [d2_restatement(s) for s in sr]
            for i in range(S):
                for j in range(L):
                    if ta[i] is None or tr[j] is None:
                        ints[b, i, j, ci, :2] = int(sa[i].sum()), int(sr[j].sum())
                    else:
                        ints[b, i, j, ci], sums[b, i, j, ci], _ = cell_from_multisets(tr[j][sa[i]], ta[i][sr[j]], q)
    out = {name: ints[..., f] for f, name in enumerate(INT_FIELDS)}
    out.update(sum_ar=sums[..., 0], sum_ra=sums[..., 1], q=[int(q[0]), int(q[1])], classes=classes)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _disc(m, cy, cx, r, c):
    H, W = m.shape
    yy, xx = np.mgrid[0:H, 0:W]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c


@functools.lru_cache(maxsize=None)
def blob_case(B, S, L, H, W, K, seed=0):
    """seeded blob maps: a few filled discs per sample map, every scored class in every map; a rater is a sample shifted by 0-4
    pixels.  8x8: bars of two rows, at most 2 wide, instead, so that every mask pixel is a surface pixel.
    -> (samples, raters, restated stats)"""
    rng = np.random.default_rng(7000 + 131 * H + 17 * W + 5 * K + S + 1000 * seed)
    samples = np.zeros((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        for s in range(S):
            for n, c in enumerate(list(range(1, K)) + [int(rng.integers(1, K))]):
                if H <= 8:                                    # bars at most 2 wide in row bands of their own: no pixel has both row neighbours
                    x = int(rng.integers(0, W - 1))
                    samples[b, s, 2 * n:2 * n + 2, x:x + int(rng.integers(1, 3))] = c
                else:
                    _disc(samples[b, s], int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, max(3, min(H, W) // 5))), c)
    raters = np.stack([np.roll(samples[:, j % S], (int(rng.integers(0, 5)), int(rng.integers(0, 5))), axis=(1, 2)) for j in range(L)], axis=1)
    for s in (samples, raters):
        s.setflags(write=False)
    return samples, raters, stats_restatement(samples, raters, K)


def undefined_share(stats) -> float:
    defined = (stats["n_ar"] > 0) & (stats["n_ra"] > 0)
    return 1.0 - float(defined.mean())


def corner_case(name: str):
    """tiny hand-made stacks -> (samples [1,S,H,W], raters [1,L,H,W], K, q)"""
    H, W, K, q = 12, 14, 2, (95, 100)
    a, r = np.zeros((1, 1, H, W), dtype=np.uint8), np.zeros((1, 1, H, W), dtype=np.uint8)
    if name == "one_side_empty":
        a[0, 0, 3:7, 4:9] = 1
    elif name == "both_empty":
        pass
    elif name == "full_image":
        a[:] = 1
        r[0, 0, 2:10, 2:12] = 1
    elif name == "single_pixel":
        a[0, 0, 5, 6] = 1
        r[0, 0, 9, 2] = 1
    elif name == "line":
        a[0, 0, 4, 1:13] = 1
        r[0, 0, 1:11, 7] = 1
    elif name == "identical":
        a[0, 0, 2:9, 3:10] = 1
        a[0, 0, 10, 12] = 1
        r[:] = a
    elif name == "touching_edges":
        a[0, 0, 0, 3:6] = 1; a[0, 0, H - 1, 8:12] = 1; a[0, 0, 4:8, 0] = 1; a[0, 0, 2:5, W - 1] = 1
        r[0, 0, 0:2, 0:2] = 1; r[0, 0, H - 2:, W - 3:] = 1
    elif name == "diagonal_ties":
        a[0, 0, 6, 6] = 1                                     # (6,6) is equally far from the four corners of r's ring
        r[0, 0, 3, 3] = r[0, 0, 3, 9] = r[0, 0, 9, 3] = r[0, 0, 9, 9] = 1
    elif name == "no_class_bytes":
        K = 3
        a[0, 0, 2:9, 3:10] = 1; a[0, 0, 4:6, 5:7] = 3; a[0, 0, 9:11, 9:13] = 2; a[0, 0, 0, 0] = 255
        r[0, 0, 3:10, 2:8] = 1; r[0, 0, 3, 2] = 7; r[0, 0, 8:11, 8:12] = 2; r[0, 0, 9, 9] = 3
    elif name == "bucket_edge":
        # D = {9, 9, 1409}: ranks 1 and 2 at pos 1.9; 9 is the last element of the bucket of the digit 0, 1409 lies in bucket 5
        H, W = 40, 40
        a, r = np.zeros((1, 1, H, W), dtype=np.uint8), np.zeros((1, 1, H, W), dtype=np.uint8)
        a[0, 0, 2, 2] = a[0, 0, 30, 30] = 1
        r[0, 0, 2, 5] = 1
    elif name == "bucket_edge_low_digit":
        # D = {4, 4, 25}: the same below 256, where a single digit is walked
        a[0, 0, 2, 2] = a[0, 0, 5, 8] = 1
        r[0, 0, 2, 4] = 1
    else:
        raise KeyError(name)
    return a, r, K, q


CORNERS = ["one_side_empty", "both_empty", "full_image", "single_pixel", "line", "identical", "touching_edges", "diagonal_ties",
           "no_class_bytes", "bucket_edge", "bucket_edge_low_digit"]


# ------------------------------------------------------------------------------------------------ CPU: restatement against scipy
def _against_scipy(m: np.ndarray, K: int):
    from scipy import ndimage
    for c in scored_classes(K):
        mask = m == c
        surf = surface_restatement(m, c)
        np.testing.assert_array_equal(surf, mask & ~ndimage.binary_erosion(mask))             # default: cross structure, border_value=0
        d2 = d2_restatement(surf)
        if d2 is None:
            assert not surf.any()
            continue
        np.testing.assert_array_equal(d2, np.rint(ndimage.distance_transform_edt(~surf) ** 2).astype(np.int64))


def test_restatement_matches_scipy():
    for (B, S, L, H, W, K) in ((1, 3, 2, 8, 8, 2), (2, 3, 2, 33, 47, 2), (1, 5, 4, 40, 56, 4)):
        samples, raters, _ = blob_case(B, S, L, H, W, K)
        for stack in (samples, raters):
            for m in stack.reshape(-1, H, W):
                _against_scipy(m, K)
    for name in CORNERS:
        a, r, K, _ = corner_case(name)
        _against_scipy(a[0, 0], K)
        _against_scipy(r[0, 0], K)
    samples, _, _ = blob_case(1, 3, 2, 8, 8, 2)
    assert all((surface_restatement(m, 1) == (m == 1)).all() for m in samples[0])            # 8x8: every mask pixel is on the surface


def test_random_cases_are_mostly_defined():
    """the cap the GPU tests rely on, by the restatement alone"""
    for shape in RANDOM_SHAPES:
        stats = blob_case(*shape)[2]
        assert undefined_share(stats) <= 0.25, shape
        assert int(stats["d2_max"].max()) > 0, shape


# ------------------------------------------------------------------------------------------------ CPU: host scores
def _one_cell_stats(d_ar, d_ra, q):
    ints, sums, D = cell_from_multisets(np.asarray(d_ar, dtype=np.int64), np.asarray(d_ra, dtype=np.int64), q)
    stats = {name: np.array(ints[f], dtype=np.int64).reshape(1, 1, 1, 1) for f, name in enumerate(INT_FIELDS)}
    stats.update(sum_ar=np.array(sums[0]).reshape(1, 1, 1, 1), sum_ra=np.array(sums[1]).reshape(1, 1, 1, 1), q=list(q), classes=[1])
    return stats, D


def _ulps(got: float, want: float) -> float:
    return abs(got - want) / np.spacing(max(abs(want), np.finfo(np.float64).tiny))


def _check_one_cell(d_ar, d_ra, q, tag):
    stats, D = _one_cell_stats(d_ar, d_ra, q)
    r = M.surface_scores_from_stats(stats)
    dist = np.sqrt(D.astype(np.float64))
    want_hd, want_q = float(dist.max()), float(np.percentile(dist, 100.0 * q[0] / q[1]))
    want_assd = (float(np.mean(np.sqrt(np.asarray(d_ar, dtype=np.float64)))) + float(np.mean(np.sqrt(np.asarray(d_ra, dtype=np.float64))))) / 2
    n = D.size
    print(f"surface_scores[{tag} n={n} q={q}] hd={r['hd']!r}/{want_hd!r} hdq={r['hd_percentile']!r}/{want_q!r} assd={r['assd']!r}/{want_assd!r}")
    assert _ulps(r["hd"], want_hd) <= 4 and _ulps(r["hd_percentile"], want_q) <= 4
    assert abs(r["assd"] - want_assd) <= n * 2.0 ** -52 * want_assd
    assert r["cells_defined"] == 1 and r["cells_undefined"] == 0 and r["cells_both_empty"] == 0
    assert r["hd_per_class"] == [r["hd"]] and r["assd_per_class"] == [r["assd"]] and r["hd_percentile_per_class"] == [r["hd_percentile"]]
    assert json.loads(json.dumps(r)) == r
    return stats, r


def test_host_scores_match_numpy():
    rng = np.random.default_rng(3)
    # multisets of the restatement: geometric cells
    for name in ("single_pixel", "line", "touching_edges", "diagonal_ties", "bucket_edge", "identical", "full_image"):
        a, r, K, q = corner_case(name)
        d_ar, d_ra, _ = pooled(a[0, 0], r[0, 0], 1)
        _check_one_cell(d_ar, d_ra, q, name)
    samples, raters, _ = blob_case(2, 3, 2, 33, 47, 2)
    for q in ((95, 100), (19, 20), (1, 2), (100, 100), (1, 3)):
        d_ar, d_ra, _ = pooled(samples[0, 1], raters[0, 0], 1)
        _check_one_cell(d_ar, d_ra, q, "blob")
    # one surface pixel per direction (pooled n = 2: the two order statistics are the two elements), lo != hi
    stats, r = _check_one_cell([1], [9], (95, 100), "n=2")
    assert int(stats["d2_lo"][0, 0, 0, 0]) == 1 and int(stats["d2_hi"][0, 0, 0, 0]) == 9
    assert r["hd_percentile"] == 1.0 + 0.95 * 2.0 and r["hd"] == 3.0 and r["assd"] == 2.0
    _check_one_cell([2], [2, 50], (95, 100), "n=3")
    # pos an exact integer: n - 1 = 20 at 95/100 is rank 19, lo == hi and no interpolation
    d = rng.integers(0, 5000, 21)
    stats, r = _check_one_cell(d[:8], d[8:], (95, 100), "integer pos")
    assert ranks(21, (95, 100)) == (19, 19, 0) and int(stats["d2_lo"][0, 0, 0, 0]) == int(stats["d2_hi"][0, 0, 0, 0]) == int(np.sort(d)[19])
    assert r["hd_percentile"] == float(np.sqrt(np.float64(np.sort(d)[19])))
    # the percentile 100/100 is the maximum
    stats, r = _check_one_cell(d[:5], d[5:17], (100, 100), "100/100")
    assert r["hd_percentile"] == r["hd"] and int(stats["d2_lo"][0, 0, 0, 0]) == int(stats["d2_max"][0, 0, 0, 0])
    for n in (2, 5, 64, 1000):
        d = rng.integers(0, 1 << 21, n)
        k = int(rng.integers(1, n))
        _check_one_cell(d[:k], d[k:], (95, 100), "random")


def test_host_scores_count_undefined_cells_and_average_per_image():
    """B = 2, S = 2, L = 1, two scored classes.  Image 0: cells with distances, one undefined (one side empty), one both empty;
    image 1: nothing defined.  The mean over images is over image 0 alone; undefined cells never enter a mean."""
    q = (95, 100)
    ints = np.zeros((2, 2, 1, 2, 5), dtype=np.int64)
    sums = np.zeros((2, 2, 1, 2, 2), dtype=np.float64)
    ints[0, 0, 0, 0], sums[0, 0, 0, 0], _ = cell_from_multisets(np.array([0, 4]), np.array([16]), q)
    ints[0, 1, 0, 0], sums[0, 1, 0, 0], _ = cell_from_multisets(np.array([36]), np.array([36]), q)
    ints[0, 0, 0, 1, :2] = (7, 0)                             # one pixel set alone: undefined
    ints[1, 1, 0, 0, :2] = (0, 3)
    stats = {name: ints[..., f] for f, name in enumerate(INT_FIELDS)}
    stats.update(sum_ar=sums[..., 0], sum_ra=sums[..., 1], q=list(q), classes=[1, 2])
    r = M.surface_scores_from_stats(stats, class_names=["nodule", "other"])
    assert (r["cells_defined"], r["cells_undefined"], r["cells_both_empty"], r["images_scored"], r["images"]) == (2, 6, 4, 1, 2)
    assert r["hd"] == (4.0 + 6.0) / 2 and r["hd_per_class"] == [5.0, None] and r["cells_defined_per_class"] == [2, 0]
    assert r["assd"] == ((1.0 + 4.0) / 2 + 6.0) / 2 and r["assd_per_class"][1] is None and r["hd_percentile_per_class"][1] is None
    np.testing.assert_allclose(r["hd_percentile"], ((2.0 + 0.9 * 2.0) + 6.0) / 2, rtol=1e-15)
    assert r["class_names"] == ["nodule", "other"] and r["classes"] == [1, 2] and r["percentile"] == 95.0
    assert json.loads(json.dumps(r)) == r
    none = M.surface_scores_from_stats({**stats, **{k: np.zeros_like(stats[k]) for k in INT_FIELDS}})
    assert none["hd"] is None and none["assd"] is None and none["hd_percentile"] is None and none["cells_both_empty"] == 8
    assert json.loads(json.dumps(none)) == none
    with pytest.raises(ValueError, match="class_names"):
        M.surface_scores_from_stats(stats, class_names=["a"])
    with pytest.raises(ValueError, match="q:"):
        M.surface_scores_from_stats({**stats, "q": [3, 2]})
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        M.surface_distance_stats(torch.zeros((1, 2, 4, 4), dtype=torch.uint8), torch.zeros((1, 2, 4, 4), dtype=torch.uint8), 2)


# ------------------------------------------------------------------------------------------------ CPU: ABI
def test_surfdist_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_surfdist[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_surfdist")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
        assert not name.startswith(("ccdm_seg_", "ccdm_segboundary", "ccdm_segcalib", "ccdm_lidc", "ccdm_css", "ccdm_vote_"))
    assert len(hip.SIGNATURES["ccdm_surfdist"][1]) == 15 and len(hip.SIGNATURES["ccdm_surfdist_workspace_bytes"][1]) == 6
    assert "ccdm_surfdist.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_surfdist.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    assert lib.ccdm_surfdist_workspace_bytes(4, 100, 4, 128, 128, 2) == 4 * 4 * 104 * 128 * 128
    assert lib.ccdm_surfdist_workspace_bytes(1, 3, 2, 5, 7, 4) == 4 * 5 * 3 * 35 and lib.ccdm_surfdist_workspace_bytes(1, 3, 2, 5, 7, 1) == 4 * 5 * 35
    assert lib.ccdm_surfdist_workspace_bytes(0, 3, 2, 5, 7, 2) == 0


def test_surfdist_refuses_what_it_cannot_score():
    """the limits are checked before anything is launched or read: host buffers stand in for the device's"""
    lib = hip.load()
    buf = np.zeros(4096, dtype=np.int64)
    p = buf.ctypes.data
    ok = dict(B=1, S=3, L=2, H=8, W=8, K=2, q_num=95, q_den=100)
    for change, what in ((dict(K=33), "K=33"), (dict(K=0), "K=0"), (dict(S=256), "S=256"), (dict(S=0), "S=0"), (dict(L=256), "L=256"),
                         (dict(H=1025), "H=1025"), (dict(W=1025), "W=1025"), (dict(W=0), "W=0"), (dict(q_num=0), "q_num=0"),
                         (dict(q_num=101), "q_num=101 q_den=100"), (dict(q_num=-1), "q_num=-1"), (dict(B=-1), "B=-1"),
                         (dict(B=0, K=33), "K=33")):
        a = {**ok, **change}
        rc = lib.ccdm_surfdist(p, p, a["B"], a["S"], a["L"], a["H"], a["W"], a["K"], a["q_num"], a["q_den"], p, p, p, buf.nbytes, None)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "surfdist")
    rc = lib.ccdm_surfdist(p, p, 1, 3, 2, 8, 8, 2, 95, 100, p, p, p, 4 * 5 * 64 - 1, None)                 # one byte short
    assert rc < 0 and "workspace" in hip.last_error()
    assert lib.ccdm_surfdist(p, p, 1, 3, 2, 8, 8, 2, 95, 100, p, None, p, buf.nbytes, None) < 0 and "null" in hip.last_error()
    assert lib.ccdm_surfdist(p, p, 0, 3, 2, 8, 8, 2, 95, 100, p, p, p, 0, None) == 0 and not buf.any()    # B = 0: nothing launched, nothing written


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def kernel(samples: torch.Tensor, raters: torch.Tensor, K: int, q=(95, 100)):
    """one ccdm_surfdist call on uint8 device stacks [B,S,H,W] / [B,L,H,W] (as they lie in memory) -> the dict of per-cell arrays;
    the outputs start from a non-zero fill: the call overwrites"""
    lib = hip.load()
    assert samples.is_cuda and raters.is_cuda and samples.dtype == raters.dtype == torch.uint8
    assert samples.is_contiguous() and raters.is_contiguous()
    B, S, H, W = samples.shape
    L = raters.shape[1]
    Cn = len(scored_classes(K))
    stats = torch.full((B, S, L, Cn, 5), 77, dtype=torch.int32, device="cuda")
    sums = torch.full((B, S, L, Cn, 2), -5.0, dtype=torch.float64, device="cuda")
    need = int(lib.ccdm_surfdist_workspace_bytes(B, S, L, H, W, K))
    assert need == 4 * B * (S + L) * Cn * H * W
    ws = torch.full((need // 4,), -1, dtype=torch.int32, device="cuda")
    hip.check(lib.ccdm_surfdist(samples.data_ptr(), raters.data_ptr(), B, S, L, H, W, K, q[0], q[1], stats.data_ptr(), sums.data_ptr(),
                                ws.data_ptr(), need, None), "surfdist")
    torch.cuda.synchronize()
    st, sm = stats.cpu().numpy().astype(np.int64), sums.cpu().numpy()
    out = {name: st[..., f] for f, name in enumerate(INT_FIELDS)}
    out.update(sum_ar=sm[..., 0], sum_ra=sm[..., 1], q=list(q), classes=scored_classes(K))
    return out


def assert_stats_match(got, want, tag=""):
    n = want["n_ar"] + want["n_ra"]
    bad = {name: int((got[name] != want[name]).sum()) for name in INT_FIELDS}
    rel = max(float(np.max(np.abs(got[k] - want[k]) / np.maximum(want[k], 1e-300) / np.maximum(n, 1))) for k in ("sum_ar", "sum_ra"))
    print(f"surfdist[{tag} {want['n_ar'].shape}] cells={n.size} undefined={undefined_share(want):.3f} d2_max={int(want['d2_max'].max())} "
          f"mismatches={bad} sum rel err / n = {rel / 2.0 ** -52:.3f} * 2^-52")
    for name in INT_FIELDS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for k in ("sum_ar", "sum_ra"):
        assert (np.abs(got[k] - want[k]) <= n * 2.0 ** -52 * want[k]).all(), k           # undefined cells: 0 on both sides
    assert got["classes"] == want["classes"]


def check_exact(samples: np.ndarray, raters: np.ndarray, K: int, q=(95, 100), want=None, tag=""):
    got = kernel(torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda(), K, q)      # copies: the cached cases are read-only
    want = stats_restatement(samples, raters, K, q) if want is None else want
    assert_stats_match(got, want, tag)
    return got, want


# (B, S, L, H, W, K): 8x8 one tile; 33x47 the byte path and ragged chunks / strips; 40x56 the dword path; 128x128 the workload's row, once
RANDOM_SHAPES = [(1, 3, 2, 8, 8, 2), (1, 5, 4, 8, 8, 4), (2, 3, 2, 33, 47, 2), (1, 5, 4, 33, 47, 4), (1, 3, 2, 40, 56, 2), (2, 5, 4, 40, 56, 4),
                 (1, 3, 2, 128, 128, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,L,H,W,K", RANDOM_SHAPES)
def test_kernel_matches_restatement(B, S, L, H, W, K):
    samples, raters, want = blob_case(B, S, L, H, W, K)
    assert undefined_share(want) <= 0.25                      # an all-undefined input cannot pass silently
    check_exact(samples, raters, K, want=want, tag="random")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CORNERS)
def test_kernel_corner_inputs(name):
    a, r, K, q = corner_case(name)
    d_ar, d_ra, both_empty = pooled(a[0, 0], r[0, 0], 1)
    D = np.sort(np.concatenate([d_ar, d_ra]))
    # the construction holds, by the restatement, before the kernel is asked
    if name == "one_side_empty":
        assert d_ar.size > 0 and d_ra.size == 0 and not both_empty
    elif name == "both_empty":
        assert both_empty
    elif name == "full_image":
        assert d_ar.size == 2 * (a.shape[2] + a.shape[3]) - 4                     # the image border only
    elif name == "single_pixel":
        assert d_ar.size == d_ra.size == 1 and D.tolist() == [32, 32]
    elif name == "line":
        assert d_ar.size == int(a.sum()) and d_ra.size == int(r.sum())            # every pixel of a line is a surface pixel
    elif name == "identical":
        assert D.size > 0 and not D.any()
    elif name == "diagonal_ties":
        assert d_ar.tolist() == [18] and d_ra.tolist() == [18] * 4
    elif name == "no_class_bytes":
        assert (a >= K).sum() == 5 and (r >= K).sum() == 2
    elif name in ("bucket_edge", "bucket_edge_low_digit"):
        lo, hi, rem = ranks(D.size, q)
        shift = 8 if name == "bucket_edge" else 0
        assert rem != 0 and hi == lo + 1 and (D[lo] >> shift) != (D[hi] >> shift)
        assert int(((D >> shift) <= (D[lo] >> shift)).sum()) == lo + 1            # lo is the last element of its bucket, hi lies in a later one
        assert (int(D[-1]) >= 256) == (name == "bucket_edge")
    got, want = check_exact(a, r, K, q, tag=name)
    scores = M.surface_scores_from_stats(got)
    if name in ("one_side_empty", "both_empty"):
        for k in INT_FIELDS[2:] + ("sum_ar", "sum_ra"):
            assert not got[k].any(), k                         # zeros are written over the prefill
        assert scores["cells_undefined"] == 1 and scores["cells_defined"] == 0 and scores["hd"] is None
        assert scores["cells_both_empty"] == (1 if name == "both_empty" else 0)
    else:
        assert scores["cells_undefined"] == 0 and scores["hd"] is not None
    if name == "identical":
        assert scores["hd"] == 0.0 and scores["assd"] == 0.0 and scores["hd_percentile"] == 0.0
    # the maps swapped: the pooled integers are the same, the directions trade places
    swapped = kernel(torch.from_numpy(r).cuda(), torch.from_numpy(a).cuda(), K, q)
    for k1, k2 in (("n_ar", "n_ra"), ("n_ra", "n_ar"), ("d2_max", "d2_max"), ("d2_lo", "d2_lo"), ("d2_hi", "d2_hi")):
        np.testing.assert_array_equal(swapped[k1], got[k2])


@pytest.mark.gpu
def test_kernel_other_percentiles_and_single_class():
    samples, raters, _ = blob_case(2, 3, 2, 33, 47, 2)
    for q in ((100, 100), (1, 2), (1, 1000)):
        check_exact(samples, raters, 2, q, tag=f"q={q}")
    # K = 1 scores class 0, the background; the blobs' bytes belong to no class
    check_exact(np.where(samples > 0, 9, 0).astype(np.uint8), np.where(raters > 0, 9, 0).astype(np.uint8), 1, tag="K=1")


@pytest.mark.gpu
def test_kernel_unaligned_base_pointers():
    """W % 4 == 0 but the stacks start one byte off a dword: the byte path, on either stack or both"""
    B, S, L, H, W, K = 2, 5, 4, 40, 56, 4
    samples, raters, want = blob_case(B, S, L, H, W, K)
    s_buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    r_buf = torch.zeros(raters.size + 1, dtype=torch.uint8, device="cuda")
    s_dev, r_dev = s_buf[1:].view(B, S, H, W), r_buf[1:].view(B, L, H, W)
    s_dev.copy_(torch.from_numpy(np.array(samples))); r_dev.copy_(torch.from_numpy(np.array(raters)))
    assert s_dev.data_ptr() % 4 == 1 and r_dev.data_ptr() % 4 == 1
    for s_t, r_t in ((s_dev, r_dev), (s_dev, torch.from_numpy(np.array(raters)).cuda()), (torch.from_numpy(np.array(samples)).cuda(), r_dev)):
        assert_stats_match(kernel(s_t, r_t, K), want, "unaligned")


@pytest.mark.gpu
def test_kernel_repeated_call_is_bit_identical():
    lib = hip.load()
    samples, raters, want = blob_case(2, 5, 4, 40, 56, 4)
    s_dev, r_dev = torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda()
    first, second = kernel(s_dev, r_dev, 4), kernel(s_dev, r_dev, 4)
    for name in INT_FIELDS:
        np.testing.assert_array_equal(first[name], second[name])
    for k in ("sum_ar", "sum_ra"):
        np.testing.assert_array_equal(first[k].view(np.int64), second[k].view(np.int64))      # the fp64 sums bit for bit
    assert_stats_match(first, want, "repeat")
    # B = 0 leaves prefilled outputs as they are
    st = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    sm = torch.full((8,), 9.0, dtype=torch.float64, device="cuda")
    assert lib.ccdm_surfdist(s_dev.data_ptr(), r_dev.data_ptr(), 0, 5, 4, 40, 56, 4, 95, 100, st.data_ptr(), sm.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((st == 9).all()) and bool((sm == 9.0).all())


@pytest.mark.gpu
def test_surface_distance_stats_takes_index_maps():
    samples, raters, want = blob_case(2, 3, 2, 33, 47, 2)
    s64, r64 = torch.from_numpy(samples.astype(np.int64)).cuda(), torch.from_numpy(raters.astype(np.int64)).cuda()
    got = M.surface_distance_stats(s64, r64, 2)
    assert got["n_ar"].dtype == np.int64 and got["sum_ar"].dtype == np.float64 and got["n_ar"].shape == (2, 3, 2, 1) and got["q"] == [95, 100]
    assert_stats_match(got, want, "int64 maps")
    sliced = M.surface_distance_stats(s64[:, :2], r64, 2, q=(1, 2))                          # the evaluator's pred_idx[:, :s]
    assert_stats_match(sliced, stats_restatement(samples[:, :2], raters, 2, (1, 2)), "sliced")
    both = M.concat_surface_stats([got, got])
    assert both["n_ar"].shape == (4, 3, 2, 1) and both["q"] == [95, 100] and both["classes"] == [1]
    with pytest.raises(ValueError, match="expected"):
        M.surface_distance_stats(s64[:, :, :8], r64, 2)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_surface_distances_end_to_end(tmp_path):
    from ccdm_stochastic_segmentation_amd import evaluation as E
    from tests.golden_util import harness_case
    vote = "majority"
    batches, _, K, predict = harness_case(vote)
    evaluations = [2, 3]

    class DS(torch.utils.data.Dataset):
        items = [(b[0][i], b[1][i], b[2][i]) for b in batches for i in range(b[0].shape[0])]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    def fake():
        class Fake:
            step_T_sample = vote
            calls = 0

            def __call__(self, x, image, **kw):
                p = predict(self.calls, x.shape[0]).to(x.device)
                self.calls += 1
                return {"diffusion_out": p}
        return Fake()

    params = {"dataset_file": "datasets.lidc", "batch_size": 2, "evaluations": evaluations, "output_path": str(tmp_path / "out")}
    plain = E.eval_lidc_uncertainty(dict(params), dataset=DS(), device="cuda:0", model=fake())
    assert set(plain) == {"evaluations", "GED", "diversity_samples", "diversity_experts", "HM_IoU", "IoU", "mIoU", "Dice", "nonzero", "images",
                          "world_size"}                       # today's keys, exactly
    assert not (tmp_path / "out").exists()
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"surface_distances": True, "surface_distance_percentile": 95}}, dataset=DS(),
                                  device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"surface_distances"}
    for key, value in plain.items():                          # everything the evaluator returns today is untouched
        assert res[key] == value, key

    # the predictions and labels the evaluator saw, batch by batch
    S = max(evaluations)
    pred, lab = [], []
    for call, (image, labels, _) in enumerate(batches):
        p = predict(call, labels.shape[0] * S).reshape(labels.shape[0], S, *labels.shape[2:])
        pred.append(p.argmax(dim=2))
        lab.append(labels.argmax(dim=2))
    pred, lab = torch.cat(pred).numpy().astype(np.uint8), torch.cat(lab).numpy().astype(np.uint8)
    assert pred.shape == (5, 3, 32, 32) and lab.shape == (5, 4, 32, 32)
    assert len(res["surface_distances"]) == len(evaluations)
    for s, got in zip(evaluations, res["surface_distances"]):
        want = M.surface_scores_from_stats(stats_restatement(pred[:, :s], lab, K, (19, 20)))      # 95 / 100 as the evaluator reduces it
        print(f"surface_distances[{s}] got={got} want={want}")
        assert got["samples"] == s and got["images"] == 5 and got["raters"] == 4 and got["q"] == [19, 20] and got["cells_defined"] > 0
        assert got["cells_undefined"] > 0                     # some annotations are empty
        assert set(got) == set(want)
        for key in got:
            if key.startswith("assd"):                        # the fp64 sums: n * 2^-52 per cell, n <= 2048 here
                np.testing.assert_allclose(got[key], want[key], rtol=2048 * 2.0 ** -52, atol=0, err_msg=key)
            else:                                             # counts, and scores that follow from integers alone
                assert got[key] == want[key], key
    half = E.eval_lidc_uncertainty({**params, "evaluation": {"surface_distances": True, "surface_distance_percentile": 50}, "output_path": None},
                                   dataset=DS(), device="cuda:0", model=fake())["surface_distances"]
    assert half[0]["q"] == [1, 2] and half[0]["hd"] == res["surface_distances"][0]["hd"]
    assert half[0]["hd_percentile"] == M.surface_scores_from_stats(stats_restatement(pred[:, :2], lab, K, (1, 2)))["hd_percentile"]
    with open(tmp_path / "out" / "lidc_surface_distances.json") as f:
        assert json.load(f) == res["surface_distances"] == json.loads(json.dumps(res["surface_distances"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_surface_distances.json"]
