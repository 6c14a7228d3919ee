"""LIDC lesion-level scores: the labelling and pair kernels (ccdm_lesions), metrics.lesion_stats, metrics.lesion_scores_from_stats
and the `evaluation.lesions` keys of eval_lidc_uncertainty.  Nothing in the reference computes these.  Everything the kernels
write is an integer, so every kernel test asks for equality: the label planes of the workspace with scipy.ndimage.label (which
numbers components in raster order of their first pixel, as the contract in include/ccdm_hip.h does), the per-cell counts with a
numpy restatement of the definition (a flood fill in raster order, then np.bincount over the label planes); the restatement's
labels are held against scipy on every map the tests use."""
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
SYMBOLS = {"ccdm_lesions", "ccdm_lesions_workspace_bytes"}
FIELDS = ("n_a", "n_r", "hit_a", "hit_r")
OVERLAPS = ((0, 1), (1, 2))


# ------------------------------------------------------------------------------------------------ restatement
def scored_classes(K: int):
    return list(range(1, K)) if K > 1 else [0]


def label_restatement(mask: np.ndarray, connectivity: int):
    """flood fill from every unlabelled mask pixel in raster order -> (int32 labels [H,W], number of lesions)"""
    H, W = mask.shape
    inside = np.asarray(mask, dtype=bool).tolist()
    lab = [[0] * W for _ in range(H)]
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    n = 0
    for p in np.flatnonzero(mask).tolist():
        y, x = divmod(p, W)
        if lab[y][x]:
            continue
        n += 1
        lab[y][x] = n
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in steps:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < H and 0 <= nx < W and inside[ny][nx] and not lab[ny][nx]:
                    lab[ny][nx] = n
                    stack.append((ny, nx))
    return np.array(lab, dtype=np.int32).reshape(H, W), n


def scipy_labels(mask: np.ndarray, connectivity: int):
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    return lab.astype(np.int32), int(n)


def planes_restatement(stack: np.ndarray, K: int, connectivity: int):
    """[B,N,H,W] -> (labels [B,N,C,H,W] int32, counts [B,N,C])"""
    B, N, H, W = stack.shape
    classes = scored_classes(K)
    lab = np.zeros((B, N, len(classes), H, W), dtype=np.int32)
    cnt = np.zeros((B, N, len(classes)), dtype=np.int64)
    for b in range(B):
        for i in range(N):
            for ci, c in enumerate(classes):
                lab[b, i, ci], cnt[b, i, ci] = label_restatement(stack[b, i] == c, connectivity)
    return lab, cnt


def stats_restatement(samples: np.ndarray, raters: np.ndarray, K: int, connectivity: int = 8, overlaps=OVERLAPS):
    """samples [B,S,H,W], raters [B,L,H,W] -> the dict metrics.lesion_stats returns, by the definition"""
    B, S = samples.shape[:2]
    L = raters.shape[1]
    classes = scored_classes(K)
    T = len(overlaps)
    la, na = planes_restatement(samples, K, connectivity)
    lr, nr = planes_restatement(raters, K, connectivity)
    n_a = np.zeros((B, S, L, len(classes)), dtype=np.int64)
    n_r = np.zeros_like(n_a)
    hit_a = np.zeros((B, S, L, len(classes), T), dtype=np.int64)
    hit_r = np.zeros_like(hit_a)

    def hits(own, n, other):
        size = np.bincount(own.ravel(), minlength=n + 1)[1:].astype(np.int64)
        cov = np.bincount(own.ravel(), weights=(other.ravel() > 0), minlength=n + 1)[1:].astype(np.int64)
        return [int(((cov >= 1) & (cov * den >= num * size)).sum()) for num, den in overlaps]

    for b in range(B):
        for i in range(S):
            for j in range(L):
                for ci in range(len(classes)):
                    n_a[b, i, j, ci], n_r[b, i, j, ci] = na[b, i, ci], nr[b, j, ci]
                    hit_a[b, i, j, ci] = hits(la[b, i, ci], int(na[b, i, ci]), lr[b, j, ci])
                    hit_r[b, i, j, ci] = hits(lr[b, j, ci], int(nr[b, j, ci]), la[b, i, ci])
    return {"n_a": n_a, "n_r": n_r, "hit_a": hit_a, "hit_r": hit_r, "overlaps": [[int(n), int(d)] for n, d in overlaps],
            "connectivity": int(connectivity), "classes": classes}


# ------------------------------------------------------------------------------------------------ inputs
def _disc(m, cy, cx, r, c):
    H, W = m.shape
    yy, xx = np.mgrid[0:H, 0:W]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c


@functools.lru_cache(maxsize=None)
def lesion_case(B, S, L, H, W, K):
    """seeded maps.  H <= 8: every pixel set with probability 0.45 to a uniform scored class.  Otherwise, per sample map, 2-4 rounds
    over the classes of one filled disc each.  Rater j is sample j % S rolled by 0-3 pixels on each axis; per image, one disc of a
    quarter of the smaller side is cleared in the raters, so that they miss lesions the samples have.  -> (samples, raters)"""
    rng = np.random.default_rng(9000 + 131 * H + 17 * W + 5 * K + S)
    samples = np.zeros((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        for s in range(S):
            if H <= 8:
                samples[b, s] = np.where(rng.random((H, W)) < 0.45, rng.integers(1, K, (H, W)), 0)
            else:
                for _ in range(int(rng.integers(2, 5))):
                    for c in range(1, K):
                        _disc(samples[b, s], int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, max(3, min(H, W) // 8))), c)
    raters = np.stack([np.roll(samples[:, j % S], (int(rng.integers(0, 4)), int(rng.integers(0, 4))), axis=(1, 2)) for j in range(L)], axis=1)
    for b in range(B):
        hole = np.zeros((H, W), dtype=np.uint8)
        _disc(hole, int(rng.integers(0, H)), int(rng.integers(0, W)), min(H, W) // 4, 1)
        raters[b, :, hole > 0] = 0
    for s in (samples, raters):
        s.setflags(write=False)
    return samples, raters


@functools.lru_cache(maxsize=None)
def lesion_case_stats(shape, connectivity):
    samples, raters = lesion_case(*shape)
    return stats_restatement(samples, raters, shape[5], connectivity)


# (B, S, L, H, W, K): 8x8 one chunk of rows; 33x47 the byte path with ragged rows; 40x56 the dword path; 128x128 the workload's size, once
RANDOM_SHAPES = [(1, 3, 2, 8, 8, 2), (1, 5, 4, 8, 8, 4), (2, 3, 2, 33, 47, 2), (1, 5, 4, 33, 47, 4), (2, 5, 4, 40, 56, 4), (1, 3, 2, 128, 128, 2)]
SMALL = [(13, 14), (14, 20)]      # corner maps: the byte path; the dword path, whose 256-pixel chunks cut a row of 20 at x = 16


def _spiral(H, W):
    """a one-pixel-wide rectangular spiral with one-pixel gaps, from the top left corner inwards"""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny < H and 0 <= nx < W and not m[ny, nx]
        ay, ax = ny + dy, nx + dx
        blocked = ahead and 0 <= ay < H and 0 <= ax < W and m[ay, ax]            # the next arm of the spiral two pixels ahead
        if ahead and not blocked:
            y, x = ny, nx
            m[y, x] = 1
            continue
        dy, dx = dx, -dy                                                          # turn right
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx
        if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx] or (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            return m
        y, x = ny, nx
        m[y, x] = 1


def corner_map(name: str, H: int, W: int):
    """-> (map [H,W] uint8, K)"""
    K = 2
    m = np.zeros((H, W), dtype=np.uint8)
    if name == "empty":
        pass
    elif name == "full_image":
        m[:] = 1
    elif name == "single_pixel":
        m[H // 2, W // 3] = 1
    elif name == "anti_diagonal":
        for i in range(min(H, W)):
            m[i, W - 1 - i] = 1
    elif name == "checkerboard":
        yy, xx = np.mgrid[0:H, 0:W]
        m[(yy + xx) % 2 == 0] = 1
    elif name == "serpentine":                                # every other row full, joined at alternating ends: one path
        m[0::2] = 1
        for n, y in enumerate(range(1, H - 1, 2)):
            m[y, W - 1 if n % 2 == 0 else 0] = 1
        if H % 2 == 0:
            m[H - 1] = 0
    elif name == "spiral":
        m = _spiral(H, W)
    elif name == "comb":                                      # teeth from row 0, joined only by the last row
        m[:, 0::2] = 1
        m[H - 1] = 1
    elif name == "u_and_pixel":                               # a U opening upwards and a pixel of row 0 between its arms
        m[0:9, 2] = 1; m[0:9, 8] = 1; m[8, 2:9] = 1; m[0, 5] = 1
    elif name == "four_edges":
        m[0, 3:6] = 1; m[H - 1, 1:W - 2] = 1; m[4:8, 0] = 1; m[2:5, W - 1] = 1; m[0, 0] = 1; m[H - 1, W - 1] = 1; m[0, W - 1] = 1
    elif name == "no_class_bytes":
        K = 3
        m[2:9, 3:10] = 1; m[4:6, 5:7] = 3; m[5, 3:10] = 7; m[9:11, 9:13] = 2; m[0, 0] = 255; m[10, 10] = 255; m[1, 3:10] = 2
    elif name == "class_zero":                                # K = 1 scores class 0; the other bytes belong to no class
        K = 1
        m[:] = 9
        m[2:5, 2:6] = 0; m[7, 1:W - 1] = 0; m[9:12, 8] = 0; m[H - 1, W - 1] = 0
    elif name == "diagonal_touch":
        m[2:4, 2:4] = 1; m[4:6, 4:6] = 1
    else:
        raise KeyError(name)
    return m, K


CORNERS = ["empty", "full_image", "single_pixel", "anti_diagonal", "spiral", "comb", "u_and_pixel", "four_edges", "no_class_bytes",
           "class_zero", "diagonal_touch"]
BIG_CORNERS = ["checkerboard", "serpentine", "spiral", "comb"]          # at 128x128: the array worst case and the longest chains


def corner_case(name: str, H: int, W: int):
    """-> (samples [1,1,H,W], raters [1,2,H,W], K): the map against itself rolled by (1, 2) and against itself"""
    m, K = corner_map(name, H, W)
    raters = np.stack([np.roll(m, (1, 2), axis=(0, 1)), m])[None]
    if name == "empty":
        raters = raters.copy()
        raters[0, 0, 2:4, 2:5] = 1
    return m[None, None], np.ascontiguousarray(raters), K


def assert_construction(name, m, K, connectivity):
    """what a corner map is there for, by the restatement, before a kernel is asked"""
    c = scored_classes(K)[0]
    lab, n = label_restatement(m == c, connectivity)
    H, W = m.shape
    if name == "empty":
        assert n == 0
    elif name in ("full_image", "single_pixel", "serpentine", "spiral", "comb"):
        assert n == 1
        if name == "serpentine":
            assert int((m == c).sum()) == (H + 1) // 2 * W + (H - 1) // 2           # a path: the full rows and one pixel between them
        if name == "spiral":
            assert int((m == c).sum()) > H * W // 3
        if name == "comb":
            assert (m[0, 0::2] == 1).all() and not m[0:H - 1, 1::2].any()
    elif name == "anti_diagonal":
        assert n == (1 if connectivity == 8 else min(H, W))
    elif name == "checkerboard":
        assert n == (1 if connectivity == 8 else (H * W + 1) // 2)
    elif name == "u_and_pixel":
        assert n == 2 and lab[0, 2] == 1 and lab[0, 5] == 2 and lab[0, 8] == 1   # raster order of the first pixel: left arm, pixel; the right arm is the left arm's lesion
    elif name == "four_edges":
        assert n >= 4 and (lab[0] > 0).any() and (lab[-1] > 0).any() and (lab[:, 0] > 0).any() and (lab[:, -1] > 0).any()
    elif name == "no_class_bytes":
        assert sorted(set(m[m >= K].tolist())) == [3, 7, 255] and n == 2            # the row of 7s cuts the square in two
    elif name == "class_zero":
        assert n == 4 and int((m == 0).sum()) < H * W // 2
    elif name == "diagonal_touch":
        assert n == (1 if connectivity == 8 else 2)
    return n


# ------------------------------------------------------------------------------------------------ CPU: restatement against scipy
def _against_scipy(m: np.ndarray, K: int):
    for connectivity in (4, 8):
        for c in scored_classes(K):
            lab, n = label_restatement(m == c, connectivity)
            want, want_n = scipy_labels(m == c, connectivity)
            assert n == want_n
            np.testing.assert_array_equal(lab, want)


def test_restatement_labels_equal_scipy():
    for shape in RANDOM_SHAPES:
        samples, raters = lesion_case(*shape)
        for stack in (samples, raters):
            for m in stack.reshape(-1, shape[3], shape[4]):
                _against_scipy(m, shape[5])
    for H, W in SMALL:
        for name in CORNERS:
            a, r, K = corner_case(name, H, W)
            for m in (a[0, 0], r[0, 0]):
                _against_scipy(m, K)
    for name in BIG_CORNERS:
        m, K = corner_map(name, 128, 128)
        _against_scipy(m, K)


def test_corner_maps_are_what_they_are_for():
    for connectivity in (4, 8):
        for H, W in SMALL:
            for name in CORNERS:
                m, K = corner_map(name, H, W)
                assert_construction(name, m, K, connectivity)
        for name in BIG_CORNERS:
            m, K = corner_map(name, 128, 128)
            n = assert_construction(name, m, K, connectivity)
            if name == "checkerboard" and connectivity == 4:
                assert n == 8192                              # the most lesions a map can have


def test_random_cases_are_not_trivial():
    """what the GPU tests rely on, by the restatement alone: an all-empty input cannot pass silently"""
    for shape in RANDOM_SHAPES:
        for connectivity in (4, 8):
            st = lesion_case_stats(shape, connectivity)
            n_a, n_r, hit_a, hit_r = (st[k] for k in FIELDS)
            both_empty = float(((n_a == 0) & (n_r == 0)).mean())
            partial_a = float(((hit_a[..., 0] > 0) & (hit_a[..., 0] < n_a)).mean())
            partial_r = float(((hit_r[..., 0] > 0) & (hit_r[..., 0] < n_r)).mean())
            differ = float((hit_a[..., 0] != hit_a[..., 1]).mean())
            print(f"lesion_case{shape} conn={connectivity}: both empty {both_empty:.3f} partial a {partial_a:.3f} r {partial_r:.3f} "
                  f"thresholds differ {differ:.3f} max n_a {int(n_a.max())} n_r {int(n_r.max())}")
            assert both_empty <= 0.25, shape
            assert partial_a > 0 and partial_r > 0 and differ > 0 and int(n_a.max()) >= 2, shape


# ------------------------------------------------------------------------------------------------ CPU: host scores
def _hand_built():
    """B = 2, S = 2, L = 1, two scored classes, overlaps 0/1 and 1/2.  Image 0: two defined cells (class 1), a cell with only the
    sample side and a cell with only the rater side (class 2); image 1: nothing anywhere."""
    n_a = np.zeros((2, 2, 1, 2), dtype=np.int64)
    n_r = np.zeros_like(n_a)
    hit_a = np.zeros((2, 2, 1, 2, 2), dtype=np.int64)
    hit_r = np.zeros_like(hit_a)
    n_a[0, 0, 0, 0], n_r[0, 0, 0, 0], hit_a[0, 0, 0, 0], hit_r[0, 0, 0, 0] = 2, 4, (2, 1), (3, 1)
    n_a[0, 1, 0, 0], n_r[0, 1, 0, 0], hit_a[0, 1, 0, 0], hit_r[0, 1, 0, 0] = 1, 1, (1, 1), (1, 0)
    n_a[0, 0, 0, 1] = 3
    n_r[0, 1, 0, 1] = 2
    return {"n_a": n_a, "n_r": n_r, "hit_a": hit_a, "hit_r": hit_r, "overlaps": [[0, 1], [1, 2]], "connectivity": 8, "classes": [1, 2]}


def test_host_scores_on_hand_built_stats():
    stats = _hand_built()
    r = M.lesion_scores_from_stats(stats, class_names=["nodule", "other"])
    # image 1 has no defined cell and is left out; image 0's defined cells are averaged per score
    assert r["recall"] == [(0.75 + 1.0 + 0.0) / 3, (0.25 + 0.0 + 0.0) / 3]                   # cells with n_r > 0
    assert r["precision"] == [(1.0 + 1.0 + 0.0) / 3, (0.5 + 1.0 + 0.0) / 3]                  # cells with n_a > 0
    assert r["f1"] == [(5 / 6 + 1.0 + 0.0 + 0.0) / 4, (2 / 6 + 0.5 + 0.0 + 0.0) / 4]         # cells with a lesion on either side
    assert r["recall_per_class"] == [[(0.75 + 1.0) / 2, (0.25 + 0.0) / 2], [0.0, 0.0]]
    assert r["precision_per_class"] == [[1.0, 0.75], [0.0, 0.0]]
    assert r["f1_per_class"] == [[(5 / 6 + 1.0) / 2, (2 / 6 + 0.5) / 2], [0.0, 0.0]]
    assert (r["cells"], r["cells_both_empty"], r["cells_sample_empty"], r["cells_rater_empty"], r["images_scored"], r["images"]) == (8, 4, 5, 5, 1, 2)
    assert r["count_error"] == (2 + 0 + 3 + 2) / 8 and r["count_exact"] == 5 / 8
    assert r["lesions_per_sample_map"] == 6 / 8 and r["lesions_per_rater_map"] == 7 / 8
    assert r["class_names"] == ["nodule", "other"] and r["classes"] == [1, 2] and r["connectivity"] == 8
    assert r["overlaps"] == [[0, 1], [1, 2]] and r["thresholds"] == [0.0, 0.5] and r["samples"] == 2 and r["raters"] == 1
    assert json.loads(json.dumps(r)) == r
    # only the rater side anywhere: precision has no defined cell
    only_r = M.lesion_scores_from_stats({**stats, "n_a": np.zeros_like(stats["n_a"]), "hit_a": np.zeros_like(stats["hit_a"])})
    assert only_r["precision"] == [None, None] and only_r["precision_per_class"] == [[None, None], [None, None]]
    assert only_r["recall"] == r["recall"] and only_r["f1"][0] == (3 / 4 + 1.0 + 0.0) / 3
    none = M.lesion_scores_from_stats({**stats, **{k: np.zeros_like(stats[k]) for k in FIELDS}})
    assert none["recall"] == none["precision"] == none["f1"] == [None, None] and none["cells_both_empty"] == 8 and none["images_scored"] == 0
    assert none["count_error"] == 0.0 and none["count_exact"] == 1.0
    assert json.loads(json.dumps(none)) == none
    both = M.concat_lesion_stats([stats, stats])
    assert both["n_a"].shape == (4, 2, 1, 2) and both["hit_r"].shape == (4, 2, 1, 2, 2) and both["overlaps"] == [[0, 1], [1, 2]]
    twice = M.lesion_scores_from_stats(both)
    assert twice["recall"] == r["recall"] and twice["cells"] == 16 and twice["images_scored"] == 2
    with pytest.raises(ValueError, match="class_names"):
        M.lesion_scores_from_stats(stats, class_names=["a"])
    with pytest.raises(ValueError, match="overlaps"):
        M.lesion_scores_from_stats({**stats, "overlaps": [[3, 2], [1, 2]]})
    with pytest.raises(ValueError, match="hit_a"):
        M.lesion_scores_from_stats({**stats, "overlaps": [[1, 2]]})
    with pytest.raises(ValueError, match="connectivity"):
        M.lesion_scores_from_stats({**stats, "connectivity": 6})
    with pytest.raises(ValueError, match=r"expected \[B,S,L,C\]"):
        M.lesion_scores_from_stats({**stats, "n_a": stats["n_a"][0]})
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        M.lesion_stats(torch.zeros((1, 2, 4, 4), dtype=torch.uint8), torch.zeros((1, 2, 4, 4), dtype=torch.uint8), 2)


# ------------------------------------------------------------------------------------------------ CPU: ABI
def workspace_formula(B, S, L, H, W, K):
    return 4 * B * (S + L) * len(scored_classes(K)) * (H * W + 1)      # the label planes, then one lesion count per plane


def test_lesions_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_lesions[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_lesions")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
        assert not name.startswith(("ccdm_seg_", "ccdm_segboundary", "ccdm_segcalib", "ccdm_lidc", "ccdm_surfdist", "ccdm_css", "ccdm_vote_"))
    assert len(hip.SIGNATURES["ccdm_lesions"][1]) == 15 and len(hip.SIGNATURES["ccdm_lesions_workspace_bytes"][1]) == 6
    assert "ccdm_lesions.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_lesions.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    assert lib.ccdm_lesions_workspace_bytes(4, 100, 4, 128, 128, 2) == 4 * 4 * 104 * (128 * 128 + 1) == workspace_formula(4, 100, 4, 128, 128, 2)
    assert lib.ccdm_lesions_workspace_bytes(1, 3, 2, 5, 7, 4) == 4 * 5 * 3 * 36 and lib.ccdm_lesions_workspace_bytes(1, 3, 2, 5, 7, 1) == 4 * 5 * 36
    assert lib.ccdm_lesions_workspace_bytes(0, 3, 2, 5, 7, 2) == 0 and lib.ccdm_lesions_workspace_bytes(1, 3, 2, 5, 0, 2) == 0


def test_lesions_refuses_what_it_cannot_score():
    """the limits are checked before anything is launched or read: host buffers stand in for the device's"""
    lib = hip.load()
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data

    def call(B=1, S=3, L=2, H=8, W=8, K=2, conn=8, overlaps=((0, 1), (1, 2)), T=None, stats=p, ws=p, ws_bytes=buf.nbytes):
        ov = None if overlaps is None else np.ascontiguousarray(overlaps, dtype=np.int32)
        T = (0 if ov is None else len(ov)) if T is None else T
        return lib.ccdm_lesions(p, p, B, S, L, H, W, K, conn, None if ov is None else ov.ctypes.data, T, stats, ws, ws_bytes, None)

    nine = ((1, 2),) * 9
    for change, what in ((dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(S=0), "S=0"), (dict(S=256), "S=256"), (dict(L=256), "L=256"),
                         (dict(W=0), "W=0"), (dict(H=0), "H=0"), (dict(H=128, W=129), "H*W=16512"), (dict(H=1, W=16385), "H*W=16385"),
                         (dict(conn=6), "connectivity=6"), (dict(T=0), "T=0"), (dict(overlaps=nine), "T=9"),
                         (dict(overlaps=((0, 1), (1, 0))), "den=0"), (dict(overlaps=((1, 65537),)), "den=65537"),
                         (dict(overlaps=((3, 2),)), "num=3 den=2"), (dict(overlaps=((0, 1), (-1, 2))), "num=-1"), (dict(B=-1), "B=-1"),
                         (dict(B=0, K=33), "K=33"), (dict(B=0, overlaps=((3, 2),)), "num=3 den=2"), (dict(stats=None), "null"),
                         (dict(overlaps=None, T=2), "null"), (dict(ws=None), "workspace"),
                         (dict(ws_bytes=workspace_formula(1, 3, 2, 8, 8, 2) - 1), f"workspace of {workspace_formula(1, 3, 2, 8, 8, 2) - 1} bytes"),
                         # 129 x 127 = 16383 pixels pass the size check: the call fails at the next one, on its workspace
                         (dict(H=129, W=127, ws_bytes=workspace_formula(1, 3, 2, 129, 127, 2) - 1), f"{workspace_formula(1, 3, 2, 129, 127, 2)} needed"),
                         (dict(ws=p + 2), "4-byte aligned")):
        rc = call(**change)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "lesions")
    assert not buf.any()
    assert call(B=0) == 0 and call(B=0, ws=None, ws_bytes=0) == 0 and not buf.any()      # B = 0: nothing launched, nothing written


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def kernel(samples: torch.Tensor, raters: torch.Tensor, K: int, connectivity: int = 8, overlaps=OVERLAPS):
    """one ccdm_lesions call on uint8 device stacks [B,S,H,W] / [B,L,H,W] (as they lie in memory) -> (the dict of per-cell arrays,
    the label planes [B*S + B*L, C, H, W], the lesion counts [B*S + B*L, C]); the outputs start from a non-zero fill: the call overwrites"""
    lib = hip.load()
    assert samples.is_cuda and raters.is_cuda and samples.dtype == raters.dtype == torch.uint8
    assert samples.is_contiguous() and raters.is_contiguous()
    B, S, H, W = samples.shape
    L = raters.shape[1]
    Cn, T = len(scored_classes(K)), len(overlaps)
    ov = np.ascontiguousarray(overlaps, dtype=np.int32)
    stats = torch.full((B, S, L, Cn, 2 + 2 * T), 77, dtype=torch.int32, device="cuda")
    need = int(lib.ccdm_lesions_workspace_bytes(B, S, L, H, W, K))
    assert need == workspace_formula(B, S, L, H, W, K)
    ws = torch.full((need // 4,), -7, dtype=torch.int32, device="cuda")
    hip.check(lib.ccdm_lesions(samples.data_ptr(), raters.data_ptr(), B, S, L, H, W, K, connectivity, ov.ctypes.data, T, stats.data_ptr(),
                               ws.data_ptr(), need, None), "lesions")
    torch.cuda.synchronize()
    st = stats.cpu().numpy().astype(np.int64)
    nplanes = B * (S + L) * Cn
    host = ws.cpu().numpy()
    out = {"n_a": st[..., 0], "n_r": st[..., 1], "hit_a": st[..., 2:2 + T], "hit_r": st[..., 2 + T:],
           "overlaps": [[int(n), int(d)] for n, d in overlaps], "connectivity": connectivity, "classes": scored_classes(K)}
    return out, host[:nplanes * H * W].reshape(B * (S + L), Cn, H, W), host[nplanes * H * W:].reshape(B * (S + L), Cn)


def assert_stats_equal(got, want, tag=""):
    bad = {k: int((got[k] != want[k]).sum()) for k in FIELDS}
    print(f"lesions[{tag} {want['n_a'].shape}] max n_a={int(want['n_a'].max(initial=0))} n_r={int(want['n_r'].max(initial=0))} "
          f"hits a={int(want['hit_a'].sum())} r={int(want['hit_r'].sum())} mismatches={bad}")
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["classes"] == want["classes"] and got["overlaps"] == want["overlaps"] and got["connectivity"] == want["connectivity"]


def check_exact(samples: np.ndarray, raters: np.ndarray, K: int, connectivity: int, overlaps=OVERLAPS, want=None, tag=""):
    """labels against scipy for every map and class, lesion counts, stats against the restatement"""
    got, planes, counts = kernel(torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda(), K, connectivity, overlaps)
    H, W = samples.shape[2:]
    maps = np.concatenate([samples.reshape(-1, H, W), raters.reshape(-1, H, W)])
    for mi, m in enumerate(maps):
        for ci, c in enumerate(scored_classes(K)):
            lab, n = scipy_labels(m == c, connectivity)
            np.testing.assert_array_equal(planes[mi, ci], lab, err_msg=f"{tag}: labels of map {mi} class {c}")
            assert counts[mi, ci] == n, (tag, mi, c)
    want = stats_restatement(samples, raters, K, connectivity, overlaps) if want is None else want
    assert_stats_equal(got, want, tag)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("B,S,L,H,W,K", RANDOM_SHAPES)
def test_labels_match_scipy(B, S, L, H, W, K, connectivity):
    samples, raters = lesion_case(B, S, L, H, W, K)
    want = lesion_case_stats((B, S, L, H, W, K), connectivity)
    assert float(((want["n_a"] == 0) & (want["n_r"] == 0)).mean()) <= 0.25 and int(want["n_a"].max()) >= 2
    check_exact(samples, raters, K, connectivity, want=want, tag="random")


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SMALL)
@pytest.mark.parametrize("name", CORNERS)
def test_corner_maps(name, H, W, connectivity):
    a, r, K = corner_case(name, H, W)
    n = assert_construction(name, a[0, 0], K, connectivity)
    got, _ = check_exact(a, r, K, connectivity, tag=name)
    assert int(got["n_a"][0, 0, 1, 0]) == int(got["n_r"][0, 0, 1, 0]) == n
    np.testing.assert_array_equal(got["hit_a"][0, 0, 1, 0], [n, n])                # against itself every lesion is wholly covered
    if name == "empty":
        assert not got["hit_a"].any() and not got["hit_r"].any() and got["n_r"][0, 0, 0, 0] == 1     # zeros are written over the prefill


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", BIG_CORNERS)
def test_corner_maps_at_the_largest_map(name, connectivity):
    a, r, K = corner_case(name, 128, 128)
    n = assert_construction(name, a[0, 0], K, connectivity)
    got, _ = check_exact(a, r, K, connectivity, tag=name + "@128")
    assert int(got["n_a"][0, 0, 0, 0]) == n and got["hit_a"][0, 0, 1, 0].tolist() == [n, n]
    if name == "checkerboard" and connectivity == 4:
        # rolled by (1, 2) the board is its complement: 8192 lesions a side, none covered
        assert n == 8192 and int(got["n_r"][0, 0, 0, 0]) == 8192 and not got["hit_a"][0, 0, 0].any() and not got["hit_r"][0, 0, 0].any()


@pytest.mark.gpu
def test_threshold_edges():
    H, W = 12, 16
    a, r = np.zeros((1, 1, H, W), dtype=np.uint8), np.zeros((1, 1, H, W), dtype=np.uint8)
    r[0, 0, 2, 2:6] = 1                                       # 4 pixels, 2 of them covered
    a[0, 0, 2, 4:9] = 1
    r[0, 0, 6, 1:4] = 1                                       # covered by nothing
    r[0, 0, 9:11, 9:11] = 1                                   # wholly inside the sample's mask
    a[0, 0, 8:12, 8:12] = 1
    ov = ((0, 1), (1, 2), (3, 4), (1, 1), (2, 4), (65536, 65536), (1, 65536), (32769, 65536))
    want = stats_restatement(a, r, 2, 8, ov)
    assert want["n_r"].item() == 3 and want["n_a"].item() == 2
    assert want["hit_r"][0, 0, 0, 0].tolist() == [2, 2, 1, 1, 2, 1, 2, 1]     # half covered: hit at 1/2 and 2/4, not at 3/4 or 32769/65536
    assert want["hit_a"][0, 0, 0, 0].tolist() == [2, 0, 0, 0, 0, 0, 2, 0]     # 2 of 5 and 4 of 16 pixels covered
    got, _ = check_exact(a, r, 2, 8, ov, want=want, tag="thresholds")
    s_dev, r_dev = torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda()
    for t, o in enumerate(ov):                                # T = 8 in one call is eight calls with T = 1
        one, _, _ = kernel(s_dev, r_dev, 2, 8, (o,))
        assert one["hit_a"].shape == (1, 1, 1, 1, 1)
        np.testing.assert_array_equal(one["hit_a"][..., 0], got["hit_a"][..., t])
        np.testing.assert_array_equal(one["hit_r"][..., 0], got["hit_r"][..., t])
        np.testing.assert_array_equal(one["n_a"], got["n_a"])
    # the same eight thresholds on a random case
    samples, raters = lesion_case(2, 3, 2, 33, 47, 2)
    check_exact(samples, raters, 2, 4, ov, tag="thresholds random")


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
def test_swapped_stacks_trade_sides(connectivity):
    samples, raters = lesion_case(2, 5, 4, 40, 56, 4)
    want = lesion_case_stats((2, 5, 4, 40, 56, 4), connectivity)
    swapped, _, _ = kernel(torch.from_numpy(np.array(raters)).cuda(), torch.from_numpy(np.array(samples)).cuda(), 4, connectivity)
    for k1, k2 in (("n_a", "n_r"), ("n_r", "n_a"), ("hit_a", "hit_r"), ("hit_r", "hit_a")):
        np.testing.assert_array_equal(swapped[k1], np.swapaxes(want[k2], 1, 2), err_msg=k1)


@pytest.mark.gpu
def test_unaligned_base_pointers():
    """W % 4 == 0 but the stacks start one byte off a dword: the byte path, on either stack or both"""
    B, S, L, H, W, K = 2, 5, 4, 40, 56, 4
    samples, raters = lesion_case(B, S, L, H, W, K)
    want = lesion_case_stats((B, S, L, H, W, K), 8)
    s_buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    r_buf = torch.zeros(raters.size + 1, dtype=torch.uint8, device="cuda")
    s_dev, r_dev = s_buf[1:].view(B, S, H, W), r_buf[1:].view(B, L, H, W)
    s_dev.copy_(torch.from_numpy(np.array(samples))); r_dev.copy_(torch.from_numpy(np.array(raters)))
    assert s_dev.data_ptr() % 4 == 1 and r_dev.data_ptr() % 4 == 1
    aligned, planes, counts = kernel(torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda(), K)
    assert_stats_equal(aligned, want, "aligned")
    for s_t, r_t in ((s_dev, r_dev), (s_dev, torch.from_numpy(np.array(raters)).cuda()), (torch.from_numpy(np.array(samples)).cuda(), r_dev)):
        got, p, c = kernel(s_t, r_t, K)
        assert_stats_equal(got, want, "unaligned")
        np.testing.assert_array_equal(p, planes)
        np.testing.assert_array_equal(c, counts)


@pytest.mark.gpu
def test_repeated_call_is_identical_and_no_image_is_no_work():
    lib = hip.load()
    samples, raters = lesion_case(2, 5, 4, 40, 56, 4)
    s_dev, r_dev = torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda()
    first, second = kernel(s_dev, r_dev, 4, 4), kernel(s_dev, r_dev, 4, 4)
    for k in FIELDS:
        np.testing.assert_array_equal(first[0][k], second[0][k])
    np.testing.assert_array_equal(first[1], second[1])
    np.testing.assert_array_equal(first[2], second[2])
    assert_stats_equal(first[0], lesion_case_stats((2, 5, 4, 40, 56, 4), 4), "repeat")
    # B = 0 leaves prefilled outputs as they are
    st = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    ws = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    ov = np.array(OVERLAPS, dtype=np.int32)
    assert lib.ccdm_lesions(s_dev.data_ptr(), r_dev.data_ptr(), 0, 5, 4, 40, 56, 4, 8, ov.ctypes.data, 2, st.data_ptr(), ws.data_ptr(), 32, None) == 0
    torch.cuda.synchronize()
    assert bool((st == 9).all()) and bool((ws == 9).all())


@pytest.mark.gpu
def test_lesion_stats_takes_index_maps():
    samples, raters = lesion_case(2, 3, 2, 33, 47, 2)
    s64, r64 = torch.from_numpy(samples.astype(np.int64)).cuda(), torch.from_numpy(raters.astype(np.int64)).cuda()
    got = M.lesion_stats(s64, r64, 2)
    assert got["n_a"].dtype == np.int64 and got["hit_a"].dtype == np.int64 and got["n_a"].shape == (2, 3, 2, 1) and got["hit_r"].shape == (2, 3, 2, 1, 2)
    assert_stats_equal(got, lesion_case_stats((2, 3, 2, 33, 47, 2), 8), "int64 maps")
    sliced = M.lesion_stats(s64[:, :2], r64, 2, connectivity=4, overlaps=((1, 4),))          # the evaluator's pred_idx[:, :s]
    assert_stats_equal(sliced, stats_restatement(samples[:, :2], raters, 2, 4, ((1, 4),)), "sliced")
    both = M.concat_lesion_stats([got, got])
    assert both["n_a"].shape == (4, 3, 2, 1) and both["hit_a"].shape == (4, 3, 2, 1, 2) and both["classes"] == [1] and both["connectivity"] == 8
    with pytest.raises(ValueError, match="expected"):
        M.lesion_stats(s64[:, :, :8], r64, 2)
    with pytest.raises(hip.CcdmHipError, match="connectivity=6"):
        M.lesion_stats(s64, r64, 2, connectivity=6)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_lesions_end_to_end(tmp_path):
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
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"lesions": True}}, dataset=DS(), device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"lesions"}
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
    assert len(res["lesions"]) == len(evaluations)
    for s, got in zip(evaluations, res["lesions"]):
        want = M.lesion_scores_from_stats(stats_restatement(pred[:, :s], lab, K, 8, ((0, 1), (1, 2))))
        print(f"lesions[{s}] got={got}")
        assert got["samples"] == s and got["images"] == 5 and got["raters"] == 4 and got["overlaps"] == [[0, 1], [1, 2]] and got["connectivity"] == 8
        assert got["cells_rater_empty"] > 0 and got["cells"] - got["cells_rater_empty"] > 0 and got["recall"][0] is not None   # some annotations are empty
        assert got == want                                    # ratios of integers, reduced in the same order
    quarter = E.eval_lidc_uncertainty({**params, "evaluation": {"lesions": True, "lesion_overlaps": [0.25], "lesion_connectivity": 4},
                                       "output_path": None}, dataset=DS(), device="cuda:0", model=fake())["lesions"]
    want4 = M.lesion_scores_from_stats(stats_restatement(pred[:, :2], lab, K, 4, ((1, 4),)))
    assert quarter[0]["overlaps"] == [[1, 4]] and quarter[0]["connectivity"] == 4 and quarter[0] == want4
    assert quarter[0]["lesions_per_sample_map"] > res["lesions"][0]["lesions_per_sample_map"]            # fewer joins, more lesions
    for bad in ({"lesion_overlaps": [1.5]}, {"lesion_overlaps": [-0.1]}, {"lesion_connectivity": 6}):
        with pytest.raises(ValueError, match="lesion_"):
            E.eval_lidc_uncertainty({**params, "evaluation": {"lesions": True, **bad}, "output_path": None}, dataset=DS(), device="cuda:0",
                                    model=fake())
    with open(tmp_path / "out" / "lidc_lesions.json") as f:
        assert json.load(f) == res["lesions"] == json.loads(json.dumps(res["lesions"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_lesions.json"]
