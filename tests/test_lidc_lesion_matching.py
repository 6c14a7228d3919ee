"""LIDC matched-lesion scores: the size and pair kernels (ccdm_lesion_match), metrics.lesion_match_stats,
metrics.lesion_match_scores_from_stats and the `evaluation.lesion_matching` keys of eval_lidc_uncertainty.  Nothing in the reference
computes these.  Everything the kernels write is an integer, so every kernel test asks for equality of all four arrays (n_a, n_r, tp,
iou_sum) with a restatement of the definition in include/ccdm_hip.h: scipy.ndimage.label per map and class, sizes by np.bincount,
pair counts by np.unique over the doubly-masked pixels, the match test and floor(inter * 2^32 / union) in Python integers.  The
restatement itself is held against a double loop over all lesion pairs on small maps."""
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
SYMBOLS = {"ccdm_lesion_match", "ccdm_lesion_match_workspace_bytes"}
FIELDS = ("n_a", "n_r", "tp", "iou_sum")
THRESHOLDS = ((1, 2), (3, 4))
ONE = 1 << 32
BLOB_SEED = 4118          # chosen on the CPU so that the restatement alone meets assert_not_trivial on every shape below


# ------------------------------------------------------------------------------------------------ restatement
def scored_classes(K: int):
    return list(range(1, K)) if K > 1 else [0]


def labels_and_sizes(mask: np.ndarray, connectivity: int):
    """-> (labels [H,W], sizes [n]: the pixels of lesion 1..n)"""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    return lab.astype(np.int64), np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)


def cell_restatement(la, size_a, lr, size_r, thresholds, min_size):
    """one cell -> (n_a, n_r, tp [T], iou_sum [T]) in Python integers"""
    n_r = len(size_r)
    both = (la > 0) & (lr > 0)
    codes, inters = np.unique(la[both] * (n_r + 1) + lr[both], return_counts=True)
    tp, q = [0] * len(thresholds), [0] * len(thresholds)
    for code, inter in zip(codes.tolist(), inters.tolist()):
        a, r = divmod(code, n_r + 1)
        sa, sr = int(size_a[a - 1]), int(size_r[r - 1])
        if sa < min_size or sr < min_size:
            continue
        union = sa + sr - inter
        for t, (num, den) in enumerate(thresholds):
            if inter * den > num * union:
                tp[t] += 1
                q[t] += (inter << 32) // union
    return int((size_a >= min_size).sum()), int((size_r >= min_size).sum()), tp, q


def cell_brute_force(la, size_a, lr, size_r, thresholds, min_size):
    """the same by a double loop over all lesion pairs; a lesion with two partners would be an error of the definition"""
    keep_a = [a for a in range(1, len(size_a) + 1) if size_a[a - 1] >= min_size]
    keep_r = [r for r in range(1, len(size_r) + 1) if size_r[r - 1] >= min_size]
    tp, q = [0] * len(thresholds), [0] * len(thresholds)
    for t, (num, den) in enumerate(thresholds):
        partners_a, partners_r = {}, {}
        for a in keep_a:
            for r in keep_r:
                inter = int(((la == a) & (lr == r)).sum())
                union = int((la == a).sum()) + int((lr == r).sum()) - inter
                if inter * den > num * union:
                    tp[t] += 1
                    q[t] += inter * ONE // union
                    partners_a[a] = partners_a.get(a, 0) + 1
                    partners_r[r] = partners_r.get(r, 0) + 1
        assert all(v == 1 for v in partners_a.values()) and all(v == 1 for v in partners_r.values())
    return len(keep_a), len(keep_r), tp, q


def stats_restatement(samples: np.ndarray, raters: np.ndarray, K: int, connectivity: int = 8, thresholds=THRESHOLDS, min_size: int = 1,
                      cell=cell_restatement):
    """samples [B,S,H,W], raters [B,L,H,W] -> the dict metrics.lesion_match_stats returns, by the definition"""
    B, S = samples.shape[:2]
    L = raters.shape[1]
    classes = scored_classes(K)
    T = len(thresholds)
    n_a = np.zeros((B, S, L, len(classes)), dtype=np.int64)
    n_r = np.zeros_like(n_a)
    tp = np.zeros((B, S, L, len(classes), T), dtype=np.int64)
    iou_sum = np.zeros_like(tp)
    for b in range(B):
        for ci, c in enumerate(classes):
            side_a = [labels_and_sizes(samples[b, i] == c, connectivity) for i in range(S)]
            side_r = [labels_and_sizes(raters[b, j] == c, connectivity) for j in range(L)]
            for i in range(S):
                for j in range(L):
                    n_a[b, i, j, ci], n_r[b, i, j, ci], tp[b, i, j, ci], iou_sum[b, i, j, ci] = cell(*side_a[i], *side_r[j], thresholds, min_size)
    return {"n_a": n_a, "n_r": n_r, "tp": tp, "iou_sum": iou_sum, "thresholds": [[int(n), int(d)] for n, d in thresholds],
            "connectivity": int(connectivity), "min_size": int(min_size), "classes": classes}


# ------------------------------------------------------------------------------------------------ inputs
def _perturbed(m: np.ndarray, rng, K: int):
    """a copy of the map: half of the time moved by one pixel, a share of the pixels next to a lesion added to it, now and then a
    lesion cut away or a speck added"""
    H, W = m.shape
    out = m.copy()
    if rng.random() < 0.5:
        out = np.roll(out, int(rng.choice([-1, 1])), axis=int(rng.integers(0, 2)))
    grown = np.maximum.reduce([out, np.roll(out, 1, 0), np.roll(out, -1, 0), np.roll(out, 1, 1), np.roll(out, -1, 1)])
    out = np.where((rng.random((H, W)) < 0.25) & (out == 0), grown, out)
    if rng.random() < 0.3:                                            # a lesion the copy misses, or a part of one
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        out[max(0, y - H // 5):y + H // 5 + 1, max(0, x - W // 5):x + W // 5 + 1] = 0
    if rng.random() < 0.5:                                            # a lesion only the copy has
        out[int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.integers(1, K))
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def blob_case(B, S, L, H, W, K):
    """seeded maps: per image a base map with one to three boxes per scored class; every rater and every sample is a perturbed copy of
    it, so that most lesions have a partner above IoU 1/2, some only below 3/4, some none.  -> (samples, raters)"""
    rng = np.random.default_rng(BLOB_SEED + 131 * H + 17 * W + 5 * K)
    samples = np.zeros((B, S, H, W), dtype=np.uint8)
    raters = np.zeros((B, L, H, W), dtype=np.uint8)
    for b in range(B):
        base = np.zeros((H, W), dtype=np.uint8)
        for c in range(1, K):
            for _ in range(1 if H * W < 100 else int(rng.integers(2, 4))):
                h, w = int(rng.integers(2, max(3, H // 3))), int(rng.integers(2, max(3, W // 3)))
                y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                base[y:y + h, x:x + w] = c
        for j in range(L):
            raters[b, j] = _perturbed(base, rng, K)
        for i in range(S):
            samples[b, i] = _perturbed(base, rng, K)
    for s in (samples, raters):
        s.setflags(write=False)
    return samples, raters


@functools.lru_cache(maxsize=None)
def blob_case_stats(shape, connectivity):
    samples, raters = blob_case(*shape)
    return stats_restatement(samples, raters, shape[5], connectivity)


def assert_not_trivial(want, tag):
    """what the issue asks of a random case, by the restatement alone, before a kernel is asked"""
    n_a, n_r, tp = want["n_a"], want["n_r"], want["tp"]
    matched = float((tp[..., 0] > 0).mean())
    print(f"blob_case{tag}: cells matched {matched:.3f} fp cells {int((n_a > tp[..., 0]).sum())} fn cells {int((n_r > tp[..., 0]).sum())} "
          f"cells that lose a pair at 3/4 {int((tp[..., 1] < tp[..., 0]).sum())} max n_a {int(n_a.max())} n_r {int(n_r.max())}")
    assert matched >= 0.5, tag
    assert (n_a > tp[..., 0]).any() and (n_r > tp[..., 0]).any() and (tp[..., 1] < tp[..., 0]).any(), tag


# (B, S, L, H, W, K): 7x9 the byte path of the labelling; 16x16 and 32x48 its dword path, 32x48 with more than one chunk of pixels per wave
BLOB_SHAPES = [(2, 3, 2, 7, 9, 2), (2, 3, 2, 7, 9, 3), (2, 3, 2, 16, 16, 2), (2, 3, 2, 16, 16, 3), (2, 3, 2, 32, 48, 2), (2, 3, 2, 32, 48, 3)]


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def sized_lesions():
    """lesions of 1, 2 and 5 pixels (connectivity 8), far apart"""
    m = np.zeros((12, 16), dtype=np.uint8)
    m[1, 1] = 1
    m[4, 3:5] = 1
    m[8, 8:13] = 1
    return m


# ------------------------------------------------------------------------------------------------ CPU: restatement
def test_restatement_equals_brute_force_over_all_pairs():
    rng = np.random.default_rng(77)
    some_tp = 0
    for trial in range(12):
        K = 2 + trial % 2
        raters = np.where(rng.random((1, 2, 6, 7)) < 0.5, rng.integers(1, K, (1, 2, 6, 7)), 0).astype(np.uint8)
        samples = np.stack([_perturbed(raters[0, i % 2], rng, K) for i in range(3)])[None]
        for connectivity in (4, 8):
            for min_size in (1, 3):
                fast = stats_restatement(samples, raters, K, connectivity, ((1, 2), (2, 3), (3, 4)), min_size)
                slow = stats_restatement(samples, raters, K, connectivity, ((1, 2), (2, 3), (3, 4)), min_size, cell=cell_brute_force)
                for k in FIELDS:
                    np.testing.assert_array_equal(fast[k], slow[k], err_msg=k)
                some_tp += int(fast["tp"].sum())
                assert (fast["tp"] <= np.minimum(fast["n_a"], fast["n_r"])[..., None]).all()
                assert (fast["iou_sum"] <= fast["tp"] * ONE).all() and (2 * fast["iou_sum"] > fast["tp"] * ONE)[fast["tp"] > 0].all()
    assert some_tp > 50


def test_blob_cases_are_not_trivial():
    for shape in BLOB_SHAPES:
        for connectivity in (4, 8):
            assert_not_trivial(blob_case_stats(shape, connectivity), (shape, connectivity))


# ------------------------------------------------------------------------------------------------ CPU: host scores
def _hand_built():
    """B = 2, S = 1, L = 2, one class, thresholds 1/2 and 3/4.
    image 0: cell (0,0): 2 sample and 2 rater lesions, both matched at 1/2 with IoUs 0.75 and 0.625, none at 3/4
             cell (0,1): 1 sample lesion, 3 rater lesions, nothing matched
    image 1: cell (0,0): nothing on either side;  cell (0,1): 1 and 1, matched at both thresholds with IoU 1"""
    n_a = np.array([[[[2], [1]]], [[[0], [1]]]], dtype=np.int64)
    n_r = np.array([[[[2], [3]]], [[[0], [1]]]], dtype=np.int64)
    tp = np.zeros((2, 1, 2, 1, 2), dtype=np.int64)
    iou_sum = np.zeros_like(tp)
    tp[0, 0, 0, 0], iou_sum[0, 0, 0, 0] = (2, 0), (ONE * 3 // 4 + ONE * 5 // 8, 0)
    tp[1, 0, 1, 0], iou_sum[1, 0, 1, 0] = (1, 1), (ONE, ONE)
    return {"n_a": n_a, "n_r": n_r, "tp": tp, "iou_sum": iou_sum, "thresholds": [[1, 2], [3, 4]], "connectivity": 8, "min_size": 1, "classes": [1]}


def test_host_scores_on_hand_built_stats():
    stats = _hand_built()
    r = M.lesion_match_scores_from_stats(stats, class_names=["nodule"])
    # at 1/2: image 0 has rq (1, 0), pq (1.375/2, 0), sq (1.375/2) in its one matched cell; image 1 has one defined cell: 1, 1, 1
    assert r["rq"] == [(0.5 + 1.0) / 2, (0.0 + 1.0) / 2]
    assert r["pq"] == [((2 * 1.375 / 4 + 0.0) / 2 + 1.0) / 2, (0.0 + 1.0) / 2]
    assert r["sq"] == [(1.375 / 2 + 1.0) / 2, 1.0]                   # tp = 0 leaves sq undefined: at 3/4 only image 1 has a value
    assert r["rq_per_class"] == [r["rq"]] and r["pq_per_class"] == [r["pq"]] and r["sq_per_class"] == [r["sq"]]
    # pooled over all cells at 1/2: tp 3, fp 4 - 3, fn 6 - 3, q = 2.375: not the mean of means
    assert (r["tp_total"], r["fp_total"], r["fn_total"]) == ([3, 1], [1, 3], [3, 5])
    assert r["pq_pooled"] == [2.375 / 5.0, 1.0 / 5.0] and r["sq_pooled"] == [2.375 / 3, 1.0] and r["rq_pooled"] == [3 / 5.0, 1 / 5.0]
    assert r["pq_pooled"][0] != r["pq"][0]
    assert (r["cells"], r["cells_both_empty"], r["cells_matched"], r["images_scored"], r["images"]) == (4, 1, [2, 1], 2, 2)
    assert r["thresholds"] == [[1, 2], [3, 4]] and r["ious"] == [0.5, 0.75] and r["samples"] == 1 and r["raters"] == 2
    assert r["class_names"] == ["nodule"] and r["classes"] == [1] and r["connectivity"] == 8 and r["min_size"] == 1
    assert json.loads(json.dumps(r)) == r
    # a cell with lesions and tp = 0: sq undefined, pq = rq = 0
    unmatched = {**stats, "n_a": stats["n_a"][:1, :, 1:], "n_r": stats["n_r"][:1, :, 1:], "tp": stats["tp"][:1, :, 1:], "iou_sum": stats["iou_sum"][:1, :, 1:]}
    u = M.lesion_match_scores_from_stats(unmatched)
    assert u["sq"] == [None, None] and u["pq"] == [0.0, 0.0] and u["rq"] == [0.0, 0.0] and u["sq_pooled"] == [None, None] and u["pq_pooled"] == [0.0, 0.0]
    assert json.loads(json.dumps(u)) == u
    # both sides empty everywhere: undefined everywhere, and counted
    none = M.lesion_match_scores_from_stats({**stats, **{k: np.zeros_like(stats[k]) for k in FIELDS}})
    assert none["pq"] == none["sq"] == none["rq"] == none["pq_pooled"] == none["sq_pooled"] == none["rq_pooled"] == [None, None]
    assert none["cells_both_empty"] == 4 and none["images_scored"] == 0 and none["cells_matched"] == [0, 0]
    assert json.loads(json.dumps(none)) == none
    both = M.concat_lesion_match_stats([stats, stats])
    assert both["n_a"].shape == (4, 1, 2, 1) and both["iou_sum"].shape == (4, 1, 2, 1, 2) and both["thresholds"] == [[1, 2], [3, 4]] and both["min_size"] == 1
    twice = M.lesion_match_scores_from_stats(both)
    assert twice["pq"] == r["pq"] and twice["cells"] == 8 and twice["images_scored"] == 4 and twice["pq_pooled"] == r["pq_pooled"]
    with pytest.raises(ValueError, match="class_names"):
        M.lesion_match_scores_from_stats(stats, class_names=["a", "b"])
    with pytest.raises(ValueError, match="thresholds"):
        M.lesion_match_scores_from_stats({**stats, "thresholds": [[2, 5], [3, 4]]})
    with pytest.raises(ValueError, match="thresholds"):
        M.lesion_match_scores_from_stats({**stats, "thresholds": [[1, 1], [3, 4]]})
    with pytest.raises(ValueError, match="tp"):
        M.lesion_match_scores_from_stats({**stats, "thresholds": [[1, 2]]})
    with pytest.raises(ValueError, match="min_size"):
        M.lesion_match_scores_from_stats({**stats, "min_size": 0})
    with pytest.raises(ValueError, match=r"expected \[B,S,L,C\]"):
        M.lesion_match_scores_from_stats({**stats, "n_a": stats["n_a"][0]})
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        M.lesion_match_stats(torch.zeros((1, 2, 4, 4), dtype=torch.uint8), torch.zeros((1, 2, 4, 4), dtype=torch.uint8), 2)


def test_evaluation_keys_are_parsed_as_written():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    assert E.lesion_match_thresholds([0.5, 0.75]) == [(1, 2), (3, 4)] and E.lesion_match_thresholds(0.5) == [(1, 2)]
    assert E.lesion_match_thresholds([0.6, "0.9"]) == [(3, 5), (9, 10)]          # the decimal as written, not the nearest double
    for bad in (0.4, 1, [0.5, 1.0], [], [0.5] * 9, "half", True, 0.50001):
        with pytest.raises(ValueError, match="lesion_match_ious"):
            E.lesion_match_thresholds(bad)
    assert E.lesion_min_size(1) == 1 and E.lesion_min_size(7) == 7
    for bad in (0, -1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="lesion_min_size"):
            E.lesion_min_size(bad)
    assert E.lesion_connectivity({}) == 8 and E.lesion_connectivity({"lesion_connectivity": 4}) == 4
    with pytest.raises(ValueError, match="lesion_connectivity"):
        E.lesion_connectivity({"lesion_connectivity": 6})


# ------------------------------------------------------------------------------------------------ CPU: ABI
def lesions_workspace_formula(B, S, L, H, W, K):
    return 4 * B * (S + L) * len(scored_classes(K)) * (H * W + 1)


def workspace_formula(B, S, L, H, W, K):
    """what ccdm_lesions leaves, then a size per possible lesion and one kept-lesion count per plane"""
    return lesions_workspace_formula(B, S, L, H, W, K) + 4 * B * (S + L) * len(scored_classes(K)) * ((H * W + 1) // 2 + 1)


def test_lesion_match_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_lesion_match[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_lesion_match")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
    assert len(hip.SIGNATURES["ccdm_lesion_match"][1]) == 14 and len(hip.SIGNATURES["ccdm_lesion_match_workspace_bytes"][1]) == 6
    assert "ccdm_lesionmatch.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_lesionmatch.hip"))
    lib = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_lesion_match_workspace_bytes(4, 100, 4, 128, 128, 2) == workspace_formula(4, 100, 4, 128, 128, 2) \
        == 4 * 4 * 104 * (16385 + 8193)
    assert lib.ccdm_lesion_match_workspace_bytes(1, 3, 2, 5, 7, 4) == 4 * 5 * 3 * (36 + 19)
    assert lib.ccdm_lesion_match_workspace_bytes(1, 3, 2, 5, 7, 1) == 4 * 5 * (36 + 19)
    assert lib.ccdm_lesion_match_workspace_bytes(0, 3, 2, 5, 7, 2) == 0 and lib.ccdm_lesion_match_workspace_bytes(1, 3, 2, 5, 0, 2) == 0
    for shape in ((4, 100, 4, 128, 128, 2), (1, 3, 2, 5, 7, 4)):      # the front of the buffer is ccdm_lesions' own
        assert lib.ccdm_lesion_match_workspace_bytes(*shape) > lib.ccdm_lesions_workspace_bytes(*shape) == lesions_workspace_formula(*shape)


REFUSALS = ((dict(thresholds=((2, 5),)), "threshold 0: num=2 den=5"), (dict(thresholds=((1, 2), (1, 1))), "threshold 1: num=1 den=1"),
            (dict(min_size=0), "min_size=0"), (dict(H=128, W=129), "H*W=16512"))


def test_lesion_match_refuses_what_it_cannot_score():
    """the limits are checked before anything is launched or read: host buffers stand in for the device's"""
    lib = hip.load()
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data

    def call(B=1, S=3, L=2, H=8, W=8, K=2, thresholds=THRESHOLDS, T=None, min_size=1, stats=p, iou=p, ws=p, ws_bytes=buf.nbytes):
        th = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.int32)
        T = (0 if th is None else len(th)) if T is None else T
        return lib.ccdm_lesion_match(B, S, L, H, W, K, None if th is None else th.ctypes.data, T, min_size, stats, iou, ws, ws_bytes, None)

    need = workspace_formula(1, 3, 2, 8, 8, 2)
    for change, what in REFUSALS + (
            (dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(S=0), "S=0"), (dict(S=256), "S=256"), (dict(L=256), "L=256"), (dict(W=0), "W=0"),
            (dict(H=0), "H=0"), (dict(H=1, W=16385), "H*W=16385"), (dict(T=0), "T=0"), (dict(thresholds=((1, 2),) * 9), "T=9"),
            (dict(thresholds=((0, 1),)), "threshold 0: num=0 den=1"), (dict(thresholds=((1, 2), (49, 100))), "threshold 1: num=49 den=100"),
            (dict(thresholds=((3, 2),)), "threshold 0: num=3 den=2"), (dict(thresholds=((1, 0),)), "threshold 0: den=0"),
            (dict(thresholds=((65536, 65537),)), "threshold 0: den=65537"), (dict(thresholds=((-1, -2),)), "threshold 0: den=-2"),
            (dict(min_size=-3), "min_size=-3"), (dict(B=-1), "B=-1"), (dict(B=0, min_size=0), "min_size=0"),
            (dict(B=0, thresholds=((2, 5),)), "num=2 den=5"), (dict(stats=None), "null"), (dict(iou=None), "null"), (dict(iou=p + 4), "8-byte aligned"),
            (dict(thresholds=None, T=2), "null"), (dict(ws=None), "workspace"), (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes, {need} needed"),
            # a buffer of ccdm_lesions' own size is too small for the sizes behind it
            (dict(ws_bytes=lesions_workspace_formula(1, 3, 2, 8, 8, 2)), f"{need} needed"), (dict(ws=p + 2), "4-byte aligned")):
        rc = call(**change)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "lesion_match")
    assert not buf.any()
    assert call(B=0) == 0 and call(B=0, ws=None, ws_bytes=0) == 0 and not buf.any()      # B = 0: nothing launched, nothing written


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def kernel(samples: torch.Tensor, raters: torch.Tensor, K: int, connectivity: int = 8, thresholds=THRESHOLDS, min_size: int = 1):
    """ccdm_lesions, then ccdm_lesion_match on its workspace, on uint8 device stacks [B,S,H,W] / [B,L,H,W] (as they lie in memory) ->
    the dict of per-cell arrays; the outputs and the workspace start from a non-zero fill: the call overwrites"""
    lib = hip.load()
    assert samples.is_cuda and raters.is_cuda and samples.dtype == raters.dtype == torch.uint8
    assert samples.is_contiguous() and raters.is_contiguous()
    B, S, H, W = samples.shape
    L = raters.shape[1]
    Cn, T = len(scored_classes(K)), len(thresholds)
    th = np.ascontiguousarray(thresholds, dtype=np.int32)
    any_overlap = np.array([[0, 1]], dtype=np.int32)
    need = int(lib.ccdm_lesion_match_workspace_bytes(B, S, L, H, W, K))
    assert need == workspace_formula(B, S, L, H, W, K)
    ws = torch.full((need // 4,), -7, dtype=torch.int32, device="cuda")
    hits = torch.zeros((B, S, L, Cn, 4), dtype=torch.int32, device="cuda")
    stats = torch.full((B, S, L, Cn, 2 + T), 77, dtype=torch.int32, device="cuda")
    iou = torch.full((B, S, L, Cn, T), -5, dtype=torch.int64, device="cuda")
    hip.check(lib.ccdm_lesions(samples.data_ptr(), raters.data_ptr(), B, S, L, H, W, K, connectivity, any_overlap.ctypes.data, 1, hits.data_ptr(),
                               ws.data_ptr(), need, None), "lesions")
    hip.check(lib.ccdm_lesion_match(B, S, L, H, W, K, th.ctypes.data, T, min_size, stats.data_ptr(), iou.data_ptr(), ws.data_ptr(), need, None),
              "lesion_match")
    torch.cuda.synchronize()
    st = stats.cpu().numpy().astype(np.int64)
    return {"n_a": st[..., 0], "n_r": st[..., 1], "tp": st[..., 2:], "iou_sum": iou.cpu().numpy(), "thresholds": [[int(n), int(d)] for n, d in thresholds],
            "connectivity": connectivity, "min_size": min_size, "classes": scored_classes(K)}


def assert_stats_equal(got, want, tag=""):
    bad = {k: int((got[k] != want[k]).sum()) for k in FIELDS}
    print(f"lesion_match[{tag} {want['n_a'].shape}] max n_a={int(want['n_a'].max(initial=0))} n_r={int(want['n_r'].max(initial=0))} "
          f"tp={want['tp'].reshape(-1, want['tp'].shape[-1]).sum(axis=0).tolist()} mismatches={bad}")
    for k in FIELDS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("classes", "thresholds", "connectivity", "min_size"):
        assert got[k] == want[k], k


def check_exact(samples: np.ndarray, raters: np.ndarray, K: int, connectivity: int = 8, thresholds=THRESHOLDS, min_size: int = 1, want=None, tag=""):
    got = kernel(torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda(), K, connectivity, thresholds, min_size)
    want = stats_restatement(samples, raters, K, connectivity, thresholds, min_size) if want is None else want
    assert_stats_equal(got, want, tag)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("B,S,L,H,W,K", BLOB_SHAPES)
def test_random_blobs(B, S, L, H, W, K, connectivity):
    samples, raters = blob_case(B, S, L, H, W, K)
    want = blob_case_stats((B, S, L, H, W, K), connectivity)
    assert_not_trivial(want, (B, S, L, H, W, K, connectivity))
    check_exact(samples, raters, K, connectivity, want=want, tag="blobs")


@pytest.mark.gpu
def test_exact_threshold_is_not_a_match():
    a, r = np.zeros((1, 2, 8, 8), dtype=np.uint8), np.zeros((1, 2, 8, 8), dtype=np.uint8)
    a[0, 0, 2, 2:4] = 1                                       # 2 pixels over 1: inter 1, union 2, IoU exactly 1/2
    r[0, 0, 2, 2] = 1
    a[0, 1, 5, 1:4] = 1                                       # 3 pixels over 2 of them: IoU 2/3
    r[0, 1, 5, 1:3] = 1
    got, want = check_exact(a, r, 2, 8, tag="exact threshold")
    assert got["tp"][0, 0, 0, 0].tolist() == [0, 0] and got["iou_sum"][0, 0, 0, 0].tolist() == [0, 0] and got["n_a"][0, 0, 0, 0] == got["n_r"][0, 0, 0, 0] == 1
    assert got["tp"][0, 1, 1, 0].tolist() == [1, 0] and got["iou_sum"][0, 1, 1, 0].tolist() == [2 * ONE // 3, 0]
    assert not got["tp"][0, 0, 1].any() and not got["tp"][0, 1, 0].any()           # the crossed cells do not overlap at all
    # the same rational written otherwise, IoU 2/3 against 2/3 itself, and eight thresholds in one call
    eight = ((1, 2), (2, 4), (32768, 65536), (2, 3), (3, 4), (65535, 65536), (21845, 32768), (5, 8))
    got8, _ = check_exact(a, r, 2, 8, eight, tag="eight thresholds")
    assert got8["tp"][0, 1, 1, 0].tolist() == [1, 1, 1, 0, 0, 0, 1, 1] and got8["tp"][0, 0, 0, 0].tolist() == [0] * 8


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
def test_identical_maps_match_every_lesion(connectivity):
    samples, _ = blob_case(2, 3, 2, 32, 48, 3)
    got, _ = check_exact(samples, samples[:, :2], 3, connectivity, tag="identical")
    for i in range(2):
        n = got["n_a"][:, i, i]
        assert int(n.sum()) > 4
        np.testing.assert_array_equal(got["n_r"][:, i, i], n)
        np.testing.assert_array_equal(got["tp"][:, i, i], np.stack([n, n], axis=-1))
        np.testing.assert_array_equal(got["iou_sum"][:, i, i], np.stack([n, n], axis=-1) * ONE)


@pytest.mark.gpu
def test_table_at_its_bound():
    """128x128, connectivity 4: the checkerboard against itself has 8192 pairs, all matched; the full map against it 8192 pairs,
    none matched; 16384 slots hold either at a load of exactly 1/2"""
    board = checkerboard(128, 128)
    samples = np.stack([board, np.ones_like(board)])[None]
    got, _ = check_exact(samples, board[None, None], 2, 4, tag="checkerboard")
    assert got["n_a"][0, :, 0, 0].tolist() == [8192, 1] and got["n_r"][0, :, 0, 0].tolist() == [8192, 8192]
    assert got["tp"][0, 0, 0, 0].tolist() == [8192, 8192] and got["iou_sum"][0, 0, 0, 0].tolist() == [8192 * ONE, 8192 * ONE]
    assert got["tp"][0, 1, 0, 0].tolist() == [0, 0] and got["iou_sum"][0, 1, 0, 0].tolist() == [0, 0]


@pytest.mark.gpu
def test_every_lesion_crosses_every_lesion():
    """row stripes against column stripes at 64x64: 32 x 32 pairs of one pixel each, every lesion with 32 partners below any threshold"""
    rows, cols = np.zeros((64, 64), dtype=np.uint8), np.zeros((64, 64), dtype=np.uint8)
    rows[0::2] = 1
    cols[:, 0::2] = 1
    got, _ = check_exact(rows[None, None], np.stack([cols, rows])[None], 2, 8, tag="stripes")
    assert got["n_a"][0, 0, :, 0].tolist() == [32, 32] and got["n_r"][0, 0, :, 0].tolist() == [32, 32]
    assert got["tp"][0, 0, 0, 0].tolist() == [0, 0] and got["tp"][0, 0, 1, 0].tolist() == [32, 32]
    # 16 x 32 = 512 pairs in a table of 1024 slots, 16 x 33 = 528 in one of 2048
    for W in (64, 66):
        rows, cols = np.zeros((32, W), dtype=np.uint8), np.zeros((32, W), dtype=np.uint8)
        rows[0::2] = 1
        cols[:, 0::2] = 1
        thick = cols.copy()
        thick[:, 1::4] = 1                                    # columns of 3: fewer lesions, each over two of `cols`
        check_exact(np.stack([rows, cols])[None], np.stack([cols, thick])[None], 2, 4, tag=f"stripes 32x{W}")


@pytest.mark.gpu
@pytest.mark.parametrize("min_size", [1, 2, 3, 4, 6])
def test_min_size_drops_lesions_from_both_sides(min_size):
    m = sized_lesions()
    part = m.copy()
    part[8, 11:13] = 0                                        # 3 of the 5 pixels: IoU 3/5
    got, _ = check_exact(m[None, None], np.stack([m, part])[None], 2, 8, min_size=min_size, tag=f"min_size {min_size}")
    kept = sum(s >= min_size for s in (1, 2, 5))
    assert got["n_a"][0, 0, :, 0].tolist() == [kept, kept] and got["n_r"][0, 0, 0, 0] == kept
    assert got["tp"][0, 0, 0, 0].tolist() == [kept, kept] and got["iou_sum"][0, 0, 0, 0].tolist() == [kept * ONE, kept * ONE]
    kept_part = sum(s >= min_size for s in (1, 2, 3))
    assert got["n_r"][0, 0, 1, 0] == kept_part
    # the 5-pixel lesion loses its 3-pixel partner at min_size 4 although it is kept itself
    assert got["tp"][0, 0, 1, 0].tolist() == [kept_part, sum(s >= min_size for s in (1, 2))]


@pytest.mark.gpu
def test_one_class_scores_class_zero():
    m = np.full((1, 2, 13, 14), 9, dtype=np.uint8)
    m[0, 0, 2:5, 2:6] = 0; m[0, 0, 7, 1:13] = 0; m[0, 0, 12, 13] = 0
    m[0, 1, 2:5, 3:7] = 0; m[0, 1, 7, 1:12] = 0; m[0, 1, 10, 5] = 0
    got, _ = check_exact(m, m[:, ::-1].copy(), 1, 8, tag="K = 1")
    assert got["classes"] == [0] and got["n_a"][0, :, 0, 0].tolist() == [3, 3] and got["tp"][0, 0, 0, 0].tolist() == [2, 1]


@pytest.mark.gpu
def test_unaligned_base_pointers():
    """the stacks start one byte off a dword: the labelling's byte path; the planes the match reads are the same"""
    B, S, L, H, W, K = 2, 3, 2, 32, 48, 3
    samples, raters = blob_case(B, S, L, H, W, K)
    want = blob_case_stats((B, S, L, H, W, K), 8)
    s_buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    r_buf = torch.zeros(raters.size + 1, dtype=torch.uint8, device="cuda")
    s_dev, r_dev = s_buf[1:].view(B, S, H, W), r_buf[1:].view(B, L, H, W)
    s_dev.copy_(torch.from_numpy(np.array(samples))); r_dev.copy_(torch.from_numpy(np.array(raters)))
    assert s_dev.data_ptr() % 4 == 1 and r_dev.data_ptr() % 4 == 1
    assert_stats_equal(kernel(s_dev, r_dev, K), want, "unaligned")


@pytest.mark.gpu
def test_repeated_call_is_identical_and_no_image_is_no_work():
    lib = hip.load()
    samples, raters = blob_case(2, 3, 2, 32, 48, 3)
    s_dev, r_dev = torch.from_numpy(np.array(samples)).cuda(), torch.from_numpy(np.array(raters)).cuda()
    first, second = kernel(s_dev, r_dev, 3, 4), kernel(s_dev, r_dev, 3, 4)
    for k in FIELDS:
        assert first[k].tobytes() == second[k].tobytes(), k
    assert_stats_equal(first, blob_case_stats((2, 3, 2, 32, 48, 3), 4), "repeat")
    # B = 0 leaves prefilled outputs as they are
    st = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    iou = torch.full((8,), 9, dtype=torch.int64, device="cuda")
    ws = torch.full((8,), 9, dtype=torch.int32, device="cuda")
    th = np.array(THRESHOLDS, dtype=np.int32)
    assert lib.ccdm_lesion_match(0, 3, 2, 32, 48, 3, th.ctypes.data, 2, 1, st.data_ptr(), iou.data_ptr(), ws.data_ptr(), 32, None) == 0
    torch.cuda.synchronize()
    assert bool((st == 9).all()) and bool((iou == 9).all()) and bool((ws == 9).all())


@pytest.mark.gpu
def test_refusals_leave_device_outputs_untouched():
    lib = hip.load()
    B, S, L, H, W, K = 1, 3, 2, 8, 8, 2
    need = workspace_formula(B, S, L, H, W, K)
    st = torch.full((B * S * L * 4,), 9, dtype=torch.int32, device="cuda")
    iou = torch.full((B * S * L * 2,), 9, dtype=torch.int64, device="cuda")
    ws = torch.full((2 * need // 4,), 9, dtype=torch.int32, device="cuda")
    for change, what in REFUSALS:
        args = dict(H=H, W=W, thresholds=THRESHOLDS, min_size=1)
        args.update(change)
        th = np.ascontiguousarray(args["thresholds"], dtype=np.int32)
        rc = lib.ccdm_lesion_match(B, S, L, args["H"], args["W"], K, th.ctypes.data, len(th), args["min_size"], st.data_ptr(), iou.data_ptr(),
                                   ws.data_ptr(), 2 * need, None)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
    torch.cuda.synchronize()
    assert bool((st == 9).all()) and bool((iou == 9).all()) and bool((ws == 9).all())
    s64 = torch.zeros((1, 3, 8, 8), dtype=torch.int64, device="cuda")
    for kw, what in ((dict(thresholds=((2, 5),)), "num=2 den=5"), (dict(min_size=0), "min_size=0"), (dict(connectivity=6), "connectivity=6")):
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            M.lesion_match_stats(s64, s64[:, :2], 2, **kw)
    with pytest.raises(ValueError, match="expected"):
        M.lesion_match_stats(s64[:, :, :4], s64[:, :2], 2)


@pytest.mark.gpu
def test_lesion_match_stats_takes_index_maps():
    samples, raters = blob_case(2, 3, 2, 32, 48, 3)
    s64, r64 = torch.from_numpy(samples.astype(np.int64)).cuda(), torch.from_numpy(raters.astype(np.int64)).cuda()
    got = M.lesion_match_stats(s64, r64, 3)
    assert got["n_a"].shape == (2, 3, 2, 2) and got["iou_sum"].shape == (2, 3, 2, 2, 2)
    assert_stats_equal(got, blob_case_stats((2, 3, 2, 32, 48, 3), 8), "int64 maps")
    sliced = M.lesion_match_stats(s64[:, :2], r64, 3, connectivity=4, thresholds=((2, 3),), min_size=2)      # the evaluator's pred_idx[:, :s]
    assert_stats_equal(sliced, stats_restatement(samples[:, :2], raters, 3, 4, ((2, 3),), 2), "sliced")
    both = M.concat_lesion_match_stats([got, got])
    assert both["n_a"].shape == (4, 3, 2, 2) and both["tp"].shape == (4, 3, 2, 2, 2) and both["classes"] == [1, 2] and both["connectivity"] == 8


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_lesion_matching_end_to_end(tmp_path):
    from ccdm_stochastic_segmentation_amd import evaluation as E
    K, H, W, evaluations, batch = 2, 32, 48, [2, 3], 2
    S = max(evaluations)
    samples, raters = blob_case(3, S, 4, H, W, K)                # 3 images in batches of 2: the last batch holds one
    one_hot = lambda idx: torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), K).movedim(-1, -3).float()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return samples.shape[0]

        def __getitem__(self, b):
            return torch.zeros((1, H, W)), one_hot(raters[b]), np.array([0.25] * 4)

    def fake():
        class Fake:
            step_T_sample = "majority"
            calls = 0

            def __call__(self, x, image, **kw):
                first = self.calls * batch
                p = one_hot(samples[first:first + x.shape[0] // S]).reshape(x.shape[0], K, H, W)
                self.calls += 1
                return {"diffusion_out": p.to(x.device)}
        return Fake()

    params = {"dataset_file": "datasets.lidc", "batch_size": batch, "evaluations": evaluations, "output_path": str(tmp_path / "out")}
    plain = E.eval_lidc_uncertainty(dict(params), dataset=DS(), device="cuda:0", model=fake())
    assert set(plain) == {"evaluations", "GED", "diversity_samples", "diversity_experts", "HM_IoU", "IoU", "mIoU", "Dice", "nonzero", "images",
                          "world_size"}                       # today's keys, exactly
    assert not (tmp_path / "out").exists()
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"lesion_matching": True}}, dataset=DS(), device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"lesion_matching"}
    for key, value in plain.items():                          # everything the evaluator returns today is untouched
        assert res[key] == value, key
    assert len(res["lesion_matching"]) == len(evaluations)
    for s, got in zip(evaluations, res["lesion_matching"]):
        want = M.lesion_match_scores_from_stats(stats_restatement(samples[:, :s], raters, K, 8, ((1, 2), (3, 4))))
        print(f"lesion_matching[{s}] got={got}")
        assert got["samples"] == s and got["images"] == 3 and got["raters"] == 4 and got["thresholds"] == [[1, 2], [3, 4]] and got["min_size"] == 1
        assert got["cells_matched"][0] > got["cells_matched"][1] > 0 and got["fp_total"][0] > 0 and got["fn_total"][0] > 0
        assert got == want                                    # ratios of integers, reduced in the same order
    other = E.eval_lidc_uncertainty({**params, "evaluation": {"lesion_matching": True, "lesion_match_ious": [0.6], "lesion_min_size": 3,
                                                              "lesion_connectivity": 4}, "output_path": None},
                                    dataset=DS(), device="cuda:0", model=fake())["lesion_matching"]
    want4 = M.lesion_match_scores_from_stats(stats_restatement(samples[:, :2], raters, K, 4, ((3, 5),), 3))
    assert other[0]["thresholds"] == [[3, 5]] and other[0]["connectivity"] == 4 and other[0]["min_size"] == 3 and other[0] == want4
    for bad, key in (({"lesion_match_ious": [0.4]}, "lesion_match_ious"), ({"lesion_match_ious": [1]}, "lesion_match_ious"),
                     ({"lesion_min_size": 0}, "lesion_min_size"), ({"lesion_connectivity": 6}, "lesion_connectivity")):
        with pytest.raises(ValueError, match=key):
            E.eval_lidc_uncertainty({**params, "evaluation": {"lesion_matching": True, **bad}, "output_path": None}, dataset=DS(), device="cuda:0",
                                    model=fake())
    with open(tmp_path / "out" / "lidc_lesion_matching.json") as f:
        assert json.load(f) == res["lesion_matching"] == json.loads(json.dumps(res["lesion_matching"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_lesion_matching.json"]
