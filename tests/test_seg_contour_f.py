"""The boundary F-score of a segmentation prediction (Csurka et al.'s BF score, MATLAB's bfscore, the DAVIS F-measure): the
contour-match kernel (ccdm_contourf), the tolerance rule (resolve_contour_tolerances), contour_f_from_counts, SegmentationContourF
and the `evaluation.contour_f` keys of eval_segmentation.  Nothing in the reference computes these.  Every count is an integer, so
the GPU tests ask for equality with a numpy restatement of the definition in include/ccdm_hip.h (contours by shifted comparisons,
matches by OR-ing the other map's contour pixels over every offset of the disc); the CPU tests hold that restatement against
scipy's exact Euclidean distance transform (the squared integer distance to the nearest contour pixel it returns) and against
hand-made cases."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import segmentation as SEG
from tests.test_seg_boundary import SIZES, _pred_map, masked_maps
from tests.test_seg_eval import SHAPES, Recorder, _dirichlet, _k20_model, _labels, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTOUR_SYMBOLS = {"ccdm_contourf", "ccdm_contourf_workspace_bytes"}


# ------------------------------------------------------------------------------------------------ numpy restatement
def contour_codes(x: np.ndarray, C: int) -> np.ndarray:
    """x [H,W] int64, 255 = none -> the class of every contour pixel, -1 elsewhere: a pixel of class c is a contour pixel when one of
    its 4-neighbours inside the image holds a counted class other than c"""
    H, W = x.shape
    pad = np.full((H + 2, W + 2), 255, dtype=np.int64)
    pad[1:-1, 1:-1] = x
    cont = np.zeros((H, W), dtype=bool)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        n = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        cont |= (x < C) & (n < C) & (n != x)
    return np.where(cont, x, -1)


def matched_by_offsets(a: np.ndarray, b: np.ndarray, theta: int) -> np.ndarray:
    """a, b: contour_codes of the two maps -> the contour pixels of a that have a contour pixel of their class in b at an offset
    with dx^2 + dy^2 <= theta^2 (b padded with "no contour")"""
    H, W = a.shape
    pad = np.full((H + 2 * theta, W + 2 * theta), -1, dtype=np.int64)
    pad[theta:theta + H, theta:theta + W] = b
    hit = np.zeros((H, W), dtype=bool)
    for dy in range(-theta, theta + 1):
        for dx in range(-theta, theta + 1):
            if dx * dx + dy * dy <= theta * theta:
                hit |= pad[theta + dy:theta + dy + H, theta + dx:theta + dx + W] == a
    return hit & (a >= 0)


def matched_by_edt(a: np.ndarray, b: np.ndarray, theta: int) -> np.ndarray:
    """the same by scipy, per class: the exact Euclidean distance transform's nearest contour pixel of the class in b, and the
    squared integer distance to it against theta^2"""
    import scipy.ndimage as ndi          # scipy is a requirement of the package
    H, W = a.shape
    yy, xx = np.mgrid[0:H, 0:W]
    hit = np.zeros((H, W), dtype=bool)
    for c in np.unique(a[a >= 0]):
        other = b == c
        if not other.any():
            continue
        iy, ix = ndi.distance_transform_edt(~other, return_distances=False, return_indices=True)
        hit |= (a == c) & ((iy - yy) ** 2 + (ix - xx) ** 2 <= theta * theta)
    return hit


def restatement(pred, labels, K: int, theta: int, matched=matched_by_offsets) -> np.ndarray:
    """pred, labels [B,H,W] integer arrays -> counts int64 [B,C,4] = {nP, mP, nG, mG} by the definition"""
    C = K - 1
    g, p = masked_maps(np.asarray(pred), np.asarray(labels), C)
    out = np.zeros((g.shape[0], C, 4), dtype=np.int64)
    for b in range(g.shape[0]):
        cg, cp = contour_codes(g[b], C), contour_codes(p[b], C)
        mp, mg = matched(cp, cg, theta), matched(cg, cp, theta)
        out[b, :, 0] = np.bincount(cp[cp >= 0], minlength=C)
        out[b, :, 1] = np.bincount(cp[mp], minlength=C)
        out[b, :, 2] = np.bincount(cg[cg >= 0], minlength=C)
        out[b, :, 3] = np.bincount(cg[mg], minlength=C)
    return out


def kernel(pred: torch.Tensor, labels: torch.Tensor, K: int, theta: int, counts=None) -> torch.Tensor:
    """one ccdm_contourf call on uint8 maps [B,H,W] -> counts [B,C,4] on the host; counts: a device table to add to"""
    lib = hip.load()
    pred, labels = pred.to(torch.uint8).cuda().contiguous(), SEG._labels_u8(labels, "cuda")
    B, H, W = (int(v) for v in labels.shape)
    counts = torch.zeros((B, K - 1, 4), dtype=torch.int64, device="cuda") if counts is None else counts
    need = int(lib.ccdm_contourf_workspace_bytes(B, H, W))
    assert need == 2 * B * H * W
    ws = torch.empty(max(need, 2), dtype=torch.uint8, device="cuda")
    hip.check(lib.ccdm_contourf(pred.data_ptr(), labels.data_ptr(), B, H, W, K, theta, counts.data_ptr(), ws.data_ptr(), need, None), "contourf")
    torch.cuda.synchronize()
    return counts.cpu()


def check_exact(pred, labels, K, theta, tag="", matched=matched_by_offsets) -> np.ndarray:
    got = kernel(pred, labels, K, theta).numpy()
    want = restatement(pred.numpy(), labels.numpy(), K, theta, matched)
    print(f"contourf[{tag} K{K} theta{theta}] nP,mP,nG,mG={want.sum((0, 1)).tolist()} diff={int(np.abs(got - want).sum())}")
    np.testing.assert_array_equal(got, want)
    return want


def some_matched_some_not(counts: np.ndarray) -> bool:
    """0 < mP < nP and 0 < mG < nG in at least one class (summed over the images)"""
    t = counts.sum(0)
    return bool(((0 < t[:, 1]) & (t[:, 1] < t[:, 0])).any() and ((0 < t[:, 3]) & (t[:, 3] < t[:, 2])).any())


def _pred_partly_off(rng, labels: torch.Tensor, C: int) -> torch.Tensor:
    """a _pred_map-style class map [B,H,W] in [0, C): the labels' blocks a few pixels off with a little salt noise (contours that
    match and salt contours that do not), and class 0 alone over the right half (true contours there that nothing matches)"""
    lab = labels.numpy()
    p = np.roll(lab, (3, 2), axis=(1, 2))
    p = np.where(p < C, p, rng.integers(0, C, p.shape))
    noise = rng.random(p.shape) < 0.01
    p[noise] = rng.integers(0, C, p.shape)[noise]
    p[:, :, p.shape[2] // 2:] = 0
    return torch.from_numpy(p.astype(np.uint8))


def _two_dots(H, W, p, q, K=3):
    """class 0 everywhere, one pixel of class 1 at p in the prediction and at q in the labels: class 1 has one contour pixel per map"""
    lab = torch.zeros((1, H, W), dtype=torch.int64)
    pred = torch.zeros((1, H, W), dtype=torch.uint8)
    pred[0, p[0], p[1]] = 1
    lab[0, q[0], q[1]] = 1
    return pred, lab


# ------------------------------------------------------------------------------------------------ CPU
def test_contour_f_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_contourf[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == CONTOUR_SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_contourf")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
    assert len(hip.SIGNATURES["ccdm_contourf"][1]) == 11 and len(hip.SIGNATURES["ccdm_contourf_workspace_bytes"][1]) == 3
    assert "ccdm_contourf.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_contourf.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in CONTOUR_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    # host-side size query: one byte per pixel and map, within the 4 bytes per pixel the design allows
    assert lib.ccdm_contourf_workspace_bytes(4, 1024, 2048) == 2 * 4 * 1024 * 2048
    assert lib.ccdm_contourf_workspace_bytes(1, 5, 7) == 70
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.ccdm_contourf_workspace_bytes(*shape) == 0


def test_tolerance_rule():
    assert SEG.CONTOUR_MAX_TOLERANCE == 32 and list(SEG.CONTOUR_DEFAULT_TOLERANCES) == ["ratio:0.0075"]
    assert SEG.resolve_contour_tolerances(["ratio:0.0075"], (1024, 2048)) == [17]
    assert SEG.resolve_contour_tolerances(list(SEG.CONTOUR_DEFAULT_TOLERANCES), (1024, 2048)) == [17]
    assert SEG.resolve_contour_tolerances(["ratio:0.0075"], (5, 5)) == [1]
    assert SEG.resolve_contour_tolerances([1, 3, 32, "ratio:0.01", "ratio:0.02"], (300, 400)) == [1, 3, 32, 5, 10]       # a mixed list
    assert SEG.resolve_contour_tolerances((2, "ratio:0.5")) == [2, 0]              # no size: the entries are checked only
    for bad in ([0], [33], [3, 3], ["ratio:0.01", "ratio:0.01"], [], ["junk"], ["ratio:-1"], "ratio:0.0075", "junk", ["ratio:abc"], [2.5],
                [True], [None], 3, None):
        with pytest.raises(ValueError):
            SEG.resolve_contour_tolerances(bad, (64, 64))
        with pytest.raises(ValueError):
            SEG.resolve_contour_tolerances(bad)
    for bad in ([0], [33]):
        with pytest.raises(ValueError, match="32"):                               # the limit is named
            SEG.resolve_contour_tolerances(bad)
    with pytest.raises(ValueError, match="32"):                                   # 0.02 * 2290 = 46 pixels
        SEG.resolve_contour_tolerances(["ratio:0.02"], (1024, 2048))
    assert SEG.resolve_contour_tolerances(["ratio:0.02"]) == [0]                   # fine until the size is known
    # the rounding is the boundary widths' own
    for ratio, size in (("ratio:0.0075", (1024, 2048)), ("ratio:0.01", (97, 211)), ("ratio:0.001", (40, 56)), ("ratio:0.0137", (300, 520))):
        assert SEG.resolve_contour_tolerances([ratio], size) == SEG.resolve_boundary_widths([ratio], size)
    for bad in ([0], [33], ["ratio:-1"], "junk"):
        with pytest.raises(ValueError):
            SEG.SegmentationContourF(20, "cuda", tolerances=bad)                  # before the device is looked at
    with pytest.raises(ValueError, match="num_classes"):
        SEG.SegmentationContourF(33, "cuda")
    with pytest.raises(hip.CcdmHipError):
        SEG.SegmentationContourF(20, "cpu")


def test_contour_f_from_counts_on_hand_made_tables():
    # two images, four classes; per cell {nP, mP, nG, mG}
    ct = np.array([
        # class 0: perfect          class 1: nothing predicted   class 2: only predicted   class 3: P 1/2, R 1/4
        [[10, 10, 12, 12],          [0, 0, 5, 0],                [7, 0, 0, 0],             [4, 2, 8, 2]],
        # class 0: P 3/4, R 1/2     class 1: absent              class 2: absent           class 3: P 1, R 1
        [[4, 3, 2, 1],              [0, 0, 0, 0],                [0, 0, 0, 0],             [100, 100, 100, 100]],
    ], dtype=np.int64)
    r = SEG.contour_f_from_counts(ct)
    f3 = 2 * 0.5 * 0.25 / 0.75                                     # = 1/3
    f0 = 2 * 0.75 * 0.5 / 1.25                                     # = 0.6
    np.testing.assert_allclose(r["bf_score"][0], (1.0 + f0) / 2, rtol=1e-15)
    assert r["bf_score"][1] == 0.0 and r["precision"][1] == 0.0 and r["recall"][1] == 0.0        # nP = 0 < nG: F = 0, and scored
    assert r["bf_score"][2] is None and r["precision"][2] is None and r["recall"][2] is None    # no scored image
    np.testing.assert_allclose(r["bf_score"][3], (f3 + 1.0) / 2, rtol=1e-15)
    np.testing.assert_allclose(r["precision"][3], 0.75, rtol=1e-15)
    np.testing.assert_allclose(r["recall"][3], 0.625, rtol=1e-15)
    np.testing.assert_allclose(r["precision"][0], (1 + 0.75) / 2, rtol=1e-15)
    np.testing.assert_allclose(r["recall"][0], (1 + 0.5) / 2, rtol=1e-15)
    assert r["images"] == [2, 1, 0, 2] and r["pred_only"] == [0, 0, 1, 0]
    np.testing.assert_allclose(r["mean_bf_score"], ((1.0 + f0) / 2 + 0.0 + (f3 + 1.0) / 2) / 3, rtol=1e-15)     # class 2 is left out
    # pooled: class 3 sums to {104, 102, 108, 102}: the large image dominates, unlike in the per-image mean
    pp, pr = 102 / 104, 102 / 108
    np.testing.assert_allclose(r["pooled"]["precision"][3], pp, rtol=1e-15)
    np.testing.assert_allclose(r["pooled"]["recall"][3], pr, rtol=1e-15)
    np.testing.assert_allclose(r["pooled"]["bf_score"][3], 2 * pp * pr / (pp + pr), rtol=1e-15)
    assert abs(r["pooled"]["bf_score"][3] - r["bf_score"][3]) > 0.25               # 0.962 against 0.667
    p0, r0 = 13 / 14, 13 / 14
    np.testing.assert_allclose(r["pooled"]["bf_score"][0], 2 * p0 * r0 / (p0 + r0), rtol=1e-15)
    assert r["pooled"]["bf_score"][1] == 0.0 and r["pooled"]["bf_score"][2] is None
    np.testing.assert_allclose(r["pooled"]["mean_bf_score"], (13 / 14 + 0.0 + 2 * pp * pr / (pp + pr)) / 3, rtol=1e-15)
    np.testing.assert_allclose(r["pooled"]["mean_precision"], (p0 + 0.0 + pp) / 3, rtol=1e-15)
    np.testing.assert_allclose(r["pooled"]["mean_recall"], (r0 + 0.0 + pr) / 3, rtol=1e-15)
    assert r["counts"] == ct.sum(0).tolist()
    assert json.loads(json.dumps(r)) == r
    # a perfect cell alone gives 1 everywhere
    one = SEG.contour_f_from_counts(np.array([[[9, 9, 9, 9]]]))
    assert one["bf_score"] == [1.0] and one["mean_bf_score"] == 1.0 and one["pooled"]["mean_bf_score"] == 1.0
    # matched on neither side: P + R = 0 gives F = 0
    assert SEG.contour_f_from_counts(np.array([[[5, 0, 6, 0]]]))["bf_score"] == [0.0]
    named = SEG.contour_f_from_counts(ct, class_names=("a", "b", "c", "d"))
    assert named["images"] == {"a": 2, "b": 1, "c": 0, "d": 2} and named["bf_score"]["c"] is None
    assert set(named["pooled"]["bf_score"]) == {"a", "b", "c", "d"} and named["mean_bf_score"] == r["mean_bf_score"]
    empty = SEG.contour_f_from_counts(np.zeros((0, 3, 4), np.int64))
    assert empty["bf_score"] == [None] * 3 and empty["mean_bf_score"] is None and empty["pooled"]["mean_bf_score"] is None
    for bad in (np.zeros((2, 3)), np.zeros((2, 3, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            SEG.contour_f_from_counts(bad)
    with pytest.raises(ValueError):
        SEG.contour_f_from_counts(ct, class_names=("a",))


@pytest.mark.parametrize("theta", [1, 2, 5, 11])
def test_restatement_equals_scipy_distance_transform(theta):
    """the yardstick itself: the OR over the offsets of the disc is "the nearest contour pixel of the class is within theta" by
    scipy's exact Euclidean distance transform"""
    rng = np.random.default_rng(theta)
    for H, W, K in ((97, 211, 6), (40, 56, 20), (9, 30, 4), (30, 4, 3)):
        labels = _labels(rng, 2, H, W, K - 1)                       # blocky, with ignored pixels sprinkled in
        labels[0, H // 3:H // 2, W // 4:W // 2] = 255               # and an ignored region
        pred = _pred_map(rng, labels, K - 1)
        a = restatement(pred.numpy(), labels.numpy(), K, theta)
        b = restatement(pred.numpy(), labels.numpy(), K, theta, matched_by_edt)
        np.testing.assert_array_equal(a, b)
        assert a[:, :, 0].sum() > 0 and a[:, :, 2].sum() > 0
        assert (a[:, :, 1] <= a[:, :, 0]).all() and (a[:, :, 3] <= a[:, :, 2]).all()


def test_restatement_on_hand_made_cases():
    # two one-pixel-wide vertical edges k columns apart match iff k <= theta
    H, W = 12, 40
    for theta in (1, 3, 7):
        for k in range(0, 10):
            g = np.zeros((1, H, W), dtype=np.int64)
            g[:, :, 15:] = 1
            p = np.zeros((1, H, W), dtype=np.int64)
            p[:, :, 15 + k:] = 1
            ct = restatement(p, g, 3, theta)[0]
            assert ct[:, 0].tolist() == [H, H] and ct[:, 2].tolist() == [H, H]          # columns 14 | 15 and 14 + k | 15 + k
            want = H if k <= theta else 0
            assert ct[:, 1].tolist() == [want, want] and ct[:, 3].tolist() == [want, want], (theta, k)
    # at theta = 5 the offsets (3, 4) and (5, 0) match, (4, 4) and (5, 1) do not
    for off, hit in (((3, 4), 1), ((4, 3), 1), ((5, 0), 1), ((0, 5), 1), ((-3, -4), 1), ((4, 4), 0), ((5, 1), 0), ((1, 5), 0), ((0, 6), 0)):
        pred, lab = _two_dots(30, 30, (12, 12), (12 + off[0], 12 + off[1]))
        ct = restatement(pred.numpy(), lab.numpy(), 3, 5)[0]
        assert ct[1].tolist() == [1, hit, 1, hit], off
        assert ct[0, 0] == 4 and ct[0, 2] == 4                      # the four neighbours of either dot are contour pixels of class 0
    # an edge along the image frame is no contour: only the class edge in the middle is
    g = np.zeros((1, 9, 9), dtype=np.int64)
    g[:, :, 5:] = 1
    codes = contour_codes(g[0], 2)
    assert (codes[:, 4] == 0).all() and (codes[:, 5] == 1).all() and (np.delete(codes, (4, 5), axis=1) == -1).all()
    one = np.full((1, 9, 9), 1, dtype=np.int64)
    assert restatement(one, one, 3, 2).sum() == 0                   # one class: the frame alone makes nothing
    # an edge along an ignored region is no contour
    g = np.zeros((1, 9, 9), dtype=np.int64)
    g[:, 3:6, 3:6] = 255
    assert (contour_codes(masked_maps(g[0], g[0], 2)[0], 2) == -1).all()
    assert restatement(np.zeros_like(g), g, 3, 2).sum() == 0
    g[:, 3:6, 3:6] = 2                                              # label K - 1 = 2 is ignored as well
    assert restatement(np.zeros_like(g), g, 3, 2).sum() == 0
    # a prediction of class K - 1 is "none": it makes no contour in P', and hides nothing of G'
    g = np.zeros((1, 9, 9), dtype=np.int64)
    p = np.zeros((1, 9, 9), dtype=np.int64)
    p[:, 3:6, 3:6] = 2
    assert restatement(p, g, 3, 2).sum() == 0
    p[:, 3:6, 3:6] = 1                                              # a counted class there does
    ct = restatement(p, g, 3, 2)[0]
    assert ct[:, 0].tolist() == [12, 8] and ct[:, 2].tolist() == [0, 0] and ct[:, 1].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ GPU: kernel, exact
@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1, 3, 8])
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
def test_kernel_equals_restatement(size, K, theta):
    """the prediction is _pred_partly_off rather than test_seg_boundary._pred_map: that one is 3 and 2 pixels off with salt on 4 % of
    the pixels, which at theta = 8 leaves no true contour pixel without a match.  K = 2 has one counted class, and a contour
    needs two: there the counts are all zero by the definition, and that is what is asserted"""
    tag, H, W = size
    rng = np.random.default_rng(K * 1000 + H + theta)
    labels = _labels(rng, 2, H, W, K - 1)
    ct = check_exact(_pred_partly_off(rng, labels, K - 1), labels, K, theta, tag)
    if K == 2:          # one counted class: no pixel has a neighbour of another counted class, so the definition leaves no contour
        assert ct.sum() == 0
    else:               # some contour pixels match and some do not: the test cannot pass on empty work
        assert some_matched_some_not(ct)


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [17, 32])
@pytest.mark.parametrize("size", [SIZES[1], SIZES[2]], ids=[SIZES[1][0], SIZES[2][0]])
def test_wide_tolerances_across_tiles_and_halos(size, theta):
    """a disc that reaches into the neighbouring tiles on every side: 128 x 192 and 97 x 211 have 2 x 3 and 2 x 4 tiles.  Blocks of
    40 pixels with a prediction 21 pixels off leave contours without a match at 17"""
    tag, H, W = size
    rng = np.random.default_rng(theta + H)
    K = 20
    coarse = rng.integers(0, K - 1, (2, H // 40 + 1, W // 40 + 1))
    lab = coarse[:, np.arange(H) // 40][:, :, np.arange(W) // 40].astype(np.int64)
    lab[rng.random(lab.shape) < 0.01] = 255
    shifted = np.roll(lab, (21, -20), axis=(1, 2))
    pred = np.where(shifted < K - 1, shifted, 0)
    salt = rng.random(lab.shape) < 0.002
    pred[salt] = rng.integers(0, K - 1, lab.shape)[salt]
    ct = check_exact(torch.from_numpy(pred.astype(np.uint8)), torch.from_numpy(lab), K, theta, tag)
    assert some_matched_some_not(ct)


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [5, 30])
@pytest.mark.parametrize("direction", ["horizontal", "vertical", "diagonal_3_4", "diagonal_4_3"])
def test_the_only_match_lies_exactly_theta_away_across_a_boundary(direction, theta):
    """one contour pixel of class 1 per map, theta apart (a match) and theta + 1 apart or one step off the circle (none), with the
    two pixels on either side of the 64-column boundary between row chunks and of the 64-row boundary between tiles"""
    dy, dx = {"horizontal": (0, theta), "vertical": (theta, 0), "diagonal_3_4": (3 * theta // 5, 4 * theta // 5),
              "diagonal_4_3": (4 * theta // 5, 3 * theta // 5)}[direction]
    assert dy * dy + dx * dx == theta * theta
    H = W = 160
    for p, sign in (((63, 63), 1), ((64, 64), -1), ((63, 64), 1), ((64, 63), -1)):
        q = (p[0] + sign * dy, p[1] + sign * dx)
        for pred, lab in (_two_dots(H, W, p, q), _two_dots(H, W, q, p)):
            ct = check_exact(pred, lab, 3, theta, f"{direction} {p}->{q}")
            assert ct[0, 1].tolist() == [1, 1, 1, 1]
            ct = check_exact(pred, lab, 3, theta - 1, f"{direction} {p}->{q}")
            assert ct[0, 1].tolist() == [1, 0, 1, 0]
        far = (q[0] + sign * (dy > 0), q[1] + sign * (dy == 0))     # one step further out
        ct = check_exact(*_two_dots(H, W, p, far), 3, theta, f"{direction} {p}->{far}")
        assert ct[0, 1].tolist() == [1, 0, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1, 8, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 200), (200, 5), (7, 7), (16, 17), (3, 300), (130, 2), (33, 67)])
def test_small_narrow_and_odd_shapes(H, W, theta):
    """images smaller than the disc, than a tile and than a row chunk, W not divisible by 4, one row and one column past a tile"""
    rng = np.random.default_rng(H * 1000 + W)
    labels = _labels(rng, 3, H, W, 4)
    ct = check_exact(_pred_map(rng, labels, 4), labels, 5, theta, f"{H}x{W}")
    if max(H, W) >= 16:         # more than one block of labels: both maps have contours
        assert ct[:, :, 0].sum() > 0 and ct[:, :, 2].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1, 8, 32])
def test_degenerate_images(theta):
    H, W, K = 150, 200, 20
    pred = torch.full((2, H, W), 7, dtype=torch.uint8)
    assert int(kernel(pred, torch.full((2, H, W), 7, dtype=torch.int64), K, theta).sum()) == 0          # one class
    rng = np.random.default_rng(theta)
    busy = _labels(rng, 1, H, W, K - 1)
    busy_pred = _pred_map(rng, busy, K - 1)
    for ignore in (19, 255, 200):                                   # all ignored, whatever the prediction
        assert int(kernel(busy_pred.expand(2, H, W), torch.full((2, H, W), ignore, dtype=torch.int64), K, theta).sum()) == 0
    # one ignored pixel in a one-class image is the rim of an ignored region: still nothing
    hole = torch.full((1, H, W), 7, dtype=torch.int64)
    hole[:, 75, 100] = 255
    assert int(kernel(pred[:1], hole, K, theta).sum()) == 0
    # one image of a batch is degenerate, the others are not
    labels = torch.cat([busy, torch.full((1, H, W), 7, dtype=torch.int64), busy, torch.full((1, H, W), 255, dtype=torch.int64)])
    preds = torch.cat([busy_pred, pred[:1], busy_pred, busy_pred])
    ct = check_exact(preds, labels, K, theta, "mixed batch")
    assert ct[0].sum() > 0 and ct[1].sum() == 0 and (ct[2] == ct[0]).all() and ct[3].sum() == 0


@pytest.mark.gpu
def test_per_image_layout_accumulation_and_bit_identical_calls():
    rng = np.random.default_rng(5)
    K, theta = 20, 3
    labels = _labels(rng, 3, 97, 211, K - 1)
    pred = _pred_map(rng, labels, K - 1)
    one = kernel(pred, labels, K, theta)
    again = kernel(pred, labels, K, theta)
    assert torch.equal(one, again) and int(one.sum()) > 0           # two identical calls are bit-identical
    singles = torch.cat([kernel(pred[i:i + 1], labels[i:i + 1], K, theta) for i in range(3)])
    assert torch.equal(one, singles)                                # a batch is its images stacked
    assert all(int(one[i].sum()) > 0 for i in range(3)) and not torch.equal(one[0], one[1])
    table = torch.zeros((3, K - 1, 4), dtype=torch.int64, device="cuda")
    kernel(pred, labels, K, theta, table)
    twice = kernel(pred, labels, K, theta, table)                   # a table that was not cleared is added to
    assert torch.equal(twice, 2 * one)
    # the class over three updates, ratio and pixel tolerances side by side
    s1, s3 = (SEG.SegmentationContourF(K, "cuda", tolerances=[3, "ratio:0.02", 1]) for _ in range(2))
    s1.update(pred.cuda(), labels.cuda())
    for s in (slice(0, 1), slice(1, 3)):
        s3.update(pred[s].cuda(), labels[s].cuda())
    s3.update(pred[:0].cuda(), labels[:0].cuda())                   # an empty batch changes nothing
    assert torch.equal(s1.counts, s3.counts) and tuple(s1.counts.shape) == (3, 3, K - 1, 4)
    assert torch.equal(s1.counts[0], one)
    assert s3.pixels == [[3], [5], [1]]                             # round(0.02 * sqrt(97^2 + 211^2)) = round(4.64) = 5
    np.testing.assert_array_equal(s1.counts[1].numpy(), restatement(pred.numpy(), labels.numpy(), K, 5))
    r = s3.result()
    assert r["tolerances"] == [{"entry": 3, "pixels": [3]}, {"entry": "ratio:0.02", "pixels": [5]}, {"entry": 1, "pixels": [1]}]
    assert set(r["by_tolerance"]) == {"3", "ratio:0.02", "1"} and r["by_tolerance"]["3"] == SEG.contour_f_from_counts(one.numpy())
    assert json.loads(json.dumps(r)) == r
    empty = SEG.SegmentationContourF(K, "cuda")
    assert tuple(empty.counts.shape) == (1, 0, K - 1, 4) and empty.result()["by_tolerance"]["ratio:0.0075"]["mean_bf_score"] is None


@pytest.mark.gpu
def test_cityscapes_size():
    """1024 x 2048 at bfscore's tolerance there, 17 pixels: more tiles than a block has, so the blocks walk several; six classes in
    blocks of 150 pixels, an ignored strip and a few ignored pixels; the prediction is 9 and 12 pixels off (15 along the diagonal),
    salted, so most of the contour matches and the salt away from the edges does not; the right quarter is predicted as one class"""
    rng = np.random.default_rng(17)
    H, W, K = 1024, 2048, 20
    coarse = rng.integers(0, 6, (1, H // 150 + 1, W // 150 + 1))
    lab = coarse[:, np.arange(H) // 150][:, :, np.arange(W) // 150].astype(np.int64)
    lab[:, H - 70:] = 255
    lab[rng.random((1, H, W)) < 0.00002] = 19
    shifted = np.roll(lab, (9, 12), axis=(1, 2))
    pred = np.where(shifted < K - 1, shifted, 1)
    salt = rng.random((1, H, W)) < 0.0005
    pred[salt] = rng.integers(0, 6, (1, H, W))[salt]
    pred[:, :, 3 * W // 4:] = 0                                     # and true contours that nothing matches
    assert SEG.resolve_contour_tolerances(list(SEG.CONTOUR_DEFAULT_TOLERANCES), (H, W)) == [17]
    ct = check_exact(torch.from_numpy(pred.astype(np.uint8)), torch.from_numpy(lab), K, 17, "1024x2048", matched_by_edt)
    assert some_matched_some_not(ct) and ct[:, 6:].sum() == 0


@pytest.mark.gpu
def test_bad_arguments_and_empty_batch():
    lib = hip.load()
    z = torch.zeros(4096, dtype=torch.int64, device="cuda")
    args = lambda B, K, theta, ws_bytes: (z.data_ptr(), z.data_ptr(), B, 8, 8, K, theta, z.data_ptr(), z.data_ptr() + 16384, ws_bytes, None)
    for K, theta, what in ((33, 3, "K=33"), (1, 3, "K=1"), (20, 0, "theta=0"), (20, 33, "theta=33"), (20, -1, "theta=-1")):
        for B in (0, 1):
            assert lib.ccdm_contourf(*args(B, K, theta, 1024)) < 0 and what in hip.last_error()
    assert lib.ccdm_contourf(*args(1, 20, 3, 2 * 64 - 1)) < 0 and "workspace" in hip.last_error()
    assert lib.ccdm_contourf(z.data_ptr(), z.data_ptr(), 1, 0, 8, 20, 3, z.data_ptr(), z.data_ptr() + 16384, 1024, None) < 0
    assert lib.ccdm_contourf(z.data_ptr(), z.data_ptr(), -1, 8, 8, 20, 3, z.data_ptr(), z.data_ptr() + 16384, 1024, None) < 0
    assert lib.ccdm_contourf(None, z.data_ptr(), 1, 8, 8, 20, 3, z.data_ptr(), z.data_ptr() + 16384, 1024, None) < 0 and "null" in hip.last_error()
    assert lib.ccdm_contourf(*args(0, 20, 3, 0)) == 0                           # B = 0: nothing launched, nothing written
    torch.cuda.synchronize()
    assert int(z.sum()) == 0


# ------------------------------------------------------------------------------------------------ GPU: the class the others count
@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 20])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=[s[0] for s in SHAPES[:4]])
def test_update_counts_the_class_the_export_writes(shape, K):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(K + h)
    nhwc = _dirichlet(rng, 2, h, w, K)
    labels = _labels(rng, 2, H, W, K - 1)
    pred = nhwc.permute(0, 3, 1, 2).cuda()                          # fp32 probabilities at the low resolution
    sc = SEG.SegmentationContourF(K, "cuda", tolerances=[2, 8])
    sc.update(pred, labels.cuda())
    tables = dict(id_table=list(range(K)), color_table=np.zeros((K, 3), np.uint8))
    train_id = SEG.export_predictions(pred, (H, W), outputs=("train_id",), **tables)["train_id"]
    for i, theta in enumerate((2, 8)):
        assert torch.equal(sc.counts[i], kernel(train_id, labels, K, theta))
    np.testing.assert_array_equal(sc.counts[0].numpy(), restatement(train_id.cpu().numpy(), labels.numpy(), K, 2))
    assert int(sc.counts[0].sum()) > 0
    # a uint8 class map, its int64 one-hot and its float one-hot give the same counts
    cls = torch.from_numpy(rng.integers(0, K, (2, h, w)))
    got = []
    for form in (cls.to(torch.uint8), F.one_hot(cls, K).permute(0, 3, 1, 2).contiguous(), F.one_hot(cls, K).float().permute(0, 3, 1, 2)):
        s = SEG.SegmentationContourF(K, "cuda", tolerances=[2, 8])
        s.update(form.cuda(), labels.cuda())
        got.append(s.counts)
    assert all(torch.equal(got[0], g) for g in got[1:]) and int(got[0].sum()) > 0


# ------------------------------------------------------------------------------------------------ GPU: evaluator
@pytest.mark.gpu
def test_eval_segmentation_contour_f_end_to_end(tmp_path, parity_log):
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    params = _params("original", 2, "confidence")
    params["output_path"] = str(tmp_path / "out")
    plain = SEG.eval_segmentation(dict(params), dataset=ds, model=Recorder(_k20_model("confidence")))
    assert "contour_f" not in plain and not os.path.exists(tmp_path / "out")
    params["evaluation"] = dict(params["evaluation"], contour_f=True)
    rec = Recorder(_k20_model("confidence"))
    res = SEG.eval_segmentation(params, dataset=ds, model=rec)
    assert set(res) == set(plain) | {"contour_f"}
    for k in plain:                                                 # the mIoU result is unchanged
        assert res[k] == plain[k], k
    ctf = res["contour_f"]
    assert ctf["tolerances"] == [{"entry": "ratio:0.0075", "pixels": [1]}]     # round(0.0075 * sqrt(48^2 + 80^2)) = round(0.70)
    assert json.load(open(tmp_path / "out" / "contour_f.json")) == ctf
    assert os.listdir(tmp_path / "out") == ["contour_f.json"]
    # the counts against the restatement on the recorded predictions
    tables = dict(id_table=SEG.TRAIN_ID_TO_ID, color_table=SEG.TRAIN_ID_TO_COLOR)

    def restated(recorder, theta):
        out, i0 = [], 0
        for pred in recorder.preds:
            lab = torch.stack([ds[i][2] for i in range(i0, i0 + pred.shape[0])])
            i0 += pred.shape[0]
            train_id = SEG.export_predictions(pred, (48, 80), outputs=("train_id",), **tables)["train_id"]
            out.append(restatement(train_id.cpu().numpy(), lab.numpy(), 20, theta))
        return np.concatenate(out)
    ct = restated(rec, 1)
    s = ctf["by_tolerance"]["ratio:0.0075"]
    assert ct.shape == (3, 19, 4) and s == SEG.contour_f_from_counts(ct, SEG.TRAIN_ID_NAMES)
    assert s["counts"] == ct.sum(0).tolist() and ct[:, :, 2].sum() > 0
    assert set(s["bf_score"]) == set(SEG.TRAIN_ID_NAMES) and 0 <= s["mean_bf_score"] <= 1
    parity_log("eval_segmentation[contour_f]", mean_bf_score=s["mean_bf_score"], pooled=s["pooled"]["mean_bf_score"], mIoU=res["mIoU"])
    # several tolerances, together with the boundary scores
    params["output_path"] = str(tmp_path / "both")
    params["evaluation"].update(boundary=True, contour_tolerances=[4, "ratio:0.1", 32])
    rec = Recorder(_k20_model("confidence"))
    res = SEG.eval_segmentation(params, dataset=ds, model=rec)
    assert sorted(os.listdir(tmp_path / "both")) == ["boundary.json", "contour_f.json"]
    ctf = res["contour_f"]
    assert [t["pixels"] for t in ctf["tolerances"]] == [[4], [9], [32]]        # round(0.1 * 93.3) = 9
    assert ctf["by_tolerance"]["4"] == SEG.contour_f_from_counts(restated(rec, 4), SEG.TRAIN_ID_NAMES)
    f = [ctf["by_tolerance"][k]["pooled"]["mean_recall"] for k in ("4", "ratio:0.1", "32")]
    assert f[0] <= f[1] <= f[2]                                     # a wider disc matches no less


@pytest.mark.gpu
@pytest.mark.parametrize("tolerances", [[0], [33], [3, 3], ["ratio:-1"], ["junk"], [], "ratio:0.0075", ["ratio:0.9"]])
def test_eval_segmentation_bad_contour_tolerances_raise_before_sampling(tolerances):
    params = _params("original", 1, "confidence")
    params["evaluation"].update(contour_f=True, contour_tolerances=tolerances)
    with pytest.raises(ValueError, match="contour tolerance"):
        SEG.eval_segmentation(params, dataset=SEG.SyntheticCityscapes(size=1), model=object())       # object(): no model is ever called
