"""Boundary IoU and trimap scores of a segmentation prediction: the two-pass run-length kernel (ccdm_segboundary), the width rule
(resolve_boundary_widths), boundary_from_counts, SegmentationBoundary and the `evaluation.boundary` keys of eval_segmentation.
Nothing in the reference computes these.  Every count is an integer, so the GPU tests ask for equality with a numpy restatement of
the definition in include/ccdm_hip.h (the window formulation, by box sums over an integral image); the CPU tests hold that
restatement against scipy's binary erosion (3x3 square, d iterations, zero border: the published Boundary IoU code)."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import segmentation as SEG
from tests.test_seg_eval import SHAPES, Recorder, _dirichlet, _k20_model, _labels, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY_SYMBOLS = {"ccdm_segboundary", "ccdm_segboundary_workspace_bytes"}
SIZES = [(s[0], s[3], s[4]) for s in SHAPES]          # (tag, H, W) of the scored maps: 40x56, 128x192, 97x211, 40x48, 32x280


# ------------------------------------------------------------------------------------------------ numpy restatement
def interior(mask: np.ndarray, d: int) -> np.ndarray:
    """mask [H,W] bool -> the pixels whose (2d+1) x (2d+1) window lies inside the image and inside the mask: the box sum over the
    mask padded with d zeros on every side, from an integral image, equals the window area"""
    H, W = mask.shape
    pad = np.zeros((H + 2 * d + 1, W + 2 * d + 1), dtype=np.int64)
    pad[d + 1:d + 1 + H, d + 1:d + 1 + W] = mask
    ii = pad.cumsum(0).cumsum(1)
    n = 2 * d + 1
    box = ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]
    return box == n * n


def masked_maps(pred: np.ndarray, labels: np.ndarray, C: int):
    """(G', P') as int64 with 255 for "not counted": the label where it is < C; the prediction where the label is counted"""
    g = np.where((labels >= 0) & (labels < C), labels, 255).astype(np.int64)
    p = np.where((g < C) & (pred >= 0) & (pred < C), pred, 255).astype(np.int64)
    return g, p


def restatement(pred, labels, K: int, d: int):
    """pred, labels [B,H,W] integer arrays -> (bcounts int64 [C,3], trimap int64 [C,C]) by the definition"""
    C = K - 1
    g, p = masked_maps(np.asarray(pred), np.asarray(labels), C)
    bc = np.zeros((C, 3), dtype=np.int64)
    tm = np.zeros((C, C), dtype=np.int64)
    for b in range(g.shape[0]):
        for c in range(C):
            mg, mp = g[b] == c, p[b] == c
            if not (mg.any() or mp.any()):
                continue
            bg, bp = mg & ~interior(mg, d), mp & ~interior(mp, d)
            bc[c] += (int(bg.sum()), int(bp.sum()), int((bg & bp).sum()))
            sel = bg & (p[b] < C)
            tm[c] += np.bincount(p[b][sel], minlength=C)[:C]
    return bc, tm


def _pred_map(rng, labels: torch.Tensor, C: int) -> torch.Tensor:
    """a class map [B,H,W] in [0, C) that follows the labels' blocks a few pixels off, with salt noise: bands that overlap in part"""
    lab = labels.numpy()
    p = np.roll(lab, (3, 2), axis=(1, 2))
    p = np.where(p < C, p, rng.integers(0, C, p.shape))
    noise = rng.random(p.shape) < 0.04
    p[noise] = rng.integers(0, C, p.shape)[noise]
    return torch.from_numpy(p.astype(np.uint8))


def kernel(pred: torch.Tensor, labels: torch.Tensor, K: int, d: int, bc=None, tm=None):
    """one ccdm_segboundary call on uint8 maps [B,H,W] -> (bcounts, trimap) on the host; bc / tm: device tables to add to"""
    lib = hip.load()
    pred, labels = pred.to(torch.uint8).cuda().contiguous(), SEG._labels_u8(labels, "cuda")
    B, H, W = (int(v) for v in labels.shape)
    C = K - 1
    bc = torch.zeros((C, 3), dtype=torch.int64, device="cuda") if bc is None else bc
    tm = torch.zeros((C, C), dtype=torch.int64, device="cuda") if tm is None else tm
    need = int(lib.ccdm_segboundary_workspace_bytes(B, H, W))
    assert need == 2 * B * H * W
    ws = torch.empty(max(need, 2), dtype=torch.uint8, device="cuda")
    hip.check(lib.ccdm_segboundary(pred.data_ptr(), labels.data_ptr(), B, H, W, K, d, bc.data_ptr(), tm.data_ptr(), ws.data_ptr(), need, None),
              "segboundary")
    torch.cuda.synchronize()
    return bc.cpu(), tm.cpu()


def check_exact(pred, labels, K, d, tag=""):
    bc_k, tm_k = kernel(pred, labels, K, d)
    bc_r, tm_r = restatement(pred.numpy(), labels.numpy(), K, d)
    print(f"segboundary[{tag} K{K} d{d}] bands={bc_r.sum(0).tolist()} trimap={int(tm_r.sum())} "
          f"diff={int(np.abs(bc_k.numpy() - bc_r).sum())},{int(np.abs(tm_k.numpy() - tm_r).sum())}")
    np.testing.assert_array_equal(bc_k.numpy(), bc_r)
    np.testing.assert_array_equal(tm_k.numpy(), tm_r)
    return bc_r, tm_r


# ------------------------------------------------------------------------------------------------ CPU
def test_boundary_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_segboundary[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == BOUNDARY_SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_segboundary")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
        assert not name.startswith("ccdm_seg_")
    assert len(hip.SIGNATURES["ccdm_segboundary"][1]) == 12 and len(hip.SIGNATURES["ccdm_segboundary_workspace_bytes"][1]) == 3
    assert {k for k in hip.SIGNATURES if k.startswith("ccdm_seg_")} == {"ccdm_seg_confusion", "ccdm_seg_confusion_workspace_bytes"}
    assert "ccdm_segboundary.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_segboundary.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in BOUNDARY_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    # host-side size query: one byte per pixel and map
    assert lib.ccdm_segboundary_workspace_bytes(4, 1024, 2048) == 2 * 4 * 1024 * 2048
    assert lib.ccdm_segboundary_workspace_bytes(1, 5, 7) == 70
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.ccdm_segboundary_workspace_bytes(*shape) == 0


def test_width_rule():
    assert SEG.resolve_boundary_widths(["ratio:0.02"], (1024, 2048)) == [46]
    assert SEG.resolve_boundary_widths(list(SEG.BOUNDARY_DEFAULT_WIDTHS), (1024, 2048)) == [46]
    assert SEG.resolve_boundary_widths(["ratio:0.02"], (5, 5)) == [1]
    assert SEG.resolve_boundary_widths([1, 3, 64, "ratio:0.01", "ratio:0.02"], (300, 400)) == [1, 3, 64, 5, 10]
    assert SEG.resolve_boundary_widths((2, "ratio:0.5")) == [2, 0]                # no size: the entries are checked only
    for bad in ([0], [65], ["ratio:-1"], ["ratio:0"], ["ratio:abc"], ["ratio:nan"], ["wide"], [2.5], [True], [None], [], "ratio:0.02", 3, None,
                [3, 3], ["ratio:0.02", "ratio:0.02"]):
        with pytest.raises(ValueError):
            SEG.resolve_boundary_widths(bad, (64, 64))
        with pytest.raises(ValueError):
            SEG.resolve_boundary_widths(bad)
    for bad in ([0], [65]):
        with pytest.raises(ValueError, match="64"):                              # the limit is named
            SEG.resolve_boundary_widths(bad)
    with pytest.raises(ValueError, match="64"):                                  # 0.05 * 2290 = 114 pixels
        SEG.resolve_boundary_widths(["ratio:0.05"], (1024, 2048))
    for bad in ([0], [65], ["ratio:-1"], "junk"):
        with pytest.raises(ValueError):
            SEG.SegmentationBoundary(20, "cuda", widths=bad)                     # before the device is looked at
    with pytest.raises(ValueError, match="num_classes"):
        SEG.SegmentationBoundary(33, "cuda")
    with pytest.raises(hip.CcdmHipError):
        SEG.SegmentationBoundary(20, "cpu")


def test_boundary_from_counts_on_hand_made_tables():
    # class 0: bands of 10 and 8 pixels sharing 6; class 1: only predicted (IoU 0); class 2: no band on either side; class 3: identical
    bc = np.array([[10, 8, 6], [0, 5, 0], [0, 0, 0], [7, 7, 7]], dtype=np.int64)
    tm = np.array([[6, 2, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 7]], dtype=np.int64)
    r = SEG.boundary_from_counts(bc, tm)
    assert r["boundary_iou"] == [6 / 12, 0.0, None, 1.0]
    np.testing.assert_allclose(r["mean_boundary_iou"], (0.5 + 0.0 + 1.0) / 3, rtol=1e-15)      # the empty class is left out
    np.testing.assert_array_equal(r["trimap_iou"], SEG.iou_from_confusion(tm).numpy())
    np.testing.assert_allclose(r["trimap_iou"], [6 / 10, 0.0, 0.0, 7 / 9], rtol=1e-14)
    assert r["trimap_miou"] == float(SEG.iou_from_confusion(tm).mean()) and r["trimap_pixels"] == 17
    assert r["bcounts"] == bc.tolist() and r["trimap"] == tm.tolist()
    assert json.loads(json.dumps(r)) == r
    named = SEG.boundary_from_counts(bc, tm, class_names=("a", "b", "c", "d"))
    assert named["boundary_iou"] == {"a": 0.5, "b": 0.0, "c": None, "d": 1.0} and set(named["trimap_iou"]) == {"a", "b", "c", "d"}
    empty = SEG.boundary_from_counts(np.zeros((2, 3), np.int64), np.zeros((2, 2), np.int64))
    assert empty["boundary_iou"] == [None, None] and empty["mean_boundary_iou"] is None and empty["trimap_pixels"] == 0
    for bad in ((np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros((2, 3)), np.zeros((3, 3))), (np.zeros(3), np.zeros((1, 1)))):
        with pytest.raises(ValueError):
            SEG.boundary_from_counts(*bad)
    with pytest.raises(ValueError):
        SEG.boundary_from_counts(bc, tm, class_names=("a",))


@pytest.mark.parametrize("d", [1, 2, 5, 11])
def test_restatement_equals_scipy_binary_erosion(d):
    """the yardstick itself: mask minus interior() is the mask minus its erosion by a 3x3 square, d iterations, zero border"""
    import scipy.ndimage as ndi          # scipy is a requirement of the package
    rng = np.random.default_rng(d)
    for H, W, C in ((97, 211, 5), (40, 56, 19), (9, 30, 3), (30, 4, 2)):
        lab = _labels(rng, 1, H, W, C)[0].numpy()
        for c in range(C):
            mask = lab == c
            eroded = ndi.binary_erosion(mask, structure=np.ones((3, 3)), iterations=d, border_value=0) if mask.any() else mask
            np.testing.assert_array_equal(interior(mask, d), eroded)
    # and the counts on a hand-made case: a 6 x 8 map, left half class 0, right half class 1, prediction one column off
    g = np.zeros((1, 6, 8), dtype=np.int64)
    g[:, :, 4:] = 1
    p = np.zeros((1, 6, 8), dtype=np.int64)
    p[:, :, 5:] = 1
    bc, tm = restatement(p, g, 3, 1)
    # d = 1: the interior of a 6 x 4 block is 4 x 2, of 6 x 5 it is 4 x 3, of 6 x 3 it is 4 x 1; column 3 (rows 1..4) is in the
    # target's band of class 0 and inside the prediction's block, column 5 is in the prediction's band of class 1 and inside the target's
    assert bc.tolist() == [[24 - 8, 30 - 12, 16 - 4], [24 - 8, 18 - 4, 14 - 4]]
    # the target-0 band is its whole frame, predicted 0 throughout; the target-1 band holds column 4 (6 pixels predicted 0)
    assert tm.tolist() == [[16, 0], [6, 10]]


# ------------------------------------------------------------------------------------------------ GPU: kernel, exact
@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
def test_kernel_equals_restatement(size, K, d):
    tag, H, W = size
    rng = np.random.default_rng(K * 1000 + H + d)
    labels = _labels(rng, 2, H, W, K - 1)
    bc, tm = check_exact(_pred_map(rng, labels, K - 1), labels, K, d, tag)
    assert bc[:, 0].sum() > 0 and tm.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", [17, 46, 64])
def test_wide_bands_across_tiles_and_strips(d):
    """d beyond the 16 rows a wave of the tile walk takes, the paper's width at Cityscapes size, and the widest; 300 x 520 spans
    several strips and chunks, and its blocks of 40 pixels leave interiors at d = 17 only"""
    rng = np.random.default_rng(d)
    B, H, W, K = 2, 300, 520, 20
    coarse = rng.integers(0, K - 1, (B, H // 40 + 1, W // 40 + 1))
    lab = coarse[:, np.arange(H) // 40][:, :, np.arange(W) // 40].astype(np.int64)
    lab[:, 20:200, 30:300] = 3                                     # a region with an interior at d = 64: 180 x 270
    r = rng.random((B, H, W))
    lab[r < 0.0002] = 255
    labels = torch.from_numpy(lab)
    pred = torch.from_numpy(np.where(np.roll(lab, (5, -7), axis=(1, 2)) < K - 1, np.roll(lab, (5, -7), axis=(1, 2)), 0).astype(np.uint8))
    bc, _ = check_exact(pred, labels, K, d, "300x520")
    g, _ = masked_maps(pred.numpy(), lab, K - 1)
    assert 0 < bc[3, 0] < int((g == 3).sum())                      # class 3 has band pixels and interior pixels


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 46])
def test_cityscapes_size(d):
    """3 x 1024 x 2048: more tiles than blocks, so a block of the row pass walks several; blocks of 150 pixels keep interiors at
    the paper's width, an ignored strip and a few ignored pixels make borders of their own"""
    rng = np.random.default_rng(46)
    B, H, W, K = 3, 1024, 2048, 20
    coarse = rng.integers(0, K - 1, (B, H // 150 + 1, W // 150 + 1))
    lab = coarse[:, np.arange(H) // 150][:, :, np.arange(W) // 150].astype(np.int64)
    lab[:, H - 70:] = 255
    lab[rng.random((B, H, W)) < 0.00002] = 19
    labels = torch.from_numpy(lab)
    pred = torch.from_numpy(np.where(np.roll(lab, (4, 9), axis=(1, 2)) < K - 1, np.roll(lab, (4, 9), axis=(1, 2)), 1).astype(np.uint8))
    bc, _ = check_exact(pred, labels, K, d, "1024x2048")
    assert 0 < bc[:, 0].sum() < int((lab < K - 1).sum())            # band pixels and interior pixels


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,d", [(5, 200, 8), (200, 5, 8), (7, 7, 8), (16, 17, 8), (1, 1, 1), (3, 300, 64), (130, 2, 64), (33, 67, 3),
                                   (129, 257, 5)])
def test_small_narrow_and_odd_shapes(H, W, d):
    """images narrower or shorter than 2d + 1 (every counted pixel is in its band), W not divisible by 4, one past the strip and
    the block's 256 columns"""
    rng = np.random.default_rng(H * 1000 + W)
    labels = _labels(rng, 3, H, W, 4)
    pred = _pred_map(rng, labels, 4)
    bc, tm = check_exact(pred, labels, 5, d, f"{H}x{W}")
    if H < 2 * d + 1 or W < 2 * d + 1:
        g, p = masked_maps(pred.numpy(), labels.numpy(), 4)
        assert bc[:, 0].tolist() == [int((g == c).sum()) for c in range(4)] and int(tm.sum()) == int((g < 4).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 8, 64])
def test_one_class_image_and_all_ignored_image(d):
    H, W, K = 150, 200, 20
    labels = torch.full((2, H, W), 7, dtype=torch.int64)
    pred = torch.full((2, H, W), 7, dtype=torch.uint8)
    bc, tm = check_exact(pred, labels, K, d, "one class")
    frame = H * W - max(0, H - 2 * d) * max(0, W - 2 * d)           # the whole band comes from the image border
    want = np.zeros((K - 1, 3), dtype=np.int64)
    want[7] = 2 * frame
    np.testing.assert_array_equal(bc, want)
    assert tm[7, 7] == 2 * frame and tm.sum() == 2 * frame
    for ignore in (19, 255, 200):
        bc, tm = kernel(pred, torch.full((2, H, W), ignore, dtype=torch.int64), K, d)
        assert int(bc.sum()) == 0 and int(tm.sum()) == 0
    # one ignored pixel in the middle makes a border in both maps alike
    labels[:, 75, 100] = 255
    bc, _ = check_exact(pred, labels, K, d, "one class, one hole")
    assert bc[7, 0] == bc[7, 1] == bc[7, 2] and bc[7, 0] > 2 * frame - 2 * (d >= 64)


@pytest.mark.gpu
def test_updates_accumulate_and_identical_calls_are_bit_identical():
    rng = np.random.default_rng(5)
    K, d = 20, 3
    labels = _labels(rng, 4, 97, 211, K - 1)
    pred = _pred_map(rng, labels, K - 1)
    one = kernel(pred, labels, K, d)
    again = kernel(pred, labels, K, d)
    assert torch.equal(one[0], again[0]) and torch.equal(one[1], again[1])
    bc = torch.zeros((K - 1, 3), dtype=torch.int64, device="cuda")
    tm = torch.zeros((K - 1, K - 1), dtype=torch.int64, device="cuda")
    for s in (slice(0, 1), slice(1, 3), slice(3, 4)):               # B = 1, 2, 1
        three = kernel(pred[s], labels[s], K, d, bc, tm)
    assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1])
    # the class over three updates, ratio and pixel widths side by side
    sb1, sb3 = SEG.SegmentationBoundary(K, "cuda", widths=[3, "ratio:0.02", 1]), SEG.SegmentationBoundary(K, "cuda", widths=[3, "ratio:0.02", 1])
    sb1.update(pred.cuda(), labels.cuda())
    for s in (slice(0, 1), slice(1, 3), slice(3, 4)):
        sb3.update(pred[s].cuda(), labels[s].cuda())
    sb3.update(pred[:0].cuda(), labels[:0].cuda())                  # an empty batch changes nothing
    assert torch.equal(sb1.bcounts, sb3.bcounts) and torch.equal(sb1.trimap, sb3.trimap)
    assert torch.equal(sb1.bcounts[0], one[0]) and torch.equal(sb1.trimap[0], one[1])
    assert sb3.pixels == [[3], [5], [1]]                            # round(0.02 * sqrt(97^2 + 211^2)) = round(4.64) = 5
    np.testing.assert_array_equal(sb1.bcounts[1].numpy(), restatement(pred.numpy(), labels.numpy(), K, 5)[0])
    r = sb3.result()
    assert r["widths"] == [{"entry": 3, "pixels": [3]}, {"entry": "ratio:0.02", "pixels": [5]}, {"entry": 1, "pixels": [1]}]
    assert set(r["by_width"]) == {"3", "ratio:0.02", "1"} and r["by_width"]["3"]["bcounts"] == one[0].tolist()
    assert json.loads(json.dumps(r)) == r


@pytest.mark.gpu
def test_bad_arguments_and_empty_batch():
    lib = hip.load()
    z = torch.zeros(4096, dtype=torch.int64, device="cuda")
    args = lambda B, K, d, ws_bytes: (z.data_ptr(), z.data_ptr(), B, 8, 8, K, d, z.data_ptr(), z.data_ptr(), z.data_ptr() + 16384, ws_bytes, None)
    for K, d, what in ((33, 3, "K=33"), (1, 3, "K=1"), (20, 0, "d=0"), (20, 65, "d=65")):
        for B in (0, 1):
            assert lib.ccdm_segboundary(*args(B, K, d, 1024)) < 0 and what in hip.last_error()
    assert lib.ccdm_segboundary(*args(1, 20, 3, 2 * 64 - 1)) < 0 and "workspace" in hip.last_error()
    assert lib.ccdm_segboundary(*args(0, 20, 3, 0)) == 0                        # B = 0: nothing launched, nothing written
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
    sb = SEG.SegmentationBoundary(K, "cuda", widths=[2, 8])
    sb.update(pred, labels.cuda())
    tables = dict(id_table=list(range(K)), color_table=np.zeros((K, 3), np.uint8))
    train_id = SEG.export_predictions(pred, (H, W), outputs=("train_id",), **tables)["train_id"]
    for i, d in enumerate((2, 8)):
        bc, tm = kernel(train_id, labels, K, d)
        assert torch.equal(sb.bcounts[i], bc) and torch.equal(sb.trimap[i], tm)
    np.testing.assert_array_equal(sb.bcounts[0].numpy(), restatement(train_id.cpu().numpy(), labels.numpy(), K, 2)[0])
    # a uint8 class map, its int64 one-hot and its float one-hot give the same counts
    cls = torch.from_numpy(rng.integers(0, K, (2, h, w)))
    got = []
    for form in (cls.to(torch.uint8), F.one_hot(cls, K).permute(0, 3, 1, 2).contiguous(), F.one_hot(cls, K).float().permute(0, 3, 1, 2)):
        s = SEG.SegmentationBoundary(K, "cuda", widths=[2, 8])
        s.update(form.cuda(), labels.cuda())
        got.append((s.bcounts, s.trimap))
    assert all(torch.equal(got[0][0], g[0]) and torch.equal(got[0][1], g[1]) for g in got[1:]) and int(got[0][0].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
def test_trimap_of_a_band_wider_than_the_image_is_the_confusion_matrix(K):
    rng = np.random.default_rng(K)
    h, w, H, W = 12, 20, 40, 56                                     # d = 64 >= max(H, W): every counted pixel is in its band
    pred = _dirichlet(rng, 2, h, w, K).permute(0, 3, 1, 2).cuda()
    labels = _labels(rng, 2, H, W, K - 1).cuda()
    sb = SEG.SegmentationBoundary(K, "cuda", widths=[64, 56])
    sb.update(pred, labels)
    conf = SEG.SegmentationConfusion(K, "cuda")
    conf.update(pred, labels)
    assert torch.equal(sb.trimap[0], conf.confusion) and torch.equal(sb.trimap[1], conf.confusion)
    assert torch.equal(sb.bcounts[0][:, 0], conf.confusion.sum(1)) and torch.equal(sb.bcounts[0][:, 1], conf.confusion.sum(0))
    assert torch.equal(sb.bcounts[0][:, 2], conf.confusion.diag())
    assert sb.result()["by_width"]["64"]["trimap_miou"] == conf.miou()


# ------------------------------------------------------------------------------------------------ GPU: evaluator
@pytest.mark.gpu
def test_eval_segmentation_boundary_end_to_end(tmp_path, parity_log):
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    params = _params("original", 2, "confidence")
    params["output_path"] = str(tmp_path / "out")
    plain = SEG.eval_segmentation(dict(params), dataset=ds, model=Recorder(_k20_model("confidence")))
    assert "boundary" not in plain and not os.path.exists(tmp_path / "out")
    params["evaluation"] = dict(params["evaluation"], boundary=True)
    rec = Recorder(_k20_model("confidence"))
    res = SEG.eval_segmentation(params, dataset=ds, model=rec)
    assert set(res) == set(plain) | {"boundary"}
    for k in plain:
        assert res[k] == plain[k], k
    bnd = res["boundary"]
    assert bnd["widths"] == [{"entry": "ratio:0.02", "pixels": [2]}]          # round(0.02 * sqrt(48^2 + 80^2)) = round(1.87)
    assert json.load(open(tmp_path / "out" / "boundary.json")) == bnd
    # the counts against the restatement on the recorded predictions
    bc, tm, i0 = np.zeros((19, 3), np.int64), np.zeros((19, 19), np.int64), 0
    tables = dict(id_table=SEG.TRAIN_ID_TO_ID, color_table=SEG.TRAIN_ID_TO_COLOR)
    for pred in rec.preds:
        lab = torch.stack([ds[i][2] for i in range(i0, i0 + pred.shape[0])])
        i0 += pred.shape[0]
        train_id = SEG.export_predictions(pred, (48, 80), outputs=("train_id",), **tables)["train_id"]
        b, t = restatement(train_id.cpu().numpy(), lab.numpy(), 20, 2)
        bc += b
        tm += t
    s = bnd["by_width"]["ratio:0.02"]
    assert s["bcounts"] == bc.tolist() and s["trimap"] == tm.tolist() and s["trimap_pixels"] == int(tm.sum()) > 0
    assert set(s["boundary_iou"]) == set(SEG.TRAIN_ID_NAMES) and 0 <= s["mean_boundary_iou"] <= 1 and 0 <= s["trimap_miou"] <= 1
    assert s == SEG.boundary_from_counts(bc, tm, SEG.TRAIN_ID_NAMES)
    parity_log("eval_segmentation[boundary]", mean_boundary_iou=s["mean_boundary_iou"], trimap_miou=s["trimap_miou"], mIoU=res["mIoU"])
    # several widths at the dataloader resolution
    params = _params("dataloader", 1, "majority")
    params["output_path"] = str(tmp_path / "widths")
    params["evaluation"].update(boundary=True, boundary_widths=[1, "ratio:0.1", 64])
    res = SEG.eval_segmentation(params, dataset=ds, model=Recorder(_k20_model("majority")))
    bnd = res["boundary"]
    assert [w["pixels"] for w in bnd["widths"]] == [[1], [5], [64]]           # round(0.1 * sqrt(2) * 32) = round(4.53)
    assert bnd["by_width"]["64"]["trimap"] == res["confusion"]               # wider than the 32 x 32 image: every counted pixel
    assert bnd["by_width"]["1"]["trimap_pixels"] <= bnd["by_width"]["ratio:0.1"]["trimap_pixels"] <= bnd["by_width"]["64"]["trimap_pixels"]


@pytest.mark.gpu
@pytest.mark.parametrize("widths", [[0], [65], ["ratio:-1"], ["junk"], [], "ratio:0.02", ["ratio:0.9"]])
def test_eval_segmentation_bad_boundary_widths_raise_before_sampling(widths):
    params = _params("original", 1, "confidence")
    params["evaluation"].update(boundary=True, boundary_widths=widths)
    with pytest.raises(ValueError, match="boundary width"):
        SEG.eval_segmentation(params, dataset=SEG.SyntheticCityscapes(size=1), model=object())       # object(): no model is ever called
