"""Calibration scores of a segmentation prediction: the fused upsample-and-bin kernel (ccdm_segcalib), calibration_from_counts,
SegmentationCalibration and the `evaluation.calibration` key of eval_segmentation.  Nothing in the reference computes these, so
the GPU tests compare against a float64 restatement of the definition in include/ccdm_hip.h (F.interpolate in float64, the
renormalised probabilities, bins, NLL and Brier sums), on the inputs of tests/test_seg_eval.py; the class binned is held against
the confusion kernel exactly (both go through the device helpers of ccdm_seg_common.h)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import segmentation as SEG
from tests.test_seg_eval import NEAR, SHAPES, SOFT_RTOL, Recorder, _dirichlet, _k20_model, _labels, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB_SYMBOLS = {"ccdm_segcalib", "ccdm_segcalib_workspace_bytes"}
EDGE = 1e-5          # float64 distance of the confidence to an interior bin edge below which the fp32 kernel may pick the other bin
RTOL = 1e-14


# ------------------------------------------------------------------------------------------------ float64 restatement
def ref64(pred_bkhw: torch.Tensor, labels: torch.Tensor, M: int):
    """The definition in float64 -> dict(bins int64 [C,M,2], conf_sum, nll, brier, qt (sums), near (pixels), counted (pixels))."""
    K = pred_bkhw.shape[1]
    C = K - 1
    H, W = labels.shape[1:]
    p = pred_bkhw.double()
    up = F.interpolate(p, (H, W), mode="bilinear", align_corners=False) if tuple(p.shape[2:]) != (H, W) else p
    up = up[:, :C]
    pred = up.argmax(1)
    s = up.sum(1, keepdim=True)
    q = torch.where(s > 0, up / s.clamp_min(1e-300), torch.full_like(up, 1.0 / C))
    lab = labels.long()
    counted = (lab >= 0) & (lab < C)
    t = torch.where(counted, lab, torch.zeros_like(lab))
    conf = q.gather(1, pred[:, None])[:, 0]
    qt = q.gather(1, t[:, None])[:, 0]
    b = (conf * M).floor().long().clamp(max=M - 1)
    near = torch.zeros_like(counted)
    if C >= 2:
        top2 = up.topk(2, dim=1).values
        k = (conf * M).round()
        near = (top2[:, 0] - top2[:, 1] < NEAR) | (((conf - k / M).abs() < EDGE) & (k > 0) & (k < M))
    m = counted.reshape(-1)
    cell = (pred * M + b).reshape(-1)[m]
    right = (pred == lab).reshape(-1)[m]
    bins = torch.stack([torch.bincount(cell, minlength=C * M), torch.bincount(cell[right], minlength=C * M)], dim=1).reshape(C, M, 2)
    onehot = F.one_hot(t, C).permute(0, 3, 1, 2).double()
    brier = ((q - onehot) ** 2).sum(1)
    nll = -qt.clamp_min(1e-12).log()
    return dict(bins=bins, conf_sum=float(conf[counted].sum()), nll=float(nll[counted].sum()), brier=float(brier[counted].sum()),
                qt=float(qt[counted].sum()), near=int((near & counted).sum()), counted=int(counted.sum()),
                min_qt=float(qt[counted].min()) if counted.any() else 1.0)


def kernel(pred, labels, K, M):
    """one SegmentationCalibration.update -> (bins int64 [C,M,2], conf_sum float64 [C,M], sums float64 [3])"""
    sc = SEG.SegmentationCalibration(K, "cuda", bins=M)
    sc.update(pred, labels)
    return sc.bins_count, sc.conf_sum.clone(), sc.sums.clone()


# ------------------------------------------------------------------------------------------------ CPU
def test_calibration_from_counts_perfectly_calibrated():
    # C = 2, M = 4: class 0 in bin [0.5, 0.75): 8 pixels, 5 right, mean confidence 5/8; class 1 in the top bin: 10, 9 right, 9/10
    bins = np.zeros((2, 4, 2), np.int64)
    conf = np.zeros((2, 4))
    bins[0, 2], conf[0, 2] = (8, 5), 5.0
    bins[1, 3], conf[1, 3] = (10, 9), 9.0
    r = SEG.calibration_from_counts(bins, conf, [18 * 0.25, 18 * 0.5, 18 * 0.75])
    assert r["pixels"] == 18 and r["bins"] == 4
    assert r["ece"] == 0.0 and r["mce"] == 0.0 and r["ece_per_class"] == [0.0, 0.0]
    np.testing.assert_allclose([r["accuracy"], r["mean_confidence"]], [14 / 18, 14 / 18], rtol=RTOL)
    np.testing.assert_allclose([r["nll"], r["brier"], r["mean_true_class_probability"]], [0.25, 0.5, 0.75], rtol=RTOL)
    assert r["reliability"]["count"] == [0, 0, 8, 10]
    assert r["reliability"]["accuracy"][:2] == [None, None] and r["reliability"]["confidence"][:2] == [None, None]
    np.testing.assert_allclose(r["reliability"]["accuracy"][2:], [5 / 8, 9 / 10], rtol=RTOL)
    np.testing.assert_allclose(r["reliability"]["confidence"][2:], [5 / 8, 9 / 10], rtol=RTOL)
    # right = [0,0,5,9], wrong = [0,0,3,1]: 5 * (0 + 3/2) + 9 * (3 + 1/2) = 39 of 14 * 4 pairs
    np.testing.assert_allclose(r["auroc_error_detection"], 39 / 56, rtol=RTOL)
    assert json.loads(json.dumps(r)) == r


def test_calibration_from_counts_overconfident_empty_bin_and_unpredicted_class():
    # C = 3, M = 5: class 0 in the top bin, 10 pixels, 6 right, mean confidence 0.95 (over-confident by 0.35);
    # class 1 in bin [0.2, 0.4), 10 pixels, 3 right, mean confidence 0.3 (calibrated); class 2 never predicted; bins 0, 2, 3 empty
    bins = np.zeros((3, 5, 2), np.int64)
    conf = np.zeros((3, 5))
    bins[0, 4], conf[0, 4] = (10, 6), 9.5
    bins[1, 1], conf[1, 1] = (10, 3), 3.0
    r = SEG.calibration_from_counts(bins, conf, [14.0, 8.0, 10.0], class_names=("a", "b", "c"))
    np.testing.assert_allclose(r["ece"], 0.5 * 0.35, rtol=RTOL)
    np.testing.assert_allclose(r["mce"], 0.35, rtol=RTOL)
    np.testing.assert_allclose([r["accuracy"], r["mean_confidence"], r["nll"], r["brier"], r["mean_true_class_probability"]],
                               [9 / 20, 12.5 / 20, 0.7, 0.4, 0.5], rtol=RTOL)
    assert r["reliability"]["count"] == [0, 10, 0, 0, 10]
    assert [a is None for a in r["reliability"]["accuracy"]] == [True, False, True, True, False]
    np.testing.assert_allclose([r["reliability"]["accuracy"][1], r["reliability"]["accuracy"][4]], [0.3, 0.6], rtol=RTOL)
    np.testing.assert_allclose([r["reliability"]["confidence"][1], r["reliability"]["confidence"][4]], [0.3, 0.95], rtol=RTOL)
    assert set(r["ece_per_class"]) == {"a", "b", "c"} and r["ece_per_class"]["c"] is None and r["ece_per_class"]["b"] == 0.0
    np.testing.assert_allclose(r["ece_per_class"]["a"], 0.35, rtol=RTOL)
    # right = [0,3,0,0,6], wrong = [0,7,0,0,4]: 3 * 7/2 + 6 * (7 + 4/2) = 64.5 of 9 * 11 pairs
    np.testing.assert_allclose(r["auroc_error_detection"], 64.5 / 99, rtol=RTOL)
    # two bins inside one class: class 0 has 4 pixels at (acc 1/4, conf 1/2) and 12 at (acc 1, conf 3/4): 4/16 * 1/4 + 12/16 * 1/4
    bins = np.zeros((2, 4, 2), np.int64)
    conf = np.zeros((2, 4))
    bins[0, 2], conf[0, 2] = (4, 1), 2.0
    bins[0, 3], conf[0, 3] = (12, 12), 9.0
    r = SEG.calibration_from_counts(bins, conf, [0.0, 0.0, 0.0])
    np.testing.assert_allclose(r["ece_per_class"][0], 0.25, rtol=RTOL)
    assert r["ece_per_class"][1] is None


def test_calibration_from_counts_auroc_one_half_and_none():
    def one(right, wrong):
        bins = np.zeros((1, len(right), 2), np.int64)
        bins[0, :, 0] = np.add(right, wrong)
        bins[0, :, 1] = right
        return SEG.calibration_from_counts(bins, bins[:, :, 0] * 0.5, [0.0, 0.0, 0.0])["auroc_error_detection"]
    assert one([0, 5], [4, 0]) == 1.0                   # every wrong pixel below every right one
    assert one([5, 0], [0, 4]) == 0.0
    assert one([0, 5], [0, 5]) == 0.5                   # one bin: every pair ties
    assert one([0, 5], [0, 0]) is None and one([0, 0], [3, 0]) is None
    empty = SEG.calibration_from_counts(np.zeros((2, 3, 2), np.int64), np.zeros((2, 3)), np.zeros(3))
    assert empty["pixels"] == 0 and empty["ece"] is None and empty["auroc_error_detection"] is None and empty["ece_per_class"] == [None, None]
    with pytest.raises(ValueError):
        SEG.calibration_from_counts(np.zeros((2, 3, 2)), np.zeros((2, 4)), np.zeros(3))


def test_calib_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_segcalib[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == CALIB_SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_segcalib")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
        assert not name.startswith("ccdm_seg_")
    assert len(hip.SIGNATURES["ccdm_segcalib"][1]) == 17 and len(hip.SIGNATURES["ccdm_segcalib_workspace_bytes"][1]) == 5
    assert "ccdm_segcalib.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_segcalib.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in CALIB_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    # host-side size query: C * M fixed-point sums and at most 1024 slab rows of three fp64 sums (the C4 shape has 8192 tiles)
    assert lib.ccdm_segcalib_workspace_bytes(16, 1024, 2048, 20, 15) == (19 * 15 + 1024 * 3) * 8
    assert lib.ccdm_segcalib_workspace_bytes(1, 64, 64, 5, 10) == (4 * 10 + 3) * 8
    for K, M in ((33, 15), (1, 15), (20, 1), (20, 65)):
        assert lib.ccdm_segcalib_workspace_bytes(1, 64, 64, K, M) == 0


def test_calibration_rejects_bad_bins_and_classes_before_the_device():
    for bins in (0, 1, 65, -3):
        with pytest.raises(ValueError, match="bins"):
            SEG.SegmentationCalibration(20, "cuda", bins=bins)
    for K in (0, 1, 33):
        with pytest.raises(ValueError, match="num_classes"):
            SEG.SegmentationCalibration(K, "cuda")
    with pytest.raises(hip.CcdmHipError):
        SEG.SegmentationCalibration(20, "cpu")


# ------------------------------------------------------------------------------------------------ GPU: kernel against float64
@pytest.mark.gpu
@pytest.mark.parametrize("M", [10, 15])
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_vs_float64_dirichlet(shape, K, M, parity_log):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(K * 1000 + h)
    B = 2
    nhwc = _dirichlet(rng, B, h, w, K)
    labels = _labels(rng, B, H, W, K - 1)
    pred = nhwc.permute(0, 3, 1, 2)                                 # BCHW view of channels-last memory
    bins_k, conf_k, sums_k = kernel(pred.cuda(), labels.cuda(), K, M)
    r = ref64(pred, labels, M)
    n, n_near = r["counted"], r["near"]
    diff_n = int((bins_k[..., 0] - r["bins"][..., 0]).abs().sum())
    diff_c = int((bins_k[..., 1] - r["bins"][..., 1]).abs().sum())
    got = {"conf_sum": float(conf_k.sum()), "nll": float(sums_k[0]), "brier": float(sums_k[1]), "qt": float(sums_k[2])}
    rel = {k: abs(got[k] - r[k]) / abs(r[k]) if r[k] else abs(got[k]) for k in got}
    parity_log(f"segcalib[{tag}_K{K}_M{M}]", near=n_near, pixels=n, count_diff=diff_n, correct_diff=diff_c, min_qt=r["min_qt"],
               **{f"{k}_rel": v for k, v in rel.items()})
    print(f"segcalib[{tag}_K{K}_M{M}] near={n_near} pixels={n} count_diff={diff_n} correct_diff={diff_c} rel={rel}")
    assert int(bins_k[..., 0].sum()) == n
    if K == 2:                      # one scored class: confidence exactly 1 on both sides, bin M - 1
        assert torch.equal(bins_k, r["bins"]) and int(bins_k[0, M - 1, 0]) == n and float(conf_k[0, M - 1]) == float(n)
    assert diff_n <= 2 * n_near and diff_c <= 2 * n_near, (tag, diff_n, diff_c, n_near)
    assert n_near <= max(4, 0.002 * n), (tag, n_near, n)
    for k, v in rel.items():
        assert v <= SOFT_RTOL, (tag, k, got[k], r[k], v)


# ------------------------------------------------------------------------------------------------ GPU: exactness
def _case(K, shape=SHAPES[2], seed=11, B=2):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(seed + K)
    return _dirichlet(rng, B, h, w, K), _labels(rng, B, H, W, K - 1).cuda()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[:3], ids=[s[0] for s in SHAPES[:3]])
def test_two_identical_calls_are_bit_identical(shape):
    nhwc, labels = _case(20, shape)
    pred = nhwc.permute(0, 3, 1, 2).cuda()
    assert _same(kernel(pred, labels, 20, 15), kernel(pred, labels, 20, 15))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=[s[0] for s in SHAPES[:4]])
def test_class_map_bitwise_equals_float_onehot(shape, K):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(K + 7)
    cls = torch.from_numpy(rng.integers(0, K, (2, h, w)))
    labels = _labels(rng, 2, H, W, K - 1).cuda()
    onehot_f = F.one_hot(cls, K).float().cuda().permute(0, 3, 1, 2)          # channels-last fp32 one-hot
    onehot_i = F.one_hot(cls, K).permute(0, 3, 1, 2).contiguous().cuda()       # int64 BCHW one-hot ("majority" diffusion_out)
    want = kernel(onehot_f, labels, K, 15)
    assert _same(want, kernel(cls.to(torch.uint8).cuda(), labels, K, 15))
    assert _same(want, kernel(onehot_i, labels, K, 15))


@pytest.mark.gpu
@pytest.mark.parametrize("K,pad", [(20, 1), (5, 3), (32, 2), (8, 4)])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=[s[0] for s in SHAPES[:3]])
def test_float4_path_equals_scalar_path(shape, K, pad):
    """pixel stride K against a padded stride: one of the two is a multiple of 4 (float4 loads), or both / neither at (8, 4)"""
    nhwc, labels = _case(K, shape)
    B, h, w, _ = nhwc.shape
    padded = torch.full((B, h, w, K + pad), 7.0)
    padded[..., :K] = nhwc
    padded = padded.cuda()[..., :K].permute(0, 3, 1, 2)                         # read in place with pixel stride K + pad
    assert SEG.prediction_form(padded, K, "cuda")[1] == K + pad
    assert _same(kernel(nhwc.permute(0, 3, 1, 2).cuda(), labels, K, 15), kernel(padded, labels, K, 15))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_class_binned_is_the_class_the_confusion_kernel_counts(shape, K):
    nhwc, labels = _case(K, shape)
    pred = nhwc.permute(0, 3, 1, 2).cuda()
    bins, _, _ = kernel(pred, labels, K, 15)
    conf = SEG.SegmentationConfusion(K, "cuda")
    conf.update(pred, labels)
    hard = conf.confusion                                                      # rows = target, columns = argmax class
    assert torch.equal(bins[:, :, 0].sum(1), hard.sum(0))
    assert torch.equal(bins[:, :, 1].sum(1), hard.diag())


@pytest.mark.gpu
def test_two_updates_accumulate_bins_and_add_sums():
    nhwc, labels = _case(20, SHAPES[1], B=4)
    pred = nhwc.permute(0, 3, 1, 2).cuda()
    a, b = kernel(pred[:1], labels[:1], 20, 15), kernel(pred[1:], labels[1:], 20, 15)
    both = SEG.SegmentationCalibration(20, "cuda", bins=15)
    both.update(pred[:1], labels[:1])
    both.update(pred[1:], labels[1:])
    assert torch.equal(both.bins_count, a[0] + b[0])
    assert torch.equal(both.conf_sum, a[1] + b[1]) and torch.equal(both.sums, a[2] + b[2])
    one = kernel(pred, labels, 20, 15)
    assert torch.equal(one[0], both.bins_count) and torch.equal(one[1], both.conf_sum)     # integer and fixed-point sums: exact
    torch.testing.assert_close(one[2], both.sums, rtol=1e-12, atol=0)
    both.update(pred[:0], labels[:0])                                          # an empty batch changes nothing
    assert torch.equal(one[0], both.bins_count) and torch.equal(one[1], both.conf_sum)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 64])
@pytest.mark.parametrize("K", [5, 32])
def test_fewest_and_most_bins(K, M):
    nhwc, labels = _case(K, SHAPES[2])
    pred = nhwc.permute(0, 3, 1, 2)
    bins, conf_sum, sums = kernel(pred.cuda(), labels, K, M)
    r = ref64(pred, labels.cpu(), 15)
    fine = kernel(pred.cuda(), labels, K, 15)
    assert bins.shape == (K - 1, M, 2) and int(bins[..., 0].sum()) == r["counted"]
    # the binning does not touch the class or the sums: per class the counts and the confidence sum are those of 15 bins
    assert torch.equal(bins.sum(1), fine[0].sum(1))
    assert torch.equal(sums, fine[2])
    assert torch.equal(conf_sum.sum(1), fine[1].sum(1))                        # multiples of 2^-28: exact in any grouping
    assert _same((bins, conf_sum, sums), kernel(pred.cuda(), labels, K, M))
    lib = hip.load()
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    for bad_K, bad_M, what in ((K, 1, "M=1"), (K, 65, "M=65"), (33, 15, "K=33")):
        rc = lib.ccdm_segcalib(z.data_ptr(), 64, None, z.data_ptr(), 0, 4, 4, 4, 4, bad_K, bad_M, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                               None, 0, None)
        assert rc < 0 and what in hip.last_error()
    assert lib.ccdm_segcalib(z.data_ptr(), 64, None, z.data_ptr(), 0, 4, 4, 4, 4, K, M, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0,
                             None) == 0 and int(z.sum()) == 0                  # B = 0: nothing launched, nothing written


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 20])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=[s[0] for s in SHAPES[:2]])
def test_all_mass_on_the_ignore_channel(shape, K):
    tag, h, w, H, W = shape
    C, M, B = K - 1, 15, 2
    rng = np.random.default_rng(K)
    p = torch.zeros((B, h, w, K))
    p[..., C] = 1.0
    labels = _labels(rng, B, H, W, C)
    bins, conf_sum, sums = kernel(p.permute(0, 3, 1, 2).cuda(), labels.cuda(), K, M)
    n, n0 = int((labels < C).sum()), int((labels == 0).sum())
    u = np.float32(1.0) / np.float32(C)                                         # the kernel's fp32 1/C
    b = min(int(u * np.float32(M)), M - 1)
    want = torch.zeros((C, M, 2), dtype=torch.int64)
    want[0, b] = torch.tensor([n, n0])
    assert torch.equal(bins, want)                                             # class 0, confidence 1/C
    assert float(conf_sum[0, b]) == n * float(u) and float(conf_sum.sum()) == n * float(u)
    uf = float(u)
    # q_c = 1/C for every c: C - 1 classes miss by 1/C, the target's by 1/C - 1 (fp32 sums in the kernel)
    np.testing.assert_allclose(sums.numpy(), [n * -math.log(uf), n * ((C - 1) * uf ** 2 + (uf - 1) ** 2), n * uf], rtol=1e-6)
    # mixed with ordinary rows: against the float64 restatement
    nhwc = _dirichlet(rng, B, h, w, K)
    nhwc[:, : h // 2] = p[:, : h // 2]
    pred = nhwc.permute(0, 3, 1, 2)
    bins, conf_sum, sums = kernel(pred.cuda(), labels.cuda(), K, M)
    r = ref64(pred, labels, M)
    assert int((bins[..., 0] - r["bins"][..., 0]).abs().sum()) <= 2 * r["near"]
    np.testing.assert_allclose([float(conf_sum.sum()), *sums.tolist()], [r["conf_sum"], r["nll"], r["brier"], r["qt"]], rtol=SOFT_RTOL)


# ------------------------------------------------------------------------------------------------ GPU: evaluator
@pytest.mark.gpu
def test_eval_segmentation_calibration_end_to_end(tmp_path, parity_log):
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    params = _params("original", 2, "confidence")
    params["output_path"] = str(tmp_path / "with")
    plain = SEG.eval_segmentation(dict(params), dataset=ds, model=Recorder(_k20_model("confidence")))
    assert "calibration" not in plain and not os.path.exists(tmp_path / "with")
    params["evaluation"] = dict(params["evaluation"], calibration=True)
    res = SEG.eval_segmentation(params, dataset=ds, model=Recorder(_k20_model("confidence")))
    assert res["mIoU"] == plain["mIoU"] and res["confusion"] == plain["confusion"] and res["IoU_soft"] == plain["IoU_soft"]
    cal = res["calibration"]
    hard = np.array(res["confusion"])
    assert cal["bins"] == 15 and cal["pixels"] == int(hard.sum())
    assert cal["accuracy"] == float(np.trace(hard)) / float(hard.sum())
    assert sum(cal["reliability"]["count"]) == cal["pixels"] and len(cal["reliability"]["count"]) == 15
    assert set(cal["ece_per_class"]) == set(SEG.TRAIN_ID_NAMES)
    assert 0 <= cal["ece"] <= cal["mce"] <= 1 and cal["nll"] > 0 and 0 <= cal["brier"] <= 2
    assert 1 / 19 - 1e-6 <= cal["mean_confidence"] <= 1 and 0 <= cal["mean_true_class_probability"] <= 1
    assert json.load(open(tmp_path / "with" / "calibration.json")) == cal
    parity_log("eval_segmentation[calibration]", **{k: cal[k] for k in ("ece", "mce", "nll", "brier", "accuracy", "mean_confidence")})
    # another bin count; a one-hot prediction (majority, one evaluation) is scored as well
    params = _params("original", 1, "majority")
    params["output_path"] = str(tmp_path / "onehot")
    params["evaluation"].update(calibration=True, calibration_bins=7)
    res = SEG.eval_segmentation(params, dataset=ds, model=Recorder(_k20_model("majority")))
    cal = res["calibration"]
    assert cal["bins"] == 7 and cal["pixels"] == int(np.array(res["confusion"]).sum())
    assert cal["accuracy"] == float(np.trace(np.array(res["confusion"]))) / cal["pixels"]
