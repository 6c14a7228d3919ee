"""LIDC soft-label scores: the counting kernel (ccdm_lidcscore), metrics.vote_joint_counts, metrics.soft_label_scores_from_counts and
the `evaluation.soft_labels` keys of eval_lidc_uncertainty.  Nothing in the reference computes these.  The kernel's outputs are
integers, so every kernel test asks for equality with a numpy restatement of the definition in include/ccdm_hip.h (np.add.at on
per-pixel counts); the host scores are held against hand-computed cases and against a float64 restatement taken pixel by pixel."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ccdm_lidcscore"}


# ------------------------------------------------------------------------------------------------ restatements
def counts_restatement(samples: np.ndarray, raters: np.ndarray, K: int):
    """samples [B,S,HW], raters [B,L,HW] integer arrays -> (joint int64 [B,K,S+1,L+1], moments int64 [B,5]) by the definition"""
    samples, raters = np.asarray(samples).astype(np.int64), np.asarray(raters).astype(np.int64)
    B, S, HW = samples.shape
    L = raters.shape[1]
    ks = np.arange(K)[None, None, :, None]
    n = (samples[:, :, None, :] == ks).sum(1)                 # [B,K,HW]
    m = (raters[:, :, None, :] == ks).sum(1)
    joint = np.zeros((B, K, S + 1, L + 1), dtype=np.int64)
    bi, ki = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
    np.add.at(joint, (bi[:, :, None], ki[:, :, None], n, m), 1)
    u, v = S * S - (n * n).sum(1), L * L - (m * m).sum(1)     # [B,HW]
    moments = np.stack([u.sum(1), v.sum(1), (u * u).sum(1), (v * v).sum(1), (u * v).sum(1)], axis=1).astype(np.int64)
    return joint, moments


def scores_restatement(samples: torch.Tensor, raters: torch.Tensor, K: int, bins: int, thresholds):
    """The scores of soft_label_scores_from_counts taken pixel by pixel in float64 torch, without the joint table.
    samples [B,S,HW], raters [B,L,HW] int64."""
    from fractions import Fraction
    B, S, HW = samples.shape
    L = raters.shape[1]
    ks = torch.arange(K, device=samples.device)[None, None, :, None]
    n = (samples[:, :, None, :] == ks).sum(1)                 # [B,K,HW] int64
    m = (raters[:, :, None, :] == ks).sum(1)
    p, q = n.double() / S, m.double() / L
    N = B * HW
    level = torch.clamp(n * bins // S, max=bins - 1)
    scored = list(range(1, K)) if K > 1 else [0]
    rel, ece_k = [], []
    for k in range(K):
        cnt, mp, mq, e = [], [], [], 0.0
        for i in range(bins):
            sel = level[:, k] == i
            c = int(sel.sum())
            cnt.append(c)
            if c:
                a, b = float(p[:, k][sel].sum() / c), float(q[:, k][sel].sum() / c)
                e += c / N * abs(a - b)
            mp.append(a if c else None); mq.append(b if c else None)
        rel.append({"count": cnt, "mean_p": mp, "mean_q": mq})
        ece_k.append(e)
    dice = torch.empty((len(thresholds), len(scored), B), dtype=torch.float64)
    for ti, t in enumerate(thresholds):
        f = Fraction(str(t))
        for ci, k in enumerate(scored):
            P = n[:, k] * f.denominator >= f.numerator * S            # n/S >= t without a division
            Q = m[:, k] * f.denominator >= f.numerator * L
            den = (P.sum(1) + Q.sum(1)).double()
            d = 2.0 * (P & Q).sum(1).double() / den
            dice[ti, ci] = torch.where(den == 0, torch.ones_like(d), d).cpu()
    u = (S * S - (n * n).sum(1)).double()
    v = (L * L - (m * m).sum(1)).double()
    corr = []
    for b in range(B):
        du, dv = u[b] - u[b].mean(), v[b] - v[b].mean()
        if float(du.abs().max()) > 0 and float(dv.abs().max()) > 0:
            corr.append(float((du * dv).sum() / torch.sqrt((du * du).sum() * (dv * dv).sum())))
    return {"pixels": N, "images": B, "samples": S, "raters": L, "bins": bins, "reliability": rel, "ece_soft_per_class": ece_k,
            "ece_soft": float(np.mean([ece_k[k] for k in scored])), "brier_soft": float(((p - q) ** 2).sum() / N),
            "cross_entropy_soft": float(-(q * torch.log(torch.clamp(p, min=1e-12))).sum() / N), "dice_soft": float(dice.mean()),
            "dice_soft_per_threshold": [float(x) for x in dice.mean(dim=(1, 2))], "ncc": float(np.mean(corr)) if corr else None,
            "ncc_images": len(corr)}


def assert_scores_close(got: dict, want: dict, rtol: float):
    for key in ("pixels", "images", "samples", "raters", "bins", "ncc_images"):
        assert got[key] == want[key], key
    for key in ("ece_soft", "brier_soft", "cross_entropy_soft", "dice_soft", "ncc"):
        print(f"soft_labels[{key}] got={got[key]!r} want={want[key]!r}")
        if want[key] is None:
            assert got[key] is None, key
        else:
            np.testing.assert_allclose(got[key], want[key], rtol=rtol, atol=0, err_msg=key)
    for key in ("ece_soft_per_class", "dice_soft_per_threshold"):
        np.testing.assert_allclose(got[key], want[key], rtol=rtol, atol=0, err_msg=key)
    assert len(got["reliability"]) == len(want["reliability"])
    for g, w in zip(got["reliability"], want["reliability"]):
        assert g["count"] == w["count"]
        for key in ("mean_p", "mean_q"):
            assert [x is None for x in g[key]] == [x is None for x in w[key]]
            np.testing.assert_allclose([x for x in g[key] if x is not None], [x for x in w[key] if x is not None], rtol=rtol, atol=0)


def _maps(rng, B, S, L, HW, K, top=None):
    """seeded class maps: samples [B,S,HW] that follow a per-pixel preference (so that the levels spread), raters alike"""
    top = K if top is None else top
    pref = rng.integers(0, top, (B, 1, HW))
    samples = np.where(rng.random((B, S, HW)) < 0.6, pref, rng.integers(0, top, (B, S, HW))).astype(np.uint8)
    raters = np.where(rng.random((B, L, HW)) < 0.7, pref, rng.integers(0, top, (B, L, HW))).astype(np.uint8)
    return samples, raters


# ------------------------------------------------------------------------------------------------ CPU: host scores
def _two_level_case():
    """K = 2, S = 2, L = 4, one image of 4 pixels.  (n_1, m_1): A = (1, 4), B = (0, 0) twice, C = (2, 1); class 0 is the complement."""
    joint = np.zeros((1, 2, 3, 5), dtype=np.int64)
    joint[0, 1, 1, 4] = 1; joint[0, 1, 0, 0] = 2; joint[0, 1, 2, 1] = 1
    joint[0, 0, 1, 0] = 1; joint[0, 0, 2, 4] = 2; joint[0, 0, 0, 3] = 1
    # u = 4 - n_0^2 - n_1^2 = [2, 0, 0, 0], v = 16 - m_0^2 - m_1^2 = [0, 0, 0, 6] for (A, B, B, C)
    moments = np.array([[2, 6, 4, 36, 0]], dtype=np.int64)
    return joint, moments


def test_two_level_case_by_hand():
    joint, moments = _two_level_case()
    r = M.soft_label_scores_from_counts(joint, moments, bins=2)
    assert (r["pixels"], r["images"], r["samples"], r["raters"], r["bins"]) == (4, 1, 2, 4, 2)
    # levels 0 | 1, 2.  Class 1: bin 0 = B, B (p 0, q 0); bin 1 = A (0.5, 1), C (1, 0.25): means 0.75, 0.625 -> 2/4 * 0.125
    # class 0: bin 0 = C (0, 0.75) -> 1/4 * 0.75; bin 1 = A (0.5, 0), B, B (1, 1): means 2.5/3, 2/3 -> 3/4 * 0.5/3
    rtol = 1e-14
    np.testing.assert_allclose(r["ece_soft_per_class"], [0.1875 + 0.125, 0.0625], rtol=rtol)
    np.testing.assert_allclose(r["ece_soft"], 0.0625, rtol=rtol)                       # class 0 is dropped
    np.testing.assert_allclose(r["brier_soft"], (0.25 + 0.5625) * 2 / 4, rtol=rtol)
    # q log p: class 1: A 1 * log 0.5, C 0.25 * log 1; class 0: B 1 * log 1, C 0.75 * log(floor)
    np.testing.assert_allclose(r["cross_entropy_soft"], -(math.log(0.5) + 0.75 * math.log(1e-12)) / 4, rtol=rtol)
    assert r["reliability"][1] == {"count": [2, 2], "mean_p": [0.0, 0.75], "mean_q": [0.0, 0.625]}
    assert r["reliability"][0]["count"] == [1, 3]
    # class 1: ceil(2t) = 1 up to t = 0.5, then 2; ceil(4t) = 1, 1, 2, 2, 2, 3, 3, 4, 4.  {n>=1} = {A,C}, {n>=2} = {C}, {m>=1} = {A,C}, {m>=2..4} = {A}
    np.testing.assert_allclose(r["dice_soft_per_threshold"], [1, 1, 2 / 3, 2 / 3, 2 / 3, 0, 0, 0, 0], rtol=rtol)
    np.testing.assert_allclose(r["dice_soft"], 4 / 9, rtol=rtol)
    # HW * sum(uv) - sum(u) sum(v) = -12, variances 4*4 - 4 = 12 and 4*36 - 36 = 108
    np.testing.assert_allclose(r["ncc"], -1 / 3, rtol=rtol)
    assert r["ncc_images"] == 1
    assert json.loads(json.dumps(r)) == r


def test_samples_equal_raters_is_perfect():
    rng = np.random.default_rng(11)
    maps = rng.integers(0, 3, (2, 3, 50))
    joint, moments = counts_restatement(maps, maps, 3)
    r = M.soft_label_scores_from_counts(joint, moments, bins=4, class_names=["bg", "a", "b"])
    assert r["ece_soft"] == 0.0 and r["brier_soft"] == 0.0 and r["dice_soft"] == 1.0
    assert r["ece_soft_per_class"] == [0.0, 0.0, 0.0] and r["dice_soft_per_threshold"] == [1.0] * 9
    assert r["ncc"] == pytest.approx(1.0, abs=1e-15) and r["ncc_images"] == 2 and r["class_names"] == ["bg", "a", "b"]
    assert json.loads(json.dumps(r)) == r


def test_threshold_on_a_boundary_is_exact():
    """t = 0.3 at S = 10 means n >= 3, t = 0.7 means n >= 7: the ceilings are taken of the decimal as written (in floating point
    0.07 * 100 > 7 and its ceiling is 8)"""
    assert M._ceil_fraction(0.3, 10) == 3 and M._ceil_fraction(0.7, 10) == 7
    assert math.ceil(0.07 * 100) == 8 and M._ceil_fraction(0.07, 100) == 7
    joint = np.zeros((1, 2, 11, 11), dtype=np.int64)
    joint[0, 1, 3, 5] = 1; joint[0, 1, 7, 9] = 1; joint[0, 1, 0, 0] = 2              # X: 3 samples, 5 raters; Y: 7 samples, 9 raters
    joint[0, 0, 7, 5] = 1; joint[0, 0, 3, 1] = 1; joint[0, 0, 10, 10] = 2
    moments = np.array([[84, 68, 3528, 2824, 2856]], dtype=np.int64)                  # u = [42, 42, 0, 0], v = [50, 18, 0, 0]

    def dice(t):
        return M.soft_label_scores_from_counts(joint, moments, thresholds=(t,))["dice_soft"]
    assert dice(0.3) == 1.0                                   # P = Q = {X, Y}; with n >= 4, P = {Y}: 2/3
    assert dice(0.31) == 2 / 3
    assert dice(0.7) == 1.0                                   # P = Q = {Y}; with n >= 8, P is empty: 0
    assert dice(0.71) == 0.0                                  # P is empty, Q = {Y}


def test_zero_variance_image_is_left_out_of_ncc_and_empty_bin_is_none():
    joint, moments = _two_level_case()
    flat = np.zeros_like(joint)
    flat[0, 1, 0, 0] = 4; flat[0, 0, 2, 4] = 4                # an image everyone calls background: u = v = 0 everywhere
    r = M.soft_label_scores_from_counts(np.concatenate([joint, flat]), np.concatenate([moments, np.zeros((1, 5), dtype=np.int64)]), bins=4)
    assert r["images"] == 2 and r["pixels"] == 8 and r["ncc_images"] == 1
    np.testing.assert_allclose(r["ncc"], -1 / 3, rtol=1e-14)
    # levels of S = 2 fall in bins 0, 2, 3 of 4: bin 1 is empty for every class
    for k in (0, 1):
        assert r["reliability"][k]["count"][1] == 0 and r["reliability"][k]["mean_p"][1] is None and r["reliability"][k]["mean_q"][1] is None
    # a constant v with a varying u is left out too
    only = M.soft_label_scores_from_counts(flat, np.array([[4, 0, 8, 0, 0]], dtype=np.int64))
    assert only["ncc"] is None and only["ncc_images"] == 0
    assert only["dice_soft"] == 1.0                           # both sets empty at every threshold: the nan -> 1 rule
    assert json.loads(json.dumps(only)) == only


def test_single_class_uses_class_zero():
    joint = np.zeros((1, 1, 3, 3), dtype=np.int64)
    joint[0, 0, 2, 2] = 3; joint[0, 0, 1, 2] = 1              # one sample byte of one pixel is no class
    r = M.soft_label_scores_from_counts(joint, np.array([[3, 0, 9, 0, 0]], dtype=np.int64), bins=2, thresholds=(0.5, 1.0))
    np.testing.assert_allclose(r["ece_soft"], 0.125, rtol=1e-14)                    # one bin: means 3.5/4 and 1
    assert r["ece_soft_per_class"] == [r["ece_soft"]]
    np.testing.assert_allclose(r["dice_soft_per_threshold"], [1.0, 2 * 3 / 7], rtol=1e-14)        # t = 1: P = 3 pixels, Q = 4
    assert r["ncc"] is None


def test_scores_from_counts_match_per_pixel_restatement():
    rng = np.random.default_rng(5)
    for (B, S, L, HW, K, bins) in ((3, 7, 4, 300, 3, 10), (2, 10, 3, 200, 2, 15), (1, 16, 4, 128, 5, 4)):
        samples, raters = _maps(rng, B, S, L, HW, K, top=K + 1)          # some bytes are no class
        joint, moments = counts_restatement(samples, raters, K)
        got = M.soft_label_scores_from_counts(joint, moments, bins=bins)
        want = scores_restatement(torch.from_numpy(samples.astype(np.int64)), torch.from_numpy(raters.astype(np.int64)), K, bins,
                                  M.SOFT_LABEL_THRESHOLDS)
        assert_scores_close(got, want, rtol=1e-12)            # a few hundred float64 terms on either side


def test_bad_arguments_are_named():
    joint, moments = _two_level_case()
    with pytest.raises(ValueError, match="thresholds"):
        M.soft_label_scores_from_counts(joint, moments, thresholds=(0.0,))
    with pytest.raises(ValueError, match="class_names"):
        M.soft_label_scores_from_counts(joint, moments, class_names=["a"])
    with pytest.raises(ValueError, match="no pixel"):
        M.soft_label_scores_from_counts(np.zeros_like(joint), moments)
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        M.vote_joint_counts(torch.zeros((1, 2, 4), dtype=torch.uint8), torch.zeros((1, 2, 4), dtype=torch.uint8), 2)


# ------------------------------------------------------------------------------------------------ CPU: ABI
def test_lidcscore_symbol_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_lidcscore[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_lidc")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")) == 10, name
        assert not name.startswith(("ccdm_seg_", "ccdm_segcalib", "ccdm_segboundary", "ccdm_vote_"))
    assert "ccdm_lidcscore.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_lidcscore.hip"))
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11


def test_lidcscore_refuses_what_it_cannot_count():
    """the limits are checked before anything is launched or read: host buffers stand in for the device's"""
    lib = hip.load()
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    for (B, S, L, HW, K, joint, moments), what in (((1, 100, 5, 16, 32, p, p), "K*(S+1)*(L+1)"), ((1, 0, 4, 16, 2, p, p), "S=0"),
                                                   ((1, 256, 1, 16, 2, p, p), "S=256"), ((1, 4, 0, 16, 2, p, p), "L=0"),
                                                   ((1, 4, 4, 16, 33, p, p), "K=33"), ((1, 4, 4, 16, 0, p, p), "K=0"),
                                                   ((1, 4, 4, 0, 2, p, p), "HW=0"), ((1, 4, 4, 16, 2, None, None), "both NULL"),
                                                   ((0, 0, 4, 16, 2, p, p), "S=0")):
        rc = lib.ccdm_lidcscore(p, p, B, S, L, HW, K, joint, moments, None)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "lidcscore")
    assert lib.ccdm_lidcscore(p, p, 0, 4, 4, 16, 2, p, p, None) == 0 and not buf.any()          # B = 0: nothing launched, nothing written


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def kernel(samples: torch.Tensor, raters: torch.Tensor, K: int, want_joint=True, want_moments=True):
    """one ccdm_lidcscore call on uint8 device maps [B,S,HW] / [B,L,HW] (as they lie in memory) -> (joint, moments) numpy; the
    outputs start from a non-zero fill: the call overwrites"""
    lib = hip.load()
    assert samples.is_cuda and raters.is_cuda and samples.dtype == raters.dtype == torch.uint8
    assert samples.is_contiguous() and raters.is_contiguous()
    B, S, HW = samples.shape
    L = raters.shape[1]
    joint = torch.full((B, K, S + 1, L + 1), 77, dtype=torch.int32, device="cuda")
    moments = torch.full((B, 5), -5, dtype=torch.int64, device="cuda")
    hip.check(lib.ccdm_lidcscore(samples.data_ptr(), raters.data_ptr(), B, S, L, HW, K, joint.data_ptr() if want_joint else None,
                                 moments.data_ptr() if want_moments else None, None), "lidcscore")
    torch.cuda.synchronize()
    return joint.cpu().numpy().astype(np.int64), moments.cpu().numpy()


def check_exact(samples: np.ndarray, raters: np.ndarray, K: int, tag=""):
    joint, moments = kernel(torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda(), K)
    joint_r, moments_r = counts_restatement(samples, raters, K)
    print(f"lidcscore[{tag} {samples.shape} {raters.shape} K{K}] cells={int((joint_r > 0).sum())} "
          f"diff={int(np.abs(joint - joint_r).sum())},{int(np.abs(moments - moments_r).sum())}")
    np.testing.assert_array_equal(joint, joint_r)
    np.testing.assert_array_equal(moments, moments_r)
    HW = samples.shape[2]
    assert (joint.sum(axis=(2, 3)) == HW).all()               # every pixel is in one cell of every class
    return joint, moments


KERNEL_SHAPES = [(1, 1, 1, 1, 2), (2, 3, 4, 63, 2), (2, 16, 4, 4096, 2), (1, 100, 4, 16384, 2), (3, 5, 3, 1000, 8), (1, 7, 2, 260, 20),
                 (1, 100, 4, 256, 32), (1, 255, 1, 512, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,L,HW,K", KERNEL_SHAPES)
def test_kernel_matches_restatement(B, S, L, HW, K):
    rng = np.random.default_rng(1000 + 7 * S + HW + K)
    samples, raters = _maps(rng, B, S, L, HW, K)
    joint, _ = check_exact(samples, raters, K, "random")
    n = np.arange(S + 1)[None, None, :, None]
    assert int((joint * n).sum()) == B * S * HW               # every byte is a class: the samples' votes are all counted


@pytest.mark.gpu
def test_kernel_byte_packed_counts_at_their_maximum():
    """S = 255 samples that all say the same class: the packed byte of that class stays 0, the other's reaches 255"""
    samples = np.ones((1, 255, 512), dtype=np.uint8)
    samples[:, :, ::3] = 0
    raters = np.ones((1, 1, 512), dtype=np.uint8)
    joint, moments = check_exact(samples, raters, 2, "max")
    assert joint[0, 1, 255, 1] == 512 - 171 and joint[0, 0, 255, 0] == 171 and (moments == 0).all()


@pytest.mark.gpu
def test_kernel_unaligned_base_pointer():
    """HW % 4 == 0 but the maps start one byte off a dword: the byte path"""
    rng = np.random.default_rng(21)
    B, S, L, HW, K = 2, 6, 4, 256, 2
    samples, raters = _maps(rng, B, S, L, HW, K)
    s_buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    r_buf = torch.zeros(raters.size + 1, dtype=torch.uint8, device="cuda")
    s_dev, r_dev = s_buf[1:].view(B, S, HW), r_buf[1:].view(B, L, HW)
    s_dev.copy_(torch.from_numpy(samples)); r_dev.copy_(torch.from_numpy(raters))
    assert s_dev.data_ptr() % 4 == 1 and r_dev.data_ptr() % 4 == 1
    want = counts_restatement(samples, raters, K)
    for s_t, r_t in ((s_dev, r_dev), (s_dev, torch.from_numpy(raters).cuda()), (torch.from_numpy(samples).cuda(), r_dev)):
        joint, moments = kernel(s_t, r_t, K)
        np.testing.assert_array_equal(joint, want[0])
        np.testing.assert_array_equal(moments, want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,L,HW,K", [(2, 5, 3, 1000, 8), (1, 9, 4, 63, 2), (1, 6, 4, 512, 20)])
def test_kernel_bytes_that_are_no_class(B, S, L, HW, K):
    rng = np.random.default_rng(31 + K)
    samples, raters = _maps(rng, B, S, L, HW, K, top=K + 3)
    samples[:, :, ::7] = 255
    raters[:, 0, ::5] = K
    joint, _ = check_exact(samples, raters, K, "no-class")
    n = np.arange(S + 1)[None, None, :, None]
    assert int((joint * n).sum()) == int((samples < K).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 1])
def test_kernel_all_equal_maps(value):
    """every lane of every wave holds the same cell: the wave-aggregated add"""
    samples = np.full((2, 16, 4096), value, dtype=np.uint8)
    raters = np.full((2, 4, 4096), value, dtype=np.uint8)
    joint, moments = check_exact(samples, raters, 2, "equal")
    assert joint[:, value, 16, 4].tolist() == [4096, 4096] and joint[:, 1 - value, 0, 0].tolist() == [4096, 4096]
    assert (moments == 0).all()
    check_exact(samples[:, :, :999].copy(), raters[:, :, :999].copy(), 2, "equal-bytes")


@pytest.mark.gpu
def test_kernel_agrees_with_pair_counts_and_vote_counts():
    lib = hip.load()
    rng = np.random.default_rng(41)
    # S = L = 1: the cells of one map against one map are the intersection and the union of ccdm_pairwise_class_counts
    for K, HW in ((2, 1024), (5, 777)):
        a, b = _maps(rng, 3, 1, 1, HW, K)
        joint, _ = kernel(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), K)
        pc = M.pairwise_class_counts(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), K)[:, 0, 0].astype(np.int64)       # [B,K,2]
        np.testing.assert_array_equal(joint[:, :, 1, 1], pc[..., 0])
        np.testing.assert_array_equal(joint[:, :, 1, 0] + joint[:, :, 0, 1] + joint[:, :, 1, 1], pc[..., 1])
    # the marginal over the raters is the histogram of the per-pixel counts of ccdm_vote_reduce_stack
    B, S, L, HW, K = 2, 12, 4, 1500, 3
    samples, raters = _maps(rng, B, S, L, HW, K)
    s_dev = torch.from_numpy(samples).cuda()
    joint, _ = kernel(s_dev, torch.from_numpy(raters).cuda(), K)
    counts = torch.zeros((B, HW, K), dtype=torch.int32, device="cuda")
    hip.check(lib.ccdm_vote_reduce_stack(s_dev.data_ptr(), B, S, HW, K, counts.data_ptr(), None, None, None, None), "vote_reduce_stack")
    counts = counts.cpu().numpy()
    for b in range(B):
        for k in range(K):
            np.testing.assert_array_equal(joint[b, k].sum(axis=1), np.bincount(counts[b, :, k], minlength=S + 1))


@pytest.mark.gpu
def test_kernel_outputs_optional_overwritten_and_repeatable():
    lib = hip.load()
    rng = np.random.default_rng(51)
    B, S, L, HW, K = 2, 16, 4, 4096, 2
    samples, raters = _maps(rng, B, S, L, HW, K)
    s_dev, r_dev = torch.from_numpy(samples).cuda(), torch.from_numpy(raters).cuda()
    want = counts_restatement(samples, raters, K)
    first, second = kernel(s_dev, r_dev, K), kernel(s_dev, r_dev, K)
    for a, b, w in zip(first, second, want):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, w)
    joint, moments = kernel(s_dev, r_dev, K, want_moments=False)              # either output alone; the other is not touched
    np.testing.assert_array_equal(joint, want[0])
    assert (moments == -5).all()
    joint, moments = kernel(s_dev, r_dev, K, want_joint=False)
    np.testing.assert_array_equal(moments, want[1])
    assert (joint == 77).all()
    # B = 0 leaves prefilled outputs as they are
    j = torch.full((1, K, S + 1, L + 1), 9, dtype=torch.int32, device="cuda")
    m = torch.full((1, 5), 9, dtype=torch.int64, device="cuda")
    assert lib.ccdm_lidcscore(s_dev.data_ptr(), r_dev.data_ptr(), 0, S, L, HW, K, j.data_ptr(), m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((j == 9).all()) and bool((m == 9).all())
    # the limits raise through the binding, named
    for args, what in (((s_dev.data_ptr(), r_dev.data_ptr(), 1, 100, 5, 16, 32, j.data_ptr(), m.data_ptr(), None), "K*(S+1)*(L+1)"),
                       ((s_dev.data_ptr(), r_dev.data_ptr(), 1, 0, L, HW, K, j.data_ptr(), m.data_ptr(), None), "S=0"),
                       ((s_dev.data_ptr(), r_dev.data_ptr(), B, S, L, HW, K, None, None, None), "both NULL")):
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(lib.ccdm_lidcscore(*args), "lidcscore")


@pytest.mark.gpu
def test_vote_joint_counts_takes_index_maps_of_any_shape():
    rng = np.random.default_rng(61)
    samples = torch.from_numpy(rng.integers(0, 3, (2, 5, 9, 7)))              # int64 [B,S,H,W]
    raters = torch.from_numpy(rng.integers(0, 3, (2, 4, 9, 7)))
    joint, moments = M.vote_joint_counts(samples.cuda(), raters.cuda(), 3)
    want = counts_restatement(samples.reshape(2, 5, -1).numpy(), raters.reshape(2, 4, -1).numpy(), 3)
    assert joint.dtype == np.int64 and moments.dtype == np.int64 and joint.shape == (2, 3, 6, 5) and moments.shape == (2, 5)
    np.testing.assert_array_equal(joint, want[0])
    np.testing.assert_array_equal(moments, want[1])
    sliced, _ = M.vote_joint_counts(samples.cuda()[:, :2], raters.cuda(), 3)              # the evaluator's pred_idx[:, :s]
    np.testing.assert_array_equal(sliced, counts_restatement(samples[:, :2].reshape(2, 2, -1).numpy(), raters.reshape(2, 4, -1).numpy(), 3)[0])


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("vote", ["confidence", "majority"])
def test_evaluator_soft_labels_end_to_end(vote, tmp_path):
    from ccdm_stochastic_segmentation_amd import evaluation as E
    from tests.golden_util import harness_case
    batches, evaluations, K, predict = harness_case(vote)

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
    assert "soft_labels" not in plain and not (tmp_path / "out").exists()
    bins, thresholds = 8, [0.25, 0.5, 0.75]
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"soft_labels": True, "soft_label_bins": bins, "soft_label_thresholds": thresholds}},
                                  dataset=DS(), device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"soft_labels"}
    for key, value in plain.items():                          # everything the evaluator returns today is untouched
        assert res[key] == value, key

    # the predictions and labels the evaluator saw, batch by batch
    S = max(evaluations)
    pred, lab = [], []
    for call, (image, labels, _) in enumerate(batches):
        p = predict(call, labels.shape[0] * S).reshape(labels.shape[0], S, *labels.shape[2:])
        pred.append(p.argmax(dim=2).reshape(labels.shape[0], S, -1))
        lab.append(labels.argmax(dim=2).reshape(labels.shape[0], labels.shape[1], -1))
    pred, lab = torch.cat(pred).cuda(), torch.cat(lab).cuda()
    assert len(res["soft_labels"]) == len(evaluations)
    for s, got in zip(evaluations, res["soft_labels"]):
        want = scores_restatement(pred[:, :s], lab, K, bins, thresholds)
        assert got["thresholds"] == thresholds and got["samples"] == s and got["images"] == 5
        assert_scores_close(got, want, rtol=1e-9)             # N * 2^-53 for N ~ 10^6 summed terms, float64 on both sides
    default = E.eval_lidc_uncertainty({**params, "evaluation": {"soft_labels": True}, "output_path": None}, dataset=DS(), device="cuda:0",
                                      model=fake())["soft_labels"]
    assert default[0]["bins"] == 10 and default[0]["thresholds"] == list(M.SOFT_LABEL_THRESHOLDS)
    with open(tmp_path / "out" / "lidc_soft_labels.json") as f:
        assert json.load(f) == res["soft_labels"] == json.loads(json.dumps(res["soft_labels"]))
