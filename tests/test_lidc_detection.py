"""LIDC lesion findings of the sample set: the kernels of ccdm_findings, metrics.sample_findings / concat_findings /
detection_scores_from_findings, DenoisingModel.predict_findings and the `evaluation.detection` keys of eval_lidc_uncertainty.  Nothing
in the reference computes these.  Everything the kernels write is an integer, so every kernel test asks for equality with the numpy
restatement of the definition in include/ccdm_hip.h (detection_util), whose labels are held against scipy.ndimage.label; the host
scores are held against a brute-force loop over the thresholds and against an example worked out by hand."""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import detection_util as U
from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"ccdm_findings", "ccdm_findings_workspace_bytes"}
ARRAYS = ("counts", "candidates", "references")
# (B, S, L, H, W, K, connectivity): the dword path; the byte path with a sample bitset that crosses a word; the most samples; the
# largest map; no raters; K = 1, which scores class 0
SHAPES = [(2, 5, 4, 24, 20, 2, 8), (3, 33, 1, 7, 9, 4, 4), (1, 255, 4, 32, 32, 2, 8), (1, 16, 4, 128, 128, 2, 8), (2, 4, 0, 16, 16, 3, 8),
          (1, 1, 1, 4, 4, 1, 4)]
CAP = 8


# ------------------------------------------------------------------------------------------------ CPU: restatement against scipy
def test_restatement_labels_equal_scipy():
    """the flood fill numbers components as scipy.ndimage.label does, under both structures, on every mask the tests use; and the
    records built on scipy's labels are the records built on the flood fill's"""
    for shape in SHAPES:
        samples, raters = U.lesion_like_case(*shape[:6])
        n_min, m_min = U.default_thresholds(shape[1], shape[2])
        for connectivity in (4, 8):
            own = U.findings_restatement(samples, raters, shape[5], n_min, m_min, connectivity, CAP)
            by_scipy = U.findings_restatement(samples, raters, shape[5], n_min, m_min, connectivity, CAP, label=U.scipy_labels)
            for k in ARRAYS + ("confidence_map", "labels"):
                np.testing.assert_array_equal(own[k], by_scipy[k], err_msg=f"{shape} {connectivity} {k}")
    for name in U.HAND_MAPS:
        m = U.hand_map(name)
        for connectivity in (4, 8):
            lab, n = U.flood_labels(m > 0, connectivity)
            want, want_n = U.scipy_labels(m > 0, connectivity)
            assert n == want_n, name
            np.testing.assert_array_equal(lab, want, err_msg=name)


def test_restatement_fields_on_a_worked_map():
    """S = 3, L = 2, one class, 4-connectivity, n_min = 2, m_min = 1, on a 4x6 map:
         n = 3 3 . . 1 .      m = 1 . . . . .      A (n >= 2): candidate 1 = the 2x2 block (rows 0-1, columns 0-1), candidate 2 = (3,4), (3,5)
             2 2 . . . .          . . . . . .      R (m >= 1): lesion 1 = (0,0), lesion 2 = (2,2)
             . . . . . .          . . 2 . . .
             . . . . 2 2          . . . . . .
       candidate 1: size 4, support 3, peak 3, mass 10, ref_cov 1, rater_hits 1, box (0,0)-(1,1), sums 2, 2; candidate 2: size 2,
       support 2 (samples 0 and 2), peak 2, mass 4, ref_cov 0, rater_hits 0, box (3,4)-(3,5), sums 6, 9
       lesion 1: size 1, cov 1, best_support 3, best_peak 3; lesion 2: size 1, cov 0, touched by nothing"""
    s = np.zeros((1, 3, 4, 6), dtype=np.uint8)
    s[0, :, 0, 0:2] = 1; s[0, 0:2, 1, 0:2] = 1; s[0, 1, 0, 4] = 1; s[0, 0, 3, 4:6] = 1; s[0, 2, 3, 4:6] = 1
    r = np.zeros((1, 2, 4, 6), dtype=np.uint8)
    r[0, 0, 0, 0] = 1; r[0, :, 2, 2] = 1
    f = U.findings_restatement(s, r, 2, 2, 1, 4, 3)
    assert f["counts"].tolist() == [[[2, 2]]]
    assert f["candidates"][0, 0].tolist() == [[4, 3, 3, 10, 1, 1, 0, 0, 1, 1, 2, 2], [2, 2, 2, 4, 0, 0, 3, 4, 3, 5, 6, 9], [0] * 12]
    assert f["references"][0, 0].tolist() == [[1, 1, 3, 3], [1, 0, 0, 0], [0] * 4]
    assert f["confidence_map"][0, 0].tolist() == [[3, 3, 0, 0, 0, 0], [3, 3, 0, 0, 0, 0], [0] * 6, [0, 0, 0, 0, 2, 2]]


def test_generator_is_lesion_like():
    """what the GPU tests rely on, by the restatement alone: a few candidates per (image, class), true and false ones, many support
    values, and max_candidates = 8 holds"""
    supports, true, false = set(), 0, 0
    for shape in SHAPES:
        for connectivity in (4, 8):
            f = U.lesion_like_findings(shape[:6], connectivity, 64)
            counts, cand = f["counts"], f["candidates"]
            assert int(counts.max()) <= 5 <= CAP, shape
            if shape[3] * shape[4] > 16:
                assert int(counts[..., 0].max()) >= 2, shape
            for b, ci in np.ndindex(*counts.shape[:2]):
                for rec in cand[b, ci, :counts[b, ci, 0]]:
                    assert rec[1] >= rec[2] >= f["n_min"] and rec[0] >= 1 and rec[3] >= rec[2]          # support >= peak >= n_min
                    if connectivity == shape[6]:
                        supports.add((shape, int(rec[1])))
                        true += int(rec[4] >= 1)
                        false += int(rec[4] == 0)
    print(f"lesion_like_case: {len(supports)} (shape, support) values, {true} true and {false} false candidates")
    assert 5 <= len(supports) <= 20 and true >= 3 and false >= 3
    first = U.lesion_like_findings(SHAPES[0][:6], 8, 64)
    assert 1 <= int(first["counts"][..., 0].min()) and int(first["counts"][..., 1].max()) >= 1
    assert (first["candidates"][..., 4] >= 1).any() and ((first["candidates"][..., 4] == 0) & (first["candidates"][..., 0] > 0)).any()


# ------------------------------------------------------------------------------------------------ CPU: host scores
def _hand_findings():
    """S = 4, n_min = 1 (thresholds 4, 3, 2, 1), three images, classes 1 and 2, score = support.
    Class 1.  Image 0: candidate a (support 4) covers the reference lesions r1 and r2 (one candidate, two lesions); candidate b
    (support 4) covers none.  Image 1: candidates c (support 3) and d (support 1) both lie on lesion r3 (two candidates, one lesion:
    best_support 3); lesion r4 is touched by nothing.  Image 2: nothing.  N_ref = 4, images = 3.
       theta  FP  TPc  det  sensitivity  precision  FP/image
         4     1   1    2      1/2          1/2        1/3
         3     1   2    3      3/4          2/3        1/3
         2     1   2    3      3/4          2/3        1/3
         1     1   3    3      3/4          3/4        1/3
    sensitivity at 1/8 and 1/4 false positives per image: 0 (only the empty threshold qualifies); at 1/2, 1, 2, 4, 8: 3/4;
    CPM = (5 * 3/4) / 7 = 15/28.  AP = (1/2 - 0) * 1/2 + (3/4 - 1/2) * 2/3 = 5/12.
    Class 2.  Image 2 holds one candidate (support 2) and there is no reference lesion anywhere: sensitivity, CPM and AP are None,
    precision is 0 from theta = 2 down."""
    counts = np.zeros((3, 2, 2), dtype=np.int64)
    cand = np.zeros((3, 2, 2, 12), dtype=np.int64)
    ref = np.zeros((3, 2, 2, 4), dtype=np.int64)
    counts[0, 0] = 2, 2
    cand[0, 0, 0, :6] = 30, 4, 4, 90, 9, 2
    cand[0, 0, 1, :6] = 5, 4, 2, 8, 0, 0
    ref[0, 0, 0] = 5, 5, 4, 4
    ref[0, 0, 1] = 4, 4, 4, 4
    counts[1, 0] = 2, 2
    cand[1, 0, 0, :6] = 6, 3, 3, 12, 4, 1
    cand[1, 0, 1, :6] = 2, 1, 1, 2, 2, 1
    ref[1, 0, 0] = 9, 6, 3, 3
    ref[1, 0, 1] = 3, 0, 0, 0
    counts[2, 1] = 1, 0
    cand[2, 1, 0, :6] = 7, 2, 2, 9, 0, 0
    return {"counts": counts, "candidates": cand, "references": ref, "samples": 4, "raters": 3, "n_min": 1, "m_min": 2, "connectivity": 8,
            "classes": [1, 2], "max_candidates": 2}


def test_scores_on_the_hand_example():
    f = _hand_findings()
    r = M.detection_scores_from_findings(f, class_names=["nodule", "other"])
    one, two = r["per_class"]
    assert one["froc"] == {"thresholds": [4, 3, 2, 1], "fp_per_image": [1 / 3] * 4, "sensitivity": [0.5, 0.75, 0.75, 0.75],
                           "precision": [0.5, 2 / 3, 2 / 3, 0.75]}
    assert one["sensitivity_at_fp"] == [0.0, 0.0, 0.75, 0.75, 0.75, 0.75, 0.75] and one["cpm"] == float(Fraction(15, 28))
    assert one["average_precision"] == float(Fraction(5, 12))
    assert (one["candidates"], one["true_candidates"], one["reference_lesions"], one["images_without_reference"]) == (4, 3, 4, 1)
    assert two["froc"]["sensitivity"] == [None] * 4 and two["froc"]["precision"] == [None, None, 0.0, 0.0]
    assert two["froc"]["fp_per_image"] == [0.0, 0.0, 1 / 3, 1 / 3]
    assert two["sensitivity_at_fp"] is None and two["cpm"] is None and two["average_precision"] is None
    assert (two["candidates"], two["true_candidates"], two["reference_lesions"], two["images_without_reference"]) == (1, 0, 0, 3)
    assert r["cpm"] == one["cpm"] and r["average_precision"] == one["average_precision"]         # over the classes with a lesion
    assert (r["images"], r["samples"], r["raters"], r["n_min"], r["m_min"], r["score"]) == (3, 4, 3, 1, 2, "support")
    assert r["fp_rates"] == [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0] and r["class_names"] == ["nodule", "other"] and r["classes"] == [1, 2]
    assert json.loads(json.dumps(r)) == r
    # by peak, candidate b (peak 2, false) drops below the true ones: no false positive at theta = 4 and 3
    p = M.detection_scores_from_findings(f, score="peak")["per_class"][0]
    assert p["froc"]["fp_per_image"] == [0.0, 0.0, 1 / 3, 1 / 3] and p["sensitivity_at_fp"] == [0.75] * 7 and p["average_precision"] == 0.75
    # a higher n_min drops the thresholds below it; custom rates
    high = M.detection_scores_from_findings({**f, "n_min": 3}, fp_rates=[0, 0.4])["per_class"][0]
    assert high["froc"]["thresholds"] == [4, 3] and high["sensitivity_at_fp"] == [0.0, 0.75]
    both = M.concat_findings([f, f])
    assert both["counts"].shape == (6, 2, 2) and both["candidates"].shape == (6, 2, 2, 12) and both["classes"] == [1, 2]
    twice = M.detection_scores_from_findings(both)
    assert twice["per_class"][0]["froc"] == one["froc"] and twice["images"] == 6 and twice["per_class"][0]["reference_lesions"] == 8
    with pytest.raises(ValueError, match="differ in"):
        M.concat_findings([f, {**f, "n_min": 2}])
    for change, what in ((dict(score="mass"), "score"), (dict(fp_rates=[]), "fp_rates"), (dict(fp_rates=[-1]), "fp_rates"),
                         (dict(class_names=["a"]), "class_names")):
        with pytest.raises(ValueError, match=what):
            M.detection_scores_from_findings(f, **change)
    for change, what in (({"raters": 0}, "without raters"), ({"counts": f["counts"][0]}, r"expected \[B,C,2\]"), ({"n_min": 5}, "n_min"),
                         ({"classes": [1]}, "classes"), ({"candidates": f["candidates"][:, :, :1]}, "records")):
        with pytest.raises(ValueError, match=what):
            M.detection_scores_from_findings({**f, **change})
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        M.sample_findings(torch.zeros((1, 2, 4, 4), dtype=torch.uint8), None, 2, n_min=1)


def _assert_scores_equal_brute_force(findings, score, fp_rates):
    got = M.detection_scores_from_findings(findings, score=score, fp_rates=fp_rates)
    want = U.scores_restatement(findings, score, fp_rates)
    B = findings["counts"].shape[0]
    for g, w in zip(got["per_class"], want):
        assert g["froc"]["thresholds"] == [c[0] for c in w["curve"]]
        assert g["froc"]["fp_per_image"] == [float(Fraction(c[1], B)) for c in w["curve"]]
        assert g["froc"]["sensitivity"] == [float(Fraction(c[3], w["reference_lesions"])) if w["reference_lesions"] else None for c in w["curve"]]
        assert g["froc"]["precision"] == [float(Fraction(c[2], c[1] + c[2])) if c[1] + c[2] else None for c in w["curve"]]
        assert g["sensitivity_at_fp"] == (None if w["sensitivity_at_fp"] is None else [float(v) for v in w["sensitivity_at_fp"]])
        assert g["cpm"] == (None if w["cpm"] is None else float(w["cpm"]))
        assert g["average_precision"] == (None if w["average_precision"] is None else float(w["average_precision"]))
        assert (g["candidates"], g["reference_lesions"], g["images_without_reference"]) == \
            (w["candidates"], w["reference_lesions"], w["images_without_reference"])
    return got


def test_scores_equal_brute_force():
    for f in (_hand_findings(), {**_hand_findings(), "n_min": 2}):
        for score in ("support", "peak"):
            _assert_scores_equal_brute_force(f, score, (1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8))
    seen = 0
    for shape in SHAPES:
        if shape[2] == 0:
            continue
        for score in ("support", "peak"):
            f = U.lesion_like_findings(shape[:6], shape[6], CAP)
            got = _assert_scores_equal_brute_force(f, score, (0, 0.3, 1, 2.5))
            seen += sum(c["cpm"] is not None and 0 < c["cpm"] for c in got["per_class"])
    assert seen >= 4                                                  # the cases do detect something
    no_raters = U.lesion_like_findings(SHAPES[4][:6], 8, CAP)
    with pytest.raises(ValueError, match="without raters"):
        M.detection_scores_from_findings(no_raters)


# ------------------------------------------------------------------------------------------------ CPU: evaluator keys
def test_evaluator_keys_are_parsed_and_refused():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    assert E.detection_min_frequency(0.1) == 0.1 and E.detection_min_frequency(1) == 1 and E.detection_min_frequency(0) == 0
    assert M._ceil_fraction(E.detection_min_frequency(0.3), 10) == 3           # the decimal as written, not 0.3 * 10 = 3.0000000000000004
    for bad in (-0.1, 1.5, True, None, "a", [0.1]):
        with pytest.raises(ValueError, match="detection_min_frequency"):
            E.detection_min_frequency(bad)
    assert E.detection_rater_agreement("majority", 4) == 3 and E.detection_rater_agreement("majority", 1) == 1
    assert E.detection_rater_agreement("majority", 3) == 2 and E.detection_rater_agreement(1, 4) == 1 and E.detection_rater_agreement(4, 4) == 4
    for bad in (0, 5, True, 2.0, "all", None):
        with pytest.raises(ValueError, match="detection_rater_agreement"):
            E.detection_rater_agreement(bad, 4)
    assert E.detection_score("support") == "support" and E.detection_score("peak") == "peak"
    for bad in ("mass", None, 1):
        with pytest.raises(ValueError, match="detection_score"):
            E.detection_score(bad)
    assert E.detection_fp_rates([0.125, 1, 8]) == [0.125, 1, 8] and E.detection_fp_rates(2) == [2] and E.detection_fp_rates((0,)) == [0]
    for bad in ([], [-1], [True], ["1"], [float("inf")], [float("nan")], None):
        with pytest.raises(ValueError, match="detection_fp_rates"):
            E.detection_fp_rates(bad)
    assert E.detection_max_candidates(64) == 64 and E.detection_max_candidates(1) == 1 and E.detection_max_candidates(1024) == 1024
    for bad in (0, 1025, True, 8.0, "8", None):
        with pytest.raises(ValueError, match="detection_max_candidates"):
            E.detection_max_candidates(bad)
    assert M.FINDINGS_MAX_CANDIDATES == 1024 and M.DETECTION_FP_RATES == (0.125, 0.25, 0.5, 1, 2, 4, 8)


def test_evaluator_without_the_key_is_as_before(monkeypatch):
    """a stub model with fixed predictions through eval_lidc_uncertainty on the CPU (the pair counts of the GED, the one thing the plain
    evaluator asks the device for, are restated with numpy): no `detection` key, or a false one, and the result is the plain run's"""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    K, H, W, evaluations, batch = 2, 9, 7, [2, 3], 2
    S = max(evaluations)
    rng = np.random.default_rng(5)
    samples, raters = rng.integers(0, K, (3, S, H, W)), rng.integers(0, K, (3, 4, H, W))
    one_hot = lambda idx: torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), K).movedim(-1, -3).float()

    def counts(a, b, num_classes):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        out = np.zeros((a.shape[0], a.shape[1], b.shape[1], num_classes, 2), dtype=np.int32)
        for k in range(num_classes):
            x, y = (a == k)[:, :, None], (b == k)[:, None, :]
            out[..., k, 0], out[..., k, 1] = (x & y).sum(axis=(3, 4)), (x | y).sum(axis=(3, 4))
        return out
    monkeypatch.setattr(M, "pairwise_class_counts", counts)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, b):
            return torch.zeros((1, H, W)), one_hot(raters[b]), np.array([0.25] * 4)

    def fake():
        class Fake:
            step_T_sample = "majority"
            calls = 0

            def __call__(self, x, image, **kw):
                first = self.calls * batch
                self.calls += 1
                return {"diffusion_out": one_hot(samples[first:first + x.shape[0] // S]).reshape(x.shape[0], K, H, W)}
        return Fake()

    params = {"dataset_file": "datasets.lidc", "batch_size": batch, "evaluations": evaluations, "output_path": None}
    plain = E.eval_lidc_uncertainty(dict(params), dataset=DS(), device="cpu", model=fake())
    assert set(plain) == {"evaluations", "GED", "diversity_samples", "diversity_experts", "HM_IoU", "IoU", "mIoU", "Dice", "nonzero", "images",
                          "world_size"}
    for section in ({}, {"detection": False}, {"detection": False, "detection_max_candidates": 0, "detection_score": "mass"}):
        res = E.eval_lidc_uncertainty({**params, "evaluation": section}, dataset=DS(), device="cpu", model=fake())
        assert json.dumps(res, sort_keys=True) == json.dumps(plain, sort_keys=True)
    # with the key the values are checked before the first batch; there is no CPU path behind them
    for bad, key in (({"detection_min_frequency": 2}, "detection_min_frequency"), ({"detection_rater_agreement": 5}, "detection_rater_agreement"),
                     ({"detection_score": "mass"}, "detection_score"), ({"detection_fp_rates": [-1]}, "detection_fp_rates"),
                     ({"detection_max_candidates": 0}, "detection_max_candidates"), ({"lesion_connectivity": 6}, "lesion_connectivity")):
        model = fake()
        with pytest.raises(ValueError, match=key):
            E.eval_lidc_uncertainty({**params, "evaluation": {"detection": True, **bad}}, dataset=DS(), device="cpu", model=model)
        assert model.calls == 0
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):
        E.eval_lidc_uncertainty({**params, "evaluation": {"detection": True}}, dataset=DS(), device="cpu", model=fake())


# ------------------------------------------------------------------------------------------------ CPU: ABI
def workspace_formula(B, S, L, H, W, K, cap):
    # int32 labels of two masks, the n plane, the two masks; a byte per candidate and group of 8 samples or 8 raters
    return B * len(U.scored_classes(K)) * (11 * H * W + (-(-S // 8) - (-L // 8)) * cap)


def test_findings_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    assert "ccdm_findings_workspace_bytes(B,S,L,H,W,K,cap) = B*C*(11*H*W + G*cap) bytes" in hdr and "1 <= cap <= 1024" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ccdm_findings[a-z0-9_]*)\s*\(([^;]*)\)\s*;", hdr)}
    assert set(decl) == SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_findings")}
    for name, args in decl.items():
        assert len(hip.SIGNATURES[name][1]) == len(args.split(",")), name
        assert not name.startswith(("ccdm_lesions", "ccdm_lesion_match", "ccdm_lidc", "ccdm_surfdist", "ccdm_seg_", "ccdm_segcalib",
                                    "ccdm_segboundary", "ccdm_contourf", "ccdm_uncscore", "ccdm_css", "ccdm_vote_"))
    assert len(hip.SIGNATURES["ccdm_findings"][1]) == 19 and len(hip.SIGNATURES["ccdm_findings_workspace_bytes"][1]) == 7
    assert "ccdm_findings.hip" in hip.SOURCES and os.path.exists(os.path.join(hip.CSRC, "ccdm_findings.hip"))
    assert hip.ABI_VERSION == 11
    import __graft_entry__ as g
    g.build()
    lib = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ccdm_version() == 11
    assert lib.ccdm_findings_workspace_bytes(16, 100, 4, 128, 128, 2, 64) == 16 * (11 * 16384 + 14 * 64) == workspace_formula(16, 100, 4, 128, 128, 2, 64)
    assert lib.ccdm_findings_workspace_bytes(3, 9, 0, 5, 7, 4, 8) == 3 * 3 * (11 * 35 + 2 * 8) == workspace_formula(3, 9, 0, 5, 7, 4, 8)
    assert lib.ccdm_findings_workspace_bytes(3, 8, 255, 5, 7, 1, 1) == 3 * (11 * 35 + 33) == workspace_formula(3, 8, 255, 5, 7, 1, 1)
    assert lib.ccdm_findings_workspace_bytes(0, 3, 2, 5, 7, 2, 8) == 0 and lib.ccdm_findings_workspace_bytes(1, 3, 2, 5, 0, 2, 8) == 0


def test_findings_refuses_what_it_cannot_score():
    """the limits are checked before anything is launched or read: host buffers stand in for the device's, and nothing is written"""
    lib = hip.load()
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data

    def call(B=1, S=3, L=2, H=8, W=8, K=2, conn=8, n_min=1, m_min=1, cap=8, samples=p, raters=p, counts=p, cand=p, ref=p, conf=p, ws=p,
             ws_bytes=buf.nbytes):
        return lib.ccdm_findings(samples, raters, B, S, L, H, W, K, conn, n_min, m_min, cap, counts, cand, ref, conf, ws, ws_bytes, None)

    need = workspace_formula(1, 3, 2, 8, 8, 2, 8)
    for change, what in ((dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(S=0), "S=0"), (dict(S=256), "S=256"), (dict(L=-1), "L=-1"),
                         (dict(L=256), "L=256"), (dict(W=0), "W=0"), (dict(H=0), "H=0"), (dict(H=128, W=129), "H*W=16512"),
                         (dict(H=1, W=16385), "H*W=16385"), (dict(conn=6), "connectivity=6"), (dict(n_min=0), "n_min=0"),
                         (dict(n_min=4), "n_min=4"), (dict(m_min=0), "m_min=0"), (dict(m_min=3), "m_min=3"), (dict(cap=0), "cap=0"),
                         (dict(cap=1025), "cap=1025"), (dict(B=-1), "B=-1"), (dict(B=0, K=33), "K=33"), (dict(B=0, cap=0), "cap=0"),
                         (dict(raters=None), "raters null with L=2"), (dict(L=0), "raters given with L=0"), (dict(samples=None), "null"),
                         (dict(counts=None), "null"), (dict(cand=None), "null"), (dict(ref=None), "null"), (dict(ws=None), "workspace"),
                         (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes, {need} needed"),
                         (dict(H=129, W=127, ws_bytes=workspace_formula(1, 3, 2, 129, 127, 2, 8) - 1), f"{workspace_formula(1, 3, 2, 129, 127, 2, 8)} needed"),
                         (dict(ws=p + 2), "4-byte aligned")):
        rc = call(**change)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "findings")
    assert not buf.any()
    # B = 0: nothing launched, nothing written; m_min is ignored without raters
    assert call(B=0) == 0 and call(B=0, ws=None, ws_bytes=0) == 0 and call(B=0, L=0, raters=None, m_min=-5) == 0 and not buf.any()


# ------------------------------------------------------------------------------------------------ GPU: the kernels
GUARD = 64


def kernel(samples: torch.Tensor, raters, K: int, connectivity: int, n_min: int, m_min: int, cap: int, want_map: bool = True):
    """one ccdm_findings call on uint8 device stacks (as they lie in memory) -> the dict of host arrays.  Every output and the workspace
    start from a non-zero fill and carry GUARD sentinel elements behind them, which have to survive."""
    lib = hip.load()
    assert samples.is_cuda and samples.dtype == torch.uint8 and samples.is_contiguous()
    B, S, H, W = samples.shape
    L = 0 if raters is None else raters.shape[1]
    Cn = len(U.scored_classes(K))
    need = int(lib.ccdm_findings_workspace_bytes(B, S, L, H, W, K, cap))
    assert need == workspace_formula(B, S, L, H, W, K, cap)
    sizes = {"counts": B * Cn * 2, "candidates": B * Cn * cap * 12, "references": B * Cn * cap * 4, "ws": (need + 3) // 4}
    bufs = {k: torch.full((n + GUARD,), -77, dtype=torch.int32, device="cuda") for k, n in sizes.items()}
    conf = torch.full((B * Cn * H * W + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    hip.check(lib.ccdm_findings(samples.data_ptr(), None if raters is None else raters.data_ptr(), B, S, L, H, W, K, connectivity, n_min, m_min,
                                cap, bufs["counts"].data_ptr(), bufs["candidates"].data_ptr(), bufs["references"].data_ptr(),
                                conf.data_ptr() if want_map else None, bufs["ws"].data_ptr(), need, None), "findings")
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((bufs[k][n:] == -77).all()), f"guard behind {k}"
    assert bool((conf[B * Cn * H * W:] == 0xA5).all()), "guard behind conf_map"
    if not want_map:
        assert bool((conf == 0xA5).all())
    host = {k: bufs[k][:sizes[k]].cpu().numpy().astype(np.int64) for k in ARRAYS}
    labels = bufs["ws"][:B * Cn * 2 * H * W].cpu().numpy().reshape(B, Cn, 2, H, W)
    return {"counts": host["counts"].reshape(B, Cn, 2), "candidates": host["candidates"].reshape(B, Cn, cap, 12),
            "references": host["references"].reshape(B, Cn, cap, 4), "confidence_map": conf[:B * Cn * H * W].cpu().numpy().reshape(B, Cn, H, W),
            "labels": labels}


def assert_findings_equal(got, want, tag="", keys=ARRAYS + ("confidence_map", "labels")):
    counts = want["counts"]
    print(f"findings[{tag}] candidates {counts[..., 0].ravel().tolist()} reference lesions {counts[..., 1].ravel().tolist()} "
          f"supports {sorted(set(want['candidates'][..., 1].ravel().tolist()) - {0})}")
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{tag}: {k}")
    for b, ci in np.ndindex(*counts.shape[:2]):                       # rows beyond the count are zero; support >= peak >= n_min
        rows = got["candidates"][b, ci]
        n = int(counts[b, ci, 0])
        assert not rows[n:].any() and not got["references"][b, ci, int(counts[b, ci, 1]):].any()
        assert (rows[:n, 1] >= rows[:n, 2]).all() and (rows[:n, 2] >= want["n_min"]).all()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,L,H,W,K,connectivity", SHAPES)
def test_findings_equal_the_restatement(B, S, L, H, W, K, connectivity):
    samples, raters = U.lesion_like_case(B, S, L, H, W, K)
    n_min, m_min = U.default_thresholds(S, L)
    want = U.lesion_like_findings((B, S, L, H, W, K), connectivity, CAP)
    got = kernel(_dev(samples), _dev(raters), K, connectivity, n_min, m_min, CAP)
    assert_findings_equal(got, want, f"{(B, S, L, H, W, K)} conn {connectivity}")
    again = kernel(_dev(samples), _dev(raters), K, connectivity, n_min, m_min, CAP)
    for k in got:
        np.testing.assert_array_equal(got[k], again[k], err_msg=k)   # two calls are bit-identical
    other = 12 - connectivity
    want_other = U.lesion_like_findings((B, S, L, H, W, K), other, CAP)
    assert_findings_equal(kernel(_dev(samples), _dev(raters), K, other, n_min, m_min, CAP, want_map=False), want_other, f"conn {other}", ARRAYS)
    # other thresholds: every sample has to agree, any rater suffices
    strict = U.findings_restatement(samples, raters, K, S, 1, connectivity, CAP)
    assert_findings_equal(kernel(_dev(samples), _dev(raters), K, connectivity, S, 1, CAP), strict, "n_min = S, m_min = 1")
    if S == 255:                                                      # the most records: the tables take more than 48 KB of LDS
        wide = U.findings_restatement(samples, raters, K, n_min, m_min, connectivity, 1024)
        assert_findings_equal(kernel(_dev(samples), _dev(raters), K, connectivity, n_min, m_min, 1024), wide, "cap 1024")


@pytest.mark.gpu
def test_unaligned_base_pointers():
    """W % 4 == 0 but the stacks start one byte off a dword: the counting stage takes bytes, on either stack or both"""
    B, S, L, H, W, K, connectivity = SHAPES[0]
    samples, raters = U.lesion_like_case(B, S, L, H, W, K)
    n_min, m_min = U.default_thresholds(S, L)
    want = U.lesion_like_findings((B, S, L, H, W, K), connectivity, CAP)
    s_buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    r_buf = torch.zeros(raters.size + 1, dtype=torch.uint8, device="cuda")
    s_off, r_off = s_buf[1:].view(B, S, H, W), r_buf[1:].view(B, L, H, W)
    s_off.copy_(_dev(samples)); r_off.copy_(_dev(raters))
    assert s_off.data_ptr() % 4 == 1 and r_off.data_ptr() % 4 == 1 and W % 4 == 0
    for s_t, r_t in ((s_off, r_off), (s_off, _dev(raters)), (_dev(samples), r_off)):
        assert_findings_equal(kernel(s_t, r_t, K, connectivity, n_min, m_min, CAP), want, "unaligned")


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", U.HAND_MAPS)
def test_hand_made_maps(name, connectivity):
    samples, raters = U.hand_case(name)
    m = U.hand_map(name)
    n = U.scipy_labels(m > 0, connectivity)[1]
    cap = 128
    for n_min, m_min in ((2, 1), (1, 2), (3, 2)):
        want = U.findings_restatement(samples, raters, 2, n_min, m_min, connectivity, cap)
        got = kernel(_dev(samples), _dev(raters), 2, connectivity, n_min, m_min, cap)
        assert_findings_equal(got, want, f"{name} conn {connectivity} n_min {n_min} m_min {m_min}")
        if n_min == 2:                                                # two of the three samples hold the map itself: A is the map
            np.testing.assert_array_equal(got["labels"][0, 0, 0], U.scipy_labels(m > 0, connectivity)[0])
            assert got["counts"][0, 0, 0] == n
    expect = {"empty": (0, 0), "full": (1, 1), "checkerboard": (128, 1), "spiral": (1, 1), "u_last_row": (2, 2), "diagonal": (5, 2)}[name]
    assert n == expect[0 if connectivity == 4 else 1], (name, n)


@pytest.mark.gpu
def test_more_candidates_than_cap():
    samples, raters = U.hand_case("checkerboard")
    want = U.findings_restatement(samples, raters, 2, 2, 1, 4, 128)
    assert want["counts"].tolist() == [[[128, 128]]]                  # shifted by two columns the board is itself: R is the board too
    got = kernel(_dev(samples), _dev(raters), 2, 4, 2, 1, 128)
    assert_findings_equal(got, want, "checkerboard at cap 128")
    small = kernel(_dev(samples), _dev(raters), 2, 4, 2, 1, 64)       # the guards hold, the counts are true
    assert small["counts"].tolist() == [[[128, 128]]]
    with pytest.raises(hip.CcdmHipError, match="128 candidates.*max_candidates=128 needed"):
        M.sample_findings(_dev(samples), _dev(raters), 2, n_min=2, m_min=1, connectivity=4, max_candidates=64)
    ok = M.sample_findings(_dev(samples), _dev(raters), 2, n_min=2, m_min=1, connectivity=4, max_candidates=128)
    np.testing.assert_array_equal(ok["candidates"], want["candidates"])


@pytest.mark.gpu
def test_sample_findings_takes_index_maps():
    B, S, L, H, W, K, connectivity = SHAPES[0]
    samples, raters = U.lesion_like_case(B, S, L, H, W, K)
    n_min, m_min = U.default_thresholds(S, L)
    want = U.lesion_like_findings((B, S, L, H, W, K), connectivity, CAP)
    s64, r64 = torch.from_numpy(samples.astype(np.int64)).cuda(), torch.from_numpy(raters.astype(np.int64)).cuda()
    got = M.sample_findings(s64, r64, K, n_min=n_min, max_candidates=CAP, return_map=True)       # m_min: a majority by default
    assert set(got) == set(ARRAYS) | {"samples", "raters", "n_min", "m_min", "connectivity", "classes", "max_candidates", "confidence_map"}
    for k in ARRAYS:
        assert got[k].dtype == np.int64
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("samples", "raters", "n_min", "m_min", "connectivity", "classes", "max_candidates"):
        assert got[k] == want[k], k
    conf = got["confidence_map"]
    assert conf.is_cuda and conf.dtype == torch.uint8 and conf.shape == (B, K - 1, H, W)
    np.testing.assert_array_equal(conf.cpu().numpy(), want["confidence_map"])
    # conf_map is the support painted over the labels
    painted = np.zeros_like(want["confidence_map"])
    for b, ci in np.ndindex(B, K - 1):
        for i in range(int(want["counts"][b, ci, 0])):
            painted[b, ci][want["labels"][b, ci, 0] == i + 1] = got["candidates"][b, ci, i, 1]
    np.testing.assert_array_equal(conf.cpu().numpy(), painted)
    sliced = M.sample_findings(s64[:, :3], None, K, n_min=1, connectivity=4, max_candidates=CAP)          # the evaluator's pred_idx[:, :s]
    assert "confidence_map" not in sliced and sliced["raters"] == 0 and sliced["m_min"] is None
    want3 = U.findings_restatement(samples[:, :3], None, K, 1, None, 4, CAP)
    for k in ARRAYS:
        np.testing.assert_array_equal(sliced[k], want3[k], err_msg=k)
    assert not sliced["references"].any() and not sliced["counts"][..., 1].any()
    scores = M.detection_scores_from_findings(M.concat_findings([got, got]))
    assert scores["images"] == 2 * B and scores["per_class"][0]["reference_lesions"] == 2 * int(want["counts"][..., 1].sum())
    with pytest.raises(ValueError, match="expected"):
        M.sample_findings(s64[:, :, :8], r64, K, n_min=1)
    with pytest.raises(hip.CcdmHipError, match="n_min=6"):
        M.sample_findings(s64, r64, K, n_min=6)
    with pytest.raises(hip.CcdmHipError, match="cap=1025"):
        M.sample_findings(s64, r64, K, n_min=1, max_candidates=1025)


# ------------------------------------------------------------------------------------------------ GPU: the sampler
@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5])
def test_predict_findings_on_the_small_model(K):
    from tests import sampler_util
    B, S = 2, 5
    H, W, DEV = sampler_util.H, sampler_util.W, sampler_util.DEV
    model, _ = sampler_util.small_model(K)
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, True
    rng = np.random.default_rng(17)
    cond = torch.from_numpy(rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)).to(DEV)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (S, B, H, W))), K).permute(0, 1, 4, 2, 3).float().to(DEV)
    flat = x.transpose(0, 1).reshape(B * S, K, H, W)
    model.philox_call = 2
    before = model(flat, cond.repeat_interleave(S, dim=0))["diffusion_out"]
    assert model.philox_call == 3
    out = model.predict_findings(cond, num_evaluations=S, min_frequency=0.3, x=x, max_candidates=1024)
    assert model.philox_call == 4 and model.step_T_sample == "majority"      # advanced like one call
    assert set(out) == {"counts", "candidates", "confidence_map", "samples", "n_min", "classes"}
    assert out["n_min"] == 2 and out["classes"] == list(range(1, K))          # ceil(0.3 * 5), the decimal as written
    assert out["samples"].shape == (B, S, H, W) and out["samples"].dtype == torch.uint8 and out["confidence_map"].shape == (B, K - 1, H, W)
    model.philox_call = 3
    ref = model(flat, cond.repeat_interleave(S, dim=0))["diffusion_out"]
    assert torch.equal(out["samples"].long(), ref.argmax(dim=1).reshape(B, S, H, W))
    want = M.sample_findings(out["samples"], None, K, n_min=2, max_candidates=1024, return_map=True)
    np.testing.assert_array_equal(out["counts"], want["counts"])
    np.testing.assert_array_equal(out["candidates"], want["candidates"])
    assert torch.equal(out["confidence_map"], want["confidence_map"])
    by_definition = U.findings_restatement(out["samples"].cpu().numpy(), None, K, 2, None, 8, 1024)
    np.testing.assert_array_equal(out["counts"], by_definition["counts"])
    np.testing.assert_array_equal(out["candidates"], by_definition["candidates"])
    print(f"predict_findings K={K}: candidates {out['counts'][..., 0].tolist()}")
    # a plain call before and after is what it is without the findings call in between
    model.philox_call = 2
    assert torch.equal(model(flat, cond.repeat_interleave(S, dim=0))["diffusion_out"], before)
    # the guidance keywords are handed through: temperature 1 is no shaping
    model.philox_call = 3
    same = model.predict_findings(cond, num_evaluations=S, min_frequency=0.3, x=x, max_candidates=1024, temperature=1.0)
    assert torch.equal(same["samples"], out["samples"])
    model.philox_call = 3
    colder = model.predict_findings(cond, num_evaluations=S, min_frequency=0.3, x=x, max_candidates=1024, temperature=0.25)
    assert colder["samples"].shape == out["samples"].shape and model.philox_call == 4
    for kw, name in ((dict(num_evaluations=256), "num_evaluations"), (dict(min_frequency=1.5), "min_frequency"), (dict(connectivity=6), "connectivity"),
                     (dict(max_candidates=1025), "max_candidates"), (dict(temperature=-1.0), "temperature")):
        args = dict(num_evaluations=S)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            model.predict_findings(cond, **args)
    assert model.philox_call == 4                                     # a refused call draws nothing


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_detection_end_to_end(tmp_path):
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
    assert not (tmp_path / "out").exists()
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"detection": True}}, dataset=DS(), device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"detection"}
    for key, value in plain.items():                                  # everything the evaluator returns today is untouched
        assert res[key] == value, key
    S = max(evaluations)
    pred, lab = [], []
    for call, (image, labels, _) in enumerate(batches):
        p = predict(call, labels.shape[0] * S).reshape(labels.shape[0], S, *labels.shape[2:])
        pred.append(p.argmax(dim=2))
        lab.append(labels.argmax(dim=2))
    pred, lab = torch.cat(pred).numpy().astype(np.uint8), torch.cat(lab).numpy().astype(np.uint8)
    assert len(res["detection"]) == len(evaluations)
    for s, got in zip(evaluations, res["detection"]):
        want = M.detection_scores_from_findings(U.findings_restatement(pred[:, :s], lab, K, 1, 3, 8, 64))
        print(f"detection[{s}] cpm={got['cpm']} ap={got['average_precision']} per class={[(c['candidates'], c['reference_lesions']) for c in got['per_class']]}")
        assert got["samples"] == s and got["images"] == 5 and got["raters"] == 4 and got["n_min"] == 1 and got["m_min"] == 3
        assert got == want
    other = E.eval_lidc_uncertainty({**params, "output_path": None, "evaluation": {
        "detection": True, "detection_min_frequency": 0.5, "detection_rater_agreement": 1, "detection_score": "peak", "detection_fp_rates": [0.5, 2],
        "detection_max_candidates": 128, "lesion_connectivity": 4}}, dataset=DS(), device="cuda:0", model=fake())["detection"]
    want = M.detection_scores_from_findings(U.findings_restatement(pred[:, :3], lab, K, 2, 1, 4, 128), score="peak", fp_rates=[0.5, 2])
    assert other[1] == want and other[1]["n_min"] == 2 and other[1]["m_min"] == 1 and other[1]["connectivity"] == 4 and other[1]["score"] == "peak"
    with open(tmp_path / "out" / "lidc_detection.json") as f:
        assert json.load(f) == res["detection"] == json.loads(json.dumps(res["detection"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_detection.json"]
