"""Metric-optimal consensus of the samples: the kernels ccdm_consensus / ccdm_consensus_maps, metrics.sample_consensus,
DenoisingModel.predict_consensus and the `evaluation.consensus` keys of eval_lidc_uncertainty.  Nothing in the reference computes these.
Everything the kernels write is an integer, so every kernel test asks for equality with the numpy / int64 restatement of the definition
in include/ccdm_hip.h (consensus_util); the expected scores are IEEE float64 quotients of those integers and are asked for exactly too.
No tolerance appears anywhere.  The restatement itself is held against brute force, and the seeded cases are shown on the CPU to
exercise what they are there for (a threshold away from the majority's, IoU and Dice disagreeing, the empty map winning, exact ties)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import consensus_util as U
from tests import sampler_util
from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import metrics as M

LIDC_SHAPES = ((3, 7, 9, 11), (2, 16, 12, 13))                   # (B, S, H, W) of lidc_like, seeds 0..7 each
LIDC_SEEDS = tuple(range(8))


def lidc_stack(shape):
    """the eight seeded cases of a shape as one stack of 8 B images"""
    return np.concatenate([U.lidc_like(seed, *shape) for seed in LIDC_SEEDS], axis=0)


def foreign_case():
    return U.random_case(3, 1, 6, 5, 7, 5, foreign=3)            # K = 5, S = 6, HW = 35, three bytes that are no class


# ------------------------------------------------------------------------------------------------ CPU: ABI
@pytest.mark.parametrize("symbol,nargs", [("ccdm_consensus", 11), ("ccdm_consensus_maps", 10)])
def test_symbol_declared_bound_and_built(symbol, nargs):
    sampler_util.assert_symbol_declared_bound_and_built(symbol, nargs, "ccdm_consensus.hip")


def test_workspace_symbol_declared_bound_and_built():
    """(a size_t, so by hand)"""
    lib = sampler_util.assert_symbol_declared_bound_and_built("ccdm_consensus", 11, "ccdm_consensus.hip")
    res, args = hip.SIGNATURES["ccdm_consensus_workspace_bytes"]
    assert res is C.c_size_t and args == [C.c_int] * 4 and hasattr(lib, "ccdm_consensus_workspace_bytes")
    assert "size_t ccdm_consensus_workspace_bytes(int B, int S, int HW, int K);" in open(os.path.join(sampler_util.ROOT, "include", "ccdm_hip.h")).read()
    assert lib.ccdm_consensus_workspace_bytes(3, 7, 99, 5) == 3 * 4 * 7 * 8 * 4                # int32 [B][C][S][S+1]
    assert lib.ccdm_consensus_workspace_bytes(2, 255, 1 << 20, 32) == 2 * 31 * 255 * 256 * 4
    assert lib.ccdm_consensus_workspace_bytes(0, 7, 99, 5) == 0


def test_library_refuses_what_it_cannot_score():
    """the limits are checked before anything is launched or read: a host buffer stands in for the device's"""
    lib = hip.load()
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data
    big = 1 << 15

    def consensus(B=1, S=4, HW=16, K=2, a=p, freq=p, curve=p, best=p, ws=p, ws_bytes=big):
        return lib.ccdm_consensus(a, B, S, HW, K, freq, curve, best, ws, ws_bytes, None)

    def maps(B=1, S=4, HW=16, K=2, metric=0, freq=p, best=p, mask=p, label=p):
        return lib.ccdm_consensus_maps(freq, best, B, S, HW, K, metric, mask, label, None)

    need = lib.ccdm_consensus_workspace_bytes(1, 4, 16, 2)
    assert need == 4 * 5 * 4
    for call, change, what in ((consensus, dict(K=1), "K=1"), (consensus, dict(K=33), "K=33"), (consensus, dict(S=0), "S=0"),
                               (consensus, dict(S=256), "S=256"), (consensus, dict(HW=0), "HW=0"), (consensus, dict(B=-1), "B=-1"),
                               (consensus, dict(B=65536), "B=65536"), (consensus, dict(a=None), "samples"), (consensus, dict(freq=None), "freq"),
                               (consensus, dict(curve=None), "curve"), (consensus, dict(best=None), "best"),
                               (consensus, dict(ws=None), "workspace"), (consensus, dict(curve=p + 4), "curve must be 8-byte aligned"),
                               (consensus, dict(ws_bytes=need - 1), f"workspace_bytes={need - 1}"),
                               (maps, dict(K=1), "K=1"), (maps, dict(K=33), "K=33"), (maps, dict(S=0), "S=0"), (maps, dict(S=256), "S=256"),
                               (maps, dict(HW=0), "HW=0"), (maps, dict(B=-1), "B=-1"), (maps, dict(B=65536), "B=65536"),
                               (maps, dict(metric=2), "metric=2"), (maps, dict(freq=None), "freq"), (maps, dict(best=None), "best"),
                               (maps, dict(mask=None, label=None), "mask and label")):
        rc = call(**change)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "consensus")
    assert consensus(B=0) == 0 and maps(B=0) == 0 and not buf.any()                       # B = 0: nothing launched, nothing written


def test_sample_consensus_refuses_bad_arguments():
    a = torch.zeros((1, 4, 5, 7), dtype=torch.uint8)
    for kw, name in ((dict(num_classes=1), "num_classes"), (dict(num_classes=33), "num_classes"), (dict(num_classes=2.0), "num_classes"),
                     (dict(metric="f1"), "metric"), (dict(metric=0), "metric"), (dict(maps=("label", "vote")), "maps")):
        args = dict(num_classes=2)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            M.sample_consensus(a, **args)
    with pytest.raises(ValueError, match="S=256"):
        M.sample_consensus(torch.zeros((1, 256, 2, 2), dtype=torch.uint8), 2)
    with pytest.raises(ValueError, match="S=0"):
        M.sample_consensus(torch.zeros((1, 0, 2, 2), dtype=torch.uint8), 2)
    for bad in (torch.zeros((4, 5, 7), dtype=torch.uint8), torch.zeros((1, 4, 5, 7)), np.zeros((1, 4, 5, 7), dtype=np.uint8)):
        with pytest.raises(ValueError, match="samples_idx"):
            M.sample_consensus(bad, 2)
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):                          # no CPU path, as sample_modes
        M.sample_consensus(a, 2)
    assert M.CONSENSUS_METRICS == ("iou", "dice") and M.CONSENSUS_ONE == 1 << 20 == U.ONE and M.CONSENSUS_MAX_SAMPLES == 255


def test_predict_consensus_refuses_bad_arguments():
    """refused before anything is sampled: no device is needed"""
    model, _ = sampler_util.small_model(2)
    model.philox_call = 5
    cond = torch.zeros((1, 1, sampler_util.H, sampler_util.W))
    for kw, name in ((dict(num_evaluations=0), "num_evaluations"), (dict(num_evaluations=256), "num_evaluations"),
                     (dict(num_evaluations=True), "num_evaluations"), (dict(metric="f1"), "metric"), (dict(maps=("mean",)), "maps")):
        args = dict(num_evaluations=4)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            model.predict_consensus(cond, **args)
    with pytest.raises(TypeError, match="predict_consensus.*guide"):
        model.predict_consensus(cond, num_evaluations=4, guide=1)
    assert model.philox_call == 5                                # a refused call draws nothing


def test_evaluation_key_is_validated():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    assert E.consensus_metric("iou") == "iou" and E.consensus_metric("dice") == "dice"
    for bad in ("IoU", "f1", 0, None, True, ["iou"]):
        with pytest.raises(ValueError, match="consensus_metric"):
            E.consensus_metric(bad)
    assert "consensus_metric" in E.eval_lidc_uncertainty.__doc__ and "lidc_consensus.json" in E.eval_lidc_uncertainty.__doc__


# ------------------------------------------------------------------------------------------------ CPU: the restatement
def test_restatement_equals_brute_force():
    for samples, K in [(lidc_stack(shape), 2) for shape in LIDC_SHAPES] + [(foreign_case(), 5)]:
        B, S = samples.shape[:2]
        want = U.consensus_restatement(samples, K)
        assert int((samples >= K).sum()) == (3 if K == 5 else 0)
        for b in range(B):
            for k in range(1, K):
                assert np.array_equal(want["curve"][b, k - 1], U.curves_brute_force(samples[b].reshape(S, -1), k)), (b, k)
        assert want["curve"].min() >= 0 and want["curve"].max() <= S * U.ONE and want["best"].min() >= 1 and want["best"].max() <= S + 1
        # the masks are nested in j and the label is a class whose mask holds the pixel, or 0
        for m in range(2):
            lab, mask = want["label"][m].astype(np.int64), want["mask"][m]
            held = np.take_along_axis(np.concatenate([np.ones_like(mask[:, :1]), mask], axis=1), lab[:, None], axis=1)[:, 0]
            assert held.all() and ((lab == 0) == (mask.sum(axis=1) == 0)).all()


def test_seeded_cases_exercise_what_they_are_for():
    beats_majority = metrics_differ = 0
    largest_gain = 0.0
    for shape in LIDC_SHAPES:
        S = shape[1]
        want = U.consensus_restatement(lidc_stack(shape), 2)
        curve, best = want["curve"][:, 0], want["best"][:, 0]
        iou_best = np.take_along_axis(curve[:, 0], best[:, :1] - 1, axis=1)[:, 0]
        gain = iou_best - curve[:, 0, S // 2]
        assert (gain >= 0).all()
        beats_majority += int(((best[:, 0] != S // 2 + 1) & (gain > 0)).sum())
        metrics_differ += int((best[:, 0] != best[:, 1]).sum())
        largest_gain = max(largest_gain, float(gain.max()) / (S * U.ONE))
    print(f"lidc_like: {beats_majority} images beat the majority threshold, by up to {largest_gain:.3f} IoU; IoU and Dice disagree in {metrics_differ}")
    assert beats_majority >= 1 and metrics_differ >= 1 and largest_gain > 0.3
    # empty wins: four of eight samples empty, the others one distinct pixel each
    want = U.consensus_restatement(U.empty_wins_case(), 2)
    assert want["best"].tolist() == [[[2, 2]]] and not want["mask"].any() and not want["label"].any()
    assert int(want["curve"][0, 0, 0, 1]) == 4 * U.ONE           # expected IoU 1/2: the four empty samples score 0/0 = 1, the others 0
    assert want["curve"][0, 0, 0, 1] > want["curve"][0, 0, 0, 0] and want["curve"][0, 0, 1, 1] > want["curve"][0, 0, 1, 0]
    # exact ties: identical samples, and empty samples
    one = U.random_case(1, 1, 1, 5, 7, 3)
    want = U.consensus_restatement(np.repeat(one, 6, axis=1), 3)
    assert (want["best"] == 1).all() and (want["curve"][..., 0] == 6 * U.ONE).all()               # expected score exactly 1 at j = 1
    assert np.array_equal(want["label"][0], one[:, 0]) and np.array_equal(want["label"][1], one[:, 0])
    want = U.consensus_restatement(np.zeros((1, 6, 5, 7), dtype=np.uint8), 3)
    assert (want["best"] == 1).all() and (want["curve"] == 6 * U.ONE).all() and not want["label"].any()
    # the label rule: equal n under two masks, and a pixel no mask holds
    want = U.consensus_restatement(U.label_rule_case(), 3)
    assert want["freq"].reshape(2, 4).tolist() == [[2, 1, 4, 0], [2, 3, 0, 1]] and want["best"][0, :, 1].tolist() == [2, 2]
    assert want["mask"][1].reshape(2, 4).tolist() == [[1, 0, 1, 0], [1, 1, 0, 0]] and want["label"][1].reshape(4).tolist() == [1, 2, 1, 0]


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def run_kernels(dev_stack: torch.Tensor, K: int):
    """ccdm_consensus and ccdm_consensus_maps (both metrics) on a device stack uint8 [B,S,HW], every output prefilled with garbage"""
    lib = hip.load()
    B, S, HW = dev_stack.shape
    Cn = K - 1
    freq = torch.full((B, Cn, HW), 201, dtype=torch.uint8, device="cuda")
    curve = torch.full((B, Cn, 2, S + 1), -7, dtype=torch.int64, device="cuda")
    best = torch.full((B, Cn, 2), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.ccdm_consensus_workspace_bytes(B, S, HW, K)
    ws = torch.full((nbytes // 4,), 5, dtype=torch.int32, device="cuda")                # (the call clears its workspace)
    hip.check(lib.ccdm_consensus(dev_stack.data_ptr(), B, S, HW, K, freq.data_ptr(), curve.data_ptr(), best.data_ptr(), ws.data_ptr(), nbytes,
                                 None), "consensus")
    mask = torch.full((2, B, Cn, HW), 201, dtype=torch.uint8, device="cuda")
    label = torch.full((2, B, HW), 201, dtype=torch.uint8, device="cuda")
    for m in range(2):
        hip.check(lib.ccdm_consensus_maps(freq.data_ptr(), best.data_ptr(), B, S, HW, K, m, mask[m].data_ptr(), label[m].data_ptr(), None),
                  "consensus_maps")
    torch.cuda.synchronize()
    return {"freq": freq, "curve": curve, "best": best, "mask": mask, "label": label}


def check_exact(samples: np.ndarray, K: int, tag="", dev_stack=None):
    """the kernels on the device against the restatement: every integer equal"""
    B, S, H, W = samples.shape
    if dev_stack is None:
        dev_stack = torch.from_numpy(np.array(samples)).cuda().reshape(B, S, H * W)
    got = run_kernels(dev_stack, K)
    want = U.consensus_restatement(np.asarray(samples), K)
    bad = {k: int((got[k].cpu().long().reshape(-1) != torch.from_numpy(want[k].astype(np.int64)).reshape(-1)).sum()) for k in want}
    print(f"consensus[{tag} {samples.shape} K={K}] best={want['best'].reshape(-1, 2)[:6].tolist()} mismatches={bad}")
    for k in want:
        assert got[k].numel() == want[k].size, k
        assert torch.equal(got[k].cpu().long().reshape(-1), torch.from_numpy(want[k].astype(np.int64)).reshape(-1)), k
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LIDC_SHAPES)
def test_lidc_like_cases(shape):
    check_exact(lidc_stack(shape), 2, tag="lidc_like")


@pytest.mark.gpu
def test_bytes_that_are_no_class():
    check_exact(foreign_case(), 5, tag="foreign bytes")


@pytest.mark.gpu
def test_empty_wins_and_exact_ties():
    got, _ = check_exact(U.empty_wins_case(), 2, tag="empty wins")
    assert got["best"].cpu().tolist() == [[[2, 2]]] and not bool(got["mask"].any()) and int(got["curve"][0, 0, 0, 1]) == 4 * U.ONE
    one = U.random_case(1, 1, 1, 5, 7, 3)
    got, _ = check_exact(np.repeat(one, 6, axis=1), 3, tag="identical")
    assert bool((got["best"] == 1).all()) and bool((got["curve"][..., 0] == 6 * U.ONE).all())
    got, _ = check_exact(np.zeros((1, 6, 5, 7), dtype=np.uint8), 3, tag="all empty")
    assert bool((got["best"] == 1).all()) and bool((got["curve"] == 6 * U.ONE).all())


# S = 1; S = 255 at HW = 33: sixteen groups of samples, the byte path, a pixel every sample marks (n = 255); HW = 128 x 128: sixteen pixel
# shares merged by the global atomics; K = 20: the 32-counter path; S = 33: a last group of one sample; S = 111 at HW = 36: one chunk
@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H,W,K", [(2, 1, 5, 7, 3), (2, 255, 3, 11, 3), (1, 4, 128, 128, 2), (3, 5, 8, 8, 20), (1, 33, 5, 7, 2),
                                       (1, 111, 6, 6, 2)])
def test_random_maps(B, S, H, W, K):
    a = np.array(U.random_case(7 * S + H, B, S, H, W, K))
    a[:, :, 0, 0] = 1
    check_exact(a, K, tag="random")


@pytest.mark.gpu
def test_unaligned_stack_and_two_calls():
    """the stack starts one byte off a dword with HW % 4 == 0: the byte loads; two identical calls are bit-identical"""
    B, S, H, W, K = 2, 17, 8, 8, 3
    samples = U.random_case(11, B, S, H, W, K)
    buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    dev = buf[1:].view(B, S, H * W)
    dev.copy_(torch.from_numpy(np.array(samples)).reshape(B, S, H * W))
    assert dev.data_ptr() % 4 == 1
    got, _ = check_exact(samples, K, tag="unaligned", dev_stack=dev)
    again = run_kernels(dev, K)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.gpu
def test_label_rules_on_constructed_planes():
    """ccdm_consensus_maps on planes and thresholds given by hand: K = 3, S = 4, HW = 5"""
    lib = hip.load()
    freq = torch.tensor([[[2, 1, 4, 0, 3], [2, 3, 0, 1, 4]]], dtype=torch.uint8, device="cuda")
    for best, mask, label in (([2, 2], [[1, 0, 1, 0, 1], [1, 1, 0, 0, 1]], [1, 2, 1, 0, 2]),      # pixel 0: equal n under both masks: class 1
                              ([5, 2], [[0, 0, 0, 0, 0], [1, 1, 0, 0, 1]], [2, 2, 0, 0, 2]),      # class 1 reports the empty map
                              ([1, 5], [[1, 1, 1, 0, 1], [0, 0, 0, 0, 0]], [1, 1, 1, 0, 1])):
        thr = torch.tensor([[[best[0], 9], [best[1], 9]]], dtype=torch.int32, device="cuda")
        m = torch.full((1, 2, 5), 201, dtype=torch.uint8, device="cuda")
        lab = torch.full((1, 5), 201, dtype=torch.uint8, device="cuda")
        hip.check(lib.ccdm_consensus_maps(freq.data_ptr(), thr.data_ptr(), 1, 4, 5, 3, 0, m.data_ptr(), lab.data_ptr(), None), "consensus_maps")
        assert m.cpu().tolist() == [mask] and lab.cpu().tolist() == [label]
        only = torch.full((1, 5), 201, dtype=torch.uint8, device="cuda")                 # either output alone
        hip.check(lib.ccdm_consensus_maps(freq.data_ptr(), thr.data_ptr(), 1, 4, 5, 3, 0, None, only.data_ptr(), None), "consensus_maps")
        assert torch.equal(only, lab)
    got, want = check_exact(U.label_rule_case(), 3, tag="label rule")
    assert got["label"][1].cpu().tolist() == [[1, 2, 1, 0]]
    got, _ = check_exact(lidc_stack(LIDC_SHAPES[0])[:3], 2, tag="K = 2")
    assert torch.equal(got["label"].reshape(-1), got["mask"].reshape(-1))               # K = 2: the label is the mask


# ------------------------------------------------------------------------------------------------ GPU: the host function
@pytest.mark.gpu
@pytest.mark.parametrize("metric", M.CONSENSUS_METRICS)
def test_sample_consensus_returns_the_restatement(metric):
    B, S, H, W, K = 3, 5, 8, 8, 20
    samples = U.random_case(41, B, S, H, W, K)
    want = U.consensus_restatement(samples, K)
    m = M.CONSENSUS_METRICS.index(metric)
    got = M.sample_consensus(torch.from_numpy(samples.astype(np.int64)).cuda(), K, metric=metric, maps=("label", "mask"))
    assert set(got) == {"threshold", "thresholds", "curve", "expected", "expected_majority", "frequency", "label", "mask"}
    for key, ref, dtype in (("thresholds", want["best"], torch.int32), ("threshold", want["best"][:, :, m], torch.int32),
                            ("curve", want["curve"], torch.int64), ("frequency", want["freq"], torch.uint8), ("label", want["label"][m], torch.uint8),
                            ("mask", want["mask"][m], torch.uint8)):
        assert got[key].dtype == dtype and tuple(got[key].shape) == ref.shape, key
        assert torch.equal(got[key].cpu().long(), torch.from_numpy(ref.astype(np.int64))), key
    at_best = np.take_along_axis(want["curve"][:, :, m], want["best"][:, :, m, None] - 1, axis=2)[:, :, 0]
    for key, num in (("expected", at_best), ("expected_majority", want["curve"][:, :, m, S // 2])):
        assert got[key].dtype == torch.float64 and got[key].device.type == "cuda"
        assert np.array_equal(got[key].cpu().numpy(), num.astype(np.float64) / float(S * U.ONE)), key
    assert bool((got["expected"] >= got["expected_majority"]).all())
    plain = M.sample_consensus(torch.from_numpy(np.array(samples)).cuda()[:, :4], K, metric=metric)          # the evaluator's pred_idx[:, :s]
    assert set(plain) == set(got) - {"mask"}
    assert torch.equal(plain["label"].cpu().long(), torch.from_numpy(U.consensus_restatement(samples[:, :4], K)["label"][m].astype(np.int64)))
    assert set(M.sample_consensus(torch.from_numpy(np.array(samples)).cuda(), K, maps=())) == set(got) - {"mask", "label"}


# ------------------------------------------------------------------------------------------------ GPU: the sampler
@pytest.mark.gpu
def test_predict_consensus_on_the_small_model():
    K, B, S = 2, 2, 5
    H, W, DEV = sampler_util.H, sampler_util.W, sampler_util.DEV
    model, _ = sampler_util.small_model(K)
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, True
    rng = np.random.default_rng(17)
    cond = torch.from_numpy(rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)).to(DEV)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (S, B, H, W))), K).permute(0, 1, 4, 2, 3).float().to(DEV)
    flat = x.transpose(0, 1).reshape(B * S, K, H, W)
    model.philox_call = 3
    after_modes = model.predict_modes(cond, num_evaluations=S, modes=1, x=x, maps=())
    plain_after_modes = model(flat, cond.repeat_interleave(S, dim=0))["diffusion_out"]
    model.philox_call = 3
    out = model.predict_consensus(cond, num_evaluations=S, x=x, maps=("label", "mask"))
    assert model.philox_call == 4                                # advanced like one call
    assert model.step_T_sample == "majority"
    plain = model(flat, cond.repeat_interleave(S, dim=0))["diffusion_out"]
    assert model.philox_call == 5 and torch.equal(plain, plain_after_modes)          # the call after it draws what it would have drawn
    assert out["samples"].shape == (B, S, H, W) and out["samples"].dtype == torch.uint8
    assert torch.equal(out["samples"], after_modes["samples"])                       # the same counter state, the same samples
    want = M.sample_consensus(out["samples"], K, maps=("label", "mask"))
    assert set(out) == set(want) | {"samples"}
    for k, v in want.items():
        assert torch.equal(out[k], v), k
    ref = U.consensus_restatement(out["samples"].cpu().numpy(), K)
    assert torch.equal(out["label"].cpu().long(), torch.from_numpy(ref["label"][0].astype(np.int64)))
    print(f"predict_consensus: thresholds {out['thresholds'].cpu().tolist()} expected {out['expected'].cpu().tolist()}")
    model.philox_call = 3
    dice = model.predict_consensus(cond, num_evaluations=S, x=x, metric="dice", maps=())
    assert torch.equal(dice["samples"], out["samples"]) and torch.equal(dice["threshold"], out["thresholds"][:, :, 1]) and "label" not in dice
    model.philox_call = 3
    cool = model.predict_consensus(cond, num_evaluations=S, x=x, temperature=0.5)        # the guidance keywords pass through
    model.philox_call = 3
    cool_modes = model.predict_modes(cond, num_evaluations=S, modes=1, x=x, maps=(), temperature=0.5)
    assert torch.equal(cool["samples"], cool_modes["samples"]) and model.philox_call == 4


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_consensus_end_to_end(tmp_path):
    """the evaluator with fixed predictions (its maps come from the device, so it needs one)"""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    K, H, W, evaluations, batch = 2, 13, 11, [2, 4], 2
    S = max(evaluations)
    samples = U.lidc_like(6, 3, S, H, W)                         # 3 images in batches of 2: the last batch holds one
    raters = U.lidc_like(7, 3, 4, H, W)
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
    assert not (tmp_path / "out").exists()
    for metric in M.CONSENSUS_METRICS:
        section = {"consensus": True} if metric == "iou" else {"consensus": True, "consensus_metric": metric}      # iou is the default
        res = E.eval_lidc_uncertainty({**params, "evaluation": section}, dataset=DS(), device="cuda:0", model=fake())
        assert set(res) == set(plain) | {"consensus"}
        for key, value in plain.items():                         # everything the evaluator returns today is untouched
            assert res[key] == value, key
        assert len(res["consensus"]) == len(evaluations)
        m = M.CONSENSUS_METRICS.index(metric)
        for s, got in zip(evaluations, res["consensus"]):
            print(f"consensus[{s}, {metric}] got={got}")
            assert set(got) == {"samples", "images", "metric", "iou_consensus", "dice_consensus", "iou_majority", "dice_majority", "expected",
                                "expected_majority", "threshold_share"}
            assert got["samples"] == s and got["images"] == 3 and got["metric"] == metric
            want = U.consensus_restatement(samples[:, :s], K)
            major = np.stack([U.maps_restatement(want["freq"][b].reshape(K - 1, -1), np.full(K - 1, s // 2 + 1))[1] for b in range(3)])
            for name, label in (("consensus", want["label"][m]), ("majority", major.reshape(3, H, W))):
                iou, dice = U.rater_scores(label, raters, K)
                assert got[f"iou_{name}"] == float(iou.mean()) and got[f"dice_{name}"] == float(dice.mean()), name
            best = want["best"][:, :, m]
            at_best = np.take_along_axis(want["curve"][:, :, m], best[:, :, None] - 1, axis=2)[:, :, 0]
            assert got["expected"] == float((at_best / float(s * U.ONE)).mean(axis=1).mean())
            assert got["expected_majority"] == float((want["curve"][:, :, m, s // 2] / float(s * U.ONE)).mean(axis=1).mean())
            assert got["threshold_share"] == float((best.astype(np.float64).mean(axis=1) / s).mean())
            assert got["expected"] >= got["expected_majority"]
        with open(tmp_path / "out" / "lidc_consensus.json") as f:
            assert json.load(f) == res["consensus"] == json.loads(json.dumps(res["consensus"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_consensus.json"]
    with pytest.raises(ValueError, match="consensus_metric"):
        E.eval_lidc_uncertainty({**params, "evaluation": {"consensus": True, "consensus_metric": "f1"}, "output_path": None}, dataset=DS(),
                                device="cuda:0", model=fake())
