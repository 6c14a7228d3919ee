"""Temperature and truncation sampling: DenoisingModel(..., temperature=, truncation=) and the fused shape-and-draw step kernel
ccdm_shaped_step (include/ccdm_hip.h has the definition).  The numpy restatement below is the definition in fp32 in front of the evidence
tests' restatement of the step (the oracle's theta_post_prob, cascade normalisation and sample_index on philox_exponential's noise); it is
held against the definition in float64 on the CPU, the kernel is held bit for bit against it wherever no power is formed (the device's
power function is not numpy's: the tempered cases are held against float64 to a counted bound), and the sampler is checked launch by launch
on the device's own inputs, free-running against the oracle's loop, for what must not change without the keywords, and for independence of
the execution shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import guidance, hip
from tests.guided_util import (POWER_ERROR_ALLOWED, SHAPES, TEMPERED_OFF, TEMPERED_ROW, bits, coefficients, evidence_restatement, mixed_inputs, nhwk,
                               random_inputs, sampler_evidence, shape_rows, shaped_restatement, tempered_cases, tempered_reference, threshold_margin64,
                               weighted)
from tests.guided_util import run_shaped_kernel as run_kernel
from tests.ladder_util import LADDER_RS, margin_seed, rung_of, shape_of
from tests.sampler_util import (DEV, H, SEED, SMALL_CFG, T_SMALL, T_STRIDED, W, assert_symbol_declared_bound_and_built, load_lib, make_sampler,
                                onehot_np, sample_sharded_keywords, settings, small_model)

SYMBOL = "ccdm_shaped_step"
T_VALUES = [6, 4, 3, 1]          # t = 10004 walks the small model strided
# the inputs of the definition test (CPU) and of the tempered kernel test: a seed at which no pixel of any shape lies within 1e-5
# (relative) of a truncation threshold at r in {0.9, 0.6}, tau in {1, 0.7, 1.5}, with or without evidence — the CPU test asserts it.
# ladder_util.margin_seed has the seed per shape: 4100 + K at the four shapes the suite began with, a recorded one at the shapes of the
# class-count ladder, where r = 0.5 is held to the same margin.


# ------------------------------------------------------------------------------------------------ CPU
def test_shaped_symbol_declared_bound_and_built():
    """hip.py binds the symbol with argtypes that match the header's declaration (19 arguments), the source is in the build list, the
    library cross-built from it exports it under the unchanged ABI number, and every bad argument is refused before anything is launched
    (host pointers: a launch would fault) with the expected word and the entry's name in the error string."""
    lib = assert_symbol_declared_bound_and_built(SYMBOL, 19, "ccdm_guided.hip")
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    good = dict(x0=p, ev=p, N=1, HW=8, K=2, inv=1.0, r=1.0, a=0.5, c=0.5, mode=hip.STEP_SAMPLE, step_row=0, seed=0, off=0, xt=p, xin=None,
                stride=4, probs=None, onehot=None, stream=None)
    nan, inf = float("nan"), float("inf")
    for change, text in ((dict(N=0), "N=0"), (dict(N=-1), "N=-1"), (dict(HW=0), "HW=0"), (dict(K=0), "K=0"), (dict(K=256), "K=256"),
                         (dict(x0=None), "null"), (dict(xt=None), "null"), (dict(xin=p, stride=1), "xin_stride"),
                         (dict(mode=hip.STEP_SOFTMAX_ONLY), "mode"), (dict(mode=7), "mode"), (dict(mode=-1), "mode"),
                         (dict(step_row=-1), "step_row"), (dict(N=2 ** 31 - 1, HW=2 ** 31 - 1), "too many pixels"),
                         (dict(inv=nan), "inv_temperature"), (dict(inv=inf), "inv_temperature"), (dict(inv=0.049), "inv_temperature"),
                         (dict(inv=20.5), "inv_temperature"), (dict(inv=-1.0), "inv_temperature"), (dict(inv=0.0), "inv_temperature"),
                         (dict(r=nan), "top_r"), (dict(r=inf), "top_r"), (dict(r=0.0), "top_r"), (dict(r=-0.5), "top_r"),
                         (dict(r=1.0000001), "top_r")):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert text in hip.last_error() and SYMBOL in hip.last_error(), (change, hip.last_error())


def test_shaping_keyword_validation():
    """Every refusal of guidance.check_shaping is a ValueError naming the keyword, through forward, forward_denoising and predict_multiple, before
    anything runs (a model that was never moved to a GPU: nothing can run); the accepted forms and what they become."""
    m, _ = small_model(3)
    m.eval()
    N, K = 2, 3
    x = torch.nn.functional.one_hot(torch.zeros((N, H, W), dtype=torch.int64), K).permute(0, 3, 1, 2).float()
    cond = torch.zeros(N, 1, H, W)

    def calls(model):
        return (lambda **kw: model(x, cond, t=T_STRIDED, **kw), lambda **kw: model.forward_denoising(x, cond, None, 10004, **kw),
                lambda **kw: model.predict_multiple(cond, num_evaluations=2, voting="majority", t=T_STRIDED, **kw))
    bad = [("temperature", v) for v in (0.0, 0.049, 20.5, -1.0, float("nan"), float("inf"), "1.0", True, 1 + 0j, torch.tensor(1.0), [1.0])]
    bad += [("truncation", v) for v in (0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), "0.5", True, torch.tensor(0.5), (0.5,))]
    for name, value in bad:
        for call in calls(m):
            with pytest.raises(ValueError, match="^" + name):
                call(**{name: value})
    with pytest.raises(ValueError, match="^truncation"):         # a good temperature does not hide a bad truncation
        m(x, cond, t=T_STRIDED, temperature=1.0, truncation=0.0)
    m.rng = "torch_cpu"
    for name in ("temperature", "truncation"):
        for call in calls(m):
            with pytest.raises(ValueError, match=name + ".*torch_cpu"):
                call(**{name: 0.5})
    m.rng = "philox"
    for name in ("temperature", "truncation"):
        with pytest.raises(ValueError, match=name + ".*sampling call"):
            m(x, cond, t=torch.full((N,), 3.0), validation=True, **{name: 0.5})           # forward_step has no draw to shape
        m.train()
        with pytest.raises(ValueError, match=name + ".*sampling call"):
            m(x, cond, t=torch.full((N,), 3.0), **{name: 0.5})
        with pytest.raises(ValueError, match=name + ".*sampling call"):
            m.forward_denoising(x, cond, None, 10004, **{name: 0.5})
        m.eval()
    logits_model, _ = small_model(3, softmax_output=False)
    logits_model.eval()
    for name in ("temperature", "truncation"):
        for call in calls(logits_model):
            with pytest.raises(ValueError, match=name + ".*softmax_output"):
                call(**{name: 0.5})
    assert m.philox_call == 0 and m._engines == {} and logits_model._engines == {}          # nothing ran
    # the accepted forms: Python ints and floats, numpy scalars, the ends of both ranges; (inv_temperature as fp32, top_r as fp32)
    assert guidance.check_shaping(m, None, None) is None
    assert guidance.check_shaping(m, 1, 1) == (1.0, 1.0) and guidance.check_shaping(m, 1.0, None) == (1.0, 1.0) and guidance.check_shaping(m, None, 1.0) == (1.0, 1.0)
    assert guidance.check_shaping(m, np.float32(0.5), np.float64(0.25)) == (2.0, 0.25) and guidance.check_shaping(m, np.int64(2), np.int32(1)) == (0.5, 1.0)
    assert guidance.check_shaping(m, 20, 1e-6) == (float(np.float32(0.05)), float(np.float32(1e-6))) and guidance.check_shaping(m, 0.05, None) == (20.0, 1.0)
    assert guidance.check_shaping(m, 0.7, 0.9) == (float(np.float32(1.0 / 0.7)), float(np.float32(0.9)))
    # Guidance carries the pair: set means guided, and a repeated batch keeps it
    from ccdm_stochastic_segmentation_amd.models import Guidance
    assert not Guidance() and Guidance(shaping=(1.0, 1.0)) and Guidance(shaping=(2.0, 0.5)).repeat_interleave(3).shaping == (2.0, 0.5)
    assert guidance.check_guidance(m, dict(temperature=0.5), (N, K, H, W)).shaping == (2.0, 1.0)


@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_the_restatement_meets_the_definition(N, HW, K):
    """shape_rows in fp32 against the definition walked class by class in float64 (a Python loop per pixel): the kept sets agree on every
    pixel; in float64 the kept mass reaches r Z and falls below it without the smallest kept class; dropped classes are exactly 0 and
    kept ones bit-unchanged; tau = 1 and r = 1 return the input bits; a tempered row's maximum is exactly 1 (and its entries lie in
    [0,1]).  Also what the kernel tests rely on: the kept sets of these inputs range from one class to nearly all, and no pixel lies
    within 1e-5 (relative) of a truncation threshold (r in {0.9, 0.6}; at the shapes of the class-count ladder r = 0.5 too)."""
    rng = np.random.default_rng(margin_seed(N, HW, K))
    x0, ev, _ = mixed_inputs(rng, N, HW, K)
    sizes, margin = [], np.inf
    for e in (None, ev):
        v = weighted(x0, e)
        assert np.array_equal(bits(shape_rows(v, 1.0, 1.0)), bits(v))
        for tau in (1.0, 0.7, 1.5):
            inv = np.float32(1.0 / tau)
            q = shape_rows(v, inv, 1.0)
            if tau != 1.0:
                assert np.all(q.max(-1) == 1.0) and q.min() >= 0.0
                q64 = shape_rows(v, float(inv), 1.0, np.float64)
                big = q64 > 1e-30
                assert np.abs(q[big] - q64[big]).max() <= 1e-5 * q64[big].max() and np.all((q64 == 0) == (q == 0))
            else:
                assert np.array_equal(bits(q), bits(v))
            for r in (LADDER_RS if (N, HW, K) == shape_of(K) else (0.9, 0.6)):
                out = shape_rows(v, inv, r)
                kept = out != 0
                assert np.array_equal(bits(out[kept]), bits(q[kept])) and np.all(bits(out[~kept & (q != 0)]) == 0)
                q64 = q.astype(np.float64)
                margin = min(margin, float(threshold_margin64(q64, r).min()))
                assert threshold_margin64(q64, r).min() > 1e-5
                r64 = float(np.float32(r))
                for row, keep_row in zip(q64.reshape(-1, K), kept.reshape(-1, K)):
                    theta, cum, mine = r64 * float(np.cumsum(row)[-1]), 0.0, []
                    for k in sorted(range(K), key=lambda k: (-row[k], k)):
                        if cum < theta:
                            mine.append(k)
                        cum += row[k]
                    assert sorted(mine) == list(np.flatnonzero(keep_row)), "the fp32 and the float64 kept sets differ"
                    mass = sum(row[k] for k in mine)
                    assert mass >= theta and mass - row[mine[-1]] < theta and mine[0] == int(np.argmax(row))
                sizes.append(kept.sum(-1))
    sizes = np.concatenate([s.reshape(-1) for s in sizes])
    print(f"K={K} (rung {rung_of(K)}) at ({N}, {HW}): kept sets of {sizes.min()} .. {sizes.max()} classes, the smallest threshold margin {margin:.3e}")
    assert sizes.min() == 1 and sizes.max() >= max(2, (3 * K) // 5)


def test_sample_sharded_hands_temperature_and_truncation_through():
    seen = sample_sharded_keywords(temperature=0.7, truncation=0.9)
    assert seen["temperature"] == 0.7 and seen["truncation"] == 0.9
    seen = sample_sharded_keywords(truncation=0.5)
    assert seen["truncation"] == 0.5 and "temperature" not in seen
    seen = sample_sharded_keywords()
    assert "temperature" not in seen and "truncation" not in seen


def test_the_sampling_params_key_reaches_the_sampling_call():
    """`sampling: {temperature, truncation}` becomes keywords of the model call (one evaluation), of predict_multiple (several) and of
    eval_lidc_uncertainty's sampling call (recording stubs); an unknown key raises; without the key no keyword is added."""
    from ccdm_stochastic_segmentation_amd import evaluation as E

    class Reached(Exception):
        pass

    class Stub:
        step_T_sample = "majority"

        class diffusion:
            num_classes = 2

        def __init__(self):
            self.calls = []

        def __call__(self, x, image, fc=None, **kw):
            self.calls.append(("call", kw))
            return {"diffusion_out": x}

        def predict_multiple(self, image, fc=None, **kw):
            self.calls.append(("multi", kw))
            return {"mean": image}
    image = torch.zeros(2, 1, 8, 8)
    assert E.sampling_keywords({}) == {} and E.sampling_keywords({"sampling": None}) == {} and E.sampling_keywords({"sampling": {}}) == {}
    assert E.sampling_keywords({"sampling": {"temperature": 0.7}}) == {"temperature": 0.7}
    assert E.sampling_keywords({"sampling": {"truncation": 0.9, "temperature": None}}) == {"truncation": 0.9}
    for bad in ({"sampling": {"temperatur": 1.0}}, {"sampling": {"temperature": 1.0, "top_p": 0.9}}, {"sampling": [0.7, 0.9]}):
        with pytest.raises(ValueError, match="sampling"):
            E.sampling_keywords(bad)
        with pytest.raises(ValueError, match="sampling"):
            E.predict_multiple(Stub(), image, bad)
    both = {"sampling": {"temperature": 0.7, "truncation": 0.9}}
    m = Stub()
    E.predict_multiple(m, image, {})
    E.predict_multiple(m, image, both)
    E.predict_multiple(m, image, {"evaluations": 3, "evaluation_vote_strategy": "majority"})
    E.predict_multiple(m, image, {"evaluations": 3, "evaluation_vote_strategy": "majority", "sampling": {"truncation": 0.5}})
    assert [c[0] for c in m.calls] == ["call", "call", "multi", "multi"]
    assert m.calls[0][1] == {} and m.calls[1][1] == both["sampling"]
    assert "temperature" not in m.calls[2][1] and "truncation" not in m.calls[2][1]
    assert m.calls[3][1]["truncation"] == 0.5 and "temperature" not in m.calls[3][1] and m.calls[3][1]["num_evaluations"] == 3

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return torch.zeros(1, 8, 8), torch.nn.functional.one_hot(torch.zeros((4, 8, 8), dtype=torch.int64), 2).permute(0, 3, 1, 2).float(), 0

    class Recorder(Stub):
        def __call__(self, x, image, fc=None, **kw):
            self.calls.append(kw)
            raise Reached()
    params = {"dataset_file": "datasets.lidc", "batch_size": 2, "evaluations": [2]}
    for extra, want in (({}, {}), (both, both["sampling"])):
        rec = Recorder()
        with pytest.raises(Reached):
            E.eval_lidc_uncertainty({**params, **extra}, dataset=DS(), device="cpu", model=rec)
        assert rec.calls == [want]
        rec = Recorder()
        with pytest.raises(Reached):
            E.eval_lidc_uncertainty({**params, **extra}, dataset=DS(), device="cpu", model=rec, init_t=10004)
        assert len(rec.calls) == 1 and {k: v for k, v in rec.calls[0].items() if k != "t"} == want and int(rec.calls[0]["t"]) == 10004
    rec = Recorder()
    with pytest.raises(ValueError, match="sampling"):
        E.eval_lidc_uncertainty({**params, "sampling": {"min_p": 0.1}}, dataset=DS(), device="cpu", model=rec)
    assert rec.calls == []


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run_posterior_sample(lib, rows, xt, a, c, mode, row, off, seed=SEED):
    """ccdm_posterior_sample (softmax = 0) on probability rows [N,HW,K]: (xt_next, out_probs) after the launch"""
    N, HW, K = rows.shape
    table = torch.zeros((row + 1, 4), dtype=torch.float32)
    table[row] = torch.tensor([a, c, float(mode), 0.0])
    d = dict(head=torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), xt=torch.from_numpy(np.asarray(xt).astype(np.uint8)).to(DEV),
             table=table.to(DEV), step=torch.tensor([row], dtype=torch.int32, device=DEV), nxt=torch.zeros((N, HW), dtype=torch.uint8, device=DEV),
             probs=torch.zeros((N, HW, K), dtype=torch.float32, device=DEV), onehot=torch.zeros((N, HW, K), dtype=torch.int64, device=DEV))
    p = hip.PostArgs()
    p.head, p.softmax, p.head_stride = d["head"].data_ptr(), 0, K
    p.xt, p.N, p.HW, p.K = d["xt"].data_ptr(), N, HW, K
    p.step_table, p.step_ptr = d["table"].data_ptr(), d["step"].data_ptr()
    p.philox_seed, p.sample_offset = seed, off
    p.xt_next, p.out_probs, p.out_onehot = d["nxt"].data_ptr(), d["probs"].data_ptr(), d["onehot"].data_ptr()
    hip.check(lib.ccdm_posterior_sample(C.byref(p), 0), "posterior_sample")
    torch.cuda.synchronize()
    return d["nxt"].cpu().numpy(), d["probs"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_truncating_kernel_equals_the_restatement(lib, N, HW, K):
    """tau = 1 (no power is formed), r in {0.9, 0.5}, with and without evidence, STEP_SAMPLE, bit equality: xt and the one-hot channels
    equal the restatement, with and without xin (a stride > K that is no multiple of 4), at two (sample offset, step row) pairs and at a
    high and a low t of a cosine schedule; the image channels >= K of xin, x0 and the evidence are bit-unchanged; sharding."""
    rng = np.random.default_rng(5000 + K)
    stride = (K + 4) // 4 * 4 + 1
    x0, ev_all, xt = mixed_inputs(rng, N, HW, K)
    xin0 = rng.standard_normal((N, HW, stride)).astype(np.float32)
    for r in (0.9, 0.5):
        for ev in (None, ev_all):
            for t in (200, 2):
                a, c = coefficients(t)
                for off, row in ((0, 0), (5, 3)):
                    _, want = shaped_restatement(x0, ev, xt, 1.0, r, a, c, hip.STEP_SAMPLE, row, SEED, off)
                    for with_xin in (True, False):
                        got = run_kernel(lib, x0, ev, xt, 1.0, r, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off,
                                         xin=xin0 if with_xin else None)
                        what = f"r={r} ev={ev is not None} t={t} off={off} row={row} xin={with_xin}"
                        got_xt = got["xt"].astype(np.int64)
                        assert np.array_equal(got_xt, want), what + f": {int((got_xt != want).sum())} of {want.size} pixels differ"
                        assert np.array_equal(bits(got["x0"]), bits(x0)) and (ev is None or np.array_equal(bits(got["ev"]), bits(ev))), what
                        if with_xin:
                            assert np.array_equal(bits(got["xin"][..., K:]), bits(xin0[..., K:])), what + ": an image channel changed"
                            assert np.array_equal(got["xin"][..., :K], onehot_np(want, K).astype(np.float32)), what
            if N > 1:           # samples 1.. of a batch at offset 5 are samples 0.. of a batch at offset 6
                a, c = coefficients(200)
                full = run_kernel(lib, x0, ev, xt, 1.0, r, a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=5)
                tail = run_kernel(lib, x0[1:], None if ev is None else ev[1:], xt[1:], 1.0, r, a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=6)
                assert np.array_equal(full["xt"][1:], tail["xt"])


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_neutral_values_are_the_plain_and_the_evidence_step(lib, N, HW, K):
    """(inv_temperature, top_r) = (1, 1): without evidence the bits of ccdm_posterior_sample (softmax = 0) on the same inputs, with
    evidence those of the numpy evidence restatement — xt, and out_probs in confidence mode with x0 aliased.  ccdm_evidence_step launches
    this kernel at (1, 1), so the two entries are held to agree as well: that guards the entry's wiring, not the arithmetic."""
    rng = np.random.default_rng(6000 + K)
    x0, ev, xt = mixed_inputs(rng, N, HW, K)
    row, off = 3, 5
    for t in (200, 2):
        a, c = coefficients(t)
        got = run_kernel(lib, x0, None, xt, 1.0, 1.0, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off)["xt"]
        assert np.array_equal(got, run_posterior_sample(lib, x0, xt, a, c, hip.STEP_SAMPLE, row, off)[0]), t
        got = run_kernel(lib, x0, None, xt, 1.0, 1.0, a, c, hip.STEP_LAST_CONFIDENCE, step_row=row, sample_offset=off, alias=True)
        assert np.array_equal(bits(got["x0"]), bits(run_posterior_sample(lib, x0, xt, a, c, hip.STEP_LAST_CONFIDENCE, row, off)[1])), t
        assert np.array_equal(got["xt"], xt.astype(np.uint8))
        kw = dict(step_row=row, sample_offset=off)
        probs, idx = evidence_restatement(x0, ev, xt, a, c, hip.STEP_SAMPLE, row, SEED, off)
        got = run_kernel(lib, x0, ev, xt, 1.0, 1.0, a, c, hip.STEP_SAMPLE, **kw)["xt"]
        assert np.array_equal(got.astype(np.int64), idx), f"t={t}: {int((got != idx).sum())} of {idx.size} pixels differ"
        assert np.array_equal(got, run_kernel(lib, x0, ev, xt, 1.0, 1.0, a, c, hip.STEP_SAMPLE, symbol="ccdm_evidence_step", **kw)["xt"]), t
        got = run_kernel(lib, x0, ev, xt, 1.0, 1.0, a, c, hip.STEP_LAST_CONFIDENCE, alias=True, **kw)["x0"]
        assert np.array_equal(bits(got), bits(probs)), f"t={t}: {int((bits(got) != bits(probs)).sum())} probabilities differ"
        assert not np.array_equal(bits(got), bits(x0)), t


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_one_kept_class_is_the_step_on_the_argmax(lib, N, HW, K):
    """top_r = 1e-6 keeps the top class alone (its mass is at least Z / K): the draw is ccdm_posterior_sample's on onehot(argmax v); at
    t = 1 the majority mode returns argmax v."""
    rng = np.random.default_rng(7000 + K)
    x0, ev_all, xt = mixed_inputs(rng, N, HW, K)
    row, off = 2, 1
    for ev in (None, ev_all):
        top = weighted(x0, ev).argmax(-1)
        rows = onehot_np(top, K).astype(np.float32)
        for t in (200, 2):
            a, c = coefficients(t)
            got = run_kernel(lib, x0, ev, xt, 1.0, 1e-6, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off)["xt"]
            assert np.array_equal(got, run_posterior_sample(lib, rows, xt, a, c, hip.STEP_SAMPLE, row, off)[0]), t
        a, c = coefficients(1)
        onehot0 = np.zeros((N, HW, K), dtype=np.int64)
        got = run_kernel(lib, x0, ev, xt, 1.0, 1e-6, a, c, hip.STEP_LAST_MAJORITY, onehot=onehot0, alias=True)
        assert np.array_equal(got["xt"].astype(np.int64), top) and np.array_equal(got["onehot"], onehot_np(top, K).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_shaped_kernel_last_step_modes_with_aliased_x0(lib, N, HW, K):
    """tau = 1, r = 0.5, the three last-step modes with x0 and out_probs the same buffer (as in the engine), bit equality: confidence
    leaves the restated (shaped) probabilities there and xt alone; majority the argmax one-hot in out_onehot, its index in xt, and x0
    alone; keep writes nothing."""
    rng = np.random.default_rng(8000 + K)
    x0, ev_all, xt = mixed_inputs(rng, N, HW, K)
    onehot0 = rng.integers(-5, 5, (N, HW, K))
    for ev in (None, ev_all):
        for t in (1, 3):
            a, c = coefficients(t, T_SMALL)
            probs, idx = shaped_restatement(x0, ev, xt, 1.0, 0.5, a, c, hip.STEP_LAST_MAJORITY, 0, SEED, 0)
            r = run_kernel(lib, x0, ev, xt, 1.0, 0.5, a, c, hip.STEP_LAST_CONFIDENCE, onehot=onehot0, alias=True)
            assert np.array_equal(bits(r["x0"]), bits(probs)), f"t={t}: {int((bits(r['x0']) != bits(probs)).sum())} probabilities differ"
            assert np.array_equal(r["xt"], xt.astype(np.uint8)) and np.array_equal(r["onehot"], onehot0)
            r = run_kernel(lib, x0, ev, xt, 1.0, 0.5, a, c, hip.STEP_LAST_MAJORITY, onehot=onehot0, alias=True, step_row=3, sample_offset=2)
            assert np.array_equal(r["xt"].astype(np.int64), idx) and np.array_equal(r["onehot"], onehot_np(idx, K).astype(np.int64))
            assert r["onehot"].dtype == np.int64 and np.array_equal(bits(r["x0"]), bits(x0))
            r = run_kernel(lib, x0, ev, xt, 1.0, 0.5, a, c, hip.STEP_LAST_KEEP, onehot=onehot0, alias=True)
            assert np.array_equal(r["xt"], xt.astype(np.uint8)) and np.array_equal(r["onehot"], onehot0) and np.array_equal(bits(r["x0"]), bits(x0))


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_tempered_kernel_against_float64(lib, parity_log, N, HW, K):
    """tau in {0.7, 1.5}, r in {1, 0.9}, with and without evidence.  The device forms the power as exp2f(inv_tau * log2f(u)), numpy as
    pow: no bit equality here.
    Confidence mode: the probabilities against the float64 form of the definition (float64 shaping of the fp32 v with the fp32
    inv_temperature and top_r, float64 Bayes posterior) at every entry > 1e-9, to a relative bound counted as
    test_the_restatement_is_bayes_rule counts it — n = 5 K + 31 roundings of at most half an ulp (its 5 K + 30, of which `x0 w` is the
    one rounding of v, plus the division u = v / m), relative error n u / (1 - n u), u = 2^-24 — plus the clamp's 2 K 1e-12 (a tempered
    row's maximum is 1, so the posterior's total is at least about 1 / K and the clamp raises it by at most K 1e-12) plus the device
    power's error.  The ROCm installation documents no ulp bound for exp2f / log2f, so that term is measured: the kernel's largest
    relative error against float64 on these inputs on an MI355X was 2.849e-6 (K = 255 at (2, 75); on the four shapes the suite began
    with 1.851e-6 at K = 255, tau = 1.5, r = 1, no evidence, t = 2, 1.642e-6 at K = 2, 1.717e-6 at K = 5, 1.226e-6 at K = 20; guided_util
    has the largest per rung of the class-count ladder: the exponent inv_tau * log2(u) reaches -28 for the floored entries, and half an
    ulp of it on top of an ulp of log2f is that much of the power), and four times that is allowed: POWER_ERROR_ALLOWED = 1.1396e-5.
    With it the bound is 1.38e-5 at K = 2 and 8.9e-5 at K = 255, where the counted roundings dominate.
    Sample mode: the draws equal the fp32 restatement's at every pixel whose float64 race margin exceeds 1e-4 and whose float64
    threshold margins exceed 1e-5; the pixels left out are at most 2 % of the shape (at least 2 pixels are allowed)."""
    rng = np.random.default_rng(margin_seed(N, HW, K))
    x0, ev_all, xt = mixed_inputs(rng, N, HW, K)
    n = 5 * K + 31
    bound = n * 2.0 ** -24 / (1 - n * 2.0 ** -24) + 2 * K * 1e-12 + POWER_ERROR_ALLOWED
    worst = 0.0
    for tau, r, ev, t in tempered_cases(ev_all):
        inv, (a, c), want, big, skip = tempered_reference(x0, ev, xt, tau, r, t)
        what = f"tau={tau} r={r} ev={ev is not None} t={t}"
        got = run_kernel(lib, x0, ev, xt, inv, r, a, c, hip.STEP_LAST_CONFIDENCE, alias=True)["x0"].astype(np.float64)
        rel = float((np.abs(got - want)[big] / want[big]).max())
        worst = max(worst, rel)
        print(f"tempered K={K} {what}: max relative error {rel:.3e} (bound {bound:.3e}) over {int(big.sum())} of {big.size} entries")
        parity_log("ladder_shaped_step", **{f"rung{rung_of(K)}_K{K}_HW{HW}_max_rel_err_vs_float64": worst, f"K{K}_bound": bound})
        assert big.mean() > 0.5 and rel <= bound, (what, rel, bound)
        _, idx = shaped_restatement(x0, ev, xt, inv, r, a, c, hip.STEP_SAMPLE, TEMPERED_ROW, SEED, TEMPERED_OFF)
        got = run_kernel(lib, x0, ev, xt, inv, r, a, c, hip.STEP_SAMPLE, step_row=TEMPERED_ROW, sample_offset=TEMPERED_OFF)["xt"].astype(np.int64)
        print(f"tempered K={K} {what}: {int(skip.sum())} of {skip.size} pixels left out, {int((got != idx)[~skip].sum())} differ")
        assert skip.sum() <= max(2, 0.02 * skip.size), (what, int(skip.sum()))
        assert np.array_equal(got[~skip], idx[~skip]), what
    print(f"tempered K={K}: the largest relative error {worst:.3e}")


@pytest.mark.gpu
def test_shaped_kernel_refuses_bad_arguments(lib):
    N, HW, K = 2, 64, 3
    x0 = torch.full((N, HW, K), 0.25, device=DEV)
    ev = torch.ones((N, HW, K), device=DEV)
    xt = torch.full((N, HW), 2, dtype=torch.uint8, device=DEV)
    xin = torch.full((N, HW, 4), 7.5, device=DEV)
    probs = torch.full((N, HW, K), 3.5, device=DEV)
    onehot = torch.full((N, HW, K), 9, dtype=torch.int64, device=DEV)
    good = dict(x0=x0.data_ptr(), ev=ev.data_ptr(), N=N, HW=HW, K=K, inv=2.0, r=0.5, a=0.0, c=1.0, mode=hip.STEP_LAST_MAJORITY, step_row=0,
                seed=0, off=0, xt=xt.data_ptr(), xin=xin.data_ptr(), stride=4, probs=probs.data_ptr(), onehot=onehot.data_ptr(), stream=0)
    nan, inf = float("nan"), float("inf")
    for change in (dict(N=0), dict(N=-1), dict(HW=0), dict(K=0), dict(K=256), dict(x0=None), dict(xt=None), dict(stride=2),
                   dict(mode=hip.STEP_SOFTMAX_ONLY), dict(mode=-1), dict(mode=5), dict(step_row=-1), dict(inv=nan), dict(inv=inf),
                   dict(inv=0.04), dict(inv=21.0), dict(inv=-2.0), dict(r=nan), dict(r=inf), dict(r=0.0), dict(r=-0.5), dict(r=1.5)):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert SYMBOL in hip.last_error()
    torch.cuda.synchronize()
    assert bool((xt == 2).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all()) and bool((onehot == 9).all())    # nothing ran
    ev[..., 1:] = 0.0           # only class 0 is possible
    assert getattr(lib, SYMBOL)(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((xt == 0).all()) and bool((onehot.cpu() == torch.tensor([1, 0, 0])).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all())
    assert getattr(lib, SYMBOL)(*dict(good, ev=None, x0=probs.data_ptr(), probs=None).values()) == 0          # without evidence: a tie, class 0
    torch.cuda.synchronize()
    assert bool((xt == 0).all()) and bool((probs == 3.5).all())


# ------------------------------------------------------------------------------------------------ GPU: the sampler
EVIDENCE_SEED = 170


@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def sampler(request):
    """K = 2: stem conv and fused head-and-posterior launch (x_t travels as the uint8 index only); K = 5: the general epilogue, and the
    stem reads its one-hot from xin, which the shaped step writes."""
    s = make_sampler(request.param)
    s["ev"], _, _ = sampler_evidence(np.random.default_rng(EVIDENCE_SEED + s["K"]), s["N"], s["K"])
    return s


class Spy:
    """Stands in for lib.ccdm_shaped_step: clones the launch's inputs (out_probs = x0, xt) before it and its outputs (xt, out_probs,
    out_onehot, xin) behind it, on the stream the launch runs on."""

    def __init__(self, lib, engines):
        self.real, self.engines, self.seen = getattr(lib, SYMBOL), {e.out_probs.data_ptr(): e for e in engines}, []

    def __call__(self, *args):
        eng = self.engines[args[0]]
        assert args[13] == eng.xt.data_ptr() and args[16] == args[0] and args[17] == eng.out_onehot.data_ptr()
        assert args[14] == (None if eng.stem_onehot_on_load else eng.xin.ptr)
        with torch.cuda.stream(eng.stream):
            before = dict(x0=eng.out_probs.clone(), xt=eng.xt.clone())
            rc = self.real(*args)
            after = dict(xt=eng.xt.clone(), probs=eng.out_probs.clone(), onehot=eng.out_onehot.clone(),
                         xin=None if eng.stem_onehot_on_load else eng.xin.buf.clone())
        self.seen.append(dict(ev=args[1], N=args[2], inv=args[5], r=args[6], a=args[7], c=args[8], mode=args[9], row=args[10], seed=args[11],
                              off=args[12], before=before, after=after))
        return rc


def check_launch(rec, ev_nhwk, K):
    """One captured launch against the restatement on the launch's own inputs: exact (the callers temper with tau = 1 only)."""
    N = rec["N"]
    assert rec["inv"] == 1.0 and (rec["ev"] is None) == (ev_nhwk is None)
    x0 = rec["before"]["x0"].cpu().numpy().reshape(N, H * W, K)
    xt0 = rec["before"]["xt"].cpu().numpy().reshape(N, H * W)
    probs, idx = shaped_restatement(x0, ev_nhwk, xt0, rec["inv"], rec["r"], rec["a"], rec["c"], rec["mode"], rec["row"], rec["seed"], rec["off"])
    got_xt = rec["after"]["xt"].cpu().numpy().reshape(N, H * W).astype(np.int64)
    got_probs = rec["after"]["probs"].cpu().numpy().reshape(N, H * W, K)
    what = f"row {rec['row']} mode {rec['mode']}"
    if rec["mode"] == hip.STEP_SAMPLE:
        assert np.array_equal(got_xt, idx), what + f": {int((got_xt != idx).sum())} pixels differ"
        assert np.array_equal(bits(got_probs), bits(x0)), what
        if rec["after"]["xin"] is not None:
            assert np.array_equal(rec["after"]["xin"].cpu().numpy().reshape(N, H * W, -1)[..., :K], onehot_np(idx, K).astype(np.float32)), what
    elif rec["mode"] == hip.STEP_LAST_MAJORITY:
        assert np.array_equal(got_xt, idx), what
        assert np.array_equal(rec["after"]["onehot"].cpu().numpy().reshape(N, H * W, K), onehot_np(idx, K).astype(np.int64)), what
    elif rec["mode"] == hip.STEP_LAST_CONFIDENCE:
        assert np.array_equal(bits(got_probs), bits(probs)), what
        assert np.array_equal(got_xt, xt0), what
    return probs, idx


@pytest.mark.gpu
@pytest.mark.parametrize("vote", ["majority", "confidence"])
def test_without_the_keywords_nothing_changes(sampler, vote):
    """A plain call, temperature = truncation = None and temperature = truncation = 1.0 (the new path end to end against the old one)
    give bit-identical outputs; a plain call afterwards is unchanged; truncation = 0.5 differs."""
    s, model = sampler, sampler["model"]
    settings(model, step_T_sample=vote, substreams=0, use_graph=True)
    try:
        plain = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()
        none = model(s["x"], s["image"], t=T_STRIDED, temperature=None, truncation=None)["diffusion_out"].clone()
        ones = model(s["x"], s["image"], t=T_STRIDED, temperature=1.0, truncation=1.0)["diffusion_out"].clone()
        again = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()            # (the engine's table is the plain one again)
        assert plain.dtype == (torch.int64 if vote == "majority" else torch.float32)
        assert torch.equal(plain, none) and torch.equal(plain, ones) and torch.equal(plain, again)
        assert plain.dtype == ones.dtype and plain.stride() == ones.stride()
        cut = model(s["x"], s["image"], t=T_STRIDED, truncation=0.5)["diffusion_out"]
        assert not torch.equal(plain, cut)
    finally:
        settings(model, step_T_sample="majority")


@pytest.mark.gpu
@pytest.mark.parametrize("with_evidence", [False, True], ids=["alone", "with-evidence"])
def test_every_shaped_step_equals_the_restatement_on_the_devices_inputs(sampler, with_evidence, monkeypatch):
    """The strided 4-row walk with truncation = 0.6: restating each launch from the x0 and x_t it was handed reproduces what it left,
    exactly.  Rows 0..3, modes [SAMPLE] * 3 + [LAST_MAJORITY], the real coefficients, the call's key and offset; with evidence too it is
    still one launch per entry, and ccdm_evidence_step is not launched."""
    s, model = sampler, sampler["model"]
    K, N = s["K"], s["N"]
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    eng = model._engine(s["x"], s["image"], None)
    spy = Spy(lib, [eng])
    monkeypatch.setattr(lib, SYMBOL, spy)
    evidence_launches = []
    monkeypatch.setattr(lib, "ccdm_evidence_step", lambda *a, _real=lib.ccdm_evidence_step: (evidence_launches.append(1), _real(*a))[1])
    kw = dict(evidence=s["ev"].to(DEV)) if with_evidence else {}
    out = model(s["x"], s["image"], t=T_STRIDED, truncation=0.6, **kw)["diffusion_out"].cpu()
    monkeypatch.undo()
    assert evidence_launches == []
    assert [r["row"] for r in spy.seen] == [0, 1, 2, 3] and [r["mode"] for r in spy.seen] == [hip.STEP_SAMPLE] * 3 + [hip.STEP_LAST_MAJORITY]
    assert all(r["seed"] == model._philox_key() and r["off"] == 0 and r["N"] == N for r in spy.seen)
    assert all((r["inv"], r["r"]) == (1.0, float(np.float32(0.6))) for r in spy.seen)
    for r, t in zip(spy.seen, T_VALUES):
        a, c = model.diffusion.posterior_coeffs(t)
        assert (r["a"], r["c"]) == (a, c)
        assert bool(((r["before"]["x0"].sum(-1) - 1).abs() < 1e-5).all()), "the network pass did not stop at x0"
        _, idx = check_launch(r, nhwk(s["ev"]) if with_evidence else None, K)
    assert torch.equal(out, O.one_hot_bchw(torch.from_numpy(idx).reshape(N, H, W), K, torch.int64))


WALK_R = 0.6
# test_shaped_walk_against_the_oracle_step_by_step: the small_model seed per K.  Seed 3 (the fixture's) does not qualify — its oracle-only
# walk comes within 7.9e-5 (K = 2) and 7.6e-6 (K = 5) of a truncation threshold — so the next seed that does is taken: 16 for K = 2
# (margins 1.9e-4 / 1.2e-4), 67 for K = 5 (1.8e-4 / 1.2e-4), found on the CPU from the oracle alone
WALK_SEED = {2: 16, 5: 67}


def oracle_shaped_walk(sd, K, x, image, r, t_values, seed):
    """The oracle's loop with the restated shaped step (tau = 1) in between: U-Net forward on the CPU, shaped_restatement on its output.
    Returns every step's class map [N,H,W], the smallest relative gap between the winner and the runner-up of any race or argmax, and the
    smallest relative distance of a prefix mass to a truncation threshold."""
    _, alphas, cum = O.make_schedule("cosine", T_SMALL, {"s": 0.008})
    N = x.shape[0]
    xt, maps, gap, edge = x, [], np.inf, np.inf
    for j, t in enumerate(t_values):
        x0 = nhwk(O.unet_forward(sd, SMALL_CFG, xt, image, None, torch.full((N,), float(t)))["diffusion_out"])
        a, c = O.posterior_coeffs(alphas, cum, t)
        mode = hip.STEP_SAMPLE if t > 1 else hip.STEP_LAST_MAJORITY
        probs, idx = shaped_restatement(x0, None, xt.argmax(1).reshape(N, H * W).numpy(), 1.0, r, a, c, mode, j, seed, 0)
        score = probs.astype(np.float64) / (O.philox_exponential(seed, j, 0, N, H * W, K).astype(np.float64) if t > 1 else 1.0)
        top = np.sort(score, axis=-1)
        gap = min(gap, float(((top[..., -1] - top[..., -2]) / top[..., -1]).min()))
        edge = min(edge, float(threshold_margin64(x0.astype(np.float64), r).min()))
        idx = torch.from_numpy(idx).reshape(N, H, W)
        maps.append(idx)
        xt = O.one_hot_bchw(idx, K)
    return maps, gap, edge


@pytest.mark.gpu
def test_shaped_walk_against_the_oracle_step_by_step(sampler, monkeypatch):
    """The seeded 4-step strided walk with truncation = 0.6 (tau = 1), default precision (PREC_F16X3), N = 2, free-running: every step's
    class map equals the oracle's loop with the restated shaped step in between.  A last-bit difference of the network can flip a pixel
    at the race and at the truncation threshold, so the test is valid for weights whose oracle-only walk keeps both margins >= 1e-4 at
    every step: WALK_SEED has the seed per K, computed on the CPU beforehand (the margins are printed and asserted here).  The fixture's
    inputs, key and settings; its weights only where its seed qualifies."""
    s = sampler
    K, N = s["K"], 2
    model, sd = small_model(K, seed=WALK_SEED[K])
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, False
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    eng = model._engine(s["x"][:N], s["image"][:N], None)
    spy = Spy(lib, [eng])
    monkeypatch.setattr(lib, SYMBOL, spy)
    out = model(s["x"][:N], s["image"][:N], t=T_STRIDED, truncation=WALK_R)["diffusion_out"].cpu()
    monkeypatch.undo()
    ref, gap, edge = oracle_shaped_walk(sd, K, s["x_cpu"][:N], s["image_cpu"][:N], WALK_R, T_VALUES, model._philox_key())
    print(f"shaped walk K={K}: the oracle's smallest relative winner margin {gap:.2e}, smallest relative threshold margin {edge:.2e}")
    assert gap >= 1e-4 and edge >= 1e-4
    assert len(spy.seen) == 4
    for j, r in enumerate(spy.seen):
        got = r["after"]["xt"].cpu().reshape(N, H, W).long()
        mism = (got != ref[j]).float().mean().item()
        print(f"shaped walk K={K} step {j} (t={T_VALUES[j]}): class mismatch {mism:.2e}")
        assert mism == 0.0, (j, mism)
    assert torch.equal(out, O.one_hot_bchw(ref[-1], K, torch.int64))


@pytest.mark.gpu
def test_shaped_samples_do_not_depend_on_the_execution_shape(sampler):
    """N = 4, temperature = 0.7 and truncation = 0.8: bit-identical across substreams 1 / 2, graph replay on / off, and two calls of two
    samples at sample_offset 0 / 2."""
    s, model = sampler, sampler["model"]
    kw = dict(t=T_STRIDED, temperature=0.7, truncation=0.8)
    try:
        outs = {}
        for sub, graph in ((1, True), (2, True), (1, False), (2, False)):
            settings(model, substreams=sub, use_graph=graph, step_T_sample="majority")
            outs[(sub, graph)] = model(s["x"], s["image"], **kw)["diffusion_out"].clone()
            assert model.last_mode == (sub, graph)
        ref = outs[(1, True)]
        assert all(torch.equal(ref, v) for v in outs.values())
        halves = []
        for lo in (0, 2):
            settings(model, substreams=1, use_graph=True, sample_offset=lo)
            halves.append(model(s["x"][lo:lo + 2], s["image"][lo:lo + 2], **kw)["diffusion_out"].clone())
        settings(model, sample_offset=0)
        assert torch.equal(torch.cat(halves, 0), ref)
    finally:
        settings(model, substreams=0, use_graph=True, sample_offset=0)


@pytest.mark.gpu
def test_shaping_composes_with_known_labels_resampling_and_evidence(sampler, monkeypatch):
    """The full 6-row walk with 30 % of the pixels known, resample = (2, 2), evidence and truncation = 0.8: every walk entry launches
    renoise (after a jump), the network, the shaped step, the clamp — and no evidence step; the known pixels come back as their labels."""
    s, model = sampler, sampler["model"]
    K, known = s["K"], s["known"]
    is_known = known < K
    lib = hip.load()
    order = []
    for name in (SYMBOL, "ccdm_evidence_step", "ccdm_known_labels_step", "ccdm_renoise_step", "ccdm_engine_run"):
        def wrap(*args, _real=getattr(lib, name), _name=name):
            order.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, name, wrap)
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    out = model(s["x"], s["image"], known_labels=known, resample=(2, 2), evidence=s["ev"], truncation=0.8)["diffusion_out"].cpu()
    monkeypatch.undo()
    from ccdm_stochastic_segmentation_amd.models import resample_walk
    walk = resample_walk(T_SMALL, 2, 2)
    assert len(walk) > T_SMALL
    want = []
    for row, p, src in walk:
        want += (["ccdm_renoise_step"] if src is not None else []) + ["ccdm_engine_run", SYMBOL, "ccdm_known_labels_step"]
    assert order == want
    mask = is_known[:, None].expand_as(out)
    labels = O.one_hot_bchw(torch.where(is_known, known, torch.zeros_like(known)), K, torch.int64)
    assert torch.equal(out[mask], labels[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
@pytest.mark.parametrize("voting", ["majority", "confidence"])
def test_predict_multiple_is_shaped_in_every_pass(sampler, voting, batched, monkeypatch):
    """S = 3, truncation = 0.6: every launch of every pass equals the restatement on its own inputs; philox_call advances as it does for
    evidence."""
    s, model = sampler, sampler["model"]
    K, B, S = s["K"], 2, 3
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, philox_advance=True, philox_call=0)
    x = O.one_hot_bchw(torch.from_numpy(np.random.default_rng(7).integers(0, K, (S * B, H, W))), K).reshape(S, B, K, H, W).to(DEV)
    engines = [model._engine(x[0].repeat_interleave(S, dim=0) if batched else x[0], s["image"][:B].repeat_interleave(S if batched else 1, dim=0), None)]
    spy = Spy(lib, engines)
    monkeypatch.setattr(lib, SYMBOL, spy)
    try:
        out = model.predict_multiple(s["image"][:B], num_evaluations=S, voting=voting, t=T_STRIDED, batched=batched, truncation=0.6, x=x,
                                     maps=("mean", "vote"))
        monkeypatch.undo()
        assert model.philox_call == (1 if batched else S)
        assert len(spy.seen) == (4 if batched else 4 * S)
        last = hip.STEP_LAST_MAJORITY if voting == "majority" else hip.STEP_LAST_CONFIDENCE
        for i, r in enumerate(spy.seen):
            assert r["row"] == i % 4 and r["mode"] == (hip.STEP_SAMPLE if i % 4 < 3 else last) and r["N"] == (B * S if batched else B)
            assert (r["inv"], r["r"]) == (1.0, float(np.float32(0.6)))
            check_launch(r, None, K)
        assert tuple(out["vote"].shape) == (B, H, W) and tuple(out["mean"].shape) == (B, K, H, W)
    finally:
        monkeypatch.undo()
        settings(model, philox_advance=False, philox_call=0, substreams=0)
