"""Sampling under per-pixel soft evidence: DenoisingModel(..., evidence=) and the fused reweight-and-draw step kernel
ccdm_evidence_step (include/ccdm_hip.h).  The numpy restatement below is built from the oracle's public functions (theta_post_prob,
normalise_probs in cascade order, sample_index on philox_exponential's noise); it is held against Bayes' rule in float64 on the CPU,
the kernel is held bit for bit against it, and the sampler is checked launch by launch on the device's own inputs, free-running
against the oracle's loop, for what must not change without the keyword, and for independence of the execution shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import guidance, hip
from tests.guided_util import SHAPES, bits, coefficients, evidence_restatement, nhwk, random_inputs, sampler_evidence
from tests.sampler_util import (DEV, FREE, H, SEED, SMALL_CFG, T_SMALL, T_STRIDED, W, assert_symbol_declared_bound_and_built, load_lib,
                                make_sampler, onehot_np, sample_sharded_keywords, settings, small_model)

SYMBOL = "ccdm_evidence_step"
T_VALUES = [6, 4, 3, 1]          # t = 10004 walks the small model strided


# ------------------------------------------------------------------------------------------------ CPU
def test_evidence_symbol_declared_bound_and_built():
    """hip.py binds the symbol with argtypes that match the header's declaration (17 arguments), the source is in the build list, the
    library cross-built from it exports it under the unchanged ABI number, and every bad argument is refused before anything is launched
    (host pointers: a launch would fault) with the expected word in the error string."""
    lib = assert_symbol_declared_bound_and_built(SYMBOL, 17, "ccdm_guided.hip")
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    good = dict(x0=p, ev=p, N=1, HW=8, K=2, a=0.5, c=0.5, mode=hip.STEP_SAMPLE, step_row=0, seed=0, off=0, xt=p, xin=None, stride=4,
                probs=None, onehot=None, stream=None)
    for change, text in ((dict(N=0), "N=0"), (dict(N=-1), "N=-1"), (dict(HW=0), "HW=0"), (dict(K=0), "K=0"), (dict(K=256), "K=256"),
                         (dict(x0=None), "null"), (dict(ev=None), "null"), (dict(xt=None), "null"), (dict(xin=p, stride=1), "xin_stride"),
                         (dict(mode=hip.STEP_SOFTMAX_ONLY), "mode"), (dict(mode=7), "mode"), (dict(mode=-1), "mode"),
                         (dict(step_row=-1), "step_row"), (dict(N=2 ** 31 - 1, HW=2 ** 31 - 1), "too many pixels")):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert text in hip.last_error() and "evidence_step" in hip.last_error(), (change, hip.last_error())


def test_evidence_argument_validation():
    """Every refusal of guidance.check_evidence is a ValueError naming `evidence`, through forward, forward_denoising and predict_multiple, before
    anything runs (a model that was never moved to a GPU: nothing can run); the accepted forms and the returned layout."""
    m, _ = small_model(3)
    m.eval()
    N, K = 2, 3
    x = torch.nn.functional.one_hot(torch.zeros((N, H, W), dtype=torch.int64), K).permute(0, 3, 1, 2).float()
    cond = torch.zeros(N, 1, H, W)
    ok = torch.ones((N, K, H, W))

    def one(value, n=1):
        t = ok.clone()
        t[0, :n, 3, 5] = value
        return t
    cases = [("shape", torch.ones((N, K, H, W + 1))), ("shape", torch.ones((N, H, W, K))), ("shape", torch.ones((N, K, H * W))),
             ("floating", torch.ones((N, K, H, W), dtype=torch.int64)), ("floating", torch.ones((N, K, H, W), dtype=torch.bool)),
             ("finite", one(float("nan"))), ("finite", one(float("inf"))), ("finite", one(float("-inf"))),
             (r"\[0,1\]", one(-0.25)), (r"\[0,1\]", one(1.5)), ("all 0", one(0.0, K))]
    for text, bad in cases:
        for call in (lambda e: m(x, cond, t=T_STRIDED, evidence=e), lambda e: m.forward_denoising(x, cond, None, 10004, evidence=e)):
            with pytest.raises(ValueError, match="evidence.*" + text):
                call(bad)
        with pytest.raises(ValueError, match="evidence.*" + text):
            m.predict_multiple(cond, num_evaluations=2, voting="majority", t=T_STRIDED, evidence=bad)
    m.rng = "torch_cpu"
    for call in (lambda: m(x, cond, t=T_STRIDED, evidence=ok), lambda: m.forward_denoising(x, cond, None, 10004, evidence=ok),
                 lambda: m.predict_multiple(cond, num_evaluations=2, voting="majority", evidence=ok)):
        with pytest.raises(ValueError, match="evidence.*torch_cpu"):
            call()
    m.rng = "philox"
    with pytest.raises(ValueError, match="evidence.*sampling call"):
        m(x, cond, t=torch.full((N,), 3.0), validation=True, evidence=ok)           # forward_step has no walk to guide
    m.train()
    with pytest.raises(ValueError, match="evidence.*sampling call"):
        m(x, cond, t=torch.full((N,), 3.0), evidence=ok)
    with pytest.raises(ValueError, match="evidence.*sampling call"):
        m.forward_denoising(x, cond, None, 10004, evidence=ok)
    m.eval()
    logits_model, _ = small_model(3, softmax_output=False)
    logits_model.eval()
    for call in (lambda: logits_model(x, cond, t=T_STRIDED, evidence=ok), lambda: logits_model.forward_denoising(x, cond, None, 10004, evidence=ok),
                 lambda: logits_model.predict_multiple(cond, num_evaluations=2, voting="majority", evidence=ok)):
        with pytest.raises(ValueError, match="evidence.*softmax_output"):
            call()
    # resample still needs known_labels, with evidence or without
    with pytest.raises(ValueError, match="resample.*known_labels"):
        m(x, cond, t=T_STRIDED, evidence=ok, resample=(2, 2))
    assert m.philox_call == 0 and m._engines == {} and logits_model._engines == {}          # nothing ran
    # the accepted forms: any floating dtype, 0 and 1 included, a single positive weight per pixel; returned as fp32 [N,H*W,K]
    rng = np.random.default_rng(5)
    good = torch.from_numpy(rng.random((N, K, H, W)))
    good[:, 1:, :4] = 0.0
    good[:, 0, :4] = 1.0
    for dtype in (torch.float64, torch.float32, torch.float16):
        got = guidance.check_evidence(m, good.to(dtype), (N, K, H, W))
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, H * W, K) and got.is_contiguous()
        assert torch.equal(got.reshape(N, H, W, K).permute(0, 3, 1, 2), good.to(dtype).float())


@pytest.mark.parametrize("K", [2, 5, 20])
def test_the_restatement_is_bayes_rule(K):
    """p(x_{t-1} = k | x_t, e) = sum_d theta(k | x_t, d) x0_d w_d, normalised, with theta(. | x_t, d) = q(x_{t-1} | x_t, x_0 = d) — in
    float64, brute force over d — equals the restated probabilities wherever it exceeds 1e-9, to a relative bound counted from the
    restatement's fp32 operations (each at most half an ulp, u = 2^-24; all terms are positive, so a sum's relative error is its worst
    term's plus one u per addition):
        u_ = (1 - a) / K, b = (1 - c) / K: 2 each; A_k = a [k = x_t] + u_: 3; S = sum A: K + 2; b S: K + 5; c A_k + b S: K + 6;
        x0' = x0 w: 1; r = x0' / (.): K + 8; R = sum r: 2 K + 7; c r_k + b R: 2 K + 11; P_k = A_k (.): 2 K + 15;
        total = sum P: 3 K + 14; P_k / total: n = 5 K + 30 roundings, relative error <= n u / (1 - n u).
    The clamp at 1e-12 raises the total by at most K 1e-12 against sum_k P_k = sum_d x0_d w_d >= 0.5e-3 (random_inputs): 2 K 1e-9."""
    rng = np.random.default_rng(300 + K)
    N, HW = 2, 257
    x0, ev, xt = random_inputs(rng, N, HW, K)
    _, alphas, cum = O.make_schedule("cosine", 250, {"s": 0.008})
    n = 5 * K + 30
    bound = n * 2.0 ** -24 / (1 - n * 2.0 ** -24) + 2 * K * 1e-9
    for t in (250, 100, 1):
        a, c = O.posterior_coeffs(alphas, cum, t)
        probs, _ = evidence_restatement(x0, ev, xt, a, c, hip.STEP_LAST_CONFIDENCE, 0, 0, 0)
        a64, c64 = float(np.float32(a)), float(np.float32(c))          # (the fp32 coefficients the step is handed)
        eye = np.eye(K)
        A = a64 * onehot_np(xt, K) + (1 - a64) / K                      # [N,HW,k]   q(x_t | x_{t-1} = k)
        B = c64 * eye + (1 - c64) / K                                   # [k,d]      q(x_{t-1} = k | x_0 = d)
        joint = A[..., :, None] * B[None, None]                         # [N,HW,k,d]
        theta = joint / joint.sum(axis=2, keepdims=True)                # theta(k | x_t, d)
        want = (theta * (x0.astype(np.float64) * ev.astype(np.float64))[..., None, :]).sum(-1)
        want = want / want.sum(-1, keepdims=True)
        big = want > 1e-9
        rel = np.abs(probs.astype(np.float64) - want)[big] / want[big]
        print(f"Bayes K={K} t={t}: max relative error {rel.max():.3e} (bound {bound:.3e}) over {int(big.sum())} of {big.size} entries")
        assert big.mean() > 0.5 and rel.max() <= bound, (t, rel.max(), bound)
        # a class the evidence rules out keeps only the clamp's floor
        if t == 1:
            assert probs[ev == 0].max() <= 1e-12 / 0.5e-3 * (1 + 1e-6)


def test_sample_sharded_hands_the_callers_evidence_through():
    """distributed.sample_sharded slices x and the conditions, not evidence: the caller passes its shard's slice."""
    ev = torch.ones(3, 2, 4, 4)
    kl = torch.full((3, 4, 4), FREE)
    seen = sample_sharded_keywords(evidence=ev)
    assert seen["evidence"] is ev and "known_labels" not in seen
    seen = sample_sharded_keywords(known_labels=kl, resample=(2, 3), evidence=ev)
    assert seen["evidence"] is ev and seen["known_labels"] is kl and seen["resample"] == (2, 3)
    assert "evidence" not in sample_sharded_keywords()


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run_kernel(lib, x0, ev, xt, a, c, mode, *, step_row=0, seed=SEED, sample_offset=0, xin=None, probs=None, onehot=None, alias=False):
    """x0, ev: fp32 [N,HW,K]; xt: integer [N,HW]; xin [N,HW,stride] / probs / onehot [N,HW,K] numpy or None; alias: out_probs IS x0.
    Returns the buffers after the launch (numpy)."""
    N, HW, K = x0.shape
    host = dict(x0=x0, ev=ev, xt=np.asarray(xt).astype(np.uint8), xin=xin, probs=probs, onehot=onehot)
    d = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in host.items()}

    def ptr(name):
        return None if d[name] is None else d[name].data_ptr()
    hip.check(getattr(lib, SYMBOL)(ptr("x0"), ptr("ev"), N, HW, K, float(a), float(c), mode, step_row, seed, sample_offset, ptr("xt"),
                                   ptr("xin"), 0 if xin is None else xin.shape[2], ptr("x0") if alias else ptr("probs"), ptr("onehot"), 0),
              SYMBOL)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_evidence_kernel_equals_the_restatement(lib, N, HW, K):
    """STEP_SAMPLE, bit equality: xt and the one-hot channels equal the restatement, with and without xin (a stride > K that is no
    multiple of 4), at two (sample offset, step row) pairs and at a high and a low t of a cosine schedule; the image channels >= K of
    xin, x0 and the evidence are bit-unchanged; the draw moves with the offset and the row; sharding."""
    rng = np.random.default_rng(1000 + K)
    stride = (K + 4) // 4 * 4 + 1
    x0, ev, xt = random_inputs(rng, N, HW, K)
    xin0 = rng.standard_normal((N, HW, stride)).astype(np.float32)
    draws = {}
    for t in (200, 2):
        a, c = coefficients(t)
        for off, row in ((0, 0), (5, 3)):
            _, want = evidence_restatement(x0, ev, xt, a, c, hip.STEP_SAMPLE, row, SEED, off)
            for with_xin in (True, False):
                r = run_kernel(lib, x0, ev, xt, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off, xin=xin0 if with_xin else None)
                what = f"t={t} off={off} row={row} xin={with_xin}"
                got = r["xt"].astype(np.int64)
                assert np.array_equal(got, want), what + f": {int((got != want).sum())} of {got.size} pixels differ from the restatement"
                assert np.array_equal(bits(r["x0"]), bits(x0)) and np.array_equal(bits(r["ev"]), bits(ev)), what
                if with_xin:
                    assert np.array_equal(bits(r["xin"][..., K:]), bits(xin0[..., K:])), what + ": an image channel changed"
                    assert np.array_equal(r["xin"][..., :K], onehot_np(want, K).astype(np.float32)), what
            draws[(t, off, row)] = want
    if K < 255:         # (K = 255: 64 pixels)
        assert not np.array_equal(draws[(200, 0, 0)], draws[(200, 5, 3)])
    if N > 1:           # samples 1.. of a batch at offset 5 are samples 0.. of a batch at offset 6
        a, c = coefficients(200)
        full = run_kernel(lib, x0, ev, xt, a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=5)
        tail = run_kernel(lib, x0[1:], ev[1:], xt[1:], a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=6)
        assert np.array_equal(full["xt"][1:], tail["xt"])


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_evidence_kernel_last_step_modes_with_aliased_x0(lib, N, HW, K):
    """The three last-step modes with x0 and out_probs the same buffer (as in the engine), bit equality: confidence leaves the restated
    probabilities there and xt alone; majority the argmax one-hot in out_onehot, its index in xt, and x0 alone; keep writes nothing."""
    rng = np.random.default_rng(2000 + K)
    x0, ev, xt = random_inputs(rng, N, HW, K)
    onehot0 = rng.integers(-5, 5, (N, HW, K))
    for t in (1, 3):
        a, c = coefficients(t, T_SMALL)
        probs, idx = evidence_restatement(x0, ev, xt, a, c, hip.STEP_LAST_MAJORITY, 0, SEED, 0)
        r = run_kernel(lib, x0, ev, xt, a, c, hip.STEP_LAST_CONFIDENCE, onehot=onehot0, alias=True)
        assert np.array_equal(bits(r["x0"]), bits(probs)), f"t={t}: {int((bits(r['x0']) != bits(probs)).sum())} probabilities differ"
        assert np.array_equal(r["xt"], xt.astype(np.uint8)) and np.array_equal(r["onehot"], onehot0)
        r = run_kernel(lib, x0, ev, xt, a, c, hip.STEP_LAST_MAJORITY, onehot=onehot0, alias=True, step_row=3, sample_offset=2)
        assert np.array_equal(r["xt"].astype(np.int64), idx) and np.array_equal(r["onehot"], onehot_np(idx, K).astype(np.int64))
        assert r["onehot"].dtype == np.int64 and np.array_equal(bits(r["x0"]), bits(x0))
        r = run_kernel(lib, x0, ev, xt, a, c, hip.STEP_LAST_KEEP, onehot=onehot0, alias=True)
        assert np.array_equal(r["xt"], xt.astype(np.uint8)) and np.array_equal(r["onehot"], onehot0) and np.array_equal(bits(r["x0"]), bits(x0))
    # one-hot evidence at t = 1 (every x0 entry >= 1e-3): the majority is exactly the evidence's class
    cls = rng.integers(0, K, (N, HW))
    a, c = coefficients(1)
    r = run_kernel(lib, x0, onehot_np(cls, K).astype(np.float32), xt, a, c, hip.STEP_LAST_MAJORITY, onehot=onehot0, alias=True)
    assert np.array_equal(r["xt"].astype(np.int64), cls) and np.array_equal(r["onehot"], onehot_np(cls, K).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", SHAPES)
def test_all_ones_evidence_is_the_unguided_step(lib, N, HW, K):
    """All-ones evidence gives the xt of ccdm_posterior_sample on the same probabilities (softmax = 0), same key, offset and row."""
    rng = np.random.default_rng(3000 + K)
    x0, _, xt = random_inputs(rng, N, HW, K)
    row, off = 3, 5
    for t in (200, 2):
        a, c = coefficients(t)
        got = run_kernel(lib, x0, np.ones_like(x0), xt, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off)["xt"]
        table = torch.zeros((row + 1, 4), dtype=torch.float32)
        table[row] = torch.tensor([a, c, float(hip.STEP_SAMPLE), 0.0])
        d = dict(head=torch.from_numpy(x0).to(DEV), xt=torch.from_numpy(xt.astype(np.uint8)).to(DEV), table=table.to(DEV),
                 step=torch.tensor([row], dtype=torch.int32, device=DEV), nxt=torch.zeros((N, HW), dtype=torch.uint8, device=DEV))
        p = hip.PostArgs()
        p.head, p.softmax, p.head_stride = d["head"].data_ptr(), 0, K
        p.xt, p.N, p.HW, p.K = d["xt"].data_ptr(), N, HW, K
        p.step_table, p.step_ptr = d["table"].data_ptr(), d["step"].data_ptr()
        p.philox_seed, p.sample_offset = SEED, off
        p.xt_next = d["nxt"].data_ptr()
        hip.check(lib.ccdm_posterior_sample(C.byref(p), 0), "posterior_sample")
        torch.cuda.synchronize()
        assert np.array_equal(got, d["nxt"].cpu().numpy()), t


@pytest.mark.gpu
def test_evidence_kernel_refuses_bad_arguments(lib):
    N, HW, K = 2, 64, 3
    x0 = torch.full((N, HW, K), 0.25, device=DEV)
    ev = torch.ones((N, HW, K), device=DEV)
    xt = torch.full((N, HW), 2, dtype=torch.uint8, device=DEV)
    xin = torch.full((N, HW, 4), 7.5, device=DEV)
    probs = torch.full((N, HW, K), 3.5, device=DEV)
    onehot = torch.full((N, HW, K), 9, dtype=torch.int64, device=DEV)
    good = dict(x0=x0.data_ptr(), ev=ev.data_ptr(), N=N, HW=HW, K=K, a=0.0, c=1.0, mode=hip.STEP_LAST_MAJORITY, step_row=0, seed=0, off=0,
                xt=xt.data_ptr(), xin=xin.data_ptr(), stride=4, probs=probs.data_ptr(), onehot=onehot.data_ptr(), stream=0)
    for change in (dict(N=0), dict(N=-1), dict(HW=0), dict(K=0), dict(K=256), dict(x0=None), dict(ev=None), dict(xt=None), dict(stride=2),
                   dict(mode=hip.STEP_SOFTMAX_ONLY), dict(mode=-1), dict(mode=5), dict(step_row=-1)):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert "evidence_step" in hip.last_error()
    torch.cuda.synchronize()
    assert bool((xt == 2).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all()) and bool((onehot == 9).all())    # nothing ran
    ev[..., 1:] = 0.0           # only class 0 is possible
    assert getattr(lib, SYMBOL)(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((xt == 0).all()) and bool((onehot.cpu() == torch.tensor([1, 0, 0])).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all())


# ------------------------------------------------------------------------------------------------ GPU: the sampler
@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def sampler(request):
    """K = 2: stem conv and fused head-and-posterior launch (x_t travels as the uint8 index only); K = 5: the general epilogue, and the
    stem reads its one-hot from xin, which the evidence step writes."""
    s = make_sampler(request.param)
    s["ev"], _, _ = sampler_evidence(np.random.default_rng(EVIDENCE_SEED + s["K"]), s["N"], s["K"])
    return s


EVIDENCE_SEED = 70


class Spy:
    """Stands in for lib.ccdm_evidence_step: clones the launch's inputs (out_probs = x0, xt) before it and its outputs (xt, out_probs,
    out_onehot, xin) behind it, on the stream the launch runs on."""

    def __init__(self, lib, engines):
        self.real, self.engines, self.seen = getattr(lib, SYMBOL), {e.out_probs.data_ptr(): e for e in engines}, []

    def __call__(self, *args):
        eng = self.engines[args[0]]
        assert args[11] == eng.xt.data_ptr() and args[14] == args[0] and args[15] == eng.out_onehot.data_ptr()
        assert args[12] == (None if eng.stem_onehot_on_load else eng.xin.ptr)
        with torch.cuda.stream(eng.stream):
            before = dict(x0=eng.out_probs.clone(), xt=eng.xt.clone())
            rc = self.real(*args)
            after = dict(xt=eng.xt.clone(), probs=eng.out_probs.clone(), onehot=eng.out_onehot.clone(),
                         xin=None if eng.stem_onehot_on_load else eng.xin.buf.clone())
        self.seen.append(dict(N=args[2], a=args[5], c=args[6], mode=args[7], row=args[8], seed=args[9], off=args[10], before=before, after=after))
        return rc


def check_launch(rec, ev_nhwk, K):
    """One captured launch against the restatement on the launch's own inputs: exact."""
    N = rec["N"]
    x0 = rec["before"]["x0"].cpu().numpy().reshape(N, H * W, K)
    xt0 = rec["before"]["xt"].cpu().numpy().reshape(N, H * W)
    probs, idx = evidence_restatement(x0, ev_nhwk, xt0, rec["a"], rec["c"], rec["mode"], rec["row"], rec["seed"], rec["off"])
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
def test_without_evidence_nothing_changes(sampler, vote):
    """A plain call, evidence = None and all-ones evidence (the new path end to end against the old one) give bit-identical outputs."""
    s, model = sampler, sampler["model"]
    settings(model, step_T_sample=vote, substreams=0, use_graph=True)
    try:
        plain = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()
        none = model(s["x"], s["image"], t=T_STRIDED, evidence=None)["diffusion_out"].clone()
        ones = model(s["x"], s["image"], t=T_STRIDED, evidence=torch.ones((s["N"], s["K"], H, W)))["diffusion_out"].clone()
        again = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()            # (the engine's table is the plain one again)
        assert plain.dtype == (torch.int64 if vote == "majority" else torch.float32)
        assert torch.equal(plain, none) and torch.equal(plain, ones) and torch.equal(plain, again)
        assert plain.dtype == ones.dtype and plain.stride() == ones.stride()
        guided = model(s["x"], s["image"], t=T_STRIDED, evidence=s["ev"])["diffusion_out"]
        assert not torch.equal(plain, guided)
    finally:
        settings(model, step_T_sample="majority")


@pytest.mark.gpu
def test_every_evidence_step_equals_the_restatement_on_the_devices_inputs(sampler, monkeypatch):
    """The strided 4-row walk under soft evidence: restating each launch from the x0 and x_t it was handed reproduces what it left,
    exactly — an assertion no rounding of the network can flip.  Rows 0..3, modes [SAMPLE] * 3 + [LAST_MAJORITY], the real coefficients,
    the call's key."""
    s, model = sampler, sampler["model"]
    K, N = s["K"], s["N"]
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    eng = model._engine(s["x"], s["image"], None)
    spy = Spy(lib, [eng])
    monkeypatch.setattr(lib, SYMBOL, spy)
    out = model(s["x"], s["image"], t=T_STRIDED, evidence=s["ev"].to(DEV))["diffusion_out"].cpu()
    monkeypatch.undo()
    assert [r["row"] for r in spy.seen] == [0, 1, 2, 3] and [r["mode"] for r in spy.seen] == [hip.STEP_SAMPLE] * 3 + [hip.STEP_LAST_MAJORITY]
    assert all(r["seed"] == model._philox_key() and r["off"] == 0 and r["N"] == N for r in spy.seen)
    for r, t in zip(spy.seen, T_VALUES):
        a, c = model.diffusion.posterior_coeffs(t)
        assert (r["a"], r["c"]) == (a, c)
        x0 = r["before"]["x0"]
        assert bool(((x0.sum(-1) - 1).abs() < 1e-5).all()), "the network pass did not stop at x0"
        _, idx = check_launch(r, nhwk(s["ev"]), K)
    assert torch.equal(out, O.one_hot_bchw(torch.from_numpy(idx).reshape(N, H, W), K, torch.int64))


def oracle_guided_walk(sd, K, x, image, ev_bchw, t_values, seed):
    """The oracle's loop with the restated evidence step in between: U-Net forward on the CPU, evidence_restatement on its output.
    Returns every step's class map [N,H,W] and the smallest relative gap between the winner and the runner-up of any race or argmax."""
    _, alphas, cum = O.make_schedule("cosine", T_SMALL, {"s": 0.008})
    N = x.shape[0]
    ev = nhwk(ev_bchw)
    xt, maps, gap = x, [], np.inf
    for j, t in enumerate(t_values):
        x0 = O.unet_forward(sd, SMALL_CFG, xt, image, None, torch.full((N,), float(t)))["diffusion_out"]
        a, c = O.posterior_coeffs(alphas, cum, t)
        mode = hip.STEP_SAMPLE if t > 1 else hip.STEP_LAST_MAJORITY
        probs, idx = evidence_restatement(nhwk(x0), ev, xt.argmax(1).reshape(N, H * W).numpy(), a, c, mode, j, seed, 0)
        score = probs.astype(np.float64) / (O.philox_exponential(seed, j, 0, N, H * W, K).astype(np.float64) if t > 1 else 1.0)
        top = np.sort(score, axis=-1)
        gap = min(gap, float(((top[..., -1] - top[..., -2]) / top[..., -1]).min()))
        idx = torch.from_numpy(idx).reshape(N, H, W)
        maps.append(idx)
        xt = O.one_hot_bchw(idx, K)
    return maps, gap


@pytest.mark.gpu
def test_guided_walk_against_the_oracle_step_by_step(sampler, monkeypatch):
    """The seeded 4-step strided walk under soft evidence, default precision (PREC_F16X3), free-running: every step's class map equals
    the oracle's loop with the restated evidence step in between — the rule of the known-label walk: equality."""
    s, model = sampler, sampler["model"]
    K, N = s["K"], 2
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    eng = model._engine(s["x"][:N], s["image"][:N], None)
    spy = Spy(lib, [eng])
    monkeypatch.setattr(lib, SYMBOL, spy)
    out = model(s["x"][:N], s["image"][:N], t=T_STRIDED, evidence=s["ev"][:N])["diffusion_out"].cpu()
    monkeypatch.undo()
    ref, gap = oracle_guided_walk(s["sd"], K, s["x_cpu"][:N], s["image_cpu"][:N], s["ev"][:N], T_VALUES, model._philox_key())
    print(f"guided walk K={K}: the oracle's smallest relative winner margin {gap:.2e}")
    assert len(spy.seen) == 4
    for j, r in enumerate(spy.seen):
        got = r["after"]["xt"].cpu().reshape(N, H, W).long()
        mism = (got != ref[j]).float().mean().item()
        print(f"guided walk K={K} step {j} (t={T_VALUES[j]}): class mismatch {mism:.2e}")
        assert mism == 0.0, (j, mism)
    assert torch.equal(out, O.one_hot_bchw(ref[-1], K, torch.int64))


@pytest.mark.gpu
def test_guided_samples_do_not_depend_on_the_execution_shape(sampler):
    """N = 4: bit-identical across substreams 1 / 2, graph replay on / off, and two calls of two samples at sample_offset 0 / 2 with the
    matching slices of the evidence."""
    s, model = sampler, sampler["model"]
    ev = s["ev"].to(DEV)
    try:
        outs = {}
        for sub, graph in ((1, True), (2, True), (1, False), (2, False)):
            settings(model, substreams=sub, use_graph=graph, step_T_sample="majority")
            outs[(sub, graph)] = model(s["x"], s["image"], t=T_STRIDED, evidence=ev)["diffusion_out"].clone()
            assert model.last_mode == (sub, graph)
        ref = outs[(1, True)]
        assert all(torch.equal(ref, v) for v in outs.values())
        halves = []
        for lo in (0, 2):
            settings(model, substreams=1, use_graph=True, sample_offset=lo)
            halves.append(model(s["x"][lo:lo + 2], s["image"][lo:lo + 2], t=T_STRIDED, evidence=ev[lo:lo + 2])["diffusion_out"].clone())
        settings(model, sample_offset=0)
        assert torch.equal(torch.cat(halves, 0), ref)
    finally:
        settings(model, substreams=0, use_graph=True, sample_offset=0)


@pytest.mark.gpu
def test_evidence_composes_with_known_labels_and_resampling(sampler, monkeypatch):
    """The full 6-row walk with 30 % of the pixels known and resample = (2, 2): the known pixels come back as their labels; evidence
    that is one-hot on a random class over a random 30 % of the free pixels changes free pixels; every walk entry launches the
    evidence step behind the network and in front of the clamp."""
    s, model = sampler, sampler["model"]
    K, known = s["K"], s["known"]
    is_known = known < K
    rng = np.random.default_rng(900 + K)
    pick = torch.from_numpy(rng.random(tuple(known.shape)) < 0.3) & ~is_known
    cls = torch.from_numpy(rng.integers(0, K, tuple(known.shape)))
    ev = torch.where(pick[:, None], O.one_hot_bchw(cls, K), torch.ones((s["N"], K, H, W)))
    lib = hip.load()
    order = []
    for name in (SYMBOL, "ccdm_known_labels_step", "ccdm_renoise_step", "ccdm_engine_run"):
        def wrap(*args, _real=getattr(lib, name), _name=name):
            order.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, name, wrap)
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    guided = model(s["x"], s["image"], known_labels=known, resample=(2, 2), evidence=ev)["diffusion_out"].cpu()
    monkeypatch.undo()
    from ccdm_stochastic_segmentation_amd.models import resample_walk
    walk = resample_walk(T_SMALL, 2, 2)
    assert len(walk) > T_SMALL
    want = []
    for row, p, src in walk:
        want += (["ccdm_renoise_step"] if src is not None else []) + ["ccdm_engine_run", SYMBOL, "ccdm_known_labels_step"]
    assert order == want
    plain = model(s["x"], s["image"], known_labels=known, resample=(2, 2))["diffusion_out"].cpu()
    mask = is_known[:, None].expand_as(guided)
    labels = O.one_hot_bchw(torch.where(is_known, known, torch.zeros_like(known)), K, torch.int64)
    assert torch.equal(guided[mask], labels[mask]) and torch.equal(plain[mask], labels[mask])
    assert not torch.equal(guided[~mask], plain[~mask])
    # the last row is t = 1: a one-hot pixel of the evidence returns the evidence's class
    assert torch.equal(guided.argmax(1)[pick], cls[pick])


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
@pytest.mark.parametrize("voting", ["majority", "confidence"])
def test_predict_multiple_is_guided_in_every_pass(sampler, voting, batched, monkeypatch):
    """S = 3: every launch of every pass equals the restatement on its own inputs (the evidence of image b in every pass of it); where
    the passes' restated predictions agree — they do where the evidence is one-hot — `vote` is that class; philox_call advances as it
    does for known_labels."""
    s, model = sampler, sampler["model"]
    K, B, S = s["K"], 2, 3
    ev, pick, cls = sampler_evidence(np.random.default_rng(EVIDENCE_SEED + 10 + K), B, K, onehot_share=0.3)
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, philox_advance=True, philox_call=0)
    x = O.one_hot_bchw(torch.from_numpy(np.random.default_rng(7).integers(0, K, (S * B, H, W))), K).reshape(S, B, K, H, W).to(DEV)
    engines = [model._engine(x[0].repeat_interleave(S, dim=0) if batched else x[0], s["image"][:B].repeat_interleave(S if batched else 1, dim=0), None)]
    spy = Spy(lib, engines)
    monkeypatch.setattr(lib, SYMBOL, spy)
    try:
        out = model.predict_multiple(s["image"][:B], num_evaluations=S, voting=voting, t=T_STRIDED, batched=batched, evidence=ev, x=x,
                                     maps=("mean", "vote"))
        monkeypatch.undo()
        assert model.philox_call == (1 if batched else S)
        assert len(spy.seen) == (4 if batched else 4 * S)
        last = hip.STEP_LAST_MAJORITY if voting == "majority" else hip.STEP_LAST_CONFIDENCE
        ev_launch = nhwk(ev.repeat_interleave(S, dim=0) if batched else ev)
        preds = []
        for i, r in enumerate(spy.seen):
            assert r["row"] == i % 4 and r["mode"] == (hip.STEP_SAMPLE if i % 4 < 3 else last) and r["N"] == (B * S if batched else B)
            probs, idx = check_launch(r, ev_launch, K)
            if i % 4 == 3:
                preds.append(idx)
        passes = np.stack(preds[0].reshape(B, S, H * W).transpose(1, 0, 2) if batched else preds)        # [S,B,HW]
        agree = (passes == passes[0]).all(0)
        onehot_pix = pick.reshape(B, H * W).numpy()
        assert agree[onehot_pix].all() and np.array_equal(passes[0][onehot_pix], cls.reshape(B, H * W).numpy()[onehot_pix])
        vote = out["vote"].cpu().reshape(B, H * W).numpy()
        where = agree if voting == "majority" else onehot_pix          # (confidence: the argmax of a mean whose winner holds 1 - 1e-9)
        assert np.array_equal(vote[where], passes[0][where])
    finally:
        monkeypatch.undo()
        settings(model, philox_advance=False, philox_call=0, substreams=0)
