"""Sampling with known pixel labels: DenoisingModel(..., known_labels=) and the per-step clamp kernel ccdm_known_labels_step
(include/ccdm_hip.h).  The kernel is checked for equality against a numpy restatement built on the oracle's Philox4x32-10; the
sampler for the constraint itself, for what must not change without the keyword, for independence of the execution shape, and step
by step against the conditioned loop restated from the oracle's public step functions."""
import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import guidance, hip
from tests.sampler_util import (DEV, FREE, H, SEED, SMALL_CFG, T_SMALL, T_STRIDED, W, assert_symbol_declared_bound_and_built, clamp_restatement,
                                load_lib, make_sampler, onehot_np, probabilities, sample_sharded_keywords, settings, small_model)

SYMBOL = "ccdm_known_labels_step"
T_ONE_STEP = torch.as_tensor(10001)          # one step at t = T: the walk stops above t = 1 and returns the kept index


# ------------------------------------------------------------------------------------------------ CPU
def test_known_labels_symbol_declared_bound_and_built():
    """hip.py binds the symbol with argtypes that match the header's declaration, the source is in the build list, the library built
    from it (cross-compiled for gfx950 by build()) exports it, and bad arguments are refused before anything is launched."""
    lib = assert_symbol_declared_bound_and_built(SYMBOL, 16, "ccdm_known.hip")
    buf = np.zeros(64, dtype=np.uint8)           # (host memory: the refused calls below never reach a launch)
    p = buf.ctypes.data
    good = dict(known=p, N=1, HW=8, K=2, p_hit=1.0, p_miss=0.0, mode=hip.STEP_SAMPLE, step_row=0, seed=0, off=0, xt=p, xin=None, stride=4,
                probs=None, onehot=None, stream=None)
    for change, text in ((dict(N=0), "N=0"), (dict(HW=0), "HW=0"), (dict(K=0), "K=0"), (dict(K=256), "K=256"), (dict(known=None), "null"),
                         (dict(xt=None), "null"), (dict(xin=p, stride=1), "xin_stride"), (dict(mode=hip.STEP_SOFTMAX_ONLY), "mode")):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert text in hip.last_error(), (change, hip.last_error())


def test_known_labels_argument_validation():
    """Wrong shape, a value in [K,255), a non-integer dtype and rng = 'torch_cpu' raise ValueError naming the argument before anything
    runs (a model that was never moved to a GPU: nothing can run)."""
    m, _ = small_model(3)
    m.eval()
    N, K = 2, 3
    x = torch.nn.functional.one_hot(torch.zeros((N, H, W), dtype=torch.int64), K).permute(0, 3, 1, 2).float()
    cond = torch.zeros(N, 1, H, W)
    ok = torch.full((N, H, W), FREE, dtype=torch.int64)
    cases = [("shape", torch.full((N, H, W + 1), FREE, dtype=torch.int64)), ("shape", torch.full((N, 1, H, W), FREE, dtype=torch.int64)),
             ("values", torch.full((N, H, W), K, dtype=torch.int64)), ("values", torch.full((N, H, W), 254, dtype=torch.uint8)),
             ("values", torch.full((N, H, W), -1, dtype=torch.int64)), ("values", torch.full((N, H, W), 256, dtype=torch.int64)),
             ("integer", torch.zeros((N, H, W), dtype=torch.float32)), ("integer", torch.zeros((N, H, W), dtype=torch.bool))]
    for text, bad in cases:
        for call in (lambda kl: m(x, cond, t=T_STRIDED, known_labels=kl), lambda kl: m.forward_denoising(x, cond, None, 10004, known_labels=kl)):
            with pytest.raises(ValueError, match="known_labels.*" + text):
                call(bad)
        with pytest.raises(ValueError, match="known_labels.*" + text):
            m.predict_multiple(cond, num_evaluations=2, voting="majority", t=T_STRIDED, known_labels=bad)
    m.rng = "torch_cpu"
    with pytest.raises(ValueError, match="known_labels.*torch_cpu"):
        m(x, cond, t=T_STRIDED, known_labels=ok)
    with pytest.raises(ValueError, match="known_labels.*torch_cpu"):
        m.predict_multiple(cond, num_evaluations=2, voting="majority", known_labels=ok)
    m.rng = "philox"
    with pytest.raises(ValueError, match="known_labels"):
        m(x, cond, t=torch.full((N,), 3.0), validation=True, known_labels=ok)       # forward_step has no walk to condition
    assert m.philox_call == 0 and m._engines == {}          # nothing ran
    # the accepted forms: any integer dtype, classes and 255
    good = torch.full((N, H, W), FREE, dtype=torch.int32)
    good[:, :4] = 2
    u8 = guidance.check_known_labels(m, good, (N, H, W), K)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (N, H * W) and torch.equal(u8.reshape(N, H, W).int(), good)


def test_sample_sharded_hands_the_callers_slice_through():
    """distributed.sample_sharded slices x and the conditions, not known_labels: the caller passes its shard's slice."""
    kl = torch.full((3, 4, 4), FREE)
    assert sample_sharded_keywords(known_labels=kl)["known_labels"] is kl
    assert "known_labels" not in sample_sharded_keywords()


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run_kernel(lib, known, xt, K, c, mode, *, step_row=0, seed=SEED, sample_offset=0, xin=None, probs=None, onehot=None):
    """known, xt: uint8 [N,HW] cpu; xin [N,HW,stride] / probs [N,HW,K] / onehot [N,HW,K] cpu or None.  Returns the buffers after the
    launch (cpu)."""
    N, HW = known.shape
    d = {k: (None if v is None else v.contiguous().to(DEV)) for k, v in dict(known=known, xt=xt, xin=xin, probs=probs, onehot=onehot).items()}
    p_hit, p_miss = probabilities(c, K)

    def ptr(name):
        return None if d[name] is None else d[name].data_ptr()
    hip.check(getattr(lib, SYMBOL)(ptr("known"), N, HW, K, float(p_hit), float(p_miss), mode, step_row, seed, sample_offset, ptr("xt"),
                                   ptr("xin"), 0 if xin is None else xin.shape[2], ptr("probs"), ptr("onehot"), 0), SYMBOL)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in d.items()}


def masks(rng, N, HW, K):
    """all free, all known, a random half with stray bytes in [K,255) (which count as free)"""
    labels = rng.integers(0, K, (N, HW))
    half = np.where(rng.random((N, HW)) < 0.5, labels, FREE)
    if K < FREE - 1:
        stray = rng.random((N, HW)) < 0.1
        half = np.where(stray, rng.integers(K, FREE, (N, HW)), half)
    return {"free": np.full((N, HW), FREE), "all": labels, "half": half}


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", [(3, 63, 2), (2, 256, 3), (2, 256, 5), (2, 64, 20), (1, 64, 255)])
def test_clamp_kernel_equals_the_restatement(lib, N, HW, K):
    """STEP_SAMPLE: xt and the one-hot channels equal the numpy restatement at the known pixels and are bit-identical to their input at
    the free ones (stray bytes in [K,255) included); the image channels >= K survive; c = 1 gives the label; the draw moves with the
    sample offset and the step row."""
    rng = np.random.default_rng(1000 + K)
    stride = (K + 4) // 4 * 4 + 1                     # > K, and no multiple of 4
    for tag, known in masks(rng, N, HW, K).items():
        is_known = known < K
        xt0 = rng.integers(0, K, (N, HW))
        xin0 = rng.standard_normal((N, HW, stride)).astype(np.float32)           # (junk in the one-hot channels of the free pixels must stay)
        draws = {}
        for c in (0.0, 0.37, 1.0):
            for off, row, with_xin in ((0, 0, True), (5, 3, False), (5, 3, True), (0, 3, True)):
                r = run_kernel(lib, torch.from_numpy(known.astype(np.uint8)), torch.from_numpy(xt0.astype(np.uint8)), K, c, hip.STEP_SAMPLE,
                               step_row=row, sample_offset=off, xin=torch.from_numpy(xin0) if with_xin else None)
                want = clamp_restatement(known, xt0, K, c, row, SEED, off)
                got = r["xt"].numpy().astype(np.int64)
                what = f"{tag} c={c} off={off} row={row} xin={with_xin}"
                assert np.array_equal(got[~is_known], xt0[~is_known]), what + ": a free pixel of xt changed"
                assert np.array_equal(got, want), what + f": {int((got != want).sum())} known pixels differ from the restatement"
                assert np.array_equal(r["known"].numpy(), known.astype(np.uint8))
                if c == 1.0:
                    assert np.array_equal(got[is_known], known[is_known]), what
                if with_xin:
                    xin = r["xin"].numpy()
                    assert np.array_equal(xin[..., K:].view(np.uint32), xin0[..., K:].view(np.uint32)), what + ": an image channel changed"
                    assert np.array_equal(xin[~is_known].view(np.uint32), xin0[~is_known].view(np.uint32)), what + ": xin of a free pixel changed"
                    assert np.array_equal(xin[..., :K][is_known], onehot_np(want, K)[is_known].astype(np.float32)), what
                draws[(c, off, row)] = got
        if tag != "free" and K < 255:
            # (c = 0.37: a fair share of the pixels leave their label, and which ones depends on the counters)
            assert not np.array_equal(draws[(0.37, 0, 3)], draws[(0.37, 5, 3)]) and not np.array_equal(draws[(0.37, 0, 3)], draws[(0.37, 0, 0)])
        if tag == "all" and K < 255:
            # P(x != y) = (1 - c)(K - 1)/K <= 0.63; N*HW >= 128 draws: a standard deviation <= sqrt(0.25 / 128) = 0.044
            left = (draws[(0.37, 0, 0)] != known).mean()
            assert abs(left - 0.63 * (K - 1) / K) < 0.2, left
    # sharding: samples 1.. of a batch at offset 5 are samples 0.. of a batch at offset 6
    known = masks(rng, N, HW, K)["all"]
    if N > 1:
        a = run_kernel(lib, torch.from_numpy(known.astype(np.uint8)), torch.zeros((N, HW), dtype=torch.uint8), K, 0.37, hip.STEP_SAMPLE,
                       step_row=2, sample_offset=5)
        b = run_kernel(lib, torch.from_numpy(known[1:].astype(np.uint8)), torch.zeros((N - 1, HW), dtype=torch.uint8), K, 0.37,
                       hip.STEP_SAMPLE, step_row=2, sample_offset=6)
        assert torch.equal(a["xt"][1:], b["xt"])


@pytest.mark.gpu
@pytest.mark.parametrize("N,HW,K", [(3, 63, 2), (2, 256, 5), (1, 64, 255)])
def test_clamp_kernel_last_step_modes(lib, N, HW, K):
    """The three last-step modes draw nothing: xt = y, exact one-hots in out_probs / out_onehot / xin at the known pixels, everything
    else untouched, whatever the seed, the probabilities, the step row."""
    rng = np.random.default_rng(2000 + K)
    stride = K + 3
    known = masks(rng, N, HW, K)["half"]
    is_known = known < K
    xt0 = rng.integers(0, K, (N, HW))
    xin0 = rng.standard_normal((N, HW, stride)).astype(np.float32)
    probs0 = rng.random((N, HW, K)).astype(np.float32)
    onehot0 = rng.integers(-5, 5, (N, HW, K))
    want_oh = onehot_np(known, K)
    for mode in (hip.STEP_LAST_CONFIDENCE, hip.STEP_LAST_MAJORITY, hip.STEP_LAST_KEEP):
        outs = []
        for seed, c, row, with_out in ((1, 1.0, 0, True), (SEED, 0.37, 4, True), (1, 1.0, 0, False)):
            r = run_kernel(lib, torch.from_numpy(known.astype(np.uint8)), torch.from_numpy(xt0.astype(np.uint8)), K, c, mode, step_row=row,
                           seed=seed, sample_offset=row, xin=torch.from_numpy(xin0) if with_out else None,
                           probs=torch.from_numpy(probs0) if with_out else None, onehot=torch.from_numpy(onehot0) if with_out else None)
            xt = r["xt"].numpy().astype(np.int64)
            assert np.array_equal(xt, np.where(is_known, known, xt0)), mode
            if with_out:
                probs, onehot, xin = r["probs"].numpy(), r["onehot"].numpy(), r["xin"].numpy()
                assert np.array_equal(probs[is_known], want_oh[is_known].astype(np.float32)) and probs.dtype == np.float32
                assert np.array_equal(onehot[is_known], want_oh[is_known].astype(np.int64)) and onehot.dtype == np.int64
                assert np.array_equal(probs[~is_known].view(np.uint32), probs0[~is_known].view(np.uint32))
                assert np.array_equal(onehot[~is_known], onehot0[~is_known])
                assert np.array_equal(xin[..., :K][is_known], want_oh[is_known].astype(np.float32))
                assert np.array_equal(xin[..., K:].view(np.uint32), xin0[..., K:].view(np.uint32))
                assert np.array_equal(xin[~is_known].view(np.uint32), xin0[~is_known].view(np.uint32))
                outs.append((xt, probs, onehot, xin))
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])), "a last-step output depends on the seed"


@pytest.mark.gpu
def test_clamp_kernel_refuses_bad_arguments(lib):
    N, HW, K = 2, 64, 3
    known = torch.zeros((N, HW), dtype=torch.uint8, device=DEV)
    xt = torch.full((N, HW), 2, dtype=torch.uint8, device=DEV)
    xin = torch.full((N, HW, 4), 7.5, device=DEV)
    good = dict(known=known.data_ptr(), N=N, HW=HW, K=K, p_hit=1.0, p_miss=0.0, mode=hip.STEP_SAMPLE, step_row=0, seed=0, off=0,
                xt=xt.data_ptr(), xin=xin.data_ptr(), stride=4, probs=None, onehot=None, stream=0)
    for change in (dict(N=0), dict(N=-1), dict(HW=0), dict(K=0), dict(K=256), dict(known=None), dict(xt=None), dict(stride=2),
                   dict(mode=hip.STEP_SOFTMAX_ONLY), dict(mode=-1), dict(step_row=-1)):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert "known_labels_step" in hip.last_error()
    torch.cuda.synchronize()
    assert bool((xt == 2).all()) and bool((xin == 7.5).all())           # nothing was launched
    assert getattr(lib, SYMBOL)(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((xt == 0).all()) and bool((xin[..., :K].cpu() == torch.tensor([1.0, 0.0, 0.0])).all()) and bool((xin[..., K:] == 7.5).all())


# ------------------------------------------------------------------------------------------------ GPU: the sampler
@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def sampler(request):
    """K = 2: stem conv and fused head-and-posterior launch (x_t travels as the uint8 index only); K = 5: the general epilogue, which
    writes the one-hot into the stem's input."""
    return make_sampler(request.param)


@pytest.mark.gpu
@pytest.mark.parametrize("vote", ["majority", "confidence"])
def test_without_known_labels_nothing_changes(sampler, vote):
    """known_labels = None, an all-free map and a call without the keyword give bit-identical outputs."""
    s, model = sampler, sampler["model"]
    settings(model, step_T_sample=vote, substreams=0, use_graph=True)
    plain = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()
    none = model(s["x"], s["image"], t=T_STRIDED, known_labels=None)["diffusion_out"].clone()
    free = model(s["x"], s["image"], t=T_STRIDED, known_labels=torch.full((s["N"], H, W), FREE, dtype=torch.uint8))["diffusion_out"].clone()
    assert plain.dtype == (torch.int64 if vote == "majority" else torch.float32)
    assert torch.equal(plain, none) and torch.equal(plain, free)
    assert plain.dtype == free.dtype and plain.stride() == free.stride()
    settings(model, step_T_sample="majority")


@pytest.mark.gpu
def test_known_pixels_come_back_as_their_labels(sampler):
    """30 % of the pixels known: the returned map is exactly the label there — an int64 one-hot (majority), an fp32 one-hot
    (confidence), the kept index (a walk that stops above t = 1); with every pixel known the output is the label map."""
    s, model = sampler, sampler["model"]
    K, known, labels = s["K"], s["known"], s["labels"]
    is_known = known < K
    assert 0.2 < is_known.float().mean() < 0.4
    try:
        for vote, t, dtype in (("majority", T_STRIDED, torch.int64), ("confidence", T_STRIDED, torch.float32), ("majority", T_ONE_STEP, torch.float32),
                               (None, T_STRIDED, torch.int64), ("keep", T_STRIDED, torch.float32)):
            settings(model, step_T_sample=vote)
            out = model(s["x"], s["image"], t=t, known_labels=known.to(DEV))["diffusion_out"].cpu()
            assert out.dtype == dtype and tuple(out.shape) == (s["N"], K, H, W), (vote, int(t))
            want = O.one_hot_bchw(torch.where(is_known, known, torch.zeros_like(known)), K, dtype)
            mask = is_known[:, None].expand_as(out)
            assert torch.equal(out[mask], want[mask]), (vote, int(t))
            if not (vote == "confidence" and int(t) == 10004):
                assert torch.equal(out.sum(1), torch.ones_like(out.sum(1)))                  # a one-hot everywhere
            plain = model(s["x"], s["image"], t=t)["diffusion_out"].cpu()
            assert not torch.equal(plain[mask], want[mask]), "the unconditioned walk does not hit random labels"
            full = model(s["x"], s["image"], t=t, known_labels=labels.int())["diffusion_out"].cpu()           # (a CPU int32 map: accepted too)
            assert torch.equal(full, O.one_hot_bchw(labels, K, dtype)), (vote, int(t))
    finally:
        settings(model, step_T_sample="majority")


@pytest.mark.gpu
def test_conditioned_samples_do_not_depend_on_the_execution_shape(sampler):
    """N = 4: bit-identical across substreams 1 / 2, graph replay on / off, and two calls of two samples at sample_offset 0 / 2 with the
    matching slices of known_labels; another philox_seed changes free pixels of a walk that does not end at t = 1."""
    s, model = sampler, sampler["model"]
    known = s["known"].to(DEV)
    try:
        for t in (T_STRIDED, T_ONE_STEP):
            outs = {}
            for sub, graph in ((1, True), (2, True), (1, False), (2, False)):
                settings(model, substreams=sub, use_graph=graph, step_T_sample="majority")
                outs[(sub, graph)] = model(s["x"], s["image"], t=t, known_labels=known)["diffusion_out"].clone()
                assert model.last_mode == (sub, graph)
            ref = outs[(1, True)]
            assert all(torch.equal(ref, v) for v in outs.values()), int(t)
            halves = []
            for lo in (0, 2):
                settings(model, substreams=1, use_graph=True, sample_offset=lo)
                halves.append(model(s["x"][lo:lo + 2], s["image"][lo:lo + 2], t=t, known_labels=known[lo:lo + 2])["diffusion_out"].clone())
            settings(model, sample_offset=0)
            assert torch.equal(torch.cat(halves, 0), ref), int(t)
        # (ref: the one-step walk, the kept index as an fp32 one-hot)
        settings(model, philox_seed=100)
        other = model(s["x"], s["image"], t=T_ONE_STEP, known_labels=known)["diffusion_out"]
        free = (s["known"] == FREE)[:, None].expand_as(ref).to(DEV)
        assert not torch.equal(other[free], ref[free]) and torch.equal(other[~free], ref[~free])
    finally:
        settings(model, philox_seed=99, substreams=0, use_graph=True, sample_offset=0)


def oracle_conditioned_walk(sd, K, x, image, known, t_values, seed):
    """The conditioned loop restated from the oracle's step functions: U-Net forward, posterior, clamp and normalisation (the cascade
    order the epilogue implements), sample_index on philox_exponential's noise, and the clamp restatement between the steps (the last
    row with cumalpha = 1).  Returns every step's class map [N,H,W] after its clamp."""
    _, alphas, cum = O.make_schedule("cosine", T_SMALL, {"s": 0.008})
    N = x.shape[0]
    kn = known.reshape(N, H * W).numpy()
    xt, maps = x, []
    for j, t in enumerate(t_values):
        x0pred = O.unet_forward(sd, SMALL_CFG, xt, image, None, torch.full((N,), float(t)))["diffusion_out"]
        a, c = O.posterior_coeffs(alphas, cum, t)
        p_hat = O.normalise_probs(torch.clamp(O.theta_post_prob_ref(xt, x0pred, a, c), min=1e-12), "cascade")
        if t > 1:
            e = torch.from_numpy(O.philox_exponential(seed, j, 0, N, H * W, K)).reshape(N, H, W, K)
            idx = O.sample_index(p_hat, e)
        else:
            idx = p_hat.argmax(dim=-1)
        idx = clamp_restatement(kn, idx.reshape(N, H * W).numpy(), K, 1.0 if j == len(t_values) - 1 else c, j, seed, 0)
        idx = torch.from_numpy(idx).reshape(N, H, W)
        maps.append(idx)
        xt = O.one_hot_bchw(idx, K)
    return maps


@pytest.mark.gpu
def test_conditioned_walk_against_the_oracle_step_by_step(sampler, monkeypatch):
    """The seeded 4-step strided walk with 30 % of the pixels known, default precision (PREC_F16X3), free-running: every step's class
    map after its clamp equals the oracle restatement's — the assertion of the seeded free-running walks of test_hip_parity
    (FREE_RUN_FRAC = 0: equality).  The device's per-step maps are read from the engine right behind each clamp launch."""
    s, model = sampler, sampler["model"]
    K, N = s["K"], 2
    lib = hip.load()
    real = getattr(lib, SYMBOL)
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    eng = model._engine(s["x"][:N], s["image"][:N], None)
    seen = []

    def spy(*args):
        rc = real(*args)
        assert args[10] == eng.xt.data_ptr()
        with torch.cuda.stream(eng.stream):
            seen.append((args[7], args[6], eng.xt.clone()))
        return rc
    monkeypatch.setattr(lib, SYMBOL, spy)
    out = model(s["x"][:N], s["image"][:N], t=T_STRIDED, known_labels=s["known"][:N])["diffusion_out"].cpu()
    monkeypatch.undo()
    t_values = [6, 4, 3, 1]
    assert [r for r, _, _ in seen] == [0, 1, 2, 3]
    assert [m for _, m, _ in seen] == [hip.STEP_SAMPLE] * 3 + [hip.STEP_LAST_MAJORITY]
    ref = oracle_conditioned_walk(s["sd"], K, s["x_cpu"][:N], s["image_cpu"][:N], s["known"][:N], t_values, model._philox_key())
    for j, (_, _, xt) in enumerate(seen):
        got = xt.cpu().reshape(N, H, W).long()
        mism = (got != ref[j]).float().mean().item()
        print(f"conditioned walk K={K} step {j} (t={t_values[j]}): class mismatch {mism:.2e}")
        assert mism == 0.0, (j, mism)
    assert torch.equal(out, O.one_hot_bchw(ref[-1], K, torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
@pytest.mark.parametrize("voting", ["majority", "confidence"])
def test_predict_multiple_is_conditioned_in_every_pass(sampler, voting, batched):
    """S = 3: `vote` equals the label and `entropy` is exactly 0 at the known pixels; the free pixels are still sampled."""
    s, model = sampler, sampler["model"]
    K, B = s["K"], 2
    known = s["known"][:B]
    is_known = known < K
    settings(model, substreams=0, use_graph=True, philox_advance=True, philox_call=0)
    try:
        out = model.predict_multiple(s["image"][:B], num_evaluations=3, voting=voting, t=T_STRIDED, batched=batched, known_labels=known,
                                     maps=("mean", "vote", "entropy"))
        vote, ent, mean = out["vote"].cpu(), out["entropy"].cpu(), out["mean"].cpu()
        assert torch.equal(vote[is_known], known[is_known])
        assert bool((ent[is_known] == 0).all())
        assert torch.equal(mean.permute(0, 2, 3, 1)[is_known], torch.nn.functional.one_hot(known[is_known], K).float())
        assert model.philox_call == (1 if batched else 3)
        assert bool((ent[~is_known] > 0).any())
    finally:
        settings(model, philox_advance=False, philox_call=0)
