"""Flip-averaged sampling: DenoisingModel(..., views=) and the fused view-mean-and-draw step kernel ccdm_views_step (include/ccdm_hip.h
has the definition).  The numpy restatement below is the definition's mirror map and view mean in fp32 in front of the shaped tests'
restatement of the step; it is held against np.flip and float64 on the CPU, the kernel is held bit for bit against it (and against
float64 to the shaped test's counted bound where a power is formed) and against ccdm_shaped_step itself where the definition says the
two agree, and the sampler is checked launch by launch on the device's own inputs, free-running against the oracle's loop with its
denoiser wrapped in the view mean, for exact equivariance end to end, and for what must not change."""
import itertools

import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import guidance, hip
from ccdm_stochastic_segmentation_amd.models import DenoisingModel, Guidance
from tests.guided_util import (POWER_ERROR_ALLOWED, bits, coefficients, mixed_inputs, nhwk, posterior64, run_shaped_kernel, sampler_evidence, shape_rows,
                               shaped_restatement, threshold_margin64, weighted)
from tests.ladder_util import RUNG_KS, rung_of
from tests.sampler_util import (DEV, H, SEED, SMALL_CFG, T_SMALL, T_STRIDED, W, assert_symbol_declared_bound_and_built, load_lib, make_sampler,
                                onehot_np, sample_sharded_keywords, settings, small_model)

SYMBOL = "ccdm_views_step"
T_VALUES = [6, 4, 3, 1]          # t = 10004 walks the small model strided
HFLIP, VFLIP, HVFLIP = 1, 2, 3   # the kernel's two bits per view: bit 0 mirrors x, bit 1 mirrors y
# every flip combination the API can hand to the kernel: the ordered selections of distinct names (the sum runs in view order)
API_FLIPS = [c for n in range(4) for c in itertools.permutations((HFLIP, VFLIP, HVFLIP), n)]
MODES = (hip.STEP_SAMPLE, hip.STEP_LAST_CONFIDENCE, hip.STEP_LAST_MAJORITY, hip.STEP_LAST_KEEP)


# ------------------------------------------------------------------------------------------------ the definition, restated
def view_source(Hh, Ww, f):
    """src_v of the definition for every pixel y * W + x of the identity view: the flat index of the pixel of a view with flip bits f
    that shows it"""
    y, x = np.divmod(np.arange(Hh * Ww), Ww)
    return (Hh - 1 - y if f & 2 else y) * Ww + (Ww - 1 - x if f & 1 else x)


def view_mean(x0v, N, Hh, Ww, flips):
    """m of the definition: x0v fp32 [V*N,HW,K] view-major -> fp32 [N,HW,K], summed in view order in fp32, one multiply by fp32(1/V)"""
    x0v = np.ascontiguousarray(x0v, dtype=np.float32)
    acc = x0v[:N].copy()
    for v, f in enumerate(flips, 1):
        acc = (acc + x0v[v * N:(v + 1) * N][:, view_source(Hh, Ww, f)]).astype(np.float32)
    return (acc * (np.float32(1.0) / np.float32(1 + len(flips)))).astype(np.float32)


def scatter_views(idx, N, Hh, Ww, flips):
    """The class map idx [N,HW] of the identity view as the xt rows of all views [V*N,HW]: xt[v*N+n][src_v] = idx[n]"""
    out = [idx]
    for f in flips:
        row = np.empty_like(idx)
        row[:, view_source(Hh, Ww, f)] = idx
        out.append(row)
    return np.concatenate(out, 0)


def views_restatement(x0v, ev, xtv, N, Hh, Ww, flips, inv_tau, r, a, c, mode, step_row, seed, sample0):
    """What ccdm_views_step computes: the view mean, then shaped_restatement on it with view 0's x_t and the counters of samples
    sample0 .. sample0 + N - 1.  Returns (probabilities fp32 [N,HW,K], class index int64 [N,HW], xt of every view after the launch
    [V*N,HW] int64)."""
    xtv = np.asarray(xtv).astype(np.int64)
    probs, idx = shaped_restatement(view_mean(x0v, N, Hh, Ww, flips), ev, xtv[:N], inv_tau, r, a, c, mode, step_row, seed, sample0)
    xt_after = scatter_views(idx, N, Hh, Ww, flips) if mode in (hip.STEP_SAMPLE, hip.STEP_LAST_MAJORITY) else xtv
    return probs, idx, xt_after


def flip_bchw(a, f):
    """[...,h,w] tensor mirrored as flip bits f say"""
    dims = [d for b, d in ((1, -1), (2, -2)) if f & b]
    return torch.flip(a, dims) if dims else a


def mirrored_rows(rows, N, Hh, Ww, flips):
    """View-major [V*N,HW,...] rows whose views >= 1 are exact mirror images of `rows` [N,HW,...] (view 0)"""
    out = [rows]
    for f in flips:
        v = np.empty_like(rows)
        v[:, view_source(Hh, Ww, f)] = rows
        out.append(v)
    return np.concatenate(out, 0)


# ------------------------------------------------------------------------------------------------ CPU
def test_views_symbol_declared_bound_and_built():
    """hip.py binds the symbol with argtypes that match the header's declaration (22 arguments), the source is in the build list, the
    library cross-built from it exports it under the unchanged ABI number, and every bad argument is refused before anything is launched
    (host pointers: a launch would fault) with the expected word and the entry's name in the error string."""
    lib = assert_symbol_declared_bound_and_built(SYMBOL, 22, "ccdm_guided.hip")
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    good = dict(x0=p, ev=p, N=1, H=2, W=4, K=2, V=2, flips=HFLIP << 2, inv=1.0, r=1.0, a=0.5, c=0.5, mode=hip.STEP_SAMPLE, step_row=0, seed=0,
                off=0, xt=p, xin=None, stride=4, probs=None, onehot=None, stream=None)
    nan, inf = float("nan"), float("inf")
    for change, text in ((dict(V=0), "V=0"), (dict(V=5, flips=0), "V=5"), (dict(V=-1), "V=-1"), (dict(flips=1), "flips"),
                         (dict(flips=(HFLIP << 2) | 2), "flips"), (dict(V=1), "flips"), (dict(flips=1 << 4), "flips"), (dict(flips=-4), "flips"),
                         (dict(N=0), "N=0"), (dict(N=-1), "N=-1"), (dict(H=0), "H=0"), (dict(W=0), "W=0"), (dict(W=-3), "W=-3"),
                         (dict(H=2 ** 16, W=2 ** 16), "bad shape"), (dict(K=0), "K=0"), (dict(K=256), "K=256"), (dict(x0=None), "null"),
                         (dict(xt=None), "null"), (dict(xin=p, stride=1), "xin_stride"), (dict(mode=hip.STEP_SOFTMAX_ONLY), "mode"),
                         (dict(mode=7), "mode"), (dict(mode=-1), "mode"), (dict(step_row=-1), "step_row"),
                         (dict(N=2 ** 20, H=2 ** 5, W=2 ** 5), "too many pixels"), (dict(inv=nan), "inv_temperature"),
                         (dict(inv=inf), "inv_temperature"), (dict(inv=0.049), "inv_temperature"), (dict(inv=20.5), "inv_temperature"),
                         (dict(inv=-1.0), "inv_temperature"), (dict(r=nan), "top_r"), (dict(r=inf), "top_r"), (dict(r=0.0), "top_r"),
                         (dict(r=-0.5), "top_r"), (dict(r=1.0000001), "top_r")):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert text in hip.last_error() and SYMBOL in hip.last_error(), (change, hip.last_error())


@pytest.mark.parametrize("Hh,Ww", [(3, 5), (9, 37), (4, 4)])
def test_the_restatement_meets_the_definition(Hh, Ww):
    """The mirror map is np.flip's; the fp32 view mean lies within its counted roundings of the float64 mean (V - 1 additions and one
    multiply by a rounded 1/V: (V + 1) half-ulps, relative); then shaped_restatement follows on m.  The three properties of the
    definition hold in the restatement: V = 1 is the shaped step bit for bit; views that are exact mirror images give the shaped step on
    view 0 bit for bit at V = 2 and 4, and xt rows that are mirror images of one another; at V = 2 the mean of a call on mirrored
    inputs is the mirror of the original call's mean, bit for bit."""
    N, K, HW = 2, 5, Hh * Ww
    rng = np.random.default_rng(900 + Ww)
    grid = np.arange(HW).reshape(Hh, Ww)
    for f, axes in ((0, ()), (HFLIP, (1,)), (VFLIP, (0,)), (HVFLIP, (0, 1))):
        src = view_source(Hh, Ww, f)
        assert np.array_equal(src.reshape(Hh, Ww), np.flip(grid, axes) if axes else grid)
        assert np.array_equal(src[src], np.arange(HW))                      # an involution: g^-1 = g
    a, c = coefficients(200)
    for flips in API_FLIPS:
        V = 1 + len(flips)
        x0v, ev, xtv = mixed_inputs(rng, V * N, HW, K)
        m = view_mean(x0v, N, Hh, Ww, flips)
        m64 = sum(x0v[v * N:(v + 1) * N][:, view_source(Hh, Ww, f)].astype(np.float64) for v, f in enumerate((0,) + flips)) / V
        assert np.all(np.abs(m - m64) <= (V + 2) * 2.0 ** -24 * m64)                # (V + 1 roundings; one more covers their products)
        probs, idx, xt_after = views_restatement(x0v, ev[:N], xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_SAMPLE, 2, SEED, 3)
        want = shaped_restatement(m, ev[:N], xtv[:N], 1.0, 0.6, a, c, hip.STEP_SAMPLE, 2, SEED, 3)
        assert np.array_equal(bits(probs), bits(want[0])) and np.array_equal(idx, want[1]) and np.array_equal(xt_after[:N], idx)
        for v, f in enumerate(flips, 1):                                   # the views' states are mirror images of view 0
            got = torch.from_numpy(xt_after[v * N:(v + 1) * N].reshape(N, Hh, Ww))
            assert torch.equal(got, flip_bchw(torch.from_numpy(idx.reshape(N, Hh, Ww)), f))
        if V == 1:
            assert np.array_equal(bits(m), bits(x0v))
        if V in (2, 4):                                                    # exact mirror images: the mean is view 0 itself
            mirrored = mirrored_rows(x0v[:N], N, Hh, Ww, flips)
            assert np.array_equal(bits(view_mean(mirrored, N, Hh, Ww, flips)), bits(x0v[:N]))
        if V == 2:                                                         # a + b = b + a: the call on mirrored inputs
            src = view_source(Hh, Ww, flips[0])
            swapped = np.concatenate([x0v[N:], x0v[:N]], 0)                # its view 0 is the original's view 1 and the reverse
            assert np.array_equal(bits(view_mean(swapped, N, Hh, Ww, flips)), bits(m[:, src]))


def test_views_keyword_validation():
    """Every refusal of guidance.check_views is a ValueError naming the keyword, through forward, forward_denoising and predict_multiple, before
    anything runs (a model that was never moved to a GPU: nothing can run); views=() and None give no guidance."""
    m, _ = small_model(3)
    m.eval()
    N, K = 2, 3
    x = torch.nn.functional.one_hot(torch.zeros((N, H, W), dtype=torch.int64), K).permute(0, 3, 1, 2).float()
    cond = torch.zeros(N, 1, H, W)

    def calls(model):
        return (lambda **kw: model(x, cond, t=T_STRIDED, **kw), lambda **kw: model.forward_denoising(x, cond, None, 10004, **kw),
                lambda **kw: model.predict_multiple(cond, num_evaluations=2, voting="majority", t=T_STRIDED, **kw))
    for value in (("flip",), ("hflip", "rot90"), ("hflip", "hflip"), ("hvflip", "vflip", "hvflip"), "hflip", 1, ("hflip", 2), {"hflip"},
                  ("identity",), (None,), torch.tensor([1])):
        for call in calls(m):
            with pytest.raises(ValueError, match="^views"):
                call(views=value)
    m.rng = "torch_cpu"
    for call in calls(m):
        with pytest.raises(ValueError, match="views.*torch_cpu"):
            call(views=("hflip",))
    m.rng = "philox"
    with pytest.raises(ValueError, match="views.*sampling call"):
        m(x, cond, t=torch.full((N,), 3.0), validation=True, views=("hflip",))
    m.train()
    with pytest.raises(ValueError, match="views.*sampling call"):
        m(x, cond, t=torch.full((N,), 3.0), views=("hflip",))
    with pytest.raises(ValueError, match="views.*sampling call"):
        m.forward_denoising(x, cond, None, 10004, views=("hflip",))
    m.eval()
    logits_model, _ = small_model(3, softmax_output=False)
    logits_model.eval()
    for call in calls(logits_model):
        with pytest.raises(ValueError, match="views.*softmax_output"):
            call(views=("vflip",))
    known = torch.full((N, H, W), 255, dtype=torch.int64)
    for call in calls(m):
        with pytest.raises(ValueError, match="^views.*known_labels"):
            call(views=("hflip",), known_labels=known)
        with pytest.raises(ValueError, match="^views.*known_labels"):
            call(views=("hflip",), known_labels=known, resample=(2, 2))
    with pytest.raises(ValueError, match="^views.*resample"):
        guidance.check_views(m, ("hflip",), resample=(2, 2))
    # a model that takes a feature_condition needs the features of every view
    feat_model, _ = small_model(3)
    feat_model.eval()
    feat_model.unet.spec.feature_condition_idx = [1]                       # (only the check reads it: nothing runs)
    for fc in (torch.zeros(N, 4, 8, 8), torch.zeros(3, N, 4, 8, 8), torch.zeros(2, N + 1, 4, 8, 8)):
        with pytest.raises(ValueError, match="^views.*feature_condition"):
            guidance.check_guidance(feat_model, dict(views=("hflip",)), (N, K, H, W), fc)
    assert guidance.check_guidance(feat_model, dict(views=("hflip",)), (N, K, H, W), torch.zeros(2, N, 4, 8, 8)).views == (HFLIP,)
    assert guidance.check_guidance(m, dict(views=("hflip",)), (N, K, H, W), torch.zeros(N, 4, 8, 8)).views == (HFLIP,)   # ignored there
    assert m.philox_call == 0 and m._engines == {} and logits_model._engines == {}          # nothing ran
    # the accepted forms and what they become
    assert guidance.check_views(m, None) is None and guidance.check_views(m, ()) is None and guidance.check_views(m, []) is None
    assert guidance.check_views(m, ("hflip",)) == (HFLIP,) and guidance.check_views(m, ["vflip", "hflip"]) == (VFLIP, HFLIP)
    assert guidance.check_views(m, ("hflip", "vflip", "hvflip")) == (HFLIP, VFLIP, HVFLIP) and DenoisingModel.VIEW_FLIPS["hvflip"] == HFLIP | VFLIP
    g = guidance.check_guidance(m, dict(views=()), (N, K, H, W))
    assert g == Guidance() and not g
    g = guidance.check_guidance(m, dict(views=("hvflip",)), (N, K, H, W))
    assert g and g.views == (HVFLIP,) and g.repeat_interleave(3).views == (HVFLIP,) and g.shaping is None


def test_sample_sharded_hands_views_through():
    assert sample_sharded_keywords(views=("hflip", "vflip"))["views"] == ("hflip", "vflip")
    assert "views" not in sample_sharded_keywords()
    # a per-view feature condition is sliced along its sample axis
    from ccdm_stochastic_segmentation_amd.distributed import sample_sharded
    seen = {}

    class Stub:
        rng, sample_offset, noise_slice = "philox", 0, None

        def __call__(self, x, cond, fc, **kw):
            seen["fc"] = tuple(fc.shape)
            return {"diffusion_out": x}
    sample_sharded(Stub(), torch.zeros(3, 2, 4, 4), torch.zeros(3, 1, 4, 4), torch.zeros(2, 3, 5, 2, 2), views=("hflip",))
    assert seen["fc"] == (2, 3, 5, 2, 2)
    sample_sharded(Stub(), torch.zeros(3, 2, 4, 4), torch.zeros(3, 1, 4, 4), torch.zeros(3, 5, 2, 2))
    assert seen["fc"] == (3, 5, 2, 2)


def test_the_sampling_params_key_carries_views():
    """`sampling: {views: [...]}` becomes the keyword (a tuple) next to temperature and truncation; view_features runs the encoder once
    per view on the mirrored image."""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    assert E.sampling_keywords({"sampling": {"views": ["hflip", "vflip"]}}) == {"views": ("hflip", "vflip")}
    assert E.sampling_keywords({"sampling": {"views": None, "truncation": 0.9}}) == {"truncation": 0.9}
    assert E.sampling_keywords({"sampling": {"temperature": 0.7, "views": ["hvflip"]}}) == {"temperature": 0.7, "views": ("hvflip",)}
    with pytest.raises(ValueError, match="sampling"):
        E.sampling_keywords({"sampling": {"view": ["hflip"]}})
    calls = []

    class Stub:
        step_T_sample = "majority"

        class diffusion:
            num_classes = 2

        def __call__(self, x, image, fc=None, **kw):
            calls.append(kw)
            return {"diffusion_out": x}
    E.predict_multiple(Stub(), torch.zeros(2, 1, 8, 8), {"sampling": {"views": ["hflip"]}})
    assert calls == [{"views": ("hflip",)}]
    image = torch.arange(2 * 1 * 3 * 4, dtype=torch.float32).reshape(2, 1, 3, 4)
    feats = E.view_features(lambda im: im[..., :2, :2] * 2, image, ("hflip", "hvflip"))
    assert tuple(feats.shape) == (3, 2, 1, 2, 2)
    assert torch.equal(feats[0], image[..., :2, :2] * 2) and torch.equal(feats[1], torch.flip(image, [3])[..., :2, :2] * 2)
    assert torch.equal(feats[2], torch.flip(image, [2, 3])[..., :2, :2] * 2)


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, inv_tau, r, a, c, mode, *, step_row=0, seed=SEED, sample_offset=0, xin=None, probs=None,
               onehot=None, alias=False):
    """x0v: fp32 [V*N,HW,K]; ev: [N,HW,K] or None; xtv: integer [V*N,HW]; xin [V*N,HW,stride] / probs / onehot numpy or None; alias:
    out_probs IS x0.  Returns the buffers after the launch (numpy)."""
    K = x0v.shape[2]
    V = 1 + len(flips)
    assert x0v.shape[:2] == (V * N, Hh * Ww)
    host = dict(x0=x0v, ev=ev, xt=np.asarray(xtv).astype(np.uint8), xin=xin, probs=probs, onehot=onehot)
    d = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in host.items()}

    def ptr(name):
        return None if d[name] is None else d[name].data_ptr()
    code = sum(f << (2 * v) for v, f in enumerate(flips, 1))
    hip.check(getattr(lib, SYMBOL)(ptr("x0"), ptr("ev"), N, Hh, Ww, K, V, code, float(inv_tau), float(r), float(a), float(c), mode, step_row, seed,
                                   sample_offset, ptr("xt"), ptr("xin"), 0 if xin is None else xin.shape[2],
                                   ptr("x0") if alias else ptr("probs"), ptr("onehot"), 0), SYMBOL)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


KERNEL_SHAPES = [(2, 3, 5), (2, 9, 37)]          # odd both ways, one partial block; 666 pixels: block edges at 256 and at 64
KERNEL_KS = sorted({2, 3, 4, 5, 20, 40} | set(RUNG_KS))          # both ends of every rung of the kernels' class-count ladder
TEMPERED_KS = [2, 5, 16, 24, 32, 40, 128]
MIRRORED_KS = [2, 16, 20, 32, 255]


@pytest.mark.gpu
@pytest.mark.parametrize("K", KERNEL_KS)
@pytest.mark.parametrize("N,Hh,Ww", KERNEL_SHAPES)
def test_views_kernel_equals_the_restatement(lib, N, Hh, Ww, K):
    """No power is formed (tau = 1): bit equality with the restatement for every flip combination of the API (V = 1 .. 4), all four
    step modes, with and without evidence, with and without xin (a stride > K that is no multiple of 4), a sample offset and a step row
    that are not 0, neutral shaping and truncation r = 0.6, x0 and out_probs the same buffer in the last-step modes.  Checked: xt of
    every view; the one-hot channels of xin of every view, and that its channels >= K are bit-unchanged; that x0 (all of it in sample,
    majority and keep mode, the rows of the views >= 1 in confidence mode), the evidence and what a mode does not write stay bit-
    unchanged."""
    rng = np.random.default_rng(9000 + 100 * Ww + K)
    HW = Hh * Ww
    stride = (K + 4) // 4 * 4 + 1
    off, row = 5, 3
    for flips in API_FLIPS:
        V = 1 + len(flips)
        x0v, ev_all, xtv = mixed_inputs(rng, V * N, HW, K)
        ev_all = ev_all[:N]
        xin0 = rng.standard_normal((V * N, HW, stride)).astype(np.float32)
        onehot0 = rng.integers(-5, 5, (V * N, HW, K))
        for r in (1.0, 0.6):
            for ev in (None, ev_all):
                a, c = coefficients(200 if r == 1.0 else 2)
                what = f"flips={flips} r={r} ev={ev is not None}"
                probs, idx, xt_after = views_restatement(x0v, ev, xtv, N, Hh, Ww, flips, 1.0, r, a, c, hip.STEP_SAMPLE, row, SEED, off)
                for with_xin in (True, False):
                    got = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, 1.0, r, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off,
                                     xin=xin0 if with_xin else None, onehot=onehot0, alias=True)
                    got_xt = got["xt"].astype(np.int64)
                    assert np.array_equal(got_xt, xt_after), what + f" xin={with_xin}: {int((got_xt != xt_after).sum())} of {xt_after.size} differ"
                    assert np.array_equal(bits(got["x0"]), bits(x0v)) and np.array_equal(got["onehot"], onehot0), what
                    assert ev is None or np.array_equal(bits(got["ev"]), bits(ev)), what
                    if with_xin:
                        assert np.array_equal(bits(got["xin"][..., K:]), bits(xin0[..., K:])), what + ": an image channel changed"
                        assert np.array_equal(got["xin"][..., :K], onehot_np(xt_after, K).astype(np.float32)), what
        # the last-step modes (t = 1 and a t inside the chain), truncating, evidence on alternate combinations
        ev = ev_all if len(flips) % 2 else None
        for t in (1, 3):
            a, c = coefficients(t, T_SMALL)
            what = f"flips={flips} t={t}"
            probs, idx, xt_after = views_restatement(x0v, ev, xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_LAST_MAJORITY, row, SEED, off)
            g = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_LAST_CONFIDENCE, xin=xin0, onehot=onehot0, alias=True)
            assert np.array_equal(bits(g["x0"][:N]), bits(probs)), what + f": {int((bits(g['x0'][:N]) != bits(probs)).sum())} probabilities differ"
            assert np.array_equal(bits(g["x0"][N:]), bits(x0v[N:])), what + ": a row of another view was written"
            assert np.array_equal(g["xt"], xtv.astype(np.uint8)) and np.array_equal(g["onehot"], onehot0), what
            assert np.array_equal(bits(g["xin"]), bits(xin0)), what
            g = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_LAST_MAJORITY, step_row=row, sample_offset=off,
                           xin=xin0, onehot=onehot0, alias=True)
            assert np.array_equal(g["xt"].astype(np.int64), xt_after), what
            assert np.array_equal(g["onehot"][:N], onehot_np(idx, K).astype(np.int64)) and np.array_equal(g["onehot"][N:], onehot0[N:]), what
            assert np.array_equal(bits(g["x0"]), bits(x0v)) and np.array_equal(bits(g["xin"]), bits(xin0)), what
            g = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_LAST_KEEP, xin=xin0, onehot=onehot0, alias=True)
            assert np.array_equal(g["xt"], xtv.astype(np.uint8)) and np.array_equal(g["onehot"], onehot0), what
            assert np.array_equal(bits(g["x0"]), bits(x0v)) and np.array_equal(bits(g["xin"]), bits(xin0)), what
    if True:            # samples 1.. of a batch at offset 5 are samples 0.. of a batch at offset 6: the draw is keyed by the sample
        flips = (HFLIP, HVFLIP)
        x0v, _, xtv = mixed_inputs(rng, 3 * N, HW, K)
        a, c = coefficients(200)
        full = run_kernel(lib, x0v, None, xtv, N, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=5)["xt"]
        keep = np.concatenate([np.arange(v * N + 1, (v + 1) * N) for v in range(3)])
        tail = run_kernel(lib, x0v[keep], None, xtv[keep], N - 1, Hh, Ww, flips, 1.0, 0.6, a, c, hip.STEP_SAMPLE, step_row=2, sample_offset=6)["xt"]
        assert np.array_equal(full[keep], tail)


def tempered_views_reference(K):
    """The float64 side of test_tempered_views_kernel_against_float64, from the definition and the oracle alone: the geometry and
    inv_temperature, the seeded inputs, and per (r, evidence, t) the coefficients, the float64 probabilities and the entries they are
    compared at."""
    N, Hh, Ww = 2, 9, 37
    flips = (VFLIP, HFLIP)
    rng = np.random.default_rng(9500 + K)
    x0v, ev_all, xtv = mixed_inputs(rng, 3 * N, Hh * Ww, K)
    inv = float(np.float32(1.0 / 0.7))
    m = view_mean(x0v, N, Hh, Ww, flips)
    cases = []
    for r in (1.0, 0.9):
        for ev in (None, ev_all[:N]):
            v = weighted(m, ev)
            q64 = shape_rows(v, inv, float(np.float32(r)), np.float64)
            near = threshold_margin64(shape_rows(v, inv, 1.0, np.float64), r) <= 1e-5 if r != 1.0 else np.zeros(v.shape[:2], dtype=bool)
            for t in (200, 2):
                a, c = coefficients(t)
                want = posterior64(q64, xtv[:N], a, c)
                cases.append((r, ev, t, (a, c), want, (want > 1e-9) & ~near[..., None]))
    return (N, Hh, Ww, flips, inv), (x0v, xtv), cases


@pytest.mark.gpu
@pytest.mark.parametrize("K", TEMPERED_KS)
def test_tempered_views_kernel_against_float64(lib, parity_log, K):
    """tau = 0.7 and r in {1, 0.9} at V = 3: the device's power is not numpy's, so the confidence-mode probabilities are held against
    the float64 form of the shaping and of the posterior on the fp32 view mean (and its fp32 product with the evidence), to the shaped
    test's bound: its 5 K + 31 counted roundings, the clamp's 2 K 1e-12 and POWER_ERROR_ALLOWED.  Entries > 1e-9 of pixels that are not
    within 1e-5 of a truncation threshold."""
    (N, Hh, Ww, flips, inv), (x0v, xtv), cases = tempered_views_reference(K)
    n = 5 * K + 31
    bound = n * 2.0 ** -24 / (1 - n * 2.0 ** -24) + 2 * K * 1e-12 + POWER_ERROR_ALLOWED
    worst = 0.0
    for r, ev, t, (a, c), want, big in cases:
        got = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, inv, r, a, c, hip.STEP_LAST_CONFIDENCE, alias=True)["x0"][:N].astype(np.float64)
        rel = float((np.abs(got - want)[big] / want[big]).max())
        worst = max(worst, rel)
        print(f"tempered views K={K} r={r} ev={ev is not None} t={t}: max relative error {rel:.3e} (bound {bound:.3e})")
        parity_log("ladder_views_step", **{f"rung{rung_of(K)}_K{K}_max_rel_err_vs_float64": worst, f"K{K}_bound": bound})
        assert big.mean() > 0.5 and rel <= bound, (r, ev is not None, t, rel, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("K", MIRRORED_KS)
def test_one_view_and_mirrored_views_are_the_shaped_step(lib, K):
    """Against ccdm_shaped_step itself on the device, bit for bit: V = 1 is that step; V = 2 and V = 4 on views whose x0 are exact
    mirror images of view 0 are that step on view 0 (xt in sample mode with tau = 0.7 and r = 0.8 — the same device power on the same
    bits — and the probabilities in confidence mode with x0 aliased), and the xt rows of all views are mirror images of view 0's."""
    N, Hh, Ww = 2, 9, 37
    HW = Hh * Ww
    rng = np.random.default_rng(9700 + K)
    x0, ev_all, xt = mixed_inputs(rng, N, HW, K)
    stride = K + 3
    xin0 = rng.standard_normal((N, HW, stride)).astype(np.float32)
    inv, r, row, off = float(np.float32(1.0 / 0.7)), 0.8, 2, 7
    for flips in ((), (HFLIP,), (VFLIP,), (HVFLIP,), (HFLIP, VFLIP, HVFLIP), (HVFLIP, HFLIP, VFLIP)):
        V = 1 + len(flips)
        x0v, xtv = mirrored_rows(x0, N, Hh, Ww, flips), mirrored_rows(xt, N, Hh, Ww, flips)
        xinv = np.concatenate([xin0] * V, 0)
        for ev in (None, ev_all):
            for t in (200, 2):
                a, c = coefficients(t)
                what = f"flips={flips} ev={ev is not None} t={t}"
                ref = run_shaped_kernel(lib, x0, ev, xt, inv, r, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off, xin=xin0)
                got = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, inv, r, a, c, hip.STEP_SAMPLE, step_row=row, sample_offset=off, xin=xinv)
                assert np.array_equal(got["xt"][:N], ref["xt"]), what
                assert np.array_equal(got["xt"], mirrored_rows(ref["xt"], N, Hh, Ww, flips)), what
                assert np.array_equal(bits(got["xin"][:N]), bits(ref["xin"])), what
                ref = run_shaped_kernel(lib, x0, ev, xt, inv, r, a, c, hip.STEP_LAST_CONFIDENCE, alias=True)["x0"]
                got = run_kernel(lib, x0v, ev, xtv, N, Hh, Ww, flips, inv, r, a, c, hip.STEP_LAST_CONFIDENCE, alias=True)["x0"]
                assert np.array_equal(bits(got[:N]), bits(ref)) and not np.array_equal(bits(ref), bits(x0)), what


@pytest.mark.gpu
def test_views_kernel_refuses_bad_arguments(lib):
    N, Hh, Ww, K, V = 2, 8, 8, 3, 2
    x0 = torch.full((V * N, Hh * Ww, K), 0.25, device=DEV)
    xt = torch.full((V * N, Hh * Ww), 2, dtype=torch.uint8, device=DEV)
    xin = torch.full((V * N, Hh * Ww, 4), 7.5, device=DEV)
    probs = torch.full((N, Hh * Ww, K), 3.5, device=DEV)
    onehot = torch.full((N, Hh * Ww, K), 9, dtype=torch.int64, device=DEV)
    good = dict(x0=x0.data_ptr(), ev=None, N=N, H=Hh, W=Ww, K=K, V=V, flips=HFLIP << 2, inv=2.0, r=0.5, a=0.0, c=1.0, mode=hip.STEP_LAST_MAJORITY,
                step_row=0, seed=0, off=0, xt=xt.data_ptr(), xin=xin.data_ptr(), stride=4, probs=probs.data_ptr(), onehot=onehot.data_ptr(),
                stream=0)
    for change in (dict(V=0), dict(V=5), dict(flips=1), dict(flips=HFLIP << 4), dict(N=0), dict(H=0), dict(W=-1), dict(K=0), dict(K=256),
                   dict(x0=None), dict(xt=None), dict(stride=2), dict(mode=hip.STEP_SOFTMAX_ONLY), dict(mode=5), dict(step_row=-1),
                   dict(inv=float("nan")), dict(inv=21.0), dict(r=0.0), dict(r=1.5)):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert SYMBOL in hip.last_error()
    torch.cuda.synchronize()
    assert bool((xt == 2).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all()) and bool((onehot == 9).all())    # nothing ran
    assert getattr(lib, SYMBOL)(*good.values()) == 0                       # flat rows: a tie, class 0, in every view
    torch.cuda.synchronize()
    assert bool((xt == 0).all()) and bool((onehot.cpu() == torch.tensor([1, 0, 0])).all()) and bool((xin == 7.5).all()) and bool((probs == 3.5).all())


# ------------------------------------------------------------------------------------------------ GPU: the sampler
EVIDENCE_SEED = 270


@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def sampler(request):
    """K = 2: stem conv and fused head-and-posterior launch (x_t travels as the uint8 index only); K = 5: the general epilogue, and the
    stem reads its one-hot from xin, which the views step writes for every view."""
    s = make_sampler(request.param)
    s["ev"], _, _ = sampler_evidence(np.random.default_rng(EVIDENCE_SEED + s["K"]), s["N"], s["K"])
    return s


def views_engine(model, x, image, V, slot=0):
    """The engine a call with V views of these inputs runs on (V times the rows)"""
    return model._engine(x.repeat(V, 1, 1, 1), image.repeat(V, 1, 1, 1), None, slot=slot)


class Spy:
    """Stands in for lib.ccdm_views_step: clones the launch's inputs (out_probs = x0, xt) before it and its outputs (xt, out_probs,
    out_onehot, xin) behind it, on the stream the launch runs on."""

    def __init__(self, lib, engines):
        self.real, self.engines, self.seen = getattr(lib, SYMBOL), {e.out_probs.data_ptr(): e for e in engines}, []

    def __call__(self, *args):
        eng = self.engines[args[0]]
        assert args[16] == eng.xt.data_ptr() and args[19] == args[0] and args[20] == eng.out_onehot.data_ptr()
        assert args[17] == (None if eng.stem_onehot_on_load else eng.xin.ptr)
        assert (args[3], args[4], args[5]) == (eng.H, eng.W, eng.K) and args[2] * args[6] == eng.N
        with torch.cuda.stream(eng.stream):
            before = dict(x0=eng.out_probs.clone(), xt=eng.xt.clone())
            rc = self.real(*args)
            after = dict(xt=eng.xt.clone(), probs=eng.out_probs.clone(), onehot=eng.out_onehot.clone(),
                         xin=None if eng.stem_onehot_on_load else eng.xin.buf.clone())
        self.seen.append(dict(ev=args[1], N=args[2], V=args[6], flips=args[7], inv=args[8], r=args[9], a=args[10], c=args[11], mode=args[12],
                              row=args[13], seed=args[14], off=args[15], before=before, after=after))
        return rc


def check_launch(rec, ev_nhwk, K):
    """One captured launch against the restatement on the launch's own inputs: exact (the callers temper with tau = 1 only)."""
    N, V = rec["N"], rec["V"]
    flips = tuple((rec["flips"] >> (2 * v)) & 3 for v in range(1, V))
    assert rec["inv"] == 1.0 and (rec["ev"] is None) == (ev_nhwk is None) and rec["flips"] & 3 == 0
    x0v = rec["before"]["x0"].cpu().numpy().reshape(V * N, H * W, K)
    xt0 = rec["before"]["xt"].cpu().numpy().reshape(V * N, H * W)
    for v, f in enumerate(flips, 1):          # what the launch relies on: the views' states are mirror images of view 0's
        assert np.array_equal(xt0[v * N:(v + 1) * N][:, view_source(H, W, f)], xt0[:N]), f"x_t of view {v} is not the mirror image"
    probs, idx, xt_after = views_restatement(x0v, ev_nhwk, xt0, N, H, W, flips, rec["inv"], rec["r"], rec["a"], rec["c"], rec["mode"],
                                             rec["row"], rec["seed"], rec["off"])
    got_xt = rec["after"]["xt"].cpu().numpy().reshape(V * N, H * W).astype(np.int64)
    got_probs = rec["after"]["probs"].cpu().numpy().reshape(V * N, H * W, K)
    what = f"row {rec['row']} mode {rec['mode']}"
    assert np.array_equal(got_xt, xt_after), what + f": {int((got_xt != xt_after).sum())} pixels differ"
    assert np.array_equal(bits(got_probs[N:]), bits(x0v[N:])), what
    if rec["mode"] == hip.STEP_SAMPLE:
        assert np.array_equal(bits(got_probs), bits(x0v)), what
        if rec["after"]["xin"] is not None:
            assert np.array_equal(rec["after"]["xin"].cpu().numpy().reshape(V * N, H * W, -1)[..., :K], onehot_np(xt_after, K).astype(np.float32)), what
    elif rec["mode"] == hip.STEP_LAST_MAJORITY:
        assert np.array_equal(rec["after"]["onehot"].cpu().numpy().reshape(V * N, H * W, K)[:N], onehot_np(idx, K).astype(np.int64)), what
    elif rec["mode"] == hip.STEP_LAST_CONFIDENCE:
        assert np.array_equal(bits(got_probs[:N]), bits(probs)), what
    return probs, idx


@pytest.mark.gpu
@pytest.mark.parametrize("views,extra", [(("hflip",), False), (("hflip", "vflip", "hvflip"), False), (("vflip", "hflip"), True)],
                         ids=["hflip", "all-three", "two-with-evidence-and-truncation"])
def test_every_views_step_equals_the_restatement_on_the_devices_inputs(sampler, views, extra, monkeypatch):
    """The strided 4-row walk: restating each launch from the x0 and x_t (of all views) it was handed reproduces what it left, exactly,
    in every view; the final output is the restated walk's.  Rows 0..3, modes [SAMPLE] * 3 + [LAST_MAJORITY], the real coefficients, the
    call's key and offset, N samples on V * N engine rows; with evidence and truncation too it is still one launch per entry, and neither
    ccdm_evidence_step nor ccdm_shaped_step is launched."""
    s, model = sampler, sampler["model"]
    K, N, V = s["K"], s["N"], 1 + len(views)
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    spy = Spy(lib, [views_engine(model, s["x"], s["image"], V)])
    monkeypatch.setattr(lib, SYMBOL, spy)
    others = []
    for name in ("ccdm_evidence_step", "ccdm_shaped_step"):
        monkeypatch.setattr(lib, name, lambda *a, _real=getattr(lib, name): (others.append(1), _real(*a))[1])
    kw = dict(evidence=s["ev"].to(DEV), truncation=0.6) if extra else {}
    out = model(s["x"], s["image"], t=T_STRIDED, views=views, **kw)["diffusion_out"].cpu()
    monkeypatch.undo()
    assert others == [] and model.last_mode == (1, True)
    assert [r["row"] for r in spy.seen] == [0, 1, 2, 3] and [r["mode"] for r in spy.seen] == [hip.STEP_SAMPLE] * 3 + [hip.STEP_LAST_MAJORITY]
    assert all(r["seed"] == model._philox_key() and r["off"] == 0 and r["N"] == N and r["V"] == V for r in spy.seen)
    assert all(r["flips"] == sum(DenoisingModel.VIEW_FLIPS[n] << (2 * v) for v, n in enumerate(views, 1)) for r in spy.seen)
    assert all((r["inv"], r["r"]) == (1.0, float(np.float32(0.6)) if extra else 1.0) for r in spy.seen)
    for r, t in zip(spy.seen, T_VALUES):
        a, c = model.diffusion.posterior_coeffs(t)
        assert (r["a"], r["c"]) == (a, c)
        assert bool(((r["before"]["x0"].sum(-1) - 1).abs() < 1e-5).all()), "the network pass did not stop at x0"
        _, idx = check_launch(r, nhwk(s["ev"]) if extra else None, K)
    assert tuple(out.shape) == (N, K, H, W) and torch.equal(out, O.one_hot_bchw(torch.from_numpy(idx).reshape(N, H, W), K, torch.int64))


WALK_R = 0.6
# test_views_walk_against_the_oracle_step_by_step: the small_model seed per K for which the oracle-only walk with views = ("hflip",)
# and truncation 0.6 keeps every race and argmax margin and every truncation-threshold margin >= 1e-4, found on the CPU from the
# oracle alone (the test prints and asserts the margins): 45 for K = 2 (margins 9.9e-4 / 2.0e-4; every seed from 3 to 26 comes within
# 1e-4 of a truncation threshold or of a race tie, seed 27 keeps 1.07e-4 only), 99 for K = 5 (1.38e-4 / 1.23e-4; no seed below it qualifies)
WALK_SEED = {2: 45, 5: 99}


def oracle_views_walk(sd, K, x, image, flips, r, t_values, seed):
    """The oracle's loop with its denoiser wrapped in the view mean (U-Net forward on the CPU on every mirrored input, view_mean on the
    outputs) and the restated shaped step (tau = 1) behind it.  Returns every step's class map [N,H,W], the smallest relative gap
    between the winner and the runner-up of any race or argmax, and the smallest relative distance of a prefix mass to a truncation
    threshold."""
    _, alphas, cum = O.make_schedule("cosine", T_SMALL, {"s": 0.008})
    N = x.shape[0]
    xt, maps, gap, edge = x, [], np.inf, np.inf
    for j, t in enumerate(t_values):
        x0v = np.concatenate([nhwk(O.unet_forward(sd, SMALL_CFG, flip_bchw(xt, f), flip_bchw(image, f), None,
                                                  torch.full((N,), float(t)))["diffusion_out"]) for f in (0,) + tuple(flips)], 0)
        m = view_mean(x0v, N, H, W, flips)
        a, c = O.posterior_coeffs(alphas, cum, t)
        mode = hip.STEP_SAMPLE if t > 1 else hip.STEP_LAST_MAJORITY
        probs, idx = shaped_restatement(m, None, xt.argmax(1).reshape(N, H * W).numpy(), 1.0, r, a, c, mode, j, seed, 0)
        score = probs.astype(np.float64) / (O.philox_exponential(seed, j, 0, N, H * W, K).astype(np.float64) if t > 1 else 1.0)
        top = np.sort(score, axis=-1)
        gap = min(gap, float(((top[..., -1] - top[..., -2]) / top[..., -1]).min()))
        edge = min(edge, float(threshold_margin64(m.astype(np.float64), r).min()))
        idx = torch.from_numpy(idx).reshape(N, H, W)
        maps.append(idx)
        xt = O.one_hot_bchw(idx, K)
    return maps, gap, edge


@pytest.mark.gpu
def test_views_walk_against_the_oracle_step_by_step(sampler, monkeypatch):
    """The seeded 4-step strided walk with views = ("hflip",) and truncation = 0.6, default precision (PREC_F16X3), N = 2, free-running:
    every step's class map equals the oracle's loop with its denoiser wrapped in the view mean.  A last-bit difference of the network can
    flip a pixel at the race and at the truncation threshold, so the test is valid for weights whose oracle-only walk keeps both margins
    >= 1e-4 at every step: WALK_SEED has the seed per K, computed on the CPU beforehand (the margins are printed and asserted here)."""
    s = sampler
    K, N, flips = s["K"], 2, (HFLIP,)
    model, sd = small_model(K, seed=WALK_SEED[K])
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, False
    lib = hip.load()
    settings(model, substreams=1, use_graph=True, step_T_sample="majority")
    spy = Spy(lib, [views_engine(model, s["x"][:N], s["image"][:N], 2)])
    monkeypatch.setattr(lib, SYMBOL, spy)
    out = model(s["x"][:N], s["image"][:N], t=T_STRIDED, views=("hflip",), truncation=WALK_R)["diffusion_out"].cpu()
    monkeypatch.undo()
    ref, gap, edge = oracle_views_walk(sd, K, s["x_cpu"][:N], s["image_cpu"][:N], flips, WALK_R, T_VALUES, model._philox_key())
    print(f"views walk K={K}: the oracle's smallest relative winner margin {gap:.2e}, smallest relative threshold margin {edge:.2e}")
    assert gap >= 1e-4 and edge >= 1e-4
    assert len(spy.seen) == 4
    for j, r in enumerate(spy.seen):
        got = r["after"]["xt"].cpu().reshape(2 * N, H, W).long()
        mism = (got[:N] != ref[j]).float().mean().item()
        print(f"views walk K={K} step {j} (t={T_VALUES[j]}): class mismatch {mism:.2e}")
        assert mism == 0.0, (j, mism)
        assert torch.equal(got[N:], torch.flip(ref[j], [2]))
    assert torch.equal(out, O.one_hot_bchw(ref[-1], K, torch.int64))


@pytest.mark.gpu
def test_a_flip_averaged_denoiser_is_exactly_equivariant(sampler):
    """views = ("hflip",), step_T_sample = "confidence", a single row with t = 1 (no draw): the output for (flip x, flip image) equals
    the flip of the output for (x, image), bit for bit — at V = 2 the mean's sum is commutative.  Without views the network alone is not
    equivariant to the bit: the two then differ somewhere (so the first statement is not vacuous)."""
    s, model = sampler, sampler["model"]
    settings(model, step_T_sample="confidence", substreams=1, use_graph=True)
    try:
        t1 = torch.as_tensor(1)
        xf, imf = torch.flip(s["x"], [3]).contiguous(), torch.flip(s["image"], [3]).contiguous()
        a = model(s["x"], s["image"], t=t1, views=("hflip",))["diffusion_out"].clone()
        b = model(xf, imf, t=t1, views=("hflip",))["diffusion_out"].clone()
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(s["x"].shape)
        assert torch.equal(b, torch.flip(a, [3]))
        a0 = model(s["x"], s["image"], t=t1)["diffusion_out"].clone()
        b0 = model(xf, imf, t=t1)["diffusion_out"].clone()
        differ = (b0 != torch.flip(a0, [3])).float().mean().item()
        print(f"equivariance K={s['K']}: without views {differ:.2e} of the probabilities differ from the mirrored call's")
        assert differ > 0.0
        assert not torch.equal(a, a0)
    finally:
        settings(model, step_T_sample="majority", substreams=0)


@pytest.mark.gpu
@pytest.mark.parametrize("vote", ["majority", "confidence"])
def test_without_views_nothing_changes(sampler, vote):
    """A plain call, views = None and views = () give bit-identical outputs (no views launch, the engine of N rows); a plain call after
    a call with views is unchanged; a call with views differs."""
    s, model = sampler, sampler["model"]
    settings(model, step_T_sample=vote, substreams=0, use_graph=True)
    lib = hip.load()
    launches = []
    real = getattr(lib, SYMBOL)
    try:
        setattr(lib, SYMBOL, lambda *a: (launches.append(1), real(*a))[1])
        plain = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()
        none = model(s["x"], s["image"], t=T_STRIDED, views=None)["diffusion_out"].clone()
        empty = model(s["x"], s["image"], t=T_STRIDED, views=())["diffusion_out"].clone()
        assert launches == []
        mean = model(s["x"], s["image"], t=T_STRIDED, views=("hflip", "vflip"))["diffusion_out"].clone()
        assert len(launches) == 4
        again = model(s["x"], s["image"], t=T_STRIDED)["diffusion_out"].clone()
        assert torch.equal(plain, none) and torch.equal(plain, empty) and torch.equal(plain, again)
        assert plain.dtype == mean.dtype and plain.shape == mean.shape and plain.stride() == mean.stride()
        assert not torch.equal(plain, mean)
    finally:
        setattr(lib, SYMBOL, real)
        settings(model, step_T_sample="majority")


@pytest.mark.gpu
def test_view_samples_do_not_depend_on_the_execution_shape(sampler):
    """N = 4, views = ("hflip", "hvflip") with truncation = 0.8: bit-identical across substreams 1 / 2, graph replay on / off, and two
    calls of two samples at sample_offset 0 / 2 (the draw is keyed by the sample, never by the engine row)."""
    s, model = sampler, sampler["model"]
    kw = dict(t=T_STRIDED, views=("hflip", "hvflip"), truncation=0.8)
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
@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
def test_predict_multiple_with_views_equals_the_per_pass_calls(sampler, batched):
    """S = 3, views = ("hflip",), majority voting: the counts equal the sum of the one-hot outputs of the per-pass calls — S calls of B
    samples under advancing philox_call (sequential), or the one call of B * S samples (batched: sample b * S + s is pass s of image b)
    — so the consumer reads view 0's rows of an engine that holds V times as many; with confidence voting the mean is the reference's
    fp32 accumulation of the per-pass probabilities, bit for bit."""
    s, model = sampler, sampler["model"]
    K, B, S = s["K"], 2, 3
    views = ("hflip",)
    x = O.one_hot_bchw(torch.from_numpy(np.random.default_rng(17).integers(0, K, (S * B, H, W))), K).reshape(S, B, K, H, W).to(DEV)
    image = s["image"][:B]
    try:
        for voting in ("majority", "confidence"):
            settings(model, substreams=1, use_graph=True, philox_advance=True, philox_call=0, step_T_sample=voting)
            if batched:
                per = model(x.transpose(0, 1).reshape(B * S, K, H, W), image.repeat_interleave(S, dim=0), t=T_STRIDED, views=views)["diffusion_out"]
                passes = [per.reshape(B, S, K, H, W)[:, i] for i in range(S)]
            else:
                passes = [model(x[i], image, t=T_STRIDED, views=views)["diffusion_out"].clone() for i in range(S)]
            settings(model, philox_call=0)
            out = model.predict_multiple(image, num_evaluations=S, voting=voting, t=T_STRIDED, batched=batched, views=views, x=x,
                                         maps=("mean", "counts") if voting == "majority" else ("mean",))
            assert model.philox_call == (1 if batched else S)
            if voting == "majority":
                assert torch.equal(out["counts"].long(), sum(p.long() for p in passes))
            else:
                total = torch.zeros_like(passes[0])
                for p in passes:
                    total = total + p * float(np.float32(1.0 / S))
                assert torch.equal(out["mean"], total)
    finally:
        settings(model, philox_advance=False, philox_call=0, substreams=0, step_T_sample="majority")
