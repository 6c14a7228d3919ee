"""What the tests of the guided step entries (test_evidence_sampling, test_shaped_sampling, test_view_sampling, test_tiled_sampling,
test_sampling_queue) share: the numpy restatements of the evidence step and of the shaping in front of it, their float64 counterparts,
the seeded inputs, the kernel shapes and the launch of ccdm_shaped_step on host arrays.  The restatements are built from the oracle's
public functions and the definition in include/ccdm_hip.h, not from the kernels.  A plain module: no fixture, no pytest setting."""
import numpy as np
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import hip
from tests import ladder_util
from tests.sampler_util import DEV, H, SEED, W, onehot_np

# a partial block; a block boundary inside a sample; staged; the largest K; then one shape per class count at the ends of every rung of
# the kernels' class-count ladder (ladder_util)
SHAPES = [(3, 63, 2), (2, 300, 5), (2, 64, 20), (1, 64, 255)] + ladder_util.SHAPES
# test_tempered_kernel_against_float64: the kernel's largest relative error against the float64 definition on that test's inputs, measured
# on an MI355X, and what the test allows the device's power for it (four times that: the ROCm installation states no ulp bound for exp2f
# and log2f).  The largest per rung of the class-count ladder, over SHAPES: 2.085e-6 (rung 2: K = 2), 1.600e-6 (4: K = 4), 1.717e-6 (8:
# K = 5), 1.968e-6 (16: K = 9), 1.307e-6 (20: K = 20), 1.279e-6 (24: K = 21), 2.095e-6 (32: K = 32), 1.323e-6 (64: K = 64), 2.284e-6
# (128: K = 128), 2.849e-6 (256: K = 255 at (2, 75); 1.851e-6 at (1, 64), the largest of the four shapes the constant was first taken on)
POWER_ERROR_MEASURED = 2.849e-6
POWER_ERROR_ALLOWED = 4 * POWER_ERROR_MEASURED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def coefficients(t, T=250):
    _, alphas, cum = O.make_schedule("cosine", T, {"s": 0.008})
    return O.posterior_coeffs(alphas, cum, t)


def nhwk(ev_bchw):
    n, k = ev_bchw.shape[:2]
    return ev_bchw.permute(0, 2, 3, 1).reshape(n, H * W, k).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ the evidence step
def evidence_restatement(x0, ev, xt, a, c, mode, step_row, seed, sample0):
    """What ccdm_evidence_step computes, from the oracle's functions.  x0, ev: fp32 [N,HW,K]; xt: integer [N,HW].
    x0' = x0 * ev in fp32; the O(K) posterior in the epilogue's op order; clamp at 1e-12; cascade normalisation; STEP_SAMPLE: the Exp(1)
    race on the unguided step's counters (pixel, sample0 + n, step_row, k // 4), first maximum wins; last-step modes: the argmax.
    Returns (probabilities fp32 [N,HW,K], class index int64 [N,HW])."""
    N, HW, K = x0.shape
    x0p = (torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)) * torch.from_numpy(np.ascontiguousarray(ev, dtype=np.float32)))
    theta = x0p.reshape(N, 1, HW, K).permute(0, 3, 1, 2)
    xt_oh = O.one_hot_bchw(torch.from_numpy(np.asarray(xt).astype(np.int64)).reshape(N, 1, HW), K)
    p_hat = O.normalise_probs(torch.clamp(O.theta_post_prob(xt_oh, theta, a, c), min=1e-12), "cascade")          # [N,1,HW,K]
    if mode == hip.STEP_SAMPLE:
        e = torch.from_numpy(O.philox_exponential(seed, step_row, sample0, N, HW, K)).reshape(N, 1, HW, K)
        idx = O.sample_index(p_hat, e)
    else:
        idx = p_hat.argmax(dim=-1)
    return p_hat.reshape(N, HW, K).numpy(), idx.reshape(N, HW).numpy().astype(np.int64)


def random_inputs(rng, N, HW, K):
    """x0: every entry >= 1e-3 (K <= 255: >= 1 / (3 K)), rows normalised; weights in [0,1], a fifth of them exactly 0, one class per
    pixel with a weight in [0.5,1] (so no pixel is ruled out, and sum_k x0_k w_k >= 0.5e-3); x_t random."""
    r = (rng.random((N, HW, K)) + 0.5).astype(np.float32)
    x0 = (r / r.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    assert x0.min() >= 1e-3
    ev = rng.random((N, HW, K)).astype(np.float32)
    ev[rng.random((N, HW, K)) < 0.2] = 0.0
    sure = rng.integers(0, K, (N, HW))
    np.put_along_axis(ev, sure[..., None], rng.uniform(0.5, 1.0, (N, HW, 1)).astype(np.float32), axis=-1)
    xt = rng.integers(0, K, (N, HW))
    return x0, ev, xt


def sampler_evidence(rng, N, K, onehot_share=0.0):
    """[N,K,H,W] fp32: a soft map (weights in [0.05,1]), and on a share of the pixels a one-hot on a random class"""
    ev = rng.uniform(0.05, 1.0, (N, K, H, W)).astype(np.float32)
    pick = rng.random((N, H, W)) < onehot_share
    cls = rng.integers(0, K, (N, H, W))
    ev = np.where(pick[:, None], (np.arange(K)[None, :, None, None] == cls[:, None]).astype(np.float32), ev)
    return torch.from_numpy(ev), torch.from_numpy(pick), torch.from_numpy(cls)


# ------------------------------------------------------------------------------------------------ the shaping in front of it
def shape_rows(v, inv_tau, r, dtype=np.float32):
    """The shaping of include/ccdm_hip.h on rows v [...,K] (>= 0) in `dtype` arithmetic: temper relative to the row's maximum (skipped at
    inv_tau == 1), then keep class pi(j) iff the mass of the classes before it in the order (q descending, index ascending) is below
    r * Z (skipped at r == 1).  Sums are sequential (np.cumsum), the power is numpy's."""
    q = np.array(v, dtype=dtype)
    inv_tau, r = dtype(inv_tau), dtype(r)
    if inv_tau != 1:
        m = q.max(-1, keepdims=True)
        u = q / np.where(m == 0, dtype(1), m)
        t = np.where(u == 1, dtype(1), np.where(u == 0, dtype(0), np.power(u, inv_tau, dtype=dtype)))
        q = np.where(m == 0, q, t).astype(dtype)
    if r != 1:
        theta = (r * np.cumsum(q, axis=-1, dtype=dtype)[..., -1:]).astype(dtype)
        order = np.argsort(-q, axis=-1, kind="stable")
        before = np.cumsum(np.take_along_axis(q, order, -1), axis=-1, dtype=dtype)
        before = np.concatenate([np.zeros_like(before[..., :1]), before[..., :-1]], axis=-1)          # c_j
        keep = np.zeros(q.shape, dtype=bool)
        np.put_along_axis(keep, order, before < theta, -1)
        q = np.where(keep, q, dtype(0))
    return q


def weighted(x0, ev):
    """v = x0 * w in fp32 (x0 itself without evidence)"""
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    return x0 if ev is None else (x0 * np.ascontiguousarray(ev, dtype=np.float32)).astype(np.float32)


def shaped_restatement(x0, ev, xt, inv_tau, r, a, c, mode, step_row, seed, sample0):
    """What ccdm_shaped_step computes: the definition in numpy fp32, then the evidence restatement's step (O.theta_post_prob, the clamp,
    O.normalise_probs(..., "cascade"), O.sample_index on O.philox_exponential) on the shaped row.  x0: fp32 [N,HW,K]; ev: the same or None;
    xt: integer [N,HW].  Returns (probabilities fp32 [N,HW,K], class index int64 [N,HW])."""
    q = shape_rows(weighted(x0, ev), np.float32(inv_tau), np.float32(r))
    return evidence_restatement(q, np.ones_like(q), xt, a, c, mode, step_row, seed, sample0)


def posterior64(q, xt, a, c):
    """The step's posterior of rows q [N,HW,K] in float64, brute force over x_0 = d (Bayes, as test_the_restatement_is_bayes_rule forms it),
    with the fp32 coefficients the step is handed."""
    K = q.shape[-1]
    a64, c64 = float(np.float32(a)), float(np.float32(c))
    A = a64 * onehot_np(np.asarray(xt), K) + (1 - a64) / K
    B = c64 * np.eye(K) + (1 - c64) / K
    joint = A[..., :, None] * B[None, None]
    theta = joint / joint.sum(axis=2, keepdims=True)
    want = (theta * q.astype(np.float64)[..., None, :]).sum(-1)
    return want / want.sum(-1, keepdims=True)


def threshold_margin64(q64, r):
    """Per row, the smallest relative distance |c_j - theta| / theta of a prefix mass c_j (j >= 1) to the threshold, in float64."""
    theta = float(np.float32(r)) * q64.sum(-1, keepdims=True)
    c = np.cumsum(-np.sort(-q64, axis=-1), axis=-1)
    return (np.abs(c - theta) / theta).min(-1)


def mixed_inputs(rng, N, HW, K):
    """The evidence tests' random_inputs (flat rows) at the even pixels; at the odd ones peaked rows: softmax of 4 N(0,1) logits, floored
    at 1e-6, normalised in fp32.  Flat rows alone never truncate at K = 2."""
    x0, ev, xt = random_inputs(rng, N, HW, K)
    logits = 4.0 * rng.standard_normal((N, HW, K))
    p = np.exp(logits - logits.max(-1, keepdims=True))
    p = np.maximum(p / p.sum(-1, keepdims=True), 1e-6).astype(np.float32)
    p = (p / p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    x0[:, 1::2] = p[:, 1::2]
    return x0, ev, xt


TEMPERED_TAUS, TEMPERED_RS, TEMPERED_TS = (0.7, 1.5), (1.0, 0.9), (200, 2)
TEMPERED_ROW, TEMPERED_OFF = 1, 3


def tempered_reference(x0, ev, xt, tau, r, t, row=TEMPERED_ROW, off=TEMPERED_OFF, seed=SEED):
    """The float64 side of test_tempered_kernel_against_float64 for one (tau, r, evidence, t), from the definition and the oracle alone:
    float64 shaping of the fp32 v with the fp32 inv_temperature and top_r, float64 Bayes posterior.  Returns inv_temperature, (a, c),
    `want` [N,HW,K], `big` (the entries the probabilities are compared at: > 1e-9, of pixels not within 1e-5 of a truncation threshold)
    and `skip` (the pixels the draws are not compared at: near a threshold, or a float64 race margin <= 1e-4)."""
    N, HW, K = x0.shape
    inv = float(np.float32(1.0 / tau))
    v = weighted(x0, ev)
    q64 = shape_rows(v, inv, float(np.float32(r)), np.float64)
    near = threshold_margin64(shape_rows(v, inv, 1.0, np.float64), r) <= 1e-5 if r != 1.0 else np.zeros((N, HW), dtype=bool)
    a, c = coefficients(t)
    want = posterior64(q64, xt, a, c)
    big = (want > 1e-9) & ~near[..., None]
    score = np.sort(want / O.philox_exponential(seed, row, off, N, HW, K).astype(np.float64), axis=-1)
    skip = near | ((score[..., -1] - score[..., -2]) / score[..., -1] <= 1e-4)
    return inv, (a, c), want, big, skip


def tempered_cases(ev_all):
    """Every (tau, r, evidence, t) of the tempered test, in its order"""
    return [(tau, r, ev, t) for tau in TEMPERED_TAUS for r in TEMPERED_RS for ev in (None, ev_all) for t in TEMPERED_TS]


def run_shaped_kernel(lib, x0, ev, xt, inv_tau, r, a, c, mode, *, step_row=0, seed=SEED, sample_offset=0, xin=None, probs=None, onehot=None,
                      alias=False, symbol="ccdm_shaped_step"):
    """x0: fp32 [N,HW,K]; ev: the same or None; xt: integer [N,HW]; xin [N,HW,stride] / probs / onehot [N,HW,K] numpy or None; alias:
    out_probs IS x0.  symbol = "ccdm_evidence_step": that entry on the same buffers (inv_tau, r unused).  Returns the buffers after the
    launch (numpy)."""
    N, HW, K = x0.shape
    host = dict(x0=x0, ev=ev, xt=np.asarray(xt).astype(np.uint8), xin=xin, probs=probs, onehot=onehot)
    d = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in host.items()}

    def ptr(name):
        return None if d[name] is None else d[name].data_ptr()
    shaping = (float(inv_tau), float(r)) if symbol == "ccdm_shaped_step" else ()
    hip.check(getattr(lib, symbol)(ptr("x0"), ptr("ev"), N, HW, K, *shaping, float(a), float(c), mode, step_row, seed, sample_offset, ptr("xt"),
                                   ptr("xin"), 0 if xin is None else xin.shape[2], ptr("x0") if alias else ptr("probs"), ptr("onehot"), 0),
              symbol)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}
