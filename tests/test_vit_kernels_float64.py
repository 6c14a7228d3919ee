"""The ViT encoder's own kernels against float64 on trained-like data.

The DINO feature encoder (ccdm_stochastic_segmentation_amd/dino.py) runs LayerNorm and GELU kernels of its own (ccdm_layernorm, ccdm_gelu)
and every linear layer as a 1x1 ccdm_conv2d over a 16-wide token image.  The descriptor tests check all of it at once, against the fp32
oracle, on N(0, 1/fan_in) weights and with one bar of 2e-4 max|ref|.  Here every case is computed three times on the same inputs — by
the kernel, in float64, and by the plain fp32 torch operator on the CPU — and the kernel's error against float64 is held to a stated
multiple of the fp32 operator's error against float64.  No bar is derived from the kernel's output.  Both errors go to parity_log.

  1. LayerNorm (eps 1e-6): C in {1, 63, 65, 100, 384, 768, 1536} x rows in {1, 5, 185}, nine row populations.  Error of a row:
     max_c |out - ref64| / (max|gamma| max_c |x - mean64| rstd64 + max|beta|).  Bar per population: 2 x the worst fp32 F.layer_norm row over
     all 21 geometries.  The exact-zero row must be beta bit for bit.
  2. GELU: absolute error per (sign, decade of |x|) bin, bar 2 x the worst F.gelu fp32 error of the bin; a 16384 * 256 + 1000 element
     buffer (second, ragged trip of the grid-stride loop) must repeat the sweep's bits; +inf -> +inf, NaN -> NaN.
  3. Token-image linear (the argument block of ViTExtractor._linear): per output element
         |out - ref64| <= c sum_k |x_k w_k| + 2^-29 sum_k |w_k| + ulp32(|ref64|),   c = 2^-22 + 2 r32,
     r32 = max |x32 @ w32^T - x64 @ w64^T| / sum_k |x_k w_k| of torch.matmul in fp32 on the CPU (the product alone: the bias and residual
     additions are the ulp32 term).  Where the library takes the LDS-free 1x1 kernel the same call through the general kernel
     (DIAG_GENERAL_KERNEL) must give the same bits.  A CPU emulation of the split shows that the bar fails by orders of magnitude when one
     32-channel chunk of the weights is lost or one split term is dropped.
  4. The encoder end to end on trained-like weights (large LayerNorm gains, residual-stream outlier channels of several hundred, unit
     position embedding, fc1 rows x 8), keys of layers 0, 1, 5, 11 against the float64 oracle: max|got - ref64| / max|ref64| per layer,
     bar 8 x the fp32 oracle's own deviation on the same case (4 x for 2^-22 against 2^-24 per product, 2 x for ordering).

FIGURES (MI355X for the kernels, CPU for the fp32 operators; all against float64 on this file's inputs).

  1. LayerNorm, worst row measure over the 21 geometries:
     population           F.layer_norm   k_layernorm
                          fp32           before      after the fix this file led to
     plain                1.06e-07       1.33e-07    1.33e-07
     offset_100           4.52e-06       3.83e-06    9.90e-08
     offset_1000          3.90e-05       3.30e-05    1.12e-07
     outlier              1.77e-07       1.35e-07    1.35e-07
     low_variance         2.02e-04       1.87e-04    8.97e-08
     constant_0.7         0              1.47e-04    0
     constant_zero        0              0           0
     gains_large          1.44e-07       1.44e-07    1.44e-07
     gains_zero_gamma     0              0           0
     The constant row is the finding: ATen's Welford mean of equal values is exact, the kernel's fp32 sum was not, and rstd = 1000
     turned one ulp of the mean into 1.5e-4 of the output.  k_layernorm now subtracts the residuals' own mean before the variance pass
     (csrc/ccdm_misc.hip); on a constant row every partial sum of the residuals is exact and the output is beta bit for bit.

  2. GELU, worst absolute error of a bin, kernel / F.gelu fp32: [0.1, 1) 7.8e-08 / 8.5e-08, (-1, -0.1] 3.9e-08 / 3.2e-08 (the worst
     ratio, 1.22), [1, 10) 4.5e-07 / 1.1e-06, (-10, -1] 8.3e-08 / 1.0e-06, 1e-3 decade 4.7e-10 / 5.3e-10; equal in the subnormal decades.

  3. Token linear, r32 of fp32 torch.matmul (c = 2^-22 + 2 r32):
     Cin x Cout, rows      plain     gelu_like  outlier   mixed
      192 x  384,  32      2.64e-07  2.77e-07   1.25e-06  2.59e-07
      768 x  768,  32      1.38e-07  1.58e-07   2.04e-06  1.35e-07
      384 x 1152,  32      2.85e-07  3.42e-07   1.69e-06  2.77e-07
      768 x 2304,  32      1.51e-07  1.67e-07   1.92e-06  2.41e-07
      384 x 1536,  32      2.61e-07  3.82e-07   1.92e-06  2.43e-07
     1536 x  384,  32      8.38e-08  1.13e-07   1.62e-06  7.16e-08
     1536 x  768,  32      7.58e-08  1.10e-07   1.68e-06  9.77e-08
     2048 x  384,  32      5.25e-08  7.66e-08   1.56e-06  7.24e-08
      384 x  384,  96      1.79e-07  2.27e-07   1.13e-06  1.50e-07
     (outlier: the partial sum sits at ~150 after the +-3000 channels and every later fp32 addition rounds at that magnitude.)
     On the device every case sits at 0.15-0.94 of the bar (worst: 2048x384 outlier 0.94, 1536x768 outlier 0.88, 1536x384 outlier 0.77;
     the split-K chain 0.44 / 0.49) and the 1x1 kernel repeats the general kernel's bits at every width.  (The logged err / sum|xw| of the
     kernel, up to 0.15, is the rounding of the bias and residual at the 1e-4-weight channels, where sum|xw| is ~1e-6: the bar's ulp32 term.)
     FINDING: before the fix this file led to, eight cases, the split-K chain (plain) and one loudness case failed, all with a bias and a
     residual, at the channels with 1e-4 weights: err / bar 1.08 (192x384 plain), 3.77 (768x768 mixed), 1.78 (768x2304 gelu_like), 2.39
     (384x1536 plain), 1.97 (1536x384 mixed), 6.13 (2048x384 gelu_like), 2.72 (384x384, 48 rows, plain), 1309 (384x384, 16432 rows, mixed),
     1.19 (split-K plain), 1.94 (loudness, 1x1 kernel).  The epilogues rounded fma(acc, wscale, bias) at the magnitude of the bias (~0.1:
     3.7e-9) before adding the residual; where the residual cancels the bias and sum|xw| is tiny, |ref64| and its ulp are far below that
     (16432 rows: |ref64| ~ 1e-5).  A 1x1 conv with bias and residual now adds the three terms in fp64 and rounds once, in k_conv1x1 and in
     k_conv's 1x1 epilogue alike (ccdm_conv1x1.hip, ccdm_conv.hip); the same cases then sit at 0.44-0.59 of the bar.
     The emulated split product sits at 0.05-0.12 of the bar; with chunk 7 of the weights zeroed at 8e3-2e5 x the bar, with either cross
     term dropped at 110-150 x.

  4. Encoder, fp32 oracle against the float64 oracle, max|d| / max|ref64| at layers 0 / 1 / 5 / 11:
     dino_vits8  stride 8 40x72    1.10e-06  1.52e-06  1.60e-06  1.44e-06
     dino_vits8  stride 4 40x72    1.32e-06  1.58e-06  1.29e-06  1.23e-06
     dino_vitb16 64x96             8.91e-07  8.90e-07  1.45e-06  1.30e-06
     kernels / fp32 oracle on the device: 0.65-1.05 (ViT-S/8 stride 8), 0.93-1.04 (stride 4), 1.13-1.32 (ViT-B/16, worst at layer 5).
     (float64 probe: residual stream up to 900-935, LayerNorm outputs up to 70-99, GELU outputs up to 80-94, 16% of them below 2e-3.)
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd.dino import VIT_CONFIGS, DinoViT, make_synthetic_vit_state_dict

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from tests import hip_util
    hip.load()
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    return hip_util


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------ 1. LayerNorm
LN_EPS = 1e-6
LN_CS = (1, 63, 65, 100, 384, 768, 1536)
LN_ROWS = (1, 5, 185)
LN_MULT = 2.0
LN_POPULATIONS = ("plain", "offset_100", "offset_1000", "outlier", "low_variance", "constant_0.7", "constant_zero", "gains_large",
                  "gains_zero_gamma")


def ln_population(pop, rows, C):
    """-> (x [rows, C], gamma [C], beta [C]) fp32"""
    r = _rng("ln", pop, rows, C)
    z = r.standard_normal((rows, C))
    gamma, beta = r.standard_normal(C), r.standard_normal(C)
    if pop == "plain":
        x = z
    elif pop.startswith("offset_"):                     # mean / sigma = 100, 1000 (either sign)
        x = z + float(pop[7:]) * r.choice([-1.0, 1.0], (rows, 1))
    elif pop == "outlier":                              # the massive-activation row: one channel at 3000 (channel 0 in row 0)
        x = z
        x[np.arange(rows), (np.arange(rows) * 7) % C] = 3000.0
    elif pop == "low_variance":
        x = 5.0 + 1e-3 * z
    elif pop == "constant_0.7":
        x = np.full((rows, C), 0.7)
    elif pop == "constant_zero":
        x = np.zeros((rows, C))
    elif pop == "gains_large":                          # gamma up to 10 on a few channels, beta = 0
        x = 3.0 * z + 0.7
        gamma = 1.0 + 0.1 * gamma
        for c, g in ((0, 10.0), (C // 3, -7.0), (C - 1, 4.0)):
            gamma[c] = g
        beta = np.zeros(C)
    elif pop == "gains_zero_gamma":                     # gamma = 0, beta != 0: the output is beta
        x = 3.0 * z + 0.7
        gamma = np.zeros(C)
    else:
        raise KeyError(pop)
    return _f32(x), _f32(gamma), _f32(beta)


def ln_ref64(x, gamma, beta):
    """-> (LayerNorm in float64 [rows, C], the row's error scale [rows])"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    d = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS)
    scale = gamma.abs().max() * (d.abs() * rstd).amax(-1) + beta.abs().max()
    return d * rstd * gamma + beta, scale


def ln_measure(got, ref, scale):
    """max over the rows of max_c |got - ref| / scale (a row of scale 0 must be exact)"""
    err = (got.double() - ref).abs().amax(-1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err)).max().item()


@functools.lru_cache(maxsize=None)
def ln_case(pop, rows, C):
    """inputs, float64 reference and the fp32 operator's error of one (population, geometry), computed once"""
    x, gamma, beta = ln_population(pop, rows, C)
    ref, scale = ln_ref64(x, gamma, beta)
    e32 = ln_measure(F.layer_norm(x, (C,), gamma, beta, LN_EPS), ref, scale)
    return x, gamma, beta, ref, scale, e32


@gpu
@pytest.mark.parametrize("pop", LN_POPULATIONS)
def test_layernorm_vs_float64(U, parity_log, pop):
    worst32 = worstk = 0.0
    where = None
    for C in LN_CS:
        for rows in LN_ROWS:
            x, gamma, beta, ref, scale, e32 = ln_case(pop, rows, C)
            got = U.layernorm(x, gamma, beta, LN_EPS)
            assert torch.isfinite(got).all(), (pop, rows, C)
            ek = ln_measure(got, ref, scale)
            print(f"layernorm {pop} C={C} rows={rows}: kernel {ek:.3e} fp32 {e32:.3e}")
            if pop == "constant_zero":
                assert torch.equal(got, beta.expand(rows, C)), f"exact-zero rows must give beta bit for bit (C={C}, rows={rows})"
            worst32 = max(worst32, e32)
            if ek >= worstk:
                worstk, where = ek, (C, rows)
    parity_log(f"vit_float64[layernorm/{pop}]", err_kernel=worstk, err_fp32=worst32, bar=LN_MULT * worst32, worst_C=where[0], worst_rows=where[1])
    assert worstk <= LN_MULT * worst32, f"layernorm {pop}: kernel {worstk:.3e} at C={where[0]}, rows={where[1]} against float64, bar " \
                                        f"{LN_MULT:g} x {worst32:.3e} (F.layer_norm fp32 over all geometries)"


@gpu
def test_layernorm_refusals(U):
    """C beyond 64 * LN_MAX_PER_LANE, C = 0, rows = 0 and a null pointer: a negative return, a message, no launch (the output stays)"""
    lib = hip.load()
    x = torch.ones((4, 1537), device=U.DEV)
    g, b = torch.ones(1537, device=U.DEV), torch.zeros(1537, device=U.DEV)
    out = torch.full((4, 1537), -3.0, device=U.DEV)
    p = (x.data_ptr(), g.data_ptr(), b.data_ptr())
    for what, rc in [("C=1537", lib.ccdm_layernorm(*p, LN_EPS, 4, 1537, out.data_ptr(), 0)),
                     ("C=0", lib.ccdm_layernorm(*p, LN_EPS, 4, 0, out.data_ptr(), 0)),
                     ("rows=0", lib.ccdm_layernorm(*p, LN_EPS, 0, 384, out.data_ptr(), 0)),
                     ("null x", lib.ccdm_layernorm(None, p[1], p[2], LN_EPS, 4, 384, out.data_ptr(), 0)),
                     ("null gamma", lib.ccdm_layernorm(p[0], None, p[2], LN_EPS, 4, 384, out.data_ptr(), 0)),
                     ("null beta", lib.ccdm_layernorm(p[0], p[1], None, LN_EPS, 4, 384, out.data_ptr(), 0)),
                     ("null out", lib.ccdm_layernorm(*p, LN_EPS, 4, 384, None, 0))]:
        assert rc < 0, what
        assert "layernorm" in hip.last_error(), what
    U.sync()
    assert torch.all(out == -3.0)
    out2 = torch.full((4, 1536), -3.0, device=U.DEV)
    assert lib.ccdm_layernorm(*p, LN_EPS, 4, 1536, out2.data_ptr(), 0) == 0        # the documented limit itself runs: rows of ones -> beta
    U.sync()
    assert torch.all(out2 == 0.0)


# ------------------------------------------------------------------------------------------ 2. GELU
GELU_MULT = 2.0
GELU_GRID = 16384 * 256             # elements of one trip of k_gelu's grid-stride loop


def gelu_ref64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def gelu_sweep():
    """-> (x fp32: a dense sweep of [-10, 10], 512 log-spaced magnitudes per decade from 1e-45 to 10 in both signs, +-0, subnormals, the
    smallest normal, +-1e4, +-3e38; float64 reference; F.gelu fp32; bin index per element; bin names)"""
    r = _rng("gelu")
    mags = 10.0 ** r.uniform(-45.0, 1.0, 47 * 512)
    special = np.array([0.0, 1e-45, 3e-42, 1e-40, 5e-39, 1.1754944e-38, 1e4, 3e38])
    x = np.concatenate([np.linspace(-10.0, 10.0, 400001), mags, -mags, special, -special]).astype(np.float32)
    x = torch.from_numpy(x)
    with np.errstate(divide="ignore"):
        dec = np.floor(np.log10(np.abs(x.double().numpy())))
    dec = np.where(x.numpy() == 0, -99, dec).astype(np.int64)
    key = dec * 2 + (np.signbit(x.numpy())).astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    names = [("-" if k % 2 else "+") + ("0" if k // 2 == -99 else f"1e{k // 2}") for k in uniq]
    return x, gelu_ref64(x), F.gelu(x), torch.from_numpy(inv), names


def _per_bin_max(err, inv, nbins):
    out = torch.zeros(nbins, dtype=torch.float64)
    return out.scatter_reduce(0, inv, err, "amax", include_self=True)


@gpu
def test_gelu_vs_float64(U, parity_log):
    x, ref, f32, inv, names = gelu_sweep()
    got = U.gelu(x)
    assert torch.isfinite(got).all()
    ek = _per_bin_max((got.double() - ref).abs(), inv, len(names))
    e32 = _per_bin_max((f32.double() - ref).abs(), inv, len(names))
    bad = []
    for i, nm in enumerate(names):
        if ek[i] > 0 or e32[i] > 0:
            print(f"gelu bin {nm}: kernel {ek[i].item():.3e} fp32 {e32[i].item():.3e}")
        if nm[1:] in ("1e-5", "1e-3", "1e-1", "1e0", "1e1", "1e4", "1e38", "1e-39", "0"):
            parity_log(f"vit_float64[gelu/{nm}]", err_kernel=ek[i].item(), err_fp32=e32[i].item(), bar=GELU_MULT * e32[i].item())
        if ek[i] > GELU_MULT * e32[i]:
            bad.append(f"{nm}: kernel {ek[i].item():.3e} > {GELU_MULT:g} x fp32 {e32[i].item():.3e}")
    ratio = torch.where(e32 > 0, ek / e32.clamp_min(1e-300), torch.zeros_like(ek))
    w = int(torch.argmax(ratio))
    parity_log("vit_float64[gelu/worst_bin]", bin=names[w], err_kernel=ek[w].item(), err_fp32=e32[w].item(), ratio=ratio[w].item())
    assert not bad, "gelu against float64, per (sign, decade) bin: " + "; ".join(bad)


@gpu
def test_gelu_sizes_and_second_grid_trip(U):
    """n = 1, 255, 257 and one buffer of 16384 * 256 + 1000 elements (a second, ragged trip through the grid-stride loop): the bits of the
    sweep, element for element; nothing written behind n"""
    x, _, _, _, _ = gelu_sweep()
    got = U.gelu(x)
    for n in (1, 255, 257):
        assert torch.equal(U.gelu(x[200000:200000 + n].clone()), got[200000:200000 + n]), n
    n = GELU_GRID + 1000
    idx = (torch.arange(n) * 7 + 3) % x.numel()
    assert torch.equal(U.gelu(x[idx]), got[idx])


@gpu
def test_gelu_infinity_and_nan(U):
    got = U.gelu(torch.tensor([math.inf, math.nan, 1.0]))
    assert got[0].item() == math.inf and math.isnan(got[1].item()) and abs(got[2].item() - 0.8413447) < 1e-6


# ------------------------------------------------------------------------------------------ 3. token-image linear
LIN_MULT = 2.0
LIN_CASES = [(192, 384, 1, 32), (768, 768, 1, 32), (384, 1152, 1, 32), (768, 2304, 1, 32), (384, 1536, 1, 32), (1536, 384, 1, 32),
             (1536, 768, 1, 32), (2048, 384, 1, 32),
             (384, 384, 2, 48),             # 48 rows: no block size of the 1x1 kernel divides them
             (384, 384, 1, 16432)]          # beyond the 1x1 kernel's 16384 pixels: the stride-4 full-resolution regime
LIN_REGIMES = ("plain", "gelu_like", "outlier", "mixed")
LIN_VARIANTS = [(True, True), (True, False), (False, True), (False, False)]          # (bias, residual)
F16X3_WINDOW = 4094.0


def takes_1x1_kernel(cin, cout, rows):
    """conv1x1_eligible (ccdm_conv1x1.hip) for a plain token linear without statistics"""
    return cin % 16 == 0 and cout % 32 == 0 and cin <= 1024 and rows % 32 == 0 and rows <= 16384


def lin_inputs(cin, cout, N, rows, regime, bias, resid, key=""):
    r = _rng("lin", cin, cout, N, rows, regime, key)
    z = r.standard_normal((N, rows, cin))
    if regime == "plain":
        x = z
    elif regime == "gelu_like":                         # most inputs below the 2e-3 full-precision floor or small
        x = gelu_ref64(torch.from_numpy(z)).numpy()
    elif regime == "outlier":                           # two input channels at +-3000
        x = z
        x[..., 5] = 3000.0 * (1 + 0.05 * np.clip(z[..., 5], -3, 3))
        x[..., cin - 3] = -3000.0 * (1 + 0.05 * np.clip(z[..., cin - 3], -3, 3))
    elif regime == "mixed":                             # rows alternating between 1e-3 and 1e3 (draws clipped at 3.5 sigma: inside the window)
        x = np.clip(z, -3.5, 3.5) * np.where(np.arange(rows) % 2, 1e3, 1e-3)[None, :, None]
    else:
        raise KeyError(regime)
    w = r.standard_normal((cout, cin)) / math.sqrt(cin)
    w[:8] *= 1e-4                                       # a few output channels with tiny weights (as test_f16x3_dynamic_range)
    b = _f32(0.1 * r.standard_normal(cout)) if bias else None
    rs = _f32(r.standard_normal((N, rows, cout))) if resid else None
    x = _f32(x)
    assert x.abs().max().item() < F16X3_WINDOW
    return x, _f32(w), b, rs


def lin_reference(x, w, b, rs):
    """-> (ref64, S = sum_k |x_k w_k|, SW = sum_k |w_k| [Cout], r32 = fp32 torch.matmul's worst error over S)"""
    x64, w64 = x.double(), w.double()
    mm = x64 @ w64.T
    S = x64.abs() @ w64.abs().T
    ref = mm + (b.double() if b is not None else 0.0) + (rs.double() if rs is not None else 0.0)
    r32 = (((x @ w.T).double() - mm).abs() / S.clamp_min(1e-300)).max().item()
    return ref, S, w64.abs().sum(1), r32


def ulp32(a):
    return torch.from_numpy(np.spacing(a.abs().float().numpy()).astype(np.float64))


def lin_bar(ref, S, SW, r32, extra=0.0):
    return (2.0 ** -22 + LIN_MULT * r32) * S + 2.0 ** -29 * SW + ulp32(ref) + extra


def lin_check(what, got, ref, S, SW, r32, parity_log=None, extra=0.0, rows=None, **logged):
    err = (got.double() - ref).abs()
    bar = lin_bar(ref, S, SW, r32, extra)
    if rows is not None:
        err, bar, S = err[:, rows], bar[:, rows], S[:, rows]
    rk = (err / S.clamp_min(1e-300)).max().item()
    over = (err / bar).max().item()
    print(f"{what}: err / sum|xw| kernel {rk:.3e} fp32 matmul {r32:.3e}; worst err / bar {over:.3f}")
    if parity_log is not None:
        parity_log(f"vit_float64[linear/{what}]", ratio_kernel=rk, ratio_fp32=r32, c=2.0 ** -22 + LIN_MULT * r32, worst_err_over_bar=over, **logged)
    return over


@gpu
@pytest.mark.parametrize("regime", LIN_REGIMES)
@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_token_linear_vs_float64(U, parity_log, case, regime):
    cin, cout, N, rows = case
    bias, resid = LIN_VARIANTS[(LIN_CASES.index(case) + LIN_REGIMES.index(regime)) % 4]
    x, w, b, rs = lin_inputs(cin, cout, N, rows, regime, bias, resid)
    ref, S, SW, r32 = lin_reference(x, w, b, rs)
    rd = rs.to(U.DEV) if rs is not None else None
    packed = torch.from_numpy(hip.pack_conv_weight(w.numpy().reshape(cout, cin, 1, 1), 1, hip.PREC_F16X3)).to(U.DEV)
    out = U.token_linear(x, w.numpy(), None if b is None else b.numpy(), rd, packed=packed)
    one = takes_1x1_kernel(cin, cout, rows)
    if one:     # same products in the same order (ccdm_conv1x1.hip): the general kernel's bits
        gen = U.token_linear(x, w.numpy(), None if b is None else b.numpy(), rd, diag=hip.DIAG_GENERAL_KERNEL, packed=packed)
        assert torch.equal(out, gen), f"1x1 kernel and general kernel differ: max {(out - gen).abs().max().item():.3e}"
    got = out.cpu()
    assert torch.isfinite(got).all()
    what = f"{cin}x{cout}_N{N}_rows{rows}/{regime}"
    over = lin_check(what, got, ref, S, SW, r32, parity_log, kernel="k_conv1x1" if one else "k_conv", bias=bias, resid=resid)
    assert over <= 1.0, f"{what}: worst |out - ref64| / bar = {over:.3f}"


@gpu
@pytest.mark.parametrize("regime", ["gelu_like", "plain"])
def test_split_k_chain_vs_float64(U, parity_log, regime):
    """ViT-B's fc2 as the encoder runs it: 3072 input columns in two parts of 1536; part 0 carries the bias and the residual, part 1 a NULL
    bias and part 0's output as its residual.  Reference: the single 3072-wide float64 product.  (The stored part 0 is one more fp32
    rounding: its ulp is added to the bar.)"""
    cin, cout, N, rows = 3072, 768, 1, 32
    x, w, b, rs = lin_inputs(cin, cout, N, rows, regime, True, True, "splitk")
    ref, S, SW, r32 = lin_reference(x, w, b, rs)
    h = cin // 2
    p0 = U.token_linear(x[..., :h], w[:, :h].numpy(), b.numpy(), rs.to(U.DEV))
    p1 = U.token_linear(x[..., h:], w[:, h:].numpy(), None, p0)
    ref0 = x[..., :h].double() @ w[:, :h].double().T + b.double() + rs.double()
    over = lin_check(f"splitk_3072x768/{regime}", p1.cpu(), ref, S, SW, r32, parity_log, extra=ulp32(ref0), kernel="k_conv x 2")
    assert over <= 1.0


@gpu
@pytest.mark.parametrize("cin,cout", [(384, 384), (1536, 384)], ids=["k_conv1x1", "k_conv"])
def test_token_linear_out_of_window_input_is_loud(U, cin, cout):
    """one input value of 1e4 (beyond the 4094 window): every output of the token rows that read it is non-finite, never a finite clipped
    number; the other rows stay within the bar"""
    N, rows = 1, 32
    x, w, b, rs = lin_inputs(cin, cout, N, rows, "plain", True, True, "loud")
    hot = [3, 17, 31]
    for j, t in enumerate(hot):
        x[0, t, (5 + 100 * j) % cin] = 1e4 if j % 2 == 0 else -1e4
    out = U.token_linear(x, w.numpy(), b.numpy(), rs.to(U.DEV)).cpu()
    assert not torch.isfinite(out[0, hot]).any(), "an input beyond the window left finite outputs"
    cold = [t for t in range(rows) if t not in hot]
    assert torch.isfinite(out[0, cold]).all()
    ref, S, SW, r32 = lin_reference(x, w, b, rs)
    assert lin_check(f"loud_{cin}x{cout}", out, ref, S, SW, r32, rows=cold) <= 1.0


def f16x3_emulation(x, w, drop_term=None, zero_chunk=None):
    """NumPy emulation of the split product (ccdm_conv.hip): activations x 2^4 and weights x 2^e (max|w| of the row in [2^9, 2^10)) split
    into fp16 hi + lo; lo*hi + hi*lo + hi*hi accumulated (here in float64).  drop_term: one of 'lo*hi', 'hi*lo' left out; zero_chunk:
    index of a 32-channel chunk whose weights are lost."""
    x16 = x.astype(np.float32) * np.float32(16)
    xh = x16.astype(np.float16).astype(np.float32)
    xl = (x16 - xh).astype(np.float16).astype(np.float32)
    e = 10 - np.frexp(np.abs(w).max(1))[1]
    ws = (w * np.exp2(e)[:, None]).astype(np.float32)
    wh = ws.astype(np.float16).astype(np.float32)
    wl = (ws - wh).astype(np.float16).astype(np.float32)
    if zero_chunk is not None:
        wh, wl = wh.copy(), wl.copy()
        wh[:, 32 * zero_chunk:32 * zero_chunk + 32] = 0
        wl[:, 32 * zero_chunk:32 * zero_chunk + 32] = 0
    xh, xl, wh, wl = (a.astype(np.float64) for a in (xh, xl, wh, wl))
    acc = xh @ wh.T
    if drop_term != "lo*hi":
        acc += xl @ wh.T
    if drop_term != "hi*lo":
        acc += xh @ wl.T
    return (acc / 16.0 / np.exp2(e)[None, :]).astype(np.float32)


@pytest.mark.parametrize("regime", LIN_REGIMES)
def test_linear_bar_catches_a_lost_chunk_and_a_dropped_split_term(regime):
    """no GPU: the bar of section 3 passes the emulated split product and fails, by orders of magnitude, one with a 32-channel chunk of the
    weights zeroed or with either cross term of the split left out"""
    cin, cout, N, rows = 384, 384, 1, 32
    x, w, b, rs = lin_inputs(cin, cout, N, rows, regime, False, False)
    ref, S, SW, r32 = lin_reference(x, w, b, rs)
    xn, wn = x[0].numpy(), w.numpy()
    good = lin_check(f"emulation/{regime}", torch.from_numpy(f16x3_emulation(xn, wn))[None], ref, S, SW, r32)
    assert good <= 1.0, good
    lost = lin_check(f"emulation/{regime}/lost chunk", torch.from_numpy(f16x3_emulation(xn, wn, zero_chunk=7))[None], ref, S, SW, r32)
    assert lost > 1e3, lost
    for term in ("lo*hi", "hi*lo"):
        dropped = lin_check(f"emulation/{regime}/no {term}", torch.from_numpy(f16x3_emulation(xn, wn, drop_term=term))[None], ref, S, SW, r32)
        assert dropped > 30.0, (term, dropped)


# ------------------------------------------------------------------------------------------ 4. the encoder on trained-like weights
E2E_MULT = 8.0
E2E_CASES = [("dino_vits8", 8, 40, 72), ("dino_vits8", 4, 40, 72), ("dino_vitb16", 16, 64, 96)]
E2E_LAYERS = (0, 1, 5, 11)
E2E_BATCH = 2
OUTLIER_CHANNELS = (7, 200)
GAIN_CHANNELS = (3, 7, 50, 131, 260, 383)
GAINS = (4.0, 5.0, 6.0, 7.0, 8.0, 4.5)


def make_trained_like_vit_state_dict(model_type, seed):
    """make_synthetic_vit_state_dict with what a trained ViT has and N(0, 1/fan_in) weights do not: norm1 / norm2 gains of 4-8 on a handful
    of channels; attn.proj.bias and mlp.fc2.bias of +-150 on two fixed channels in blocks 1-3, so that the residual stream carries
    outliers of several hundred from then on; a position embedding of sigma 1; a few fc1 rows scaled x 8."""
    sd = {k: v.copy() for k, v in make_synthetic_vit_state_dict(model_type, seed).items()}
    r = np.random.default_rng(seed + 1000)
    depth = VIT_CONFIGS[model_type]["depth"]
    for i in range(depth):
        p = f"blocks.{i}."
        for n, flip in (("norm1.weight", 1.0), ("norm2.weight", -1.0)):
            sd[p + n][list(GAIN_CHANNELS)] = np.asarray(GAINS, np.float32) * np.float32(flip if i % 2 else 1.0)
        rows = r.choice(sd[p + "mlp.fc1.weight"].shape[0], 12, replace=False)
        sd[p + "mlp.fc1.weight"][rows] *= 8.0
        if 1 <= i <= 3:
            sd[p + "attn.proj.bias"][list(OUTLIER_CHANNELS)] = [150.0, -150.0]
            sd[p + "mlp.fc2.bias"][list(OUTLIER_CHANNELS)] = [150.0, -150.0]
    sd["pos_embed"] = r.standard_normal(sd["pos_embed"].shape).astype(np.float32)
    return sd


def probe_f64(sd, x, heads, patch, stride, depth):
    """The oracle's blocks restated with their intermediate operands in view (every block's output is checked against
    dino_oracle.vit_block): the largest value the kernels stage per kind, and the largest residual-stream value."""
    from oracle import dino_oracle as D
    from tests.test_dino_variants import _pos_embed
    B, _, H, W = x.shape
    h0, w0 = 1 + (H - patch) // stride, 1 + (W - patch) // stride
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride).flatten(2).transpose(1, 2)
    t = torch.cat([sd["cls_token"].expand(B, -1, -1), t], 1) + _pos_embed(sd["pos_embed"], h0, w0, H, W)
    mx = dict(ln=0.0, qkv=0.0, attn_out=0.0, gelu=0.0, stream=0.0, patches=x.abs().max().item())
    frac_small = []
    for i in range(depth):
        p = f"blocks.{i}."
        C = t.shape[-1]
        y = F.layer_norm(t, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        q, k, v = qkv.reshape(B, -1, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
        a = (((q @ k.transpose(-2, -1)) * (C // heads) ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, -1, C)
        t2 = t + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y2 = F.layer_norm(t2, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        g = F.gelu(F.linear(y2, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
        out = t2 + F.linear(g, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        want = D.vit_block(sd, i, t, heads)
        assert (out - want).abs().max().item() <= 1e-11 * want.abs().max().item(), i
        for name, val in (("ln", max(y.abs().max(), y2.abs().max())), ("qkv", qkv.abs().max()), ("attn_out", a.abs().max()), ("gelu", g.abs().max()),
                          ("stream", out.abs().max())):
            mx[name] = max(mx[name], float(val))
        frac_small.append((g.abs() < 2e-3).double().mean().item())
        t = want
    mx["gelu_frac_below_2e-3"] = float(np.mean(frac_small))
    return mx


@functools.lru_cache(maxsize=None)
def e2e_case(case):
    """weights, image, the float64 and fp32 oracles' keys per layer, and the float64 probe of one case, computed once"""
    from tests.test_dino_variants import ref_keys
    model, stride, H, W = case
    cfg = VIT_CONFIGS[model]
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    sd = make_trained_like_vit_state_dict(model, 11)
    x = _f32(_rng("e2e", *case).standard_normal((E2E_BATCH, 3, H, W)))
    sd32 = {k: torch.from_numpy(v) for k, v in sd.items()}
    sd64 = {k: v.double() for k, v in sd32.items()}
    ref = {L: ref_keys(sd64, x.double(), cfg["heads"], cfg["patch"], stride, layer=L) for L in E2E_LAYERS}
    f32 = {L: ref_keys(sd32, x, cfg["heads"], cfg["patch"], stride, layer=L) for L in E2E_LAYERS}
    assert all(v.dtype == torch.float64 for v in ref.values()) and all(v.dtype == torch.float32 for v in f32.values())
    return sd, x, ref, f32, probe_f64(sd64, x.double(), cfg["heads"], cfg["patch"], stride, cfg["depth"])


def e2e_dev(a, ref):
    return (a.double() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: f"{c[0]}_s{c[1]}_{c[2]}x{c[3]}")
def test_trained_like_weights_stay_inside_the_f16x3_window(case):
    """no GPU: on the float64 oracle every operand the kernels stage (patches, LayerNorm outputs, q / k / v, attention outputs, GELU outputs)
    stays below 4094 at the test geometries — the end-to-end test measures accuracy, not the overflow contract — while the weights do what
    they are for: a residual stream of several hundred and GELU outputs mostly below the 2e-3 floor or far above it"""
    _, _, ref, f32, mx = e2e_case(case)
    print(case, mx, {L: e2e_dev(f32[L], ref[L]) for L in E2E_LAYERS})
    for kind in ("patches", "ln", "qkv", "attn_out", "gelu"):
        assert mx[kind] < F16X3_WINDOW / 2, (kind, mx[kind])
    assert mx["stream"] > 300.0, mx["stream"]
    assert mx["ln"] > 30.0, mx["ln"]              # large gains on outlier channels: LayerNorm outputs far from O(1)
    assert all(torch.isfinite(v).all() for v in ref.values())


@gpu
@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: f"{c[0]}_s{c[1]}_{c[2]}x{c[3]}")
def test_encoder_layers_vs_float64_oracle(U, parity_log, case):
    model, stride, H, W = case
    sd, x, ref, f32, mx = e2e_case(case)
    enc = DinoViT(model, False, "concat_pixels_concat_features", stride=stride, state_dict=sd)
    xd = x.to(U.DEV)
    bad = []
    for L in E2E_LAYERS:
        got = enc.extractor.extract_descriptors(xd, L).cpu()
        assert got.shape == ref[L].shape and torch.isfinite(got).all(), L
        ek, e32 = e2e_dev(got, ref[L]), e2e_dev(f32[L], ref[L])
        print(f"{model} stride {stride} {H}x{W} layer {L}: kernel {ek:.3e} fp32 oracle {e32:.3e} (x {ek / e32:.2f}); max|ref| {ref[L].abs().max().item():.1f}")
        parity_log(f"vit_float64[encoder/{model}_s{stride}_{H}x{W}/layer{L}]", err_kernel=ek, err_fp32_oracle=e32, bar=E2E_MULT * e32,
                   stream_max=mx["stream"], ln_max=mx["ln"], gelu_max=mx["gelu"])
        if ek > E2E_MULT * e32:
            bad.append(f"layer {L}: {ek:.3e} > {E2E_MULT:g} x {e32:.3e}")
    assert not bad, f"{model} stride {stride} {H}x{W} against the float64 oracle: " + "; ".join(bad)
