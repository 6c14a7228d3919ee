"""GroupNorm statistics against float64 at offset and low-variance activations.

Every GroupNorm of the U-Net reads (sum x, sum x^2) partials [N][slices][C][2] that the previous kernel's epilogue left, and forms
var = sum x^2 / n - mean^2 (gn_mean_rstd64, csrc/ccdm_gn.h).  That difference loses digits in proportion to mean^2 / var of the
group: a conv bias or a residual that moves a group's mean to tens or hundreds of standard deviations turns any fp32 rounding of the
running sums into an error of rstd.  The producer sweep drives every kernel that writes partials with its output offset at
mean/std in {0, 10, 100, 1000} and compares the (mean, rstd) the partials give with float64 statistics of the tensor the kernel stored;
the consumer sweep hands every kernel that applies GroupNorm while staging exact statistics of awkward groups (constant, variance <= eps,
large mean with a small spread, large gamma, FiLM) and compares its output with a float64 evaluation of the same operator.

Bars.  Producers: |d mean| / sigma <= 2e-6 and |d rstd| / rstd <= 2e-6 per (sample, group), sigma = 1 / rstd = sqrt(var + eps) — the
normalised value at |x^| <= 4 then moves by at most 1e-5, a tenth of the 1e-4 output contract.  Consumers: the bar of the kernel's own
parity test in tests/test_hip_parity.py.  Every reference here is float64 on the CPU."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from oracle import ccdm_oracle as O

pytestmark = pytest.mark.gpu

EPS = 1e-5
BAR = 2e-6
RATIOS = (0.0, 10.0, 100.0, 1000.0)            # output mean / std of every group
PRECS = [hip.PREC_F32, hip.PREC_F16X3]
PREC_IDS = ["f32", "f16x3"]


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from tests import hip_util
    hip.load()
    return hip_util


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))


# ------------------------------------------------------------------------------------------ statistics helpers
def groups_of(Cc):
    """GroupNorm(32) groups; a channel count that is no multiple of 32 (the scalar-epilogue heads) is checked per channel."""
    return 32 if Cc % 32 == 0 else Cc


def mean_rstd_from_partials(st, count_per_channel):
    """st [N, S, C, 2] fp64 partials -> per-(sample, group) mean, rstd, exactly as gn_group_sums + gn_mean_rstd form them: slices and the
    group's channels summed in fp64, var = sum x^2 / n - mean^2 clamped at 0, rstd = 1 / sqrt(var + eps)."""
    st = st.detach().cpu().double()
    N, _, Cc, _ = st.shape
    G = groups_of(Cc)
    s = st.sum(1).reshape(N, G, Cc // G, 2).sum(2)
    n = count_per_channel * (Cc // G)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + EPS)


def mean_rstd_f64(y_nhwc):
    """float64 (two-pass) statistics of the stored tensor [N, H, W, C]."""
    y = y_nhwc.detach().cpu().double()
    N, H, W, Cc = y.shape
    G = groups_of(Cc)
    g = y.permute(0, 3, 1, 2).reshape(N, G, -1)
    mean = g.mean(-1)
    var = ((g - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + EPS)


def stats_errors(y_nhwc, st):
    """(worst |d mean| / sigma, worst |d rstd| / rstd) of the partials st against the stored output y."""
    N, H, W, _ = y_nhwc.shape
    m_k, r_k = mean_rstd_from_partials(st, H * W)
    m_r, r_r = mean_rstd_f64(y_nhwc)
    return ((m_k - m_r).abs() * r_r).max().item(), ((r_k - r_r).abs() / r_r).max().item()


def sweep(produce, what):
    """produce(ratio) -> (stored output NHWC, partials): one run per offset; every offset must meet the bar.  The message names every
    offset's worst error, so a failing run shows how far each offset is off."""
    rows, bad = [], False
    for r in RATIOS:
        y, st = produce(r)
        dm, dr = stats_errors(y, st)
        m, rs = mean_rstd_f64(y)
        achieved = (m.abs() * rs).median().item()          # the offset the groups really have (mean / sigma)
        rows.append(f"mean/std {r:g} (measured {achieved:.3g}): dmean/sigma {dm:.2e}  drstd/rstd {dr:.2e}")
        bad |= not (dm <= BAR and dr <= BAR)
    report = f"{what}:\n  " + "\n  ".join(rows)
    print(report)
    assert not bad, report


def offset_bias(rng, cout, r):
    """biases that put every output channel at mean r (in units of the output's spread, which the weights make ~1): a common offset
    with a small per-channel spread, so the groups keep ~unit standard deviation"""
    return (r + 0.05 * rng.standard_normal(cout)).astype(np.float32)


def unit_weight(rng, cout, cin, k):
    return rnd(rng, cout, cin, k, k) / np.sqrt(cin * k * k)


# ------------------------------------------------------------------------------------------ 1. producers
# (label, c0, c1, cout, H, W, k, stride, up, fine, resid, diag, N) at the engine's shapes (LIDC C2: 32 / 32 / 64 / 96 / 128 channels at
# 128^2 / 64^2 / 32^2 / 16^2 / 8^2); diag = run the general kernel k_conv where the library would pick a specialised one
K_CONV_CASES = [
    ("c2_128_fast", 32, 0, 32, 128, 128, 3, 1, 0, 0, 0, 0, 2),
    ("c2_128_resid", 32, 0, 32, 128, 128, 3, 1, 0, 0, 1, 0, 2),
    ("c2_64", 32, 0, 32, 64, 64, 3, 1, 0, 0, 0, 0, 2),
    ("c2_32", 64, 0, 64, 32, 32, 3, 1, 0, 0, 1, 0, 2),
    ("c2_16_general", 96, 0, 96, 16, 16, 3, 1, 0, 0, 0, 1, 2),
    ("c2_8_general", 128, 0, 128, 8, 8, 3, 1, 0, 0, 1, 1, 2),
    ("scalar_epilogue_128", 32, 0, 6, 128, 128, 3, 1, 0, 0, 0, 0, 2),     # Cout % 4 != 0: the scalar epilogue
    ("scalar_epilogue_resid_64", 32, 0, 2, 64, 64, 3, 1, 0, 0, 1, 0, 2),
    ("stride2_128_to_64", 32, 0, 32, 128, 128, 3, 2, 0, 0, 0, 0, 2),
    ("upsample_on_load_64_to_128", 32, 0, 32, 64, 64, 3, 1, 1, 0, 0, 0, 2),
    ("fine1_128", 32, 0, 32, 128, 128, 3, 1, 0, 1, 1, 0, 2),
    ("fine2_128", 32, 0, 32, 128, 128, 3, 1, 0, 2, 0, 0, 2),
    ("fine2_64", 32, 0, 32, 64, 64, 3, 1, 0, 2, 0, 0, 2),
    ("concat_128", 32, 32, 32, 128, 128, 3, 1, 0, 0, 0, 0, 2),
    ("concat_16_general", 128, 96, 96, 16, 16, 3, 1, 0, 0, 0, 1, 2),
    ("one_by_one_32_general", 64, 0, 64, 32, 32, 1, 1, 0, 0, 1, 1, 2),
]


def _conv_producer(U, rng, prec, c0, c1, cout, H, W, k, stride, up, fine, resid, diag, N, skip=None, gn=False):
    xa = rnd(rng, N, c0, H, W)
    xb = rnd(rng, N, c1, H, W) if c1 else None
    w = unit_weight(rng, cout, c0 + c1, k)
    srcs = [U.nhwc(xa)] + ([U.nhwc(xb)] if c1 else [])
    Hc, Wc = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hc - 1) // stride + 1, (Wc - 1) // stride + 1
    res0 = rnd(rng, N, cout, Ho, Wo) if resid else None
    # gn: GroupNorm + SiLU on load, as the engine's ResBlock convs (exact statistics of the input)
    gnkw = dict(stats=[U.gn_stats(s, 1) for s in srcs], gamma=np.ones(c0 + c1, np.float32), beta=np.zeros(c0 + c1, np.float32),
                act=hip.ACT_SILU) if gn else {}

    def produce(r):
        # with a residual the offset comes half from the bias, half from the residual stream
        b = offset_bias(rng, cout, r / 2 if resid else r)
        rs = U.nhwc(res0 + r / 2) if resid else None
        return U.conv2d(srcs, w.numpy(), b, k, stride=stride, up=up, fine=fine, resid=rs, prec=prec,
                        diag=hip.DIAG_GENERAL_KERNEL if diag else 0, skip=skip, **gnkw)
    return produce


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("case", K_CONV_CASES, ids=lambda c: c[0])
def test_k_conv_output_statistics(U, case, prec):
    label, c0, c1, cout, H, W, k, stride, up, fine, resid, diag, N = case
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    if c1 and prec == hip.PREC_F32 and c0 % 32:
        pytest.skip("exact-fp32 chunks are 32 channels wide")
    sweep(_conv_producer(U, rng, prec, c0, c1, cout, H, W, k, stride, up, fine, resid, diag, N), f"k_conv {label} prec={prec}")


# the sub-pixel upsample form (up == 2, F16X3): the general kernel k_conv (per-phase slots where a block holds one phase) and k_upconv
UP2_CASES = [(32, 32, 64, 64), (64, 64, 32, 32), (96, 96, 16, 16), (128, 128, 8, 8)]


@pytest.mark.parametrize("general", [True, False], ids=["k_conv_up2", "k_upconv"])
@pytest.mark.parametrize("cin,cout,H,W", UP2_CASES)
def test_subpixel_upsample_output_statistics(U, cin, cout, H, W, general):
    rng = np.random.default_rng(cin * 7 + H)
    N = 2
    x = U.nhwc(rnd(rng, N, cin, H, W))
    w = unit_weight(rng, cout, cin, 3)

    def produce(r):
        return U.conv2d([x], w.numpy(), offset_bias(rng, cout, r), 3, up=2, prec=hip.PREC_F16X3,
                        diag=hip.DIAG_GENERAL_KERNEL if general else 0)
    sweep(produce, f"{'k_conv up=2' if general else 'k_upconv'} {cin}->{cout} {H}x{W}")


@pytest.mark.parametrize("fused_skip", [False, True], ids=["plain", "fused_skip"])
@pytest.mark.parametrize("c0,cout,H,W", [(128, 128, 8, 8), (96, 96, 16, 16), (256, 128, 8, 8)])
def test_k_conv_ks_output_statistics(U, c0, cout, H, W, fused_skip):
    """ccdm_conv_ks.hip (few-pixel images: one partial per 8x8 tile) as the engine runs it — GroupNorm + SiLU on load — with and
    without the fused 1x1 skip segment"""
    rng = np.random.default_rng(c0 + cout + H)
    N = 2
    x = U.nhwc(rnd(rng, N, c0, H, W))
    skip = ([x], unit_weight(rng, cout, c0, 1).numpy() * 0.5, np.zeros(cout, np.float32)) if fused_skip else None
    produce = _conv_producer(U, rng, hip.PREC_F16X3, c0, 0, cout, H, W, 3, 1, 0, 0, 0, 0, N, skip=skip, gn=True)
    # the library must pick the few-pixel kernel here (one statistics slice per 8x8 tile)
    _, st = produce(0.0)
    assert st.shape[1] == (H // 8) * (W // 8)
    sweep(produce, f"k_conv_ks {c0}->{cout} {H}x{W} skip={fused_skip}")


@pytest.mark.parametrize("resid", [0, 1], ids=["plain", "residual"])
@pytest.mark.parametrize("cin,cout,H,W", [(128, 128, 8, 8), (96, 96, 16, 16), (64, 64, 32, 32)])
def test_k_conv1x1_output_statistics(U, cin, cout, H, W, resid):
    """ccdm_conv1x1.hip: AttentionBlock.proj_out (+ residual) at the low-resolution stages"""
    rng = np.random.default_rng(cin + 3 * H + resid)
    sweep(_conv_producer(U, rng, hip.PREC_F16X3, cin, 0, cout, H, W, 1, 1, 0, 0, resid, 0, 2), f"k_conv1x1 {cin}->{cout} {H}x{W} resid={resid}")


@pytest.mark.parametrize("H,W", [(128, 128), (64, 64)])
def test_k_stem_output_statistics(U, H, W):
    """ccdm_stem.hip: one-hot x_t (K = 2) + image; the input is one-hot, so the output offset is the bias alone"""
    rng = np.random.default_rng(H)
    N, K, cout = 2, 2, 32
    xt = torch.from_numpy(rng.integers(0, K, (N, H, W))).to(torch.uint8).to(U.DEV)
    xin = torch.zeros((N, H, W, 4))
    xin[..., K] = torch.from_numpy(rng.uniform(-1, 1, (N, H, W)).astype(np.float32))
    xin = xin.to(U.DEV)
    w = rnd(rng, cout, K + 1, 3, 3) / np.sqrt(3 * 9) * 2

    def produce(r):
        return U.stem_conv(xt, xin, K, w.numpy(), offset_bias(rng, cout, r))
    sweep(produce, f"k_stem {H}x{W}")


@pytest.mark.parametrize("C_,H,W,slices", [(32, 128, 128, 12), (64, 32, 32, 4), (128, 8, 8, 1), (32, 256, 512, 16)])
def test_gn_stats_offset(U, C_, H, W, slices):
    rng = np.random.default_rng(C_ + W)
    x0 = rnd(rng, 2, C_, H, W)

    def produce(r):
        xs = U.nhwc(x0 + r)
        return xs, U.gn_stats(xs, slices)
    sweep(produce, f"ccdm_gn_stats {C_}x{H}x{W} slices={slices}")


def test_cityscapes_sized_conv_and_stats_fold(U):
    """A Cityscapes-sized layer (256x512, 32 channels) leaves more than CCDM_STATS_MAX_SLICES partials; ccdm_stats_fold folds them to 16
    before any GroupNorm reads them.  Both the raw partials and the folded ones must give the float64 statistics."""
    rng = np.random.default_rng(5)
    lib = hip.load()
    produce = _conv_producer(U, rng, hip.PREC_F16X3, 32, 0, 32, 256, 512, 3, 1, 0, 0, 0, 0, 1)

    def produce_folded(r):
        y, st = produce(r)
        N, S, Cc, _ = st.shape
        assert S > hip.STATS_MAX_SLICES
        out = torch.full((N, hip.STATS_FOLD_SLICES, Cc, 2), float("nan"), dtype=torch.float64, device=U.DEV)
        hip.check(lib.ccdm_stats_fold(st.data_ptr(), N, S, Cc, hip.STATS_FOLD_SLICES, out.data_ptr(), 0), "stats_fold")
        U.sync()
        return y, out
    sweep(produce, "k_conv 256x512 (raw partials)")
    sweep(produce_folded, "ccdm_stats_fold 256x512 -> 16 slices")


# ------------------------------------------------------------------------------------------ 2. consumers
def exact_stats(x_nhwc):
    """fp64 partials [N, 1, C, 2] of an fp32 tensor: products of fp32 values are exact in fp64"""
    xd = x_nhwc.detach().cpu().double()
    return torch.stack([xd.sum((1, 2)), (xd * xd).sum((1, 2))], -1)[:, None].contiguous().to(x_nhwc.device)


def awkward_input(rng, N, Cc, H, W):
    """groups (32 of them) of every kind that goes wrong: group 0 constant (var clamps to 0, rstd = 1/sqrt(eps)), group 1 with variance
    below eps, group 2 at variance ~eps, groups 3-4 with mean / std = 100, the rest ordinary"""
    x = rnd(rng, N, Cc, H, W) * 1.3 + 0.2
    cpg = Cc // 32
    grp = lambda g: slice(g * cpg, (g + 1) * cpg)
    x[:, grp(0)] = 0.75
    x[:, grp(1)] = 0.5 + rnd(rng, N, cpg, H, W) * 1e-3
    x[:, grp(2)] = -1.25 + rnd(rng, N, cpg, H, W) * 3e-3
    x[:, grp(3)] = 100.0 + rnd(rng, N, cpg, H, W)
    x[:, grp(4)] = -37.0 + rnd(rng, N, cpg, H, W) * 0.37
    return x


def affine_params(rng, Cc, big_gamma):
    g = 1 + rnd(rng, Cc, scale=0.2)
    if big_gamma:
        g[: Cc // 2] *= 25.0
    return g, rnd(rng, Cc, scale=0.2)


def gn_f64(x, g, b, film=None):
    h = F.group_norm(x.double(), 32, g.double(), b.double(), EPS)
    if film is not None:                                  # h * (1 + scale) + shift (unet.py:254-258)
        sc, sh = film
        h = h * (1 + sc.double()[:, :, None, None]) + sh.double()[:, :, None, None]
    return h


# (c0, cout, H, W, prec, diag): k_conv at the full-resolution and the 32^2 shapes, k_conv_ks at 16^2 / 8^2
CONSUMER_CONV_CASES = [(32, 32, 128, 128, hip.PREC_F32, 0), (32, 32, 128, 128, hip.PREC_F16X3, 0), (64, 64, 32, 32, hip.PREC_F16X3, 0),
                       (96, 96, 16, 16, hip.PREC_F16X3, 0), (128, 128, 8, 8, hip.PREC_F16X3, 0), (128, 128, 8, 8, hip.PREC_F16X3, 1)]


@pytest.mark.parametrize("mode", ["plain", "big_gamma", "film"])
@pytest.mark.parametrize("case", CONSUMER_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gn_consumer_conv(U, case, mode):
    """GroupNorm + SiLU staged by k_conv / k_conv_ks against float64 conv(SiLU(GN(x))), bar of test_conv (2e-5)"""
    c0, cout, H, W, prec, diag = case
    rng = np.random.default_rng(c0 + H + len(mode))
    N = 2
    x = awkward_input(rng, N, c0, H, W)
    g, b = affine_params(rng, c0, mode == "big_gamma")
    w = unit_weight(rng, cout, c0, 3)
    if mode == "big_gamma":
        w = w / 25.0                                       # keeps the output O(1): the bar is absolute
    bias = rnd(rng, cout, scale=0.1)
    film = (rnd(rng, N, c0, scale=0.5), rnd(rng, N, c0, scale=0.5)) if mode == "film" else None
    ref = F.conv2d(F.silu(gn_f64(x, g, b, film)), w.double(), bias.double(), padding=1)
    xs = U.nhwc(x)
    out, _ = U.conv2d([xs], w.numpy(), bias.numpy(), 3, stats=[exact_stats(xs)], gamma=g.numpy(), beta=b.numpy(), act=hip.ACT_SILU,
                      film=torch.cat(film, 1).numpy() if film else None, emb_rows=np.arange(N) if film else None, prec=prec,
                      want_stats=False, diag=hip.DIAG_GENERAL_KERNEL if diag else 0)
    err = (U.bchw(out).double() - ref).abs()
    print(f"consumer conv {case} {mode}: max err {err.max().item():.2e}")
    assert err.max().item() <= 2e-5


@pytest.mark.parametrize("cin,cout,H,W", [(96, 288, 16, 16), (128, 384, 32, 64)])
def test_gn_consumer_norm_qkv_1x1(U, cin, cout, H, W):
    """AttentionBlock.norm + qkv as a GroupNorm-on-load 1x1 conv, bar of test_norm_qkv_1x1_conv_kernel (3e-5)"""
    rng = np.random.default_rng(cin + W)
    N = 2
    x = awkward_input(rng, N, cin, H, W)
    g, b = affine_params(rng, cin, False)
    w = unit_weight(rng, cout, cin, 1)
    bias = rnd(rng, cout, scale=0.1)
    ref = F.conv2d(gn_f64(x, g, b), w.double(), bias.double())
    xs = U.nhwc(x)
    out, _ = U.conv2d([xs], w.numpy(), bias.numpy(), 1, stats=[exact_stats(xs)], gamma=g.numpy(), beta=b.numpy(), prec=hip.PREC_F16X3,
                      want_stats=False)
    err = (U.bchw(out).double() - ref).abs().max().item()
    print(f"consumer norm+qkv {cin}->{cout} {H}x{W}: max err {err:.2e}")
    assert err <= 3e-5


@pytest.mark.parametrize("C_,H,W", [(96, 16, 16), (128, 8, 8)])
def test_gn_consumer_attention_block_prologue(U, C_, H, W):
    """ccdm_norm_qkv_attention: GroupNorm applied in the fused attention block's prologue, against a float64 GN -> qkv -> attention,
    bar of the attention block tests (3e-5)"""
    rng = np.random.default_rng(C_ + H)
    N = 2
    x = awkward_input(rng, N, C_, H, W)
    g, b = affine_params(rng, C_, False)
    qw = (rnd(rng, 3 * C_, C_, 1) / np.sqrt(C_)).numpy()
    qb = rnd(rng, 3 * C_, scale=0.1).numpy()
    qkv = F.conv1d(gn_f64(x, g, b).reshape(N, C_, -1), torch.from_numpy(qw).double(), torch.from_numpy(qb).double())
    ref = O.qkv_attention_legacy(qkv, C_ // 32).reshape(N, C_, H, W)
    got = U.norm_qkv_attention(U.nhwc(x), g.numpy(), b.numpy(), qw, qb, C_ // 32, False)
    err = (U.bchw(got).double() - ref).abs().max().item()
    print(f"consumer attention prologue {C_} {H}x{W}: max err {err:.2e}")
    assert err <= 3e-5


@pytest.mark.parametrize("H,W", [(128, 128), (24, 96)])
def test_gn_consumer_head(U, H, W):
    """ccdm_head.hip (GroupNorm -> SiLU -> conv3x3 to K logits) against float64, bar of test_head_conv_fused_with_the_epilogue (2e-5)"""
    rng = np.random.default_rng(H + W)
    N, Cc, K = 2, 32, 2
    x = awkward_input(rng, N, Cc, H, W)
    g, b = affine_params(rng, Cc, False)
    w = rnd(rng, K, Cc, 3, 3) / np.sqrt(Cc * 9) * 2.0
    bias = rnd(rng, K, scale=0.3)
    ref = F.conv2d(F.silu(gn_f64(x, g, b)), w.double(), bias.double(), padding=1)
    xt = torch.from_numpy(rng.integers(0, K, (N, H * W))).to(torch.uint8).to(U.DEV)
    got = U.head_posterior(U.nhwc(x), g.numpy(), b.numpy(), w.numpy(), bias.numpy(), xt, 0.93, 0.41, hip.STEP_SAMPLE)
    logits = got["logits"].reshape(N, H, W, K).permute(0, 3, 1, 2).double()
    err = (logits - ref).abs().max().item()
    print(f"consumer head {H}x{W}: max err {err:.2e}")
    assert err <= 2e-5 and got["flag"] == 0


# ------------------------------------------------------------------------------------------ 3. block level
def resblock_f64(x, p, emb_out):
    """ResBlock (use_scale_shift_norm=False, identity skip) in float64: x + conv(SiLU(GN(conv(SiLU(GN(x))) + emb)))"""
    d = lambda t: torch.as_tensor(t).double()
    h = F.conv2d(F.silu(F.group_norm(x.double(), 32, d(p["g0"]), d(p["b0"]), EPS)), d(p["w1"]), d(p["c1"]), padding=1)
    h = h + d(emb_out)[:, :, None, None]
    h = F.conv2d(F.silu(F.group_norm(h, 32, d(p["g1"]), d(p["b1"]), EPS)), d(p["w2"]), d(p["c2"]), padding=1)
    return x.double() + h


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("C_,H,W", [(32, 128, 128), (64, 32, 32), (128, 8, 8)])
def test_resblock_with_offset_groups_vs_float64(U, C_, H, W, prec):
    """Two chained ResBlocks on synthetic weights whose conv biases push half the groups of every GroupNorm input to mean/std ~100:
    each GroupNorm reads the partials the previous kernel left.  Against a float64 evaluation, under the 1e-4 output contract."""
    rng = np.random.default_rng(C_ + H + prec)
    N = 2
    x = rnd(rng, N, C_, H, W)
    x[:, : C_ // 2] += 100.0                              # the block input itself: mean/std ~100 in half the groups
    blocks = []
    for _ in range(2):
        p = dict(g0=1 + rnd(rng, C_, scale=0.1), b0=rnd(rng, C_, scale=0.1), g1=1 + rnd(rng, C_, scale=0.1), b1=rnd(rng, C_, scale=0.1),
                 w1=unit_weight(rng, C_, C_, 3), w2=unit_weight(rng, C_, C_, 3) * 0.5)
        p["c1"] = torch.zeros(C_)
        p["c1"][: C_ // 2] = 100.0 * 0.55                 # conv1 output spread ~0.55: mean/std ~100 in the GroupNorm that reads it
        p["c2"] = rnd(rng, C_, scale=0.05)
        blocks.append((p, rnd(rng, N, C_, scale=0.3)))
    ref = x.double()
    xs = U.nhwc(x)
    st = U.gn_stats(xs, 1)
    for p, emb in blocks:
        ref = resblock_f64(ref, p, emb)
        h, hst = U.conv2d([xs], p["w1"].numpy(), p["c1"].numpy(), 3, stats=[st], gamma=p["g0"].numpy(), beta=p["b0"].numpy(), act=hip.ACT_SILU,
                          emb=emb.numpy(), emb_rows=np.arange(N), prec=prec)
        xs, st = U.conv2d([h], p["w2"].numpy(), p["c2"].numpy(), 3, stats=[hst], gamma=p["g1"].numpy(), beta=p["b1"].numpy(), act=hip.ACT_SILU,
                          resid=xs, prec=prec)
    y = U.bchw(xs).double()
    err = (y - ref).abs().max().item()
    print(f"resblock x2 {C_}x{H}x{W} prec={prec}: max err {err:.2e}")
    assert err < 1e-4


# ------------------------------------------------------------------------------------------ 3. step level
class _Float64Oracle:
    """The oracle's U-Net (oracle/ccdm_oracle.py) evaluated in float64: inside this context `Tensor.float()` — the only place the oracle
    fixes a precision — returns float64, and the state dict is handed over in float64.  Every GroupNorm input it meets is recorded as
    (weight key, max over groups of |mean| / std, mean over groups of std)."""

    def __init__(self, sd):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.key_of = {id(v): k for k, v in self.sd.items()}
        self.seen = []

    def __enter__(self):
        self._float, self._gn = torch.Tensor.float, O.group_norm32

        def gn(x, w, b):
            g = x.double().reshape(x.shape[0], 32, -1)
            std = g.std(-1, unbiased=False)
            self.seen.append((self.key_of.get(id(w)), (g.mean(-1).abs() / std.clamp_min(1e-30)).max().item(), std.mean().item()))
            return self._gn(x, w, b)
        torch.Tensor.float = lambda t, *a, **k: t.double()
        O.group_norm32 = gn
        return self

    def __exit__(self, *exc):
        torch.Tensor.float, O.group_norm32 = self._float, self._gn

    def step(self, x, image, t):
        self.seen = []
        return O.unet_forward(self.sd, dict(num_heads=1, num_head_channels=32), x.double(), image.double(), None, t)["diffusion_out"]


LIDC_BP = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32,
               softmax_output=True)


def _offset_lidc(prec):
    """the LIDC C2 network on synthetic weights whose ResBlock conv1 biases put half the channels of every ResBlock's second GroupNorm
    input at mean / std ~100 (calibrated on a float64 pass of the plain weights: 100 x that GroupNorm input's measured spread)"""
    from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict
    model = build_model(250, "cosine", {"s": 0.008}, [(1, 128, 128), (2, 128, 128)], (1, 128, 128), "unet_openai", LIDC_BP,
                        "datasets.lidc", "confidence", None)
    sd = {k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}
    rng = np.random.default_rng(99)
    image = torch.from_numpy(rng.uniform(-1, 1, (1, 1, 128, 128)).astype(np.float32))
    x = torch.from_numpy(np.eye(2, dtype=np.float32)[rng.integers(0, 2, (1, 128, 128))]).permute(0, 3, 1, 2).contiguous()
    with _Float64Oracle(sd) as ref:
        ref.step(x, image, torch.full((1,), 37.0))
        spread = {k: s for k, _, s in ref.seen if k and k.endswith("out_layers.0.weight")}
    assert spread, "no ResBlock GroupNorm recorded"
    for k, s in spread.items():
        bias = sd[k.replace("out_layers.0.weight", "in_layers.2.bias")]
        bias[: bias.shape[0] // 2] += 100.0 * s
    model.unet.load_state_dict(sd, strict=True)
    model.prec = prec
    return model.to("cuda:0").eval(), sd, image


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_unet_step_and_walk_with_offset_groups_vs_float64(U, prec):
    """A whole C2 U-Net step (128^2) with groups at mean / std ~100 in every ResBlock, against the float64 evaluation of the same
    operations: the output probabilities within the 1e-4 contract.  Then a short strided walk (t = 200, 120, 40), teacher-forced on the
    float64 draws: at every step the class draw argmax p / E of the kernels' probabilities must equal the float64 one except at near-ties
    whose runner-up is the float64 class (assert_only_near_ties)."""
    from tests.test_hip_parity import assert_only_near_ties
    model, sd, image = _offset_lidc(prec)
    rng = np.random.default_rng(7)
    xt = torch.from_numpy(rng.integers(0, 2, (1, 128, 128)))
    with _Float64Oracle(sd) as ref:
        for j, t in enumerate((37.0, 200.0, 120.0, 40.0)):
            x = O.one_hot_bchw(xt, 2)
            tt = torch.full((1,), t)
            want = ref.step(x, image, tt)
            ratios = [r for k, r, _ in ref.seen if k and k.endswith("out_layers.0.weight")]
            got = model(x.to(U.DEV), image.to(U.DEV), t=tt, validation=True)["diffusion_out"].cpu().double()
            err = (got - want).abs().max().item()
            print(f"prec={prec} t={t:g}: max|dp| {err:.2e}; ResBlock GroupNorm inputs at mean/std {min(ratios):.0f}..{max(ratios):.0f}")
            assert min(ratios) > 30, "the offset did not reach the GroupNorm inputs"
            assert err < 1e-4
            if j == 0:
                continue                                        # the first t is the plain step check
            noise = torch.from_numpy(rng.exponential(1.0, (1, 128, 128, 2)))
            p_ref = want.permute(0, 2, 3, 1)
            idx_ref = torch.argmax(p_ref / noise, -1)
            assert_only_near_ties(got.permute(0, 2, 3, 1), noise, idx_ref, f"offset walk prec={prec} t={t:g}")
            xt = idx_ref
