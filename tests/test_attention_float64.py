"""Attention kernels against float64 on peaked softmax rows.

The other attention tests draw q, k, v at about 1.3 N(0, 1): scores of standard deviation ~1, a row's largest probability a few percent,
the running sum l in the tens to hundreds.  A trained denoiser's rows are peaked instead — one or two keys carry the weight and the scores
span tens of units — and that reaches arithmetic diffuse rows never test: P = 2^(s - max) split into fp16 hi / lo while most of it is
below fp16's smallest normal 2^-14, the online rescale exp(m - mx) ~ 0 after o and l have built up (dominant key in a late or ragged last
tile), the split's relative error on scores of |s| ~ 100-300, and near-ties between two dominant keys whose v rows differ.

Every case is compared with softmax((q s)(k s)^T) v evaluated in float64 on the CPU, and with the oracle's fp32 evaluation of the same
inputs (what the reference itself computes).  Bar: err_kernel <= max(2 err_fp32, FLOOR vmax), errors = max |out - float64|; in the
v_range regime also per head channel c, with an absolute floor 2^-24 (what the fp16 split keeps of a v below fp16's normal range).
Every case asserts from the float64 evaluation that its regime was reached, and logs both errors and the regime metric through
parity_log.

  1. the core (ccdm_attention / ccdm_attention_ex): every dispatch branch of launch_attention / launch_attention_mfma, six regimes;
  2. the fused GroupNorm + qkv + attention kernel (ccdm_norm_qkv_attention) at every geometry it is built for, the regime set through
     the block's parameters, and the general GroupNorm-on-load qkv conv + core at a geometry the fused kernel does not take;
  3. whole C2 U-Net steps whose AttentionBlocks all have peaked rows, against the float64 step."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from oracle import ccdm_oracle as O
from tests.test_gn_statistics import _Float64Oracle

pytestmark = pytest.mark.gpu

SUB = 2.0 ** -14                    # fp16's smallest normal: P below it is split into subnormal halves
FLOOR_CORE = 3e-6                   # x vmax
FLOOR_FUSED = 5e-6                  # x vmax: the fused kernel's own qkv GEMM adds its split's error
FLOOR_ABS = 2.0 ** -24              # absolute floor of the fp16 split (per-channel bar of v_range)
PEAK_STD = (8.0, 30.0)              # score standard deviation of the peaked rows (alternating over (sample, head))
OFFSET = (100.0, 300.0)             # |common score offset| of the offset regime
LATE_BOOST = 60.0                   # score of the late dominant key over the rest
TIE_BOOST = 40.0                    # score of the two near-tied keys over the rest
TIE_GAP = 1e-3                      # |score difference| of the near-tied keys
FP16_OPERAND_MAX = 1e3              # |q s log2 e|, |k s| of every case (overflow is tested elsewhere)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from tests import hip_util
    hip.load()
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    return hip_util


# ------------------------------------------------------------------------------------------ float64 reference
def attn_f64(q, k, v):
    """softmax((q s)(k s)^T) v in float64, q, k, v [B, T, D] (any float type), s = D^-1/4; query rows in chunks of at most 2^25
    scores.  Returns (out [B, T, D] float64, per-row statistics of P and of the scores)."""
    q, k, v = q.double(), k.double(), v.double()
    B, T, D = q.shape
    sc = 1 / math.sqrt(math.sqrt(D))
    out = torch.empty((B, T, D), dtype=torch.float64)
    st = {n: torch.empty((B, T), dtype=torch.float64) for n in ("p1", "p2", "smax", "sstd")}
    arg = torch.empty((B, T), dtype=torch.int64)
    nsub = 0
    chunk = max(1, (1 << 25) // T)
    for b in range(B):
        kb = k[b] * sc
        for t0 in range(0, T, chunk):
            s = (q[b, t0:t0 + chunk] * sc) @ kb.T
            p = torch.softmax(s, -1)
            out[b, t0:t0 + chunk] = p @ v[b]
            top = torch.topk(p, min(2, T), -1)
            st["p1"][b, t0:t0 + chunk] = top.values[:, 0]
            st["p2"][b, t0:t0 + chunk] = top.values[:, -1]
            arg[b, t0:t0 + chunk] = top.indices[:, 0]
            st["smax"][b, t0:t0 + chunk] = s.abs().amax(-1)
            st["sstd"][b, t0:t0 + chunk] = s.std(-1)
            nsub += int((p < SUB).sum())
    st["argmax"] = arg
    st["frac_sub"] = nsub / (B * T * T)
    return out, st


def metrics(st):
    """the regime metrics of a case (logged for every case)"""
    return dict(maxp_median=st["p1"].median().item(), frac_p_below_2m14=st["frac_sub"], smax_median=st["smax"].median().item(),
                score_std_median=st["sstd"].median().item(), gap_median=(st["p1"].log() - st["p2"].log()).median().item(),
                top2_median=(st["p1"] + st["p2"]).median().item(),
                top2_asym_median=((st["p1"] - st["p2"]) / (st["p1"] + st["p2"])).median().item())


def regime_problem(regime, st, planned=None):
    """None if the float64 evaluation shows the regime's defining property, else what is missing"""
    m = metrics(st)
    if regime in ("peaked", "v_range") and not (m["maxp_median"] >= 0.5 and m["frac_p_below_2m14"] >= 0.5):
        return f"peaked rows not reached: median row max p {m['maxp_median']:.3f} (want >= 0.5), fraction of p < 2^-14 " \
               f"{m['frac_p_below_2m14']:.3f} (want >= 0.5)"
    if regime == "offset" and not (m["maxp_median"] >= 0.5 and m["smax_median"] >= 0.5 * OFFSET[0]):
        return f"offset scores not reached: median row max |s| {m['smax_median']:.1f} (want >= {0.5 * OFFSET[0]:g}), median row max p " \
               f"{m['maxp_median']:.3f}"
    if regime == "late_max":
        hit = (st["argmax"] == planned).double().mean().item() if planned is not None else 1.0
        if not (hit >= 0.9 and m["gap_median"] >= LATE_BOOST / 2):
            return f"late dominant key not reached: argmax at the planned key in {hit:.3f} of the rows (want >= 0.9), median score gap " \
                   f"to the runner-up {m['gap_median']:.1f} (want >= {LATE_BOOST / 2:g})"
    if regime == "near_tie" and not (m["top2_median"] >= 0.9 and abs(m["top2_asym_median"]) <= TIE_GAP):
        return f"near-ties not reached: median p1 + p2 {m['top2_median']:.3f} (want >= 0.9), median (p1 - p2) / (p1 + p2) " \
               f"{m['top2_asym_median']:.2e} (want <= {TIE_GAP:g})"
    return None


# ------------------------------------------------------------------------------------------ layouts
def qkv_rows(heads, D, order, which):
    """channel indices of q (which = 0), k (1) or v (2) of every head, [heads, D], in the reference's qkv tensor"""
    h, d = np.arange(heads)[:, None], np.arange(D)[None]
    return h * 3 * D + which * D + d if order == 0 else which * heads * D + h * D + d


def pack_qkv(q, k, v, order):
    """q, k, v [N, heads, T, D] -> the reference's qkv [N, 3C, T] in channel order `order`"""
    N, H, T, D = q.shape
    qkv = torch.empty((N, 3 * H * D, T), dtype=q.dtype)
    for j, a in enumerate((q, k, v)):
        qkv[:, torch.from_numpy(qkv_rows(H, D, order, j).reshape(-1))] = a.permute(0, 1, 3, 2).reshape(N, H * D, T)
    return qkv


def unpack_qkv(qkv, heads, order):
    """the reference's qkv [N, 3C, T] -> q, k, v [N * heads, T, D]"""
    N, C3, T = qkv.shape
    D = C3 // (3 * heads)
    return [qkv[:, torch.from_numpy(qkv_rows(heads, D, order, j).reshape(-1))].reshape(N, heads, D, T).permute(0, 1, 3, 2)
            .reshape(N * heads, T, D) for j in range(3)]


def oracle_fp32(qkv, heads, order):
    """the oracle's fp32 attention of the reference's qkv [N, 3C, T], one sample at a time -> [N * heads, T, D]"""
    f = O.qkv_attention_new if order else O.qkv_attention_legacy
    out = torch.cat([f(qkv[n:n + 1].float(), heads) for n in range(qkv.shape[0])])
    N, C, T = out.shape
    return out.reshape(N, heads, C // heads, T).permute(0, 1, 3, 2).reshape(N * heads, T, C // heads)


def operand_range(q, k):
    D = q.shape[-1]
    s = 1 / math.sqrt(math.sqrt(D))
    return max(q.abs().max().item() * s * math.log2(math.e), k.abs().max().item() * s)


# ------------------------------------------------------------------------------------------ regimes (q, k, v per (sample, head))
def _distinct_keys(T, want):
    """`want` distinct key positions that matter to the kernels' tiling: the first key, the last key (ragged last tile), the first key of
    the last 64-key tile, a middle key, the end of the first tile, ..."""
    cand = [0, T - 1, 64 * ((T - 1) // 64), T // 2, min(63, T - 2), 1, T - 2, T // 3, 2 * T // 3, 33]
    keys = []
    for j in cand:
        if 0 <= j < T and j not in keys:
            keys.append(j)
    assert len(keys) >= want, (T, want)
    return keys[:want]


def regime_diffuse(rng, N, T, heads, D):
    """the existing tests' inputs: every operand 1.3 N(0, 1), score std ~1.7"""
    return [1.3 * rng.standard_normal((N, heads, T, D)) for _ in range(3)], None


def regime_peaked(rng, N, T, heads, D):
    """q, k entries N(0, a^2): the score std is a^2 = PEAK_STD, alternating 8 / 30 over (sample, head)"""
    std = np.array(PEAK_STD)[(np.arange(N)[:, None] * heads + np.arange(heads)[None]) % 2]
    a = np.sqrt(std)[..., None, None]
    return [a * rng.standard_normal((N, heads, T, D)), a * rng.standard_normal((N, heads, T, D)),
            1.3 * rng.standard_normal((N, heads, T, D))], None


def regime_offset(rng, N, T, heads, D):
    """peaked rows shifted by a common c, |c| in [100, 300]: a unit direction e is projected out of every q and k, then
    q += alpha e, k += beta e with alpha beta / sqrt(D) = c, so every score of the (sample, head) moves by c and softmax does not"""
    (q, k, v), _ = regime_peaked(rng, N, T, heads, D)
    for n in range(N):
        for h in range(heads):
            e = rng.standard_normal(D)
            e /= np.linalg.norm(e)
            c = rng.uniform(*OFFSET) * rng.choice([-1.0, 1.0])
            ab = math.sqrt(abs(c) * math.sqrt(D))
            q[n, h] += (ab - q[n, h] @ e)[:, None] * e
            k[n, h] += (math.copysign(ab, c) - k[n, h] @ e)[:, None] * e
    return [q, k, v], None


def _boosted(rng, N, T, heads, D, keys_per_query, boost, groups):
    """diffuse q, k, v whose last `groups` channels are markers: query t of group g = t % groups gets `boost` added to its scores with
    the key(s) of group g.  Returns (q, k, v, the group's keys)."""
    (q, k, v), _ = regime_diffuse(rng, N, T, heads, D)
    keys = _distinct_keys(T, groups * keys_per_query)
    keys = [keys[g * keys_per_query:(g + 1) * keys_per_query] for g in range(groups)]
    beta = math.sqrt(boost * math.sqrt(D))
    q[..., D - groups:] = 0.0
    k[..., D - groups:] = 0.0
    for g, ks in enumerate(keys):
        ch = D - groups + g
        q[:, :, g::groups, ch] = boost * math.sqrt(D) / beta
        for j in ks:
            k[:, :, j, ch] = beta
    return q, k, v, keys


def regime_late_max(rng, N, T, heads, D):
    """one key per query LATE_BOOST above the rest: key 0, the last key T - 1 (ragged last tile: the masked keys beyond T sit next to it),
    the first key of the last tile and a middle key — a running sum built over the earlier tiles is rescaled by exp(-60) ~ 0"""
    groups = 4
    q, k, v, keys = _boosted(rng, N, T, heads, D, 1, LATE_BOOST, groups)
    planned = torch.tensor([keys[t % groups][0] for t in range(T)])
    return [q, k, v], planned.expand(N * heads, T)


def regime_near_tie(rng, N, T, heads, D):
    """two keys per query TIE_BOOST above the rest and within TIE_GAP of each other (the second key's row is a copy of the first's, its
    marker moved by the gap); their v rows are independent draws, so the output is a ~50/50 blend of two O(1)-apart rows"""
    groups = 3
    q, k, v, keys = _boosted(rng, N, T, heads, D, 2, TIE_BOOST, groups)
    for g, (j1, j2) in enumerate(keys):
        ch = D - groups + g
        k[:, :, j2] = k[:, :, j1]
        k[:, :, j2, ch] *= 1.0 + rng.uniform(-1.0, 1.0, (N, heads)) * TIE_GAP / TIE_BOOST
    return [q, k, v], None


def v_channel_scales(D):
    """v_range: two channels at 1e3, a quarter of them at 1e-3, a quarter at 1e-6 (below fp16's normal range), the rest at 1"""
    s = np.ones(D)
    s[:2] = 1e3
    s[2:2 + D // 4] = 1e-3
    s[2 + D // 4:2 + D // 2] = 1e-6
    return s


def regime_v_range(rng, N, T, heads, D):
    """peaked rows whose v channels span 1e-6 .. 1e3"""
    (q, k, v), _ = regime_peaked(rng, N, T, heads, D)
    return [q, k, v * v_channel_scales(D)], None


REGIMES = dict(diffuse=regime_diffuse, peaked=regime_peaked, offset=regime_offset, late_max=regime_late_max, near_tie=regime_near_tie,
               v_range=regime_v_range)


def make_case(regime, rng, N, T, heads, D):
    """-> (q, k, v as fp32-valued float64 [N * heads, T, D], planned argmax or None)"""
    qkv, planned = REGIMES[regime](rng, N, T, heads, D)
    q, k, v = [torch.from_numpy(a.astype(np.float32)).double().reshape(N * heads, T, D) for a in qkv]
    return q, k, v, planned


# ------------------------------------------------------------------------------------------ bar
def check_bar(what, regime, kernel, got, ref, f32, v, floor, parity_log, st, per_channel=False):
    """got, ref, f32 [B, T, D]: the kernel's, the float64 and the oracle-fp32 outputs; v [B, T, D] the values"""
    err_k = (got.double() - ref).abs()
    err_f = (f32.double() - ref).abs()
    vmax = v.abs().max().item()
    ek, ef = err_k.max().item(), err_f.max().item()
    bar = max(2 * ef, floor * vmax)
    m = metrics(st)
    parity_log(f"attention_float64[{what}]", regime=regime, kernel=kernel, err_kernel_over_vmax=ek / vmax, err_fp32_over_vmax=ef / vmax,
               vmax=vmax, bar_over_vmax=bar / vmax, **m)
    print(f"{what}: err/vmax kernel {ek / vmax:.2e} fp32 {ef / vmax:.2e} (bar {bar / vmax:.2e}); median max p {m['maxp_median']:.3f}, "
          f"p < 2^-14 {m['frac_p_below_2m14']:.3f}, median max|s| {m['smax_median']:.1f}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert ek <= bar, f"{what} ({kernel}, {regime}): max err {ek:.3e} = {ek / vmax:.2e} vmax against float64, bar {bar:.3e} " \
                      f"(fp32 reference {ef:.3e}); regime {m}"
    if per_channel:
        ekc, efc = err_k.amax((0, 1)), err_f.amax((0, 1))
        vmc = v.abs().amax((0, 1))
        barc = torch.maximum(torch.maximum(2 * efc, floor * vmc), torch.full_like(vmc, FLOOR_ABS))
        worst = int(torch.argmax(ekc / barc))
        parity_log(f"attention_float64[{what}]", worst_channel=worst, worst_channel_err_over_bar=(ekc / barc)[worst].item())
        assert (ekc <= barc).all(), f"{what}: channel {worst} (|v| <= {vmc[worst].item():.1e}) err {ekc[worst].item():.3e} against float64, " \
                                    f"bar {barc[worst].item():.3e} (fp32 reference {efc[worst].item():.3e})"


# ------------------------------------------------------------------------------------------ 1. the core
# (id, head width D, T, allocated rows Ta, heads, N, order incl. the force-VALU bit): every branch of launch_attention /
# launch_attention_mfma
CORE_CASES = [
    ("d32_t32_1wave", 32, 32, 32, 2, 2, 0),
    ("d32_t64_2waves", 32, 64, 64, 2, 2, 1),
    ("d32_t256_4waves", 32, 256, 256, 3, 2, 0),
    ("d32_t256_4waves_new", 32, 256, 256, 3, 2, 1),
    ("d32_t2048_4waves", 32, 2048, 2048, 2, 1, 1),
    ("d32_t2048_8waves", 32, 2048, 2048, 4, 8, 0),          # cdiv(T, 256) * heads * N = 256: 8-wave blocks
    ("d32_t100_valu", 32, 100, 100, 2, 2, 0),               # T % 32 != 0: the VALU kernel
    ("d64_dino197", 64, 197, 208, 6, 2, 1),                 # the ViT encoder's padded rows
    ("d64_dino785", 64, 785, 800, 6, 1, 1),
    ("d96", 96, 256, 256, 1, 2, 0),
    ("d128_ragged", 128, 333, 333, 1, 2, 1),
    ("d24_padded", 24, 256, 256, 4, 2, 0),
    ("d80_padded", 80, 100, 100, 2, 2, 1),
    ("d32_forced_valu", 32, 256, 256, 2, 2, hip.ATTENTION_FORCE_VALU),
    ("d64_forced_valu", 64, 197, 208, 2, 2, 1 | hip.ATTENTION_FORCE_VALU),
]
LONG_CASES = [("d32_t8192_c5", 32, 8192, 8192, 2, 1, 0)]


def core_kernel(D, T, Ta, order):
    """which kernel launch_attention runs the case on (ccdm_misc.hip)"""
    if order & hip.ATTENTION_FORCE_VALU or (D == 32 and (T % 32 or Ta != T)):
        return "k_attention(valu)"
    return "k_attention_mfma"


def run_core_case(U, parity_log, case, regime):
    name, D, T, Ta, heads, N, order = case
    rng = np.random.default_rng(zlib.crc32(f"{name}/{regime}".encode()))
    q, k, v, planned = make_case(regime, rng, N, T, heads, D)
    kernel = core_kernel(D, T, Ta, order)
    what = f"{name}/{regime}"
    ref, st = attn_f64(q, k, v)
    problem = regime_problem(regime, st, planned)
    assert problem is None, f"{what}: {problem}"
    assert operand_range(q, k) <= FP16_OPERAND_MAX, f"{what}: operands beyond the range this test is for"
    qkv = pack_qkv(*(a.reshape(N, heads, T, D) for a in (q, k, v)), order & 255)          # [N, 3C, T]
    f32 = oracle_fp32(qkv, heads, order & 255)
    C = heads * D
    buf = torch.full((N, Ta, 3 * C), 7.0)
    buf[:, :T] = qkv.permute(0, 2, 1).float()
    buf = buf.to(U.DEV)
    out = torch.full((N, Ta, C), float("nan"), device=U.DEV)
    hip.check(hip.load().ccdm_attention_ex(buf.data_ptr(), out.data_ptr(), N, T, Ta, C, heads, order, 0), "attention_ex")
    U.sync()
    got = out.cpu()
    assert torch.isnan(got[:, T:]).all(), f"{what}: padding rows written"
    got = got[:, :T].reshape(N, T, heads, D).permute(0, 2, 1, 3).reshape(N * heads, T, D)
    check_bar(what, regime, kernel, got, ref, f32, v, FLOOR_CORE, parity_log, st, per_channel=regime == "v_range")


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("case", CORE_CASES, ids=lambda c: c[0])
def test_attention_core_vs_float64(U, parity_log, case, regime):
    run_core_case(U, parity_log, case, regime)


@pytest.mark.parametrize("regime", ["peaked", "late_max"])
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c[0])
def test_attention_core_long_sequence_vs_float64(U, parity_log, case, regime):
    """the C5 shape: 8192 tokens at head width 32"""
    run_core_case(U, parity_log, case, regime)


# ------------------------------------------------------------------------------------------ 2. fused block and the general path
FUSED_GEOMS = [(64, 96), (64, 128), (256, 96), (256, 128), (128, 128), (128, 256)]      # every (T, C) ccdm_norm_qkv_attention is built for
HW_OF = {64: (8, 8), 128: (8, 16), 256: (16, 16), 512: (16, 32)}
EPS = 1e-5
LATE_KEY_FROM_END = 5               # the fused late_max regime's outlier token: T - 5, in the last round of key tiles


def chain_f64(x, nw, nb, qw, qb):
    """AttentionBlock.norm + qkv in float64: x [N, C, T] -> qkv [N, 3C, T]"""
    return F.conv1d(F.group_norm(x.double(), 32, nw.double(), nb.double(), EPS), qw.double(), qb.double())


def chain_f32(x, nw, nb, qw, qb):
    """the oracle's fp32 evaluation of the same"""
    return F.conv1d(O.group_norm32(x, nw, nb), qw, qb)


def block_regime(regime, rng, N, T, C, heads, order):
    """AttentionBlock parameters (x [N, C, T], norm weight / bias, qkv weight [3C, C, 1] / bias, fp32) whose attention rows are in
    `regime`, calibrated on float64 passes; returns them with the planned argmax key (late_max) or None."""
    D = C // heads
    x = torch.from_numpy((1.5 * rng.standard_normal((N, C, T)) + 0.3).astype(np.float32))
    nw = torch.from_numpy((1 + 0.1 * rng.standard_normal(C)).astype(np.float32))
    nb = torch.from_numpy((0.1 * rng.standard_normal(C)).astype(np.float32))
    qw = rng.standard_normal((3 * C, C, 1)) / np.sqrt(C)
    qb = 0.1 * rng.standard_normal(3 * C)
    rq, rk = qkv_rows(heads, D, order, 0), qkv_rows(heads, D, order, 1)

    def stats_of(x_, qw_, qb_):
        q, k, v = unpack_qkv(chain_f64(x_, nw, nb, torch.from_numpy(qw_), torch.from_numpy(qb_)), heads, order)
        return q, k, attn_f64(q, k, v)[1]
    planned = None
    if regime in ("peaked", "offset"):
        # q and k rows scaled by alpha: the score std grows as alpha^2
        alpha = math.sqrt(PEAK_STD[0] / stats_of(x, qw, qb)[2]["sstd"].median().item())
        for r in (rq, rk):
            qw[r.reshape(-1)] *= alpha
            qb[r.reshape(-1)] *= alpha
    if regime == "offset":
        # a large k bias along a unit direction r_h per head moves every score of query t by q_t . b_k / sqrt(D), softmax does not
        q = stats_of(x, qw, qb)[0].reshape(N, heads, T, D)
        for h in range(heads):
            r = rng.standard_normal(D)
            r /= np.linalg.norm(r)
            mu = (q[:, h] @ torch.from_numpy(r)).abs().median().item() / math.sqrt(D)
            qb[rk[h]] += 0.5 * (OFFSET[0] + OFFSET[1]) / mu * r
    if regime == "late_max":
        # one outlier token j of x along a unit direction d of the channels; every head's k rows map d onto a unit u_h that every
        # query leans towards through its q bias; the outlier's size is searched so that its key dominates every row by far
        j = T - LATE_KEY_FROM_END
        d = rng.standard_normal(C)
        d /= np.linalg.norm(d)
        for h in range(heads):
            u = rng.standard_normal(D)
            u /= np.linalg.norm(u)
            wk = qw[rk[h], :, 0]
            qw[rk[h], :, 0] = wk - np.outer(wk @ d, d) + 3.0 * np.outer(u, d)
            qb[rq[h]] += 4.0 * u
        planned = torch.full((N * heads, T), j)
        x0 = x.clone()
        for lam in 2.0 ** np.arange(0, 14):
            x = x0.clone()
            x[:, :, j] += torch.from_numpy((lam * d).astype(np.float32))
            if regime_problem(regime, stats_of(x, qw, qb)[2], planned) is None:
                break
    qw, qb = torch.from_numpy(qw.astype(np.float32)), torch.from_numpy(qb.astype(np.float32))
    return x, nw, nb, qw, qb, planned


def run_block_case(U, parity_log, what, regime, T, C, heads, order, fused):
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    N, D = 2, C // heads
    x, nw, nb, qw, qb, planned = block_regime(regime, rng, N, T, C, heads, order)
    qkv64 = chain_f64(x, nw, nb, qw, qb)
    q, k, v = unpack_qkv(qkv64, heads, order)
    ref, st = attn_f64(q, k, v)
    problem = regime_problem(regime, st, planned)
    assert problem is None, f"{what}: {problem}"
    assert operand_range(q, k) <= FP16_OPERAND_MAX, f"{what}: operands beyond the range this test is for"
    f32 = oracle_fp32(chain_f32(x, nw, nb, qw, qb), heads, order)
    h, w = HW_OF[T]
    xs = U.nhwc(x.reshape(N, C, h, w))
    if fused:
        assert hip.load().ccdm_norm_qkv_attention_supported(T, C, heads) == 1
        out = U.norm_qkv_attention(xs, nw.numpy(), nb.numpy(), qw.numpy(), qb.numpy(), heads, bool(order))
        kernel = "k_qkv_attention"
    else:
        assert hip.load().ccdm_norm_qkv_attention_supported(T, C, heads) == 0
        qkv, _ = U.conv2d([xs], qw.numpy(), qb.numpy(), 1, stats=[U.gn_stats(xs, 1)], gamma=nw.numpy(), beta=nb.numpy(), want_stats=False,
                          prec=hip.PREC_F16X3)
        out = U.attention(qkv.reshape(N, T, 3 * C), heads, order)
        kernel = "k_conv(gn+qkv)+" + core_kernel(D, T, T, order)
    got = out.reshape(N, T, heads, D).permute(0, 2, 1, 3).reshape(N * heads, T, D).cpu()
    check_bar(what, regime, kernel, got, ref, f32, v, FLOOR_FUSED, parity_log, st)


@pytest.mark.parametrize("regime", ["diffuse", "peaked", "offset", "late_max"])
@pytest.mark.parametrize("order", [0, 1], ids=["legacy", "new"])
@pytest.mark.parametrize("T,C", FUSED_GEOMS)
def test_norm_qkv_attention_vs_float64(U, parity_log, T, C, order, regime):
    run_block_case(U, parity_log, f"fused_T{T}_C{C}_{'new' if order else 'legacy'}/{regime}", regime, T, C, C // 32, order, True)


@pytest.mark.parametrize("regime", ["peaked", "offset", "late_max"])
def test_gn_qkv_conv_then_attention_vs_float64(U, parity_log, regime):
    """the general path of the C4 / C5 networks' long-sequence blocks: GroupNorm-on-load qkv 1x1 conv, then the attention core
    (T = 512 at C = 128, 4 heads: a geometry the fused kernel does not take)"""
    run_block_case(U, parity_log, f"conv_core_T512_C128/{regime}", regime, 512, 128, 4, 0, False)


# ------------------------------------------------------------------------------------------ 3. whole step
LIDC_BP = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32,
               softmax_output=True)


class _Float64Attention(_Float64Oracle):
    """_Float64Oracle (the oracle's U-Net in float64) that also records, per AttentionBlock prefix, the float64 statistics of its softmax
    rows — as `seen` records the GroupNorm inputs — under a network config `cfg`."""

    def __init__(self, sd, cfg):
        super().__init__(sd)
        self.cfg = cfg
        self.attn = {}

    def __enter__(self):
        super().__enter__()
        self._block, self._legacy = O.attention_block, O.qkv_attention_legacy
        cur = [None]

        def block(sd, p, x, n_heads, new_order=False):
            cur[0] = p
            return self._block(sd, p, x, n_heads, new_order)

        def legacy(qkv, n_heads):
            self.attn[cur[0]] = metrics(attn_f64(*unpack_qkv(qkv.double(), n_heads, 0))[1])
            return self._legacy(qkv, n_heads)
        O.attention_block, O.qkv_attention_legacy = block, legacy
        return self

    def __exit__(self, *exc):
        O.attention_block, O.qkv_attention_legacy = self._block, self._legacy
        super().__exit__(*exc)

    def step(self, x, image, t):
        self.seen, self.attn = [], {}
        return O.unet_forward(self.sd, self.cfg, x.double(), image.double(), None, t)["diffusion_out"]


def _peaked_lidc(prec, bp, cfg, image, x):
    """the LIDC C2 network on synthetic weights whose AttentionBlocks all have peaked rows: the q and k rows of every qkv weight and
    bias scaled by alpha per block, calibrated on float64 passes to a median row score std of PEAK_STD[0] (and raised until every
    block's median row max p is >= 0.5)"""
    from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict
    model = build_model(250, "cosine", {"s": 0.008}, [(1, 128, 128), (2, 128, 128)], (1, 128, 128), "unet_openai", bp,
                        "datasets.lidc", "confidence", None)
    sd = {k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 0).items()}
    t = torch.full((1,), 37.0)
    scale = {}
    for _ in range(4):
        with _Float64Attention(sd, cfg) as ref:
            ref.step(x, image, t)
            seen = dict(ref.attn)
        assert len(seen) == 11, sorted(seen)
        todo = {p: m for p, m in seen.items() if (m["maxp_median"] < 0.5 or p not in scale)}
        if not todo:
            break
        for p, m in todo.items():
            w = sd[p + "qkv.weight"]
            C = w.shape[1]
            heads = O._heads(C, cfg["num_heads"], cfg["num_head_channels"])
            a = math.sqrt(PEAK_STD[0] / m["score_std_median"]) if p not in scale else 1.5
            scale[p] = scale.get(p, 1.0) * a
            r = torch.from_numpy(np.concatenate([qkv_rows(heads, C // heads, 0, 0).reshape(-1), qkv_rows(heads, C // heads, 0, 1).reshape(-1)]))
            w[r] *= a
            sd[p + "qkv.bias"][r] *= a
    model.unet.load_state_dict(sd, strict=True)
    model.prec = prec
    return model.to("cuda:0").eval(), sd


def assert_only_near_ties(ph, noise, idx_ref, what, tol):
    """tests/test_hip_parity.assert_only_near_ties with the near-tie tolerance `tol` (relative gap of the two best ratios) as a
    parameter: every pixel whose argmax p / E differs from the reference's must be a near-tie whose runner-up is the reference's class"""
    q = ph / noise
    bad = torch.argmax(q, -1) != idx_ref
    if bad.any():
        top, which = torch.topk(q, 2, -1)
        hard = bad & ~(((top[..., 0] - top[..., 1]) <= tol * top[..., 0]) & (which[..., 1] == idx_ref))
        assert not hard.any(), f"{what}: {int(hard.sum())} draw(s) differ from the reference's beyond a near-tie (tol {tol:.1e}), first at " \
                               f"{tuple(int(v) for v in torch.nonzero(hard)[0])}: ratios {top[tuple(torch.nonzero(hard)[0])].tolist()}"
        print(f"{what}: {int(bad.sum())} near-tie pixel(s) differ from the reference's draw (tol {tol:.1e})")

STEP_CASES = [("c2", LIDC_BP, dict(num_heads=1, num_head_channels=32), True),
              ("c2_default_heads", dict(LIDC_BP, num_heads=1, num_head_channels=-1), dict(num_heads=1, num_head_channels=-1), False)]


@pytest.mark.parametrize("prec", [hip.PREC_F32, hip.PREC_F16X3], ids=["f32", "f16x3"])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: c[0])
def test_unet_step_with_peaked_attention_vs_float64(U, parity_log, case, prec):
    """A whole C2 U-Net step (128^2) whose 11 AttentionBlocks all have peaked rows, against the float64 evaluation of the same
    operations: the output probabilities within the 1e-4 contract.  For the 32-wide heads then a teacher-forced strided walk
    (t = 200, 120, 40) as in test_unet_step_and_walk_with_offset_groups_vs_float64, its near-tie tolerance set by the reference's own
    fp32 step (assert_only_near_ties).  The default heads (num_head_channels = -1: one
    head of 96 / 128) run the general qkv conv + ccdm_attention path."""
    name, bp, cfg, walk = case
    rng = np.random.default_rng(7)
    image = torch.from_numpy(rng.uniform(-1, 1, (1, 1, 128, 128)).astype(np.float32))
    xt = torch.from_numpy(rng.integers(0, 2, (1, 128, 128)))
    model, sd = _peaked_lidc(prec, bp, cfg, image, O.one_hot_bchw(xt, 2))
    sd32 = {k: v.float() for k, v in sd.items()}
    for j, t in enumerate((37.0, 200.0, 120.0, 40.0) if walk else (37.0,)):
        x = O.one_hot_bchw(xt, 2)
        tt = torch.full((1,), t)
        with _Float64Attention(sd, cfg) as ref:
            want = ref.step(x, image, tt)
            maxp = {p: m["maxp_median"] for p, m in ref.attn.items()}
        got = model(x.to(U.DEV), image.to(U.DEV), t=tt, validation=True)["diffusion_out"].cpu().double()
        err = (got - want).abs().max().item()
        print(f"{name} prec={prec} t={t:g}: max|dp| {err:.2e}; AttentionBlock median row max p {min(maxp.values()):.3f}..{max(maxp.values()):.3f}")
        parity_log(f"attention_float64[unet_{name}_prec{prec}_t{t:g}]", max_dp=err, bar=1e-4, maxp_median_min=min(maxp.values()),
                   maxp_median_max=max(maxp.values()))
        assert len(maxp) == 11 and min(maxp.values()) >= 0.5, f"peaked rows not reached in every AttentionBlock: {maxp}"
        assert err < 1e-4
        if j == 0:
            continue
        noise = torch.from_numpy(rng.exponential(1.0, (1, 128, 128, 2)))
        idx_ref = torch.argmax(want.permute(0, 2, 3, 1) / noise, -1)
        # Peaked attention amplifies fp32 rounding upstream of it: the reference's own fp32 step (the oracle on fp32 weights) moves
        # the probabilities by up to ~6e-5 here and flips draws whose ratios are 3e-5 apart.  A draw may therefore differ from the
        # float64 one only where its two best ratios agree to twice that step's worst |dp| relative to p = 1/2 (and at least 1e-5).
        f32 = O.unet_forward(sd32, cfg, x, image, None, tt)["diffusion_out"].double()
        tie = max(1e-5, 2 * (f32 - want).abs().max().item() / 0.5)
        parity_log(f"attention_float64[unet_{name}_prec{prec}_t{t:g}]", max_dp_fp32_oracle=(f32 - want).abs().max().item(), tie_tol=tie)
        assert_only_near_ties(got.permute(0, 2, 3, 1), noise, idx_ref, f"peaked-attention walk {name} prec={prec} t={t:g}", tie)
        xt = idx_ref
    if prec == hip.PREC_F16X3:
        eng = model._engine(O.one_hot_bchw(xt, 2).to(U.DEV), image.to(U.DEV), None)
        kinds = [o["kind"] for o in eng.op_info]
        assert not model.f32_layers, sorted(model.f32_layers)
        if walk:       # the fused kernel's split path is what ran, not a range fallback
            assert kinds.count("norm_qkv_attention") == 11 and kinds.count("attention") == 0
        else:
            assert kinds.count("attention") == 11
