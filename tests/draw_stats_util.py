"""What test_draw_statistics shares: the statistics that hold observed frequencies and joint frequencies of the sampler's draws to the
float64 law of the operation, the float64 laws themselves (the step's posterior, the reverse walk's marginal), the patterns the frequency
tests draw from, and a numpy restatement of the recipe with knobs for the faults the negative controls put in.  Every statistic is a
z-score: under the law it is (close to) a standard normal, so a bar of 5 is a two-sided tail of 5.7e-7.  A plain module: no fixture, no
pytest setting."""
import math

import numpy as np

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import hip
from tests.guided_util import posterior64

BAR_GPU, BAR_CPU = 5.0, 4.0          # the device's draws; the restatement's (the margin for last-ulp near-ties where the two may differ)
MIN_EXPECTED = 50.0                  # a cell below this expectation is pooled
MAX_DROPPED = 1e-3                   # the share of the draws a pool that stays below it may hold


# ------------------------------------------------------------------------------------------------ the statistics
def _pooled(obs, exp):
    """Cells with expectation < MIN_EXPECTED pooled into one; a pool that is still below it joins the smallest cell that is left (a
    table, unlike a single class's score, loses nothing by that, and a histogram of a few thousand pixels has nothing to drop).
    Returns (observed, expected) of the cells that are left."""
    obs, exp = np.asarray(obs, dtype=np.float64).ravel(), np.asarray(exp, dtype=np.float64).ravel()
    small = exp < MIN_EXPECTED
    o, e = obs[~small], exp[~small]
    if small.any():
        po, pe = obs[small].sum(), exp[small].sum()
        if pe >= MIN_EXPECTED or len(e) == 0:
            o, e = np.append(o, po), np.append(e, pe)
        else:
            j = int(np.argmin(e))
            o[j], e[j] = o[j] + po, e[j] + pe
    return o, e


def cell_z(counts, n, p):
    """Per-class z-scores (count - n p) / sqrt(n p (1 - p)) of `counts` [K] of n draws.  p [K]: the law of every draw; p [n,K]: one law
    per draw (mean and variance summed over the draws).  Classes with expectation < 50 are pooled into one cell; a pool still below 50 is
    dropped (at most 1e-3 of n).  A cell without variance (p = 0 or 1 in float64) must hold its expectation exactly and scores 0."""
    counts, p = np.asarray(counts, dtype=np.float64), np.asarray(p, dtype=np.float64)
    assert abs(counts.sum() - n) < 0.5, (counts.sum(), n)
    mean, var = (n * p, n * p * (1 - p)) if p.ndim == 1 else (p.sum(0), (p * (1 - p)).sum(0))
    assert p.ndim == 1 or p.shape[0] == n
    small = mean < MIN_EXPECTED
    c, m, v = counts[~small], mean[~small], var[~small]
    if small.any():
        ps = p[small].sum() if p.ndim == 1 else p[:, small].sum(1)
        pm, pv = (n * ps, n * ps * (1 - ps)) if p.ndim == 1 else (ps.sum(), (ps * (1 - ps)).sum())
        if pm >= MIN_EXPECTED:
            c, m, v = np.append(c, counts[small].sum()), np.append(m, pm), np.append(v, pv)
        else:
            assert pm <= MAX_DROPPED * n, f"the dropped pool holds {pm / n:.2e} of the draws"
    flat = v <= 1e-9 * np.maximum(m, 1.0)
    assert (np.abs(c[flat] - m[flat]) < 0.5).all(), "a cell without variance is off its expectation"
    return np.where(flat, 0.0, (c - m) / np.sqrt(np.where(flat, 1.0, v)))


def own_cells(n, p):
    """How many classes of law p [K] cell_z scores on their own at n draws"""
    return int((n * np.asarray(p, dtype=np.float64) >= MIN_EXPECTED).sum())


def agreement_z(a, b, p, p_b=None):
    """z-score of the number of positions where the class maps a and b agree.  p [...,K] (broadcast against the maps): the law of a, and of
    b unless p_b is given.  Under independence a pixel agrees with probability m = sum_k p_k p_b_k; mean and variance m (1 - m) are summed
    over the pixels.  Identical maps of uniform K = 16 rows of n pixels score sqrt(15 n)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    p = np.asarray(p, dtype=np.float64)
    m = np.broadcast_to((p * (p if p_b is None else np.asarray(p_b, dtype=np.float64))).sum(-1), a.shape)
    return float(((a == b).sum() - m.sum()) / math.sqrt((m * (1 - m)).sum()))


def wilson_hilferty(chi2, dof):
    """A chi-square value on dof degrees of freedom as a z-score (Wilson & Hilferty 1931: (chi2 / dof)^(1/3) is close to normal)"""
    s = 2.0 / (9.0 * dof)
    return float(((chi2 / dof) ** (1.0 / 3.0) - (1.0 - s)) / math.sqrt(s))


def chi2_z(obs, exp):
    """Pearson's chi-square of observed against expected counts (laws known, nothing estimated: cells - 1 degrees of freedom), cells
    pooled to expectation >= 50, as a z-score.  One cell left (a law without spread): 0 if it holds every draw that is expected there."""
    o, e = _pooled(obs, exp)
    if len(o) < 2:
        assert len(o) == 1 and abs(o[0] - e[0]) < 0.5, (o, e)
        return 0.0
    return wilson_hilferty(float(((o - e) ** 2 / e).sum()), len(o) - 1)


def pair_table_z(x, y, joint):
    """z-score of the K x K table of the pairs (x_i, y_i) against n * joint; joint [K,K]: the law of a pair (np.outer(px, py) under
    independence)."""
    x, y, joint = np.asarray(x).ravel(), np.asarray(y).ravel(), np.asarray(joint, dtype=np.float64)
    K = joint.shape[0]
    table = np.bincount(x.astype(np.int64) * K + y.astype(np.int64), minlength=K * K)
    return chi2_z(table, x.size * joint.ravel())


def binomial_hist_z(counts_per_pixel, S, pi):
    """z-score of the histogram of per-pixel counts (how many of S passes drew the class) against Binomial(S, pi); pi: one value, or one
    per pixel (the expected histogram is then the sum of the pixels' laws).  Passes that share their noise pile the histogram up at 0 and
    S."""
    c = np.asarray(counts_per_pixel).ravel().astype(np.int64)
    pi = np.broadcast_to(np.asarray(pi, dtype=np.float64).ravel(), c.shape)
    j = np.arange(S + 1)
    choose = np.array([math.comb(S, int(i)) for i in j], dtype=np.float64)
    vals, weight = np.unique(pi, return_counts=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        pmf = choose[None] * np.where(j[None] == 0, 1.0, vals[:, None] ** j[None]) * np.where(j[None] == S, 1.0, (1 - vals[:, None]) ** (S - j[None]))
    return chi2_z(np.bincount(c, minlength=S + 1), (pmf * weight[:, None]).sum(0))


# ------------------------------------------------------------------------------------------------ the laws, in float64
def softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def step_law64(x0, xt, a, c):
    """The law of the class a reverse step draws (include/ccdm_hip.h): the posterior of x0 rows [...,K] (any positive scale) given x_t
    [...] in float64 with the fp32 coefficients the step is handed, clamped at 1e-12, normalised."""
    x0 = np.asarray(x0, dtype=np.float64)
    lead = x0.shape[:-1]
    p = posterior64(x0.reshape(1, -1, x0.shape[-1]), np.asarray(xt).reshape(1, -1), a, c)[0]
    p = np.maximum(p, 1e-12)
    return (p / p.sum(-1, keepdims=True)).reshape(lead + (x0.shape[-1],))


def race_law64(own, K, c):
    """The law of the two-valued race (clamp, renoise, the bound's noising): c onehot(own) + (1 - c) / K, from the fp32 pair the host hands
    the kernel.  own [...] -> [...,K]"""
    p_miss = (1.0 - float(c)) / K
    p_hit, p_miss = float(np.float32(float(c) + p_miss)), float(np.float32(p_miss))
    p = np.where(np.arange(K) == np.asarray(own)[..., None], p_hit, p_miss)
    return p / p.sum(-1, keepdims=True)


def chain_matrix64(q, K, rows):
    """M[x_T, x] = P(the walk over `rows`, in walking order, ends in class x | it starts in x_T), when the network's x0 is q [K] at every
    step: the product of the K x K transition matrices.  A row (a, c, mode) is a reverse step, its matrix step_law64's; with
    STEP_LAST_MAJORITY it maps every state to the argmax of its posterior (first maximum), with STEP_LAST_KEEP it keeps the state.  A row
    ("renoise", p_stay, p_move) is a resampling jump's way back up: p_stay on the diagonal, p_move elsewhere, normalised."""
    q = np.asarray(q, dtype=np.float64)
    M = np.eye(K)
    for row in rows:
        if row[0] == "renoise":
            step = np.where(np.eye(K, dtype=bool), float(row[1]), float(row[2]))
            step = step / step.sum(-1, keepdims=True)
        else:
            a, c, mode = row
            step = step_law64(np.broadcast_to(q, (K, K)), np.arange(K), a, c)          # [x_t, x_{t-1}]
            if mode == hip.STEP_LAST_MAJORITY:
                step = np.eye(K)[step.argmax(-1)]
            elif mode == hip.STEP_LAST_KEEP:
                step = np.eye(K)
            else:
                assert mode == hip.STEP_SAMPLE, mode
        M = M @ step
    return M


def chain_law64(q, K, rows):
    """The float64 marginal of the reverse walk from a uniform x_T"""
    return np.full(K, 1.0 / K) @ chain_matrix64(q, K, rows)


# ------------------------------------------------------------------------------------------------ what the frequency tests draw from
R_PATTERNS = 8          # interleaved over the pixels as pixel % 8, so kernels that stage rows in LDS mix them within a block


def epilogue_patterns(K):
    """Eight (x0 row, x_t) patterns of K classes: near-uniform rows, rows with 0.99 on one class (the last class: past the first Philox
    block for K > 4; class 0 with x_t elsewhere), a row with a class at 1e-3, a geometric row and random ones.  Returns x0 fp32 [8,K]
    (rows sum to 1 up to fp32 rounding) and x_t int64 [8]."""
    rng = np.random.default_rng(1300 + K)
    last = K - 1

    def peaked(k):
        row = np.full(K, 0.01 / max(K - 1, 1))
        row[k] = 0.99
        return row
    rare = rng.random(K) + 0.5
    rare_k = min(5, last)
    rare[rare_k] = 0.0
    rare = rare / rare.sum() * (1 - 1e-3)
    rare[rare_k] = 1e-3
    geo = 0.8 ** (np.arange(K) % 24)
    rows = [1.0 + 0.2 * rng.random(K), 1.0 + 0.2 * rng.random(K), peaked(last), peaked(0), rare, rng.random(K) + 0.05, geo, rng.random(K) ** 3 + 0.01]
    x0 = np.stack([r / r.sum() for r in rows]).astype(np.float32)
    xt = np.array([0, last, last, 1 % K, rare_k, K // 2, 0, last], dtype=np.int64)
    return x0, xt


def tiled(rows, N, HW):
    """rows [8,...] -> [N,HW,...]: pattern pixel % 8 at every pixel of every sample"""
    rows = np.asarray(rows)
    return np.ascontiguousarray(np.broadcast_to(rows[np.arange(HW) % R_PATTERNS][None], (N, HW) + rows.shape[1:]))


def pattern_counts(idx, K):
    """idx [N,HW] classes -> counts [8,K] per pattern (pixel % 8), every sample counted"""
    idx = np.asarray(idx).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < K, "a drawn class outside [0, K)"
    pat = np.broadcast_to(np.arange(idx.shape[1]) % R_PATTERNS, idx.shape)
    return np.bincount((pat * K + idx).ravel(), minlength=R_PATTERNS * K).reshape(R_PATTERNS, K)


def pattern_z(idx, laws):
    """cell_z of every pattern's counts against its law; laws [8,K].  Returns the z-scores of all cells, concatenated."""
    K = laws.shape[1]
    counts = pattern_counts(idx, K)
    return np.concatenate([cell_z(counts[r], int(counts[r].sum()), laws[r]) for r in range(R_PATTERNS)])


def worst(z):
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    return float(np.abs(z).max()) if z.size else 0.0


# ------------------------------------------------------------------------------------------------ the recipe, with knobs for faults
def exponentials(seed, row, sample0, n, hw, k, *, tag=0, word_mod=4, power=1.0, pix0=0):
    """O.philox_exponential's recipe — counter (pixel, sample0 + n, row, tag | k // 4), word k % 4, U = (bits >> 8 + 0.5) 2^-24,
    E = -log U in fp32 — for the pixels pix0 .. pix0 + hw - 1, every Philox block evaluated once, with the knobs of the negative
    controls: word k % word_mod in place of k % 4, E ** power in place of E."""
    pix = (np.arange(hw, dtype=np.uint32) + np.uint32(pix0))[None, :, None]
    smp = (np.arange(n, dtype=np.uint32) + np.uint32(sample0 & 0xFFFFFFFF))[:, None, None]
    kq = (np.uint32(tag) | np.arange((k + 3) // 4, dtype=np.uint32))[None, None, :]
    ctr = np.stack(np.broadcast_arrays(pix, smp, np.uint32(row), kq), axis=-1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    blk = O.philox4x32_10(ctr, key)                                                  # [n,hw,blocks,4]
    word = blk[:, :, np.arange(k) // 4, np.arange(k) % word_mod]
    u = ((word >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    e = (-np.log(u)).astype(np.float32)
    return e if power == 1.0 else np.power(e, np.float32(power)).astype(np.float32)


def race(p, e):
    """argmax_k p_k / E_k in fp32, the first maximum wins.  p broadcast against e [n,hw,k]."""
    with np.errstate(divide="ignore"):
        return np.argmax(np.asarray(p, dtype=np.float32) / e, axis=-1).astype(np.int64)


def restated_draw(rows, seed, row, sample0, n, hw, chunk=2 ** 15, **knobs):
    """The restatement's draw on the unguided step's counters from the patterns' rows [8,K] (pattern pixel % 8 at every pixel of every
    sample) or from one row [K], in chunks of pixels."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.empty((n, hw), dtype=np.int64)
    for lo in range(0, hw, chunk):
        m = min(chunk, hw - lo)
        p = rows[(lo + np.arange(m)) % R_PATTERNS][None] if rows.ndim == 2 else rows
        out[:, lo:lo + m] = race(p, exponentials(seed, row, sample0, n, m, rows.shape[-1], pix0=lo, **knobs))
    return out
