"""The sampler's draws held to their law.  Every other test of the sampling path compares a kernel with a restatement of the same recipe
(the Philox counter layout, bits -> U -> -log U, argmax p_k / E_k); such a mirror cannot show that the recipe draws from the distribution
it claims to, or that two draws meant to be independent are.  These tests compare observed frequencies and joint frequencies of the
device's draws with the float64 law of the operation (include/ccdm_hip.h), and the agreement of maps from streams that must not meet with
what independence gives.  The statistics are z-scores (draw_stats_util): the device's must stay within 5 (a two-sided tail of 5.7e-7 per
statistic, about 1e-3 over the file), the restatement's, on the CPU at the same seeds, within 4; negative controls show that each
statistic sees the fault it is for."""
import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import hip, serving
from ccdm_stochastic_segmentation_amd.models import pass_key
from tests import draw_stats_util as D
from tests import guided_util as GU
from tests import hip_util as HU
from tests import sampler_util as SU
from tests import test_known_labels as TK
from tests import test_label_bound as TB
from tests import test_queue_guided as TG
from tests import test_resample_jumps as TR
from tests import test_sampling_queue as TQ
from tests import test_tiled_sampling as TT
from tests import test_view_sampling as TV

SEED, FREE = SU.SEED, SU.FREE
BAR, BAR_CPU = D.BAR_GPU, D.BAR_CPU
# the table rows of the frequency tests: both ends and the middle of a T = 250 cosine schedule, at the row a full walk has them in
EPI_ROWS = {249: 1, 100: 150, 2: 248}
EPI_KS, EPI_MANY_KS = (2, 3, 5, 20, 33, 64), (5, 33, 128)
EPI_CASES = [(K, False) for K in EPI_KS] + [(K, True) for K in EPI_MANY_KS]
EPI_OFFSET = 3
TAIL_PS = (2.0 ** -4, 2.0 ** -7, 2.0 ** -10)
RACE_KS = (2, 5, 20)
SHAPED_KS = (2, 5, 20, 33)
# (entry, tau, r, evidence): the evidence step; the extremes of the temperature; a truncation; everything at once
SHAPED_CASES = [("ccdm_evidence_step", 1.0, 1.0, True), ("ccdm_shaped_step", 0.25, 1.0, False), ("ccdm_shaped_step", 4.0, 1.0, False),
                ("ccdm_shaped_step", 1.0, 0.5, False), ("ccdm_shaped_step", 0.7, 0.9, True)]
IND_K, IND_N, IND_HW, IND_ROW, IND_OFFSET = 16, 2, 2 ** 14, 3, 5


def coefficients(t):
    a, c = GU.coefficients(t)
    return float(np.float32(a)), float(np.float32(c))


def cumalpha(t, T=250):
    from oracle import ccdm_oracle as O
    return float(O.make_schedule("cosine", T, {"s": 0.008})[2].double()[t - 1])


def epilogue_case(K, softmax):
    """The head rows of the patterns (logits = log x0 with the softmax, x0 without) in fp32, and the float64 x0 they stand for"""
    x0, xt = D.epilogue_patterns(K)
    head = np.log(x0).astype(np.float32) if softmax else x0
    return head, (D.softmax64(head) if softmax else head.astype(np.float64)), xt


def pattern_evidence(K):
    """Weights [8,K] in [0.05,1], a fifth of them exactly 0, never the row's largest class"""
    rng = np.random.default_rng(1700 + K)
    ev = rng.uniform(0.05, 1.0, (D.R_PATTERNS, K)).astype(np.float32)
    zero = rng.random((D.R_PATTERNS, K)) < 0.2
    zero[np.arange(D.R_PATTERNS), D.epilogue_patterns(K)[0].argmax(-1)] = False
    ev[zero] = 0.0
    return ev


def shaped_laws(x0, ev, xt, tau, r, a, c):
    """The float64 law of the reweighted, tempered, truncated row, per pattern.  The truncation must sit far from every prefix mass: 1e-4
    of the threshold, some thirty times what the kernel's fp32 power (guided_util.POWER_ERROR_ALLOWED) and prefix sums (K 2^-24) can move
    one, so kernel and law keep the same classes."""
    inv = float(np.float32(1.0 / tau))
    v = GU.weighted(x0, ev)
    if r != 1.0:
        assert GU.threshold_margin64(GU.shape_rows(v, inv, 1.0, np.float64), r).min() > 1e-4, "a prefix mass next to the threshold"
    return inv, D.step_law64(GU.shape_rows(v, inv, float(np.float32(r)), np.float64), xt, a, c)


# ================================================================================================ 0. the helpers, on the CPU
def test_cell_z_pools_and_drops():
    """Cells below expectation 50 are pooled; a pool still below 50 is dropped if it holds at most 1e-3 of the draws, and refused if
    more; a law per draw sums mean and variance over the draws; exact counts score 0 and a shifted cell its shift in sigmas."""
    n = 100000
    p = np.array([0.5, 0.3, 0.1997, 0.0002, 0.0001])
    z = D.cell_z(n * p, n, p)
    assert z.shape == (3,) and np.abs(z).max() < 1e-9                                                    # 30 expected in the pool: dropped
    p2 = np.array([0.5, 0.3, 0.199, 0.0004, 0.0003, 0.0003])
    assert D.cell_z(n * p2, n, p2).shape == (4,) and D.own_cells(n, p2) == 3                                # 100 expected in the pool: kept
    shifted = n * p + np.array([300, -300, 0, 0, 0])
    np.testing.assert_allclose(D.cell_z(shifted, n, p)[:2], [300 / np.sqrt(n * 0.25), -300 / np.sqrt(n * 0.21)])
    with pytest.raises(AssertionError, match="dropped pool"):
        D.cell_z(np.array([960, 40]), 1000, np.array([0.96, 0.04]))
    per_draw = np.broadcast_to(p, (n, 5))
    np.testing.assert_allclose(D.cell_z(shifted, n, per_draw), D.cell_z(shifted, n, p), atol=1e-9)
    assert D.cell_z(np.array([n, 0]), n, np.array([1.0, 0.0])).tolist() == [0.0]                           # a law without spread
    with pytest.raises(AssertionError, match="without variance"):
        D.cell_z(np.array([n - 1, 1]), n, np.array([1.0, 0.0]))


def test_statistics_are_standard_normal_under_the_law_and_large_off_it():
    """numpy's own generator in the sampler's place: every statistic of independent draws from the law stays within 4, identical maps
    score sqrt(15 n) at uniform K = 16, a pair table of dependent pairs and a histogram of repeated passes are far out, and
    Wilson-Hilferty maps the chi-square's mean to (nearly) 0."""
    rng = np.random.default_rng(5)
    K, n = 16, 2 ** 15
    p = np.full(K, 1.0 / K)
    a, b = rng.integers(0, K, n), rng.integers(0, K, n)
    assert abs(D.agreement_z(a, b, p)) < BAR_CPU and abs(D.pair_table_z(a, b, np.outer(p, p))) < BAR_CPU
    np.testing.assert_allclose(D.agreement_z(a, a, p), np.sqrt(15 * n))
    assert D.pair_table_z(a, (a + (b < 2)) % K, np.outer(p, p)) > 50
    # P(chi2 on 2 degrees of freedom > x) = exp(-x / 2): the 3-sigma and 5-sigma upper tails, where the approximation is at its worst
    assert abs(D.wilson_hilferty(255.0, 255)) < 0.05
    assert 2.8 < D.wilson_hilferty(-2 * np.log(1.35e-3), 2) < 3.2 and 4.6 < D.wilson_hilferty(-2 * np.log(2.87e-7), 2) < 5.4
    law = np.array([0.7, 0.2, 0.1])
    rows = rng.random((n, 3)) + 0.1
    rows /= rows.sum(1, keepdims=True)
    draws = (rng.random(n)[:, None] > np.cumsum(rows, 1)).sum(1)
    assert D.worst(D.cell_z(np.bincount(draws, minlength=3), n, rows)) < BAR_CPU                            # one law per draw
    assert D.worst(D.cell_z(np.bincount(draws, minlength=3), n, law)) > 50                                  # ... and not another one
    S = 16
    counts = rng.binomial(S, 0.3, n)
    assert abs(D.binomial_hist_z(counts, S, 0.3)) < BAR_CPU and D.binomial_hist_z(counts, S, 0.31) > BAR
    pi = np.where(np.arange(n) % 2 == 0, 0.3, 0.05)
    assert abs(D.binomial_hist_z(rng.binomial(S, pi), S, pi)) < BAR_CPU
    assert D.binomial_hist_z(S * rng.binomial(1, 0.3, n), S, 0.3) > 100                                    # every pass repeats the first
    assert D.binomial_hist_z(np.full(n, S), S, 1.0) == 0.0                                                  # a law without spread


def test_chain_law_is_the_product_of_the_steps():
    """chain_law64 against a brute-force sum over all paths of a three-row walk at K = 3; a last row at t = 1 (a = 0, c = 1) has the
    posterior x0 itself, so a majority vote there returns argmax x0 whatever came before, and STEP_LAST_KEEP returns the state the row
    before drew."""
    K = 3
    q = np.array([0.2, 0.5, 0.3])
    rows = [(0.9, 0.3, hip.STEP_SAMPLE), (0.95, 0.6, hip.STEP_SAMPLE), (0.97, 0.9, hip.STEP_SAMPLE)]
    steps = [D.step_law64(np.broadcast_to(q, (K, K)), np.arange(K), a, c) for a, c, _ in rows]
    want = np.zeros(K)
    for x3 in range(K):
        for x2 in range(K):
            for x1 in range(K):
                for x0 in range(K):
                    want[x0] += steps[0][x3, x2] * steps[1][x2, x1] * steps[2][x1, x0] / K
    np.testing.assert_allclose(D.chain_law64(q, K, rows), want, rtol=1e-13)
    np.testing.assert_allclose(D.chain_matrix64(q, K, rows).sum(1), 1.0, rtol=1e-13)
    np.testing.assert_allclose(D.step_law64(q, 2, 0.0, 1.0), q, rtol=1e-13)
    assert D.chain_law64(q, K, rows + [(0.0, 1.0, hip.STEP_LAST_MAJORITY)]).tolist() == [0.0, 1.0, 0.0]
    np.testing.assert_allclose(D.chain_law64(q, K, rows + [(0.0, 1.0, hip.STEP_LAST_KEEP)]), want, rtol=1e-13)
    # the step law is Bayes' rule: q(x_{t-1} | x_t, x_0) summed over x_0 ~ q, here at K = 2 by hand
    a, c, p0 = 0.8, 0.4, 0.25
    A = np.array([a + (1 - a) / 2, (1 - a) / 2])                                   # q(x_t = 0 | x_{t-1} = k)
    post = []
    for d, pd in enumerate((p0, 1 - p0)):
        B = np.where(np.arange(2) == d, c + (1 - c) / 2, (1 - c) / 2)               # q(x_{t-1} = k | x_0 = d)
        post.append(pd * A * B / (A * B).sum())
    np.testing.assert_allclose(D.step_law64(np.array([p0, 1 - p0]), 0, a, c), np.sum(post, 0), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ the restatement at the GPU tests' seeds
CPU_N, CPU_HW = 4, 2 ** 17          # 2^16 draws a pattern


def test_the_chunked_recipe_is_the_oracles_stream():
    """draw_stats_util.exponentials (every Philox block evaluated once, pixels in chunks) is O.philox_exponential bit for bit, and under a
    tag it is the stream sampler_util.race_restatement draws from"""
    from oracle import ccdm_oracle as O
    for K in (2, 5, 33):
        want = O.philox_exponential(SEED, 9, EPI_OFFSET, 2, 100, K)
        got = np.concatenate([D.exponentials(SEED, 9, EPI_OFFSET, 2, 60, K), D.exponentials(SEED, 9, EPI_OFFSET, 2, 40, K, pix0=60)], 1)
        assert (GU.bits(want) == GU.bits(got)).all()
    own = np.broadcast_to(race_patterns(5)[np.arange(64) % 8] % 5, (2, 64))
    p_hit, p_miss = SU.probabilities(0.3, 5)
    rows = np.where(np.arange(5) == (race_patterns(5) % 5)[:, None], p_hit, p_miss)
    assert (D.restated_draw(rows, SEED, 9, EPI_OFFSET, 2, 64, chunk=24, tag=SU.TAG_CLAMP)
            == SU.race_restatement(own, 5, 0.3, 9, SEED, EPI_OFFSET, SU.TAG_CLAMP)).all()


@pytest.mark.parametrize("K", EPI_KS + (128,))
def test_restated_epilogue_follows_the_float64_law(K):
    """The restatement (guided_util.evidence_restatement's fp32 posterior of the patterns, raced on O.philox_exponential's stream) at the
    frequency tests' patterns, seed, rows and sample offset, 2^16 draws a pattern: every class's z-score within 4.  K > 33: one row (the
    cost is the numpy Philox)."""
    head, q, xt = epilogue_case(K, False)
    worst = 0.0
    for t, row in EPI_ROWS.items():
        if K > 33 and t != 100:
            continue
        a, c = coefficients(t)
        p_hat, _ = GU.evidence_restatement(head[None], np.ones_like(head[None]), xt[None], a, c, hip.STEP_SAMPLE, row, SEED, EPI_OFFSET)
        idx = D.restated_draw(p_hat[0], SEED, row, EPI_OFFSET, CPU_N, CPU_HW)
        worst = max(worst, D.worst(D.pattern_z(idx, D.step_law64(q, xt, a, c))))
    print(f"K={K}: largest |z| {worst:.2f}")
    assert worst <= BAR_CPU


def tail_patterns(p):
    """(class that holds p, x_t) four times over, twice: x0 [8,2], x_t [8]"""
    x0 = np.array([[p, 1 - p], [p, 1 - p], [1 - p, p], [1 - p, p]] * 2, dtype=np.float32)
    return x0, np.array([0, 1, 0, 1] * 2, dtype=np.int64)


def tail_z(idx, x0):
    """The four patterns' counts (each in two of the eight interleaved slots) against their laws: at a = 0, c = 1 the law is x0"""
    counts = D.pattern_counts(idx, 2)
    counts = counts[:4] + counts[4:]
    return np.concatenate([D.cell_z(counts[r], int(counts[r].sum()), x0[r].astype(np.float64) / x0[r].astype(np.float64).sum()) for r in range(4)])


@pytest.mark.parametrize("p", TAIL_PS)
def test_restated_race_tails(p):
    """K = 2 with p = 2^-4, 2^-7, 2^-10 on either class: the rare class wins when its E is small or the other's is large, so this is
    the view of both tails of -log U.  2^17 draws a pattern here (2^19 on the device)."""
    x0, xt = tail_patterns(p)
    N, HW = 4, 2 ** 17
    idx = D.restated_draw(x0, SEED, 7, EPI_OFFSET, N, HW)
    z = tail_z(idx, x0)
    print(f"p={p}: largest |z| {D.worst(z):.2f}")
    assert D.worst(z) <= BAR_CPU


def race_patterns(K):
    """The own class of the two-valued race per pattern; FREE at three of them (the clamp's free pixels)"""
    return np.array([0, K - 1, FREE, 1 % K, FREE, K // 2, 0, FREE], dtype=np.int64)


@pytest.mark.parametrize("K", RACE_KS)
def test_restated_two_valued_race_follows_its_law(K):
    """sampler_util.race_restatement under the clamp's and the renoise's tag at c = cumalpha of t = 249, 100, 2"""
    own = np.where(race_patterns(K) == FREE, 2 % K, race_patterns(K))
    worst = 0.0
    for t, row in EPI_ROWS.items():
        c = cumalpha(t)
        p_hit, p_miss = SU.probabilities(c, K)
        rows = np.where(np.arange(K) == own[:, None], p_hit, p_miss)
        for tag in (SU.TAG_CLAMP, SU.TAG_RENOISE):
            idx = D.restated_draw(rows, SEED, row, EPI_OFFSET, CPU_N, CPU_HW, tag=tag)
            worst = max(worst, D.worst(D.pattern_z(idx, D.race_law64(own, K, c))))
    print(f"K={K}: largest |z| {worst:.2f}")
    assert worst <= BAR_CPU


@pytest.mark.parametrize("K", (5, 20))
def test_restated_shaped_step_follows_the_float64_law(K):
    """guided_util.shaped_restatement on the shaped frequency test's patterns against the float64 law of the shaped row"""
    x0, xt = D.epilogue_patterns(K)
    ev = pattern_evidence(K)
    a, c = coefficients(100)
    worst = 0.0
    for _, tau, r, with_ev in SHAPED_CASES:
        e = ev if with_ev else None
        inv, laws = shaped_laws(x0, e, xt, tau, r, a, c)
        p_hat, _ = GU.shaped_restatement(x0[None], None if e is None else e[None], xt[None], inv, r, a, c, hip.STEP_SAMPLE, EPI_ROWS[100], SEED,
                                         EPI_OFFSET)
        idx = D.restated_draw(p_hat[0], SEED, EPI_ROWS[100], EPI_OFFSET, CPU_N, CPU_HW)
        worst = max(worst, D.worst(D.pattern_z(idx, laws)))
    print(f"K={K}: largest |z| {worst:.2f}")
    assert worst <= BAR_CPU


def independence_scores(draw):
    """Every independence statistic of section 2 that one drawing function can give.  draw(row, seed, sample0, tag) -> class map
    [IND_N, IND_HW] of uniform K = 16 rows.  Returns {name: z}; maps that must be equal are asserted to be."""
    p = np.full(IND_K, 1.0 / IND_K)
    joint = np.outer(p, p)
    key = SEED
    base = draw(IND_ROW, key, IND_OFFSET, 0)
    z = {"row": D.agreement_z(base, draw(IND_ROW + 1, key, IND_OFFSET, 0), p),
         "seed": D.agreement_z(base, draw(IND_ROW, key + 1, IND_OFFSET, 0), p),
         "batch index": D.agreement_z(base[0], base[1], p),
         "pass key": D.agreement_z(draw(IND_ROW, pass_key(key, 0), IND_OFFSET, 0), draw(IND_ROW, pass_key(key, 1), IND_OFFSET, 0), p)}
    # pass 1 of call 0 against call 1 (call 0's key is the seed itself: one Weyl increment for calls and passes would make them one key)
    k0, k1 = model_keys(99)[:2]
    z["pass 1 of call 0 / call 1"] = D.agreement_z(draw(IND_ROW, pass_key(k0, 1), IND_OFFSET, 0), draw(IND_ROW, k1, IND_OFFSET, 0), p)
    shifted = draw(IND_ROW, key, IND_OFFSET + 1, 0)
    assert (shifted[0] == base[1]).all(), "sample_offset + 1, batch 0 is not sample_offset, batch 1"
    z["sample offset"] = D.agreement_z(base[0], shifted[0], p)
    tags = {"epilogue": 0, "clamp": SU.TAG_CLAMP, "renoise": SU.TAG_RENOISE, "bound": TB.TAG_BOUND}
    maps = {name: (base if tag == 0 else draw(IND_ROW, key, IND_OFFSET, tag)) for name, tag in tags.items()}
    names = list(tags)
    for i, m in enumerate(names):
        for n in names[i + 1:]:
            z[f"{m} / {n}"] = D.agreement_z(maps[m], maps[n], p)
    z["adjacent pixels"] = D.pair_table_z(base[:, 0::2], base[:, 1::2], joint)
    z["pixels HW/2 apart"] = D.pair_table_z(base[:, :IND_HW // 2], base[:, IND_HW // 2:], joint)
    return z


def model_keys(seed):
    """The Philox keys DenoisingModel hands out for calls 0, 1, 2 under `seed` (label_bound's come from the same function of its own
    counter)"""
    from ccdm_stochastic_segmentation_amd.models import DenoisingModel
    stub = type("M", (), {"philox_seed": seed, "philox_call": 0})()
    return [DenoisingModel._philox_key(stub, call) for call in range(3)]


def test_restated_streams_are_independent():
    """Rows, seeds, samples, passes, calls, tags and pixels on the restatement, uniform rows at K = 16 (expected agreement 1/16)"""
    def draw(row, seed, sample0, tag):
        return D.race(np.float32(1.0 / IND_K), D.exponentials(seed, row, sample0, IND_N, IND_HW, IND_K, tag=tag))
    z = independence_scores(draw)
    p = np.full(IND_K, 1.0 / IND_K)
    calls = [draw(IND_ROW, k, IND_OFFSET, 0) for k in model_keys(99)]
    for i in range(3):
        for j in range(i + 1, 3):
            z[f"call {i} / {j}"] = D.agreement_z(calls[i], calls[j], p)
    print({k: round(v, 2) for k, v in z.items()})
    assert D.worst(list(z.values())) <= BAR_CPU, z


def test_restated_two_step_walk_has_the_float64_joint():
    """K = 3: the class drawn at row r and the class drawn at row r + 1 given it, against the joint the step laws give"""
    z = two_step_z(lambda x0, xt, a, c, row: GU.evidence_restatement(x0, np.ones_like(x0), xt, a, c, hip.STEP_SAMPLE, row, SEED, IND_OFFSET)[1])
    print(f"largest |z| {z:.2f}")
    assert abs(z) <= BAR_CPU


def two_step_z(step):
    """step(x0 [N,HW,3] fp32, x_t [N,HW], a, c, row) -> drawn map.  x_T = 0 everywhere, x0 the same row everywhere."""
    K, N, HW = 3, 2, 2 ** 14
    row0 = np.array([0.2, 0.5, 0.3], dtype=np.float32)
    x0 = np.ascontiguousarray(np.broadcast_to(row0, (N, HW, K)))
    (a1, c1), (a2, c2) = coefficients(120), coefficients(119)
    x1 = step(x0, np.zeros((N, HW), dtype=np.int64), a1, c1, 130)
    x2 = step(x0, x1, a2, c2, 131)
    q = row0.astype(np.float64)
    joint = D.step_law64(q, 0, a1, c1)[:, None] * D.step_law64(np.broadcast_to(q, (K, K)), np.arange(K), a2, c2)
    return D.pair_table_z(x1, x2, joint)


# ------------------------------------------------------------------------------------------------ negative controls
def test_controls_shared_noise_is_seen():
    """The same noise for two table rows, two passes that share sample0, and the clamp's and the renoise's tag set to one value: the
    maps are equal, and agreement_z is sqrt(15 n) = 701 at n = 2^15 pixels where independence gives 0 +- 1."""
    p = np.full(IND_K, 1.0 / IND_K)

    def draw(row, sample0, tag):
        return D.race(np.float32(1.0 / IND_K), D.exponentials(SEED, row, sample0, IND_N, IND_HW, IND_K, tag=tag))
    for what, a, b in (("rows", draw(3, 5, 0), draw(3, 5, 0)), ("passes", draw(3, 5, 0), draw(3, 5, 0)),
                       ("tags", draw(3, 5, SU.TAG_CLAMP), draw(3, 5, SU.TAG_CLAMP))):
        assert D.agreement_z(a, b, p) > 700, what
    # the clamp and the renoise with one tag but different own classes: correlated, not equal — still far out
    c = 0.5
    own_a, own_b = np.zeros((IND_N, IND_HW), dtype=np.int64), np.ones((IND_N, IND_HW), dtype=np.int64)
    a = SU.race_restatement(own_a, IND_K, c, 3, SEED, 5, SU.TAG_CLAMP)
    b = SU.race_restatement(own_b, IND_K, c, 3, SEED, 5, SU.TAG_CLAMP)
    assert D.agreement_z(a, b, D.race_law64(own_a, IND_K, c), D.race_law64(own_b, IND_K, c)) > 100
    ok = SU.race_restatement(own_b, IND_K, c, 3, SEED, 5, SU.TAG_RENOISE)
    assert abs(D.agreement_z(a, ok, D.race_law64(own_a, IND_K, c), D.race_law64(own_b, IND_K, c))) <= BAR_CPU
    # half of the pixels shared: the pass histogram piles up, the pair table of two passes leaves the outer product
    half = np.where(np.arange(IND_HW) % 2 == 0, draw(3, 5, 0), draw(4, 5, 0))
    assert D.pair_table_z(draw(3, 5, 0), half, np.outer(p, p)) > 100
    S = 16
    fresh = np.stack([draw(3, 2 * s, 0)[0] == 0 for s in range(S)]).sum(0)
    stuck = np.stack([draw(3, 2 * (s // 2), 0)[0] == 0 for s in range(S)]).sum(0)           # passes 2j and 2j + 1 share sample0
    assert abs(D.binomial_hist_z(fresh, S, 1.0 / IND_K)) <= BAR_CPU and D.binomial_hist_z(stuck, S, 1.0 / IND_K) > 50


def test_control_wrong_word_is_seen():
    """Word k % 2 in place of k % 4: classes k and k + 2 of a Philox block share their E, the later one never wins a tie on equal p,
    and cell_z of a uniform K = 8 row is far out (measured: 98 at 2^16 draws)."""
    K, N, HW = 8, 4, 2 ** 14
    p = np.full(K, 1.0 / K)
    good = D.race(np.float32(1.0 / K), D.exponentials(SEED, 3, 0, N, HW, K))
    bad = D.race(np.float32(1.0 / K), D.exponentials(SEED, 3, 0, N, HW, K, word_mod=2))
    assert D.worst(D.cell_z(np.bincount(good.ravel(), minlength=K), N * HW, p)) <= BAR_CPU
    z = D.worst(D.cell_z(np.bincount(bad.ravel(), minlength=K), N * HW, p))
    print(f"largest |z| {z:.1f}")
    assert z > 50


def test_control_a_mildly_wrong_law_is_seen():
    """E ** 1.05 in place of E (a Weibull race): at K = 2, p = (1/16, 15/16) the rare class then wins with probability r / (1 + r),
    r = 15 ** (-1 / 1.05), = 0.0705 in place of 0.0625.  2^19 draws see it at z = 24 (measured: 24.1; by the same formula the exponent 1.02 would give 9.5);
    the true recipe on the same counters stays within 4."""
    N, HW = 4, 2 ** 17
    p = np.array([1.0 / 16, 15.0 / 16])
    score = {}
    for power in (1.0, 1.05):
        idx = D.restated_draw(p, SEED, 7, 0, N, HW, power=power)
        score[power] = D.cell_z(np.bincount(idx.ravel(), minlength=2), N * HW, p)[0]
    print(score)
    assert abs(score[1.0]) <= BAR_CPU and score[1.05] > 15


# ================================================================================================ 1. frequencies on the device
@pytest.fixture(scope="module")
def lib():
    return SU.load_lib()


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(SU.DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("K,many", EPI_CASES, ids=[f"K{K}-{'lds' if many else 'reg'}" for K, many in EPI_CASES])
def test_epilogue_frequencies_follow_the_float64_law(parity_log, K, many):
    """ccdm_posterior_sample, the register kernels and the LDS-row kernel: logits and probabilities, table rows t = 249, 100, 2 of a
    T = 250 cosine schedule, eight patterns interleaved over 4 x 2^17 pixels (2^16 draws a pattern).  At t = 249 and t = 2 every class of
    the near-uniform patterns is scored on its own, so a wrong counter word 3 or a wrong word of the block shows in the classes past the first block."""
    N, HW = 4, 2 ** 17
    worst = 0.0
    for softmax in (True, False):
        head, q, xt = epilogue_case(K, softmax)
        head_d, xt_d = torch.from_numpy(D.tiled(head, N, HW)).to(SU.DEV), dev_u8(D.tiled(xt, N, HW))
        for t, row in EPI_ROWS.items():
            a, c = coefficients(t)
            laws = D.step_law64(q, xt, a, c)
            if t != 100:          # (t = 100 holds most of the mass at x_t; at t = 249 the law is near uniform, at t = 2 near x0)
                assert D.own_cells(N * HW // D.R_PATTERNS, laws[0]) == K and D.own_cells(N * HW // D.R_PATTERNS, laws[1]) == K
            got = HU.posterior_sample(head_d, xt_d, a, c, hip.STEP_SAMPLE, softmax=softmax, philox_seed=SEED, sample_offset=EPI_OFFSET, step=row,
                                      many=many)
            z = D.worst(D.pattern_z(got["xt_next"].numpy(), laws))
            print(f"K={K} many={many} softmax={softmax} t={t}: largest |z| {z:.2f}")
            worst = max(worst, z)
    parity_log("draw_statistics_frequencies", **{f"epilogue_K{K}_{'lds' if many else 'reg'}": worst})
    assert worst <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("p", TAIL_PS)
def test_race_tails_on_the_device(parity_log, p):
    """K = 2, p = 2^-4, 2^-7, 2^-10 on either class under either x_t, 2^19 draws a pattern (a = 0, c = 1: the law is x0 itself)"""
    x0, xt = tail_patterns(p)
    N, HW = 4, 2 ** 19
    got = HU.posterior_sample(torch.from_numpy(D.tiled(x0, N, HW)).to(SU.DEV), dev_u8(D.tiled(xt, N, HW)), 0.0, 1.0, hip.STEP_SAMPLE, softmax=False,
                              philox_seed=SEED, sample_offset=EPI_OFFSET, step=7)
    z = D.worst(tail_z(got["xt_next"].numpy(), x0))
    parity_log("draw_statistics_frequencies", **{f"tail_p{p:.0e}": z})
    assert z <= BAR


@pytest.mark.gpu
def test_fused_head_frequencies_follow_the_float64_law(parity_log):
    """ccdm_head_posterior at 16 x 64 with conv weights of zero: the logits are the bias exactly (asserted), so the law needs no float64
    convolution.  128 samples: 2^16 draws per x_t."""
    rng = np.random.default_rng(2)
    N, Hh, Ww, Cc, K = 128, 16, 64, 32, 2
    x = HU.nhwc(torch.from_numpy((rng.standard_normal((N, Cc, Hh, Ww)) * 1.7 + 0.2).astype(np.float32)))
    gamma, beta = (1 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
    bias = np.array([0.4, -0.9], dtype=np.float32)
    xt = np.broadcast_to(np.arange(Hh * Ww) % 2, (N, Hh * Ww))
    worst = 0.0
    for t, row in EPI_ROWS.items():
        a, c = coefficients(t)
        got = HU.head_posterior(x, gamma, beta, np.zeros((K, Cc, 3, 3), np.float32), bias, dev_u8(xt), a, c, hip.STEP_SAMPLE, philox_seed=SEED,
                                sample_offset=EPI_OFFSET, step=row)
        assert (got["logits"].numpy() == bias).all() and got["flag"] == 0
        idx = got["xt_next"].numpy()
        for own in (0, 1):
            counts = np.bincount(idx[xt == own], minlength=K)
            worst = max(worst, D.worst(D.cell_z(counts, int(counts.sum()), D.step_law64(D.softmax64(bias), own, a, c))))
    parity_log("draw_statistics_frequencies", fused_head=worst)
    assert worst <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("K", RACE_KS)
def test_clamp_and_renoise_frequencies_follow_their_law(lib, parity_log, K):
    """ccdm_known_labels_step: known pixels follow (p_hit, p_miss) around the label, free pixels come back untouched;
    ccdm_renoise_step: every pixel follows (p_stay, p_move) around its class.  c = cumalpha of t = 249, 100, 2; 4 x 2^17 pixels, 2^16 draws a
    pattern (at 50000 draws or more a pool below 50 is below 1e-3 of them, so cell_z never has to refuse one)."""
    N, HW = 4, 2 ** 17
    known = D.tiled(race_patterns(K), N, HW)
    state = (np.arange(N * HW).reshape(N, HW) * 7 + 3) % K
    worst = 0.0
    for t, row in EPI_ROWS.items():
        c = cumalpha(t)
        got = TK.run_kernel(lib, torch.from_numpy(known.astype(np.uint8)), torch.from_numpy(state.astype(np.uint8)), K, c, hip.STEP_SAMPLE,
                            step_row=row, seed=SEED, sample_offset=EPI_OFFSET)["xt"].numpy().astype(np.int64)
        free = known == FREE
        assert (got[free] == state[free]).all(), "a free pixel was changed"
        laws = D.race_law64(np.where(race_patterns(K) == FREE, 0, race_patterns(K)), K, c)
        counts = D.pattern_counts(np.where(free, 0, got), K)
        z = [D.cell_z(counts[r], int(counts[r].sum()), laws[r]) for r in range(D.R_PATTERNS) if race_patterns(K)[r] != FREE]
        own = np.where(race_patterns(K) == FREE, 2 % K, race_patterns(K))
        new, _ = TR.run_renoise(lib, D.tiled(own, N, HW), K, c, step_row=row, seed=SEED, sample_offset=EPI_OFFSET)
        worst = max(worst, D.worst(np.concatenate(z)), D.worst(D.pattern_z(new, D.race_law64(own, K, c))))
    parity_log("draw_statistics_frequencies", **{f"clamp_renoise_K{K}": worst})
    assert worst <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("K", (2, 20))
def test_bound_noise_frequencies_follow_the_forward_law(lib, parity_log, K):
    """ccdm_bound_noise: x_t ~ Cat(cumalpha_t onehot(y) + (1 - cumalpha_t) / K) per table row, t = 1 .. 6 of the 6-level schedule on two
    label maps, 2^14 pixels a row; pixels that are not counted come back as pixel % K."""
    dm = TB.diffusion(K)
    HW = 2 ** 14
    labels = np.stack([np.arange(HW) % K, (np.arange(HW) * 3 + 1) % K]).astype(np.uint8)
    labels[:, 5::64] = 255
    spec = [(t, 10 + t, t % 2) for t in range(1, TB.T_K + 1)]
    tab = TB.make_table(dm, K, spec)
    N = len(spec)
    out = torch.full((N * HW,), 255, dtype=torch.uint8, device=SU.DEV)
    labels_d, tab_d = TB.dev(labels), TB.table_dev(tab)
    hip.check(lib.ccdm_bound_noise(labels_d.data_ptr(), tab_d.data_ptr(), N, 2, HW, K, SEED, out.data_ptr(), TB.stream()), "bound_noise")
    got = out.cpu().numpy().reshape(N, HW).astype(np.int64)
    worst = 0.0
    for n, (t, _, lr) in enumerate(spec):
        y = labels[lr].astype(np.int64)
        counted = y < K
        assert (got[n][~counted] == np.arange(HW)[~counted] % K).all()
        laws = D.race_law64(y[counted], K, float(dm.cumalphas.double()[t - 1]))
        counts = np.bincount(got[n][counted], minlength=K)
        # per label class as well: the draw relative to the label, (y - x) mod K, has the law of label 0
        rel = np.bincount((got[n][counted] - y[counted]) % K, minlength=K)
        worst = max(worst, D.worst(D.cell_z(counts, int(counted.sum()), laws)),
                    D.worst(D.cell_z(rel, int(counted.sum()), D.race_law64(0, K, float(dm.cumalphas.double()[t - 1])))))
    parity_log("draw_statistics_frequencies", **{f"bound_noise_K{K}": worst})
    assert worst <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("K", SHAPED_KS)
def test_evidence_and_shaped_frequencies_follow_the_float64_law(lib, parity_log, K):
    """ccdm_evidence_step and ccdm_shaped_step: the law of the reweighted, tempered (tau = 0.25, 4), truncated (r = 0.5; every prefix mass
    at least 1e-4 from the threshold) row, t = 100 and 2, 4 x 2^17 pixels (2^16 draws a pattern)"""
    N, HW = 4, 2 ** 17
    x0, xt = D.epilogue_patterns(K)
    ev = pattern_evidence(K)
    worst = 0.0
    for symbol, tau, r, with_ev in SHAPED_CASES:
        e = ev if with_ev else None
        for t in (100, 2):
            a, c = coefficients(t)
            inv, laws = shaped_laws(x0, e, xt, tau, r, a, c)
            got = GU.run_shaped_kernel(lib, D.tiled(x0, N, HW), None if e is None else D.tiled(e, N, HW), D.tiled(xt, N, HW), inv, r, a, c,
                                       hip.STEP_SAMPLE, step_row=EPI_ROWS[t], seed=SEED, sample_offset=EPI_OFFSET, symbol=symbol)
            z = D.worst(D.pattern_z(got["xt"], laws))
            print(f"K={K} {symbol} tau={tau} r={r} ev={with_ev} t={t}: largest |z| {z:.2f}")
            worst = max(worst, z)
    parity_log("draw_statistics_frequencies", **{f"evidence_shaped_K{K}": worst})
    assert worst <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("flips", [(TV.HFLIP,), (TV.HFLIP, TV.VFLIP, TV.HVFLIP)], ids=["V2", "V4"])
def test_view_mean_frequencies_follow_the_float64_law(lib, parity_log, flips):
    """ccdm_views_step: view v holds pattern (pixel + v) % 8 at its mirrored pixel, so the drawn class follows the float64 mean of V
    different rows; every view comes back with the same class at its mirrored pixel.  K = 5, 8 x 256 x 256 (2^16 draws a pattern)."""
    N, Hh, Ww, K = 8, 256, 256, 5
    HW, V = Hh * Ww, 1 + len(flips)
    x0, xt = D.epilogue_patterns(K)
    per_view = [np.roll(x0, -v, axis=0) for v in range(V)]
    x0v = np.concatenate([TV.mirrored_rows(D.tiled(per_view[v], N, HW), N, Hh, Ww, (f,))[N:] if v else D.tiled(per_view[0], N, HW)
                          for v, f in enumerate((0,) + tuple(flips))], 0)
    xtv = TV.scatter_views(D.tiled(xt, N, HW), N, Hh, Ww, flips)
    mean = np.mean(np.stack(per_view).astype(np.float64), axis=0)
    worst = 0.0
    for t in (100, 2):
        a, c = coefficients(t)
        got = TV.run_kernel(lib, x0v, None, xtv, N, Hh, Ww, flips, 1.0, 1.0, a, c, hip.STEP_SAMPLE, step_row=EPI_ROWS[t], seed=SEED,
                            sample_offset=EPI_OFFSET)["xt"].astype(np.int64)
        assert (got == TV.scatter_views(got[:N], N, Hh, Ww, flips)).all(), "a view does not hold view 0's class at its mirrored pixel"
        worst = max(worst, D.worst(D.pattern_z(got[:N], D.step_law64(mean, xt, a, c))))
    parity_log("draw_statistics_frequencies", **{f"views_V{V}": worst})
    assert worst <= BAR


@pytest.mark.gpu
def test_tile_mean_frequencies_follow_the_float64_law(lib, parity_log):
    """ccdm_tiled_step: a 256 x 256 canvas under two overlapping 192 x 192 tiles per axis; tile r holds pattern (pixel + r) % 8, so the law
    is the float64 tile mean (of 2 or 4 different rows) where tiles overlap and the single tile's row elsewhere.  Overlap and non-overlap
    pixels are counted separately (2^16 draws under a single tile).  K = 5, N = 4."""
    N, K = 4, 5
    geom = (256, 256, 192, 192, 64, 64)
    HWc = geom[0] * geom[1]
    where, cover = TT.tile_pixels(geom), TT.cover_count(geom)
    assert len(where) == 4 and sorted(set(cover.tolist())) == [1, 2, 4]
    x0, xt = D.epilogue_patterns(K)
    x0t = np.concatenate([D.tiled(np.roll(x0, -r, axis=0), N, HWc)[:, pix] for r, pix in enumerate(where)], 0)
    cxt = D.tiled(xt, N, HWc)
    mean = TT.tile_mean(x0t, N, geom, np.float64)[0]                                   # [HWc,K]
    worst = {}
    for t in (100, 2):
        a, c = coefficients(t)
        got = TT.run_kernel(lib, x0t, None, cxt, TT.crop_tiles(cxt, geom), N, geom, 1.0, 1.0, a, c, hip.STEP_SAMPLE, step_row=EPI_ROWS[t], seed=SEED,
                            sample_offset=EPI_OFFSET)
        idx = got["cxt"].astype(np.int64)
        assert (got["xt"] == TT.crop_tiles(got["cxt"], geom)).all(), "a tile does not hold the canvas's class"
        laws = D.step_law64(mean, cxt[0], a, c)
        for name, sel in (("single", cover == 1), ("overlap", cover > 1)):
            draws = idx[:, sel].ravel()
            z = D.cell_z(np.bincount(draws, minlength=K), draws.size, np.broadcast_to(laws[sel], (N,) + laws[sel].shape).reshape(-1, K))
            worst[name] = max(worst.get(name, 0.0), D.worst(z))
    parity_log("draw_statistics_frequencies", tiled_single=worst["single"], tiled_overlap=worst["overlap"])
    assert max(worst.values()) <= BAR


SLOT_TS, SLOT_ROWS, SLOT_SAMPLES = (200, 2, 120, 77), (3, 249, 0, 17), (0, 7, 0xFFFFFFFE, 1000)
SLOT_KEYS = (0xFEEDFACE12345678, 0x0123456789ABCDEF, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF)


def slot_case(K, HW, rows=SLOT_ROWS, keys=SLOT_KEYS, samples=SLOT_SAMPLES, ts=SLOT_TS, uniform=False):
    """Four drawing slots at different rows, keys and sample indices: the slot table, the device buffers (slot n holds the patterns
    rolled by n; uniform: 1 / K everywhere), and per slot the patterns' (x0, x_t)."""
    x0, xt = D.epilogue_patterns(K)
    if uniform:
        x0 = np.full_like(x0, 1.0 / K)
    table = np.zeros(4, serving.SLOT_DTYPE)
    per_slot = []
    for n in range(4):
        a, c = (0.0, 1.0) if uniform else coefficients(ts[n])
        table[n] = (a, c, hip.STEP_SAMPLE, rows[n], keys[n] & 0xFFFFFFFF, keys[n] >> 32, samples[n], 0)
        per_slot.append((np.roll(x0, -n, axis=0), np.roll(xt, -n)))
    stride = (K + 4) // 4 * 4
    host = dict(x0=np.stack([D.tiled(r, 1, HW)[0] for r, _ in per_slot]), xt=np.stack([D.tiled(s, 1, HW)[0] for _, s in per_slot]).astype(np.uint8),
                xin=np.zeros((4, HW, stride), np.float32), probs=np.zeros((4, HW, K), np.float32), onehot=np.zeros((4, HW, K), np.int64))
    return table, {k: torch.from_numpy(v).to(SU.DEV) for k, v in host.items()}, per_slot


@pytest.mark.gpu
def test_slot_frequencies_follow_each_slots_own_law(lib, parity_log):
    """ccdm_slots_step: four slots at different table rows, keys and sample indices, each held to the law of its own coefficients.
    K = 5, 2^19 pixels a slot (2^16 draws a pattern)."""
    K, HW = 5, 2 ** 19
    table, d, per_slot = slot_case(K, HW)
    got = TQ.run_slots(lib, d, table, True, False)["xt"].cpu().numpy()
    worst = max(D.worst(D.pattern_z(got[n:n + 1], D.step_law64(x0.astype(np.float64), xt, float(table[n]["alpha_t"]), float(table[n]["cumalpha_tm1"]))))
                for n, (x0, xt) in enumerate(per_slot))
    parity_log("draw_statistics_frequencies", slots=worst)
    assert worst <= BAR


@pytest.mark.gpu
def test_guided_slot_frequencies_follow_each_slots_own_law(lib, parity_log):
    """ccdm_slots_guided_step: slot 0 under evidence, slot 1 tempered and truncated, slot 2 with known labels, slot 3 with all of them.
    Free pixels follow the law of the slot's shaped row, known pixels (p_hit, p_miss) around the label.  K = 5, 2^19 pixels a slot."""
    K, HW = 5, 2 ** 19
    table, d, per_slot = slot_case(K, HW)
    ev_rows = pattern_evidence(K)
    known_rows = race_patterns(K)
    kinds = [dict(ev=True, known=False, tau=1.0, r=1.0), dict(ev=False, known=False, tau=0.7, r=0.9), dict(ev=False, known=True, tau=1.0, r=1.0),
             dict(ev=True, known=True, tau=1.5, r=0.9)]
    guide = np.zeros(4, serving.GUIDE_DTYPE)
    ev = np.stack([D.tiled(ev_rows, 1, HW)[0]] * 4)
    known = np.stack([D.tiled(known_rows, 1, HW)[0]] * 4).astype(np.uint8)
    laws = []
    for n, kind in enumerate(kinds):
        x0, xt = per_slot[n]
        a, c = float(table[n]["alpha_t"]), float(table[n]["cumalpha_tm1"])
        inv, law = shaped_laws(x0, ev_rows if kind["ev"] else None, xt, kind["tau"], kind["r"], a, c)
        p_hit, p_miss = SU.probabilities(c, K)
        guide[n] = (np.float32(inv), np.float32(kind["r"]), p_hit, p_miss, (TG.EV if kind["ev"] else 0) | (TG.KNOWN if kind["known"] else 0), (0, 0, 0))
        if kind["known"]:
            clamp = D.race_law64(np.where(known_rows == FREE, 0, known_rows), K, c)
            law = np.where((known_rows != FREE)[:, None], clamp, law)
        laws.append(law)
    got = TG.run_guided(lib, d, table, guide, ev, known, True, False)["xt"].cpu().numpy()
    worst = max(D.worst(D.pattern_z(got[n:n + 1], laws[n])) for n in range(4))
    parity_log("draw_statistics_frequencies", slots_guided=worst)
    assert worst <= BAR


# ================================================================================================ 2. independence on the device
def device_draw(lib):
    """draw(row, seed, sample0, tag) of independence_scores on the device: uniform rows at K = 16 through the epilogue (tag 0), the clamp
    (every pixel known, c = 0), the renoise (r = 0) and the bound's noising (p_hit = p_miss; its counter's third word is the row's t)"""
    K, N, HW = IND_K, IND_N, IND_HW
    head = torch.full((N, HW, K), 1.0 / K, device=SU.DEV)
    own = (np.arange(N * HW).reshape(N, HW) * 5 + 1) % K

    def draw(row, seed, sample0, tag):
        if tag == 0:
            return HU.posterior_sample(head, dev_u8(own), 0.0, 1.0, hip.STEP_SAMPLE, softmax=False, philox_seed=seed, sample_offset=sample0,
                                       step=row)["xt_next"].numpy().astype(np.int64)
        if tag == SU.TAG_CLAMP:
            return TK.run_kernel(lib, torch.from_numpy(own.astype(np.uint8)), torch.zeros((N, HW), dtype=torch.uint8), K, 0.0, hip.STEP_SAMPLE,
                                 step_row=row, seed=seed, sample_offset=sample0)["xt"].numpy().astype(np.int64)
        if tag == SU.TAG_RENOISE:
            return TR.run_renoise(lib, own, K, 0.0, step_row=row, seed=seed, sample_offset=sample0)[0]
        assert tag == TB.TAG_BOUND
        tab = np.zeros(N, dtype=hip.bound_dtype())
        for n in range(N):
            tab[n] = (np.float32(1.0 / K), np.float32(1.0 / K), np.float32(0.5), np.float32(0.5), row, sample0 + n, 0, 0)
        out = torch.full((N * HW,), 255, dtype=torch.uint8, device=SU.DEV)
        labels_d, tab_d = TB.dev(own[:1].astype(np.uint8)), TB.table_dev(tab)
        hip.check(lib.ccdm_bound_noise(labels_d.data_ptr(), tab_d.data_ptr(), N, 1, HW, K, seed, out.data_ptr(), TB.stream()), "bound_noise")
        return out.cpu().numpy().reshape(N, HW).astype(np.int64)
    return draw


@pytest.mark.gpu
def test_streams_that_must_not_meet_are_independent(lib, parity_log):
    """Uniform rows at K = 16, N = 2, 2^14 pixels: the maps of row r and r + 1, of sample s and s + 1 (through sample_offset and through
    the batch index, which must give the same map), of seed and seed + 1, of pass_key(key, 0) and (key, 1), of the keys of calls 0, 1, 2,
    and of every pair among the epilogue's, the clamp's, the renoise's and the bound noising's tag at one (pixel, sample, row, key) agree
    at 1/16 of the pixels within 5 sigma; the pair tables of adjacent pixels and of pixels HW/2 apart are the outer product."""
    draw = device_draw(lib)
    z = independence_scores(draw)
    p = np.full(IND_K, 1.0 / IND_K)
    calls = [draw(IND_ROW, k, IND_OFFSET, 0) for k in model_keys(99)]
    bound_calls = [draw(IND_ROW, k, IND_OFFSET, TB.TAG_BOUND) for k in model_keys(99)[:2]]
    for i in range(3):
        for j in range(i + 1, 3):
            z[f"call {i} / {j}"] = D.agreement_z(calls[i], calls[j], p)
    z["bound call 0 / 1"] = D.agreement_z(bound_calls[0], bound_calls[1], p)
    print({k: round(v, 2) for k, v in z.items()})
    parity_log("draw_statistics_independence", streams=D.worst(list(z.values())))
    assert D.worst(list(z.values())) <= BAR, z


@pytest.mark.gpu
def test_a_slot_is_its_solo_call_and_independent_of_its_neighbour(lib, parity_log):
    """ccdm_slots_step on uniform rows at K = 16: a slot's map equals the solo epilogue call with its key, sample and row; neighbouring
    slots — other keys, rows and samples, and also slots that differ in the key alone, the row alone or the sample alone — are
    independent."""
    K, HW = IND_K, IND_HW
    p = np.full(K, 1.0 / K)
    head = torch.full((1, HW, K), 1.0 / K, device=SU.DEV)
    z = {}
    for what, rows, keys, samples in (("all differ", SLOT_ROWS, SLOT_KEYS, SLOT_SAMPLES), ("key alone", (3,) * 4, SLOT_KEYS, (7,) * 4),
                                      ("row alone", SLOT_ROWS, (SEED,) * 4, (7,) * 4), ("sample alone", (3,) * 4, (SEED,) * 4, SLOT_SAMPLES)):
        table, d, per_slot = slot_case(K, HW, rows, keys, samples, uniform=True)
        got = TQ.run_slots(lib, d, table, True, False)["xt"].cpu().numpy().astype(np.int64)
        for n in range(4):
            solo = HU.posterior_sample(head, dev_u8(D.tiled(per_slot[n][1], 1, HW)), 0.0, 1.0, hip.STEP_SAMPLE, softmax=False, philox_seed=keys[n],
                                       sample_offset=samples[n], step=rows[n])["xt_next"].numpy().astype(np.int64)
            assert (got[n] == solo[0]).all(), (what, n)
            if n:
                z[f"{what}: slot {n - 1} / {n}"] = D.agreement_z(got[n - 1], got[n], p)
    parity_log("draw_statistics_independence", slots=D.worst(list(z.values())))
    assert D.worst(list(z.values())) <= BAR, z


@pytest.mark.gpu
def test_two_step_walk_has_the_float64_joint(parity_log):
    """K = 3, two epilogue launches: the pair (class drawn at one row, class drawn at the next row given it) against the float64 joint of
    the two step laws"""
    def step(x0, xt, a, c, row):
        return HU.posterior_sample(torch.from_numpy(x0).to(SU.DEV), dev_u8(xt), a, c, hip.STEP_SAMPLE, softmax=False, philox_seed=SEED,
                                   sample_offset=IND_OFFSET, step=row)["xt_next"].numpy().astype(np.int64)
    z = two_step_z(step)
    parity_log("draw_statistics_independence", two_step_walk=abs(z))
    assert abs(z) <= BAR


# ================================================================================================ 3. the whole sampler as a known-law sampler
# sampler_util.small_model (32 x 32, T = 6) with the head's last conv weights zeroed: x0 is softmax(bias) at every pixel and step whatever
# the network computes, so the returned class map is a Markov chain with known transition matrices (chain_matrix64).  The last row of
# every walk is t = 1, where a = 0 and c = 1: its posterior is x0 itself.  Under voting = "majority" the returned map is therefore
# argmax softmax(bias) with probability one — chain_law64 says so, and the tests hold the sampler to it exactly — and what the walk drew
# on its way is seen under the vote "keep" (STEP_LAST_KEEP: the last row returns the state the row before it drew), whose law has spread.
LAW_BIAS = {2: [0.3, -0.2], 5: [0.5, -0.4, 0.1, -1.2, 0.0]}
LAW_N, LAW_CALLS = 16, 4
T_ONE_STEP = 10001          # one row at t = T: the walk stops above t = 1 and returns the class that row drew


@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def law_sampler(request):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    K = request.param
    model, sd = SU.small_model(K)
    bias = torch.tensor(LAW_BIAS[K], dtype=torch.float32)
    assert sd["out.2.weight"].shape[0] == K
    sd["out.2.weight"] = torch.zeros_like(sd["out.2.weight"])
    sd["out.2.bias"] = bias
    model.unet.load_state_dict(sd, strict=True)
    model = model.to(SU.DEV).eval()
    SU.settings(model, rng="philox", philox_seed=4242, philox_advance=True, substreams=1, use_graph=True, step_T_sample="majority")
    rng = np.random.default_rng(60 + K)
    cond = torch.from_numpy(rng.uniform(-1, 1, (LAW_N, 1, SU.H, SU.W)).astype(np.float32)).to(SU.DEV)
    xT = rng.integers(0, K, (SU.H * SU.W,))
    x = torch.nn.functional.one_hot(torch.from_numpy(xT).reshape(1, SU.H, SU.W), K).permute(0, 3, 1, 2).float().repeat(LAW_N, 1, 1, 1).contiguous()
    eng = model._engine(x.to(SU.DEV), cond, None)
    assert eng.head_fused == (K == 2)
    return dict(model=model, K=K, q=D.softmax64(bias.numpy()), cond=cond, x=x.to(SU.DEV), xT=xT)


def walk_rows(model, K, t, vote, resample=None):
    """The rows of the walk model(x, cond, t=t) takes under `vote`, as chain_matrix64 reads them, the renoising rows of a resampled walk
    included (formed as the host forms them: r in float64, each probability rounded to fp32 once)"""
    from ccdm_stochastic_segmentation_amd.models import resample_walk, step_values
    tv = step_values(model.time_steps, None if t is None else int(t))
    last = {"majority": hip.STEP_LAST_MAJORITY, "keep": hip.STEP_LAST_KEEP}[vote]
    coeffs = [model.diffusion.posterior_coeffs(tt) + (hip.STEP_SAMPLE if tt > 1 else last,) for tt in tv]
    if resample is None:
        return coeffs
    cum = model.diffusion.cumalphas.detach().cpu().double()
    rows = []
    for row, _, src in resample_walk(len(tv), *resample):
        if src is not None:
            r = float(cum[tv[row] - 1]) / float(cum[tv[src] - 1])
            rows.append(("renoise", np.float32(r + (1.0 - r) / K), np.float32((1.0 - r) / K)))
        rows.append(coeffs[row])
    return rows


def pixel_laws(s, rows):
    """[HW,K]: the law of the returned class at every pixel, given the pixel's x_T"""
    return D.chain_matrix64(s["q"], s["K"], rows)[s["xT"]]


def class_maps(out):
    return out.argmax(dim=1).reshape(out.shape[0], -1).cpu().numpy().astype(np.int64)


def sample(s, t, vote, call, **kw):
    m = s["model"]
    SU.settings(m, step_T_sample=vote, philox_call=call)
    try:
        return class_maps(m(s["x"], s["cond"], t=t, **kw)["diffusion_out"])
    finally:
        SU.settings(m, step_T_sample="majority")


def disjoint_pairs_z(maps, laws):
    """agreement_z over the sample pairs (0, 1), (2, 3), ... of maps [n,HW] whose pixels share the laws [HW,K]"""
    return D.agreement_z(maps[0::2], maps[1::2], laws[None])


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("t", [None, SU.T_STRIDED], ids=["full", "strided"])
def test_walks_follow_the_chain_law(law_sampler, parity_log, t, use_graph):
    """Full and strided walk, eager and graph, 16 samples x 1024 pixels x 4 calls: under "majority" every pixel is argmax softmax(bias),
    the chain law's single class; under "keep" the class counts follow the float64 chain law of each pixel's x_T."""
    s = law_sampler
    m, K = s["model"], s["K"]
    m.use_graph = use_graph
    try:
        worst = 0.0
        for vote in ("majority", "keep"):
            laws = pixel_laws(s, walk_rows(m, K, t, vote))
            maps = np.stack([sample(s, t, vote, call) for call in range(LAW_CALLS)])                  # [calls,N,HW]
            assert m.philox_call == LAW_CALLS
            per_draw = np.broadcast_to(laws, maps.shape + (K,)).reshape(-1, K)
            z = D.cell_z(np.bincount(maps.ravel(), minlength=K), maps.size, per_draw)
            if vote == "majority":
                assert (maps == int(np.argmax(s["q"]))).all() and (laws.max(-1) > 1 - 1e-12).all()
            else:
                assert 0.02 < laws.min() and laws.max() < 0.98                                        # a law with spread at every pixel
                # per x_T as well: the pixels that started in class j, against row j of the chain matrix
                for j in range(K):
                    sel = s["xT"] == j
                    draws = maps[..., sel].ravel()
                    z = np.append(z, D.cell_z(np.bincount(draws, minlength=K), draws.size, laws[sel][0]))
            worst = max(worst, D.worst(z))
    finally:
        m.use_graph = True
    parity_log("draw_statistics_sampler", **{f"walk_K{K}_{'full' if t is None else 'strided'}_{'graph' if use_graph else 'eager'}": worst})
    assert worst <= BAR


@pytest.mark.gpu
def test_calls_samples_and_sub_batches_are_independent(law_sampler, parity_log):
    """Successive calls (philox_advance), the samples of one call, and the two sub-batches of a call on two streams (substreams = 2, which
    must return the one-stream call's samples) agree at sum_k p_k^2 of the pixels, all samples sharing x_T and so the law of every pixel"""
    s = law_sampler
    m, K = s["model"], s["K"]
    laws = pixel_laws(s, walk_rows(m, K, None, "keep"))
    calls = [sample(s, None, "keep", call) for call in range(3)]
    z = {"samples of a call": disjoint_pairs_z(calls[0], laws)}
    for i in range(3):
        for j in range(i + 1, 3):
            z[f"call {i} / {j}"] = D.agreement_z(calls[i], calls[j], laws[None])
    m.substreams = 2
    try:
        split = sample(s, None, "keep", 0)
        assert m.last_mode[0] == 2
    finally:
        m.substreams = 1
    assert (split == calls[0]).all()
    z["sub-batches"] = D.agreement_z(split[:LAW_N // 2], split[LAW_N // 2:], laws[None])
    parity_log("draw_statistics_sampler", **{f"calls_K{K}": D.worst(list(z.values()))})
    assert D.worst(list(z.values())) <= BAR, z


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
def test_predict_multiple_counts_are_binomial(law_sampler, parity_log, batched):
    """predict_multiple, S = 16, B = 2, voting = "majority".  The full walk: every pass returns argmax softmax(bias), so `counts` is S
    there and `mean` 1 (the binomial law at pi = 0 or 1, held exactly).  The one-row walk (t = 10001, which returns what the row at t = T
    drew from the passes' common x_T): per class the histogram of `counts` over the pixels follows Binomial(16, pi) with pi the step law
    of the pixel's x_T — passes that shared their noise would pile it up at 0 and S — and `mean` lies in the 5-sigma band of pi."""
    s = law_sampler
    m, K = s["model"], s["K"]
    S, B = 16, 2
    x = s["x"][:B][None].repeat(S, 1, 1, 1, 1)
    m.philox_call = 0
    full = m.predict_multiple(s["cond"][:B], num_evaluations=S, voting="majority", x=x, batched=batched, maps=("mean", "counts"))
    top = int(np.argmax(s["q"]))
    want = torch.zeros(K, dtype=torch.int32, device=SU.DEV)
    want[top] = S
    assert (full["counts"] == want[None, :, None, None]).all() and (full["mean"][:, top] == 1.0).all()
    m.philox_call = 0
    one = m.predict_multiple(s["cond"][:B], num_evaluations=S, voting="majority", x=x, t=torch.as_tensor(T_ONE_STEP), batched=batched,
                             maps=("mean", "counts"))
    counts = one["counts"].reshape(B, K, -1).cpu().numpy()
    mean = one["mean"].reshape(B, K, -1).cpu().numpy().astype(np.float64)
    assert (counts.sum(1) == S).all()
    a, c = m.diffusion.posterior_coeffs(m.time_steps)
    laws = D.step_law64(np.broadcast_to(s["q"], (len(s["xT"]), K)), s["xT"], a, c)                   # [HW,K]
    z = [D.binomial_hist_z(counts[:, k], S, np.broadcast_to(laws[:, k], (B, laws.shape[0]))) for k in range(K)]
    band = 5.0 * np.sqrt(laws * (1 - laws) / S).T[None]
    assert (np.abs(mean - laws.T[None]) <= band + 1e-6).all()
    totals = counts.sum((0, 2))
    z += list(D.cell_z(totals, int(totals.sum()), np.broadcast_to(laws, (B, S) + laws.shape).reshape(-1, K)))
    parity_log("draw_statistics_sampler", **{f"predict_multiple_K{K}_{'batched' if batched else 'sequential'}": D.worst(z)})
    assert D.worst(z) <= BAR, z


@pytest.mark.gpu
def test_shards_are_independent_and_equal_the_unsharded_call(law_sampler, parity_log, monkeypatch):
    """distributed.sample_sharded in one process as rank 0 and as rank 1 of 2 (gather = False: the local shard): the shards put together
    are the unsharded call's samples, and the two shards' samples are independent of each other"""
    from ccdm_stochastic_segmentation_amd import distributed
    s = law_sampler
    m, K = s["model"], s["K"]
    laws = pixel_laws(s, walk_rows(m, K, None, "keep"))
    whole = sample(s, None, "keep", 0)
    shards = []
    SU.settings(m, step_T_sample="keep")
    try:
        for rank in (0, 1):
            monkeypatch.setattr(distributed.dist, "is_initialized", lambda: True)
            monkeypatch.setattr(distributed.dist, "get_world_size", lambda: 2)
            monkeypatch.setattr(distributed.dist, "get_rank", lambda rank=rank: rank)
            m.philox_call = 0
            shards.append(class_maps(distributed.sample_sharded(m, s["x"], s["cond"], gather=False)))
            monkeypatch.undo()
    finally:
        SU.settings(m, step_T_sample="majority")
    assert shards[0].shape[0] == shards[1].shape[0] == LAW_N // 2 and (np.concatenate(shards) == whole).all() and m.sample_offset == 0
    z = D.agreement_z(shards[0], shards[1], laws[None])
    parity_log("draw_statistics_sampler", **{f"shards_K{K}": abs(z)})
    assert abs(z) <= BAR


@pytest.mark.gpu
def test_resampled_walk_follows_the_chain_law_with_its_jumps(law_sampler, parity_log):
    """resample = (2, 2) under a known_labels map that is free except for one 8 x 8 corner: the known pixels come back as their labels;
    the free pixels follow the product of the walk's matrices, the renoising ones (p_stay on the diagonal, p_move off it) included — the
    revisits draw under pass_key(key, 1), so a key shared with another call or pass would show as a wrong law or as agreement between
    calls.  "majority" returns argmax softmax(bias) at the free pixels here too."""
    s = law_sampler
    m, K = s["model"], s["K"]
    known = torch.full((LAW_N, SU.H, SU.W), FREE, dtype=torch.int64)
    known[:, :8, :8] = torch.from_numpy(np.random.default_rng(8).integers(0, K, (8, 8)))
    free = (known[0] == FREE).reshape(-1).numpy()
    rows = walk_rows(m, K, None, "keep", resample=(2, 2))
    assert len(rows) == 6 + 2 + 1
    laws = pixel_laws(s, rows)
    calls = [sample(s, None, "keep", call, known_labels=known.to(SU.DEV), resample=(2, 2)) for call in range(LAW_CALLS)]
    maps = np.stack(calls)
    assert (maps[..., ~free] == known[0].reshape(-1).numpy()[~free]).all()
    draws = maps[..., free]
    per_draw = np.broadcast_to(laws[free], draws.shape + (K,)).reshape(-1, K)
    z = list(D.cell_z(np.bincount(draws.ravel(), minlength=K), draws.size, per_draw))
    z += [D.agreement_z(calls[i][:, free], calls[j][:, free], laws[free][None]) for i in range(LAW_CALLS) for j in range(i + 1, LAW_CALLS)]
    z.append(disjoint_pairs_z(calls[0][:, free], laws[free]))
    major = sample(s, None, "majority", 0, known_labels=known.to(SU.DEV), resample=(2, 2))
    assert (major[:, free] == int(np.argmax(s["q"]))).all()
    parity_log("draw_statistics_sampler", **{f"resampled_K{K}": D.worst(z)})
    assert D.worst(z) <= BAR, z


@pytest.mark.gpu
def test_queued_requests_follow_the_law_and_are_independent(law_sampler, parity_log):
    """Three requests of 8, 4 and 4 samples admitted to a queue of capacity 8 at different ticks (full and strided walks, vote "keep"):
    each follows the chain law of its walk; two requests with the same inputs are independent; a request agrees with the solo call of
    its call index at every pixel (the bit-for-bit equality has its own test in test_sampling_queue)."""
    s = law_sampler
    m, K = s["model"], s["K"]
    reqs = [dict(n=8, t=None, tick=0), dict(n=4, t=int(SU.T_STRIDED), tick=1), dict(n=4, t=None, tick=3)]
    q = m.sampling_queue(8, (1, SU.H, SU.W))
    m.philox_call = 0
    res = []
    for tick in range(4):
        for r in reqs:
            if r["tick"] == tick:
                res.append(q.submit(s["cond"][:r["n"]], x=s["x"][:r["n"]], t=r["t"], vote="keep"))
        q.step()
    q.run_until_idle()
    z = []
    maps = []
    for call, (r, got) in enumerate(zip(reqs, res)):
        assert got.call == call
        idx = class_maps(got.result()["diffusion_out"])
        maps.append(idx)
        laws = pixel_laws(s, walk_rows(m, K, r["t"], "keep"))
        per_draw = np.broadcast_to(laws, idx.shape + (K,)).reshape(-1, K)
        z += list(D.cell_z(np.bincount(idx.ravel(), minlength=K), idx.size, per_draw))
        z.append(disjoint_pairs_z(idx, laws))
        solo = sample(s, None if r["t"] is None else torch.as_tensor(r["t"]), "keep", call)[:r["n"]]
        assert (solo == idx).mean() == 1.0
    full = pixel_laws(s, walk_rows(m, K, None, "keep"))
    z.append(D.agreement_z(maps[0][:4], maps[2], full[None]))                                      # the same inputs, another request
    parity_log("draw_statistics_sampler", **{f"queue_K{K}": D.worst(z)})
    assert D.worst(z) <= BAR, z
