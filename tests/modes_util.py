"""What the mode-summary tests (test_sample_modes) share: the numpy / int64 restatement of the definition in include/ccdm_hip.h (the
fixed-point distance Q, PAM with its tie rules, assignment, ordering, the per-mode maps) and the seeded inputs.  The restatement is
written from the definition, not from the kernels: intersections by a matrix product of the class masks, the cost of a swap by
rebuilding the nearest-medoid distances from the trial medoid set.  A plain module: no fixture, no pytest setting."""
import functools

import numpy as np

ONE = 1 << 20
UNUSED = 255


# ------------------------------------------------------------------------------------------------ restatement
def q_from_counts(inter, n_i, n_j):
    """per-class q in units of 2^-20 from integer arrays: (2 (U - I) 2^20 + U) // (2 U), 0 where U == 0"""
    inter, n_i, n_j = (np.asarray(v, dtype=np.int64) for v in (inter, n_i, n_j))
    uni = n_i + n_j - inter
    return np.where(uni > 0, (2 * (uni - inter) * ONE + uni) // (2 * np.maximum(uni, 1)), 0)


def distance_restatement(a: np.ndarray, K: int) -> np.ndarray:
    """a [S,HW] class maps -> Q int64 [S,S]"""
    S = a.shape[0]
    Q = np.zeros((S, S), dtype=np.int64)
    for k in range(1, K):
        m = (a == k).astype(np.float64)                      # counts below 2^53: the float64 product is exact
        inter = np.rint(m @ m.T).astype(np.int64)
        n = inter.diagonal().copy()
        Q += q_from_counts(inter, n[:, None], n[None, :])
    assert (Q.diagonal() == 0).all() and (Q == Q.T).all()
    return Q


def cost_of(Q, meds):
    return int(Q[list(meds)].min(axis=0).sum())


def swap_costs(Q, med):
    """cost'(c, h) int64 [filled,S]; a medoid h gets the largest int64"""
    S = Q.shape[0]
    out = np.empty((len(med), S), dtype=np.int64)
    for c in range(len(med)):
        others = [m for s, m in enumerate(med) if s != c]
        rest = Q[others].min(axis=0) if others else np.full(S, np.iinfo(np.int64).max)
        out[c] = np.minimum(rest[None, :], Q).sum(axis=1)            # row h: the cost with h in slot c
    out[:, med] = np.iinfo(np.int64).max
    return out


def pam_restatement(Q: np.ndarray, M: int, max_swaps: int = 64):
    """-> dict of medoid [M], assign [S], size [M], spread [M], cost, swaps, converged, plus build_cost, build_medoids and `ties`: how
    often a decision met an exact tie (BUILD's choices, an applied swap, the assignment of a sample)"""
    Q = np.asarray(Q, dtype=np.int64)
    S = Q.shape[0]
    ties = {"build": 0, "swap": 0, "assign": 0}
    sums = Q.sum(axis=1)
    med = [int(np.argmin(sums))]                                      # (argmin / argmax: the first, i.e. the lowest index)
    ties["build"] += int((sums == sums.min()).sum() > 1)
    near = Q[med[0]].copy()
    for _ in range(1, M):
        gain = np.maximum(0, near[None, :] - Q).sum(axis=1)
        gain[med] = -1
        i = int(np.argmax(gain))
        if gain[i] <= 0:
            break
        ties["build"] += int((gain == gain[i]).sum() > 1)
        med.append(i)
        near = np.minimum(near, Q[i])
    build_medoids, build_cost = list(med), int(near.sum())
    cost, swaps = build_cost, 0
    while True:
        if len(med) == S:
            converged = 1
            break
        trial = swap_costs(Q, med)
        flat = int(np.argmin(trial))                                  # row-major: lowest c, then lowest h
        c, h = divmod(flat, S)
        best = int(trial[c, h])
        assert best == cost_of(Q, [m if s != c else h for s, m in enumerate(med)])
        if not best < cost:
            converged = 1
            break
        if swaps >= max_swaps:
            converged = 0
            break
        ties["swap"] += int((trial == best).sum() > 1)
        med[c], cost, swaps = h, best, swaps + 1
    D = Q[med]                                                        # [filled,S]
    slot = np.argmin(D, axis=0)
    ties["assign"] += int(((D == D.min(axis=0)[None, :]).sum(axis=0) > 1).sum())
    assert cost == int(D.min(axis=0).sum())
    sizes = np.bincount(slot, minlength=len(med))
    spreads = np.array([int(D[c][slot == c].sum()) for c in range(len(med))], dtype=np.int64)
    order = sorted(range(len(med)), key=lambda c: (-int(sizes[c]), med[c]))
    rank = {c: r for r, c in enumerate(order)}
    out = {"medoid": np.full(M, -1, dtype=np.int64), "size": np.zeros(M, dtype=np.int64), "spread": np.zeros(M, dtype=np.int64),
           "assign": np.array([rank[int(c)] for c in slot], dtype=np.int64), "cost": cost, "swaps": swaps, "converged": converged,
           "build_cost": build_cost, "build_medoids": build_medoids, "slot_medoids": list(med), "ties": ties}
    for r, c in enumerate(order):
        out["medoid"][r], out["size"][r], out["spread"][r] = med[c], sizes[c], spreads[c]
    return out


def maps_restatement(a: np.ndarray, assign: np.ndarray, M: int, K: int):
    """a [S,HW], assign [S] -> (vote uint8 [M,HW], counts int64 [M,HW,K], entropy float64 [M,HW])"""
    HW = a.shape[1]
    vote = np.full((M, HW), UNUSED, dtype=np.uint8)
    counts = np.zeros((M, HW, K), dtype=np.int64)
    entropy = np.zeros((M, HW), dtype=np.float64)
    for m in range(M):
        members = a[assign == m]
        if len(members) == 0:
            continue
        counts[m] = (members[:, :, None] == np.arange(K)[None, None, :]).sum(axis=0)
        vote[m] = np.argmax(counts[m], axis=-1)
        p = counts[m] / float(len(members))
        with np.errstate(divide="ignore", invalid="ignore"):
            entropy[m] = -np.where(p > 0, p * np.log(p), 0.0).sum(axis=-1)
    return vote, counts, entropy


def modes_restatement(samples: np.ndarray, K: int, M: int, max_swaps: int = 64):
    """samples [B,S,H,W] -> the arrays metrics.sample_modes returns, stacked over the images, plus the per-image PAM records"""
    B, S, H, W = samples.shape
    flat = samples.reshape(B, S, H * W)
    per = []
    out = {k: [] for k in ("distance", "medoid", "assign", "size", "spread", "cost", "swaps", "converged", "mode_map", "mode_vote", "mode_counts",
                           "mode_entropy")}
    for b in range(B):
        Q = distance_restatement(flat[b], K)
        r = pam_restatement(Q, M, max_swaps)
        vote, counts, entropy = maps_restatement(flat[b], r["assign"], M, K)
        mode_map = np.stack([flat[b][m] if m >= 0 else np.full(H * W, UNUSED, dtype=np.uint8) for m in r["medoid"]])
        per.append(r)
        for k, v in (("distance", Q), ("mode_map", mode_map.reshape(M, H, W)), ("mode_vote", vote.reshape(M, H, W)),
                     ("mode_counts", counts.reshape(M, H, W, K)), ("mode_entropy", entropy.reshape(M, H, W))):
            out[k].append(v)
        for k in ("medoid", "assign", "size", "spread", "cost", "swaps", "converged"):
            out[k].append(r[k])
    res = {k: np.stack([np.asarray(x) for x in v]) for k, v in out.items()}
    res["per_image"] = per
    return res


# ------------------------------------------------------------------------------------------------ inputs
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_case(seed, B, S, H, W, K):
    """noisy copies of a few random maps per image: distances of every size, clusters that PAM has to find"""
    rng = np.random.default_rng(seed)
    out = np.empty((B, S, H, W), dtype=np.uint8)
    for b in range(B):
        bases = rng.integers(0, K, (3, H, W))
        for s in range(S):
            m = bases[rng.integers(0, 3)].copy()
            noise = rng.random((H, W)) < rng.choice([0.02, 0.1, 0.3])
            m[noise] = rng.integers(0, K, int(noise.sum()))
            out[b, s] = m
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def duplicate_case(seed, S, H, W, K, distinct):
    """S samples that are exact copies of `distinct` different maps, in a seeded order -> (samples [1,S,H,W], group of every sample)"""
    rng = np.random.default_rng(seed)
    while True:
        bases = rng.integers(0, K, (distinct, H, W)).astype(np.uint8)
        if len({m.tobytes() for m in bases}) == distinct:
            break
    group = np.concatenate([np.arange(distinct), rng.integers(0, distinct, S - distinct)]) if S >= distinct else np.arange(S)
    group = rng.permutation(group)
    return _frozen(bases[group][None]), _frozen(group)


@functools.lru_cache(maxsize=None)
def planted_case(seed, S, flips=3):
    """13x11, K = 2: three rectangles, every sample one of them with `flips` pixels flipped -> (samples [1,S,13,11], planted group)"""
    rng = np.random.default_rng(seed)
    H, W = 13, 11
    bases = np.zeros((3, H, W), dtype=np.uint8)
    bases[0, 1:6, 1:6] = 1
    bases[1, 6:12, 4:10] = 1
    bases[2, 2:10, 7:11] = 1
    group = rng.permutation(np.concatenate([np.arange(3), rng.choice(3, S - 3, p=[0.55, 0.3, 0.15])]))
    out = bases[group].copy()
    for s in range(S):
        for p in rng.choice(H * W, flips, replace=False):
            out[s].reshape(-1)[p] ^= 1
    return _frozen(out[None]), _frozen(group)


@functools.lru_cache(maxsize=None)
def mirrored_case(seed, pairs, H=5, W=7):
    """K = 2: `pairs` maps with their mirror images and two mirror-symmetric maps, the foreground kept to a few pixels so that the
    Jaccard distances take few values: exact ties between a map and its mirror image, and many more by coincidence"""
    rng = np.random.default_rng(seed)
    half = np.zeros((pairs + 2, H, W), dtype=np.uint8)
    half[:, 1:4, 0:3] = rng.random((pairs + 2, 3, 3)) < 0.5
    maps = []
    for x in half[:pairs]:
        maps += [x, x[:, ::-1]]
    for y in half[pairs:]:
        maps.append(y | y[:, ::-1])
    order = rng.permutation(len(maps))
    return _frozen(np.stack(maps)[order][None])


def same_partition(assign, group):
    """do the two labelings split the samples into the same sets?"""
    pairs = {(int(a), int(g)) for a, g in zip(assign, group)}
    return len(pairs) == len({a for a, _ in pairs}) == len({g for _, g in pairs})
