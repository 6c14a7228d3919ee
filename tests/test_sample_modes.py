"""Mode summary of a multi-sample prediction: the kernels ccdm_modes_distance / ccdm_modes_pam / ccdm_modes_maps, metrics.sample_modes,
DenoisingModel.predict_modes and the `evaluation.modes` keys of eval_lidc_uncertainty.  Nothing in the reference computes these.
Everything the kernels write but the entropy is an integer, so every kernel test asks for equality with the numpy / int64 restatement
of the definition in include/ccdm_hip.h (modes_util); the entropy of integer frequencies is held against float64 at 1e-6, the bound of
test_predict_multiple.  The restatement itself is held against brute force, and the seeded cases are shown on the CPU to exercise
what they are there for (a swap, exact ties at every decision, the planted partition)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import modes_util as U
from tests import sampler_util
from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import metrics as M

INT_KEYS = ("distance", "medoid", "assign", "size", "spread", "cost", "swaps", "mode_map", "mode_vote", "mode_counts")
ALL_MAPS = ("vote", "entropy", "counts")
# seeds chosen on the CPU with the restatement alone (the CPU tests below assert what each was chosen for)
SWAP_CASES = ((6, 16, 5, 7, 2, 3), (3, 33, 13, 11, 3, 4))          # (seed, S, H, W, K, M) of random_case: BUILD is no local optimum
MIRROR_CASES = ((5, 9, 5), (12, 6, 5), (3, 4, 5))                   # (seed, pairs, M) of mirrored_case: ties in BUILD, SWAP and assignment
PLANTED_SEEDS = (0, 2)


# ------------------------------------------------------------------------------------------------ CPU: ABI
@pytest.mark.parametrize("symbol,nargs", [("ccdm_modes_distance", 8), ("ccdm_modes_pam", 13), ("ccdm_modes_maps", 12)])
def test_symbol_declared_bound_and_built(symbol, nargs):
    sampler_util.assert_symbol_declared_bound_and_built(symbol, nargs, "ccdm_modes.hip")


def test_library_refuses_what_it_cannot_cluster():
    """the limits are checked before anything is launched or read: a host buffer stands in for the device's"""
    lib = hip.load()
    buf = np.zeros(1 << 12, dtype=np.int64)
    p = buf.ctypes.data

    def distance(B=1, S=4, HW=16, K=2, a=p, ws=p, Q=p):
        return lib.ccdm_modes_distance(a, B, S, HW, K, ws, Q, None)

    def pam(B=1, S=4, M=2, max_swaps=64, Q=p, out=p, spread=p):
        return lib.ccdm_modes_pam(Q, B, S, M, max_swaps, out, out, out, spread, p, out, out, None)

    def maps(B=1, S=4, M=2, HW=16, K=2, a=p, vote=p):
        return lib.ccdm_modes_maps(a, p, p, B, S, M, HW, K, vote, None, None, None)

    for call, change, what in ((distance, dict(K=1), "K=1"), (distance, dict(K=33), "K=33"), (distance, dict(S=0), "S=0"),
                               (distance, dict(S=257), "S=257"), (distance, dict(HW=0), "HW=0"), (distance, dict(B=-1), "B=-1"),
                               (distance, dict(a=None), "null"), (distance, dict(ws=None), "null"), (distance, dict(Q=None), "null"),
                               (pam, dict(S=0), "S=0"), (pam, dict(S=257), "S=257"), (pam, dict(M=0), "M=0"), (pam, dict(M=17), "M=17"),
                               (pam, dict(max_swaps=-1), "max_swaps=-1"), (pam, dict(Q=None), "null"), (pam, dict(out=None), "null"),
                               (pam, dict(spread=p + 4), "8-byte aligned"), (pam, dict(B=65536), "B=65536"),
                               (maps, dict(K=1), "K=1"), (maps, dict(M=17), "M=17"), (maps, dict(S=300), "S=300"), (maps, dict(vote=None), "null"),
                               (maps, dict(HW=-3), "HW=-3")):
        rc = call(**change)
        assert rc < 0 and what in hip.last_error(), (what, hip.last_error())
        with pytest.raises(hip.CcdmHipError, match=re.escape(what)):
            hip.check(rc, "modes")
    assert distance(B=0) == 0 and pam(B=0) == 0 and maps(B=0) == 0 and not buf.any()      # B = 0: nothing launched, nothing written


def test_sample_modes_refuses_bad_arguments():
    a = torch.zeros((1, 4, 5, 7), dtype=torch.uint8)
    for kw, name in ((dict(num_classes=1), "num_classes"), (dict(num_classes=33), "num_classes"), (dict(num_classes=2.0), "num_classes"),
                     (dict(modes=0), "modes"), (dict(modes=17), "modes"), (dict(modes=True), "modes"), (dict(max_swaps=-1), "max_swaps"),
                     (dict(maps=("vote", "mean")), "maps")):
        args = dict(num_classes=2, modes=3)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            M.sample_modes(a, **args)
    with pytest.raises(ValueError, match="S=257"):
        M.sample_modes(torch.zeros((1, 257, 2, 2), dtype=torch.uint8), 2, 3)
    with pytest.raises(ValueError, match="S=0"):
        M.sample_modes(torch.zeros((1, 0, 2, 2), dtype=torch.uint8), 2, 3)
    for bad in (torch.zeros((4, 5, 7), dtype=torch.uint8), torch.zeros((1, 4, 5, 7)), np.zeros((1, 4, 5, 7), dtype=np.uint8)):
        with pytest.raises(ValueError, match="samples_idx"):
            M.sample_modes(bad, 2, 3)
    with pytest.raises(hip.CcdmHipError, match="GPU tensors"):                          # no CPU path, as pairwise_class_counts
        M.sample_modes(a, 2, 3)


def test_evaluation_keys_are_validated():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    assert E.mode_count(4) == 4 and E.mode_count(1) == 1 and E.mode_count(16) == 16
    for bad in (0, 17, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="mode_count"):
            E.mode_count(bad)
    assert E.mode_max_swaps(0) == 0 and E.mode_max_swaps(64) == 64
    for bad in (-1, 1.5, True, "8"):
        with pytest.raises(ValueError, match="mode_max_swaps"):
            E.mode_max_swaps(bad)


# ------------------------------------------------------------------------------------------------ CPU: the restatement
def test_fixed_point_distance_is_within_half_a_unit_of_the_float_distance():
    rng = np.random.default_rng(5)
    K = 5
    n_i, n_j = rng.integers(0, 40, (2, 400, K))
    n_i[::7] = 0
    n_j[::7] = 0                                                 # U_k = 0 in every class of these rows
    n_j[3::11, 2] = 0
    n_i[3::11, 2] = 0                                            # and in one class of these
    inter = rng.integers(0, np.minimum(n_i, n_j) + 1)
    counts = np.stack([inter, n_i + n_j - inter], axis=-1)       # what pairwise_class_counts returns: (intersection, union)
    assert (counts[..., 1] == 0).any() and (counts[::7, 1:, 1] == 0).all()
    Q = U.q_from_counts(inter, n_i, n_j)[:, 1:].sum(axis=-1)
    got = Q / float((K - 1) * U.ONE)
    want = M._distance_from_counts(counts)
    err = np.abs(got - want).max()
    print(f"fixed point against float distance: max error {err:.3e} (bound {2.0 ** -21:.3e})")
    assert err <= 2.0 ** -21
    assert (Q[::7] == 0).all() and Q.max() <= (K - 1) * U.ONE


def _brute_force_best_swap(Q, med):
    best = None
    for c in range(len(med)):
        for h in range(Q.shape[0]):
            if h not in med:
                t = U.cost_of(Q, [m if s != c else h for s, m in enumerate(med)])
                if best is None or t < best:
                    best = t
    return best


def test_restatement_ends_in_a_swap_local_optimum_no_worse_than_build():
    checked = 0
    for seed in range(12):
        S, H, W, K, Mn = [(16, 5, 7, 2, 3), (12, 5, 7, 3, 5), (20, 13, 11, 2, 2)][seed % 3]
        Q = U.distance_restatement(U.random_case(100 + seed, 1, S, H, W, K)[0].reshape(S, -1), K)
        r = U.pam_restatement(Q, Mn)
        meds = r["slot_medoids"]
        assert r["converged"] == 1 and r["cost"] <= r["build_cost"] and r["cost"] == U.cost_of(Q, meds) == int(r["spread"].sum())
        assert r["build_cost"] == U.cost_of(Q, r["build_medoids"])
        best = _brute_force_best_swap(Q, meds)
        assert best is None or best >= r["cost"]                 # no single (c, h) swap lowers the cost
        assert (r["swaps"] == 0) == (meds == r["build_medoids"])
        assert int(r["size"].sum()) == S and (np.diff(r["size"]) <= 0).all()
        checked += r["swaps"]
    assert checked >= 3                                          # (some of these did swap)


def test_restatement_returns_the_groups_of_identical_maps():
    for S, distinct, Mn in ((9, 4, 4), (9, 4, 7), (5, 5, 16), (7, 1, 3)):
        samples, group = U.duplicate_case(31 + S, S, 5, 7, 3, distinct)
        r = U.pam_restatement(U.distance_restatement(samples[0].reshape(S, -1), 3), Mn)
        assert int((r["medoid"] >= 0).sum()) == distinct and U.same_partition(r["assign"], group)
        assert r["cost"] == 0 and not r["spread"].any() and r["swaps"] == 0 and r["converged"] == 1
        assert (r["medoid"][distinct:] == -1).all() and not r["size"][distinct:].any()
        assert sorted(r["size"][:distinct].tolist(), reverse=True) == sorted(np.bincount(group).tolist(), reverse=True)


def test_seeded_cases_exercise_what_they_are_for():
    for seed, S, H, W, K, Mn in SWAP_CASES:
        Q = U.distance_restatement(U.random_case(seed, 1, S, H, W, K)[0].reshape(S, -1), K)
        r = U.pam_restatement(Q, Mn)
        assert r["swaps"] >= 1 and r["cost"] < r["build_cost"]
        r0 = U.pam_restatement(Q, Mn, max_swaps=0)
        assert r0["swaps"] == 0 and r0["converged"] == 0 and r0["cost"] == r0["build_cost"] and r0["slot_medoids"] == r["build_medoids"]
    ties = {"build": 0, "swap": 0, "assign": 0}
    for seed, pairs, Mn in MIRROR_CASES:
        a = U.mirrored_case(seed, pairs)
        r = U.pam_restatement(U.distance_restatement(a[0].reshape(a.shape[1], -1), 2), Mn)
        assert all(r["ties"][k] >= 1 for k in ties), r["ties"]   # every tie rule decides something in every one of them
        for k in ties:
            ties[k] += r["ties"][k]
    print("ties met by the mirrored cases:", ties)
    for seed in PLANTED_SEEDS:
        samples, group = U.planted_case(seed, 33)
        r = U.pam_restatement(U.distance_restatement(samples[0].reshape(33, -1), 2), 3)
        assert U.same_partition(r["assign"], group) and r["size"].tolist() == sorted(np.bincount(group).tolist(), reverse=True)


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def check_exact(samples: np.ndarray, K: int, Mn: int, max_swaps: int = 64, tag=""):
    """metrics.sample_modes on the device against the restatement: every integer equal, the entropy within 1e-6"""
    got = M.sample_modes(torch.from_numpy(np.array(samples)).cuda(), K, Mn, max_swaps=max_swaps, maps=ALL_MAPS, return_distance=True)
    torch.cuda.synchronize()
    want = U.modes_restatement(np.asarray(samples), K, Mn, max_swaps)
    S = samples.shape[1]
    err = float((got["mode_entropy"].cpu().double() - torch.from_numpy(want["mode_entropy"])).abs().max())
    bad = {k: int((got[k].cpu().long() != torch.from_numpy(want[k]).long()).sum()) for k in INT_KEYS + ("converged",)}
    print(f"sample_modes[{tag} {samples.shape} K={K} M={Mn}] found={(want['medoid'] >= 0).sum(axis=1).tolist()} swaps={want['swaps'].tolist()} "
          f"mismatches={bad} entropy err={err:.2e}")
    for k in INT_KEYS + ("converged",):
        assert tuple(got[k].shape) == want[k].shape, k
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k]).to(got[k].dtype)), k
    assert got["distance"].dtype == got["medoid"].dtype == got["assign"].dtype == got["size"].dtype == got["swaps"].dtype == torch.int32
    assert got["spread"].dtype == got["cost"].dtype == torch.int64 and got["mode_vote"].dtype == got["mode_map"].dtype == torch.uint8
    assert err < 1e-6
    assert torch.equal(got["share"].cpu(), got["size"].cpu().float() / float(S)) and got["share"].dtype == torch.float32
    assert torch.allclose(got["share"].sum(dim=1).cpu(), torch.ones(samples.shape[0]))
    return got, want


# (B, S, H, W, K, M): HW 35 and 143 take the byte loads and less than one chunk of pixels (35: less than one wave), 4096 the dword
# loads and four chunks, 33x35 and 36x36 a partial second chunk on either path; S 1 .. 16 one tile of pairs, 33 and 100 several, 129 more
# than the LDS-resident Q; K 2 / 3 / 20 the three class-count paths
RANDOM_SHAPES = [(1, 1, 5, 7, 2, 1), (3, 2, 5, 7, 3, 3), (1, 5, 13, 11, 20, 8), (3, 16, 13, 11, 2, 3), (1, 33, 5, 7, 3, 16), (1, 100, 64, 64, 2, 8),
                 (1, 129, 13, 11, 3, 16), (3, 129, 5, 7, 2, 3), (1, 16, 64, 64, 20, 3), (1, 17, 33, 35, 3, 8), (1, 33, 36, 36, 2, 1),
                 (2, 128, 5, 7, 2, 4)]                           # (S = 128: the largest Q that lives in LDS, 64 KB of it)


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H,W,K,Mn", RANDOM_SHAPES)
def test_random_maps(B, S, H, W, K, Mn):
    check_exact(U.random_case(7 * S + H, B, S, H, W, K), K, Mn, tag="random")


@pytest.mark.gpu
def test_identical_samples_are_one_mode():
    one = U.random_case(1, 1, 1, 13, 11, 3)
    got, _ = check_exact(np.repeat(one, 16, axis=1), 3, 3, tag="identical")
    assert got["medoid"].cpu().tolist() == [[0, -1, -1]] and got["size"].cpu().tolist() == [[16, 0, 0]] and int(got["cost"]) == 0
    assert bool((got["mode_vote"][0, 1:] == 255).all()) and bool((got["mode_map"][0, 1:] == 255).all())
    assert not bool(got["mode_entropy"].any()) and not bool(got["mode_counts"][0, 1:].any())
    assert torch.equal(got["mode_vote"][0, 0].cpu(), torch.from_numpy(np.array(one[0, 0])))


@pytest.mark.gpu
@pytest.mark.parametrize("S,Mn", [(2, 3), (5, 8), (5, 16), (1, 16)])
def test_fewer_samples_than_modes(S, Mn):
    got, want = check_exact(U.random_case(3, 3, S, 5, 7, 2), 2, Mn, tag="S < M")
    assert bool((got["medoid"][:, S:] == -1).all()) and not bool(got["size"][:, S:].any())


@pytest.mark.gpu
@pytest.mark.parametrize("S,distinct,Mn", [(9, 4, 4), (9, 4, 7), (33, 5, 16), (129, 3, 3)])
def test_exact_duplicate_groups(S, distinct, Mn):
    samples, group = U.duplicate_case(31 + S, S, 5, 7, 3, distinct)
    got, _ = check_exact(samples, 3, Mn, tag="duplicates")
    assert U.same_partition(got["assign"][0].cpu().numpy(), group) and int(got["cost"]) == 0 and not bool(got["spread"].any())
    assert int((got["medoid"] >= 0).sum()) == distinct


@pytest.mark.gpu
def test_class_absent_from_every_sample():
    a = np.array(U.random_case(9, 3, 16, 13, 11, 3))
    a[a == 1] = 0                                                # class 1 of K = 3, then classes 1..18 of K = 20: U_k = 0
    check_exact(a, 3, 3, tag="absent class")
    check_exact(np.where(a == 2, 19, 0).astype(np.uint8), 20, 3, tag="absent classes")
    check_exact(np.zeros((1, 5, 5, 7), dtype=np.uint8), 2, 3, tag="background only")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,pairs,Mn", MIRROR_CASES)
def test_exact_ties_follow_the_tie_rules(seed, pairs, Mn):
    _, want = check_exact(U.mirrored_case(seed, pairs), 2, Mn, tag="mirrored")
    assert all(want["per_image"][0]["ties"][k] >= 1 for k in ("build", "swap", "assign"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,S,H,W,K,Mn", SWAP_CASES)
def test_swap_improves_build_and_max_swaps_zero_returns_build(seed, S, H, W, K, Mn):
    samples = U.random_case(seed, 1, S, H, W, K)
    got, want = check_exact(samples, K, Mn, tag="swap")
    assert want["per_image"][0]["swaps"] >= 1 and int(got["swaps"]) >= 1 and int(got["converged"]) == 1
    got0, want0 = check_exact(samples, K, Mn, max_swaps=0, tag="max_swaps 0")
    assert int(got0["swaps"]) == 0 and int(got0["converged"]) == 0 and int(got0["cost"]) == want["per_image"][0]["build_cost"] > int(got["cost"])
    assert sorted(got0["medoid"][0].cpu().tolist()) == sorted(want["per_image"][0]["build_medoids"])
    got1, _ = check_exact(np.repeat(samples[:, :1], 4, axis=1), K, Mn, max_swaps=0, tag="max_swaps 0, no swap left")
    assert int(got1["converged"]) == 1                           # converged is 0 only where a swap exists


@pytest.mark.gpu
@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_clusters_are_recovered(seed):
    samples, group = U.planted_case(seed, 33)
    got, _ = check_exact(samples, 2, 3, tag="planted")
    assert U.same_partition(got["assign"][0].cpu().numpy(), group)
    assert got["size"][0].cpu().tolist() == sorted(np.bincount(group).tolist(), reverse=True)


@pytest.mark.gpu
def test_unaligned_stack_and_index_maps():
    """the stack starts one byte off a dword with HW % 4 == 0: the byte loads; int64 maps and a sliced stack go through sample_modes"""
    lib = hip.load()
    B, S, H, W, K = 2, 17, 8, 8, 3
    samples = U.random_case(11, B, S, H, W, K)
    want = U.modes_restatement(samples, K, 3)
    buf = torch.zeros(samples.size + 1, dtype=torch.uint8, device="cuda")
    dev = buf[1:].view(B, S, H * W)
    dev.copy_(torch.from_numpy(np.array(samples)).reshape(B, S, H * W))
    assert dev.data_ptr() % 4 == 1
    ws = torch.full((B, S, S, K), 5, dtype=torch.int32, device="cuda")          # (the call clears its workspace)
    Q = torch.full((B, S, S), -7, dtype=torch.int32, device="cuda")
    hip.check(lib.ccdm_modes_distance(dev.data_ptr(), B, S, H * W, K, ws.data_ptr(), Q.data_ptr(), None), "modes_distance")
    torch.cuda.synchronize()
    assert torch.equal(Q.cpu().long(), torch.from_numpy(want["distance"]))
    s64 = torch.from_numpy(samples.astype(np.int64)).cuda()
    got = M.sample_modes(s64, K, 3)
    assert set(got) == {"medoid", "assign", "size", "share", "spread", "cost", "swaps", "converged", "mode_map", "mode_vote", "mode_entropy"}
    assert torch.equal(got["assign"].cpu().long(), torch.from_numpy(want["assign"]))
    sliced = M.sample_modes(s64[:, :5], K, 3, maps=(), return_distance=True)          # the evaluator's pred_idx[:, :s]
    assert set(sliced) == {"medoid", "assign", "size", "share", "spread", "cost", "swaps", "converged", "mode_map", "distance"}
    assert torch.equal(sliced["medoid"].cpu().long(), torch.from_numpy(U.modes_restatement(samples[:, :5], K, 3)["medoid"]))
    again = M.sample_modes(s64, K, 3)
    for k in got:
        assert torch.equal(got[k], again[k]), k                  # two calls are bit-identical


# ------------------------------------------------------------------------------------------------ GPU: the sampler
@pytest.mark.gpu
def test_predict_modes_on_the_small_model():
    K, B, S, Mn = 2, 2, 5, 3
    H, W, DEV = sampler_util.H, sampler_util.W, sampler_util.DEV
    model, _ = sampler_util.small_model(K)
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, True
    rng = np.random.default_rng(17)
    cond = torch.from_numpy(rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32)).to(DEV)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (S, B, H, W))), K).permute(0, 1, 4, 2, 3).float().to(DEV)
    model.philox_call = 3
    out = model.predict_modes(cond, num_evaluations=S, modes=Mn, x=x, maps=ALL_MAPS)
    assert model.philox_call == 4                                # advanced like one call
    assert model.step_T_sample == "majority"
    assert out["samples"].shape == (B, S, H, W) and out["samples"].dtype == torch.uint8
    model.philox_call = 3
    ref = model(x.transpose(0, 1).reshape(B * S, K, H, W), cond.repeat_interleave(S, dim=0))["diffusion_out"]
    assert torch.equal(out["samples"].long(), ref.argmax(dim=1).reshape(B, S, H, W))
    want = M.sample_modes(out["samples"], K, Mn, maps=ALL_MAPS)
    assert set(out) == set(want) | {"samples"}
    for k, v in want.items():
        assert torch.equal(out[k], v), k
    assert torch.allclose(out["share"].sum(dim=1).cpu(), torch.ones(B))
    print(f"predict_modes: sizes {out['size'].cpu().tolist()} medoids {out['medoid'].cpu().tolist()}")
    for kw, name in ((dict(modes=0), "modes"), (dict(modes=17), "modes"), (dict(num_evaluations=257), "num_evaluations"),
                     (dict(maps=("mean",)), "maps"), (dict(max_swaps=-1), "max_swaps")):
        args = dict(num_evaluations=S, modes=Mn)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            model.predict_modes(cond, **args)
    assert model.philox_call == 4                                # a refused call draws nothing


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_evaluator_modes_end_to_end(tmp_path):
    """the evaluator with fixed predictions (its distances come from the device, so it needs one)"""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    K, H, W, evaluations, batch = 2, 13, 11, [2, 4], 2
    S = max(evaluations)
    samples = U.random_case(21, 3, S, H, W, K)                   # 3 images in batches of 2: the last batch holds one
    raters = U.random_case(22, 3, 4, H, W, K)
    one_hot = lambda idx: torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), K).movedim(-1, -3).float()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return samples.shape[0]

        def __getitem__(self, b):
            return torch.zeros((1, H, W)), one_hot(raters[b]), np.array([0.25] * 4)

    def fake():
        class Fake:
            step_T_sample = "majority"
            calls = 0

            def __call__(self, x, image, **kw):
                first = self.calls * batch
                p = one_hot(samples[first:first + x.shape[0] // S]).reshape(x.shape[0], K, H, W)
                self.calls += 1
                return {"diffusion_out": p.to(x.device)}
        return Fake()

    params = {"dataset_file": "datasets.lidc", "batch_size": batch, "evaluations": evaluations, "output_path": str(tmp_path / "out")}
    plain = E.eval_lidc_uncertainty(dict(params), dataset=DS(), device="cuda:0", model=fake())
    assert not (tmp_path / "out").exists()
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"modes": True}}, dataset=DS(), device="cuda:0", model=fake())
    assert set(res) == set(plain) | {"modes"}
    for key, value in plain.items():                             # everything the evaluator returns today is untouched
        assert res[key] == value, key
    assert len(res["modes"]) == len(evaluations)
    for i, (s, got) in enumerate(zip(evaluations, res["modes"])):
        print(f"modes[{s}] got={got} plain GED={plain['GED'][i]!r}")
        want = U.modes_restatement(samples[:, :s], K, 4)
        assert got["samples"] == s and got["images"] == 3 and got["mode_count"] == 4 and got["max_swaps"] == 64 and got["converged"] == 1.0
        assert got["modes_found"] == float((want["medoid"] >= 0).sum(axis=1).mean()) == s      # random maps: all distinct
        assert got["largest_share"] == float((want["size"][:, 0] / s).mean())
        # mode_count >= the distinct samples: the share-weighted medoids ARE the sample distribution
        assert abs(got["ged_summary"] - plain["GED"][i]) <= 1e-12
        assert 0.0 <= got["coverage"] <= 1.0
    # fewer modes than distinct samples: another distribution, another GED; the nearest of fewer medoids is no nearer
    one = E.eval_lidc_uncertainty({**params, "evaluation": {"modes": True, "mode_count": 1, "mode_max_swaps": 0}, "output_path": None},
                                  dataset=DS(), device="cuda:0", model=fake())["modes"]
    assert one[1]["mode_count"] == 1 and one[1]["max_swaps"] == 0 and one[1]["modes_found"] == 1.0 and one[1]["largest_share"] == 1.0
    assert abs(one[1]["ged_summary"] - plain["GED"][1]) > 1e-6 and one[1]["coverage"] >= res["modes"][1]["coverage"]
    for bad, key in (({"mode_count": 0}, "mode_count"), ({"mode_count": 17}, "mode_count"), ({"mode_max_swaps": -1}, "mode_max_swaps")):
        with pytest.raises(ValueError, match=key):
            E.eval_lidc_uncertainty({**params, "evaluation": {"modes": True, **bad}, "output_path": None}, dataset=DS(), device="cuda:0",
                                    model=fake())
    with open(tmp_path / "out" / "lidc_modes.json") as f:
        assert json.load(f) == res["modes"] == json.loads(json.dumps(res["modes"]))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_modes.json"]
