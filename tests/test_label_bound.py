"""The variational bound on the likelihood of held-out labels: the kernels ccdm_bound_noise / ccdm_bound_terms, the host arithmetic
(models.bound_timesteps, bound_prior, bound_rows), DenoisingModel.label_bound and the `evaluation.label_bound` keys of
eval_lidc_uncertainty.  include/ccdm_hip.h has the definition.  The draw is held bit for bit against the tests' restatement of the
two-valued Exp(1) race (sampler_util.race_restatement, tag 0x20000000); the per-pixel term against the oracle's training-time pieces
(theta_post_t, theta_post_prob_t, kl_clamped) on the same fp32 inputs in float64.

The per-pixel tolerance is absolute, TOL(K) = (K + 256) * 2^-24, derived and not tuned: the relative rounding of q_k through the closed
form is <= (K / 2 + 10) ulp and enters the term through log q_k as that many ulp absolute, times p_k; p_k is a few ulp, times
|log p_k - log q_k| + 1 <= 29 (q_k >= 1e-12: -log q_k <= 27.7); the two logf results are each <= 1 ulp of a value <= 27.7; and
sum_k p_k = 1.  Measured maximum on an MI355X, as test_terms_kernel_against_float64 prints it: 44.9 * 2^-24.
The t = 1 rows are held to 1 ulp of -logf(max(x0_y, floor)) with logf the device's own fp32 logarithm (0 ulp measured); that function is
up to 2 ulp from the correctly rounded float64 logarithm, which the test prints beside it."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from tests import sampler_util as U
from tests.ladder_util import RUNG_KS, rung_of
from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import models as MD

TAG_BOUND = 0x20000000
FLOOR = float(np.float32(1e-12))
T_K = 6                                     # the schedule of the kernel tests: cosine, 6 levels (the small model's)
FIELDS = ["p_hit", "p_miss", "alpha_t", "cumalpha_tm1", "t", "sample", "label_row", "reserved"]


def tol(K):
    return (K + 256) * 2.0 ** -24


def diffusion(K, T=T_K):
    return MD.DiffusionModel("cosine", T, K, {"s": 0.008})


def make_table(dm, K, spec):
    """spec: per engine row (t, sample, label_row) or None for an idle row -> the numpy table, by hand (not through bound_rows)"""
    tab = np.zeros(len(spec), dtype=hip.bound_dtype())
    tab["t"] = hip.BOUND_IDLE
    for n, row in enumerate(spec):
        if row is None:
            continue
        t, sample, lr = row
        p_hit, p_miss = U.probabilities(float(dm.cumalphas.double()[t - 1]), K)
        a, c = dm.posterior_coeffs(t)
        tab[n] = (p_hit, p_miss, np.float32(a), np.float32(c), t, sample, lr, 0)
    return tab


def rows_for(N):
    """N = 1: a mid-walk row on the second label map; N = 3: t = 1 and t = T on one shared map around an idle row"""
    return [(3, 11, 1)] if N == 1 else [(1, 5, 0), None, (T_K, 9, 0)]


def noise_restatement(labels, tab, K, seed, dm):
    """x_t per busy row (None for an idle one): the race at the counted pixels, pixel % K at the others"""
    HW = labels.shape[1]
    out = []
    for r in tab:
        if r["t"] < 1:
            out.append(None)
            continue
        y = labels[r["label_row"]].astype(np.int64)
        c = float(dm.cumalphas.double()[int(r["t"]) - 1])
        assert U.probabilities(c, K) == (r["p_hit"], r["p_miss"])              # race_restatement forms the pair from c as the host does
        draw = U.race_restatement(np.where(y < K, y, 0)[None], K, c, int(r["t"]), seed, int(r["sample"]), TAG_BOUND)[0]
        out.append(np.where(y < K, draw, np.arange(HW) % K))
    return out


def terms_restatement(x0, xt, y, a, c, K, weights=None):
    """float64 per-pixel terms [N,HW] (0 at uncounted pixels) from the oracle's training-time pieces on the same fp32 inputs.
    x0 fp32 [N,HW,K]; xt, y int [N,HW]; a, c fp32 [N]."""
    N, HW = xt.shape
    counted = y < K
    oh = lambda idx: torch.from_numpy(U.onehot_np(np.where(idx < K, idx, 0), K).astype(np.float64)).permute(0, 2, 1)[..., None]   # [N,K,HW,1]
    a64, c64 = torch.from_numpy(a.astype(np.float64)), torch.from_numpy(c.astype(np.float64))
    p = O.theta_post_t(oh(xt), oh(y), a64, c64)
    q = O.theta_post_prob_t(oh(xt), torch.from_numpy(x0.astype(np.float64)).permute(0, 2, 1)[..., None], a64, c64)
    l = O.kl_clamped(p, q, FLOOR).sum(1)[..., 0].numpy()
    w = np.ones(K) if weights is None else np.asarray(weights, dtype=np.float64)
    return np.where(counted, l * w[np.where(counted, y, 0)], 0.0)


def random_x0(rng, N, HW, K):
    """softmax rows: a third ordinary, a third near one-hot (entries far below the floor), a third with one entry just below it"""
    logits = rng.normal(0, 3, (N, HW, K))
    kind = rng.integers(0, 3, (N, HW))
    logits[kind == 1] *= 40.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    low = rng.integers(0, K, (N, HW))
    p[kind == 2, low[kind == 2]] = 3e-13
    return p.astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU
def test_bound_symbols_declared_bound_and_built():
    """both entry points as every step symbol is checked; the workspace call (a size_t, so by hand); the row's layout by the C compiler"""
    lib = U.assert_symbol_declared_bound_and_built("ccdm_bound_noise", 9, "ccdm_bound.hip")
    U.assert_symbol_declared_bound_and_built("ccdm_bound_terms", 15, "ccdm_bound.hip")
    res, args = hip.SIGNATURES["ccdm_bound_terms_workspace_bytes"]
    assert res is C.c_size_t and args == [C.c_int] * 3 and hasattr(lib, "ccdm_bound_terms_workspace_bytes")
    assert "size_t ccdm_bound_terms_workspace_bytes(int N, int HW, int K);" in open(os.path.join(U.ROOT, "include", "ccdm_hip.h")).read()
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ccdm_hip.h"\nint main(){ printf("%zu %d", sizeof(ccdm_bound_row), CCDM_BOUND_IDLE);\n' + \
          "".join(f'printf(" %zu", offsetof(ccdm_bound_row, {f}));\n' for f in FIELDS) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    R = hip.BoundRow
    assert out == [32, hip.BOUND_IDLE] + [getattr(R, f).offset for f in FIELDS] == [32, -1, 0, 4, 8, 12, 16, 20, 24, 28]
    assert C.sizeof(R) == 32 and [f for f, _ in R._fields_] == FIELDS
    dt = hip.bound_dtype()
    assert dt.itemsize == 32 and list(dt.names) == FIELDS and [dt.fields[f][1] for f in FIELDS] == out[2:]
    # 16 bytes per (block, row) pair: 256 pixels per block up to K = 32, 64 above; 0 for what the launch refuses
    ws = lib.ccdm_bound_terms_workspace_bytes
    assert ws(64, 16384, 2) == 16 * (64 * 64 + 64) and ws(3, 77, 5) == 16 * (1 + 3) and ws(3, 77, 33) == 16 * (4 + 3)
    assert ws(0, 4, 2) == ws(1, 0, 2) == ws(1, 4, 0) == ws(1, 4, 256) == ws(1 << 16, 1 << 16, 2) == 0


def test_bound_kernels_refuse_bad_arguments():
    """every refusal happens with host pointers, so nothing is launched (a launch would fault)"""
    import __graft_entry__ as g
    g.build()
    lib = hip.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    noise = dict(labels=p, table=p, N=1, R=1, HW=4, K=2, philox_seed=1, xt_out=p, stream=None)
    terms = dict(x0=p, xt=p, labels=p, table=p, class_weights=None, N=1, R=1, HW=4, K=2, floor=1e-12, ws=p, row_sum=p, row_weight=p, map=None,
                 stream=None)
    shape_cases = ((dict(N=0), "shape"), (dict(R=0), "shape"), (dict(HW=0), "shape"), (dict(K=0), "K="), (dict(K=256), "K="),
                   (dict(N=1 << 16, HW=1 << 16), "pixels"), (dict(R=1 << 16, HW=1 << 16), "pixels"), (dict(table=p + 1), "table"))
    for fn, good, cases in ((lib.ccdm_bound_noise, noise, tuple((dict([(k, None)]), "null") for k in ("labels", "table", "xt_out")) + shape_cases),
                            (lib.ccdm_bound_terms, terms,
                             tuple((dict([(k, None)]), "null") for k in ("x0", "xt", "labels", "table", "ws", "row_sum", "row_weight")) + shape_cases +
                             ((dict(floor=0.0), "floor"), (dict(floor=1.0), "floor"), (dict(floor=-1e-12), "floor"), (dict(floor=float("nan")), "floor"),
                              (dict(ws=p + 4), "workspace")))):
        for change, word in cases:
            args = dict(good)
            args.update(change)
            assert fn(*args.values()) < 0, change
            assert word in hip.last_error(), (change, hip.last_error())


def test_bound_timesteps():
    t, w = MD.bound_timesteps(7, None, 1, 3)
    assert t.shape == w.shape == (3, 7) and (t == np.arange(1, 8)).all() and (w == 1).all() and t.dtype == np.int64 and w.dtype == np.float64
    t, w = MD.bound_timesteps(9, [9, 2, 5], 1, 2)
    assert (t == [[9, 2, 5]] * 2).all() and (w == 1).all()
    # T = 6, M = 4: floor(j * 6 / 4) = 0, 1, 3, 4, 6 -> the strata {1}, {2, 3}, {4}, {5, 6}
    t, w = MD.bound_timesteps(6, 4, 77, 50)
    assert (w == [[1, 2, 1, 2]] * 50).all()
    assert (t[:, 0] == 1).all() and np.isin(t[:, 1], [2, 3]).all() and (t[:, 2] == 4).all() and np.isin(t[:, 3], [5, 6]).all()
    assert set(t[:, 1]) == {2, 3} and set(t[:, 3]) == {5, 6}                    # 50 labels: both members of a stratum of two turn up
    for T, M in ((250, 10), (250, 7), (13, 13), (5, 1)):
        t, w = MD.bound_timesteps(T, M, 5, 4)
        edges = [(j * T) // M for j in range(M + 1)]
        assert (w.sum(axis=1) == T).all() and edges[0] == 0 and edges[-1] == T
        assert sorted(v for j in range(M) for v in range(edges[j] + 1, edges[j + 1] + 1)) == list(range(1, T + 1))      # a partition of 1..T
        for j in range(M):
            assert ((t[:, j] > edges[j]) & (t[:, j] <= edges[j + 1])).all() and (w[:, j] == edges[j + 1] - edges[j]).all()
    a, b, c = (MD.bound_timesteps(250, 10, key, 4)[0] for key in (123, 123, 124))
    assert (a == b).all() and (a != c).any()
    for bad in ([0], [7], [2, 2], [], [1.5], 0, 7, "x"):
        with pytest.raises(ValueError, match="timesteps"):
            MD.bound_timesteps(6, bad, 1, 1)


@pytest.mark.parametrize("K", (2, 5, 20))
@pytest.mark.parametrize("c", (0.0, 0.3))
def test_bound_prior_against_brute_force(K, c):
    q = np.full(K, (1.0 - c) / K, dtype=np.float64)
    q[0] += c
    brute = float(sum(v * math.log(v * K) for v in q if v > 0))
    assert abs(MD.bound_prior(c, K) - brute) <= 1e-15 * max(1.0, brute)
    if c == 0.0:
        assert MD.bound_prior(c, K) == 0.0
    assert abs(MD.bound_prior(1.0, K) - math.log(K)) <= 1e-15


def test_bound_rows_packing():
    """2 labels x 3 timesteps x 2 draws on 5 rows: 3 passes, the last padded with 3 idle rows"""
    K, D = 5, 2
    dm = diffusion(K)
    cum = [float(v) for v in dm.cumalphas.double()]
    ts = np.array([[1, 3, 6], [2, 3, 5]])
    passes = MD.bound_rows(ts, D, 5, K, cum, dm.posterior_coeffs, 2)
    assert len(passes) == 3 and all(tab.shape == (5,) and tab.dtype == hip.bound_dtype() and slot.shape == (5,) for tab, slot in passes)
    tab = np.concatenate([t for t, _ in passes])
    slot = np.concatenate([s for _, s in passes])
    assert (slot[:12] == np.arange(12)).all() and (slot[12:] == -1).all() and (tab["t"][12:] == hip.BOUND_IDLE).all()
    want = [(l, m, d) for l in range(2) for m in range(3) for d in range(D)]
    for r, (l, m, d) in zip(tab[:12], want):
        t = int(ts[l, m])
        p_hit, p_miss = U.probabilities(cum[t - 1], K)
        a, c = dm.posterior_coeffs(t)
        assert (r["t"], r["sample"], r["label_row"], r["reserved"]) == (t, l * D + d, l, 0)
        assert (r["p_hit"], r["p_miss"], r["alpha_t"], r["cumalpha_tm1"]) == (p_hit, p_miss, np.float32(a), np.float32(c))
    assert len(MD.bound_rows(ts, D, 12, K, cum, dm.posterior_coeffs)) == 1 and len(MD.bound_rows(ts, D, 1, K, cum, dm.posterior_coeffs)) == 12
    with pytest.raises(ValueError, match="label rows"):
        MD.bound_rows(ts, D, 5, K, cum, dm.posterior_coeffs, 1)             # a label row the label tensor does not have
    for kw in (dict(draws=0), dict(rows=0)):
        with pytest.raises(ValueError, match="bound_rows"):
            MD.bound_rows(ts, **{"draws": D, "rows": 5, **kw}, K=K, cumalphas=cum, coeffs=dm.posterior_coeffs)


def test_label_bound_refusals_name_the_argument():
    model, _ = U.small_model(2)
    model.eval()
    lab, img = torch.zeros((2, 2, U.H, U.W), dtype=torch.int64), torch.zeros((2, 1, U.H, U.W))
    for kw, word in ((dict(draws=0), "draws"), (dict(rows=0), "rows"), (dict(timesteps=[0]), "timesteps"), (dict(timesteps=[7]), "timesteps"),
                     (dict(timesteps=[2, 2]), "timesteps"), (dict(labels=lab[:, :, :-1]), "labels"), (dict(labels=lab[:1]), "labels"),
                     (dict(labels=torch.zeros((2, 3, U.H, U.W))), "labels"), (dict(labels=lab - 1), "labels"),
                     (dict(class_weights=torch.ones(3)), "class_weights")):
        args = dict(labels=lab, condition=img)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            model.label_bound(args.pop("labels"), args.pop("condition"), **args)
    model.rng = "torch_cpu"
    with pytest.raises(ValueError, match="torch_cpu"):
        model.label_bound(lab, img)
    logit_model, _ = U.small_model(2, softmax_output=False)
    with pytest.raises(ValueError, match="softmax_output"):
        logit_model.eval().label_bound(lab, img)
    assert model.bound_call == 0 and model.philox_call == 0                    # a refused call draws nothing


def test_evaluator_label_bound_keys(tmp_path, monkeypatch):
    """a recording stub model: `label_bound: yes` adds the key and writes the JSON; without it the result's keys are today's.  (The
    evaluator's own scores come from the device; here they are stubbed, the bound's plumbing is what is looked at.)"""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    K, H, W, L, batch, Tn = 2, 6, 5, 4, 2, 3
    monkeypatch.setattr(E.M, "calc_batched_generalised_energy_distance", lambda lab, pred, k: (np.zeros(lab.shape[0]),) * 3)
    monkeypatch.setattr(E.M, "batched_hungarian_matching", lambda lab, pred, k: np.zeros(lab.shape[0]))
    rng = np.random.default_rng(3)
    raters = rng.integers(0, K, (3, L, H, W))
    one_hot = lambda idx: torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), K).movedim(-1, -3).float()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, b):
            return torch.full((1, H, W), float(b)), one_hot(raters[b]), np.array([0.25] * 4)

    class Stub:
        step_T_sample = "majority"

        def __init__(self):
            self.bound_calls = []

        def __call__(self, x, image, **kw):
            p = torch.zeros_like(x)                                          # (x_T is drawn from the host generator: not a fixed prediction)
            p[:, 0] = 1.0
            return {"diffusion_out": p}

        def label_bound(self, labels, condition, **kw):
            self.bound_calls.append((labels.clone(), condition.clone(), kw))
            B = labels.shape[0]
            base = condition[:, 0, 0, 0].double()[:, None] + torch.arange(L).double()[None]             # image + rater
            ts = kw["timesteps"] if isinstance(kw["timesteps"], list) else list(range(1, Tn + 1))
            terms = base[..., None] * torch.ones(len(ts)).double()
            return {"bound": base * 10, "bits_per_pixel": base / 4, "terms": terms, "timesteps": torch.tensor(ts).expand(B, L, len(ts)),
                    "prior": base * 0 + 0.5, "pixels": torch.full((B, L), H * W), "complete": not isinstance(kw["timesteps"], list)}

    params = {"dataset_file": "datasets.lidc", "batch_size": batch, "evaluations": [1], "output_path": str(tmp_path / "out")}
    plain_model = Stub()
    plain = E.eval_lidc_uncertainty(dict(params), dataset=DS(), device="cpu", model=plain_model)
    assert plain_model.bound_calls == [] and not (tmp_path / "out").exists()
    stub = Stub()
    res = E.eval_lidc_uncertainty({**params, "evaluation": {"label_bound": True}}, dataset=DS(), device="cpu", model=stub)
    assert set(res) == set(plain) | {"label_bound"}
    for key, value in plain.items():
        assert res[key] == value, key
    assert len(stub.bound_calls) == 2                                          # 3 images in batches of 2: once per batch
    for i, (lab, cond, kw) in enumerate(stub.bound_calls):
        assert torch.equal(lab, torch.from_numpy(raters[2 * i:2 * i + 2])) and kw == {"timesteps": None, "draws": 1}
        assert tuple(cond.shape) == (lab.shape[0], 1, H, W) and cond[:, 0, 0, 0].tolist() == [float(b) for b in range(2 * i, 2 * i + lab.shape[0])]
    got = res["label_bound"]
    assert got["images"] == 3 and got["raters"] == L and got["draws"] == 1 and got["complete"] is True and got["timesteps"] == [1, 2, 3]
    assert got["bound_per_rater"] == [10.0 * (1 + r) for r in range(L)] and got["bits_per_pixel_per_rater"] == [(1 + r) / 4 for r in range(L)]
    assert got["bound"] == 25.0 and got["bits_per_pixel"] == 0.625 and got["prior"] == 0.5 and got["timestep_curve"] == [2.5] * 3
    with open(tmp_path / "out" / "lidc_label_bound.json") as f:
        assert json.load(f) == got == json.loads(json.dumps(got))
    assert sorted(os.listdir(tmp_path / "out")) == ["lidc_label_bound.json"]
    part = Stub()
    got = E.eval_lidc_uncertainty({**params, "evaluation": {"label_bound": True, "label_bound_timesteps": [3, 1], "label_bound_draws": 2},
                                   "output_path": None}, dataset=DS(), device="cpu", model=part)["label_bound"]
    assert part.bound_calls[0][2] == {"timesteps": [3, 1], "draws": 2} and got["draws"] == 2 and got["complete"] is False
    assert got["timesteps"] == [3, 1]
    strat = Stub()
    E.eval_lidc_uncertainty({**params, "evaluation": {"label_bound": True, "label_bound_timesteps": 2}, "output_path": None}, dataset=DS(),
                            device="cpu", model=strat)
    assert strat.bound_calls[0][2] == {"timesteps": 2, "draws": 1}


# ------------------------------------------------------------------------------------------------ GPU: the kernels
@pytest.fixture(scope="module")
def lib():
    return U.load_lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(U.DEV)


def table_dev(tab):
    return dev(tab.view(np.int32).reshape(-1, 8))


def stream():
    return torch.cuda.current_stream(U.DEV).cuda_stream


def random_labels(rng, R, HW, K):
    y = rng.integers(0, K, (R, HW)).astype(np.uint8)
    y[rng.random((R, HW)) < 0.2] = 255
    y[0, :3] = (K, 254, 255)                                                   # any byte >= K is a pixel that is not counted
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("K", (2, 5, 33))
@pytest.mark.parametrize("HW", (77, 1024))
@pytest.mark.parametrize("N", (1, 3))
def test_noise_kernel_equals_restatement(lib, N, HW, K):
    dm = diffusion(K)
    rng = np.random.default_rng(1000 * N + HW + K)
    labels = random_labels(rng, 2, HW, K)
    tab = make_table(dm, K, rows_for(N))
    GUARD = 64
    out = torch.full((N * HW + GUARD,), 255, dtype=torch.uint8, device=U.DEV)
    labels_d, tab_d = dev(labels), table_dev(tab)                              # (held: a temporary's memory is handed out again at once)
    hip.check(lib.ccdm_bound_noise(labels_d.data_ptr(), tab_d.data_ptr(), N, 2, HW, K, U.SEED, out.data_ptr(), stream()), "bound_noise")
    got = out.cpu().numpy()
    assert (got[N * HW:] == 255).all()                                         # the guard tail
    want = noise_restatement(labels, tab, K, U.SEED, dm)
    for n, w in enumerate(want):
        g = got[n * HW:(n + 1) * HW]
        if w is None:
            assert (g == 255).all()                                            # an idle row is not written
            continue
        assert (g == w).all(), (n, int((g != w).sum()))
        y = labels[tab[n]["label_row"]]
        assert (g[y >= K] == np.arange(HW)[y >= K] % K).all()
    if N == 3:
        # t = 1 and t = T of the same map: nearly the label itself, nearly uniform
        y = labels[0]
        assert (got[:HW][y < K] == y[y < K]).mean() > 0.97 and (got[2 * HW:3 * HW][y < K] == y[y < K]).mean() < 1.0 / K + 0.2
    # a label row outside [0, R) never reaches the labels: the row is treated as idle
    bad = tab.copy()
    bad["label_row"][0] = 2
    out.fill_(255)
    bad_d = table_dev(bad)
    hip.check(lib.ccdm_bound_noise(labels_d.data_ptr(), bad_d.data_ptr(), N, 2, HW, K, U.SEED, out.data_ptr(), stream()), "bound_noise")
    assert (out.cpu().numpy()[:HW] == 255).all()


def run_terms(lib, x0, xt, labels, tab, K, weights=None, want_map=True, guard=8):
    N, HW = xt.shape
    nws = lib.ccdm_bound_terms_workspace_bytes(N, HW, K)
    assert nws > 0
    ws = torch.full((nws // 8,), float("nan"), dtype=torch.float64, device=U.DEV)
    rs = torch.full((N + guard,), 7.0, dtype=torch.float64, device=U.DEV)
    rw = torch.full((N + guard,), 7.0, dtype=torch.float64, device=U.DEV)
    mp = torch.full((N * HW + guard,), 7.0, dtype=torch.float32, device=U.DEV)
    keep = (dev(x0), dev(xt.astype(np.uint8)), dev(labels), table_dev(tab), None if weights is None else dev(np.asarray(weights, np.float32)))
    hip.check(lib.ccdm_bound_terms(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                                   None if weights is None else keep[4].data_ptr(), N, labels.shape[0], HW, K, FLOOR, ws.data_ptr(),
                                   rs.data_ptr(), rw.data_ptr(), mp.data_ptr() if want_map else None, stream()), "bound_terms")
    torch.cuda.synchronize()
    for v in (rs, rw, mp):
        assert (v[-guard:] == 7.0).all()                                       # the guard tails
    return rs[:N].cpu(), rw[:N].cpu(), mp[:N * HW].reshape(N, HW).cpu()


# k_bound_terms is built per rung of the class-count ladder (256 pixels per block up to K = 32, 64 above): both ends of every rung.  Above
# K = 33 the short map alone (77 = 64 + 13 pixels): 1024 pixels of up to 255 classes add time and no other path.
TERMS_KS = sorted({2, 5, 20, 33} | set(RUNG_KS))
TERMS_HW_K = [(HW, K) for HW in (77, 1024) for K in TERMS_KS if HW == 77 or K <= 33]
TERMS_MAXIMA = {}          # (K, HW) -> the largest error against float64 seen in this session (parity_log: ladder_bound_terms)


def row_inputs(tab, labels, K):
    """per engine row: the label map it scores (idle rows: all 255, so the restatement gives 0) and its coefficients"""
    y = np.stack([labels[r["label_row"]] if r["t"] >= 1 else np.full(labels.shape[1], 255, np.uint8) for r in tab]).astype(np.int64)
    return y, tab["alpha_t"].copy(), tab["cumalpha_tm1"].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("HW,K", TERMS_HW_K)
@pytest.mark.parametrize("N", (1, 3))
def test_terms_kernel_against_float64(lib, parity_log, N, HW, K):
    dm = diffusion(K)
    rng = np.random.default_rng(2000 * N + HW + K)
    labels = random_labels(rng, 2, HW, K)
    tab = make_table(dm, K, rows_for(N))
    xt = rng.integers(0, K, (N, HW))
    x0 = random_x0(rng, N, HW, K)
    y, a, c = row_inputs(tab, labels, K)
    want = terms_restatement(x0, xt, y, a, c, K)
    rs, rw, mp = run_terms(lib, x0, xt, labels, tab, K)
    err = np.abs(mp.numpy().astype(np.float64) - want)
    print(f"bound_terms N={N} HW={HW} K={K}: max |l - float64| = {err.max():.3e} = {err.max() / 2.0 ** -24:.1f} * 2^-24 (bound {K + 256}), "
          f"largest term {want.max():.3f}")
    TERMS_MAXIMA[(K, HW)] = max(TERMS_MAXIMA.get((K, HW), 0.0), float(err.max()))
    parity_log("ladder_bound_terms", **{f"rung{rung_of(K)}_K{K}_HW{HW}_max_abs_err_vs_float64": TERMS_MAXIMA[(K, HW)], f"K{K}_bound": tol(K)})
    assert err.max() <= tol(K)
    counted = y < K
    assert (mp.numpy()[~counted] == 0).all() and np.array_equal(rw.numpy(), counted.sum(1).astype(np.float64))
    np.testing.assert_allclose(rs.numpy(), mp.double().sum(1).numpy(), rtol=1e-12, atol=0)
    for n, r in enumerate(tab):
        if r["t"] < 1:
            assert rs[n] == 0 and rw[n] == 0 and (mp[n] == 0).all()            # an idle row: sums 0, its map row 0
        if r["t"] == 1:
            # the decoder term: -logf(max(x0_y, floor)) to 1 ulp — logf being the device's fp32 logarithm (torch's fp32 log on the GPU is
            # that function), which is itself not correctly rounded: the distance to the rounded float64 logarithm is printed
            x0y = np.take_along_axis(x0[n], np.where(counted[n], y[n], 0)[:, None], axis=1)[:, 0]
            ref = np.where(counted[n], -torch.log(torch.clamp(dev(x0y), min=FLOOR)).cpu().numpy(), np.float32(0.0)).astype(np.float32)
            exact = np.where(counted[n], -np.log(np.maximum(x0y.astype(np.float64), FLOOR)), 0.0).astype(np.float32)
            ulps = np.abs(mp[n].numpy() - ref) / np.spacing(np.abs(ref))
            worst = int(ulps.argmax())
            print(f"   t = 1 row: {ulps[worst]:.0f} ulp from the device's logf, "
                  f"{(np.abs(mp[n].numpy() - exact) / np.spacing(np.abs(exact))).max():.0f} ulp from the rounded float64 logarithm")
            assert ulps[worst] <= 1, (worst, float(x0y[worst]), float(mp[n, worst]), float(ref[worst]), float(ulps[worst]))
    # two launches: the same bits; without the map the sums are the same
    rs2, rw2, _ = run_terms(lib, x0, xt, labels, tab, K)
    rs3, rw3, _ = run_terms(lib, x0, xt, labels, tab, K, want_map=False)
    assert torch.equal(rs, rs2) and torch.equal(rw, rw2) and torch.equal(rs, rs3) and torch.equal(rw, rw3)


@pytest.mark.gpu
@pytest.mark.parametrize("K", TERMS_KS)
def test_terms_kernel_exact_cases(lib, K):
    """x0 = onehot(y): every term within the tolerance of 0, so the bound of a label under the perfect denoiser is the prior alone;
    class weights with a zero entry: those pixels are out, row_weight is the exact sum of the weights"""
    dm = diffusion(K)
    HW = 77
    rng = np.random.default_rng(50 + K)
    labels = random_labels(rng, 2, HW, K)
    tab = make_table(dm, K, [(t, t, 0) for t in range(1, T_K + 1)] + [None])   # every level of label 0, and an idle row
    N = len(tab)
    y, a, c = row_inputs(tab, labels, K)
    xt = rng.integers(0, K, (N, HW))
    x0 = U.onehot_np(np.where(y < K, y, 0), K).astype(np.float32)
    rs, rw, mp = run_terms(lib, x0, xt, labels, tab, K)
    print(f"bound_terms K={K} x0 = onehot(y): max |l| = {mp.abs().max():.3e} (bound {tol(K):.3e})")
    assert mp.abs().max() <= tol(K)
    pixels = int((labels[0] < K).sum())
    prior = pixels * MD.bound_prior(float(dm.cumalphas.double()[-1]), K)
    assert abs((prior + float(rs.sum())) - prior) <= tol(K) * pixels * T_K
    # weights
    w = np.ones(K, np.float32)
    w[0], w[K - 1] = 0.0, 0.5
    x0 = random_x0(rng, N, HW, K)
    rs, rw, mp = run_terms(lib, x0, xt, labels, tab, K, weights=w)
    want = terms_restatement(x0, xt, y, a, c, K, weights=w)
    assert np.abs(mp.numpy() - want).max() <= tol(K)
    out = (y >= K) | (y == 0)
    assert (mp.numpy()[out] == 0).all() and (mp.numpy()[~out] != 0).any()
    assert np.array_equal(rw.numpy(), np.where(y < K, w[np.where(y < K, y, 0)], 0).astype(np.float64).sum(1))
    np.testing.assert_allclose(rs.numpy(), mp.double().sum(1).numpy(), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.fixture(scope="module", params=(2, 5))
def bound_case(request):
    """the small model (K = 2: fused head; K = 5: general epilogue), labels [2,2,H,W] with a 255 region, one label_bound call with every
    timestep and two draws, and its restatement from tested pieces — computed once, shared, left unchanged"""
    K = request.param
    s = U.make_sampler(K)
    model = s["model"]
    model.philox_seed, model.philox_advance, model.bound_call = 99, False, 0
    rng = np.random.default_rng(60 + K)
    B, L, D, T, HW = 2, 2, 2, U.T_SMALL, U.H * U.W
    labels = rng.integers(0, K, (B, L, U.H, U.W))
    labels[1, 0, 4:9, :] = 255
    image = s["image"][:B]
    got = model.label_bound(torch.from_numpy(labels), image, return_map=True, draws=D, rows=8)
    # the restatement: x_t from the race, x0 from forward_step, the terms in float64
    dm = model.diffusion
    triples = [(l, t, d) for l in range(B * L) for t in range(1, T + 1) for d in range(D)]
    tab = make_table(dm, K, [(t, l * D + d, l) for l, t, d in triples])
    flat = labels.reshape(B * L, HW).astype(np.uint8)
    xt = np.stack(noise_restatement(flat, tab, K, 99, dm))
    x_oh = torch.from_numpy(U.onehot_np(xt, K).astype(np.float32)).permute(0, 2, 1).reshape(-1, K, U.H, U.W)
    rows_image = image[torch.tensor([l // L for l, _, _ in triples])]
    t_rows = torch.tensor([t for _, t, _ in triples])
    x0 = model.forward_step(x_oh.to(U.DEV), rows_image, None, t_rows)["diffusion_out"].permute(0, 2, 3, 1).reshape(-1, HW, K).cpu().numpy()
    y, a, c = row_inputs(tab, flat, K)
    per_pixel = terms_restatement(x0, xt, y, a, c, K).reshape(B, L, T, D, HW)
    return dict(K=K, model=model, labels=labels, image=image, got=got, per_pixel=per_pixel, D=D)


@pytest.mark.gpu
def test_label_bound_end_to_end(bound_case):
    c = bound_case
    K, got, pp, model = c["K"], c["got"], c["per_pixel"], c["model"]
    B, L, T, D, HW = pp.shape
    assert got["bound"].dtype == torch.float64 and tuple(got["terms"].shape) == (B, L, T) and got["complete"] is True
    assert torch.equal(got["timesteps"].cpu(), torch.arange(1, T + 1).expand(B, L, T))
    pixels = (c["labels"] < K).reshape(B, L, HW).sum(-1)
    assert np.array_equal(got["pixels"].cpu().numpy(), pixels) and pixels[1, 0] == HW - 5 * U.W and pixels[0, 0] == HW
    terms = got["terms"].cpu().numpy()
    err = np.abs(terms - pp.sum(-1).mean(-1))
    print(f"label_bound K={K}: terms {terms[0, 0]} max |terms - float64| = {err.max():.3e} (bound {tol(K) * HW:.3e})")
    assert (err <= tol(K) * pixels[..., None]).all()
    prior = pixels * MD.bound_prior(float(model.diffusion.cumalphas.double()[-1]), K)
    np.testing.assert_allclose(got["prior"].cpu().numpy(), prior, rtol=1e-12)
    np.testing.assert_allclose(got["bound"].cpu().numpy(), got["prior"].cpu().numpy() + terms.sum(-1), rtol=1e-12)
    np.testing.assert_allclose(got["bits_per_pixel"].cpu().numpy(), got["bound"].cpu().numpy() / (pixels * math.log(2.0)), rtol=1e-12)
    surprise = got["surprise"].cpu().numpy().reshape(B, L, HW)
    assert got["surprise"].dtype == torch.float32 and tuple(got["surprise"].shape) == (B, L, U.H, U.W)
    serr = np.abs(surprise - pp.mean(3).sum(2))
    print(f"label_bound K={K}: max |surprise - float64| = {serr.max():.3e} (bound {tol(K) * T:.3e})")
    assert (serr <= tol(K) * T + T * D * 2.0 ** -33 + 29 * T * 2.0 ** -24).all()          # the terms, the fixed point, the fp32 result
    assert (surprise[1, 0].reshape(U.H, U.W)[4:9] == 0).all()
    # the bound is not vacuous and not absurd: a random network knows nothing, so it pays about log K per pixel and level on top of the prior
    assert (got["bound"] > got["prior"]).all() and (got["bits_per_pixel"] < 64 * T).all()


@pytest.mark.gpu
def test_label_bound_does_not_depend_on_packing_or_repeat(bound_case):
    c = bound_case
    model, lab, image = c["model"], torch.from_numpy(c["labels"]), c["image"]
    for rows in (3, 8):
        again = model.label_bound(lab, image, return_map=True, draws=c["D"], rows=rows)
        for k, v in c["got"].items():
            assert torch.equal(v, again[k]) if isinstance(v, torch.Tensor) else v == again[k], (rows, k)
    # [B,H,W] labels and one-hot labels are the same call as their [B,1,H,W] index maps; a partial sum says so
    one = model.label_bound(lab[:, 0], image, timesteps=[2, 5])
    hot = model.label_bound(torch.nn.functional.one_hot(lab[:, :1].clamp(max=c["K"] - 1), c["K"]).movedim(-1, 2).float(), image, timesteps=[2, 5])
    assert one["complete"] is False and tuple(one["bound"].shape) == (2, 1)
    full = (lab[:, 0] < c["K"]).reshape(2, -1).all(1)                          # (the one-hot form cannot say "not counted")
    assert torch.equal(one["terms"][full], hot["terms"][full])
    assert tuple(one["terms"].shape) == (2, 1, 2)


@pytest.mark.gpu
def test_label_bound_streams_do_not_interfere(bound_case):
    c = bound_case
    model, lab, image, K = c["model"], torch.from_numpy(c["labels"]), c["image"], c["K"]
    x = O.one_hot_bchw(torch.from_numpy(np.random.default_rng(5).integers(0, K, (2, U.H, U.W))), K).to(U.DEV)
    try:
        model.philox_advance, model.philox_call, model.bound_call = True, 0, 0
        a1 = model(x, image)["diffusion_out"].clone()
        a2 = model(x, image)["diffusion_out"].clone()
        model.philox_call = 0
        b1 = model(x, image)["diffusion_out"].clone()
        first = model.label_bound(lab, image, timesteps=[1, 3, 6])
        assert model.philox_call == 1 and model.bound_call == 1
        b2 = model(x, image)["diffusion_out"].clone()
        assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)
        second = model.label_bound(lab, image, timesteps=[1, 3, 6])
        assert model.bound_call == 2 and not torch.equal(first["terms"], second["terms"])
        model.bound_call = 0
        replay = model.label_bound(lab, image, timesteps=[1, 3, 6])
        assert torch.equal(first["terms"], replay["terms"]) and torch.equal(first["bound"], replay["bound"])
    finally:
        model.philox_advance, model.philox_call, model.bound_call = False, 0, 0


@pytest.mark.gpu
def test_stratified_estimator_averages_to_the_full_sum(bound_case):
    """timesteps = 3 strata over 64 keys against the full sum (16 draws, so its own noise is small beside one estimate's): within 4
    standard errors of the 64 estimates, per label.  The keys are bound_call = 0..63 of one seed: deterministic."""
    c = bound_case
    model, lab, image = c["model"], torch.from_numpy(c["labels"]), c["image"]
    try:
        model.philox_advance, model.bound_call = False, 1000
        full = model.label_bound(lab, image, draws=16)["bound"].cpu().numpy()
        est = []
        for call in range(64):
            model.bound_call = call
            r = model.label_bound(lab, image, timesteps=3)
            assert r["complete"] is True and tuple(r["terms"].shape) == (2, 2, 3)
            est.append(r["bound"].cpu().numpy())
        est = np.stack(est)
        mean, se = est.mean(0), est.std(0, ddof=1) / np.sqrt(len(est))
        print(f"stratified K={c['K']}: full {full.ravel()} mean {mean.ravel()} se {se.ravel()} z {((mean - full) / se).ravel()}")
        assert (se > 0).all() and (np.abs(mean - full) <= 4 * se).all()
    finally:
        model.bound_call = 0
