"""The sampling queue: continuous batching (serving.SamplingQueue) on the per-slot fused step kernel ccdm_slots_step (include/ccdm_hip.h has
the definition).  The scheduling decisions are pure functions and are checked on the CPU against a schedule derived by hand; the kernel is
held bit for bit against ccdm_shaped_step at (1, 1), one call per slot, and against the evidence tests' restatement of the step built on
the oracle's functions; the queue is held to its contract: whatever the arrival schedule and whatever else is in flight, a request's result
is torch.equal to its solo call."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import SamplingQueue, hip, serving, step_values
from tests.guided_util import bits, coefficients, evidence_restatement, random_inputs, shaped_restatement
from tests.ladder_util import RUNG_KS
from tests.sampler_util import (DEV, H, ROOT, T_SMALL, T_STRIDED, W, assert_symbol_declared_bound_and_built, load_lib, make_sampler, onehot_np,
                                small_model)

SYMBOL = "ccdm_slots_step"
# the four requests of the scheduler test and of the end-to-end test: (name, n, t, vote, the tick before which it arrives)
REQUESTS = [("A", 3, None, None, 0), ("B", 2, int(T_STRIDED), None, 1), ("C", 1, 3, "confidence", 2), ("D", 5, None, None, 2)]
CAPACITY = 4
TICKS, BUSY = 18, 59          # test_scheduler_on_four_requests derives them


# ------------------------------------------------------------------------------------------------ CPU
def test_slots_symbol_declared_bound_and_built():
    """hip.py binds the symbol with argtypes that match the header's declaration (11 arguments), ccdm_guided.hip defines it and the
    library cross-built from it exports it under the unchanged ABI number; the ctypes row and the numpy row have the header's size (32
    bytes) and field order, by the C compiler's layout; every bad argument is refused before anything is launched (host pointers: a
    launch would fault)."""
    lib = assert_symbol_declared_bound_and_built(SYMBOL, 11, "ccdm_guided.hip")
    fields = ["alpha_t", "cumalpha_tm1", "mode", "step_row", "key_lo", "key_hi", "sample", "reserved"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ccdm_hip.h"\nint main(){ printf("%zu %d", sizeof(ccdm_slot_row), CCDM_SLOT_IDLE);\n' + \
          "".join(f'printf(" %zu", offsetof(ccdm_slot_row, {f}));\n' for f in fields) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    R = hip.SlotRow
    assert out == [32, hip.SLOT_IDLE] + [getattr(R, f).offset for f in fields] == [32, -1, 0, 4, 8, 12, 16, 20, 24, 28]
    assert C.sizeof(R) == 32 and [f for f, _ in R._fields_] == fields
    assert serving.SLOT_DTYPE.itemsize == 32 and list(serving.SLOT_DTYPE.names) == fields
    assert [serving.SLOT_DTYPE.fields[f][1] for f in fields] == out[2:]
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    good = dict(x0=p, table=p, N=1, HW=4, K=2, xt=p, xin=p, xin_stride=4, out_probs=p, out_onehot=p, stream=None)
    for change, word in ((dict(x0=None), "null"), (dict(table=None), "null"), (dict(xt=None), "null"), (dict(N=0), "shape"), (dict(HW=0), "shape"),
                         (dict(K=0), "K="), (dict(K=256), "K="), (dict(xin_stride=1), "xin_stride"), (dict(N=1 << 16, HW=1 << 16), "pixels"),
                         (dict(table=p + 1), "table")):
        assert getattr(lib, SYMBOL)(*dict(good, **change).values()) < 0, change
        assert word in hip.last_error(), (change, hip.last_error())


def expected_walk(model, t, vote):
    """step_values / posterior_coeffs / the vote's mode, formed here without the module under test"""
    vote = model.step_T_sample if vote is None else vote
    last = hip.STEP_LAST_MAJORITY if vote == "majority" else hip.STEP_LAST_CONFIDENCE if vote == "confidence" else hip.STEP_LAST_KEEP
    return [(T_SMALL - tv, *model.diffusion.posterior_coeffs(tv), hip.STEP_SAMPLE if tv > 1 else last) for tv in step_values(T_SMALL, t)]


def test_scheduler_on_four_requests():
    """Capacity 4; A (3 samples, 6 rows) before tick 0, B (2, strided: 4 rows) before tick 1, C (1, t = 3: 3 rows, confidence) and D (5, 6
    rows) before tick 2.  By hand:
      tick 0     A0 A1 A2 -> slots 0 1 2; slot 3 idle
      tick 1     B0 -> slot 3 (B1 waits)
      ticks 2-3  full: B1, C0, D0 .. D4 wait
      tick 4     B0 runs its 4th row and leaves slot 3
      tick 5     B1 -> slot 3; A0 A1 A2 run their 6th row and leave slots 0 1 2
      tick 6     C0 D0 D1 -> slots 0 1 2
      tick 8     C0 (3rd row) and B1 (4th row) leave slots 0 and 3
      tick 9     D2 D3 -> slots 0 3
      tick 11    D0 D1 (6th row) leave slots 1 2
      tick 12    D4 -> slot 1; slot 2 idle from here on
      tick 14    D2 D3 leave; ticks 15-17: D4 alone, its 6th row at tick 17
    18 ticks; 3 * 6 + 2 * 4 + 1 * 3 + 5 * 6 = 59 busy slot-steps, 18 * 4 - 59 = 13 idle ones."""
    model, _ = small_model(2)
    walks = {i: serving.plan_walk(T_SMALL, t, vote or model.step_T_sample, model.diffusion.posterior_coeffs)
             for i, (_, n, t, vote, _) in enumerate(REQUESTS)}
    for i, (_, n, t, vote, _) in enumerate(REQUESTS):
        assert walks[i] == expected_walk(model, t, vote)
    assert [len(walks[i]) for i in range(4)] == [6, 4, 3, 6] and walks[2][-1][3] == hip.STEP_LAST_CONFIDENCE and walks[0][-1][3] == hip.STEP_LAST_MAJORITY
    assert [w[0] for w in walks[1]] == [0, 2, 3, 5]          # the strided walk's emb rows: t = 6, 4, 3, 1 in the all-levels table
    keys = {i: 0x1111111122222222 * (i + 1) for i in range(4)}
    sample0 = {i: 100 * i for i in range(4)}
    ticks = serving.simulate(CAPACITY, [(tick, i, n, len(walks[i])) for i, (_, n, _, _, tick) in enumerate(REQUESTS)])
    assert len(ticks) == TICKS and sum(len(active) for _, active, _ in ticks) == BUSY
    assert [(k, a) for k, (a, _, _) in enumerate(ticks) if a] == [
        (0, [(0, 0, 0), (1, 0, 1), (2, 0, 2)]), (1, [(3, 1, 0)]), (5, [(3, 1, 1)]), (6, [(0, 2, 0), (1, 3, 0), (2, 3, 1)]),
        (9, [(0, 3, 2), (3, 3, 3)]), (12, [(1, 3, 4)])]
    # first in, first out
    assert [(r, j) for a, _, _ in ticks for _, r, j in a] == [(i, j) for i, (_, n, _, _, _) in enumerate(REQUESTS) for j in range(n)]
    seen = {}          # (request, sample) -> [(tick, slot, row)]
    for k, (admitted, active, finished) in enumerate(ticks):
        slots = [s for s, _, _, _ in active]
        assert len(set(slots)) == len(slots) and len({(r, j) for _, r, j, _ in active}) == len(active)          # one sample per slot, one slot per sample
        rowmap, table = serving.slot_rows(CAPACITY, active, walks, keys, sample0)
        assert rowmap.dtype == np.int32 and table.dtype == serving.SLOT_DTYPE
        for s in range(CAPACITY):
            if s not in slots:
                assert table[s]["mode"] == hip.SLOT_IDLE and rowmap[s] == 0
        for s, r, j, row in active:
            seen.setdefault((r, j), []).append((k, s, row))
            emb, a, c, mode = walks[r][row]
            assert rowmap[s] == emb and 0 <= emb < T_SMALL
            assert table[s].tolist() == (np.float32(a), np.float32(c), mode, row, keys[r] & 0xFFFFFFFF, keys[r] >> 32, sample0[r] + j, 0)
        assert finished == [(s, r, j) for s, r, j, row in active if row == len(walks[r]) - 1]
        assert all(any(a_[:3] == adm for a_ in active) for adm in admitted)
    for (r, j), runs in seen.items():
        # exactly len(walk) consecutive ticks in one slot, rows 0, 1, 2, ...
        assert [row for _, _, row in runs] == list(range(len(walks[r]))) and len({s for _, s, _ in runs}) == 1
        assert [k for k, _, _ in runs] == list(range(runs[0][0], runs[0][0] + len(runs)))
    assert len(seen) == 11
    # the pure function mutates nothing
    slots0, pending0 = (None, (0, 0, 1)), ((1, 0),)
    out = serving.schedule_tick(slots0, pending0, {0: 2, 1: 1})
    assert (slots0, pending0) == ((None, (0, 0, 1)), ((1, 0),)) and out == ((None, None), (), [(0, 1, 0)], [(0, 1, 0, 0), (1, 0, 0, 1)], [(0, 1, 0), (1, 0, 0)])


def test_queue_refusals():
    """Each names the thing; nothing runs (no engine is built: these pass without a device)."""
    m, _ = small_model(2)
    m.eval()
    shape = (1, H, W)
    with pytest.raises(ValueError, match="capacity"):
        SamplingQueue(m, 0, shape)
    m.rng = "torch_cpu"
    with pytest.raises(ValueError, match="torch_cpu"):
        m.sampling_queue(4, shape)
    m.rng = "philox"
    m.train()
    with pytest.raises(ValueError, match="training"):
        SamplingQueue(m, 4, shape)
    m.eval()
    logits_model, _ = small_model(2, softmax_output=False)
    with pytest.raises(ValueError, match="softmax_output"):
        SamplingQueue(logits_model.eval(), 4, shape)
    fc, _ = small_model(2)
    fc.unet.spec.feature_condition_idx = [1]          # (a throwaway model: the refusal reads this list alone)
    with pytest.raises(ValueError, match="feature_condition.*not built"):
        SamplingQueue(fc.eval(), 4, shape)
    q = m.sampling_queue(4, shape)
    assert isinstance(q, SamplingQueue) and q.stats == dict(ticks=0, busy_slot_steps=0, idle_slot_steps=0, requests_finished=0)
    cond = torch.zeros((2, 1, H, W))
    for kw in serving.GUIDANCE_KEYWORDS:
        with pytest.raises(ValueError, match=kw):
            q.submit(cond, **{kw: 1.0})
    for bad in (torch.zeros((2, 1, H, W + 1)), torch.zeros((2, 2, H, W)), torch.zeros((1, H, W))):
        with pytest.raises(ValueError, match="condition"):
            q.submit(bad)
    with pytest.raises(ValueError, match="x: shape"):
        q.submit(cond, x=torch.zeros((2, 3, H, W)))
    m.train()
    with pytest.raises(ValueError, match="training"):
        q.submit(cond)
    assert m.philox_call == 0 and m._engines == {} and q.idle


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
@pytest.fixture(scope="module")
def lib():
    return load_lib()


MODES = [hip.STEP_SAMPLE, hip.STEP_LAST_CONFIDENCE, hip.SLOT_IDLE, hip.STEP_LAST_MAJORITY, hip.STEP_LAST_KEEP]
SLOT_T = [200, 2, 77, 120, 1]          # the timestep whose coefficients the slot carries (cosine schedule, T = 250)
SLOT_ROW = [3, 249, 9, 0, 17]
SLOT_KEY = [0xFEEDFACE12345678, 0x0123456789ABCDEF, 0x1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF]
SLOT_SAMPLE = [0, 7, 3, 0xFFFFFFFE, 1000]
IDLE = MODES.index(hip.SLOT_IDLE)


def slot_table():
    t = np.zeros(len(MODES), serving.SLOT_DTYPE)
    for n, mode in enumerate(MODES):
        a, c = coefficients(SLOT_T[n])
        t[n] = (a, c, mode, SLOT_ROW[n], SLOT_KEY[n] & 0xFFFFFFFF, SLOT_KEY[n] >> 32, SLOT_SAMPLE[n], 0)
    return t


def slot_buffers(K, HW, stride):
    """Five slots: random x0 rows (positive, normalised), random x_t, and sentinel-filled outputs; the idle slot's x_t is a sentinel too."""
    rng = np.random.default_rng(7000 + 10 * K + HW)
    N = len(MODES)
    x0, _, xt = random_inputs(rng, N, HW, K)
    xt = xt.astype(np.uint8)
    xt[IDLE] = 0xA5
    host = dict(x0=x0, xt=xt, xin=rng.standard_normal((N, HW, stride)).astype(np.float32), probs=np.full((N, HW, K), -7.0, np.float32),
                onehot=np.full((N, HW, K), -7, np.int64))
    return {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}


def run_slots(lib, d, table, with_xin, alias):
    """ccdm_slots_step on copies of the buffers `d`; alias: out_probs IS x0, as in the engine"""
    g = {k: v.clone() for k, v in d.items()}
    N, HW, K = g["x0"].shape
    tab = torch.from_numpy(table.view(np.int32).reshape(N, 8)).to(DEV)
    hip.check(getattr(lib, SYMBOL)(g["x0"].data_ptr(), tab.data_ptr(), N, HW, K, g["xt"].data_ptr(), g["xin"].data_ptr() if with_xin else None,
                                   g["xin"].shape[2], (g["x0"] if alias else g["probs"]).data_ptr(), g["onehot"].data_ptr(), 0), SYMBOL)
    torch.cuda.synchronize()
    return g


def run_shaped_per_slot(lib, d, table, with_xin, alias):
    """The definition: one ccdm_shaped_step call per real slot, N = 1, pointers offset to the slot, at (1.0, 1.0)"""
    g = {k: v.clone() for k, v in d.items()}
    N, HW, K = g["x0"].shape
    stride = g["xin"].shape[2]
    for n in range(N):
        r = table[n]
        if r["mode"] == hip.SLOT_IDLE:
            continue
        x0 = g["x0"].data_ptr() + n * HW * K * 4
        hip.check(lib.ccdm_shaped_step(x0, None, 1, HW, K, 1.0, 1.0, float(r["alpha_t"]), float(r["cumalpha_tm1"]), int(r["mode"]), int(r["step_row"]),
                                       int(r["key_lo"]) | int(r["key_hi"]) << 32, int(r["sample"]), g["xt"].data_ptr() + n * HW,
                                       g["xin"].data_ptr() + n * HW * stride * 4 if with_xin else None, stride,
                                       x0 if alias else g["probs"].data_ptr() + n * HW * K * 4, g["onehot"].data_ptr() + n * HW * K * 8, 0),
                  "ccdm_shaped_step")
    torch.cuda.synchronize()
    return g


SLOT_HW_K = [(195, K) for K in RUNG_KS] + [(256, 2), (256, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("HW,K", SLOT_HW_K)
def test_slots_kernel_equals_the_shaped_step_slot_by_slot(lib, HW, K):
    """Five slots with different coefficients, step rows, keys and sample indices: the four real modes and an idle slot.  HW = 195: blocks
    straddle slot boundaries (K <= 4: 256 threads; K <= 32: 256 staged pixels; K >= 33: 64 staged pixels) and the runs are unaligned, with
    an odd xin stride, at both ends of every rung of the class-count ladder; HW = 256: the aligned vector paths, xin stride a multiple of
    4.  With xin and without, with out_probs a buffer of
    its own and aliased to x0 as in the engine: every buffer is torch.equal to what five ccdm_shaped_step calls at (1.0, 1.0) leave, the
    idle slot's bytes are the fill they started with, the image channels of xin are untouched."""
    stride = (K + 4) // 4 * 4 + 1 if HW == 195 else (K + 3) // 4 * 4
    d = slot_buffers(K, HW, stride)
    table = slot_table()
    for with_xin in (True, False):
        for alias in (False, True):
            got, want = run_slots(lib, d, table, with_xin, alias), run_shaped_per_slot(lib, d, table, with_xin, alias)
            what = f"xin={with_xin} alias={alias}"
            for k in d:
                assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} places"
                assert torch.equal(got[k][IDLE], d[k][IDLE]), f"{what}: the idle slot's {k} changed"
            assert torch.equal(got["xin"][..., K:], d["xin"][..., K:]), what + ": an image channel changed"
            if not with_xin:
                assert torch.equal(got["xin"], d["xin"]), what
            if not alias:
                assert torch.equal(got["x0"], d["x0"]), what
            # the launch did something in every real slot's own way (so the comparison is not of untouched buffers)
            assert not torch.equal(got["xt"][0], d["xt"][0]) and torch.equal(got["xt"][4], d["xt"][4]) and torch.equal(got["xt"][1], d["xt"][1])
            probs = got["x0"] if alias else got["probs"]
            assert bool(((probs[1].sum(-1) - 1).abs() < 1e-5).all()) and bool((got["onehot"][3].sum(-1) == 1).all())
            assert torch.equal(got["onehot"][3].argmax(-1).to(torch.uint8), got["xt"][3])
            if with_xin:
                assert torch.equal(got["xin"][0, :, :K].argmax(-1).to(torch.uint8), got["xt"][0]) and bool((got["xin"][0, :, :K].sum(-1) == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5])
def test_slots_kernel_against_the_cpu_restatement(lib, K):
    """HW = 195, per slot the evidence tests' restatement of the step (the oracle's theta_post_prob, cascade normalisation and
    sample_index on philox_exponential's noise) with all-ones weights and the slot's key, sample and row: the classes are equal (the
    drawn ones and the majority vote), the confidence probabilities lie within the bar the posterior parity test holds this arithmetic to
    (test_hip_parity.test_posterior_matches_oracle_and_reference_golden: rtol 2e-6, atol 1e-9)."""
    HW = 195
    d = slot_buffers(K, HW, K + 1)
    table = slot_table()
    got = {k: v.cpu().numpy() for k, v in run_slots(lib, d, table, True, False).items()}
    x0, xt = d["x0"].cpu().numpy(), d["xt"].cpu().numpy()
    for n, mode in enumerate(MODES):
        if mode in (hip.SLOT_IDLE, hip.STEP_LAST_KEEP):
            continue
        r = table[n]
        probs, idx = evidence_restatement(x0[n:n + 1], np.ones_like(x0[n:n + 1]), xt[n:n + 1], float(r["alpha_t"]), float(r["cumalpha_tm1"]), mode,
                                          int(r["step_row"]), SLOT_KEY[n], SLOT_SAMPLE[n])
        if mode == hip.STEP_LAST_CONFIDENCE:
            np.testing.assert_allclose(got["probs"][n], probs[0], rtol=2e-6, atol=1e-9)
        else:
            assert np.array_equal(got["xt"][n].astype(np.int64), idx[0]), f"slot {n}: {int((got['xt'][n] != idx[0]).sum())} of {HW} classes differ"
        if mode == hip.STEP_LAST_MAJORITY:
            assert np.array_equal(got["onehot"][n].argmax(-1), idx[0])
    assert bits(got["x0"]).tobytes() == bits(x0).tobytes()


ANCHOR_KS = RUNG_KS          # the slot-by-slot definition above is another kernel, held at most of these by the shaped tests' new cases alone


@pytest.mark.gpu
@pytest.mark.parametrize("K", ANCHOR_KS)
def test_slots_kernel_equals_the_cpu_restatement_bit_for_bit(lib, K):
    """HW = 195, one running slot of each step mode, against the shaped tests' numpy restatement at (1, 1) with the slot's coefficients,
    key, sample and row, directly (the slot-by-slot test compares two kernels): the drawn classes and their one-hot in xin, the
    confidence probabilities bit for bit, the majority class and its one-hot; what a mode does not write, the keeping slot and the idle
    slot are the bytes they started with."""
    HW = 195
    d = slot_buffers(K, HW, K + 1)
    table = slot_table()
    got = {k: v.cpu().numpy() for k, v in run_slots(lib, d, table, True, False).items()}
    was = {k: v.cpu().numpy() for k, v in d.items()}
    for n, mode in enumerate(MODES):
        r = table[n]
        sl = slice(n, n + 1)
        wrote = set()
        if mode not in (hip.SLOT_IDLE, hip.STEP_LAST_KEEP):
            probs, idx = shaped_restatement(was["x0"][sl], None, was["xt"][sl], 1.0, 1.0, float(r["alpha_t"]), float(r["cumalpha_tm1"]), mode,
                                            int(r["step_row"]), SLOT_KEY[n], SLOT_SAMPLE[n])
            if mode == hip.STEP_LAST_CONFIDENCE:
                assert np.array_equal(bits(got["probs"][n]), bits(probs[0])), f"slot {n}: {int((bits(got['probs'][n]) != bits(probs[0])).sum())} probabilities differ"
                wrote = {"probs"}
            else:
                assert np.array_equal(got["xt"][n].astype(np.int64), idx[0]), f"slot {n}: {int((got['xt'][n] != idx[0]).sum())} of {HW} classes differ"
                wrote = {"xt", "xin"} if mode == hip.STEP_SAMPLE else {"xt", "onehot"}
            if mode == hip.STEP_SAMPLE:
                assert np.array_equal(got["xin"][n, :, :K], onehot_np(idx, K)[0].astype(np.float32)), n
                assert np.array_equal(bits(got["xin"][n, :, K:]), bits(was["xin"][n, :, K:])), n
            if mode == hip.STEP_LAST_MAJORITY:
                assert np.array_equal(got["onehot"][n], onehot_np(idx, K)[0].astype(np.int64)), n
        for k in set(d) - wrote:
            assert got[k][n].tobytes() == was[k][n].tobytes(), f"slot {n} (mode {mode}): {k} changed"


# ------------------------------------------------------------------------------------------------ GPU: the queue
@pytest.fixture(scope="module", params=[2, 5], ids=["K2-fused-head", "K5-epilogue-xin"])
def sampler(request):
    """The small model, the four requests' inputs and — computed once — each request's solo call: model(x, condition, t=t) with
    philox_call = the request's call index (A: 0 .. D: 3) and step_T_sample = its vote."""
    s = make_sampler(request.param)
    model, K = s["model"], s["K"]
    model.philox_advance = True
    rng = np.random.default_rng(900 + K)
    reqs = {}
    for call, (name, n, t, vote, tick) in enumerate(REQUESTS):
        cond = torch.from_numpy(rng.uniform(-1, 1, (n, 1, H, W)).astype(np.float32)).to(DEV)
        x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, K, (n, H, W))), K).permute(0, 3, 1, 2).float().contiguous().to(DEV)
        reqs[name] = dict(name=name, n=n, t=t, vote=vote, tick=tick, call=call, cond=cond, x=x)
        reqs[name]["solo"] = solo(model, reqs[name])
    s["reqs"] = reqs
    return s


def solo(model, r):
    keep = model.philox_call, model.step_T_sample
    model.philox_call, model.step_T_sample = r["call"], r["vote"] or "majority"
    try:
        return model(r["x"], r["cond"], t=None if r["t"] is None else torch.as_tensor(r["t"]))["diffusion_out"]
    finally:
        model.philox_call, model.step_T_sample = keep


def submit(q, model, r):
    model.philox_call = r["call"]
    return q.submit(r["cond"], x=r["x"], t=r["t"], vote=r["vote"])


def assert_equals_solo(res, r, what=""):
    out = res.result()["diffusion_out"]
    want = r["solo"]
    assert out.dtype == want.dtype and out.shape == want.shape and out.device == want.device, (what, r["name"])
    assert torch.equal(out, want), f"{what} request {r['name']}: {int((out != want).sum())} of {out.numel()} values differ from the solo call"


def run_schedule(q, model, reqs, arrivals):
    """arrivals: {tick: [names]}; submits before that tick, steps one tick at a time, then runs the queue empty"""
    res = {}
    for tick in range(max(arrivals) + 1):
        for name in arrivals.get(tick, []):
            res[name] = submit(q, model, reqs[name])
        q.step()
    q.run_until_idle()
    return res


ARRIVALS = {tick: [name for name, _, _, _, at in REQUESTS if at == tick] for tick in (0, 1, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_every_request_equals_its_solo_call(sampler, use_graph):
    """The four requests on a queue of capacity 4, submitted and stepped as the scheduler test has them: class maps (A, B, D) and the
    confidence probabilities (C) are torch.equal to the solo calls, the form and dtype included; q.stats are the scheduler's counts."""
    model, reqs = sampler["model"], sampler["reqs"]
    model.use_graph = use_graph
    try:
        q = model.sampling_queue(CAPACITY, (1, H, W))
        res = run_schedule(q, model, reqs, ARRIVALS)
        assert all(r.done for r in res.values()) and q.idle
        for name, r in res.items():
            assert_equals_solo(r, reqs[name], f"graph={use_graph}")
        assert reqs["C"]["solo"].dtype == torch.float32 and reqs["A"]["solo"].dtype == torch.int64
        assert q.stats == dict(ticks=TICKS, busy_slot_steps=BUSY, idle_slot_steps=TICKS * CAPACITY - BUSY, requests_finished=4)
        assert [res[n].call for n in "ABCD"] == [0, 1, 2, 3] and not any(k[7] == ("queue", id(q)) for k in model._engines)
    finally:
        model.use_graph = True


@pytest.mark.gpu
def test_another_arrival_order_and_capacity_gives_the_same_results(sampler):
    """The same requests in another order at other ticks, on a queue of capacity 3 (D larger than the queue: admitted piecewise)."""
    model, reqs = sampler["model"], sampler["reqs"]
    q = SamplingQueue(model, 3, (1, H, W))
    res = run_schedule(q, model, reqs, {0: ["D", "C"], 3: ["A"], 4: ["B"]})
    for name, r in res.items():
        assert_equals_solo(r, reqs[name], "reordered")
    assert q.stats["busy_slot_steps"] == BUSY and q.stats["requests_finished"] == 4


@pytest.mark.gpu
def test_two_queues_and_a_plain_call_do_not_disturb_each_other(sampler):
    """Two queues on one model, stepped in turn, and between two ticks a plain model(x, image) call: the call returns what it returns
    alone, and every queued request still equals its solo call."""
    model, reqs = sampler["model"], sampler["reqs"]
    q1, q2 = model.sampling_queue(CAPACITY, (1, H, W)), model.sampling_queue(CAPACITY, (1, H, W))
    assert q1.engine is not q2.engine
    res = {n: submit(q1 if n in "AB" else q2, model, reqs[n]) for n in "ABCD"}
    plain = None
    for tick in range(40):
        q1.step()
        q2.step()
        if tick == 2:
            plain = solo(model, reqs["A"])
    assert q1.idle and q2.idle and torch.equal(plain, reqs["A"]["solo"])
    for name, r in res.items():
        assert_equals_solo(r, reqs[name], "two queues")


@pytest.mark.gpu
def test_result_drives_the_queue_and_a_range_flag_fails_until_reset(sampler):
    """result() before completion drives the queue until the request is done (documented in QueueRequest).  A range flag set by hand on
    the queue's engine makes the next finishing request raise CcdmRangeError, and submit / step refuse until reset(); after it a
    resubmitted request reproduces its solo result.  reset() drops what was in flight."""
    model, reqs = sampler["model"], sampler["reqs"]
    q = model.sampling_queue(CAPACITY, (1, H, W))
    r = submit(q, model, reqs["B"])
    assert not r.done and q.stats["ticks"] == 0
    assert_equals_solo(r, reqs["B"], "driven by result()")
    assert r.done and q.stats["ticks"] == 4          # two samples side by side, four rows each
    eng = q.engine
    with eng.enter():
        eng.flag.fill_(1)
    eng.leave()
    bad = submit(q, model, reqs["C"])
    with pytest.raises(hip.CcdmRangeError):
        bad.result()
    with pytest.raises(hip.CcdmRangeError):
        submit(q, model, reqs["C"])
    dropped = None
    q.reset()
    dropped = submit(q, model, reqs["D"])
    q.step()
    q.reset()
    with pytest.raises(RuntimeError, match="dropped"):
        dropped.result()
    assert q.idle
    for name in "CA":
        assert_equals_solo(submit(q, model, reqs[name]), reqs[name], "after reset")


@pytest.mark.gpu
def test_a_vote_that_keeps_the_state_returns_it_one_hot(sampler):
    """A vote that is neither "majority" nor "confidence" (STEP_LAST_KEEP): the result is x_t turned one-hot in fp32, as the solo call's."""
    model, reqs = sampler["model"], sampler["reqs"]
    r = dict(reqs["B"], vote="keep", name="B-keep")
    r["solo"] = solo(model, r)
    assert r["solo"].dtype == torch.float32 and not torch.equal(r["solo"], reqs["B"]["solo"].float())
    q = model.sampling_queue(CAPACITY, (1, H, W))
    other = submit(q, model, reqs["C"])
    assert_equals_solo(submit(q, model, r), r, "keep")
    assert_equals_solo(other, reqs["C"], "beside keep")


@pytest.mark.gpu
def test_set_tables_restores_the_rowmap_a_queue_changed(sampler):
    """SamplerEngine.set_rows invalidates the tables' key: a plain call on an engine whose rowmap was changed reloads its tables."""
    model, r = sampler["model"], sampler["reqs"]["A"]
    assert torch.equal(solo(model, r), r["solo"])
    eng = model._engine(r["x"], r["cond"], None)
    with eng.enter():
        eng.set_rows(torch.full((eng.N,), 2, dtype=torch.int32))
    eng.leave()
    assert eng._tables_key is None and torch.equal(solo(model, r), r["solo"])
    assert bool((eng.rowmap == 0).all())
