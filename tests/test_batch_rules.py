"""The launch rules that read the batch size, held to equal bits on both sides of their thresholds (run with `-m gpu` on an MI355X).

A sample's output must not depend on how many samples share the launch: multi-GPU sharding, the sampling queue and every "a shard
reproduces its slice" assertion rest on it.  Two rules of the hot path still look at N (the other two, the 8-wave attention blocks and
ctb of ccdm_upconv.hip, have their tests in tests/test_hip_parity.py):

  * the general conv kernel computes TWO 32-channel output tiles per block from one staged halo (k_conv<..., NI = 2>: another B-fragment
    slab layout, another statistics exchange, narrow instead of wide chunks for a fused 1x1 skip) exactly when the padded tile count is
    even and N * slices * (ntiles / 2) >= 512 — which no BASELINE network reaches on LIDC and only C4's 64x128 level reaches at N = 16;
  * the LDS-free 1x1 kernel without output statistics walks ntb = (N * blocks * tiles + 256) / 512 output tiles per block
    (k_conv1x1_multi: a double-buffered walk with three exits).

Each test asks ccdm_conv_plan which variant a call runs BEFORE launching (a changed rule fails loudly instead of testing nothing), runs
the batch on the far side of the threshold, the same samples alone on the near side, and requires torch.equal outputs and statistics
partials; two samples of the batch are held to the float64 operator at the project's bars for these input distributions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from tests import plan_util as PU  # noqa: E402
from tests.test_hip_parity import assert_group_stats, rnd  # noqa: E402

F16X3, F32 = hip.PREC_F16X3, hip.PREC_F32
PREC_NAME = {F16X3: "f16x3", F32: "f32"}
MAXIMA = {}          # family -> largest error against float64 seen in this session (parity_log: batch_rules_*)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from tests import hip_util
    hip.load()
    return hip_util


def record(parity_log, family, case, err, bar):
    MAXIMA[family] = max(MAXIMA.get(family, 0.0), err)
    parity_log("batch_rules_" + family, **{case: err, "bar_" + ("fused_skip_or_groupnorm_1x1" if bar == 3e-5 else "plain"): bar},
               max_abs_err_vs_float64=MAXIMA[family])


# ------------------------------------------------------------------------------------------ general conv: NI = 1 against NI = 2
# operands of one conv call; c0 / c1: the (concatenated) input, skip: channel counts of the fused 1x1 skip sources
CONV_CASES = {
    "in_layers": dict(c0=64, cout=64, gn=1, act=1, emb=1),                    # ResBlock.in_layers: 3x3 GN + SiLU + emb
    "out_layers_residual": dict(c0=64, cout=64, gn=1, act=1, resid=1),        # out_layers + identity residual
    "concat_seam": dict(c0=64, c1=32, cout=64, gn=1, act=1, emb=1),           # decoder: 96 channels, 3 per group across the seam
    "concat_seam_64": dict(c0=64, c1=64, cout=64, gn=1, act=1, emb=1),        # the seam the exact-fp32 chunks (32 channels) allow
    "film": dict(c0=64, cout=64, gn=1, act=1, film=1),                        # use_scale_shift_norm
    "fused_skip": dict(c0=64, cout=64, gn=1, act=1, skip=(64, 64)),           # 1x1 skip of two sources: wide chunks at NI = 1, narrow at NI = 2
    "concat_1x1": dict(c0=64, c1=32, cout=64, k=1),                           # the concat keeps a 1x1 on the general kernel
    "upsample_on_load": dict(c0=32, cout=64, up=1, gn=1, act=1, emb=1),       # up = 1 from half the size
    "raw_16_to_128": dict(c0=16, cout=128),                                   # no GroupNorm, no activation, four n-tiles
    "cout_40": dict(c0=64, cout=40, gn=1, act=1, emb=1),                      # second tile: 8 real channels
    "cout_160": dict(c0=64, cout=160, gn=1, act=1, emb=1),                    # 5 tiles padded to 8
    "cout_96": dict(c0=64, cout=96, gn=1, act=1, emb=1),                      # 3 tiles (odd): the control, NI = 1 at any N
}
F16X3_CASES = [c for c in CONV_CASES if c != "concat_seam_64"]
F32_CASES = ["in_layers", "out_layers_residual", "fused_skip", "concat_seam_64"]


class ConvOperands:
    """One conv call's tensors, on the host in BCHW (for the float64 operator) and on the device in NHWC, in the input distributions of
    test_conv (and of test_conv_with_fused_skip for the ResBlock tail with a fused skip: skip weights of another magnitude)."""

    def __init__(self, U, name, N, H, W, seed, **over):
        c = dict(c0=0, c1=0, cout=0, k=3, up=0, gn=0, act=0, emb=0, film=0, resid=0, skip=(), fine=0)
        c.update(CONV_CASES[name] if name in CONV_CASES else {})
        c.update(over)
        self.__dict__.update(c)
        self.N, self.H, self.W = N, H, W
        self.hin, self.win = (H // 2, W // 2) if self.up else (H, W)
        rng = np.random.default_rng(seed)
        cin, cout, k = self.c0 + self.c1, self.cout, self.k
        self.xa = rnd(rng, N, self.c0, self.hin, self.win) * 1.2 if self.skip else rnd(rng, N, self.c0, self.hin, self.win) * 1.5 + 0.3
        self.xb = rnd(rng, N, self.c1, self.hin, self.win) * 0.7 - 0.2 if self.c1 else None
        self.w = rnd(rng, cout, cin, k, k) / np.sqrt(cin * k * k)
        self.b = rnd(rng, cout, scale=0.1)
        self.gamma, self.beta = 1 + rnd(rng, cin, scale=0.1), rnd(rng, cin, scale=0.1)
        self.embt = rnd(rng, N, cout) if self.emb else None
        # FiLM rows (scale | shift): 1 + scale stays near one, so the staged activations keep the magnitude the bars were set for
        self.filmt = rnd(rng, N, 2 * cin, scale=0.3) if self.film else None
        self.res = rnd(rng, N, cout, H, W) if self.resid else None
        if self.skip:
            self.sa = rnd(rng, N, self.skip[0], H, W) * 1.5 + 0.2
            self.sb = rnd(rng, N, self.skip[1], H, W) * 0.8
            self.ws = rnd(rng, cout, sum(self.skip), 1, 1) / np.sqrt(sum(self.skip)) * 3.0
            self.bs = rnd(rng, cout, scale=0.1)
        self.U = U
        self.srcs = [U.nhwc(self.xa)] + ([U.nhwc(self.xb)] if self.c1 else [])
        self.stats = [U.gn_stats(s, 3) for s in self.srcs] if self.gn else None          # the producers' partials, computed once for the batch
        self.res_d = U.nhwc(self.res) if self.resid else None
        self.skip_d = [U.nhwc(self.sa), U.nhwc(self.sb)] if self.skip else None

    def plan(self, N, prec, **kw):
        """the launch plan of this call for a batch of N, from shapes alone (nothing is launched)"""
        return PU.plan(N, self.hin, self.win, self.c0, self.cout, self.k, c1=self.c1, up=self.up, gn=bool(self.gn),
                       act=hip.ACT_SILU if self.act else hip.ACT_NONE, emb=bool(self.emb), film=bool(self.film), resid=bool(self.resid),
                       skip=self.skip, prec=prec, fine=kw.get("fine", self.fine))

    def launch(self, prec, first=0, fine=None):
        """the call on samples [first, N): every per-sample operand sliced as test_conv_few_pixel_kernel slices them.  Returns
        (out, statistics partials, the plan of the launched argument struct)."""
        U, n, sl = self.U, self.N - first, slice(first, None)
        plan = {}
        out, ost = U.conv2d([s[sl].contiguous() for s in self.srcs], self.w.numpy(), self.b.numpy(), self.k,
                            stats=[s[sl] for s in self.stats] if self.gn else None, gamma=self.gamma.numpy(), beta=self.beta.numpy(),
                            act=hip.ACT_SILU if self.act else hip.ACT_NONE, up=bool(self.up),
                            emb=self.embt[sl].numpy() if self.emb else None, film=self.filmt[sl].numpy() if self.film else None,
                            emb_rows=np.arange(n) if (self.emb or self.film) else None,
                            resid=self.res_d[sl].contiguous() if self.resid else None,
                            skip=([s[sl].contiguous() for s in self.skip_d], self.ws.numpy(), self.bs.numpy()) if self.skip else None,
                            prec=prec, fine=self.fine if fine is None else fine, plan=plan)
        return out, ost, plan

    def float64(self, idx):
        """the operator on samples `idx` in float64 (F.group_norm / F.silu / F.conv2d on .double() inputs)"""
        x = torch.cat([self.xa[idx], self.xb[idx]], 1) if self.c1 else self.xa[idx]
        cin = x.shape[1]
        h = x.double()
        if self.gn:
            h = F.group_norm(h, 32, self.gamma.double(), self.beta.double(), 1e-5)
        if self.film:
            t = self.filmt[idx].double()
            h = h * (1 + t[:, :cin, None, None]) + t[:, cin:, None, None]
        if self.act:
            h = F.silu(h)
        if self.up:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
        ref = F.conv2d(h, self.w.double(), self.b.double(), padding=self.k // 2)
        if self.emb:
            ref = ref + self.embt[idx].double()[:, :, None, None]
        if self.resid:
            ref = ref + self.res[idx].double()
        if self.skip:
            ref = ref + F.conv2d(torch.cat([self.sa[idx], self.sb[idx]], 1).double(), self.ws.double(), self.bs.double())
        return ref


def check_both_sides(U, op, prec, ni_batch, parity_log, family, case, shard=3, fine=None):
    """The batch (NI = ni_batch per the plan), twice; its last `shard` samples alone (NI = 1 per the plan): outputs and statistics partials
    torch.equal.  Samples 0 and N - 1 of the batch against float64, and the group statistics a consumer forms from their partials."""
    N = op.N
    kw = {} if fine is None else dict(fine=fine)
    pre, pre_shard = op.plan(N, prec, **kw), op.plan(shard, prec, **kw)
    assert pre["kernel"] == pre_shard["kernel"] == hip.CONV_KERNEL_GENERAL and pre["tile_w"] == pre_shard["tile_w"] == 32, (pre, pre_shard)
    assert (pre["ntiles_per_block"], pre_shard["ntiles_per_block"]) == (ni_batch, 1), (pre, pre_shard)
    assert pre["slices"] == pre_shard["slices"] and pre["chunk"] == pre_shard["chunk"] == (32 if prec == F32 else 16)
    if op.skip:           # crossing the threshold also moves the fused skip from 32-channel core-only chunks to 16-channel halo chunks
        assert (pre_shard["skip_wide"], pre["skip_wide"]) == ((1, 1 if ni_batch == 1 else 0) if prec == F16X3 else (0, 0))
    out, ost, ran = op.launch(prec, fine=fine)
    assert ran == pre, (ran, pre)
    again, ost2, _ = op.launch(prec, fine=fine)
    assert torch.equal(out, again) and torch.equal(ost, ost2), "run-to-run nondeterminism"
    part, pst, ran_shard = op.launch(prec, first=N - shard, fine=fine)
    assert ran_shard == pre_shard, (ran_shard, pre_shard)
    assert torch.equal(part, out[N - shard:]), f"outputs differ between NI = {ni_batch} and NI = 1: max |d| = {(part - out[N - shard:]).abs().max().item():.3e}"
    assert torch.equal(pst, ost[N - shard:]), "statistics partials differ between the two variants"
    idx = [0, N - 1]
    got = U.bchw(out[idx]).double()
    err = (got - op.float64(idx)).abs().max().item()
    bar = 3e-5 if op.skip else 2e-5
    record(parity_log, family, case, err, bar)
    assert err <= bar, f"max |out - float64| = {err:.3e} (bar {bar:g})"
    assert_group_stats(got, ost[idx].cpu().sum(1))
    return out, ost


@pytest.mark.parametrize("H,W", PU.NI_GEOMETRIES, ids=lambda v: str(v))
@pytest.mark.parametrize("prec,name", [(F16X3, c) for c in F16X3_CASES] + [(F32, c) for c in F32_CASES],
                         ids=lambda v: PREC_NAME.get(v, v) if isinstance(v, int) else v)
def test_two_n_tiles_per_block_is_bit_neutral(U, parity_log, prec, name, H, W):
    """k_conv<..., NI = 2> against k_conv<..., NI = 1> on the same samples: the batch at the smallest N the plan gives two n-tiles per block
    for (22 for two tiles, 11 for four, 6 for the five tiles of Cout = 160 padded to eight; 22 with NI = 1 on both sides for the odd
    control), its last three samples alone.  48x128 tiles exactly, 44x100 is ragged in both directions (no unmasked core)."""
    cout = CONV_CASES[name]["cout"]
    n2, _ = PU.NI_OF_COUT[cout]
    N = n2 or 22
    op = ConvOperands(U, name, N, H, W, seed=1000 * H + cout + len(name))
    check_both_sides(U, op, prec, 2 if n2 else 1, parity_log, "conv_" + PREC_NAME[prec], f"{name}_{H}x{W}")


def test_two_n_tiles_per_block_under_latency_slicing(U, parity_log):
    """32 -> 64 at 128x128, N = 8: fine_slices = 2 gives 64 one-tile slices, so 8 * 64 * 1 = 512 blocks of two n-tiles, where the default
    slicing (12 slices) runs one n-tile per block — outputs torch.equal (test_conv_latency_slicing asserts the pair at N = 2, where both
    run NI = 1), the 64 partials add up to the 12; within the mode, the last three samples alone (NI = 1) give equal bits."""
    N = 8
    op = ConvOperands(U, "latency", N, 128, 128, seed=8128, c0=32, cout=64)
    dflt = op.plan(N, F16X3, fine=0)
    assert (dflt["ntiles_per_block"], dflt["slices"]) == (1, 12)
    fine, fst = check_both_sides(U, op, F16X3, 2, parity_log, "conv_f16x3", "latency_slicing_128x128", fine=2)
    base, bst, ran = op.launch(F16X3, fine=0)
    assert ran == dflt and fst.shape[1] == 64 and bst.shape[1] == 12
    assert torch.equal(base, fine), f"fine_slices = 2 (NI = 2) against the default slicing (NI = 1): max |d| = {(base - fine).abs().max().item():.3e}"
    np.testing.assert_allclose(fst.sum(1).cpu().numpy(), bst.sum(1).cpu().numpy(), rtol=1e-6, atol=1e-3)


# ------------------------------------------------------------------------------------------ LDS-free 1x1: the n-tile walk
# (case of PU.CONV1X1_MULTI_CASES, GroupNorm on load, residual).  GroupNorm(32, C) needs C % 32 == 0, so the one-k-step case (C0 = 16)
# has no GroupNorm form: the launcher refuses it (tests/test_host_logic.py asserts the refusal).
MULTI_RUNS = [(i, gn, 0) for i, c in enumerate(PU.CONV1X1_MULTI_CASES) for gn in (0, 1) if not (gn and c[0] % 32)] + [(1, 0, 1), (0, 1, 1)]


@pytest.mark.parametrize("i,gn,resid", MULTI_RUNS,
                         ids=["-".join(map(str, PU.CONV1X1_MULTI_CASES[i])) + ("-gn" if gn else "") + ("-resid" if r else "") for i, gn, r in MULTI_RUNS])
def test_1x1_n_tile_walk_is_bit_neutral(U, parity_log, i, gn, resid):
    """k_conv1x1_multi<GN> (no output statistics) at the walk's exits — an odd ntb with a ragged last group (5, 5, 2), a last group of
    one, groups of 5 and 4, ntb = every tile of the layer, one k-step: torch.equal to the general kernel on the same call
    (CCDM_DIAG_GENERAL_KERNEL) and, for the last two samples run alone (the one-tile kernel), to their slice of the batch; samples 0 and
    N - 1 against float64 at the bars of test_plain_1x1_conv_kernel (2e-5) and test_norm_qkv_1x1_conv_kernel (3e-5 with GroupNorm)."""
    c0, cout, H, W, N, ntb = PU.CONV1X1_MULTI_CASES[i]
    if N is None:
        N = PU.smallest_batch_with_ntb(c0, cout, H, W, ntb)
    pre = PU.plan(N, H, W, c0, cout, 1, gn=bool(gn), resid=bool(resid), want_stats=False)
    pre2 = PU.plan(2, H, W, c0, cout, 1, gn=bool(gn), resid=bool(resid), want_stats=False)
    assert (pre["kernel"], pre["ntiles_per_block"]) == (hip.CONV_KERNEL_1X1_MULTI, ntb), pre
    assert (pre2["kernel"], pre2["ntiles_per_block"]) == (hip.CONV_KERNEL_1X1, 1), pre2
    rng = np.random.default_rng(c0 + cout + H + N + 7 * gn + resid)
    x = rnd(rng, N, c0, H, W) * 1.7 - 0.4 if gn else rnd(rng, N, c0, H, W) * 1.4 + 0.1
    w = rnd(rng, cout, c0, 1, 1) / np.sqrt(c0)
    b = rnd(rng, cout, scale=0.1)
    g, be = 1 + rnd(rng, c0, scale=0.2), rnd(rng, c0, scale=0.2)
    res = rnd(rng, N, cout, H, W) if resid else None
    xs, rs = U.nhwc(x), (U.nhwc(res) if resid else None)
    st = U.gn_stats(xs, 4) if gn else None

    def launch(first=0, diag=0):
        plan = {}
        out, _ = U.conv2d([xs[first:].contiguous()], w.numpy(), b.numpy(), 1, stats=[st[first:]] if gn else None, gamma=g.numpy(), beta=be.numpy(),
                          resid=rs[first:].contiguous() if resid else None, prec=F16X3, want_stats=False, diag=diag, plan=plan)
        return out, plan
    out, ran = launch()
    assert ran == pre, (ran, pre)
    gen, ran_gen = launch(diag=hip.DIAG_GENERAL_KERNEL)
    assert ran_gen["kernel"] == hip.CONV_KERNEL_GENERAL
    assert torch.equal(out, gen), f"the walk against the general kernel: max |d| = {(out - gen).abs().max().item():.3e}"
    again, _ = launch()
    assert torch.equal(out, again), "run-to-run nondeterminism"
    two, ran2 = launch(first=N - 2)
    assert ran2 == pre2, (ran2, pre2)
    assert torch.equal(two, out[N - 2:]), f"ntb = {ntb} against the one-tile kernel: max |d| = {(two - out[N - 2:]).abs().max().item():.3e}"
    idx = [0, N - 1]
    h = x[idx].double()
    if gn:
        h = F.group_norm(h, 32, g.double(), be.double(), 1e-5)
    ref = F.conv2d(h, w.double(), b.double()) + (res[idx].double() if resid else 0)
    err = (U.bchw(out[idx]).double() - ref).abs().max().item()
    bar = 3e-5 if gn else 2e-5
    record(parity_log, "conv1x1_multi", "-".join(map(str, (c0, cout, H, W, N))) + ("_gn" if gn else "") + ("_resid" if resid else ""), err, bar)
    assert err <= bar, f"max |out - float64| = {err:.3e} (bar {bar:g})"
