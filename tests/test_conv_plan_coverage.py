"""Every conv launch plan the shipped networks run, against the float64 operator (run with `-m gpu` on an MI355X).

tests/plan_util.PLAN_CASES holds one small case per signature — kernel family, tile geometry, chunk width, tap split, masked or unmasked
core, slice rung, ksize / stride / up, precision, fine_slices and operand set — and tests/test_host_logic.py proves on the CPU that every
signature a shipped network emits is in the table.  Here each case runs at N = 2 on the kernel its signature names:

  * the plan of the argument struct that is launched has the case's signature (a rule change cannot move a case onto another kernel
    without this failing);
  * the output against the float64 operator rounded to fp32, at the per-layer bars of tests/test_hip_parity.py: 2e-5, or 3e-5 where a
    fused 1x1 skip or a GroupNorm-on-load 1x1 adds a second product chain — in both precisions; the measured maximum goes to the
    parity log under the signature;
  * the statistics partials, where the call writes them: the two raw-sum checks of test_conv and assert_group_stats at 2e-6;
  * the specialised families against the general kernel on the same call (CCDM_DIAG_GENERAL_KERNEL): ccdm_upconv and ccdm_conv1x1 bit
    for bit, ccdm_conv_ks to the 8e-6 of test_conv_few_pixel_kernel;
  * a second run gives equal bits, and the last sample run alone equals its slice of the batch, outputs and partials;
  * an exact-fp32 call whose concat seam is off a 32-channel boundary is refused.

Inputs are those of test_conv (offset Gaussians per source, weights scaled by 1 / sqrt(fan-in)), of test_conv_with_fused_skip for a
ResBlock tail with a fused skip (skip weights of another magnitude), and FiLM rows whose 1 + scale stays near one."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ccdm_stochastic_segmentation_amd import hip  # noqa: E402
from tests import plan_util as PU  # noqa: E402
from tests.test_hip_parity import assert_group_stats, rnd  # noqa: E402

N = 2


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from tests import hip_util
    hip.load()
    return hip_util


class Operands:
    """the tensors of one case: on the host in BCHW for the float64 operator, on the device in NHWC"""

    def __init__(self, U, c):
        self.U, self.c = U, c
        H, W = c.shape()
        rng = np.random.default_rng(zlib.crc32(c.id.encode()))
        cin, cout, k = c.c0 + c.c1, c.cout, c.k
        hc, wc = (2 * H, 2 * W) if c.up else (H, W)
        ho, wo = (hc + 2 * (k // 2) - k) // c.stride + 1, (wc + 2 * (k // 2) - k) // c.stride + 1
        self.xa = rnd(rng, N, c.c0, H, W) * 1.2 if c.skip else rnd(rng, N, c.c0, H, W) * 1.5 + 0.3
        self.xb = rnd(rng, N, c.c1, H, W) * 0.7 - 0.2 if c.c1 else None
        self.w = rnd(rng, cout, cin, k, k) / np.sqrt(cin * k * k)
        self.b = rnd(rng, cout, scale=0.1)
        self.gamma, self.beta = 1 + rnd(rng, cin, scale=0.1), rnd(rng, cin, scale=0.1)
        self.embt = rnd(rng, N, cout) if c.emb else None
        self.filmt = rnd(rng, N, 2 * cin, scale=0.3) if c.film else None
        self.res = rnd(rng, N, cout, ho, wo) if c.resid else None
        self.skip_x = None
        if c.skip:
            sc = sum(c.skip)
            self.skip_x = [rnd(rng, N, c.skip[0], ho, wo) * 1.5 + 0.2] + ([rnd(rng, N, c.skip[1], ho, wo) * 0.8] if len(c.skip) > 1 else [])
            self.ws = rnd(rng, cout, sc, 1, 1) / np.sqrt(sc) * 3.0          # another magnitude than w: the shared exponents matter
            self.bs = rnd(rng, cout, scale=0.1)
        self.srcs = [U.nhwc(self.xa)] + ([U.nhwc(self.xb)] if c.c1 else [])
        self.stats = [U.gn_stats(s, 3 if H * W >= 64 else 1) for s in self.srcs] if c.gn else None
        self.res_d = U.nhwc(self.res) if c.resid else None
        self.skip_d = [U.nhwc(s) for s in self.skip_x] if c.skip else None

    def launch(self, first=0, diag=0):
        """the call on samples [first, N): (out, statistics partials or None, the argument struct that was launched)"""
        U, c, sl, n = self.U, self.c, slice(first, None), N - first
        launched = []
        out, ost = U.conv2d([s[sl].contiguous() for s in self.srcs], self.w.numpy(), self.b.numpy(), c.k,
                            stats=[s[sl] for s in self.stats] if c.gn else None, gamma=self.gamma.numpy(), beta=self.beta.numpy(),
                            act=hip.ACT_SILU if c.silu else hip.ACT_NONE, stride=c.stride, up=c.up,
                            emb=self.embt[sl].numpy() if c.emb else None, film=self.filmt[sl].numpy() if c.film else None,
                            emb_rows=np.arange(n) if (c.emb or c.film) else None, resid=self.res_d[sl].contiguous() if c.resid else None,
                            skip=([s[sl].contiguous() for s in self.skip_d], self.ws.numpy(), self.bs.numpy()) if c.skip else None,
                            want_stats=c.stats, prec=c.prec, fine=c.fine, diag=diag, launched=launched)
        return out, ost, launched[0]

    def float64(self):
        c = self.c
        return self.U.conv_float64(torch.cat([self.xa, self.xb], 1) if c.c1 else self.xa, self.w, self.b,
                                   gamma=self.gamma if c.gn else None, beta=self.beta if c.gn else None, film=self.filmt, silu=c.silu,
                                   up=bool(c.up), stride=c.stride, emb=self.embt, resid=self.res,
                                   skip=(torch.cat(self.skip_x, 1), self.ws, self.bs) if c.skip else None)


@pytest.mark.parametrize("c", PU.PLAN_CASES, ids=[c.id for c in PU.PLAN_CASES])
def test_conv_plan_case_against_float64(U, parity_log, c):
    want = c.signature()
    op = Operands(U, c)
    if c.refused:           # exact-fp32 chunks are 32 channels wide: the seam must fall on a chunk boundary
        with pytest.raises(hip.CcdmHipError, match=c.refused):
            op.launch()
        return
    out, ost, args = op.launch()
    assert args.N == N and PU.signature(args, hip.conv_plan(args)) == want, (PU.signature(args, hip.conv_plan(args)), want)
    # ---- the float64 operator
    got = U.bchw(out)
    ref = op.float64().float()
    assert got.shape == ref.shape
    err = (got.double() - ref.double()).abs().max().item()
    bar = 3e-5 if (c.skip or (c.k == 1 and c.gn)) else 2e-5
    parity_log("conv_plan_coverage", **{repr(want): err})
    print(f"{c.id}: max |out - float64| = {err:.3e} (bar {bar:g})")
    assert torch.isfinite(got).all() and err <= bar, f"max |out - float64| = {err:.3e} (bar {bar:g})"
    # ---- fused output statistics == statistics of what was stored
    assert (ost is not None) == c.stats
    if c.stats:
        st, gd = ost.cpu().sum(1), got.double()
        np.testing.assert_allclose(st[..., 0].numpy(), gd.sum((2, 3)).numpy(), rtol=0, atol=2e-6 * gd.abs().sum((2, 3)).max().item())
        np.testing.assert_allclose(st[..., 1].numpy(), (gd * gd).sum((2, 3)).numpy(), rtol=2e-6, atol=0)
        assert_group_stats(gd, st)
    # ---- a specialised family against the general kernel on the same call
    if want[0] != "general":
        gen, gst, gargs = op.launch(diag=hip.DIAG_GENERAL_KERNEL)
        assert hip.conv_plan(gargs).kernel == hip.CONV_KERNEL_GENERAL
        d = (out - gen).abs().max().item()
        if want[0] == "ks":     # the same products in another summation order over K
            assert d <= 8e-6, f"ccdm_conv_ks against the general kernel: max |d| = {d:.3e}"
        else:
            assert torch.equal(out, gen), f"{want[0]} against the general kernel: max |d| = {d:.3e}"
        if c.stats:
            np.testing.assert_allclose(ost.sum(1).cpu().numpy(), gst.sum(1).cpu().numpy(), rtol=2e-6, atol=1e-4)
    # ---- determinism: run to run, and under batch sharding
    again, ost2, _ = op.launch()
    assert torch.equal(out, again), "run-to-run nondeterminism"
    one, ost1, args1 = op.launch(first=N - 1)
    assert args1.N == 1 and PU.signature(args1, hip.conv_plan(args1)) == want
    assert torch.equal(one, out[N - 1:]), f"the last sample alone differs from its slice: max |d| = {(one - out[N - 1:]).abs().max().item():.3e}"
    if c.stats:
        assert torch.equal(ost, ost2), "run-to-run nondeterminism of the statistics partials"
        assert torch.equal(ost1, ost[N - 1:]), "the statistics partials of the last sample alone differ from its slice"
