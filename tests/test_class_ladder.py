"""The class-count ladder of the guided step kernels (ccdm_guided.hip) and of the bound-term kernel (ccdm_bound.hip): every kernel family
there is compiled once per rung of KP_LADDER (csrc/ccdm_sampler_common.h) and a launch picks the first rung >= K.  The kernel tests sweep
both ends of every rung (ladder_util.RUNG_KS); what is held here, without a device, is that the sweep is the ladder's: the parsed ladder
is the one the launchers walk, RUNG_KS has both ends of every rung, the block size changes where ladder_util says it does, every K list
of the kernel tests contains RUNG_KS, and the seeded inputs keep the float64 comparisons inside their caps by the reference alone."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ccdm_stochastic_segmentation_amd import hip
from tests import guided_util, ladder_util
from tests.guided_util import mixed_inputs, tempered_cases, tempered_reference
from tests.ladder_util import LADDER, MAX_CLASSES, RUNG_KS, block_of, margin_seed, rung_of

WALK_SRC = """#include "ccdm_sampler_common.h"
#include <cstdio>
int main() {
    for (int K = 1; K <= %d; ++K) {
        int guided = 0, plain = 0;
        ccdm::dispatch_kp<256>(K, [&](auto kp) { guided = decltype(kp)::value; });
        ccdm::dispatch_kp(K, [&](auto kp) { plain = decltype(kp)::value; });
        std::printf("%%d %%d %%d\\n", K, guided, plain);
    }
    return 0;
}
""" % MAX_CLASSES


def test_the_parsed_ladder_is_what_dispatch_kp_walks():
    """The header compiled for the host alone (dispatch_kp is host code): for every K in [1, 255] dispatch_kp<256>, the guided and bound
    launchers' walk, picks ladder_util.rung_of(K), and the plain epilogue's dispatch_kp (MAX = 32) picks the same rung up to 32 and 32
    above it.  The ladder is ascending, begins at 2, holds 32 (the last register rung) and ends at 256 > CCDM_MAX_CLASSES."""
    print("the parsed ladder:", LADDER)
    assert LADDER == sorted(set(LADDER)) and LADDER[0] == 2 and LADDER[-1] == 256 and ladder_util.REGISTER_TOP in LADDER
    assert MAX_CLASSES == hip.MAX_CLASSES < LADDER[-1]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "walk.cpp"), os.path.join(d, "walk")
        open(src, "w").write(WALK_SRC)
        subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-I" + os.path.join(ladder_util.ROOT, "include"),
                               "-I" + hip.CSRC, src, "-o", exe])
        rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe]).decode().splitlines()]
    assert [r[0] for r in rows] == list(range(1, MAX_CLASSES + 1))
    for K, guided, plain in rows:
        assert guided == rung_of(K) and plain == min(rung_of(K), ladder_util.REGISTER_TOP), (K, guided, plain)
    assert sorted({r[1] for r in rows}) == LADDER


def test_rung_ks_are_the_lowest_and_the_highest_k_of_every_rung():
    by_rung = {}
    for K in range(2, MAX_CLASSES + 1):
        by_rung.setdefault(rung_of(K), []).append(K)
    assert sorted(by_rung) == LADDER
    ends = sorted({k for ks in by_rung.values() for k in (ks[0], ks[-1])})
    print("RUNG_KS:", RUNG_KS)
    assert RUNG_KS == ends
    for kp, ks in by_rung.items():
        assert ks[-1] == min(kp, MAX_CLASSES) and {rung_of(ks[0]), rung_of(ks[-1])} == {kp}
    # a K equal to a rung (no padding) and a K one above a rung (a full rung in front of a one-class tail), for every rung below the last
    assert all(kp in RUNG_KS and kp + 1 in RUNG_KS for kp in LADDER[:-1])
    for K in RUNG_KS:
        N, HW, k = ladder_util.shape_of(K)
        blk = block_of(K)
        assert k == K and N >= 2 and N * HW > blk and HW % blk != 0 and (N * HW) % blk != 0          # > 1 block, an edge inside a sample, a partial last


def test_the_bound_workspace_changes_its_block_between_32_and_33_classes():
    """ccdm_bound_terms_workspace_bytes = (ceil(N HW / BLK) + N) 16 bytes with BLK = bound_blk of the rung: 256 up to K = 32, 64 from
    K = 33 on — exactly where ladder_util.block_of changes, for every K."""
    import __graft_entry__ as g
    g.build()
    lib = hip.load()
    N, HW = 3, 1000
    got = [int(lib.ccdm_bound_terms_workspace_bytes(N, HW, K)) for K in range(1, MAX_CLASSES + 1)]
    want = [(-(-N * HW // block_of(K)) + N) * 16 for K in range(1, MAX_CLASSES + 1)]
    assert got == want
    changes = [K for K in range(2, MAX_CLASSES + 1) if got[K - 1] != got[K - 2]]
    assert changes == [33] and block_of(32) == 256 and block_of(33) == 64


def test_every_k_list_of_the_kernel_tests_contains_the_rung_ends():
    from tests import test_label_bound, test_queue_guided, test_sampling_queue, test_tiled_sampling, test_view_sampling
    lists = {"ccdm_evidence_step / ccdm_shaped_step (guided_util.SHAPES)": [K for _, _, K in guided_util.SHAPES],
             "ccdm_views_step (KERNEL_KS)": test_view_sampling.KERNEL_KS, "ccdm_tiled_step (KERNEL_KS)": test_tiled_sampling.KERNEL_KS,
             "ccdm_slots_step (SLOT_HW_K)": [K for _, K in test_sampling_queue.SLOT_HW_K], "ccdm_slots_guided_step (KS)": test_queue_guided.KS,
             "ccdm_bound_terms (TERMS_KS)": test_label_bound.TERMS_KS, "ccdm_bound_terms (TERMS_HW_K)": [K for _, K in test_label_bound.TERMS_HW_K]}
    # the one exception: the last rung of ccdm_slots_guided_step (test_queue_guided.RUNG_KS_LEFT_OUT says why)
    left_out = {"ccdm_slots_guided_step (KS)": set(test_queue_guided.RUNG_KS_LEFT_OUT)}
    assert left_out["ccdm_slots_guided_step (KS)"] == {K for K in RUNG_KS if rung_of(K) == LADDER[-1]}
    for name, ks in lists.items():
        print(f"{name}: K in {sorted(set(ks))} -> rungs {sorted({rung_of(K) for K in ks})}")
        out = left_out.get(name, set())
        assert set(RUNG_KS) - out <= set(ks), (name, sorted(set(RUNG_KS) - out - set(ks)))
        assert {rung_of(K) for K in ks} == set(LADDER) - {rung_of(K) for K in out}, name
    assert guided_util.SHAPES[:4] == [(3, 63, 2), (2, 300, 5), (2, 64, 20), (1, 64, 255)] and guided_util.SHAPES[4:] == ladder_util.SHAPES
    for ks, need in ((test_view_sampling.TEMPERED_KS, {2, 5, 40, 16, 24, 32, 128}), (test_view_sampling.MIRRORED_KS, {2, 20, 16, 32, 255}),
                     (test_sampling_queue.ANCHOR_KS, {24, 32, 128, 255}), (test_queue_guided.ANCHOR_KS, {24, 32, 128})):
        assert need <= set(ks)


@pytest.mark.parametrize("N,HW,K", guided_util.SHAPES)
def test_ladder_inputs_keep_the_float64_comparison_inside_its_caps(N, HW, K):
    """test_tempered_kernel_against_float64 leaves out of its sample comparison the pixels whose float64 race margin is <= 1e-4 or that lie
    within 1e-5 of a truncation threshold, at most max(2, 2 %) of the shape, and compares the probabilities at more than half of the
    entries.  Both are conditions on the inputs: with the recorded seed the float64 reference alone meets them, for every (tau, r,
    evidence, t) of that test."""
    x0, ev_all, xt = mixed_inputs(np.random.default_rng(margin_seed(N, HW, K)), N, HW, K)
    left_out, compared = 0.0, 1.0
    for tau, r, ev, t in tempered_cases(ev_all):
        _, _, _, big, skip = tempered_reference(x0, ev, xt, tau, r, t)
        assert skip.sum() <= max(2, 0.02 * skip.size), (tau, r, ev is not None, t, int(skip.sum()))
        assert big.mean() > 0.5, (tau, r, ev is not None, t, float(big.mean()))
        left_out, compared = max(left_out, float(skip.mean())), min(compared, float(big.mean()))
    print(f"K={K} (rung {rung_of(K)}) at ({N}, {HW}), seed {margin_seed(N, HW, K)}: at most {100 * left_out:.2f} % of the pixels left out, "
          f"at least {100 * compared:.1f} % of the entries compared")


def test_ladder_inputs_of_the_tempered_views_test_are_compared_at_most_entries():
    """test_tempered_views_kernel_against_float64 compares more than half of the entries: the float64 reference alone says so."""
    from tests import test_view_sampling
    for K in test_view_sampling.TEMPERED_KS:
        _, _, cases = test_view_sampling.tempered_views_reference(K)
        share = min(float(big.mean()) for *_, big in cases)
        print(f"views K={K} (rung {rung_of(K)}): at least {100 * share:.1f} % of the entries compared")
        assert share > 0.5
