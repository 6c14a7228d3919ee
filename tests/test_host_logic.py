"""CPU-only tests: host logic of the product (spec, schedules, boundary classes), the C-ABI library's
symbol table and host-side packer, and the multi-process sharding path on gloo."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ccdm_stochastic_segmentation_amd as P
from ccdm_stochastic_segmentation_amd import hip, models
from ccdm_stochastic_segmentation_amd.distributed import shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIDC_BP = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1,
               num_head_channels=32, softmax_output=True)


def lidc_model(vote="confidence"):
    return P.build_model(250, "cosine", {"s": 0.008}, [(1, 128, 128), (2, 128, 128)], (1, 128, 128), "unet_openai", LIDC_BP,
                         "datasets.lidc", vote, None)


def test_shipped_library_reads_no_environment_and_allocates_nothing():
    """The library imports neither getenv nor hipMalloc* (include/ccdm_hip.h: no allocation inside, no global state besides the
    thread-local error string)."""
    import subprocess
    import __graft_entry__ as g
    g.build()
    syms = subprocess.run(["nm", "-D", "--undefined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    bad = [ln for ln in syms.splitlines() if any(t in ln for t in ("getenv", "hipMalloc", "hipHostMalloc", "hipMallocAsync"))]
    assert not bad, bad


def test_library_exports_every_declared_symbol_abi11():
    """The C-ABI library loads here (no GPU) and exports exactly what include/ccdm_hip.h declares."""
    import __graft_entry__ as g
    g.build()
    lib = hip.load()
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ccdm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(hip.SIGNATURES), declared ^ set(hip.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ccdm_version() == hip.ABI_VERSION == 11
    assert ctypes.sizeof(hip.ConvArgs) % 8 == 0 and ctypes.sizeof(hip.PostArgs) % 8 == 0


def test_struct_layout_matches_header():
    """ctypes mirrors of the two argument structs agree with the C compiler's layout."""
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ccdm_hip.h"
    int main(){
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ccdm_conv_args), offsetof(ccdm_conv_args, gamma), offsetof(ccdm_conv_args, w),
             offsetof(ccdm_conv_args, emb_row_of_sample), offsetof(ccdm_conv_args, out), offsetof(ccdm_conv_args, out_slices),
             offsetof(ccdm_conv_args, SC1), offsetof(ccdm_conv_args, skip_w));
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ccdm_post_args), offsetof(ccdm_post_args, step_table), offsetof(ccdm_post_args, philox_seed),
             offsetof(ccdm_post_args, xin_stride), offsetof(ccdm_post_args, posterior_out), offsetof(ccdm_post_args, noise_row0),
             offsetof(ccdm_post_args, range_flag));
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ccdm_resample_args), offsetof(ccdm_resample_args, stats), offsetof(ccdm_resample_args, gamma),
             offsetof(ccdm_resample_args, eps), offsetof(ccdm_resample_args, N), offsetof(ccdm_resample_args, mode), offsetof(ccdm_resample_args, out_raw));
      printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ccdm_stem_args), offsetof(ccdm_stem_args, K), offsetof(ccdm_stem_args, bias), offsetof(ccdm_stem_args, Cout),
             offsetof(ccdm_stem_args, out), offsetof(ccdm_stem_args, out_slices), sizeof(ccdm_post_run));
      printf("%zu %zu %zu %zu %zu %zu\n", sizeof(ccdm_head_args), offsetof(ccdm_head_args, slices), offsetof(ccdm_head_args, eps), offsetof(ccdm_head_args, w),
             offsetof(ccdm_head_args, K), offsetof(ccdm_head_args, logits_out));
      printf("%zu %zu %zu %zu\n", offsetof(ccdm_post_args, run), offsetof(ccdm_post_run, sample_offset), offsetof(ccdm_post_run, noise_row0),
             offsetof(ccdm_post_run, posterior_out));
      return 0; }'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    A, B, R, S, Hd = hip.ConvArgs, hip.PostArgs, hip.ResampleArgs, hip.StemArgs, hip.HeadArgs
    mine = [ctypes.sizeof(A), A.gamma.offset, A.w.offset, A.emb_row_of_sample.offset, A.out.offset, A.out_slices.offset,
            A.SC1.offset, A.skip_w.offset,
            ctypes.sizeof(B), B.step_table.offset, B.philox_seed.offset, B.xin_stride.offset, B.posterior_out.offset,
            B.noise_row0.offset, B.range_flag.offset,
            ctypes.sizeof(R), R.stats.offset, R.gamma.offset, R.eps.offset, R.N.offset, R.mode.offset, R.out_raw.offset,
            ctypes.sizeof(S), S.K.offset, S.bias.offset, S.Cout.offset, S.out.offset, S.out_slices.offset, hip.POST_RUN_BYTES,
            ctypes.sizeof(Hd), Hd.slices.offset, Hd.eps.offset, Hd.w.offset, Hd.K.offset, Hd.logits_out.offset,
            B.run.offset, 24, 28, 48]            # ccdm_post_run: noise 0, stride 8, seed 16, sample_offset 24, noise_row0 28, out_probs 32, out_onehot 40, posterior_out 48
    assert [int(v) for v in out] == mine


def test_pack_conv_weight_layout():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((40, 6, 3, 3)).astype(np.float32)       # Cout 40 -> 2 n-tiles, Cin 6 -> padded to 32
    buf = hip.pack_conv_weight(w, 3).view(np.float32).reshape(9, 16, 2, 64)
    for tap, kp, nt, l in [(0, 0, 0, 0), (4, 2, 1, 7), (8, 1, 0, 45), (3, 2, 1, 63), (5, 10, 0, 3)]:
        co, ci = nt * 32 + (l & 31), 2 * kp + (l >> 5)
        exp = w[co, ci, tap // 3, tap % 3] if (co < 40 and ci < 6) else 0.0
        assert buf[tap, kp, nt, l] == exp
    assert hip.load().ccdm_conv_slices(128, 128, 1, 3) == 12
    assert hip.load().ccdm_conv_slices(16, 16, 1, 3) == 2
    assert hip.load().ccdm_conv_slices(8, 8, 1, 3) == 1
    lib = hip.load()
    # ccdm_conv_slices_ex: from the INPUT geometry; fine = the latency slicing (up to 32 slices where the default gives fewer)
    assert lib.ccdm_conv_slices_ex(128, 128, 3, 1, 0, 0) == 12 and lib.ccdm_conv_slices_ex(128, 128, 3, 1, 0, 1) == 32
    assert lib.ccdm_conv_slices_ex(128, 128, 3, 1, 0, 2) == 64 and lib.ccdm_conv_slices_ex(64, 64, 3, 1, 0, 2) == 16
    assert lib.ccdm_conv_slices_ex(128, 128, 3, 2, 0, 0) == lib.ccdm_conv_slices(64, 64, 2, 3)
    assert lib.ccdm_conv_slices_ex(64, 64, 3, 1, 0, 1) == 16 and lib.ccdm_conv_slices_ex(8, 8, 3, 1, 0, 1) == 1
    assert lib.ccdm_conv_slices_ex(64, 64, 3, 1, 2, 0) == lib.ccdm_upconv_slices(64, 64) == 8 and lib.ccdm_conv_slices_ex(64, 64, 3, 1, 2, 1) == 32
    assert lib.ccdm_conv_slices_ex(256, 512, 3, 1, 0, 1) == lib.ccdm_conv_slices(256, 512, 1, 3) == 96


@pytest.mark.parametrize("hin,win", [(8, 8), (8, 16), (16, 16), (32, 32), (64, 64), (128, 256)])
def test_upconv_slice_counts_agree_across_entry_points(hin, win):
    """The statistics slices an `up = 2` conv leaves, asked three ways (ccdm_conv_slices_ex from the input geometry,
    ccdm_conv_out_slices from the argument struct, ccdm_upconv_slices for the default slicing), are one number.  8-wide inputs
    tile with one phase per block (x 4 slots), wider ones with four phases per block.  Only the agreement is asserted."""
    lib = hip.load()
    for fine in (0, 1, 2):
        a = hip.ConvArgs(C0=32, N=1, Hin=hin, Win=win, Hout=2 * hin, Wout=2 * win, ksize=3, stride=1, up=2, Cout=32,
                         prec=hip.PREC_F16X3, emb_off=-1, fine_slices=fine)
        ex = lib.ccdm_conv_slices_ex(hin, win, 3, 1, 2, fine)
        assert lib.ccdm_conv_out_slices(ctypes.byref(a)) == ex, (fine, ex)
        if fine == 0:
            assert lib.ccdm_upconv_slices(hin, win) == ex


def test_pack_upconv_weight_is_the_phase_summed_2x2_kernel():
    """ccdm_pack_upconv_weight (include/ccdm_hip.h, `up = 2`): Upsample + conv 3x3 (unet.py:106-116) as four 2x2 kernels — the 3x3 taps
    that fall on one low-resolution pixel added in fp64, rounded once, packed as a 2x2 conv with n-tile = 4 * (channel tile) + phase.  The
    numpy restatement below also checks the operator identity itself against F.interpolate + F.conv2d."""
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    cout, cin = 64, 8
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    w2 = np.zeros((4, cout, cin, 2, 2), np.float64)
    for dy in range(2):
        for dx in range(2):
            for u in range(3):
                for v in range(3):
                    w2[2 * dy + dx, :, :, (dy + u + 1) // 2 - dy, (dx + v + 1) // 2 - dx] += w[:, :, u, v]
    # packed channel = (4 * (co // 32) + phase) * 32 + co % 32: the four phases of a 32-channel tile are adjacent n-tiles
    w2f = w2.astype(np.float32).reshape(4, cout // 32, 32, cin, 2, 2).transpose(1, 0, 2, 3, 4, 5).reshape(4 * cout, cin, 2, 2)
    assert np.array_equal(hip.pack_upconv_weight(w), hip.pack_conv_weight(w2f, 2, hip.PREC_F16X3))
    assert hip.load().ccdm_upconv_slices(64, 64) == 8 and hip.load().ccdm_upconv_slices(8, 8) == 4
    assert hip.load().ccdm_upconv_supported(cin, 48, hip.PREC_F16X3) == 0
    # operator identity: out(2y+dy, 2x+dx) = sum_ab W'[dy,dx][a,b] in(y+dy-1+a, x+dx-1+b), zero outside the image
    x = torch.from_numpy(rng.standard_normal((1, cin, 5, 7)))
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), torch.from_numpy(w).double(), padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    got = torch.zeros_like(ref)
    for dy in range(2):
        for dx in range(2):
            ph = F.conv2d(xp, torch.from_numpy(w2[2 * dy + dx]))             # [1,cout,H+1,W+1]: window origin (y-1+., x-1+.)
            got[:, :, dy::2, dx::2] = ph[:, :, dy:dy + 5, dx:dx + 7]
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=1e-12)


def test_missing_library_is_a_hard_error(monkeypatch, tmp_path):
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setenv("CCDM_NO_AUTOBUILD", "1")
    with pytest.raises(hip.CcdmHipError, match="no CPU fallback"):
        hip.load()


def test_no_cpu_path():
    m = lidc_model().eval()
    x = torch.zeros(1, 2, 128, 128); x[:, 0] = 1
    with pytest.raises(hip.CcdmHipError, match="no CPU path"):
        m(x, torch.zeros(1, 1, 128, 128))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "ccdm_stochastic_segmentation_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("# oracle", ""), fn


def test_state_dict_layout_and_strict_load(golden):
    m = lidc_model()
    keys = [[k, list(v.shape)] for k, v in m.unet.state_dict().items()]
    assert keys == golden.meta["lidc_keys"] and len(keys) == 398
    assert m.unet.spec.num_params() == 5699138
    assert list(m.state_dict())[:3] == ["diffusion.betas", "diffusion.alphas", "diffusion.cumalphas"]
    sd = {k: torch.from_numpy(v) for k, v in P.make_synthetic_state_dict(m.unet.spec, 0).items()}
    v0 = m.unet._weights_version
    m.unet.load_state_dict(sd, strict=True)
    assert m.unet._weights_version > v0
    assert torch.equal(m.unet.state_dict()["out.2.weight"], sd["out.2.weight"])
    bad = dict(sd); bad.pop("out.2.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        m.unet.load_state_dict(bad, strict=True)
    bad = dict(sd); bad["extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.unet.load_state_dict(bad, strict=True)
    # an ignite-style checkpoint dict {"model":..., "average_model":...} loads the same way
    ckpt = {"model": sd, "average_model": sd, "optimizer": {}, "engine": {}}
    m.unet.load_state_dict(ckpt["average_model"], strict=True)
    assert m.time_steps == 250 and m.diffusion.num_classes == 2


def test_auto_substreams_rule():
    """substreams = 0: two concurrent sub-batches once the batch holds the pixels of 32 samples of 128 x 128 — a rule of (N, H, W) only."""
    from ccdm_stochastic_segmentation_amd.models import auto_substreams
    assert [auto_substreams(n, 128, 128) for n in (1, 8, 31, 32, 64)] == [1, 1, 1, 2, 2]
    assert auto_substreams(16, 256, 512) == 2 and auto_substreams(4, 512, 1024) == 2 and auto_substreams(1, 512, 1024) == 1
    assert auto_substreams(2, 256, 512) == 1 and auto_substreams(8, 64, 128) == 1


def test_builder_contract():
    with pytest.raises(ValueError, match="256 classes"):         # x_t travels as a uint8 class index
        P.build_model(250, "cosine", None, [(3, 64, 64), (256, 64, 64)], (3, 64, 64), "unet_openai", dict(base_channels=32), "datasets.lidc", "confidence", None)
    assert P.build_model(250, "cosine", None, [(3, 64, 64), (40, 64, 64)], (3, 64, 64), "unet_openai", LIDC_BP, "datasets.lidc", "confidence", None).diffusion.num_classes == 40
    with pytest.raises(NotImplementedError, match="backbone resnet50"):
        P.build_model(250, "cosine", None, [(1, 128, 128), (2, 128, 128)], None, "resnet50", {}, "x")
    with pytest.raises(ValueError, match="unsupported image size"):
        P.build_model(250, "cosine", None, [(1, 100, 100), (2, 100, 100)], None, "unet_openai", LIDC_BP, "x")
    with pytest.raises(ValueError, match="GroupNorm"):          # C5 at base 32: GroupNorm(32, 16)
        P.build_model(250, "cosine", None, [(3, 512, 1024), (20, 512, 1024)], None, "unet_openai", LIDC_BP, "x")
    m = lidc_model()
    m.train()
    with pytest.raises(ValueError, match="'t' needs to be a Tensor"):
        m(torch.zeros(1, 2, 128, 128), torch.zeros(1, 1, 128, 128))
    m.eval()
    with pytest.raises(AttributeError, match="guidance_scale_weights"):
        m(torch.zeros(1, 2, 128, 128), torch.zeros(1, 1, 128, 128), label_ref_logits=torch.zeros(1, 2, 128, 128))


def test_schedules_and_steps_match_reference_golden(golden):
    g = golden["g1_schedules"]
    for name, sched, T, sp in [("cosine250", "cosine", 250, {"s": 0.008}), ("cosine1000", "cosine", 1000, None), ("linear250", "linear", 250, None)]:
        d = P.DiffusionModel(sched, T, 2, sp)
        assert np.array_equal(d.betas.numpy(), g[name + "_betas"])
        assert np.array_equal(d.alphas.numpy(), g[name + "_alphas"])
        assert np.array_equal(d.cumalphas.numpy(), g[name + "_cumalphas"])
    for T, K in [(250, 10), (250, 25), (250, 200), (250, 150), (250, 100), (250, 50), (1000, 16)]:
        assert P.step_values(T, 10000 + K) == list(g[f"steps_T{T}_K{K}"])
    assert P.step_values(250, None) == list(range(250, 0, -1))
    assert P.step_values(250, 3) == [3, 2, 1]
    with pytest.raises(AssertionError):
        P.step_values(250, 10000 + 251)
    d = P.DiffusionModel("cosine", 250, 2)
    assert d.posterior_coeffs(1) == (0.0, 1.0)
    assert d.posterior_coeffs(250) == (float(d.alphas[249]), float(d.cumalphas[248]))


def test_one_hot_categorical_bchw_matches_reference_golden(golden):
    g = golden["g6_sampler"]
    for K in (2, 20):
        probs = torch.from_numpy(g[f"K{K}_probs"])
        torch.manual_seed(6)
        d = P.OneHotCategoricalBCHW(probs=probs)
        s = d.sample()
        assert np.array_equal(s.argmax(1).numpy(), g[f"K{K}_idx"])
        assert s.dtype == torch.float32 and s.shape == probs.shape
        assert np.array_equal(d.max_prob_sample().numpy(), g[f"K{K}_maxprob"])
        assert np.array_equal(d.prob_sample().numpy(), g[f"K{K}_probsample"])
    torch.manual_seed(42)
    x = P.OneHotCategoricalBCHW(logits=torch.zeros(3, 2, 8, 8)).sample()
    assert np.array_equal(x.argmax(1).numpy(), g["xT_seed42_K2"])
    assert tuple(x.stride()) == (128, 1, 16, 2)                       # BCHW view of channels-last memory
    torch.manual_seed(42)
    x = P.OneHotCategoricalBCHW(logits=torch.zeros(2, 20, 8, 8)).sample()
    assert np.array_equal(x.argmax(1).numpy(), g["xT_seed42_K20"])
    with pytest.raises(ValueError):
        P.OneHotCategoricalBCHW(probs=torch.ones(3))
    with pytest.raises(ValueError):
        P.OneHotCategoricalBCHW()


def test_shard_range_partitions():
    for n in (0, 1, 7, 64, 65):
        for w in (1, 2, 3, 8):
            rs = [shard_range(n, r, w) for r in range(w)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
            sizes = [b - a for a, b in rs]
            assert max(sizes) - min(sizes) <= 1


WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["CCDM_ROOT"])
from ccdm_stochastic_segmentation_amd.distributed import init_from_env, sample_sharded, shard_range
rank, local, world = init_from_env("gloo")
class Fake:                      # stands in for DenoisingModel: output encodes (global sample index, offset seen)
    sample_offset = 0; noise_slice = None
    def __call__(self, x, cond, feat=None, **kw):
        n = x.shape[0]
        assert self.noise_slice == (7, self.sample_offset)
        out = x.clone()
        out[:, 0, 0, 0] = torch.arange(n, dtype=x.dtype) + self.sample_offset
        out[:, 1, 0, 0] = cond[:, 0, 0, 0]
        return {"diffusion_out": out}
N = 7
x = torch.zeros(N, 2, 4, 4); cond = torch.arange(N, dtype=torch.float32).reshape(N, 1, 1, 1).expand(N, 1, 4, 4).contiguous() * 10
out = sample_sharded(Fake(), x, cond)
assert out.shape == (N, 2, 4, 4)
assert torch.equal(out[:, 0, 0, 0], torch.arange(N, dtype=torch.float32)), out[:, 0, 0, 0]
assert torch.equal(out[:, 1, 0, 0], torch.arange(N, dtype=torch.float32) * 10)
lo, hi = shard_range(N, rank, world)
loc = sample_sharded(Fake(), x, cond, gather=False)
assert loc.shape[0] == hi - lo
dist.barrier(); dist.destroy_process_group()
sys.stdout.write(f"rank{rank}ok\n"); sys.stdout.flush()
'''


def test_sharded_sampling_world_size_2_gloo(tmp_path):
    """N > 1 path on CPU: two processes, gloo, ragged shard sizes (7 samples over 2 ranks)."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, CCDM_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29611")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29611", str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rank0ok" in r.stdout and "rank1ok" in r.stdout


def test_evaluation_harness_host_side():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    ds = E.SyntheticLIDC(size=3)
    img, labs, w = ds[1]
    assert img.shape == (1, 128, 128) and labs.shape == (4, 2, 128, 128) and img.abs().max() <= 1
    assert torch.equal(labs.sum(1), torch.ones(4, 128, 128)) and list(w) == [0.25] * 4
    img2, labs2, _ = ds[1]
    assert torch.equal(img, img2) and torch.equal(labs, labs2)            # deterministic
    assert E._as_list(8) == [8] and E._as_list([1, 4]) == [1, 4]         # `evaluations: 8` (shipped yml) or a list
    assert isinstance(E.make_dataset({"dataset_file": "synthetic.lidc", "dataset_val_max_size": 5}), E.SyntheticLIDC)
    with pytest.raises(ValueError, match="Unknown dataset"):
        E.make_dataset({"dataset_file": "ade20k"})
    import yaml
    p = yaml.safe_load(open(os.path.join(ROOT, "params_eval.yml")))
    for key in ("time_steps", "beta_schedule", "beta_schedule_params", "backbone", "unet_openai", "feature_cond_encoder",
                "evaluation_vote_strategy", "evaluations", "batch_size", "load_from", "dataset_file"):
        assert key in p, key
    m = E.build_from_params(p, [(1, 128, 128), (2, 128, 128)], "cpu")
    assert m.step_T_sample == "confidence" and m.time_steps == 250


def test_ddpm_eval_dispatch(tmp_path, monkeypatch):
    import yaml
    import ddpm_eval
    p = yaml.safe_load(open(os.path.join(ROOT, "params_eval.yml")))
    p["dataset_file"] = "datasets.ade20k"
    f = tmp_path / "params_x.yml"
    yaml.safe_dump(p, open(f, "w"))
    with pytest.raises(ValueError, match="Unknown dataset"):
        ddpm_eval.main(["ddpm_eval.py", str(f)])
    p["dataset_file"] = "datasets.cityscapes"
    yaml.safe_dump(p, open(f, "w"))
    with pytest.raises(NotImplementedError):
        ddpm_eval.main(["ddpm_eval.py", str(f)])


def test_lidc_reader_layout_and_transform(tmp_path):
    """`Test_LIDC` + `batch_transform` (datasets/lidc.py:164-210) on a data_lidc.hdf5-layout source: images [n,128,128] float in
    [-0.5, 0.5] -> [1,128,128] * 2; labels [n,4,128,128] -> [4,2,128,128] one-hot floats; max_size caps the split.  The mapping
    form runs everywhere; the same data written to a real HDF5 file is read back when h5py is installed."""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    rng = np.random.default_rng(3)
    images = rng.uniform(-0.5, 0.5, (5, 128, 128)).astype(np.float32)
    labels = (rng.random((5, 4, 128, 128)) > 0.7).astype(np.uint8)
    src = {"test": {"images": images, "labels": labels}}
    ds = E.TestLIDC(src, "test", None)
    assert len(ds) == 5 and len(E.TestLIDC(src, "test", 3)) == 3 and len(E.TestLIDC(src, "test", 500)) == 5
    img, lab, w = ds[2]
    assert img.shape == (1, 128, 128) and img.dtype == torch.float32 and torch.equal(img[0], torch.from_numpy(images[2]) * 2)
    assert lab.shape == (4, 2, 128, 128) and lab.dtype == torch.float32 and torch.equal(lab.argmax(1), torch.from_numpy(labels[2]).long())
    assert torch.equal(lab.sum(1), torch.ones(4, 128, 128)) and list(w) == [0.25] * 4
    # dataset_val_max_size: null (the shipped params_eval.yml) = the whole split, as the reference's test_dataset(None)
    import yaml
    p = yaml.safe_load(open(os.path.join(ROOT, "params_eval.yml")))
    assert p["dataset_val_max_size"] is None
    # file form 1 (runs everywhere): the .npz mirror of the HDF5 layout, through make_dataset like a params file would name it
    fz = tmp_path / "data_lidc.npz"
    np.savez(fz, **{"test/images": images, "test/labels": labels, "val/images": images[:1], "val/labels": labels[:1]})
    dz = E.make_dataset({"dataset_file": "datasets.lidc", "dataset_path": str(fz), "dataset_val_max_size": 4})
    assert len(dz) == 4 and torch.equal(dz[2][0], img) and torch.equal(dz[2][1], lab)
    with pytest.raises(KeyError, match="train/images"):
        E.TestLIDC(str(fz), "train", None)
    # file form 2: a real HDF5 file — needs h5py (README.md lists it); where h5py exists this leg runs and must pass
    try:
        import h5py
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            E.TestLIDC(str(tmp_path / "data_lidc.hdf5"), "test", None)
        pytest.skip("h5py is not installed in this image: the HDF5 leg of the reader cannot run here (the .npz leg above did)")
    f = tmp_path / "data_lidc.hdf5"
    with h5py.File(f, "w") as h:
        gtest = h.create_group("test")
        gtest.create_dataset("images", data=images)
        gtest.create_dataset("labels", data=labels)
    ds2 = E.make_dataset({"dataset_file": "datasets.lidc", "dataset_path": str(f), "dataset_val_max_size": 4})
    assert len(ds2) == 4 and torch.equal(ds2[2][0], img) and torch.equal(ds2[2][1], lab)


class _NotATensor:                    # stands for an arbitrary class inside a checkpoint (module level: picklable)
    pass


def test_checkpoint_reader_refuses_unsafe_pickle_without_opt_in(tmp_path, monkeypatch):
    from ccdm_stochastic_segmentation_amd import evaluation as E

    m = lidc_model()
    sd = {k: torch.from_numpy(v) for k, v in P.make_synthetic_state_dict(m.unet.spec, 0).items()}
    good = tmp_path / "good.pt"
    torch.save({"model": sd, "average_model": sd}, good)
    E.load_checkpoint(m, str(good))
    assert torch.equal(m.unet.state_dict()["out.2.weight"], sd["out.2.weight"])
    bad = tmp_path / "bad.pt"
    torch.save({"average_model": sd, "engine": _NotATensor()}, bad)
    monkeypatch.delenv("CCDM_ALLOW_UNSAFE_PICKLE", raising=False)
    with pytest.raises(RuntimeError, match="allow_pickle"):
        E.load_checkpoint(m, str(bad))
    E.load_checkpoint(m, str(bad), allow_pickle=True)


def test_sampler_options_from_params_file():
    from ccdm_stochastic_segmentation_amd import evaluation as E
    m = lidc_model()
    assert m.prec == hip.PREC_F16X3 and m.rng == "philox"            # the defaults ARE the benchmarked configuration
    E.apply_sampler_options(m, {})
    assert m.prec == hip.PREC_F16X3 and m.rng == "philox" and m.on_range_error == "layers"
    E.apply_sampler_options(m, {"prec": "f32", "rng": "torch_cpu", "philox_seed": 9, "substreams": 2, "slicing": "latency"})
    assert m.prec == hip.PREC_F32 and m.rng == "torch_cpu" and m.philox_seed == 9 and m.substreams == 2 and m.slicing == "latency"
    with pytest.raises(ValueError, match="prec"):
        E.apply_sampler_options(m, {"prec": "bf16"})


def test_weights_key_sees_in_place_updates():
    m = lidc_model()
    k0 = m._weights_key()
    with torch.no_grad():
        next(m.unet.parameters()).mul_(1.0)                          # optimizer step / Polyak update style
    k1 = m._weights_key()
    assert k1 != k0
    with torch.no_grad():
        m.unet.state_dict()["out.2.bias"].copy_(torch.ones(2))       # p.data.copy_ style
    assert m._weights_key() != k1


def test_feature_condition_on_an_unwired_model_fails_like_the_reference():
    """target_layer / output_stride that do not line up: the reference builds the model and fails on the channel mismatch when a
    feature tensor is passed; a model without any feature encoder ignores the tensor."""
    fce = dict(type="dino", channels=384, output_stride=4, scale="single", target_layer=10)       # block 10 sits at stride 8
    m = P.build_model(250, "cosine", None, [(3, 64, 128), (20, 64, 128)], (3, 64, 128), "unet_openai",
                      dict(LIDC_BP, channel_mult=[1, 1, 2, 2, 4, 4]), "datasets.cityscapes", "confidence", fce).eval()
    assert m.unet.spec.feature_condition_unwired == [10] and not m.unet.spec.feature_condition_idx
    x = torch.zeros(1, 20, 64, 128); x[:, 0] = 1
    with pytest.raises(RuntimeError, match="channel mismatch"):
        m(x, torch.zeros(1, 3, 64, 128), torch.zeros(1, 384, 8, 16))


def test_bench_self_launch_command(monkeypatch):
    """`python bench.py --gpus N` without a launcher environment starts its own ranks with torch.distributed.run."""
    import bench
    seen = {}
    monkeypatch.setattr(bench, "_run_ranks", lambda cmd, env=None: (seen.update(cmd=cmd, env=env) or 0, ""))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "2", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_self_launch_retries_once_without_its_own_ipc_override(monkeypatch):
    """Where bench.py itself had to set HSA_ENABLE_IPC_MODE_LEGACY=0 and the N-rank job fails WITH AN IPC / RCCL ERROR, it is started
    once more without the override; an override that came from the environment is never removed, and any other failure is not retried."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for preset, stderr, want in ((None, "hipIpcGetMemHandle: invalid argument", ["0", None]), ("0", "hipIpcGetMemHandle: invalid argument", ["0"]),
                                 (None, "AssertionError: something else", ["0"])):
        envs = []
        monkeypatch.setattr(bench, "_run_ranks", lambda cmd, env=None, stderr=stderr: (envs.append(env.get("HSA_ENABLE_IPC_MODE_LEGACY")) or 7, stderr))
        if preset is None:
            monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
        else:
            monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", preset)
        with pytest.raises(SystemExit) as e:
            bench.main()
        assert e.value.code == 7 and envs == want, (preset, stderr, envs)


def test_bench_extras_need_full(monkeypatch, capsys):
    """--per-op and --secondary ask for what only a --full run makes: without --full they are refused before anything starts."""
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(bench, "_run_ranks", lambda cmd, env=None: pytest.fail("no ranks may start"))
    for argv in (["--per-op", "x.json"], ["--gpus", "2", "--secondary"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit) as e:
            bench.main()
        assert e.value.code == 2 and "--full" in capsys.readouterr().err, argv


def test_bench_dump_outputs_within_budget(tmp_path):
    """--dump-outputs: a small output is written whole as float32; a larger one as the same seeded sample of its rows on every call,
    with the row indices beside it, within the byte budget; a row over the budget falls back to a seeded sample of elements."""
    import bench
    small = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    info = bench.dump_outputs(str(tmp_path / "s"), {"out": small})
    got = np.load(tmp_path / "s" / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.float().numpy()) and "sample" not in info["out"]
    assert not (tmp_path / "s" / "out_index.npy").exists()
    big = torch.randn(10, 4, 8, 8)                                  # 10 rows of 1 KiB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out": big}, limit=4000)
    rows = np.load(tmp_path / "a" / "out_index.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "out_index.npy"))
    got = np.load(tmp_path / "a" / "out.npy")
    assert 1 <= len(rows) and got.nbytes + rows.nbytes <= 4000 and np.array_equal(got, big.numpy()[rows.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "e"), {"out": big}, limit=600)
    idx = np.load(tmp_path / "e" / "out_index.npy").astype(np.int64)
    got = np.load(tmp_path / "e" / "out.npy")
    assert got.ndim == 1 and got.nbytes + idx.nbytes <= 600 and np.array_equal(got, big.numpy().reshape(-1)[idx])


def test_execution_mode_is_measured_once_and_only_where_it_pays(monkeypatch):
    """substreams = 0 (host logic on a stub engine whose run() sleeps by mode): a sampling call of >= CALIBRATION_MIN_STEPS steps on a
    batch the static rule gives two streams times {2, 1 streams} x {graph, eager}, keeps the fastest, re-sets every engine's inputs
    for the real walk, and does not measure again for the same geometry and weights; short walks, small batches, explicit
    `substreams`, `calibrate_mode = False` and the host-noise parity mode take the static rule without measuring."""
    import time
    from ccdm_stochastic_segmentation_amd import models as Mo
    m = lidc_model().eval()
    log = []

    class Eng:
        device = torch.device("cpu"); stream = None
        def __init__(self, n): self.N = n; self.xt = torch.zeros(n, 128 * 128, dtype=torch.uint8); self.out_probs = torch.zeros(n, 128, 128, 2)
        def enter(self):
            import contextlib; return contextlib.nullcontext()
        def leave(self): pass
        def set_inputs(self, *a): log.append(("inputs", self.N))
        def set_tables(self, *a): pass
        def raise_if_flagged(self): pass
        def check_and_clear_flag(self): return False
        def run(self, n_steps, *, first_row, use_graph, **kw):
            log.append(("run", self.N, n_steps, first_row, use_graph))
            # one stream eager is the fastest "mode" of this stub: everything else pays 0.3 ms per step and engine
            time.sleep(n_steps * (1e-5 if (self.N == 32 and not use_graph) else 3e-4))
    engines = {}
    monkeypatch.setattr(Mo.DenoisingModel, "_engine", lambda self, x, c, f, slot=0: engines.setdefault((x.shape[0], slot), Eng(x.shape[0])))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    m.CALIBRATION_MIN_STEPS, m.CALIBRATION_STEPS, m.CALIBRATION_ROUNDS = 20, (1, 2), 2
    x = torch.zeros(32, 2, 128, 128); x[:, 0] = 1
    cond = torch.zeros(32, 1, 128, 128)
    m._forward_denoising(x, cond, None, init_t=10020)
    assert len(m.mode_choice) == 1 and m.last_mode == (1, False)
    choice = next(iter(m.mode_choice.values()))
    assert set(choice["ms_per_denoise_step"]) == {"2 streams, graph", "2 streams, eager", "1 stream, graph", "1 stream, eager"}
    # the real walk: inputs set again after the probes, then ONE run of all 20 steps on the chosen (single, eager) engine
    last_inputs = max(i for i, e in enumerate(log) if e[0] == "inputs")
    assert log[last_inputs] == ("inputs", 32) and log[last_inputs + 1:] == [("run", 32, 20, 0, False)]
    n_probe = len(log)
    log.clear()
    m._forward_denoising(x, cond, None, init_t=10020)                         # same geometry and weights: no second measurement
    assert [e for e in log if e[0] == "run"] == [("run", 32, 20, 0, False)] and len(log) < n_probe
    # no measurement: short walk | small batch | explicit substreams | calibrate_mode off | host-noise parity mode
    for kw, xs, init_t, want in (({}, x, 10004, (2, True)), ({}, x[:8], 10020, (1, True)), ({"substreams": 2}, x, 10020, (2, True)),
                                 ({"calibrate_mode": False}, x, 10020, (2, True)), ({"rng": "torch_cpu"}, x, 10020, (2, True))):
        m.mode_choice, m.substreams, m.calibrate_mode, m.rng = {}, 0, True, "philox"
        for k_, v in kw.items():
            setattr(m, k_, v)
        m._forward_denoising(xs, cond[:xs.shape[0]], None, init_t=init_t)
        assert m.mode_choice == {} and m.last_mode == want, (kw, init_t, m.last_mode)


def test_host_noise_is_drawn_in_bounded_blocks(monkeypatch):
    """rng='torch_cpu': the per-step Exp(1) draws are consumed from torch's generator in the reference's order whatever the block
    size, and no more than one block is resident (checked on the host logic with a stub engine)."""
    from ccdm_stochastic_segmentation_amd import models as Mo
    m = lidc_model().eval()
    m.rng = "torch_cpu"
    calls = []

    class Eng:
        device = torch.device("cpu"); stream = None; H = W = 8; K = 2
        def __init__(self, n): self.N = n; self.xt = torch.zeros(n, 64, dtype=torch.uint8); self.out_probs = torch.zeros(n, 8, 8, 2)
        def enter(self):
            import contextlib; return contextlib.nullcontext()
        def leave(self): pass
        def set_inputs(self, *a): pass
        def set_tables(self, *a): pass
        def raise_if_flagged(self): pass
        def check_and_clear_flag(self): return False
        def run(self, n_steps, *, first_row, noise, noise_row0, **kw):
            calls.append((first_row, n_steps, noise_row0, None if noise is None else noise.clone()))
    monkeypatch.setattr(Mo.DenoisingModel, "_engine", lambda self, x, c, f, slot=0: Eng(x.shape[0]))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    x = torch.zeros(3, 2, 8, 8); x[:, 0] = 1
    cond = torch.zeros(3, 1, 8, 8)
    per_step = 3 * 8 * 8 * 2 * 4
    outs = []
    for blk_steps in (1000, 2):
        monkeypatch.setattr(Mo, "HOST_NOISE_BLOCK_BYTES", blk_steps * per_step)
        calls.clear()
        torch.manual_seed(5)
        m._forward_denoising(x, cond, None, init_t=5)               # steps t = 5,4,3,2 draw; t = 1 does not
        outs.append([c for c in calls])
    assert [(c[0], c[1], c[2]) for c in outs[0]] == [(0, 5, 0)]
    assert [(c[0], c[1], c[2]) for c in outs[1]] == [(0, 2, 0), (2, 2, 2), (4, 1, 4)]
    whole = outs[0][0][3]
    assert max(c[3].numel() for c in outs[1]) <= 2 * 3 * 128
    assert torch.equal(torch.cat([c[3] for c in outs[1]], 0)[:4], whole[:4])          # same generator order, block by block
    torch.manual_seed(5)
    ref = torch.stack([torch.empty(3 * 64, 2).exponential_(1).reshape(3, 128) for _ in range(4)])
    assert torch.equal(whole[:4], ref)


def test_a_walk_without_jumps_is_the_plain_walk():
    """The sampling loop walks Guidance.walk(S) and draws pass p of a row under pass_key(key, p): without jumps (none asked for, a pair
    that asks for none, a jump length with no jump point) the entries are (s, 0, None) in row order and pass 0 keeps the call's key,
    so the one loop issues for a plain walk what the plain loop issued.  Also the bundle's truth value and its batched form."""
    from ccdm_stochastic_segmentation_amd.models import Guidance
    known, ev = torch.zeros(2, 16, dtype=torch.uint8), torch.ones(2, 16, 3)
    for S in (1, 4, 6, 250):
        plain = [(s, 0, None) for s in range(S)]
        for g in (Guidance(), Guidance(known=known), Guidance(evidence=ev), Guidance(known, None, ev), Guidance(known, (S, 2)), Guidance(known, (3, 2))):
            if g.jumps != (3, 2) or S <= 6:
                assert g.walk(S) == plain, (S, g.jumps)
    jumped = Guidance(known, (2, 2)).walk(6)
    assert jumped == models.resample_walk(6, 2, 2) and [e[0] for e in jumped] == [0, 1, 2, 3, 2, 3, 4, 5]
    for key in (0, 99, 0xFEEDFACE12345678, 2 ** 64 - 1):
        assert models.pass_key(key, 0) == key
    assert not Guidance() and Guidance(known=known) and Guidance(evidence=ev)
    r = Guidance(known, (2, 2), ev).repeat_interleave(3)
    assert r.jumps == (2, 2) and torch.equal(r.known, known.repeat_interleave(3, dim=0)) and torch.equal(r.evidence, ev.repeat_interleave(3, dim=0))
    assert Guidance().repeat_interleave(3) == Guidance()


# ------------------------------------------------------------------------------------------------ the conv launch plan (ccdm_conv_plan)
# The launch rules that read the batch size, asked of the library instead of restated: the tests of tests/test_batch_rules.py hold both
# sides of each threshold to equal bits on the GPU; these hold the thresholds themselves, and what the BASELINE configurations run.
@pytest.fixture(scope="module")
def plan_util():
    import __graft_entry__ as g
    g.build()
    from tests import plan_util as PU
    return PU


def lidc_spec():
    return P.make_unet_spec(image_size=128, in_channels=3, out_channels=2, **LIDC_BP)


def c4_spec():
    fce = dict(type="dino", channels=384, output_stride=8, scale="single", target_layer=10)
    return P.make_unet_spec(image_size=256, in_channels=23, out_channels=20, feature_cond_encoder=fce, **LIDC_BP)


def test_conv_plan_symbol_declared_bound_and_built(plan_util):
    """ccdm_conv_plan is declared, bound (hip.SIGNATURES, hip.ConvPlanInfo with the C compiler's layout) and built under the unchanged ABI
    number; it refuses null arguments and the shapes ccdm_conv2d refuses, launches nothing and follows no pointer (every pointer field of
    these calls is the same invalid address)."""
    from tests.sampler_util import assert_symbol_declared_bound_and_built
    lib = assert_symbol_declared_bound_and_built("ccdm_conv_plan", 2, "ccdm_conv.hip")
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ccdm_hip.h"
    int main(){ printf("%zu %zu %zu %zu %zu\n", sizeof(ccdm_conv_plan_info), offsetof(ccdm_conv_plan_info, ntiles_per_block),
                       offsetof(ccdm_conv_plan_info, out_slices), offsetof(ccdm_conv_plan_info, grid_x), offsetof(ccdm_conv_plan_info, lds_bytes));
                return 0; }'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    I = hip.ConvPlanInfo
    assert out == [ctypes.sizeof(I), I.ntiles_per_block.offset, I.out_slices.offset, I.grid_x.offset, I.lds_bytes.offset]
    assert (hip.CONV_KERNEL_GENERAL, hip.CONV_KERNEL_KS, hip.CONV_KERNEL_UPCONV, hip.CONV_KERNEL_1X1, hip.CONV_KERNEL_1X1_MULTI) == (0, 1, 2, 3, 4)
    a, info = plan_util.conv_args(2, 32, 32, 32, 32), hip.ConvPlanInfo()
    assert lib.ccdm_conv_plan(None, ctypes.byref(info)) < 0 and "null" in hip.last_error()
    assert lib.ccdm_conv_plan(ctypes.byref(a), None) < 0 and "null" in hip.last_error()
    assert lib.ccdm_conv_plan(ctypes.byref(a), ctypes.byref(info)) == 0
    assert info.out_slices == lib.ccdm_conv_out_slices(ctypes.byref(a)) == 4 and (info.grid_x, info.grid_y, info.block) == (8, 1, 256)
    for change, text in ((dict(k=5), "ksize"), (dict(c0=30), "multiples of 4"), (dict(c0=48, gn=True), "GroupNorm(32, 48)"),
                         (dict(k=1, stride=2), "stride 2"), (dict(c0=16, c1=16, prec=hip.PREC_F32), "chunk")):
        b = plan_util.conv_args(*[change.pop(f, v) for f, v in (("N", 2), ("H", 32), ("W", 32), ("c0", 32), ("cout", 32), ("k", 3))], **change)
        assert lib.ccdm_conv_plan(ctypes.byref(b), ctypes.byref(info)) < 0 and text in hip.last_error(), (text, hip.last_error())
    # every kernel family is reported
    fam = {name: plan_util.plan(*shape, **kw)["kernel"] for name, shape, kw in (
        ("general", (2, 128, 128, 32, 32), dict(gn=True, act=hip.ACT_SILU)), ("ks", (2, 8, 8, 128, 128), dict(gn=True, act=hip.ACT_SILU)),
        ("upconv", (2, 16, 16, 64, 64), dict(up=2)), ("1x1", (2, 8, 8, 128, 128, 1), dict(resid=True)),
        ("1x1_multi", (64, 16, 16, 96, 288, 1), dict(gn=True, want_stats=False)))}
    assert fam == {"general": hip.CONV_KERNEL_GENERAL, "ks": hip.CONV_KERNEL_KS, "upconv": hip.CONV_KERNEL_UPCONV, "1x1": hip.CONV_KERNEL_1X1,
                   "1x1_multi": hip.CONV_KERNEL_1X1_MULTI}
    # the diagnostic bit routes every one of them to the general kernel
    assert plan_util.plan(2, 8, 8, 128, 128, 1, resid=True, diag=hip.DIAG_GENERAL_KERNEL)["kernel"] == hip.CONV_KERNEL_GENERAL


@pytest.mark.parametrize("prec", [hip.PREC_F16X3, hip.PREC_F32], ids=["f16x3", "f32"])
@pytest.mark.parametrize("H,W", [(48, 128), (44, 100)])
def test_conv_plan_two_n_tiles_per_block_threshold(plan_util, H, W, prec):
    """The general kernel computes two n-tiles per block exactly when the padded tile count is even and N * slices * (ntiles / 2) >= 512:
    the table of tests/plan_util.py (24 wide tiles and 24 slices per sample) on both sides of the threshold, in both precisions, for the
    operand sets tests/test_batch_rules.py runs.  Crossing it also moves a fused 1x1 skip from wide core-only chunks to narrow ones."""
    for cout, ntiles, n2, n1 in plan_util.NI_TABLE:
        for N, ni in ([(1, 1), (3, 1), (21, 1), (22, 1), (64, 1), (1000, 1)] if n2 is None else [(1, 1), (3, 1), (n1, 1), (n2, 2), (4 * n2, 2)]):
            p = plan_util.plan(N, H, W, 64, cout, gn=True, act=hip.ACT_SILU, emb=True, prec=prec)
            assert (p["kernel"], p["tile_h"], p["tile_w"], p["slices"], p["out_slices"]) == (hip.CONV_KERNEL_GENERAL, 8, 32, 24, 24), p
            assert (p["ntiles"], p["ntiles_per_block"]) == (ntiles, ni), (cout, N, p)
            assert (p["grid_x"], p["grid_y"], p["block"]) == (24 * N, ntiles // ni, 256)
            assert p["core_unmasked"] == int(W % 32 == 0) and p["chunk"] == (32 if prec == hip.PREC_F32 else 16) and not p["tap_split"]
    for kw in (dict(c1=32 if prec != hip.PREC_F32 else 64, gn=True, act=hip.ACT_SILU, emb=True), dict(gn=True, act=hip.ACT_SILU, resid=True),
               dict(gn=True, act=hip.ACT_SILU, film=True), dict(k=1, c1=32 if prec != hip.PREC_F32 else 64), dict(gn=True, act=hip.ACT_SILU, skip=(64, 64))):
        lo, hi = (plan_util.plan(N, H, W, 64, 64, kw.get("k", 3), prec=prec, **{f: v for f, v in kw.items() if f != "k"}) for N in (21, 22))
        assert (lo["kernel"], lo["ntiles_per_block"], hi["kernel"], hi["ntiles_per_block"]) == (hip.CONV_KERNEL_GENERAL, 1, hip.CONV_KERNEL_GENERAL, 2), kw
        if "skip" in kw:
            assert (lo["skip_wide"], hi["skip_wide"]) == ((1, 0) if prec == hip.PREC_F16X3 else (0, 0))
    # upsample on load from half the size; 16 -> 128 channels
    lo, hi = (plan_util.plan(N, H // 2, W // 2, 32, 64, up=1, gn=True, act=hip.ACT_SILU, emb=True, prec=prec) for N in (21, 22))
    assert (lo["ntiles_per_block"], hi["ntiles_per_block"], hi["slices"], hi["tile_w"]) == (1, 2, 24, 32)
    lo, hi = (plan_util.plan(N, H, W, 16, 128, prec=prec) for N in (10, 11))
    assert (lo["ntiles_per_block"], hi["ntiles_per_block"]) == (1, 2)


def test_conv_plan_latency_slicing_reaches_two_n_tiles_at_batch_8(plan_util):
    """fine_slices = 2 gives a 128x128 conv 64 one-tile slices: 8 * 64 * 1 = 512 blocks of two n-tiles for 32 -> 64 at N = 8, where the
    default slicing (12 slices) keeps one n-tile per block; at N = 2 both run one."""
    fine, dflt = (plan_util.plan(8, 128, 128, 32, 64, fine=f) for f in (2, 0))
    assert (fine["slices"], fine["ntiles_per_block"], dflt["slices"], dflt["ntiles_per_block"]) == (64, 2, 12, 1)
    assert [plan_util.plan(2, 128, 128, 32, 64, fine=f)["ntiles_per_block"] for f in (2, 0)] == [1, 1]
    assert plan_util.plan(7, 128, 128, 32, 64, fine=2)["ntiles_per_block"] == 1


def test_conv_plan_of_the_baseline_configurations(plan_util):
    """What the BASELINE configurations run, from make_unet_spec's layers: no conv of the LIDC network reaches two n-tiles per block at
    N = 64 (its wide-tile layers have one n-tile, or too few blocks at 32x32); C4's 64-channel convs at 64x128 run two at N = 16 and one
    at N = 8 — the shard of a two-rank run; beside them only the qkv convs on the 1x1 kernel's n-tile walk differ between the two batches."""
    lidc = plan_util.spec_conv_calls(lidc_spec(), 64, 128, 128, 4)
    assert len(lidc) == 86 and lidc[0][0] == "input_blocks.0.0" and lidc[-1][0] == "out.2"
    for name, a in lidc:
        p = plan_util.plan_dict(hip.conv_plan(a))
        if p["kernel"] == hip.CONV_KERNEL_GENERAL:      # (the Upsample convs run ccdm_upconv.hip, whose ctb rule has its own test at N = 64)
            assert a.up != 2 and p["ntiles_per_block"] == 1, (name, p)
        if p["kernel"] == hip.CONV_KERNEL_GENERAL and p["tile_w"] == 32:
            assert p["ntiles"] == 1 or a.N * p["slices"] * (p["ntiles"] // 2) < 512, (name, p)
    wide_two = [n for n, a in lidc if hip.conv_plan(a).tile_w == 32 and hip.conv_plan(a).ntiles > 1]
    assert wide_two and all(hip.conv_plan(a).slices == 4 for n, a in lidc if n in wide_two)      # the 32x32 stage: 64 * 4 * 1 = 256 blocks
    c4 = {N: plan_util.spec_conv_calls(c4_spec(), N, 256, 512, 24) for N in (16, 8)}
    changed = []
    for (name, a16), (name8, a8) in zip(c4[16], c4[8]):
        p16, p8 = plan_util.plan_dict(hip.conv_plan(a16)), plan_util.plan_dict(hip.conv_plan(a8))
        assert name == name8
        if p16["ntiles_per_block"] != p8["ntiles_per_block"] and name.endswith(".qkv"):
            assert p16["kernel"] == hip.CONV_KERNEL_1X1_MULTI, name          # the n-tile walk of the 1x1 kernel (its own tests)
        elif p16["ntiles_per_block"] != p8["ntiles_per_block"]:
            changed.append(name)
            assert (p16["kernel"], p8["kernel"]) == (hip.CONV_KERNEL_GENERAL, hip.CONV_KERNEL_GENERAL), name
            assert (a16.Hout, a16.Wout, a16.Cout, p16["tile_w"], p16["slices"]) == (64, 128, 64, 32, 32), name
            assert (p16["ntiles_per_block"], p8["ntiles_per_block"]) == (2, 1), name
    at_level = [n for n, a in c4[16] if (a.Hout, a.Wout, a.Cout, a.up, a.stride) == (64, 128, 64, 0, 1) and a.ksize == 3]
    assert changed == at_level and len(changed) >= 8, (changed, at_level)


def test_conv_plan_1x1_multi_tile_walk(plan_util):
    """ntb of the LDS-free 1x1 kernel without output statistics, (N * pixel blocks * tiles + 256) / 512 clamped to [1, tiles]: the cases of
    tests/test_batch_rules.py (an odd ntb with a ragged last group, a last group of one, all tiles of the layer in one block, one k-step),
    the plain kernel below ntb = 2 and whenever statistics are wanted, with or without GroupNorm on load."""
    for c0, cout, H, W, N, ntb in plan_util.CONV1X1_MULTI_CASES:
        if N is None:
            N = plan_util.smallest_batch_with_ntb(c0, cout, H, W, ntb)
            assert N == 192
        for gn in ((False, True) if c0 % 32 == 0 else (False,)):
            p = plan_util.plan(N, H, W, c0, cout, 1, gn=gn, want_stats=False)
            ppb = 128 if H * W % 128 == 0 else (64 if H * W % 64 == 0 else 32)
            assert (p["kernel"], p["ntiles_per_block"], p["tile_w"], p["block"]) == (hip.CONV_KERNEL_1X1_MULTI, ntb, ppb, ppb * 2), (c0, cout, N, p)
            assert (p["slices"], p["grid_x"], p["grid_y"]) == (H * W // ppb, N * H * W // ppb, -(-(cout // 32) // ntb))
            small = plan_util.plan(2, H, W, c0, cout, 1, gn=gn, want_stats=False)
            assert (small["kernel"], small["ntiles_per_block"], small["grid_y"]) == (hip.CONV_KERNEL_1X1, 1, cout // 32)
            assert plan_util.plan(N, H, W, c0, cout, 1, gn=gn, resid=True, want_stats=False)["ntiles_per_block"] == ntb
        assert plan_util.plan(N, H, W, c0, cout, 1)["ntiles_per_block"] == 1                  # statistics wanted: one n-tile per block
    assert plan_util.plan(64, 8, 12, 64, 384, 1, want_stats=False)["block"] == 64             # one-wave blocks
    with pytest.raises(hip.CcdmHipError, match=r"GroupNorm\(32, 16\)"):                        # the one-k-step case has no GroupNorm form
        plan_util.plan(192, 16, 16, 16, 64, 1, gn=True, want_stats=False)


def test_conv_plan_depends_on_the_batch_only_through_the_block_partition(plan_util):
    """Over every conv of the LIDC and C4 networks and the threshold cases: the kernel family, the tile geometry, the chunk width, the
    tap split, the slices and the statistics partials of a call are the same at every N; only the n-tiles per block (with them the grid,
    the LDS of the staged B chunk, the 1x1 kernel's multi form and the wide skip chunks, which need one n-tile per block) may differ."""
    fixed = ("tile_h", "tile_w", "chunk", "ntiles", "tap_split", "slices", "out_slices", "core_unmasked", "block")
    family = {hip.CONV_KERNEL_1X1_MULTI: hip.CONV_KERNEL_1X1}
    calls = plan_util.spec_conv_calls(lidc_spec(), 1, 128, 128, 4) + plan_util.spec_conv_calls(c4_spec(), 1, 256, 512, 24)
    calls += [("table", plan_util.conv_args(1, H, W, 64, cout, gn=True, act=hip.ACT_SILU, skip=(64, 64), prec=prec))
              for H, W in plan_util.NI_GEOMETRIES for cout, *_ in plan_util.NI_TABLE for prec in (hip.PREC_F16X3, hip.PREC_F32)]
    calls += [("1x1", plan_util.conv_args(1, H, W, c0, cout, 1, want_stats=False)) for c0, cout, H, W, _, _ in plan_util.CONV1X1_MULTI_CASES]
    calls += [("fine", plan_util.conv_args(1, 128, 128, 32, 64, fine=2)), ("up", plan_util.conv_args(1, 32, 32, 64, 64, up=2))]
    seen_ni = set()
    for name, a in calls:
        base = None
        for N in (1, 2, 3, 5, 6, 8, 10, 11, 16, 21, 22, 27, 64, 128, 192, 1024):
            a.N = N
            p = plan_util.plan_dict(hip.conv_plan(a))
            key = tuple(p[f] for f in fixed) + (family.get(p["kernel"], p["kernel"]),)
            base = base or key
            assert key == base, (name, N, p)
            assert p["grid_x"] == N * p["slices"] and p["grid_y"] * p["ntiles_per_block"] >= (a.Cout // 32 if p["kernel"] != hip.CONV_KERNEL_GENERAL else p["ntiles"])
            assert not p["skip_wide"] or p["ntiles_per_block"] == 1, (name, N, p)
            seen_ni.add((p["kernel"], p["ntiles_per_block"]))
    assert {(hip.CONV_KERNEL_GENERAL, 1), (hip.CONV_KERNEL_GENERAL, 2), (hip.CONV_KERNEL_UPCONV, 2), (hip.CONV_KERNEL_1X1_MULTI, 5)} <= seen_ni


# ------------------------------------------------------------------------------------------------ the ledger of conv launch plans
# Every signature (tests/plan_util.signature) a shipped network emits has a kernel-level float64 case in plan_util.PLAN_CASES, which
# tests/test_conv_plan_coverage.py runs on the GPU.  Nothing is exempt: a signature without a case fails the first test below.
@pytest.fixture(scope="module")
def ledger(plan_util):
    """(signature -> layers that have it over plan_util.shipped_conv_calls(), the signature of every case of the table)"""
    shipped = {}
    for tag, name, a in plan_util.shipped_conv_calls():
        shipped.setdefault(plan_util.signature_of(a), []).append(tag + ":" + name)
    return shipped, [c.signature() for c in plan_util.PLAN_CASES]


def missing_signatures(shipped, case_signatures):
    """the shipped signatures no case has, each with up to three layers that have it"""
    have = set(case_signatures)
    return ["%r: %s" % (s, ", ".join(layers[:3])) for s, layers in shipped.items() if s not in have]


def test_every_shipped_conv_signature_has_a_kernel_case(plan_util, ledger):
    """The signature set of shipped_conv_calls() — LIDC at every fine_slices the model can choose, C4 at both image sizes, the
    resblock_updown and the use_scale_shift_norm networks, each in both precisions — is a subset of the signature set of PLAN_CASES."""
    shipped, cases = ledger
    assert len(shipped) > 100 and sum(map(len, shipped.values())) == len(plan_util.shipped_conv_calls())
    missing = missing_signatures(shipped, cases)
    assert not missing, "%d shipped conv signatures have no kernel-level case in plan_util.PLAN_CASES:\n%s" % (len(missing), "\n".join(missing))


def test_signature_is_a_function_of_the_layer_never_of_the_batch(plan_util):
    """a layer keeps its signature at every batch size (what lets a case run at N = 2 and its last sample alone)"""
    for tag, name, a in plan_util.shipped_conv_calls()[::7]:
        want = plan_util.signature_of(a)
        for N in (1, 2, 3, 22, 64, 1024):
            a.N = N
            assert plan_util.signature_of(a) == want, (tag, name, N)


def test_plan_case_table_has_one_case_per_signature_and_no_unexplained_case(plan_util, ledger):
    """No two cases share a signature (or an id); a case either has a signature that ships or says with edge="..." why it is there, and an
    edge case has a signature that does not ship.  A shrunk case runs a smaller image than its layer, with the layer's signature."""
    shipped, cases = ledger
    table = plan_util.PLAN_CASES
    assert len(set(cases)) == len(cases) == len(table), [c.id for c, s in zip(table, cases) if cases.count(s) > 1]
    assert len({c.id for c in table}) == len(table)
    for c, s in zip(table, cases):
        assert (s in shipped) == (c.edge is None), (c.id, s, c.edge)
        assert c.refused is None or c.edge, c.id
        if c.shrink:
            h, w = c.shape()
            assert h * w <= c.H * c.W and s == plan_util.signature_of(c.args(H=c.H, W=c.W)), (c.id, h, w)


def test_plan_case_ledger_negative_control(plan_util, ledger):
    """Each case that is no edge case is load-bearing: with it deleted from the table the ledger test fails, naming its signature; with an
    edge case deleted it still passes."""
    shipped, cases = ledger
    assert not missing_signatures(shipped, cases)
    for i, c in enumerate(plan_util.PLAN_CASES):
        missing = missing_signatures(shipped, cases[:i] + cases[i + 1:])
        if c.edge:
            assert not missing, c.id
        else:
            assert len(missing) == 1 and missing[0].startswith(repr(cases[i])), (c.id, missing)


def test_philox_keys_passes_and_tag_ranges_never_meet():
    """The host's part of keeping the sampler's noise streams apart: `_philox_key` over calls 0 .. 4095 of three seeds (label_bound takes
    its keys from the same function of its own counter) and `pass_key` over p = 0 .. 63 of each of them are pairwise distinct, none of them
    is the key of another seed's call 0, and the fourth counter words of the epilogue (k / 4 < 64), the clamp (0x80000000 | k / 4), the
    renoise (0x40000000 | k / 4) and the bound's noising (0x20000000 | k / 4) are pairwise disjoint for every k / 4 < 64."""
    seeds = (0, 99, 0xFEEDFACE12345678)
    stub = type("M", (), {"philox_seed": 0, "philox_call": 0})()
    keys = {}
    for seed in seeds:
        stub.philox_seed = seed
        keys[seed] = [models.DenoisingModel._philox_key(stub, call) for call in range(4096)]
        assert keys[seed][0] == seed and all(0 <= k < 2 ** 64 for k in keys[seed])
    every = [models.pass_key(k, p) for seed in seeds for k in keys[seed] for p in range(64)]
    assert len(every) == 3 * 4096 * 64 and len(set(every)) == len(every)
    assert [models.pass_key(k, 0) for k in keys[99][:8]] == keys[99][:8]
    # a seed's call 0 uses the seed itself as its key: no other (seed, call, pass) may land on it
    for seed in seeds:
        assert every.count(seed) == 1 and every.index(seed) == seeds.index(seed) * 4096 * 64
    ranges = [{tag | kq for kq in range(64)} for tag in (0, 0x80000000, 0x40000000, 0x20000000)]
    assert all(len(r) == 64 for r in ranges) and len(set().union(*ranges)) == 4 * 64
    assert (hip.MAX_CLASSES + 3) // 4 <= 64          # every class count the kernels take keeps k / 4 below 64
