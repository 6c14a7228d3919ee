"""What the guided-sampling test files (test_known_labels, test_resample_jumps, test_evidence_sampling) share: the small model and its
sampler fixture, the numpy restatements of the two-valued Exp(1) race built on the oracle's Philox4x32-10, and the CPU checks that every
step symbol gets (declared, bound and built; handed through by sample_sharded).  A plain module: no fixture, no pytest setting."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import ccdm_oracle as O
from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE = 255
TAG_RENOISE, TAG_CLAMP = 0x40000000, 0x80000000
# the 32x32 two-level network of the sub-batch parity test (test_hip_parity.test_substreams_do_not_change_the_samples), T = 6:
# t = None walks its 6 rows, t = 10004 walks it strided, t = 6, 4, 3, 1
SMALL_BP = dict(base_channels=32, channel_mult=(1, 2), attention_resolutions=[2], num_heads=1, num_head_channels=32, softmax_output=True)
SMALL_CFG = dict(num_heads=1, num_head_channels=32)
T_SMALL, H, W = 6, 32, 32
T_STRIDED = torch.as_tensor(10004)
DEV = torch.device("cuda:0")
SEED = 0xFEEDFACE12345678


def small_model(K, vote="majority", seed=3, **bp):
    m = build_model(T_SMALL, "cosine", {"s": 0.008}, [(1, H, W), (K, H, W)], (1, H, W), "unet_openai", dict(SMALL_BP, **bp), "datasets.lidc",
                    vote, None)
    sd = {k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(m.unet.spec, seed).items()}
    m.unet.load_state_dict(sd, strict=True)
    return m, sd


def settings(model, **kw):
    for k, v in kw.items():
        setattr(model, k, v)


def onehot_np(idx, K):
    return np.arange(K)[None, None, :] == idx[..., None]


def probabilities(c, K):
    """(p_hit, p_miss) = (p_stay, p_move) as the host forms them: in float64, each rounded to fp32 once"""
    p_miss = (1.0 - float(c)) / K
    return np.float32(float(c) + p_miss), np.float32(p_miss)


def race_restatement(own, K, c, step_row, seed, sample0, tag):
    """argmax_k p_k / E_k with p_k = p_hit for k == own[n, pixel], p_miss otherwise, following oracle.philox_exponential: the same
    bits -> uniform -> -log map in fp32, counter word 3 = tag | k // 4, the division in fp32, the first maximum wins.
    own: [N,HW] integer array of classes < K."""
    N, HW = own.shape
    p_hit, p_miss = probabilities(c, K)
    pix = np.arange(HW, dtype=np.uint32)[None, :, None]
    smp = (np.arange(N, dtype=np.uint32) + np.uint32(sample0))[:, None, None]
    kq = (np.uint32(tag) | (np.arange(K, dtype=np.uint32) // 4))[None, None, :]
    ctr = np.stack(np.broadcast_arrays(pix, smp, np.uint32(step_row), kq), axis=-1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    blk = O.philox4x32_10(ctr, key)
    word = np.take_along_axis(blk, np.broadcast_to((np.arange(K) % 4)[None, None, :, None], (N, HW, K, 1)).astype(np.int64), axis=-1)[..., 0]
    u = ((word >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    e = (-np.log(u.astype(np.float32))).astype(np.float32)
    p = np.where(np.arange(K)[None, None, :] == own[..., None], p_hit, p_miss).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (p / e).astype(np.float32)
    q = np.where(np.isnan(q), -np.inf, q)                  # `qv > best` is false for a NaN (0 / 0): it never wins
    return np.argmax(q, axis=-1).astype(np.int64)


def renoise_restatement(xt, K, r, step_row, seed, sample0):
    """What ccdm_renoise_step leaves in xt: every pixel redrawn, own class = xt."""
    return race_restatement(xt, K, r, step_row, seed, sample0, TAG_RENOISE)


def clamp_restatement(known, xt, K, c, step_row, seed, sample0):
    """What ccdm_known_labels_step leaves in xt in mode STEP_SAMPLE: the race at the known pixels (own class = the label), xt at the free
    ones (255, or any byte that is no class).  known, xt: [N,HW] integer arrays."""
    draw = race_restatement(np.where(known < K, known, 0), K, c, step_row, seed, sample0, TAG_CLAMP)
    return np.where(known < K, draw, xt).astype(np.int64)


def load_lib():
    """The body of the test files' module-scoped `lib` fixtures."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    return hip.load()


def make_sampler(K):
    """The body of the test files' module-scoped `sampler` fixtures.  K = 2: stem conv and fused head-and-posterior launch (x_t travels
    as the uint8 index only); K = 5: the general epilogue, which writes the one-hot into the stem's input.  `ev`: for the caller to fill."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    model, sd = small_model(K)
    model = model.to(DEV).eval()
    model.rng, model.philox_seed, model.philox_advance = "philox", 99, False          # every call replays call 0's stream
    rng = np.random.default_rng(40 + K)
    N = 4
    image = torch.from_numpy(rng.uniform(-1, 1, (N, 1, H, W)).astype(np.float32))
    x = O.one_hot_bchw(torch.from_numpy(rng.integers(0, K, (N, H, W))), K)
    labels = torch.from_numpy(rng.integers(0, K, (N, H, W)))
    known = torch.where(torch.from_numpy(rng.random((N, H, W)) < 0.3), labels, torch.full_like(labels, FREE))
    eng = model._engine(x.to(DEV), image.to(DEV), None)
    assert eng.head_fused == (K == 2) and eng.stem_onehot_on_load == (K == 2)
    return dict(model=model, sd=sd, K=K, N=N, image=image.to(DEV), x=x.to(DEV), labels=labels, known=known, image_cpu=image, x_cpu=x, ev=None)


CTYPE_OF = {"int": C.c_int, "float": C.c_float, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}


def assert_symbol_declared_bound_and_built(symbol, nargs, source):
    """hip.py binds the symbol with argtypes that match the header's declaration (`nargs` of them), `source` defines it and is in the
    build list, and the library built from it (cross-compiled for gfx950 by build()) exports it under the unchanged ABI number.
    Returns the library."""
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "not declared in include/ccdm_hip.h"
    want = []
    for arg in m.group(1).split(","):
        words = arg.replace("*", " * ").split()
        want.append(C.c_void_p if "*" in words else CTYPE_OF[[w for w in words if w != "const"][0]])
    res, args = hip.SIGNATURES[symbol]
    # (a pointer to an argument struct may be bound by its type, C.POINTER(hip.ConvArgs), as ccdm_conv_out_slices is: still a pointer)
    args = [C.c_void_p if isinstance(t, type) and issubclass(t, C._Pointer) else t for t in args]
    assert res is C.c_int and args == want and len(args) == nargs
    assert source in hip.SOURCES and symbol in open(os.path.join(hip.CSRC, source)).read()
    assert hip.ABI_VERSION == 11 and hip.MAX_CLASSES == 255
    import __graft_entry__ as g
    g.build()
    lib = hip.load()
    assert hasattr(lib, symbol) and lib.ccdm_version() == 11
    return lib


def sample_sharded_keywords(**kw):
    """The keywords distributed.sample_sharded hands to the model (a stub that records them) for a 3-sample call with `kw`."""
    from ccdm_stochastic_segmentation_amd.distributed import sample_sharded
    seen = {}

    class Stub:
        rng, sample_offset, noise_slice = "philox", 0, None

        def __call__(self, x, cond, fc, **kw_):
            seen.update(kw_)
            return {"diffusion_out": x}
    sample_sharded(Stub(), torch.zeros(3, 2, 4, 4), torch.zeros(3, 1, 4, 4), **kw)
    return seen
