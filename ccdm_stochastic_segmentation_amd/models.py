"""Drop-in host interface of the sampler: same names, arguments and error behaviour as the reference's
``ddpm.models`` package for the hot path, backed by the HIP engine.

    build_model(...)                         /root/reference/ddpm/models/builder.py:14-51
    DenoisingModel.forward(x, condition, feature_condition=None, t=None, label_ref_logits=None, validation=False)
                                             /root/reference/ddpm/models/diffusion_denoising.py:144-159
    DiffusionModel (schedule buffers)        /root/reference/ddpm/models/diffusion_denoising.py:42-70
    UNetModel (parameter container with the reference's state_dict key layout)
    OneHotCategoricalBCHW                    /root/reference/ddpm/models/one_hot_categorical.py:10-54

Inference only: there is no autograd through the HIP kernels.
"""
from __future__ import annotations

import logging
import math
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union, cast

import numpy as np
import torch
from torch import Tensor, nn

from . import guidance as G
from . import hip
from .engine import SamplerEngine, TileCanvas
from .guidance import GUIDANCE_KEYWORDS, KNOWN_FREE, VIEW_FLIPS, Guidance, resample_walk, tile_origins  # noqa: F401  (their home is guidance.py)
from .unet_spec import UNetSpec, make_unet_spec

LOGGER = logging.getLogger(__name__)

__all__ = ["build_model", "DiffusionModel", "DenoisingModel", "UNetModel", "OneHotCategoricalBCHW",
           "linear_schedule", "cosine_schedule", "step_values", "resample_walk", "pass_key",
           "bound_timesteps", "bound_prior", "bound_rows"]


# --------------------------------------------------------------------------------------------------
# schedules (host, once per model) — same expressions, same dtypes as the reference so the three
# buffers are bit-identical (diffusion_denoising.py:18-39)
# --------------------------------------------------------------------------------------------------
def linear_schedule(time_steps: int, start=1e-2, end=0.2) -> Tuple[Tensor, Tensor, Tensor]:
    betas = torch.linspace(start, end, time_steps)
    alphas = 1 - betas
    return betas, alphas, torch.cumprod(alphas, dim=0)


def cosine_schedule(time_steps: int, s: float = 8e-3) -> Tuple[Tensor, Tensor, Tensor]:
    s = 0.008                                     # the reference ignores the argument (:27)
    t = torch.arange(0, time_steps)
    cumalphas = torch.cos(((t / time_steps + s) / (1 + s)) * (math.pi / 2)) ** 2

    def f(u):
        return math.cos((u + s) / (1.0 + s) * math.pi / 2) ** 2

    betas = torch.tensor([min(1 - f((i + 1) / time_steps) / f(i / time_steps), 0.999) for i in range(time_steps)])
    return betas, 1 - betas, cumalphas


def step_values(time_steps: int, init_t: Optional[int]) -> List[int]:
    """Step list of forward_denoising (:178-187): full range, a shortened range, or (init_t > 10000) a
    strided walk of K = init_t % 10000 steps from T to 1 (python round = half-to-even)."""
    if init_t is None:
        init_t = time_steps
    if init_t > 10000:
        k = init_t % 10000
        assert 0 < k <= time_steps
        if k == time_steps:
            return list(range(k, 0, -1))
        vals = [round(v) for v in np.linspace(time_steps, 1, k)]
        LOGGER.warning(f"Override default {time_steps} time steps with {len(vals)}.")
        return vals
    return list(range(init_t, 0, -1))


PASS_STRIDE = 0xD1342543DE82EF95         # pass_key's Weyl increment: odd, and not the call counter's 0x9E3779B97F4A7C15


def pass_key(key: int, p: int) -> int:
    """Philox key of pass `p` of a table row (p = the number of earlier visits of the row in a resampled walk): the call's key itself
    for p = 0, else the splitmix64 finaliser of key + PASS_STRIDE * p.  A revisit must not replay the first visit's noise: the epilogue
    keys its draws by the table row.  The increment is NOT the one DenoisingModel._philox_key steps (philox_seed, philox_call) by: call 0
    uses the seed itself as its key, so with one increment for both, pass p of call 0 would run under the key of call p and replay that
    call's first visit of the row, pixel for pixel (tests/test_host_logic.py holds calls and passes apart)."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    if int(p) == 0:
        return key
    z = (key + PASS_STRIDE * int(p)) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


# --------------------------------------------------------------------------------------------------
# the label bound's host arithmetic (DenoisingModel.label_bound; include/ccdm_hip.h has the definition)
# --------------------------------------------------------------------------------------------------
def bound_timesteps(T: int, timesteps, key: int, n_labels: int) -> Tuple[np.ndarray, np.ndarray]:
    """The estimator over t: (t int64 [n_labels, M], weight float64 [n_labels, M]).  None: every t in 1..T at weight 1.  A sequence:
    those t at weight 1 (a partial sum unless it covers 1..T).  An int M <= T: stratified — stratum j = (floor(j T / M), floor((j + 1) T
    / M)], one t drawn uniformly per label and stratum from np.random.Generator(np.random.Philox(key)) (labels outer, strata inner),
    weighted by the stratum's size: unbiased in t, reproducible from the key."""
    T, n_labels = int(T), int(n_labels)
    if T < 1 or n_labels < 1:
        raise ValueError(f"bound_timesteps: T = {T}, n_labels = {n_labels}")
    if timesteps is None:
        t = np.arange(1, T + 1, dtype=np.int64)
        return np.tile(t, (n_labels, 1)), np.ones((n_labels, T), dtype=np.float64)
    if isinstance(timesteps, (int, np.integer)) and not isinstance(timesteps, bool):
        M = int(timesteps)
        if not 1 <= M <= T:
            raise ValueError(f"timesteps: {M} strata for T = {T} (expected 1 <= M <= T)")
        edges = np.array([(j * T) // M for j in range(M + 1)], dtype=np.int64)
        rng = np.random.Generator(np.random.Philox(key=int(key) & 0xFFFFFFFFFFFFFFFF))
        t = rng.integers(edges[None, :-1] + 1, edges[None, 1:] + 1, size=(n_labels, M), dtype=np.int64)
        return t, np.tile((edges[1:] - edges[:-1]).astype(np.float64), (n_labels, 1))
    try:
        ts = [int(v) for v in timesteps]
        exact = all(float(v) == int(v) for v in timesteps)
    except (TypeError, ValueError):
        raise ValueError(f"timesteps: expected None, an int or a sequence of ints, got {timesteps!r}") from None
    if not ts or not exact or any(not 1 <= v <= T for v in ts):
        raise ValueError(f"timesteps: every t must be an integer in 1..{T}, got {list(timesteps)!r}")
    if len(set(ts)) != len(ts):
        raise ValueError(f"timesteps: repeated timestep in {ts!r}")
    return np.tile(np.array(ts, dtype=np.int64), (n_labels, 1)), np.ones((n_labels, len(ts)), dtype=np.float64)


def bound_prior(cumalpha_T: float, K: int) -> float:
    """L_T per counted pixel of weight 1: KL(q(x_T | x_0) || uniform) = p_hit log(K p_hit) + (K - 1) p_miss log(K p_miss) in float64
    (0 log 0 = 0), p_miss = (1 - cumalpha_T) / K, p_hit = cumalpha_T + p_miss."""
    c, K = float(cumalpha_T), int(K)
    p_miss = (1.0 - c) / K
    p_hit = c + p_miss
    return sum(n * p * math.log(K * p) for n, p in ((1, p_hit), (K - 1, p_miss)) if p > 0.0 and n > 0)


def bound_rows(timesteps: np.ndarray, draws: int, rows: int, K: int, cumalphas: Sequence[float], coeffs: Callable[[int], Tuple[float, float]],
               n_label_rows: Optional[int] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The packing of the (label, timestep, draw) triples — labels outer, draws inner — into passes of `rows` engine rows, the tail
    padded with idle rows.  timesteps: int [n_labels, M] (bound_timesteps); cumalphas[t - 1] = cumalpha_t; coeffs(t) = posterior_coeffs.
    Per pass (table, slot): `table` the `rows` records of hip.bound_dtype() — p_hit / p_miss formed in float64 and rounded to fp32 once,
    sample = label * draws + draw, label_row = label — and `slot` int64 [rows], (label * M + m) * draws + draw of the triple the row
    holds, -1 for an idle row.  A label row outside [0, n_label_rows) is refused here: the kernels never see one."""
    ts = np.asarray(timesteps)
    draws, rows, K = int(draws), int(rows), int(K)
    if ts.ndim != 2 or draws < 1 or rows < 1:
        raise ValueError(f"bound_rows: timesteps {ts.shape}, draws = {draws}, rows = {rows}")
    n_labels, M = ts.shape
    n_label_rows = n_labels if n_label_rows is None else int(n_label_rows)
    if n_labels > n_label_rows:
        raise ValueError(f"bound_rows: label rows 0..{n_labels - 1} outside [0,{n_label_rows})")
    triples = [(l, m, d) for l in range(n_labels) for m in range(M) for d in range(draws)]
    passes = []
    for p0 in range(0, len(triples), rows):
        table = np.zeros(rows, dtype=hip.bound_dtype())
        table["t"] = hip.BOUND_IDLE
        slot = np.full(rows, -1, dtype=np.int64)
        for n, (l, m, d) in enumerate(triples[p0:p0 + rows]):
            t = int(ts[l, m])
            c = float(cumalphas[t - 1])
            p_miss = (1.0 - c) / K
            a, cm1 = coeffs(t)
            table[n] = (np.float32(c + p_miss), np.float32(p_miss), np.float32(a), np.float32(cm1), t, l * draws + d, l, 0)
            slot[n] = (l * M + m) * draws + d
        passes.append((table, slot))
    return passes


class OneHotCategoricalBCHW:
    """Categorical over dim=1 of a BCHW tensor, sampled as torch.multinomial does: argmax_k p_k / E_k with
    E ~ Exp(1) drawn as one [B*H*W, K] block from the generator of the tensor's device.  Host-side helper
    for callers (x_T is drawn with it on the CPU, evaluate_lidc_uncertainty.py:100); the per-step draws
    inside the loop run in the HIP epilogue."""

    def __init__(self, probs: Optional[Tensor] = None, logits: Optional[Tensor] = None, validate_args=None):
        if (probs is None) == (logits is None):
            raise ValueError("Either `probs` or `logits` must be specified, but not both.")
        if probs is not None and probs.ndim < 2:
            raise ValueError("`probs.ndim` should be at least 2")
        if logits is not None and logits.ndim < 2:
            raise ValueError("`logits.ndim` should be at least 2")
        if probs is not None:
            p = self.channels_last(probs)
            self.probs = p / p.sum(-1, keepdim=True)
        else:
            lg = self.channels_last(logits)
            self.probs = torch.softmax(lg - lg.logsumexp(dim=-1, keepdim=True), dim=-1)

    @staticmethod
    def channels_last(arr: Tensor) -> Tensor:
        return arr.permute((0,) + tuple(range(2, arr.ndim)) + (1,))

    @staticmethod
    def channels_second(arr: Tensor) -> Tensor:
        return arr.permute((0, arr.ndim - 1) + tuple(range(1, arr.ndim - 1)))

    def sample(self, sample_shape=torch.Size(), generator: Optional[torch.Generator] = None) -> Tensor:
        if len(sample_shape) != 0:
            raise NotImplementedError("sample_shape other than () is not used on this path")
        k = self.probs.shape[-1]
        p2d = self.probs.reshape(-1, k)
        q = torch.empty_like(p2d).exponential_(1, generator=generator)
        idx = torch.argmax(p2d / q, dim=-1)
        res = torch.nn.functional.one_hot(idx, k).to(self.probs.dtype).reshape(self.probs.shape)
        return self.channels_second(res)

    def max_prob_sample(self) -> Tensor:
        k = self.probs.shape[-1]
        return self.channels_second(torch.nn.functional.one_hot(self.probs.argmax(dim=-1), k))

    def prob_sample(self) -> Tensor:
        return self.channels_second(self.probs)


class DiffusionModel(nn.Module):
    betas: Tensor
    alphas: Tensor
    cumalphas: Tensor

    def __init__(self, schedule: str, time_steps: int, num_classes: int, schedule_params=None):
        super().__init__()
        fn = {"linear": linear_schedule, "cosine": cosine_schedule}[schedule]
        betas, alphas, cumalphas = fn(time_steps, **schedule_params) if schedule_params is not None else fn(time_steps)
        self.register_buffer("betas", betas)
        self.register_buffer("alphas", alphas)
        self.register_buffer("cumalphas", cumalphas)
        self.num_classes = num_classes

    @property
    def time_steps(self) -> int:
        return len(self.betas)

    def posterior_coeffs(self, t: int) -> Tuple[float, float]:
        """(alpha_t, cumalpha_{t-1}) as theta_post_prob uses them; t == 1 -> (0, 1) (:112-113)."""
        i = t - 1
        if i == 0:
            return 0.0, 1.0
        return float(self.alphas[i]), float(self.cumalphas[i - 1])

    # ------------------------------------------------------------------ training-time forward pieces
    # Same names, arguments and results as the reference's methods (diffusion_denoising.py:72-129); the arithmetic runs in
    # the HIP kernels behind ccdm_mix_uniform / ccdm_theta_post (device tensors only: there is no CPU path).
    @staticmethod
    def _dev(x: Tensor, what: str) -> Tensor:
        if not x.is_cuda:
            raise hip.CcdmHipError(f"{what}: tensors must live on the GPU (the HIP kernels are the only implementation)")
        return x.contiguous().float()

    def _per_sample(self, table: Tensor, t: Tensor, N: int, device) -> Tensor:
        v = table.to(device)[(t.to(device).long() - 1).reshape(-1)].float()
        return (v.expand(N) if v.numel() == 1 else v).contiguous()

    def _coeffs(self, t: Tensor, N: int, device) -> Tuple[Tensor, Tensor]:
        """(alpha_t, cumalpha_{t-1}) per sample with the t == 1 override (:91-94, :110-113)."""
        i = (t.to(device).long() - 1).reshape(-1)
        a = self.alphas.to(device)[i].clone().float()
        c = self.cumalphas.to(device)[i - 1].clone().float()
        a[i == 0] = 0.0
        c[i == 0] = 1.0
        if a.numel() == 1:
            a, c = a.expand(N), c.expand(N)
        return a.contiguous(), c.contiguous()

    def _mix(self, x: Tensor, s: Tensor) -> Tensor:
        x = self._dev(x, "q_xt")
        N, K, H, W = x.shape
        out = torch.empty_like(x)
        lib = hip.load()
        hip.check(lib.ccdm_mix_uniform(x.data_ptr(), s.data_ptr(), N, K, H * W, out.data_ptr(),
                                       torch.cuda.current_stream(x.device).cuda_stream), "mix_uniform")
        return out

    def q_xt_given_xtm1(self, xtm1: Tensor, t: Tensor) -> OneHotCategoricalBCHW:
        """(1 - beta_t) * x_{t-1} + beta_t / K   (:72-78)"""
        s = 1.0 - self._per_sample(self.betas, t, xtm1.shape[0], xtm1.device)
        return OneHotCategoricalBCHW(self._mix(xtm1, s.contiguous()))

    def q_xt_given_x0(self, x0: Tensor, t: Tensor) -> OneHotCategoricalBCHW:
        """cumalpha_t * x_0 + (1 - cumalpha_t) / K   (:80-86)"""
        return OneHotCategoricalBCHW(self._mix(x0, self._per_sample(self.cumalphas, t, x0.shape[0], x0.device)))

    def _theta(self, xt: Tensor, other: Tensor, t: Tensor, prob_mode: int) -> Tensor:
        xt, other = self._dev(xt, "theta_post"), self._dev(other, "theta_post")
        N, K, H, W = xt.shape
        if other.shape != xt.shape:
            raise ValueError(f"theta_post: shapes differ {tuple(xt.shape)} vs {tuple(other.shape)}")
        a, c = self._coeffs(t, N, xt.device)
        out = torch.empty_like(xt)
        lib = hip.load()
        hip.check(lib.ccdm_theta_post(xt.data_ptr(), other.data_ptr(), a.data_ptr(), c.data_ptr(), N, K, H * W, prob_mode,
                                      out.data_ptr(), torch.cuda.current_stream(xt.device).cuda_stream), "theta_post")
        return out

    def theta_post(self, xt: Tensor, x0: Tensor, t: Tensor) -> Tensor:
        """q(x_{t-1} | x_t, x_0)   (:88-97)"""
        return self._theta(xt, x0, t, 0)

    def theta_post_prob(self, xt: Tensor, theta_x0: Tensor, t: Tensor) -> Tensor:
        """sum over x_0 of q(x_{t-1} | x_t, x_0) * theta_x0   (:99-129), O(K) per pixel"""
        return self._theta(xt, theta_x0, t, 1)

    def kl_clamped(self, prob_true: Tensor, prob_pred: Tensor, floor: float = 1e-12) -> Tensor:
        """The diffusion term of the reference's train_step (trainer.py:266-270):
        kl_div(log(clamp(prob_pred, min=floor)), prob_true, reduction='none')."""
        p, q = self._dev(prob_true, "kl_clamped"), self._dev(prob_pred, "kl_clamped")
        if p.shape != q.shape:
            raise ValueError(f"kl_clamped: shapes differ {tuple(p.shape)} vs {tuple(q.shape)}")
        out = torch.empty_like(p)
        hip.check(hip.load().ccdm_kl_clamped(p.data_ptr(), q.data_ptr(), p.numel(), float(floor), out.data_ptr(),
                                             torch.cuda.current_stream(p.device).cuda_stream), "kl_clamped")
        return out


class UNetModel(nn.Module):
    """Parameter container with the reference network's exact state_dict layout (398 tensors for the LIDC
    config), so `load_state_dict(strict=True)` and ignite's `load_objects` work unchanged.  It has no
    torch forward: the forward pass is the HIP op list built by SamplerEngine from these parameters."""

    def __init__(self, spec: UNetSpec):
        super().__init__()
        self.spec = spec
        self.in_channels, self.model_channels, self.out_channels = spec.in_channels, spec.model_channels, spec.out_channels
        self._version_seen = 0
        self._weights_version = 0

        def container_for(path: List[str]) -> nn.Module:
            mod: nn.Module = self
            for part in path:
                if not hasattr(mod, part):
                    mod.add_module(part, nn.Module())
                mod = getattr(mod, part)
            return mod

        for key, shape in spec.param_shapes().items():
            *path, leaf = key.split(".")
            container_for(path).register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.mark_weights_changed())

    def mark_weights_changed(self) -> None:
        self._weights_version += 1

    def _apply(self, fn, *a, **k):   # .to()/.cuda(): parameters are re-created
        r = super()._apply(fn, *a, **k)
        self._weights_version += 1
        return r

    def forward(self, *args, **kwargs):
        raise RuntimeError("UNetModel has no eager forward; call it through DenoisingModel (HIP engine)")


# host-noise staging budget of rng="torch_cpu": the Exp(1) draws are made and uploaded in blocks of whole steps no larger
# than this many bytes (the reference never holds more than one step of noise; one block of a few steps keeps the copies
# large without O(T) memory on the host and the device)
HOST_NOISE_BLOCK_BYTES = 256 << 20


def auto_substreams(N: int, H: int, W: int) -> int:
    """`substreams = 0`: how many concurrent sub-batch streams a batch of N samples of H x W is sampled on."""
    return 2 if (N >= 2 and N * H * W >= 32 * 128 * 128) else 1


def _num_evaluations(value, hi: Optional[int] = None) -> int:
    """`num_evaluations` of the predict_* methods: a whole number of samples from 1, up to `hi` where the summary has a cap."""
    if isinstance(value, bool) or int(value) != value or int(value) < 1 or (hi is not None and int(value) > hi):
        raise ValueError(f"num_evaluations: {value!r} (expected an integer " + (">= 1)" if hi is None else f"in [1, {hi}])"))
    return int(value)


class DenoisingModel(nn.Module):
    """The sampler.  `rng` selects where the Exp(1) noise of the categorical draws comes from:
    "philox" (default) — Philox4x32-10 inside the epilogue kernel, keyed by (pixel, global sample index, step) under a 64-bit key
      derived from (`philox_seed`, `philox_call`): the throughput mode, statistically identical to the reference's draws.
      `philox_call` counts the sampling calls made on this model and advances by one after every `forward_denoising`, so successive
      calls — the batches of an evaluation loop, S calls at batch 1 to draw S samples of one image — see independent noise, like
      successive draws from the reference's generator do.  The key does not depend on how the batch is split over ranks or
      sub-batches (every rank makes the same sequence of calls), so sharding stays invariant; set `philox_call` back (or
      `philox_advance = False`) to replay a call bit for bit.  torch.manual_seed does not reach this stream: seed it with
      `philox_seed` (params file key of the same name);
    "torch_cpu" — drawn on the host from torch's global CPU generator in exactly the order the reference's CPU path
      consumes it (parity mode: seeded runs reproduce the reference's class indices; the host RNG is the bottleneck).
    `prec` selects the conv arithmetic: hip.PREC_F16X3 (default; fp16 hi/lo split x3 on the matrix cores, ~2^-22 per
    product, with the exact-fp32 kernel taking over any layer whose raw input leaves the split's range) or
    hip.PREC_F32 (exact fp32 MFMA everywhere, the validation mode).  hip.PREC_F16 is the OPT-IN single-pass fast mode (every conv on the
    general kernel with one fp16 MFMA per product; attention cores keep the split): narrower arithmetic than the reference's, outside the
    parity contract, never a default.
    The guidance keywords of a sampling call (guidance.GUIDANCE_KEYWORDS) are described, keyword by keyword, in guidance.py's docstring."""

    VIEW_FLIPS, KNOWN_FREE = VIEW_FLIPS, KNOWN_FREE           # (aliases: their home is guidance.py)

    def __init__(self, diffusion: DiffusionModel, unet: UNetModel, dataset_file: str, step_T_sample: str = "majority"):
        super().__init__()
        self.diffusion = diffusion
        self.unet = unet
        self.dataset_file = dataset_file
        self.step_T_sample = step_T_sample
        self.rng = "philox"
        self.philox_seed = 0
        self.philox_call = 0            # index of the next sampling call's noise stream (see the class docstring)
        self.philox_advance = True
        self.bound_call = 0             # index of the next label_bound call's key: a counter of its own, so a bound between two sampling calls changes neither
        self.sample_offset = 0          # global index of sample 0 when the batch is sharded over ranks
        self.noise_slice: Optional[Tuple[int, int]] = None   # (global_batch, first_sample) for torch_cpu sharding
        # each denoise step is replayed as one captured HIP graph (identical results to eager launches, tested)
        self.use_graph = True
        # the batch is sampled as this many contiguous sub-batches on concurrent HIP streams (bit-identical samples).  0 (default) =
        # automatic: two once the batch holds as many pixels as 32 samples of 128x128 (+7-10 % at N = 64: the low-resolution kernels of one half run beside the full-width
        # kernels of the other), one below.  bench.py times this default and collects its per-kernel taps in a separate
        # single-stream pass (under concurrency a launch's duration no longer describes the kernel).
        self.substreams = 0
        # Round 6: with substreams = 0 the choice between the bit-identical execution modes — one stream or two sub-batch streams, HIP-graph
        # replay or eager launches — is MEASURED once per (batch geometry, weights) on the box at hand (`_calibrate_mode`: a dozen denoise
        # steps of the call's own workload in each mode, results discarded), because the ranking moves with the box by a few per cent
        # (round 5: two graph streams 89.7 against 85.9 samples/s on one box, 89.4 against 91.9 on another).  The samples do not depend on it.
        # False = the static rule (auto_substreams) and `use_graph` as set.  `mode_choice` records what was measured and picked.
        self.calibrate_mode = True
        self.mode_choice: Dict[Any, dict] = {}
        self.last_mode: Optional[Tuple[int, bool]] = None           # (sub-batch streams, graph replay) of the most recent sampling call
        self.prec = hip.PREC_F16X3
        # what to do when a PREC_F16X3 run reports a range overflow (hip.CcdmRangeError):
        # "layers" (default) = repeat the call with the exact-fp32 kernels (same seeds, so its samples are the ones an all-fp32 run
        #   would have drawn), measure on that run what every conv stages (ccdm_engine_input_absmax) and pin the layers whose staged
        #   values come within RANGE_MARGIN of the fp16 split's limit to the exact-fp32 kernels from then on (`f32_layers`): later
        #   calls run the F16X3 engine with those few layers in fp32 instead of paying 4x for everything;
        # "f32" = only repeat the call in fp32 (round-2 behaviour); "raise" = propagate the error
        self.on_range_error = "layers"
        self.f32_layers: set = set()
        # what the range fallback changed by itself, and for which weights: automatic pins and an automatic switch to fp32 are undone
        # when the U-Net's parameters change (they describe THOSE weights); `range_events` counts them so a caller can see the mode change
        self._auto_pins: set = set()
        self._auto_f32_from: Optional[int] = None           # the precision an unattributable overflow switched away from
        self._auto_weights_key: Optional[Tuple[int, int]] = None
        self.range_events = {"overflows": 0, "layers_pinned": 0, "switched_to_f32": 0, "reset_on_new_weights": 0}
        self._range_probe: Optional[Dict[str, float]] = None        # filled while a diagnosing fp32 re-run is under way
        # workgroup slicing of the conv kernels: "throughput" (default) = the batch-size-independent rule — samples do not depend on how
        # a batch is sharded over ranks or sub-batches, bit for bit; "latency" = up to 32 one- or two-tile workgroups per sample
        # (ccdm_conv_args.fine_slices) for batches too small to fill the chip (LIDC batch 8: 2.05 -> 1.39 ms per denoise step; batch
        # 64 loses 5 %): GroupNorm's partial sums are then added in another order, so its samples may differ from the default mode's in
        # the last bit of a probability (never between two runs of the same mode and batch split)
        self.slicing = "throughput"
        self._engines: Dict[Any, Tuple[int, SamplerEngine]] = {}

    @property
    def time_steps(self) -> int:
        return self.diffusion.time_steps

    def _fine_slices(self, N: int) -> int:
        """ccdm_conv_args.fine_slices for a batch of N: 0 = the batch-size-independent rule; latency mode: 2 (up to 64 slices: one tile per
        workgroup at 128x128) for N <= 8, else 1 (up to 32)."""
        if self.slicing not in ("throughput", "latency"):
            raise ValueError(f"slicing: {self.slicing!r} (expected 'throughput' or 'latency')")
        return 0 if self.slicing != "latency" else (2 if N <= 8 else 1)

    # ------------------------------------------------------------------ reference API
    def forward(self, x: Tensor, condition: Tensor, feature_condition: Tensor = None, t: Optional[Tensor] = None,
                label_ref_logits: Optional[Tensor] = None, validation: bool = False, *,
                known_labels: Optional[Tensor] = None, resample: Optional[Tuple[int, int]] = None,
                evidence: Optional[Tensor] = None, temperature: Optional[float] = None,
                truncation: Optional[float] = None, views: Optional[Sequence[str]] = None,
                tiles: Optional[Sequence[int]] = None) -> Union[Tensor, dict]:
        guidance = dict(known_labels=known_labels, resample=resample, evidence=evidence, temperature=temperature, truncation=truncation,
                        views=views, tiles=tiles)
        if self.training or validation:
            G.refuse_outside_sampling(self, guidance)
        if self.training:
            if not isinstance(t, Tensor):
                raise ValueError("'t' needs to be a Tensor at training time")
            if not isinstance(x, Tensor):
                raise ValueError("'x' needs to be a Tensor at training time")
            return self.forward_step(x, condition, feature_condition, t)
        if validation:
            return self.forward_step(x, condition, feature_condition, t)
        return self.forward_denoising(x, condition, feature_condition, None if t is None else cast(int, t.item()), label_ref_logits, **guidance)

    # ------------------------------------------------------------------ engine plumbing
    def _weights_key(self) -> Tuple[int, int]:
        """Changes whenever the U-Net's parameters do: load_state_dict / .to() bump the explicit counter, in-place updates
        (optimizer steps, Polyak averaging, p.data.copy_) bump the tensors' own version counters."""
        return self.unet._weights_version, sum(int(p._version) for p in self.unet.parameters())

    def _engine(self, x: Tensor, condition: Tensor, feature_condition: Optional[Tensor], slot: Any = 0) -> SamplerEngine:
        """The step executor for this input geometry (cached).  `slot` tells apart the engines of concurrent sub-batches (an int) and
        the engine a sampling queue owns (a key of its own, so no plain call shares it)."""
        N, K, H, W = x.shape
        spec = self.unet.spec
        if feature_condition is not None and spec.feature_condition_unwired:
            # the reference concatenates at these blocks without having widened them and fails in the conv (unet.py:770-788)
            raise RuntimeError(f"feature_condition given, but input block(s) {spec.feature_condition_unwired} were not widened for it "
                               "(feature_cond_encoder target_layer / output_stride do not line up): channel mismatch")
        fshape = tuple(feature_condition.shape[1:]) if feature_condition is not None else None
        if not spec.feature_condition_idx:
            fshape = None                        # no injection point configured: the reference ignores the tensor too
        dev = next(self.unet.parameters()).device
        f32_layers = frozenset(self.f32_layers) if self.prec == hip.PREC_F16X3 else frozenset()
        key = (N, H, W, int(condition.shape[1]), fshape, str(dev), self.prec, slot, self._fine_slices(N), f32_layers)
        wkey = self._weights_key()
        hit = self._engines.get(key)
        if hit is not None and hit[0] == wkey:
            return hit[1]
        eng = SamplerEngine(spec, self.unet.state_dict(), N, H, W, K, int(condition.shape[1]), dev,
                            max_steps=self.time_steps, feature_shape=fshape, prec=self.prec, fine_slices=self._fine_slices(N),
                            f32_layers=f32_layers)
        self._engines = {k: v for k, v in self._engines.items() if v[0] == wkey}
        self._engines[key] = (wkey, eng)
        return eng

    def sampling_queue(self, capacity: int, image_shape: Sequence[int], guided: bool = False):
        """A continuous-batching queue on this model (serving.SamplingQueue): requests of any size and walk length share one engine of
        `capacity` rows, each reproducing its solo call bit for bit.  guided: its requests take evidence=, known_labels=, temperature=
        and truncation= as a solo call does."""
        from .serving import SamplingQueue
        return SamplingQueue(self, capacity, image_shape, guided=guided)

    def _philox_key(self, call: Optional[int] = None) -> int:
        """64-bit Philox key of the current sampling call: splitmix64 of (philox_seed, philox_call).  `call`: another counter in
        philox_call's place (label_bound's own, `bound_call`)."""
        call = int(self.philox_call if call is None else call)
        if call == 0:
            return int(self.philox_seed) & 0xFFFFFFFFFFFFFFFF        # call 0 uses the seed itself (the key the kernel tests pin)
        z = (int(self.philox_seed) + 0x9E3779B97F4A7C15 * call) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    @staticmethod
    def _to_index(x: Tensor, device) -> Tensor:
        return x.argmax(dim=1).to(device=device, dtype=torch.uint8).contiguous()

    # staged values within this factor of hip.F16X3_LIMIT pin a layer to fp32 (the probe sees the steps of one call, not every input)
    RANGE_MARGIN = 0.5

    def _probe_ranges(self, engines) -> None:
        """diagnosing fp32 re-run: fold what every conv / attention core of these (exact-fp32) engines staged in the step they just ran
        into the probe — enqueued on the engine's stream into a device buffer per engine (a running maximum over all steps of the call),
        read once at the end (`_collect_probe`)"""
        if self._range_probe is None:
            return
        for eng in engines:
            hit = self._range_probe.get(id(eng))
            if hit is None:
                hit = self._range_probe[id(eng)] = (eng, eng.probe_buffer())
            eng.probe_ranges(hit[1])

    def _collect_probe(self) -> Optional[Dict[str, float]]:
        if self._range_probe is None:
            return None
        out: Dict[str, float] = {}
        for eng, buf in self._range_probe.values():
            for name, v in eng.read_ranges(buf).items():
                out[name] = max(out.get(name, 0.0), v)
        return out

    def _with_range_fallback(self, fn):
        if self.on_range_error not in ("layers", "f32", "raise"):
            raise ValueError(f"on_range_error: {self.on_range_error!r} (expected 'layers', 'f32' or 'raise')")
        state = torch.get_rng_state() if self.rng == "torch_cpu" else None
        if self._auto_weights_key is not None and self._auto_weights_key != self._weights_key():
            # new weights: what the fallback learned about the old ones (pins, the switch to fp32) no longer applies
            self.f32_layers -= self._auto_pins
            if self._auto_f32_from is not None and self.prec == hip.PREC_F32:
                self.prec = self._auto_f32_from
            self._auto_pins, self._auto_f32_from, self._auto_weights_key = set(), None, None
            self.range_events["reset_on_new_weights"] += 1
        try:
            return fn()
        except hip.CcdmRangeError as e:
            if self.prec == hip.PREC_F32 or self.on_range_error == "raise":
                raise
            self.range_events["overflows"] += 1
            LOGGER.warning("%s -- repeating this call with the exact-fp32 kernels", e)
            if state is not None:
                torch.set_rng_state(state)
            prec, self.prec = self.prec, hip.PREC_F32
            self._range_probe = {} if self.on_range_error == "layers" else None
            probe = None
            try:
                out = fn()
                probe = self._collect_probe()
            finally:
                self.prec = prec
                self._range_probe = None
            if probe is not None:
                limit = hip.F16X3_LIMIT * self.RANGE_MARGIN
                hot = sorted(k for k, v in probe.items() if not (v < limit))
                new = [k for k in hot if k not in self.f32_layers]
                if new:
                    self.f32_layers.update(new)
                    self._auto_pins.update(new)
                    self._auto_weights_key = self._weights_key()
                    self.range_events["layers_pinned"] += len(new)
                    LOGGER.warning("F16X3 range: %d layer(s) stage values beyond %.0f (%s ...); they run the exact-fp32 kernels from now on "
                                   "(DenoisingModel.f32_layers)", len(new), limit, ", ".join(new[:4]))
                    # the engines built for the old pin set and the diagnosing all-fp32 ones are dead weight now — at Cityscapes-sized
                    # batches three activation sets per sub-batch slot is what runs a GPU out of memory exactly when the fallback triggers
                    self._engines.clear()
                else:
                    # an overflow the probe cannot attribute to a pinnable layer (every step of this call was looked at): without a
                    # new pin every later call would run F16X3, overflow and be repeated in fp32 — about 5x the cost, forever
                    LOGGER.warning("F16X3 range: the overflow could not be attributed to a layer (largest staged value %.3g); this model "
                                   "runs the exact-fp32 kernels until its weights change (DenoisingModel.prec = PREC_F32; range_events counts it)",
                                   max(probe.values()) if probe else float("nan"))
                    self._auto_f32_from, self._auto_weights_key = prec, self._weights_key()
                    self.range_events["switched_to_f32"] += 1
                    self.prec = hip.PREC_F32
                    self._engines = {k: v for k, v in self._engines.items() if k[6] == hip.PREC_F32}
            return out

    # ------------------------------------------------------------------ measured choice of the execution mode (substreams = 0)
    CALIBRATION_MIN_STEPS = 100         # shorter walks are not worth a calibration (~200 denoise steps of probing): the static rule decides
    CALIBRATION_STEPS = (4, 16)         # (untimed, timed) denoise steps per candidate mode and round
    CALIBRATION_ROUNDS = 3              # interleaved timing rounds; the minimum counts (C2: ~0.6 s once per geometry and set of weights)

    def _calibrate_mode(self, x: Tensor, condition: Tensor, feature_condition: Optional[Tensor], prepare, run_steps,
                        nsub_rule: int, graph_allowed: bool, n_rows: int) -> Tuple[int, bool]:
        """Time the bit-identical execution modes on this call's own workload and return the fastest (sub-batch streams, graph replay).
        Candidates: one stream or `nsub_rule` streams; graph replay (if `use_graph` allows it) or eager launches.  Each runs
        CALIBRATION_ROUNDS x CALIBRATION_STEPS denoise steps from x_T with the call's tables (the draws are discarded: every engine's inputs are set again
        by the caller, Philox counters depend on the step row only, the host generator is not touched — this path is never taken with
        rng = "torch_cpu").  Once per (geometry, precision, slicing, weights); `mode_choice` keeps the timings."""
        import time
        N, K, H, W = x.shape
        ck = (N, K, H, W, int(condition.shape[1]), None if feature_condition is None else tuple(feature_condition.shape[1:]), self.prec,
              self._fine_slices(N), graph_allowed, nsub_rule, self._weights_key())
        hit = self.mode_choice.get(ck)
        if hit is not None:
            return hit["nsub"], hit["use_graph"]
        warm, timed = (max(1, min(int(v), n_rows)) for v in self.CALIBRATION_STEPS)       # (rows of the call's own tables)
        cands = [(ns, g) for ns in (nsub_rule, 1) for g in ((True, False) if graph_allowed else (False,))]
        try:
            parts_of = {ns: prepare(ns) for ns in (nsub_rule, 1)}       # (both engine sets exist from here on: twice the activation memory)
        except torch.cuda.OutOfMemoryError:
            LOGGER.warning("execution-mode measurement skipped for N=%d %dx%d: no memory for both engine sets; static rule (%d streams)", N, H, W, nsub_rule)
            self._engines = {}
            torch.cuda.empty_cache()
            self.mode_choice[ck] = {"nsub": nsub_rule, "use_graph": graph_allowed, "ms_per_denoise_step": {}}
            return nsub_rule, graph_allowed
        dev = parts_of[1][0][0].device
        for ns, g in cands:                                                   # untimed: captures each engine's graph, warms weights and code
            run_steps(parts_of[ns], 0, warm, [None] * ns, 0, g)
        torch.cuda.synchronize(dev)
        times = {c: float("inf") for c in cands}
        for _ in range(self.CALIBRATION_ROUNDS):                              # interleaved rounds, minimum per candidate: the modes differ by 1-4 %
            for ns, g in cands:
                t0 = time.perf_counter()
                run_steps(parts_of[ns], 0, timed, [None] * ns, 0, g)
                torch.cuda.synchronize(dev)
                times[(ns, g)] = min(times[(ns, g)], (time.perf_counter() - t0) / timed * 1e3)
        for parts_ in parts_of.values():
            for eng, lo, hi in parts_:
                eng.check_and_clear_flag()                                   # (the real call reports overflows; a probe run must not leave a flag behind)
        best = min(times, key=times.get)
        self.mode_choice = {k_: v for k_, v in self.mode_choice.items() if k_[-1] == ck[-1]}      # (entries of older weights go)
        self.mode_choice[ck] = {"nsub": best[0], "use_graph": best[1],
                                "ms_per_denoise_step": {f"{ns} stream{'s' if ns > 1 else ''}, {'graph' if g else 'eager'}": round(v, 4) for (ns, g), v in times.items()}}
        LOGGER.info("execution mode for N=%d %dx%d: %d stream(s), %s (ms per denoise step: %s)", N, H, W, best[0], "graph" if best[1] else "eager",
                    self.mode_choice[ck]["ms_per_denoise_step"])
        return best

    def forward_step(self, x: Tensor, condition: Tensor, feature_condition: Tensor, t: Tensor) -> dict:
        return self._with_range_fallback(lambda: self._forward_step(x, condition, feature_condition, t))

    def forward_denoising(self, x: Optional[Tensor], condition: Tensor, feature_condition: Tensor,
                          init_t: Optional[int] = None, label_ref_logits: Optional[Tensor] = None, *,
                          consume: Optional[Callable[[SamplerEngine, int, int], None]] = None,
                          known_labels: Optional[Tensor] = None, resample: Optional[Tuple[int, int]] = None,
                          evidence: Optional[Tensor] = None, temperature: Optional[float] = None,
                          truncation: Optional[float] = None, views: Optional[Sequence[str]] = None,
                          tiles: Optional[Sequence[int]] = None) -> dict:
        """`consume` (predict_multiple): instead of returning the call's output, hand every sub-batch engine (eng, lo, hi) to
        consume(eng, lo, hi) once the call has succeeded, with the engine's stream current; the result is then {}.  With `tiles` the
        first argument is the sub-batch's canvas holder (engine.TileCanvas: the xt / out_probs / out_onehot of the canvas) instead.
        `known_labels`: integer [N,H,W], a class where the label is known, 255 where the pixel is free (see guidance.py's docstring).
        `resample`: (jump_length, resamples), RePaint's resampling jumps of a walk with known labels (guidance.py's docstring).
        `evidence`: float [N,K,H,W], per-pixel class weights in [0,1] (guidance.py's docstring).
        `temperature` in [0.05, 20], `truncation` in (0, 1]: temper and truncate x0 before every reverse step (guidance.py's docstring).
        `views`: names from "hflip", "vflip", "hvflip": x0 is averaged over these mirror images of the input (guidance.py's docstring).
        `tiles`: (h, w, sy, sx): x and condition are a canvas larger than the network's geometry, sampled as ONE chain whose x0 is the
          per-pixel mean over overlapping h x w tiles at strides (sy, sx) (guidance.py's docstring)."""
        guidance = dict(known_labels=known_labels, resample=resample, evidence=evidence, temperature=temperature, truncation=truncation,
                        views=views, tiles=tiles)
        guide = G.check_guidance(self, guidance, None if x is None else tuple(x.shape), feature_condition)
        return self._sample(x, condition, feature_condition, init_t, label_ref_logits, consume, guide)

    def _sample(self, x: Optional[Tensor], condition: Tensor, feature_condition: Tensor, init_t: Optional[int],
                label_ref_logits: Optional[Tensor], consume, guide: Guidance) -> dict:
        """One sampling call; `guide`: what guidance.check_guidance returned."""
        out = self._with_range_fallback(lambda: self._forward_denoising(x, condition, feature_condition, init_t, label_ref_logits,
                                                                        consume, guide))
        if self.philox_advance:
            self.philox_call += 1           # the next call draws from a fresh stream (a range-error re-run above replayed this one)
        return out

    # ------------------------------------------------------------------ multi-sample prediction
    MULTI_MAPS = ("mean", "vote", "entropy", "mutual_info", "counts")

    @torch.no_grad()
    def predict_multiple(self, condition: Tensor, feature_condition: Optional[Tensor] = None, *, num_evaluations: int,
                         voting: Optional[str] = None, x: Optional[Tensor] = None, t: Optional[Tensor] = None, batched: bool = False,
                         maps: Sequence[str] = ("mean", "vote", "entropy", "mutual_info"),
                         known_labels: Optional[Tensor] = None, resample: Optional[Tuple[int, int]] = None,
                         evidence: Optional[Tensor] = None, temperature: Optional[float] = None,
                         truncation: Optional[float] = None, views: Optional[Sequence[str]] = None,
                         tiles: Optional[Sequence[int]] = None) -> Dict[str, Tensor]:
        """S = `num_evaluations` samples of every image of `condition` [B,C,H,W], combined on the device into one prediction and
        per-pixel uncertainty maps — the reference's Evaluator.predict_multiple (evaluation/eval_cdm.py:176-193), which sums S
        `predict_single` outputs as `total += prediction_i * (1 / S)`.

        voting (default `step_T_sample`, the params key `evaluation_vote_strategy`):
          "confidence": every pass ends in the posterior probabilities; `mean` is the reference's `prediction_onehot_total` bit for bit
                        (fp32 multiply by fp32(1/S), then fp32 add, pass by pass); `vote` its argmax;
          "majority":   every pass ends in the argmax class (the reference raises NotImplementedError here); `mean` holds the class
                        frequencies counts / S, `vote` the majority class (ties to the lowest class index), `counts` the int32 counts.
        `entropy` is H(mean) in nats; `mutual_info` is H(mean) - (1/S) sum_s H(p_s) (the spread between the samples; with one-hot
        majority passes every H(p_s) is 0, so it equals `entropy`).
        x: optional one-hot x_T [S,B,K,H,W]; default: drawn per pass as predict_single does (uniform one-hot on condition's device).
        t: as in forward (e.g. 10000 + steps for a strided walk).
        known_labels: integer [B,H,W] (a class where the label is known, 255 where the pixel is free): every pass is conditioned on it
          (guidance.py), so `vote` equals the label and `entropy` is 0 at the known pixels.
        resample: (jump_length, resamples): every pass walks with RePaint's resampling jumps (guidance.py); needs known_labels.
        evidence: float [B,K,H,W] per-pixel class weights in [0,1] (guidance.py): every pass is sampled under it.
        temperature, truncation: every pass tempers and truncates x0 before every reverse step (guidance.py), all with the same pair.
        views: every pass averages x0 over these mirror images of the input (guidance.py); a model that takes a feature_condition
          then needs [V,B,Cf,h,w].
        tiles: (h, w, sy, sx): `condition` is a canvas larger than the network's geometry and every pass samples it tiled
          (guidance.py); a model that takes a feature_condition then needs [R,B,Cf,hf,wf].  The passes are folded from the canvas.
        batched=False: S sampling calls of B samples, each advancing `philox_call` exactly like S calls of model(x_i, condition);
          after each call the pass is folded into device accumulators straight from the engine (ccdm_vote_accumulate), so memory
          is one pass plus the accumulators.  The range-error fallback and the execution-mode choice apply per pass.
        batched=True: one call of B*S samples (condition repeat-interleaved, sample b*S + s = pass s of image b, as
          eval_lidc_uncertainty lays them out), reduced by ccdm_vote_reduce_stack (majority) or S strided accumulations
          (confidence).  Faster for small B; its noise differs from the sequential mode's because the Philox stream is keyed by
          call and global sample index — a different, equally valid draw.
        Returns the requested `maps` on the model's device: mean / counts [B,K,H,W] (fp32 / int32, BCHW views of channels-last
        memory like the sampler's output), vote [B,H,W] int64, entropy / mutual_info [B,H,W] fp32."""
        voting = self.step_T_sample if voting is None else voting
        if voting not in ("confidence", "majority"):
            raise ValueError(f"voting: {voting!r} (expected 'confidence' or 'majority')")
        S = _num_evaluations(num_evaluations)
        maps = tuple(maps)
        bad = [m for m in maps if m not in self.MULTI_MAPS or (m == "counts" and voting != "majority")]
        if bad:
            raise ValueError(f"maps: {bad} not available (choose from {self.MULTI_MAPS}; 'counts' with voting='majority')")
        guidance = dict(known_labels=known_labels, resample=resample, evidence=evidence, temperature=temperature, truncation=truncation,
                        views=views, tiles=tiles)
        init_t, guide, batch = self._samples_per_image(condition, feature_condition, S, x, t, guidance, interleaved=batched)
        B, H, W = int(condition.shape[0]), int(condition.shape[2]), int(condition.shape[3])
        K, HW = self.diffusion.num_classes, H * W
        dev = next(self.unet.parameters()).device
        lib = hip.load()
        majority = voting == "majority"
        want_mi = "mutual_info" in maps
        w = float(np.float32(1.0 / S))          # the reference's (1 / S) as the fp32 scalar torch multiplies an fp32 tensor by

        def stream() -> int:
            return torch.cuda.current_stream(dev).cuda_stream

        total = None if majority else torch.zeros((B, H, W, K), dtype=torch.float32, device=dev)
        counts = torch.zeros((B, H, W, K), dtype=torch.int32, device=dev) if majority else None
        ent_sum = torch.zeros((B, H, W), dtype=torch.float32, device=dev) if (want_mi and not majority) else None

        def ptr(a: Optional[Tensor], off: int = 0):
            return None if a is None else a.data_ptr() + off * a.element_size()

        saved = self.step_T_sample
        self.step_T_sample = voting
        try:
            if not batched:
                def consume(eng, lo: int, hi: int) -> None:
                    src_cls, src_probs = (eng.xt, None) if majority else (None, eng.out_probs)
                    hip.check(lib.ccdm_vote_accumulate(ptr(src_cls), ptr(src_probs), 0, hi - lo, HW, K, w, ptr(total, lo * HW * K),
                                                       ptr(counts, lo * HW * K), ptr(ent_sum, lo * HW), stream()), "vote_accumulate")

                for i in range(S):
                    self._sample(x[i] if x is not None else self._draw_x_T(B, H, W, condition.device), condition, feature_condition, init_t, None,
                                 consume, guide)
            else:
                xr, cond, fc = batch
                # the pass outputs of all B*S samples: class maps (1 byte a pixel) or probabilities
                buf = torch.empty((B * S, HW) if majority else (B * S, HW, K), dtype=torch.uint8 if majority else torch.float32, device=dev)

                def consume(eng, lo: int, hi: int) -> None:
                    # (the first hi - lo rows: with views the engine holds V times as many, view 0 first)
                    buf[lo:hi].copy_(eng.xt.reshape(-1, HW)[:hi - lo] if majority else eng.out_probs.reshape(-1, HW, K)[:hi - lo])

                self._sample(xr, cond, fc, init_t, None, consume, guide)
                if majority:
                    vote8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
                    mean = torch.empty((B, H, W, K), dtype=torch.float32, device=dev) if "mean" in maps else None
                    ent = torch.empty((B, H, W), dtype=torch.float32, device=dev) if ("entropy" in maps or want_mi) else None
                    hip.check(lib.ccdm_vote_reduce_stack(buf.data_ptr(), B, S, HW, K, ptr(counts), ptr(mean), vote8.data_ptr(),
                                                         ptr(ent), stream()), "vote_reduce_stack")
                    # one-hot passes: every H(p_s) is 0, the mutual information is the entropy of the mean
                    return self._multi_maps(maps, mean=mean, counts=counts, vote8=vote8, entropy=ent,
                                            mutual_info=ent.clone() if (want_mi and "entropy" in maps) else ent)
                for s in range(S):          # pass s of image b is sample b*S + s: image stride S*HW*K
                    hip.check(lib.ccdm_vote_accumulate(None, ptr(buf, s * HW * K), S * HW * K, B, HW, K, w, ptr(total), None,
                                                       ptr(ent_sum), stream()), "vote_accumulate")
                del buf
        finally:
            self.step_T_sample = saved
        vote8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        ent = torch.empty((B, H, W), dtype=torch.float32, device=dev) if "entropy" in maps else None
        mi = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_mi else None
        mean = torch.empty((B, H, W, K), dtype=torch.float32, device=dev) if (majority and "mean" in maps) else total
        hip.check(lib.ccdm_vote_finalize(ptr(total), ptr(counts), ptr(ent_sum), B, HW, K, S, ptr(mean) if majority else None,
                                         vote8.data_ptr(), ptr(ent), ptr(mi), stream()), "vote_finalize")
        return self._multi_maps(maps, mean=mean, counts=counts, vote8=vote8, entropy=ent, mutual_info=mi)

    @staticmethod
    def _multi_maps(maps: Sequence[str], **got: Optional[Tensor]) -> Dict[str, Tensor]:
        out: Dict[str, Tensor] = {}
        for m in maps:
            if m in ("mean", "counts"):
                out[m] = cast(Tensor, got[m]).permute(0, 3, 1, 2)
            elif m == "vote":
                out[m] = cast(Tensor, got["vote8"]).long()
            else:
                out[m] = cast(Tensor, got[m])
        return out

    def _draw_x_T(self, n: int, H: int, W: int, device) -> Tensor:
        """predict_single's x_T (eval_cdm.py:160-165): uniform one-hot [n,K,H,W]."""
        return OneHotCategoricalBCHW(logits=torch.zeros((n, self.diffusion.num_classes, H, W), device=device)).sample()

    def _samples_per_image(self, condition: Tensor, feature_condition: Optional[Tensor], S: int, x: Optional[Tensor], t: Optional[Tensor],
                           guidance: Mapping, interleaved: bool = True):
        """What a call of S samples per image of `condition` [B,C,H,W] checks and lays out: (init_t, guide, batch) — `guide` the checked
        guidance (guidance.check_guidance) of the B images.  interleaved: `batch` = (xr, cond, fc), the ONE batch of B*S samples (x_T
        [S,B,K,H,W] or a fresh draw, condition and features repeat-interleaved: sample b*S + s = sample s of image b) and `guide` repeated
        like it; else `batch` is None."""
        K = self.diffusion.num_classes
        if condition.ndim != 4:
            raise ValueError(f"condition: expected [B,C,H,W], got {tuple(condition.shape)}")
        B, H, W = int(condition.shape[0]), int(condition.shape[2]), int(condition.shape[3])
        if x is not None and tuple(x.shape) != (S, B, K, H, W):
            raise ValueError(f"x: expected one-hot x_T of shape {(S, B, K, H, W)} = [S,B,K,H,W], got {tuple(x.shape)}")
        init_t = None if t is None else int(t.item() if isinstance(t, Tensor) else t)
        guide = G.check_guidance(self, guidance, (B, K, H, W), feature_condition)
        if not interleaved:
            return init_t, guide, None
        xr = x.transpose(0, 1).reshape(B * S, K, H, W) if x is not None else self._draw_x_T(B * S, H, W, condition.device)
        cond = condition.repeat_interleave(S, dim=0)
        # (with views or tiles on a model that takes features: [V,B,...] / [R,B,...], the samples on dim 1)
        fc = None if feature_condition is None else \
            feature_condition.repeat_interleave(S, dim=G.sample_axis(feature_condition, guide.views, guide.tiles))
        return init_t, guide.repeat_interleave(S), (xr, cond, fc)

    def _sample_class_maps(self, condition: Tensor, feature_condition: Optional[Tensor], S: int, x: Optional[Tensor], t: Optional[Tensor],
                           guidance: Mapping) -> Tensor:
        """One sampling call of B*S samples (condition repeat-interleaved, sample b*S + s = sample s of image b), every pass ending in its
        argmax class ("majority"), the class maps read straight from the engine -> uint8 [B,S,H,W] on the model's device.  What
        predict_modes and predict_findings sample; `philox_call` advances as for one call.  guidance: the call's keywords by name."""
        init_t, guide, (xr, cond, fc) = self._samples_per_image(condition, feature_condition, S, x, t, guidance)
        B, H, W = int(condition.shape[0]), int(condition.shape[2]), int(condition.shape[3])
        HW = H * W
        dev = next(self.unet.parameters()).device
        stack = torch.empty((B * S, HW), dtype=torch.uint8, device=dev)

        def consume(eng, lo: int, hi: int) -> None:
            # (the first hi - lo rows: with views the engine holds V times as many, view 0 first)
            stack[lo:hi].copy_(eng.xt.reshape(-1, HW)[:hi - lo])

        saved = self.step_T_sample
        self.step_T_sample = "majority"
        try:
            self._sample(xr, cond, fc, init_t, None, consume, guide)
        finally:
            self.step_T_sample = saved
        return stack.reshape(B, S, H, W)

    @torch.no_grad()
    def predict_modes(self, condition: Tensor, feature_condition: Optional[Tensor] = None, *, num_evaluations: int, modes: int,
                      x: Optional[Tensor] = None, t: Optional[Tensor] = None, max_swaps: int = 64,
                      maps: Sequence[str] = ("vote", "entropy"), **guidance) -> Dict[str, Tensor]:
        """S = `num_evaluations` samples of every image of `condition` [B,C,H,W], summarised on the device as M = `modes` distinct
        segmentations with the share of the samples behind each: "three hypotheses: no nodule 55 %, small nodule 30 %, large nodule
        15 %", where predict_multiple folds the samples per pixel and loses which segmentations they were.

        One sampling call of B*S samples laid out as predict_multiple(batched=True) lays them out (condition repeat-interleaved,
        sample b*S + s = sample s of image b), every pass ending in its argmax class ("majority"); the class maps are read straight
        from the engine into a uint8 stack and clustered by metrics.sample_modes: k-medoids (PAM) under the distance of the LIDC
        scores, 1 - mean foreground IoU, in exact integers (include/ccdm_hip.h has the definition).  `philox_call` advances as for
        one call.  2 <= K <= 32, 1 <= S <= 256, 1 <= modes <= 16.
        x: optional one-hot x_T [S,B,K,H,W]; default: drawn as predict_multiple draws it.  t: as in forward.
        max_swaps: the most swaps PAM applies after its greedy BUILD (`converged` tells whether it stopped by itself).
        maps: per-mode maps from "vote", "entropy", "counts" (metrics.MODE_MAPS).
        **guidance: the keywords of guidance.GUIDANCE_KEYWORDS, as in predict_multiple, for every sample.
        Returns, on the model's device, what metrics.sample_modes returns — medoid [B,M] (the sample that stands for the mode, -1:
        unused), assign [B,S], size, share (= size / S), spread, cost, swaps, converged, mode_map [B,M,H,W] uint8 (the medoid sample,
        255 where unused), mode_vote / mode_entropy / mode_counts as asked for — and `samples` [B,S,H,W] uint8, the class maps."""
        from . import metrics as MT
        G.known_keywords("DenoisingModel.predict_modes", guidance)
        S = _num_evaluations(num_evaluations, MT.MODES_MAX_SAMPLES)
        K = self.diffusion.num_classes
        MT.whole_number(K, "num_classes", 2, MT.MODES_MAX_CLASSES, f"predict_modes: expected a model of 2 to {MT.MODES_MAX_CLASSES} classes")
        MT.whole_number(modes, "modes", 1, MT.MODES_MAX_MODES, f"expected a whole number in [1, {MT.MODES_MAX_MODES}]")
        MT.whole_number(max_swaps, "max_swaps", 0, 2 ** 31 - 1, "expected a whole number, at least 0")
        maps = tuple(maps)
        bad = [m for m in maps if m not in MT.MODE_MAPS]
        if bad:
            raise ValueError(f"maps: {bad} not available (choose from {MT.MODE_MAPS})")
        samples = self._sample_class_maps(condition, feature_condition, S, x, t, guidance)
        out = MT.sample_modes(samples, K, modes, max_swaps=max_swaps, maps=maps)
        out["samples"] = samples
        return out

    @torch.no_grad()
    def predict_consensus(self, condition: Tensor, feature_condition: Optional[Tensor] = None, *, num_evaluations: int, metric: str = "iou",
                          x: Optional[Tensor] = None, t: Optional[Tensor] = None, maps: Sequence[str] = ("label",),
                          **guidance) -> Dict[str, Tensor]:
        """S = `num_evaluations` samples of every image of `condition` [B,C,H,W], answered with the ONE map to report: per class the
        thresholded sample frequency with the largest expected `metric` ("iou" or "dice") under the samples themselves.  The majority
        vote of predict_multiple is the best map for per-pixel accuracy; under IoU and Dice the best threshold is in general not 1/2,
        and with many empty samples it is the empty map.

        One sampling call of B*S samples laid out as predict_modes lays them out, every pass ending in its argmax class ("majority");
        the class maps are read straight from the engine into a uint8 stack and handed to metrics.sample_consensus (include/ccdm_hip.h
        has the definition).  `philox_call` advances as for one call.  2 <= K <= 32, 1 <= S <= 255.
        x: optional one-hot x_T [S,B,K,H,W]; default: drawn as predict_multiple draws it.  t: as in forward.
        maps: from "label", "mask" (metrics.CONSENSUS_MAPS).
        **guidance: the keywords of guidance.GUIDANCE_KEYWORDS, as in predict_multiple, for every sample.
        Returns, on the model's device, what metrics.sample_consensus returns — threshold [B,K-1], thresholds, curve, expected,
        expected_majority, frequency, label [B,H,W] / mask [B,K-1,H,W] as asked for — and `samples` [B,S,H,W] uint8, the class maps."""
        from . import metrics as MT
        G.known_keywords("DenoisingModel.predict_consensus", guidance)
        S = _num_evaluations(num_evaluations, MT.CONSENSUS_MAX_SAMPLES)
        K = self.diffusion.num_classes
        MT.whole_number(K, "num_classes", 2, MT.MODES_MAX_CLASSES, f"predict_consensus: expected a model of 2 to {MT.MODES_MAX_CLASSES} classes")
        if metric not in MT.CONSENSUS_METRICS:
            raise ValueError(f"metric: {metric!r} (choose from {MT.CONSENSUS_METRICS})")
        maps = tuple(maps)
        bad = [m for m in maps if m not in MT.CONSENSUS_MAPS]
        if bad:
            raise ValueError(f"maps: {bad} not available (choose from {MT.CONSENSUS_MAPS})")
        samples = self._sample_class_maps(condition, feature_condition, S, x, t, guidance)
        out = MT.sample_consensus(samples, K, metric=metric, maps=maps)
        out["samples"] = samples
        return out

    @torch.no_grad()
    def predict_findings(self, condition: Tensor, feature_condition: Optional[Tensor] = None, *, num_evaluations: int,
                         min_frequency: float = 0.1, connectivity: int = 8, max_candidates: int = 64,
                         x: Optional[Tensor] = None, t: Optional[Tensor] = None, **guidance) -> Dict[str, Any]:
        """S = `num_evaluations` samples of every image of `condition` [B,C,H,W], read as ONE list of lesions per image and class with
        a confidence each: a structure that 90 of 100 samples draw is a finding, one that 12 draw a hypothesis, where predict_multiple
        folds the samples per pixel and loses which structure a pixel belongs to.

        One sampling call of B*S samples laid out as predict_modes lays them out, every pass ending in its argmax class ("majority");
        the class maps are read straight from the engine into a uint8 stack and handed to metrics.sample_findings without raters:
        the candidates are the connected components (under `connectivity`) of the pixels that at least n_min = max(1,
        ceil(min_frequency * S)) samples give the class, `min_frequency` read as the decimal it is written as (include/ccdm_hip.h has
        the definition).  `philox_call` advances as for one call.  1 <= K <= 32, 1 <= S <= 255, H*W <= 16384.
        x: optional one-hot x_T [S,B,K,H,W]; default: drawn as predict_multiple draws it.  t: as in forward.
        max_candidates: the records kept per image and class (at most 1024); an image with more raises, naming the value needed.
        **guidance: the keywords of guidance.GUIDANCE_KEYWORDS, as in predict_multiple, for every sample.
        Returns `counts` int64 [B,C,2] and `candidates` int64 [B,C,max_candidates,12] on the host (metrics.FINDING_CANDIDATE_FIELDS:
        size, support, peak, mass, ..., the box, the coordinate sums), `confidence_map` uint8 [B,C,H,W] (the support of the candidate
        that holds the pixel, 0 outside) and `samples` uint8 [B,S,H,W] on the model's device, and `n_min`, `classes`."""
        from . import metrics as MT
        G.known_keywords("DenoisingModel.predict_findings", guidance)
        S = _num_evaluations(num_evaluations, 255)
        K = self.diffusion.num_classes
        if isinstance(min_frequency, bool) or not isinstance(min_frequency, (int, float)) or not 0 <= min_frequency <= 1:
            raise ValueError(f"min_frequency: {min_frequency!r} (expected a share of the samples in [0, 1])")
        n_min = max(1, MT._ceil_fraction(min_frequency, S))
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity: {connectivity!r} (expected 4 or 8)")
        MT.whole_number(max_candidates, "max_candidates", 1, MT.FINDINGS_MAX_CANDIDATES,
                        f"expected a whole number in [1, {MT.FINDINGS_MAX_CANDIDATES}]")
        MT.whole_number(K, "num_classes", 1, 32, "predict_findings: expected a model of 1 to 32 classes")
        if condition.ndim == 4 and int(condition.shape[2]) * int(condition.shape[3]) > 16384:
            raise ValueError(f"condition: {tuple(condition.shape)} (predict_findings: maps of at most 16384 pixels)")
        samples = self._sample_class_maps(condition, feature_condition, S, x, t, guidance)
        got = MT.sample_findings(samples, None, K, n_min=n_min, connectivity=connectivity, max_candidates=max_candidates, return_map=True)
        return {"counts": got["counts"], "candidates": got["candidates"], "confidence_map": got["confidence_map"], "samples": samples,
                "n_min": n_min, "classes": got["classes"]}

    # ------------------------------------------------------------------ likelihood bound of held-out labels
    BOUND_LOG_FLOOR = 1e-12             # the trainer's clamp under the logarithm (trainer.py:267)

    @torch.no_grad()
    def label_bound(self, labels: Tensor, condition: Tensor, feature_condition: Optional[Tensor] = None, *, timesteps=None,
                    draws: int = 1, class_weights: Optional[Tensor] = None, rows: int = 64, return_map: bool = False) -> Dict[str, Any]:
        """How probable the model finds label maps somebody drew: the variational bound, in nats,
            -log p(y | image) <= L_T + sum_t E_{x_t ~ q(x_t | x_0 = y)} l_t(y, x_t)
        whose per-timestep term is the reference's training loss (include/ccdm_hip.h has the definition).  No walk: every network kernel
        reads its time-embedding row per engine row, so one pass of `rows` rows holds (label, timestep, draw) triples at different noise
        levels — all 250 levels of one LIDC label are four 64-row passes.  Per pass: ccdm_bound_noise draws x_t, the network runs to x0
        (STEP_SOFTMAX_ONLY), ccdm_bound_terms sums the per-pixel terms per row; one stream, one host synchronisation at the end.
        labels: integer [B,H,W] or [B,L,H,W] (L maps per image, e.g. the raters), a class < K or 255 = pixel not counted; or one-hot float
        [B,(L,)K,H,W], taken by argmax.  timesteps: None = every t in 1..T; a sequence = those t (a partial sum); an int M = M strata
        with one t drawn per label and stratum, weighted by the stratum's size (unbiased; bound_timesteps).  draws: independent x_t per
        (label, t), averaged.  class_weights: fp32 [K], the trainer's per-class mask (0 drops a class: Cityscapes' ignore).
        Returns float64 tensors: "bound" [B,L], "bits_per_pixel" [B,L] = bound / (sum of the pixel weights * ln 2), "terms" [B,L,M] (mean
        over draws, not weighted by the stratum), "timesteps" [B,L,M] (int64), "prior" [B,L], "pixels" [B,L] (int64: the counted pixels),
        "complete" (bool: the estimator covers 1..T); with return_map "surprise" [B,L,H,W] fp32, the estimator-weighted sum of the
        per-pixel terms (accumulated in 2^-32 fixed point: the same bits however the rows are packed).
        The draws are keyed by (pixel, label, draw, t) under a key of the call's own counter `bound_call` (it advances with
        `philox_advance`; `philox_call` is not touched) on a Philox counter range no sampling draw uses: a bound between two sampling calls
        changes neither, and the result does not depend on `rows` (default slicing).  The floor 1e-12 under the logarithm is the
        trainer's: where the model gives a class the posterior needs less than that, the term is capped — a bound up to those pixels.
        Under WORLD_SIZE > 1 every rank computes the same numbers (no sharding).  Refused: rng = "torch_cpu", `softmax_output: no`, labels
        whose geometry is not the call's, draws < 1, rows < 1, timesteps outside 1..T or repeated."""
        if self.rng not in ("philox", "torch_cpu"):
            raise ValueError(f"rng: {self.rng!r}")
        G.require(self, "label_bound", sampling=None)         # (not rng = "torch_cpu", a model whose x0 holds probabilities)
        K, T = int(self.diffusion.num_classes), int(self.time_steps)
        if isinstance(draws, bool) or int(draws) != draws or int(draws) < 1:
            raise ValueError(f"draws: expected an integer >= 1, got {draws!r}")
        if isinstance(rows, bool) or int(rows) != rows or int(rows) < 1:
            raise ValueError(f"rows: expected an integer >= 1, got {rows!r}")
        draws, rows = int(draws), int(rows)
        if not isinstance(condition, Tensor) or condition.dim() != 4:
            raise ValueError("condition: expected the images [B,C,H,W]")
        B, _, H, W = (int(v) for v in condition.shape)
        if not isinstance(labels, Tensor) or labels.dtype == torch.bool or labels.dtype.is_complex:
            raise ValueError(f"labels: expected an integer or one-hot float tensor, got {getattr(labels, 'dtype', type(labels).__name__)}")
        if labels.dtype.is_floating_point:
            if labels.dim() not in (4, 5) or int(labels.shape[-3]) != K:
                raise ValueError(f"labels: one-hot labels must be [B,K,H,W] or [B,L,K,H,W] with K = {K}, got {tuple(labels.shape)}")
            idx = labels.detach().argmax(dim=-3)
        else:
            idx = labels.detach()
            host = idx.cpu()
            if bool(((host < 0) | (host > 255)).any()):
                raise ValueError("labels: values must be classes in [0,K) or 255 (not counted)")
        if idx.dim() == 3:
            idx = idx[:, None]
        if idx.dim() != 4 or (int(idx.shape[0]), int(idx.shape[2]), int(idx.shape[3])) != (B, H, W) or int(idx.shape[1]) < 1:
            raise ValueError(f"labels: geometry {tuple(labels.shape)} does not match the call's: expected [{B},(L,){H},{W}] "
                             f"(or one-hot [{B},(L,){K},{H},{W}])")
        L = int(idx.shape[1])
        dev = next(self.unet.parameters()).device
        w_dev = None
        if class_weights is not None:
            w_dev = torch.as_tensor(class_weights, dtype=torch.float32).reshape(-1).to(dev).contiguous()
            if w_dev.numel() != K or not bool(torch.isfinite(w_dev).all()) or bool((w_dev < 0).any()):
                raise ValueError(f"class_weights: expected {K} finite weights >= 0")
        key = self._philox_key(self.bound_call)
        t_np, wt_np = bound_timesteps(T, timesteps, key, B * L)
        complete = timesteps is None or (isinstance(timesteps, (int, np.integer)) and not isinstance(timesteps, bool)) or \
            set(int(v) for v in t_np[0]) == set(range(1, T + 1))
        labels_dev = idx.to(device=dev, dtype=torch.uint8).reshape(B * L, H * W).contiguous()
        out = self._with_range_fallback(lambda: self._label_bound(labels_dev, condition, feature_condition, t_np, wt_np, draws, rows, w_dev,
                                                                  return_map, key, (B, L, H, W)))
        out["complete"] = bool(complete)
        if self.philox_advance:
            self.bound_call += 1
        return out

    def _label_bound(self, labels_dev: Tensor, condition: Tensor, feature_condition: Optional[Tensor], t_np: np.ndarray, wt_np: np.ndarray,
                     draws: int, rows: int, w_dev: Optional[Tensor], return_map: bool, key: int, shape: Tuple[int, int, int, int]) -> Dict[str, Any]:
        B, L, H, W = shape
        K, T, R, M, HW = int(self.diffusion.num_classes), int(self.time_steps), B * L, int(t_np.shape[1]), H * W
        dev = labels_dev.device
        cum = [float(v) for v in self.diffusion.cumalphas.double().cpu()]
        passes = bound_rows(t_np, draws, rows, K, cum, self.diffusion.posterior_coeffs, R)
        P = len(passes)
        tables = np.stack([tab for tab, _ in passes])                                    # [P, rows] records
        slots = np.stack([slot for _, slot in passes])                                   # [P, rows], -1 = idle
        busy = slots >= 0
        label_of = np.where(busy, slots // (M * draws), 0)
        m_of = np.where(busy, (slots // draws) % M, 0)
        # everything the passes read, uploaded once: no host-to-device copy, no synchronisation inside the loop
        tables_dev = torch.from_numpy(tables.view(np.int32).reshape(P, rows, 8)).to(dev)
        rowmap_dev = torch.from_numpy(np.where(busy, tables["t"] - 1, 0).astype(np.int32)).to(dev)
        image_of = torch.from_numpy(label_of // L).to(dev)
        slot_dev = torch.from_numpy(np.where(busy, slots, R * M * draws)).to(dev)        # idle rows add their zeros to a slot of their own
        eng = self._engine(torch.empty((rows, K, H, W), device="meta"), condition, feature_condition)
        acc = torch.zeros((R * M * draws + 1,), dtype=torch.float64, device=dev)
        row_sum = torch.zeros((rows,), dtype=torch.float64, device=dev)
        row_weight = torch.zeros((rows,), dtype=torch.float64, device=dev)
        pix_map = surprise_fx = scale_dev = label_dev = None
        if return_map:
            pix_map = torch.zeros((rows, HW), dtype=torch.float32, device=dev)
            surprise_fx = torch.zeros((R + 1, HW), dtype=torch.int64, device=dev)
            scale = np.where(busy, wt_np[label_of, m_of] / draws, 0.0) * 2.0 ** 32
            scale_dev = torch.from_numpy(scale).to(dev)
            label_dev = torch.from_numpy(np.where(busy, label_of, R)).to(dev)
        with eng.enter():
            cond = condition.to(dev, torch.float32)
            feat = None if feature_condition is None else feature_condition.to(dev, torch.float32)
            # all T levels, row t - 1 holds timestep t; every row's network pass stops at x0
            eng.set_tables([float(t) for t in range(1, T + 1)], [(0.0, 1.0, hip.STEP_SOFTMAX_ONLY)] * T)
            for p in range(P):
                xt = eng.bound_noise(labels_dev, tables_dev[p], philox_seed=key)
                eng.set_inputs(xt, cond.index_select(0, image_of[p]), None if feat is None else feat.index_select(0, image_of[p]))
                eng.set_rows(rowmap_dev[p])
                eng.run(1, with_epilogue=True, use_graph=False)
                eng.bound_terms(labels_dev, tables_dev[p], w_dev, self.BOUND_LOG_FLOOR, row_sum, row_weight, pix_map)
                acc.index_add_(0, slot_dev[p], row_sum)                                   # (one row per slot: no two addends meet)
                if return_map:
                    # integer adds: the same sum in any order, so the map does not depend on the packing either
                    surprise_fx.index_add_(0, label_dev[p], torch.round(pix_map.double() * scale_dev[p][:, None]).to(torch.int64))
                self._probe_ranges([eng])
            counted = labels_dev < K
            pixels = counted.sum(dim=1)
            if w_dev is None:
                weight = pixels.double()
            else:
                weight = (w_dev.double()[labels_dev.clamp(max=K - 1).long()] * counted).sum(dim=1)
            terms = acc[:-1].reshape(R, M, draws).sum(dim=2) / draws
        eng.leave()
        eng.raise_if_flagged()                      # the call's one host synchronisation
        prior = weight * bound_prior(cum[T - 1], K)
        bound = prior + (terms * torch.from_numpy(wt_np).to(dev)).sum(dim=1)
        out = {"bound": bound.reshape(B, L), "bits_per_pixel": (bound / (weight * math.log(2.0))).reshape(B, L),
               "terms": terms.reshape(B, L, M), "timesteps": torch.from_numpy(t_np).to(dev).reshape(B, L, M), "prior": prior.reshape(B, L),
               "pixels": pixels.reshape(B, L)}
        if return_map:
            out["surprise"] = (surprise_fx[:-1].double() * 2.0 ** -32).float().reshape(B, L, H, W)
        return out

    def _forward_step(self, x: Tensor, condition: Tensor, feature_condition: Tensor, t: Tensor) -> dict:
        """One U-Net evaluation at per-sample timesteps `t` (diffusion_denoising.py:161-162 -> unet.py:744-808): the
        network's own output (probabilities, or logits with `softmax_output: no`) and, with `ce_head`, the extra head's
        logits (unet.py:716-726,805-807).  `x` must be one-hot (it is everywhere on this path)."""
        eng = self._engine(x, condition, feature_condition)
        N = x.shape[0]
        tt = t.detach().float().reshape(-1).cpu()
        if tt.numel() == 1:
            tt = tt.expand(N)
        with eng.enter():
            eng.set_inputs(self._to_index(x, eng.device), condition.to(eng.device), feature_condition)
            eng.set_tables([float(v) for v in tt], [(0.0, 1.0, hip.STEP_SOFTMAX_ONLY)] * N, per_sample=True)
            eng.run(1, with_epilogue=True, use_graph=False)
            out = eng.out_probs.clone().permute(0, 3, 1, 2)
            logits = eng.ce_logits()
        eng.leave()
        eng.raise_if_flagged()
        self._probe_ranges([eng])
        return {"diffusion_out": out, "logits": logits}

    def _forward_denoising(self, x: Optional[Tensor], condition: Tensor, feature_condition: Tensor,
                           init_t: Optional[int] = None, label_ref_logits: Optional[Tensor] = None, consume=None,
                           guide: Guidance = Guidance()) -> dict:
        """`guide`: the call's checked guidance (guidance.check_guidance), on the model's device."""
        known, evidence, shaping, views, tiles = guide.known, guide.evidence, guide.shaping, guide.views, guide.tiles
        V = 1 if views is None else 1 + len(views)
        if label_ref_logits is not None:
            # the reference's guidance branch reads attributes that do not exist (guidance_scale_weights,
            # diffusion_denoising.py:172-174): it raises AttributeError there too.
            raise AttributeError("'DenoisingModel' object has no attribute 'guidance_scale_weights'")
        T = self.time_steps
        t_values = step_values(T, init_t)
        N, K, H, W = x.shape
        S = len(t_values)
        vote = self.step_T_sample
        last_mode = (hip.STEP_LAST_MAJORITY if vote is None or vote == "majority"
                     else hip.STEP_LAST_CONFIDENCE if vote == "confidence" else hip.STEP_LAST_KEEP)
        coeffs = []
        for t in t_values:
            a, c = self.diffusion.posterior_coeffs(t)
            coeffs.append((a, c, hip.STEP_SAMPLE if t > 1 else last_mode))
        if self.rng not in ("philox", "torch_cpu"):
            raise ValueError(f"unknown rng mode {self.rng!r}")
        host_rng = self.rng == "torch_cpu"
        # evidence, shaping, views, tiles: the network pass of every row stops at x0 (out_probs; x_t untouched), the row's real step follows
        # in guided_step
        stop_at_x0 = evidence is not None or shaping is not None or views is not None or tiles is not None
        # tiles: x and condition are the canvas; the engine's rows are the R tiles of every sample, h x w each (tile_origins)
        oys, oxs = tile_origins(H, W, *tiles) if tiles is not None else ([0], [0])
        R = len(oys) * len(oxs)
        canvases: Dict[int, TileCanvas] = {}                 # the canvas holder of the sub-batch that starts at sample `lo`
        table = coeffs if not stop_at_x0 else [(a_, c_, hip.STEP_SOFTMAX_ONLY) for a_, c_, m_ in coeffs]
        # known labels: cumalpha of the state each row produces; the last row returns the labels themselves (guidance.py)
        clamp_c = [1.0 if j == S - 1 else c_ for j, (a_, c_, m_) in enumerate(coeffs)]
        key = self._philox_key()
        # The rows in the order the walk visits them — (row, 0, None) for row 0 .. S - 1 unless resampling jumps are taken — and per entry
        # the renoising pair (p_stay, p_move) of the jump that precedes it.  From level L to level M = L - j (the state before row M):
        # r = cumalpha_{t_M} / cumalpha_{t_L} in float64, each probability rounded to fp32 once.
        walk = guide.walk(S)
        renoise_p: Dict[int, Tuple[float, float]] = {}
        cum = self.diffusion.cumalphas.detach().cpu().double() if len(walk) > S else None           # (cumalpha_t = cum[t - 1])
        for e, (row, _, src) in enumerate(walk):
            if src is not None:
                r_ = float(cum[t_values[row] - 1]) / float(cum[t_values[src] - 1])
                p_move = (1.0 - r_) / K
                renoise_p[e] = (float(np.float32(r_ + p_move)), float(np.float32(p_move)))
        gN, first = self.noise_slice if (host_rng and self.noise_slice is not None) else (N, 0)
        # Samples are independent through all T steps: the batch may be walked as several contiguous
        # sub-batches, each with its own step executor on its own HIP stream.  The kernels of the low-resolution stages
        # fill a fraction of the GPU; two sub-batches half a step apart fill each other's gaps.  Nothing a sample sees
        # depends on the split (statistics are per sample, slices are a function of the spatial size only, noise is keyed
        # by the global sample index or sliced from the full-batch host draw): the results are bit-identical.
        # automatic: two sub-batches once the batch holds as many pixels as 32 LIDC samples (N >= 32 at 128x128; the Cityscapes-shaped
        # batches of 16 x 256x512 and 4 x 512x1024 qualify: +2.3 % / +2.0 % measured), one below
        def mirrored(a: Tensor) -> Tensor:
            """The V views of a sub-batch's [n,C,h,w] tensor as the engine's rows, view-major: [V * n,C,h,w], view v flipped as it says."""
            return torch.cat([a] + [torch.flip(a, [d for b, d in ((1, 3), (2, 2)) if f & b]) for f in cast(tuple, views)], 0)

        def tiled(a: Tensor) -> Tensor:
            """The R tiles of a sub-batch's [n,C,Hc,Wc] tensor as the engine's rows, tile-major: [R * n,C,h,w], plain crops."""
            h_, w_ = cast(tuple, tiles)[:2]
            return torch.cat([a[:, :, oy:oy + h_, ox:ox + w_] for oy in oys for ox in oxs], 0)

        rows = tiled if tiles is not None else None if views is None else mirrored         # a sub-batch's tensor as the engine's rows
        fc_axis = G.sample_axis(feature_condition, views, tiles)

        def prepare(nsub_: int):
            bounds = [(N * j) // nsub_ for j in range(nsub_ + 1)]
            parts_ = []
            for j in range(nsub_):
                lo, hi = bounds[j], bounds[j + 1]
                xs, cs = (x[lo:hi], condition[lo:hi]) if rows is None else (rows(x[lo:hi]), rows(condition[lo:hi]))
                fc = None
                # [N,...]; with views or tiles [V,N,...] / [R,N,...] (check_views, check_tiles), which a model without an injection point
                # ignores
                if feature_condition is not None and (rows is None or self.unet.spec.feature_condition_idx):
                    fc = feature_condition.narrow(fc_axis, lo, hi - lo)
                    fc = fc.flatten(0, 1) if fc_axis == 1 else fc
                eng = self._engine(xs, cs, fc, slot=j)
                with eng.enter():
                    eng.set_inputs(self._to_index(xs, eng.device), cs.to(eng.device), fc)
                    eng.set_tables([float(t) for t in t_values], table)
                    if tiles is not None:          # the canvas state starts as x_T's class index
                        canvases[lo] = eng.tile_canvas(hi - lo, H, W, tiles[2], tiles[3])
                        canvases[lo].xt.copy_(self._to_index(x[lo:hi], eng.device).reshape(hi - lo, H * W))
                parts_.append((eng, lo, hi))
            return parts_

        def run_row(eng, lo: int, hi: int, row: int, kp: int, renoise, noise, noise_row0_: int, graph_: bool):
            """One walk entry of one sub-batch, all on the engine's stream: the renoise back up the chain to the state before `row` (if a
            jump precedes the entry), the network's step, the guided step behind a network pass that stopped at x0 (one launch: views,
            evidence and shaping), the clamp (the next step reads the clamped state).  kp: the Philox key of this pass of the row."""
            off = self.sample_offset + lo
            if renoise is not None:
                eng.renoise(*renoise, row, philox_seed=kp, sample_offset=off)
            eng.run(1, first_row=row, noise=noise, noise_row0=noise_row0_, philox_seed=kp, sample_offset=off, use_graph=graph_)
            if stop_at_x0:
                eng.guided_step(None if evidence is None else evidence[lo:hi], shaping, views, *coeffs[row], row, philox_seed=kp, sample_offset=off,
                                canvas=canvases.get(lo))
            if known is not None:
                eng.clamp_known_labels(known[lo:hi], clamp_c[row], coeffs[row][2], row, philox_seed=kp, sample_offset=off)

        def run_steps(parts_, s0_: int, s1_: int, noises_, noise_row0_: int, graph_: bool):       # s0_, s1_ count the walk's entries
            if len(parts_) == 1 and not guide:
                parts_[0][0].run(s1_ - s0_, first_row=s0_, noise=noises_[0], noise_row0=noise_row0_, philox_seed=key,
                                 sample_offset=self.sample_offset, use_graph=graph_)
                return
            for e in range(s0_, s1_):                  # one entry of every sub-batch in turn: the streams advance side by side
                row, p, _ = walk[e]
                for j, (eng, lo, hi) in enumerate(parts_):
                    run_row(eng, lo, hi, row, pass_key(key, p), renoise_p.get(e), noises_[j], noise_row0_, graph_)

        nsub = int(self.substreams) if int(self.substreams) > 0 else (
            auto_substreams(V * N, H, W) if tiles is None else auto_substreams(R * N, tiles[0], tiles[1]))
        nsub = max(1, min(nsub, N))
        use_graph = bool(self.use_graph)
        if (int(self.substreams) <= 0 and self.calibrate_mode and not host_rng and self._range_probe is None and nsub > 1
                and S >= self.CALIBRATION_MIN_STEPS and not guide):
            nsub, use_graph = self._calibrate_mode(x, condition, feature_condition, prepare, run_steps, nsub, use_graph, S)
        self.last_mode = (nsub, use_graph)
        parts = prepare(nsub)
        # Step blocks.  Device RNG: one block.  Host RNG (parity mode): the Exp(1) noise is drawn from torch's CPU generator
        # one [gN*H*W, K] block per sampling step — exactly the reference's consumption order, whatever the blocking — and
        # uploaded a bounded number of steps at a time, so host and device hold O(block), not O(T), noise.
        if host_rng:
            per_step = gN * H * W * K * 4
            blk = max(1, HOST_NOISE_BLOCK_BYTES // max(per_step, 1))
            blocks = [(s0, min(s0 + blk, S)) for s0 in range(0, S, blk)]
        else:
            blocks = [(0, len(walk))]
        if self._range_probe is not None:      # diagnosing fp32 re-run: one step per block, every step's activations are probed
            blocks = [(s, s + 1) for s in range(len(walk))]
        for s0, s1 in blocks:
            noises: List[Optional[Tensor]] = [None] * nsub
            if host_rng:
                host = torch.empty((s1 - s0, gN, H * W * K), dtype=torch.float32)
                for j in range(s0, s1):             # one draw per step with t > 1, like torch.multinomial; the last step draws nothing
                    if t_values[j] > 1:
                        host[j - s0].view(-1).exponential_(1)
                for j, (eng, lo, hi) in enumerate(parts):
                    with torch.cuda.stream(eng.stream):
                        noises[j] = host[:, first + lo:first + hi].contiguous().to(eng.device)
            run_steps(parts, s0, s1, noises, s0, use_graph)
            self._probe_ranges([p_[0] for p_ in parts])
        outs = []
        for eng, lo, hi in (parts if consume is None else []):
            with eng.enter():
                n_ = hi - lo                                   # (with views the engine holds V * n_ rows: view 0 is the first n_)
                src = canvases.get(lo, eng)                    # (with tiles the outputs are the canvas's: n_ rows of H x W)
                if t_values[-1] > 1 or last_mode == hip.STEP_LAST_KEEP:
                    idx = src.xt.reshape(-1, H, W)[:n_].long()
                    out = torch.nn.functional.one_hot(idx, K).permute(0, 3, 1, 2).to(torch.float32)
                elif last_mode == hip.STEP_LAST_CONFIDENCE:
                    out = src.out_probs[:n_].clone().permute(0, 3, 1, 2)     # BCHW view of channels-last memory, like the reference
                else:
                    out = src.out_onehot[:n_].clone().permute(0, 3, 1, 2)
            eng.leave()
            outs.append(out)
        # read AND clear the sticky range flag of every sub-batch engine before raising: a flag left set on a cached engine would
        # fail the next, unrelated call on it
        flagged = [eng.check_and_clear_flag() for eng, lo, hi in parts]
        if any(flagged):
            parts[0][0].raise_range_error()
        if consume is not None:            # (only after the flag check: a range-error re-run must not be consumed twice)
            for eng, lo, hi in parts:
                with eng.enter():
                    consume(canvases.get(lo, eng), lo, hi)
                eng.leave()
            return {}
        out = outs[0] if nsub == 1 else torch.cat(outs, 0)
        if out.device != x.device:
            out = out.to(x.device)
        return {"diffusion_out": out}


def build_model(
        time_steps: int,
        schedule: str,
        schedule_params: Union[dict, None],
        input_shapes: List[Tuple[int, int, int]],
        cond_encoded_shape,
        backbone: str,
        backbone_params: Dict[str, Any],
        dataset_file: str,
        step_T_sample: str = None,
        feature_cond_encoder: dict = None
) -> DenoisingModel:
    """Same signature and dispatch as the reference's backbone registry (builder.py:14-51)."""
    img_shape, label_shape = input_shapes
    img_channels = img_shape[0]
    num_classes = label_shape[0]
    if not 2 <= num_classes <= hip.MAX_CLASSES:
        # x_t travels as a uint8 class index; up to 32 classes a pixel's K values stay in registers, more go through LDS rows
        # (ccdm_sampler.hip: k_posterior_many).  The reference's datasets have 2 (LIDC) and 20 (Cityscapes) classes.
        raise ValueError(f"label shape {tuple(label_shape)}: {num_classes} classes, the HIP sampler is built for 2..{hip.MAX_CLASSES} (DESIGN.md section 8)")
    diffusion = DiffusionModel(schedule, time_steps, num_classes, schedule_params=schedule_params)
    if backbone == "unet_openai":
        spec = make_unet_spec(
            image_size=min(img_shape[1], img_shape[2]),
            in_channels=num_classes + img_channels,
            out_channels=num_classes,
            num_res_blocks=2,
            cond_encoded_shape=cond_encoded_shape,
            feature_cond_encoder=feature_cond_encoder,
            **backbone_params
        )
        model = UNetModel(spec)
    else:
        raise NotImplementedError(f"backbone {backbone}")
    LOGGER.info("%s trainable params: %d", backbone, spec.num_params())
    return DenoisingModel(diffusion, model, dataset_file, step_T_sample)
