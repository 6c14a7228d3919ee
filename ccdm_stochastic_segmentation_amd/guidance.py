"""What the host knows about a sampling call's guidance: the seven keywords of DenoisingModel's `forward`, `forward_denoising` and
`predict_multiple` (GUIDANCE_KEYWORDS), their host-side checks (before anything runs), and the checked bundle the sampler walks with
(`Guidance`).  The keywords:

`known_labels` (keyword of `forward`, `forward_denoising`, `predict_multiple`): sample segmentations that agree with labels already at
hand — an integer map [N,H,W] holding a class in [0,K) where the label is known and 255 where the pixel is free.  The replacement
method of RePaint (Lugmayr et al. 2022) for categorical diffusion, no retraining: after every reverse step each known pixel is
overwritten with a draw from the forward process at that step's noise level, q(x_{t-1} | x_0 = y) = Cat(cumalpha_{t-1} onehot(y) +
(1 - cumalpha_{t-1}) / K) (ccdm_known_labels_step, one launch per step and sub-batch), so the network sees known pixels that carry the
right amount of noise and denoises the free ones in agreement with them.  x_T is left as given (at t = T the forward process is
uniform to within cumalpha_T); the state a walk returns carries the labels themselves: its last row is clamped with cumalpha = 1, at
t = 1 (where cumalpha_0 = 1 anyway) and on a walk that stops above it.  The draw is keyed by (pixel, global sample index, step row)
under the call's Philox key on counters the epilogue never uses: results do not depend on `substreams`, `use_graph` or how the
batch is sharded (a caller that shards passes its shard's slice of the map).  A conditioned call walks every engine one step at a
time and takes the static execution-mode rule (no `calibrate_mode` measurement); rng = "torch_cpu" has no reference stream for this
draw and is refused.  Without the keyword nothing changes: no extra launch, no per-step stepping.
`resample` = (jump_length, resamples) (keyword next to `known_labels`, which it needs): RePaint's resampling jumps.  With the
clamp alone the free pixels get one reverse step per noise level to agree with known pixels that were drawn independently of them.
A resampled walk goes back up the chain by `jump_length` levels at every jump point and walks down again, `resamples` times per
band (`resample_walk` is the order of the rows), so the free pixels are denoised again with the known ones in view.  Going up is
one launch of ccdm_renoise_step whatever the jump length: every pixel is redrawn from q(x_t | x_{t-j}) = Cat(r onehot(x_{t-j}) +
(1 - r) / K), r = cumalpha_t / cumalpha_{t-j}.  Pass p of a row draws under pass_key(key, p), so a revisit sees fresh noise and the
walk up to the first jump is the plain conditioned walk bit for bit.  The step tables, the captured graphs and the independence of
`substreams`, `use_graph` and sharding are those of a conditioned call.  None, (j, 1), (0, r) and a jump_length without a jump
point change nothing.
`evidence` (keyword next to `known_labels`): sample under per-pixel SOFT evidence — a float map [N,K,H,W] of class weights in
[0,1], w_k proportional to the likelihood p(e | x_0 = k) of independent evidence e at that pixel: a scribble the annotator is fairly
sure of (0.9 on its class, 0.1 elsewhere), another model's or rater's probability map, classes that are impossible in a region
(weight 0), a per-class re-weighting for prior shift; all-ones is no evidence.  Exact for categorical diffusion, no gradient, no
scale, no retraining: the network predicts x0 = p(x_0 | x_t), Bayes gives p(x_0 | x_t, e) proportional to x0_k w_k, and the
reverse step's posterior is linear in that vector up to its normalisation — so every row's network pass stops at x0
(STEP_SOFTMAX_ONLY) and ccdm_evidence_step multiplies it by w and does the row's step with the counters of the unguided draw
(all-ones evidence reproduces the unguided call bit for bit).  The call walks like one with known labels: one step at a time, the
static execution-mode rule, results independent of `substreams`, `use_graph` and sharding (a caller that shards passes its shard's
slice).  Per walk entry: renoise (if a jump precedes), the network, the evidence step, the clamp — `evidence` composes with
`known_labels` and `resample`, whose rules do not change.  A pixel whose weights are all 0, a value outside [0,1], rng =
"torch_cpu" and a model with `softmax_output: no` (its x0 holds logits) are refused.
`temperature`, `truncation` (keywords next to `known_labels`): the two controls of a generative sampler, applied per pixel to the
network's x0 before the reverse step (ccdm_shaped_step; include/ccdm_hip.h has the definition).  temperature tau in [0.05, 20]
raises x0, relative to the pixel's largest value, to the power 1 / tau: below 1 the samples get less diverse and individually more
accurate, above 1 the reverse.  truncation r in (0, 1] ("top-r", the truncation sampling of Improved VQ-Diffusion, Tang et al.
2022) keeps the smallest set of classes whose mass reaches r and drops the rest, so a draw never picks a class the network gives
1 % to; it matters most on short strided walks.  Temper first, then truncate; nothing is renormalised, because the step posterior
is linear in x0 up to its own normalisation.  The last row's vote sees the shaped x0 too.  A shaped call walks like one with
evidence (every row's network pass stops at x0, one ccdm_shaped_step launch per walk entry, which also applies the evidence where
the call has some: no ccdm_evidence_step launch then), takes the static execution-mode rule and composes with `known_labels`,
`resample` and `evidence`.  A set keyword runs this path even at the neutral value 1.0, which reproduces the plain call bit for
bit; None for both changes nothing.  One (tau, r) per call: every row and every pass of predict_multiple uses it.  A training or
validation call, rng = "torch_cpu" and a model with `softmax_output: no` are refused.
`views` (keyword next to `known_labels`): flip test-time augmentation inside the sampler.  A tuple of distinct names from "hflip"
(mirrors x), "vflip" (mirrors y) and "hvflip" (both); the identity is always view 0, so V = 1 + len(views) <= 4.  At every reverse
step the network runs on all V mirror images of (x_t, image) and x0 is their mean, each mapped back: x0_sym = 1/V sum_g g^-1
x0(g x_t, g image), a denoiser that is exactly equivariant under the listed flips where the trained one is only approximately so.
Exact for categorical diffusion (a mean of probability vectors is one; the step posterior is linear in x0 up to its own
normalisation), no retraining, V network passes per step.  The V views of a sample are V rows of the engine's batch, view-major
(row v * n + j of a sub-batch of n samples is view v of sample j; the host mirrors x_T, the image and the features with torch.flip);
every row's network pass stops at x0 and ONE ccdm_views_step launch per walk entry takes the mean, applies `evidence`, `temperature`
and `truncation` where the call has them (it replaces those launches), draws with the counters of the plain call — keyed by the
identity view's pixel and the sample, never by the engine row — and writes the drawn class to every view at its mirrored place
(include/ccdm_hip.h has the definition).  Results are read from view 0.  A call with views takes the static execution-mode rule
(`auto_substreams` sees V * N samples) and does not depend on `substreams`, `use_graph` or sharding.  A model that takes a
`feature_condition` needs the features of every view from the caller's own encoder, [V,N,Cf,h,w] with view v computed from the
mirrored image.  Refused: unknown or duplicate names, a training or validation call, rng = "torch_cpu", `softmax_output: no`, and
`known_labels` / `resample` together with views (the clamp and the renoise draw per engine row, so the views would stop being
mirror images of one another: not built).  `views=()` or None is the plain call: no code path changes.
`tiles` = (h, w, sy, sx) (keyword next to `known_labels`): sample a canvas larger than the geometry the network was trained at — a
180x180 slice with a 128x128 model, a whole frame with a model trained on crops.  `x` is then the canvas x_T [N,K,Hc,Wc] and
`condition` the canvas image [N,C,Hc,Wc].  Windows sampled independently and pasted would disagree at the seams; this is the
MultiDiffusion construction (Bar-Tal et al. 2023) instead: ONE chain runs on the canvas, at every reverse step the network runs on
overlapping h x w tiles of the current canvas state (strides sy <= h, sx <= w; `tile_origins` has the tiling: the last tile along an
axis is pushed back to end at the border) and x0 of a canvas pixel is the mean over the c >= 1 tiles that cover it.  Exact for
categorical diffusion in the sense of `views` (a mean of probability vectors is one; the step posterior is linear in x0 up to its
own normalisation), no retraining, R network passes of h x w per step.  The R tiles of a sample are R rows of the engine's batch,
tile-major (row r * n + j of a sub-batch of n samples is tile r of sample j; the host crops x_T and the image by plain slicing);
every row's network pass stops at x0 and ONE ccdm_tiled_step launch per walk entry takes the per-pixel mean, applies `evidence`
(a canvas map [N,K,Hc,Wc]), `temperature` and `truncation` where the call has them (it replaces those launches), draws with the
counters of a plain call at the canvas's size — keyed by the canvas pixel and the sample, never by the engine row or tile — and
writes the drawn class to the canvas state and to every covering tile, so the tiles stay crops of one state (include/ccdm_hip.h
has the definition).  Results [N,K,Hc,Wc] are read from the canvas holder (engine.TileCanvas), which is also what `consume` gets.
A tiled call takes the static execution-mode rule (`auto_substreams` sees R * N samples of h x w; sub-batches split by sample, all
tiles of a sample in one engine) and does not depend on `substreams`, `use_graph` or sharding; one tile that is the canvas
reproduces the plain call bit for bit.  A model that takes a `feature_condition` needs the features of every tile from the caller's
own encoder, [R,N,Cf,hf,wf] (evaluation.tile_features).  Refused: anything but four integers, a stride < 1 or beyond the tile, a
tile larger than the canvas, a training or validation call, rng = "torch_cpu", `softmax_output: no`, and `views`, `known_labels`
or `resample` together with tiles (the clamp and the renoise draw per engine row, so overlapping tiles would stop being crops of
one state: not built).  The mean is uniform (no feathered weights) and all R * N rows run in one engine (no chunking).  None is the
plain call: no code path changes.

The checks take the model as their first argument and read `model.training`, `model.rng`, `model.unet.spec` and the device of its
parameters.  The order in which keywords are checked is behaviour (it decides which of two bad keywords is named): `check_guidance`
has the order of a sampling call, `refuse_outside_sampling` that of a training or validation call."""
from __future__ import annotations

import dataclasses
import math
from typing import Iterable, List, Mapping, Optional, Tuple, cast

import numpy as np
import torch
from torch import Tensor

GUIDANCE_KEYWORDS = ("known_labels", "resample", "evidence", "temperature", "truncation", "views", "tiles")

VIEW_FLIPS = {"hflip": 1, "vflip": 2, "hvflip": 3}        # ccdm_views_step's two bits per view: bit 0 mirrors x, bit 1 mirrors y

KNOWN_FREE = 255        # the value of a free pixel in `known_labels`


def resample_walk(S: int, jump_length: int, resamples: int) -> List[Tuple[int, int, Optional[int]]]:
    """The order in which a walk of S table rows with RePaint's resampling jumps (Lugmayr et al. 2022) visits its rows: a list of
    (row, pass, renoise_from).  Level L is the state before row L, R = S - L rows remain below it.  Jump points are the levels with
    R in {j, 2j, 3j, ...} and R < S - j (j = jump_length): the walk never jumps back to the pure-noise level (RePaint's rule).  Each
    jump point has `resamples` - 1 jumps; walking down, a level that has jumps left uses one: the state is renoised from level L to
    level L - j and the walk continues at row L - j.  `pass` counts the earlier visits of the row (it selects the noise key of the
    visit, see pass_key); `renoise_from` is the level the state is renoised from before this row runs, or None.
    A deviation from RePaint: no jump starts at R = 0.  The last row returns an argmax or a probability map, not a draw of the chain,
    so there is nothing to renoise.  resamples = 1 or jump_length = 0 gives the plain walk; so does a jump_length with no jump point.
    The length is S + (resamples - 1) * j * #{m >= 1 : m * j < S - j}."""
    S, j, r = int(S), int(jump_length), int(resamples)
    left = {R: r - 1 for R in range(j, S - j, j)} if (j > 0 and r > 1) else {}
    visits = [0] * S
    walk: List[Tuple[int, int, Optional[int]]] = []
    L, renoise_from = 0, None
    while L < S:
        walk.append((L, visits[L], renoise_from))
        visits[L] += 1
        renoise_from = None
        L += 1
        if left.get(S - L, 0) > 0:
            left[S - L] -= 1
            renoise_from = L
            L -= j
    return walk


def tile_origins(Hc: int, Wc: int, h: int, w: int, sy: int, sx: int) -> Tuple[List[int], List[int]]:
    """The tiling of a canvas Hc x Wc by tiles h x w at strides (sy, sx), 1 <= sy <= h <= Hc and 1 <= sx <= w <= Wc, as include/ccdm_hip.h
    defines it (ccdm_tiled_step derives the same origins): (oys, oxs) with oys[i] = min(i * sy, Hc - h) for the Ty = 1 + ceil((Hc - h) /
    sy) tiles along y — the last tile is pushed back so that it ends at the border; the origins are distinct and leave no gap — and the
    same along x.  Tile r = i * len(oxs) + j covers rows oys[i] .. oys[i] + h - 1 and columns oxs[j] .. oxs[j] + w - 1."""
    Hc, Wc, h, w, sy, sx = (int(v) for v in (Hc, Wc, h, w, sy, sx))
    if not (1 <= sy <= h <= Hc and 1 <= sx <= w <= Wc):
        raise ValueError(f"tiles: need 1 <= sy <= h <= Hc and 1 <= sx <= w <= Wc, got canvas {Hc}x{Wc}, tile {h}x{w}, strides ({sy}, {sx})")
    return ([min(i * sy, Hc - h) for i in range(1 + -((h - Hc) // sy))],
            [min(j * sx, Wc - w) for j in range(1 + -((w - Wc) // sx))])


@dataclasses.dataclass(frozen=True)
class Guidance:
    """What guides one sampling call, as check_guidance returns it: `known` uint8 [N,H*W] (check_known_labels), `jumps`
    (jump_length, resamples) (check_resample), `evidence` fp32 [N,H*W,K] (check_evidence), `shaping` (inv_temperature, top_r)
    (check_shaping), `views` the flip codes of views 1 .. V - 1 (check_views: bit 0 mirrors x, bit 1 mirrors y; view 0 is the identity),
    `tiles` (h, w, sy, sx) (check_tiles); None each where the call has none."""
    known: Optional[Tensor] = None
    jumps: Optional[Tuple[int, int]] = None
    evidence: Optional[Tensor] = None
    shaping: Optional[Tuple[float, float]] = None
    views: Optional[Tuple[int, ...]] = None
    tiles: Optional[Tuple[int, int, int, int]] = None

    def __bool__(self) -> bool:
        """The walk has something to do between the network's steps (jumps need known labels)."""
        return self.known is not None or self.evidence is not None or self.shaping is not None or self.views is not None \
            or self.tiles is not None

    def walk(self, S: int) -> List[Tuple[int, int, Optional[int]]]:
        """The (row, pass, renoise_from) entries of a walk of S table rows: resample_walk's; [(s, 0, None) ...] without jumps."""
        return resample_walk(S, *(self.jumps or (0, 1)))

    def repeat_interleave(self, S: int) -> "Guidance":
        """For a batch in which every sample is repeated S times (predict_multiple(batched=True))."""
        return Guidance(*(v.repeat_interleave(S, dim=0) if isinstance(v, Tensor) else v
                          for v in (self.known, self.jumps, self.evidence, self.shaping, self.views, self.tiles)))


def known_keywords(where: str, names: Iterable[str]) -> None:
    """What Python says of a keyword that function `where` does not take, for the entry points that take the guidance as `**guidance`."""
    for k in names:
        if k not in GUIDANCE_KEYWORDS:
            raise TypeError(f"{where}() got an unexpected keyword argument {k!r}")


def sample_axis(feature_condition: Optional[Tensor], views, tiles) -> int:
    """The dimension of `feature_condition` that counts the samples: 1 where a call with views or tiles carries the features of every
    view or tile, [V,N,...] / [R,N,...] (check_views, check_tiles), else 0.  views, tiles: the raw keywords or the checked values."""
    per_row = (views is not None and len(views) > 0) or tiles is not None
    return 1 if (per_row and feature_condition is not None and feature_condition.ndim == 5) else 0


# ------------------------------------------------------------------------------------------------------------------ the checks
# the sentence tails of the three shared preconditions, per keyword (and label_bound, which shares two): why only a sampling call takes
# it, what the host-noise parity mode lacks for it, what logits cannot do for it (None: not asked)
_NO_STEP = "replays the reference's draws, and the reference has no {} step to be in parity with"
_NO_MEAN = ", whose mean is not the mean of the probabilities"
_NO_SHAPE = ", which cannot be tempered or truncated as probabilities"
PRECONDITION_TAILS = {
    "tiles": ("has a canvas to sample", _NO_STEP.format("tiled"), _NO_MEAN),
    "views": ("has a denoiser to average", _NO_STEP.format("view-averaged"), _NO_MEAN),
    "temperature": ("has a draw to shape", _NO_STEP.format("shaped"), _NO_SHAPE),
    "truncation": ("has a draw to shape", _NO_STEP.format("shaped"), _NO_SHAPE),
    "evidence": ("takes evidence", _NO_STEP.format("guided"), ", which weights cannot multiply"),
    "resample": ("has a walk to resample", "has no reference stream for the renoising draws", None),
    "known_labels": ("takes known labels", "has no reference stream for the draw at the known pixels", None),
    "label_bound": (None, "has no reference stream for the forward draws", ""),
}


def require(model, name: str, sampling: Optional[bool] = True) -> None:
    """The shared preconditions of `name`, in this order: a sampling call (sampling = False: the call is a training or validation
    one; None: not asked here), not rng = "torch_cpu", a model whose x0 holds probabilities."""
    call, parity, logits = PRECONDITION_TAILS[name]
    if sampling is not None and (not sampling or model.training):
        raise ValueError(f"{name}: only a sampling call (eval mode, validation=False) {call}")
    if model.rng == "torch_cpu":
        raise ValueError(f"{name}: not available with rng = 'torch_cpu' (the host-noise parity mode {parity}); use rng = 'philox'")
    if logits is not None and not model.unet.spec.softmax_output:
        raise ValueError(f"{name}: needs a model whose output is a probability vector; with `softmax_output: no` x0 holds logits{logits}")


def _integer(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _need_row_features(model, name: str, feature_condition, rows: Optional[int], shape, layout: str, source: str) -> None:
    """A model that takes a feature_condition needs one leading entry per view or tile: [rows,N,...] (`shape`: the call's, or None)."""
    if feature_condition is None or not model.unet.spec.feature_condition_idx:
        return
    want = None if shape is None else (rows, int(shape[0]))
    if not isinstance(feature_condition, Tensor) or feature_condition.ndim != 5 or \
            (want is not None and tuple(feature_condition.shape[:2]) != want):
        raise ValueError(f"{name}: this model takes a feature_condition, and with {name} it needs the features of every {name[:-1]}, "
                         f"{layout} ({source}), got {tuple(getattr(feature_condition, 'shape', ()))}")


def _refuse_with_rows(name: str, known_labels, resample, consequence: str) -> None:
    if known_labels is not None or resample is not None:
        raise ValueError(f"{name}: not available together with {'known_labels' if known_labels is not None else 'resample'} (the clamp "
                         f"and the renoise draw per engine row, so {consequence})")


def check_tiles(model, tiles, sampling: bool = True, *, views=None, known_labels=None, resample=None, feature_condition=None,
                shape: Optional[Tuple[int, int, int, int]] = None) -> Optional[Tuple[int, int, int, int]]:
    """The one host-side check of a call's `tiles` (before anything runs): (h, w, sy, sx) as four ints, or None where the call has
    none.  shape: the call's (N,K,Hc,Wc), the canvas."""
    if tiles is None:
        return None
    if isinstance(tiles, (str, bytes)) or not isinstance(tiles, (tuple, list)) or len(tiles) != 4 or not all(_integer(v) for v in tiles):
        raise ValueError(f"tiles: expected (h, w, sy, sx), four integers (tile height and width, strides along y and x), got {tiles!r}")
    h, w, sy, sx = (int(v) for v in tiles)
    if not (1 <= sy <= h and 1 <= sx <= w):
        raise ValueError(f"tiles: need 1 <= sy <= h and 1 <= sx <= w (a stride beyond the tile would leave gaps), got tile {h}x{w}, "
                         f"strides ({sy}, {sx})")
    if shape is not None and (h > int(shape[2]) or w > int(shape[3])):
        raise ValueError(f"tiles: the tile {h}x{w} is larger than the canvas {int(shape[2])}x{int(shape[3])}")
    require(model, "tiles", sampling)
    if views is not None and len(views) > 0:
        raise ValueError("tiles: not available together with views (not built)")
    _refuse_with_rows("tiles", known_labels, resample, "overlapping tiles would stop being crops of one state")
    R = None if shape is None else math.prod(len(o) for o in tile_origins(int(shape[2]), int(shape[3]), h, w, sy, sx))
    _need_row_features(model, "tiles", feature_condition, R, shape, f"[R,N,Cf,hf,wf]{'' if R is None else f' with R = {R}'}",
                        "tile r from the caller's encoder on the cropped image: evaluation.tile_features")
    return h, w, sy, sx


def check_views(model, views, sampling: bool = True, *, known_labels=None, resample=None, feature_condition=None,
                shape: Optional[Tuple[int, int, int, int]] = None) -> Optional[Tuple[int, ...]]:
    """The one host-side check of a call's `views` (before anything runs): the flip codes of views 1 .. V - 1 as ccdm_views_step
    takes them (VIEW_FLIPS), or None where the call has no views (None or an empty sequence: the plain call).  shape: the call's
    (N,K,H,W)."""
    if views is None:
        return None
    if isinstance(views, (str, bytes)) or not isinstance(views, (tuple, list)):
        raise ValueError(f"views: expected a sequence of names from {list(VIEW_FLIPS)}, got {views!r}")
    if len(views) == 0:
        return None
    bad = [v for v in views if not isinstance(v, str) or v not in VIEW_FLIPS]
    if bad:
        raise ValueError(f"views: unknown name(s) {bad} (expected names from {list(VIEW_FLIPS)}; the identity is always a view)")
    if len(set(views)) != len(views):
        raise ValueError(f"views: duplicate name(s) in {list(views)} (every view counts once in the mean)")
    require(model, "views", sampling)
    _refuse_with_rows("views", known_labels, resample, "the views would stop being mirror images of one another")
    V = 1 + len(views)
    _need_row_features(model, "views", feature_condition, V, shape, f"[V,N,Cf,h,w] with V = {V}",
                        "view v from the caller's encoder on the mirrored image")
    return tuple(VIEW_FLIPS[v] for v in views)


def check_shaping(model, temperature, truncation, sampling: bool = True) -> Optional[Tuple[float, float]]:
    """The one host-side check of a call's `temperature` and `truncation` (before anything runs): (inv_temperature, top_r) as
    ccdm_shaped_step takes them — inv_temperature = 1 / temperature in float64, rounded to fp32 once — or None where neither
    keyword is set.  A keyword that is not set counts as 1.0."""
    if temperature is None and truncation is None:
        return None
    if temperature is not None and not (_real(temperature) and 0.05 <= float(temperature) <= 20.0):          # (a NaN fails both)
        raise ValueError(f"temperature: expected a real number in [0.05, 20], got {temperature!r}")
    if truncation is not None and not (_real(truncation) and 0.0 < float(truncation) <= 1.0):
        raise ValueError(f"truncation: expected a real number in (0, 1], got {truncation!r}")
    require(model, "temperature" if temperature is not None else "truncation", sampling)
    inv_temperature = 1.0 if temperature is None else float(np.float32(1.0 / float(temperature)))
    return inv_temperature, (1.0 if truncation is None else float(np.float32(float(truncation))))


def check_evidence(model, evidence: Tensor, shape: Optional[Tuple[int, int, int, int]], sampling: bool = True) -> Tensor:
    """The one host-side check of a call's `evidence` (before anything runs): the map as contiguous fp32 [N,H*W,K] on the model's
    device.  shape: the call's (N,K,H,W)."""
    require(model, "evidence", sampling)
    if not isinstance(evidence, Tensor) or not evidence.dtype.is_floating_point:
        raise ValueError(f"evidence: expected a floating-point tensor of class weights in [0,1], got "
                         f"{getattr(evidence, 'dtype', type(evidence).__name__)}")
    shape = tuple(int(v) for v in cast(tuple, shape))
    if tuple(evidence.shape) != shape:
        raise ValueError(f"evidence: expected shape {shape} = [N,K,H,W], got {tuple(evidence.shape)}")
    host = evidence.detach().to(torch.float32).cpu()
    if not bool(torch.isfinite(host).all()):
        raise ValueError("evidence: values must be finite weights in [0,1]; found NaN or infinity")
    if bool((host < 0).any()) or bool((host > 1).any()):
        bad = host[(host < 0) | (host > 1)][0]
        raise ValueError(f"evidence: values must be weights in [0,1]; found {float(bad)}")
    if bool((host.max(dim=1).values <= 0).any()):
        raise ValueError("evidence: a pixel whose K weights are all 0 rules out every class there")
    N, K, H, W = shape
    return host.permute(0, 2, 3, 1).reshape(N, H * W, K).contiguous().to(next(model.unet.parameters()).device)


def check_resample(model, resample, known_labels) -> Optional[Tuple[int, int]]:
    """The one host-side check of a call's `resample` (before anything runs): (jump_length, resamples) as two ints, or None where
    the pair asks for no jump."""
    if resample is None:
        return None
    if known_labels is None:
        raise ValueError("resample: needs known_labels (the jumps harmonise the free pixels with the known ones; without any there "
                         "is nothing to harmonise)")
    require(model, "resample", None)
    ok = isinstance(resample, (tuple, list)) and len(resample) == 2 and all(_integer(v) for v in resample)
    if not ok or int(resample[0]) < 0 or int(resample[1]) < 1:
        raise ValueError(f"resample: expected (jump_length, resamples), two integers with jump_length >= 0 and resamples >= 1, got {resample!r}")
    j, r = int(resample[0]), int(resample[1])
    return None if (j == 0 or r == 1) else (j, r)


def check_known_labels(model, known_labels: Tensor, shape: Tuple[int, int, int], K: int) -> Tensor:
    """The one host-side check of a call's `known_labels` (before anything runs): the map as uint8 [N,H*W] on the model's device."""
    require(model, "known_labels", None)
    if not isinstance(known_labels, Tensor) or known_labels.dtype in (torch.bool,) or known_labels.dtype.is_floating_point \
            or known_labels.dtype.is_complex:
        raise ValueError(f"known_labels: expected an integer tensor (a class in [0,{K}) where the label is known, {KNOWN_FREE} where the "
                         f"pixel is free), got {getattr(known_labels, 'dtype', type(known_labels).__name__)}")
    shape = tuple(int(v) for v in shape)
    if tuple(known_labels.shape) != shape:
        raise ValueError(f"known_labels: expected shape {shape} = [N,H,W], got {tuple(known_labels.shape)}")
    host = known_labels.detach().cpu()
    bad = ((host < 0) | (host >= K)) & (host != KNOWN_FREE)
    if bool(bad.any()):
        raise ValueError(f"known_labels: values must be classes in [0,{K}) or {KNOWN_FREE} (free); found {int(host[bad][0])}")
    return host.to(torch.uint8).reshape(shape[0], shape[1] * shape[2]).contiguous().to(next(model.unet.parameters()).device)


def check_guidance(model, guidance: Mapping, shape: Optional[Tuple[int, int, int, int]], feature_condition=None) -> Guidance:
    """The host-side checks of a sampling call's guidance keywords (before anything runs), in this order; guidance: the keywords by
    name (one that is missing counts as None), shape: the call's (N,K,H,W)."""
    known_labels, resample, evidence, temperature, truncation, views, tiles = (guidance.get(k) for k in GUIDANCE_KEYWORDS)
    geom = check_tiles(model, tiles, views=views, known_labels=known_labels, resample=resample, feature_condition=feature_condition,
                       shape=shape)
    flips = check_views(model, views, known_labels=known_labels, resample=resample, feature_condition=feature_condition, shape=shape)
    shaping = check_shaping(model, temperature, truncation)
    ev = None if evidence is None else check_evidence(model, evidence, shape)
    jumps = check_resample(model, resample, known_labels)
    known = None if known_labels is None else check_known_labels(model, known_labels, (shape[0], shape[2], shape[3]), shape[1])
    return Guidance(known, jumps, ev, shaping, flips, geom)


def refuse_outside_sampling(model, guidance: Mapping) -> None:
    """A training or validation call refuses every guidance keyword that is set, in this order (each check keeps its own: `tiles`
    looks at its four integers first, `evidence` refuses the call first)."""
    if guidance.get("evidence") is not None:
        check_evidence(model, guidance["evidence"], None, sampling=False)
    check_tiles(model, guidance.get("tiles"), sampling=False)
    check_shaping(model, guidance.get("temperature"), guidance.get("truncation"), sampling=False)
    check_views(model, guidance.get("views"), sampling=False)
    for name in ("known_labels", "resample"):
        if guidance.get(name) is not None:
            require(model, name, sampling=False)
