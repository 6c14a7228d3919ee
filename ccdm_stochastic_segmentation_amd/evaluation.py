"""Evaluation harness around the sampler: the callers of the hot path, with the reference's
parameter-file keys.

    eval_lidc_uncertainty(params)      /root/reference/evaluation/evaluate_lidc_uncertainty.py:164-216 (Tester.test_step :89-136)
    eval_lidc_sampling_speed(params)   /root/reference/evaluation/evaluate_lidc_sampling_speed.py:165-223 (t = 10000 + K sweep)
    predict_multiple(model, image, params)  /root/reference/evaluation/eval_cdm.py:206-212 (Evaluator: predict_single / predict_multiple)

No ignite: the loop is a plain `for batch in loader`.  The dataset is `datasets.lidc`'s Test_LIDC re-stated on h5py
when `data_lidc.hdf5` is available, or a deterministic synthetic stand-in (`dataset_file: synthetic.lidc`) so the
entry point runs end to end without the (non-redistributable) data.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass
from fractions import Fraction
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import metrics as M
from .guidance import VIEW_FLIPS, tile_origins
from .models import OneHotCategoricalBCHW, build_model

LOGGER = logging.getLogger(__name__)


def expanduservars(path: str) -> str:
    return os.path.expanduser(os.path.expandvars(path))


# ------------------------------------------------------------------------------------------------ data
class SyntheticLIDC(torch.utils.data.Dataset):
    """LIDC-shaped stand-in: image [1,128,128] in [-1,1], four one-hot annotations [4,2,128,128] (discs of jittered radius)."""
    NUM_CLASSES, RESOLUTION = 2, 128

    def __init__(self, size: int = 8, seed: int = 0):
        self.size, self.seed = size, seed

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed * 100003 + i)
        r = self.RESOLUTION
        yy, xx = np.mgrid[0:r, 0:r]
        cy, cx, rad = rng.uniform(40, 88), rng.uniform(40, 88), rng.uniform(6, 20)
        image = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * rad ** 2)) + 0.1 * rng.standard_normal((r, r))
        image = torch.from_numpy(((image - 0.5) * 2).astype(np.float32))[None].clamp(-1, 1)
        labs = []
        for a in range(4):
            ra = rad * rng.uniform(0.6, 1.3) if rng.random() > 0.2 else 0.0       # an annotator may mark nothing
            m = ((yy - cy) ** 2 + (xx - cx) ** 2 <= ra ** 2).astype(np.int64)
            labs.append(torch.nn.functional.one_hot(torch.from_numpy(m), 2).permute(2, 0, 1).float())
        return image, torch.stack(labs), np.array([0.25, 0.25, 0.25, 0.25])


class TestLIDC(torch.utils.data.Dataset):
    """`Test_LIDC` + `batch_transform` of the reference (datasets/lidc.py:164-198): image*2 -> [-1,1]; labels
    [4,2,128,128] one-hot; uniform annotator weights.  `source` is the path of `data_lidc.hdf5` (read with h5py) or any
    mapping with the file's layout: source[split]["images"][i] -> [128,128] float, source[split]["labels"][i] -> [4,128,128]
    integer.  A path ending in `.npz` is read with numpy as a mirror of the HDF5 file (arrays named "<split>/images" and
    "<split>/labels": `tools/lidc_hdf5_to_npz.py` writes one where h5py exists) — the file form that runs on hosts without h5py.
    `max_size` follows `test_dataset(max_size)` (datasets/lidc.py:201-210): None = the whole split, else the
    first max_size items (the reference's Subset(range(max_size)) fails when the split is smaller; here it is capped)."""

    def __init__(self, source, split: str = "test", max_size: Optional[int] = None):
        if isinstance(source, (str, os.PathLike)) and str(source).endswith(".npz"):
            arrays = np.load(source)
            missing = [k for k in (f"{split}/images", f"{split}/labels") if k not in arrays.files]
            if missing:
                raise KeyError(f"{source}: no array named {missing[0]!r} (an .npz mirror of data_lidc.hdf5 holds '<split>/images' and '<split>/labels')")
            source = {split: {"images": arrays[f"{split}/images"], "labels": arrays[f"{split}/labels"]}}
        elif isinstance(source, (str, os.PathLike)):
            try:
                import h5py
            except ImportError as e:
                raise ImportError("reading data_lidc.hdf5 needs h5py (README.md, requirements), which is not installed here; "
                                  "tools/lidc_hdf5_to_npz.py writes an .npz mirror this reader takes without it") from e
            source = h5py.File(source, "r")
        self.ds = source[split]
        self.n = len(self.ds["images"]) if max_size is None else min(int(max_size), len(self.ds["images"]))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        image = torch.from_numpy(np.asarray(self.ds["images"][i], dtype=np.float32))[None] * 2
        labs = [torch.nn.functional.one_hot(torch.from_numpy(np.asarray(self.ds["labels"][i][a]).astype(np.int64)), 2).permute(2, 0, 1).float()
                for a in range(4)]
        return image, torch.stack(labs), np.array([0.25, 0.25, 0.25, 0.25])


def make_dataset(params: dict):
    name = params["dataset_file"]
    # the reference passes params["dataset_val_max_size"] straight to test_dataset() (evaluate_lidc_uncertainty.py:174):
    # null in the YAML = the whole test split; only when the key were absent would test_dataset's own default of 500 apply
    max_size = params.get("dataset_val_max_size", 500)
    if "synthetic" in name:
        return SyntheticLIDC(size=max_size or 8)
    if "lidc" in name:
        path = expanduservars(params.get("dataset_path", os.environ.get("LIDC_HDF5", "data_lidc.hdf5")))
        return TestLIDC(path, "test", max_size)
    raise ValueError("Unknown dataset")


# ------------------------------------------------------------------------------------------------ model
def build_from_params(params: dict, input_shapes, device) :
    """`_build_model` (ddpm/trainer.py:589-601) key mapping."""
    fce = params.get("feature_cond_encoder", {"type": "none"})
    model = build_model(
        time_steps=params["time_steps"], schedule=params["beta_schedule"],
        schedule_params=params.get("beta_schedule_params", None), cond_encoded_shape=input_shapes[0],
        input_shapes=input_shapes, backbone=params["backbone"], backbone_params=params[params["backbone"]],
        dataset_file=params["dataset_file"], step_T_sample=params.get("evaluation_vote_strategy", None),
        feature_cond_encoder=fce if fce.get("type", "none") != "none" else None).to(device)
    return model.eval()


def load_checkpoint(model, filename: str, key: str = "average_model", allow_pickle: Optional[bool] = None) -> None:
    """ignite ModelCheckpoint files are plain dicts of state_dicts (trainer.py:357-376); LIDC evaluation reads
    `average_model` (evaluate_lidc_uncertainty.py:138-143,157-161).  The file is read with torch's restricted unpickler
    (tensors, containers, numbers).  A checkpoint whose optimizer / engine entries need arbitrary classes is only read with
    the full unpickler — which executes code from the file — when the caller opts in: allow_pickle=True, or
    CCDM_ALLOW_UNSAFE_PICKLE=1 in the environment."""
    import pickle
    LOGGER.info("Loading state from %s...", filename)
    try:
        state = torch.load(filename, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if allow_pickle is None:
            allow_pickle = os.environ.get("CCDM_ALLOW_UNSAFE_PICKLE", "") == "1"
        if not allow_pickle:
            raise RuntimeError(f"{filename} holds objects torch's safe loader rejects ({e}); if you trust the file, pass "
                               "allow_pickle=True or set CCDM_ALLOW_UNSAFE_PICKLE=1 to read it with the full unpickler") from e
        LOGGER.warning("reading %s with the full (unsafe) unpickler", filename)
        state = torch.load(filename, map_location="cpu", weights_only=False)
    sd = state[key] if key in state else state
    model.unet.load_state_dict(sd, strict=True)


def apply_sampler_options(model, params: dict) -> None:
    """Build-owned keys of the params file (absent in the reference's YAML, so an unchanged file runs the defaults):
         rng:  "philox" (default, device RNG) | "torch_cpu" (host generator in the reference's consumption order, parity mode)
         prec: "f16x3" (default) | "f32" (exact-fp32 kernels) | "f16" (OPT-IN single-pass fast mode: operands rounded to fp16, outside
               the 1e-4 parity contract — tools/fast_mode_report.py prints its error; logged as a warning)
         philox_seed, use_graph, substreams, calibrate_mode, on_range_error (layers | f32 | raise), f32_layers, slicing: DenoisingModel
         attributes of the same names."""
    from . import hip
    model.rng = str(params.get("rng", "philox"))
    prec = str(params.get("prec", "f16x3")).lower()
    if prec not in ("f16x3", "f32", "f16"):
        raise ValueError(f"prec: {prec!r} (expected 'f16x3', 'f32' or 'f16')")
    if prec == "f16":
        import logging
        logging.getLogger(__name__).warning("prec: f16 — single-pass fp16 products (~2^-11 per operand): faster, NOT the reference's arithmetic "
                                            "(outside the 1e-4 parity contract; see tools/fast_mode_report.py)")
    model.prec = {"f32": hip.PREC_F32, "f16x3": hip.PREC_F16X3, "f16": hip.PREC_F16}[prec]
    model.philox_seed = int(params.get("philox_seed", 0))
    model.use_graph = bool(params.get("use_graph", True))
    model.substreams = int(params.get("substreams", 0))          # 0 = automatic (DenoisingModel): the execution mode is measured once per geometry
    model.calibrate_mode = bool(params.get("calibrate_mode", True))    # False: the static rule (two streams from 32 x 128x128 pixels) and use_graph as set
    model.on_range_error = str(params.get("on_range_error", "layers"))
    model.f32_layers = set(params.get("f32_layers", []) or [])       # conv layers pinned to fp32 up front (tools/range_report.py --pin)
    model.slicing = str(params.get("slicing", "throughput"))
    model._fine_slices(1)                                         # validates the value


SAMPLING_KEYS = ("temperature", "truncation", "views", "tiles")


def sampling_keywords(params: dict) -> dict:
    """The keywords the params key `sampling: {temperature: ..., truncation: ..., views: [...], tiles: [...]}` (each optional) adds to every sampling
    call and to predict_multiple (DenoisingModel's keywords of those names, which check the values; `views`, a YAML list of names from
    hflip / vflip / hvflip, travels as a tuple, and so does `tiles`, a YAML list of the four integers h, w, sy, sx); {} without the key.
    An unknown key under `sampling:` raises."""
    section = params.get("sampling")
    if section is None:
        return {}
    if not isinstance(section, dict):
        raise ValueError(f"sampling: expected a mapping with keys from {list(SAMPLING_KEYS)}, got {section!r}")
    unknown = [k for k in section if k not in SAMPLING_KEYS]
    if unknown:
        raise ValueError(f"sampling: unknown key(s) {unknown} (expected keys from {list(SAMPLING_KEYS)})")
    return {k: tuple(section[k]) if (k in ("views", "tiles") and isinstance(section[k], list)) else section[k]
            for k in SAMPLING_KEYS if section.get(k) is not None}


def view_features(encoder, image: torch.Tensor, views) -> torch.Tensor:
    """The feature condition of a call with `views` (DenoisingModel's keyword): [V,B,Cf,h,w], view 0 the encoder's features of the
    image, view v >= 1 those of the image mirrored as views[v - 1] says — the encoder runs once per view on the mirrored pixels, its
    output is not flipped after the fact (a ViT's features of a mirrored image are not the mirrored features)."""
    flips = [VIEW_FLIPS[v] for v in views]
    return torch.stack([encoder(image)] + [encoder(torch.flip(image, [d for b, d in ((1, 3), (2, 2)) if f & b])) for f in flips], 0)


def tile_features(encoder, image: torch.Tensor, tiles) -> torch.Tensor:
    """The feature condition of a call with `tiles` = (h, w, sy, sx) (DenoisingModel's keyword): [R,B,Cf,hf,wf], tile r the encoder's
    features of the image cropped to tile r (guidance.tile_origins, r = i * Tx + j) — the encoder runs once per tile on the cropped
    pixels, as the network does."""
    h, w, sy, sx = (int(v) for v in tiles)
    oys, oxs = tile_origins(int(image.shape[2]), int(image.shape[3]), h, w, sy, sx)
    return torch.stack([encoder(image[:, :, oy:oy + h, ox:ox + w]) for oy in oys for ox in oxs], 0)


def _as_list(v) -> List[int]:
    return [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)]


# ------------------------------------------------------------------------------------------------ evaluation
def soft_label_bins(value) -> int:
    """`soft_label_bins`: the level bins of the reliability curve, a whole number from 1 (10 when absent)."""
    if int(value) < 1:
        raise ValueError(f"soft_label_bins: {value!r} (expected a whole number, at least 1)")
    return int(value)


def soft_label_thresholds(values) -> List[float]:
    """`soft_label_thresholds`: the shares at which the soft Dice cuts both frequencies, each in (0, 1] ([0.1, ..., 0.9] when absent)."""
    thresholds = [float(t) for t in values]
    if not thresholds or any(not 0.0 < t <= 1.0 for t in thresholds):
        raise ValueError(f"soft_label_thresholds: {values!r} (expected values in (0, 1])")
    return thresholds


def surface_distance_quantile(value) -> Tuple[int, int]:
    """`surface_distance_percentile` -> the quantile (num, den), the value read as the decimal it is written as (95 -> (19, 20))."""
    quantile = Fraction(str(value)) / 100
    if not 0 < quantile <= 1:
        raise ValueError(f"surface_distance_percentile: {value!r} (expected a value in (0, 100])")
    return quantile.numerator, quantile.denominator


def lesion_overlaps(values) -> List[Tuple[int, int]]:
    """`lesion_overlaps` -> [(num, den), ...]: the shares of a lesion the other mask has to cover, each in [0, 1] and read as the decimal it is
    written as (0.5 -> (1, 2); 0: any overlap)."""
    fractions = [Fraction(str(v)) for v in (values if isinstance(values, (list, tuple)) else [values])]
    if not fractions or any(not 0 <= f <= 1 for f in fractions):
        raise ValueError(f"lesion_overlaps: {values!r} (expected values in [0, 1])")
    return [(f.numerator, f.denominator) for f in fractions]


def lesion_connectivity(section: dict) -> int:
    """`lesion_connectivity` of the `evaluation` section: 4 or 8 (8 when absent)."""
    value = section.get("lesion_connectivity", 8)
    if isinstance(value, bool) or not isinstance(value, int) or value not in (4, 8):
        raise ValueError(f"lesion_connectivity: {value!r} (expected 4 or 8)")
    return value


def lesion_match_thresholds(values) -> List[Tuple[int, int]]:
    """`lesion_match_ious` -> [(num, den), ...], each value read as the decimal it is written as (0.5 -> (1, 2), 0.75 -> (3, 4)).
    A pair is matched when its IoU EXCEEDS the value; only above 1/2 is the matching unique, so the values lie in [0.5, 1)."""
    values = list(values) if isinstance(values, (list, tuple)) else [values]
    try:
        fractions = [Fraction(str(v)) for v in values]
    except (ValueError, ZeroDivisionError):
        fractions = []
    if not 1 <= len(fractions) <= 8 or any(isinstance(v, bool) for v in values) or any(not Fraction(1, 2) <= f < 1 for f in fractions) \
            or any(f.denominator > 65536 for f in fractions):
        raise ValueError(f"lesion_match_ious: {values!r} (expected 1 to 8 decimals in [0.5, 1) with denominators up to 65536)")
    return [(f.numerator, f.denominator) for f in fractions]


def lesion_min_size(value) -> int:
    """`lesion_min_size`: a whole number of pixels, at least 1."""
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"lesion_min_size: {value!r} (expected a whole number of pixels, at least 1)")
    return value


def detection_min_frequency(value):
    """`detection_min_frequency`: the share of the samples a pixel needs to belong to a candidate, a decimal in [0, 1] (0.1 when absent);
    with s samples n_min = max(1, ceil(value * s)), the value read as the decimal it is written as."""
    try:
        ok = not isinstance(value, bool) and isinstance(value, (int, float, str)) and 0 <= Fraction(str(value)) <= 1
    except (ValueError, ZeroDivisionError):
        ok = False
    if not ok:
        raise ValueError(f"detection_min_frequency: {value!r} (expected a share of the samples in [0, 1])")
    return value


def detection_rater_agreement(value, raters: int) -> int:
    """`detection_rater_agreement` -> m_min, the raters a pixel needs to belong to a reference lesion: `majority` (the default) is
    raters // 2 + 1, otherwise a whole number in 1..raters."""
    if value == "majority":
        return raters // 2 + 1
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= raters:
        raise ValueError(f"detection_rater_agreement: {value!r} (expected 'majority' or a whole number in [1, {raters}])")
    return value


def detection_score(value) -> str:
    """`detection_score`: the confidence of a candidate, `support` (the samples that draw it; the default) or `peak`."""
    if value not in M.DETECTION_SCORES:
        raise ValueError(f"detection_score: {value!r} (expected one of {list(M.DETECTION_SCORES)})")
    return value


def detection_fp_rates(values) -> List[float]:
    """`detection_fp_rates`: the false positives per image at which the sensitivity is read (1/8 ... 8 when absent), none negative."""
    values = list(values) if isinstance(values, (list, tuple)) else [values]
    if not values or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf") for v in values):
        raise ValueError(f"detection_fp_rates: {values!r} (expected at least one number of false positives per image, none negative)")
    return values


def detection_max_candidates(value) -> int:
    """`detection_max_candidates`: the candidates and reference lesions kept per image and class, 1 to 1024 (64 when absent)."""
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= M.FINDINGS_MAX_CANDIDATES:
        raise ValueError(f"detection_max_candidates: {value!r} (expected a whole number in [1, {M.FINDINGS_MAX_CANDIDATES}])")
    return value


def mode_count(value) -> int:
    """`mode_count`: how many modes the mode summary looks for, 1 to 16 (metrics.MODES_MAX_MODES)."""
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= M.MODES_MAX_MODES:
        raise ValueError(f"mode_count: {value!r} (expected a whole number in [1, {M.MODES_MAX_MODES}])")
    return value


def mode_max_swaps(value) -> int:
    """`mode_max_swaps`: the most swaps the clustering applies after its greedy start, at least 0."""
    if isinstance(value, bool) or not isinstance(value, int) or value < 0:
        raise ValueError(f"mode_max_swaps: {value!r} (expected a whole number, at least 0)")
    return value


def mode_summary_scores(pred_idx: torch.Tensor, lab_idx: torch.Tensor, num_classes: int, count: int, max_swaps: int) -> Dict[str, np.ndarray]:
    """Per image of pred_idx [B,S,H,W] against the raters lab_idx [B,L,H,W], float64 [B] each: `found` (the modes metrics.sample_modes
    finds among `count`), `largest_share`, `ged_summary` (the GED between the raters and the medoids weighted by their shares,
    2 sum_m w_m mean_l d(m,l) - sum_{m,m'} w_m w_m' d(m,m') - mean_{l,l'} d(l,l'), d = metrics.batched_distance) and `coverage` (the
    mean over the raters of the distance to the nearest medoid); `converged` as the clustering reports it."""
    modes = M.sample_modes(pred_idx, num_classes, count, max_swaps=max_swaps, maps=())
    used = (modes["medoid"] >= 0).cpu().numpy()                                  # [B,M]
    w = modes["size"].cpu().numpy().astype(np.float64) / float(pred_idx.shape[1])     # (size / S in float64, as a mean over samples weighs)
    to_raters = M.batched_distance(modes["mode_map"], lab_idx, num_classes)          # [B,M,L]; an unused mode weighs 0
    among = M.batched_distance(modes["mode_map"], modes["mode_map"], num_classes)    # [B,M,M]
    raters = M.batched_distance(lab_idx, lab_idx, num_classes)                       # [B,L,L]
    ged = 2.0 * (w * to_raters.mean(axis=2)).sum(axis=1) - (w[:, :, None] * w[:, None, :] * among).sum(axis=(1, 2)) - raters.mean(axis=(1, 2))
    nearest = np.where(used[:, :, None], to_raters, np.inf).min(axis=1)              # [B,L]
    return {"found": used.sum(axis=1).astype(np.float64), "largest_share": w[:, 0], "ged_summary": ged, "coverage": nearest.mean(axis=1),
            "converged": modes["converged"].cpu().numpy().astype(np.float64)}


def consensus_metric(value) -> str:
    """`consensus_metric`: the score the consensus map is chosen for, `iou` or `dice` (metrics.CONSENSUS_METRICS)."""
    if not isinstance(value, str) or value not in M.CONSENSUS_METRICS:
        raise ValueError(f"consensus_metric: {value!r} (expected one of {M.CONSENSUS_METRICS})")
    return value


def _rater_scores(label: torch.Tensor, lab_idx: torch.Tensor, num_classes: int) -> Tuple[np.ndarray, np.ndarray]:
    """One map per image, label [B,H,W], against the raters lab_idx [B,L,H,W] -> (IoU, Dice), float64 [B] each: the mean over the raters
    of the mean over the foreground classes, an empty class on both sides counting 1 (the reference's 0/0)."""
    counts = M.pairwise_class_counts(label[:, None], lab_idx, num_classes)[:, 0].astype(np.int64)      # [B,L,K,2]: (intersection, union)
    inter, uni = counts[..., 1:, 0], counts[..., 1:, 1]
    both = uni + inter                                                                                  # n_a + n_b
    iou = np.where(uni > 0, inter / np.maximum(uni, 1), 1.0)
    dice = np.where(both > 0, 2 * inter / np.maximum(both, 1), 1.0)
    return iou.mean(axis=-1).mean(axis=-1), dice.mean(axis=-1).mean(axis=-1)


def consensus_scores(pred_idx: torch.Tensor, lab_idx: torch.Tensor, num_classes: int, metric: str) -> Dict[str, np.ndarray]:
    """Per image of pred_idx [B,S,H,W] against the raters lab_idx [B,L,H,W], float64 [B] each: IoU and Dice of the consensus map
    (metrics.sample_consensus for `metric`) and of the majority-vote map (every class thresholded at S // 2 + 1) against the raters,
    the expected `metric` the samples themselves predict for either (the mean over the classes), and the chosen threshold over S."""
    S = int(pred_idx.shape[1])
    cons = M.sample_consensus(pred_idx, num_classes, metric=metric, maps=("label",))
    major = M.threshold_maps(cons["frequency"], torch.full_like(cons["thresholds"], S // 2 + 1), S, metric, maps=("label",))["label"]
    iou_c, dice_c = _rater_scores(cons["label"], lab_idx, num_classes)
    iou_m, dice_m = _rater_scores(major, lab_idx, num_classes)
    return {"iou_consensus": iou_c, "dice_consensus": dice_c, "iou_majority": iou_m, "dice_majority": dice_m,
            "expected": cons["expected"].cpu().numpy().mean(axis=1), "expected_majority": cons["expected_majority"].cpu().numpy().mean(axis=1),
            "threshold_share": cons["threshold"].cpu().numpy().astype(np.float64).mean(axis=1) / float(S)}


@dataclass(frozen=True)
class LidcScore:
    """One optional score of eval_lidc_uncertainty, on with `key: yes` in the `evaluation` section: the result gains `key`, one dict per entry
    of `evaluations`, also written as lidc_<key>.json under `output_path`."""
    key: str
    configure: Callable      # (section, ctx) -> settings: every check of the option's keys, before the first batch; ctx: raters, num_classes
    collect: Callable        # (settings, pred_idx[:, :s], lab_idx, s) -> part: the metrics call of one batch and entry
    finish: Callable         # (settings, parts, s, ctx) -> dict: the scores of an entry from the parts of every batch
    log: Callable            # (s, r): one line on an entry's scores


def _soft_label_settings(section: dict, ctx) -> dict:
    scoring = {"bins": soft_label_bins(section.get("soft_label_bins", 10))}
    if section.get("soft_label_thresholds") is not None:
        scoring["thresholds"] = soft_label_thresholds(section["soft_label_thresholds"])
    return {"num_classes": ctx.num_classes, "scoring": scoring}


def _detection_settings(section: dict, ctx) -> dict:
    connectivity = lesion_connectivity(section)
    min_frequency = detection_min_frequency(section.get("detection_min_frequency", 0.1))
    m_min = detection_rater_agreement(section.get("detection_rater_agreement", "majority"), ctx.raters)
    scoring = {"score": detection_score(section.get("detection_score", "support")),
               "fp_rates": detection_fp_rates(section.get("detection_fp_rates", list(M.DETECTION_FP_RATES)))}
    findings = {"num_classes": ctx.num_classes, "m_min": m_min, "connectivity": connectivity,
                "max_candidates": detection_max_candidates(section.get("detection_max_candidates", 64))}
    return {"min_frequency": min_frequency, "findings": findings, "scoring": scoring}


def _mean_per_image(parts: Sequence[Dict[str, np.ndarray]], s: int, **settings) -> Dict[str, object]:
    """The per-image scores of every batch (float64 [B] each) as their means over the images, behind `samples`, `images` and the settings."""
    per_image = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return {"samples": int(s), "images": int(next(iter(per_image.values())).size), **settings, **{k: float(v.mean()) for k, v in per_image.items()}}


def _mode_scores(parts: Sequence[Dict[str, np.ndarray]], s: int, settings: dict) -> Dict[str, object]:
    scores = _mean_per_image(parts, s, mode_count=settings["count"], max_swaps=settings["max_swaps"])
    return {("modes_found" if k == "found" else k): v for k, v in scores.items()}


# in the order their keys are checked and their results are added; label_bound, once per batch on the images, stands beside them
LIDC_SCORES = (
    LidcScore("soft_labels", _soft_label_settings,
              collect=lambda st, pred_idx, lab_idx, s: M.vote_joint_counts(pred_idx, lab_idx, st["num_classes"]),
              finish=lambda st, parts, s, ctx: M.soft_label_scores_from_counts(np.concatenate([j for j, _ in parts]),
                                                                                np.concatenate([m for _, m in parts]), **st["scoring"]),
              log=lambda s, r: LOGGER.info("soft labels (%d): ECE %.4g  Brier %.4g  Dice %.4g  NCC %s", s, r["ece_soft"], r["brier_soft"],
                                           r["dice_soft"], r["ncc"])),
    LidcScore("surface_distances",
              configure=lambda section, ctx: {"num_classes": ctx.num_classes,
                                              "q": surface_distance_quantile(section.get("surface_distance_percentile", 95))},
              collect=lambda st, pred_idx, lab_idx, s: M.surface_distance_stats(pred_idx, lab_idx, **st),
              finish=lambda st, parts, s, ctx: M.surface_scores_from_stats(M.concat_surface_stats(parts)),
              log=lambda s, r: LOGGER.info("surface distances (%d): HD%g %s  ASSD %s  HD %s  (%d of %d cells defined)", s, r["percentile"],
                                           r["hd_percentile"], r["assd"], r["hd"], r["cells_defined"], r["cells_defined"] + r["cells_undefined"])),
    LidcScore("lesions",
              configure=lambda section, ctx: {"num_classes": ctx.num_classes, "connectivity": lesion_connectivity(section),
                                              "overlaps": lesion_overlaps(section.get("lesion_overlaps", [0, 0.5]))},
              collect=lambda st, pred_idx, lab_idx, s: M.lesion_stats(pred_idx, lab_idx, **st),
              finish=lambda st, parts, s, ctx: M.lesion_scores_from_stats(M.concat_lesion_stats(parts)),
              log=lambda s, r: LOGGER.info("lesions (%d): recall %s  precision %s  F1 %s at overlaps %s  count error %.4g  (%d of %d cells without "
                                           "a lesion)", s, r["recall"], r["precision"], r["f1"], r["thresholds"], r["count_error"],
                                           r["cells_both_empty"], r["cells"])),
    LidcScore("lesion_matching",
              configure=lambda section, ctx: {"num_classes": ctx.num_classes, "connectivity": lesion_connectivity(section),
                                              "thresholds": lesion_match_thresholds(section.get("lesion_match_ious", [0.5, 0.75])),
                                              "min_size": lesion_min_size(section.get("lesion_min_size", 1))},
              collect=lambda st, pred_idx, lab_idx, s: M.lesion_match_stats(pred_idx, lab_idx, **st),
              finish=lambda st, parts, s, ctx: M.lesion_match_scores_from_stats(M.concat_lesion_match_stats(parts)),
              log=lambda s, r: LOGGER.info("lesion matching (%d): PQ %s  SQ %s  RQ %s at IoU > %s  pooled PQ %s  (%d of %d cells without a lesion)",
                                           s, r["pq"], r["sq"], r["rq"], r["ious"], r["pq_pooled"], r["cells_both_empty"], r["cells"])),
    LidcScore("detection", _detection_settings,
              collect=lambda st, pred_idx, lab_idx, s: M.sample_findings(pred_idx, lab_idx, n_min=max(1, M._ceil_fraction(st["min_frequency"], s)),
                                                                         **st["findings"]),
              finish=lambda st, parts, s, ctx: M.detection_scores_from_findings(M.concat_findings(parts), **st["scoring"]),
              log=lambda s, r: LOGGER.info("detection (%d): CPM %s  AP %s by %s, candidates from %d of %d samples  (%d candidates, %d reference "
                                           "lesions)", s, r["cpm"], r["average_precision"], r["score"], r["n_min"], s,
                                           sum(c["candidates"] for c in r["per_class"]), sum(c["reference_lesions"] for c in r["per_class"]))),
    LidcScore("modes",
              configure=lambda section, ctx: {"num_classes": ctx.num_classes, "count": mode_count(section.get("mode_count", 4)),
                                              "max_swaps": mode_max_swaps(section.get("mode_max_swaps", 64))},
              collect=lambda st, pred_idx, lab_idx, s: mode_summary_scores(pred_idx, lab_idx, **st),
              finish=lambda st, parts, s, ctx: _mode_scores(parts, s, st),
              log=lambda s, r: LOGGER.info("modes (%d): %.3g of %d found  largest share %.3g  GED of the summary %.4g  coverage %.4g", s,
                                           r["modes_found"], r["mode_count"], r["largest_share"], r["ged_summary"], r["coverage"])),
    LidcScore("consensus",
              configure=lambda section, ctx: {"num_classes": ctx.num_classes, "metric": consensus_metric(section.get("consensus_metric", "iou"))},
              collect=lambda st, pred_idx, lab_idx, s: consensus_scores(pred_idx, lab_idx, **st),
              finish=lambda st, parts, s, ctx: _mean_per_image(parts, s, metric=st["metric"]),
              log=lambda s, r: LOGGER.info("consensus (%d, %s): IoU %.4g  Dice %.4g  (majority vote: %.4g, %.4g)  expected %.4g (%.4g)  threshold "
                                           "%.3g of the samples", s, r["metric"], r["iou_consensus"], r["dice_consensus"], r["iou_majority"],
                                           r["dice_majority"], r["expected"], r["expected_majority"], r["threshold_share"])),
)


def _write_result(params: dict, rank: int, key: str, result) -> None:
    """lidc_<key>.json under `output_path`, by rank 0, when the path is set."""
    if params.get("output_path") and rank == 0:
        import json
        out_dir = expanduservars(params["output_path"])
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"lidc_{key}.json"), "w") as f:
            json.dump(result, f, indent=1)


@torch.no_grad()
def eval_lidc_uncertainty(params: dict, dataset=None, device=None, init_t: Optional[int] = None, synthetic_weights_seed: Optional[int] = None,
                          model=None) -> Dict[str, object]:
    """`eval_lidc_uncertainty` + `Tester.test_step` of the reference (evaluate_lidc_uncertainty.py:89-136,164-216).

    Launched under torchrun (WORLD_SIZE > 1, BASELINE config C3) every rank walks the same batches and samples its contiguous
    shard of the B_img*S flattened batch (distributed.sample_sharded: no collective inside the T loop, one gather of the
    predictions per batch); the metrics are then computed identically on every rank.
    `model`: a ready DenoisingModel-like callable (tests inject fixed predictions); default: built from `params`.
    The params key `sampling: {temperature: ..., truncation: ..., views: [...], tiles: [...]}` (sampling_keywords; each optional) is handed to every sampling call
    and echoed as "sampling" in the result; without the key nothing changes.

    Build-owned keys of the `evaluation` section (absent: the returned dict and everything else is as without them):
         soft_labels: yes   the result gains "soft_labels": one dict per entry of `evaluations` with the scores of the first s
                            samples' frequencies against the raters' soft labels (metrics.soft_label_scores_from_counts: calibration,
                            Brier, cross-entropy, soft Dice, NCC; counts from one ccdm_lidcscore launch per batch and entry, kept per
                            image and scored after the last batch); with `output_path` set, also written as lidc_soft_labels.json
         soft_label_bins (10), soft_label_thresholds ([0.1, ..., 0.9])
         surface_distances: yes   the result gains "surface_distances": one dict per entry of `evaluations` with HD95, ASSD and
                            the Hausdorff distance of the first s samples against the raters (metrics.surface_scores_from_stats; the
                            per-cell integers from one ccdm_surfdist call per batch and entry, kept per image and scored after the
                            last batch); with `output_path` set, also written as lidc_surface_distances.json
         surface_distance_percentile (95): the percentile of HD95, read as the decimal it is written as
         lesions: yes       the result gains "lesions": one dict per entry of `evaluations` with lesion-wise recall, precision, F1
                            and the agreement on the number of lesions of the first s samples against the raters
                            (metrics.lesion_scores_from_stats; the per-cell integers from one ccdm_lesions call per batch and entry,
                            kept per image and scored after the last batch); with `output_path` set, also written as
                            lidc_lesions.json
         lesion_connectivity (8): 4 or 8;  lesion_overlaps ([0, 0.5]): the shares of a lesion the other mask has to cover for a
                            hit, each read as the decimal it is written as (0: any overlap)
         lesion_matching: yes   the result gains "lesion_matching": one dict per entry of `evaluations` with panoptic, segmentation
                            and recognition quality of the first s samples' lesions paired one to one with the raters' by IoU
                            (metrics.lesion_match_scores_from_stats; the per-cell integers from one ccdm_lesions and one
                            ccdm_lesion_match call per batch and entry, kept per image and scored after the last batch); with
                            `output_path` set, also written as lidc_lesion_matching.json
         lesion_match_ious ([0.5, 0.75]): the IoUs a pair has to exceed, in [0.5, 1), each read as the decimal it is written as;
                            lesion_min_size (1): lesions of fewer pixels are dropped; lesion_connectivity as above
         detection: yes     the result gains "detection": one dict per entry of `evaluations` with FROC, the sensitivity at fixed
                            false positives per image (and their mean, the LUNA16 CPM) and the average precision of the first s
                            samples read as one list of lesion candidates per image with a confidence each, against the lesions the
                            raters agree on (metrics.detection_scores_from_findings; the records from one ccdm_findings call per batch
                            and entry, kept per image and scored after the last batch); with `output_path` set, also written as
                            lidc_detection.json
         detection_min_frequency (0.1): the share of the samples a pixel needs to belong to a candidate;
                            detection_rater_agreement (majority): the raters a pixel needs to belong to a reference lesion, `majority`
                            or a whole number; detection_score (support): support or peak; detection_fp_rates ([1/8 ... 8]);
                            detection_max_candidates (64); lesion_connectivity as above
         modes: yes         the result gains "modes": one dict per entry of `evaluations` with the mode summary of the first s
                            samples (metrics.sample_modes: k-medoids under the GED's own distance, on the device): the mean number
                            of modes found, the mean share of the largest, `ged_summary` (the GED between the raters and the medoids
                            weighted by their shares) and `coverage` (the mean over raters of the distance to the nearest medoid),
                            each a mean over the images (mode_summary_scores); with `output_path` set, also written as
                            lidc_modes.json
         mode_count (4): the modes looked for, 1 to 16;  mode_max_swaps (64): the most swaps of the clustering
         consensus: yes     the result gains "consensus": one dict per entry of `evaluations` for the single map the first s samples
                            give (metrics.sample_consensus: per class the thresholded sample frequency with the largest expected
                            score under the samples, on the device): the IoU and Dice of that map and of the majority-vote map
                            (threshold s // 2 + 1) against the raters — the mean over the images of the mean over the raters of the
                            mean over the foreground classes, 0/0 = 1 —, the expected score the samples predicted for either and the
                            mean chosen threshold over s (consensus_scores); with `output_path` set, also written as
                            lidc_consensus.json
         consensus_metric (iou): iou or dice, the score the map is chosen for
         label_bound: yes   the result gains "label_bound": the variational bound on -log p(rater's map | image) in nats
                            (DenoisingModel.label_bound, one call per batch on the batch's images and all raters' maps): per rater the
                            mean bound and bits per pixel over the images, their mean over the raters — an upper bound on the
                            cross-entropy between the raters' distribution and the model's — and the per-timestep curve averaged over
                            images and raters, with `images`, `timesteps`, `draws`, `complete`; with `output_path` set, also written as
                            lidc_label_bound.json.  Under WORLD_SIZE > 1 every rank computes the same numbers (the bound is not sharded)
         label_bound_timesteps (all): a list of timesteps (a partial sum) or a number of strata;  label_bound_draws (1)"""
    from . import distributed as D
    rank, local_rank, world = D.init_from_env()
    if device is None:
        device = torch.device("cuda", local_rank) if torch.cuda.is_available() else torch.device("cuda")
    device = torch.device(device)
    dataset = dataset if dataset is not None else make_dataset(params)
    LOGGER.info("%d images in test dataset '%s'", len(dataset), params["dataset_file"])
    loader = torch.utils.data.DataLoader(dataset, batch_size=params["batch_size"], shuffle=False, num_workers=params.get("mp_loaders", 0))
    image0, labels0, _ = dataset[0]
    input_shapes = [tuple(image0.shape), tuple(labels0.shape[1:])]
    num_classes = input_shapes[1][0]
    if model is None:
        model = build_from_params(params, input_shapes, device)
        if params.get("load_from"):
            load_checkpoint(model, expanduservars(params["load_from"]))
        elif synthetic_weights_seed is not None:
            from .unet_spec import make_synthetic_state_dict
            model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, synthetic_weights_seed).items()})
        apply_sampler_options(model, params)
    evaluations = _as_list(params["evaluations"])
    S = max(evaluations)
    geds, div_s, div_e, hm = (np.zeros(len(evaluations)) for _ in range(4))
    conf = torch.zeros((num_classes, num_classes), dtype=torch.int64)
    nonzero_total, n_img = 0, 0
    majority = getattr(model, "step_T_sample", None) in (None, "majority")
    section = params.get("evaluation") or {}
    sampling = sampling_keywords(params)
    ctx = SimpleNamespace(raters=int(labels0.shape[0]), num_classes=num_classes, evaluations=evaluations)
    # per option that is on: (option, settings, per entry the parts of every batch)
    scores = [(option, option.configure(section, ctx), [[] for _ in evaluations]) for option in LIDC_SCORES if section.get(option.key, False)]
    bound = [] if section.get("label_bound", False) else None                                    # the result of every batch
    if bound is not None:
        bound_ts = section.get("label_bound_timesteps")
        bound_ts = [int(v) for v in bound_ts] if isinstance(bound_ts, (list, tuple)) else (None if bound_ts is None else int(bound_ts))
        bound_draws = int(section.get("label_bound_draws", 1))
    for image, labels, _ in loader:                                              # Tester.test_step, :89-136
        if bound is not None:
            got = model.label_bound(labels.to(device).argmax(dim=2), image.to(device), timesteps=bound_ts, draws=bound_draws)
            bound.append({k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()})
        image = image.to(device).repeat_interleave(S, dim=0)
        # x_T: uniform one-hot from the CPU generator, full batch on every rank (same seed => same draw)
        x = OneHotCategoricalBCHW(logits=torch.zeros(labels[:, 0].repeat_interleave(S, dim=0).shape)).sample().to(device)
        t = None if init_t is None else torch.as_tensor(init_t)
        if world > 1:
            # one-hot ("majority") predictions travel as uint8 class maps, probabilities as fp32
            prediction = D.sample_sharded(model, x, image, t=t, gather="index" if majority else True, **sampling)
        else:
            prediction = model(x, image, **({} if t is None else {"t": t}), **sampling)["diffusion_out"]
        prediction = prediction.reshape(labels.shape[0], -1, *labels.shape[2:])
        lab_idx = labels.to(device).argmax(dim=2)
        pred_idx = prediction.argmax(dim=2)
        for i, s in enumerate(evaluations):
            ged, sim_e, sim_s = M.calc_batched_generalised_energy_distance(lab_idx, pred_idx[:, :s], num_classes)
            geds[i] += ged.sum(); div_e[i] += sim_e.sum(); div_s[i] += sim_s.sum()
            lcm = int(np.lcm(s, lab_idx.shape[1]))
            hm[i] += np.sum(M.batched_hungarian_matching(lab_idx.repeat_interleave(lcm // lab_idx.shape[1], dim=1),
                                                          pred_idx[:, :s].repeat_interleave(lcm // s, dim=1), num_classes))
            for option, settings, parts in scores:
                parts[i].append(option.collect(settings, pred_idx[:, :s], lab_idx, s))
        # log-mean vote exactly as the reference takes it (:125): log(0) = -inf stays -inf (one-hot "majority" predictions:
        # a class any sample rejects is out; where every class is rejected by someone argmax falls to class 0)
        mean_pred = torch.log(prediction).mean(dim=1).argmax(dim=1)
        nz = torch.count_nonzero(lab_idx, dim=(2, 3)) > 0
        nonzero_total += int(nz.sum())
        for b in range(lab_idx.shape[0]):
            for a in range(lab_idx.shape[1]):
                if nz[b, a]:                                                     # y = labels[nonzero], y_pred repeated per annotation (:127-136)
                    idx = (lab_idx[b, a].reshape(-1) * num_classes + mean_pred[b].reshape(-1)).cpu()
                    conf += torch.bincount(idx, minlength=num_classes ** 2).reshape(num_classes, num_classes)
        n_img += lab_idx.shape[0]
    # ignite.metrics IoU / mIoU / DiceCoefficient on the accumulated confusion matrix (rows = y, columns = y_pred)
    cm = conf.double()
    iou = cm.diag() / (cm.sum(dim=1) + cm.sum(dim=0) - cm.diag() + 1e-15)
    dice = 2.0 * cm.diag() / (cm.sum(dim=1) + cm.sum(dim=0) + 1e-15)
    res = {"evaluations": evaluations, "GED": (geds / n_img).tolist(), "diversity_samples": (div_s / n_img).tolist(),
           "diversity_experts": float(div_e[0] / n_img), "HM_IoU": (hm / n_img).tolist(), "IoU": iou.tolist(), "mIoU": float(iou.mean()),
           "Dice": dice.tolist(), "nonzero": nonzero_total / (n_img * 4), "images": n_img, "world_size": world}
    if params.get("sampling") is not None:
        res["sampling"] = dict(sampling)
    for i, s in enumerate(evaluations):
        LOGGER.info("GED (%d): %.4g  diversity samples: %.4g  HM IoU: %.4g", s, res["GED"][i], res["diversity_samples"][i], res["HM_IoU"][i])
    for option, settings, parts in scores:
        res[option.key] = [option.finish(settings, p, s, ctx) for s, p in zip(evaluations, parts)]
        for s, r in zip(evaluations, res[option.key]):
            option.log(s, r)
        _write_result(params, rank, option.key, res[option.key])
    if bound is not None:
        res["label_bound"] = r = label_bound_summary(bound, bound_draws)
        LOGGER.info("label bound: %.6g nats per map, %.4g bits per pixel over %d images (%d timesteps, %d draw(s)%s)", r["bound"],
                    r["bits_per_pixel"], r["images"], len(r["timestep_curve"]), r["draws"], "" if r["complete"] else ", partial sum")
        _write_result(params, rank, "label_bound", r)
    return res


def label_bound_summary(parts: Sequence[Dict[str, object]], draws: int) -> Dict[str, object]:
    """What eval_lidc_uncertainty reports of DenoisingModel.label_bound's results over the batches (`parts`: numpy arrays, [B,L] and
    [B,L,M]): per rater the mean over the images of the bound (nats) and of the bits per pixel, their mean over the raters (the
    cross-entropy bound of the rater distribution), and the per-timestep curve — the mean term per position of the estimator, with the
    timestep where every label used the same one (None under stratified draws)."""
    bound = np.concatenate([p["bound"] for p in parts])
    bpp = np.concatenate([p["bits_per_pixel"] for p in parts])
    terms = np.concatenate([p["terms"] for p in parts])
    ts = np.concatenate([p["timesteps"] for p in parts])
    same = [bool((ts[..., m] == ts[0, 0, m]).all()) for m in range(ts.shape[-1])]
    return {"bound_per_rater": bound.mean(axis=0).tolist(), "bits_per_pixel_per_rater": bpp.mean(axis=0).tolist(),
            "bound": float(bound.mean()), "bits_per_pixel": float(bpp.mean()), "prior": float(np.concatenate([p["prior"] for p in parts]).mean()),
            "timestep_curve": terms.mean(axis=(0, 1)).tolist(),
            "timesteps": [int(ts[0, 0, m]) if same[m] else None for m in range(ts.shape[-1])],
            "images": int(bound.shape[0]), "raters": int(bound.shape[1]), "draws": int(draws), "complete": bool(all(p["complete"] for p in parts))}


def eval_lidc_sampling_speed(params: dict, timesteps: Sequence[int] = (250, 200, 150, 100, 50, 25, 10), **kw) -> Dict[int, dict]:
    """Strided-step sweep: the sampler is called with t = 10000 + K (evaluate_lidc_sampling_speed.py:195-199,:103)."""
    out = {}
    for k in timesteps:
        if k > params["time_steps"]:
            continue
        LOGGER.info("Evaluate model with sampling step %d...", k)
        out[k] = eval_lidc_uncertainty(params, init_t=10000 + k, **kw)
    return out


VOTE_STRATEGIES = ("confidence", "majority")


def vote_settings(params: dict):
    """(evaluations, evaluation_vote_strategy) as the reference's Evaluator reads them (eval_cdm.py:111-114: the `evaluation`
    section, defaults 1 and "confidence"), falling back to the top-level keys of the LIDC-style params files.  A list of
    evaluations (the LIDC evaluator's sweep) means its largest entry."""
    section = params.get("evaluation") or {}
    evaluations = section.get("evaluations", params.get("evaluations", 1))
    strategy = section.get("evaluation_vote_strategy", params.get("evaluation_vote_strategy", "confidence"))
    n = max(_as_list(evaluations))
    if n < 1:
        raise ValueError(f"evaluations: {evaluations!r} (expected >= 1)")
    if strategy not in VOTE_STRATEGIES:
        raise ValueError(f"evaluation_vote_strategy: {strategy!r} is not in {list(VOTE_STRATEGIES)}")
    return n, strategy


@torch.no_grad()
def predict_multiple(model, image: torch.Tensor, params: dict, feature_condition: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The prediction of the reference Evaluator's inference step (eval_cdm.py:206-212): one sample from a uniform one-hot x_T
    (`predict_single`, :160-165) when `evaluations` is 1, else the mean of `evaluations` samples voted with
    `evaluation_vote_strategy` (`predict_multiple`, :176-193) — computed on the device by DenoisingModel.predict_multiple.
    "confidence" gives the reference's `prediction_onehot_total` bit for bit; "majority" (NotImplementedError in the reference)
    gives the class frequencies.  The params key `sampling:` (sampling_keywords) is handed to either call.  Returns [B,K,H,W]."""
    n, strategy = vote_settings(params)
    sampling = sampling_keywords(params)
    if n == 1:
        K = model.diffusion.num_classes
        x = OneHotCategoricalBCHW(logits=torch.zeros((image.shape[0], K, *image.shape[2:]), device=image.device)).sample()
        return model(x, image, feature_condition, **sampling)["diffusion_out"]
    return model.predict_multiple(image, feature_condition, num_evaluations=n, voting=strategy, maps=("mean",), **sampling)["mean"]
