"""Cityscapes-type segmentation evaluation: mIoU of a sampled prediction against the labels, at the dataloader resolution or
against the original full-resolution labels — the reference's `evaluation/eval_cdm.py` (`Evaluator.infer_step`, `update_cm`,
`get_miou_and_ious`, `run_inference`), which is broken on its main branch (it calls the undefined
`predict_condition`, reads the absent key `cdm_only`, and scores raw Cityscapes label ids).

    SegmentationConfusion(num_classes, device)   ignite's ConfusionMatrix / IoU / mIoU and the reference's "soft" matrix, built by
                                                 one HIP kernel (ccdm_seg_confusion) that upsamples, classifies and counts without
                                                 a full-resolution probability tensor
    eval_segmentation(params, ...)               the evaluation loop (no ignite), built like evaluation.eval_lidc_uncertainty
    CityscapesVal(root, ...)                     the validation split, re-stated with PIL and numpy (no torchvision)
    SyntheticCityscapes(...)                     a deterministic stand-in so the entry point runs without the data
"""
from __future__ import annotations

import glob
import logging
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip

LOGGER = logging.getLogger(__name__)

# ------------------------------------------------------------------------------------------------ label definition
# (name, label id, train id) of the public Cityscapes label definition (cityscapesScripts, helpers/labels.py); train id 255 =
# not evaluated.  tests/golden/cityscapes_train_ids.json pins it.
CITYSCAPES_LABELS: Tuple[Tuple[str, int, int], ...] = (
    ("unlabeled", 0, 255), ("ego vehicle", 1, 255), ("rectification border", 2, 255), ("out of roi", 3, 255), ("static", 4, 255),
    ("dynamic", 5, 255), ("ground", 6, 255), ("road", 7, 0), ("sidewalk", 8, 1), ("parking", 9, 255), ("rail track", 10, 255),
    ("building", 11, 2), ("wall", 12, 3), ("fence", 13, 4), ("guard rail", 14, 255), ("bridge", 15, 255), ("tunnel", 16, 255),
    ("pole", 17, 5), ("polegroup", 18, 255), ("traffic light", 19, 6), ("traffic sign", 20, 7), ("vegetation", 21, 8),
    ("terrain", 22, 9), ("sky", 23, 10), ("person", 24, 11), ("rider", 25, 12), ("car", 26, 13), ("truck", 27, 14),
    ("bus", 28, 15), ("caravan", 29, 255), ("trailer", 30, 255), ("train", 31, 16), ("motorcycle", 32, 17), ("bicycle", 33, 18),
    ("license plate", -1, 255),
)
NUM_CLASSES = 20            # 19 evaluated train ids + the ignore class
IGNORE_CLASS = 19           # the model's ignore channel / label value (datasets/cityscapes.py: BACKGROUND_CLASS)
TRAIN_ID_NAMES: Tuple[str, ...] = tuple(n for n, _, t in sorted(CITYSCAPES_LABELS, key=lambda r: r[2]) if t != 255)


def id_to_train_id_lut() -> np.ndarray:
    """uint8 [256]: Cityscapes label id -> train id, every id that is not evaluated (and every id the definition lacks) -> 19."""
    lut = np.full(256, IGNORE_CLASS, dtype=np.uint8)
    for _, i, t in CITYSCAPES_LABELS:
        if i >= 0 and t != 255:
            lut[i] = t
    return lut


# ------------------------------------------------------------------------------------------------ metrics
def iou_from_confusion(cm) -> torch.Tensor:
    """ignite's IoU on a [C,C] confusion matrix (rows = target): diag / (rowsum + colsum - diag + 1e-15) in float64.
    A class without pixels in either role gives 0."""
    cm = torch.as_tensor(cm).double()
    return cm.diag() / (cm.sum(dim=1) + cm.sum(dim=0) - cm.diag() + 1e-15)


def iou_soft_from_confusion(cm) -> torch.Tensor:
    """The reference's get_miou_and_ious (eval_cdm.py) on its soft matrix (rows = prediction): diag / (colsum + rowsum - diag),
    NaN -> 0.  In float64 (the reference's float32 sums lose integers past 2^24)."""
    cm = torch.as_tensor(cm).double()
    diag = cm.diag()
    iou = diag / (cm.sum(dim=0) + cm.sum(dim=1) - diag)
    iou[iou != iou] = 0
    return iou


class SegmentationConfusion:
    """The two confusion matrices of the reference's Cityscapes evaluator over `num_classes` = K model channels, of which the
    first C = K - 1 are scored (the last is the ignore class, dropped as `prediction_onehot[:, 0:K-1]` drops it):
      confusion  int64 [C,C], rows = target, columns = argmax class: ignite's ConfusionMatrix(num_classes=C), accumulated;
      soft       int64 [C,C], rows = class, columns = target: the reference's update_cm, sum of the class probabilities per
                 target, truncated toward zero per update (its `.to(torch.int)`); soft_exact keeps the untruncated float64 sums.
    Pixels whose label is not in [0, C) are not counted (19, 255, ...).

    update(prediction, labels): prediction is [B,K,h,w] float (a view of channels-last memory — diffusion_out and the mean of
    predict_multiple — is read in place, any other layout is copied once at the low resolution), an integer or bool one-hot
    [B,K,h,w] (a "majority" diffusion_out) or a class map [B,h,w]; labels are [B,H,W] integers.  When (H,W) differs from (h,w)
    the prediction is upsampled bilinearly exactly as F.interpolate(mode="bilinear", align_corners=False) computes it in fp32.
    A one-hot or class map goes through the same arithmetic as the float32 of its one-hot, bit for bit; the reference cannot
    score those at resolution "original" (F.interpolate raises on the int64 one-hot).  Never builds a full-resolution tensor."""

    def __init__(self, num_classes: int, device=None):
        if not 2 <= int(num_classes) <= 32:
            raise ValueError(f"num_classes: {num_classes} (the kernel takes 2..32 channels, the last one the ignore class)")
        self.num_classes = int(num_classes)
        self.C = self.num_classes - 1
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hip.CcdmHipError("SegmentationConfusion runs on the GPU (no CPU path)")
        self._hard = torch.zeros((self.C, self.C), dtype=torch.int64, device=self.device)
        self.soft = torch.zeros((self.C, self.C), dtype=torch.int64)
        self.soft_exact = torch.zeros((self.C, self.C), dtype=torch.float64)
        self._ws: Optional[torch.Tensor] = None

    @property
    def confusion(self) -> torch.Tensor:
        return self._hard.cpu()

    def _prediction(self, prediction: torch.Tensor):
        """-> (fp32 channels-last tensor or None, pixel stride, uint8 class map or None, h, w)"""
        K = self.num_classes
        prediction = prediction.to(self.device)
        if prediction.ndim == 3:
            return None, 0, prediction.to(torch.uint8).contiguous(), int(prediction.shape[1]), int(prediction.shape[2])
        if prediction.ndim != 4 or prediction.shape[1] != K:
            raise ValueError(f"prediction: expected [B,{K},h,w] or a class map [B,h,w], got {tuple(prediction.shape)}")
        h, w = int(prediction.shape[2]), int(prediction.shape[3])
        if not prediction.is_floating_point():
            return None, 0, prediction.argmax(dim=1).to(torch.uint8).contiguous(), h, w
        p = prediction.to(torch.float32).permute(0, 2, 3, 1)
        ps = p.stride(2)
        if not (p.stride(3) == 1 and ps >= K and p.stride(1) == w * ps and p.stride(0) == h * w * ps):
            p, ps = p.contiguous(), K
        return p, ps, None, h, w

    @torch.no_grad()
    def update(self, prediction: torch.Tensor, labels: torch.Tensor) -> None:
        if labels.ndim != 3 or labels.shape[0] != prediction.shape[0]:
            raise ValueError(f"labels: expected [B,H,W] with B = {prediction.shape[0]}, got {tuple(labels.shape)}")
        probs, ps, cls, h, w = self._prediction(prediction)
        lab = labels.to(self.device)
        if lab.dtype != torch.uint8:      # anything outside [0, 255] is not counted either way: 255 stands for it
            lab = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab).to(torch.uint8)
        lab = lab.contiguous()
        B, H, W = (int(s) for s in lab.shape)
        lib = hip.load()
        need = int(lib.ccdm_seg_confusion_workspace_bytes(B, H, W, self.num_classes)) if B > 0 else 0
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        soft = torch.empty((self.C, self.C), dtype=torch.float64, device=self.device)
        ws = self._ws.data_ptr() if need else None
        hip.check(lib.ccdm_seg_confusion(probs.data_ptr() if probs is not None else None, ps, cls.data_ptr() if cls is not None else None,
                                         lab.data_ptr(), B, h, w, H, W, self.num_classes, self._hard.data_ptr(), soft.data_ptr(), ws, need,
                                         torch.cuda.current_stream(self.device).cuda_stream), "seg_confusion")
        soft = soft.cpu()
        self.soft_exact += soft
        self.soft += soft.trunc().to(torch.int64)

    def iou(self) -> torch.Tensor:
        return iou_from_confusion(self.confusion)

    def miou(self) -> float:
        return float(self.iou().mean())

    def iou_soft(self) -> torch.Tensor:
        return iou_soft_from_confusion(self.soft)

    def miou_soft(self) -> float:
        return float(self.iou_soft().mean())


# ------------------------------------------------------------------------------------------------ data
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class CityscapesVal(torch.utils.data.Dataset):
    """The Cityscapes split the reference's `datasets.cityscapes.validation_dataset` reads with a "resize" pipeline, re-stated
    with PIL and numpy.  Items are (image [3,H,W] fp32, one-hot labels [20,H,W] fp32, original labels [H0,W0] int64):
      pairs   leftImg8bit/<split>/<city>/*_leftImg8bit.png with gtFine/<split>/<city>/*_gtFine_labelIds.png, sorted by city and
              file name (torchvision walks `os.listdir`, whose order depends on the filesystem);
      image   PIL resize to target_size = (H, W) with BILINEAR, /255, normalised with the ImageNet mean and std;
      labels  PIL resize with NEAREST, label id -> train id (not evaluated -> 19), one-hot over 20 classes;
      original labels: the full-resolution train ids.  The reference hands `infer_step` the raw label ids here, which do not
              compare with train-id predictions; this is what its evaluator needs.
    max_size: the subset random_split(dataset, [max_size, n - max_size], generator=Generator().manual_seed(1)) keeps, in its order.
    root defaults to ${TMPDIR}/cityscapes/ (the reference's BASE_PATH)."""

    def __init__(self, root: Optional[str] = None, split: str = "val", target_size: Sequence[int] = (256, 512),
                 max_size: Optional[int] = None):
        self.root = os.path.expandvars(root if root else "${TMPDIR}/cityscapes/")
        self.split = split
        self.target_size = (int(target_size[0]), int(target_size[1]))
        img_dir = os.path.join(self.root, "leftImg8bit", split)
        if not os.path.isdir(img_dir):
            raise FileNotFoundError(f"{img_dir}: no Cityscapes images (set dataset_path to the directory holding leftImg8bit/ and gtFine/)")
        self.pairs: List[Tuple[str, str]] = []
        for city in sorted(os.listdir(img_dir)):
            for img in sorted(glob.glob(os.path.join(img_dir, city, "*_leftImg8bit.png"))):
                lbl = os.path.join(self.root, "gtFine", split, city,
                                   os.path.basename(img)[:-len("_leftImg8bit.png")] + "_gtFine_labelIds.png")
                if not os.path.exists(lbl):
                    raise FileNotFoundError(f"{lbl}: the label of {img} is missing")
                self.pairs.append((img, lbl))
        self.indices = list(range(len(self.pairs)))
        if max_size:
            n = len(self.pairs)
            if max_size > n:
                raise ValueError(f"dataset_val_max_size = {max_size} > {n} images in {img_dir}")
            self.indices = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:max_size].tolist()
        self.lut = id_to_train_id_lut()

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        from PIL import Image
        img_path, lbl_path = self.pairs[self.indices[i]]
        H, W = self.target_size
        with Image.open(img_path) as im:
            img = np.asarray(im.convert("RGB").resize((W, H), Image.BILINEAR))
        with Image.open(lbl_path) as lb:
            ids = np.asarray(lb)
            small = np.asarray(lb.resize((W, H), Image.NEAREST))
        image = torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255)
        image = image.sub(torch.tensor(IMAGENET_MEAN)[:, None, None]).div(torch.tensor(IMAGENET_STD)[:, None, None])
        train = torch.from_numpy(self.lut[small.astype(np.int64) & 255].astype(np.int64))
        onehot = torch.nn.functional.one_hot(train, NUM_CLASSES).permute(2, 0, 1).float()
        original = torch.from_numpy(self.lut[ids.astype(np.int64) & 255].astype(np.int64))
        return image, onehot, original


class SyntheticCityscapes(torch.utils.data.Dataset):
    """Cityscapes-shaped stand-in: image [3,h,w], one-hot labels [20,h,w] and original train-id labels at `original_size`:
    a few class blobs over a background class, with ignore pixels (19 and 255) sprinkled in.  Deterministic per (seed, item)."""

    def __init__(self, size: int = 4, resolution: Sequence[int] = (32, 32), original_size: Sequence[int] = (64, 96), seed: int = 0):
        self.size, self.seed = int(size), int(seed)
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.original_size = (int(original_size[0]), int(original_size[1]))

    def __len__(self):
        return self.size

    def __getitem__(self, i):
        rng = np.random.default_rng(self.seed * 100003 + i)
        H0, W0 = self.original_size
        yy, xx = np.mgrid[0:H0, 0:W0] / np.array([H0, W0])[:, None, None]
        lab = np.full((H0, W0), rng.integers(0, 19), dtype=np.int64)
        for _ in range(4):
            cy, cx, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.3)
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(0, 19)
        lab[rng.random((H0, W0)) < 0.03] = IGNORE_CLASS
        lab[rng.random((H0, W0)) < 0.01] = 255
        h, w = self.resolution
        ry = np.minimum((np.arange(h) * H0) // h, H0 - 1)
        rx = np.minimum((np.arange(w) * W0) // w, W0 - 1)
        small = lab[ry][:, rx]
        small = np.where(small == 255, IGNORE_CLASS, small)
        onehot = torch.nn.functional.one_hot(torch.from_numpy(small), NUM_CLASSES).permute(2, 0, 1).float()
        colour = rng.uniform(-1, 1, (NUM_CLASSES, 3)).astype(np.float32)
        image = colour[small].transpose(2, 0, 1) + 0.2 * rng.standard_normal((3, h, w)).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)), onehot, torch.from_numpy(lab)


def make_segmentation_dataset(params: dict):
    """`dataset_file` "...synthetic..." -> SyntheticCityscapes, else CityscapesVal at dataset_path (default ${TMPDIR}/cityscapes/).
    The size comes from dataset_pipeline_val_settings.target_size (the reference's "resize" setting), the subset from
    dataset_val_max_size; the stand-in's original label size from the build-owned key `original_size`."""
    settings = params.get("dataset_pipeline_val_settings") or {}
    max_size = params.get("dataset_val_max_size", None)
    if "synthetic" in params["dataset_file"]:
        return SyntheticCityscapes(size=max_size or 4, resolution=settings.get("target_size", (32, 32)),
                                   original_size=params.get("original_size", (64, 96)))
    return CityscapesVal(params.get("dataset_path") or None, "val", settings.get("target_size", (256, 512)), max_size)


# ------------------------------------------------------------------------------------------------ evaluation
RESOLUTIONS = ("original", "dataloader")


def _feature_encoder(params: dict, synthetic_weights_seed: Optional[int], device):
    fce = params.get("feature_cond_encoder") or {"type": "none"}
    if fce.get("type", "none") == "none":
        return None
    if "dino" not in fce["type"]:
        raise ValueError(f"feature_cond_encoder.type: {fce['type']!r} (expected 'none' or 'dino')")
    from .dino import DinoViT, make_synthetic_vit_state_dict
    model_type = fce.get("model", "dino_vits8")
    path = fce.get("weights")
    if path:
        path = os.path.expanduser(os.path.expandvars(path))
        if not os.path.exists(path):
            raise FileNotFoundError(f"feature_cond_encoder.weights: {path} does not exist (the {model_type} checkpoint's state_dict)")
        sd = torch.load(path, map_location="cpu", weights_only=True)
    elif synthetic_weights_seed is not None:
        sd = make_synthetic_vit_state_dict(model_type, synthetic_weights_seed)
    else:
        raise ValueError("feature_cond_encoder.type is 'dino' but feature_cond_encoder.weights names no checkpoint: set it to the "
                         f"{model_type} weights file (there is no hub download)")
    return DinoViT(model_type, bool(fce.get("train", False)), fce.get("conditioning", "concat_pixels_concat_features"),
                   stride=int(fce.get("output_stride", 8)), state_dict=sd, device=str(device))


@torch.no_grad()
def eval_segmentation(params: dict, dataset=None, device=None, model=None, synthetic_weights_seed: Optional[int] = None) -> Dict[str, object]:
    """The reference Evaluator's inference loop (eval_cdm.py: `infer_step` over the validation loader, ignite's IoU / mIoU and its
    own soft mIoU), without ignite.  Per batch: feature condition (DinoViT when feature_cond_encoder.type is dino), prediction
    through evaluation.predict_multiple (`evaluations`, `evaluation_vote_strategy`, the `evaluation:` section), the labels of
    `evaluation.resolution` ("original": the full-resolution labels, "dataloader" (default): the argmax of the one-hot labels),
    and both confusion matrices (SegmentationConfusion).  The checkpoint is `load_from`'s "average_model".
    `model`: a ready DenoisingModel-like callable (tests inject one); default: built from `params`."""
    from . import evaluation as E
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1:
        raise NotImplementedError(f"eval_segmentation runs on one rank: sharding the evaluation over WORLD_SIZE = {world} ranks is not "
                                  "built yet (launch it without torchrun)")
    device = torch.device(device if device is not None else "cuda")
    dataset = dataset if dataset is not None else make_segmentation_dataset(params)
    LOGGER.info("%d images in validation dataset '%s'", len(dataset), params["dataset_file"])
    section = params.get("evaluation") or {}
    resolution = section.get("resolution", "dataloader")
    if resolution not in RESOLUTIONS:
        raise ValueError(f"evaluation.resolution: {resolution!r} is not in {list(RESOLUTIONS)}")
    evaluations, vote = E.vote_settings(params)
    loader = torch.utils.data.DataLoader(dataset, batch_size=params["batch_size"], shuffle=False, num_workers=params.get("mp_loaders", 0))
    image0, labels0, _ = dataset[0]
    input_shapes = [tuple(image0.shape), tuple(labels0.shape)]
    num_classes = input_shapes[1][0]
    encoder = _feature_encoder(params, synthetic_weights_seed, device)
    if model is None:
        model = E.build_from_params(params, input_shapes, device)
        if params.get("load_from"):
            E.load_checkpoint(model, E.expanduservars(params["load_from"]), key="average_model")
        elif synthetic_weights_seed is not None:
            from .unet_spec import make_synthetic_state_dict
            model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, synthetic_weights_seed).items()})
        E.apply_sampler_options(model, params)
    conf = SegmentationConfusion(num_classes, device)
    n_img = 0
    for image, labels, labels_orig in loader:
        image = image.to(device)
        feature_condition = encoder(image) if encoder is not None else None
        prediction = E.predict_multiple(model, image, params, feature_condition)
        target = labels_orig if resolution == "original" else labels.argmax(dim=1)
        conf.update(prediction, target.to(device))
        n_img += image.shape[0]
    iou, iou_soft = conf.iou(), conf.iou_soft()
    names = TRAIN_ID_NAMES if conf.C == len(TRAIN_ID_NAMES) else tuple(str(c) for c in range(conf.C))
    for name, a, b in zip(names, iou.tolist(), iou_soft.tolist()):
        LOGGER.info("IoU %-14s %.4f  (soft %.4f)", name, a, b)
    res = {"mIoU": float(iou.mean()), "IoU": iou.tolist(), "mIoU_soft": float(iou_soft.mean()), "IoU_soft": iou_soft.tolist(),
           "confusion": conf.confusion.tolist(), "images": n_img, "resolution": resolution, "evaluations": evaluations, "vote": vote}
    LOGGER.info("mIoU %.4f  soft mIoU %.4f over %d images (resolution %s, %d evaluation(s), %s)", res["mIoU"], res["mIoU_soft"], n_img,
                resolution, evaluations, vote)
    return res
