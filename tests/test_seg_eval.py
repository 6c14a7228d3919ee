"""Cityscapes mIoU evaluation: the fused upsample-and-confusion kernel (ccdm_seg_confusion), SegmentationConfusion, the dataset
readers, eval_segmentation and its entry point.  The GPU tests compare against float64 re-statements of the reference's
Evaluator.infer_step / update_cm (evaluation/eval_cdm.py) and of ignite's ConfusionMatrix / IoU (ignite is not installed here;
its target mask `(y >= 0) & (y < num_classes)` and `diag / (rowsum + colsum - diag + 1e-15)` are restated below)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import build_model, hip, make_synthetic_state_dict
from ccdm_stochastic_segmentation_amd import segmentation as SEG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_SYMBOLS = {"ccdm_seg_confusion", "ccdm_seg_confusion_workspace_bytes"}
LIDC_BP = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1,
               num_head_channels=32, softmax_output=True)
NEAR = 1e-5          # float64 top-two margin below which the fp32 kernel may pick the other class
SOFT_RTOL = 1e-5


# ------------------------------------------------------------------------------------------------ float64 re-statements
def ignite_confusion(pred: torch.Tensor, target: torch.Tensor, C: int) -> torch.Tensor:
    """ignite.metrics.ConfusionMatrix.update on class indices: rows = target, columns = prediction, target outside [0, C) dropped."""
    t, p = target.reshape(-1).long(), pred.reshape(-1).long()
    m = (t >= 0) & (t < C)
    return torch.bincount(t[m] * C + p[m], minlength=C * C).reshape(C, C)


def ignite_iou(cm) -> np.ndarray:
    cm = np.asarray(cm, dtype=np.float64)
    return np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm) + 1e-15)


def reference_soft_iou(cm) -> np.ndarray:
    """get_miou_and_ious: rows of cm = prediction; NaN -> 0"""
    cm = np.asarray(cm, dtype=np.float64)
    d = np.diag(cm)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = d / (cm.sum(0) + cm.sum(1) - d)
    iou[np.isnan(iou)] = 0
    return iou


def ref64(pred_bkhw: torch.Tensor, labels: torch.Tensor, interp=None):
    """(hard [C,C] int64, soft [C,C] float64 (rows = class), near-tie mask [B,H,W], counted mask) of infer_step in float64."""
    K = pred_bkhw.shape[1]
    C = K - 1
    H, W = labels.shape[1:]
    p = pred_bkhw.double()
    if interp is not None:
        up = interp
    elif tuple(p.shape[2:]) != (H, W):
        up = F.interpolate(p, (H, W), mode="bilinear", align_corners=False)
    else:
        up = p
    up = up[:, :C]
    pred = up.argmax(1)
    lab = labels.long()
    counted = (lab >= 0) & (lab < C)
    if C >= 2:
        top2 = up.topk(2, dim=1).values
        near = (top2[:, 0] - top2[:, 1] < NEAR) & counted
    else:
        near = torch.zeros_like(counted)
    hard = ignite_confusion(pred, lab, C)
    flat = up.permute(1, 0, 2, 3).reshape(C, -1)
    t = lab.reshape(-1)
    oh = F.one_hot(torch.where(counted.reshape(-1), t, torch.full_like(t, C)), C + 1)[:, :C].double()
    soft = flat @ oh
    return hard, soft, near, counted


def kernel(pred, labels, K, device="cuda"):
    """one SegmentationConfusion.update: (hard int64 [C,C], untruncated soft float64 [C,C])"""
    sc = SEG.SegmentationConfusion(K, device)
    sc.update(pred, labels)
    return sc.confusion, sc.soft_exact.clone()


def check_against(hard_k, soft_k, hard_r, soft_r, near, counted, max_near_frac=0.002, log=None, tag=""):
    n_near = int(near.sum())
    n = int(counted.sum())
    # every counted pixel lands in its target row whatever its class: row sums are exact
    assert torch.equal(hard_k.sum(1), hard_r.sum(1)), (hard_k.sum(1), hard_r.sum(1))
    diff = int((hard_k - hard_r).abs().sum())
    assert diff <= 2 * n_near, (tag, diff, n_near)
    assert n_near <= max(4, max_near_frac * n), (tag, n_near, n)
    err = (soft_k - soft_r).abs()
    assert torch.all(err <= SOFT_RTOL * soft_r.abs()), (tag, float((err / soft_r.abs().clamp_min(1e-300)).max()))
    rel = float((err / soft_r.abs().clamp_min(1e-300)).max()) if soft_r.numel() else 0.0
    if log is not None:
        log(f"seg_confusion[{tag}]", near=n_near, pixels=n, hard_diff=diff, soft_max_rel=rel)


# ------------------------------------------------------------------------------------------------ CPU
def test_seg_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ccdm_seg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == SEG_SYMBOLS == {k for k in hip.SIGNATURES if k.startswith("ccdm_seg_")}
    assert "ccdm_segeval.hip" in hip.SOURCES and hip.ABI_VERSION == 11
    lib = hip.load()
    for name in SEG_SYMBOLS:
        assert hasattr(lib, name)
    # host-side size query: at most 1024 blocks of a [C,C] fp64 + int32 slab row (the C4 shape has 8192 tiles)
    assert lib.ccdm_seg_confusion_workspace_bytes(16, 1024, 2048, 20) == 1024 * 19 * 19 * 12
    assert lib.ccdm_seg_confusion_workspace_bytes(1, 64, 64, 5) == 1 * 16 * 12
    assert lib.ccdm_seg_confusion_workspace_bytes(1, 64, 64, 33) == 0


def test_iou_formulas_on_hand_made_matrices():
    cm = torch.tensor([[5, 1, 0, 0], [2, 7, 0, 1], [0, 0, 0, 0], [0, 3, 0, 4]], dtype=torch.int64)     # class 2: no pixels at all
    iou = SEG.iou_from_confusion(cm).numpy()
    np.testing.assert_array_equal(iou, ignite_iou(cm.numpy()))
    assert iou[2] == 0.0 and not np.isnan(iou).any()
    np.testing.assert_allclose(iou, [5 / 8, 7 / 14, 0.0, 4 / 8], rtol=1e-14)
    soft = torch.tensor([[3, 1, 0, 2], [0, 6, 0, 1], [0, 0, 0, 0], [1, 0, 0, 5]], dtype=torch.int64)
    isoft = SEG.iou_soft_from_confusion(soft).numpy()
    np.testing.assert_array_equal(isoft, reference_soft_iou(soft.numpy()))
    assert isoft[2] == 0.0 and not np.isnan(isoft).any()
    np.testing.assert_allclose(isoft, [3 / (4 + 6 - 3), 6 / (7 + 7 - 6), 0.0, 5 / (8 + 6 - 5)], rtol=1e-14)


def test_train_id_table_matches_golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "cityscapes_train_ids.json")))
    assert [list(r) for r in SEG.CITYSCAPES_LABELS] == g["classes"]
    lut = SEG.id_to_train_id_lut()
    for name, i, t in g["classes"]:
        if i >= 0:
            assert lut[i] == (19 if t == 255 else t), name
    assert all(lut[i] == 19 for i in range(34, 256))
    assert len(SEG.TRAIN_ID_NAMES) == 19 and SEG.TRAIN_ID_NAMES[0] == "road" and SEG.TRAIN_ID_NAMES[18] == "bicycle"


def _write_tree(root, split, files):
    from PIL import Image
    rng = np.random.default_rng(5)
    for city, stem in files:
        for d in ("leftImg8bit", "gtFine"):
            os.makedirs(os.path.join(root, d, split, city), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)).save(os.path.join(root, "leftImg8bit", split, city, stem + "_leftImg8bit.png"))
        ids = rng.integers(0, 36, (24, 40)).astype(np.uint8)
        ids[0, :4] = [0, 7, 33, 34]
        Image.fromarray(ids).save(os.path.join(root, "gtFine", split, city, stem + "_gtFine_labelIds.png"))


def test_cityscapes_reader(tmp_path):
    from PIL import Image
    files = [("zurich", "zurich_000001_000019"), ("aachen", "aachen_000002_000019"), ("aachen", "aachen_000000_000019"),
             ("bremen", "bremen_000000_000019"), ("zurich", "zurich_000000_000019")]
    _write_tree(str(tmp_path), "val", files)
    ds = SEG.CityscapesVal(str(tmp_path), "val", target_size=(12, 16))
    stems = [os.path.basename(a)[:-len("_leftImg8bit.png")] for a, _ in ds.pairs]
    assert stems == sorted(s for _, s in files)                       # sorted by city, then by file name
    for a, b in ds.pairs:
        assert os.path.basename(b) == os.path.basename(a).replace("_leftImg8bit.png", "_gtFine_labelIds.png")
    image, onehot, orig = ds[1]
    img_path, lbl_path = ds.pairs[1]
    rgb = np.asarray(Image.open(img_path).convert("RGB").resize((16, 12), Image.BILINEAR)).astype(np.float32) / 255
    want = (rgb - np.array(SEG.IMAGENET_MEAN, np.float32)) / np.array(SEG.IMAGENET_STD, np.float32)
    assert image.shape == (3, 12, 16) and image.dtype == torch.float32
    np.testing.assert_allclose(image.permute(1, 2, 0).numpy(), want, rtol=0, atol=1e-6)
    ids_full = np.asarray(Image.open(lbl_path))
    ids_small = np.asarray(Image.open(lbl_path).resize((16, 12), Image.NEAREST))
    golden = {i: (19 if t == 255 else t) for _, i, t in json.load(open(os.path.join(ROOT, "tests", "golden", "cityscapes_train_ids.json")))["classes"]}
    tid = np.vectorize(lambda i: golden.get(int(i), 19))
    assert onehot.shape == (20, 12, 16) and torch.all(onehot.sum(0) == 1)
    np.testing.assert_array_equal(onehot.argmax(0).numpy(), tid(ids_small))
    assert orig.shape == (24, 40) and orig.dtype == torch.int64                     # full resolution, train ids
    np.testing.assert_array_equal(orig.numpy(), tid(ids_full))
    assert orig[0, :4].tolist() == [19, 0, 18, 19]                                    # unlabeled, road, bicycle, unknown id 34
    # max_size: the subset random_split(..., generator=manual_seed(1)) keeps
    sub = SEG.CityscapesVal(str(tmp_path), "val", target_size=(12, 16), max_size=3)
    want_idx = torch.utils.data.random_split(range(5), [3, 2], generator=torch.Generator().manual_seed(1))[0].indices
    assert sub.indices == list(want_idx) and len(sub) == 3
    torch.testing.assert_close(sub[0][2], ds[want_idx[0]][2], rtol=0, atol=0)
    with pytest.raises(FileNotFoundError):
        SEG.CityscapesVal(str(tmp_path / "nowhere"))


def test_synthetic_cityscapes_shapes():
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(64, 96))
    image, onehot, orig = ds[1]
    assert image.shape == (3, 32, 32) and onehot.shape == (20, 32, 32) and orig.shape == (64, 96)
    assert torch.all(onehot.sum(0) == 1)
    assert (orig == 19).any() and (orig == 255).any() and (orig < 19).any()
    torch.testing.assert_close(ds[1][2], orig, rtol=0, atol=0)


def test_ddpm_eval_routes_cityscapes_miou(tmp_path, monkeypatch):
    import yaml
    import ddpm_eval
    calls = []

    def fake(params, **kw):
        calls.append((params["dataset_file"], kw))
        return {"mIoU": 0.5}
    monkeypatch.setattr(SEG, "eval_segmentation", fake)
    p = yaml.safe_load(open(os.path.join(ROOT, "params_eval_cityscapes_synthetic.yml")))
    f = tmp_path / "params_x.yml"
    for name in ("synthetic.cityscapes_miou", "datasets.cityscapes_miou"):
        p["dataset_file"] = name
        yaml.safe_dump(p, open(f, "w"))
        ddpm_eval.main(["ddpm_eval.py", str(f)])
        assert calls[-1][0] == name
    assert calls[0][1]["synthetic_weights_seed"] == 0 and calls[1][1]["synthetic_weights_seed"] is None
    p["dataset_file"] = "datasets.cityscapes"
    yaml.safe_dump(p, open(f, "w"))
    with pytest.raises(NotImplementedError, match="cityscapes_miou"):
        ddpm_eval.main(["ddpm_eval.py", str(f)])


def test_eval_segmentation_refuses_several_ranks(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="sharding"):
        SEG.eval_segmentation({"dataset_file": "synthetic.cityscapes_miou"})


# ------------------------------------------------------------------------------------------------ GPU: kernel
def _dirichlet(rng, B, h, w, K):
    return torch.from_numpy(rng.dirichlet(np.ones(K), (B, h, w)).astype(np.float32))        # [B,h,w,K] channels-last


def _labels(rng, B, H, W, C):
    """spatially coherent blocks of targets, with 19, 255 and other values >= C sprinkled in"""
    coarse = rng.integers(0, C, (B, max(1, H // 8) + 1, max(1, W // 8) + 1))
    lab = coarse[:, np.arange(H) // 8][:, :, np.arange(W) // 8].astype(np.int64)
    r = rng.random((B, H, W))
    lab[r < 0.03] = 19
    lab[(r >= 0.03) & (r < 0.05)] = 255
    lab[(r >= 0.05) & (r < 0.06)] = C + 3
    return torch.from_numpy(lab)


SHAPES = [("identity", 40, 56, 40, 56), ("x8", 16, 24, 128, 192), ("non_integer", 30, 50, 97, 211), ("down", 64, 64, 40, 48),
          ("x4_wide", 8, 70, 32, 280)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_vs_float64_dirichlet(shape, K, parity_log):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(K * 1000 + h)
    B = 2
    nhwc = _dirichlet(rng, B, h, w, K)
    labels = _labels(rng, B, H, W, K - 1)
    pred = nhwc.permute(0, 3, 1, 2)                                 # BCHW view of channels-last memory
    hard_k, soft_k = kernel(pred.cuda(), labels.cuda(), K)
    hard_r, soft_r, near, counted = ref64(pred, labels)
    check_against(hard_k, soft_k, hard_r, soft_r, near, counted, log=parity_log, tag=f"{tag}_K{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 20])
def test_kernel_tied_and_peaked_rows(K, parity_log):
    """Rows whose two top classes tie exactly — the same pair over an image, so the interpolated values of the pair tie exactly too
    (the same operations on the same values) and both sides take the lowest index — and rows peaked at 1 - 1e-7."""
    rng = np.random.default_rng(K)
    B, h, w, H, W = 2, 12, 20, 50, 70
    C = K - 1
    tied = rng.dirichlet(np.ones(K - 2), (B, h, w)).astype(np.float32) * np.float32(0.1)
    top = rng.integers(0, C - 1, B)
    tied = np.stack([np.insert(tied[b], [top[b], top[b]], np.float32(0.45), axis=2) for b in range(B)])
    assert tied.shape == (B, h, w, K)
    labels = _labels(rng, B, H, W, C)
    t = torch.from_numpy(tied)
    hard_k, soft_k = kernel(t.permute(0, 3, 1, 2).cuda(), labels.cuda(), K)
    hard_r, soft_r, near, counted = ref64(t.permute(0, 3, 1, 2), labels)
    torch.testing.assert_close(hard_k, hard_r, rtol=0, atol=0)                           # exact ties: exact matrix
    check_against(hard_k, soft_k, hard_r, soft_r, torch.zeros_like(near), counted)
    peaked = np.full((B, h, w, K), 1e-7 / (K - 1), np.float32)
    cls = rng.integers(0, K, (B, h, w))
    np.put_along_axis(peaked, cls[..., None], np.float32(1 - 1e-7), axis=3)
    p = torch.from_numpy(peaked)
    hard_k, soft_k = kernel(p.permute(0, 3, 1, 2).cuda(), labels.cuda(), K)
    hard_r, soft_r, near, counted = ref64(p.permute(0, 3, 1, 2), labels)
    # peaked rows act like a one-hot map: where two classes meet, the bilinear weights themselves tie (about 13 % of the
    # pixels at this ratio); those pixels may go either way, every other pixel must agree
    check_against(hard_k, soft_k, hard_r, soft_r, near, counted, max_near_frac=0.25, log=parity_log, tag=f"peaked_K{K}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=[s[0] for s in SHAPES[:4]])
def test_class_map_bitwise_equals_float_onehot(shape, K):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(K + 7)
    B = 2
    cls = torch.from_numpy(rng.integers(0, K, (B, h, w)))
    labels = _labels(rng, B, H, W, K - 1).cuda()
    onehot_f = F.one_hot(cls, K).float().cuda().permute(0, 3, 1, 2)          # channels-last fp32 one-hot
    onehot_i = F.one_hot(cls, K).permute(0, 3, 1, 2).contiguous().cuda()       # int64 BCHW one-hot ("majority" diffusion_out)
    hf, sf = kernel(onehot_f, labels, K)
    hc, sc = kernel(cls.to(torch.uint8).cuda(), labels, K)
    hi, si = kernel(onehot_i, labels, K)
    for h2, s2 in ((hc, sc), (hi, si)):
        assert torch.equal(hf, h2)
        assert torch.equal(sf, s2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[1:4], ids=[s[0] for s in SHAPES[1:4]])
def test_kernel_vs_torch_gpu_interpolate(shape):
    tag, h, w, H, W = shape
    K = 20
    C = K - 1
    rng = np.random.default_rng(h + w)
    B = 2
    pred = _dirichlet(rng, B, h, w, K).permute(0, 3, 1, 2).cuda()
    labels = _labels(rng, B, H, W, C).cuda()
    up = F.interpolate(pred, (H, W), mode="bilinear", align_corners=False)[:, :C]
    hard_t = ignite_confusion(up.argmax(1), labels, C).cpu()
    top2 = up.topk(2, dim=1).values
    counted = ((labels >= 0) & (labels < C)).cpu()
    near = ((top2[:, 0] - top2[:, 1]) < NEAR).cpu() & counted
    hard_k, soft_k = kernel(pred, labels, K)
    _, soft_r, _, _ = ref64(pred.cpu(), labels.cpu())
    check_against(hard_k, soft_k, hard_t, soft_r, near, counted)


def _c4_inputs(B=16, h=256, w=512, H=1024, W=2048, K=20, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.rand((B, h, w, K), generator=g, device="cuda") ** 4
    p = p / p.sum(-1, keepdim=True)
    coarse = torch.randint(0, 21, (B, H // 32, W // 32), generator=g, device="cuda")
    lab = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)
    lab = torch.where(lab == 20, torch.full_like(lab, 255), lab).to(torch.uint8)
    return p.permute(0, 3, 1, 2), lab


@pytest.mark.gpu
def test_c4_shape_deterministic_and_lean():
    pred, lab = _c4_inputs()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    sc = SEG.SegmentationConfusion(20, "cuda")
    sc.update(pred, lab)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    full = 16 * 20 * 1024 * 2048 * 4
    assert peak < 64 * 2 ** 20, peak                      # one full-resolution probability tensor would be 2.7 GB
    hard1, soft1 = sc.confusion, sc.soft_exact.clone()
    sc2 = SEG.SegmentationConfusion(20, "cuda")
    sc2.update(pred, lab)
    assert torch.equal(hard1, sc2.confusion) and torch.equal(soft1, sc2.soft_exact)
    assert int(hard1.sum()) == int((lab < 19).sum())
    assert peak < full / 40


@pytest.mark.gpu
def test_three_updates_equal_one():
    rng = np.random.default_rng(3)
    K, C = 20, 19
    pred = _dirichlet(rng, 6, 20, 30, K).permute(0, 3, 1, 2).cuda()
    labels = _labels(rng, 6, 70, 90, C).cuda()
    one = SEG.SegmentationConfusion(K, "cuda")
    one.update(pred, labels)
    three = SEG.SegmentationConfusion(K, "cuda")
    for s in (slice(0, 1), slice(1, 4), slice(4, 6)):
        three.update(pred[s], labels[s])
    assert torch.equal(one.confusion, three.confusion)
    torch.testing.assert_close(three.soft_exact, one.soft_exact, rtol=1e-12, atol=1e-9)
    assert torch.all((three.soft - one.soft).abs() <= 3)          # truncation is per update


# ------------------------------------------------------------------------------------------------ GPU: evaluator
class Recorder:
    """Wraps a DenoisingModel; records every prediction and feature condition evaluation.predict_multiple obtains from it."""

    def __init__(self, m):
        self.m, self.diffusion = m, m.diffusion
        self.preds, self.fcs = [], []

    def __call__(self, x, image, feature_condition=None):
        out = self.m(x, image, feature_condition)
        self.preds.append(out["diffusion_out"].clone())
        self.fcs.append(feature_condition)
        return out

    def predict_multiple(self, image, feature_condition=None, **kw):
        out = self.m.predict_multiple(image, feature_condition, **kw)
        self.preds.append(out["mean"].clone())
        self.fcs.append(feature_condition)
        return out


def _k20_model(vote):
    m = build_model(250, "cosine", {"s": 0.008}, [(3, 32, 32), (20, 32, 32)], (3, 32, 32), "unet_openai",
                    dict(LIDC_BP, channel_mult=[1, 2, 4], attention_resolutions=[8]), "datasets.cityscapes", vote, None)
    m.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(m.unet.spec, 0).items()}, strict=True)
    m = m.cuda().eval()
    m.rng = "philox"
    return m


def _params(resolution, evaluations, vote, fce_type="none"):
    return {"dataset_file": "synthetic.cityscapes_miou", "batch_size": 2, "mp_loaders": 0,
            "evaluation": {"resolution": resolution, "evaluations": evaluations, "evaluation_vote_strategy": vote},
            "feature_cond_encoder": {"type": fce_type, "model": "dino_vits8", "channels": 384, "conditioning": "concat_pixels_concat_features",
                                     "output_stride": 8, "scale": "single", "train": False}}


@pytest.mark.gpu
@pytest.mark.parametrize("vote", ["confidence", "majority"])
@pytest.mark.parametrize("evaluations", [1, 3])
@pytest.mark.parametrize("resolution", ["original", "dataloader"])
def test_eval_segmentation_end_to_end(resolution, evaluations, vote, parity_log):
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    rec = Recorder(_k20_model(vote))
    res = SEG.eval_segmentation(_params(resolution, evaluations, vote), dataset=ds, model=rec)
    assert res["images"] == 3 and res["resolution"] == resolution and res["evaluations"] == evaluations and res["vote"] == vote
    assert len(rec.preds) == 2                                             # batches of 2 and 1
    # host re-statement of infer_step on the recorded predictions
    hard_r = torch.zeros((19, 19), dtype=torch.int64)
    soft_exact = torch.zeros((19, 19), dtype=torch.float64)
    n_near, i0 = 0, 0
    for pred in rec.preds:
        b = pred.shape[0]
        items = [ds[i] for i in range(i0, i0 + b)]
        i0 += b
        lab = torch.stack([it[2] for it in items]) if resolution == "original" else torch.stack([it[1] for it in items]).argmax(1)
        h, s, near, counted = ref64(pred.float().cpu(), lab)
        hard_r += h
        soft_exact += s
        n_near += int(near.sum())
    hard_k = torch.tensor(res["confusion"])
    assert torch.equal(hard_k.sum(1), hard_r.sum(1))
    assert int((hard_k - hard_r).abs().sum()) <= 2 * n_near
    if n_near == 0:
        assert torch.equal(hard_k, hard_r)
        np.testing.assert_allclose(res["IoU"], ignite_iou(hard_r.numpy()), rtol=0, atol=1e-15)
        assert abs(res["mIoU"] - float(ignite_iou(hard_r.numpy()).mean())) < 1e-15
    assert len(res["IoU"]) == 19 and len(res["IoU_soft"]) == 19 and 0 <= res["mIoU"] <= 1 and 0 <= res["mIoU_soft"] <= 1
    parity_log(f"eval_segmentation[{resolution},{evaluations},{vote}]", near=n_near, mIoU=res["mIoU"], mIoU_soft=res["mIoU_soft"])


@pytest.mark.gpu
def test_eval_segmentation_dino_feature_condition():
    from ccdm_stochastic_segmentation_amd.dino import DinoViT, make_synthetic_vit_state_dict
    fce = dict(type="dino", model="dino_vits8", channels=384, conditioning="concat_pixels_concat_features", output_stride=8,
               scale="single", train=False, source_layer=11, target_layer=10)
    K, H, W = 20, 64, 64
    model = build_model(4, "cosine", {"s": 0.008}, [(3, H, W), (K, H, W)], (3, H, W), "unet_openai",
                        dict(LIDC_BP, channel_mult=[1, 1, 2, 2, 4, 4]), "datasets.cityscapes", "confidence", fce)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 2).items()}, strict=True)
    model = model.cuda().eval()
    rec = Recorder(model)
    ds = SEG.SyntheticCityscapes(size=2, resolution=(H, W), original_size=(96, 128), seed=1)
    res = SEG.eval_segmentation(_params("original", 1, "confidence", "dino"), dataset=ds, model=rec, synthetic_weights_seed=4)
    enc = DinoViT("dino_vits8", False, "concat_pixels_concat_features", stride=8, state_dict=make_synthetic_vit_state_dict("dino_vits8", 4))
    image = torch.stack([ds[i][0] for i in range(2)]).cuda()
    want = enc(image)
    assert len(rec.fcs) == 1 and rec.fcs[0] is not None and rec.fcs[0].shape == (2, 384, H // 8, W // 8)
    assert torch.equal(rec.fcs[0], want)
    assert res["images"] == 2 and len(res["IoU"]) == 19


@pytest.mark.gpu
def test_eval_segmentation_dino_needs_weights():
    p = _params("original", 1, "confidence", "dino")
    with pytest.raises(ValueError, match="weights"):
        SEG.eval_segmentation(p, dataset=SEG.SyntheticCityscapes(size=1), model=object())
    p["feature_cond_encoder"]["weights"] = "/nonexistent/dino_vits8.pth"
    with pytest.raises(FileNotFoundError):
        SEG.eval_segmentation(p, dataset=SEG.SyntheticCityscapes(size=1), model=object())


@pytest.mark.gpu
def test_ddpm_eval_cityscapes_synthetic_entry_point():
    r = subprocess.run([sys.executable, "ddpm_eval.py", "params_eval_cityscapes_synthetic.yml"], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert len(res["IoU"]) == 19 and 0.0 <= res["mIoU"] <= 1.0 and res["resolution"] == "original" and res["images"] == 4
