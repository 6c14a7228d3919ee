"""Cityscapes prediction export: the fused upsample-and-classify kernel (ccdm_segexport) that writes train ids, label ids and
colours, export_predictions / export_labels, PredictionWriter and the `evaluation.save_predictions` key of eval_segmentation.
The exported class is held against the confusion kernel (exactly: both go through the device helpers of ccdm_seg_common.h) and
against float64 bilinear interpolation on the CPU (everywhere but at near-tie pixels)."""
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import segmentation as SEG
from tests.test_seg_eval import NEAR, SHAPES, Recorder, _c4_inputs, _dirichlet, _k20_model, _labels, _params, ignite_confusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_seg_eval.py's shapes, one whose W is not a multiple of 4 (rows start at any byte, a ragged last group of 3) and one
# narrower than a tile
EXPORT_SHAPES = SHAPES + [("w_mod4", 12, 33, 37, 131), ("narrow", 9, 14, 30, 45)]
GOLDEN_IDS = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33, 0]


def _tables(K, seed=0):
    """Cityscapes' tables at K = 20, otherwise made-up ones without repeated entries"""
    if K == 20:
        return np.array(SEG.TRAIN_ID_TO_ID, np.uint8), np.array(SEG.TRAIN_ID_TO_COLOR, np.uint8)
    rng = np.random.default_rng(seed + K)
    ids = rng.permutation(256)[:K].astype(np.uint8)
    col = rng.integers(0, 256, (K, 3)).astype(np.uint8)
    col[:, 0] = rng.permutation(256)[:K]
    return ids, col


# ------------------------------------------------------------------------------------------------ CPU
def test_export_symbol_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+ccdm_segexport\s*\(", hdr)
    assert "ccdm_segexport" in hip.SIGNATURES and len(hip.SIGNATURES["ccdm_segexport"][1]) == 16
    assert "ccdm_segexport.hip" in hip.SOURCES and "ccdm_segeval.hip" in hip.SOURCES
    assert hip.ABI_VERSION == 11
    lib = hip.load()
    assert hasattr(lib, "ccdm_segexport") and lib.ccdm_version() == 11


def test_export_tables_match_golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "cityscapes_export_tables.json")))
    assert g["train_id_to_id"] == GOLDEN_IDS
    assert len(g["train_id_to_color"]) == 20 and all(len(c) == 3 for c in g["train_id_to_color"])
    assert g["train_id_to_color"][0] == [128, 64, 128] and g["train_id_to_color"][19] == [0, 0, 0]
    assert list(SEG.TRAIN_ID_TO_ID) == g["train_id_to_id"]
    assert [list(c) for c in SEG.TRAIN_ID_TO_COLOR] == g["train_id_to_color"]
    # the id table inverts the evaluator's id -> train id lookup on the 19 evaluated classes
    lut = SEG.id_to_train_id_lut()
    assert [int(lut[i]) for i in SEG.TRAIN_ID_TO_ID[:19]] == list(range(19))
    assert len(SEG.CITYSCAPES_COLORS) == len(SEG.CITYSCAPES_LABELS)


def _fake_exports(monkeypatch, calls):
    """export_predictions / export_labels replaced by fixed arrays that depend on the running image number only"""
    def maps(B, H, W, first):
        ids = np.stack([np.full((H, W), 10 * (first + i), np.uint8) for i in range(B)])
        ids[:, 0, :3] = [7, 8, 33]
        rgb = np.stack([ids, ids + 1, ids + 2], axis=-1).astype(np.uint8)
        return ids, rgb

    def fake_pred(prediction, size, *, outputs=("label_id", "color"), **kw):
        calls.append(("pred", tuple(size), tuple(outputs)))
        ids, rgb = maps(prediction.shape[0], size[0], size[1], fake_pred.n)
        fake_pred.n += prediction.shape[0]
        return {"label_id": torch.from_numpy(ids), "color": torch.from_numpy(rgb)}

    def fake_lab(labels, *, outputs=("label_id",), **kw):
        calls.append(("lab", tuple(labels.shape[1:]), tuple(outputs)))
        ids, _ = maps(labels.shape[0], labels.shape[1], labels.shape[2], fake_lab.n)
        fake_lab.n += labels.shape[0]
        return {"label_id": torch.from_numpy(ids + 100)}
    fake_pred.n = fake_lab.n = 1
    monkeypatch.setattr(SEG, "export_predictions", fake_pred)
    monkeypatch.setattr(SEG, "export_labels", fake_lab)
    return maps


def test_prediction_writer_layout_numbering_and_pixels(tmp_path, monkeypatch):
    from PIL import Image
    calls = []
    maps = _fake_exports(monkeypatch, calls)
    wr = SEG.PredictionWriter(str(tmp_path), split="val")
    base = tmp_path / "outputs" / "val"
    assert sorted(os.listdir(base)) == ["debug", "label", "submit"]
    H, W = 6, 10
    wr.write(torch.zeros((2, 20, 3, 5)), torch.zeros((2, H, W), dtype=torch.int64), (H, W))
    wr.write(torch.zeros((1, 20, 3, 5)), torch.zeros((1, H, W), dtype=torch.int64), (H, W))
    assert [c[0] for c in calls] == ["pred", "lab", "pred", "lab"] and all(c[1] == (H, W) for c in calls)
    assert sorted(os.listdir(base / "submit")) == ["1_id.png", "2_id.png", "3_id.png"]
    assert sorted(os.listdir(base / "debug")) == ["1_rgb.png", "2_rgb.png", "3_rgb.png"]
    assert sorted(os.listdir(base / "label")) == ["1_label.png", "2_label.png", "3_label.png"]
    assert wr.pred_list == [str(base / "submit" / f"{n}_id.png") for n in (1, 2, 3)]
    assert wr.label_list == [str(base / "label" / f"{n}_label.png") for n in (1, 2, 3)]
    assert wr.images_cnt == 3
    for n in (1, 2, 3):
        ids, rgb = maps(1, H, W, n)
        with Image.open(base / "submit" / f"{n}_id.png") as im:
            assert im.mode == "L" and im.size == (W, H)
            np.testing.assert_array_equal(np.asarray(im), ids[0])
        with Image.open(base / "debug" / f"{n}_rgb.png") as im:
            assert im.mode == "RGB" and im.size == (W, H)
            np.testing.assert_array_equal(np.asarray(im), rgb[0])
        with Image.open(base / "label" / f"{n}_label.png") as im:
            assert im.mode == "L" and im.size == (W, H)
            np.testing.assert_array_equal(np.asarray(im), ids[0] + 100)


class _FakeConfusion:
    C = 19

    def __init__(self, num_classes, device):
        self.updates = []

    def update(self, prediction, labels):
        self.updates.append(prediction)

    confusion = torch.zeros((19, 19), dtype=torch.int64)

    def iou(self):
        return torch.zeros(19, dtype=torch.float64)

    iou_soft = iou


@pytest.mark.parametrize("key", [None, False, True])
def test_eval_segmentation_writes_only_with_the_key(tmp_path, monkeypatch, key):
    """Injected model, patched confusion and writer (no GPU): without evaluation.save_predictions no writer is made and the result
    has no lists; with it the writer gets the tensor the confusion got, the labels being scored and their size."""
    from ccdm_stochastic_segmentation_amd import evaluation as E
    made = []

    class FakeWriter:
        def __init__(self, directory, split="val"):
            self.directory, self.writes, self.pred_list, self.label_list = directory, [], [], []
            self.path_submit = os.path.join(directory, "outputs", split, "submit")
            made.append(self)

        def write(self, prediction, labels, size):
            self.writes.append((prediction, labels, tuple(size)))
            n = len(self.pred_list)
            self.pred_list += [f"p{n + i}" for i in range(prediction.shape[0])]
            self.label_list += [f"l{n + i}" for i in range(prediction.shape[0])]
    conf = []
    monkeypatch.setattr(SEG, "PredictionWriter", FakeWriter)
    monkeypatch.setattr(SEG, "SegmentationConfusion", lambda k, d: conf.append(_FakeConfusion(k, d)) or conf[-1])
    monkeypatch.setattr(E, "predict_multiple", lambda model, image, params, fc: torch.full((image.shape[0], 20, 32, 32), 0.05))
    params = {"dataset_file": "synthetic.cityscapes_miou", "batch_size": 2, "mp_loaders": 0, "output_path": str(tmp_path / "out"),
              "evaluation": {"resolution": "original", "evaluations": 1, "evaluation_vote_strategy": "confidence"}}
    if key is not None:
        params["evaluation"]["save_predictions"] = key
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    res = SEG.eval_segmentation(params, dataset=ds, device="cpu", model=object())
    assert res["images"] == 3 and len(conf[0].updates) == 2
    if not key:
        assert made == [] and "pred_list" not in res and "label_list" not in res
        assert not os.path.exists(tmp_path / "out")
        assert set(res) == {"mIoU", "IoU", "mIoU_soft", "IoU_soft", "confusion", "images", "resolution", "evaluations", "vote"}
    else:
        assert len(made) == 1 and made[0].directory == str(tmp_path / "out")
        assert [w[2] for w in made[0].writes] == [(48, 80), (48, 80)]
        assert all(w[0] is u for w, u in zip(made[0].writes, conf[0].updates))          # the tensor scored, no second pass
        assert torch.equal(made[0].writes[1][1].cpu(), ds[2][2][None])
        assert res["pred_list"] == ["p0", "p1", "p2"] and res["label_list"] == ["l0", "l1", "l2"]


def test_export_argument_checks():
    with pytest.raises(ValueError, match="outputs"):
        SEG._export(None, 0, None, 1, 4, 4, 4, 4, 20, 19, ("depth",), None, None, "cpu")
    with pytest.raises(ValueError, match="outputs"):
        SEG._export(None, 0, None, 1, 4, 4, 4, 4, 20, 19, (), None, None, "cpu")
    with pytest.raises(ValueError, match="tables"):
        SEG._export(None, 0, None, 1, 4, 4, 4, 4, 5, 4, ("train_id",), None, None, "cpu")
    with pytest.raises(ValueError, match="id_table"):
        SEG._export(None, 0, None, 1, 4, 4, 4, 4, 5, 4, ("train_id",), [1, 2, 3], np.zeros((5, 3)), "cpu")
    with pytest.raises(hip.CcdmHipError):
        SEG.export_predictions(torch.zeros((1, 20, 4, 4)), (8, 8), device="cpu")


# ------------------------------------------------------------------------------------------------ GPU: kernel
def _forms(nhwc, K):
    """the same prediction as a BCHW view of channels-last memory and as contiguous BCHW"""
    view = nhwc.cuda().permute(0, 3, 1, 2)
    return {"channels_last_view": view, "contiguous_bchw": view.contiguous()}


def _export(pred, size, K, outputs=("train_id", "label_id", "color")):
    ids, col = _tables(K)
    return SEG.export_predictions(pred, size, outputs=outputs, id_table=ids, color_table=col, num_classes=K)


def _check_tables(out, K):
    ids, col = _tables(K)
    t = out["train_id"].cpu().numpy()
    np.testing.assert_array_equal(out["label_id"].cpu().numpy(), ids[t])
    np.testing.assert_array_equal(out["color"].cpu().numpy(), col[t])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 20, 32])
@pytest.mark.parametrize("shape", EXPORT_SHAPES, ids=[s[0] for s in EXPORT_SHAPES])
def test_export_equals_confusion_kernel(shape, K):
    """A bincount of (labels, exported train id) over the counted pixels is SegmentationConfusion.confusion: zero differences, in
    every prediction form."""
    tag, h, w, H, W = shape
    C = K - 1
    rng = np.random.default_rng(K * 1000 + h)
    B = 2
    nhwc = _dirichlet(rng, B, h, w, K)
    labels = _labels(rng, B, H, W, C).cuda()
    cls = torch.from_numpy(rng.integers(0, K, (B, h, w)))
    forms = _forms(nhwc, K)
    forms["onehot_int"] = F.one_hot(cls, K).permute(0, 3, 1, 2).contiguous().cuda()
    forms["class_map"] = cls.to(torch.uint8).cuda()
    forms["onehot_float_of_class_map"] = F.one_hot(cls, K).float().cuda().permute(0, 3, 1, 2)
    got = {}
    for name, pred in forms.items():
        sc = SEG.SegmentationConfusion(K, "cuda")
        sc.update(pred, labels)
        out = _export(pred, (H, W), K)
        assert out["train_id"].shape == (B, H, W) and out["color"].shape == (B, H, W, 3)
        assert all(v.dtype == torch.uint8 and v.is_cuda for v in out.values())
        assert int(out["train_id"].max()) < C
        cm = ignite_confusion(out["train_id"], labels, C).cpu()
        assert int((cm - sc.confusion).abs().sum()) == 0, (name, tag, K)
        _check_tables(out, K)
        got[name] = out["train_id"]
    assert torch.equal(got["channels_last_view"], got["contiguous_bchw"])
    assert torch.equal(got["class_map"], got["onehot_int"]) and torch.equal(got["class_map"], got["onehot_float_of_class_map"])


def _ref64_classes(pred_bkhw, size, C):
    """(argmax, near-tie mask) of the float64 bilinear interpolation on the CPU over the first C channels"""
    p = pred_bkhw.double()
    up = F.interpolate(p, size, mode="bilinear", align_corners=False) if tuple(p.shape[2:]) != tuple(size) else p
    up = up[:, :C]
    if C >= 2:
        top2 = up.topk(2, dim=1).values
        near = top2[:, 0] - top2[:, 1] < NEAR
    else:
        near = torch.zeros(up[:, 0].shape, dtype=torch.bool)
    return up.argmax(1), near


F64_SHAPES = [s for s in SHAPES if s[0] in ("x8", "non_integer")] + [("c4_one_image", 256, 512, 1024, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", F64_SHAPES, ids=[s[0] for s in F64_SHAPES])
def test_export_vs_float64(shape, parity_log):
    """Every pixel whose exported class differs from the float64 argmax is a near-tie pixel (float64 top-two margin < NEAR), and the
    inputs keep the share of such pixels within test_seg_eval's cap max(4, 0.002 n).  The float64 reference alone measures shares
    of 3.5e-4, 4.4e-4 and 3.5e-4 at these three shapes with this generator."""
    tag, h, w, H, W = shape
    K, C = 20, 19
    rng = np.random.default_rng(K * 1000 + h)
    B = 2 if h < 256 else 1
    nhwc = _dirichlet(rng, B, h, w, K)
    pred = nhwc.permute(0, 3, 1, 2)
    want, near = _ref64_classes(pred, (H, W), C)
    got = _export(pred.cuda(), (H, W), K, outputs=("train_id",))["train_id"].cpu().long()
    wrong = got != want
    n, n_near, n_wrong = want.numel(), int(near.sum()), int(wrong.sum())
    parity_log(f"seg_export[{tag}]", pixels=n, near=n_near, mismatches=n_wrong, mismatches_off_near=int((wrong & ~near).sum()))
    print(f"seg_export[{tag}]: pixels={n} near={n_near} mismatches={n_wrong}")
    assert n_near <= max(4, 0.002 * n), (tag, n_near, n)
    assert not bool((wrong & ~near).any()), (tag, int((wrong & ~near).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 20])
def test_export_exact_ties_go_to_the_lower_class(K):
    """test_kernel_tied_and_peaked_rows' tied rows: the two top classes hold the same value over an image, so their interpolated
    values tie exactly and the lower index wins, as in the float64 argmax."""
    rng = np.random.default_rng(K)
    B, h, w, H, W = 2, 12, 20, 50, 70
    C = K - 1
    tied = rng.dirichlet(np.ones(K - 2), (B, h, w)).astype(np.float32) * np.float32(0.1)
    top = rng.integers(0, C - 1, B)
    tied = np.stack([np.insert(tied[b], [top[b], top[b]], np.float32(0.45), axis=2) for b in range(B)])
    pred = torch.from_numpy(tied).permute(0, 3, 1, 2)
    got = _export(pred.cuda(), (H, W), K, outputs=("train_id",))["train_id"].cpu().long()
    want, _ = _ref64_classes(pred, (H, W), C)
    assert torch.equal(got, want)
    for b in range(B):
        assert torch.all(got[b] == int(top[b]))
    # the ignore channel is dropped before the argmax: all the mass there gives class 0
    only_ignore = torch.zeros((1, K, 6, 6))
    only_ignore[:, K - 1] = 1
    assert int(_export(only_ignore.cuda(), (24, 24), K, outputs=("train_id",))["train_id"].max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in EXPORT_SHAPES if s[0] in ("non_integer", "w_mod4", "x8")], ids=["x8", "non_integer", "w_mod4"])
def test_export_writes_only_requested_outputs(shape):
    """Every non-empty subset of outputs, written into views of poisoned buffers with one guard byte on each side: the requested
    maps equal the all-outputs call, the guard bytes and the buffers not requested keep the poison."""
    tag, h, w, H, W = shape
    K = 20
    rng = np.random.default_rng(11)
    B = 2
    probs = _dirichlet(rng, B, h, w, K).cuda()
    ids, col = _tables(K)
    idt, colt = torch.from_numpy(ids).cuda(), torch.from_numpy(col).reshape(-1).cuda()
    full = _export(probs.permute(0, 3, 1, 2), (H, W), K)
    names = ("train_id", "label_id", "color")
    sizes = {"train_id": B * H * W, "label_id": B * H * W, "color": B * H * W * 3}
    lib = hip.load()
    POISON = 0xA5
    for r in (1, 2, 3):
        for subset in itertools.combinations(names, r):
            bufs = {n: torch.full((sizes[n] + 2,), POISON, dtype=torch.uint8, device="cuda") for n in names}
            ptr = {n: bufs[n].data_ptr() + 1 if n in subset else None for n in names}
            hip.check(lib.ccdm_segexport(probs.data_ptr(), K, None, B, h, w, H, W, K, K - 1, idt.data_ptr(), colt.data_ptr(), ptr["train_id"],
                                         ptr["label_id"], ptr["color"], torch.cuda.current_stream().cuda_stream), "segexport")
            torch.cuda.synchronize()
            for n in names:
                if n in subset:
                    assert int(bufs[n][0]) == POISON and int(bufs[n][-1]) == POISON, (subset, n)
                    assert torch.equal(bufs[n][1:-1], full[n].reshape(-1)), (subset, n)
                else:
                    assert bool((bufs[n] == POISON).all()), (subset, n)
    # the host function returns exactly what was asked for
    for subset in (("color",), ("train_id", "color"), ("label_id",)):
        out = _export(probs.permute(0, 3, 1, 2), (H, W), K, outputs=subset)
        assert tuple(sorted(out)) == tuple(sorted(subset))
        for n in subset:
            assert torch.equal(out[n], full[n])


@pytest.mark.gpu
def test_export_entry_point_refuses_bad_arguments():
    lib = hip.load()
    K, B, h, w, H, W = 20, 1, 4, 4, 8, 8
    probs = torch.zeros((B, h, w, K), device="cuda")
    cls = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    idt = torch.zeros(K, dtype=torch.uint8, device="cuda")
    colt = torch.zeros(3 * K, dtype=torch.uint8, device="cuda")
    out = torch.zeros(B * H * W, dtype=torch.uint8, device="cuda")

    def call(p, ps, c, k, scored, o, b=B):
        return lib.ccdm_segexport(p, ps, c, b, h, w, H, W, k, scored, idt.data_ptr(), colt.data_ptr(), o, None, None, None)
    assert call(probs.data_ptr(), K, None, K, K - 1, out.data_ptr()) == 0
    assert call(probs.data_ptr(), K, cls.data_ptr(), K, K - 1, out.data_ptr()) < 0 and "exactly one" in hip.last_error()
    assert call(None, 0, None, K, K - 1, out.data_ptr()) < 0
    assert call(probs.data_ptr(), K, None, 33, 32, out.data_ptr()) < 0
    assert call(probs.data_ptr(), K, None, 1, 1, out.data_ptr()) < 0
    assert call(probs.data_ptr(), K, None, K, K - 2, out.data_ptr()) < 0 and "scored" in hip.last_error()
    assert call(probs.data_ptr(), K - 1, None, K, K - 1, out.data_ptr()) < 0 and "pixel_stride" in hip.last_error()
    assert call(probs.data_ptr(), K, None, K, K - 1, None) < 0 and "no output" in hip.last_error()
    assert call(probs.data_ptr(), K, None, K, K - 1, None, b=0) < 0                   # checked before the B = 0 return
    assert call(probs.data_ptr(), K, None, K, K - 1, out.data_ptr(), b=0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="tables"):
        SEG.export_predictions(torch.zeros((1, 5, 4, 4), device="cuda"), (8, 8))


@pytest.mark.gpu
def test_export_labels_maps_ignore_and_out_of_range_to_id_0():
    rng = np.random.default_rng(4)
    B, H, W = 2, 37, 53
    lab = torch.from_numpy(rng.integers(0, 19, (B, H, W)))
    lab[0, 0, :6] = torch.tensor([19, 255, 20, -1, 1000, 18])
    lab[1, 5] = 255
    out = SEG.export_labels(lab.cuda(), outputs=("train_id", "label_id", "color"))
    train = torch.where((lab < 0) | (lab > 19), torch.full_like(lab, 19), lab)
    np.testing.assert_array_equal(out["train_id"].cpu().numpy(), train.numpy())
    np.testing.assert_array_equal(out["label_id"].cpu().numpy(), np.array(SEG.TRAIN_ID_TO_ID, np.uint8)[train.numpy()])
    np.testing.assert_array_equal(out["color"].cpu().numpy(), np.array(SEG.TRAIN_ID_TO_COLOR, np.uint8)[train.numpy()])
    assert out["label_id"][0, 0, :6].tolist() == [0, 0, 0, 0, 0, 33]
    assert bool((out["label_id"][1, 5] == 0).all())
    assert tuple(SEG.export_labels(lab.to(torch.uint8).cuda())) == ("label_id",)
    # read back through the evaluator's lookup, the label image gives the train ids again
    back = SEG.id_to_train_id_lut()[out["label_id"].cpu().numpy()]
    np.testing.assert_array_equal(back, train.numpy())


@pytest.mark.gpu
def test_export_c4_shape_deterministic_and_lean():
    """Two calls are byte-identical, and a call allocates less than one full-resolution fp32 channel (B H W 4 bytes) above its
    inputs and outputs: nothing of the upsampled probabilities is ever stored (the torch path needs K such channels)."""
    pred, lab = _c4_inputs()
    B, H, W = 16, 1024, 2048
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    one = SEG.export_predictions(pred, (H, W), outputs=("train_id", "label_id", "color"))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = sum(v.numel() for v in one.values())
    assert outputs == B * H * W * 5
    print(f"seg_export C4: peak above inputs = {peak} bytes, outputs = {outputs} bytes")
    assert peak - outputs < B * H * W * 4, (peak, outputs)
    two = SEG.export_predictions(pred, (H, W), outputs=("train_id", "label_id", "color"))
    for n in one:
        assert torch.equal(one[n], two[n]), n
    sc = SEG.SegmentationConfusion(20, "cuda")
    sc.update(pred, lab)
    assert torch.equal(ignite_confusion(one["train_id"], lab, 19).cpu(), sc.confusion)
    t = one["train_id"].long()
    assert torch.equal(one["label_id"], torch.tensor(SEG.TRAIN_ID_TO_ID, dtype=torch.uint8, device="cuda")[t])
    assert torch.equal(one["color"], torch.tensor(SEG.TRAIN_ID_TO_COLOR, dtype=torch.uint8, device="cuda")[t])


# ------------------------------------------------------------------------------------------------ GPU: evaluator
@pytest.mark.gpu
@pytest.mark.parametrize("evaluations", [1, 3])
@pytest.mark.parametrize("resolution", ["original", "dataloader"])
def test_eval_segmentation_saves_predictions(resolution, evaluations, tmp_path):
    from PIL import Image
    vote = "confidence"
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    params = dict(_params(resolution, evaluations, vote), output_path=str(tmp_path / "run"))
    plain = SEG.eval_segmentation(params, dataset=ds, model=Recorder(_k20_model(vote)))
    assert "pred_list" not in plain and not os.path.exists(tmp_path / "run")
    params["evaluation"] = dict(params["evaluation"], save_predictions=True)
    rec = Recorder(_k20_model(vote))
    res = SEG.eval_segmentation(params, dataset=ds, model=rec)
    assert len(rec.preds) == 2                                              # no second sampling pass
    assert res["mIoU"] == plain["mIoU"] and res["confusion"] == plain["confusion"] and res["IoU"] == plain["IoU"]
    base = tmp_path / "run" / "outputs" / "val"
    assert res["pred_list"] == [str(base / "submit" / f"{n}_id.png") for n in (1, 2, 3)]
    assert res["label_list"] == [str(base / "label" / f"{n}_label.png") for n in (1, 2, 3)]
    size = (48, 80) if resolution == "original" else (32, 32)
    lut = SEG.id_to_train_id_lut()
    color = np.array(SEG.TRAIN_ID_TO_COLOR, np.uint8)
    cm = torch.zeros((19, 19), dtype=torch.int64)
    for n, (fp, fl) in enumerate(zip(res["pred_list"], res["label_list"]), start=1):
        with Image.open(fp) as im:
            assert im.mode == "L" and im.size == (size[1], size[0])
            pid = np.asarray(im)
        with Image.open(fl) as im:
            assert im.mode == "L" and im.size == (size[1], size[0])
            lid = np.asarray(im)
        with Image.open(base / "debug" / f"{n}_rgb.png") as im:
            assert im.mode == "RGB"
            rgb = np.asarray(im)
        pt, lt = lut[pid], lut[lid]
        assert pt.max() < 19                                                # a prediction is never the ignore class
        np.testing.assert_array_equal(rgb, color[pt])
        want = ds[n - 1][2] if resolution == "original" else ds[n - 1][1].argmax(0)
        np.testing.assert_array_equal(lt, np.where((want.numpy() < 0) | (want.numpy() > 18), 19, want.numpy()))
        cm += ignite_confusion(torch.from_numpy(pt.astype(np.int64)), torch.from_numpy(lt.astype(np.int64)), 19)
    assert torch.equal(cm, torch.tensor(res["confusion"]))
