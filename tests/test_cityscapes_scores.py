"""The official Cityscapes script's scores from device counts: the ccdm_csscore kernel (fused and ids form), CityscapesScores, the
fp64 restatement of the script's formulas (scores_from_counts) and `evaluation.cityscapes_script` of eval_segmentation.

The golden (tests/golden/cs_script_inputs.npz, cs_script_results.json; tools/gen_goldens_cs_script.py) is what the reference's
vendored script returns on a small set of images, with instance-level scoring off (the reference's setting) and on.  Counts are
compared exactly against numpy (bincount for the matrix, per-id bincounts for the instances), floats with relative 1e-12: each is
a quotient of exact integers or of fp64 sums of a few hundred terms added in the script's order, so equality is expected and
1e-12 only absorbs a differently associated sum (n * 2^-53, n < 1000)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import cityscapes_scores as CS
from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd import segmentation as SEG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "cs_script_results.json")))
RTOL = 1e-12
L = 34
# the script's tables as the golden holds them (read from the reference), not the module's
G_IGN = np.array([r[5] for r in GOLD["labels"] if r[1] >= 0], bool)
G_CAT = np.array([GOLD["categories"].index(r[3]) for r in GOLD["labels"] if r[1] >= 0])
FLOAT_DICTS = ("priors", "classScores", "classInstScores", "categoryScores", "categoryInstScores")
AVERAGES = ("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories")


def golden_inputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "cs_script_inputs.npz"))
    return [(z[f"pred_ids_{g}"], z[f"gt_ids_{g}"], z[f"inst_ids_{g}"]) for g in ("a", "b")]


def np_counts(pred, gt, inst=None, first=0):
    """numpy counts of one batch: (conf [L,L], per_image [B][4], instances [(image, id, size, tp, category tp)])."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    conf = np.bincount((gt * L + pred).ravel(), minlength=L * L).reshape(L, L)
    ign = G_IGN[gt]
    per_image = [[int(ign[b].sum()), int((ign[b] & (pred[b] != gt[b])).sum()), int((~ign[b]).sum()),
                  int((~ign[b] & (pred[b] == gt[b])).sum())] for b in range(gt.shape[0])]
    instances = []
    if inst is not None:
        inst = np.asarray(inst).astype(np.int64)
        for b in range(gt.shape[0]):
            i, p = inst[b].ravel(), pred[b].ravel()
            lab = i // 1000
            size = np.bincount(i, minlength=65536)
            tp = np.bincount(i[p == lab], minlength=65536)
            ct = np.bincount(i[G_CAT[p] == G_CAT[np.minimum(lab, L - 1)]], minlength=65536)
            for iid in np.unique(i[i > 1000]):
                if not G_IGN[iid // 1000]:
                    instances.append((first + b, int(iid), int(size[iid]), int(tp[iid]), int(ct[iid])))
    return conf, per_image, instances


def same_float(a, b):
    a = float("nan") if a is None else a
    b = float("nan") if b is None else b
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= RTOL * abs(b)


def assert_result(ours, gold, names=None):
    """`ours` against a golden result dictionary: integers, key sets, the key order of `labels` and NaN positions exactly, floats to
    RTOL.  names[i]: our perImageScores key of the golden's image i."""
    assert set(ours) == set(gold)
    assert ours["confMatrix"] == gold["confMatrix"]
    assert list(ours["labels"].items()) == list(gold["labels"].items())
    for k in FLOAT_DICTS:
        assert list(ours[k]) == list(gold[k]), k
        for n in gold[k]:
            assert same_float(ours[k][n], gold[k][n]), (k, n, ours[k][n], gold[k][n])
    for k in AVERAGES:
        assert same_float(ours[k], gold[k]), (k, ours[k], gold[k])
    assert len(ours["perImageScores"]) == len(gold["perImageScores"])
    for i, want in gold["perImageScores"].items():
        got = ours["perImageScores"][names[int(i)] if names is not None else int(i)]
        assert set(got) == set(want) | {"nbEvaluatedPixels", "nbEvaluatedCorrectPixels"}
        assert all(got[f] == v for f, v in want.items()), (i, got, want)


def numpy_result(with_instances):
    conf, per_image, instances = np.zeros((L, L), np.int64), [], []
    for pred, gt, inst in golden_inputs():
        c, p, i = np_counts(pred, gt, inst if with_instances else None, first=len(per_image))
        conf, per_image, instances = conf + c, per_image + p, instances + i
    return conf, per_image, instances


# ------------------------------------------------------------------------------------------------ CPU
def test_label_tables_match_golden():
    # (license plate, id -1, never in an image: the reference's labels.py gives it train id -1, its cityscapes_config.py 255, which
    # segmentation.CITYSCAPES_LABELS is pinned to; both mean "no train id")
    assert [list(r) for r in CS.CS_LABELS] == [r[:2] + [255 if r[2] == -1 else r[2]] + r[3:] for r in GOLD["labels"]]
    assert list(CS.CATEGORIES) == GOLD["categories"]
    assert CS.AVG_CLASS_SIZE == GOLD["avgClassSize"]
    names, ign, cat, has, cats = CS.label_tables()
    assert len(names) == CS.NUM_LABELS == L and cats == GOLD["categories"]
    assert ign.tolist() == G_IGN.astype(int).tolist() and cat.tolist() == G_CAT.tolist()
    things = [r[1] for r in GOLD["labels"] if r[4]]
    assert has.nonzero()[0].tolist() == things == list(range(24, 34))
    assert CS.INSTANCE_BASE == 1000 * min(things) and CS.INSTANCE_BASE + CS.INSTANCE_SLOTS == 1000 * (max(things) + 1)
    assert L <= hip.CSSCORE_MAX_LABELS


@pytest.mark.parametrize("setting", ["pixel", "instance"])
def test_formulas_on_numpy_counts_equal_the_script(setting):
    conf, per_image, instances = numpy_result(setting == "instance")
    assert conf.sum() == sum(p.size for p, _, _ in golden_inputs())
    assert (len(instances) > 0) == (setting == "instance")
    assert_result(CS.scores_from_counts(conf, per_image, instances), GOLD[setting])
    if setting == "instance":          # the golden covers a missed instance, a skipped one, and the 0 / NaN pair of thing classes
        assert any(tp == 0 for _, _, _, tp, _ in instances) and not any(i // 1000 in (29, 30) for _, i, _, _, _ in instances)
        assert sum(1 for _, i, _, _, _ in instances if i == 24001) == 3
        inst = GOLD[setting]["classInstScores"]
        assert inst["train"] is None and inst["motorcycle"] == 0.0 and inst["person"] > 0


def test_per_image_fields_reproduce_the_inverted_counts():
    """The script's nbNotIgnoredPixels / nbCorrectPixels count the IGNORED pixels and the mismatches among them (its np.in1d(...,
    invert=True)); the two extra fields are the evaluated pixels and the correct ones among them."""
    conf, per_image, _ = numpy_result(False)
    res = CS.scores_from_counts(conf, per_image, [])
    n = 0
    for pred, gt, _ in golden_inputs():
        for b in range(gt.shape[0]):
            ignored = ~np.isin(gt[b], [r[1] for r in GOLD["labels"] if not r[5]])
            got = res["perImageScores"][n]
            assert got["nbNotIgnoredPixels"] == ignored.sum() == GOLD["pixel"]["perImageScores"][str(n)]["nbNotIgnoredPixels"]
            assert got["nbCorrectPixels"] == (ignored & (pred[b] != gt[b])).sum()
            assert got["nbEvaluatedPixels"] == (~ignored).sum() == gt[b].size - got["nbNotIgnoredPixels"]
            assert got["nbEvaluatedCorrectPixels"] == (~ignored & (pred[b] == gt[b])).sum() > 0
            n += 1
    named = CS.scores_from_counts(conf, per_image, [], names=["x", "y", "z"])
    assert list(named["perImageScores"]) == ["x", "y", "z"] and named["perImageScores"]["y"] == res["perImageScores"][1]


def test_formulas_hand_made():
    conf = np.zeros((L, L), np.int64)
    conf[7, 7], conf[7, 8], conf[8, 7], conf[8, 8], conf[0, 7], conf[26, 26], conf[26, 7] = 6, 2, 1, 3, 50, 10, 5
    res = CS.scores_from_counts(conf, [], [(0, 26001, 10, 8, 9), (0, 26002, 5, 2, 2), (0, 29001, 4, 0, 0)])
    assert res["classScores"]["road"] == 6 / (6 + 2 + 1 + 5)            # the ignored row (unlabeled) gives no false positive
    assert res["classScores"]["sidewalk"] == 3 / (3 + 1 + 2) and math.isnan(res["classScores"]["unlabeled"])
    assert math.isnan(res["classScores"]["sky"]) and res["categoryScores"]["flat"] == 12 / (12 + 5)
    w1, w2 = CS.AVG_CLASS_SIZE["car"] / 10.0, CS.AVG_CLASS_SIZE["car"] / 5.0
    tp, fn = 8.0 * w1 + 2.0 * w2, 2.0 * w1 + 3.0 * w2
    assert res["classInstScores"]["car"] == tp / (tp + 0 + fn)
    ctp, cfn = 9.0 * w1 + 2.0 * w2, 1.0 * w1 + 3.0 * w2
    assert res["categoryInstScores"]["vehicle"] == ctp / (ctp + 0 + cfn)
    assert res["priors"]["unlabeled"] == 50 / 77 and "perImageScores" not in res
    assert res["averageScoreClasses"] == (res["classScores"]["road"] + res["classScores"]["sidewalk"] + res["classScores"]["car"]) / 3
    with pytest.raises(ValueError, match="no instances"):
        CS.scores_from_counts(conf, [], [(0, 7001, 3, 1, 1)])


def test_instances_need_the_original_resolution(tmp_path):
    params = {"dataset_file": "synthetic.cityscapes_miou", "batch_size": 2, "mp_loaders": 0, "output_path": str(tmp_path),
              "evaluation": {"resolution": "dataloader", "cityscapes_script": True, "cityscapes_script_instances": True}}
    with pytest.raises(ValueError, match="resolution: original"):
        SEG.eval_segmentation(params, device="cpu", model=object())
    del params["evaluation"]["resolution"]
    with pytest.raises(ValueError, match="resolution: original"):
        SEG.eval_segmentation(params, device="cpu", model=object())
    params["evaluation"] = {"resolution": "original", "cityscapes_script": True, "cityscapes_script_instances": True}
    with pytest.raises(ValueError, match="no instance image"):
        SEG.eval_segmentation(params, dataset=SEG.SyntheticCityscapes(size=2), device="cpu", model=object())


def test_synthetic_instances_are_a_fourth_item():
    plain = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2)
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2, instances=True)
    found = 0
    for i in range(3):
        assert len(plain[i]) == 3 and len(ds[i]) == 4
        for a, b in zip(plain[i], ds[i]):
            assert torch.equal(a, b)
        lab, inst = ds[i][2].numpy(), ds[i][3].numpy()
        assert inst.dtype == np.int32 and inst.shape == lab.shape
        ids = np.array(SEG.TRAIN_ID_TO_ID)[np.where((lab < 0) | (lab > 19), 19, lab)]
        big = inst > 1000
        np.testing.assert_array_equal(inst[~big], ids[~big])
        np.testing.assert_array_equal(inst[big] // 1000, ids[big])
        assert (ids[big] >= 24).all()
        found += len(np.unique(inst[big]))
    assert found >= 2
    p = {"dataset_file": "synthetic.cityscapes_miou", "evaluation": {"cityscapes_script_instances": True}}
    assert len(SEG.make_segmentation_dataset(p)[0]) == 4 and len(SEG.make_segmentation_dataset({"dataset_file": "synthetic.x"})[0]) == 3


def test_cityscapes_reader_returns_instances(tmp_path):
    from PIL import Image
    from tests.test_seg_eval import _write_tree
    files = [("aachen", "aachen_000000_000019"), ("bremen", "bremen_000000_000019")]
    _write_tree(str(tmp_path), "val", files)
    with pytest.raises(FileNotFoundError, match="instanceIds"):
        SEG.CityscapesVal(str(tmp_path), "val", target_size=(12, 16), return_instances=True)
    rng = np.random.default_rng(3)
    want = {}
    for city, stem in files:
        inst = rng.integers(0, 34000, (24, 40)).astype(np.uint16)
        Image.fromarray(inst).save(os.path.join(str(tmp_path), "gtFine", "val", city, stem + "_gtFine_instanceIds.png"))
        want[stem] = inst
    ds = SEG.CityscapesVal(str(tmp_path), "val", target_size=(12, 16), return_instances=True)
    plain = SEG.CityscapesVal(str(tmp_path), "val", target_size=(12, 16))
    for i, (_, stem) in enumerate(files):
        assert len(plain[i]) == 3 and len(ds[i]) == 4 and ds[i][3].dtype == torch.int32
        np.testing.assert_array_equal(ds[i][3].numpy(), want[stem])
        assert torch.equal(ds[i][2], plain[i][2])


def test_csscore_symbols_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ccdm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ccdm_csscore[a-z0-9_]*)\s*\(", hdr))
    assert declared == {"ccdm_csscore", "ccdm_csscore_ids"} == {k for k in hip.SIGNATURES if k.startswith("ccdm_css")}
    assert not any(k.startswith("ccdm_seg_") for k in declared)
    assert len(hip.SIGNATURES["ccdm_csscore"][1]) == 23 and len(hip.SIGNATURES["ccdm_csscore_ids"][1]) == 17
    assert "ccdm_csscore.hip" in hip.SOURCES and hip.ABI_VERSION == 11
    assert re.search(r"#define\s+CCDM_CSSCORE_MAX_LABELS\s+%d\b" % hip.CSSCORE_MAX_LABELS, hdr)
    lib = hip.load()
    assert hasattr(lib, "ccdm_csscore") and hasattr(lib, "ccdm_csscore_ids")


# ------------------------------------------------------------------------------------------------ GPU: kernel
def _targets(rng, B, H, W, ids=None):
    """Blocky ground truth over the label ids and an instance image as Cityscapes writes it: a cell of a label with instances is
    instance label * 1000 + (0..6), so ids repeat over disjoint cells; some stay plain; caravan / trailer instances occur."""
    ids = np.arange(L) if ids is None else np.asarray(ids)
    gh, gw = H // 8 + 1, W // 8 + 1
    cell = ids[rng.integers(0, len(ids), (B, gh, gw))]
    num = rng.integers(0, 9, (B, gh, gw))
    up = lambda a: a[:, np.arange(H) // 8][:, :, np.arange(W) // 8]      # noqa: E731
    inst = np.where((cell >= 24) & (num < 7), cell * 1000 + num, cell)
    return np.ascontiguousarray(up(cell), dtype=np.uint8), np.ascontiguousarray(up(inst), dtype=np.int32)


def _scores_equal(sc, conf, per_image, instances):
    assert torch.equal(sc.conf, torch.from_numpy(conf))
    assert sc.per_image == per_image
    assert sc.instances == instances


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["pixel", "instance"])
def test_ids_form_on_the_golden(setting):
    sc = CS.CityscapesScores(20, "cuda")
    for pred, gt, inst in golden_inputs():
        sc.update_ids(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(inst.astype(np.int32)) if setting == "instance" else None)
    _scores_equal(sc, *numpy_result(setting == "instance"))
    assert_result(sc.result(), GOLD[setting])


FUSED_SHAPES = [("identity", 40, 56, 40, 56), ("x2", 36, 48, 72, 96), ("x4", 16, 24, 64, 96), ("non_integer", 30, 50, 97, 211),
                ("w_mod4", 20, 33, 70, 90)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["probs", "class_map"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=[s[0] for s in FUSED_SHAPES])
def test_fused_form_equals_ids_form_on_the_exported_image(shape, form):
    tag, h, w, H, W = shape
    rng = np.random.default_rng(h * 1000 + W)
    B, K = 3, 20
    if form == "probs":
        pred = torch.from_numpy(rng.dirichlet(np.ones(K), (B, h, w)).astype(np.float32)).permute(0, 3, 1, 2).cuda()
    else:
        pred = torch.from_numpy(rng.integers(0, K, (B, h, w))).cuda()
    gt, inst = _targets(rng, B, H, W)
    label_id = SEG.export_predictions(pred, (H, W), outputs=("label_id",), num_classes=K)["label_id"]
    for with_inst in (False, True):
        i = torch.from_numpy(inst) if with_inst else None
        fused, ids = CS.CityscapesScores(K, "cuda"), CS.CityscapesScores(K, "cuda")
        fused.update(pred, torch.from_numpy(gt), i)
        ids.update_ids(label_id, torch.from_numpy(gt), i)
        want = np_counts(label_id.cpu().numpy(), gt, inst if with_inst else None)
        _scores_equal(ids, *want)
        _scores_equal(fused, *want)
        assert int(fused.conf.sum()) == B * H * W
        if with_inst:
            assert len(want[2]) > 5


def _raw(lib, fn, pred, gt, inst, conf, per_image, instances, unknown, B=None, K=20):
    """one call of the C ABI on cuda tensors (pred: ids [B,H,W] for ccdm_csscore_ids, a class map [B,h,w] for ccdm_csscore)"""
    _, ign, cat, has, _ = CS.label_tables()
    tabs = [torch.from_numpy(t).cuda() for t in (np.array(SEG.TRAIN_ID_TO_ID, np.uint8), ign, cat, has)]
    B = gt.shape[0] if B is None else B
    H, W = gt.shape[1:]
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    tail = (ptr(gt), ptr(inst), L, ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), CS.INSTANCE_BASE, CS.INSTANCE_SLOTS, ptr(conf), ptr(per_image),
            ptr(instances), ptr(unknown), None)
    if fn == "ids":
        rc = lib.ccdm_csscore_ids(ptr(pred), B, H, W, *tail)
    else:
        rc = lib.ccdm_csscore(None, 0, ptr(pred), B, pred.shape[1], pred.shape[2], H, W, K, ptr(tabs[0]), *tail)
    torch.cuda.synchronize()
    return rc


def _i16(inst):
    return torch.from_numpy(inst.astype(np.uint16).view(np.int16)).cuda()


@pytest.mark.gpu
def test_accumulation_overwrite_determinism_and_no_ops():
    lib = hip.load()
    rng = np.random.default_rng(11)
    B, H, W = 2, 72, 96
    gt, inst = _targets(rng, B, H, W)
    pred = np.array(SEG.TRAIN_ID_TO_ID[:19], np.uint8)[rng.integers(0, 19, (B, H // 4, W // 4))].repeat(4, 1).repeat(4, 2)
    want_conf, want_pi, want_inst = np_counts(pred, gt, inst)
    d_pred, d_gt, d_inst = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), _i16(inst)
    conf = torch.zeros((L, L), dtype=torch.int64, device="cuda")
    per_image = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    instances = torch.full((B, CS.INSTANCE_SLOTS, 3), 99, dtype=torch.int32, device="cuda")
    unknown = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    assert _raw(lib, "ids", d_pred, d_gt, d_inst, conf, per_image, instances, unknown) == 0
    first = [t.clone() for t in (conf, per_image, instances, unknown)]
    assert torch.equal(conf.cpu(), torch.from_numpy(want_conf)) and per_image.cpu().tolist() == want_pi and unknown.tolist() == [0, 0]
    rows = [(b, CS.INSTANCE_BASE + s) + tuple(instances[b, s].tolist()) for b, s in (instances[:, :, 0] > 0).nonzero().tolist()]
    assert rows == want_inst
    skipped = (instances[:, 5000:7000] == 0).all()                  # caravan / trailer slots stay empty
    assert skipped and ((inst >= 29000) & (inst < 31000)).any()
    # a second identical call: conf accumulates, the rest is overwritten with the same bits
    assert _raw(lib, "ids", d_pred, d_gt, d_inst, conf, per_image, instances, unknown) == 0
    assert torch.equal(conf, 2 * first[0]) and torch.equal(per_image, first[1]) and torch.equal(instances, first[2])
    fresh = torch.zeros_like(conf)
    assert _raw(lib, "ids", d_pred, d_gt, d_inst, fresh, per_image, instances, unknown) == 0
    assert torch.equal(fresh, first[0])                               # two identical calls are bit-identical
    # inst_ids = NULL leaves the instance table untouched (and needs none)
    instances.fill_(42)
    assert _raw(lib, "ids", d_pred, d_gt, None, fresh, per_image, instances, unknown) == 0
    assert (instances == 42).all() and torch.equal(fresh, 2 * first[0]) and torch.equal(per_image, first[1])
    assert _raw(lib, "ids", d_pred, d_gt, None, fresh, per_image, None, unknown) == 0
    # B = 0 is a no-op: nothing is written, nothing is launched
    per_image.fill_(-3)
    unknown.fill_(9)
    before = fresh.clone()
    assert _raw(lib, "ids", d_pred, d_gt, d_inst, fresh, per_image, instances, unknown, B=0) == 0
    cls = torch.zeros((B, 8, 8), dtype=torch.uint8, device="cuda")
    assert _raw(lib, "fused", cls, d_gt, d_inst, fresh, per_image, instances, unknown, B=0) == 0
    assert torch.equal(fresh, before) and (per_image == -3).all() and (instances == 42).all() and unknown.tolist() == [9, 9]
    # argument checks
    assert _raw(lib, "fused", cls, d_gt, None, fresh, per_image, None, unknown, K=33) < 0 and "K=33" in hip.last_error()
    assert _raw(lib, "ids", d_pred, d_gt, d_inst, fresh, per_image, None, unknown) < 0 and "instance" in hip.last_error()
    assert torch.equal(fresh, before)


@pytest.mark.gpu
def test_unknown_ids_raise_and_leave_the_accumulator_alone():
    rng = np.random.default_rng(5)
    gt, inst = _targets(rng, 1, 40, 52)
    pred = torch.from_numpy(rng.integers(0, 20, (1, 10, 13)))
    sc = CS.CityscapesScores(20, "cuda")
    sc.update(pred, torch.from_numpy(gt), torch.from_numpy(inst), names=["first"])
    state = (sc.conf.clone(), list(sc.per_image), list(sc.instances), list(sc.names))
    bad_gt = gt.copy()
    bad_gt[0, 3, 4] = 34
    with pytest.raises(ValueError, match="unknown label"):
        sc.update(pred, torch.from_numpy(bad_gt), torch.from_numpy(inst))
    for bad in (7001, 23999, 34000, 65535):          # a label without instances; ids without a slot
        bad_inst = inst.copy()
        bad_inst[0, 20, 20:23] = bad
        with pytest.raises(ValueError, match="instance ids"):
            sc.update(pred, torch.from_numpy(gt), torch.from_numpy(bad_inst))
    with pytest.raises(ValueError, match="unknown label"):
        sc.update_ids(torch.full((1, 40, 52), 40), torch.from_numpy(gt), torch.from_numpy(inst))
    with pytest.raises(ValueError, match="every update"):
        sc.update(pred, torch.from_numpy(gt), None)
    assert torch.equal(sc.conf, state[0]) and (sc.per_image, sc.instances, sc.names) == state[1:]
    ok = inst.copy()
    ok[0, 20, 20:23] = 1000                            # not above 1000: no instance
    sc.update(pred, torch.from_numpy(gt), torch.from_numpy(ok))
    assert sc.names == ["first", 1] and int(sc.conf.sum()) == 2 * 40 * 52


@pytest.mark.gpu
def test_cityscapes_sized_case():
    """B = 2, 256x512 -> 1024x2048 with synthetic blob instances: 64-bit totals and many blocks per image."""
    B, h, w, H, W, K = 2, 256, 512, 1024, 2048, 20
    rng = np.random.default_rng(2048)
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.rand((B, h, w, K), generator=g, device="cuda") ** 4
    pred = (p / p.sum(-1, keepdim=True)).permute(0, 3, 1, 2)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((B, H, W), np.uint8)
    inst = np.zeros((B, H, W), np.int32)
    for b in range(B):
        gt[b] = np.arange(L)[(yy // 128 * 16 + xx // 128 + b) % L]
        inst[b] = gt[b]
        for j in range(1, 41):
            cy, cx, r, lab = rng.integers(0, H), rng.integers(0, W), rng.integers(10, 200), rng.integers(24, 34)
            m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            gt[b][m], inst[b][m] = lab, lab * 1000 + j % 13          # ids repeat: one instance over several blobs
    sc = CS.CityscapesScores(K, "cuda")
    sc.update(pred, torch.from_numpy(gt), torch.from_numpy(inst))
    label_id = SEG.export_predictions(pred, (H, W), outputs=("label_id",))["label_id"].cpu().numpy()
    want = np_counts(label_id, gt, inst)
    _scores_equal(sc, *want)
    assert int(sc.conf.sum()) == B * H * W and max(n for _, _, n, _, _ in want[2]) > 65536
    again = CS.CityscapesScores(K, "cuda")
    again.update(pred, torch.from_numpy(gt), torch.from_numpy(inst))
    _scores_equal(again, *want)
    res = sc.result()
    assert 0 < res["averageScoreInstClasses"] < 1 and math.isnan(res["classInstScores"]["caravan"])


# ------------------------------------------------------------------------------------------------ GPU: evaluator
def _same_tree(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a):
        return math.isnan(b)
    return a == b


@pytest.mark.gpu
def test_eval_segmentation_scores_like_the_script_on_its_pngs(tmp_path):
    from PIL import Image
    from tests.test_seg_eval import _k20_model, _params
    ds = SEG.SyntheticCityscapes(size=3, resolution=(32, 32), original_size=(48, 80), seed=2, instances=True)
    params = dict(_params("original", 1, "confidence"), output_path=str(tmp_path / "run"))
    plain = SEG.eval_segmentation(params, dataset=ds, model=_k20_model("confidence"))
    assert "cs_script" not in plain and not os.path.exists(tmp_path / "run")
    params["evaluation"] = dict(params["evaluation"], save_predictions=True, cityscapes_script=True, cityscapes_script_instances=True)
    res = SEG.eval_segmentation(params, dataset=ds, model=_k20_model("confidence"))
    assert res["IoU"] == plain["IoU"] and res["confusion"] == plain["confusion"]
    # the host restatement on the PNGs it wrote
    conf, per_image, instances = np.zeros((L, L), np.int64), [], []
    for n, (fp, fl) in enumerate(zip(res["pred_list"], res["label_list"])):
        with Image.open(fp) as im:
            pid = np.asarray(im)[None]
        with Image.open(fl) as im:
            lid = np.asarray(im)[None]
        c, p, i = np_counts(pid, lid, ds[n][3].numpy()[None], first=n)
        conf, per_image, instances = conf + c, per_image + p, instances + i
    want = CS.scores_from_counts(conf, per_image, instances, names=res["pred_list"])
    assert len(instances) >= 2 and _same_tree(res["cs_script"], want)
    assert list(res["cs_script"]["perImageScores"]) == res["pred_list"]
    path = tmp_path / "run" / "cs_script_results.json"
    assert _same_tree(json.load(open(path)), json.loads(json.dumps(want)))
    assert open(path).read() == json.dumps(res["cs_script"], indent=2, sort_keys=True)
    # classScores and the run's IoU list: the same quantity from two kernels
    cm = np.array(res["confusion"])
    for t, name in enumerate(SEG.TRAIN_ID_NAMES):
        score = res["cs_script"]["classScores"][name]
        if cm[t].sum() + cm[:, t].sum() > 0:
            assert abs(score - res["IoU"][t]) <= 1e-12 * abs(res["IoU"][t]), (name, score, res["IoU"][t])
        else:
            assert math.isnan(score) and res["IoU"][t] == 0.0
    occur = [res["IoU"][t] for t in range(19) if cm[t].sum() + cm[:, t].sum() > 0]
    assert abs(res["cs_script"]["averageScoreClasses"] - sum(occur) / len(occur)) <= 1e-12
    # without the writer and without instances: keyed by the image number, the script's pixel-level setting
    params["evaluation"] = dict(params["evaluation"], save_predictions=False, cityscapes_script_instances=False)
    params["output_path"] = str(tmp_path / "run2")
    res2 = SEG.eval_segmentation(params, dataset=ds, model=_k20_model("confidence"))
    want2 = CS.scores_from_counts(conf, per_image, [])
    assert "pred_list" not in res2 and _same_tree(res2["cs_script"], want2) and os.path.exists(tmp_path / "run2" / "cs_script_results.json")
    assert not os.path.exists(tmp_path / "run2" / "outputs")
