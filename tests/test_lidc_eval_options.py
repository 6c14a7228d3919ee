"""The optional scores of eval_lidc_uncertainty as one table (evaluation.LIDC_SCORES, with `label_bound` beside it): an option that is off
looks at none of its settings, one that is on checks all of them before the first sampling call, and the options do not see each other:
with every one on, each result is the one the option gives alone.  The scores themselves are held against their restatements in the
tests of each option; here a stub model with fixed predictions goes through the evaluator."""
import json
import os

import numpy as np
import pytest
import torch

from ccdm_stochastic_segmentation_amd import evaluation as E
from ccdm_stochastic_segmentation_amd import metrics as M

ORDER = ["soft_labels", "surface_distances", "lesions", "lesion_matching", "detection", "modes", "consensus", "label_bound"]
# per option a value every one of its settings refuses
BAD = {"soft_labels": {"soft_label_bins": 0, "soft_label_thresholds": [0.0]},
       "surface_distances": {"surface_distance_percentile": 0},
       "lesions": {"lesion_connectivity": 6, "lesion_overlaps": [1.5]},
       "lesion_matching": {"lesion_connectivity": 6, "lesion_match_ious": [0.4], "lesion_min_size": 0},
       "detection": {"lesion_connectivity": 6, "detection_min_frequency": 2, "detection_rater_agreement": 5, "detection_score": "mass",
                     "detection_fp_rates": [-1], "detection_max_candidates": 0},
       "modes": {"mode_count": 0, "mode_max_swaps": -1},
       "consensus": {"consensus_metric": "f1"}}
EVALUATIONS, BATCH, IMAGES, RATERS, TIMESTEPS = [2, 3], 2, 3, 4, 3


def stub_case(K, H, W, seed=5):
    """(dataset, model factory): IMAGES images with RATERS annotations each, and a model whose predictions are fixed one-hot maps, which
    counts its sampling calls and answers label_bound with fixed arrays of the shapes DenoisingModel.label_bound documents."""
    S = max(EVALUATIONS)
    rng = np.random.default_rng(seed)
    samples, raters = rng.integers(0, K, (IMAGES, S, H, W)), rng.integers(0, K, (IMAGES, RATERS, H, W))
    one_hot = lambda idx: torch.nn.functional.one_hot(torch.from_numpy(idx.astype(np.int64)), K).movedim(-1, -3).float()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return IMAGES

        def __getitem__(self, b):
            return torch.full((1, H, W), float(b)), one_hot(raters[b]), np.array([1.0 / RATERS] * RATERS)

    class Fake:
        step_T_sample = "majority"
        calls = 0

        def __call__(self, x, image, **kw):
            first = self.calls * BATCH
            self.calls += 1
            return {"diffusion_out": one_hot(samples[first:first + x.shape[0] // S]).reshape(x.shape[0], K, H, W).to(x.device)}

        def label_bound(self, labels, condition, timesteps=None, draws=1):
            B = labels.shape[0]
            base = condition[:, 0, 0, 0].double()[:, None] + torch.arange(RATERS, device=condition.device).double()[None]      # image + rater
            return {"bound": base * 10, "bits_per_pixel": base / 4, "terms": base[..., None].expand(B, RATERS, TIMESTEPS).clone(),
                    "timesteps": torch.arange(1, TIMESTEPS + 1).expand(B, RATERS, TIMESTEPS), "prior": base * 0 + 0.5,
                    "pixels": torch.full((B, RATERS), H * W), "complete": True}
    return DS(), Fake


def numpy_pair_counts(a, b, num_classes):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    out = np.zeros((a.shape[0], a.shape[1], b.shape[1], num_classes, 2), dtype=np.int32)
    for k in range(num_classes):
        x, y = (a == k)[:, :, None], (b == k)[:, None, :]
        out[..., k, 0], out[..., k, 1] = (x & y).sum(axis=(3, 4)), (x | y).sum(axis=(3, 4))
    return out


@pytest.mark.parametrize("key", ORDER[:-1])
def test_an_option_reads_its_settings_only_when_on(key, monkeypatch):
    assert [option.key for option in E.LIDC_SCORES] == ORDER[:-1] == list(BAD)
    monkeypatch.setattr(M, "pairwise_class_counts", numpy_pair_counts)
    ds, fake = stub_case(2, 9, 7)
    params = {"dataset_file": "datasets.lidc", "batch_size": BATCH, "evaluations": EVALUATIONS, "output_path": None}
    plain = E.eval_lidc_uncertainty(dict(params), dataset=ds, device="cpu", model=fake())
    off = E.eval_lidc_uncertainty({**params, "evaluation": {key: False, **BAD[key]}}, dataset=ds, device="cpu", model=fake())
    assert json.dumps(off) == json.dumps(plain)
    for setting, value in BAD[key].items():
        model = fake()
        with pytest.raises(ValueError, match=setting):
            E.eval_lidc_uncertainty({**params, "evaluation": {key: True, setting: value}}, dataset=ds, device="cpu", model=model)
        assert model.calls == 0
    doc = E.eval_lidc_uncertainty.__doc__
    for word in (f"{key}: yes", f'"{key}"', f"lidc_{key}.json", *BAD[key]):
        assert word in doc, word


def options_alone_and_together(out_dir, K, H, W, keys):
    ds, fake = stub_case(K, H, W)
    params = {"dataset_file": "datasets.lidc", "batch_size": BATCH, "evaluations": EVALUATIONS, "output_path": None}
    run = lambda **kw: E.eval_lidc_uncertainty({**params, **kw}, dataset=ds, device="cuda:0", model=fake())
    plain = run()
    together = run(evaluation={key: True for key in reversed(keys)}, output_path=str(out_dir))      # (the section's own order does not matter)
    assert [key for key in together if key not in plain] == keys
    assert json.dumps({key: together[key] for key in plain}) == json.dumps(plain)
    for key in keys:
        alone = run(evaluation={key: True})
        assert list(alone) == list(plain) + [key]
        assert json.dumps(together[key]) == json.dumps(alone[key]), key
        if key != "label_bound":
            assert [r["samples"] for r in together[key]] == EVALUATIONS and all(r["images"] == IMAGES for r in together[key]), key
        with open(out_dir / f"lidc_{key}.json") as f:
            assert json.load(f) == together[key], key
    assert sorted(os.listdir(out_dir)) == sorted(f"lidc_{key}.json" for key in keys)
    return together


@pytest.mark.gpu
def test_every_option_on_at_once(tmp_path):
    """three images in batches of two, so the ragged last batch goes through every concatenation; 9x7 maps: narrower than a wave, the width
    no multiple of four"""
    together = options_alone_and_together(tmp_path / "out", 2, 9, 7, ORDER)
    assert together["label_bound"]["images"] == IMAGES and together["label_bound"]["timesteps"] == list(range(1, TIMESTEPS + 1))


@pytest.mark.gpu
def test_two_scored_classes_on_aligned_maps(tmp_path):
    """K = 3 on 8x8 maps (the dword path): the per-class lists hold two scored classes"""
    keys = ["surface_distances", "lesions", "lesion_matching", "detection"]
    together = options_alone_and_together(tmp_path / "out", 3, 8, 8, keys)
    for key in keys:
        assert all(r["classes"] == [1, 2] for r in together[key]), key
