"""DINO feature encoder variants: ViT-B/8, the patch-16 models and patch strides below the patch size (overlapping patches,
reference ViTExtractor.patch_vit_resolution / _fix_pos_enc, ddpm/models/dino.py:84-140), and the key-resize kernel
(ccdm_vit_key_resize).  The CPU tests need no device; the GPU tests (-m gpu) compare on synthetic weights against the CPU
restatement in oracle/dino_oracle.py (parity unpinned, as for the ViT-S/8 path)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ccdm_stochastic_segmentation_amd import hip
from ccdm_stochastic_segmentation_amd.dino import VIT_CONFIGS, DinoViT, ViTExtractor, make_synthetic_vit_state_dict, token_grid, vit_param_shapes

LIDC_BP = dict(base_channels=32, channel_mult=None, attention_resolutions=[32, 16, 8], num_heads=1, num_head_channels=32, softmax_output=True)
LIDC_CFG = dict(num_heads=1, num_head_channels=32)
PRECS = [hip.PREC_F32, hip.PREC_F16X3]
PREC_IDS = ["f32", "f16x3"]


# ------------------------------------------------------------------------------------------ host side (no device)
@pytest.mark.parametrize("model,count", [("dino_vits8", 21_670_272), ("dino_vits16", 21_665_664), ("dino_vitb8", 85_807_872),
                                         ("dino_vitb16", 85_798_656)])
def test_parameter_counts(model, count):
    assert sum(int(np.prod(s)) for s in vit_param_shapes(model).values()) == count
    sd = make_synthetic_vit_state_dict(model, 0)
    assert {k: v.shape for k, v in sd.items()} == vit_param_shapes(model)


def test_model_table():
    for name, dim, heads, patch in [("dino_vits8", 384, 6, 8), ("dino_vits16", 384, 6, 16), ("dino_vitb8", 768, 12, 8), ("dino_vitb16", 768, 12, 16)]:
        c = VIT_CONFIGS[name]
        assert (c["dim"], c["heads"], c["patch"], c["depth"], c["mlp_ratio"], c["pretrain_size"]) == (dim, heads, patch, 12, 4, 224)


@pytest.mark.parametrize("H,W,p,s,grid", [(256, 512, 8, 4, (63, 127)), (256, 512, 8, 8, (32, 64)), (224, 224, 16, 16, (14, 14)),
                                          (224, 224, 16, 8, (27, 27)), (64, 96, 16, 4, (13, 21)), (512, 1024, 8, 4, (127, 255)),
                                          (40, 72, 8, 2, (17, 33)), (16, 16, 16, 1, (1, 1))])
def test_token_grid(H, W, p, s, grid):
    assert token_grid(H, W, p, s) == grid
    assert grid == (1 + (H - p) // s, 1 + (W - p) // s)


@pytest.mark.parametrize("H,W,p,s", [(64, 96, 8, 3), (64, 96, 16, 6), (66, 96, 8, 4), (4, 96, 8, 4), (64, 8, 16, 8)])
def test_token_grid_rejects(H, W, p, s):
    with pytest.raises(ValueError):
        token_grid(H, W, p, s)


@pytest.mark.parametrize("model,stride", [("dino_vits8", 3), ("dino_vitb8", 5), ("dino_vits16", 6), ("dino_vitb16", 12), ("dino_vits8", 16)])
def test_stride_must_divide_the_patch(model, stride):
    """ValueError in the constructor, before any device or weight work (device='cpu' would fail later, weights are absent)."""
    with pytest.raises(ValueError, match="divide"):
        ViTExtractor(model, stride, device="cpu")
    with pytest.raises(ValueError, match="divide"):
        DinoViT(model, False, "concat_pixels_concat_features", stride=stride, device="cpu")


@pytest.mark.parametrize("model", ["vit_small_patch8_224", "vit_base_patch16_224", "dino_vitl16"])
def test_unbuilt_model_types(model):
    with pytest.raises(NotImplementedError):
        ViTExtractor(model, 8, device="cpu")


def test_training_the_encoder_stays_out_of_scope():
    with pytest.raises(NotImplementedError):
        DinoViT("dino_vitb8", True, "concat_pixels_concat_features", stride=8, device="cpu")


# ------------------------------------------------------------------------------------------ CPU reference at any stride
def _pos_embed(pos: torch.Tensor, h0: int, w0: int, H: int, W: int) -> torch.Tensor:
    """ViTExtractor._fix_pos_enc's interpolate_pos_encoding (dino.py:93-113): its `w`, `h` are dims 2, 3 of the image."""
    n0, dim = pos.shape[1] - 1, pos.shape[2]
    if h0 * w0 == n0 and H == W:
        return pos
    g = int(math.sqrt(n0))
    grid = F.interpolate(pos[:, 1:].reshape(1, g, g, dim).permute(0, 3, 1, 2), scale_factor=((h0 + 0.1) / g, (w0 + 0.1) / g),
                         mode="bicubic", align_corners=False, recompute_scale_factor=False)
    assert grid.shape[-2:] == (h0, w0)
    return torch.cat([pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, h0 * w0, dim)], 1)


def ref_keys(sd, x, heads, patch, stride, layer=11, size=None):
    """extract_descriptors(x, layer, 'key') of a ViT patched to `stride` (patch_vit_resolution): conv patch embedding at that
    stride, the stride-aware position embedding, blocks 0..layer-1, block `layer`'s keys, bilinear resize to (H//s, W//s)."""
    from oracle import dino_oracle as D
    B, _, H, W = x.shape
    h0, w0 = 1 + (H - patch) // stride, 1 + (W - patch) // stride
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride).flatten(2).transpose(1, 2)
    t = torch.cat([sd["cls_token"].expand(B, -1, -1), t], 1) + _pos_embed(sd["pos_embed"], h0, w0, H, W)
    for i in range(layer):
        t = D.vit_block(sd, i, t, heads)
    C = t.shape[-1]
    k = D.vit_block_qkv(sd, layer, t).reshape(B, -1, 3, heads, C // heads).permute(2, 0, 3, 1, 4)[1][:, :, 1:, :]
    k = k.permute(0, 2, 3, 1).flatten(-2, -1).reshape(B, h0, w0, -1).permute(0, 3, 1, 2)
    return F.interpolate(k, size or (H // stride, W // stride), mode="bilinear")


def _torch_sd(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    hip.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ a. stride == patch
@pytest.mark.gpu
@pytest.mark.parametrize("model,H,W", [("dino_vitb8", 64, 96), ("dino_vitb8", 224, 224), ("dino_vitb8", 40, 72),
                                       ("dino_vits16", 64, 96), ("dino_vits16", 224, 224), ("dino_vits16", 48, 80),
                                       ("dino_vitb16", 64, 96), ("dino_vitb16", 224, 224), ("dino_vitb16", 48, 80)])
def test_descriptors_at_patch_stride_vs_oracle(model, H, W):
    from oracle import dino_oracle
    dev = _gpu()
    c = VIT_CONFIGS[model]
    sd = make_synthetic_vit_state_dict(model, 5)
    enc = DinoViT(model, False, "concat_pixels_concat_features", stride=c["patch"], state_dict=sd)
    x = torch.from_numpy(np.random.default_rng(H + W).standard_normal((2, 3, H, W)).astype(np.float32))
    got = enc(x.to(dev)).cpu()
    torch.set_num_threads(16)
    ref = dino_oracle.extract_key_descriptors(_torch_sd(sd), x, heads=c["heads"], patch=c["patch"])
    assert got.shape == ref.shape == (2, c["dim"], H // c["patch"], W // c["patch"])
    err = (got - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err


# ------------------------------------------------------------------------------------------ b. overlapping strides
@pytest.mark.gpu
@pytest.mark.parametrize("model,stride,H,W", [("dino_vits8", 4, 64, 96), ("dino_vits8", 4, 40, 72), ("dino_vits8", 4, 48, 48),
                                              ("dino_vitb8", 4, 64, 96), ("dino_vits16", 8, 64, 96), ("dino_vits16", 8, 48, 80)])
def test_descriptors_at_overlapping_stride(model, stride, H, W):
    dev = _gpu()
    c = VIT_CONFIGS[model]
    sd = make_synthetic_vit_state_dict(model, 6)
    enc = DinoViT(model, False, "concat_pixels_concat_features", stride=stride, state_dict=sd)
    x = torch.from_numpy(np.random.default_rng(H * W).standard_normal((2, 3, H, W)).astype(np.float32))
    got = enc(x.to(dev)).cpu()
    assert enc.extractor.num_patches == token_grid(H, W, c["patch"], stride)
    torch.set_num_threads(16)
    ref = ref_keys(_torch_sd(sd), x, c["heads"], c["patch"], stride)
    assert got.shape == ref.shape == (2, c["dim"], H // stride, W // stride)
    err = (got - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err


# ------------------------------------------------------------------------------------------ c. the resize kernel alone
@pytest.mark.gpu
@pytest.mark.parametrize("N,h0,w0,dim,heads,Ht,Wt", [
    (2, 63, 127, 384, 6, 64, 128),      # stride 4 on ViT-S/8 at 256x512: one row and one column short
    (1, 7, 9, 768, 12, 20, 31),         # upsampling, odd grid, 12 heads
    (2, 33, 45, 384, 6, 16, 21),        # downsampling
    (1, 5, 130, 768, 12, 11, 67),       # up in y, down in x, two column tiles
    (1, 13, 21, 384, 6, 13, 21),        # identity sizes through the kernel
    (3, 1, 1, 384, 6, 3, 2),            # a single token
])
def test_key_resize_kernel_vs_float64(N, h0, w0, dim, heads, Ht, Wt):
    dev = _gpu()
    lib = hip.load()
    T = 1 + h0 * w0
    Ta = (T + 31) // 32 * 32 + 32
    g = np.random.default_rng(N * 1000 + h0 + w0)
    buf = torch.full((N, Ta, 3 * dim), float("nan"))
    keys = torch.from_numpy(g.standard_normal((N, h0 * w0, dim)).astype(np.float32) * 2 + 0.3)
    buf[:, 1:T, dim:2 * dim] = keys                         # class row, q and v thirds and the padding rows stay NaN
    out = torch.full((N, dim, Ht, Wt), -7.0, device=dev)
    hip.check(lib.ccdm_vit_key_resize(buf.to(dev).data_ptr(), N, Ta, h0, w0, dim, heads, Ht, Wt, out.data_ptr(), 0), "key resize")
    torch.cuda.synchronize()
    got = out.cpu().double()
    k = keys.double().reshape(N, h0, w0, heads, dim // heads).permute(0, 4, 3, 1, 2).reshape(N, dim, h0, w0)
    ref = F.interpolate(k, (Ht, Wt), mode="bilinear", align_corners=False)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err <= 1e-6 * ref.abs().max().item(), err


@pytest.mark.gpu
def test_key_resize_rejects_a_grid_beyond_the_buffer():
    dev = _gpu()
    lib = hip.load()
    buf = torch.zeros((1, 64, 3 * 384), device=dev)
    out = torch.zeros((1, 384, 8, 8), device=dev)
    assert lib.ccdm_vit_key_resize(buf.data_ptr(), 1, 64, 8, 8, 384, 6, 8, 8, out.data_ptr(), 0) < 0       # 65 tokens > 64 rows
    assert "allocated" in hip.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("model,stride,shape", [("dino_vits8", 8, (13, 21)), ("dino_vitb16", 16, (9, 5)), ("dino_vits8", 4, (20, 20))])
def test_explicit_resize_shape(model, stride, shape):
    dev = _gpu()
    c = VIT_CONFIGS[model]
    sd = make_synthetic_vit_state_dict(model, 7)
    enc = DinoViT(model, False, "concat_pixels_concat_features", stride=stride, resize_shape=shape, state_dict=sd)
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((1, 3, 64, 96)).astype(np.float32))
    got = enc(x.to(dev)).cpu()
    torch.set_num_threads(16)
    ref = ref_keys(_torch_sd(sd), x, c["heads"], c["patch"], stride, size=shape)
    assert got.shape == ref.shape == (1, c["dim"], *shape)
    err = (got - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err


# ------------------------------------------------------------------------------------------ d. ViT-S/8 at stride 8 runs what it ran
class _CountingLib:
    """The library with ccdm_vit_key_resize counted; every other symbol passes through."""

    def __init__(self, lib):
        self._lib, self.resize_calls = lib, 0

    def ccdm_vit_key_resize(self, *a):
        self.resize_calls += 1
        return self._lib.ccdm_vit_key_resize(*a)

    def __getattr__(self, name):
        return getattr(self._lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("model,stride,H,W,calls", [("dino_vits8", 8, 64, 96, 0), ("dino_vits8", 8, 224, 224, 0), ("dino_vitb8", 8, 40, 72, 0),
                                                    ("dino_vits8", 4, 64, 96, 1)])
def test_identity_resize_launches_no_resize_kernel(model, stride, H, W, calls):
    dev = _gpu()
    enc = DinoViT(model, False, "concat_pixels_concat_features", stride=stride, state_dict=make_synthetic_vit_state_dict(model, 3))
    spy = _CountingLib(enc.extractor.lib)
    enc.extractor.lib = spy
    x = torch.randn((1, 3, H, W), device=dev)
    assert enc(x).shape == (1, VIT_CONFIGS[model]["dim"], H // stride, W // stride)
    assert spy.resize_calls == calls


# ------------------------------------------------------------------------------------------ attention at ViT-B / stride-4 sizes
@pytest.mark.gpu
def test_attention_ex_at_vitb_stride4_full_resolution():
    """ccdm_attention_ex at 512x1024 with stride 4 (T = 32,386 tokens in 32,416 rows) and ViT-B's 12 heads of 64: sampled query
    rows of every head against float64; the padding rows of the output are not written."""
    dev = _gpu()
    lib = hip.load()
    C, heads, T = 768, 12, 1 + 127 * 255
    Ta = (T + 31) // 32 * 32
    assert (T, Ta) == (32386, 32416)
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn((1, Ta, 3 * C), generator=g)
    qkv[:, T:] = float("nan")
    out = torch.full((1, Ta, C), -5.0, device=dev)
    qd = qkv.to(dev)
    hip.check(lib.ccdm_attention_ex(qd.data_ptr(), out.data_ptr(), 1, T, Ta, C, heads, 1, 0), "attention_ex")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.all(got[:, T:] == -5.0)
    rows = torch.cat([torch.arange(0, 64), torch.randint(64, T - 64, (128,), generator=g), torch.arange(T - 64, T)])
    d = C // heads
    for h in range(heads):
        q = qkv[0, rows, h * d:(h + 1) * d].double()
        k = qkv[0, :T, C + h * d:C + (h + 1) * d].double()
        v = qkv[0, :T, 2 * C + h * d:2 * C + (h + 1) * d].double()
        ref = torch.softmax(q @ k.T / math.sqrt(d), -1) @ v
        err = (got[0, rows, h * d:(h + 1) * d].double() - ref).abs().max().item()
        assert err < 1e-5, (h, err)


# ------------------------------------------------------------------------------------------ e. U-Net step with the new feature shapes
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("channels,output_stride,target_layer", [(768, 8, 10), (384, 4, 7)])
def test_unet_step_with_new_feature_shapes(prec, channels, output_stride, target_layer):
    from oracle import ccdm_oracle as O
    from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict
    dev = _gpu()
    fce = dict(type="dino", channels=channels, output_stride=output_stride, scale="single", target_layer=target_layer)
    model = build_model(250, "cosine", None, [(3, 64, 128), (20, 64, 128)], (3, 64, 128), "unet_openai",
                        dict(LIDC_BP, channel_mult=[1, 1, 2, 2, 4, 4]), "datasets.cityscapes", "confidence", fce)
    assert model.unet.spec.feature_condition_idx == [target_layer] and model.unet.spec.feature_channels == channels
    sd = {k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 8).items()}
    model.unet.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    model.prec = prec
    rng = np.random.default_rng(channels + output_stride)
    img = torch.from_numpy(rng.standard_normal((1, 3, 64, 128)).astype(np.float32))
    feat = torch.from_numpy(rng.standard_normal((1, channels, 64 // output_stride, 128 // output_stride)).astype(np.float32))
    x = O.one_hot_bchw(torch.from_numpy(rng.integers(0, 20, (1, 64, 128))), 20)
    t = torch.full((1,), 120.0)
    out = model(x.to(dev), img.to(dev), feat.to(dev), t=t, validation=True)["diffusion_out"].cpu()
    ref = O.unet_forward(sd, dict(LIDC_CFG, feature_condition_idx=[target_layer]), x, img, feat, t)["diffusion_out"]
    err = (out - ref).abs().max().item()
    assert err < 1e-4, err


# ------------------------------------------------------------------------------------------ f. end to end
class _Recorder:
    def __init__(self, m):
        self.m, self.diffusion, self.fcs = m, m.diffusion, []

    def __call__(self, x, image, feature_condition=None):
        self.fcs.append(feature_condition)
        return self.m(x, image, feature_condition)

    def predict_multiple(self, image, feature_condition=None, **kw):
        self.fcs.append(feature_condition)
        return self.m.predict_multiple(image, feature_condition, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("model_type,channels,output_stride,target_layer", [("dino_vitb8", 768, 8, 10), ("dino_vits8", 384, 4, 7)])
def test_eval_segmentation_with_encoder_variants(model_type, channels, output_stride, target_layer):
    from ccdm_stochastic_segmentation_amd import build_model, make_synthetic_state_dict
    from ccdm_stochastic_segmentation_amd import segmentation as SEG
    _gpu()
    fce = dict(type="dino", model=model_type, channels=channels, conditioning="concat_pixels_concat_features", output_stride=output_stride,
               scale="single", train=False, source_layer=11, target_layer=target_layer)
    K, H, W = 20, 64, 64
    model = build_model(4, "cosine", {"s": 0.008}, [(3, H, W), (K, H, W)], (3, H, W), "unet_openai",
                        dict(LIDC_BP, channel_mult=[1, 1, 2, 2, 4, 4]), "datasets.cityscapes", "confidence", fce)
    model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, 2).items()}, strict=True)
    model = model.cuda().eval()
    rec = _Recorder(model)
    params = {"dataset_file": "synthetic.cityscapes_miou", "batch_size": 2, "mp_loaders": 0,
              "evaluation": {"resolution": "original", "evaluations": 1, "evaluation_vote_strategy": "confidence"},
              "feature_cond_encoder": fce}
    ds = SEG.SyntheticCityscapes(size=2, resolution=(H, W), original_size=(96, 128), seed=1)
    res = SEG.eval_segmentation(params, dataset=ds, model=rec, synthetic_weights_seed=4)
    assert len(rec.fcs) == 1 and rec.fcs[0].shape == (2, channels, H // output_stride, W // output_stride)
    assert torch.isfinite(rec.fcs[0]).all()
    assert res["images"] == 2 and len(res["IoU"]) == 19
    assert math.isfinite(res["mIoU"]) and math.isfinite(res["mIoU_soft"])
