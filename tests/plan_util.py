"""Shape-only conv calls for ccdm_conv_plan (include/ccdm_hip.h): the launch plan is host code, so a ConvArgs whose pointer fields only say
"operand present" is enough to ask which kernel a call runs and how it partitions the work — no GPU, no tensors.  Shared by the CPU tests
of the plan (tests/test_host_logic.py) and the GPU tests that hold both sides of each batch-size threshold to equal bits
(tests/test_batch_rules.py), so the two cannot speak of different cases."""
from ccdm_stochastic_segmentation_amd import hip

PRESENT = 1 << 12       # any non-null value: ccdm_conv_plan follows no pointer

# the general kernel's two-n-tiles-per-block rule (launch plan of ccdm_conv.hip): geometries with 24 wide (8x32) tiles and 24 slices per
# sample — 48x128 tiles exactly, 44x100 is ragged in both directions (no unmasked core) — and per output width
# (Cout, padded n-tiles, smallest N with NI = 2, largest N with NI = 1); None: NI = 1 at any N (odd tile count)
NI_GEOMETRIES = [(48, 128), (44, 100)]
NI_TABLE = [(64, 2, 22, 21), (40, 2, 22, 21), (128, 4, 11, 10), (160, 8, 6, 5), (96, 3, None, None)]
NI_OF_COUT = {cout: (lo_n, hi_n) for cout, _, lo_n, hi_n in NI_TABLE}

# the LDS-free 1x1 kernel's n-tile walk (ccdm_conv1x1.hip, no output statistics): (C0, Cout, H, W, N, ntb); N = None: the smallest batch
# the plan gives `ntb` for (asked of the plan, see smallest_batch_with_ntb)
CONV1X1_MULTI_CASES = [
    (64, 384, 8, 12, 64, 5),        # 32 pixels per block (one-wave blocks); 12 tiles in groups of 5, 5, 2: odd ntb, ragged last group
    (96, 288, 16, 16, 64, 2),       # 9 tiles in pairs: a last group of one
    (96, 288, 16, 16, 128, 5),      # groups of 5 and 4
    (32, 96, 32, 64, 27, 3),        # ntb = all three tiles of the layer
    (16, 64, 16, 16, None, 2),      # one k-step (every clamped operand load of the walk is the same fragment)
]

PLAN_FIELDS = [f for f, _ in hip.ConvPlanInfo._fields_]


def conv_args(N, H, W, c0, cout, k=3, *, c1=0, stride=1, up=0, gn=False, act=hip.ACT_NONE, emb=False, film=False, resid=False, skip=(),
              want_stats=True, prec=hip.PREC_F16X3, fine=0, diag=0):
    """The ConvArgs of a call as tests.hip_util.conv2d would fill it in, from shapes alone.  H, W: the INPUT size; skip: channel counts of
    the fused 1x1 skip sources."""
    a = hip.ConvArgs()
    a.in0, a.C0 = PRESENT, c0
    if c1:
        a.in1, a.C1 = PRESENT, c1
    if gn:
        a.stats0, a.slices0, a.gamma, a.beta = PRESENT, 1, PRESENT, PRESENT
        if c1:
            a.stats1, a.slices1 = PRESENT, 1
    a.eps, a.act = 1e-5, act
    hc, wc = (2 * H, 2 * W) if up else (H, W)
    pad = k // 2
    a.N, a.Hin, a.Win = N, H, W
    a.Hout, a.Wout = (hc + 2 * pad - k) // stride + 1, (wc + 2 * pad - k) // stride + 1
    a.ksize, a.stride, a.up, a.fine_slices = k, stride, int(up), int(fine)
    a.w, a.bias, a.Cout, a.prec = PRESENT, PRESENT, cout, prec | int(diag)
    a.emb_off = -1
    if emb or film:
        a.emb_table, a.emb_stride, a.emb_row_of_sample = PRESENT, 2 * (c0 + c1) if film else cout, PRESENT
        if emb:
            a.emb_off = 0
        if film:
            a.film, a.film_off = 1, 0
    if resid:
        a.resid = PRESENT
    if skip:
        a.skip0, a.SC0, a.skip_w = PRESENT, skip[0], PRESENT
        if len(skip) > 1:
            a.skip1, a.SC1 = PRESENT, skip[1]
    a.out = PRESENT
    if want_stats:
        a.out_stats = PRESENT
    return a


def plan(*shape, **kw):
    """ccdm_conv_plan of conv_args(*shape, **kw) as a dict"""
    return plan_dict(hip.conv_plan(conv_args(*shape, **kw)))


def plan_dict(info):
    return {f: getattr(info, f) for f in PLAN_FIELDS}


def smallest_batch_with_ntb(c0, cout, H, W, ntb, limit=4096):
    """the smallest N at which the plan walks `ntb` n-tiles per block of this 1x1 conv without output statistics"""
    for n in range(1, limit):
        p = plan(n, H, W, c0, cout, 1, want_stats=False)
        if p["kernel"] == hip.CONV_KERNEL_1X1_MULTI and p["ntiles_per_block"] == ntb:
            return n
    raise AssertionError(f"no batch below {limit} gives ntb = {ntb}")


def spec_conv_calls(spec, N, H, W, Cs, prec=hip.PREC_F16X3):
    """(name, ConvArgs) of every conv the engine emits for one U-Net step of `spec` on N samples of H x W (engine.SamplerEngine._layers,
    shapes only; the qkv conv of every AttentionBlock is listed whether or not the fused attention kernel would take it).  Cs: channels of
    the padded stem input."""
    lib = hip.load()
    calls = []

    def conv(name, src, cout, k, h, w, **kw):
        calls.append((name, conv_args(N, h, w, src[0], cout, k, c1=src[1] if len(src) > 1 else 0, prec=prec, **kw)))

    def layers(blk, src, h, w):
        cur = list(src)
        for l in blk:
            if l.kind == "conv":
                conv(l.name, cur, l.cout, 3, h, w)
                cur = [l.cout]
            elif l.kind == "res":
                if l.updown:
                    raise NotImplementedError("updown ResBlocks: not a BASELINE configuration")
                conv(l.name + ".in_layers.2", cur, l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, emb=not l.film)
                tail = dict(skip=tuple(cur)) if l.has_skip_conv else dict(resid=True)
                conv(l.name + ".out_layers.3", [l.cout], l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, film=l.film, **tail)
                cur = [l.cout]
            elif l.kind == "attn":
                conv(l.name + ".qkv", [l.ch], 3 * l.ch, 1, h, w, gn=True, want_stats=False)
                conv(l.name + ".proj_out", [l.ch], l.ch, 1, h, w, resid=True)
                cur = [l.ch]
            elif l.kind == "down":
                conv(l.name + ".op", cur, l.cout, 3, h, w, stride=2)
                cur, h, w = [l.cout], (h - 1) // 2 + 1, (w - 1) // 2 + 1
            elif l.kind == "up":
                conv(l.name + ".conv", cur, l.cout, 3, h, w, up=2 if lib.ccdm_upconv_supported(cur[0], l.cout, prec) else 1)
                cur, h, w = [l.cout], 2 * h, 2 * w
            else:  # pragma: no cover
                raise AssertionError(l.kind)
        return cur[0], h, w

    hs = []
    c, h, w = Cs, H, W
    for i, blk in enumerate(spec.input_blocks):
        src = [c, spec.feature_channels] if i in spec.feature_condition_idx else [c]
        c, h, w = layers(blk, src, h, w)
        hs.append(c)
    c, h, w = layers(spec.middle_block, [c], h, w)
    for blk in spec.output_blocks:
        c, h, w = layers(blk, [c, hs.pop()], h, w)
    assert (h, w) == (H, W) and not hs
    conv("out.2", [c], (spec.out_channels + 3) // 4 * 4, 3, h, w, gn=True, act=hip.ACT_SILU, want_stats=False)
    return calls
