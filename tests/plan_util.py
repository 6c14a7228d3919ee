"""Shape-only conv calls for ccdm_conv_plan (include/ccdm_hip.h): the launch plan is host code, so a ConvArgs whose pointer fields only say
"operand present" is enough to ask which kernel a call runs and how it partitions the work — no GPU, no tensors.  Shared by the CPU tests
of the plan (tests/test_host_logic.py) and the GPU tests that hold both sides of each batch-size threshold to equal bits
(tests/test_batch_rules.py), so the two cannot speak of different cases.  The second half is the ledger of launch plans: signature() names
what a call runs, shipped_conv_calls() lists every conv of the shipped networks, and PLAN_CASES holds one kernel-level case per signature
(proved complete on the CPU by tests/test_host_logic.py, run against float64 on the GPU by tests/test_conv_plan_coverage.py)."""
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


def spec_conv_calls(spec, N, H, W, Cs, prec=hip.PREC_F16X3, fine=0, film=None):
    """(name, ConvArgs) of every conv the engine emits for one U-Net step of `spec` on N samples of H x W (engine.SamplerEngine._layers,
    shapes only; the qkv conv of every AttentionBlock is listed whether or not the fused attention kernel would take it, the first and the
    last conv whether or not the fused stem and head kernels would).  Cs: channels of the padded stem input; fine: the engine's
    fine_slices; film: None = as the spec's ResBlocks say, True / False = every ResBlock with / without use_scale_shift_norm.  The
    resample launches of a resblock_updown network (engine.SamplerEngine._res_updown) are no convs and are not listed."""
    lib = hip.load()
    calls = []

    def conv(name, src, cout, k, h, w, **kw):
        calls.append((name, conv_args(N, h, w, src[0], cout, k, c1=src[1] if len(src) > 1 else 0, prec=prec, fine=fine, **kw)))

    def layers(blk, src, h, w):
        cur = list(src)
        for l in blk:
            lfilm = bool(l.film if film is None else film) if l.kind == "res" else False
            if l.kind == "conv":
                conv(l.name, cur, l.cout, 3, h, w)
                cur = [l.cout]
            elif l.kind == "res" and l.updown:
                assert len(cur) == 1 and l.cin == l.cout, l.name
                if l.updown == "down":      # in_layers.2 reads the pooled SiLU(GN(x)) the resample launch leaves: a raw input
                    h, w = h // 2, w // 2
                    conv(l.name + ".in_layers.2", cur, l.cout, 3, h, w, emb=not lfilm)
                else:                       # GroupNorm + SiLU, then nearest x2 on load (never the sub-pixel form: it takes raw inputs only)
                    conv(l.name + ".in_layers.2", cur, l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, up=1, emb=not lfilm)
                    h, w = 2 * h, 2 * w
                conv(l.name + ".out_layers.3", [l.cout], l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, film=lfilm, resid=True)
                cur = [l.cout]
            elif l.kind == "res":
                conv(l.name + ".in_layers.2", cur, l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, emb=not lfilm)
                tail = dict(skip=tuple(cur)) if l.has_skip_conv else dict(resid=True)
                conv(l.name + ".out_layers.3", [l.cout], l.cout, 3, h, w, gn=True, act=hip.ACT_SILU, film=lfilm, **tail)
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


# ------------------------------------------------------------------------------------------ the signature ledger of the conv launch plans
# A signature names what a conv call runs: the kernel family, its tile geometry and chunk width, the tap split, masked or unmasked core
# items, how the tiles are cut into slices, the call's own kernel-selecting fields and its operand set.  Two calls of one signature run the
# same kernel instantiation over the same code paths; the ledger test of tests/test_host_logic.py requires a kernel-level float64 case
# (PLAN_CASES, run by tests/test_conv_plan_coverage.py) for every signature a shipped network emits.  ntiles_per_block, skip_wide, the
# grid and the LDS size stay out: they follow the batch size, and tests/test_batch_rules.py holds them bit for bit.
OPERANDS = ("gn", "silu", "emb", "film", "resid", "skip", "concat_in", "concat_skip", "stats")
SLICE_RUNGS = ("tile_per_slice", "even_slices", "uneven_slices")
KERNEL_NAME = {hip.CONV_KERNEL_GENERAL: "general", hip.CONV_KERNEL_KS: "ks", hip.CONV_KERNEL_UPCONV: "upconv", hip.CONV_KERNEL_1X1: "1x1"}


def _lg_quads(channels):
    """lanes per staged pixel of the few-pixel kernel, as a power of two: the channel quads of ceil(C / 16) k-steps rounded up to 16, 32
    or 64 (pow2_lg_quads of ccdm_conv_ks.hip)"""
    q = 4 * -(-channels // 16)
    return 4 if q <= 16 else (5 if q <= 32 else 6)


def signature(args, plan):
    """The hashable signature of a ConvArgs and its ccdm_conv_plan (a ConvPlanInfo or plan_dict of one):
    (kernel family, tile_h, tile_w, chunk, tap_split, core_unmasked, slice rung, ksize, stride, up, prec & 255, fine_slices, operands).

    kernel family: 1X1_MULTI counts as 1X1 (the walk over several n-tiles is a batch-size rule).
    slice rung: slices == tiles, tiles % slices == 0, or uneven, with tiles = ceil(H / tile_h) * ceil(W / tile_w) of the tiled space (the
      low-resolution input for up = 2, the output otherwise; the 1x1 kernels tile the flat pixel axis in blocks of tile_w).
    chunk of the few-pixel kernel: the plan reports the whole channel count there (the halo tile is staged once), which selects nothing.
      What does select an instantiation or a staging layout in conv_ks_plan stands in its place: (log2 of the lanes per staged pixel of
      the main segment, the same of the fused skip segment or None, the halo-item instantiation "13+0" / "8+8" / "20+0" = stride 1
      without and with a fused skip, stride 2).  Its n-tiles per block are a rule of the image size and Cout alone there (never of N) and
      pick the template instantiation, so they join the triple.
    operands: the subset of OPERANDS the call has, as a tuple in that order."""
    p = plan if isinstance(plan, dict) else plan_dict(plan)
    kernel = hip.CONV_KERNEL_1X1 if p["kernel"] == hip.CONV_KERNEL_1X1_MULTI else p["kernel"]
    H, W = (args.Hin, args.Win) if args.up == 2 else (args.Hout, args.Wout)
    if kernel == hip.CONV_KERNEL_1X1:
        tiles = H * W // p["tile_w"]
    else:
        tiles = -(-H // p["tile_h"]) * -(-W // p["tile_w"])
    rung = SLICE_RUNGS[0 if p["slices"] == tiles else (1 if tiles % p["slices"] == 0 else 2)]
    chunk = p["chunk"]
    if kernel == hip.CONV_KERNEL_KS:
        sc = args.SC0 + args.SC1 if args.skip0 else 0
        chunk = (_lg_quads(args.C0 + args.C1), _lg_quads(sc) if sc else None, "20+0" if args.stride == 2 else ("8+8" if sc else "13+0"),
                 p["ntiles_per_block"])
    has = dict(gn=bool(args.stats0), silu=args.act == hip.ACT_SILU, emb=args.emb_off >= 0, film=bool(args.film), resid=bool(args.resid),
               skip=bool(args.skip0), concat_in=args.C1 > 0, concat_skip=bool(args.skip0) and args.SC1 > 0, stats=bool(args.out_stats))
    return (KERNEL_NAME[kernel], p["tile_h"], p["tile_w"], chunk, p["tap_split"], p["core_unmasked"], rung, args.ksize, args.stride, args.up,
            args.prec & 255, args.fine_slices, tuple(o for o in OPERANDS if has[o]))


def signature_of(args):
    """signature(args, its ccdm_conv_plan): always asked of the library"""
    return signature(args, hip.conv_plan(args))


PRECS = (hip.PREC_F16X3, hip.PREC_F32)


def shipped_conv_calls():
    """(tag, layer name, ConvArgs) of every conv the shipped configurations run: the one list the ledger stands for.  Each configuration in
    PREC_F16X3 and in PREC_F32 (what the range fallback and DenoisingModel.f32_layers pin layers to):
      LIDC (128x128, 4 stem channels) at N = 64 (fine_slices 0), N = 16 (1), N = 8 and N = 1 (0 and 2): every value
        DenoisingModel._fine_slices returns;
      C4 (the DINO-conditioned Cityscapes network of tests/test_host_logic.c4_spec) at 256x512 (N = 16, 8, 1) and 512x1024 (N = 4, 1);
      the resblock_updown topology (tests/golden_util.UPDOWN_BP) and a use_scale_shift_norm LIDC network, at 128x128 and N = 2."""
    import ccdm_stochastic_segmentation_amd as P
    from tests.golden_util import UPDOWN_BP
    from tests.test_host_logic import LIDC_BP, c4_spec, lidc_spec
    configs = [("lidc_n%d_fine%d" % (n, f), lidc_spec(), n, 128, 128, 4, f) for n, f in ((64, 0), (16, 1), (8, 0), (8, 2), (1, 0), (1, 2))]
    configs += [("c4_%dx%d_n%d" % (h, w, n), c4_spec(), n, h, w, 24, 0) for h, w, ns in ((256, 512, (16, 8, 1)), (512, 1024, (4, 1))) for n in ns]
    configs.append(("updown_n2", P.make_unet_spec(image_size=128, in_channels=3, out_channels=2, **UPDOWN_BP), 2, 128, 128, 4, 0))
    configs.append(("film_n2", P.make_unet_spec(image_size=128, in_channels=3, out_channels=2, **dict(LIDC_BP, use_scale_shift_norm=True)),
                    2, 128, 128, 4, 0))
    calls = []
    for tag, spec, n, h, w, cs, fine in configs:
        for prec in PRECS:
            calls += [("%s_%s" % (tag, "f32" if prec == hip.PREC_F32 else "f16x3"), name, a)
                      for name, a in spec_conv_calls(spec, n, h, w, cs, prec=prec, fine=fine)]
    return calls


class PlanCase:
    """One kernel-level case of the ledger, as shape and operand set only: its signature is asked of the library whenever it is needed
    and never written down.  H, W: the INPUT size; ops: words of "gn silu emb film resid stats" (a fused skip and the two concats follow
    from `skip` and `c1`); shrink: H x W is the layer's own size, whose float64 reference is too costly (over about 2 GFLOP at N = 2) — the
    case then runs the smallest image whose plan has the same signature (shape()); edge: why a case whose signature no shipped network
    emits is in the table; refused: the library refuses the call by its shape, and the case asserts that."""

    def __init__(self, layer, H, W, c0, cout, k, ops, prec, fine=0, *, c1=0, stride=1, up=0, skip=(), shrink=False, edge=None, refused=None):
        ops = ops.split()
        assert set(ops) <= {"gn", "silu", "emb", "film", "resid", "stats"}, ops
        self.layer, self.H, self.W, self.c0, self.cout, self.k, self.prec, self.fine = layer, H, W, c0, cout, k, prec, fine
        self.c1, self.stride, self.up, self.skip, self.shrink, self.edge, self.refused = c1, stride, up, tuple(skip), shrink, edge, refused
        self.gn, self.silu, self.emb, self.film, self.resid, self.stats = (o in ops for o in ("gn", "silu", "emb", "film", "resid", "stats"))
        self.id = "%s-%s-%dx%d-%d+%d-%d-k%ds%du%d-%s%s-f%d" % ("f32" if prec == hip.PREC_F32 else "f16x3", layer, H, W, c0, c1, cout, k, stride, up,
                                                                "_".join(ops) or "raw", "-skip%s" % "+".join(map(str, skip)) if skip else "", fine)
        self._shape = None

    def args(self, N=2, H=None, W=None, diag=0):
        """the shape-only ConvArgs of the case at its run shape (or at H x W)"""
        if H is None:
            H, W = self.shape()
        return conv_args(N, H, W, self.c0, self.cout, self.k, c1=self.c1, stride=self.stride, up=self.up, gn=self.gn,
                         act=hip.ACT_SILU if self.silu else hip.ACT_NONE, emb=self.emb, film=self.film, resid=self.resid, skip=self.skip,
                         want_stats=self.stats, prec=self.prec, fine=self.fine, diag=diag)

    def shape(self):
        """the input size the case runs at"""
        if self._shape is None:
            self._shape = smallest_image_with_same_plan(self) if self.shrink else (self.H, self.W)
        return self._shape

    def signature(self):
        if self.refused:
            with_error = None
            try:
                hip.conv_plan(self.args())
            except hip.CcdmHipError as e:
                with_error = str(e)
            assert with_error and self.refused in with_error, (self.id, with_error)
            return ("refused", self.refused, self.k, self.stride, self.up, self.prec & 255, self.fine)
        return signature_of(self.args())


def smallest_image_with_same_plan(case, step=8):
    """The smallest input size (in steps of `step` pixels, at most the layer's own) at which ccdm_conv_plan gives the case's call the
    signature it has at the layer's own size: the rules are asked, not restated."""
    want = signature_of(case.args(H=case.H, W=case.W))
    sizes = sorted(((h, w) for h in range(step, case.H + 1, step) for w in range(step, case.W + 1, step)), key=lambda s: (s[0] * s[1], s))
    for h, w in sizes:
        try:
            if signature_of(case.args(H=h, W=w)) == want:
                return h, w
        except hip.CcdmHipError:      # a size the library refuses
            continue
    raise AssertionError("no size up to %dx%d has the signature of %s" % (case.H, case.W, case.id))


F16X3, F32 = hip.PREC_F16X3, hip.PREC_F32

# One case per signature (tests/test_host_logic.py holds the table to that).  Each row is a layer of a shipped network that has the signature,
# the cheapest one: "<network>.<block>" with in / mid / out for input_blocks / middle_block / output_blocks and conv1 / conv2 for
# in_layers.2 / out_layers.3; lidc, c4, updown and film are the four networks of shipped_conv_calls().  The last positional argument is
# fine_slices.  The rows at the end, with edge="...", are no shipped layers.
PLAN_CASES = [
    # ---- LIDC, PREC_F16X3, fine_slices 0
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F16X3, 0),
    PlanCase("lidc.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("lidc.in3.0.op", 128, 128, 32, 32, 3, "stats", F16X3, 0, stride=2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F16X3, 0, stride=2),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 0, skip=(32,)),
    PlanCase("updown.in6.0.conv2", 32, 32, 32, 32, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("lidc.in9.0.op", 32, 32, 64, 64, 3, "stats", F16X3, 0, stride=2),
    PlanCase("lidc.in10.0.conv1", 16, 16, 64, 96, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in10.0.conv2", 16, 16, 96, 96, 3, "gn silu stats", F16X3, 0, skip=(64,)),
    PlanCase("c4.in16.1.qkv", 8, 16, 128, 384, 1, "gn", F16X3, 0),
    PlanCase("lidc.in10.1.proj_out", 16, 16, 96, 96, 1, "resid stats", F16X3, 0),
    PlanCase("lidc.in11.0.conv1", 16, 16, 96, 96, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in11.0.conv2", 16, 16, 96, 96, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F16X3, 0, stride=2),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 0, skip=(96,)),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F16X3, 0),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F16X3, 0),
    PlanCase("updown.in12.0.conv2", 8, 8, 96, 96, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 0, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 0, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F16X3, 0, up=2),
    PlanCase("lidc.out5.0.conv1", 16, 16, 96, 96, 3, "gn silu emb stats", F16X3, 0, c1=64),
    PlanCase("lidc.out5.0.conv2", 16, 16, 96, 96, 3, "gn silu stats", F16X3, 0, skip=(96, 64)),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F16X3, 0, up=2),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F16X3, 0, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 0, skip=(64, 32)),
    PlanCase("lidc.out8.1.conv", 32, 32, 64, 64, 3, "stats", F16X3, 0, up=2),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 0, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F16X3, 0, skip=(32, 32)),
    PlanCase("lidc.out11.1.conv", 64, 64, 32, 32, 3, "stats", F16X3, 0, up=2),
    PlanCase("lidc.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F16X3, 0, c1=32),
    PlanCase("lidc.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu stats", F16X3, 0, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F16X3, 0),
    # ---- LIDC, PREC_F32, fine_slices 0
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F32, 0),
    PlanCase("lidc.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F32, 0),
    PlanCase("lidc.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu resid stats", F32, 0),
    PlanCase("lidc.in3.0.op", 128, 128, 32, 32, 3, "stats", F32, 0, stride=2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 0),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F32, 0),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F32, 0, stride=2),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F32, 0),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 0, skip=(32,)),
    PlanCase("updown.in6.0.conv2", 32, 32, 32, 32, 3, "gn silu resid stats", F32, 0),
    PlanCase("lidc.in10.0.conv1", 16, 16, 64, 96, 3, "gn silu emb stats", F32, 0),
    PlanCase("lidc.in10.0.conv2", 16, 16, 96, 96, 3, "gn silu stats", F32, 0, skip=(64,)),
    PlanCase("lidc.in10.1.qkv", 16, 16, 96, 288, 1, "gn", F32, 0),
    PlanCase("lidc.in10.1.proj_out", 16, 16, 96, 96, 1, "resid stats", F32, 0),
    PlanCase("updown.in9.0.conv2", 16, 16, 64, 64, 3, "gn silu resid stats", F32, 0),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F32, 0, stride=2),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F32, 0),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 0, skip=(96,)),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F32, 0),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F32, 0),
    PlanCase("updown.in12.0.conv2", 8, 8, 96, 96, 3, "gn silu resid stats", F32, 0),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F32, 0, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 0, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F32, 0, up=1),
    PlanCase("lidc.out5.0.conv1", 16, 16, 96, 96, 3, "gn silu emb stats", F32, 0, c1=64),
    PlanCase("lidc.out5.0.conv2", 16, 16, 96, 96, 3, "gn silu stats", F32, 0, skip=(96, 64)),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F32, 0, up=1),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F32, 0, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 0, skip=(64, 32)),
    PlanCase("lidc.out8.1.conv", 32, 32, 64, 64, 3, "stats", F32, 0, up=1),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 0, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F32, 0, skip=(32, 32)),
    PlanCase("lidc.out11.1.conv", 64, 64, 32, 32, 3, "stats", F32, 0, up=1),
    PlanCase("lidc.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F32, 0, c1=32),
    PlanCase("lidc.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu stats", F32, 0, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F32, 0),
    # ---- LIDC, PREC_F16X3, fine_slices 1 (latency slicing at N = 16)
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F16X3, 1),
    PlanCase("lidc.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F16X3, 1),
    PlanCase("lidc.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu resid stats", F16X3, 1),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F16X3, 1, stride=2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 1),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F16X3, 1),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F16X3, 1),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 1, skip=(32,)),
    PlanCase("lidc.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu resid stats", F16X3, 1),
    PlanCase("lidc.in14.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 1),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 1, skip=(96,)),
    PlanCase("lidc.in10.1.qkv", 16, 16, 96, 288, 1, "gn", F16X3, 1),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F16X3, 1),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F16X3, 1),
    PlanCase("lidc.in11.0.conv2", 16, 16, 96, 96, 3, "gn silu resid stats", F16X3, 1),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F16X3, 1, stride=2),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F16X3, 1),
    PlanCase("lidc.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu resid stats", F16X3, 1),
    PlanCase("lidc.out0.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 1, c1=128),
    PlanCase("lidc.out0.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 1, skip=(128, 128)),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 1, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 1, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F16X3, 1, up=2),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F16X3, 1, up=2),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F16X3, 1, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 1, skip=(64, 32)),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 1, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F16X3, 1, skip=(32, 32)),
    PlanCase("lidc.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F16X3, 1, c1=32),
    PlanCase("lidc.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu stats", F16X3, 1, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F16X3, 1),
    # ---- LIDC, PREC_F32, fine_slices 1
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F32, 1),
    PlanCase("lidc.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F32, 1),
    PlanCase("lidc.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu resid stats", F32, 1),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F32, 1, stride=2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 1),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F32, 1),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F32, 1),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 1, skip=(32,)),
    PlanCase("lidc.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu resid stats", F32, 1),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F32, 1),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 1, skip=(96,)),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F32, 1),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F32, 1),
    PlanCase("lidc.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu resid stats", F32, 1),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F32, 1, stride=2),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F32, 1, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 1, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F32, 1, up=1),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F32, 1, up=1),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F32, 1, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 1, skip=(64, 32)),
    PlanCase("lidc.out8.1.conv", 32, 32, 64, 64, 3, "stats", F32, 1, up=1),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 1, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F32, 1, skip=(32, 32)),
    PlanCase("lidc.out11.1.conv", 64, 64, 32, 32, 3, "stats", F32, 1, up=1),
    PlanCase("lidc.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu emb stats", F32, 1, c1=32),
    PlanCase("lidc.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu stats", F32, 1, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F32, 1),
    # ---- LIDC, PREC_F16X3, fine_slices 2 (latency slicing at N <= 8)
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F16X3, 2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 2),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F16X3, 2),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F16X3, 2, stride=2),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F16X3, 2),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 2, skip=(32,)),
    PlanCase("lidc.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu resid stats", F16X3, 2),
    PlanCase("lidc.in14.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 2),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 2, skip=(96,)),
    PlanCase("lidc.in10.1.qkv", 16, 16, 96, 288, 1, "gn", F16X3, 2),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F16X3, 2),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F16X3, 2),
    PlanCase("lidc.in11.0.conv2", 16, 16, 96, 96, 3, "gn silu resid stats", F16X3, 2),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F16X3, 2, stride=2),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F16X3, 2),
    PlanCase("lidc.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu resid stats", F16X3, 2),
    PlanCase("lidc.out0.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 2, c1=128),
    PlanCase("lidc.out0.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 2, skip=(128, 128)),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 2, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 2, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F16X3, 2, up=2),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F16X3, 2, up=2),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F16X3, 2, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 2, skip=(64, 32)),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 2, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F16X3, 2, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F16X3, 2),
    # ---- LIDC, PREC_F32, fine_slices 2
    PlanCase("lidc.in0.0", 128, 128, 4, 32, 3, "stats", F32, 2),
    PlanCase("lidc.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 2),
    PlanCase("lidc.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu resid stats", F32, 2),
    PlanCase("lidc.in6.0.op", 64, 64, 32, 32, 3, "stats", F32, 2, stride=2),
    PlanCase("lidc.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu emb stats", F32, 2),
    PlanCase("lidc.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 2, skip=(32,)),
    PlanCase("lidc.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu resid stats", F32, 2),
    PlanCase("lidc.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu emb stats", F32, 2),
    PlanCase("lidc.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 2, skip=(96,)),
    PlanCase("lidc.in13.1.qkv", 8, 8, 128, 384, 1, "gn", F32, 2),
    PlanCase("lidc.in13.1.proj_out", 8, 8, 128, 128, 1, "resid stats", F32, 2),
    PlanCase("lidc.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu resid stats", F32, 2),
    PlanCase("lidc.in12.0.op", 16, 16, 96, 96, 3, "stats", F32, 2, stride=2),
    PlanCase("lidc.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F32, 2, c1=96),
    PlanCase("lidc.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu stats", F32, 2, skip=(128, 96)),
    PlanCase("lidc.out2.2.conv", 8, 8, 128, 128, 3, "stats", F32, 2, up=1),
    PlanCase("lidc.out5.2.conv", 16, 16, 96, 96, 3, "stats", F32, 2, up=1),
    PlanCase("lidc.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F32, 2, c1=32),
    PlanCase("lidc.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu stats", F32, 2, skip=(64, 32)),
    PlanCase("lidc.out8.1.conv", 32, 32, 64, 64, 3, "stats", F32, 2, up=1),
    PlanCase("lidc.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 2, c1=32),
    PlanCase("lidc.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu stats", F32, 2, skip=(32, 32)),
    PlanCase("lidc.out.2", 128, 128, 32, 4, 3, "gn silu", F32, 2),
    # ---- what C4 (256x512 and 512x1024) adds
    PlanCase("c4.in6.0.op", 128, 256, 32, 32, 3, "stats", F16X3, 0, stride=2),
    PlanCase("c4.in10.1.proj_out", 32, 64, 64, 64, 1, "resid stats", F16X3, 0),
    PlanCase("c4.in13.0.conv1", 16, 32, 64, 128, 3, "gn silu emb stats", F16X3, 0),
    PlanCase("c4.in13.0.conv2", 16, 32, 128, 128, 3, "gn silu stats", F16X3, 0, skip=(64,)),
    PlanCase("c4.in14.0.conv2", 16, 32, 128, 128, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("c4.out2.2.conv", 8, 16, 128, 128, 3, "stats", F16X3, 0, up=2),
    PlanCase("c4.out5.0.conv1", 16, 32, 128, 128, 3, "gn silu emb stats", F16X3, 0, c1=64),
    PlanCase("c4.out5.0.conv2", 16, 32, 128, 128, 3, "gn silu stats", F16X3, 0, skip=(128, 64)),
    PlanCase("c4.out8.2.conv", 32, 64, 64, 64, 3, "stats", F16X3, 0, up=2),
    PlanCase("c4.out11.1.conv", 64, 128, 64, 64, 3, "stats", F16X3, 0, up=2, shrink=True),
    PlanCase("c4.out14.1.conv", 128, 256, 32, 32, 3, "stats", F16X3, 0, up=2, shrink=True),
    PlanCase("c4.in6.0.op", 128, 256, 32, 32, 3, "stats", F32, 0, stride=2),
    PlanCase("c4.in10.1.qkv", 32, 64, 64, 192, 1, "gn", F32, 0),
    PlanCase("c4.in10.1.proj_out", 32, 64, 64, 64, 1, "resid stats", F32, 0),
    PlanCase("c4.in7.0.conv2", 128, 256, 64, 64, 3, "gn silu stats", F16X3, 0, skip=(32,), shrink=True),
    PlanCase("c4.out5.2.conv", 32, 64, 128, 128, 3, "stats", F16X3, 0, up=2, shrink=True),
    PlanCase("c4.in7.0.conv2", 128, 256, 64, 64, 3, "gn silu stats", F32, 0, skip=(32,), shrink=True),
    # ---- what the resblock_updown topology adds
    PlanCase("updown.in3.0.conv1", 64, 64, 32, 32, 3, "emb stats", F16X3, 0),
    PlanCase("updown.in6.0.conv1", 32, 32, 32, 32, 3, "emb stats", F16X3, 0),
    PlanCase("updown.in9.0.conv1", 16, 16, 64, 64, 3, "emb stats", F16X3, 0),
    PlanCase("updown.in9.0.conv2", 16, 16, 64, 64, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("updown.in12.0.conv1", 8, 8, 96, 96, 3, "emb stats", F16X3, 0),
    PlanCase("updown.out2.2.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F16X3, 0, up=1),
    PlanCase("updown.out2.2.conv2", 16, 16, 128, 128, 3, "gn silu resid stats", F16X3, 0),
    PlanCase("updown.out5.2.conv1", 16, 16, 96, 96, 3, "gn silu emb stats", F16X3, 0, up=1),
    PlanCase("updown.out8.1.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F16X3, 0, up=1),
    PlanCase("updown.out11.1.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F16X3, 0, up=1),
    PlanCase("updown.in3.0.conv1", 64, 64, 32, 32, 3, "emb stats", F32, 0),
    PlanCase("updown.in6.0.conv1", 32, 32, 32, 32, 3, "emb stats", F32, 0),
    PlanCase("updown.in9.0.conv1", 16, 16, 64, 64, 3, "emb stats", F32, 0),
    PlanCase("updown.in12.0.conv1", 8, 8, 96, 96, 3, "emb stats", F32, 0),
    PlanCase("updown.out2.2.conv1", 8, 8, 128, 128, 3, "gn silu emb stats", F32, 0, up=1),
    PlanCase("updown.out5.2.conv1", 16, 16, 96, 96, 3, "gn silu emb stats", F32, 0, up=1),
    PlanCase("updown.out8.1.conv1", 32, 32, 64, 64, 3, "gn silu emb stats", F32, 0, up=1),
    PlanCase("updown.out11.1.conv1", 64, 64, 32, 32, 3, "gn silu emb stats", F32, 0, up=1),
    # ---- what use_scale_shift_norm adds: in_layers without emb, out_layers with FiLM
    PlanCase("film.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu film resid stats", F16X3, 0),
    PlanCase("film.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu film resid stats", F16X3, 0),
    PlanCase("film.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu film stats", F16X3, 0, skip=(32,)),
    PlanCase("film.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu film resid stats", F16X3, 0),
    PlanCase("film.in10.0.conv1", 16, 16, 64, 96, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in10.0.conv2", 16, 16, 96, 96, 3, "gn silu film stats", F16X3, 0, skip=(64,)),
    PlanCase("film.in11.0.conv1", 16, 16, 96, 96, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in11.0.conv2", 16, 16, 96, 96, 3, "gn silu film resid stats", F16X3, 0),
    PlanCase("film.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu stats", F16X3, 0),
    PlanCase("film.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu film stats", F16X3, 0, skip=(96,)),
    PlanCase("film.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu film resid stats", F16X3, 0),
    PlanCase("film.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu stats", F16X3, 0, c1=96),
    PlanCase("film.out0.0.conv2", 8, 8, 128, 128, 3, "gn silu film stats", F16X3, 0, skip=(128, 128)),
    PlanCase("film.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu film stats", F16X3, 0, skip=(128, 96)),
    PlanCase("film.out5.0.conv1", 16, 16, 96, 96, 3, "gn silu stats", F16X3, 0, c1=64),
    PlanCase("film.out5.0.conv2", 16, 16, 96, 96, 3, "gn silu film stats", F16X3, 0, skip=(96, 64)),
    PlanCase("film.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu stats", F16X3, 0, c1=32),
    PlanCase("film.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu film stats", F16X3, 0, skip=(64, 32)),
    PlanCase("film.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu stats", F16X3, 0, c1=32),
    PlanCase("film.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu film stats", F16X3, 0, skip=(32, 32)),
    PlanCase("film.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu stats", F16X3, 0, c1=32),
    PlanCase("film.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu film stats", F16X3, 0, skip=(32, 32)),
    PlanCase("film.in1.0.conv1", 128, 128, 32, 32, 3, "gn silu stats", F32, 0),
    PlanCase("film.in1.0.conv2", 128, 128, 32, 32, 3, "gn silu film resid stats", F32, 0),
    PlanCase("film.in4.0.conv1", 64, 64, 32, 32, 3, "gn silu stats", F32, 0),
    PlanCase("film.in4.0.conv2", 64, 64, 32, 32, 3, "gn silu film resid stats", F32, 0),
    PlanCase("film.in7.0.conv1", 32, 32, 32, 64, 3, "gn silu stats", F32, 0),
    PlanCase("film.in7.0.conv2", 32, 32, 64, 64, 3, "gn silu film stats", F32, 0, skip=(32,)),
    PlanCase("film.in8.0.conv2", 32, 32, 64, 64, 3, "gn silu film resid stats", F32, 0),
    PlanCase("film.in10.0.conv1", 16, 16, 64, 96, 3, "gn silu stats", F32, 0),
    PlanCase("film.in10.0.conv2", 16, 16, 96, 96, 3, "gn silu film stats", F32, 0, skip=(64,)),
    PlanCase("film.in11.0.conv2", 16, 16, 96, 96, 3, "gn silu film resid stats", F32, 0),
    PlanCase("film.in13.0.conv1", 8, 8, 96, 128, 3, "gn silu stats", F32, 0),
    PlanCase("film.in13.0.conv2", 8, 8, 128, 128, 3, "gn silu film stats", F32, 0, skip=(96,)),
    PlanCase("film.in14.0.conv2", 8, 8, 128, 128, 3, "gn silu film resid stats", F32, 0),
    PlanCase("film.out2.0.conv1", 8, 8, 128, 128, 3, "gn silu stats", F32, 0, c1=96),
    PlanCase("film.out2.0.conv2", 8, 8, 128, 128, 3, "gn silu film stats", F32, 0, skip=(128, 96)),
    PlanCase("film.out5.0.conv1", 16, 16, 96, 96, 3, "gn silu stats", F32, 0, c1=64),
    PlanCase("film.out5.0.conv2", 16, 16, 96, 96, 3, "gn silu film stats", F32, 0, skip=(96, 64)),
    PlanCase("film.out8.0.conv1", 32, 32, 64, 64, 3, "gn silu stats", F32, 0, c1=32),
    PlanCase("film.out8.0.conv2", 32, 32, 64, 64, 3, "gn silu film stats", F32, 0, skip=(64, 32)),
    PlanCase("film.out10.0.conv1", 64, 64, 32, 32, 3, "gn silu stats", F32, 0, c1=32),
    PlanCase("film.out10.0.conv2", 64, 64, 32, 32, 3, "gn silu film stats", F32, 0, skip=(32, 32)),
    PlanCase("film.out12.0.conv1", 128, 128, 32, 32, 3, "gn silu stats", F32, 0, c1=32),
    PlanCase("film.out12.0.conv2", 128, 128, 32, 32, 3, "gn silu film stats", F32, 0, skip=(32, 32)),
    # ---- edge cases: signatures no shipped network emits
    PlanCase("edge.ragged_wide", 40, 72, 32, 32, 3, "gn silu emb stats", F16X3, 0,
             edge="core_unmasked = 0 twin of lidc.in4.0.conv1: the last tile column and row are cut by the image"),
    PlanCase("edge.ragged_wide", 40, 72, 32, 32, 3, "gn silu resid stats", F32, 0,
             edge="the same ragged 8x32 tiling in exact fp32 (its staging has no unmasked form: the flag must not matter)"),
    PlanCase("edge.ragged_16", 12, 20, 64, 64, 3, "gn silu stats", F16X3, 0, skip=(32,),
             edge="core_unmasked = 0 twin of c4.in13.0.conv2: 8x16 tiles with 32-channel chunks, cut by the image in both directions"),
    PlanCase("edge.ragged_tap_split", 8, 12, 128, 128, 3, "gn silu emb stats", F16X3, 0,
             edge="12 pixels wide: not the few-pixel kernel; 8x8 tiles with the tap split and a half-empty second tile"),
    PlanCase("edge.seam16", 12, 20, 48, 32, 3, "silu stats", F16X3, 0, c1=16,
             edge="a concat seam at 48 channels: legal for 16-channel chunks only, SiLU without GroupNorm"),
    PlanCase("edge.seam16", 12, 20, 48, 32, 3, "silu stats", F32, 0, c1=16, refused="chunk",
             edge="the same seam in exact fp32, whose chunks are 32 channels wide: the call is refused"),
]
