/*
 * ccdm_hip.h — C ABI of libccdm_hip.so: the MI355X (gfx950) kernels of the categorical reverse-diffusion
 * sampler, plus the step executor ("engine") that replays them for T denoise steps.
 *
 * Plain pointers and sizes only; no torch types.  Every pointer marked `dev` is HIP device memory owned by
 * the caller (the Python host allocates it through torch); the library never allocates device memory and
 * keeps no global state besides a thread-local error string.  Every launch goes on the `stream` the caller
 * passes (a hipStream_t cast to void*; NULL = default stream).  Return value: 0 = ok, negative = error
 * (text via ccdm_last_error_string()).
 *
 * The reference (/root/reference, pure Python on torch) has no FFI; each entry point cites the reference
 * function whose arithmetic it replaces.  Activations are NHWC fp32; the reference's BCHW tensors are
 * re-laid-out once at the boundary (ccdm_nchw_to_nhwc / the Python host).
 */
#ifndef CCDM_HIP_H
#define CCDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCDM_ABI_VERSION 11
#define CCDM_MAX_CHANNELS 1024      /* max C0+C1 of a GroupNorm'ed conv input */
#define CCDM_STATS_MAX_SLICES 64    /* partial-statistics slices per sample a GroupNorm consumer reads (more: ccdm_stats_fold) */
#define CCDM_STATS_FOLD_SLICES 16   /* what ccdm_stats_fold reduces a larger slice count to */

int ccdm_version(void);
const char* ccdm_last_error_string(void);

/* ---------------------------------------------------------------------------------------------------
 * Per-channel statistics of an NHWC tensor, the form every GroupNorm consumer reads:
 *   stats[n][s][c][0] = sum_x, stats[n][s][c][1] = sum_x^2 over the pixels slice s covered (fp64),
 *   s in [0, slices).  The consumer adds the slices in ascending s — a fixed order, so results are
 *   run-to-run deterministic (no floating-point atomics anywhere).
 * Replaces the statistics half of GroupNorm32 (unet_openai/nn.py:17-19 -> torch group_norm).
 * ------------------------------------------------------------------------------------------------- */
int ccdm_gn_stats(const float* x /*dev [N,HW,C]*/, int N, int HW, int C, int slices,
                  double* stats /*dev [N,slices,C,2]*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused  [GroupNorm(32 groups) -> (FiLM) -> SiLU ->]  conv KxK  [+bias +emb | +residual]  (+output stats)
 * on NHWC fp32, implicit GEMM on the matrix cores.
 * Replaces: ResBlock.in_layers / out_layers (unet.py:186-219, 242-262), skip_connection 1x1 (:221-228),
 * Downsample.op (:137-146), Upsample nearest-x2 + conv (:106-116), AttentionBlock.norm+qkv and proj_out
 * (:291-300, conv1d k=1 == 1x1 conv over tokens), the stem conv (:517) and the head GN-SiLU-conv (:701-707).
 * ------------------------------------------------------------------------------------------------- */
enum { CCDM_ACT_NONE = 0, CCDM_ACT_SILU = 1 };
enum { CCDM_PREC_F32 = 0,      /* v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation          */
       CCDM_PREC_F16X3 = 1,    /* fp16 hi/lo split, 3 x v_mfma_f32_32x32x16_f16, fp32 accumulate (~2^-22) */
       CCDM_PREC_F16 = 2 };    /* OPT-IN fast mode (ccdm_conv2d only; weights packed as for CCDM_PREC_F16X3): ONE fp16 MFMA per product — operands
                                  rounded to fp16 (~2^-11 each), fp32 accumulate.  Narrower arithmetic than the reference's: outside the parity
                                  contract, never a default, never the benchmarked configuration (tools/fast_mode_report.py prints its error) */
/* Range of CCDM_PREC_F16X3: a staged activation a (after GroupNorm/SiLU, or the raw input where there is none) must satisfy
 * |a| < 4094.  Beyond that its fp16 hi half is infinite and every output the element reaches is NaN/Inf — never a silently
 * clipped number; the step epilogue (ccdm_post_args.range_flag) turns that into a sticky device flag the host checks.
 * Below |a| ~ 2e-3 the split keeps an ABSOLUTE error <= 2^-29 (fp16 subnormal spacing after the 2^4 pre-scale). */

/* Diagnostic bit of ccdm_conv_args.prec (bits 8 and up are diagnostics; the arithmetic is prec & 255): run the general staging kernel
 * even where a specialised one applies (the LDS-free 1x1 kernel).  The parity tests use it to require identical bits from both. */
#define CCDM_DIAG_GENERAL_KERNEL (2048 << 8)

typedef struct ccdm_conv_args {
    /* input: virtual channel concat [in0 | in1] (in1 may be NULL); both [N,Hin,Win,C*] */
    const float* in0; const float* in1; int32_t C0; int32_t C1;
    /* GroupNorm over the concatenated channels: partial stats of each source (NULL = no normalisation) */
    const double* stats0; const double* stats1; int32_t slices0; int32_t slices1;
    const float* gamma; const float* beta;          /* dev [C0+C1] */
    float eps; int32_t act;                         /* CCDM_ACT_* applied after the affine */
    /* FiLM (use_scale_shift_norm): h = GN(h)*(1+scale)+shift, scale|shift = emb row [film_off, +2*C) */
    int32_t film; int32_t film_off;
    /* geometry */
    int32_t N, Hin, Win, Hout, Wout;
    int32_t ksize;                                  /* 1 or 3 (pad = ksize/2) */
    int32_t stride;                                 /* 1 or 2 */
    int32_t up;                                     /* 1: nearest x2 upsample of the input on load (weights: ccdm_pack_conv_weight);
                                                     * 2: the same operator in sub-pixel form (weights: ccdm_pack_upconv_weight,
                                                     *    out_slices = ccdm_upconv_slices) — see below */
    /* weights, packed by ccdm_pack_conv_weight for `prec` */
    const void* w; const float* bias; int32_t Cout; int32_t prec;
    /* epilogue */
    const float* emb_table; int32_t emb_stride; int32_t emb_off;   /* += emb_table[row*emb_stride + emb_off + c]; emb_off<0: none */
    const int32_t* emb_row_of_sample;               /* dev [N] or NULL (row = 0) ; row += *step_ptr */
    const int32_t* step_ptr;                        /* dev scalar or NULL (0) */
    const float* resid;                             /* dev [N,Hout,Wout,Cout] added last, or NULL */
    float* out;                                     /* dev [N,Hout,Wout,Cout] */
    double* out_stats; int32_t out_slices;          /* dev [N,out_slices,Cout,2] or NULL; out_slices = ccdm_conv_slices() */
    /* fused 1x1 skip connection (ResBlock.skip_connection, unet.py:221-228,262): out += W_s * [skip0 | skip1] as extra
     * K-segments of the same GEMM (raw input, centre tap).  skip_w is packed with ksize 1 and the SAME per-channel
     * exponents as w (ccdm_pack_conv_weight_ex with a shared absmax); its bias is pre-added into `bias` by the host.
     * Requires stride 1, up 0, skip tensors [N,Hout,Wout,SC*].  skip0 == NULL: none. */
    const float* skip0; const float* skip1; int32_t SC0; int32_t SC1;
    const void* skip_w;
    /* 1 / 2: latency slicing — more, shorter workgroups per sample (ccdm_conv_slices_ex(..., fine): up to 32 / 64 slices where the
     * default rule gives fewer, e.g. 32 instead of 12 at 128x128; 32x32 images on 8x16 tiles, 16x16 on 8x8) for batches too small to fill the chip.  The
     * statistics partials — and with them the last bit of a GroupNorm — depend on the slice count, so a run is bit-reproducible
     * across batch shardings only within one slicing mode; 0 (default) is the batch-size-independent rule. */
    int32_t fine_slices;
} ccdm_conv_args;

/* number of statistics slices the conv kernel produces for an Hout x Wout output (depends only on the
 * spatial size, never on N, so sharding the batch does not change any rounding).  Large images yield more than
 * CCDM_STATS_MAX_SLICES (one slice = one workgroup per sample: 256x512 -> 96, 512x1024 -> 384): fold them with
 * ccdm_stats_fold before handing them to a GroupNorm consumer. */
int ccdm_conv_slices(int Hout, int Wout, int stride, int ksize);
/* out_slices of any conv: geometry of the INPUT, `up` as in ccdm_conv_args (2: sub-pixel form), fine as ccdm_conv_args.fine_slices */
int ccdm_conv_slices_ex(int Hin, int Win, int ksize, int stride, int up, int fine);
/* out_slices of THIS conv (every field but out / out_stats / out_slices filled in): the rule above, except where the layer runs a
 * kernel with its own tiling — 3x3 F16X3 convs of images of at most 256 pixels leave one slice per 8x8 tile (16x16: 4, where the
 * rule says 2).  A function of the layer's shape and operands, never of N.  What a caller should size out_stats by. */
int ccdm_conv_out_slices(const ccdm_conv_args* a);
/* The launch plan of THIS conv: which kernel ccdm_conv2d would run for `a` and how it partitions the work.  Host code only — nothing is
 * launched and no pointer of `a` is followed (a pointer field counts as "operand present" or "absent"; out_stats != NULL = "statistics
 * wanted", out_slices is not checked).  The launchers take every one of these decisions from the function that fills this struct.
 * Everything here is a function of the layer's shape and operands, never of N — except ntiles_per_block, the one field a batch size
 * may change: the partitions it chooses between compute every output element and every statistics partial with the same
 * instruction sequence (tests/test_batch_rules.py holds both sides of each threshold to equal bits).  Returns 0, or a negative
 * error for a call ccdm_conv2d refuses by its shape.  Added in ABI 11 as a compatible extension. */
enum { CCDM_CONV_KERNEL_GENERAL = 0,     /* k_conv: every input staged through LDS                                  (ccdm_conv.hip)    */
       CCDM_CONV_KERNEL_KS = 1,          /* few-pixel 3x3: K split over the waves of a block                         (ccdm_conv_ks.hip) */
       CCDM_CONV_KERNEL_UPCONV = 2,      /* low-resolution sub-pixel Upsample conv: wave = phase                     (ccdm_upconv.hip)  */
       CCDM_CONV_KERNEL_1X1 = 3,         /* LDS-free 1x1, one n-tile per block                                       (ccdm_conv1x1.hip) */
       CCDM_CONV_KERNEL_1X1_MULTI = 4 }; /* LDS-free 1x1 without output statistics, several n-tiles per block        (ccdm_conv1x1.hip) */
typedef struct ccdm_conv_plan_info {
    int32_t kernel;                 /* CCDM_CONV_KERNEL_* */
    int32_t tile_h, tile_w;         /* pixel tile of a block's walk (up = 2: of the low-resolution input; 1x1 kernels: 1 x pixels per block) */
    int32_t chunk;                  /* input channels staged per chunk (the 1x1 kernels: channels per k-step in flight, 16) */
    int32_t ntiles;                 /* 32-channel output tiles of the packed weights (padded; up = 2: four phases per channel tile) */
    int32_t ntiles_per_block;       /* n-tiles one block computes: NI of k_conv / k_conv_ks, ntb of the 1x1 multi kernel, ctb of k_upconv */
    int32_t skip_wide;              /* the fused 1x1 skip runs in 32-channel core-only chunks (needs ntiles_per_block == 1) */
    int32_t tap_split;              /* the 3x3 kernel rows are split over three wave groups */
    int32_t slices;                 /* blocks per sample along grid.x */
    int32_t out_slices;             /* statistics partials per sample (= ccdm_conv_out_slices) */
    int32_t core_unmasked;          /* general kernel: core halo items need no per-lane padding mask */
    int32_t grid_x, grid_y, block;  /* the launch: blocks and threads per block */
    int32_t lds_bytes;              /* dynamic LDS of the launch */
} ccdm_conv_plan_info;
int ccdm_conv_plan(const ccdm_conv_args* a, ccdm_conv_plan_info* out);
/* Upsample (nearest x2) + conv 3x3 in sub-pixel form (unet.py:106-116), `up = 2`:
 *   out(2y+dy, 2x+dx) = sum over a,b in {0,1} of W'[dy,dx][a,b] . in(y+dy-1+a, x+dx-1+b),
 *   W'[dy][..][a] = the 3x3 kernel rows that land on low-resolution row y+dy-1+a  (dy=0: {r0}, {r1+r2}; dy=1: {r0+r1}, {r2}; columns alike):
 * four 2x2 convs of the LOW-resolution input — 4 instead of 9 taps per output pixel and a quarter of the staged halo.  The four
 * phases run as adjacent output-channel tiles of one launch (one block computes all four from one staged halo).  Needs CCDM_PREC_F16X3, ksize 3, stride 1, Cout % 32 == 0, no residual / fused
 * skip (ccdm_upconv_supported).  Sums of kernel taps are formed in fp64 and rounded once to fp32 before the fp16 split: results
 * differ from `up = 1` by fp32 rounding only.  out_slices = ccdm_upconv_slices(Hin, Win): the slices of the low-resolution
 * tiling (x 4 for inputs narrower than 16 pixels, where every phase runs in its own block); a function of the spatial size only. */
int ccdm_upconv_supported(int Cin, int Cout, int prec);
int ccdm_upconv_slices(int Hin, int Win);
size_t ccdm_pack_upconv_weight(const float* oihw /*[Cout,Cin,3,3]*/, int Cout, int Cin, int prec, void* out);
/* out[n][j] = sum of in[n][i] over i in [j*S_in/S_out, (j+1)*S_in/S_out), ascending (fixed order); S_out <= CCDM_STATS_MAX_SLICES (the engine folds to CCDM_STATS_FOLD_SLICES) */
int ccdm_stats_fold(const double* in /*dev [N,S_in,C,2]*/, int N, int S_in, int C, int S_out, double* out /*dev [N,S_out,C,2]*/, void* stream);
int ccdm_conv2d(const ccdm_conv_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The resamplers of the `resblock_updown=True` topology (ResBlock(up=True / down=True), unet.py:202-219 and :242-250, built from
 * Downsample(ch, use_conv=False) = AvgPool2d(2), unet.py:137-141, and Upsample(ch, use_conv=False) = nearest x2, unet.py:106-114):
 *   out_act = R(act(GroupNorm(in)))    — the `h` branch of a down block, between in_layers' SiLU and its conv (NULL: not wanted)
 *   out_raw = R(in)                    — the `x` branch that becomes the block's residual                     (NULL: not wanted)
 * R = AvgPool2d(2) ([N,H,W,C] -> [N,H/2,W/2,C], floor; sum order ((x00 + x01) + x10) + x11 like torch's CPU kernel, so out_raw is
 * bit-exact) or nearest x2 ([N,H,W,C] -> [N,2H,2W,C]).  GroupNorm as in ccdm_conv_args: `stats` are the producer's partial-statistics
 * slices of `in` (NULL: no normalisation; then gamma/beta are unused); C % 4 == 0, with GroupNorm C % 32 == 0.
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_RESAMPLE_AVGPOOL2 0
#define CCDM_RESAMPLE_NEAREST_UP2 1
typedef struct ccdm_resample_args {
    const float* in;            /* dev NHWC fp32 [N,Hin,Win,C] */
    int32_t C;
    const double* stats;        /* dev [N,slices,C,2] or NULL */
    int32_t slices;
    const float* gamma;         /* dev [C] */
    const float* beta;          /* dev [C] */
    float eps;
    int32_t act;                /* CCDM_ACT_NONE / CCDM_ACT_SILU, applied to out_act only */
    int32_t N, Hin, Win;
    int32_t mode;               /* CCDM_RESAMPLE_* */
    float* out_act;
    float* out_raw;
} ccdm_resample_args;
int ccdm_resample(const ccdm_resample_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The stem conv for inputs of at most 4 channels (LIDC: 2 classes + 1 image channel), CCDM_PREC_F16X3:
 *     h = conv3x3( cat([one_hot(x_t), image], 1) ) + bias                          unet.py:517 fed by unet.py:760
 * x_t arrives as the uint8 class index the epilogue leaves and the one-hot is built while staging; the image is
 * read from channels [K, Cs) of `xin` (its channels [0, K) are ignored — the epilogue need not write a one-hot there:
 * ccdm_post_args.xin = NULL).  The K axis of the GEMM is (tap, channel): 3 k-steps instead of the general kernel's 9.
 * Built for Cs == 4, H % 8 == 0, W % 32 == 0, Cout % 32 == 0 (ccdm_stem_conv_supported); out_slices = ccdm_conv_slices(H, W, 1, 3).
 * Weights: ccdm_pack_stem_weight(oihw [Cout, Cin <= 4, 3, 3]).
 * ------------------------------------------------------------------------------------------------- */
typedef struct ccdm_stem_args {
    const uint8_t* xt;          /* dev [N,H*W] class index of x_t */
    const float* xin;           /* dev NHWC fp32 [N,H,W,Cs]; channels [K, Cs): the conditioning image (zero beyond it) */
    int32_t Cs, K;
    const void* w; const float* bias;
    int32_t N, H, W, Cout;
    float* out;                 /* dev [N,H,W,Cout] */
    double* out_stats; int32_t out_slices;
} ccdm_stem_args;
int ccdm_stem_conv_supported(int Cs, int Cout, int H, int W, int prec);
size_t ccdm_pack_stem_weight(const float* oihw, int Cout, int Cin, void* out);      /* out == NULL: returns the byte count */
int ccdm_stem_conv(const ccdm_stem_args* a, void* stream);

/* F16X3 range diagnostics: max |a| over everything this conv stages — the main input after GroupNorm (+ SiLU) where it normalises on
 * load, raw otherwise, and the raw input of the fused 1x1 skip segment — before the kernel's 2^4 pre-scale; Inf if any value is not
 * finite.  The result is max'ed INTO *out (dev float, >= 0: zero it first); the split is exact for values below CCDM_F16X3_LIMIT.
 * Not on the sampling path: tools/range_report.py and the host's per-layer fp32 fallback call it. */
#define CCDM_F16X3_LIMIT 4094.0f
int ccdm_conv_input_absmax(const ccdm_conv_args* a, float* out /*dev [1]*/, void* stream);

/* host-side weight packing.  `oihw` = reference layout [Cout,Cin,k,k] (conv2d) / [Cout,Cin,1] (conv1d).
 * Returns the packed size in bytes (call with out=NULL to query). */
size_t ccdm_pack_conv_weight(const float* oihw, int Cout, int Cin, int ksize, int prec, void* out);
/* same, with the per-output-channel max|W| given by the caller (dev-independent host array [Cout], or NULL): two weight
 * sets that accumulate into one GEMM (conv + fused skip) must share their F16X3 power-of-two pre-scale. */
size_t ccdm_pack_conv_weight_ex(const float* oihw, int Cout, int Cin, int ksize, int prec, const float* cout_absmax, void* out);

/* ---------------------------------------------------------------------------------------------------
 * Self-attention core over tokens, softmax(q k^T * ch^-1/2) v per head, streaming (score matrix never in HBM).
 * qkv: [N,T,3C] (the qkv 1x1 conv output, NHWC), out: [N,T,C].
 * order 0 = QKVAttentionLegacy (channel = head*3ch + {q,k,v}*ch + c, unet.py:343-360),
 * order 1 = QKVAttention        (channel = {q,k,v}*C + head*ch + c,   unet.py:376-395).
 * order | CCDM_ATTENTION_FORCE_VALU: the vector-pipe kernel (plain fp32 FMAs, head widths 4, 8, 12, 16, 24, 32, 48, 64) instead of the
 * matrix-core one, whose fp16 hi/lo split of q, k, v has the range of CCDM_PREC_F16X3 — what the host pins an attention core to
 * whose operands left that range ("<block>.attention" in DenoisingModel.f32_layers).
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_ATTENTION_FORCE_VALU 256
int ccdm_attention(const float* qkv, float* out, int N, int T, int C, int heads, int order, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * First half of an AttentionBlock in one launch, for the low-resolution stages:
 *     a = attention(qkv(GroupNorm32(x)))                                          unet.py:291-311, core :343-360 / :376-395
 * One workgroup per (sample, head): GroupNorm on load, the head's 96 rows of the qkv 1x1 conv and softmax(q k^T) v run out of
 * registers and LDS; the 3C-wide qkv tensor never reaches memory.  proj_out + residual remain a ccdm_conv2d (1x1, resid = x).
 * Built for head width 32 and (T, C) in {64,256} x {96,128} and 128 x {128,256} — ccdm_norm_qkv_attention_supported(); every
 * other geometry runs as ccdm_conv2d (GN + qkv) -> ccdm_attention.  CCDM_PREC_F16X3 arithmetic.
 *   wqkv : qkv.weight [3C,C,1] with rows in LEGACY order (channel = head*96 + {q,k,v}*32 + d; the host permutes the rows of a
 *          `use_new_attention_order` model), packed by ccdm_pack_conv_weight(…, Cout=3C, Cin=C, ksize=1, CCDM_PREC_F16X3); bqkv alike.
 * ------------------------------------------------------------------------------------------------- */
typedef struct ccdm_attn_block_args {
    const float* x;                                  /* dev [N,T,C] block input (NHWC, T = h*w) */
    const double* stats; int32_t slices;             /* dev [N,slices,C,2] partial statistics of x */
    const float* gamma; const float* beta; float eps;/* AttentionBlock.norm */
    const void* wqkv; const float* bqkv;             /* packed qkv weights (see above), dev [3C] bias in legacy order */
    float* out;                                      /* dev [N,T,C] attention output, channel = head*32 + d */
    int32_t N, T, C, heads;
} ccdm_attn_block_args;
int ccdm_norm_qkv_attention_supported(int T, int C, int heads);
int ccdm_norm_qkv_attention(const ccdm_attn_block_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Time conditioning for a list of steps (depends only on t, so computed once per run):
 *   emb = Linear(SiLU(Linear(sinusoid(t))))                  unet.py:506-510,:758
 *   out[s] = Wcat * SiLU(emb) + bcat                          all ResBlock.emb_layers at once, unet.py:205-211,:250
 * `sinus` is timestep_embedding(t, model_channels) (nn.py:103-121), evaluated by the host with the same torch
 * ops as the reference: t*freq reaches 1e3 rad, so a 1-ulp difference in exp() would already move cos/sin
 * by 1e-5 — the table is [S, mc] floats, not worth a second libm.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_time_table(const float* sinus /*dev [S,mc]*/, int S, int model_channels,
                    const float* w0, const float* b0, const float* w2, const float* b2,  /* dev, reference [out,in] layout */
                    const float* wcat /*dev [E,4mc]*/, const float* bcat /*dev [E]*/, int E,
                    float* emb_out /*dev [S,4mc] or NULL*/, float* out /*dev [S,E]*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused epilogue of one denoise step, one thread per pixel:
 *   x0 = softmax_K(head) (or head itself)                                     unet.py:706
 *   P  = theta_post_prob(x_t, x0, t)   (O(K) closed form, in registers)       diffusion_denoising.py:99-128
 *   P  = max(P, 1e-12); P^ = P / sum_K P                                      :204 ; torch Categorical
 *   t>1 : x_{t-1} = argmax_k P^_k / E_k (first index wins)                    one_hot_categorical.py:30-32
 *   t==1: "confidence" -> P^ (fp32) ; "majority" -> one_hot(argmax P^) int64  :46-54 ; diffusion_denoising.py:208-212
 * E is read from `noise` (host-drawn Exp(1), order ((n*H+h)*W+w)*K+k) or generated with Philox4x32-10.
 * ------------------------------------------------------------------------------------------------- */
enum { CCDM_STEP_SAMPLE = 0, CCDM_STEP_LAST_CONFIDENCE = 1, CCDM_STEP_LAST_MAJORITY = 2, CCDM_STEP_LAST_KEEP = 3,
       CCDM_STEP_SOFTMAX_ONLY = 4 /* out_probs = x0 (the U-Net output itself): forward_step, diffusion_denoising.py:161-162 */ };

/* The per-run fields of the epilogue as a DEVICE-resident block (ABI 7).  With ccdm_post_args.run set the kernel reads these eight
 * values from the block instead of the argument struct, like it reads the step row through step_ptr: a captured HIP graph of the
 * denoise step then survives a new Philox key, another noise buffer or another output pointer (the host rewrites the block with
 * a stream-ordered one-thread launch; nothing is re-captured, nothing is destroyed while earlier launches are in flight). */
typedef struct ccdm_post_run {
    const float* noise; int64_t noise_step_stride;
    uint64_t philox_seed; uint32_t sample_offset; int32_t noise_row0;
    float* out_probs; int64_t* out_onehot; float* posterior_out;
} ccdm_post_run;

#define CCDM_MAX_CLASSES 255        /* x_t is a uint8 class index; K <= 32 keeps a pixel's classes in registers, more go through LDS rows */
#define CCDM_POST_DIAG_MANY 256     /* diagnostic bit of ccdm_post_args.softmax: run the many-class (LDS-row) kernel at any K (parity tests) */
typedef struct ccdm_post_args {
    const float* head;           /* dev [N,HW,head_stride] head conv output (logits, or probabilities if !softmax), first K channels used */
    int32_t softmax;             /* bit 0: apply softmax over K first (| CCDM_POST_DIAG_MANY) */
    int32_t head_stride;         /* floats per pixel of `head` (>= K; the head conv pads K up to a multiple of 4) */
    const uint8_t* xt;           /* dev [N,HW] class index of x_t */
    int32_t N, HW, K;
    /* per-step coefficients: row = *step_ptr (0 if NULL) of step_table = {alpha_t, cumalpha_tm1, mode, 0} */
    const float* step_table; const int32_t* step_ptr;
    /* noise */
    const float* noise; int64_t noise_step_stride;        /* dev or NULL -> Philox; row r of the buffer is step row noise_row0 + r */
    uint64_t philox_seed; uint32_t sample_offset;         /* global index of sample 0 (batch sharding) */
    /* outputs */
    uint8_t* xt_next;            /* dev [N,HW] (may alias xt) */
    float* xin; int32_t xin_stride;  /* dev [N,HW,xin_stride]: one-hot written to channels [0,K) ; or NULL */
    float* out_probs;            /* dev [N,HW,K] fp32   (confidence) or NULL */
    int64_t* out_onehot;         /* dev [N,HW,K] int64  (majority)   or NULL */
    float* posterior_out;        /* dev [N,HW,K] optional debug/teacher-forcing tap of P^ , or NULL */
    int32_t noise_row0;          /* step row the first row of `noise` belongs to (host noise uploaded in blocks of steps) */
    int32_t* range_flag;         /* dev scalar or NULL: set to 1 (sticky, never cleared by the kernel) when the head output of
                                    any pixel is not finite — the signature of an F16X3 range overflow upstream (see above) */
    const ccdm_post_run* run;    /* dev block or NULL: when set, noise / noise_step_stride / noise_row0 / philox_seed / sample_offset /
                                    out_probs / out_onehot / posterior_out are read from it and the fields above are ignored */
} ccdm_post_args;

int ccdm_posterior_sample(const ccdm_post_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The head of the U-Net and the epilogue above in ONE launch, for few classes (9 K <= 32) and 32 head channels, CCDM_PREC_F16X3:
 *     logits = conv3x3(SiLU(GroupNorm32(x))) + bias   (self.out, unet.py:701-707)   ->   ccdm_posterior_sample's arithmetic on them
 * (the same device function: identical bits from identical logits); the logits never reach memory.  The conv's taps are the N
 * dimension of a 1x1 product over the halo tile (9 K columns), summed per pixel afterwards: results equal the general kernel's to fp32
 * rounding.  `post` is a ccdm_post_args whose head / head_stride / xin fields are unused (x_t travels as the uint8 index).
 * Built for C == 32, 2 <= K <= 3, H % 8 == 0, W % 32 == 0 (ccdm_head_posterior_supported).  Weights: ccdm_pack_head_weight.
 * ------------------------------------------------------------------------------------------------- */
typedef struct ccdm_head_args {
    const float* x;             /* dev NHWC fp32 [N,H,W,C]: the last ResBlock's output */
    const double* stats; int32_t slices;        /* its partial statistics [N,slices,C,2] */
    const float* gamma; const float* beta; float eps;       /* out.0 (GroupNorm32) */
    const void* w; const float* bias;           /* out.2: ccdm_pack_head_weight(oihw [K,C,3,3]); dev [K] */
    int32_t N, H, W, C, K;
    float* logits_out;          /* dev [N,H*W,K] optional tap of the logits (tests), or NULL */
} ccdm_head_args;
int ccdm_head_posterior_supported(int C, int K, int H, int W, int prec);
size_t ccdm_pack_head_weight(const float* oihw, int K, int Cin, void* out);         /* out == NULL: returns the byte count */
int ccdm_head_posterior(const ccdm_head_args* a, const ccdm_post_args* post, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Sampling with known pixel labels (DenoisingModel(..., known_labels=)): the replacement method of RePaint (Lugmayr et al. 2022) for
 * categorical diffusion.  Launched after a denoise step has left x_{t-1} in `xt`: every pixel whose `known` byte is a class y < K is
 * overwritten with a draw from the forward process at that step's noise level,
 *     q(x_{t-1} | x_0 = y) = Cat(c * onehot(y) + (1 - c) / K),   c = cumalpha_{t-1} (column 1 of the step's table row);
 * a pixel whose byte is >= K (255 = free; any other byte that is no class too) is not touched in any buffer.  One thread per pixel.
 *   mode == CCDM_STEP_SAMPLE: p_k = (k == y) ? p_hit : p_miss, x = argmax_k p_k / E_k (fp32 IEEE division, first maximum wins: the
 *     epilogue's Exp(1) race) with E_k = -log(U) of word k % 4 of Philox4x32-10(counter = (pixel, sample_offset + n, step_row,
 *     0x80000000 | k / 4), key = philox_seed) — the epilogue's own blocks have a fourth counter word < 64, so the two draws of a pixel
 *     and step never share a block.  The host forms p_miss = (1 - c) / K and p_hit = c + (1 - c) / K in float64 and rounds each to
 *     fp32 once.  Writes xt[i] = x and, if xin != NULL, the one-hot into xin[i * xin_stride + 0 .. K) (channels >= K: the image, untouched).
 *   the three last-step modes (c = 1, nothing is drawn): xt[i] = y; one-hot of y into out_probs (fp32) / out_onehot (int64) / xin,
 *     each if non-NULL.
 * K in [1, CCDM_MAX_CLASSES]; xin_stride >= K where xin is given.  Results depend on (pixel, global sample index, step row, key) only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_known_labels_step(const uint8_t* known /*dev [N,HW]: class < K = known, 255 = free*/, int N, int HW, int K,
                           float p_hit, float p_miss, int mode /*CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP*/,
                           int step_row, uint64_t philox_seed, uint32_t sample_offset,
                           uint8_t* xt /*dev [N,HW]*/, float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride,
                           float* out_probs /*[N,HW,K] or NULL*/, int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Resampling jumps of a walk with known labels (DenoisingModel(..., known_labels=, resample=(jump_length, resamples))): RePaint's
 * harmonisation.  The walk goes back up the chain by `jump_length` levels and down again, so that the free pixels are denoised once
 * more with the known ones in view.  Going up is this kernel: EVERY pixel of `xt`, known or free (a known pixel's state is a sample of
 * q(x_t | x_0 = y), and renoising it keeps it one), is redrawn from the forward process between the two levels,
 *     x_new ~ Cat(p_k),  p_k = p_stay for k == xt[i], p_move otherwise,
 *     p_move = (1 - r) / K,  p_stay = r + p_move,  r = cumalpha_{t of the level reached} / cumalpha_{t of the level left}
 * (formed by the host in float64, each rounded to fp32 once): uniform transition kernels compose in closed form, so a jump of any
 * length is ONE launch.  The draw is the epilogue's Exp(1) race, x_new = argmax_k p_k / E_k (fp32 IEEE division, first maximum wins)
 * with E_k = -log(U) of word k % 4 of Philox4x32-10(counter = (pixel, sample_offset + n, step_row, 0x40000000 | k / 4), key =
 * philox_seed): a counter range of its own (the epilogue's fourth word is < 64, the clamp's has bit 31 set).  step_row = the table row
 * the walk continues at.  Writes xt[i] = x_new and, if xin != NULL, the one-hot into xin[i * xin_stride + 0 .. K) (channels >= K: the
 * image, untouched).  A byte xt[i] >= K on entry is a caller's error the host never makes; it is treated as class K - 1.
 * Keying of a revisit: the epilogue keys its noise by the table row, so a row that is walked again must not see the same key.  Every
 * launch of pass p of a row (the denoise step, its clamp, and the renoise that precedes it) runs under pass_key(key, p): the call's key
 * itself for p = 0, and for p >= 1 the splitmix64 finaliser of key + 0xD1342543DE82EF95 * p (mod 2^64) — the finaliser that derives a
 * call's key from (philox_seed, philox_call), on another increment: call 0's key is the seed itself, so under the call counter's
 * increment 0x9E3779B97F4A7C15 pass p of call 0 would run under call p's key.
 * One thread per pixel; without xin one thread per 4 consecutive pixels of the flat map (one 32-bit load and store, where xt is 4-byte
 * aligned; the last N*HW % 4 bytes one by one).  K in [1, CCDM_MAX_CLASSES]; xin_stride >= K where xin is given.  Results depend on
 * (pixel, global sample index, step row, key) only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_renoise_step(int N, int HW, int K, float p_stay, float p_move, int step_row, uint64_t philox_seed, uint32_t sample_offset,
                      uint8_t* xt /*dev [N,HW]*/, float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Sampling under per-pixel soft evidence (DenoisingModel(..., evidence=)).  The network's x0 = p(x_0 | x_t) of a pixel and independent
 * evidence e with likelihood p(e | x_0 = k) proportional to w_k give p(x_0 | x_t, e) proportional to x0_k * w_k (Bayes); the reverse
 * step's posterior is linear in that vector up to its final normalisation, so the guided step is the unguided one on x0 * w.
 * Launched after a denoise step whose table row has mode CCDM_STEP_SOFTMAX_ONLY has left x0 in out_probs (and x_t untouched in `xt`).
 * Per pixel:
 *   x0'_k = x0_k * evidence_k      one fp32 multiply, no renormalisation (the scale cancels in the step's own normalisation);
 *   then ccdm_posterior_sample's arithmetic with softmax = 0 on x0' (the same device function: posterior in the documented op order
 *   with alpha_t / cumalpha_tm1 as given, clamp at 1e-12, cascade normalisation), and by `mode`
 *   CCDM_STEP_SAMPLE:          the Exp(1) race with the counters of the unguided step of that row, Philox4x32-10(counter = (pixel,
 *                              sample_offset + n, step_row, k / 4), key = philox_seed); writes xt[i] and, if xin != NULL, the one-hot
 *                              into xin[i * xin_stride + 0 .. K) (channels >= K: the image, untouched);
 *   CCDM_STEP_LAST_CONFIDENCE: the probabilities into out_probs (if non-NULL);
 *   CCDM_STEP_LAST_MAJORITY:   the argmax one-hot into out_onehot (if non-NULL), its index into xt;
 *   CCDM_STEP_LAST_KEEP:       nothing.
 * x0 and out_probs may be the same buffer: a pixel's K values are read completely before any of them is written.  All-ones evidence
 * gives the bits of the unguided step.  K in [1, CCDM_MAX_CLASSES]; xin_stride >= K where xin is given; CCDM_STEP_SOFTMAX_ONLY is
 * refused.  K <= 4: one thread per pixel; above, a block's pixels are staged through LDS so that global loads and the one-hot stores
 * are contiguous.  Results depend on (pixel, global sample index, step row, key) only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_evidence_step(const float* x0 /*dev [N,HW,K]*/, const float* evidence /*dev [N,HW,K], weights in [0,1]*/, int N, int HW, int K,
                       float alpha_t, float cumalpha_tm1, int mode /*CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP*/,
                       int step_row, uint64_t philox_seed, uint32_t sample_offset,
                       uint8_t* xt /*dev [N,HW]: x_t in, x_{t-1} out*/, float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride,
                       float* out_probs /*[N,HW,K] or NULL*/, int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Temperature and truncation ("top-r") sampling (DenoisingModel(..., temperature=, truncation=)): the network's x0 of a pixel is
 * reshaped before the reverse step.  The step's posterior is linear in x0 up to its final normalisation, so the reshaped row is handed
 * to the step as it is, without renormalising.  Launched like ccdm_evidence_step, after a denoise step whose table row has mode
 * CCDM_STEP_SOFTMAX_ONLY; where the call has evidence too, this launch replaces the evidence launch.  THE definition, per pixel, fp32:
 *   v_k = x0_k, or x0_k * evidence_k where evidence != NULL (ccdm_evidence_step's multiply).
 *   Temper (skipped when inv_temperature == 1.0f; inv_temperature = 1 / temperature):
 *     m = max_k v_k; if m == 0 the row stays as it is; otherwise u_k = v_k / m (IEEE division) and
 *     q_k = 1 where u_k == 1, 0 where u_k == 0, else u_k^inv_temperature formed as exp2f(inv_temperature * log2f(u_k)).
 *     Tempering is relative to the pixel's largest value: the winner is exactly 1 and no row underflows to all zeros.
 *     Without tempering q_k = v_k.
 *   Truncate (skipped when top_r == 1.0f):
 *     Z = q_0 + q_1 + ... + q_{K-1} summed sequentially in index order; theta = top_r * Z (one multiply);
 *     the classes ordered by q descending, ties by index ascending: pi(0), pi(1), ...; c_0 = 0, c_{j+1} = c_j + q_pi(j);
 *     class pi(j) is KEPT iff c_j < theta — the smallest prefix whose mass reaches top_r; the top class is always kept when Z > 0.
 *     A dropped class becomes 0, a kept value is not changed, nothing is renormalised (the scale cancels in the step).
 *   Step: ccdm_posterior_sample's arithmetic with softmax = 0 on the shaped row, alpha_t / cumalpha_tm1 / mode as given and the Philox
 *     counters of the unguided step of that row — exactly as ccdm_evidence_step; the outputs per `mode` are that entry's.
 * Consequences: (inv_temperature, top_r) = (1, 1) is the plain step bit for bit without evidence and ccdm_evidence_step bit for bit
 * with it; a top_r small enough to keep one class makes x0 one-hot(argmax v), and the draw is ccdm_posterior_sample on that row bit
 * for bit; the last-step modes see the shaped row too (majority: the argmax of the shaped posterior; confidence: the shaped posterior).
 * x0 and out_probs may be the same buffer.  Refused: what ccdm_evidence_step refuses (evidence may be NULL), an inv_temperature that
 * is not finite or outside [1/20, 20], a top_r that is not finite or outside (0, 1].  K <= 32: the shaping runs in registers; above, in
 * the pixel's LDS row.  Results depend on (pixel, global sample index, step row, key) only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_shaped_step(const float* x0 /*dev [N,HW,K]*/, const float* evidence /*dev [N,HW,K], weights in [0,1], or NULL*/, int N, int HW, int K,
                     float inv_temperature, float top_r, float alpha_t, float cumalpha_tm1,
                     int mode /*CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP*/, int step_row, uint64_t philox_seed,
                     uint32_t sample_offset, uint8_t* xt /*dev [N,HW]: x_t in, x_{t-1} out*/,
                     float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride, float* out_probs /*[N,HW,K] or NULL*/,
                     int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Flip-averaged sampling (DenoisingModel(..., views=)): the denoiser is averaged over V mirror images of its input, which makes it
 * exactly equivariant under those flips.  The V views of a sample are V rows of a larger batch, view-major: row v * N + n is view v of
 * sample n, fed x_t and the image mirrored as view v says; view 0 is the identity.  Launched like ccdm_shaped_step, after a denoise step
 * (on all V * N rows) whose table row has mode CCDM_STEP_SOFTMAX_ONLY, and in its place: this launch applies the evidence and the
 * shaping too.  `flips` holds 2 bits per view, view v at bits 2v and 2v + 1: fx_v = bit 0 mirrors x, fy_v = bit 1 mirrors y.
 * THE definition, per sample n < N and pixel (y, x) of the identity view, fp32:
 *   src_v = (fy_v ? H - 1 - y : y) * W + (fx_v ? W - 1 - x : x)                      the pixel of view v that shows (y, x); src_0 = y * W + x
 *   m_k = (((x0[0 * N + n][src_0][k] + x0[1 * N + n][src_1][k]) + ...) * fp32(1 / V)  summed in view order, one multiply at the end
 *   then ccdm_shaped_step's arithmetic on the row m: v_k = m_k, or m_k * evidence[n][y * W + x][k] where evidence != NULL; temper and
 *   truncate (each skipped at its neutral value); ccdm_posterior_sample's arithmetic with softmax = 0 on the shaped row, x_t =
 *   xt[0 * N + n][src_0], alpha_t / cumalpha_tm1 / mode as given, and the Philox counters of the unguided step of that row for pixel
 *   y * W + x and sample sample_offset + n: the draw is keyed as a call without views keys it, never by the engine row.
 *   Nothing is renormalised (a mean of probability vectors is one, and the scale cancels in the step anyway).
 * Outputs.  CCDM_STEP_SAMPLE: the drawn class goes to xt[v * N + n][src_v] for every view v < V, and where xin != NULL its one-hot to
 * channels [0, K) of xin[v * N + n][src_v]; channels >= K are not touched.  CCDM_STEP_LAST_CONFIDENCE: the posterior goes to
 * out_probs[n][y * W + x], xt is not touched.  CCDM_STEP_LAST_MAJORITY: the one-hot of the posterior's argmax goes to
 * out_onehot[n][y * W + x] and its index to xt[v * N + n][src_v] for every view.  CCDM_STEP_LAST_KEEP: nothing is written.
 * out_probs and out_onehot cover the view-0 rows, [N,HW,K]; rows v * N + n, v >= 1, of a larger buffer are not touched.
 * x0 and out_probs may be the same buffer: a pixel's V * K values are read before anything of the pixel is written, only view-0 rows are
 * written, each by the thread that owns the pixel, and nothing else reads those rows.
 * Consequences.  V = 1 is ccdm_shaped_step bit for bit.  V = 2 or 4 with views whose x0 are exact mirror images of view 0 is
 * ccdm_shaped_step on view 0 bit for bit (a sum of 2 or 4 equal values times 1/2 or 1/4 is exact), and the xt rows of all views are
 * mirror images of one another — as they are after every launch, whatever x0 holds.  V = 2: a + b is commutative, so m for a call on
 * mirrored inputs is the mirror of m for the original call, bit for bit (V = 3, 4: the sum's order breaks that in the last bit).
 * Refused: what ccdm_shaped_step refuses, CCDM_STEP_SOFTMAX_ONLY, V outside [1,4], non-zero bits for view 0 or bits beyond view V - 1,
 * V * N * H * W > 2^31 - 1.  Results depend on (pixel, global sample index, step row, key) only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_views_step(const float* x0 /*dev [V*N,HW,K]*/, const float* evidence /*dev [N,HW,K], weights in [0,1], or NULL*/, int N, int H, int W,
                    int K, int V, int flips, float inv_temperature, float top_r, float alpha_t, float cumalpha_tm1,
                    int mode /*CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP*/, int step_row, uint64_t philox_seed,
                    uint32_t sample_offset, uint8_t* xt /*dev [V*N,HW]: x_t in, x_{t-1} out*/,
                    float* xin /*dev [V*N,HW,xin_stride] or NULL*/, int xin_stride, float* out_probs /*[N,HW,K] or NULL*/,
                    int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Tiled sampling of a canvas larger than the engine's geometry (DenoisingModel(..., tiles=)), the MultiDiffusion construction (Bar-Tal
 * et al. 2023) for categorical diffusion: ONE chain runs on the canvas, at every reverse step the denoiser is evaluated on overlapping
 * tiles of the current canvas state, the tiles' x0 are averaged per canvas pixel and one draw is made per canvas pixel.  A mean of
 * probability vectors is one and the step posterior is linear in x0 up to its own normalisation, so the tiled step is the step on the
 * per-pixel mean of the covering tiles' x0.
 * THE geometry (host: guidance.tile_origins; the kernel derives the same origins from the six integers).  Canvas Hc x Wc, tile h x w,
 * strides sy, sx with 1 <= sy <= h <= Hc and 1 <= sx <= w <= Wc:
 *   Ty = 1 + ceil((Hc - h) / sy) tiles along y with origins oy_i = min(i * sy, Hc - h): the last tile is pushed back so that it ends at
 *   the border; the origins are distinct and leave no gap.  The same along x: Tx, ox_j = min(j * sx, Wc - w).
 *   Tile r = i * Tx + j, R = Ty * Tx.  Tile r COVERS canvas pixel (y, x) iff oy_i <= y < oy_i + h and ox_j <= x < ox_j + w;
 *   c(y, x) >= 1 is the number of covering tiles.
 * The R tiles of a sample are R rows of a larger batch of h x w rows, tile-major: row r * N + n is tile r of sample n, fed the crops of
 * the canvas state and of the image.  Launched like ccdm_views_step, after a denoise step (on all R * N rows) whose table row has mode
 * CCDM_STEP_SOFTMAX_ONLY, and in place of the evidence / shaped launch.
 * THE definition, per sample n < N and canvas pixel (y, x), fp32:
 *   m_k = (sum over the covering tiles in ascending r of x0[r * N + n][(y - oy_i) * w + (x - ox_j)][k]) * fp32(1 / c(y, x))
 *         a sequential sum, one multiply at the end (by 1.0f where c = 1);
 *   then ccdm_shaped_step's arithmetic on the row m, as ccdm_views_step does it: v_k = m_k, or m_k * evidence[n][y * Wc + x][k] where
 *   evidence != NULL; temper and truncate (each skipped at its neutral value); ccdm_posterior_sample's arithmetic with softmax = 0 on
 *   the shaped row, x_t = canvas_xt[n][y * Wc + x], alpha_t / cumalpha_tm1 / mode as given, and the Philox counters of the unguided
 *   step of that row for pixel y * Wc + x and sample sample_offset + n: the draw is keyed by the canvas pixel, never by an engine row
 *   or tile.
 * Outputs.  CCDM_STEP_SAMPLE: the drawn class goes to canvas_xt[n][y * Wc + x] and to xt[r * N + n][(y - oy_i) * w + (x - ox_j)] for
 * every covering tile, and where xin != NULL its one-hot to channels [0, K) of xin at that tile pixel; channels >= K are not touched.
 * CCDM_STEP_LAST_CONFIDENCE: the posterior goes to the canvas out_probs.  CCDM_STEP_LAST_MAJORITY: the one-hot of the posterior's
 * argmax goes to the canvas out_onehot and its index to canvas_xt and the covering tiles' xt.  CCDM_STEP_LAST_KEEP: nothing is written.
 * Every tile pixel maps to exactly one canvas pixel, so every byte and every one-hot row has one writer.  The tiles' x0 is only read;
 * the canvas out_probs is another buffer.
 * Consequences.  One tile that is the canvas (h = Hc, w = Wc) is ccdm_shaped_step bit for bit.  With sy = h / 2, sx = w / 2 and a canvas
 * that is a multiple of the strides c is in {1, 2, 4}: tiles whose x0 are exact crops of one canvas-shaped x0 give ccdm_shaped_step on
 * that x0 bit for bit (a sum of 2 or 4 equal values times 1/2 or 1/4 is exact).  After every launch each tile's xt is the crop of
 * canvas_xt, whatever x0 holds.
 * Refused: what ccdm_shaped_step refuses, CCDM_STEP_SOFTMAX_ONLY, a tile larger than the canvas, a stride < 1 or larger than the tile,
 * N * Hc * Wc or R * N * h * w > 2^31 - 1.  Results depend on (canvas pixel, global sample index, step row, key) and the geometry only.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_tiled_step(const float* x0 /*dev [R*N,h*w,K]*/, const float* evidence /*dev [N,Hc*Wc,K], weights in [0,1], or NULL*/, int N, int Hc,
                    int Wc, int h, int w, int sy, int sx, int K, float inv_temperature, float top_r, float alpha_t, float cumalpha_tm1,
                    int mode /*CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP*/, int step_row, uint64_t philox_seed,
                    uint32_t sample_offset, uint8_t* canvas_xt /*dev [N,Hc*Wc]: x_t in, x_{t-1} out*/, uint8_t* xt /*dev [R*N,h*w]*/,
                    float* xin /*dev [R*N,h*w,xin_stride] or NULL*/, int xin_stride, float* out_probs /*[N,Hc*Wc,K] or NULL*/,
                    int64_t* out_onehot /*[N,Hc*Wc,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The reverse step of a sampling queue (serving.SamplingQueue): continuous batching.  The N rows of an engine are SLOTS; each holds
 * one sample of some request at its own place in its own walk, or nothing.  Launched like ccdm_shaped_step, after a denoise step whose
 * table row has mode CCDM_STEP_SOFTMAX_ONLY (the network pass of slot n ran at time-embedding row emb_row_of_sample[n]): it does the
 * reverse step of every slot with that slot's own parameters, read from a device table of one 32-byte row per slot.
 * THE definition.  For slot n with table[n].mode one of the four real step modes, the launch leaves in xt, in channels [0, K) of xin
 * and in rows [n * HW, (n + 1) * HW) of out_probs / out_onehot exactly the bits that
 *     ccdm_shaped_step(x0 + n * HW * K, NULL, 1, HW, K, 1.0f, 1.0f, alpha_t, cumalpha_tm1, mode, step_row, key_hi << 32 | key_lo,
 *                      sample, xt + n * HW, xin + n * HW * xin_stride, xin_stride, out_probs + n * HW * K, out_onehot + n * HW * K)
 * leaves (the same device function on the same values: posterior in the documented op order, clamp, cascade normalisation, the Exp(1)
 * race with Philox4x32-10(counter = (pixel, sample, step_row, k / 4), key)): the draw is keyed by the slot's request, its global sample
 * index and the row of its own walk, never by the slot.  For a slot whose mode is CCDM_SLOT_IDLE — or any value that is no real step
 * mode — nothing of the slot is read and nothing written, in any buffer.  Channels >= K of xin are never touched.
 * x0 and out_probs may be the same buffer (in the engine they are): a pixel's K values are in registers, or its block's in LDS behind a
 * barrier, before its out_probs row is written.  K <= 4: one thread per pixel; K <= 32: 256 pixels per block staged through LDS;
 * above: 64 pixels per block.  A block's pixels may belong to several slots: the slot is found per pixel, the staging passes run per
 * slot segment of the block.  Refused: a null x0 / table / xt, N or HW < 1, N * HW > 2^31 - 1, K outside [1, CCDM_MAX_CLASSES],
 * xin_stride < K where xin is given.  The table's contents are the caller's: they are not checked on the host.
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_SLOT_IDLE (-1)         /* ccdm_slot_row.mode of a slot that holds nothing */
typedef struct ccdm_slot_row {
    float alpha_t; float cumalpha_tm1;      /* the two coefficients of the slot's current row (DiffusionModel.posterior_coeffs) */
    int32_t mode;                           /* CCDM_STEP_SAMPLE | _LAST_CONFIDENCE | _LAST_MAJORITY | _LAST_KEEP, or CCDM_SLOT_IDLE */
    int32_t step_row;                       /* the row index in the slot's own walk: the third Philox counter word */
    uint32_t key_lo; uint32_t key_hi;       /* the Philox key of the slot's request */
    uint32_t sample;                        /* the global sample index: the second Philox counter word */
    uint32_t reserved;
} ccdm_slot_row;
int ccdm_slots_step(const float* x0 /*dev [N,HW,K]*/, const ccdm_slot_row* table /*dev [N]*/, int N, int HW, int K,
                    uint8_t* xt /*dev [N,HW]: x_t in, x_{t-1} out*/, float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride,
                    float* out_probs /*[N,HW,K] or NULL*/, int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The reverse step of a GUIDED sampling queue (serving.SamplingQueue(..., guided=True)): ccdm_slots_step with every slot's own
 * guidance.  Launched like ccdm_slots_step and takes its table unchanged; beside it a second device table of one 32-byte row per slot
 * and two slot-indexed pools (plain pointers: no per-slot device pointer is ever put into a table — a stale row of a pool is a wrong
 * but harmless read, a stale pointer would be a fault).
 * THE definition.  For slot n with table[n].mode one of the four real step modes the launch leaves in xt, in channels [0, K) of xin and
 * in rows [n * HW, (n + 1) * HW) of out_probs / out_onehot exactly the bits that, with g = guide[n] and the pointers of ccdm_slots_step's
 * definition (each offset to the slot),
 *     ccdm_shaped_step(x0, g.flags & CCDM_SLOT_GUIDE_EVIDENCE ? evidence + n * HW * K : NULL, 1, HW, K, g.inv_temperature, g.top_r,
 *                      alpha_t, cumalpha_tm1, mode, step_row, key, sample, xt, xin, xin_stride, out_probs, out_onehot)
 * followed, where g.flags & CCDM_SLOT_GUIDE_KNOWN, by
 *     ccdm_known_labels_step(known + n * HW, 1, HW, K, g.p_hit, g.p_miss, mode, step_row, key, sample, xt, xin, xin_stride, out_probs,
 *                            out_onehot)
 * leave: the order of a solo call (network, guided step, clamp).  Per pixel: v = x0, or x0 * evidence (one fp32 multiply); the
 * slot's shaping ((1, 1): none); the step with the slot's key, sample, step row, coefficients and mode; then, by the same thread, the
 * clamp where the pixel's `known` byte is a class < K — in CCDM_STEP_SAMPLE the Exp(1) race on (p_hit, p_miss) with fourth counter
 * word 0x80000000 | k / 4, in the last-step modes the label and its one-hot.  One launch.  Neutral guide rows — (1, 1, ., ., 0) —
 * give ccdm_slots_step bit for bit.  A slot that is idle is neither read nor written, its rows of the pools included.
 * The caller's contract (on the device, so not checked here): a pool may be NULL only while no running slot sets its flag;
 * inv_temperature in [1/20, 20] and top_r in (0, 1] are checked by the host where it forms a row (guidance.check_shaping);
 * (p_hit, p_miss) is the pair ccdm_known_labels_step documents, float64 c + (1 - c) / K and (1 - c) / K each rounded to fp32 once,
 * c = cumalpha_tm1 of the row and 1.0 on a walk's last row.
 * The three shapes of ccdm_slots_step; K <= 4: the 8- / 16-byte loads need x0 and the evidence pool aligned alike.  Refused: what
 * ccdm_slots_step refuses, a null guide table, a table or the evidence pool not 4-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_SLOT_GUIDE_EVIDENCE 1  /* ccdm_slot_guide_row.flags: the slot's row of the evidence pool multiplies its x0 */
#define CCDM_SLOT_GUIDE_KNOWN 2     /* the slot's row of the known pool is clamped */
typedef struct ccdm_slot_guide_row {
    float inv_temperature; float top_r;     /* the slot's shaping as ccdm_shaped_step takes it; (1, 1): none */
    float p_hit; float p_miss;              /* the clamp's pair of the slot's current row; read only with CCDM_SLOT_GUIDE_KNOWN */
    int32_t flags;                          /* CCDM_SLOT_GUIDE_* */
    int32_t reserved[3];                    /* zero */
} ccdm_slot_guide_row;
int ccdm_slots_guided_step(const float* x0 /*dev [N,HW,K]*/, const ccdm_slot_row* table /*dev [N]*/,
                           const ccdm_slot_guide_row* guide /*dev [N]*/, const float* evidence /*dev [N,HW,K] or NULL*/,
                           const uint8_t* known /*dev [N,HW]: class < K = known, 255 = free; or NULL*/, int N, int HW, int K,
                           uint8_t* xt /*dev [N,HW]: x_t in, x_{t-1} out*/, float* xin /*dev [N,HW,xin_stride] or NULL*/, int xin_stride,
                           float* out_probs /*[N,HW,K] or NULL*/, int64_t* out_onehot /*[N,HW,K] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The variational bound on the likelihood of a held-out label map (DenoisingModel.label_bound):
 *     -log p(y | image) <= L_T + sum_{t=1..T} E_{x_t ~ q(x_t | x_0 = y)} l_t(y, x_t)
 * with l_t the reference's training loss (trainer.py:255-277).  Every network kernel reads its time-embedding row as rowmap[n] + step,
 * so ONE network pass holds rows at different noise levels; the two launches here sit around it and read a device table of one
 * 32-byte ccdm_bound_row per engine row.
 * THE definition.  For a label map y [HW] (class < K; any byte >= K, conventionally 255, is a pixel that is not counted), a timestep
 * t in 1..T and (a, c) = DiffusionModel.posterior_coeffs(t) (so (0, 1) at t = 1):
 *   Draw (ccdm_bound_noise).  x_t ~ q(x_t | x_0 = y) = Cat(cumalpha_t onehot(y) + (1 - cumalpha_t) / K) per pixel: the Exp(1) race of
 *     the step epilogue, argmax_k p_k / E_k with p_k = p_hit for k == y and p_miss otherwise, first maximum wins, E_k from word k % 4 of
 *     Philox4x32-10(counter = (pixel, sample, t, 0x20000000 | k / 4), key = philox_seed).  The host forms p_miss = (1 - cumalpha_t) / K
 *     and p_hit = cumalpha_t + p_miss in float64 and rounds each to fp32 once.  The tag is a range of its own (the epilogue uses fourth
 *     words < 64, the clamp 0x80000000 | k / 4, the renoise 0x40000000 | k / 4); `sample` is the global index of the (label, draw) pair,
 *     never the engine row, and the third word is the timestep itself: a draw depends on (pixel, label, draw, t, key) only, not on how
 *     rows are packed into passes.  An uncounted pixel gets x_t = pixel % K without a draw.  Only xt_out is written.
 *   Term (ccdm_bound_terms).  Per counted pixel, all in fp32, sums over k ascending, logf the accurate one:
 *       p = theta_post(x_t, onehot(y), t):       A_k = a [k == x_t] + (1 - a) / K ;  theta_k = A_k (c [k == y] + (1 - c) / K) ;  p_k = theta_k / sum theta
 *       q = theta_post_prob(x_t, x0, t):         b = (1 - c) / K ;  S = sum A_k ;  r_k = x0_k / (c A_k + b S) ;  R = sum r_k ;  q_k = A_k (c r_k + b R)
 *       l = sum_k p_k (log p_k - log max(q_k, floor)),  0 where p_k = 0
 *     — q in the O(K) closed form of the step epilogue up to and including A_k (c r_k + b R), without its clamp and normalisation, as in
 *     the trainer; floor = 1e-12 is the trainer's.  A_k takes two values and theta_k four, so S and sum theta are written out
 *     (S = (a + u) + (K - 1) u with u = (1 - a) / K, likewise sum theta: a few roundings where K equal addends in a row would make
 *     K / 2); R is the k-ascending sum, l a compensated (Kahan) sum of its K terms.  At t = 1 (a row with alpha_t = 0 and cumalpha_tm1 = 1) p = onehot(y), q = x0 and the
 *     term is evaluated as what it is, l = -logf(max(x0_y, floor)), the decoder term.  The pixel's weight is w = class_weights[y] (1
 *     without class_weights): the trainer's `mask`.  The pixel's fp32 value is w * l (0 where w = 0).
 *   Row sums.  row_sum[n] = sum_pix (double)(w l) and row_weight[n] = sum_pix (double)w over the counted pixels of engine row n, float64,
 *     accumulated from the fp32 pixel values in a fixed order: per-(block, row) partials into the workspace, folded per row by one small
 *     fixed-order launch (as ccdm_stats_fold).  No float atomics: two calls on the same inputs return the same bits.
 *   map (optional) receives the pixel's fp32 value w * l, 0 at uncounted pixels and on idle rows; nothing else of the buffer is touched.
 *   A row with t = CCDM_BOUND_IDLE (any t < 1) is idle: nothing of it is read (x0, xt, labels), no x_t is written, its sums are 0.  The
 *   table lives on the device and is not read on the host; a row whose label_row is outside [0, R) is treated as idle by both kernels,
 *   so no label row out of range is ever read (models.bound_rows refuses to build such a table).
 * The floor makes this a bound only up to pixels where some q_k < floor with p_k > 0: there the term is capped at p_k (log p_k - log floor).
 * The prior term L_T and the estimator over t (all, a subset, or stratified) are host arithmetic: models.bound_prior, models.bound_timesteps.
 * x0 is read as contiguous [pixel][class] runs through LDS rows (256 pixels per block for K <= 32, 64 above); K in [1, CCDM_MAX_CLASSES].
 * ccdm_bound_terms_workspace_bytes(N, HW, K) = 16 * (blocks + N) bytes (8-byte aligned device memory; 0 for a shape that is refused).
 * Refused before anything is launched: a null labels / table / xt_out / x0 / xt / ws / row_sum / row_weight, a table that is not 4-byte
 * aligned, N, R or HW < 1, K outside [1, CCDM_MAX_CLASSES], floor not in (0, 1), N * HW or R * HW > 2^31 - 1.
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_BOUND_IDLE (-1)        /* ccdm_bound_row.t of a row that holds nothing */
typedef struct ccdm_bound_row {
    float p_hit; float p_miss;              /* the draw, from cumalpha_t */
    float alpha_t; float cumalpha_tm1;      /* the term, posterior_coeffs(t) */
    int32_t t;                              /* timestep = third Philox word; CCDM_BOUND_IDLE: row neither read nor written, its sums 0 */
    uint32_t sample;                        /* global (label, draw) index: the second Philox word */
    int32_t label_row;                      /* row of `labels` this engine row scores: many rows share one map, nothing is gathered */
    int32_t reserved;
} ccdm_bound_row;
int ccdm_bound_noise(const uint8_t* labels /*dev [R,HW]*/, const ccdm_bound_row* table /*dev [N]*/, int N, int R, int HW, int K,
                     uint64_t philox_seed, uint8_t* xt_out /*dev [N,HW]*/, void* stream);
size_t ccdm_bound_terms_workspace_bytes(int N, int HW, int K);
int ccdm_bound_terms(const float* x0 /*dev [N,HW,K]*/, const uint8_t* xt /*dev [N,HW]*/, const uint8_t* labels /*dev [R,HW]*/,
                     const ccdm_bound_row* table /*dev [N]*/, const float* class_weights /*dev [K] or NULL*/, int N, int R, int HW, int K,
                     float floor, void* ws, double* row_sum /*dev [N]*/, double* row_weight /*dev [N]*/, float* map /*dev [N,HW] or NULL*/,
                     void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC metrics, device part: for every image and every pair (i, j) of class-index maps
 * a[img][i], b[img][j], the per-class pixel counts out[img][i][j][k] = {|a==k & b==k|, |a==k | b==k|}.
 * Replaces the [B,S,S',HW,K] boolean broadcast of `batched_distance` / `iou`
 * (evaluation/evaluate_lidc_uncertainty.py:27-39); GED and Hungarian-matched IoU follow on the host from the
 * exact integer counts.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_pairwise_class_counts(const uint8_t* a /*dev [B,S,HW]*/, const uint8_t* b /*dev [B,L,HW]*/, int B, int S, int L,
                               int HW, int K, int32_t* out /*dev [B,S,L,K,2]*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC soft-label scores, device part (beyond the reference, whose LIDC scores are all set scores): what the S samples of an
 * image imply at a pixel, p_k = n_k / S, against the L raters' soft label there, q_k = m_k / L, in one read of both stacks.
 * Per pixel p of image b:  n_k = #{s : samples[b,s,p] == k},  m_k = #{l : raters[b,l,p] == k}  for k < K; a byte >= K belongs
 * to no class.  u = S*S - sum_k n_k^2 and v = L*L - sum_k m_k^2 are the Gini impurities of the two count vectors, scaled to
 * integers.
 *   joint    int32 [B][K][S+1][L+1]: joint[b][k][n][m] = the pixels of image b with n_k == n and m_k == m.  OVERWRITTEN per call;
 *   moments  int64 [B][5]: {sum u, sum v, sum u^2, sum v^2, sum u*v} over the pixels of image b.  OVERWRITTEN per call.
 * Either output may be NULL, not both.  1 <= S, L <= 255 (the four pixels a lane takes keep their counts of a class as the
 * four bytes of a register), K in [1,32], 0 < HW < 2^31, K*(S+1)*(L+1) <= 16384 (one image's table as int32 in 64 KB of LDS;
 * LIDC at K = 2, S = 100, L = 4 needs 1010 entries).  One dword per lane and map when HW % 4 == 0 and both pointers are 4-byte
 * aligned, bytes otherwise: any alignment is accepted.  Integer arithmetic only: per-block counts in LDS, then integer atomics
 * into the outputs after a hipMemsetAsync of them on `stream`: every count is exact in any order, two identical calls are
 * bit-identical.  No workspace; B = 0 returns 0 without a launch and leaves the outputs as they are.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_lidcscore(const uint8_t* samples /*dev [B,S,HW]*/, const uint8_t* raters /*dev [B,L,HW]*/, int B, int S, int L, int HW,
                   int K, int32_t* joint /*dev [B][K][S+1][L+1] or NULL*/, int64_t* moments /*dev [B][5] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC surface-distance scores, device part (beyond the reference, whose LIDC scores are all overlap scores): the integers and
 * the two fp64 sums behind HD95, the average symmetric surface distance (ASSD) and the Hausdorff distance of every sample
 * against every rater.
 * Definition, for a class map M of shape [H,W] and a class c.  The mask is M == c.  The surface S_c(M) is the set of mask pixels
 * with at least one of their four neighbours outside the mask; a neighbour outside the image counts as outside the mask.  This
 * is mask & ~scipy.ndimage.binary_erosion(mask) with the default cross structure and border_value=0, which is MedPy's
 * __surface_distances with connectivity 1.  A byte >= K belongs to no class.
 * For image b, map i of stack A (samples [B,S,H,W]), map j of stack R (raters [B,L,H,W]) and class c:  d2(p, T) is the smallest
 * squared Euclidean pixel distance from p to a pixel of the set T, an integer.  The multiset D pools {d2(p, S_c(R_j)) : p in
 * S_c(A_i)} and {d2(p, S_c(A_i)) : p in S_c(R_j)} (MedPy's hd95 pools the two directions the same way).
 *   stats  int32 [B][S][L][C][5], C = the scored classes: 1..K-1, or class 0 when K == 1.  Per cell (b,i,j,c):
 *          {n_ar, n_ra, d2_max, d2_lo, d2_hi}.  n_ar = |S_c(A_i)|, n_ra = |S_c(R_j)|; the cell is DEFINED iff both are > 0, an
 *          undefined cell gets zeros in the remaining fields and in `sums`.  d2_max = max D.  d2_lo, d2_hi = the order statistics
 *          of D at the 0-based ranks floor(pos) and ceil(pos), pos = q_num*(n-1)/q_den, n = n_ar + n_ra, the ranks in exact
 *          integer arithmetic (q_num/q_den = 95/100: numpy's default linear-interpolation percentile).  OVERWRITTEN per call;
 *   sums   fp64 [B][S][L][C][2]: {sum_ar, sum_ra} = the sums of sqrt(d2) over each direction.  OVERWRITTEN per call.
 * The host derives  HD = sqrt(d2_max),  HDq = sqrt(d2_lo) + frac(pos)*(sqrt(d2_hi) - sqrt(d2_lo)),
 * ASSD = (sum_ar/n_ar + sum_ra/n_ra)/2 (MedPy's assd).
 * Limits: 1 <= K <= 32, 1 <= S, L <= 255, H, W <= 1024 (so d2 < 2^21), 0 < q_num <= q_den; checked before anything is launched
 * or read.  Any alignment of the stacks is accepted: one dword per lane and map row when W % 4 == 0 and both pointers are 4-byte
 * aligned, bytes otherwise.  Two stages on `stream`: once per (map, class) the exact squared distance transform to the surface
 * (1-D nearest-surface distance along rows, then the lower envelope min over y' of g(x,y')^2 + (y-y')^2 down columns) as int32 in
 * the workspace (device, 4-byte aligned, ccdm_surfdist_workspace_bytes(B,S,L,H,W,K) = 4*B*(S+L)*C*H*W bytes); then one
 * workgroup per cell takes the counts, the maximum and the sums and finds the two order statistics by an MSB-first radix select
 * over 256-bin histograms in LDS.  Integers are exact in any order; the fp64 sums are reduced in a fixed order (thread, wave,
 * block) without floating atomics: two identical calls are bit-identical.  B = 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_surfdist_workspace_bytes(int B, int S, int L, int H, int W, int K);
int ccdm_surfdist(const uint8_t* samples /*dev [B,S,H,W]*/, const uint8_t* raters /*dev [B,L,H,W]*/, int B, int S, int L, int H, int W,
                  int K, int q_num, int q_den, int32_t* stats /*dev [B][S][L][C][5]*/, double* sums /*dev [B][S][L][C][2]*/,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC lesion-level scores, device part (beyond the reference, whose LIDC scores are all overlap scores): how many lesions every
 * sample and every rater marks, and which of them the other one finds.
 * Inputs: samples uint8 [B,S,H,W] and raters uint8 [B,L,H,W], device class maps as they lie in memory; K classes; connectivity 4
 * or 8; T overlap thresholds, each a rational num/den (HOST array [T][2], read during the call).  The scored classes are 1..K-1,
 * or class 0 when K == 1: C of them, as in ccdm_surfdist.  A byte >= K belongs to no class.
 * Lesion: a lesion of a map and a class c is a connected component of the pixels equal to c under `connectivity` (4: the edge
 * neighbours, scipy's generate_binary_structure(2,1); 8: the diagonal ones too, (2,2)).  Outside the image is outside the mask.
 * Labels (stage 1, once per map and class, not per pair): int32 [H][W], 0 outside the mask, otherwise 1 + the number of lesions of
 * that map and class whose smallest pixel index y*W + x is smaller than this lesion's: lesions numbered in raster order of their
 * first pixel, which is what scipy.ndimage.label returns.
 * Cell (stage 2, per image b, sample i, rater j, class c): n_a, n_r = the lesions of the sample map and of the rater map.  For a
 * sample lesion a, size(a) is its pixel count and cov(a) the number of its pixels that have class c in the rater map; the same
 * for a rater lesion against the sample map.  A lesion is HIT at num/den iff cov >= 1 and cov*den >= num*size, in 64-bit integers:
 * 0/1 is any overlap, 1/2 at least half covered by the other mask, 1/1 wholly inside it.
 *   stats  int32 [B][S][L][C][2+2T] = {n_a, n_r, hit_a[0..T), hit_r[0..T)}: the lesions of each side and how many of them are hit
 *          at each threshold.  Every element is written, zeros included: OVERWRITTEN per call.
 * Workspace (device, 4-byte aligned, ccdm_lesions_workspace_bytes(B,S,L,H,W,K) = 4*B*(S+L)*C*(H*W + 1) bytes): first the label
 * planes int32 [B*S + B*L][C][H][W], map-major (the B*S sample maps, then the B*L rater maps), then class, then pixel; behind them
 * the lesion counts int32 [B*S + B*L][C] in the same order.  Both are valid after the call.
 * Limits, checked before anything is launched or read: 1 <= K <= 32, 1 <= S, L <= 255, H, W >= 1 and H*W <= 16384 (the LIDC map:
 * a whole map stays in the LDS of one workgroup, and a lesion's size and cov fit 16 bits each), connectivity in {4, 8}, 1 <= T <= 8,
 * 0 <= num <= den, 1 <= den <= 65536, B >= 0.  Any alignment of the stacks is accepted: one dword per lane when W % 4 == 0 and both
 * pointers are 4-byte aligned, bytes otherwise.  Two kernels on `stream`: union-find labelling, one workgroup per (map, class); then
 * one workgroup per cell counts size and cov per lesion in LDS and the hits per threshold.  Integers only, exact in any order: two
 * identical calls are bit-identical.  B = 0 returns 0 without a launch and leaves the outputs as they are.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_lesions_workspace_bytes(int B, int S, int L, int H, int W, int K);
int ccdm_lesions(const uint8_t* samples /*dev [B,S,H,W]*/, const uint8_t* raters /*dev [B,L,H,W]*/, int B, int S, int L, int H, int W,
                 int K, int connectivity, const int32_t* overlaps /*HOST [T][2]: num, den*/, int T,
                 int32_t* stats /*dev [B][S][L][C][2+2T]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC matched-lesion scores, device part (beyond the reference): which lesion of a sample is which lesion of a rater, one to
 * one, how well the matched pairs overlap and how many lesions stay unmatched: the integers behind panoptic quality (PQ),
 * segmentation quality (SQ) and recognition quality (RQ) of every sample against every rater.
 * Input: the workspace of a ccdm_lesions call with the same (B,S,L,H,W,K) on the same stream, i.e. its label planes int32
 * [B*S + B*L][C][H][W] and the lesion counts behind them; nothing of the maps is read.  The scored classes are those of
 * ccdm_lesions (1..K-1, or class 0 when K == 1: C of them); the lesions are those of the connectivity that call was given.
 * T thresholds, each a rational num/den (HOST array [T][2], read during the call), and min_size.
 * Cell (per image b, sample i, rater j, class c):
 *   Kept lesions: a lesion of fewer than min_size pixels is dropped from its side; n_a, n_r = the kept lesions of the sample map
 *   and of the rater map.  min_size = 1 keeps all.
 *   Pair: for a kept sample lesion a and a kept rater lesion r, inter(a,r) = the pixels labelled a in the sample plane and r in
 *   the rater plane, union = size(a) + size(r) - inter.  The pair is MATCHED at num/den iff inter*den > num*union in 64-bit
 *   integers: strictly above the threshold, at every threshold.
 *   Thresholds lie in [1/2, 1): den <= 2*num, num < den, 1 <= den <= 65536.  With IoU > 1/2 a lesion has at most one partner
 *   (Kirillov et al., Panoptic Segmentation: two partners would each cover more than half of it), so the matching is unique
 *   and no assignment problem is solved.
 *   stats    int32 [B][S][L][C][2+T] = {n_a, n_r, tp[0..T)}: tp[t] = the matched pairs at threshold t (false positives n_a - tp,
 *            false negatives n_r - tp).  Every element is written, zeros included: OVERWRITTEN per call.
 *   iou_sum  int64 [B][S][L][C][T]: the sum over the matched pairs at t of floor(inter * 2^32 / union), the IoU of a pair as a
 *            fixed-point integer: every sum is exact in any order (at most 8192 pairs: below 2^46).  OVERWRITTEN per call, every
 *            element written.  8-byte aligned.
 * Workspace (device, 4-byte aligned, ccdm_lesion_match_workspace_bytes(B,S,L,H,W,K) = ccdm_lesions_workspace_bytes(...) +
 * 4*B*(S+L)*C*(ceil(H*W/2) + 1) bytes): what ccdm_lesions wrote, left as it is, then this call's lesion sizes int32
 * [B*S + B*L][C][ceil(H*W/2)] and kept-lesion counts int32 [B*S + B*L][C].  Pass the same buffer, of this size, to both calls.  A
 * label outside 1..count (a workspace ccdm_lesions did not write) is read as no lesion.
 * Limits, checked before anything is launched or read, each refusal naming the argument: those of ccdm_lesions on K, S, L, H, W
 * (H*W <= 16384) and B; 1 <= T <= 8; the threshold rule above; min_size >= 1.  Two kernels on `stream`: the lesion sizes once per
 * (map, class); then one workgroup per cell counts the pixels of every (a, r) pair in an LDS hash table (a cell has at most
 * ceil(H*W/2) distinct pairs: the table is never more than half full) and tests every pair found.  Integers only: two identical
 * calls are bit-identical.  B = 0 returns 0 without a launch and leaves the outputs as they are.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_lesion_match_workspace_bytes(int B, int S, int L, int H, int W, int K);
int ccdm_lesion_match(int B, int S, int L, int H, int W, int K, const int32_t* thresholds /*HOST [T][2]: num, den*/, int T, int min_size,
                      int32_t* stats /*dev [B][S][L][C][2+T]*/, int64_t* iou_sum /*dev [B][S][L][C][T]*/, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LIDC lesion findings of the sample set, device part (beyond the reference): which lesions the S samples of an image propose
 * together and how sure the set is of each, and which lesions the raters agree on: the integers behind FROC, the sensitivity at
 * fixed false positives per image and the average precision of the model as a lesion detector.
 * Inputs: samples uint8 [B,S,H,W]; raters uint8 [B,L,H,W], or NULL with L = 0; device class maps as they lie in memory; K classes;
 * connectivity 4 or 8 (as in ccdm_lesions); integers n_min in 1..S and m_min in 1..L (m_min is ignored when L = 0); cap >= 1.  The
 * scored classes are those of ccdm_lesions: 1..K-1, or class 0 when K == 1: C of them.  A byte >= K belongs to no class.
 * Per image b and scored class c: n(p) = the samples with class c at pixel p, m(p) = the raters with class c at p.  Candidate mask
 * A = {p : n(p) >= n_min}, reference mask R = {p : m(p) >= m_min} (empty when L = 0).  CANDIDATES are the connected components of A,
 * REFERENCE LESIONS those of R, both numbered 1.. in raster order of their first pixel (scipy.ndimage.label's order under the
 * connectivity).
 *   counts  int32 [B][C][2] = {n_cand, n_ref}: always the true counts.
 *   cand    int32 [B][C][cap][12], record i-1 for candidate i = {size, support, peak, mass, ref_cov, rater_hits, ymin, xmin, ymax,
 *           xmax, sum_y, sum_x}: size its pixels; support the samples that have at least one class-c pixel inside it; peak the
 *           maximum and mass the sum of n(p) over its pixels; ref_cov its pixels that lie in R; rater_hits the raters that have a
 *           class-c pixel inside it; then its bounding box (inclusive) and the sums of its pixels' coordinates (the centroid is
 *           sum / size).  support >= peak >= n_min.
 *   ref     int32 [B][C][cap][4], record i-1 for reference lesion i = {size, cov, best_support, best_peak}: cov its pixels that lie
 *           in A; best_support and best_peak the maximum of support and of peak over the candidates that share at least one pixel
 *           with it, 0 if none does.
 *           Rows at or beyond the count are zeros; every element of counts, cand and ref is written: OVERWRITTEN per call.  When a
 *           count exceeds cap, the records of that (image, class) on that side and the values derived from them (best_*, conf_map)
 *           are not defined; nothing outside the arrays is touched.
 *   conf_map  optional (may be NULL) uint8 [B][C][H][W]: the support of the candidate that holds the pixel, 0 outside A.
 * Workspace (device, 4-byte aligned, ccdm_findings_workspace_bytes(B,S,L,H,W,K,cap) = B*C*(11*H*W + G*cap) bytes with
 * G = ceil(S/8) + ceil(L/8)): the label planes int32 [B][C][2][H][W] (candidates, then reference lesions; 0 outside the mask), then
 * n uint8 [B][C][H][W], then the two masks uint8 [B][C][2][H][W] (all valid after the call), then per candidate one byte per group of
 * 8 samples and of 8 raters uint8 [B][C][G][cap]: bit s of group g says that map 8g + s has the class inside the candidate.
 * Limits, checked before anything is launched or read, each refusal naming the argument: 1 <= K <= 32, 1 <= S <= 255,
 * 0 <= L <= 255, H, W >= 1 and H*W <= 16384, connectivity in {4, 8}, 1 <= n_min <= S, 1 <= m_min <= L unless L = 0,
 * 1 <= cap <= 1024 (a candidate and a reference record take 16 words of LDS together: 1024 of them are the 64 KB that leave room
 * for two workgroups per CU), raters NULL exactly when L = 0, B >= 0.  Any alignment of the stacks is accepted: one dword per lane
 * when W % 4 == 0 and both pointers are 4-byte aligned, bytes otherwise.  Four kernels on `stream`: counting (n and the masks); the
 * union-find labelling of ccdm_lesions on the two masks, one workgroup per (image, class, mask); the samples and raters inside every
 * candidate as bitsets, one workgroup per (image, class, group of 8 maps), LDS atomicOr; then one workgroup per (image, class) builds
 * the records in LDS with integer atomics.
 * Integers only, exact in any order: two identical calls are bit-identical.  B = 0 returns 0 without a launch and leaves the
 * outputs as they are.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_findings_workspace_bytes(int B, int S, int L, int H, int W, int K, int cap);
int ccdm_findings(const uint8_t* samples /*dev [B,S,H,W]*/, const uint8_t* raters /*dev [B,L,H,W] or NULL*/, int B, int S, int L, int H,
                  int W, int K, int connectivity, int n_min, int m_min, int cap, int32_t* counts /*dev [B][C][2]*/,
                  int32_t* cand /*dev [B][C][cap][12]*/, int32_t* ref /*dev [B][C][cap][4]*/, uint8_t* conf_map /*dev [B][C][H][W] or NULL*/,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Segmentation evaluation, device part (Cityscapes mIoU): the reference Evaluator's `infer_step` / `update_cm`
 * (evaluation/eval_cdm.py) in one pass, without a full-resolution probability tensor.  Per output pixel of [B,H,W]:
 *   - bilinear sample of the prediction [B,h,w] as ATen's upsample_bilinear2d (align_corners=False, no antialias) in fp32:
 *     src = max((in/out) * (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1,
 *     v = lh0 * (lw0 * x00 + lw1 * x01) + lh1 * (lw0 * x10 + lw1 * x11); (H,W) == (h,w) reads the pixel itself;
 *   - argmax over the first C = K-1 channels (the ignore channel K-1 is dropped), ties to the lowest index;
 *   - pixels whose label is >= C are not counted (ignite's ConfusionMatrix target mask);
 *   - hard[t][pred] += 1 (int64 [C,C], rows = target, ACCUMULATED across calls);
 *   - soft[c][t] = sum of v_c over the counted pixels of target t (fp64 [C,C], rows = prediction, OVERWRITTEN per call).
 * Prediction: probs (fp32 channels-last, pixel (b,y,x) channel c at probs[((b*h + y)*w + x)*pixel_stride + c],
 * pixel_stride >= K) XOR cls (uint8 class map [B,h,w], read as its one-hot: bit-identical to probs holding that one-hot).
 * labels: uint8 train ids [B,H,W].  K in [2,32].  The workspace (device, ccdm_seg_confusion_workspace_bytes(B,H,W,K) bytes)
 * holds per-block partial sums; no float atomics: two identical calls return bit-identical matrices.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_seg_confusion_workspace_bytes(int B, int H, int W, int K);
int ccdm_seg_confusion(const float* probs /*dev or NULL*/, int64_t pixel_stride, const uint8_t* cls /*dev [B,h,w] or NULL*/,
                       const uint8_t* labels /*dev [B,H,W]*/, int B, int h, int w, int H, int W, int K,
                       int64_t* hard /*dev [K-1,K-1]*/, double* soft /*dev [K-1,K-1]*/, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Segmentation prediction export, device part (the images of the reference Evaluator's `save_preds`): the class of every
 * output pixel of [B,H,W], written as a train id, a label id and a colour, without a full-resolution probability tensor.
 * The prediction (probs XOR cls), the bilinear sample and the argmax are those of ccdm_seg_confusion above, through the same
 * device code: the class written here is the class counted there, bit for bit.
 *   scored    the leading channels the argmax runs over: K-1 for a prediction (the ignore channel is dropped; a pixel with all
 *             its mass there becomes class 0), K for labels passed as a class map (train id K-1 reaches table entry K-1);
 *   id_table  uint8 [K], color_table uint8 [K][3], in device memory;
 *   outputs   each optional (NULL = not written), at least one: train_id uint8 [B,H,W] = the argmax class,
 *             label_id uint8 [B,H,W] = id_table[train_id], color uint8 [B,H,W,3] = color_table[train_id].
 * K in [2,32].  No workspace, nothing is reduced; B = 0 returns 0 without a launch.  (Named without the ccdm_seg_ prefix: the
 * evaluator's test pins the set of ccdm_seg_* symbols.)
 * ------------------------------------------------------------------------------------------------- */
int ccdm_segexport(const float* probs /*dev or NULL*/, int64_t pixel_stride, const uint8_t* cls /*dev [B,h,w] or NULL*/,
                   int B, int h, int w, int H, int W, int K, int scored, const uint8_t* id_table /*dev [K]*/,
                   const uint8_t* color_table /*dev [K][3]*/, uint8_t* train_id /*dev [B,H,W] or NULL*/,
                   uint8_t* label_id /*dev [B,H,W] or NULL*/, uint8_t* color /*dev [B,H,W,3] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Cityscapes script scores, device part: the integer counts behind the result file of the official pixel-level evaluation
 * script (the reference's evaluation/cs_eval.py, `evaluatePair`), in one pass over the output pixels of [B,H,W], without a
 * full-resolution probability tensor and without an id image.
 * ccdm_csscore: the prediction (probs XOR cls), the bilinear sample and the argmax over the first K-1 channels are those of
 * ccdm_seg_confusion and ccdm_segexport above, through the same device code; the predicted id of a pixel is id_table[class],
 * the byte ccdm_segexport writes as label_id, bit for bit.  ccdm_csscore_ids: the predicted ids are read from pred_ids
 * uint8 [B,H,W] instead (what the script reads from the PNGs).  Everything below is in device memory.
 *   id_table        uint8 [K];  gt_ids uint8 [B,H,W]: ground truth in label ids;
 *   inst_ids        uint16 [B,H,W] or NULL: the values of *_gtFine_instanceIds.png (label id * 1000 + running number for an
 *                   instance, the plain label id otherwise);
 *   ignore_in_eval, category, has_instances   uint8 [L], per label id; L <= CCDM_CSSCORE_MAX_LABELS (34 for Cityscapes);
 *   conf            int64 [L][L], rows = ground-truth id, columns = predicted id, ACCUMULATED across calls.  Every pixel is
 *                   counted, ignored ground truth included (the script's check: conf.sum() == pixels);
 *   per_image       int64 [B][4], OVERWRITTEN per call: {pixels whose ground truth is ignored in evaluation; of those, pixels
 *                   where prediction != ground truth; pixels whose ground truth is evaluated; of those, pixels where
 *                   prediction == ground truth}.  (The first two are what the script stores as nbNotIgnoredPixels and
 *                   nbCorrectPixels: its np.in1d(..., invert=True) inverts the mask.)
 *   instances       int32 [B][NI][3], only with inst_ids, OVERWRITTEN per call.  Slot layout: instance id i lives in slot
 *                   i - inst_base of its image, for inst_base <= i < inst_base + NI (Cityscapes: inst_base 24000, NI 10000:
 *                   the ids of the labels 24..33 that have instances).  Per slot {size of the instance; pixels whose predicted
 *                   id is the instance's label i / 1000; pixels whose predicted id is a label of that label's category}.  An
 *                   instance whose label is ignored in evaluation keeps a zero slot (the script's `continue`);
 *   unknown         int32 [2], OVERWRITTEN per call: {pixels whose ground-truth or predicted id is >= L (not counted in conf;
 *                   the script's "Unknown label with id"); pixels of an instance id > 1000 that has no slot or whose label has
 *                   no instances (the script's KeyError)}.  A caller treats a non-zero entry as an error.
 * Integer atomics only, after an on-chip reduction (an LDS copy of conf per block; per-wave groups of equal instance keys):
 * every count is exact in any order, two identical calls are bit-identical.  K in [2,32].  gt_ids, pred_ids (4 bytes) and
 * inst_ids (8 bytes) must be aligned when W % 4 == 0 (vector loads).  No workspace; B = 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------------- */
#define CCDM_CSSCORE_MAX_LABELS 64
int ccdm_csscore(const float* probs /*dev or NULL*/, int64_t pixel_stride, const uint8_t* cls /*dev [B,h,w] or NULL*/,
                 int B, int h, int w, int H, int W, int K, const uint8_t* id_table, const uint8_t* gt_ids, const uint16_t* inst_ids,
                 int L, const uint8_t* ignore_in_eval, const uint8_t* category, const uint8_t* has_instances, int inst_base, int NI,
                 int64_t* conf, int64_t* per_image, int32_t* instances, int32_t* unknown, void* stream);
int ccdm_csscore_ids(const uint8_t* pred_ids, int B, int H, int W, const uint8_t* gt_ids, const uint16_t* inst_ids,
                     int L, const uint8_t* ignore_in_eval, const uint8_t* category, const uint8_t* has_instances, int inst_base, int NI,
                     int64_t* conf, int64_t* per_image, int32_t* instances, int32_t* unknown, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Calibration scores of a segmentation prediction, device part (beyond the reference, which scores hard classes only): the
 * counts behind ECE / MCE, NLL, the Brier score and the reliability diagram, in one pass over the output pixels of [B,H,W],
 * without a full-resolution probability tensor.  The prediction (probs XOR cls), the labels, the counted pixels (label < C,
 * C = K-1), the bilinear sample v_c and the argmax `pred` are those of ccdm_seg_confusion above, through the same device code:
 * the class binned here is the class counted there, bit for bit.  Per counted pixel with label t:
 *   s = v_0 + v_1 + ... + v_{C-1}, ascending in fp32;  q_c = v_c / s (IEEE division);  s == 0 (all mass on the ignore channel):
 *   q_c = 1/C for every c (pred is 0 there);
 *   conf = q_pred;  correct = (pred == t);  bin = min((int)(conf * M), M-1) in fp32;
 *   nll = -log(max((double)q_t, 1e-12));  brier = sum over c of (q_c - [c == t])^2, ascending in fp32.
 * Outputs (device):
 *   bins      int64 [C][M][2], by (pred, bin): {pixels, correct pixels}.  ACCUMULATED across calls;
 *   conf_sum  fp64 [C][M], by (pred, bin): sum of conf.  OVERWRITTEN per call;
 *   sums      fp64 [3]: {sum of nll, sum of brier, sum of q_t}.  OVERWRITTEN per call.
 * K in [2,32], M in [2,64].  The workspace (device, ccdm_segcalib_workspace_bytes(B,H,W,K,M) bytes) holds exact fixed-point
 * confidence sums (conf is a multiple of 2^-28) and per-block fp64 partial sums; integer atomics only, no float atomics: two
 * identical calls return bit-identical outputs.  B = 0 returns 0 without a launch and leaves all three outputs as they are.
 * (Named without the ccdm_seg_ prefix: the evaluator's test pins the set of ccdm_seg_* symbols.)
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_segcalib_workspace_bytes(int B, int H, int W, int K, int M);
int ccdm_segcalib(const float* probs /*dev or NULL*/, int64_t pixel_stride, const uint8_t* cls /*dev [B,h,w] or NULL*/,
                  const uint8_t* labels /*dev [B,H,W]*/, int B, int h, int w, int H, int W, int K, int M,
                  int64_t* bins /*dev [K-1][M][2]*/, double* conf_sum /*dev [K-1][M]*/, double* sums /*dev [3]*/, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Boundary IoU (Cheng et al., CVPR 2021) and trimap counts of a segmentation prediction, device part (beyond the reference,
 * whose scores are all region scores): a stencil of radius d over two class maps at the scored resolution [B,H,W].
 *   pred    uint8 [B,H,W]: the class of every output pixel, the byte ccdm_segexport writes as train_id with scored = K-1;
 *   labels  uint8 [B,H,W]: train ids; a label >= C = K-1 is not counted (the rule of ccdm_seg_confusion).
 * Wherever the label is not counted the prediction is not counted either, so both maps share one ignore region, which makes a
 * border in both alike; a predicted byte >= C is not counted either.  For a map X, a class c < C and a width d >= 1,
 * band_X(c,d) = the pixels p with X[p] == c for which some pixel within Chebyshev distance d of p lies outside the image or has
 * X != c: the mask of c minus its erosion by a 3x3 square, d iterations, zero border (the published Boundary IoU code).
 *   bcounts  int64 [C][3], per class c: {|band_G(c,d)|, |band_P(c,d)|, |band_G(c,d) & band_P(c,d)|}.  ACCUMULATED across calls;
 *   trimap   int64 [C][C], rows = label, columns = prediction: the hard matrix of ccdm_seg_confusion restricted to the counted
 *            pixels p that lie in band_G(G[p], d).  ACCUMULATED across calls.
 * K in [2,32], d in [1,64].  Two linear passes, whatever d: rows (one byte per pixel and map into the workspace: the class and
 * whether its run covers [x-d, x+d]), then columns (a rolling run length over [y-d, y+d]).  The workspace (device, 2-byte
 * aligned, ccdm_segboundary_workspace_bytes(B,H,W) = 2*B*H*W bytes) holds those bytes.  Integer atomics only, after a per-block
 * count in LDS: every count is exact in any order, two identical calls are bit-identical.  B = 0 returns 0 without a launch.
 * (Named without the ccdm_seg_ prefix: the evaluator's test pins the set of ccdm_seg_* symbols.)
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_segboundary_workspace_bytes(int B, int H, int W);
int ccdm_segboundary(const uint8_t* pred /*dev [B,H,W] train ids*/, const uint8_t* labels /*dev [B,H,W]*/, int B, int H, int W,
                     int K, int d, int64_t* bcounts /*dev [K-1][3]*/, int64_t* trimap /*dev [K-1][K-1]*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Boundary F-score counts of a segmentation prediction (Csurka et al.'s BF score, MATLAB's bfscore, the DAVIS F-measure), device
 * part (beyond the reference): a Euclidean disc search of radius theta around every contour pixel, per class and per image.
 * pred, labels, K and C = K-1 are those of ccdm_segboundary, and so are the two masked maps:
 *   G'  the label where it is counted (< C), "none" elsewhere;
 *   P'  the predicted class where G' is counted and the class is < C, "none" elsewhere.
 * Contour pixel: a pixel of class c in map X (G' or P') is a contour pixel of c when at least one of its 4-neighbours lies inside
 * the image and holds a counted class other than c.  A neighbour that is "none", or that lies outside the image, does not make
 * a contour: the image frame and the rim of the ignored regions are the same in both maps and would match each other for free.
 * Match: with the integer tolerance theta, a contour pixel p of class c in one map is matched when the other map of the same
 * image has a contour pixel q of class c with (px-qx)^2 + (py-qy)^2 <= theta^2.  Integers throughout; no square root is taken.
 *   counts  int64 [B][C][4], per image b and class c: {nP, mP, nG, mG} = the contour pixels of P', those of them matched in G',
 *           the contour pixels of G', those of them matched in P'.  ACCUMULATED across calls: the host clears it.
 * K in [2,32], theta in [1,32], any H, W >= 1.  Two passes: one byte per pixel and map into the workspace (the class, bit 7 =
 * contour pixel), then a block stages a 64 x 64 tile of them with its halo in LDS and a wave ballots "contour pixel of class c"
 * over the rows y + dy and tests the bits within floor(sqrt(theta^2 - dy^2)) of each lane.  The workspace (device, 2-byte aligned,
 * ccdm_contourf_workspace_bytes(B,H,W) = 2*B*H*W bytes, 0 for a non-positive shape) holds those bytes.  Integer atomics only,
 * after a per-block count in LDS: every count is exact in any order, two identical calls are bit-identical.  B = 0 returns 0
 * without a launch.
 * (Named without the ccdm_seg prefixes: the evaluator's tests pin the sets of ccdm_seg_*, ccdm_segcalib* and ccdm_segboundary*
 * symbols.)
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_contourf_workspace_bytes(int B, int H, int W);
int ccdm_contourf(const uint8_t* pred /*dev [B,H,W] train ids*/, const uint8_t* labels /*dev [B,H,W]*/, int B, int H, int W, int K,
                  int theta, int64_t* counts /*dev [B][K-1][4]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Uncertainty-quality counts of a multi-sample prediction, device part (beyond the reference, which never scores its samples'
 * spread): the histograms behind the error-detection AUROC / AUPR, the sparsification curve and PAvPU (Mukhoti & Gal 2018), in
 * one pass over the output pixels of [B,H,W], without a full-resolution tensor.  The prediction (probs XOR cls), the labels, the
 * counted pixels (label < C, C = K-1), the bilinear sample and the argmax `pred` are those of ccdm_seg_confusion above, through
 * the same device code: the class judged here is the class counted there and the byte ccdm_segexport writes as train_id with
 * scored = K-1, bit for bit.  wrong = (pred != label).
 *   maps    fp32 [U][B,h,w] (device): U per-pixel uncertainty maps at the prediction's resolution (the entropy / mutual_info
 *           maps of ccdm_vote_finalize);  ranges  fp32 [U] (HOST), each > 0: the value of map m that fills the scale.
 * Per counted pixel and map m:
 *   u       the bilinear sample of maps[m] at the output pixel by the formula of ccdm_seg_confusion with the same i0, i1, l0, l1
 *           as the probabilities: u = lh0 * (lw0 * u00 + lw1 * u01) + lh1 * (lw0 * u10 + lw1 * u11) in fp32; (H,W) == (h,w)
 *           reads the pixel itself;
 *   t       u / ranges[m] (IEEE fp32 division); a t that is not > 0 (NaN included) becomes 0, t >= 1 becomes 1;
 *   q       (int)(t * 65536.0f), so 0 <= q <= 65536.  Everything after this line is integer arithmetic.
 * Outputs (device):
 *   pix     int64 [U][M][2]: pix[m][bin] += {1, wrong} with bin = min((q*M) >> 16, M-1).  ACCUMULATED across calls;
 *   patch   int64 [U][M][2]: the image is cut into aligned, non-overlapping P x P patches from pixel (0,0), truncated at the right
 *           and bottom edges.  For a patch with n >= 1 counted pixels, Q = the sum of their q, e = the number of wrong ones; the
 *           patch is inaccurate iff 2*e >= n; patch[m][bin] += {1, inaccurate} with bin = min((Q*M) / (n*65536), M-1) in 64-bit
 *           integer division.  Patches with n = 0 are not counted.  ACCUMULATED across calls.
 * K in [2,32], U in [1,4], M in [2,512], P in {2,4,8,16}: each limit is checked before anything is launched and each refusal
 * names the argument; a refused call writes nothing.  ccdm_uncscore_workspace_bytes is 0 (the per-block tables live on chip);
 * workspace may be NULL.  Integer atomics only, after a per-block count in LDS: every count is exact in any order, two identical
 * calls are bit-identical.  B = 0 returns 0 without a launch and leaves the outputs as they are.
 * (Named without the ccdm_seg prefixes: the evaluator's tests pin the sets of ccdm_seg_*, ccdm_segcalib* and ccdm_segboundary*
 * symbols.)
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_uncscore_workspace_bytes(int B, int H, int W, int K, int U, int M);
int ccdm_uncscore(const float* probs /*dev or NULL*/, int64_t pixel_stride, const uint8_t* cls /*dev [B,h,w] or NULL*/,
                  const uint8_t* labels /*dev [B,H,W]*/, const float* maps /*dev [U][B,h,w]*/, const float* ranges /*HOST [U], > 0*/,
                  int B, int h, int w, int H, int W, int K, int U, int M, int P, int64_t* pix /*dev [U][M][2]*/,
                  int64_t* patch /*dev [U][M][2]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Multi-sample prediction (DenoisingModel.predict_multiple): S sampling passes of the same B images folded into one
 * mean map, a per-pixel vote and two uncertainty maps.  The reference's Evaluator.predict_multiple
 * (evaluation/eval_cdm.py:176-193) accumulates `total += prediction_i * (1 / S)` on the host; these read a pass
 * straight from the engine's uint8 class map or its probabilities.  Channels-last [B,HW,K] like out_probs;
 * K in [1, CCDM_MAX_CLASSES].  Entropies are in nats (0 log 0 = 0), formed in fp64, stored fp32.
 *   ccdm_vote_accumulate   : add one pass, in place.  Source: cls (class map, one-hot meaning) XOR probs (fp32);
 *                            src_stride = elements from one image's source to the next (0 = dense: HW resp. HW*K).
 *                            total[b,p,k] += src[b,p,k] * w as one rounded fp32 multiply and one rounded fp32 add
 *                            (w = fp32 1/S: bit-identical to torch-CPU's `total += pred * (1 / S)`);
 *                            counts[b,p,k] += (cls == k) (class-map source only);
 *                            ent_sum[b,p] += H(probs[b,p,:]) (probability source only; a one-hot pass adds 0).
 *                            Each accumulator may be NULL.
 *   ccdm_vote_finalize     : vote = argmax of counts (if given) else of total, ties to the lowest class index;
 *                            entropy = H(mean) with mean = counts / S or total; mutual_info = max(0, H(mean) - ent_sum / S)
 *                            (ent_sum NULL: 0, one-hot passes); mean (needs counts) = (float)counts / (float)S.
 *                            Each output may be NULL.
 *   ccdm_vote_reduce_stack : the one-shot form over an S-sample stack [B,S,HW] (S samples of an image contiguous):
 *                            counts, mean = counts / S, vote, entropy in one read of the stack (each output may be NULL).
 * Bytes (fp32 total, per pass): accumulate reads HW*B bytes (class map) or 4*B*HW*K (probabilities) and reads and
 * writes each accumulator once; finalize reads the accumulators once and writes the maps once.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_vote_accumulate(const uint8_t* cls /*dev [B,HW] or NULL*/, const float* probs /*dev [B,HW,K] or NULL*/, int64_t src_stride,
                         int B, int HW, int K, float w, float* total /*dev [B,HW,K] or NULL*/,
                         int32_t* counts /*dev [B,HW,K] or NULL*/, float* ent_sum /*dev [B,HW] or NULL*/, void* stream);
int ccdm_vote_finalize(const float* total /*dev [B,HW,K] or NULL*/, const int32_t* counts /*dev [B,HW,K] or NULL*/,
                       const float* ent_sum /*dev [B,HW] or NULL*/, int B, int HW, int K, int S,
                       float* mean /*dev [B,HW,K] or NULL*/, uint8_t* vote /*dev [B,HW] or NULL*/,
                       float* entropy /*dev [B,HW] or NULL*/, float* mutual_info /*dev [B,HW] or NULL*/, void* stream);
int ccdm_vote_reduce_stack(const uint8_t* stack /*dev [B,S,HW]*/, int B, int S, int HW, int K,
                           int32_t* counts /*dev [B,HW,K] or NULL*/, float* mean /*dev [B,HW,K] or NULL*/,
                           uint8_t* vote /*dev [B,HW] or NULL*/, float* entropy /*dev [B,HW] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Mode summary of a multi-sample prediction (metrics.sample_modes, DenoisingModel.predict_modes; beyond the reference, which
 * only looks at grids of samples): which distinct segmentations the S samples of an image propose, and how likely each is.
 * k-medoids (PAM) over the samples under the reference's own distance, 1 - mean foreground IoU, in exact integers.
 * Input: class maps a[b][i][p], uint8 [B,S,HW], classes in [0,K); a byte >= K belongs to no class.
 * Limits: 2 <= K <= 32, 1 <= S <= 256, 1 <= M <= 16, 0 < HW < 2^31, B <= 65535; checked before anything is launched or read.
 *
 * Fixed-point distance.  For samples i, j of one image and every foreground class k = 1..K-1:
 *   n_i[k] = #{p : a_i[p] == k},  I_k = #{p : a_i[p] == a_j[p] == k},  U_k = n_i[k] + n_j[k] - I_k,
 *   q_k = 0 if U_k == 0, else (2*(U_k - I_k)*2^20 + U_k) / (2*U_k) rounded down: the Jaccard distance in units of 2^-20, round
 *   half up, in int64;  Q[i][j] = sum_k q_k, an int32 (at most 31 * 2^20).  Q is symmetric with a zero diagonal.
 * Q / ((K-1) * 2^20) is within 2^-21 of the reference's `batched_distance`.  No floating point enters the clustering, so
 * nothing depends on a reduction order: two calls are bit-identical.
 *
 * Clustering: per image PAM on Q, every sum in int64.
 *   BUILD  m_1 = argmin_i sum_j Q[i][j], lowest i on ties; near_j = Q[m_1][j].  For c = 2..M: gain(i) = sum_j max(0, near_j -
 *          Q[i][j]) over the non-medoids i, the argmax with the lowest i on ties; a best gain of 0 ends BUILD (every sample
 *          coincides with a medoid: fewer than M modes exist); otherwise i becomes the medoid of slot c and near is updated.
 *   SWAP   best improvement.  cost = sum_j near_j.  For every (slot c in BUILD order, non-medoid h): cost'(c,h) = the cost with
 *          slot c's medoid replaced by h; the lowest cost', ties to the lowest c and then the lowest h.  cost' < cost: apply it
 *          and repeat; otherwise stop with converged = 1.  At most max_swaps swaps are applied; converged = 0 iff an improving
 *          swap was left unapplied.
 *   Assignment: every sample to the medoid with the lowest Q, lowest slot on ties.
 *   Ordering: modes by size descending, ties by the lower medoid sample index; slots never filled come last with medoid -1,
 *          size 0, spread 0.
 *
 *   ccdm_modes_distance : Q int32 [B][S][S].  `ws` is a workspace, int32 [B][S][S][K], cleared on `stream` by the call (it
 *                         receives I_k of the pairs i <= j; I_k of a map with itself is n_i[k]).  One workgroup per (image,
 *                         16 x 16 tile of pairs i <= j, share of the pixels) stages each 1024-pixel chunk of the tile's 32 maps
 *                         once in LDS, counts I_k for its 256 pairs from there and adds them to `ws` with integer atomics
 *                         (exact in any order); a second launch forms Q from `ws` and writes it with its mirror.  Class counts
 *                         in registers, by K <= 2, <= 8, <= 32.  Dword loads when HW % 4 == 0 and `a` is 4-byte aligned, bytes
 *                         otherwise.
 *   ccdm_modes_pam      : one workgroup per image; Q in LDS for S <= 128 (64 KB), read from global memory above.  Outputs, all
 *                         OVERWRITTEN: medoid int32 [B][M] (sample index, -1 unused), assign int32 [B][S] (the mode of every
 *                         sample, in the output order), size int32 [B][M], spread int64 [B][M] (sum over the members of
 *                         Q[medoid][.]), cost int64 [B] (sum of the spreads), swaps int32 [B], converged int32 [B].  max_swaps >= 0.
 *   ccdm_modes_maps     : per (image, mode, pixel) the class counts over the mode's members (`assign`, `size` as ccdm_modes_pam
 *                         leaves them).  vote uint8 [B][M][HW]: the majority class within the mode, lowest class on ties, 255
 *                         for an unused mode.  counts int32 [B][M][HW][K] or NULL.  entropy fp32 [B][M][HW] or NULL: the entropy
 *                         in nats of counts / size, formed in fp64 (0 log 0 = 0); 0 for an unused mode.
 * B = 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_modes_distance(const uint8_t* a /*dev [B,S,HW]*/, int B, int S, int HW, int K, int32_t* ws /*dev [B,S,S,K] workspace*/,
                        int32_t* Q /*dev [B,S,S]*/, void* stream);
int ccdm_modes_pam(const int32_t* Q /*dev [B,S,S]*/, int B, int S, int M, int max_swaps, int32_t* medoid /*dev [B,M]*/,
                   int32_t* assign /*dev [B,S]*/, int32_t* size /*dev [B,M]*/, int64_t* spread /*dev [B,M]*/, int64_t* cost /*dev [B]*/,
                   int32_t* swaps /*dev [B]*/, int32_t* converged /*dev [B]*/, void* stream);
int ccdm_modes_maps(const uint8_t* a /*dev [B,S,HW]*/, const int32_t* assign /*dev [B,S]*/, const int32_t* size /*dev [B,M]*/, int B, int S,
                    int M, int HW, int K, uint8_t* vote /*dev [B,M,HW]*/, int32_t* counts /*dev [B,M,HW,K] or NULL*/,
                    float* entropy /*dev [B,M,HW] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Metric-optimal consensus of a multi-sample prediction (metrics.sample_consensus, DenoisingModel.predict_consensus; beyond the
 * reference): which single map to report.  The majority vote is the Bayes prediction for per-pixel accuracy; under IoU and Dice the
 * best threshold on the sample frequency is in general not 1/2, and with many empty samples it can be the empty map.  The samples
 * stand in for the posterior: the expected score of a candidate map is its mean score against them, and the candidates are the
 * S + 1 nested thresholded frequency maps (the majority vote among them).  In exact integers.
 * Input: class maps a[b][s][p], uint8 [B,S,HW], classes in [0,K); a byte >= K belongs to no class.  The scored classes are
 * k = 1..K-1: C = K-1 of them.
 * Limits, checked before anything is launched or read, each refusal naming the argument: 2 <= K <= 32, 1 <= S <= 255,
 * 0 < HW < 2^31, 0 <= B <= 65535, non-null pointers (of ccdm_consensus_maps' mask and label one may be NULL), curve 8-byte and
 * best and workspace 4-byte aligned, workspace_bytes >= ccdm_consensus_workspace_bytes(B,S,HW,K) = B*C*S*(S+1)*4, metric in {0, 1}.
 * B = 0 returns 0 without a launch and leaves the outputs as they are.
 *
 * Per image b and scored class k:
 *   n[p] = #{s : a_s[p] == k}, in 0..S: the frequency plane.
 *   Candidate masks P_j = {p : n[p] >= j}, j = 1..S+1: nested, P_{S+1} the empty map.
 *   A_j = |P_j|,  n_s = #{p : a_s[p] == k},  I_{j,s} = #{p : a_s[p] == k and n[p] >= j}.
 *   IoU term of (j, s):  U = A_j + n_s - I_{j,s};  2^20 if U == 0 (the reference's 0/0 = 1), else (2*I*2^20 + U) / (2*U) rounded down in
 *   int64: the quotient I / U in units of 2^-20, round half up.
 *   Dice term of (j, s): the same with numerator 2*I and denominator D = A_j + n_s: 2^20 if D == 0, else (2*(2*I)*2^20 + D) / (2*D).
 *   curve[b][k-1][m][j-1] = sum_s term, int64, m = 0 (IoU), m = 1 (Dice); the expected score is curve / (S * 2^20).
 *   best[b][k-1][m] = the j with the largest curve value, the LOWEST j on ties: the largest mask among equals.
 * No floating point enters, so nothing depends on a reduction order: two calls are bit-identical.
 *
 *   ccdm_consensus      : outputs, all OVERWRITTEN: freq uint8 [B][C][HW] (the planes n), curve int64 [B][C][2][S+1], best int32 [B][C][2].
 *                         The workspace receives h[b][k-1][s][m] = #{p : a_s[p] == k and n[p] == m}, int32 [B][C][S][S+1], cleared on
 *                         `stream` by the call.  Three launches on `stream`, no host round trip.  Counting: the stack is streamed once,
 *                         one dword per lane when HW % 4 == 0 and the pointer is 4-byte aligned, bytes otherwise; class counts in
 *                         registers as byte counters, by K <= 2, <= 8, <= 32.  Histogram: one workgroup per (image, class, group of 16
 *                         samples, share of the pixels) counts into an LDS table [16][S+1] (at most 16 KB) with LDS integer atomics and
 *                         adds it to h with global integer atomics (exact in any order); pixels with n[p] == 0 are skipped before a
 *                         sample is read.  Selection: one workgroup per (image, class); I_{j,s} = sum_{m >= j} h[s][m] as suffix sums
 *                         of the rows of h, in place; A_j from the column sums of h (the pixels with n == m are counted by m samples:
 *                         sum_s h[s][m] / m, exact); the terms of threshold j summed by the threads the block has for it (integers: any
 *                         order), every quotient an fp64 division set right by its int64 remainder (exact for these ranges); a
 *                         block argmax with the tie rule.
 *   ccdm_consensus_maps : from `freq` and `best` as ccdm_consensus leaves them (read on the device), for one metric m:
 *                         mask uint8 [B][C][HW] or NULL: n[p] >= best[b][k-1][m], written as 0 / 1;
 *                         label uint8 [B][HW] or NULL: among the scored classes whose mask holds p the one with the largest n[p], the
 *                         lowest class on ties; class 0 if no mask holds p.  For K = 2 label equals mask.  One streaming launch.
 * ------------------------------------------------------------------------------------------------- */
size_t ccdm_consensus_workspace_bytes(int B, int S, int HW, int K);
int ccdm_consensus(const uint8_t* samples /*dev [B,S,HW]*/, int B, int S, int HW, int K, uint8_t* freq /*dev [B,C,HW]*/,
                   int64_t* curve /*dev [B,C,2,S+1]*/, int32_t* best /*dev [B,C,2]*/, void* workspace, uint64_t workspace_bytes, void* stream);
int ccdm_consensus_maps(const uint8_t* freq /*dev [B,C,HW]*/, const int32_t* best /*dev [B,C,2]*/, int B, int S, int HW, int K, int metric,
                        uint8_t* mask /*dev [B,C,HW] or NULL*/, uint8_t* label /*dev [B,HW] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Training-time forward pieces of the categorical diffusion, BCHW fp32 like the reference's
 * tensors, per-sample coefficients (the host resolves t -> alpha_t / cumalpha_{t-1} incl. the t == 1 override).
 *   ccdm_mix_uniform : out = s[n]*x + (1-s[n])/K.   With s = 1-beta_t it is the probability table of
 *                      DiffusionModel.q_xt_given_xtm1 (diffusion_denoising.py:72-78), with s = cumalpha_t of
 *                      q_xt_given_x0 (:80-86).
 *   ccdm_theta_post  : prob_mode 0: DiffusionModel.theta_post (:88-97)  q(x_{t-1} | x_t, x_0), both inputs any float
 *                      tensors (one-hot in the reference's use); prob_mode 1: theta_post_prob (:99-129), the second
 *                      input a distribution over x_0 — O(K) closed form of the reference's [B,K,K,H,W] product.
 *   ccdm_kl_clamped  : p*(log p - log max(q, floor)), 0 where p == 0: the diffusion term of Trainer.train_step
 *                      (trainer.py:266-270, kl_div(log(clamp(q, 1e-12)), p, reduction='none')).
 * K in [2, 32].  a, c, s: dev [N] fp32.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_mix_uniform(const float* x /*dev [N,K,HW]*/, const float* s, int N, int K, int HW, float* out, void* stream);
int ccdm_theta_post(const float* xt /*dev [N,K,HW]*/, const float* x0 /*dev [N,K,HW]*/, const float* a, const float* c,
                    int N, int K, int HW, int prob_mode, float* out /*dev [N,K,HW]*/, void* stream);
int ccdm_kl_clamped(const float* p, const float* q, size_t n, float floor, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * DINO ViT-S/8 key-feature extractor (reference call sites ddpm/models/dino.py:211-229,279-305 and
 * condition_encoder.py:26-46; the network itself is facebookresearch/dino's VisionTransformer, fetched by the reference
 * with torch.hub (dino.py:58-82) and therefore not part of /root/reference: restated from its published form).
 * The linear layers run on ccdm_conv2d as 1x1 convs over a [N, T_alloc/16, 16, C] token image; these cover the rest:
 *   ccdm_attention_ex : ccdm_attention with T_alloc >= T token rows allocated per sample (only the first T are tokens)
 *   ccdm_layernorm    : nn.LayerNorm(C, eps) over the last axis of [rows, C]
 *   ccdm_gelu         : nn.GELU(), exact erf form
 *   ccdm_vit_key_resize : the keys of token rows 1 .. h0*w0 of a [N, T_alloc, 3*dim] qkv buffer (the middle third) as
 *                       [N, dim, Ht, Wt] descriptors, channel d_index * heads + head, bilinearly resized from the h0 x w0
 *                       token grid (F.interpolate 'bilinear', align_corners=False; dino.py:297-305).  Padding rows are not read.
 * ------------------------------------------------------------------------------------------------- */
int ccdm_attention_ex(const float* qkv /*dev [N,T_alloc,3C]*/, float* out /*dev [N,T_alloc,C]*/, int N, int T, int T_alloc, int C,
                      int heads, int order, void* stream);
int ccdm_layernorm(const float* x, const float* gamma, const float* beta, float eps, long rows, int C, float* out, void* stream);
int ccdm_gelu(const float* x, size_t n, float* out, void* stream);
int ccdm_vit_key_resize(const float* qkv /*dev [N,T_alloc,3*dim]*/, int N, int T_alloc, int h0, int w0, int dim, int heads, int Ht, int Wt,
                        float* out /*dev [N,dim,Ht,Wt]*/, void* stream);

/* boundary re-layout helpers */
int ccdm_nchw_to_nhwc(const float* src, float* dst, int N, int C, int HW, int dst_stride, int dst_off, void* stream);
int ccdm_onehot_to_xin(const uint8_t* idx, float* xin, int N, int HW, int K, int xin_stride, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Step executor.  The host describes one denoise step as a list of ops (fully resolved device pointers);
 * ccdm_engine_run replays it n_steps times with a device-resident step counter, optionally through a
 * HIP graph captured on first use.  One engine per (model, N, H, W); single-threaded like the
 * reference's DenoisingModel.forward_denoising loop (diffusion_denoising.py:189-212).
 * ------------------------------------------------------------------------------------------------- */
typedef struct ccdm_engine ccdm_engine;

ccdm_engine* ccdm_engine_create(int32_t* step_counter /*dev scalar*/);
void ccdm_engine_destroy(ccdm_engine* e);
int ccdm_engine_add_conv(ccdm_engine* e, const ccdm_conv_args* a);          /* step_ptr is overridden with the engine's counter */
int ccdm_engine_add_attention(ccdm_engine* e, const float* qkv, float* out, int N, int T, int C, int heads, int order);
int ccdm_engine_add_norm_qkv_attention(ccdm_engine* e, const ccdm_attn_block_args* a);
int ccdm_engine_add_stats_fold(ccdm_engine* e, const double* in, int N, int S_in, int C, int S_out, double* out);
int ccdm_engine_add_resample(ccdm_engine* e, const ccdm_resample_args* a);
int ccdm_engine_add_stem(ccdm_engine* e, const ccdm_stem_args* a);
/* the LAST op of the step: head conv + the epilogue set by ccdm_engine_set_epilogue in one launch (no separate epilogue launch then;
 * ccdm_engine_run needs with_epilogue = 1) */
int ccdm_engine_add_head_posterior(ccdm_engine* e, const ccdm_head_args* a);
int ccdm_engine_set_epilogue(ccdm_engine* e, const ccdm_post_args* a);      /* run after the ops of each step */
int ccdm_engine_num_ops(const ccdm_engine* e);
int ccdm_engine_num_captures(const ccdm_engine* e);   /* how often ccdm_engine_run has captured + instantiated the step's HIP graph so far */
/* per-run mutable fields of the epilogue (everything else is fixed at build time).  With a run block (ccdm_engine_set_run_block:
 * caller-owned device memory of at least sizeof(ccdm_post_run) bytes, set once before the first run) the values travel to the
 * device by a one-thread launch at the head of the next ccdm_engine_run, on its stream, and the captured graph of the step stays
 * valid; without one they are kernel arguments and a change re-captures the graph. */
int ccdm_engine_set_run_block(ccdm_engine* e, void* dev_block);
int ccdm_engine_set_run(ccdm_engine* e, const float* noise, int64_t noise_step_stride, int32_t noise_row0,
                        uint64_t philox_seed, uint32_t sample_offset,
                        float* out_probs, int64_t* out_onehot, float* posterior_out);
/* run `n_steps` denoise steps starting at table row `first_row`; use_graph: 0 eager launches, 1 HIP graph of one step */
int ccdm_engine_run(ccdm_engine* e, int first_row, int n_steps, int with_epilogue, int use_graph, void* stream);
/* timing taps: record HIP events around every launch of op `op_index` during the following runs (at most `capacity` launches
 * per series; a run that starts at table row 0 starts a new series; tapped runs launch eagerly).  Several ops may be tapped;
 * op_index < 0 removes every tap.  ccdm_engine_profile_read returns the number of samples of one tapped op and their
 * mean/min/max in ms. */
int ccdm_engine_profile_op(ccdm_engine* e, int op_index, int capacity);
int ccdm_engine_profile_read(ccdm_engine* e, int op_index, double* mean_ms, double* min_ms, double* max_ms);
/* ccdm_conv_input_absmax of every conv op of the step on the tensors the last run left behind: out[i] = max(out[i], ...) for conv op i;
 * for an attention-core op the largest |q|, |k|, |v| of its qkv tensor (what the core's own fp16 split stages; the fused
 * norm+qkv+attention op keeps qkv on chip and is not covered: probe an engine that runs the two launches).  Other ops: untouched.
 * out: dev float [ccdm_engine_num_ops], zeroed by the caller (calls accumulate: max over several steps of a run).
 * `row`: the step-table row the probed activations were produced with — GroupNorm's FiLM scale / shift are rebuilt from
 * emb_table[emb_row_of_sample[n] + row]; row < 0 = the last row the last ccdm_engine_run executed (the device counter itself stands
 * one past it).  The step counter is set to `row` for the probe and put back to where the run left it. */
int ccdm_engine_input_absmax(ccdm_engine* e, float* out, int row, void* stream);
/* describe op i: writes a short text ("conv3x3 32->32 @128x128 gn silu ...") */
int ccdm_engine_describe_op(const ccdm_engine* e, int i, char* buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* CCDM_HIP_H */
