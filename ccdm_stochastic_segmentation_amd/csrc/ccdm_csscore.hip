// Cityscapes script scores, device part: the integer counts behind the official pixel-level evaluation script's result file
// (the reference's evaluation/cs_eval.py: evaluatePair), in one pass over the output pixels of [B,H,W], without a
// full-resolution probability tensor and without an id image.  The walk is ccdm_seg_common.h's.  A pixel ends as its predicted
// label id (id_table[class]) and goes, together with the ground-truth label id and the ground-truth instance id, into three
// sets of counts:
//   conf       [L][L] label-id confusion matrix, every pixel counted (ignored ground truth included);
//   per_image  four pixel counts per image;
//   instances  per ground-truth instance its size, its true positives on class and on category level.
//
// Everything is an integer: exact in any order, two identical calls are bit-identical.  Reduction before atomics:
//   conf       one LDS atomic per pixel into the block's own [L][L] int32 copy, added to the int64 matrix once per block (non-zero
//              entries only);
//   per_image  ballots and scalar bit counts per row (wave-uniform counters), four global adds per (wave, tile);
//   instances  instances are large connected regions, so a lane walking down its column stays inside one instance for many
//              rows: each lane counts in registers while its key (the instance's slot) stays the same.  The lanes whose key
//              changes, and every lane at the end of a tile, are grouped by equal key (seg_for_each_group, as seg_flush groups
//              by target), summed over the wave by DPP, and one instruction of three lanes adds the group's three counts: one
//              global atomic per (wave, key, run), not one per pixel.
//
// Loads.  Ground truth is 1 byte and the instance id 2 bytes per pixel.  When W % 4 == 0 every row starts at a multiple of 4
// bytes: a lane then loads, once per 4 rows, the dword (ids) and the 8 bytes (instance ids) of its quad's 4 columns in row
// (batch start + lane's place in the quad), and the quad hands the values out by DPP (the transpose of k_seg_export's stores).
// Otherwise a row starts at any byte and every lane reads its own pixel.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int CSS_MAX_K = SEG_MAX_K;
constexpr int CSS_MAX_L = CCDM_CSSCORE_MAX_LABELS;

__device__ __forceinline__ int css_count(bool p) { return __popcll(__ballot(p)); }

// The label tables, one word per label id: bit 0 ignore_in_eval, bit 1 has_instances, bits 8.. category.
struct CssShared {
    uint32_t label[CSS_MAX_L];
    uint32_t pred_id[CSS_MAX_K];         // id_table
    int conf[CSS_MAX_L * CSS_MAX_L];     // [gt * L + pred]
};

// A lane's open run of one instance: key = b * NI + slot, -1 = none; the pixels, the class hits and the category hits since.
struct CssRun {
    int key, n, tp, cat;
};

// Adds the runs of the lanes with `f` set to instances[key][0..2], grouped by key, and closes them.  Wave-uniform call.
__device__ __forceinline__ void css_flush(bool f, CssRun& r, int32_t* __restrict__ instances, int lane) {
    seg_for_each_group(f, r.key, [&](int g, bool in_g) {
        // a lane holds at most SEG_ROWS = 16 pixels: the wave sums stay below 2^11
        const int s0 = seg_wave_sum(in_g ? (r.n | r.tp << 16) : 0);
        const int s1 = seg_wave_sum(in_g ? r.cat : 0);
        if (lane < 3) {
            const int v = lane == 0 ? (s0 & 0xFFFF) : lane == 1 ? (s0 >> 16) : s1;
            if (v) atomicAdd(&instances[(size_t)g * 3 + lane], v);
        }
    });
    if (f) r = CssRun{-1, 0, 0, 0};
}

struct CssArgs {
    const uint8_t* gt_ids;
    const uint16_t* inst_ids;
    int L, inst_base, NI;
    unsigned long long* conf;
    unsigned long long* per_image;
    int32_t* instances;
    int32_t* unknown;
};

// The wave-uniform counters of one wave's walk over a tile, and the kernel-long ones.
struct CssCounts {
    int ign, ign_diff, eval, eval_same;      // per tile
    int unk_label, unk_inst;                 // per kernel
};

// One output pixel per lane (`in`: the lane's pixel is inside the image): predicted id `pid`, ground-truth id `gt`, instance id `iid`.
__device__ __forceinline__ void css_pixel(bool in, int pid, int gt, int iid, int b, bool with_inst, const CssArgs& a, CssShared& sh,
                                          CssCounts& c, CssRun& run, int lane) {
    const int L = a.L;
    const bool ok = in && gt < L && pid < L;
    c.unk_label += css_count(in && !ok);
    const bool ign = ok && (sh.label[ok ? gt : 0] & 1u);
    if (ok) atomicAdd(&sh.conf[gt * L + pid], 1);
    c.ign += css_count(ign);
    c.ign_diff += css_count(ign && pid != gt);
    c.eval += css_count(ok && !ign);
    c.eval_same += css_count(ok && !ign && pid == gt);
    if (!with_inst) return;          // wave-uniform

    int key = -1;
    bool tp = false, cat = false, unk = false;
    if (in && iid > 1000) {
        const int slot = iid - a.inst_base, lab = iid / 1000;
        if (slot < 0 || slot >= a.NI || lab >= L) {
            unk = true;
        } else {
            const uint32_t tl = sh.label[lab];
            if (!(tl & 2u)) unk = true;                       // a label without instances has no statistics to add to
            else if (!(tl & 1u)) {                            // an instance of an ignored label is skipped
                key = b * a.NI + slot;
                tp = pid == lab;
                cat = pid < L && (sh.label[pid < L ? pid : 0] >> 8) == (tl >> 8);
            }
        }
    }
    c.unk_inst += css_count(unk);
    const bool leave = run.key >= 0 && key != run.key;
    if (__ballot(leave)) css_flush(leave, run, a.instances, lane);
    if (key >= 0) {
        run.key = key;
        run.n += 1;
        run.tp += tp ? 1 : 0;
        run.cat += cat ? 1 : 0;
    }
}

// Ground truth and instance id of the lane's pixel (x, y) in a walk over rows y_begin <= y < y_end.
// vec (W % 4 == 0): at the first row of a batch of 4 (slot == 0) lane q of a quad loads the quad's 4 columns of row y + q; the
// value of row y + slot comes from lane `slot` of the quad.
struct CssLoader {
    uint32_t g4;         // 4 ground-truth bytes of row (batch start + q)
    uint32_t i4[2];      // 4 instance ids of that row
};
__device__ __forceinline__ void css_load(CssLoader& ld, bool vec, bool with_inst, const uint8_t* __restrict__ ids, const uint16_t* __restrict__ inst,
                                         int b, int y, int y_begin, int y_end, int x, bool in_x, int H, int W, int q, int& gt, int& iid) {
    if (vec) {
        const int slot = (y - y_begin) & 3;
        if (slot == 0) {
            ld.g4 = 0, ld.i4[0] = 0, ld.i4[1] = 0;
            if (in_x && y + q < y_end) {              // W % 4 == 0: the quad's 4 columns are inside the row with x
                const size_t at = ((size_t)b * H + (y + q)) * W + (x - q);
                ld.g4 = *reinterpret_cast<const uint32_t*>(ids + at);
                if (with_inst) {
                    const uint2 v = *reinterpret_cast<const uint2*>(inst + at);
                    ld.i4[0] = v.x, ld.i4[1] = v.y;
                }
            }
        }
        gt = (int)((seg_quad_sel(ld.g4, slot) >> (8 * q)) & 0xFFu);
        iid = 0;
        if (with_inst) {
            const uint32_t lo = seg_quad_sel(ld.i4[0], slot), hi = seg_quad_sel(ld.i4[1], slot);
            iid = (int)(((q & 2 ? hi : lo) >> (16 * (q & 1))) & 0xFFFFu);
        }
    } else {
        const size_t pix = ((size_t)b * H + y) * W + x;
        gt = in_x ? (int)ids[pix] : 0;
        iid = in_x && with_inst ? (int)inst[pix] : 0;
    }
}

__device__ __forceinline__ void css_init(CssShared& sh, const CssArgs& a, const uint8_t* ign, const uint8_t* cat, const uint8_t* has,
                                         const uint8_t* id_table, int K) {
    for (int e = threadIdx.x; e < CSS_MAX_L; e += blockDim.x) {
        const int l = min(e, a.L - 1);
        sh.label[e] = (ign[l] ? 1u : 0u) | (has[l] ? 2u : 0u) | (uint32_t)cat[l] << 8;
    }
    if (id_table)
        for (int e = threadIdx.x; e < CSS_MAX_K; e += blockDim.x) sh.pred_id[e] = id_table[min(e, K - 1)];
    for (int e = threadIdx.x; e < a.L * a.L; e += blockDim.x) sh.conf[e] = 0;
    __syncthreads();
}

// per_image[b][0..3] += the tile's counts (one instruction of four lanes), and the counters start over
__device__ __forceinline__ void css_tile_end(CssCounts& c, CssRun& run, int b, bool with_inst, const CssArgs& a, int lane) {
    if (with_inst) css_flush(run.key >= 0, run, a.instances, lane);
    if (lane < 4) {
        const int v = lane == 0 ? c.ign : lane == 1 ? c.ign_diff : lane == 2 ? c.eval : c.eval_same;
        if (v) atomicAdd(&a.per_image[(size_t)b * 4 + lane], (unsigned long long)v);
    }
    c.ign = c.ign_diff = c.eval = c.eval_same = 0;
}

__device__ __forceinline__ void css_block_end(CssShared& sh, const CssCounts& c, const CssArgs& a, int lane) {
    if (lane == 0 && c.unk_label) atomicAdd(&a.unknown[0], c.unk_label);
    if (lane == 0 && c.unk_inst) atomicAdd(&a.unknown[1], c.unk_inst);
    __syncthreads();
    for (int e = threadIdx.x; e < a.L * a.L; e += blockDim.x) {
        const int v = sh.conf[e];
        if (v) atomicAdd(&a.conf[e], (unsigned long long)v);
    }
}

// The fused form.  SRC: 0 fp32 probabilities, 1 class map.  IDENT: (H, W) == (h, w).  C = K - 1: the channels the argmax runs over.
// The fields of SegSrc arrive as loose arguments: with the struct as one argument two of the scalar-load instantiations (KP 20 and 32)
// take 9 to 20 more VGPRs and lose a wave per SIMD.
template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_csscore(const float* __restrict__ probs, long long ps, const uint8_t* __restrict__ cls, int B, int h,
                                                 int w, int H, int W, int C, float sh_, float sw, int K, const uint8_t* __restrict__ id_table,
                                                 const uint8_t* __restrict__ ign, const uint8_t* __restrict__ cat,
                                                 const uint8_t* __restrict__ has, CssArgs a) {
    const SegSrc s{probs, ps, cls, B, h, w, H, W, C, sh_, sw};
    __shared__ CssShared sh;
    css_init(sh, a, ign, cat, has, id_table, K);
    const int lane = threadIdx.x & 63, q = lane & 3;
    const bool vec = (W & 3) == 0, with_inst = a.inst_ids != nullptr;
    CssCounts c = {0, 0, 0, 0, 0, 0};
    CssRun run = {-1, 0, 0, 0};
    CssLoader ld = {0, {0, 0}};

    for (SegTiles tiles(B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const int b = tile.b, x = tile.x, y_begin = tile.y_begin, y_end = tile.y_end;
        const bool in_x = tile.in_x;
        const SegLane<IDENT> ln(s, tile);
        float A[KP], Bv[KP];
        int yA = -1, yB = -1;
        for (int y = y_begin; y < y_end; ++y) {
            float h0, h1;
            seg_step<KP, SRC, V4, IDENT>(A, Bv, yA, yB, h0, h1, s, ln, b, y);
            const int pred = seg_argmax<KP, IDENT>(A, Bv, h0, h1, s.C);
            int gt, iid;
            css_load(ld, vec, with_inst, a.gt_ids, a.inst_ids, b, y, y_begin, y_end, x, in_x, H, W, q, gt, iid);
            css_pixel(in_x, (int)sh.pred_id[pred], gt, iid, b, with_inst, a, sh, c, run, lane);
        }
        css_tile_end(c, run, b, with_inst, a, lane);
    }
    css_block_end(sh, c, a, lane);
}

// The ids form: the prediction is an image of label ids at the ground truth's resolution (what the script reads from the PNGs).
__global__ __launch_bounds__(256) void k_csscore_ids(const uint8_t* __restrict__ pred_ids, int B, int H, int W, const uint8_t* __restrict__ ign,
                                                     const uint8_t* __restrict__ cat, const uint8_t* __restrict__ has, CssArgs a) {
    __shared__ CssShared sh;
    css_init(sh, a, ign, cat, has, nullptr, 0);
    const int lane = threadIdx.x & 63, q = lane & 3;
    const bool vec = (W & 3) == 0, with_inst = a.inst_ids != nullptr;
    CssCounts c = {0, 0, 0, 0, 0, 0};
    CssRun run = {-1, 0, 0, 0};
    CssLoader ld = {0, {0, 0}}, lp = {0, {0, 0}};

    for (SegTiles tiles(B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const int b = tile.b, x = tile.x, y_begin = tile.y_begin, y_end = tile.y_end;
        const bool in_x = tile.in_x;
        for (int y = y_begin; y < y_end; ++y) {
            int gt, iid, pid, none;
            css_load(ld, vec, with_inst, a.gt_ids, a.inst_ids, b, y, y_begin, y_end, x, in_x, H, W, q, gt, iid);
            css_load(lp, vec, false, pred_ids, nullptr, b, y, y_begin, y_end, x, in_x, H, W, q, pid, none);
            css_pixel(in_x, pid, gt, iid, b, with_inst, a, sh, c, run, lane);
        }
        css_tile_end(c, run, b, with_inst, a, lane);
    }
    css_block_end(sh, c, a, lane);
}

// The checks and the clearing both forms share; returns 1 when there is nothing to launch.
static int css_prepare(const char* who, const uint8_t* gt_ids, const uint16_t* inst_ids, int B, int H, int W, int L, const uint8_t* ign,
                       const uint8_t* cat, const uint8_t* has, int inst_base, int NI, int64_t* conf, int64_t* per_image, int32_t* instances,
                       int32_t* unknown, hipStream_t st, CssArgs& a) {
    if (const int rc = seg_check_out(who, B, H, W)) return rc;
    CCDM_REQUIRE(L >= 1 && L <= CSS_MAX_L, "%s: L=%d outside [1,%d]", who, L, CSS_MAX_L);
    CCDM_REQUIRE(ign && cat && has, "%s: null label table", who);
    if (B == 0) return 1;
    CCDM_REQUIRE(gt_ids && conf && per_image && unknown, "%s: null pointer", who);
    CCDM_REQUIRE(!inst_ids || (instances && NI > 0 && inst_base >= 0 && (long long)inst_base + NI <= 65536 && (long long)B * NI < (1LL << 30)),
                 "%s: instance ids need a table (inst_base=%d NI=%d B=%d)", who, inst_base, NI, B);
    CCDM_REQUIRE((W & 3) != 0 || ((reinterpret_cast<uintptr_t>(gt_ids) & 3) == 0 && (reinterpret_cast<uintptr_t>(inst_ids) & 7) == 0),
                 "%s: gt_ids must be 4-byte and inst_ids 8-byte aligned when W %% 4 == 0", who);
    if (const int rc = seg_check_block_counts(who, B, H, W)) return rc;
    a = CssArgs{gt_ids, inst_ids, L, inst_base, NI, reinterpret_cast<unsigned long long*>(conf), reinterpret_cast<unsigned long long*>(per_image),
                instances, unknown};
    if (hipMemsetAsync(per_image, 0, (size_t)B * 4 * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(unknown, 0, 2 * sizeof(int32_t), st) != hipSuccess ||
        (inst_ids && hipMemsetAsync(instances, 0, (size_t)B * NI * 3 * sizeof(int32_t), st) != hipSuccess))
        return fail("%s: clearing the outputs failed", who);
    return 0;
}

}  // namespace ccdm

extern "C" int ccdm_csscore(const float* probs, int64_t pixel_stride, const uint8_t* cls, int B, int h, int w, int H, int W, int K,
                            const uint8_t* id_table, const uint8_t* gt_ids, const uint16_t* inst_ids, int L, const uint8_t* ignore_in_eval,
                            const uint8_t* category, const uint8_t* has_instances, int inst_base, int NI, int64_t* conf, int64_t* per_image,
                            int32_t* instances, int32_t* unknown, void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_src("csscore", probs, pixel_stride, cls, h, w, K)) return rc;
    CCDM_REQUIRE(id_table, "csscore: null id_table");
    hipStream_t st = (hipStream_t)stream;
    CssArgs a;
    const int rc = css_prepare("csscore", gt_ids, inst_ids, B, H, W, L, ignore_in_eval, category, has_instances, inst_base, NI, conf, per_image,
                               instances, unknown, st, a);
    if (rc != 0) return rc < 0 ? rc : 0;
    const SegSrc s = seg_src(probs, pixel_stride, cls, B, h, w, H, W, K - 1);
    seg_dispatch(s, [&](auto kp, auto src, auto v4, auto ident) {
        hipLaunchKernelGGL((k_csscore<kp(), src(), v4(), ident()>), dim3(seg_blocks(B, H, W)), dim3(256), 0, st, s.probs, s.ps, s.cls, B, h, w, H, W,
                           s.C, s.sh, s.sw, K, id_table, ignore_in_eval, category, has_instances, a);
    });
    CCDM_CHECK_LAUNCH("csscore");
    return 0;
}

extern "C" int ccdm_csscore_ids(const uint8_t* pred_ids, int B, int H, int W, const uint8_t* gt_ids, const uint16_t* inst_ids, int L,
                                const uint8_t* ignore_in_eval, const uint8_t* category, const uint8_t* has_instances, int inst_base, int NI,
                                int64_t* conf, int64_t* per_image, int32_t* instances, int32_t* unknown, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(B == 0 || (pred_ids && ((W & 3) != 0 || (reinterpret_cast<uintptr_t>(pred_ids) & 3) == 0)),
                 "csscore_ids: pred_ids null, or not 4-byte aligned when W %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    CssArgs a;
    const int rc = css_prepare("csscore_ids", gt_ids, inst_ids, B, H, W, L, ignore_in_eval, category, has_instances, inst_base, NI, conf,
                               per_image, instances, unknown, st, a);
    if (rc != 0) return rc < 0 ? rc : 0;
    hipLaunchKernelGGL(k_csscore_ids, dim3(seg_blocks(B, H, W)), dim3(256), 0, st, pred_ids, B, H, W, ignore_in_eval, category, has_instances, a);
    CCDM_CHECK_LAUNCH("csscore_ids");
    return 0;
}
