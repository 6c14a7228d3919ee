// Cityscapes prediction export, device part: the class map of a low-resolution prediction at the label resolution, written as
// train ids, as label ids and as colours (the three images of the reference's `save_preds`, evaluation/eval_cdm.py) without a
// full-resolution probability tensor.  The walk is ccdm_seg_common.h's; instead of counting, a pixel ends as one byte of class, one
// byte of label id and three bytes of colour.
//
// Stores.  The kernel is write-bound (5 bytes out per pixel), and one output column per lane would give one- and three-byte
// stores.  So the four lanes of a quad exchange their values by DPP (quad_perm broadcasts) before storing:
//   train_id / label_id  the quad's 4 bytes form one dword.  A wave holds the dwords of 4 consecutive rows, lane q of the quad
//                        keeps row q's, and one store instruction with all 64 lanes writes 4 rows x 64 bytes;
//   color                the quad's 4 pixels are 12 bytes = 3 dwords; lanes q = 0..2 build and store one each: 48 lanes write
//                        the row's 192 contiguous bytes.
// A group of 4 columns starts at a multiple of 4 counted from the row start.  When W % 4 != 0 a row starts at any byte: the
// dwords go through a 1-byte-aligned type, which the compiler lowers to dword stores where the target allows unaligned access
// and to narrower stores where it does not.  Only the last partial group of a row (W % 4 columns) is written bytewise, per lane.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int SEGX_MAX_K = SEG_MAX_K;

struct __attribute__((packed, aligned(1))) seg_u32_any { uint32_t v; };      // a dword at any byte address

__device__ __forceinline__ void seg_store_u32(uint8_t* p, uint32_t v) { reinterpret_cast<seg_u32_any*>(p)->v = v; }

// SRC: 0 fp32 probabilities, 1 class map.  IDENT: (H, W) == (h, w).  C: the channels the argmax runs over.
// table[k] = r | g << 8 | b << 16 | label id << 24 of class k.
template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_seg_export(SegSrc s, int K, const uint8_t* __restrict__ id_table, const uint8_t* __restrict__ color_table,
                                                    uint8_t* __restrict__ train_id, uint8_t* __restrict__ label_id,
                                                    uint8_t* __restrict__ color) {
    __shared__ uint32_t table[SEGX_MAX_K];
    if (threadIdx.x < SEGX_MAX_K) {
        const int k = min((int)threadIdx.x, K - 1);
        table[threadIdx.x] = (uint32_t)color_table[3 * k] | (uint32_t)color_table[3 * k + 1] << 8 | (uint32_t)color_table[3 * k + 2] << 16 |
                             (uint32_t)id_table[k] << 24;
    }
    __syncthreads();
    const int q = threadIdx.x & 3, H = s.H, W = s.W;

    for (SegTiles tiles(s.B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const int b = tile.b, x = tile.x, y_begin = tile.y_begin, y_end = tile.y_end;
        const bool in_x = tile.in_x;
        const int gx = x - q;                         // first column of the lane's group of 4
        const bool full = gx + 3 < W;                 // the group lies inside the row: dword stores
        const bool edge = in_x && !full;              // the last partial group: this lane stores its own bytes
        const SegLane<IDENT> ln(s, tile);
        float A[KP], Bv[KP];
        int yA = -1, yB = -1;
        uint32_t keep_t = 0, keep_i = 0;              // the group's train-id / label-id dword of row (batch start + q)
        for (int y = y_begin; y < y_end; ++y) {
            float h0, h1;
            seg_step<KP, SRC, V4, IDENT>(A, Bv, yA, yB, h0, h1, s, ln, b, y);
            const uint32_t pred = (uint32_t)seg_argmax<KP, IDENT>(A, Bv, h0, h1, s.C);
            const uint32_t e = table[pred];
            const size_t pix = ((size_t)b * H + y) * W + x;

            const int slot = (y - y_begin) & 3;       // wave-uniform: the row's place in the batch of 4
            const bool last = slot == 3 || y + 1 == y_end;
            if (train_id) {
                const uint32_t d = seg_quad<0>(pred) | seg_quad<1>(pred) << 8 | seg_quad<2>(pred) << 16 | seg_quad<3>(pred) << 24;
                if (q == slot) keep_t = d;
                if (edge) train_id[pix] = (uint8_t)pred;
            }
            if (label_id) {
                const uint32_t i = e >> 24;
                const uint32_t d = seg_quad<0>(i) | seg_quad<1>(i) << 8 | seg_quad<2>(i) << 16 | seg_quad<3>(i) << 24;
                if (q == slot) keep_i = d;
                if (edge) label_id[pix] = (uint8_t)i;
            }
            if (last && full && q <= slot) {          // lane q writes row (y - slot + q) of the batch, columns gx .. gx + 3
                const size_t at = ((size_t)b * H + (y - slot + q)) * W + gx;
                if (train_id) seg_store_u32(train_id + at, keep_t);
                if (label_id) seg_store_u32(label_id + at, keep_i);
            }
            if (color) {
                const uint32_t c = e & 0xFFFFFFu;
                const uint32_t c0 = seg_quad<0>(c), c1 = seg_quad<1>(c), c2 = seg_quad<2>(c), c3 = seg_quad<3>(c);
                const uint32_t d = q == 0 ? (c0 | c1 << 24) : q == 1 ? (c1 >> 8 | c2 << 16) : (c2 >> 16 | c3 << 8);
                if (full) {
                    if (q < 3) seg_store_u32(color + (pix - q) * 3 + 4 * q, d);
                } else if (in_x) {
                    color[pix * 3] = (uint8_t)c;
                    color[pix * 3 + 1] = (uint8_t)(c >> 8);
                    color[pix * 3 + 2] = (uint8_t)(c >> 16);
                }
            }
        }
    }
}

}  // namespace ccdm

extern "C" int ccdm_segexport(const float* probs, int64_t pixel_stride, const uint8_t* cls, int B, int h, int w, int H, int W, int K,
                              int scored, const uint8_t* id_table, const uint8_t* color_table, uint8_t* train_id, uint8_t* label_id,
                              uint8_t* color, void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_src("segexport", probs, pixel_stride, cls, h, w, K)) return rc;
    if (const int rc = seg_check_out("segexport", B, H, W)) return rc;
    CCDM_REQUIRE(scored == K - 1 || scored == K, "segexport: scored=%d is neither K-1 nor K (K=%d)", scored, K);
    CCDM_REQUIRE(train_id || label_id || color, "segexport: no output requested");
    CCDM_REQUIRE(id_table && color_table, "segexport: null table");
    if (B == 0) return 0;
    const SegSrc s = seg_src(probs, pixel_stride, cls, B, h, w, H, W, scored);
    seg_dispatch(s, [&](auto kp, auto src, auto v4, auto ident) {
        hipLaunchKernelGGL((k_seg_export<kp(), src(), v4(), ident()>), dim3(seg_blocks(B, H, W)), dim3(256), 0, (hipStream_t)stream, s, K,
                           id_table, color_table, train_id, label_id, color);
    });
    CCDM_CHECK_LAUNCH("segexport");
    return 0;
}
