// Boundary IoU and trimap counts of a segmentation prediction, device part: a stencil of radius d <= 64 over two class maps at the
// scored resolution [B,H,W], as two run-length passes whose cost per pixel does not depend on d.  Nothing in the reference computes
// these; the definition in include/ccdm_hip.h is the contract, tests/test_seg_boundary.py restates it with numpy / scipy.
//
// Definition.  G' = the label where it is counted (< C = K - 1), "none" elsewhere; P' = the predicted class where G is counted (and
// the class is < C), "none" elsewhere.  A pixel p of a map X with class c is interior at width d when the whole (2d+1) x (2d+1)
// window around it lies inside the image and holds c; band_X(c, d) = the pixels of class c that are not interior (the mask minus
// its erosion by a 3x3 square, d iterations, zero border).
//
// Pass 1 (k_segboundary_rows, rows; the tile walk of ccdm_seg_common.h, one column per lane).  A wave holds, per map, the 64
// pixels of its chunk of a row and of the chunk on either side, and ballots "this position starts a run" (the class differs from
// its left neighbour's, or the position is the first column, or lies outside the row) into three 64-bit masks.  A pixel's row flag
// = no run starts in [x-d+1, x+d] = the run of its class covers [x-d, x+d] inside the row: two funnel shifts of the masks per
// lane, whatever d.  It writes, per pixel, one byte per map (class, 0x7F for none, bit 7 = row flag) as one 16-bit word.
// Pass 2 (k_segboundary_cols, columns).  A lane walks down a strip of BND_STRIP rows of one column with a rolling run length
// per map: up = how many consecutive rows ending at row r hold the same flagged byte.  The pixel at y = r - d is interior iff
// up(r) >= 2d + 1 (all 2d+1 bytes of [y-d, y+d] equal and flagged; a row outside the image ends the run).  The walk starts d rows
// above the strip with up = 0: a lower bound on the true run length that is exact once it can reach 2d + 1, which is from the
// strip's first output row on.  So a strip costs BND_STRIP + 2d row steps: the halo is walked, not tiled, and BND_STRIP = 128
// keeps it at or below the strip's own rows.  The tile loop of ccdm_seg_common.h is not used here: its waves walk 16 rows each,
// which would spend 2d = 92 halo steps on 16 output rows at Cityscapes size.
//
// Counting follows ccdm_csscore: a per-block int32 LDS copy of both tables, LDS integer atomics per band pixel, one 64-bit global
// integer add per non-zero entry per block.  No float atomics: exact in any order, two identical calls are bit-identical.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int BND_MAX_D = 64;         // one chunk of 64 lanes on either side covers the row window
constexpr int BND_STRIP = 128;        // output rows of one wave's column walk
constexpr int BND_NONE = 0x7F;        // the class byte of a pixel that is not counted
constexpr int BND_FLAG = 0x80;
constexpr int BND_MAX_BLOCKS = 1024;

// The positions of a 64-pixel chunk of a row (`pos`: the lane's column, `v`: its class byte) that start a run: the class differs
// from the left neighbour's (`left63`: the class byte of lane 63 of the chunk to the left, for lane 0), or the position is column 0
// or outside the row.
__device__ __forceinline__ unsigned long long bnd_starts(int v, int left63, int pos, int W, int lane) {
    const int up = __shfl_up(v, 1);
    const int left = lane == 0 ? left63 : up;
    return __ballot(pos <= 0 || pos >= W || v != left);
}

// No run starts in [x-d+1, x+d], x the lane's column: mp, mc, mn are the start masks of the chunk to the left, the lane's own and the
// chunk to the right.
__device__ __forceinline__ bool bnd_row_flag(unsigned long long mp, unsigned long long mc, unsigned long long mn, int lane, int d) {
    const unsigned long long L = (mc << (63 - lane)) | ((mp >> lane) >> 1);       // bit 63 - k: position x - k
    const unsigned long long R = ((mc >> lane) >> 1) | (mn << (63 - lane));       // bit k: position x + 1 + k
    return (L >> (64 - d)) == 0 && (R << (64 - d)) == 0;
}

__global__ __launch_bounds__(256) void k_segboundary_rows(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ labels, int B, int H, int W,
                                                          int C, int d, uint16_t* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    for (SegTiles tiles(B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        for (int y = tile.y_begin; y < tile.y_end; ++y) {
            const size_t row = ((size_t)tile.b * H + y) * W;
            int g[3], p[3], pos[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pos[k] = tile.x + (k - 1) * SEG_TW;
                const bool in = pos[k] >= 0 && pos[k] < W;
                const int gl = in ? (int)labels[row + pos[k]] : 255, pl = in ? (int)pred[row + pos[k]] : 255;
                g[k] = gl < C ? gl : BND_NONE;
                p[k] = gl < C && pl < C ? pl : BND_NONE;
            }
            // bit 0 of the left chunk's masks (column x - lane - 64) lies outside every lane's window
            const unsigned long long gp = bnd_starts(g[0], g[0], pos[0], W, lane), gc = bnd_starts(g[1], seg_readlane(g[0], 63), pos[1], W, lane),
                                     gn = bnd_starts(g[2], seg_readlane(g[1], 63), pos[2], W, lane);
            const unsigned long long pp = bnd_starts(p[0], p[0], pos[0], W, lane), pc = bnd_starts(p[1], seg_readlane(p[0], 63), pos[1], W, lane),
                                     pn = bnd_starts(p[2], seg_readlane(p[1], 63), pos[2], W, lane);
            const int gb = g[1] | (bnd_row_flag(gp, gc, gn, lane, d) ? BND_FLAG : 0);
            const int pb = p[1] | (bnd_row_flag(pp, pc, pn, lane, d) ? BND_FLAG : 0);
            if (tile.in_x) ws[row + tile.x] = (uint16_t)(gb | pb << 8);
        }
    }
}

// The rolling run length of one map's byte down a column.
__device__ __forceinline__ int bnd_run(int up, int byte, int prev) {
    return (byte & BND_FLAG) ? (byte == prev ? up + 1 : 1) : 0;
}

struct BndShared {
    int bc[SEG_MAX_K * 3];               // [class][{band_G, band_P, both}]
    int tm[SEG_MAX_K * SEG_MAX_K];       // [target][prediction]
};

// One unit = BND_STRIP rows x 256 columns of an image: wave w of the block walks down columns 64 w .. 64 w + 63 of it.
__global__ __launch_bounds__(256) void k_segboundary_cols(const uint16_t* __restrict__ ws, int B, int H, int W, int C, int d,
                                                          unsigned long long* __restrict__ bcounts, unsigned long long* __restrict__ trimap) {
    __shared__ BndShared sh;
    for (int e = threadIdx.x; e < C * 3; e += blockDim.x) sh.bc[e] = 0;
    for (int e = threadIdx.x; e < C * C; e += blockDim.x) sh.tm[e] = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, need = 2 * d + 1;
    const int strips = (H + BND_STRIP - 1) / BND_STRIP, groups = (W + 4 * SEG_TW - 1) / (4 * SEG_TW);
    const long long units = (long long)B * strips * groups;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int gx = (int)(u % groups), sy = (int)((u / groups) % strips), b = (int)(u / ((long long)groups * strips));
        const int x = (gx * 4 + wave) * SEG_TW + lane;
        if (x - lane >= W) continue;                          // wave-uniform: the wave's chunk lies past the right edge
        const bool in_x = x < W;
        const int y_begin = sy * BND_STRIP, y_end = min(y_begin + BND_STRIP, H);
        const uint16_t* col = ws + (size_t)b * H * W + (in_x ? x : 0);
        int up_g = 0, up_p = 0, prev = 0;
#pragma unroll 4
        for (int r = max(y_begin - d, 0); r < y_end + d; ++r) {
            const int y = r - d;
            const int lead = in_x && r < H ? (int)col[(size_t)r * W] : 0;                      // unflagged: ends both runs
            const int lag = in_x && y >= y_begin ? (int)col[(size_t)y * W] : BND_NONE;         // the pixel the counts are for
            up_g = bnd_run(up_g, lead & 0xFF, prev & 0xFF);
            up_p = bnd_run(up_p, lead >> 8, prev >> 8);
            prev = lead;
            const int gc = lag & 0x7F, pc = (lag >> 8) & 0x7F;
            if (gc != BND_NONE) {                             // P' is none wherever G' is
                const bool bg = up_g < need, bp = pc != BND_NONE && up_p < need;
                if (bg) atomicAdd(&sh.bc[gc * 3], 1);
                if (bp) atomicAdd(&sh.bc[pc * 3 + 1], 1);
                if (bg && bp && gc == pc) atomicAdd(&sh.bc[gc * 3 + 2], 1);
                if (bg && pc != BND_NONE) atomicAdd(&sh.tm[gc * C + pc], 1);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * 3; e += blockDim.x)
        if (const int v = sh.bc[e]) atomicAdd(&bcounts[e], (unsigned long long)v);
    for (int e = threadIdx.x; e < C * C; e += blockDim.x)
        if (const int v = sh.tm[e]) atomicAdd(&trimap[e], (unsigned long long)v);
}

static inline long long bnd_units(int B, int H, int W) { return (long long)B * cdiv(H, BND_STRIP) * cdiv(W, 4 * SEG_TW); }

}  // namespace ccdm

extern "C" size_t ccdm_segboundary_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * H * W * sizeof(uint16_t);
}

extern "C" int ccdm_segboundary(const uint8_t* pred, const uint8_t* labels, int B, int H, int W, int K, int d, int64_t* bcounts, int64_t* trimap,
                                void* workspace, size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_out("segboundary", B, H, W)) return rc;
    CCDM_REQUIRE(K >= 2 && K <= SEG_MAX_K, "segboundary: K=%d outside [2,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(d >= 1 && d <= BND_MAX_D, "segboundary: d=%d outside [1,%d]", d, BND_MAX_D);
    if (B == 0) return 0;
    CCDM_REQUIRE(pred && labels && bcounts && trimap, "segboundary: null pointer");
    const size_t need = ccdm_segboundary_workspace_bytes(B, H, W);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "segboundary: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 1) == 0, "segboundary: the workspace must be 2-byte aligned");
    // a block keeps 32-bit counts: it covers at most ceil(units / BND_MAX_BLOCKS) units of BND_STRIP x 256 pixels
    const long long units = bnd_units(B, H, W);
    CCDM_REQUIRE((units + BND_MAX_BLOCKS - 1) / BND_MAX_BLOCKS * BND_STRIP * 4 * SEG_TW < (1LL << 31), "segboundary: too many pixels");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* ws = static_cast<uint16_t*>(workspace);
    hipLaunchKernelGGL(k_segboundary_rows, dim3(seg_blocks(B, H, W)), dim3(256), 0, st, pred, labels, B, H, W, K - 1, d, ws);
    CCDM_CHECK_LAUNCH("segboundary rows");
    hipLaunchKernelGGL(k_segboundary_cols, dim3((int)(units < BND_MAX_BLOCKS ? units : BND_MAX_BLOCKS)), dim3(256), 0, st, ws, B, H, W, K - 1, d,
                       reinterpret_cast<unsigned long long*>(bcounts), reinterpret_cast<unsigned long long*>(trimap));
    CCDM_CHECK_LAUNCH("segboundary cols");
    return 0;
}
