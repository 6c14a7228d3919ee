// Boundary F-score counts of a segmentation prediction (Csurka et al.'s BF score, the DAVIS F-measure), device part: per image and
// class, how many contour pixels either map has and how many of them have a contour pixel of the same class within Euclidean
// distance theta <= 32 in the other map.  Nothing in the reference computes these; the definition in include/ccdm_hip.h is the
// contract, tests/test_seg_contour_f.py restates it with numpy / scipy.
//
// Definition.  G' and P' are the masked maps of ccdm_segboundary.hip ("none" where the label is not counted; P' also where the
// predicted class is not).  A pixel of class c is a contour pixel of c when one of its 4-neighbours lies inside the image and
// holds a counted class other than c; "none" and the image frame make no contour (both are the same in G' and P' and would match
// each other for free).  A contour pixel p of class c is matched when the other map of the same image has a contour pixel q of
// class c with |p - q|^2 <= theta^2, in integers.
//
// Pass 1 (k_contourf_flags; the tile walk of ccdm_seg_common.h, one column per lane).  A wave walks down its 16 rows with the masked
// pair of the rows above, at and below in registers (each pixel's two bytes are read once per wave, one row ahead), takes the left
// and right neighbours from the adjacent lanes (lanes 0 and 63 read the one pixel beyond the chunk) and writes, per pixel, one
// byte per map (class, 0x7F for none, bit 7 = contour pixel) as one 16-bit word: the word format of ccdm_segboundary.
// Pass 2 (k_contourf_match; the same tile walk).  A block holds its 64 x 64 tile of those words with a halo of theta rows and 32
// columns in LDS: (64 + 2 * 32) x 128 words = 32 KB.  The tile loop of ccdm_seg_common.h fits here, unlike in the column pass of
// ccdm_segboundary: the halo is staged once per block, not walked per wave, so 16 rows per wave cost no extra halo steps.  A
// wave takes a row of 64 pixels and skips it when none is a contour pixel.  Otherwise it goes through the rows y + dy, nearest
// first (dy = 0, -1, 1, -2, ...), skipping those without any contour pixel (one flag per staged row); for the others it ballots,
// per class its unmatched contour lanes hold (seg_for_each_group: two or three classes is typical, so the cost does not depend on
// K), "contour pixel of that class in the other map" over the 128 staged columns and tests the bits within
// +-floor(sqrt(theta^2 - dy^2)) of each lane by a funnel shift and a mask from a table filled once per block.  It stops as soon
// as every contour lane is matched, which is after a few rows wherever the prediction follows the labels.
//
// Counting follows ccdm_segboundary: a per-block int32 LDS table [C][4], one LDS integer atomic per class and row chunk (the lanes
// of a class are counted by popcount), one 64-bit global integer add per non-zero entry per block and image: the table is per
// image, so a block flushes when its tile walk moves to the next image.  No float atomics: exact in any order, two identical
// calls are bit-identical.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int CTF_MAX_THETA = 32;                 // half a chunk: the 32 staged columns on either side cover the disc
constexpr int CTF_NONE = 0x7F;                    // the class byte of a pixel that is not counted (BND_NONE of ccdm_segboundary)
constexpr int CTF_FLAG = 0x80;
constexpr int CTF_NONE2 = CTF_NONE | CTF_NONE << 8;
constexpr int CTF_COLS = 2 * SEG_TW;              // staged columns: x0 - 32 .. x0 + 95
constexpr int CTF_ROWS = SEG_TH + 2 * CTF_MAX_THETA;

// The masked pair (G' | P' << 8) of pixel (y, x) of image b; none for a pixel outside the image.
__device__ __forceinline__ int ctf_pair(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ labels, int b, int y, int x, int H, int W,
                                        int C) {
    if (y < 0 || y >= H || x < 0 || x >= W) return CTF_NONE2;
    const size_t i = ((size_t)b * H + y) * W + x;
    const int gl = labels[i], pl = pred[i];
    return (gl < C ? gl : CTF_NONE) | (gl < C && pl < C ? pl : CTF_NONE) << 8;
}

// Does neighbour byte n make centre byte c a contour pixel?
__device__ __forceinline__ bool ctf_differs(int c, int n) { return c != CTF_NONE && n != CTF_NONE && n != c; }

__global__ __launch_bounds__(256) void k_contourf_flags(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ labels, int B, int H, int W,
                                                        int C, uint16_t* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    for (SegTiles tiles(B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        if (tile.y_begin >= tile.y_end) continue;              // wave-uniform
        int up = ctf_pair(pred, labels, tile.b, tile.y_begin - 1, tile.x, H, W, C);
        int cur = ctf_pair(pred, labels, tile.b, tile.y_begin, tile.x, H, W, C);
        const int xe = lane == 0 ? tile.x - 1 : tile.x + 1;    // the pixel beyond the chunk, for its first and last lane
        for (int y = tile.y_begin; y < tile.y_end; ++y) {
            const int down = ctf_pair(pred, labels, tile.b, y + 1, tile.x, H, W, C);
            const int edge = lane == 0 || lane == 63 ? ctf_pair(pred, labels, tile.b, y, xe, H, W, C) : CTF_NONE2;
            const int l = __shfl_up(cur, 1), r = __shfl_down(cur, 1);
            const int left = lane == 0 ? edge : l, right = lane == 63 ? edge : r;
            const int g = cur & 0xFF, p = cur >> 8;
            const bool fg = ctf_differs(g, left & 0xFF) || ctf_differs(g, right & 0xFF) || ctf_differs(g, up & 0xFF) || ctf_differs(g, down & 0xFF);
            const bool fp = ctf_differs(p, left >> 8) || ctf_differs(p, right >> 8) || ctf_differs(p, up >> 8) || ctf_differs(p, down >> 8);
            if (tile.in_x) ws[((size_t)tile.b * H + y) * W + tile.x] = (uint16_t)((g | (fg ? CTF_FLAG : 0)) | (p | (fp ? CTF_FLAG : 0)) << 8);
            up = cur;
            cur = down;
        }
    }
}

struct CtfShared {
    uint16_t t[CTF_ROWS][CTF_COLS];                // the tile and its halo: row y0 - theta + r, column x0 - 32 + c
    unsigned long long mask[CTF_MAX_THETA + 1];    // by |dy|: the bits of the window that starts at column x - hw
    int shift[CTF_MAX_THETA + 1];                  // by |dy|: 32 - hw, hw = floor(sqrt(theta^2 - dy^2))
    int any[CTF_ROWS];                             // the staged row holds a contour pixel of either map
    int cnt[SEG_MAX_K * 4];                        // [class][{nP, mP, nG, mG}] of the image the block is in
};

// Lanes whose window [x - hw, x + hw] holds a set bit; lo / hi: the bits of columns x0 - 32 .. x0 + 31 / x0 + 32 .. x0 + 95, x = x0 + lane.
__device__ __forceinline__ bool ctf_window(unsigned long long lo, unsigned long long hi, int lane, int shift, unsigned long long mask) {
    const unsigned long long a = (lo >> lane) | ((hi << 1) << (63 - lane));        // bit i: column x - 32 + i
    // hw = 32 (shift 0, mask all ones): the window's 65th bit, column x + 32
    return ((a >> shift) & mask) != 0 || (shift == 0 && ((hi >> lane) & 1));
}

__device__ __forceinline__ void ctf_flush(CtfShared& sh, int C, int b, unsigned long long* __restrict__ counts) {
    for (int e = threadIdx.x; e < C * 4; e += blockDim.x)
        if (const int v = sh.cnt[e]) {
            atomicAdd(&counts[(size_t)b * C * 4 + e], (unsigned long long)v);
            sh.cnt[e] = 0;
        }
}

__global__ __launch_bounds__(256) void k_contourf_match(const uint16_t* __restrict__ ws, int B, int H, int W, int C, int theta,
                                                        unsigned long long* __restrict__ counts) {
    __shared__ CtfShared sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < C * 4; e += blockDim.x) sh.cnt[e] = 0;
    if (threadIdx.x <= theta) {
        int hw = 0;
        while ((hw + 1) * (hw + 1) + (int)threadIdx.x * (int)threadIdx.x <= theta * theta) ++hw;
        sh.shift[threadIdx.x] = 32 - hw;
        sh.mask[threadIdx.x] = hw == 32 ? ~0ull : (1ull << (2 * hw + 1)) - 1;
    }
    int cur_b = -1;
    for (SegTiles tiles(B, H, W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const int x0 = tile.x - lane, y0 = tile.y_begin - wave * SEG_ROWS;
        if (tile.b != cur_b) {                                  // block-uniform: the walk moved to the next image
            if (cur_b >= 0) {
                __syncthreads();
                ctf_flush(sh, C, cur_b, counts);
            }
            cur_b = tile.b;
        }
        __syncthreads();                                        // the previous tile is read, the tables are written
        for (int r = wave; r < SEG_TH + 2 * theta; r += SEG_WAVES) {
            const int y = y0 - theta + r, xa = x0 - 32 + lane, xb = xa + SEG_TW;
            const uint16_t* row = ws + ((size_t)tile.b * H + (y >= 0 && y < H ? y : 0)) * W;
            const bool in_y = y >= 0 && y < H;
            const int wa = in_y && xa >= 0 && xa < W ? (int)row[xa] : 0, wb = in_y && xb < W ? (int)row[xb] : 0;
            sh.t[r][lane] = (uint16_t)wa;
            sh.t[r][lane + SEG_TW] = (uint16_t)wb;
            const bool some = __ballot(((wa | wb) & (CTF_FLAG | CTF_FLAG << 8)) != 0) != 0;
            if (lane == 0) sh.any[r] = some;
        }
        __syncthreads();
        for (int y = tile.y_begin; y < tile.y_end; ++y) {
            const int r0 = y - y0 + theta;
            const int own = sh.t[r0][32 + lane];                // 0 beyond the right edge: no flag
            const int gc = own & 0x7F, pc = (own >> 8) & 0x7F;
            const bool fg = own & CTF_FLAG, fp = own & (CTF_FLAG << 8);
            if (__ballot(fg || fp) == 0) continue;
            bool hit_g = false, hit_p = false;
            for (int k = 0; k <= 2 * theta; ++k) {
                const int ady = (k + 1) >> 1, r = (k & 1) ? r0 - ady : r0 + ady;
                if (!__builtin_amdgcn_readfirstlane(sh.any[r])) continue;
                const int wa = sh.t[r][lane], wb = sh.t[r][lane + SEG_TW];
                const int shift = __builtin_amdgcn_readfirstlane(sh.shift[ady]);
                const unsigned long long mask = sh.mask[ady];
                seg_for_each_group(fp && !hit_p, pc, [&](int c, bool in_g) {          // contour pixels of P' against those of G'
                    const unsigned long long lo = __ballot((wa & 0xFF) == (c | CTF_FLAG)), hi = __ballot((wb & 0xFF) == (c | CTF_FLAG));
                    if ((lo | hi) && in_g && ctf_window(lo, hi, lane, shift, mask)) hit_p = true;
                });
                seg_for_each_group(fg && !hit_g, gc, [&](int c, bool in_g) {          // and of G' against those of P'
                    const unsigned long long lo = __ballot((wa >> 8) == (c | CTF_FLAG)), hi = __ballot((wb >> 8) == (c | CTF_FLAG));
                    if ((lo | hi) && in_g && ctf_window(lo, hi, lane, shift, mask)) hit_g = true;
                });
                if (__ballot((fp && !hit_p) || (fg && !hit_g)) == 0) break;
            }
            seg_for_each_group(fp, pc, [&](int c, bool in_g) {
                const int n = __popcll(__ballot(in_g)), m = __popcll(__ballot(in_g && hit_p));
                if (lane == 0) {
                    atomicAdd(&sh.cnt[c * 4 + 0], n);
                    if (m) atomicAdd(&sh.cnt[c * 4 + 1], m);
                }
            });
            seg_for_each_group(fg, gc, [&](int c, bool in_g) {
                const int n = __popcll(__ballot(in_g)), m = __popcll(__ballot(in_g && hit_g));
                if (lane == 0) {
                    atomicAdd(&sh.cnt[c * 4 + 2], n);
                    if (m) atomicAdd(&sh.cnt[c * 4 + 3], m);
                }
            });
        }
    }
    __syncthreads();
    if (cur_b >= 0) ctf_flush(sh, C, cur_b, counts);
}

}  // namespace ccdm

extern "C" size_t ccdm_contourf_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * H * W * sizeof(uint16_t);
}

extern "C" int ccdm_contourf(const uint8_t* pred, const uint8_t* labels, int B, int H, int W, int K, int theta, int64_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_out("contourf", B, H, W)) return rc;
    CCDM_REQUIRE(K >= 2 && K <= SEG_MAX_K, "contourf: K=%d outside [2,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(theta >= 1 && theta <= CTF_MAX_THETA, "contourf: theta=%d outside [1,%d]", theta, CTF_MAX_THETA);
    if (B == 0) return 0;
    CCDM_REQUIRE(pred && labels && counts, "contourf: null pointer");
    const size_t need = ccdm_contourf_workspace_bytes(B, H, W);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "contourf: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 1) == 0, "contourf: the workspace must be 2-byte aligned");
    if (const int rc = seg_check_block_counts("contourf", B, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint16_t* ws = static_cast<uint16_t*>(workspace);
    const int grid = seg_blocks(B, H, W);
    hipLaunchKernelGGL(k_contourf_flags, dim3(grid), dim3(256), 0, st, pred, labels, B, H, W, K - 1, ws);
    CCDM_CHECK_LAUNCH("contourf flags");
    hipLaunchKernelGGL(k_contourf_match, dim3(grid), dim3(256), 0, st, ws, B, H, W, K - 1, theta, reinterpret_cast<unsigned long long*>(counts));
    CCDM_CHECK_LAUNCH("contourf match");
    return 0;
}
