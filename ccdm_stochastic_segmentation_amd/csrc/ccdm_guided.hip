// The guided steps: the one launch behind a network pass that stopped at x0 = p(x_0 | x_t) (CCDM_STEP_SOFTMAX_ONLY).  The step
// posterior sum_d q(x_{t-1} | x_t, x_0 = d) p(x_0 = d | .) is linear in x0 up to its final normalisation, so anything that reshapes a
// pixel's x0 row sits in front of posterior_pixel_core (softmax = 0) without renormalising: the epilogue's arithmetic and Philox
// counters, ONE definition (ccdm_sampler_common.h), so neutral arguments reproduce the unguided step bit for bit.  In this order:
//   views     (DenoisingModel(..., views=), ccdm_views_step) the denoiser is averaged over mirror images of its input, x0_sym = 1/V *
//             sum_g g^-1 x0(g x_t, g img): exactly equivariant under those flips where the trained network is only approximately so.
//             The V views of a sample are V rows of the engine's batch, view-major (row v * N + j is view v of sample j), each fed its
//             mirrored x_t and image; per pixel of the identity view the kernel gathers the V rows at the mirrored positions, sums them
//             in view order and multiplies once by fp32(1 / V); after the draw — keyed by the identity view's pixel and sample, never
//             by the engine row — the class goes back to every view at its mirrored position, so the views stay mirror images.
//   evidence  (evidence=, ccdm_evidence_step) independent evidence e with likelihood p(e | x_0 = k) ~ w_k gives p(x_0 | x_t, e) ~
//             x0_k * w_k (Bayes): one fp32 multiply — no gradient, no scale, no retraining.
//   shaping   (temperature=, truncation=, ccdm_shaped_step) the row is tempered relative to its largest value, then cut to the
//             smallest set of classes whose mass reaches top_r: shape_row / shape_lds_row (ccdm_shaping.h).  (1, 1) skips both parts
//             by uniform branches.
//   tiles     (tiles=, ccdm_tiled_step; in the views' place, never together with them) a canvas larger than the network's geometry: the
//             engine's rows are overlapping tiles of the canvas state, tile-major, and x0 of a canvas pixel is the mean over the c >= 1
//             tiles that cover it, summed in tile order and multiplied once by fp32(1 / c); the draw is keyed by the canvas pixel and
//             the sample, and the class goes to the canvas state and back to every covering tile, so the tiles stay crops of one state.
//   slots     (serving.SamplingQueue, ccdm_slots_step; nothing reshaped) continuous batching: every engine row is a slot that holds a
//             sample of some request at its own place in its own walk, so what the other entries take as uniform launch arguments —
//             coefficients, mode, step row, key, sample index — comes per row from a device table.
//   guided slots  (SamplingQueue(..., guided=True), ccdm_slots_guided_step) the slots with each request's own evidence, shaping and
//             known labels: a second table and two slot-indexed pools, and the clamp at the known pixels in the same launch.
// THE definitions: include/ccdm_hip.h.  FOUR kernel pairs — one thread per pixel up to KP = 4, staged through LDS above — on the shared
// arithmetic (posterior_pixel_core, shape_row / shape_lds_row, stage_class_rows, store_onehot_rows, load_pixel_row) and ONE launch
// prologue on the host (launch_step) behind each launcher's own geometry checks:
//   k_guided / k_guided_staged  VIEWS = false is ccdm_shaped_step and, at (1, 1) with the evidence required, ccdm_evidence_step (a kernel
//             of its own for that was 1.003x / 1.00x of this one: DESIGN.md section 4); VIEWS = true is ccdm_views_step, which cannot
//             stand in for the other at V = 1 (1.07x / 1.14x, its extra LDS pass).
//   k_tiled / k_tiled_staged    ccdm_tiled_step: a run-time loop over a per-pixel number of contributors where the views' is an unrolled
//             loop over at most four.  Not one kernel with the views: their map is a bijection with a contiguous identity view (view 0
//             staged in 16-byte pieces, store_onehot_rows for it, all V - 1 index rows in LDS at once); the tiles' is neither.
//   k_slots / k_slots_staged    ccdm_slots_step.
//   k_slots_guided / k_slots_guided_staged    ccdm_slots_guided_step.  Not one kernel with the plain slots: a plain queue launches
//             the kernel it always launched.
// The staged passes stay written out per kernel: as shared helpers they measured 1 - 2 % slower at K = 20 (profiles/guided_passes_refactor_isa.txt).
//
// Shaped for HBM: per pixel 4 K V + 1 bytes in (+ 4 K of evidence), V bytes out (+ 4 K V where xin, 4 K where out_probs is written);
// measured, the launch's time is the core's arithmetic on the vector pipe, not those bytes.
//   K <= 4   one thread per pixel; a pixel's K values of an operand are one 8- or 16-byte load where K is 2 or 4.  The views are
//            summed in registers (an unrolled loop over the four possible views: nothing is indexed dynamically).
//   K <= 32  a block's 256 pixels move as what they are, one contiguous run of 256 K floats per operand, through odd-pitch LDS rows,
//            and the one-hot channels of xin leave the same way (stage_class_rows, store_onehot_rows: ccdm_sampler_common.h).
//            (K | 1) * 1 KiB of LDS per block: 4 blocks per CU at K = 32.  The shaping runs in registers: the classes already taken
//            are a 32-bit mask, the next class in order comes from an unrolled max scan (first maximum wins: ties go to the lower
//            index), and a pixel leaves the loop once its cumulated mass reaches the threshold — at most K scans of K compares, one
//            for a peaked pixel.  No private array is indexed dynamically, so nothing goes to scratch.
//   K <= 255 the same with 64 pixels per block (at most 65 536 bytes of LDS: no room for a second row per pixel, nor for V); the
//            pixel's classes no longer fit the register file and the core's arrays spill — no dataset has that many classes, and the
//            arithmetic is not written a second time for them.  The shaping works on the pixel's LDS row in place: a taken class is
//            marked in its sign bit (all values are >= 0) and the marks are resolved — kept value or 0 — before the core reads the
//            row.  A thread walks its own row with a k that is uniform over the wave: the pitch is odd, so the lanes' addresses tid *
//            pitch + k fall on distinct banks; only the marking store (a per-lane k) can collide.
//   views, staged: view 0's run is staged like any run, then every further view is added into the ONE row per pixel in a pass over
//            the block's [pixel][class] run, the pixel's source index coming from LDS (sb, written by the pixel's thread, one view at
//            a time).  A block's pixels are runs of image rows, and their sources in a mirrored view are the mirrored runs of the
//            same (x mirrored) or the mirrored (y mirrored) image rows: K contiguous floats per pixel, the pixels of an image row
//            next to one another, so a wave's 64 loads fall into the cache lines a forward run of that length covers.  The mean's
//            multiply and the evidence multiply are one more pass (the evidence run is contiguous).  After the draw the block's LDS
//            rows are free (every thread has its row in registers): they hold the pixels' indices in the mirrored views for the
//            one-hot stores, which run like store_onehot_rows with the pixel order mirrored.
// x0 and out_probs may be the same buffer (in the engine they are).  Only rows of the identity view (without views: every row) of
// out_probs are written, each by the thread that owns the pixel, after that pixel's x0 values are in registers (one thread per pixel)
// or the whole block's are in LDS behind a barrier (staged), and a block owns its pixels alone; rows of the other views are read by
// whatever block the mirror map sends them to and written by nobody.  xt: a thread reads the identity view's byte of its own pixel
// and writes that byte and its V - 1 mirror images; the mirror maps are bijections, so no byte has two writers.  The last-step modes
// write out_probs / out_onehot from the core, one thread per pixel: once per walk.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"
#include "ccdm_shaping.h"

#include <algorithm>
#include <cmath>

namespace ccdm {

// What a guided launch takes next to ccdm_post_args (whose N is the number of samples, not of engine rows).  !VIEWS reads ev alone.
struct guided_args {
    const float* ev;        // [N,HW,K] or null
    int H, W, V, flips;     // flips: 2 bits per view, bit 0 mirrors x, bit 1 mirrors y
    float inv_v;            // fp32(1 / V)
};

// the flat index, in a [V*N][HW] array, of the pixel of view v that shows pixel `pix` of sample n's identity view
__device__ __forceinline__ unsigned view_index(const guided_args& g, const int N, const int v, const unsigned n, const unsigned pix) {
    const unsigned f = ((unsigned)g.flips >> (2 * v)) & 3u;
    unsigned y = pix / (unsigned)g.W, x = pix - y * (unsigned)g.W;
    if (f & 1u) x = (unsigned)g.W - 1u - x;
    if (f & 2u) y = (unsigned)g.H - 1u - y;
    return ((unsigned)v * (unsigned)N + n) * (unsigned)(g.H * g.W) + y * (unsigned)g.W + x;
}

// p[0 .. K) = the K floats of pixel `at` of src — times those of the same pixel of wsrc, where wsrc is not null (uniform; per slot in
// k_slots_guided) —, p[k >= K] = 0.
// vec: K == KP and the rows KP * 4-byte aligned (the launcher checks)
template <int KP>
__device__ __forceinline__ void load_pixel_row(float (&p)[KP], const float* const src, const size_t at, const float* const wsrc, const int K,
                                               const int vec) {
    static_assert(KP <= 4, "the one-thread-per-pixel kernels");
    if (vec) {
        if constexpr (KP == 2) {
            const f32x2 t = reinterpret_cast<const f32x2*>(src)[at];
            p[0] = t[0]; p[1] = t[1];
            if (wsrc) {
                const f32x2 w = reinterpret_cast<const f32x2*>(wsrc)[at];
                p[0] = p[0] * w[0]; p[1] = p[1] * w[1];
            }
        } else {
            const f32x4 t = reinterpret_cast<const f32x4*>(src)[at];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = t[k];
            if (wsrc) {
                const f32x4 w = reinterpret_cast<const f32x4*>(wsrc)[at];
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = p[k] * w[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < KP; ++k) p[k] = k < K ? (wsrc ? src[at * K + k] * wsrc[at * K + k] : src[at * K + k]) : 0.f;
    }
}

// the staged kernels' LDS row pitch: odd, >= K
template <int KP>
constexpr int staged_pitch() { return (KP | 1) > CCDM_MAX_CLASSES ? CCDM_MAX_CLASSES : (KP | 1); }

// `a`: head = x0 (softmax = 0, head_stride = K), xt_next = xt, N = samples, no table, no noise buffer, no run block (launch_step)
template <int KP, bool VIEWS>
__global__ __launch_bounds__(256) void k_guided(const ccdm_post_args a, const guided_args g, const float inv_t, const float top_r, const float al,
                                                const float cu, const int mode, const int step, const int vec) {
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int K = a.K;
    float q[KP];
    [[maybe_unused]] unsigned at[4];
    if constexpr (VIEWS) {
        const unsigned n = (unsigned)(i / a.HW), pix = (unsigned)(i - (size_t)n * a.HW);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (v < g.V) {                         // uniform
                at[v] = v == 0 ? (unsigned)i : view_index(g, a.N, v, n, pix);
                float p[KP];
                load_pixel_row<KP>(p, a.head, at[v], nullptr, K, vec);
#pragma unroll
                for (int k = 0; k < KP; ++k) q[k] = v == 0 ? p[k] : q[k] + p[k];
            } else {
                at[v] = 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) q[k] = q[k] * g.inv_v;
        if (g.ev) {                                // uniform
            float w[KP];
            load_pixel_row<KP>(w, g.ev, i, nullptr, K, vec);
#pragma unroll
            for (int k = 0; k < KP; ++k) q[k] = q[k] * w[k];
        }
    } else {
        load_pixel_row<KP>(q, a.head, i, g.ev, K, vec);          // (one call: both loads issue inside the same vec branch)
    }
    shape_row<KP>(q, K, inv_t, top_r);
    if constexpr (!VIEWS) {
        posterior_pixel_core<KP>(a, i, q, step, al, cu, mode, (int)a.xt[i]);
    } else {
        int bi = 0;
        posterior_pixel_core<KP>(a, i, q, step, al, cu, mode, (int)a.xt[i], &bi);
        if (mode == CCDM_STEP_LAST_MAJORITY) bi = (int)a.xt_next[i];          // what the core has just stored: the argmax
        else if (mode != CCDM_STEP_SAMPLE) return;
        const bool onehot = mode == CCDM_STEP_SAMPLE && a.xin;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (v < g.V) {
                if (v > 0) a.xt_next[at[v]] = (uint8_t)bi;
                if (onehot) write_onehot(a.xin + (size_t)at[v] * a.xin_stride, K, bi);
            }
        }
    }
}

template <int KP, int BLK, bool VIEWS>
__global__ __launch_bounds__(BLK) void k_guided_staged(const ccdm_post_args a, const guided_args g, const float inv_t, const float top_r,
                                                       const float al, const float cu, const int mode, const int step) {
    constexpr int PITCH = staged_pitch<KP>();
    static_assert(!VIEWS || 3 * BLK <= BLK * PITCH, "the mirrored views' pixel indices reuse the rows");
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i0 = (size_t)blockIdx.x * BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<size_t>(BLK, npix - i0);
    const int K = a.K;
    const bool mine = tid < nvalid;
    [[maybe_unused]] unsigned n = 0u, pix = 0u;                          // the thread's pixel in its sample's identity view
    if constexpr (VIEWS) {
        if (mine) { n = (unsigned)((i0 + tid) / a.HW); pix = (unsigned)(i0 + tid - (size_t)n * a.HW); }
        stage_class_rows<BLK, PITCH, false>(sx, a.head + i0 * K, nullptr, nvalid, (unsigned)K, tid);
        __syncthreads();
        // the further views, added in view order into the one row per pixel; element idx of the block's run is thread idx % BLK's in
        // every pass below, so the barriers are for sb alone
        const RowDiv<~0u> row((unsigned)K);
        const int total = nvalid * K;
        for (int v = 1; v < g.V; ++v) {
            if (mine) sb[tid] = (int)view_index(g, a.N, v, n, pix);
            __syncthreads();
            for (int idx = tid; idx < total; idx += BLK) {
                const unsigned p = row((unsigned)idx), k = (unsigned)idx - p * (unsigned)K;
                sx[p * PITCH + k] = sx[p * PITCH + k] + a.head[(size_t)(unsigned)sb[p] * K + k];
            }
            __syncthreads();
        }
        for (int idx = tid; idx < total; idx += BLK) {
            const unsigned p = row((unsigned)idx), k = (unsigned)idx - p * (unsigned)K;
            float m = sx[p * PITCH + k] * g.inv_v;
            if (g.ev) m = m * g.ev[i0 * K + idx];                        // uniform
            sx[p * PITCH + k] = m;
        }
    } else {
        if (g.ev) stage_class_rows<BLK, PITCH, true>(sx, a.head + i0 * K, g.ev + i0 * K, nvalid, (unsigned)K, tid);          // uniform
        else stage_class_rows<BLK, PITCH, false>(sx, a.head + i0 * K, nullptr, nvalid, (unsigned)K, tid);
    }
    __syncthreads();
    int bi = 0;
    if (mine) {
        float x0[KP];
        if constexpr (KP <= 32) {
#pragma unroll
            for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
            shape_row<KP>(x0, K, inv_t, top_r);
        } else {
            shape_lds_row(sx + tid * PITCH, K, inv_t, top_r);            // the thread's own row: no barrier
#pragma unroll
            for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
        }
        // (&bi unconditionally: the core writes the one-hot itself only where xin is set, and where it is, store_onehot_rows does it below —
        // a pointer that does not depend on `onehot` lets bi live in a register: no scratch)
        posterior_pixel_core<KP>(a, i0 + tid, x0, step, al, cu, mode, (int)a.xt[i0 + tid], &bi);
        if constexpr (VIEWS)
            if (mode == CCDM_STEP_LAST_MAJORITY) bi = (int)a.xt_next[i0 + tid];          // what the core has just stored: the argmax
    }
    if constexpr (VIEWS)
        if (mode != CCDM_STEP_SAMPLE && mode != CCDM_STEP_LAST_MAJORITY) return;          // uniform
    const bool onehot = mode == CCDM_STEP_SAMPLE && a.xin;               // uniform
    if (!onehot) {
        if constexpr (VIEWS)
            if (mine)
                for (int v = 1; v < g.V; ++v) a.xt_next[view_index(g, a.N, v, n, pix)] = (uint8_t)bi;
        return;
    }
    if constexpr (VIEWS) __syncthreads();                                // every thread has its row in registers: sx is free
    [[maybe_unused]] int* const sat = reinterpret_cast<int*>(sx);        // [V - 1][BLK]: the pixels' indices in the mirrored views
    sb[tid] = bi;
    if constexpr (VIEWS) {
        if (mine) {
            for (int v = 1; v < g.V; ++v) {
                const unsigned at = view_index(g, a.N, v, n, pix);
                a.xt_next[at] = (uint8_t)bi;
                sat[(v - 1) * BLK + tid] = (int)at;
            }
        }
    }
    __syncthreads();
    const unsigned stride = (unsigned)a.xin_stride;
    store_onehot_rows<BLK>(a.xin + i0 * stride, sb, nvalid, stride, K, tid);
    if constexpr (VIEWS) {
        const RowDiv<~0u> chan(stride);
        const int span = nvalid * (int)stride;
        for (int v = 1; v < g.V; ++v) {
            for (int idx = tid; idx < span; idx += BLK) {
                const unsigned p = chan((unsigned)idx), c = (unsigned)idx - p * stride;
                if (c < (unsigned)K) a.xin[(size_t)(unsigned)sat[(v - 1) * BLK + p] * stride + c] = (int)c == sb[p] ? 1.0f : 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Tiles (ccdm_tiled_step): the same construction as the views with translations for mirrors and a per-pixel number of contributors.
// `a` describes the CANVAS (head = the tiles' x0, xt = xt_next = the canvas state, N = samples, HW = Hc * Wc, out_probs / out_onehot
// the canvas's, no xin: the core draws and writes the canvas state, the kernel carries the class to the covering tiles).

// What a tiled launch takes next to ccdm_post_args
struct tiled_args {
    const float* ev;        // canvas evidence [N,Hc*Wc,K] or null
    uint8_t* txt;           // the tiles' xt [R*N,h*w]
    float* txin;            // the tiles' xin [R*N,h*w,xin_stride] or null
    int xin_stride;
    int Hc, Wc, h, w, sy, sx, Ty, Tx;
    int cmax;               // the largest number of covering tiles of any canvas pixel
};

// Along one axis (extent L, tile extent l, stride s, T tiles with origins min(i * s, L - l): include/ccdm_hip.h): the tiles i0 .. i1
// that cover coordinate y.  Tile i < T - 1 starts at i * s < L - l, the last one at L - l.
__host__ __device__ __forceinline__ void covering_tiles(const int y, const int L, const int l, const int s, const int T, int& i0, int& i1) {
    i1 = y >= L - l ? T - 1 : y / s;
    const int first = y < l ? 0 : (y - l) / s + 1;                       // the first i with i * s + l > y
    i0 = first < T - 1 ? first : T - 1;
}

// a canvas pixel and the tiles i0 .. i1 x j0 .. j1 that cover it
struct tile_cover {
    unsigned n;
    int y, x, i0, i1, j0, j1;
    __device__ __forceinline__ int count() const { return (i1 - i0 + 1) * (j1 - j0 + 1); }
};

__device__ __forceinline__ tile_cover cover_of(const tiled_args& g, const size_t i) {
    tile_cover c;
    const unsigned hw = (unsigned)(g.Hc * g.Wc);
    c.n = (unsigned)(i / hw);
    const unsigned pix = (unsigned)(i - (size_t)c.n * hw);
    c.y = (int)(pix / (unsigned)g.Wc);
    c.x = (int)(pix - (unsigned)c.y * (unsigned)g.Wc);
    covering_tiles(c.y, g.Hc, g.h, g.sy, g.Ty, c.i0, c.i1);
    covering_tiles(c.x, g.Wc, g.w, g.sx, g.Tx, c.j0, c.j1);
    return c;
}

// the flat index, in a [R*N][h*w] array, of the pixel of tile (ti, tj) of sample c.n that shows the canvas pixel c
__device__ __forceinline__ unsigned tile_index(const tiled_args& g, const int N, const tile_cover& c, const int ti, const int tj) {
    const int oy = min(ti * g.sy, g.Hc - g.h), ox = min(tj * g.sx, g.Wc - g.w);
    return ((unsigned)(ti * g.Tx + tj) * (unsigned)N + c.n) * (unsigned)(g.h * g.w) + (unsigned)((c.y - oy) * g.w + (c.x - ox));
}

template <int KP>
__global__ __launch_bounds__(256) void k_tiled(const ccdm_post_args a, const tiled_args g, const float inv_t, const float top_r, const float al,
                                               const float cu, const int mode, const int step, const int vec) {
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int K = a.K;
    const tile_cover c = cover_of(g, i);
    float q[KP];
    load_pixel_row<KP>(q, a.head, tile_index(g, a.N, c, c.i0, c.j0), nullptr, K, vec);
    for (int ti = c.i0; ti <= c.i1; ++ti) {                              // ascending r = ti * Tx + tj
        for (int tj = ti == c.i0 ? c.j0 + 1 : c.j0; tj <= c.j1; ++tj) {
            float p[KP];
            load_pixel_row<KP>(p, a.head, tile_index(g, a.N, c, ti, tj), nullptr, K, vec);
#pragma unroll
            for (int k = 0; k < KP; ++k) q[k] = q[k] + p[k];
        }
    }
    const float inv_c = 1.0f / (float)c.count();
#pragma unroll
    for (int k = 0; k < KP; ++k) q[k] = q[k] * inv_c;
    if (g.ev) {                                    // uniform
        float w[KP];
        load_pixel_row<KP>(w, g.ev, i, nullptr, K, vec);
#pragma unroll
        for (int k = 0; k < KP; ++k) q[k] = q[k] * w[k];
    }
    shape_row<KP>(q, K, inv_t, top_r);
    int bi = 0;
    posterior_pixel_core<KP>(a, i, q, step, al, cu, mode, (int)a.xt[i], &bi);
    if (mode == CCDM_STEP_LAST_MAJORITY) bi = (int)a.xt_next[i];          // what the core has just stored: the argmax
    else if (mode != CCDM_STEP_SAMPLE) return;
    const bool onehot = mode == CCDM_STEP_SAMPLE && g.txin;
    for (int ti = c.i0; ti <= c.i1; ++ti) {
        for (int tj = c.j0; tj <= c.j1; ++tj) {
            const unsigned at = tile_index(g, a.N, c, ti, tj);
            g.txt[at] = (uint8_t)bi;
            if (onehot) write_onehot(g.txin + (size_t)at * g.xin_stride, K, bi);
        }
    }
}

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_tiled_staged(const ccdm_post_args a, const tiled_args g, const float inv_t, const float top_r,
                                                      const float al, const float cu, const int mode, const int step) {
    constexpr int PITCH = staged_pitch<KP>();
    static_assert(BLK <= BLK * PITCH, "the tile pixels' indices reuse the rows");
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i0 = (size_t)blockIdx.x * BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<size_t>(BLK, npix - i0);
    const int K = a.K;
    const bool mine = tid < nvalid;
    tile_cover c = {};
    int cnt = 0;
    if (mine) { c = cover_of(g, i0 + tid); cnt = c.count(); }
    // The covering tiles, added in ascending r into the one row per pixel, a pass over the block's [pixel][class] run per contributor
    // rank; the pixel's source index comes from LDS (sb, written by the pixel's thread; -1: the pixel has fewer contributors and sits
    // the pass out).  Element idx of the run is thread idx % BLK's in every pass, so the barriers are for sb alone.
    const RowDiv<~0u> row((unsigned)K);
    const int total = nvalid * K;
    int ti = c.i0, tj = c.j0;
    for (int rank = 0; rank < g.cmax; ++rank) {
        if (mine) {
            sb[tid] = rank < cnt ? (int)tile_index(g, a.N, c, ti, tj) : -1;
            if (++tj > c.j1) { tj = c.j0; ++ti; }
        }
        __syncthreads();
        for (int idx = tid; idx < total; idx += BLK) {
            const unsigned p = row((unsigned)idx), k = (unsigned)idx - p * (unsigned)K;
            const int s = sb[p];
            if (s >= 0) {
                const float v = a.head[(size_t)(unsigned)s * K + k];
                sx[p * PITCH + k] = rank == 0 ? v : sx[p * PITCH + k] + v;
            }
        }
        __syncthreads();
    }
    if (mine) sb[tid] = __float_as_int(1.0f / (float)cnt);
    __syncthreads();
    for (int idx = tid; idx < total; idx += BLK) {
        const unsigned p = row((unsigned)idx), k = (unsigned)idx - p * (unsigned)K;
        float m = sx[p * PITCH + k] * __int_as_float(sb[p]);
        if (g.ev) m = m * g.ev[i0 * K + idx];                            // uniform
        sx[p * PITCH + k] = m;
    }
    __syncthreads();
    int bi = 0;
    if (mine) {
        float x0[KP];
        if constexpr (KP <= 32) {
#pragma unroll
            for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
            shape_row<KP>(x0, K, inv_t, top_r);
        } else {
            shape_lds_row(sx + tid * PITCH, K, inv_t, top_r);            // the thread's own row: no barrier
#pragma unroll
            for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
        }
        posterior_pixel_core<KP>(a, i0 + tid, x0, step, al, cu, mode, (int)a.xt[i0 + tid], &bi);
        if (mode == CCDM_STEP_LAST_MAJORITY) bi = (int)a.xt_next[i0 + tid];          // what the core has just stored: the argmax
    }
    if (mode != CCDM_STEP_SAMPLE && mode != CCDM_STEP_LAST_MAJORITY) return;          // uniform
    const bool onehot = mode == CCDM_STEP_SAMPLE && g.txin;              // uniform
    if (!onehot) {
        if (mine)
            for (ti = c.i0; ti <= c.i1; ++ti)
                for (tj = c.j0; tj <= c.j1; ++tj) g.txt[tile_index(g, a.N, c, ti, tj)] = (uint8_t)bi;
        return;
    }
    __syncthreads();                                                     // every thread has its row in registers: sx and sb are free
    int* const sat = reinterpret_cast<int*>(sx);                         // [BLK]: the pixels' indices in the tile of the current rank
    sb[tid] = bi;
    const unsigned stride = (unsigned)g.xin_stride;
    const RowDiv<~0u> chan(stride);
    const int span = nvalid * (int)stride;
    ti = c.i0; tj = c.j0;
    for (int rank = 0; rank < g.cmax; ++rank) {
        if (mine) {
            const int at = rank < cnt ? (int)tile_index(g, a.N, c, ti, tj) : -1;
            if (at >= 0) g.txt[at] = (uint8_t)bi;
            sat[tid] = at;
            if (++tj > c.j1) { tj = c.j0; ++ti; }
        }
        __syncthreads();
        for (int idx = tid; idx < span; idx += BLK) {
            const unsigned p = chan((unsigned)idx), ch = (unsigned)idx - p * stride;
            const int at = sat[p];
            if (ch < (unsigned)K && at >= 0) g.txin[(size_t)(unsigned)at * stride + ch] = (int)ch == sb[p] ? 1.0f : 0.0f;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Slots (ccdm_slots_step): the plain step — no evidence, no shaping, one view — with every launch argument that describes the ROW
// coming per engine row from a device table (include/ccdm_hip.h: ccdm_slot_row).  `a` as launch_step fills it, without key and
// offset.  A block's pixels may belong to several slots (HW need not be a multiple of the block): the slot is found per pixel, and the
// two LDS passes of the staged kernel run per slot segment of the block, so an idle slot is neither read nor written.

// a real step mode: everything else (CCDM_SLOT_IDLE) holds nothing
__device__ __forceinline__ bool slot_runs(const int mode) { return (unsigned)mode <= (unsigned)CCDM_STEP_LAST_KEEP; }

// `a` for a pixel of slot n: the slot's key, and the offset that makes the core's sample index (n + sample_offset) the slot's `sample`
__device__ __forceinline__ ccdm_post_args slot_post_args(const ccdm_post_args& a_in, const ccdm_slot_row& r, const unsigned n) {
    ccdm_post_args a = a_in;
    a.philox_seed = (uint64_t)r.key_lo | ((uint64_t)r.key_hi << 32);
    a.sample_offset = r.sample - n;                                      // (mod 2^32, like the core's sum)
    return a;
}

template <int KP>
__global__ __launch_bounds__(256) void k_slots(const ccdm_post_args a_in, const ccdm_slot_row* const table, const int vec) {
    const size_t npix = (size_t)a_in.N * a_in.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const unsigned n = (unsigned)i / (unsigned)a_in.HW;                  // (N * HW < 2^31: the launcher checks)
    const ccdm_slot_row r = table[n];                                    // a wave inside one slot: 64 loads of one address
    if (!slot_runs(r.mode)) return;
    const ccdm_post_args a = slot_post_args(a_in, r, n);
    float q[KP];
    load_pixel_row<KP>(q, a.head, i, nullptr, a.K, vec);
    posterior_pixel_core<KP>(a, i, q, r.step_row, r.alpha_t, r.cumalpha_tm1, r.mode, (int)a.xt[i]);
}

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_slots_staged(const ccdm_post_args a_in, const ccdm_slot_row* const table) {
    constexpr int PITCH = staged_pitch<KP>();
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const unsigned HW = (unsigned)a_in.HW;
    const unsigned npix = (unsigned)a_in.N * HW;
    const unsigned i0 = blockIdx.x * (unsigned)BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<unsigned>((unsigned)BLK, npix - i0);
    const int K = a_in.K;
    const bool mine = tid < nvalid;
    // the block's slots n_lo .. n_hi; slot n holds the block's pixels [max(n * HW, i0), min((n + 1) * HW, i0 + nvalid)) — all uniform
    const unsigned n_lo = i0 / HW, n_hi = (i0 + (unsigned)nvalid - 1u) / HW;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        if (!slot_runs(table[n].mode)) continue;
        const unsigned s0 = std::max(n * HW, i0) - i0, s1 = std::min((n + 1u) * HW, i0 + (unsigned)nvalid) - i0;
        stage_class_rows<BLK, PITCH, false>(sx + s0 * PITCH, a_in.head + (size_t)(i0 + s0) * K, nullptr, (int)(s1 - s0), (unsigned)K, tid);
    }
    __syncthreads();
    int bi = 0;
    if (mine) {
        const unsigned n = (i0 + (unsigned)tid) / HW;
        const ccdm_slot_row r = table[n];
        if (slot_runs(r.mode)) {
            const ccdm_post_args a = slot_post_args(a_in, r, n);
            float x0[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
            // (&bi unconditionally, as in k_guided_staged: bi stays in a register)
            posterior_pixel_core<KP>(a, (size_t)i0 + tid, x0, r.step_row, r.alpha_t, r.cumalpha_tm1, r.mode, (int)a.xt[i0 + tid], &bi);
        }
    }
    if (!a_in.xin) return;                                               // uniform
    sb[tid] = bi;
    __syncthreads();
    const unsigned stride = (unsigned)a_in.xin_stride;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        if (table[n].mode != CCDM_STEP_SAMPLE) continue;
        const unsigned s0 = std::max(n * HW, i0) - i0, s1 = std::min((n + 1u) * HW, i0 + (unsigned)nvalid) - i0;
        store_onehot_rows<BLK>(a_in.xin + (size_t)(i0 + s0) * stride, sb + s0, (int)(s1 - s0), stride, K, tid);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Guided slots (ccdm_slots_guided_step): the slot step with every slot's own guidance — the evidence multiply, the shaping and the
// clamp at the known pixels, in the order a solo call runs them — from a second device table (include/ccdm_hip.h:
// ccdm_slot_guide_row) and two slot-indexed pools, `ev` [N,HW,K] and `known` [N,HW].  The kernels are k_slots / k_slots_staged with
// the three parts put in; the branches that are uniform in the other entries (evidence or not, shape_row's two parts) are per slot
// here, so a wave that straddles two slots diverges — nothing in them crosses lanes.  The clamp is the pixel's own thread's, behind
// the core's stores of the same pixel: one launch (DESIGN.md section 5.1 has the register counts).

// the clamp of pixel i of slot row r / guide row gr where the slot has known labels and the pixel's label is one: the class, else `bi`
__device__ __forceinline__ int slot_clamp(const ccdm_post_args& a, const ccdm_slot_row& r, const ccdm_slot_guide_row& gr, const uint8_t* const known,
                                          const size_t i, float* const xin, const int bi) {
    if (!(gr.flags & CCDM_SLOT_GUIDE_KNOWN)) return bi;
    const int y = known[i];
    if (y >= a.K) return bi;                 // free (255, or any byte that is no class)
    return clamp_known_pixel(y, i, a.HW, a.K, gr.p_hit, gr.p_miss, r.mode, (uint32_t)r.step_row, r.key_lo, r.key_hi, a.sample_offset, a.xt_next,
                             xin, a.xin_stride, a.out_probs, a.out_onehot);
}

template <int KP>
__global__ __launch_bounds__(256) void k_slots_guided(const ccdm_post_args a_in, const ccdm_slot_row* const table,
                                                      const ccdm_slot_guide_row* const guide, const float* const ev, const uint8_t* const known,
                                                      const int vec) {
    const size_t npix = (size_t)a_in.N * a_in.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const unsigned n = (unsigned)i / (unsigned)a_in.HW;                  // (N * HW < 2^31: the launcher checks)
    const ccdm_slot_row r = table[n];
    if (!slot_runs(r.mode)) return;
    const ccdm_slot_guide_row gr = guide[n];
    const ccdm_post_args a = slot_post_args(a_in, r, n);
    float q[KP];
    load_pixel_row<KP>(q, a.head, i, (gr.flags & CCDM_SLOT_GUIDE_EVIDENCE) ? ev : nullptr, a.K, vec);
    shape_row<KP>(q, a.K, gr.inv_temperature, gr.top_r);
    posterior_pixel_core<KP>(a, i, q, r.step_row, r.alpha_t, r.cumalpha_tm1, r.mode, (int)a.xt[i]);
    slot_clamp(a, r, gr, known, i, a.xin, 0);
}

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_slots_guided_staged(const ccdm_post_args a_in, const ccdm_slot_row* const table,
                                                             const ccdm_slot_guide_row* const guide, const float* const ev,
                                                             const uint8_t* const known) {
    constexpr int PITCH = staged_pitch<KP>();
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const unsigned HW = (unsigned)a_in.HW;
    const unsigned npix = (unsigned)a_in.N * HW;
    const unsigned i0 = blockIdx.x * (unsigned)BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<unsigned>((unsigned)BLK, npix - i0);
    const int K = a_in.K;
    const bool mine = tid < nvalid;
    // the block's slots and their segments as in k_slots_staged; a segment with evidence is staged times the pool's segment (the one
    // fp32 multiply of stage_class_rows<WEIGHTED>, as k_guided_staged has it)
    const unsigned n_lo = i0 / HW, n_hi = (i0 + (unsigned)nvalid - 1u) / HW;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        if (!slot_runs(table[n].mode)) continue;
        const unsigned s0 = std::max(n * HW, i0) - i0, s1 = std::min((n + 1u) * HW, i0 + (unsigned)nvalid) - i0;
        const size_t at = (size_t)(i0 + s0) * K;
        if (guide[n].flags & CCDM_SLOT_GUIDE_EVIDENCE)                   // uniform
            stage_class_rows<BLK, PITCH, true>(sx + s0 * PITCH, a_in.head + at, ev + at, (int)(s1 - s0), (unsigned)K, tid);
        else
            stage_class_rows<BLK, PITCH, false>(sx + s0 * PITCH, a_in.head + at, nullptr, (int)(s1 - s0), (unsigned)K, tid);
    }
    __syncthreads();
    int bi = 0;
    if (mine) {
        const unsigned n = (i0 + (unsigned)tid) / HW;
        const ccdm_slot_row r = table[n];
        if (slot_runs(r.mode)) {
            const ccdm_slot_guide_row gr = guide[n];
            const ccdm_post_args a = slot_post_args(a_in, r, n);
            float x0[KP];
            if constexpr (KP <= 32) {
#pragma unroll
                for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
                shape_row<KP>(x0, K, gr.inv_temperature, gr.top_r);
            } else {
                shape_lds_row(sx + tid * PITCH, K, gr.inv_temperature, gr.top_r);          // the thread's own row: no barrier
#pragma unroll
                for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
            }
            // (&bi unconditionally, as in k_guided_staged: bi stays in a register)
            posterior_pixel_core<KP>(a, (size_t)i0 + tid, x0, r.step_row, r.alpha_t, r.cumalpha_tm1, r.mode, (int)a.xt[i0 + tid], &bi);
            // the clamp replaces the pixel's entry of sb[] in a drawing slot (store_onehot_rows below writes its one-hot); in the
            // last-step modes, once per walk, the thread writes the label's one-hot into xin itself
            bi = slot_clamp(a, r, gr, known, (size_t)i0 + tid, r.mode == CCDM_STEP_SAMPLE ? nullptr : a.xin, bi);
        }
    }
    if (!a_in.xin) return;                                               // uniform
    sb[tid] = bi;
    __syncthreads();
    const unsigned stride = (unsigned)a_in.xin_stride;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        if (table[n].mode != CCDM_STEP_SAMPLE) continue;
        const unsigned s0 = std::max(n * HW, i0) - i0, s1 = std::min((n + 1u) * HW, i0 + (unsigned)nvalid) - i0;
        store_onehot_rows<BLK>(a_in.xin + (size_t)(i0 + s0) * stride, sb + s0, (int)(s1 - s0), stride, K, tid);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Host side.  What an entry hands to its launcher; a launcher reads the fields its entry has
struct guided_call {
    const float *x0, *evidence;
    int N, HW, K;
    int H, W, V, flips;                     // views: HW is H * W (formed behind the check of H and W); tiles: H x W is the canvas
    float inv_temperature, top_r, alpha_t, cumalpha_tm1;
    int mode, step_row;
    uint64_t philox_seed;
    uint32_t sample_offset;
    uint8_t* xt;
    float* xin;
    int xin_stride;
    float* out_probs;
    int64_t* out_onehot;
    void* stream;
};

// pixels per block of every launch here
static int step_block(const int K) { return K <= 32 ? 256 : 64; }

// What the launchers do alike behind their own geometry checks: the shaping's range where it is the caller's (takes_shaping),
// ccdm_post_args for c.N samples of HW pixels whose core sees `xin`, the grid, the vec flag of the one-thread-per-pixel kernels, the
// K -> KP fork.  entry(kp, go, vec) holds the entry's two launch lines: go(kernel, what it takes behind ccdm_post_args...).  0, or
// fail()'s code.
template <class F>
static int launch_step(const char* name, const guided_call& c, const int HW, const bool takes_shaping, float* const xin, F&& entry) {
    if (takes_shaping) {
        CCDM_REQUIRE(std::isfinite(c.inv_temperature) && c.inv_temperature >= 0.05f && c.inv_temperature <= 20.0f,
                     "%s: inv_temperature %g outside [1/20,20]", name, (double)c.inv_temperature);
        CCDM_REQUIRE(std::isfinite(c.top_r) && c.top_r > 0.0f && c.top_r <= 1.0f, "%s: top_r %g outside (0,1]", name, (double)c.top_r);
    }
    const int K = c.K, blk = step_block(K);
    ccdm_post_args a = {};
    a.head = c.x0; a.softmax = 0; a.head_stride = K;
    a.xt = c.xt; a.xt_next = c.xt;
    a.N = c.N; a.HW = HW; a.K = K;
    a.philox_seed = c.philox_seed; a.sample_offset = c.sample_offset;
    a.xin = xin; a.xin_stride = xin ? c.xin_stride : 0;
    a.out_probs = c.out_probs; a.out_onehot = c.out_onehot;
    const dim3 grid((unsigned)(((size_t)c.N * HW + blk - 1) / blk)), block(blk);
    const uintptr_t both = reinterpret_cast<uintptr_t>(c.x0) | reinterpret_cast<uintptr_t>(c.evidence);          // (null: no bits)
    const int vec = (K == 2 && (both & 7) == 0) || (K == 4 && (both & 15) == 0);
    const auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)c.stream, a, args...); };
    dispatch_kp<256>(K, [&](auto kp) { entry(kp, go, vec); });
    CCDM_CHECK_LAUNCH(name);
    return 0;
}

// `name`: the entry's, as its errors carry it; needs_evidence: a null evidence pointer is refused; takes_shaping: (inv_temperature,
// top_r) are the caller's and are checked.  0, or fail()'s code.
template <bool VIEWS>
static int launch_guided(const char* name, const bool needs_evidence, const bool takes_shaping, const guided_call& c) {
    const int N = c.N, K = c.K;
    int HW = c.HW;
    if constexpr (VIEWS) {
        CCDM_REQUIRE(c.V >= 1 && c.V <= 4, "%s: V=%d outside [1,4]", name, c.V);
        CCDM_REQUIRE(c.flips >= 0 && c.flips < (1 << (2 * c.V)) && (c.flips & 3) == 0, "%s: flips 0x%x (view 0 is the identity, %d views)", name,
                     c.flips, c.V);
        CCDM_REQUIRE(c.H >= 1 && c.W >= 1 && (size_t)c.H * c.W <= 0x7FFFFFFFull, "%s: bad shape H=%d W=%d", name, c.H, c.W);
        HW = c.H * c.W;
    }
    if (const int rc = check_step_args(name, c.x0 && c.xt && (c.evidence || !needs_evidence), N, HW, K, c.xin, c.xin_stride, c.mode, c.step_row,
                                       step_block(K)))
        return rc;
    if constexpr (VIEWS)
        CCDM_REQUIRE((size_t)c.V * N * HW <= 0x7FFFFFFFull, "%s: too many pixels (V*N*H*W = %zu)", name, (size_t)c.V * N * HW);
    const guided_args g = VIEWS ? guided_args{c.evidence, c.H, c.W, c.V, c.flips, 1.0f / (float)c.V} : guided_args{c.evidence, 0, 0, 1, 0, 1.0f};
    return launch_step(name, c, HW, takes_shaping, c.xin, [&](auto kp, auto go, const int vec) {
        constexpr int KP = decltype(kp)::value;
        if constexpr (KP <= 4) go(k_guided<KP, VIEWS>, g, c.inv_temperature, c.top_r, c.alpha_t, c.cumalpha_tm1, c.mode, c.step_row, vec);
        else go(k_guided_staged<KP, (KP <= 32 ? 256 : 64), VIEWS>, g, c.inv_temperature, c.top_r, c.alpha_t, c.cumalpha_tm1, c.mode, c.step_row);
    });
}

// `c` with N = samples, H x W = the canvas, xt = the canvas state, out_probs / out_onehot the canvas's, and xin / xin_stride the TILES'
// (next to their xt, tile_xt); V, flips and HW unused.
static int launch_tiled(const char* name, const guided_call& c, const int h, const int w, const int sy, const int sx, uint8_t* const tile_xt) {
    const int N = c.N, K = c.K, Hc = c.H, Wc = c.W;
    CCDM_REQUIRE(Hc >= 1 && Wc >= 1 && (size_t)Hc * Wc <= 0x7FFFFFFFull, "%s: bad shape Hc=%d Wc=%d", name, Hc, Wc);
    CCDM_REQUIRE(h >= 1 && h <= Hc && w >= 1 && w <= Wc, "%s: tile h=%d w=%d outside [1,Hc=%d] x [1,Wc=%d]", name, h, w, Hc, Wc);
    CCDM_REQUIRE(sy >= 1 && sy <= h && sx >= 1 && sx <= w, "%s: stride sy=%d sx=%d outside [1,h=%d] x [1,w=%d]", name, sy, sx, h, w);
    const int HW = Hc * Wc;
    if (const int rc = check_step_args(name, c.x0 && c.xt && tile_xt, N, HW, K, c.xin, c.xin_stride, c.mode, c.step_row, step_block(K))) return rc;
    const int Ty = 1 + (Hc - h + sy - 1) / sy, Tx = 1 + (Wc - w + sx - 1) / sx;
    CCDM_REQUIRE((size_t)N * HW <= 0x7FFFFFFFull && (size_t)Ty * Tx * N * h * w <= 0x7FFFFFFFull,
                 "%s: too many pixels (N*Hc*Wc = %zu, R*N*h*w = %zu)", name, (size_t)N * HW, (size_t)Ty * Tx * N * h * w);
    int cy = 1, cx = 1, lo, hi;
    for (int y = 0; y < Hc; ++y) { covering_tiles(y, Hc, h, sy, Ty, lo, hi); cy = std::max(cy, hi - lo + 1); }
    for (int x = 0; x < Wc; ++x) { covering_tiles(x, Wc, w, sx, Tx, lo, hi); cx = std::max(cx, hi - lo + 1); }
    const tiled_args g = {c.evidence, tile_xt, c.xin, c.xin_stride, Hc, Wc, h, w, sy, sx, Ty, Tx, cy * cx};
    return launch_step(name, c, HW, true, nullptr, [&](auto kp, auto go, const int vec) {
        constexpr int KP = decltype(kp)::value;
        if constexpr (KP <= 4) go(k_tiled<KP>, g, c.inv_temperature, c.top_r, c.alpha_t, c.cumalpha_tm1, c.mode, c.step_row, vec);
        else go(k_tiled_staged<KP, (KP <= 32 ? 256 : 64)>, g, c.inv_temperature, c.top_r, c.alpha_t, c.cumalpha_tm1, c.mode, c.step_row);
    });
}

// The shapes of launch_guided; mode and step row are the table's, on the device, so the shared check gets neutral ones.
static int launch_slots(const char* name, const float* x0, const ccdm_slot_row* table, const int N, const int HW, const int K, uint8_t* xt, float* xin,
                        const int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    if (const int rc = check_step_args(name, x0 && table && xt, N, HW, K, xin, xin_stride, CCDM_STEP_SAMPLE, 0, step_block(K))) return rc;
    CCDM_REQUIRE((size_t)N * HW <= 0x7FFFFFFFull, "%s: too many pixels (N*HW = %zu)", name, (size_t)N * HW);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3) == 0, "%s: misaligned table", name);
    guided_call c = {};                     // no evidence, key or offset: the table has the last two per row
    c.x0 = x0; c.N = N; c.K = K;
    c.xt = xt; c.xin_stride = xin_stride;
    c.out_probs = out_probs; c.out_onehot = out_onehot; c.stream = stream;
    return launch_step(name, c, HW, false, xin, [&](auto kp, auto go, const int vec) {
        constexpr int KP = decltype(kp)::value;
        if constexpr (KP <= 4) go(k_slots<KP>, table, vec);
        else go(k_slots_staged<KP, (KP <= 32 ? 256 : 64)>, table);
    });
}

// launch_slots with the guide table and the two pools.  The guide rows are on the device: their shaping's range is the host's to check
// where it forms a row, and whether a pool is needed is the table's to say (include/ccdm_hip.h: the caller's contract).  The vec
// flag covers the evidence pool's alignment (launch_step: c.evidence).
static int launch_slots_guided(const char* name, const float* x0, const ccdm_slot_row* table, const ccdm_slot_guide_row* guide, const float* ev,
                               const uint8_t* known, const int N, const int HW, const int K, uint8_t* xt, float* xin, const int xin_stride,
                               float* out_probs, int64_t* out_onehot, void* stream) {
    if (const int rc = check_step_args(name, x0 && table && guide && xt, N, HW, K, xin, xin_stride, CCDM_STEP_SAMPLE, 0, step_block(K))) return rc;
    CCDM_REQUIRE((size_t)N * HW <= 0x7FFFFFFFull, "%s: too many pixels (N*HW = %zu)", name, (size_t)N * HW);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3) == 0, "%s: misaligned table", name);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(guide) & 3) == 0, "%s: misaligned guide table", name);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(ev) & 3) == 0, "%s: misaligned evidence pool", name);
    guided_call c = {};
    c.x0 = x0; c.evidence = ev; c.N = N; c.K = K;
    c.xt = xt; c.xin_stride = xin_stride;
    c.out_probs = out_probs; c.out_onehot = out_onehot; c.stream = stream;
    return launch_step(name, c, HW, false, xin, [&](auto kp, auto go, const int vec) {
        constexpr int KP = decltype(kp)::value;
        if constexpr (KP <= 4) go(k_slots_guided<KP>, table, guide, ev, known, vec);
        else go(k_slots_guided_staged<KP, (KP <= 32 ? 256 : 64)>, table, guide, ev, known);
    });
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_slots_guided_step(const float* x0, const ccdm_slot_row* table, const ccdm_slot_guide_row* guide, const float* evidence,
                                      const uint8_t* known, int N, int HW, int K, uint8_t* xt, float* xin, int xin_stride, float* out_probs,
                                      int64_t* out_onehot, void* stream) {
    return launch_slots_guided("ccdm_slots_guided_step", x0, table, guide, evidence, known, N, HW, K, xt, xin, xin_stride, out_probs, out_onehot,
                               stream);
}

extern "C" int ccdm_slots_step(const float* x0, const ccdm_slot_row* table, int N, int HW, int K, uint8_t* xt, float* xin, int xin_stride,
                               float* out_probs, int64_t* out_onehot, void* stream) {
    return launch_slots("ccdm_slots_step", x0, table, N, HW, K, xt, xin, xin_stride, out_probs, out_onehot, stream);
}

extern "C" int ccdm_evidence_step(const float* x0, const float* evidence, int N, int HW, int K, float alpha_t, float cumalpha_tm1, int mode,
                                  int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin, int xin_stride,
                                  float* out_probs, int64_t* out_onehot, void* stream) {
    return launch_guided<false>("evidence_step", true, false,
                                {x0, evidence, N, HW, K, 0, 0, 1, 0, 1.0f, 1.0f, alpha_t, cumalpha_tm1, mode, step_row, philox_seed, sample_offset,
                                 xt, xin, xin_stride, out_probs, out_onehot, stream});
}

extern "C" int ccdm_shaped_step(const float* x0, const float* evidence, int N, int HW, int K, float inv_temperature, float top_r, float alpha_t,
                                float cumalpha_tm1, int mode, int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin,
                                int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    return launch_guided<false>("ccdm_shaped_step", false, true,
                                {x0, evidence, N, HW, K, 0, 0, 1, 0, inv_temperature, top_r, alpha_t, cumalpha_tm1, mode, step_row, philox_seed,
                                 sample_offset, xt, xin, xin_stride, out_probs, out_onehot, stream});
}

extern "C" int ccdm_views_step(const float* x0, const float* evidence, int N, int H, int W, int K, int V, int flips, float inv_temperature, float top_r,
                               float alpha_t, float cumalpha_tm1, int mode, int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt,
                               float* xin, int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    return launch_guided<true>("ccdm_views_step", false, true,
                               {x0, evidence, N, 0, K, H, W, V, flips, inv_temperature, top_r, alpha_t, cumalpha_tm1, mode, step_row, philox_seed,
                                sample_offset, xt, xin, xin_stride, out_probs, out_onehot, stream});
}

extern "C" int ccdm_tiled_step(const float* x0, const float* evidence, int N, int Hc, int Wc, int h, int w, int sy, int sx, int K, float inv_temperature,
                               float top_r, float alpha_t, float cumalpha_tm1, int mode, int step_row, uint64_t philox_seed, uint32_t sample_offset,
                               uint8_t* canvas_xt, uint8_t* xt, float* xin, int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    return launch_tiled("ccdm_tiled_step",
                        {x0, evidence, N, 0, K, Hc, Wc, 1, 0, inv_temperature, top_r, alpha_t, cumalpha_tm1, mode, step_row, philox_seed,
                         sample_offset, canvas_xt, xin, xin_stride, out_probs, out_onehot, stream},
                        h, w, sy, sx, xt);
}
