// Flip-averaged sampling (DenoisingModel(..., views=)): the denoiser is averaged over a set of mirror images of its input,
// x0_sym = 1/V * sum_g g^-1 x0(g x_t, g img), which makes it exactly equivariant under those flips where the trained network is only
// approximately so.  A mean of probability vectors is a probability vector and the step posterior is linear in x0 up to its own
// normalisation, so the mean sits in front of posterior_pixel_core (softmax = 0) like the evidence multiply and the shaping do.  The V
// views of a sample are V rows of the engine's batch, view-major (row v * N + j is view v of sample j), each fed its mirrored x_t and
// image; this kernel is the one launch behind the network pass that stopped at x0 (CCDM_STEP_SOFTMAX_ONLY): per pixel of the identity
// view it gathers the V rows at the mirrored positions, takes their mean, applies the evidence and the shaping (ccdm_shaped_step's
// arithmetic: ccdm_shaping.h), does the row's real step with the counters of the unguided draw — keyed by the identity view's pixel and
// sample, never by the engine row — and scatters the drawn class back to every view at its mirrored position, so the views' states
// stay mirror images of one another.  THE definition: include/ccdm_hip.h.
//
// The regimes and the K -> KP ladder are the evidence and the shaped kernel's:
//   K <= 4   one thread per pixel: V loads of 8 or 16 bytes where K is 2 or 4, summed in registers (an unrolled loop over the four
//            possible views: nothing is indexed dynamically);
//   K <= 32  256 pixels per block, K <= 255 64 pixels per block, through ONE odd-pitch LDS row per pixel (at K = 255 there is no room
//            for V of them): view 0's run is staged as the shaped kernel stages it (stage_class_rows), then every further view is
//            added into the rows in a pass over the block's [pixel][class] run, the pixel's source index coming from LDS (sb, written
//            by the pixel's thread, one view at a time).  A block's pixels are runs of image rows, and their sources in a mirrored
//            view are the mirrored runs of the same (x mirrored) or the mirrored (y mirrored) image rows: K contiguous floats per
//            pixel, the pixels of an image row next to one another, so a wave's 64 loads fall into the cache lines a forward run of
//            that length covers.  The mean's multiply and the evidence multiply are one more pass (the evidence run is contiguous).
//            After the draw the block's LDS rows are free (every thread has its row in registers): they hold the pixels' indices in
//            the mirrored views for the one-hot stores, which run like store_onehot_rows with the pixel order mirrored.
// x0 and out_probs may be the same buffer (in the engine they are): only view-0 rows of out_probs are written, each by the thread that
// owns the pixel, which is also the only reader of that pixel's view-0 row, after it has read it; rows of the other views are read by
// whatever block the mirror map sends them to and written by nobody.  xt: a thread reads view 0's byte of its own pixel and writes
// that byte and its V - 1 mirror images; the mirror maps are bijections, so no byte has two writers.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"
#include "ccdm_shaping.h"

#include <algorithm>
#include <cmath>

namespace ccdm {

// What a views launch adds to ccdm_post_args (whose N is the number of samples, not of engine rows)
struct views_args {
    const float* ev;        // [N,HW,K] or null
    int H, W, V, flips;     // flips: 2 bits per view, bit 0 mirrors x, bit 1 mirrors y
    float inv_v;            // fp32(1 / V)
};

// the flat index, in a [V*N][HW] array, of the pixel of view v that shows pixel `pix` of sample n's identity view
__device__ __forceinline__ unsigned view_index(const views_args& g, const int N, const int v, const unsigned n, const unsigned pix) {
    const unsigned f = ((unsigned)g.flips >> (2 * v)) & 3u;
    unsigned y = pix / (unsigned)g.W, x = pix - y * (unsigned)g.W;
    if (f & 1u) x = (unsigned)g.W - 1u - x;
    if (f & 2u) y = (unsigned)g.H - 1u - y;
    return ((unsigned)v * (unsigned)N + n) * (unsigned)(g.H * g.W) + y * (unsigned)g.W + x;
}

// `a`: head = x0 (softmax = 0, head_stride = K), xt_next = xt, N = samples, no table, no noise buffer, no run block (the launcher below)
template <int KP>
__global__ __launch_bounds__(256) void k_views(const ccdm_post_args a, const views_args g, const float inv_t, const float top_r, const float al,
                                               const float cu, const int mode, const int step, const int vec) {
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int K = a.K;
    const unsigned n = (unsigned)(i / a.HW), pix = (unsigned)(i - (size_t)n * a.HW);
    unsigned at[4];
    float q[KP];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (v < g.V) {                         // uniform
            at[v] = v == 0 ? (unsigned)i : view_index(g, a.N, v, n, pix);
            float p[KP];
            if (vec) {                         // K == KP and the rows KP * 4-byte aligned (the launcher checks)
                if constexpr (KP == 2) {
                    const f32x2 t = reinterpret_cast<const f32x2*>(a.head)[at[v]];
                    p[0] = t[0]; p[1] = t[1];
                } else {
                    const f32x4 t = reinterpret_cast<const f32x4*>(a.head)[at[v]];
#pragma unroll
                    for (int k = 0; k < 4; ++k) p[k] = t[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < KP; ++k) p[k] = k < K ? a.head[(size_t)at[v] * K + k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) q[k] = v == 0 ? p[k] : q[k] + p[k];
        } else {
            at[v] = 0u;
        }
    }
    float w[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) w[k] = 1.0f;
    if (g.ev) {
        if (vec) {
            if constexpr (KP == 2) {
                const f32x2 t = reinterpret_cast<const f32x2*>(g.ev)[i];
                w[0] = t[0]; w[1] = t[1];
            } else {
                const f32x4 t = reinterpret_cast<const f32x4*>(g.ev)[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = t[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) w[k] = g.ev[i * K + k];
        }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        q[k] = q[k] * g.inv_v;
        if (g.ev) q[k] = q[k] * w[k];
    }
    shape_row<KP>(q, K, inv_t, top_r);
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

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_views_staged(const ccdm_post_args a, const views_args g, const float inv_t, const float top_r,
                                                      const float al, const float cu, const int mode, const int step) {
    constexpr int PITCH = (KP | 1) > CCDM_MAX_CLASSES ? CCDM_MAX_CLASSES : (KP | 1);      // odd, >= K
    static_assert(3 * BLK <= BLK * PITCH, "the mirrored views' pixel indices reuse the rows");
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i0 = (size_t)blockIdx.x * BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<size_t>(BLK, npix - i0);
    const int K = a.K, V = g.V;
    const bool mine = tid < nvalid;
    const unsigned n = mine ? (unsigned)((i0 + tid) / a.HW) : 0u, pix = mine ? (unsigned)(i0 + tid - (size_t)n * a.HW) : 0u;
    stage_class_rows<BLK, PITCH, false>(sx, a.head + i0 * K, nullptr, nvalid, (unsigned)K, tid);
    __syncthreads();
    // the further views, added in view order into the one row per pixel; element idx of the block's run is thread idx % BLK's in every
    // pass below, so the barriers are for sb alone
    const RowDiv<~0u> row((unsigned)K);
    const int total = nvalid * K;
    for (int v = 1; v < V; ++v) {
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
    const bool onehot = mode == CCDM_STEP_SAMPLE && a.xin;               // uniform
    if (!onehot) {
        if (mine)
            for (int v = 1; v < V; ++v) a.xt_next[view_index(g, a.N, v, n, pix)] = (uint8_t)bi;
        return;
    }
    __syncthreads();                                                     // every thread has its row in registers: sx is free
    int* const sat = reinterpret_cast<int*>(sx);                         // [V - 1][BLK]: the pixels' indices in the mirrored views
    sb[tid] = bi;
    if (mine) {
        for (int v = 1; v < V; ++v) {
            const unsigned at = view_index(g, a.N, v, n, pix);
            a.xt_next[at] = (uint8_t)bi;
            sat[(v - 1) * BLK + tid] = (int)at;
        }
    }
    __syncthreads();
    const unsigned stride = (unsigned)a.xin_stride;
    store_onehot_rows<BLK>(a.xin + i0 * stride, sb, nvalid, stride, K, tid);
    const RowDiv<~0u> chan(stride);
    const int span = nvalid * (int)stride;
    for (int v = 1; v < V; ++v) {
        for (int idx = tid; idx < span; idx += BLK) {
            const unsigned p = chan((unsigned)idx), c = (unsigned)idx - p * stride;
            if (c < (unsigned)K) a.xin[(size_t)(unsigned)sat[(v - 1) * BLK + p] * stride + c] = (int)c == sb[p] ? 1.0f : 0.0f;
        }
    }
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_views_step(const float* x0, const float* evidence, int N, int H, int W, int K, int V, int flips, float inv_temperature, float top_r,
                               float alpha_t, float cumalpha_tm1, int mode, int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt,
                               float* xin, int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    const int blk = K <= 32 ? 256 : 64;
    CCDM_REQUIRE(V >= 1 && V <= 4, "ccdm_views_step: V=%d outside [1,4]", V);
    CCDM_REQUIRE(flips >= 0 && flips < (1 << (2 * V)) && (flips & 3) == 0, "ccdm_views_step: flips 0x%x (view 0 is the identity, %d views)", flips, V);
    CCDM_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= 0x7FFFFFFFull, "ccdm_views_step: bad shape H=%d W=%d", H, W);
    const int HW = H * W;
    if (const int rc = check_step_args("ccdm_views_step", x0 && xt, N, HW, K, xin, xin_stride, mode, step_row, blk)) return rc;
    CCDM_REQUIRE((size_t)V * N * HW <= 0x7FFFFFFFull, "ccdm_views_step: too many pixels (V*N*H*W = %zu)", (size_t)V * N * HW);
    CCDM_REQUIRE(std::isfinite(inv_temperature) && inv_temperature >= 0.05f && inv_temperature <= 20.0f,
                 "ccdm_views_step: inv_temperature %g outside [1/20,20]", (double)inv_temperature);
    CCDM_REQUIRE(std::isfinite(top_r) && top_r > 0.0f && top_r <= 1.0f, "ccdm_views_step: top_r %g outside (0,1]", (double)top_r);
    const size_t npix = (size_t)N * HW;
    ccdm_post_args a = {};
    a.head = x0; a.softmax = 0; a.head_stride = K;
    a.xt = xt; a.xt_next = xt;
    a.N = N; a.HW = HW; a.K = K;
    a.philox_seed = philox_seed; a.sample_offset = sample_offset;
    a.xin = xin; a.xin_stride = xin_stride;
    a.out_probs = out_probs; a.out_onehot = out_onehot;
    const views_args g = {evidence, H, W, V, flips, 1.0f / (float)V};
    const dim3 grid((unsigned)((npix + blk - 1) / blk)), block(blk);
    hipStream_t s = (hipStream_t)stream;
    const float it = inv_temperature, tr = top_r, al = alpha_t, cu = cumalpha_tm1;
    dispatch_kp<256>(K, [&](auto c) {
        constexpr int KP = decltype(c)::value;
        if constexpr (KP <= 4) {
            const uintptr_t both = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(evidence);          // (null: no bits)
            const int vec = (K == 2 && (both & 7) == 0) || (K == 4 && (both & 15) == 0);
            hipLaunchKernelGGL(k_views<KP>, grid, block, 0, s, a, g, it, tr, al, cu, mode, step_row, vec);
        } else {
            hipLaunchKernelGGL((k_views_staged<KP, (KP <= 32 ? 256 : 64)>), grid, block, 0, s, a, g, it, tr, al, cu, mode, step_row);
        }
    });
    CCDM_CHECK_LAUNCH("ccdm_views_step");
    return 0;
}
