// Temperature and truncation ("top-r") sampling (DenoisingModel(..., temperature=, truncation=)): the network's x0 = p(x_0 | x_t) of a
// pixel is reshaped before the reverse step — tempered relative to its largest value, then cut to the smallest set of classes whose mass
// reaches top_r — and the row's real step follows.  The step posterior is linear in x0 up to its final normalisation, so any per-pixel
// reshaping sits in front of posterior_pixel_core (softmax = 0) without renormalising: the epilogue's arithmetic and Philox counters, ONE
// definition (ccdm_sampler_common.h); the definition of the shaping itself is include/ccdm_hip.h's, restated by shape_row / shape_lds_row
// of ccdm_shaping.h (shared with ccdm_views.hip).  Like ccdm_evidence_step this kernel sits between a head that stopped at x0
// (CCDM_STEP_SOFTMAX_ONLY) and the draw, and where a
// call has evidence too the multiply x0_k * w_k happens on the way in (the evidence kernel's multiply), so this is ONE launch per walk
// entry with or without evidence.  Neutral values (1, 1) skip both parts by uniform branches: the plain step, or ccdm_evidence_step, bit
// for bit.
//
// The three regimes and the K -> KP ladder are the evidence kernel's (ccdm_evidence.hip):
//   K <= 4   one thread per pixel, 8- or 16-byte loads where K is 2 or 4;
//   K <= 32  256 pixels per block through odd-pitch LDS rows (stage_class_rows, store_onehot_rows); the shaping runs in registers: the
//            classes already taken are a 32-bit mask, the next class in order comes from an unrolled max scan (first maximum wins: ties
//            go to the lower index), and a pixel leaves the loop once its cumulated mass reaches the threshold — at most K scans of K
//            compares, one for a peaked pixel.  Lanes of a wave leave at different times (the wave runs as long as its flattest pixel);
//            no private array is indexed dynamically, so nothing goes to scratch;
//   K <= 255 64 pixels per block; the shaping works on the pixel's LDS row in place (65 280 bytes at K = 255: there is no room for a
//            second row): a taken class is marked in its sign bit (all values are >= 0), and the marks are resolved — kept value or 0 —
//            before the core reads the row.  A thread walks its own row with a k that is uniform over the wave: PITCH is odd, so the
//            lanes' addresses tid * PITCH + k fall on distinct banks; only the marking store (a per-lane k) can collide.
// x0 and out_probs may be the same buffer (in the engine they are): a pixel's K values are in registers (one thread per pixel) or the
// whole block's are in LDS behind a barrier (staged) before anything of them is written, and a block writes its own pixels only.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"
#include "ccdm_shaping.h"

#include <algorithm>
#include <cmath>

namespace ccdm {

// `a`: head = x0 (softmax = 0, head_stride = K), xt_next = xt, no table, no noise buffer, no run block: filled by the launcher below
template <int KP>
__global__ __launch_bounds__(256) void k_shaped(const ccdm_post_args a, const float* ev, const float inv_t, const float top_r, const float al,
                                                const float cu, const int mode, const int step, const int vec) {
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int K = a.K;
    float x0[KP];
    if (vec) {                               // K == KP and the rows KP * 4-byte aligned (the launcher checks)
        if constexpr (KP == 2) {
            const f32x2 p = reinterpret_cast<const f32x2*>(a.head)[i];
            x0[0] = p[0]; x0[1] = p[1];
            if (ev) {
                const f32x2 w = reinterpret_cast<const f32x2*>(ev)[i];
                x0[0] = x0[0] * w[0]; x0[1] = x0[1] * w[1];
            }
        } else {
            const f32x4 p = reinterpret_cast<const f32x4*>(a.head)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) x0[k] = p[k];
            if (ev) {
                const f32x4 w = reinterpret_cast<const f32x4*>(ev)[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) x0[k] = x0[k] * w[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < KP; ++k) x0[k] = k < K ? (ev ? a.head[i * K + k] * ev[i * K + k] : a.head[i * K + k]) : 0.f;
    }
    shape_row<KP>(x0, K, inv_t, top_r);
    posterior_pixel_core<KP>(a, i, x0, step, al, cu, mode, (int)a.xt[i]);
}

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_shaped_staged(const ccdm_post_args a, const float* ev, const float inv_t, const float top_r,
                                                       const float al, const float cu, const int mode, const int step) {
    constexpr int PITCH = (KP | 1) > CCDM_MAX_CLASSES ? CCDM_MAX_CLASSES : (KP | 1);      // odd, >= K
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i0 = (size_t)blockIdx.x * BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<size_t>(BLK, npix - i0);
    const int K = a.K;
    if (ev) stage_class_rows<BLK, PITCH, true>(sx, a.head + i0 * K, ev + i0 * K, nvalid, (unsigned)K, tid);          // uniform
    else stage_class_rows<BLK, PITCH, false>(sx, a.head + i0 * K, nullptr, nvalid, (unsigned)K, tid);
    __syncthreads();
    const bool onehot = mode == CCDM_STEP_SAMPLE && a.xin;               // uniform
    int bi = 0;
    if (tid < nvalid) {
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
    }
    if (!onehot) return;
    sb[tid] = bi;
    __syncthreads();
    const unsigned stride = (unsigned)a.xin_stride;
    store_onehot_rows<BLK>(a.xin + i0 * stride, sb, nvalid, stride, K, tid);
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_shaped_step(const float* x0, const float* evidence, int N, int HW, int K, float inv_temperature, float top_r, float alpha_t,
                                float cumalpha_tm1, int mode, int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin,
                                int xin_stride, float* out_probs, int64_t* out_onehot, void* stream) {
    const int blk = K <= 32 ? 256 : 64;
    if (const int rc = check_step_args("ccdm_shaped_step", x0 && xt, N, HW, K, xin, xin_stride, mode, step_row, blk)) return rc;
    CCDM_REQUIRE(std::isfinite(inv_temperature) && inv_temperature >= 0.05f && inv_temperature <= 20.0f,
                 "ccdm_shaped_step: inv_temperature %g outside [1/20,20]", (double)inv_temperature);
    CCDM_REQUIRE(std::isfinite(top_r) && top_r > 0.0f && top_r <= 1.0f, "ccdm_shaped_step: top_r %g outside (0,1]", (double)top_r);
    const size_t npix = (size_t)N * HW;
    ccdm_post_args a = {};
    a.head = x0; a.softmax = 0; a.head_stride = K;
    a.xt = xt; a.xt_next = xt;
    a.N = N; a.HW = HW; a.K = K;
    a.philox_seed = philox_seed; a.sample_offset = sample_offset;
    a.xin = xin; a.xin_stride = xin_stride;
    a.out_probs = out_probs; a.out_onehot = out_onehot;
    const dim3 grid((unsigned)((npix + blk - 1) / blk)), block(blk);
    hipStream_t s = (hipStream_t)stream;
    const float it = inv_temperature, tr = top_r, al = alpha_t, cu = cumalpha_tm1;
    dispatch_kp<256>(K, [&](auto c) {
        constexpr int KP = decltype(c)::value;
        if constexpr (KP <= 4) {
            const uintptr_t both = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(evidence);          // (null: no bits)
            const int vec = (K == 2 && (both & 7) == 0) || (K == 4 && (both & 15) == 0);
            hipLaunchKernelGGL(k_shaped<KP>, grid, block, 0, s, a, evidence, it, tr, al, cu, mode, step_row, vec);
        } else {
            hipLaunchKernelGGL((k_shaped_staged<KP, (KP <= 32 ? 256 : 64)>), grid, block, 0, s, a, evidence, it, tr, al, cu, mode, step_row);
        }
    });
    CCDM_CHECK_LAUNCH("ccdm_shaped_step");
    return 0;
}
