// Sampling under per-pixel soft evidence (DenoisingModel(..., evidence=)): the network's x0 = p(x_0 | x_t) of a pixel and independent
// evidence e with likelihood p(e | x_0 = k) ~ w_k give p(x_0 | x_t, e) ~ x0_k * w_k (Bayes), and the reverse step's posterior
// sum_d q(x_{t-1} | x_t, x_0 = d) p(x_0 = d | .) is linear in that vector up to its final normalisation: "multiply x0 by w, then do the
// step as before" is the whole method — no gradient, no scale, no retraining.  This kernel sits between a head that stopped at x0
// (CCDM_STEP_SOFTMAX_ONLY) and the draw:  x0'_k = x0_k * w_k (one fp32 multiply, no renormalisation: the scale cancels in the step's
// own normalisation), then posterior_pixel_core with softmax = 0 — the epilogue's arithmetic and Philox counters, ONE definition
// (ccdm_sampler_common.h), so all-ones evidence reproduces the unguided step bit for bit.
//
// Shaped for HBM: per pixel 8 K + 1 bytes in, 1 byte out (+ 4 K bytes where xin or out_probs is written).  Measured, those bytes are
// 28 % (64 x 128x128, K = 2) and 26 % (4 x 128x256, K = 20 with xin) of the HBM rate at the launch's time, which is the core's
// arithmetic on the vector pipe (three IEEE divisions, a logarithm and a quarter Philox block per class), as for the unguided draw
// kernel, which reads half the floats in 0.96x / 0.88x of the time: DESIGN.md section 4.
//   K <= 4   one thread per pixel; the pixel's K values of x0 and of the evidence are one 8- or 16-byte load each where K is 2 or 4.
//   K <= 32  a block's 256 pixels move as what they are, one contiguous run of 256 K floats per operand, multiplied on the way into
//            LDS rows, and the one-hot channels of xin leave the same way: k_posterior_staged's scheme, and its two passes
//            (stage_class_rows with the multiply, store_onehot_rows: ccdm_sampler_common.h).  (K | 1) * 1 KiB of LDS per block: 4
//            blocks per CU at K = 32.
//   K <= 255 the same with 64 pixels per block (at most 65 536 bytes of LDS); the pixel's classes no longer fit the register file and
//            the core's arrays spill — no dataset has that many classes, and the arithmetic is not written a second time for them.
// x0 and out_probs may be the same buffer (in the engine they are): a pixel's K values are in registers (one thread per pixel) or the
// whole block's are in LDS behind a barrier (staged) before anything of them is written, and a block writes its own pixels only.
// The last-step modes write out_probs / out_onehot from the core, one thread per pixel: once per walk.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"

#include <algorithm>

namespace ccdm {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// `a`: head = x0 (softmax = 0, head_stride = K), xt_next = xt, no table, no noise buffer, no run block: filled by the launcher below
template <int KP>
__global__ __launch_bounds__(256) void k_evidence(const ccdm_post_args a, const float* ev, const float al, const float cu, const int mode,
                                                  const int step, const int vec) {
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int K = a.K;
    float x0[KP];
    if (vec) {                               // K == KP and both rows KP * 4-byte aligned (the launcher checks)
        if constexpr (KP == 2) {
            const f32x2 p = reinterpret_cast<const f32x2*>(a.head)[i], w = reinterpret_cast<const f32x2*>(ev)[i];
            x0[0] = p[0] * w[0]; x0[1] = p[1] * w[1];
        } else {
            const f32x4 p = reinterpret_cast<const f32x4*>(a.head)[i], w = reinterpret_cast<const f32x4*>(ev)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) x0[k] = p[k] * w[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < KP; ++k) x0[k] = k < K ? a.head[i * K + k] * ev[i * K + k] : 0.f;
    }
    posterior_pixel_core<KP>(a, i, x0, step, al, cu, mode, (int)a.xt[i]);
}

template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_evidence_staged(const ccdm_post_args a, const float* ev, const float al, const float cu,
                                                         const int mode, const int step) {
    constexpr int PITCH = (KP | 1) > CCDM_MAX_CLASSES ? CCDM_MAX_CLASSES : (KP | 1);      // odd, >= K
    __shared__ float sx[BLK * PITCH];
    __shared__ int sb[BLK];
    const size_t npix = (size_t)a.N * a.HW;
    const size_t i0 = (size_t)blockIdx.x * BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<size_t>(BLK, npix - i0);
    const int K = a.K;
    stage_class_rows<BLK, PITCH, true>(sx, a.head + i0 * K, ev + i0 * K, nvalid, (unsigned)K, tid);
    __syncthreads();
    const bool onehot = mode == CCDM_STEP_SAMPLE && a.xin;               // uniform
    int bi = 0;
    if (tid < nvalid) {
        float x0[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) x0[k] = k < K ? sx[tid * PITCH + k] : 0.f;
        posterior_pixel_core<KP>(a, i0 + tid, x0, step, al, cu, mode, (int)a.xt[i0 + tid], onehot ? &bi : nullptr);
    }
    if (!onehot) return;
    sb[tid] = bi;
    __syncthreads();
    const unsigned stride = (unsigned)a.xin_stride;
    store_onehot_rows<BLK>(a.xin + i0 * stride, sb, nvalid, stride, K, tid);
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_evidence_step(const float* x0, const float* evidence, int N, int HW, int K, float alpha_t, float cumalpha_tm1, int mode,
                                  int step_row, uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin, int xin_stride,
                                  float* out_probs, int64_t* out_onehot, void* stream) {
    const int blk = K <= 32 ? 256 : 64;
    if (const int rc = check_step_args("evidence_step", x0 && evidence && xt, N, HW, K, xin, xin_stride, mode, step_row, blk)) return rc;
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
    const float al = alpha_t, cu = cumalpha_tm1;
    dispatch_kp<256>(K, [&](auto c) {
        constexpr int KP = decltype(c)::value;
        if constexpr (KP <= 4) {
            const uintptr_t both = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(evidence);
            const int vec = (K == 2 && (both & 7) == 0) || (K == 4 && (both & 15) == 0);
            hipLaunchKernelGGL(k_evidence<KP>, grid, block, 0, s, a, evidence, al, cu, mode, step_row, vec);
        } else {
            hipLaunchKernelGGL((k_evidence_staged<KP, (KP <= 32 ? 256 : 64)>), grid, block, 0, s, a, evidence, al, cu, mode, step_row);
        }
    });
    CCDM_CHECK_LAUNCH("evidence_step");
    return 0;
}
