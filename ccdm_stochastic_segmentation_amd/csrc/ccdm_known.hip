// Sampling with known pixel labels (the replacement method of RePaint, Lugmayr et al. 2022, for categorical diffusion): after a
// denoise step has produced x_{t-1}, every pixel whose label y is known is overwritten with a draw from the forward process at that
// step's noise level,  q(x_{t-1} | x_0 = y) = Cat(c * onehot(y) + (1 - c) / K),  c = cumalpha_{t-1}  — the same Exp(1) race as the
// step epilogue (argmax_k p_k / E_k, first maximum wins) on a Philox counter range of its own.  The last step has c = 1: the label.
// One thread per pixel, free pixels leave at once; HBM-bound: reads 1 byte per pixel, writes 1 byte (+ K floats of the stem's input)
// per KNOWN pixel.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"

namespace ccdm {

__global__ __launch_bounds__(256) void k_known_labels_step(const uint8_t* __restrict__ known, size_t npix, int HW, int K, float p_hit,
                                                           float p_miss, int mode, uint32_t step_row, uint32_t k0, uint32_t k1,
                                                           uint32_t sample_offset, uint8_t* __restrict__ xt, float* __restrict__ xin,
                                                           int xin_stride, float* __restrict__ out_probs, int64_t* __restrict__ out_onehot) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int y = known[i];
    if (y >= K) return;                      // free (255, or any byte that is no class): nothing of this pixel is touched
    int x = y;
    if (mode == CCDM_STEP_SAMPLE) {
        const uint32_t pix = (uint32_t)(i % HW), smp = (uint32_t)(i / HW) + sample_offset;
        float best = -INFINITY;
        x = 0;
        for (int kq = 0; kq * 4 < K; ++kq) {
            uint32_t w[4];
            Philox::run(pix, smp, step_row, 0x80000000u | (uint32_t)kq, k0, k1, w);      // (the epilogue's blocks have kq < 64)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kq * 4 + j;
                if (k < K) {
                    const float qv = (k == y ? p_hit : p_miss) / u32_to_exp1(w[j]);
                    if (qv > best) { best = qv; x = k; }
                }
            }
        }
    } else {
        if (out_probs) for (int k = 0; k < K; ++k) out_probs[i * K + k] = (k == x) ? 1.0f : 0.0f;
        if (out_onehot) for (int k = 0; k < K; ++k) out_onehot[i * K + k] = (k == x) ? 1 : 0;
    }
    xt[i] = (uint8_t)x;
    if (xin) {
        float* d = xin + i * xin_stride;
        for (int k = 0; k < K; ++k) d[k] = (k == x) ? 1.0f : 0.0f;
    }
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_known_labels_step(const uint8_t* known, int N, int HW, int K, float p_hit, float p_miss, int mode, int step_row,
                                      uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin, int xin_stride,
                                      float* out_probs, int64_t* out_onehot, void* stream) {
    CCDM_REQUIRE(known && xt, "known_labels_step: null pointer");
    CCDM_REQUIRE(N >= 1 && HW >= 1, "known_labels_step: bad shape N=%d HW=%d", N, HW);
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "known_labels_step: K=%d outside [1,%d]", K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE(!xin || xin_stride >= K, "known_labels_step: xin_stride %d < K %d", xin_stride, K);
    CCDM_REQUIRE(mode == CCDM_STEP_SAMPLE || mode == CCDM_STEP_LAST_CONFIDENCE || mode == CCDM_STEP_LAST_MAJORITY || mode == CCDM_STEP_LAST_KEEP,
                 "known_labels_step: mode %d", mode);
    CCDM_REQUIRE(step_row >= 0, "known_labels_step: step_row %d", step_row);
    const size_t npix = (size_t)N * HW;
    CCDM_REQUIRE((npix + 255) / 256 <= 0x7FFFFFFFull, "known_labels_step: too many pixels");
    hipLaunchKernelGGL(k_known_labels_step, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, known, npix, HW, K,
                       p_hit, p_miss, mode, (uint32_t)step_row, (uint32_t)philox_seed, (uint32_t)(philox_seed >> 32), sample_offset, xt, xin,
                       xin_stride, out_probs, out_onehot);
    CCDM_CHECK_LAUNCH("known_labels_step");
    return 0;
}
