// Sampling with known pixel labels (the replacement method of RePaint, Lugmayr et al. 2022, for categorical diffusion): after a
// denoise step has produced x_{t-1}, every pixel whose label y is known is overwritten with a draw from the forward process at that
// step's noise level,  q(x_{t-1} | x_0 = y) = Cat(c * onehot(y) + (1 - c) / K),  c = cumalpha_{t-1}  — the same Exp(1) race as the
// step epilogue (argmax_k p_k / E_k, first maximum wins) on a Philox counter range of its own.  The last step has c = 1: the label.
// One thread per pixel, free pixels leave at once; HBM-bound: reads 1 byte per pixel, writes 1 byte (+ K floats of the stem's input)
// per KNOWN pixel.
//
// Resampling jumps (RePaint's harmonisation): ccdm_renoise_step takes the whole state back up the chain, x_t ~ q(x_t | x_{t-j}) =
// Cat(r * onehot(x_{t-j}) + (1 - r) / K) with r the ratio of the two levels' cumalphas — j forward steps in ONE draw, because uniform
// transition kernels compose in closed form.  Every pixel, known or free; the same race on a third counter range (0x40000000 | kq).
// Reads 1 byte and writes 1 byte per pixel (+ K floats where the stem reads its one-hot from memory).  Measured, these bytes are 4 %
// (64 x 128x128, K = 2) and 11 % (4 x 128x256, K = 20 with xin) of the HBM rate at the launch's time: DESIGN.md section 4.
// The race (race_hit_miss), the clamp of one pixel (clamp_known_pixel, shared with the queue's guided step), the one-hot store
// (write_onehot) and the entry points' argument checks (check_step_args) are ccdm_sampler_common.h's.
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
    clamp_known_pixel(y, i, HW, K, p_hit, p_miss, mode, step_row, k0, k1, sample_offset, xt, xin, xin_stride, out_probs, out_onehot);
}

// one thread per pixel; a byte >= K on entry (never produced by the host) counts as class K - 1
__global__ __launch_bounds__(256) void k_renoise_step(size_t npix, int HW, int K, float p_stay, float p_move, uint32_t step_row, uint32_t k0,
                                                      uint32_t k1, uint32_t sample_offset, uint8_t* __restrict__ xt, float* __restrict__ xin,
                                                      int xin_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int own = min((int)xt[i], K - 1);
    const int x = race_hit_miss(K, own, p_stay, p_move, (uint32_t)(i % HW), (uint32_t)(i / HW) + sample_offset, step_row, 0x40000000u, k0, k1);
    xt[i] = (uint8_t)x;
    if (xin) write_onehot(xin + i * xin_stride, K, x);
}

// no xin (the stem builds its one-hot from xt): a thread takes 4 consecutive pixels of the flat [N*HW] map with one 32-bit load and
// store (xt 4-byte aligned: the launcher checks); the pixels of a group may belong to two samples; the last npix % 4 bytes go one by one
__global__ __launch_bounds__(256) void k_renoise_step_x4(size_t npix, int HW, int K, float p_stay, float p_move, uint32_t step_row, uint32_t k0,
                                                         uint32_t k1, uint32_t sample_offset, uint8_t* __restrict__ xt) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i0 = q * 4;
    if (i0 >= npix) return;
    if (i0 + 4 <= npix) {
        const uint32_t in = *reinterpret_cast<const uint32_t*>(xt + i0);
        uint32_t out = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const size_t i = i0 + b;
            const int own = min((int)((in >> (8 * b)) & 0xFFu), K - 1);
            const int x = race_hit_miss(K, own, p_stay, p_move, (uint32_t)(i % HW), (uint32_t)(i / HW) + sample_offset, step_row, 0x40000000u, k0, k1);
            out |= (uint32_t)x << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(xt + i0) = out;
    } else {
        for (size_t i = i0; i < npix; ++i) {
            const int own = min((int)xt[i], K - 1);
            xt[i] = (uint8_t)race_hit_miss(K, own, p_stay, p_move, (uint32_t)(i % HW), (uint32_t)(i / HW) + sample_offset, step_row, 0x40000000u, k0, k1);
        }
    }
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_known_labels_step(const uint8_t* known, int N, int HW, int K, float p_hit, float p_miss, int mode, int step_row,
                                      uint64_t philox_seed, uint32_t sample_offset, uint8_t* xt, float* xin, int xin_stride,
                                      float* out_probs, int64_t* out_onehot, void* stream) {
    if (const int rc = check_step_args("known_labels_step", known && xt, N, HW, K, xin, xin_stride, mode, step_row, 256)) return rc;
    const size_t npix = (size_t)N * HW;
    hipLaunchKernelGGL(k_known_labels_step, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, known, npix, HW, K,
                       p_hit, p_miss, mode, (uint32_t)step_row, (uint32_t)philox_seed, (uint32_t)(philox_seed >> 32), sample_offset, xt, xin,
                       xin_stride, out_probs, out_onehot);
    CCDM_CHECK_LAUNCH("known_labels_step");
    return 0;
}

extern "C" int ccdm_renoise_step(int N, int HW, int K, float p_stay, float p_move, int step_row, uint64_t philox_seed, uint32_t sample_offset,
                                 uint8_t* xt, float* xin, int xin_stride, void* stream) {
    // (no mode argument: a renoise is always a draw)
    if (const int rc = check_step_args("renoise_step", xt != nullptr, N, HW, K, xin, xin_stride, CCDM_STEP_SAMPLE, step_row, 256)) return rc;
    const size_t npix = (size_t)N * HW;
    const uint32_t k0 = (uint32_t)philox_seed, k1 = (uint32_t)(philox_seed >> 32);
    if (!xin && ((uintptr_t)xt & 3) == 0) {
        const size_t groups = (npix + 3) / 4;
        hipLaunchKernelGGL(k_renoise_step_x4, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, npix, HW, K, p_stay,
                           p_move, (uint32_t)step_row, k0, k1, sample_offset, xt);
    } else {
        hipLaunchKernelGGL(k_renoise_step, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, npix, HW, K, p_stay,
                           p_move, (uint32_t)step_row, k0, k1, sample_offset, xt, xin, xin_stride);
    }
    CCDM_CHECK_LAUNCH("renoise_step");
    return 0;
}
