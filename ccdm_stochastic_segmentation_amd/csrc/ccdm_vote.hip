// Multi-sample prediction (DenoisingModel.predict_multiple): S sampling passes of the same images combined on the device into a
// mean map, a per-pixel vote and two uncertainty maps.  The reference's Evaluator.predict_multiple
// (evaluation/eval_cdm.py:176-193) sums S one-hot / probability outputs on the host with `total += pred * (1 / S)`; here a pass
// is folded into running accumulators straight from the engine's uint8 class map or its channels-last probabilities, so no
// [B,K,H,W] one-hot of a pass is ever written.
//
// One thread per pixel, the pixel's K values streamed (channels-last [B,HW,K], VW-wide vector accesses where K and the pointers
// allow): a pass costs one read of its input and one read-modify-write of the accumulators, the finalize one read of them and one
// write of the maps.  The per-class counting of ccdm_vote_reduce_stack keeps K <= 32 counts in registers (compare-and-add,
// the k_pair_counts pattern of ccdm_metrics.hip) and more in an LDS column per thread.
//
// Arithmetic: total += src * w is one rounded fp32 multiply then one rounded fp32 add (no contraction), so the accumulated mean is
// bit-identical to torch-CPU's `total += pred * (1 / S)`.  Entropies are formed in fp64 from the fp32 maps (-sum p log p, nats,
// 0 log 0 = 0) and stored as fp32.
#include <initializer_list>

#include "ccdm_common.h"

namespace ccdm {

template <int VW> struct VecF;
template <> struct VecF<1> { typedef float T; };
template <> struct VecF<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <> struct VecF<4> { typedef float T __attribute__((ext_vector_type(4))); };
template <int VW> struct VecI;
template <> struct VecI<1> { typedef int32_t T; };
template <> struct VecI<2> { typedef int32_t T __attribute__((ext_vector_type(2))); };
template <> struct VecI<4> { typedef int32_t T __attribute__((ext_vector_type(4))); };

template <typename V> __device__ __forceinline__ float lane_of(const V& v, int j) { return v[j]; }
template <> __device__ __forceinline__ float lane_of<float>(const float& v, int) { return v; }
template <typename V> __device__ __forceinline__ void set_lane(V& v, int j, float x) { v[j] = x; }
template <> __device__ __forceinline__ void set_lane<float>(float& v, int, float x) { v = x; }
template <typename V> __device__ __forceinline__ int32_t ilane_of(const V& v, int j) { return v[j]; }
template <> __device__ __forceinline__ int32_t ilane_of<int32_t>(const int32_t& v, int) { return v; }
template <typename V> __device__ __forceinline__ void set_ilane(V& v, int j, int32_t x) { v[j] = x; }
template <> __device__ __forceinline__ void set_ilane<int32_t>(int32_t& v, int, int32_t x) { v = x; }

// -p log p in fp64, 0 for p <= 0
__device__ __forceinline__ double neg_plogp(double p) { return p > 0.0 ? -p * log(p) : 0.0; }

template <int VW>
__global__ __launch_bounds__(256) void k_vote_accumulate(const uint8_t* __restrict__ cls, const float* __restrict__ probs, int64_t stride,
                                                         int64_t npix, int HW, int K, float w, float* __restrict__ total,
                                                         int32_t* __restrict__ counts, float* __restrict__ ent_sum) {
    typedef typename VecF<VW>::T vf;
    typedef typename VecI<VW>::T vi;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= npix) return;
    const int64_t b = n / HW, p = n - b * HW;
    const size_t o = (size_t)n * K;
    if (cls) {
        const int c = cls[b * stride + p];
        for (int k0 = 0; k0 < K; k0 += VW) {
            if (total) {
                vf t = *reinterpret_cast<const vf*>(total + o + k0);
#pragma unroll
                for (int j = 0; j < VW; ++j) set_lane(t, j, __fadd_rn(lane_of(t, j), __fmul_rn(k0 + j == c ? 1.0f : 0.0f, w)));
                *reinterpret_cast<vf*>(total + o + k0) = t;
            }
            if (counts) {
                vi q = *reinterpret_cast<const vi*>(counts + o + k0);
#pragma unroll
                for (int j = 0; j < VW; ++j) set_ilane(q, j, ilane_of(q, j) + (k0 + j == c ? 1 : 0));
                *reinterpret_cast<vi*>(counts + o + k0) = q;
            }
        }
        // a one-hot pass has zero entropy: ent_sum is left as it is
    } else {
        const float* src = probs + b * stride + p * K;
        double h = 0.0;
        for (int k0 = 0; k0 < K; k0 += VW) {
            const vf v = *reinterpret_cast<const vf*>(src + k0);
            if (total) {
                vf t = *reinterpret_cast<const vf*>(total + o + k0);
#pragma unroll
                for (int j = 0; j < VW; ++j) set_lane(t, j, __fadd_rn(lane_of(t, j), __fmul_rn(lane_of(v, j), w)));
                *reinterpret_cast<vf*>(total + o + k0) = t;
            }
            if (ent_sum) {
#pragma unroll
                for (int j = 0; j < VW; ++j) h += neg_plogp((double)lane_of(v, j));
            }
        }
        if (ent_sum) ent_sum[n] = __fadd_rn(ent_sum[n], (float)h);
    }
}

// running state of one pixel's finish: argmax (first index wins a tie, like torch.argmax) and the entropy of the mean
struct PixelFinish {
    int bi = 0;
    float bestf = 0.f;
    int32_t besti = 0;
    double h = 0.0;
};

// class k of a pixel whose mean is counts / S
__device__ __forceinline__ void finish_count(PixelFinish& f, int k, int32_t c, int S, size_t o, int32_t* counts_out, float* mean) {
    if (counts_out) counts_out[o + k] = c;
    if (mean) mean[o + k] = (float)c / (float)S;
    if (k == 0 || c > f.besti) { f.besti = c; f.bi = k; }
    f.h += neg_plogp((double)c / (double)S);
}

__device__ __forceinline__ void finish_pixel(const PixelFinish& f, int64_t n, int S, const float* ent_sum, uint8_t* vote, float* entropy, float* mi) {
    if (vote) vote[n] = (uint8_t)f.bi;
    if (entropy) entropy[n] = (float)f.h;
    if (mi) {
        // I = H(mean) - (1/S) sum_s H(p_s) >= 0 (Jensen); the clamp only removes rounding below zero
        const double m = f.h - (ent_sum ? (double)ent_sum[n] / (double)S : 0.0);
        mi[n] = (float)(m > 0.0 ? m : 0.0);
    }
}

template <int VW>
__global__ __launch_bounds__(256) void k_vote_finalize(const float* __restrict__ total, const int32_t* __restrict__ counts,
                                                       const float* __restrict__ ent_sum, int64_t npix, int K, int S,
                                                       float* __restrict__ mean, uint8_t* __restrict__ vote,
                                                       float* __restrict__ entropy, float* __restrict__ mi) {
    typedef typename VecF<VW>::T vf;
    typedef typename VecI<VW>::T vi;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= npix) return;
    const size_t o = (size_t)n * K;
    PixelFinish f;
    if (counts) {
        for (int k0 = 0; k0 < K; k0 += VW) {
            const vi q = *reinterpret_cast<const vi*>(counts + o + k0);
            if (mean) {
                vf m;
#pragma unroll
                for (int j = 0; j < VW; ++j) set_lane(m, j, (float)ilane_of(q, j) / (float)S);
                *reinterpret_cast<vf*>(mean + o + k0) = m;
            }
#pragma unroll
            for (int j = 0; j < VW; ++j) finish_count(f, k0 + j, ilane_of(q, j), S, o, nullptr, nullptr);
        }
    } else {
        for (int k0 = 0; k0 < K; k0 += VW) {
            const vf t = *reinterpret_cast<const vf*>(total + o + k0);
#pragma unroll
            for (int j = 0; j < VW; ++j) {
                const float v = lane_of(t, j);
                if (k0 + j == 0 || v > f.bestf) { f.bestf = v; f.bi = k0 + j; }
                f.h += neg_plogp((double)v);
            }
        }
    }
    finish_pixel(f, n, S, ent_sum, vote, entropy, mi);
}

// K <= KP: the pixel's counts in registers (compare-and-add against every class, no runtime-indexed array)
template <int KP>
__global__ __launch_bounds__(256) void k_vote_reduce_stack(const uint8_t* __restrict__ stack, int64_t npix, int S, int HW, int K,
                                                           int32_t* __restrict__ counts, float* __restrict__ mean,
                                                           uint8_t* __restrict__ vote, float* __restrict__ entropy) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= npix) return;
    const int64_t b = n / HW, p = n - b * HW;
    const uint8_t* src = stack + (size_t)b * S * HW + p;
    int32_t cnt[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = 0;
    for (int s = 0; s < S; ++s) {
        const int c = src[(size_t)s * HW];
#pragma unroll
        for (int k = 0; k < KP; ++k) cnt[k] += c == k ? 1 : 0;
    }
    const size_t o = (size_t)n * K;
    PixelFinish f;
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if (k < K) finish_count(f, k, cnt[k], S, o, counts, mean);
    finish_pixel(f, n, S, nullptr, vote, entropy, nullptr);
}

// K > 32: one LDS column of counts per thread (64-thread blocks: 255 x 64 x 4 B = 63.75 KiB; lane l reads bank l % 32, no conflict)
constexpr int VOTE_LDS_THREADS = 64;

__global__ __launch_bounds__(VOTE_LDS_THREADS) void k_vote_reduce_stack_lds(const uint8_t* __restrict__ stack, int64_t npix, int S, int HW, int K,
                                                                            int32_t* __restrict__ counts, float* __restrict__ mean,
                                                                            uint8_t* __restrict__ vote, float* __restrict__ entropy) {
    __shared__ int32_t cnt[CCDM_MAX_CLASSES][VOTE_LDS_THREADS];
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= npix) return;                   // (no barrier below: every thread touches its own column only)
    const int tid = threadIdx.x;
    for (int k = 0; k < K; ++k) cnt[k][tid] = 0;
    const int64_t b = n / HW, p = n - b * HW;
    const uint8_t* src = stack + (size_t)b * S * HW + p;
    for (int s = 0; s < S; ++s) {
        const int c = src[(size_t)s * HW];
        if (c < K) cnt[c][tid] += 1;        // a byte >= K (not a class) is counted nowhere, never out of bounds
    }
    const size_t o = (size_t)n * K;
    PixelFinish f;
    for (int k = 0; k < K; ++k) finish_count(f, k, cnt[k][tid], S, o, counts, mean);
    finish_pixel(f, n, S, nullptr, vote, entropy, nullptr);
}

// widest vector access (4, 2 or 1 elements) that K, the element stride and the pointers allow
static int vote_vec_width(int K, int64_t stride, std::initializer_list<const void*> ptrs) {
    for (int vw : {4, 2}) {
        if (K % vw != 0 || stride % vw != 0) continue;
        bool ok = true;
        for (const void* q : ptrs) ok = ok && ((uintptr_t)q % (vw * 4) == 0);
        if (ok) return vw;
    }
    return 1;
}

}  // namespace ccdm

extern "C" int ccdm_vote_accumulate(const uint8_t* cls, const float* probs, int64_t src_stride, int B, int HW, int K, float w,
                                    float* total, int32_t* counts, float* ent_sum, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE((cls == nullptr) != (probs == nullptr), "vote_accumulate: exactly one of cls / probs");
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "vote_accumulate: K=%d outside [1,%d]", K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE(B >= 0 && HW >= 0 && src_stride >= 0, "vote_accumulate: negative size");
    CCDM_REQUIRE(!probs || !counts, "vote_accumulate: counts need a class-map input");
    CCDM_REQUIRE(total || counts || (probs && ent_sum), "vote_accumulate: no accumulator");
    const int64_t npix = (int64_t)B * HW;
    if (npix == 0) return 0;
    const int64_t stride = src_stride ? src_stride : (cls ? (int64_t)HW : (int64_t)HW * K);
    const int64_t blocks = (npix + 255) / 256;
    CCDM_REQUIRE(blocks <= 0x7fffffff, "vote_accumulate: %lld pixels", (long long)npix);
    hipStream_t s = (hipStream_t)stream;
    // vector width: the class-map path only touches the accumulators; the probability path also the source rows (K-aligned + stride)
    const int vw = cls ? vote_vec_width(K, 0, {total, counts}) : vote_vec_width(K, stride, {probs, total});
    if (vw == 4) hipLaunchKernelGGL(k_vote_accumulate<4>, dim3((unsigned)blocks), dim3(256), 0, s, cls, probs, stride, npix, HW, K, w, total, counts, ent_sum);
    else if (vw == 2) hipLaunchKernelGGL(k_vote_accumulate<2>, dim3((unsigned)blocks), dim3(256), 0, s, cls, probs, stride, npix, HW, K, w, total, counts, ent_sum);
    else hipLaunchKernelGGL(k_vote_accumulate<1>, dim3((unsigned)blocks), dim3(256), 0, s, cls, probs, stride, npix, HW, K, w, total, counts, ent_sum);
    CCDM_CHECK_LAUNCH("vote_accumulate");
    return 0;
}

extern "C" int ccdm_vote_finalize(const float* total, const int32_t* counts, const float* ent_sum, int B, int HW, int K, int S,
                                  float* mean, uint8_t* vote, float* entropy, float* mutual_info, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(total || counts, "vote_finalize: no accumulator");
    CCDM_REQUIRE(!mean || counts, "vote_finalize: mean is written from counts (the fp32 total is the mean already)");
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "vote_finalize: K=%d outside [1,%d]", K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE(S >= 1, "vote_finalize: S=%d", S);
    CCDM_REQUIRE(B >= 0 && HW >= 0, "vote_finalize: negative size");
    const int64_t npix = (int64_t)B * HW;
    if (npix == 0) return 0;
    const int64_t blocks = (npix + 255) / 256;
    CCDM_REQUIRE(blocks <= 0x7fffffff, "vote_finalize: %lld pixels", (long long)npix);
    hipStream_t s = (hipStream_t)stream;
    const int vw = counts ? vote_vec_width(K, 0, {counts, mean}) : vote_vec_width(K, 0, {total});
    if (vw == 4) hipLaunchKernelGGL(k_vote_finalize<4>, dim3((unsigned)blocks), dim3(256), 0, s, total, counts, ent_sum, npix, K, S, mean, vote, entropy, mutual_info);
    else if (vw == 2) hipLaunchKernelGGL(k_vote_finalize<2>, dim3((unsigned)blocks), dim3(256), 0, s, total, counts, ent_sum, npix, K, S, mean, vote, entropy, mutual_info);
    else hipLaunchKernelGGL(k_vote_finalize<1>, dim3((unsigned)blocks), dim3(256), 0, s, total, counts, ent_sum, npix, K, S, mean, vote, entropy, mutual_info);
    CCDM_CHECK_LAUNCH("vote_finalize");
    return 0;
}

extern "C" int ccdm_vote_reduce_stack(const uint8_t* stack, int B, int S, int HW, int K, int32_t* counts, float* mean, uint8_t* vote,
                                      float* entropy, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(stack, "vote_reduce_stack: null stack");
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "vote_reduce_stack: K=%d outside [1,%d]", K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE(S >= 1, "vote_reduce_stack: S=%d", S);
    CCDM_REQUIRE(B >= 0 && HW >= 0, "vote_reduce_stack: negative size");
    const int64_t npix = (int64_t)B * HW;
    if (npix == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (K <= 32) {
        const int64_t blocks = (npix + 255) / 256;
        CCDM_REQUIRE(blocks <= 0x7fffffff, "vote_reduce_stack: %lld pixels", (long long)npix);
        const dim3 g((unsigned)blocks), t(256);
        if (K <= 2) hipLaunchKernelGGL(k_vote_reduce_stack<2>, g, t, 0, s, stack, npix, S, HW, K, counts, mean, vote, entropy);
        else if (K <= 8) hipLaunchKernelGGL(k_vote_reduce_stack<8>, g, t, 0, s, stack, npix, S, HW, K, counts, mean, vote, entropy);
        else hipLaunchKernelGGL(k_vote_reduce_stack<32>, g, t, 0, s, stack, npix, S, HW, K, counts, mean, vote, entropy);
    } else {
        const int64_t blocks = (npix + VOTE_LDS_THREADS - 1) / VOTE_LDS_THREADS;
        CCDM_REQUIRE(blocks <= 0x7fffffff, "vote_reduce_stack: %lld pixels", (long long)npix);
        hipLaunchKernelGGL(k_vote_reduce_stack_lds, dim3((unsigned)blocks), dim3(VOTE_LDS_THREADS), 0, s, stack, npix, S, HW, K, counts, mean, vote, entropy);
    }
    CCDM_CHECK_LAUNCH("vote_reduce_stack");
    return 0;
}
