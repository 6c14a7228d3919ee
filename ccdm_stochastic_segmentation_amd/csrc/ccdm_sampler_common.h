// The per-pixel arithmetic of the step epilogue — softmax_K -> categorical posterior -> clamp -> normalise -> Exp(1)-race argmax (or the
// last-step outputs) — shared by the stand-alone epilogue kernel (ccdm_sampler.hip), the head kernel that ends in it (ccdm_head.hip)
// and the guided steps (ccdm_guided.hip): ONE definition, so all produce the same bits from the same values.  See ccdm_sampler.hip
// for the arithmetic order.  Also here, once each: the two LDS passes of the staged kernels (stage_class_rows, store_onehot_rows), the
// per-thread one-hot store (write_onehot), the clamp of a known pixel (clamp_known_pixel), the K -> KP ladder of the launchers (dispatch_kp) and the argument checks the step entry
// points share (check_step_args).
#pragma once
#include "ccdm_common.h"

#include <type_traits>
#include <utility>

namespace ccdm {

struct Philox {
    static constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    __device__ static inline void run(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
            const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
            const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
            c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
            k0 += W0; k1 += W1;
        }
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    }
};

__device__ __forceinline__ float u32_to_exp1(uint32_t bits) {
    const float u = ((float)(bits >> 8) + 0.5f) * 5.9604644775390625e-08f;   // (0,1), 2^-24 grid
    return -logf(u);
}

// The Exp(1) race over a two-valued categorical: p_k = p_hit for k == own, p_miss otherwise; argmax_k p_k / E_k, first maximum wins,
// E_k from word k % 4 of the Philox block with fourth counter word `tag | k / 4`.  Shared by the clamp at the known pixels (own = the
// label, tag 0x80000000) and the renoise of a resampling jump (own = x_t, tag 0x40000000): ccdm_known.hip.
__device__ __forceinline__ int race_hit_miss(const int K, const int own, const float p_hit, const float p_miss, const uint32_t pix, const uint32_t smp,
                                             const uint32_t step_row, const uint32_t tag, const uint32_t k0, const uint32_t k1) {
    float best = -INFINITY;
    int x = 0;
    for (int kq = 0; kq * 4 < K; ++kq) {
        uint32_t w[4];
        Philox::run(pix, smp, step_row, tag | (uint32_t)kq, k0, k1, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kq * 4 + j;
            if (k < K) {
                const float qv = (k == own ? p_hit : p_miss) / u32_to_exp1(w[j]);
                if (qv > best) { best = qv; x = k; }
            }
        }
    }
    return x;
}

// the per-thread form of the one-hot store: the K one-hot channels of one pixel
__device__ __forceinline__ void write_onehot(float* const d, const int K, const int x) {
    for (int k = 0; k < K; ++k) d[k] = (k == x) ? 1.0f : 0.0f;
}

// The clamp of ONE known pixel (include/ccdm_hip.h, ccdm_known_labels_step): pixel i of the flat [N,HW] map whose label is y < K.
// CCDM_STEP_SAMPLE: the race on (p_hit, p_miss) under tag 0x80000000 (the epilogue's blocks have kq < 64); the last-step modes: the
// label itself, its one-hot into out_probs / out_onehot.  The class goes to xt[i], its one-hot to xin where given, and back to the
// caller.  ONE definition for the clamp's own kernel (ccdm_known.hip) and the queue's guided step (ccdm_guided.hip).
__device__ __forceinline__ int clamp_known_pixel(const int y, const size_t i, const int HW, const int K, const float p_hit, const float p_miss,
                                                 const int mode, const uint32_t step_row, const uint32_t k0, const uint32_t k1,
                                                 const uint32_t sample_offset, uint8_t* const xt, float* const xin, const int xin_stride,
                                                 float* const out_probs, int64_t* const out_onehot) {
    int x = y;
    if (mode == CCDM_STEP_SAMPLE) {
        const uint32_t pix = (uint32_t)(i % HW), smp = (uint32_t)(i / HW) + sample_offset;
        x = race_hit_miss(K, y, p_hit, p_miss, pix, smp, step_row, 0x80000000u, k0, k1);
    } else {
        if (out_probs) write_onehot(out_probs + i * K, K, x);
        if (out_onehot) for (int k = 0; k < K; ++k) out_onehot[i * K + k] = (k == x) ? 1 : 0;
    }
    xt[i] = (uint8_t)x;
    if (xin) write_onehot(xin + i * xin_stride, K, x);
    return x;
}

// per-run fields of the epilogue: from the device-resident block when there is one (uniform scalar loads), else the arguments themselves
__device__ __forceinline__ ccdm_post_args post_resolve_run(const ccdm_post_args& a_in) {
    ccdm_post_args a = a_in;
    if (a_in.run) {
        const ccdm_post_run r = *a_in.run;
        a.noise = r.noise; a.noise_step_stride = r.noise_step_stride; a.philox_seed = r.philox_seed; a.sample_offset = r.sample_offset;
        a.noise_row0 = r.noise_row0; a.out_probs = r.out_probs; a.out_onehot = r.out_onehot; a.posterior_out = r.posterior_out;
    }
    return a;
}

// pixel i (global index n * HW + pixel) with the head's K values x0[0..K) (logits, or probabilities if !a.softmax; x0[k >= K] = -inf);
// `a` already resolved by post_resolve_run, `step` = the table row of this denoise step
// (core: the step's coefficients and the pixel's x_t are handed in, so that a caller may fetch them ahead of time)
template <int KP>
__device__ __forceinline__ void posterior_pixel_core(const ccdm_post_args& a, const size_t i, float (&x0)[KP], const int step, const float al, const float cu,
                                                     const int mode, const int xt, int* const chosen = nullptr) {
    const int K = a.K;
    if (a.range_flag) {
        // a non-finite head value is how an F16X3 range overflow anywhere upstream surfaces (include/ccdm_hip.h): NaN/Inf
        // survive every conv, GroupNorm and attention on the way here.  (The clamp below would hide it: fmaxf(NaN, 1e-12) = 1e-12.)
        float chk = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) if (k < K) chk += fabsf(x0[k]);
        if (!(chk <= 3.0e38f)) *a.range_flag = 1;        // benign race: every writer stores the same value
    }
    if (a.softmax) {
        float mx = x0[0];
#pragma unroll
        for (int k = 1; k < KP; ++k) mx = fmaxf(mx, x0[k]);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            x0[k] = k < K ? expf(x0[k] - mx) : 0.f;
            if (k < K) sum += x0[k];
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) x0[k] = x0[k] / sum;
    }
    if (mode == CCDM_STEP_SOFTMAX_ONLY) {
        if (a.out_probs) {
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) a.out_probs[i * K + k] = x0[k];
        }
        return;
    }
    const float Kf = (float)K;
    const float u = (1.0f - al) / Kf, b = (1.0f - cu) / Kf;
    float A[KP];
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        A[k] = (k == xt ? al : 0.0f) + u;          // a*1 + u  /  a*0 + u
        if (k == 0) S = A[0]; else if (k < K) S = S + A[k];
    }
    float r[KP];
    float R = 0.f;
    const float bS = b * S;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        r[k] = k < K ? x0[k] / (cu * A[k] + bS) : 0.f;
        if (k == 0) R = r[0]; else if (k < K) R = R + r[k];
    }
    const float bR = b * R;
    float P[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        P[k] = A[k] * (cu * r[k] + bR);
        P[k] = fmaxf(P[k], 1e-12f);
    }
    // normalise, cascade order (== sequential for K <= 16)
    float tot;
    {
        float hi = 0.f, tail = 0.f;
        bool have_hi = false, have_tail = false;
        const int full = (K / 16) * 16;
#pragma unroll
        for (int s0 = 0; s0 < KP; s0 += 16) {
            if (s0 + 16 <= full) {
                float blk = P[s0];
#pragma unroll
                for (int k = 1; k < 16; ++k) if (s0 + k < KP) blk = blk + P[s0 + k];
                hi = have_hi ? hi + blk : blk;
                have_hi = true;
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k >= full && k < K) { tail = have_tail ? tail + P[k] : P[k]; have_tail = true; }
        }
        tot = have_tail ? (have_hi ? tail + hi : tail) : hi;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) P[k] = P[k] / tot;

    if (a.posterior_out) {
#pragma unroll
        for (int k = 0; k < KP; ++k) if (k < K) a.posterior_out[i * K + k] = P[k];
    }

    if (mode == CCDM_STEP_SAMPLE) {
        float best = -INFINITY;
        int bi = 0;
        if (a.noise) {
            const float* e = a.noise + (size_t)(step - a.noise_row0) * a.noise_step_stride + i * K;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (k < K) {
                    const float qv = P[k] / e[k];
                    if (qv > best) { best = qv; bi = k; }
                }
            }
        } else {
            const uint32_t pix = (uint32_t)(i % a.HW), smp = (uint32_t)(i / a.HW) + a.sample_offset;
            const uint32_t k0 = (uint32_t)a.philox_seed, k1 = (uint32_t)(a.philox_seed >> 32);
#pragma unroll
            for (int kq = 0; kq < (KP + 3) / 4; ++kq) {
                if (kq * 4 < K) {
                    uint32_t w[4];
                    Philox::run(pix, smp, (uint32_t)step, (uint32_t)kq, k0, k1, w);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = kq * 4 + j;
                        if (k < K && k < KP) {
                            const float qv = P[k] / u32_to_exp1(w[j]);
                            if (qv > best) { best = qv; bi = k; }
                        }
                    }
                }
            }
        }
        a.xt_next[i] = (uint8_t)bi;
        if (chosen) *chosen = bi;            // the caller writes the one-hot channels itself (k_posterior_staged)
        else if (a.xin) {
            float* d = a.xin + i * a.xin_stride;
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) d[k] = (k == bi) ? 1.0f : 0.0f;
        }
    } else if (mode == CCDM_STEP_LAST_CONFIDENCE) {
        if (a.out_probs) {
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) a.out_probs[i * K + k] = P[k];
        }
    } else if (mode == CCDM_STEP_LAST_MAJORITY) {
        float best = P[0];
        int bi = 0;
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K && P[k] > best) { best = P[k]; bi = k; }
        if (a.out_onehot) {
#pragma unroll
            for (int k = 0; k < KP; ++k) if (k < K) a.out_onehot[i * K + k] = (k == bi) ? 1 : 0;
        }
        a.xt_next[i] = (uint8_t)bi;
    }
    // CCDM_STEP_LAST_KEEP: x_t is returned unchanged (step_T_sample neither "majority" nor "confidence")
}

template <int KP>
__device__ __forceinline__ void posterior_pixel(const ccdm_post_args& a, const size_t i, float (&x0)[KP], const int step, int* const chosen = nullptr) {
    const float* row = a.step_table + (size_t)step * 4;
    const float al = row[0], cu = row[1];
    const int mode = (int)row[2];
    const int xt = mode == CCDM_STEP_SOFTMAX_ONLY ? 0 : (int)a.xt[i];
    posterior_pixel_core<KP>(a, i, x0, step, al, cu, mode, xt, chosen);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The staged kernels (k_posterior_staged, k_guided_staged): a block's BLK pixels move as what they are, one contiguous run of
// [pixel][class] floats in and [pixel][xin_stride] floats out: 16-byte requests in lane order, exchanged through LDS rows padded to an
// odd pitch (conflict-free per-thread reads), element by element where the run is not a whole number of aligned 16-byte pieces.

// idx / d for the flat index of a block's [pixel][channel] run: (idx * ceil(2^20 / d)) >> 20 where d <= 64 (idx < 256 * d: error
// < idx / 2^20 < 1 / d), a plain division above
// (MAXD: the caller's bound on d; where it is at most 64, the choice is made at compile time)
template <unsigned MAXD>
struct RowDiv {
    unsigned d, m;
    __device__ __forceinline__ explicit RowDiv(unsigned d_) : d(d_), m(MAXD <= 64u || d_ <= 64u ? ((1u << 20) + d_ - 1u) / d_ : 0u) {}
    __device__ __forceinline__ unsigned operator()(unsigned idx) const { return MAXD <= 64u || m ? (idx * m) >> 20 : idx / d; }
};

// stage-in: sx[p * PITCH + k] = src[p * row_len + k] (WEIGHTED: * wsrc[the same]) for the block's nvalid pixels, k < row_len <= PITCH
// (MAXLEN: the caller's bound on row_len, if it has one)
template <int BLK, int PITCH, bool WEIGHTED, unsigned MAXLEN = ~0u>
__device__ __forceinline__ void stage_class_rows(float* const sx, const float* const src, const float* const wsrc, const int nvalid,
                                                 const unsigned row_len, const int tid) {
    const RowDiv<MAXLEN> row(row_len);
    const int total = nvalid * (int)row_len;
    uintptr_t addr = reinterpret_cast<uintptr_t>(src);
    if constexpr (WEIGHTED) addr |= reinterpret_cast<uintptr_t>(wsrc);
    if ((total & 3) == 0 && (addr & 15) == 0) {
        for (int q = tid; q < total / 4; q += BLK) {
            f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
            if constexpr (WEIGHTED) {
                const f32x4 w = reinterpret_cast<const f32x4*>(wsrc)[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] * w[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned idx = 4u * (unsigned)q + (unsigned)e, p = row(idx), k = idx - p * row_len;
                sx[p * PITCH + k] = v[e];
            }
        }
    } else {
        for (int idx = tid; idx < total; idx += BLK) {
            const unsigned p = row((unsigned)idx), k = (unsigned)idx - p * row_len;
            if constexpr (WEIGHTED) sx[p * PITCH + k] = src[idx] * wsrc[idx];
            else sx[p * PITCH + k] = src[idx];
        }
    }
}

// write-out: channel c < K of pixel p gets c == sb[p] ? 1 : 0; the image channels (c >= K of each `stride`-float pixel) are not touched:
// a 16-byte piece that lies wholly inside one-hot channels is one store, a piece that straddles image channels goes element by element
// (MAXSTRIDE: the caller's bound on stride, if it has one)
template <int BLK, unsigned MAXSTRIDE = ~0u>
__device__ __forceinline__ void store_onehot_rows(float* const dst, const int* const sb, const int nvalid, const unsigned stride, const int K,
                                                  const int tid) {
    const RowDiv<MAXSTRIDE> row(stride);
    const int total = nvalid * (int)stride;
    if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        for (int q = tid; q < total / 4; q += BLK) {
            f32x4 v;
            bool all = true;
            bool oh[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned idx = 4u * (unsigned)q + (unsigned)e, p = row(idx), c = idx - p * stride;
                oh[e] = c < (unsigned)K;
                all = all && oh[e];
                v[e] = (int)c == sb[p] ? 1.0f : 0.0f;
            }
            if (all) reinterpret_cast<f32x4*>(dst)[q] = v;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (oh[e]) dst[4 * q + e] = v[e];
            }
        }
    } else {
        for (int idx = tid; idx < total; idx += BLK) {
            const unsigned p = row((unsigned)idx), c = (unsigned)idx - p * stride;
            if (c < (unsigned)K) dst[idx] = (int)c == sb[p] ? 1.0f : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Host side.  The ladder from K to the padded class count KP a kernel is instantiated for: f(std::integral_constant<int, KP>{}) for the
// first rung >= K, the rung MAX for everything above the one below it.  (The per-class work — four IEEE divisions, an exponential, a
// quarter Philox block — is predicated, not skipped, beyond K: Cityscapes' K = 20 on the 32-wide instantiation did 60 % more arithmetic
// than it needed, hence 20 and 24.)  The register kernels end at 32; the rungs above are the guided kernels'.
constexpr int KP_LADDER[] = {2, 4, 8, 16, 20, 24, 32, 64, 128, 256};

template <int MAX = 32, int I = 0, class F>
inline void dispatch_kp(const int K, F&& f) {
    constexpr int KP = KP_LADDER[I];
    if constexpr (KP >= MAX) f(std::integral_constant<int, KP>{});
    else if (K <= KP) f(std::integral_constant<int, KP>{});
    else dispatch_kp<MAX, I + 1>(K, std::forward<F>(f));
}

// What ccdm_known_labels_step, ccdm_renoise_step and the guided steps check alike (`name`: the entry's, as its errors carry it; `pointers`:
// the entry's required pointers are all there; `blk`: pixels per block of the launch).  0, or fail()'s code.
inline int check_step_args(const char* name, const bool pointers, const int N, const int HW, const int K, const float* xin, const int xin_stride,
                           const int mode, const int step_row, const int blk) {
    CCDM_REQUIRE(pointers, "%s: null pointer", name);
    CCDM_REQUIRE(N >= 1 && HW >= 1, "%s: bad shape N=%d HW=%d", name, N, HW);
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "%s: K=%d outside [1,%d]", name, K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE(!xin || xin_stride >= K, "%s: xin_stride %d < K %d", name, xin_stride, K);
    CCDM_REQUIRE(mode == CCDM_STEP_SAMPLE || mode == CCDM_STEP_LAST_CONFIDENCE || mode == CCDM_STEP_LAST_MAJORITY || mode == CCDM_STEP_LAST_KEEP,
                 "%s: mode %d", name, mode);
    CCDM_REQUIRE(step_row >= 0, "%s: step_row %d", name, step_row);
    CCDM_REQUIRE(((size_t)N * HW + blk - 1) / blk <= 0x7FFFFFFFull, "%s: too many pixels", name);
    return 0;
}

}  // namespace ccdm
