// The shaping of a pixel's x0 row before the reverse step — temper relative to the row's largest value, then cut to the smallest set of
// classes whose mass reaches top_r (THE definition: include/ccdm_hip.h, ccdm_shaped_step) — in its two forms, on registers and on an LDS
// row: ONE definition for the kernels that shape a row in front of posterior_pixel_core (ccdm_guided.hip).  The branches marked
// uniform are so where (inv_t, top_r) are launch arguments; the guided slots hand in each slot's own pair, and a wave that straddles
// two slots diverges there — nothing here crosses lanes.
#pragma once
#include "ccdm_common.h"

namespace ccdm {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// u^inv_t for u in (0,1): exp2f(inv_t * log2f(u)) (include/ccdm_hip.h names this choice)
__device__ __forceinline__ float temper_pow(const float u, const float inv_t) { return exp2f(inv_t * log2f(u)); }

__device__ __forceinline__ float temper_value(const float v, const float m, const float inv_t) {
    const float u = v / m;
    return u == 1.0f ? 1.0f : (u == 0.0f ? 0.0f : temper_pow(u, inv_t));
}

// The shaping of include/ccdm_hip.h on a pixel's K values in registers, q[k >= K] = 0 on entry and on exit.  KP <= 32.
template <int KP>
__device__ __forceinline__ void shape_row(float (&q)[KP], const int K, const float inv_t, const float top_r) {
    static_assert(KP <= 32, "the taken set is a 32-bit mask");
    if (inv_t != 1.0f) {                       // uniform
        float m = q[0];
#pragma unroll
        for (int k = 1; k < KP; ++k) m = fmaxf(m, q[k]);
        if (m != 0.0f) {
#pragma unroll
            for (int k = 0; k < KP; ++k) q[k] = temper_value(q[k], m, inv_t);
        }
    }
    if (top_r != 1.0f) {                       // uniform
        float Z = q[0];
#pragma unroll
        for (int k = 1; k < KP; ++k) if (k < K) Z = Z + q[k];
        const float theta = top_r * Z;
        uint32_t taken = 0u;
        float c = 0.0f;
        for (int j = 0; j < K && c < theta; ++j) {
            float best = -1.0f;
            uint32_t bit = 1u;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float cand = (taken >> k) & 1u ? -1.0f : q[k];
                if (cand > best) { best = cand; bit = 1u << k; }
            }
            taken |= bit;
            c = c + best;
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) q[k] = (taken >> k) & 1u ? q[k] : 0.0f;
    }
}

// The same on a pixel's LDS row (row[0 .. K), the thread's own), in place
__device__ __forceinline__ void shape_lds_row(float* const row, const int K, const float inv_t, const float top_r) {
    if (inv_t != 1.0f) {                       // uniform
        float m = row[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, row[k]);
        if (m != 0.0f)
            for (int k = 0; k < K; ++k) row[k] = temper_value(row[k], m, inv_t);
    }
    if (top_r != 1.0f) {                       // uniform
        float Z = row[0];
        for (int k = 1; k < K; ++k) Z = Z + row[k];
        const float theta = top_r * Z;
        float c = 0.0f;
        for (int j = 0; j < K && c < theta; ++j) {
            float best = -1.0f;
            int bk = 0;
            for (int k = 0; k < K; ++k) {
                const float v = row[k];
                if (!(__float_as_uint(v) >> 31) && v > best) { best = v; bk = k; }
            }
            if (best < 0.0f) break;            // nothing left that compares (a NaN row): the row is garbage either way
            row[bk] = __uint_as_float(__float_as_uint(best) | 0x80000000u);
            c = c + best;
        }
        for (int k = 0; k < K; ++k) {
            const uint32_t b = __float_as_uint(row[k]);
            row[k] = (b >> 31) ? __uint_as_float(b & 0x7FFFFFFFu) : 0.0f;
        }
    }
}

}  // namespace ccdm
