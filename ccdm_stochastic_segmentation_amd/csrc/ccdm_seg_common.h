// Device helpers the segmentation kernels share (ccdm_segeval.hip: k_seg_confusion, ccdm_segexport.hip: k_seg_export): the tile
// geometry, the source coordinates and weights of ATen's upsample_bilinear2d (align_corners=False, no scale factor), the
// horizontally interpolated source rows, the vertical blend and the argmax.  Both kernels classify a pixel through these and
// nothing else, so the class one of them counts is the class the other writes, bit for bit.
#pragma once
#include "ccdm_common.h"

namespace ccdm {

constexpr int SEG_TW = 64;              // output columns of a tile (one per lane)
constexpr int SEG_WAVES = 4;
constexpr int SEG_ROWS = 16;            // output rows per wave
constexpr int SEG_TH = SEG_WAVES * SEG_ROWS;
constexpr int SEG_MAX_BLOCKS = 1024;    // slab rows

static inline int seg_blocks(int B, int H, int W) {
    const long long tiles = (long long)B * cdiv(H, SEG_TH) * cdiv(W, SEG_TW);
    return (int)(tiles < SEG_MAX_BLOCKS ? tiles : SEG_MAX_BLOCKS);
}

// ATen's area_pixel_compute_source_index without a scale factor, clamped at 0, in fp32: src = max(scale * (dst + 0.5) - 0.5, 0),
// i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
__device__ __forceinline__ void seg_coord(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

// The lane's source columns and horizontal weights for output column x, fixed over a tile walk.  A lane past the right edge
// reads column 0 with weights (1, 0): in bounds, its values are never used.
template <bool IDENT>
__device__ __forceinline__ void seg_lane_coord(int x, bool in_x, float sw, int w, int& ix0, int& ix1, float& lw0, float& lw1) {
    ix0 = 0, ix1 = 0;
    lw0 = 1.0f, lw1 = 0.0f;
    if (IDENT) ix0 = ix1 = in_x ? x : 0;
    else if (in_x) seg_coord(sw, x, w, ix0, ix1, lw0, lw1);
}

// Source row `iy` interpolated horizontally: r[c] = w0 * x[iy, ix0, c] + w1 * x[iy, ix1, c], c < C.
// SRC 0: fp32 channels-last with pixel stride `ps` (V4: float4 loads, ps % 4 == 0 and 16-byte aligned);
// SRC 1: uint8 class map read as its one-hot, through the same expression on the exact 0 / 1 values.
template <int KP, int SRC, bool V4>
__device__ __forceinline__ void seg_row(float (&r)[KP], const float* __restrict__ probs, const uint8_t* __restrict__ cls,
                                        size_t row, int ix0, int ix1, float w0, float w1, long long ps, int C) {
    if constexpr (SRC == 1) {
        const int c0 = cls[row + ix0], c1 = cls[row + ix1];
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const float x0 = c0 == c ? 1.0f : 0.0f, x1 = c1 == c ? 1.0f : 0.0f;
            r[c] = w0 * x0 + w1 * x1;
        }
    } else if constexpr (V4) {
        // channels past C - 1 re-read the last real chunk (in bounds: ps % 4 == 0 and ps > C - 1); their values are never used
        const float4* p0 = reinterpret_cast<const float4*>(probs + (row + ix0) * ps);
        const float4* p1 = reinterpret_cast<const float4*>(probs + (row + ix1) * ps);
        const int qlast = (C - 1) >> 2;
#pragma unroll
        for (int q = 0; q < (KP + 3) / 4; ++q) {
            const float4 a = p0[min(q, qlast)], b = p1[min(q, qlast)];
            const float xa[4] = {a.x, a.y, a.z, a.w}, xb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < KP) r[4 * q + j] = w0 * xa[j] + w1 * xb[j];
        }
    } else {
        const float* p0 = probs + (row + ix0) * ps;
        const float* p1 = probs + (row + ix1) * ps;
#pragma unroll
        for (int c = 0; c < KP; ++c) r[c] = w0 * p0[min(c, C - 1)] + w1 * p1[min(c, C - 1)];
    }
}

template <int KP, int SRC, bool V4>
__device__ __forceinline__ void seg_pixel(float (&r)[KP], const float* __restrict__ probs, const uint8_t* __restrict__ cls,
                                          size_t pix, long long ps, int C) {
    if constexpr (SRC == 1) {
        const int c0 = cls[pix];
#pragma unroll
        for (int c = 0; c < KP; ++c) r[c] = c0 == c ? 1.0f : 0.0f;
    } else if constexpr (V4) {
        const float4* p = reinterpret_cast<const float4*>(probs + pix * ps);
        const int qlast = (C - 1) >> 2;
#pragma unroll
        for (int q = 0; q < (KP + 3) / 4; ++q) {
            const float4 a = p[min(q, qlast)];
            const float xa[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < KP) r[4 * q + j] = xa[j];
        }
    } else {
        const float* p = probs + pix * ps;
#pragma unroll
        for (int c = 0; c < KP; ++c) r[c] = p[min(c, C - 1)];
    }
}

// One step of the row walk to output row y (wave-uniform): the vertical weights (h0, h1) and the two horizontally interpolated
// source rows A = row iy0, B = row iy1, re-read only when the pair moves (yA, yB: the rows they hold, -1 = none).
// IDENT: weights (1, 0) in both directions give x itself for finite x: A is the pixel (what ATen's same-size path copies).
template <int KP, int SRC, bool V4, bool IDENT>
__device__ __forceinline__ void seg_step(float (&A)[KP], float (&Bv)[KP], int& yA, int& yB, float& h0, float& h1,
                                         const float* __restrict__ probs, const uint8_t* __restrict__ cls, int b, int y, int h, int w,
                                         float sh, int ix0, int ix1, float lw0, float lw1, long long ps, int C) {
    h0 = 1.0f, h1 = 0.0f;
    if (IDENT) {
        seg_pixel<KP, SRC, V4>(A, probs, cls, ((size_t)b * h + y) * w + ix0, ps, C);
    } else {
        int iy0, iy1;
        seg_coord(sh, y, h, iy0, iy1, h0, h1);
        if (iy0 != yA) {
            if (iy0 == yB) {
#pragma unroll
                for (int c = 0; c < KP; ++c) A[c] = Bv[c];
            } else {
                seg_row<KP, SRC, V4>(A, probs, cls, ((size_t)b * h + iy0) * w, ix0, ix1, lw0, lw1, ps, C);
            }
            yA = iy0;
        }
        if (iy1 != yB) {
            if (iy1 == yA) {
#pragma unroll
                for (int c = 0; c < KP; ++c) Bv[c] = A[c];
            } else {
                seg_row<KP, SRC, V4>(Bv, probs, cls, ((size_t)b * h + iy1) * w, ix0, ix1, lw0, lw1, ps, C);
            }
            yB = iy1;
        }
    }
}

// Channel c of the output pixel: h0 * A + h1 * B in this order (the pixel itself under IDENT).
template <bool IDENT>
__device__ __forceinline__ float seg_value(float a, float b, float h0, float h1) {
    return IDENT ? a : h0 * a + h1 * b;
}

// Argmax step over the first C channels: the first strictly greater value wins, so ties go to the lowest index (torch.argmax).
__device__ __forceinline__ void seg_argmax_step(int c, int C, float vc, float& best, int& pred) {
    if (c == 0 || (c < C && vc > best)) { best = vc; pred = c; }
}

template <int KP, bool IDENT>
__device__ __forceinline__ int seg_argmax(const float (&A)[KP], const float (&Bv)[KP], float h0, float h1, int C) {
    int pred = 0;
    float best = 0.0f;
#pragma unroll
    for (int c = 0; c < KP; ++c) seg_argmax_step(c, C, seg_value<IDENT>(A[c], Bv[c], h0, h1), best, pred);
    return pred;
}

}  // namespace ccdm
