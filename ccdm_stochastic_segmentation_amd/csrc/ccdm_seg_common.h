// What the segmentation kernels share: the whole walk over the output pixels of [B,H,W], not only the arithmetic of one pixel.
//   device  SegSrc (the prediction, one kernel argument), SegTiles (the persistent tile loop: the only place that spells the tile
//           decomposition), SegLane / seg_step / seg_value / seg_argmax (the source coordinates and weights of ATen's
//           upsample_bilinear2d, align_corners=False, no scale factor; the horizontally interpolated source row pair; the
//           vertical blend; the argmax), SegLabels (the label byte read one row ahead and the rule for a counted pixel), and
//           the wave helpers (DPP, quad broadcast, fixed-order 64-lane sum, the loop over groups of lanes with equal key);
//   host    seg_check_src / seg_check_out / seg_check_block_counts (the argument checks), seg_src (the scales), seg_dispatch
//           (the V4 rule, the SRC and IDENT choice and the channel ladder).
// Users: ccdm_segeval.hip (k_seg_confusion), ccdm_segexport.hip (k_seg_export), ccdm_csscore.hip (k_csscore; k_csscore_ids takes
// the tiles only), ccdm_segcalib.hip (k_seg_calib).  Every one of them classifies a pixel through these and nothing else, so
// the class one counts is the class the others count, bin and write, bit for bit.  ccdm_segboundary.hip reads the class map the
// export kernel wrote; its row pass (k_segboundary_rows) takes the tiles and a wave helper.  ccdm_contourf.hip reads that class
// map too; both of its passes take the tiles, the match pass also the loop over groups of lanes with equal key.
#pragma once
#include <type_traits>

#include "ccdm_common.h"

namespace ccdm {

constexpr int SEG_TW = 64;              // output columns of a tile (one per lane)
constexpr int SEG_WAVES = 4;
constexpr int SEG_ROWS = 16;            // output rows per wave
constexpr int SEG_TH = SEG_WAVES * SEG_ROWS;
constexpr int SEG_MAX_BLOCKS = 1024;    // slab rows
constexpr int SEG_MAX_K = 32;           // channels of a prediction; sizes the per-class LDS tables of the kernels

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
// SRC 0: fp32 channels-last with pixel stride `ps` (V4: float4 loads, seg_dispatch's rule);
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
        // channels past C - 1 re-read the last real chunk (in bounds under V4: ps > C - 1 rounded up to whole float4); their values are never used
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

// The prediction: fp32 channels-last probabilities with pixel stride `ps` or a uint8 class map (exactly one is set), [B,h,w]
// sampled at [B,H,W], of which the first C channels are scored.  sh, sw: ATen's area_pixel_compute_scale (seg_src).
struct SegSrc {
    const float* probs;
    long long ps;
    const uint8_t* cls;
    int B, h, w, H, W, C;
    float sh, sw;
};

// The part of a tile one wave walks: rows y_begin <= y < y_end of image b, one output column x per lane (in_x: inside the image).
struct SegTile {
    int b, x, y_begin, y_end;
    bool in_x;
};

// The persistent tile loop: block i takes tiles i, i + gridDim.x, ... of the B * tiles_y * tiles_x tiles of SEG_TH x SEG_TW pixels.
struct SegTiles {
    int H, W, tiles_x, tiles_y;
    long long ntiles, tile;
    __device__ __forceinline__ SegTiles(int B, int H_, int W_)
        : H(H_), W(W_), tiles_x((W_ + SEG_TW - 1) / SEG_TW), tiles_y((H_ + SEG_TH - 1) / SEG_TH) {
        ntiles = (long long)B * tiles_x * tiles_y;
        tile = blockIdx.x;
    }
    __device__ __forceinline__ bool more() const { return tile < ntiles; }
    __device__ __forceinline__ void advance() { tile += gridDim.x; }
    __device__ __forceinline__ SegTile get() const {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y), b = (int)(tile / ((long long)tiles_x * tiles_y));
        const int x = tx * SEG_TW + (threadIdx.x & 63), y_begin = ty * SEG_TH + (threadIdx.x >> 6) * SEG_ROWS;
        return SegTile{b, x, y_begin, min(y_begin + SEG_ROWS, H), x < W};
    }
};

// Argmax step over the first C channels: the first strictly greater value wins, so ties go to the lowest index (torch.argmax).
// A kernel that needs the values too folds this into its own pass over the channels instead of calling seg_argmax.
__device__ __forceinline__ void seg_argmax_step(int c, int C, float vc, float& best, int& pred) {
    if (c == 0 || (c < C && vc > best)) { best = vc; pred = c; }
}

// The lane's source columns and horizontal weights, fixed over a wave's walk down a tile.
template <bool IDENT>
struct SegLane {
    int ix0, ix1;
    float lw0, lw1;
    __device__ __forceinline__ SegLane(const SegSrc& s, const SegTile& t) { seg_lane_coord<IDENT>(t.x, t.in_x, s.sw, s.w, ix0, ix1, lw0, lw1); }
};

// One step of the row walk to output row y of image b (wave-uniform): the vertical weights (h0, h1) and the two horizontally
// interpolated source rows A = row iy0, B = row iy1, re-read only when the pair moves (yA, yB: the rows they hold, -1 = none), so
// at scale s one row pair serves s output rows.  A kernel declares A, Bv, yA = yB = -1 per tile and h0, h1 per row as locals of
// its own: held in a struct they cost registers (up to 70 more in the 32-channel kernels).
// IDENT: weights (1, 0) in both directions give x itself for finite x: A is the pixel (what ATen's same-size path copies).
template <int KP, int SRC, bool V4, bool IDENT>
__device__ __forceinline__ void seg_step(float (&A)[KP], float (&Bv)[KP], int& yA, int& yB, float& h0, float& h1, const SegSrc& s,
                                         const SegLane<IDENT>& l, int b, int y) {
    h0 = 1.0f, h1 = 0.0f;
    if (IDENT) {
        seg_pixel<KP, SRC, V4>(A, s.probs, s.cls, ((size_t)b * s.h + y) * s.w + l.ix0, s.ps, s.C);
    } else {
        int iy0, iy1;
        seg_coord(s.sh, y, s.h, iy0, iy1, h0, h1);
        if (iy0 != yA) {
            if (iy0 == yB) {
#pragma unroll
                for (int c = 0; c < KP; ++c) A[c] = Bv[c];
            } else {
                seg_row<KP, SRC, V4>(A, s.probs, s.cls, ((size_t)b * s.h + iy0) * s.w, l.ix0, l.ix1, l.lw0, l.lw1, s.ps, s.C);
            }
            yA = iy0;
        }
        if (iy1 != yB) {
            if (iy1 == yA) {
#pragma unroll
                for (int c = 0; c < KP; ++c) Bv[c] = A[c];
            } else {
                seg_row<KP, SRC, V4>(Bv, s.probs, s.cls, ((size_t)b * s.h + iy1) * s.w, l.ix0, l.ix1, l.lw0, l.lw1, s.ps, s.C);
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

template <int KP, bool IDENT>
__device__ __forceinline__ int seg_argmax(const float (&A)[KP], const float (&Bv)[KP], float h0, float h1, int C) {
    int pred = 0;
    float best = 0.0f;
#pragma unroll
    for (int c = 0; c < KP; ++c) seg_argmax_step(c, C, seg_value<IDENT>(A[c], Bv[c], h0, h1), best, pred);
    return pred;
}

// The lane's label down a tile, read one row ahead of its use; 255 where there is none.
struct SegLabels {
    const uint8_t* labels;
    const SegTile& t;
    int H, W, t_next;
    __device__ __forceinline__ SegLabels(const uint8_t* labels_, const SegSrc& s, const SegTile& t_) : labels(labels_), t(t_), H(s.H), W(s.W) {
        t_next = (t.in_x && t.y_begin < t.y_end) ? (int)labels[((size_t)t.b * H + t.y_begin) * W + t.x] : 255;
    }
    // the label of row y; reads row y + 1
    __device__ __forceinline__ int next(int y) {
        const int label = t_next;
        if (y + 1 < t.y_end && t.in_x) t_next = labels[((size_t)t.b * H + y + 1) * W + t.x];
        return label;
    }
    // ignite: (y >= 0) & (y < num_classes)
    __device__ __forceinline__ bool counted(int label, int C) const { return t.in_x && label < C; }
};

// ---- wave helpers (all 64 lanes must be active)
template <int CTRL, typename T>
__device__ __forceinline__ T seg_dpp(T x) {
    static_assert(sizeof(T) == 4, "32-bit values");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
template <typename T>
__device__ __forceinline__ T seg_readlane(T x, int lane) {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}
// lane Q of the caller's quad, in every lane of the quad
template <int Q>
__device__ __forceinline__ uint32_t seg_quad(uint32_t x) {
    return seg_dpp<Q * 0x55>(x);
}
// lane `s` (wave-uniform, 0..3) of the caller's quad
__device__ __forceinline__ uint32_t seg_quad_sel(uint32_t x, int s) {
    const uint32_t a = seg_quad<0>(x), b = seg_quad<1>(x), c = seg_quad<2>(x), d = seg_quad<3>(x);
    return s == 0 ? a : s == 1 ? b : s == 2 ? c : d;
}
// Sum over the 64 lanes in a fixed order: DPP within each row of 16 lanes (quad swaps, half-row and row mirrors leave the row
// sum in every lane of the row), then the four row sums as (r0 + r1) + (r2 + r3).  Every lane returns the same value.
template <typename T>
__device__ __forceinline__ T seg_wave_sum(T x) {
    x += seg_dpp<0xB1>(x);       // quad_perm [1,0,3,2]
    x += seg_dpp<0x4E>(x);       // quad_perm [2,3,0,1]
    x += seg_dpp<0x141>(x);      // row_half_mirror
    x += seg_dpp<0x140>(x);      // row_mirror
    return (seg_readlane(x, 0) + seg_readlane(x, 16)) + (seg_readlane(x, 32) + seg_readlane(x, 48));
}
// Groups the lanes that have `flag` set by equal `key` and calls fn(key of the group, lane belongs to it) once per group, with
// all lanes active.  Wave-uniform call.
template <typename F>
__device__ __forceinline__ void seg_for_each_group(bool flag, int key, F&& fn) {
    unsigned long long rest = __ballot(flag);
    while (rest) {
        const int g = seg_readlane(key, __ffsll((long long)rest) - 1);
        const bool in_g = flag && key == g;
        fn(g, in_g);
        rest &= ~__ballot(in_g);
    }
}

// ---- host side
// The checks every entry point makes, under its own name; 0 when they hold.  On the prediction:
static inline int seg_check_src(const char* who, const float* probs, int64_t pixel_stride, const uint8_t* cls, int h, int w, int K) {
    CCDM_REQUIRE((probs != nullptr) != (cls != nullptr), "%s: pass exactly one of probs and cls", who);
    CCDM_REQUIRE(K >= 2 && K <= SEG_MAX_K, "%s: K=%d outside [2,%d]", who, K, SEG_MAX_K);
    CCDM_REQUIRE(h > 0 && w > 0, "%s: bad shape h=%d w=%d", who, h, w);
    CCDM_REQUIRE(!probs || pixel_stride >= K, "%s: pixel_stride=%lld < K=%d", who, (long long)pixel_stride, K);
    return 0;
}
// on the output shape:
static inline int seg_check_out(const char* who, int B, int H, int W) {
    CCDM_REQUIRE(B >= 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    return 0;
}

// A block keeps 32-bit counts: it covers at most ceil(tiles / SEG_MAX_BLOCKS) tiles of SEG_TW x SEG_TH pixels.
static inline int seg_check_block_counts(const char* who, int B, int H, int W) {
    const long long tiles = (long long)B * cdiv(H, SEG_TH) * cdiv(W, SEG_TW);
    CCDM_REQUIRE((tiles + SEG_MAX_BLOCKS - 1) / SEG_MAX_BLOCKS * SEG_TW * SEG_TH < (1LL << 31), "%s: too many pixels", who);
    return 0;
}

static inline SegSrc seg_src(const float* probs, int64_t pixel_stride, const uint8_t* cls, int B, int h, int w, int H, int W, int C) {
    // ATen's area_pixel_compute_scale, no scale factor given
    return SegSrc{probs, (long long)pixel_stride, cls, B, h, w, H, W, C, (float)h / (float)H, (float)w / (float)W};
}

// Calls launch(KP, SRC, V4, IDENT) with the template values of the kernel that reads `s`, as std::integral_constant objects:
// KP the channel ladder over the scored channels, SRC 1 for a class map, V4 (float4 loads) for probabilities whose pixels start
// at multiples of 16 bytes, IDENT for a prediction at the output size.
template <typename F>
static inline void seg_dispatch(const SegSrc& s, F&& launch) {
    const bool v4 = s.probs && s.ps % 4 == 0 && (reinterpret_cast<uintptr_t>(s.probs) & 15) == 0;
    const bool ident = s.H == s.h && s.W == s.w;
    auto with_kp = [&](auto kp) {
        auto with_src = [&](auto src, auto v4c) {
            if (ident) launch(kp, src, v4c, std::true_type{});
            else launch(kp, src, v4c, std::false_type{});
        };
        if (s.cls) with_src(std::integral_constant<int, 1>{}, std::false_type{});
        else if (v4) with_src(std::integral_constant<int, 0>{}, std::true_type{});
        else with_src(std::integral_constant<int, 0>{}, std::false_type{});
    };
    if (s.C <= 2) with_kp(std::integral_constant<int, 2>{});
    else if (s.C <= 8) with_kp(std::integral_constant<int, 8>{});
    else if (s.C <= 20) with_kp(std::integral_constant<int, 20>{});
    else with_kp(std::integral_constant<int, 32>{});
}

}  // namespace ccdm
