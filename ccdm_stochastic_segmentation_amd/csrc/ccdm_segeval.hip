// Cityscapes-style segmentation evaluation, device part: bilinear upsampling of the low-resolution prediction to the
// label resolution fused with the argmax and both confusion matrices the reference's Evaluator builds
// (evaluation/eval_cdm.py: `infer_step` F.interpolate + channel drop, ignite's ConfusionMatrix, `update_cm`).
// The full-resolution probability tensor is never written: each output pixel is interpolated in registers, classified
// and folded into the matrices straight away.
//
// Layout.  One block (4 waves) owns an output tile of 64 columns x 64 rows of one image; wave w walks 16 of its rows, one
// output column per lane.  Horizontal weights are per lane and fixed over the walk, vertical weights are wave-uniform.
// The two source rows a step reads are kept interpolated horizontally in registers (A = row iy0, B = row iy1): at scale
// s one source row pair serves s output rows, so upsampling reads each source pixel once per wave from L1/L2 and the
// probabilities cross HBM about once.  A fixed grid of at most SEG_MAX_BLOCKS blocks strides over the tiles.
//
// Determinism.  Hard counts are integers: one LDS atomic add per counted pixel, exact in any order.  Soft sums never use
// float atomics: each lane adds its probabilities in fp32 while its target class stays the same, at most SEG_FLUSH steps; the
// partials are then reduced across the wave per target in a fixed order (seg_wave_sum) and added in fp64 to the wave's own
// LDS slice (only that wave writes it).
// At the end the block sums its 4 slices in order into its row of the fp64 slab; k_seg_reduce sums the slab rows in a
// fixed order.  Same inputs and shapes => same grid => bit-identical matrices.
#include "ccdm_common.h"

namespace ccdm {

constexpr int SEG_TW = 64;              // output columns of a tile (one per lane)
constexpr int SEG_WAVES = 4;
constexpr int SEG_ROWS = 16;            // output rows per wave
constexpr int SEG_TH = SEG_WAVES * SEG_ROWS;
constexpr int SEG_MAX_BLOCKS = 1024;    // slab rows
constexpr int SEG_FLUSH = 4;            // fp32 steps per lane before the wave partial goes to fp64 (<= 256 pixels)

static inline int seg_blocks(int B, int H, int W) {
    const long long tiles = (long long)B * cdiv(H, SEG_TH) * cdiv(W, SEG_TW);
    return (int)(tiles < SEG_MAX_BLOCKS ? tiles : SEG_MAX_BLOCKS);
}

// Sum over the 64 lanes in a fixed order: DPP within each row of 16 lanes (quad swaps, half-row and row mirrors leave the row
// sum in every lane of the row), then the four row sums as (r0 + r1) + (r2 + r3).  Every lane returns the same value.
template <int CTRL>
__device__ __forceinline__ float seg_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float seg_wave_sum(float x) {
    x += seg_dpp<0xB1>(x);       // quad_perm [1,0,3,2]
    x += seg_dpp<0x4E>(x);       // quad_perm [2,3,0,1]
    x += seg_dpp<0x141>(x);      // row_half_mirror
    x += seg_dpp<0x140>(x);      // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 48));
    return (r0 + r1) + (r2 + r3);
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

// Adds every lane's partials to the wave's slice, lanes grouped by the target they belong to (mine >= C: nothing), one fixed-order
// wave sum per (group, channel); then clears them.
template <int KP>
__device__ __forceinline__ void seg_flush(float (&acc)[KP], double* __restrict__ slice, int mine, int C, int lane) {
    unsigned long long rest = __ballot(mine < C);
    while (rest) {
        const int g = __builtin_amdgcn_readlane(mine, __ffsll((long long)rest) - 1);
        const bool in_g = mine == g;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (c < C) {
                const float s = seg_wave_sum(in_g ? acc[c] : 0.0f);
                if (lane == 0) slice[g * C + c] += (double)s;
            }
        }
        rest &= ~__ballot(in_g);
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
}

// SRC: 0 fp32 probabilities, 1 class map.  IDENT: (H, W) == (h, w), the value is the source pixel itself.
template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_seg_confusion(const float* __restrict__ probs, long long ps, const uint8_t* __restrict__ cls,
                                                       const uint8_t* __restrict__ labels, int B, int h, int w, int H, int W,
                                                       int C, float sh, float sw, double* __restrict__ slab_soft,
                                                       int32_t* __restrict__ slab_hard) {
    extern __shared__ double seg_lds[];
    const int CC = C * C;
    double* slices = seg_lds;                                            // [SEG_WAVES][CC], target-major: [t * C + c]
    int* hard = reinterpret_cast<int*>(seg_lds + SEG_WAVES * CC);         // [CC], [t * C + pred]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < SEG_WAVES * CC; e += blockDim.x) slices[e] = 0.0;
    for (int e = threadIdx.x; e < CC; e += blockDim.x) hard[e] = 0;
    __syncthreads();
    double* slice = slices + wave * CC;

    const int tiles_x = (W + SEG_TW - 1) / SEG_TW, tiles_y = (H + SEG_TH - 1) / SEG_TH;
    const long long ntiles = (long long)B * tiles_x * tiles_y;
    float acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
    int mine = 255, nacc = 0;            // the target class this lane's acc belongs to; steps added since the last flush

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y), b = (int)(tile / ((long long)tiles_x * tiles_y));
        const int x = tx * SEG_TW + lane;
        const bool in_x = x < W;
        // ATen upsample_bilinear2d, align_corners=False: src = max(scale * (dst + 0.5) - 0.5, 0), in fp32
        int ix0 = 0, ix1 = 0;
        float lw0 = 1.0f, lw1 = 0.0f;
        if (IDENT) {
            ix0 = ix1 = in_x ? x : 0;
        } else if (in_x) {
            float s = sw * ((float)x + 0.5f) - 0.5f;
            s = s < 0.0f ? 0.0f : s;
            ix0 = min((int)s, w - 1);
            ix1 = ix0 + (ix0 < w - 1 ? 1 : 0);
            lw1 = s - (float)ix0;
            lw0 = 1.0f - lw1;
        }
        float A[KP], Bv[KP];
        int yA = -1, yB = -1;
        const int y_begin = ty * SEG_TH + wave * SEG_ROWS;
        const int y_end = min(y_begin + SEG_ROWS, H);
        int t_next = (in_x && y_begin < y_end) ? (int)labels[((size_t)b * H + y_begin) * W + x] : 255;
        for (int y = y_begin; y < y_end; ++y) {
            float h0 = 1.0f, h1 = 0.0f;
            if (IDENT) {
                // weights (1, 0) in both directions give x itself for finite x: read the pixel (what ATen's same-size path copies)
                seg_pixel<KP, SRC, V4>(A, probs, cls, ((size_t)b * h + y) * w + ix0, ps, C);
            } else {
                float s = sh * ((float)y + 0.5f) - 0.5f;
                s = s < 0.0f ? 0.0f : s;
                const int iy0 = min((int)s, h - 1);
                const int iy1 = iy0 + (iy0 < h - 1 ? 1 : 0);
                h1 = s - (float)iy0;
                h0 = 1.0f - h1;
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
            const int t = t_next;
            if (y + 1 < y_end && in_x) t_next = labels[((size_t)b * H + y + 1) * W + x];     // one step ahead
            const bool valid = in_x && t < C;            // ignite: (y >= 0) & (y < num_classes)
            const unsigned long long vmask = __ballot(valid);

            // soft sums: each lane adds its probabilities to acc while its target stays the same; a counted lane whose target
            // changes (or SEG_FLUSH steps) flushes the wave first
            if (__ballot(valid && t != mine)) {
                if (nacc) seg_flush<KP>(acc, slice, mine, C, lane);
                nacc = 0;
                mine = t;
            }

            // one pass over the first C channels: interpolate, argmax (ties to the lowest index, as torch.argmax), accumulate
            int pred = 0;
            float best = 0.0f;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                const float vc = IDENT ? A[c] : h0 * A[c] + h1 * Bv[c];
                if (c == 0 || (c < C && vc > best)) { best = vc; pred = c; }
                acc[c] += valid ? vc : 0.0f;      // channels >= C are never flushed
            }

            // hard counts: integer LDS adds, exact in any order
            if (valid) atomicAdd(&hard[t * C + pred], 1);

            if (vmask && ++nacc == SEG_FLUSH) {
                seg_flush<KP>(acc, slice, mine, C, lane);
                nacc = 0;
            }
        }
    }
    if (nacc) seg_flush<KP>(acc, slice, mine, C, lane);
    __syncthreads();
    for (int e = threadIdx.x; e < CC; e += blockDim.x) {
        double s = slices[e];
        for (int wv = 1; wv < SEG_WAVES; ++wv) s += slices[wv * CC + e];
        slab_soft[(size_t)blockIdx.x * CC + e] = s;
        slab_hard[(size_t)blockIdx.x * CC + e] = hard[e];
    }
}

// hard[t][p] += sum of the slab's counts; soft[p][t] = sum of the slab's fp64 sums, blocks in a fixed order.
__global__ __launch_bounds__(256) void k_seg_reduce(const double* __restrict__ slab_soft, const int32_t* __restrict__ slab_hard,
                                                    int nblk, int C, int64_t* __restrict__ hard, double* __restrict__ soft) {
    __shared__ double rs[SEG_WAVES][64];
    __shared__ long long rh[SEG_WAVES][64];
    const int CC = C * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    double s = 0.0;
    long long n = 0;
    if (e < CC) {
        for (int j = wave; j < nblk; j += SEG_WAVES) {
            s += slab_soft[(size_t)j * CC + e];
            n += slab_hard[(size_t)j * CC + e];
        }
    }
    rs[wave][lane] = s;
    rh[wave][lane] = n;
    __syncthreads();
    if (wave == 0 && e < CC) {
        for (int wv = 1; wv < SEG_WAVES; ++wv) { s += rs[wv][lane]; n += rh[wv][lane]; }
        const int t = e / C, p = e % C;
        hard[t * C + p] += n;
        soft[p * C + t] = s;
    }
}

template <int KP, int SRC, bool V4>
static void seg_launch(bool ident, int grid, size_t lds, hipStream_t st, const float* probs, long long ps, const uint8_t* cls,
                       const uint8_t* labels, int B, int h, int w, int H, int W, int C, float sh, float sw, double* ss, int32_t* sh32) {
    if (ident)
        hipLaunchKernelGGL((k_seg_confusion<KP, SRC, V4, true>), dim3(grid), dim3(256), lds, st, probs, ps, cls, labels, B, h, w, H, W,
                           C, sh, sw, ss, sh32);
    else
        hipLaunchKernelGGL((k_seg_confusion<KP, SRC, V4, false>), dim3(grid), dim3(256), lds, st, probs, ps, cls, labels, B, h, w, H, W,
                           C, sh, sw, ss, sh32);
}

template <int KP>
static void seg_dispatch(bool ident, int grid, size_t lds, hipStream_t st, const float* probs, long long ps, const uint8_t* cls,
                         const uint8_t* labels, int B, int h, int w, int H, int W, int C, float sh, float sw, double* ss, int32_t* sh32) {
    const bool v4 = probs && ps % 4 == 0 && (reinterpret_cast<uintptr_t>(probs) & 15) == 0;
    if (cls) seg_launch<KP, 1, false>(ident, grid, lds, st, probs, ps, cls, labels, B, h, w, H, W, C, sh, sw, ss, sh32);
    else if (v4) seg_launch<KP, 0, true>(ident, grid, lds, st, probs, ps, cls, labels, B, h, w, H, W, C, sh, sw, ss, sh32);
    else seg_launch<KP, 0, false>(ident, grid, lds, st, probs, ps, cls, labels, B, h, w, H, W, C, sh, sw, ss, sh32);
}

}  // namespace ccdm

extern "C" size_t ccdm_seg_confusion_workspace_bytes(int B, int H, int W, int K) {
    using namespace ccdm;
    if (B <= 0 || H <= 0 || W <= 0 || K < 2 || K > 32) return 0;
    const size_t CC = (size_t)(K - 1) * (K - 1);
    return (size_t)seg_blocks(B, H, W) * CC * (sizeof(double) + sizeof(int32_t));
}

extern "C" int ccdm_seg_confusion(const float* probs, int64_t pixel_stride, const uint8_t* cls, const uint8_t* labels, int B, int h,
                                  int w, int H, int W, int K, int64_t* hard, double* soft, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE((probs != nullptr) != (cls != nullptr), "seg_confusion: pass exactly one of probs and cls");
    CCDM_REQUIRE(labels && hard && soft, "seg_confusion: null pointer");
    CCDM_REQUIRE(K >= 2 && K <= 32, "seg_confusion: K=%d outside [2,32]", K);
    CCDM_REQUIRE(B >= 0 && h > 0 && w > 0 && H > 0 && W > 0, "seg_confusion: bad shape B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    CCDM_REQUIRE(!probs || pixel_stride >= K, "seg_confusion: pixel_stride=%lld < K=%d", (long long)pixel_stride, K);
    // per-block int32 counts: a block covers at most ceil(tiles / SEG_MAX_BLOCKS) tiles of SEG_TW x SEG_TH pixels
    const long long tiles = (long long)B * cdiv(H, SEG_TH) * cdiv(W, SEG_TW);
    CCDM_REQUIRE((tiles + SEG_MAX_BLOCKS - 1) / SEG_MAX_BLOCKS * SEG_TW * SEG_TH < (1LL << 31), "seg_confusion: too many pixels");
    const size_t need = B > 0 ? ccdm_seg_confusion_workspace_bytes(B, H, W, K) : 0;
    CCDM_REQUIRE((workspace || need == 0) && workspace_bytes >= need,"seg_confusion: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int C = K - 1, CC = C * C;
    const int grid = B > 0 ? seg_blocks(B, H, W) : 0;
    double* slab_soft = static_cast<double*>(workspace);
    int32_t* slab_hard = reinterpret_cast<int32_t*>(slab_soft + (size_t)grid * CC);
    hipStream_t st = (hipStream_t)stream;
    if (grid > 0) {
        const bool ident = H == h && W == w;
        const float sh = (float)h / (float)H, sw = (float)w / (float)W;     // ATen's area_pixel_compute_scale, no scale factor given
        const size_t lds = (size_t)SEG_WAVES * CC * sizeof(double) + (size_t)CC * sizeof(int);
        if (C <= 2) seg_dispatch<2>(ident, grid, lds, st, probs, pixel_stride, cls, labels, B, h, w, H, W, C, sh, sw, slab_soft, slab_hard);
        else if (C <= 8) seg_dispatch<8>(ident, grid, lds, st, probs, pixel_stride, cls, labels, B, h, w, H, W, C, sh, sw, slab_soft, slab_hard);
        else if (C <= 20) seg_dispatch<20>(ident, grid, lds, st, probs, pixel_stride, cls, labels, B, h, w, H, W, C, sh, sw, slab_soft, slab_hard);
        else seg_dispatch<32>(ident, grid, lds, st, probs, pixel_stride, cls, labels, B, h, w, H, W, C, sh, sw, slab_soft, slab_hard);
        CCDM_CHECK_LAUNCH("seg_confusion");
    }
    hipLaunchKernelGGL(k_seg_reduce, dim3(cdiv(CC, 64)), dim3(256), 0, st, slab_soft, slab_hard, grid, C, hard, soft);
    CCDM_CHECK_LAUNCH("seg_confusion reduce");
    return 0;
}
