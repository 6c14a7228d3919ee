// Cityscapes-style segmentation evaluation, device part: bilinear upsampling of the low-resolution prediction to the
// label resolution fused with the argmax and both confusion matrices the reference's Evaluator builds
// (evaluation/eval_cdm.py: `infer_step` F.interpolate + channel drop, ignite's ConfusionMatrix, `update_cm`).
// The full-resolution probability tensor is never written: each output pixel is interpolated in registers, classified
// and folded into the matrices straight away.
// The coordinates, the interpolated row pair and the argmax live in ccdm_seg_common.h, shared with the export kernel
// (ccdm_segexport.hip), which must write the class this kernel counts.
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
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int SEG_FLUSH = 4;            // fp32 steps per lane before the wave partial goes to fp64 (<= 256 pixels)

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
        int ix0, ix1;
        float lw0, lw1;
        seg_lane_coord<IDENT>(x, in_x, sw, w, ix0, ix1, lw0, lw1);
        float A[KP], Bv[KP];
        int yA = -1, yB = -1;
        const int y_begin = ty * SEG_TH + wave * SEG_ROWS;
        const int y_end = min(y_begin + SEG_ROWS, H);
        int t_next = (in_x && y_begin < y_end) ? (int)labels[((size_t)b * H + y_begin) * W + x] : 255;
        for (int y = y_begin; y < y_end; ++y) {
            float h0, h1;
            seg_step<KP, SRC, V4, IDENT>(A, Bv, yA, yB, h0, h1, probs, cls, b, y, h, w, sh, ix0, ix1, lw0, lw1, ps, C);
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
                const float vc = seg_value<IDENT>(A[c], Bv[c], h0, h1);
                seg_argmax_step(c, C, vc, best, pred);
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
