// Cityscapes-style segmentation evaluation, device part: bilinear upsampling of the low-resolution prediction to the
// label resolution fused with the argmax and both confusion matrices the reference's Evaluator builds
// (evaluation/eval_cdm.py: `infer_step` F.interpolate + channel drop, ignite's ConfusionMatrix, `update_cm`).
// The full-resolution probability tensor is never written: each output pixel is interpolated in registers, classified
// and folded into the matrices straight away.
// The walk over the output pixels (tiles, source coordinates, interpolated row pair) is ccdm_seg_common.h's, shared with the
// export, script-score and calibration kernels, which must write, count and bin the class this kernel counts.
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

// Adds every lane's partials to the wave's slice, lanes grouped by the target they belong to (mine >= C: nothing), one fixed-order
// wave sum per (group, channel); then clears them.
template <int KP>
__device__ __forceinline__ void seg_flush(float (&acc)[KP], double* __restrict__ slice, int mine, int C, int lane) {
    seg_for_each_group(mine < C, mine, [&](int g, bool in_g) {
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (c < C) {
                const float s = seg_wave_sum(in_g ? acc[c] : 0.0f);
                if (lane == 0) slice[g * C + c] += (double)s;
            }
        }
    });
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
}

template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_seg_confusion(SegSrc s, const uint8_t* __restrict__ labels, double* __restrict__ slab_soft,
                                                       int32_t* __restrict__ slab_hard) {
    extern __shared__ double seg_lds[];
    const int C = s.C, CC = C * C;
    double* slices = seg_lds;                                            // [SEG_WAVES][CC], target-major: [t * C + c]
    int* hard = reinterpret_cast<int*>(seg_lds + SEG_WAVES * CC);         // [CC], [t * C + pred]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < SEG_WAVES * CC; e += blockDim.x) slices[e] = 0.0;
    for (int e = threadIdx.x; e < CC; e += blockDim.x) hard[e] = 0;
    __syncthreads();
    double* slice = slices + wave * CC;

    float acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
    int mine = 255, nacc = 0;            // the target class this lane's acc belongs to; steps added since the last flush

    for (SegTiles tiles(s.B, s.H, s.W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const SegLane<IDENT> ln(s, tile);
        SegLabels label(labels, s, tile);
        float A[KP], Bv[KP];
        int yA = -1, yB = -1;
        for (int y = tile.y_begin; y < tile.y_end; ++y) {
            float h0, h1;
            seg_step<KP, SRC, V4, IDENT>(A, Bv, yA, yB, h0, h1, s, ln, tile.b, y);
            const int t = label.next(y);
            const bool valid = label.counted(t, C);
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

}  // namespace ccdm

extern "C" size_t ccdm_seg_confusion_workspace_bytes(int B, int H, int W, int K) {
    using namespace ccdm;
    if (B <= 0 || H <= 0 || W <= 0 || K < 2 || K > SEG_MAX_K) return 0;
    const size_t CC = (size_t)(K - 1) * (K - 1);
    return (size_t)seg_blocks(B, H, W) * CC * (sizeof(double) + sizeof(int32_t));
}

extern "C" int ccdm_seg_confusion(const float* probs, int64_t pixel_stride, const uint8_t* cls, const uint8_t* labels, int B, int h,
                                  int w, int H, int W, int K, int64_t* hard, double* soft, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_src("seg_confusion", probs, pixel_stride, cls, h, w, K)) return rc;
    if (const int rc = seg_check_out("seg_confusion", B, H, W)) return rc;
    CCDM_REQUIRE(labels && hard && soft, "seg_confusion: null pointer");
    if (const int rc = seg_check_block_counts("seg_confusion", B, H, W)) return rc;
    const size_t need = B > 0 ? ccdm_seg_confusion_workspace_bytes(B, H, W, K) : 0;
    CCDM_REQUIRE((workspace || need == 0) && workspace_bytes >= need, "seg_confusion: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int C = K - 1, CC = C * C;
    const int grid = B > 0 ? seg_blocks(B, H, W) : 0;
    double* slab_soft = static_cast<double*>(workspace);
    int32_t* slab_hard = reinterpret_cast<int32_t*>(slab_soft + (size_t)grid * CC);
    hipStream_t st = (hipStream_t)stream;
    if (grid > 0) {
        const SegSrc s = seg_src(probs, pixel_stride, cls, B, h, w, H, W, C);
        const size_t lds = (size_t)SEG_WAVES * CC * sizeof(double) + (size_t)CC * sizeof(int);
        seg_dispatch(s, [&](auto kp, auto src, auto v4, auto ident) {
            hipLaunchKernelGGL((k_seg_confusion<kp(), src(), v4(), ident()>), dim3(grid), dim3(256), lds, st, s, labels, slab_soft, slab_hard);
        });
        CCDM_CHECK_LAUNCH("seg_confusion");
    }
    hipLaunchKernelGGL(k_seg_reduce, dim3(cdiv(CC, 64)), dim3(256), 0, st, slab_soft, slab_hard, grid, C, hard, soft);
    CCDM_CHECK_LAUNCH("seg_confusion reduce");
    return 0;
}
