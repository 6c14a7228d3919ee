// Calibration scores of a segmentation prediction, device part: the walk of ccdm_seg_common.h ending in calibration counts instead
// of confusion matrices.  Nothing in the reference computes these; the definition below is the contract,
// tests/test_seg_calibration.py restates it in float64.
//
// Definition.  For every output pixel of [B,H,W] whose label t < C (C = K - 1, the ignore channel dropped: the pixels
// ccdm_seg_confusion counts):
//   v_c, c < C   the bilinear sample of ccdm_seg_confusion (seg_step / seg_value); (H,W) == (h,w) reads the pixel;
//   pred         seg_argmax_step over v_0 .. v_{C-1}: the class the confusion kernel counts and the export kernel writes;
//   s            v_0 + v_1 + ... + v_{C-1}, added in ascending order in fp32;  q_c = v_c / s (IEEE division).
//                s == 0 (all mass on the ignore channel): q_c = 1/C for every c (pred is 0 there);
//   conf         q_pred;  correct = (pred == t);  bin = min((int)(conf * M), M - 1) in fp32, M bins;
//   nll          -log(max((double)q_t, 1e-12)) in fp64;   brier = sum over c of (q_c - [c == t])^2, ascending in fp32.
// Outputs: bins[pred][bin] = {pixels, correct pixels} (int64, accumulated), conf_sum[pred][bin] = sum of conf (fp64, overwritten),
// sums = {sum nll, sum brier, sum q_t} (fp64, overwritten).
//
// Determinism: no float atomics.
//   bins      one 64-bit LDS integer add per counted pixel (pixels in the low word, correct pixels in the high word: a block counts
//             fewer than 2^31 pixels), then one int64 global add per non-zero entry per block.  Exact in any order.
//   conf_sum  exact fixed point.  conf is a fp32 in [1/C, 1] with C <= 31, so it is a multiple of 2^-28: conf * 2^28 is an
//             integer below 2^28 + 1, summed with 64-bit integer adds (LDS per block, then global into the workspace, which is
//             cleared per call).  k_segcalib_finish converts the integer to fp64 (exact below 2^53, i.e. up to 2^25 pixels in one
//             (pred, bin) cell per call, rounded once beyond).  A confidence outside [0, 1] (an input that is no probability
//             map) is clamped for this sum and for the bin index.
//   sums      each lane adds its pixels' terms to three fp64 registers in walk order; at the end the block adds its 256 lanes'
//             triples by a pairwise tree into its row of a slab in the workspace, and k_segcalib_finish adds the slab rows in a fixed
//             order (rows strided over 256 threads, then a pairwise tree).  Same inputs and shapes => same grid => bit-identical sums.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int SEGC_MAX_BINS = 64;
constexpr float SEGC_FIX = 268435456.0f;          // 2^28
constexpr double SEGC_UNFIX = 1.0 / 268435456.0;

// SRC: 0 fp32 probabilities, 1 class map.  IDENT: (H, W) == (h, w), the value is the source pixel itself.
// fix: uint64 [C*M] fixed-point confidence sums (cleared by the host); slab: fp64 [gridDim.x][3].
template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_seg_calib(SegSrc s, const uint8_t* __restrict__ labels, int M, unsigned long long* __restrict__ bins,
                                                   unsigned long long* __restrict__ fix, double* __restrict__ slab) {
    extern __shared__ unsigned long long segc_lds[];
    const int C = s.C, CM = C * M;
    unsigned long long* cnt = segc_lds;              // [CM]: pixels | correct pixels << 32
    unsigned long long* cf = segc_lds + CM;          // [CM]: sum of conf * 2^28
    for (int e = threadIdx.x; e < 2 * CM; e += blockDim.x) segc_lds[e] = 0;
    __syncthreads();

    const float uniform = 1.0f / (float)C, fM = (float)M;
    double s_nll = 0.0, s_brier = 0.0, s_qt = 0.0;

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
            if (!label.counted(t, C)) continue;

            // first pass over the first C channels: interpolate, argmax (ties to the lowest index, as torch.argmax), sum
            int pred = 0;
            float best = 0.0f, s = 0.0f;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                const float vc = seg_value<IDENT>(A[c], Bv[c], h0, h1);
                seg_argmax_step(c, C, vc, best, pred);
                s += c < C ? vc : 0.0f;
            }
            // second pass: q_c = v_c / s, the target's probability and the Brier sum (selects, no indexed registers)
            const bool zero = s == 0.0f;
            float qt = 0.0f, brier = 0.0f;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                if (c < C) {
                    const float qc = zero ? uniform : seg_value<IDENT>(A[c], Bv[c], h0, h1) / s;
                    const float d = qc - (c == t ? 1.0f : 0.0f);
                    qt = c == t ? qc : qt;
                    brier += d * d;
                }
            }
            const float conf = zero ? uniform : best / s;        // best is v_pred: the same division as q_pred above
            const float cc = fminf(fmaxf(conf, 0.0f), 1.0f);     // the identity on a probability map
            const int bin = min((int)(cc * fM), M - 1);
            const int e = pred * M + bin;
            atomicAdd(&cnt[e], 1ull | (unsigned long long)(pred == t) << 32);
            atomicAdd(&cf[e], (unsigned long long)(cc * SEGC_FIX));
            s_nll -= log(fmax((double)qt, 1e-12));
            s_brier += (double)brier;
            s_qt += (double)qt;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CM; e += blockDim.x) {
        const unsigned long long n = cnt[e], f = cf[e];
        if (n & 0xFFFFFFFFull) atomicAdd(&bins[2 * e], n & 0xFFFFFFFFull);
        if (n >> 32) atomicAdd(&bins[2 * e + 1], n >> 32);
        if (f) atomicAdd(&fix[e], f);
    }
    __syncthreads();
    // the block's three sums: a pairwise tree over the 256 lanes' triples (the LDS tables above are done with)
    double* tri = reinterpret_cast<double*>(segc_lds);      // [3][256]
    tri[threadIdx.x] = s_nll;
    tri[256 + threadIdx.x] = s_brier;
    tri[512 + threadIdx.x] = s_qt;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int k = 0; k < 3; ++k) tri[k * 256 + threadIdx.x] += tri[k * 256 + threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < 3) slab[(size_t)blockIdx.x * 3 + threadIdx.x] = tri[threadIdx.x * 256];
}

// conf_sum[e] = fix[e] * 2^-28; sums[j] = the slab's column j in a fixed order: thread i adds rows i, i + 256, ... (independent
// loads), then a pairwise tree over the 256 partials in LDS.
__global__ __launch_bounds__(256) void k_segcalib_finish(const unsigned long long* __restrict__ fix, const double* __restrict__ slab, int nblk,
                                                         int CM, double* __restrict__ conf_sum, double* __restrict__ sums) {
    __shared__ double part[3][256];
    for (int e = threadIdx.x; e < CM; e += blockDim.x) conf_sum[e] = (double)fix[e] * SEGC_UNFIX;
    double s[3] = {0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < nblk; j += 256)
        for (int k = 0; k < 3; ++k) s[k] += slab[(size_t)j * 3 + k];
    for (int k = 0; k < 3; ++k) part[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int k = 0; k < 3; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < 3) sums[threadIdx.x] = part[threadIdx.x][0];
}

}  // namespace ccdm

extern "C" size_t ccdm_segcalib_workspace_bytes(int B, int H, int W, int K, int M) {
    using namespace ccdm;
    if (B <= 0 || H <= 0 || W <= 0 || K < 2 || K > SEG_MAX_K || M < 2 || M > SEGC_MAX_BINS) return 0;
    return ((size_t)(K - 1) * M + (size_t)seg_blocks(B, H, W) * 3) * sizeof(double);
}

extern "C" int ccdm_segcalib(const float* probs, int64_t pixel_stride, const uint8_t* cls, const uint8_t* labels, int B, int h, int w,
                             int H, int W, int K, int M, int64_t* bins, double* conf_sum, double* sums, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    if (const int rc = seg_check_src("segcalib", probs, pixel_stride, cls, h, w, K)) return rc;
    if (const int rc = seg_check_out("segcalib", B, H, W)) return rc;
    CCDM_REQUIRE(labels && bins && conf_sum && sums, "segcalib: null pointer");
    CCDM_REQUIRE(M >= 2 && M <= SEGC_MAX_BINS, "segcalib: M=%d outside [2,%d]", M, SEGC_MAX_BINS);
    if (B == 0) return 0;
    if (const int rc = seg_check_block_counts("segcalib", B, H, W)) return rc;
    const size_t need = ccdm_segcalib_workspace_bytes(B, H, W, K, M);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "segcalib: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int CM = (K - 1) * M, grid = seg_blocks(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const SegSrc s = seg_src(probs, pixel_stride, cls, B, h, w, H, W, K - 1);
    unsigned long long* fix = static_cast<unsigned long long*>(workspace);
    double* slab = reinterpret_cast<double*>(fix + CM);
    CCDM_REQUIRE(hipMemsetAsync(fix, 0, (size_t)CM * sizeof(unsigned long long), st) == hipSuccess, "segcalib: clearing the workspace failed");
    // the two count tables, and room for the 256 lanes' triples that reuse them at the end
    const size_t lds = sizeof(double) * (size_t)(2 * CM > 3 * 256 ? 2 * CM : 3 * 256);
    seg_dispatch(s, [&](auto kp, auto src, auto v4, auto ident) {
        hipLaunchKernelGGL((k_seg_calib<kp(), src(), v4(), ident()>), dim3(grid), dim3(256), lds, st, s, labels, M,
                           reinterpret_cast<unsigned long long*>(bins), fix, slab);
    });
    CCDM_CHECK_LAUNCH("segcalib");
    hipLaunchKernelGGL(k_segcalib_finish, dim3(1), dim3(256), 0, st, fix, slab, grid, CM, conf_sum, sums);
    CCDM_CHECK_LAUNCH("segcalib finish");
    return 0;
}
