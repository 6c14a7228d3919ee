// Calibration scores of a segmentation prediction, device part: the walk of k_seg_confusion (ccdm_seg_common.h: the same tiles,
// source coordinates, interpolated row pair and argmax) ending in calibration counts instead of confusion matrices.  Nothing in
// the reference computes these; the definition below is the contract, tests/test_seg_calibration.py restates it in float64.
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
__global__ __launch_bounds__(256) void k_seg_calib(const float* __restrict__ probs, long long ps, const uint8_t* __restrict__ cls,
                                                   const uint8_t* __restrict__ labels, int B, int h, int w, int H, int W, int C, int M,
                                                   float sh, float sw, unsigned long long* __restrict__ bins,
                                                   unsigned long long* __restrict__ fix, double* __restrict__ slab) {
    extern __shared__ unsigned long long segc_lds[];
    const int CM = C * M;
    unsigned long long* cnt = segc_lds;              // [CM]: pixels | correct pixels << 32
    unsigned long long* cf = segc_lds + CM;          // [CM]: sum of conf * 2^28
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < 2 * CM; e += blockDim.x) segc_lds[e] = 0;
    __syncthreads();

    const int tiles_x = (W + SEG_TW - 1) / SEG_TW, tiles_y = (H + SEG_TH - 1) / SEG_TH;
    const long long ntiles = (long long)B * tiles_x * tiles_y;
    const float uniform = 1.0f / (float)C, fM = (float)M;
    double s_nll = 0.0, s_brier = 0.0, s_qt = 0.0;

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
            if (!(in_x && t < C)) continue;              // ignite: (y >= 0) & (y < num_classes)

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

struct SegcArgs {
    const float* probs; long long ps; const uint8_t* cls; const uint8_t* labels;
    int B, h, w, H, W, C, M;
    float sh, sw;
    unsigned long long *bins, *fix;
    double* slab;
};

template <int KP, int SRC, bool V4>
static void segc_launch(bool ident, int grid, size_t lds, hipStream_t st, const SegcArgs& a) {
    if (ident)
        hipLaunchKernelGGL((k_seg_calib<KP, SRC, V4, true>), dim3(grid), dim3(256), lds, st, a.probs, a.ps, a.cls, a.labels, a.B, a.h, a.w, a.H,
                           a.W, a.C, a.M, a.sh, a.sw, a.bins, a.fix, a.slab);
    else
        hipLaunchKernelGGL((k_seg_calib<KP, SRC, V4, false>), dim3(grid), dim3(256), lds, st, a.probs, a.ps, a.cls, a.labels, a.B, a.h, a.w, a.H,
                           a.W, a.C, a.M, a.sh, a.sw, a.bins, a.fix, a.slab);
}

template <int KP>
static void segc_dispatch(bool ident, int grid, size_t lds, hipStream_t st, const SegcArgs& a) {
    const bool v4 = a.probs && a.ps % 4 == 0 && (reinterpret_cast<uintptr_t>(a.probs) & 15) == 0;
    if (a.cls) segc_launch<KP, 1, false>(ident, grid, lds, st, a);
    else if (v4) segc_launch<KP, 0, true>(ident, grid, lds, st, a);
    else segc_launch<KP, 0, false>(ident, grid, lds, st, a);
}

}  // namespace ccdm

extern "C" size_t ccdm_segcalib_workspace_bytes(int B, int H, int W, int K, int M) {
    using namespace ccdm;
    if (B <= 0 || H <= 0 || W <= 0 || K < 2 || K > 32 || M < 2 || M > SEGC_MAX_BINS) return 0;
    return ((size_t)(K - 1) * M + (size_t)seg_blocks(B, H, W) * 3) * sizeof(double);
}

extern "C" int ccdm_segcalib(const float* probs, int64_t pixel_stride, const uint8_t* cls, const uint8_t* labels, int B, int h, int w,
                             int H, int W, int K, int M, int64_t* bins, double* conf_sum, double* sums, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE((probs != nullptr) != (cls != nullptr), "segcalib: pass exactly one of probs and cls");
    CCDM_REQUIRE(labels && bins && conf_sum && sums, "segcalib: null pointer");
    CCDM_REQUIRE(K >= 2 && K <= 32, "segcalib: K=%d outside [2,32]", K);
    CCDM_REQUIRE(M >= 2 && M <= SEGC_MAX_BINS, "segcalib: M=%d outside [2,%d]", M, SEGC_MAX_BINS);
    CCDM_REQUIRE(B >= 0 && h > 0 && w > 0 && H > 0 && W > 0, "segcalib: bad shape B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    CCDM_REQUIRE(!probs || pixel_stride >= K, "segcalib: pixel_stride=%lld < K=%d", (long long)pixel_stride, K);
    if (B == 0) return 0;
    // per-block 32-bit counts: a block covers at most ceil(tiles / SEG_MAX_BLOCKS) tiles of SEG_TW x SEG_TH pixels
    const long long tiles = (long long)B * cdiv(H, SEG_TH) * cdiv(W, SEG_TW);
    CCDM_REQUIRE((tiles + SEG_MAX_BLOCKS - 1) / SEG_MAX_BLOCKS * SEG_TW * SEG_TH < (1LL << 31), "segcalib: too many pixels");
    const size_t need = ccdm_segcalib_workspace_bytes(B, H, W, K, M);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "segcalib: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int C = K - 1, CM = C * M;
    const int grid = seg_blocks(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    SegcArgs a{probs, (long long)pixel_stride, cls, labels, B, h, w, H, W, C, M,
               (float)h / (float)H, (float)w / (float)W,      // ATen's area_pixel_compute_scale, no scale factor given
               reinterpret_cast<unsigned long long*>(bins), static_cast<unsigned long long*>(workspace), nullptr};
    a.slab = reinterpret_cast<double*>(a.fix + CM);
    CCDM_REQUIRE(hipMemsetAsync(a.fix, 0, (size_t)CM * sizeof(unsigned long long), st) == hipSuccess, "segcalib: clearing the workspace failed");
    const bool ident = H == h && W == w;
    // the two count tables, and room for the 256 lanes' triples that reuse them at the end
    const size_t lds = sizeof(double) * (size_t)(2 * CM > 3 * 256 ? 2 * CM : 3 * 256);
    // the ladder of ccdm_seg_confusion
    if (C <= 2) segc_dispatch<2>(ident, grid, lds, st, a);
    else if (C <= 8) segc_dispatch<8>(ident, grid, lds, st, a);
    else if (C <= 20) segc_dispatch<20>(ident, grid, lds, st, a);
    else segc_dispatch<32>(ident, grid, lds, st, a);
    CCDM_CHECK_LAUNCH("segcalib");
    hipLaunchKernelGGL(k_segcalib_finish, dim3(1), dim3(256), 0, st, a.fix, a.slab, grid, CM, conf_sum, sums);
    CCDM_CHECK_LAUNCH("segcalib finish");
    return 0;
}
