// LIDC lesion-level scores, device part (beyond the reference, whose LIDC scores are all overlap scores): per (image, sample, rater,
// class) the number of lesions (connected components) of either map and how many of them the other map's mask covers to each of T
// overlap thresholds.  The definition in include/ccdm_hip.h is the contract; tests/test_lidc_lesions.py restates it with numpy and
// holds it against scipy.ndimage.label.
//
// Label stage (k_lesions_label), once per (map, class), not per pair: one workgroup of 512 threads labels the mask by les_label of
// ccdm_lesions_common.h (union-find in LDS with the smaller index as the root; the steps, the invariant parent[p] <= p and why every
// loop ends are stated there), leaving int32 labels [H][W] in the workspace and the lesion count of the (map, class) behind the planes.
// LDS at the limit (H*W = 16384): 16384 parents + 256 chunk counts = 66,560 B: two workgroups per CU.
//
// Pair stage (k_lesions_pairs), one workgroup of 256 threads per cell (b, i, j, c).  A pixel has class c in a map iff its label there
// is not 0, so the two label planes are all the kernel reads.  Walk 1: per pixel one LDS atomicAdd per side into a table indexed by
// the dense label, size in the low and cov in the high 16 bits of one uint32 (both <= 16384: the low half cannot carry).  Walk 2: the
// lesions of each side against the T thresholds, cov*den >= num*size in 64 bits; counts per thread, fixed-order wave sums, the four
// waves added in order.  A conn-4 checkerboard has ceil(H*W/2) lesions per map, the most any mask can have (one pixel of each lesion
// is an independent set of the grid): 2 sides * 8192 * 4 B = 65,536 B of tables at the limit plus 256 B of wave sums: two workgroups
// per CU.  Integers only: exact in any order, two identical calls are bit-identical.
#include "ccdm_lesions_common.h"

namespace ccdm {

struct LesOverlaps {
    int T;
    int num[LES_MAX_T], den[LES_MAX_T];
};

template <int NPIX>
__global__ __launch_bounds__(LES_THREADS) void k_lesions_label(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters, long long nA,
                                                               int C, int c0, int H, int W, int conn8, int32_t* __restrict__ ws,
                                                               int32_t* __restrict__ counts) {
    extern __shared__ int les_lds[];
    const size_t mc = blockIdx.x;
    const long long m = (long long)(mc / C);
    const uint32_t c = (uint32_t)(c0 + (int)(mc % C));
    const size_t HW = (size_t)H * W;
    const uint8_t* map = m < nA ? samples + (size_t)m * HW : raters + (size_t)(m - nA) * HW;
    les_label<NPIX>(les_lds, map, c, H, W, conn8, ws + mc * HW, counts + mc);
}

__global__ __launch_bounds__(256) void k_lesions_pairs(const int32_t* __restrict__ ws, const int32_t* __restrict__ counts, int B, int S, int L, int C,
                                                       int HW, int nmax, LesOverlaps ov, int32_t* __restrict__ stats) {
    extern __shared__ unsigned les_tab[];                            // [2][nmax]: cov << 16 | size per lesion of the sample, of the rater
    __shared__ int wsum[4][2 * LES_MAX_T];
    const size_t cell = blockIdx.x;
    const int ci = (int)(cell % C), j = (int)(cell / C % L), i = (int)(cell / ((size_t)C * L) % S), b = (int)(cell / ((size_t)C * L * S));
    const size_t pa = ((size_t)b * S + i) * C + ci, pr = ((size_t)B * S + (size_t)b * L + j) * C + ci;
    const int32_t* la = ws + pa * HW;
    const int32_t* lr = ws + pr * HW;
    const int n_a = counts[pa], n_r = counts[pr];                    // <= nmax
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* ta = les_tab;
    unsigned* tr = les_tab + nmax;
    int32_t* st = stats + cell * (2 + 2 * ov.T);
    if (threadIdx.x == 0) { st[0] = n_a; st[1] = n_r; }
    if (n_a == 0 || n_r == 0) {                                      // block-uniform: nothing covers anything
        if (threadIdx.x < 2 * ov.T) st[2 + threadIdx.x] = 0;
        return;
    }
    for (int l = threadIdx.x; l < n_a; l += 256) ta[l] = 0;
    for (int l = threadIdx.x; l < n_r; l += 256) tr[l] = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int a = la[p], r = lr[p];                              // 1 .. n_a, 1 .. n_r, or 0
        if (a) atomicAdd(ta + a - 1, r ? 0x10001u : 1u);
        if (r) atomicAdd(tr + r - 1, a ? 0x10001u : 1u);
    }
    __syncthreads();
    int hit[2 * LES_MAX_T] = {};
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const unsigned* tab = side == 0 ? ta : tr;
        const int n = side == 0 ? n_a : n_r;
        for (int l = threadIdx.x; l < n; l += 256) {
            const unsigned v = tab[l];
            const long long size = v & 0xFFFFu, cov = v >> 16;
#pragma unroll
            for (int t = 0; t < LES_MAX_T; ++t)
                if (t < ov.T && cov >= 1 && cov * ov.den[t] >= size * ov.num[t]) ++hit[side * LES_MAX_T + t];
        }
    }
#pragma unroll
    for (int k = 0; k < 2 * LES_MAX_T; ++k) {
        if (k % LES_MAX_T < ov.T) {                                  // block-uniform
            const int s = seg_wave_sum(hit[k]);
            if (lane == 0) wsum[wave][k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * ov.T) {
        const int side = threadIdx.x / ov.T, t = threadIdx.x % ov.T, k = side * LES_MAX_T + t;
        st[2 + threadIdx.x] = (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
    }
}

}  // namespace ccdm

extern "C" size_t ccdm_lesions_workspace_bytes(int B, int S, int L, int H, int W, int K) {
    if (B <= 0 || S <= 0 || L <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return (size_t)B * ((size_t)S + L) * ccdm::les_classes(K) * ((size_t)H * W + 1) * sizeof(int32_t);
}

extern "C" int ccdm_lesions(const uint8_t* samples, const uint8_t* raters, int B, int S, int L, int H, int W, int K, int connectivity,
                            const int32_t* overlaps, int T, int32_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(K >= 1 && K <= SEG_MAX_K, "lesions: K=%d outside [1,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(S >= 1 && S <= 255, "lesions: S=%d outside [1,255]", S);
    CCDM_REQUIRE(L >= 1 && L <= 255, "lesions: L=%d outside [1,255]", L);
    CCDM_REQUIRE(H >= 1, "lesions: H=%d below 1", H);
    CCDM_REQUIRE(W >= 1, "lesions: W=%d below 1", W);
    CCDM_REQUIRE((long long)H * W <= LES_MAX_PIXELS, "lesions: H*W=%lld above %d", (long long)H * W, LES_MAX_PIXELS);
    CCDM_REQUIRE(connectivity == 4 || connectivity == 8, "lesions: connectivity=%d (expected 4 or 8)", connectivity);
    CCDM_REQUIRE(T >= 1 && T <= LES_MAX_T, "lesions: T=%d outside [1,%d]", T, LES_MAX_T);
    CCDM_REQUIRE(B >= 0, "lesions: B=%d", B);
    CCDM_REQUIRE(overlaps, "lesions: null pointer (overlaps)");
    LesOverlaps ov{};
    ov.T = T;
    for (int t = 0; t < T; ++t) {
        const int num = overlaps[2 * t], den = overlaps[2 * t + 1];
        CCDM_REQUIRE(den >= 1 && den <= LES_MAX_DEN, "lesions: overlap %d: den=%d outside [1,%d]", t, den, LES_MAX_DEN);
        CCDM_REQUIRE(num >= 0 && num <= den, "lesions: overlap %d: num=%d den=%d outside 0 <= num <= den", t, num, den);
        ov.num[t] = num;
        ov.den[t] = den;
    }
    if (B == 0) return 0;
    const int C = les_classes(K), c0 = K > 1 ? 1 : 0, HW = H * W;
    const long long nA = (long long)B * S, nmaps = nA + (long long)B * L;
    const long long planes = nmaps * C, cells = nA * L * C;
    CCDM_REQUIRE(planes <= 0x7fffffffLL && cells <= 0x7fffffffLL, "lesions: B=%d images (too many blocks)", B);
    CCDM_REQUIRE(samples && raters && stats, "lesions: null pointer");
    const size_t need = ccdm_lesions_workspace_bytes(B, S, L, H, W, K);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "lesions: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "lesions: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* ws = static_cast<int32_t*>(workspace);
    int32_t* counts = ws + (size_t)planes * HW;
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(raters)) & 3) == 0;
    const int conn8 = connectivity == 8 ? 1 : 0;
    const size_t label_lds = les_label_lds(HW);
    const int nmax = les_max_lesions(HW);
    const size_t pair_lds = (size_t)2 * nmax * sizeof(unsigned);
    constexpr size_t pair_lds_max = (size_t)2 * ((LES_MAX_PIXELS + 1) / 2) * sizeof(unsigned);
    static bool reserved[3] = {false, false, false};
    if (vec) {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_lesions_label<4>, LES_LABEL_LDS_MAX, &reserved[0], "label") < 0) return -1;
        hipLaunchKernelGGL(k_lesions_label<4>, dim3((unsigned)planes), dim3(LES_THREADS), label_lds, st, samples, raters, nA, C, c0, H, W, conn8, ws,
                           counts);
    } else {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_lesions_label<1>, LES_LABEL_LDS_MAX, &reserved[1], "label") < 0) return -1;
        hipLaunchKernelGGL(k_lesions_label<1>, dim3((unsigned)planes), dim3(LES_THREADS), label_lds, st, samples, raters, nA, C, c0, H, W, conn8, ws,
                           counts);
    }
    CCDM_CHECK_LAUNCH("lesions label");
    if (pair_lds > 48 * 1024 && les_reserve_lds(k_lesions_pairs, pair_lds_max, &reserved[2], "pair") < 0) return -1;
    hipLaunchKernelGGL(k_lesions_pairs, dim3((unsigned)cells), dim3(256), pair_lds, st, ws, counts, B, S, L, C, HW, nmax, ov, stats);
    CCDM_CHECK_LAUNCH("lesions pairs");
    return 0;
}
