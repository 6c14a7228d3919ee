// LIDC matched-lesion scores, device part (beyond the reference): per (image, sample, rater, class) the one-to-one pairing of the
// sample's lesions with the rater's by IoU, the number of matched pairs and the sum of their IoUs to each of T thresholds: what
// panoptic quality, segmentation quality and recognition quality are made of.  The definition in include/ccdm_hip.h is the contract;
// tests/test_lidc_lesion_matching.py restates it with scipy and numpy.  The kernels read the label planes and lesion counts that
// ccdm_lesions left in its workspace, nothing of the maps.
//
// Two facts the pair kernel rests on:
//   * Two 4-adjacent pixels that are in the mask of both maps lie in one lesion of either map (under 4- and under 8-connectivity),
//     so they carry the same pair (a, r).  Take one pixel of every distinct non-empty pair: no two of them are 4-adjacent, an
//     independent set of the grid.  A cell has at most ceil(H*W/2) distinct non-empty pairs, 8192 at the limit; and never more than
//     n_a * n_r.
//   * A matched pair has inter > union/2, so inter > size(a)/2 and inter > size(r)/2: a lesion's only possible partner is the
//     majority label under it, the matching is unique and nothing is assigned.
//
// Size stage (k_lesion_sizes), once per (map, class) plane, not per cell: one workgroup of 256 threads counts the pixels of every
// label in an LDS table (<= 8192 uint32 = 32 KB), writes the sizes and the number of lesions of at least min_size pixels behind the
// lesion counts of the workspace.  The sizes live in global memory because the two sides' size tables and the pair table of a cell
// do not fit the LDS of a CU together at the limit.
// Pair stage (k_lesion_match), one workgroup of 256 threads per cell.  An open-addressing table in LDS, keys a << 16 | r (uint32, 0
// = free) claimed by atomicCAS, counts (uint32) by atomicAdd, linear probing.  The table of a cell has the smallest power of two of
// slots that is >= 2 * min(ceil(H*W/2), n_a*n_r) and >= 64: by the bound above it is never more than half full, so a probe sequence
// meets a free slot or its own key; the probe loop is bounded by the slot count besides.  A wave adds the lanes that share its first
// pair as one count (the pixels of one row mostly do), the others one by one.  One walk over the table then takes the two sizes of
// every occupied slot from the size stage's tables, drops the pairs with a lesion below min_size and tests the others against the T
// thresholds; floor(inter * 2^32 / union) is one 64-bit division per pair with 2*inter > union.  tp and the fixed-point sums are
// reduced per thread, wave (fixed order) and block (the four waves in order).  Integers only: exact in any order, two identical calls
// are bit-identical.  No workgroup waits on another; no global atomics.
// LDS at the limit (H*W = 16384): 16384 slots * 8 B = 128 KB of table + 384 B of wave sums: ONE workgroup (4 waves) per CU, reserved
// once.  A smaller map takes a smaller table (32x48: 16 KB).
#include "ccdm_lesions_common.h"

namespace ccdm {

constexpr int LM_THREADS = 256;
constexpr int LM_WAVES = LM_THREADS / 64;
constexpr int LM_MIN_SLOTS = 64;

struct LmThresholds {
    int T;
    int num[LES_MAX_T], den[LES_MAX_T];
};

// the slots of a table that holds `pairs` keys at a load of at most 1/2
__host__ __device__ static inline int lm_slots(int pairs) {
    int s = LM_MIN_SLOTS;
    while (s < 2 * pairs) s <<= 1;
    return s;
}

// Adds the wave's keys (0: none) to a table through add(key, n): the lanes that hold the key of the first lane that has one as one
// call with their number, every other lane by itself.  All 64 lanes call.
template <typename F>
__device__ __forceinline__ void lm_wave_add(unsigned key, F&& add) {
    const unsigned long long todo = __ballot(key != 0);
    if (!todo) return;
    const unsigned lead = seg_readlane(key, __ffsll((long long)todo) - 1);
    const unsigned long long same = __ballot(key == lead);
    const int lane = threadIdx.x & 63;
    if (key == lead) {
        if (lane == __ffsll((long long)same) - 1) add(lead, (unsigned)__popcll(same));
    } else if (key) {
        add(key, 1u);
    }
}

// Linear probing from the key's hash.  The table is at most half full (file header), so the walk ends at the key or at a free slot
// long before the bound of the loop.
__device__ __forceinline__ void lm_table_add(unsigned* keys, unsigned* cnt, unsigned mask, int shift, unsigned key, unsigned n) {
    unsigned h = (key * 0x9E3779B1u) >> shift;
    for (unsigned i = 0; i <= mask; ++i) {
        unsigned old = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == 0) old = atomicCAS(keys + h, 0u, key);
        if (old == 0 || old == key) {
            atomicAdd(cnt + h, n);
            return;
        }
        h = (h + 1) & mask;
    }
}

__device__ __forceinline__ long long lm_wave_sum(long long x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// A label outside 1..n (a workspace that ccdm_lesions did not write) counts as no lesion: nothing is indexed with it.
__global__ __launch_bounds__(LM_THREADS) void k_lesion_sizes(const int32_t* __restrict__ ws, const int32_t* __restrict__ counts, int HW, int nmax,
                                                             int min_size, int32_t* __restrict__ sizes, int32_t* __restrict__ kept) {
    extern __shared__ unsigned lm_size[];                            // [nmax]: pixels per label
    __shared__ int wsum[LM_WAVES];
    const size_t plane = blockIdx.x;
    const int n = min(max(counts[plane], 0), nmax);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (n == 0) {                                                    // block-uniform
        if (threadIdx.x == 0) kept[plane] = 0;
        return;
    }
    for (int l = threadIdx.x; l < n; l += LM_THREADS) lm_size[l] = 0;
    __syncthreads();
    const int32_t* lab = ws + plane * HW;
    for (int p0 = wave * 64; p0 < HW; p0 += LM_THREADS) {            // wave-uniform: every lane reaches the ballots
        const int p = p0 + lane;
        const int l = p < HW ? lab[p] : 0;
        lm_wave_add(l >= 1 && l <= n ? (unsigned)l : 0u, [&](unsigned key, unsigned cnt) { atomicAdd(lm_size + key - 1, cnt); });
    }
    __syncthreads();
    int32_t* out = sizes + plane * nmax;
    int k = 0;
    for (int l = threadIdx.x; l < n; l += LM_THREADS) {
        const int s = (int)lm_size[l];
        out[l] = s;
        k += s >= min_size ? 1 : 0;
    }
    k = seg_wave_sum(k);
    if (lane == 0) wsum[wave] = k;
    __syncthreads();
    if (threadIdx.x == 0) kept[plane] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(LM_THREADS) void k_lesion_match(const int32_t* __restrict__ ws, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ sizes, const int32_t* __restrict__ kept, int B, int S, int L,
                                                             int C, int HW, int nmax, int min_size, LmThresholds th, int32_t* __restrict__ stats,
                                                             long long* __restrict__ iou_sum) {
    extern __shared__ unsigned lm_tab[];                             // keys [slots], counts [slots] of this cell
    __shared__ int wtp[LM_WAVES][LES_MAX_T];
    __shared__ long long wq[LM_WAVES][LES_MAX_T];
    const size_t cell = blockIdx.x;
    const int ci = (int)(cell % C), j = (int)(cell / C % L), i = (int)(cell / ((size_t)C * L) % S), b = (int)(cell / ((size_t)C * L * S));
    const size_t pa = ((size_t)b * S + i) * C + ci, pr = ((size_t)B * S + (size_t)b * L + j) * C + ci;
    const int la_n = min(max(counts[pa], 0), nmax), lr_n = min(max(counts[pr], 0), nmax);     // all lesions, kept or not
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* st = stats + cell * (2 + th.T);
    long long* qs = iou_sum + cell * th.T;
    if (threadIdx.x == 0) { st[0] = kept[pa]; st[1] = kept[pr]; }
    if (la_n == 0 || lr_n == 0) {                                    // block-uniform: no pair
        if (threadIdx.x < th.T) { st[2 + threadIdx.x] = 0; qs[threadIdx.x] = 0; }
        return;
    }
    const int slots = lm_slots(min(nmax, la_n * lr_n));              // la_n * lr_n <= 2^26
    const unsigned mask = (unsigned)slots - 1u;
    const int shift = __clz(slots) + 1;                              // 32 - log2(slots)
    unsigned* keys = lm_tab;
    unsigned* cnt = lm_tab + slots;
    for (int s = threadIdx.x; s < 2 * slots; s += LM_THREADS) lm_tab[s] = 0;
    __syncthreads();
    const int32_t* la = ws + pa * HW;
    const int32_t* lr = ws + pr * HW;
    for (int p0 = wave * 64; p0 < HW; p0 += LM_THREADS) {            // wave-uniform
        const int p = p0 + lane;
        unsigned key = 0;
        if (p < HW) {
            const int a = la[p], r = lr[p];
            if (a >= 1 && a <= la_n && r >= 1 && r <= lr_n) key = (unsigned)a << 16 | (unsigned)r;
        }
        lm_wave_add(key, [&](unsigned k, unsigned n) { lm_table_add(keys, cnt, mask, shift, k, n); });
    }
    __syncthreads();
    const int32_t* size_a = sizes + pa * nmax;
    const int32_t* size_r = sizes + pr * nmax;
    int tp[LES_MAX_T] = {};
    long long q[LES_MAX_T] = {};
    for (int s = threadIdx.x; s < slots; s += LM_THREADS) {
        const unsigned key = keys[s];
        if (!key) continue;
        const int sa = size_a[(key >> 16) - 1], sr = size_r[(key & 0xFFFFu) - 1];
        if (sa < min_size || sr < min_size) continue;                // a dropped lesion matches nothing
        const long long inter = cnt[s], uni = (long long)sa + sr - inter;
        if (2 * inter <= uni) continue;                              // below every valid threshold
        const long long f = (inter << 32) / uni;                     // inter <= 2^14
#pragma unroll
        for (int t = 0; t < LES_MAX_T; ++t) {
            if (t < th.T && inter * th.den[t] > uni * th.num[t]) {
                ++tp[t];
                q[t] += f;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < LES_MAX_T; ++t) {
        if (t < th.T) {                                              // block-uniform
            const int n = seg_wave_sum(tp[t]);
            const long long f = lm_wave_sum(q[t]);
            if (lane == 0) { wtp[wave][t] = n; wq[wave][t] = f; }
        }
    }
    __syncthreads();
    if (threadIdx.x < th.T) {
        const int t = threadIdx.x;
        st[2 + t] = (wtp[0][t] + wtp[1][t]) + (wtp[2][t] + wtp[3][t]);
        qs[t] = (wq[0][t] + wq[1][t]) + (wq[2][t] + wq[3][t]);
    }
}

}  // namespace ccdm

extern "C" size_t ccdm_lesion_match_workspace_bytes(int B, int S, int L, int H, int W, int K) {
    const size_t labels = ccdm_lesions_workspace_bytes(B, S, L, H, W, K);
    if (labels == 0) return 0;
    const size_t nmax = ((size_t)H * W + 1) / 2;                     // les_max_lesions, at any size
    return labels + (size_t)B * ((size_t)S + L) * ccdm::les_classes(K) * (nmax + 1) * sizeof(int32_t);
}

extern "C" int ccdm_lesion_match(int B, int S, int L, int H, int W, int K, const int32_t* thresholds, int T, int min_size, int32_t* stats,
                                 int64_t* iou_sum, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(K >= 1 && K <= SEG_MAX_K, "lesion_match: K=%d outside [1,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(S >= 1 && S <= 255, "lesion_match: S=%d outside [1,255]", S);
    CCDM_REQUIRE(L >= 1 && L <= 255, "lesion_match: L=%d outside [1,255]", L);
    CCDM_REQUIRE(H >= 1, "lesion_match: H=%d below 1", H);
    CCDM_REQUIRE(W >= 1, "lesion_match: W=%d below 1", W);
    CCDM_REQUIRE((long long)H * W <= LES_MAX_PIXELS, "lesion_match: H*W=%lld above %d", (long long)H * W, LES_MAX_PIXELS);
    CCDM_REQUIRE(T >= 1 && T <= LES_MAX_T, "lesion_match: T=%d outside [1,%d]", T, LES_MAX_T);
    CCDM_REQUIRE(min_size >= 1, "lesion_match: min_size=%d below 1", min_size);
    CCDM_REQUIRE(B >= 0, "lesion_match: B=%d", B);
    CCDM_REQUIRE(thresholds, "lesion_match: null pointer (thresholds)");
    LmThresholds th{};
    th.T = T;
    for (int t = 0; t < T; ++t) {
        const int num = thresholds[2 * t], den = thresholds[2 * t + 1];
        CCDM_REQUIRE(den >= 1 && den <= LES_MAX_DEN, "lesion_match: threshold %d: den=%d outside [1,%d]", t, den, LES_MAX_DEN);
        CCDM_REQUIRE(num >= 1 && num < den && den <= 2LL * num, "lesion_match: threshold %d: num=%d den=%d outside 1/2 <= num/den < 1", t, num, den);
        th.num[t] = num;
        th.den[t] = den;
    }
    if (B == 0) return 0;
    const int C = les_classes(K), HW = H * W;
    const long long nmaps = (long long)B * S + (long long)B * L;
    const long long planes = nmaps * C, cells = (long long)B * S * L * C;
    CCDM_REQUIRE(planes <= 0x7fffffffLL && cells <= 0x7fffffffLL, "lesion_match: B=%d images (too many blocks)", B);
    CCDM_REQUIRE(stats && iou_sum, "lesion_match: null pointer");
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(iou_sum) & 7) == 0, "lesion_match: iou_sum must be 8-byte aligned");
    const size_t need = ccdm_lesion_match_workspace_bytes(B, S, L, H, W, K);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "lesion_match: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "lesion_match: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nmax = les_max_lesions(HW);
    int32_t* ws = static_cast<int32_t*>(workspace);
    int32_t* counts = ws + (size_t)planes * HW;                      // what ccdm_lesions wrote: the planes, then the counts
    int32_t* sizes = counts + planes;                                // this call's: [planes][nmax], then the kept lesions [planes]
    int32_t* kept = sizes + (size_t)planes * nmax;
    hipLaunchKernelGGL(k_lesion_sizes, dim3((unsigned)planes), dim3(LM_THREADS), (size_t)nmax * sizeof(unsigned), st, ws, counts, HW, nmax, min_size,
                       sizes, kept);
    CCDM_CHECK_LAUNCH("lesion_match sizes");
    const size_t tab_lds = (size_t)2 * lm_slots(nmax) * sizeof(unsigned);
    const size_t tab_lds_max = (size_t)2 * lm_slots(les_max_lesions(LES_MAX_PIXELS)) * sizeof(unsigned);
    static bool reserved = false;
    if (tab_lds > 48 * 1024 && les_reserve_lds(k_lesion_match, tab_lds_max, &reserved, "match") < 0) return -1;
    hipLaunchKernelGGL(k_lesion_match, dim3((unsigned)cells), dim3(LM_THREADS), tab_lds, st, ws, counts, sizes, kept, B, S, L, C, HW, nmax, min_size,
                       th, stats, reinterpret_cast<long long*>(iou_sum));
    CCDM_CHECK_LAUNCH("lesion_match pairs");
    return 0;
}
