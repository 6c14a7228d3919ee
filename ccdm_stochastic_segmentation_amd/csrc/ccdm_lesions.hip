// LIDC lesion-level scores, device part (beyond the reference, whose LIDC scores are all overlap scores): per (image, sample, rater,
// class) the number of lesions (connected components) of either map and how many of them the other map's mask covers to each of T
// overlap thresholds.  The definition in include/ccdm_hip.h is the contract; tests/test_lidc_lesions.py restates it with numpy and
// holds it against scipy.ndimage.label.
//
// Label stage (k_lesions_label), once per (map, class), not per pair: one workgroup of 512 threads, the whole map resident in LDS as
// one int32 `parent` per pixel (-1 outside the mask), union-find with the smaller index as the root.
//   1 runs      a wave takes chunks of 64 * NPIX consecutive pixels (NPIX = 4: one dword per lane when W % 4 == 0 and both stacks are
//               4-byte aligned, so a dword never straddles a row; NPIX = 1: bytes).  A pixel's parent is the first pixel of its
//               horizontal run inside the chunk: inside the lane from its own bits, across lanes from a ballot of the lanes a run
//               cannot pass through (a bit clear, or the lane starts a row) and one shuffle of the nearest such lane's value.
//   2 unions    per mask pixel: with the pixel to the left where a run was cut at a chunk seam; with the row above (the pixel above,
//               unless the pixel to the left and the one above it are both in the mask: then the left pixel's union covers it; for
//               8-connectivity the two diagonals where the pixel above is not in the mask).  les_unite: find both roots, LDS
//               atomicMin of the smaller root into the larger root's parent, again from the displaced parent if the larger one was
//               a root no more.
//   3 flatten   every mask pixel's parent becomes its root; the root of a lesion is its smallest pixel index.
//   4 rank      root flags by ballot per 64 pixels in raster order, one wave's prefix sum over the <= 256 chunk counts: the dense
//               label of a root is 1 + the roots before it; written into the root's parent as -(label) - 1.
//   5 write     int32 labels [H][W] to the workspace, the lesion count of the (map, class) behind the planes.
// INVARIANT: parent[p] <= p for every mask pixel, at all times: step 1 writes a run's first pixel, atomicMin only ever lowers a value,
// and the value it offers is a root smaller than the pixel it is offered to.  So a find walk strictly decreases and ends after at most
// H*W reads, and a failed round of les_unite replaces its larger end by a strictly smaller pixel: at most 2*H*W rounds.  No workgroup
// waits on another; no global atomics.
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

constexpr int LES_THREADS = 512;          // of a label workgroup
constexpr int LES_WAVES = LES_THREADS / 64;

struct LesOverlaps {
    int T;
    int num[LES_MAX_T], den[LES_MAX_T];
};

// Another thread may lower the value at any time: never a cached read.
__device__ __forceinline__ int les_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int les_find(const int* parent, int p) {
    int q = les_load(parent + p);
    while (q != p) {                                                 // q < p (the invariant): at most H*W steps
        p = q;
        q = les_load(parent + p);
    }
    return p;
}

// Joins the lesions of the mask pixels a and b.  A failed round (the larger root had been linked elsewhere meanwhile) goes on from the
// parent it had, which is smaller: at most 2*H*W rounds.
__device__ __forceinline__ void les_unite(int* parent, int a, int b) {
    for (;;) {
        a = les_find(parent, a);
        b = les_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

template <int NPIX>
__global__ __launch_bounds__(LES_THREADS) void k_lesions_label(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters, long long nA,
                                                               int C, int c0, int H, int W, int conn8, int32_t* __restrict__ ws,
                                                               int32_t* __restrict__ counts) {
    extern __shared__ int les_lds[];
    const int HW = H * W, n64 = (HW + 63) / 64;
    int* parent = les_lds;                                           // [HW]
    int* cc = les_lds + HW;                                          // [n64]: roots per 64 pixels, then the roots before them
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t mc = blockIdx.x;
    const long long m = (long long)(mc / C);
    const uint32_t c = (uint32_t)(c0 + (int)(mc % C));
    const uint8_t* map = m < nA ? samples + (size_t)m * HW : raters + (size_t)(m - nA) * HW;

    // 1: runs.  Wave-uniform trip count: every lane stays active for the ballot and the shuffle.
    constexpr int CH = 64 * NPIX;
    const int nch = (HW + CH - 1) / CH;
    for (int k = wave; k < nch; k += LES_WAVES) {
        const int p0 = (k * 64 + lane) * NPIX;
        uint32_t bits = 0;
        if (p0 < HW) {
            if constexpr (NPIX == 4) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(map + p0);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((v >> (8 * j) & 0xFFu) == c) bits |= 1u << j;
            } else {
                bits = map[p0] == c ? 1u : 0u;
            }
        }
        const bool row_start = p0 % W == 0;
        const bool breaker = bits != (1u << NPIX) - 1u || row_start || lane == 0;     // lane 0: a chunk's runs start inside it
        int loc = p0;                                                // the run that leaves this lane to the right starts here
#pragma unroll
        for (int j = 0; j < NPIX; ++j)
            if (!(bits >> j & 1u)) loc = p0 + j + 1;
        const unsigned long long lower = __ballot(breaker) & ((1ull << lane) - 1ull);
        const int from = __shfl(loc, lower ? 63 - __clzll((long long)lower) : 0);
        int cur = row_start || lane == 0 ? p0 : from;                // a run cut at the chunk seam: step 2 joins it
        if (p0 < HW) {
#pragma unroll
            for (int j = 0; j < NPIX; ++j) {
                if (bits >> j & 1u) {
                    parent[p0 + j] = cur;
                } else {
                    parent[p0 + j] = -1;
                    cur = p0 + j + 1;
                }
            }
        }
    }
    __syncthreads();

    // 2: unions.  Whether a pixel is in the mask is the sign of its parent, which no union changes.
    for (int p = threadIdx.x; p < HW; p += LES_THREADS) {
        if (les_load(parent + p) < 0) continue;
        const int y = p / W, x = p - y * W;
        const bool left = x > 0 && les_load(parent + p - 1) >= 0;
        if (left && p % CH == 0) les_unite(parent, p, p - 1);
        if (y > 0) {
            if (les_load(parent + p - W) >= 0) {
                if (!(left && les_load(parent + p - W - 1) >= 0)) les_unite(parent, p, p - W);
            } else if (conn8) {
                if (x > 0 && !left && les_load(parent + p - W - 1) >= 0) les_unite(parent, p, p - W - 1);
                if (x + 1 < W && les_load(parent + p - W + 1) >= 0) les_unite(parent, p, p - W + 1);
            }
        }
    }
    __syncthreads();

    // 3: flatten
    for (int p = threadIdx.x; p < HW; p += LES_THREADS)
        if (les_load(parent + p) >= 0) parent[p] = les_find(parent, p);
    __syncthreads();

    // 4: rank the roots in raster order
    for (int k = wave; k < n64; k += LES_WAVES) {
        const int p = k * 64 + lane;
        const unsigned long long roots = __ballot(p < HW && parent[p] == p);
        if (lane == 0) cc[k] = __popcll(roots);
    }
    __syncthreads();
    if (wave == 0) {
        const int per = (n64 + 63) / 64;                             // <= 4
        int s = 0;
        for (int i = 0; i < per; ++i)
            if (lane * per + i < n64) s += cc[lane * per + i];
        int incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        int before = incl - s;
        for (int i = 0; i < per; ++i) {
            if (lane * per + i < n64) {
                const int t = cc[lane * per + i];
                cc[lane * per + i] = before;
                before += t;
            }
        }
        if (lane == 63) counts[mc] = incl;
    }
    __syncthreads();
    for (int k = wave; k < n64; k += LES_WAVES) {
        const int p = k * 64 + lane;
        const bool root = p < HW && parent[p] == p;
        const unsigned long long roots = __ballot(root);
        if (root) parent[p] = -(cc[k] + __popcll(roots & ((1ull << lane) - 1ull)) + 1) - 1;
    }
    __syncthreads();

    // 5: the dense labels
    int32_t* out = ws + mc * HW;
    for (int p = threadIdx.x; p < HW; p += LES_THREADS) {
        const int v = parent[p];
        out[p] = v == -1 ? 0 : v < -1 ? -v - 1 : -parent[v] - 1;
    }
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
    const size_t label_lds = ((size_t)HW + (HW + 63) / 64) * sizeof(int);
    const int nmax = les_max_lesions(HW);
    const size_t pair_lds = (size_t)2 * nmax * sizeof(unsigned);
    constexpr size_t label_lds_max = ((size_t)LES_MAX_PIXELS + LES_MAX_PIXELS / 64) * sizeof(int);
    constexpr size_t pair_lds_max = (size_t)2 * ((LES_MAX_PIXELS + 1) / 2) * sizeof(unsigned);
    static bool reserved[3] = {false, false, false};
    if (vec) {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_lesions_label<4>, label_lds_max, &reserved[0], "label") < 0) return -1;
        hipLaunchKernelGGL(k_lesions_label<4>, dim3((unsigned)planes), dim3(LES_THREADS), label_lds, st, samples, raters, nA, C, c0, H, W, conn8, ws,
                           counts);
    } else {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_lesions_label<1>, label_lds_max, &reserved[1], "label") < 0) return -1;
        hipLaunchKernelGGL(k_lesions_label<1>, dim3((unsigned)planes), dim3(LES_THREADS), label_lds, st, samples, raters, nA, C, c0, H, W, conn8, ws,
                           counts);
    }
    CCDM_CHECK_LAUNCH("lesions label");
    if (pair_lds > 48 * 1024 && les_reserve_lds(k_lesions_pairs, pair_lds_max, &reserved[2], "pair") < 0) return -1;
    hipLaunchKernelGGL(k_lesions_pairs, dim3((unsigned)cells), dim3(256), pair_lds, st, ws, counts, B, S, L, C, HW, nmax, ov, stats);
    CCDM_CHECK_LAUNCH("lesions pairs");
    return 0;
}
