// What the lesion kernels share: the limits, the scored classes, the layout of the workspace ccdm_lesions leaves behind, and the
// union-find labelling of one mask by one workgroup (les_label and its steps).
// Users: ccdm_lesions.hip (labels every map and class; writes the label planes and the lesion counts), ccdm_lesionmatch.hip (reads
// them), ccdm_findings.hip (labels the two masks of the sample set per image and class).
#pragma once
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int LES_MAX_PIXELS = 16384;     // H*W: a map and its bookkeeping stay in the LDS of one workgroup; size and cov fit 16 bits
constexpr int LES_MAX_T = 8;              // thresholds of one call, by value in the kernel arguments
constexpr int LES_MAX_DEN = 65536;
constexpr int LES_THREADS = 512;          // of a label workgroup
constexpr int LES_WAVES = LES_THREADS / 64;

static inline int les_classes(int K) { return K > 1 ? K - 1 : 1; }
// A conn-4 checkerboard has ceil(H*W/2) lesions, the most any mask can have: one pixel of each lesion is an independent set of the grid.
static inline int les_max_lesions(int HW) { return (HW + 1) / 2; }
// The dynamic LDS of a label workgroup: one parent per pixel, one count per 64 pixels.
static inline size_t les_label_lds(int HW) { return ((size_t)HW + (HW + 63) / 64) * sizeof(int); }
constexpr size_t LES_LABEL_LDS_MAX = ((size_t)LES_MAX_PIXELS + LES_MAX_PIXELS / 64) * sizeof(int);

// More than 48 KB of dynamic LDS for one workgroup is asked for once per kernel: what the kernel takes at LES_MAX_PIXELS (the static
// LDS of the kernel comes on top and has to fit the CU's 160 KB with it).
template <typename Kern>
static int les_reserve_lds(Kern kern, size_t bytes, bool* done, const char* what) {
    if (*done) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return fail("lesions: cannot reserve %zu bytes of LDS for the %s kernel", bytes, what);
    *done = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------- the labelling of one mask
// One workgroup of LES_THREADS threads, the whole map resident in LDS as one int32 `parent` per pixel (-1 outside the mask), union-find
// with the smaller index as the root.  The mask is the pixels of `map` equal to `c`.
//   1 runs      a wave takes chunks of 64 * NPIX consecutive pixels (NPIX = 4: one dword per lane when W % 4 == 0 and the map is
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
//   5 write     int32 labels [H][W] and the lesion count of the mask.
// INVARIANT: parent[p] <= p for every mask pixel, at all times: step 1 writes a run's first pixel, atomicMin only ever lowers a value,
// and the value it offers is a root smaller than the pixel it is offered to.  So a find walk strictly decreases and ends after at most
// H*W reads, and a failed round of les_unite replaces its larger end by a strictly smaller pixel: at most 2*H*W rounds.  Every other
// loop counts up to H*W, to the number of chunks or to 64.  No workgroup waits on another; no global atomics.

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

// Step 1.  Wave-uniform trip count: every lane stays active for the ballot and the shuffle.  The caller synchronises.
template <int NPIX>
__device__ __forceinline__ void les_runs(int* parent, const uint8_t* __restrict__ map, uint32_t c, int HW, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
}

// Step 2.  Whether a pixel is in the mask is the sign of its parent, which no union changes.  CH: the chunk of step 1.
__device__ __forceinline__ void les_unions(int* parent, int HW, int W, int CH, int conn8) {
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
}

// Step 3.
__device__ __forceinline__ void les_flatten(int* parent, int HW) {
    for (int p = threadIdx.x; p < HW; p += LES_THREADS)
        if (les_load(parent + p) >= 0) parent[p] = les_find(parent, p);
}

// Step 4: ranks the roots in raster order; cc [ceil(HW/64)] is scratch.  The lesion count goes to *count.  Ends synchronised.
__device__ __forceinline__ void les_rank(int* parent, int* cc, int HW, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n64 = (HW + 63) / 64;
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
        if (lane == 63) *count = incl;
    }
    __syncthreads();
    for (int k = wave; k < n64; k += LES_WAVES) {
        const int p = k * 64 + lane;
        const bool root = p < HW && parent[p] == p;
        const unsigned long long roots = __ballot(root);
        if (root) parent[p] = -(cc[k] + __popcll(roots & ((1ull << lane) - 1ull)) + 1) - 1;
    }
    __syncthreads();
}

// Step 5: the dense labels.
__device__ __forceinline__ void les_write(const int* parent, int HW, int32_t* __restrict__ out) {
    for (int p = threadIdx.x; p < HW; p += LES_THREADS) {
        const int v = parent[p];
        out[p] = v == -1 ? 0 : v < -1 ? -v - 1 : -parent[v] - 1;
    }
}

// All five steps: `lds` holds les_label_lds(H*W) bytes; called by every thread of a workgroup of LES_THREADS.
template <int NPIX>
__device__ __forceinline__ void les_label(int* lds, const uint8_t* __restrict__ map, uint32_t c, int H, int W, int conn8,
                                          int32_t* __restrict__ out, int32_t* __restrict__ count) {
    const int HW = H * W;
    int* parent = lds;                                               // [HW]
    int* cc = lds + HW;                                              // [ceil(HW/64)]: roots per 64 pixels, then the roots before them
    les_runs<NPIX>(parent, map, c, HW, W);
    __syncthreads();
    les_unions(parent, HW, W, 64 * NPIX, conn8);
    __syncthreads();
    les_flatten(parent, HW);
    __syncthreads();
    les_rank(parent, cc, HW, count);
    les_write(parent, HW, out);
}

}  // namespace ccdm
