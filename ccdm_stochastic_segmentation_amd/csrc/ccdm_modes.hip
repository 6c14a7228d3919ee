// Mode summary of a multi-sample prediction (metrics.sample_modes, DenoisingModel.predict_modes): k-medoids over the S samples of an
// image under the distance the evaluation itself uses, 1 - mean foreground IoU, in exact integers.  The definition (the fixed-point
// distance Q, PAM's BUILD and SWAP with their tie rules, assignment and ordering) is in include/ccdm_hip.h.
//
//   k_modes_pairs  one workgroup per (image, 16 x 16 tile of pairs i <= j, share of the pixels): each 1024-pixel chunk of the tile's 32
//                  maps is staged once in LDS and serves 256 pairs (k_pair_counts of ccdm_metrics.hip reads both maps from memory for every
//                  pair); a thread owns one pair, counts I_k sixteen pixels to the LDS read and adds its counts to the workspace with
//                  integer atomics (exact in any order).  The pair of a map with itself gives n_i[k]
//   k_modes_finish one thread per pair i <= j: Q[i][j] from I_k, n_i[k] and n_j[k], written with its mirror
//   k_modes_pam    one workgroup per image: BUILD, SWAP, assignment and ordering on Q (in LDS for S <= 128); int64 sums, argmin/argmax by
//                  wave shuffles and an LDS stage that carry the index for the tie rule
//   k_modes_maps   one thread per (image, mode, pixel): the class counts over the mode's members, their majority and their entropy
#include <climits>

#include "ccdm_common.h"

namespace ccdm {

constexpr int MODES_MAX_S = 256, MODES_MAX_M = 16, MODES_MAX_K = 32;
constexpr int MODES_TILE = 16;                       // samples per side of a tile of pairs: 256 pairs, one per thread
constexpr int MODES_CHUNK = 1024;                    // pixels of a map staged at once
constexpr int MODES_ROW_DW = MODES_CHUNK / 4 + 4;    // dwords per staged row: 16-byte aligned, and the 16 rows a wave reads 16 bytes of lie on 16 bank quads
constexpr int MODES_LDS_S = 128;                     // Q of one image lives in LDS up to here (64 KB)
constexpr int MODES_Q_ONE_LOG2 = 20;

// the four pixels at p .. p + 3 of a map as one dword; a pixel at or beyond HW reads as 0 (the background, which is never counted)
__device__ __forceinline__ uint32_t modes_load4(const uint8_t* __restrict__ map, int64_t p, int64_t HW, bool aligned) {
    if (aligned && p + 4 <= HW) return *reinterpret_cast<const uint32_t*>(map + p);
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (p + e < HW) w |= (uint32_t)map[p + e] << (8 * e);
    return w;
}

// how many of the four bytes of z are zero (exact per byte: (z & 0x7f) + 0x7f never carries into the next byte)
__device__ __forceinline__ int modes_zero_bytes(uint32_t z) {
    const uint32_t nz = ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z;
    return __popc(~nz & 0x80808080u);
}

template <int KP>
__global__ __launch_bounds__(256) void k_modes_pairs(const uint8_t* __restrict__ a, int S, int64_t HW, int K, int ntile, int chunks_per_split,
                                                     int aligned, int32_t* __restrict__ inter) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[2 * MODES_TILE * MODES_ROW_DW];
    const int tid = threadIdx.x, b = blockIdx.y;
    int t = blockIdx.x, TI = 0;                                           // the tile pairs TI <= TJ, row by row
    while (t >= ntile - TI) { t -= ntile - TI; ++TI; }
    const int TJ = TI + t;
    const bool diagonal = TI == TJ;                                       // both sides are the same 16 maps: staged once
    const int ti = tid >> 4, tj = tid & 15;
    const int i = TI * MODES_TILE + ti, j = TJ * MODES_TILE + tj;
    const uint8_t* img = a + (size_t)b * S * HW;
    const uint4* ra = reinterpret_cast<const uint4*>(tile + ti * MODES_ROW_DW);
    const uint4* rb = reinterpret_cast<const uint4*>(tile + ((diagonal ? 0 : MODES_TILE) + tj) * MODES_ROW_DW);
    const int rows = diagonal ? MODES_TILE : 2 * MODES_TILE;
    int cnt[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = 0;
    const int64_t nchunk = (HW + MODES_CHUNK - 1) / MODES_CHUNK;
    const int64_t c0 = (int64_t)blockIdx.z * chunks_per_split;
    const int64_t c1 = c0 + chunks_per_split < nchunk ? c0 + chunks_per_split : nchunk;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t p0 = c * MODES_CHUNK;
        __syncthreads();                                                  // the chunk before has been counted
        for (int d = tid; d < rows * (MODES_CHUNK / 4); d += 256) {       // (every dword of a row is written: zeros beyond HW and S)
            const int r = d / (MODES_CHUNK / 4), w = d % (MODES_CHUNK / 4);
            const int s = (r < MODES_TILE ? TI : TJ) * MODES_TILE + (r & (MODES_TILE - 1));
            tile[r * MODES_ROW_DW + w] = s < S ? modes_load4(img + (size_t)s * HW, p0 + 4 * w, HW, aligned != 0) : 0u;
        }
        __syncthreads();
#pragma unroll 2
        for (int w = 0; w < MODES_CHUNK / 16; ++w) {
            const uint4 va = ra[w], vb = rb[w];
#pragma unroll
            for (int k = 1; k < KP; ++k) {
                const uint32_t kk = 0x01010101u * k;                      // (a byte of the OR is zero iff both maps say k there)
                if (k < K)
                    cnt[k] += modes_zero_bytes((va.x ^ kk) | (vb.x ^ kk)) + modes_zero_bytes((va.y ^ kk) | (vb.y ^ kk)) +
                              modes_zero_bytes((va.z ^ kk) | (vb.z ^ kk)) + modes_zero_bytes((va.w ^ kk) | (vb.w ^ kk));
            }
        }
    }
    if (i >= S || j >= S || i > j) return;                                // (i == j stays: I_k of a map with itself is n_i[k])
    int32_t* o = inter + (((size_t)b * S + i) * S + j) * K;
#pragma unroll
    for (int k = 1; k < KP; ++k)
        if (k < K && cnt[k] != 0) atomicAdd(o + k, cnt[k]);
}

// Q of every pair i <= j from the intersections, with its mirror
__global__ __launch_bounds__(256) void k_modes_finish(const int32_t* __restrict__ inter, int S, int K, int32_t* __restrict__ Q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S * S) return;
    const int i = e / S, j = e - i * S;
    if (i > j) return;
    int32_t* Qb = Q + (size_t)blockIdx.y * S * S;
    if (i == j) { Qb[e] = 0; return; }
    const int32_t* base = inter + (size_t)blockIdx.y * S * S * K;
    const int32_t* pij = base + ((size_t)i * S + j) * K;
    const int32_t* pii = base + ((size_t)i * S + i) * K;
    const int32_t* pjj = base + ((size_t)j * S + j) * K;
    long long q = 0;
    for (int k = 1; k < K; ++k) {
        const long long in = pij[k], uni = (long long)pii[k] + (long long)pjj[k] - in;
        if (uni > 0) q += ((2 * (uni - in) << MODES_Q_ONE_LOG2) + uni) / (2 * uni);
    }
    Qb[(size_t)i * S + j] = (int32_t)q;
    Qb[(size_t)j * S + i] = (int32_t)q;
}

// ------------------------------------------------------------------------------------------------ PAM
// (value, index) with the tie rule: the lower value, then the lower index
__device__ __forceinline__ bool modes_better(long long v, int i, long long bv, int bi) { return v < bv || (v == bv && i < bi); }

struct ModesBest {
    long long v;
    int i;
};

// argmin over the 256 threads of a block; every thread calls it and gets the result
__device__ __forceinline__ ModesBest modes_block_argmin(long long v, int i, long long* sv, int* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (modes_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    ModesBest r{sv[0], si[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (modes_better(sv[w], si[w], r.v, r.i)) { r.v = sv[w]; r.i = si[w]; }
    __syncthreads();                                                      // (the stage is free again)
    return r;
}

__device__ __forceinline__ long long modes_block_sum(long long v, long long* sv) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
    __syncthreads();
    const long long r = sv[0] + sv[1] + sv[2] + sv[3];
    __syncthreads();
    return r;
}

struct ModesState {
    int32_t d1[MODES_MAX_S];          // Q to the nearest medoid
    int32_t d2[MODES_MAX_S];          // Q to the nearest medoid of another slot (INT_MAX with one medoid)
    int32_t slot[MODES_MAX_S];        // the slot of the nearest medoid, the lowest on ties: the assignment
    int32_t is_med[MODES_MAX_S];
    int32_t med[MODES_MAX_M];         // the medoid of every filled slot, in BUILD order
    int32_t rank[MODES_MAX_M];        // slot -> position in the output order
    long long sv[4];
    int si[4];
};

// d1, d2 and slot of every sample from the medoids of the first `filled` slots (Q is symmetric: row med[c] is read along j)
__device__ __forceinline__ void modes_update_near(ModesState& st, const int32_t* q, int S, int filled) {
    const int j = threadIdx.x;
    if (j < S) {
        int b1 = INT_MAX, b2 = INT_MAX, s1 = 0;
        for (int c = 0; c < filled; ++c) {
            const int v = q[(size_t)st.med[c] * S + j];
            if (v < b1) { b2 = b1; b1 = v; s1 = c; }
            else if (v < b2) b2 = v;
        }
        st.d1[j] = b1; st.d2[j] = b2; st.slot[j] = s1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_modes_pam(const int32_t* __restrict__ Qg, int S, int M, int max_swaps, int in_lds,
                                                   int32_t* __restrict__ medoid, int32_t* __restrict__ assign, int32_t* __restrict__ size,
                                                   long long* __restrict__ spread, long long* __restrict__ cost_out,
                                                   int32_t* __restrict__ swaps_out, int32_t* __restrict__ converged_out) {
    extern __shared__ int32_t pam_q[];                                    // [S][S] when in_lds
    __shared__ ModesState st;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int32_t* Qb = Qg + (size_t)b * S * S;
    if (in_lds)
        for (int e = tid; e < S * S; e += 256) pam_q[e] = Qb[e];
    const int32_t* q = in_lds ? pam_q : Qb;
    st.is_med[tid] = 0;
    __syncthreads();

    // BUILD: the sample with the lowest sum of distances, then by the largest gain
    long long v = LLONG_MAX;
    if (tid < S) {
        v = 0;
        for (int j = 0; j < S; ++j) v += q[(size_t)j * S + tid];
    }
    ModesBest r = modes_block_argmin(v, tid, st.sv, st.si);
    if (tid == 0) { st.med[0] = r.i; st.is_med[r.i] = 1; }
    int filled = 1;
    __syncthreads();
    modes_update_near(st, q, S, filled);
    for (int c = 1; c < M; ++c) {
        v = LLONG_MAX;
        if (tid < S && !st.is_med[tid]) {
            long long g = 0;
            for (int j = 0; j < S; ++j) {
                const int d = st.d1[j] - q[(size_t)j * S + tid];
                g += d > 0 ? d : 0;
            }
            v = -g;
        }
        r = modes_block_argmin(v, tid, st.sv, st.si);
        if (r.v >= 0) break;                                              // gain 0, or no sample left: fewer than M modes
        if (tid == 0) { st.med[c] = r.i; st.is_med[r.i] = 1; }
        filled = c + 1;
        __syncthreads();
        modes_update_near(st, q, S, filled);
    }
    long long cost = modes_block_sum(tid < S ? (long long)st.d1[tid] : 0, st.sv);

    // SWAP: best improvement over every (slot, non-medoid), candidate c * S + h in the order of the tie rule
    int swaps = 0, converged = 0;
    while (true) {
        v = LLONG_MAX;
        int vi = INT_MAX;
        for (int cand = tid; cand < filled * S; cand += 256) {
            const int c = cand / S, h = cand - c * S;
            if (st.is_med[h]) continue;
            long long t = 0;
            for (int j = 0; j < S; ++j) {
                const int dq = q[(size_t)j * S + h];
                const int base = st.slot[j] == c ? st.d2[j] : st.d1[j];
                t += dq < base ? dq : base;
            }
            if (modes_better(t, cand, v, vi)) { v = t; vi = cand; }
        }
        r = modes_block_argmin(v, vi, st.sv, st.si);
        if (!(r.v < cost)) { converged = 1; break; }
        if (swaps >= max_swaps) break;
        if (tid == 0) {
            const int c = r.i / S, h = r.i - c * S;
            st.is_med[st.med[c]] = 0;
            st.med[c] = h;
            st.is_med[h] = 1;
        }
        __syncthreads();
        modes_update_near(st, q, S, filled);
        cost = r.v;
        ++swaps;
    }

    // sizes and spreads per slot, then the output order: size descending, the lower medoid first
    __shared__ int32_t s_size[MODES_MAX_M];
    __shared__ long long s_spread[MODES_MAX_M];
    if (tid < MODES_MAX_M) {
        int n = 0;
        long long sp = 0;
        if (tid < filled)
            for (int j = 0; j < S; ++j)
                if (st.slot[j] == tid) { ++n; sp += st.d1[j]; }
        s_size[tid] = n; s_spread[tid] = sp;
    }
    __syncthreads();
    if (tid < filled) {
        int before = 0;
        for (int c = 0; c < filled; ++c)
            if (c != tid && (s_size[c] > s_size[tid] || (s_size[c] == s_size[tid] && st.med[c] < st.med[tid]))) ++before;
        st.rank[tid] = before;                                            // (medoids are distinct samples: a total order)
    }
    __syncthreads();
    if (tid < M) {
        if (tid < filled) {
            const int o = st.rank[tid];
            medoid[(size_t)b * M + o] = st.med[tid];
            size[(size_t)b * M + o] = s_size[tid];
            spread[(size_t)b * M + o] = s_spread[tid];
        } else {
            medoid[(size_t)b * M + tid] = -1;
            size[(size_t)b * M + tid] = 0;
            spread[(size_t)b * M + tid] = 0;
        }
    }
    if (tid < S) assign[(size_t)b * S + tid] = st.rank[st.slot[tid]];
    if (tid == 0) { cost_out[b] = cost; swaps_out[b] = swaps; converged_out[b] = converged; }
}

// ------------------------------------------------------------------------------------------------ per-mode maps
// -p log p in fp64, 0 for p <= 0
__device__ __forceinline__ double modes_neg_plogp(double p) { return p > 0.0 ? -p * log(p) : 0.0; }

template <int KP>
__global__ __launch_bounds__(256) void k_modes_maps(const uint8_t* __restrict__ a, const int32_t* __restrict__ assign,
                                                    const int32_t* __restrict__ size, int S, int M, int64_t HW, int K,
                                                    uint8_t* __restrict__ vote, int32_t* __restrict__ counts, float* __restrict__ entropy) {
    __shared__ int32_t member[MODES_MAX_S];
    const int b = blockIdx.z, m = blockIdx.y;
    member[threadIdx.x] = threadIdx.x < S && assign[(size_t)b * S + threadIdx.x] == m ? 1 : 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int n = size[(size_t)b * M + m];
    const size_t o = ((size_t)b * M + m) * HW + p;
    int cnt[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = 0;
    if (n > 0) {
        const uint8_t* src = a + (size_t)b * S * HW + p;
        for (int s = 0; s < S; ++s) {
            if (!member[s]) continue;                                     // (the same for every thread of the block)
            const int c = src[(size_t)s * HW];
#pragma unroll
            for (int k = 0; k < KP; ++k) cnt[k] += c == k ? 1 : 0;
        }
    }
    int best = 0, bi = 0;
    double h = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k < K) {
            if (counts) counts[o * K + k] = cnt[k];
            if (k == 0 || cnt[k] > best) { best = cnt[k]; bi = k; }
            if (n > 0) h += modes_neg_plogp((double)cnt[k] / (double)n);
        }
    }
    vote[o] = n > 0 ? (uint8_t)bi : (uint8_t)255;
    if (entropy) entropy[o] = (float)h;
}

static int modes_check_shape(const char* what, int B, int S, int K, int HW) {
    CCDM_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d outside [0,65535]", what, B);
    CCDM_REQUIRE(S >= 1 && S <= MODES_MAX_S, "%s: S=%d outside [1,%d]", what, S, MODES_MAX_S);
    CCDM_REQUIRE(K >= 2 && K <= MODES_MAX_K, "%s: K=%d outside [2,%d]", what, K, MODES_MAX_K);
    CCDM_REQUIRE(HW >= 1, "%s: HW=%d", what, HW);
    return 0;
}

}  // namespace ccdm

extern "C" int ccdm_modes_distance(const uint8_t* a, int B, int S, int HW, int K, int32_t* ws, int32_t* Q, void* stream) {
    using namespace ccdm;
    if (modes_check_shape("modes_distance", B, S, K, HW) < 0) return -1;
    CCDM_REQUIRE(a && ws && Q, "modes_distance: null pointer");
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int aligned = (HW % 4 == 0 && (uintptr_t)a % 4 == 0) ? 1 : 0;
    const int ntile = cdiv(S, MODES_TILE);
    // the pixels are split over up to 64 workgroups per tile of pairs, two chunks each where there are that many: blocks to fill the chip with
    const int nchunk = cdiv(HW, MODES_CHUNK);
    int nsplit = (nchunk + 1) / 2 < 64 ? (nchunk + 1) / 2 : 64;
    const int per_split = cdiv(nchunk, nsplit);
    nsplit = cdiv(nchunk, per_split);
    if (hipMemsetAsync(ws, 0, (size_t)B * S * S * K * sizeof(int32_t), s) != hipSuccess) return fail("modes_distance: cannot clear the workspace");
    const dim3 gp((unsigned)(ntile * (ntile + 1) / 2), (unsigned)B, (unsigned)nsplit), gf((unsigned)cdiv(S * S, 256), (unsigned)B), t(256);
    if (K <= 2) hipLaunchKernelGGL(k_modes_pairs<2>, gp, t, 0, s, a, S, (int64_t)HW, K, ntile, per_split, aligned, ws);
    else if (K <= 8) hipLaunchKernelGGL(k_modes_pairs<8>, gp, t, 0, s, a, S, (int64_t)HW, K, ntile, per_split, aligned, ws);
    else hipLaunchKernelGGL(k_modes_pairs<32>, gp, t, 0, s, a, S, (int64_t)HW, K, ntile, per_split, aligned, ws);
    hipLaunchKernelGGL(k_modes_finish, gf, t, 0, s, ws, S, K, Q);
    CCDM_CHECK_LAUNCH("modes_distance");
    return 0;
}

extern "C" int ccdm_modes_pam(const int32_t* Q, int B, int S, int M, int max_swaps, int32_t* medoid, int32_t* assign, int32_t* size,
                              int64_t* spread, int64_t* cost, int32_t* swaps, int32_t* converged, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(B >= 0 && B <= 65535, "modes_pam: B=%d outside [0,65535]", B);
    CCDM_REQUIRE(S >= 1 && S <= MODES_MAX_S, "modes_pam: S=%d outside [1,%d]", S, MODES_MAX_S);
    CCDM_REQUIRE(M >= 1 && M <= MODES_MAX_M, "modes_pam: M=%d outside [1,%d]", M, MODES_MAX_M);
    CCDM_REQUIRE(max_swaps >= 0, "modes_pam: max_swaps=%d", max_swaps);
    CCDM_REQUIRE(Q && medoid && assign && size && spread && cost && swaps && converged, "modes_pam: null pointer");
    CCDM_REQUIRE((uintptr_t)spread % 8 == 0 && (uintptr_t)cost % 8 == 0, "modes_pam: spread and cost must be 8-byte aligned");
    if (B == 0) return 0;
    const int in_lds = S <= MODES_LDS_S ? 1 : 0;
    const size_t lds = in_lds ? (size_t)S * S * sizeof(int32_t) : 0;
    static bool reserved = false;                     // more than 48 KB of dynamic LDS is asked for once (the static LDS comes on top)
    if (lds > 48 * 1024 && !reserved) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_modes_pam), hipFuncAttributeMaxDynamicSharedMemorySize,
                                MODES_LDS_S * MODES_LDS_S * (int)sizeof(int32_t)) != hipSuccess)
            return fail("modes_pam: cannot reserve %d bytes of LDS", MODES_LDS_S * MODES_LDS_S * (int)sizeof(int32_t));
        reserved = true;
    }
    hipLaunchKernelGGL(k_modes_pam, dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream, Q, S, M, max_swaps, in_lds, medoid, assign, size,
                       reinterpret_cast<long long*>(spread), reinterpret_cast<long long*>(cost), swaps, converged);
    CCDM_CHECK_LAUNCH("modes_pam");
    return 0;
}

extern "C" int ccdm_modes_maps(const uint8_t* a, const int32_t* assign, const int32_t* size, int B, int S, int M, int HW, int K, uint8_t* vote,
                               int32_t* counts, float* entropy, void* stream) {
    using namespace ccdm;
    if (modes_check_shape("modes_maps", B, S, K, HW) < 0) return -1;
    CCDM_REQUIRE(M >= 1 && M <= MODES_MAX_M, "modes_maps: M=%d outside [1,%d]", M, MODES_MAX_M);
    CCDM_REQUIRE(a && assign && size && vote, "modes_maps: null pointer");
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)(((int64_t)HW + 255) / 256), (unsigned)M, (unsigned)B), t(256);
    if (K <= 2) hipLaunchKernelGGL(k_modes_maps<2>, g, t, 0, s, a, assign, size, S, M, (int64_t)HW, K, vote, counts, entropy);
    else if (K <= 8) hipLaunchKernelGGL(k_modes_maps<8>, g, t, 0, s, a, assign, size, S, M, (int64_t)HW, K, vote, counts, entropy);
    else hipLaunchKernelGGL(k_modes_maps<32>, g, t, 0, s, a, assign, size, S, M, (int64_t)HW, K, vote, counts, entropy);
    CCDM_CHECK_LAUNCH("modes_maps");
    return 0;
}
