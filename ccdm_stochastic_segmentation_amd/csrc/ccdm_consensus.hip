// Metric-optimal consensus of a multi-sample prediction (metrics.sample_consensus, DenoisingModel.predict_consensus): among the S + 1
// thresholded frequency maps of an image and class, the one with the largest expected IoU (or Dice) under the samples themselves, in
// exact integers.  The definition (the candidate masks P_j, the fixed-point terms, the tie rules, the label composition) is in
// include/ccdm_hip.h.
//
//   k_cons_count   one lane per four pixels: the stack is streamed once, the counts of the scored classes kept as four byte counters to
//                  the register (S <= 255: a byte holds them), the frequency planes written
//   k_cons_hist    one workgroup per (image, class, group of 16 samples, share of the pixels): h[s][m] = #{p : a_s[p] == k and n[p] == m} of
//                  its samples in an LDS table (integer atomics), flushed to the workspace with global integer atomics (exact in any order);
//                  pixels no sample gives the class are skipped before a sample is read
//   k_cons_select  one workgroup per (image, class): I_{j,s} as suffix sums of the rows of h (in place, a wave to the row), A_j from the
//                  column sums of h (a pixel with n == m is counted by m samples), the terms of threshold j summed in int64 by as many
//                  threads as the block has for it, a block argmax with the index for the tie rule
//   k_cons_maps    one lane per four pixels: mask and label from the frequency planes and the thresholds, read from the device
#include <climits>

#include "ccdm_common.h"

namespace ccdm {

constexpr int CONS_MAX_S = 255, CONS_MAX_K = 32;
constexpr int CONS_ONE_LOG2 = 20;
constexpr int CONS_COUNT_THREADS = 64;               // one wave: 256 pixels to the workgroup, blocks to spread a 128 x 128 map over the chip with
constexpr int CONS_CHUNK = 1024;                     // pixels a 256-thread workgroup takes at once: four to the lane
constexpr int CONS_GROUP = 16;                       // samples of one workgroup of k_cons_hist: an LDS table of 16 x 256 words at most, 16 KB
constexpr int CONS_SELECT_THREADS = 1024;             // k_cons_select: 16 waves to the (image, class)
constexpr int CONS_MAX_SHARES = 64;                  // workgroups the pixels of one (image, class, group) are split over

// the four pixels at p .. p + 3 of a plane as one dword; a pixel at or beyond HW reads as 0 (class 0 and frequency 0: never counted)
__device__ __forceinline__ uint32_t cons_load4(const uint8_t* __restrict__ plane, int64_t p, int64_t HW, bool aligned) {
    if (aligned && p + 4 <= HW) return *reinterpret_cast<const uint32_t*>(plane + p);
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (p + e < HW) w |= (uint32_t)plane[p + e] << (8 * e);
    return w;
}

__device__ __forceinline__ void cons_store4(uint8_t* __restrict__ plane, int64_t p, int64_t HW, bool aligned, uint32_t w) {
    if (aligned && p + 4 <= HW) { *reinterpret_cast<uint32_t*>(plane + p) = w; return; }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (p + e < HW) plane[p + e] = (uint8_t)(w >> (8 * e));
}

// 1 in every byte of the result whose byte of z is zero (exact per byte: (z & 0x7f) + 0x7f never carries into the next byte)
__device__ __forceinline__ uint32_t cons_zero_bytes(uint32_t z) {
    const uint32_t nz = ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z;
    return (~nz & 0x80808080u) >> 7;
}

template <int KP>
__global__ __launch_bounds__(CONS_COUNT_THREADS) void k_cons_count(const uint8_t* __restrict__ a, int S, int64_t HW, int K, int a_aligned,
                                                                    int f_aligned, uint8_t* __restrict__ freq) {
    const int b = blockIdx.y;
    const int64_t p = ((int64_t)blockIdx.x * CONS_COUNT_THREADS + threadIdx.x) * 4;
    if (p >= HW) return;
    uint32_t cnt[KP];                                                     // four byte counters each: at most S <= 255 to the byte
#pragma unroll
    for (int k = 0; k < KP; ++k) cnt[k] = 0;
    const uint8_t* img = a + (size_t)b * S * HW;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
        const uint32_t w = cons_load4(img + (size_t)s * HW, p, HW, a_aligned != 0);
#pragma unroll
        for (int k = 1; k < KP; ++k)
            if (k < K) cnt[k] += cons_zero_bytes(w ^ (0x01010101u * k));
    }
#pragma unroll
    for (int k = 1; k < KP; ++k)
        if (k < K) cons_store4(freq + ((size_t)b * (K - 1) + (k - 1)) * HW, p, HW, f_aligned != 0, cnt[k]);
}

__global__ __launch_bounds__(256) void k_cons_hist(const uint8_t* __restrict__ a, const uint8_t* __restrict__ freq, int S, int64_t HW, int K,
                                                   int ngroup, int chunks_per_share, int a_aligned, int f_aligned,
                                                   int32_t* __restrict__ h) {
    __shared__ int32_t cons_tab[CONS_GROUP * (CONS_MAX_S + 1)];           // [ns][S + 1]
    const int tid = threadIdx.x, b = blockIdx.z, c = blockIdx.y / ngroup, g = blockIdx.y - c * ngroup;
    const int C = K - 1, W = S + 1, s0 = g * CONS_GROUP;
    const int ns = S - s0 < CONS_GROUP ? S - s0 : CONS_GROUP;
    for (int e = tid; e < ns * W; e += 256) cons_tab[e] = 0;
    __syncthreads();
    const uint8_t* plane = freq + ((size_t)b * C + c) * HW;
    const uint8_t* img = a + ((size_t)b * S + s0) * HW;
    const uint32_t kk = 0x01010101u * (uint32_t)(c + 1);
    const int64_t nchunk = (HW + CONS_CHUNK - 1) / CONS_CHUNK;
    const int64_t c0 = (int64_t)blockIdx.x * chunks_per_share;
    const int64_t c1 = c0 + chunks_per_share < nchunk ? c0 + chunks_per_share : nchunk;
    for (int64_t ch = c0; ch < c1; ++ch) {
        const int64_t p = (ch * 256 + tid) * 4;
        if (p >= HW) continue;
        const uint32_t nw = cons_load4(plane, p, HW, f_aligned != 0);
        if (nw == 0) continue;                                            // no sample gives the class at these four pixels
        for (int i0 = 0; i0 < ns; i0 += 8) {                              // eight samples to the round: their loads are in flight together
            uint32_t z[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                z[u] = i0 + u < ns ? cons_zero_bytes(cons_load4(img + (size_t)(i0 + u) * HW, p, HW, a_aligned != 0) ^ kk) : 0u;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (z[u] == 0) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e)                               // (n <= S: k_cons_count counted S maps)
                    if ((z[u] >> (8 * e)) & 1u) atomicAdd(&cons_tab[(i0 + u) * W + (int)((nw >> (8 * e)) & 255u)], 1);
            }
        }
    }
    __syncthreads();
    int32_t* o = h + (((size_t)b * C + c) * S + s0) * W;                  // the rows of the group lie one after the other
    for (int e = tid; e < ns * W; e += 256) {
        const int v = cons_tab[e];
        if (v != 0) atomicAdd(o + e, v);
    }
}

// (value, index) with the tie rule: the larger value, then the lower index
__device__ __forceinline__ bool cons_better(long long v, int i, long long bv, int bi) { return v > bv || (v == bv && i < bi); }

// argmax over the threads of a block of CONS_SELECT_THREADS; every thread calls it, thread 0 uses the result
__device__ __forceinline__ int cons_block_argmax(long long v, int i, long long* sv, int* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (cons_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    long long rv = sv[0];
    int ri = si[0];
#pragma unroll
    for (int w = 1; w < CONS_SELECT_THREADS / 64; ++w)
        if (cons_better(sv[w], si[w], rv, ri)) { rv = sv[w]; ri = si[w]; }
    __syncthreads();                                                      // (the stage is free again)
    return ri;
}

// N / D rounded down for D > 0, 0 <= N < 2^54 and N / D < 2^22: the fp64 quotient is within one of it (N and the division are each
// off by a relative 2^-52 at most), the remainder in int64 says which way.  (The 64-bit integer division is a long software routine on this hardware)
__device__ __forceinline__ long long cons_floor_div(long long N, long long D) {
    long long q = (long long)((double)N / (double)D);
    const long long r = N - q * D;
    if (r < 0) --q;
    else if (r >= D) ++q;
    return q;
}

// the quotient num / den in units of 2^-20, round half up; 2^20 where den == 0 (the reference's 0/0 = 1).  num <= den < 2^32
__device__ __forceinline__ long long cons_term(long long num, long long den) {
    return den == 0 ? 1ll << CONS_ONE_LOG2 : cons_floor_div((2 * num << CONS_ONE_LOG2) + den, 2 * den);
}

// inclusive suffix sum over the 64 lanes of a wave: the lane's value and those of the lanes above it
template <typename T>
__device__ __forceinline__ T cons_wave_suffix(T t) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T x = __shfl_down(t, off);
        if (lane + off < 64) t += x;
    }
    return t;
}

// One workgroup of 16 waves per (image, class): with S = 100 there are two of them on the chip and each runs 2 S (S + 1) divisions, so the
// launch is a chain of latencies; the width shortens every link of it
__global__ __launch_bounds__(CONS_SELECT_THREADS) void k_cons_select(int32_t* h, int S, long long* __restrict__ curve, int32_t* __restrict__ best) {
    constexpr int WAVES = CONS_SELECT_THREADS / 64;
    __shared__ unsigned long long col[CONS_MAX_S + 1];                    // the column sums of h
    __shared__ unsigned long long acc[2][CONS_MAX_S + 1];                 // the curve values, summed over the parts of the samples
    __shared__ long long A[CONS_MAX_S + 2];                               // A[j] = |P_j|, j = 1 .. S + 1
    __shared__ long long sv[WAVES];
    __shared__ int si[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = S + 1;
    int32_t* hc = h + (size_t)blockIdx.x * S * W;                         // [S][S + 1] of this (image, class)
    if (tid <= CONS_MAX_S) { col[tid] = 0; acc[0][tid] = 0; acc[1][tid] = 0; }
    __syncthreads();
    // a wave to the row, four words to the lane: row s becomes its suffix sums in place, h[s][j] = I_{j,s} and h[s][1] = n_s (a dependent
    // chain of S loads to the thread otherwise); the lane keeps the sums of the words as they were
    const int m0 = 4 * lane;
    unsigned long long cs[4] = {0, 0, 0, 0};
    for (int s = wave; s < S; s += 4 * WAVES) {                           // four rows to the round: their loads are in flight together
        int v[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[r][e] = (s + WAVES * r < S && m0 + e < W) ? hc[(size_t)(s + WAVES * r) * W + m0 + e] : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) cs[e] += (unsigned long long)v[r][e];
            v[r][2] += v[r][3]; v[r][1] += v[r][2]; v[r][0] += v[r][1];
            const int above = cons_wave_suffix(v[r][0]) - v[r][0];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s + WAVES * r < S && m0 + e < W) hc[(size_t)(s + WAVES * r) * W + m0 + e] = v[r][e] + above;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (cs[e] != 0) atomicAdd(&col[m0 + e], cs[e]);
    __syncthreads();
    // the pixels with n == tid: each was counted by tid samples; A as the suffix sums over the first four waves
    long long t = 0;
    if (tid >= 1 && tid <= S) t = (long long)col[tid] / tid;
    t = cons_wave_suffix(t);
    if (lane == 0) sv[wave] = t;
    __syncthreads();
    if (tid <= CONS_MAX_S) {
        for (int w = wave + 1; w < 4; ++w) t += sv[w];
        A[tid] = t;
    }
    if (tid == 0) A[CONS_MAX_S + 1] = 0;                                  // (j = S + 1 = 256; a smaller S + 1 got its 0 above)
    __syncthreads();                                                      // (also: the rows are written, sv is free again)
    // thread (part, j): the samples part, part + parts, ... of threshold j
    const int parts = CONS_SELECT_THREADS / W, part = tid / W, j = tid - part * W + 1;
    if (part < parts) {
        const long long Aj = A[j];
        long long iou = 0, dice = 0;
#pragma unroll 4
        for (int s = part; s < S; s += parts) {
            const long long I = j <= S ? hc[(size_t)s * W + j] : 0, n = hc[(size_t)s * W + 1];
            iou += cons_term(I, Aj + n - I);
            dice += cons_term(2 * I, Aj + n);
        }
        atomicAdd(&acc[0][j - 1], (unsigned long long)iou);
        atomicAdd(&acc[1][j - 1], (unsigned long long)dice);
    }
    __syncthreads();
    long long iou = LLONG_MIN, dice = LLONG_MIN;
    if (tid < W) {
        iou = (long long)acc[0][tid];
        dice = (long long)acc[1][tid];
        long long* o = curve + (size_t)blockIdx.x * 2 * W;
        o[tid] = iou;
        o[W + tid] = dice;
    }
    const int bi = cons_block_argmax(iou, tid + 1, sv, si);
    const int bd = cons_block_argmax(dice, tid + 1, sv, si);
    if (tid == 0) { best[(size_t)blockIdx.x * 2] = bi; best[(size_t)blockIdx.x * 2 + 1] = bd; }
}

__global__ __launch_bounds__(256) void k_cons_maps(const uint8_t* __restrict__ freq, const int32_t* __restrict__ best, int C, int64_t HW, int metric,
                                                   int f_aligned, int m_aligned, int l_aligned, uint8_t* __restrict__ mask,
                                                   uint8_t* __restrict__ label) {
    __shared__ int thr[CONS_MAX_K];
    const int b = blockIdx.y;
    if (threadIdx.x < C) thr[threadIdx.x] = best[((size_t)b * C + threadIdx.x) * 2 + metric];
    __syncthreads();
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= HW) return;
    uint32_t top[4] = {0, 0, 0, 0}, lab = 0;                              // per pixel: the largest n among the masks that hold it, and its class
    for (int c = 0; c < C; ++c) {
        const uint32_t nw = cons_load4(freq + ((size_t)b * C + c) * HW, p, HW, f_aligned != 0);
        const uint32_t t = (uint32_t)thr[c];
        uint32_t mw = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t n = (nw >> (8 * e)) & 255u;
            if (n >= t) {                                                 // (t >= 1: n >= 1 here; a later class needs a larger n: the lowest wins ties)
                mw |= 1u << (8 * e);
                if (n > top[e]) { top[e] = n; lab = (lab & ~(255u << (8 * e))) | ((uint32_t)(c + 1) << (8 * e)); }
            }
        }
        if (mask) cons_store4(mask + ((size_t)b * C + c) * HW, p, HW, m_aligned != 0, mw);
    }
    if (label) cons_store4(label + (size_t)b * HW, p, HW, l_aligned != 0, lab);
}

static int cons_check_shape(const char* what, int B, int S, int HW, int K) {
    CCDM_REQUIRE(K >= 2 && K <= CONS_MAX_K, "%s: K=%d outside [2,%d]", what, K, CONS_MAX_K);
    CCDM_REQUIRE(S >= 1 && S <= CONS_MAX_S, "%s: S=%d outside [1,%d]", what, S, CONS_MAX_S);
    CCDM_REQUIRE(HW >= 1, "%s: HW=%d below 1", what, HW);
    CCDM_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d outside [0,65535]", what, B);
    return 0;
}

static bool cons_aligned4(const void* p, int HW) { return HW % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace ccdm

extern "C" size_t ccdm_consensus_workspace_bytes(int B, int S, int HW, int K) {
    if (B <= 0 || S <= 0 || HW <= 0 || K < 2) return 0;
    return (size_t)B * (K - 1) * S * (S + 1) * sizeof(int32_t);
}

extern "C" int ccdm_consensus(const uint8_t* samples, int B, int S, int HW, int K, uint8_t* freq, int64_t* curve, int32_t* best, void* workspace,
                              uint64_t workspace_bytes, void* stream) {
    using namespace ccdm;
    if (cons_check_shape("consensus", B, S, HW, K) < 0) return -1;
    CCDM_REQUIRE(samples, "consensus: samples is a null pointer");
    CCDM_REQUIRE(freq, "consensus: freq is a null pointer");
    CCDM_REQUIRE(curve, "consensus: curve is a null pointer");
    CCDM_REQUIRE(best, "consensus: best is a null pointer");
    CCDM_REQUIRE(workspace, "consensus: workspace is a null pointer");
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(curve) & 7) == 0, "consensus: curve must be 8-byte aligned");
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(best) & 3) == 0, "consensus: best must be 4-byte aligned");
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "consensus: workspace must be 4-byte aligned");
    const size_t need = ccdm_consensus_workspace_bytes(B, S, HW, K);
    CCDM_REQUIRE(workspace_bytes >= need, "consensus: workspace_bytes=%llu, %zu needed", (unsigned long long)workspace_bytes, need);
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int C = K - 1;
    const int a_aligned = cons_aligned4(samples, HW) ? 1 : 0, f_aligned = cons_aligned4(freq, HW) ? 1 : 0;
    int32_t* h = static_cast<int32_t*>(workspace);
    if (hipMemsetAsync(h, 0, need, st) != hipSuccess) return fail("consensus: cannot clear the workspace");
    const dim3 gc((unsigned)(((int64_t)HW + 4 * CONS_COUNT_THREADS - 1) / (4 * CONS_COUNT_THREADS)), (unsigned)B), tc(CONS_COUNT_THREADS);
    if (K <= 2) hipLaunchKernelGGL(k_cons_count<2>, gc, tc, 0, st, samples, S, (int64_t)HW, K, a_aligned, f_aligned, freq);
    else if (K <= 8) hipLaunchKernelGGL(k_cons_count<8>, gc, tc, 0, st, samples, S, (int64_t)HW, K, a_aligned, f_aligned, freq);
    else hipLaunchKernelGGL(k_cons_count<32>, gc, tc, 0, st, samples, S, (int64_t)HW, K, a_aligned, f_aligned, freq);
    CCDM_CHECK_LAUNCH("consensus count");
    // the pixels of an (image, class, group) are split over up to 64 workgroups, a 1024-pixel chunk each where there are no more than that
    const int ngroup = cdiv(S, CONS_GROUP);
    const int nchunk = (int)(((int64_t)HW + CONS_CHUNK - 1) / CONS_CHUNK);
    int nshare = nchunk < CONS_MAX_SHARES ? nchunk : CONS_MAX_SHARES;
    const int per_share = cdiv(nchunk, nshare);
    nshare = cdiv(nchunk, per_share);
    hipLaunchKernelGGL(k_cons_hist, dim3((unsigned)nshare, (unsigned)(C * ngroup), (unsigned)B), dim3(256), 0, st, samples, freq, S, (int64_t)HW, K,
                       ngroup, per_share, a_aligned, f_aligned, h);
    CCDM_CHECK_LAUNCH("consensus histogram");
    hipLaunchKernelGGL(k_cons_select, dim3((unsigned)(B * C)), dim3(CONS_SELECT_THREADS), 0, st, h, S, reinterpret_cast<long long*>(curve), best);
    CCDM_CHECK_LAUNCH("consensus select");
    return 0;
}

extern "C" int ccdm_consensus_maps(const uint8_t* freq, const int32_t* best, int B, int S, int HW, int K, int metric, uint8_t* mask, uint8_t* label,
                                   void* stream) {
    using namespace ccdm;
    if (cons_check_shape("consensus_maps", B, S, HW, K) < 0) return -1;
    CCDM_REQUIRE(metric == 0 || metric == 1, "consensus_maps: metric=%d (expected 0: IoU, or 1: Dice)", metric);
    CCDM_REQUIRE(freq, "consensus_maps: freq is a null pointer");
    CCDM_REQUIRE(best, "consensus_maps: best is a null pointer");
    CCDM_REQUIRE(mask || label, "consensus_maps: mask and label are both null pointers");
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(best) & 3) == 0, "consensus_maps: best must be 4-byte aligned");
    if (B == 0) return 0;
    const dim3 g((unsigned)(((int64_t)HW + CONS_CHUNK - 1) / CONS_CHUNK), (unsigned)B);
    hipLaunchKernelGGL(k_cons_maps, g, dim3(256), 0, (hipStream_t)stream, freq, best, K - 1, (int64_t)HW, metric, cons_aligned4(freq, HW) ? 1 : 0,
                       cons_aligned4(mask, HW) ? 1 : 0, cons_aligned4(label, HW) ? 1 : 0, mask, label);
    CCDM_CHECK_LAUNCH("consensus_maps");
    return 0;
}
