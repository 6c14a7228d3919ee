// LIDC soft-label scores, device part (beyond the reference, whose LIDC scores are all set scores): per pixel the number of
// samples n_k and the number of raters m_k that say class k, counted into joint[b][k][n_k][m_k], and the integer moments of the
// two Gini impurities u = S^2 - sum n_k^2, v = L^2 - sum m_k^2.  Calibration against the raters' soft label, the Brier score, the
// cross-entropy, thresholded soft Dice and the uncertainty correlation follow on the host from those few thousand integers
// (metrics.soft_label_scores_from_counts).
//
// The kernel is a byte stream: B*(S+L)*HW bytes in, read once.  A lane takes four consecutive pixels (one dword per map) when
// HW % 4 == 0 and both maps are 4-byte aligned, one pixel (a byte per map) otherwise; the host picks.  S, L <= 255, so the four
// pixels' counts of one class are four bytes of one register: a dword of class bytes is compared with class k in all four bytes
// at once (xor with k in every byte, then "byte != 0" by the carry of 0x7f + low seven bits), and the register counts the bytes
// that do NOT match (at most S <= 255 per byte, no carry into the neighbour); n_k = S - that byte.  A byte >= K matches no class.
// Class ladder 2 / 8 / 32 like k_pair_counts: 2 * KP count registers.
//
// Everything is an integer: exact in any order, two identical calls are bit-identical.  Reduction before atomics:
//   joint    one LDS add per (pixel, class) into the block's own [K][S+1][L+1] int32 table (dynamic LDS, <= 64 KB).  Most of a
//            LIDC image is background, where every lane of a wave holds the same cell: the cell of the wave's first lane is
//            added once with the number of lanes that share it, the other lanes add their own.  Non-zero entries go to the
//            image's table in global memory once per block;
//   moments  five 64-bit sums per lane (u^2 <= 255^4 < 2^32), added over the wave by shuffles, five global adds per wave.
// Several blocks per image (a block walks chunks of one image), so one image fills more than one CU.
#include "ccdm_common.h"

namespace ccdm {

constexpr int LSC_MAX_ENTRIES = 16384;       // one image-class table as int32 in 64 KB of LDS

// 0x01 in every byte of w that differs from the byte k4 holds four times
__device__ __forceinline__ uint32_t lsc_bytes_differ(uint32_t w, uint32_t k4) {
    const uint32_t x = w ^ k4;
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) >> 7 & 0x01010101u;
}

// tab[key] += 1 for every lane with `valid`; the first valid lane's key is added once for all lanes that share it.  Wave-uniform call.
__device__ __forceinline__ void lsc_count(int32_t* tab, bool valid, int key, int lane) {
    const unsigned long long todo = __ballot(valid);
    if (!todo) return;
    const int lead = __ffsll((long long)todo) - 1;
    const int first = __shfl(key, lead);
    const unsigned long long same = __ballot(valid && key == first);
    if (lane == lead) atomicAdd(&tab[first], (int)__popcll(same));
    else if (valid && key != first) atomicAdd(&tab[key], 1);
}

__device__ __forceinline__ unsigned long long lsc_wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// VEC: a lane's unit is 4 pixels (one dword per map), else 1 pixel.  Grid: blocks_per_image blocks for each image.
template <int KP, bool VEC>
__global__ __launch_bounds__(256) void k_lidcscore(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters, int S, int L, int HW,
                                                   int K, int blocks_per_image, int32_t* __restrict__ joint,
                                                   unsigned long long* __restrict__ moments) {
    extern __shared__ int32_t lsc_tab[];
    constexpr int NPIX = VEC ? 4 : 1;
    const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
    const int entries = K * (S + 1) * (L + 1);
    const int lane = threadIdx.x & 63;
    if (joint) {
        for (int e = threadIdx.x; e < entries; e += blockDim.x) lsc_tab[e] = 0;
        __syncthreads();
    }
    const uint8_t* ps = samples + (size_t)b * S * HW;
    const uint8_t* pr = raters + (size_t)b * L * HW;
    const int units = HW / NPIX;
    unsigned long long su = 0, sv = 0, suu = 0, svv = 0, suv = 0;

    // wave-uniform trip count; 64-bit: the last step may pass 2^31
    for (long long base = (long long)chunk * blockDim.x; base < units; base += (long long)blocks_per_image * blockDim.x) {
        const bool valid = base + threadIdx.x < units;
        const size_t at = (size_t)(valid ? base + threadIdx.x : units - 1) * NPIX;        // a lane past the end re-reads the last unit, counts nothing
        uint32_t ns[KP], ms[KP];         // per class: the maps that do NOT say it, one byte per pixel
#pragma unroll
        for (int k = 0; k < KP; ++k) { ns[k] = 0; ms[k] = 0; }
#pragma unroll 8
        for (int s = 0; s < S; ++s) {
            const uint8_t* q = ps + (size_t)s * HW + at;
            const uint32_t w = VEC ? *reinterpret_cast<const uint32_t*>(q) : (uint32_t)*q;
#pragma unroll
            for (int k = 0; k < KP; ++k) ns[k] += lsc_bytes_differ(w, 0x01010101u * k);
        }
        for (int l = 0; l < L; ++l) {
            const uint8_t* q = pr + (size_t)l * HW + at;
            const uint32_t w = VEC ? *reinterpret_cast<const uint32_t*>(q) : (uint32_t)*q;
#pragma unroll
            for (int k = 0; k < KP; ++k) ms[k] += lsc_bytes_differ(w, 0x01010101u * k);
        }
#pragma unroll
        for (int j = 0; j < NPIX; ++j) {
            int u = S * S, v = L * L;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (k < K) {             // wave-uniform
                    const int n = S - (int)(ns[k] >> (8 * j) & 0xFFu), m = L - (int)(ms[k] >> (8 * j) & 0xFFu);      // 0 <= n <= S, 0 <= m <= L
                    u -= n * n;
                    v -= m * m;
                    if (joint) lsc_count(lsc_tab, valid, (k * (S + 1) + n) * (L + 1) + m, lane);
                }
            }
            if (valid) {
                const unsigned long long uu = (unsigned)u, vv = (unsigned)v;
                su += uu; sv += vv; suu += uu * uu; svv += vv * vv; suv += uu * vv;
            }
        }
    }

    if (moments) {
        const unsigned long long t[5] = {lsc_wave_sum(su), lsc_wave_sum(sv), lsc_wave_sum(suu), lsc_wave_sum(svv), lsc_wave_sum(suv)};
        if (lane < 5) {
            const unsigned long long x = lane == 0 ? t[0] : lane == 1 ? t[1] : lane == 2 ? t[2] : lane == 3 ? t[3] : t[4];
            if (x) atomicAdd(&moments[(size_t)b * 5 + lane], x);
        }
    }
    if (joint) {
        __syncthreads();
        int32_t* out = joint + (size_t)b * entries;
        for (int e = threadIdx.x; e < entries; e += blockDim.x) {
            const int x = lsc_tab[e];
            if (x) atomicAdd(&out[e], x);
        }
    }
}

template <int KP>
static void lsc_launch(bool vec, int blocks, int threads, size_t lds, hipStream_t st, const uint8_t* samples, const uint8_t* raters, int S, int L,
                       int HW, int K, int bpi, int32_t* joint, unsigned long long* moments) {
    if (vec) hipLaunchKernelGGL((k_lidcscore<KP, true>), dim3(blocks), dim3(threads), lds, st, samples, raters, S, L, HW, K, bpi, joint, moments);
    else hipLaunchKernelGGL((k_lidcscore<KP, false>), dim3(blocks), dim3(threads), lds, st, samples, raters, S, L, HW, K, bpi, joint, moments);
}

}  // namespace ccdm

extern "C" int ccdm_lidcscore(const uint8_t* samples, const uint8_t* raters, int B, int S, int L, int HW, int K, int32_t* joint,
                              int64_t* moments, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(joint || moments, "lidcscore: joint and moments are both NULL (at least one output)");
    CCDM_REQUIRE(S >= 1 && S <= 255, "lidcscore: S=%d outside [1,255]", S);
    CCDM_REQUIRE(L >= 1 && L <= 255, "lidcscore: L=%d outside [1,255]", L);
    CCDM_REQUIRE(K >= 1 && K <= 32, "lidcscore: K=%d outside [1,32]", K);
    CCDM_REQUIRE(HW > 0, "lidcscore: HW=%d outside (0, 2^31)", HW);
    CCDM_REQUIRE((long long)K * (S + 1) * (L + 1) <= LSC_MAX_ENTRIES, "lidcscore: K*(S+1)*(L+1)=%lld above %d (one image's table in LDS)",
                 (long long)K * (S + 1) * (L + 1), LSC_MAX_ENTRIES);
    CCDM_REQUIRE(B >= 0, "lidcscore: B=%d", B);
    if (B == 0) return 0;
    CCDM_REQUIRE(samples && raters, "lidcscore: null pointer");
    const int entries = K * (S + 1) * (L + 1);
    const bool vec = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(raters)) & 3) == 0;
    const int units = vec ? HW / 4 : HW;
    // 256-thread blocks once they cover the card's 256 CUs, single waves below that; a block walks further chunks of its image
    // when the image has more than its share of 2048 blocks
    const int threads = (long long)B * cdiv(units, 256) >= 256 ? 256 : 64;
    int bpi = cdiv(units, threads);
    if (bpi > (2048 + B - 1) / B) bpi = (2048 + B - 1) / B;
    CCDM_REQUIRE((long long)B * bpi <= 0x7fffffff, "lidcscore: B=%d images", B);
    hipStream_t st = (hipStream_t)stream;
    if ((joint && hipMemsetAsync(joint, 0, (size_t)B * entries * sizeof(int32_t), st) != hipSuccess) ||
        (moments && hipMemsetAsync(moments, 0, (size_t)B * 5 * sizeof(int64_t), st) != hipSuccess))
        return fail("lidcscore: clearing the outputs failed");
    const size_t lds = joint ? (size_t)entries * sizeof(int32_t) : 0;
    unsigned long long* mom = reinterpret_cast<unsigned long long*>(moments);
    if (K <= 2) lsc_launch<2>(vec, B * bpi, threads, lds, st, samples, raters, S, L, HW, K, bpi, joint, mom);
    else if (K <= 8) lsc_launch<8>(vec, B * bpi, threads, lds, st, samples, raters, S, L, HW, K, bpi, joint, mom);
    else lsc_launch<32>(vec, B * bpi, threads, lds, st, samples, raters, S, L, HW, K, bpi, joint, mom);
    CCDM_CHECK_LAUNCH("lidcscore");
    return 0;
}
