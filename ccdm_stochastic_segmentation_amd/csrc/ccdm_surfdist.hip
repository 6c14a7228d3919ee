// LIDC surface-distance scores, device part (beyond the reference, whose LIDC scores are all overlap scores): per (image, sample,
// rater, class) the integers and the two fp64 sums behind HD95, ASSD and the Hausdorff distance.  The definition in
// include/ccdm_hip.h is the contract; tests/test_lidc_surface_distances.py restates it with numpy and holds it against scipy.
//
// Transform stage, once per (map, class), not per pair: the exact squared Euclidean distance to the class's surface, int32 [H][W]
// in the workspace, by the separable algorithm.
//   k_surfdist_rows  one wave per (map, class, row).  A lane takes NPIX pixels of a chunk of 64 * NPIX columns (NPIX = 4: one
//                    dword per map row when W % 4 == 0 and both stacks are 4-byte aligned; NPIX = 1: bytes) and forms their
//                    surface bits from the pixel, its row neighbours and the rows above and below.  The nearest surface pixel of
//                    the row on either side: inside the lane from its own bits, inside the chunk from a ballot of the lanes that
//                    hold a surface pixel and one shuffle of the nearest such lane's bits, beyond the chunk from the wave-uniform
//                    last position of the chunks to the left (carried along) and the first position of the chunks to the right
//                    (lane k keeps chunk k's, one suffix-min over the lanes).  Writes g = that distance, SD_GINF when the row has
//                    no surface pixel.
//   k_surfdist_cols  one block per (map, class, strip of 32 columns): g of the strip as uint16 [H][32] in LDS (64 KB at H = 1024),
//                    then per pixel the lower envelope min over y' of g(x,y')^2 + (y-y')^2 by walking outwards from y until
//                    (y-y')^2 reaches the best value so far, written over g in place (a block reads and writes its strip only).
//                    A wave reads two rows of 32 consecutive uint16: 16 banks per half-wave, two lanes to a dword (a broadcast),
//                    and the two halves never conflict: no bank conflict while the lanes of a row walk in step.  An empty surface
//                    leaves every g at SD_GINF: the pixel gets SD_NONE.
// Pair stage (k_surfdist_pairs), one block per (b, i, j, c): a pixel is on a map's surface iff its transform is 0, so the block
// reads the two transforms only.  Walk 1 takes the two counts, the maximum and the two fp64 sums of sqrt(d2); then an MSB-first
// radix select over 256-bin LDS histograms finds the two order statistics, one further walk per 8-bit digit, starting at the
// highest digit the maximum has (one digit below 16 pixels, two below 256).  The two ranks share a histogram while their prefixes
// agree and take one each from where they part.  Integers are exact in any order; the fp64 sums are added per thread in pixel
// order, over the wave by a fixed butterfly, over the block in wave order: no floating atomics, two identical calls are
// bit-identical.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int SD_MAX_DIM = 1024;          // H, W: d2 < 2^21, three 8-bit digits
constexpr int SD_GINF = 32768;            // g of a row without a surface pixel: fits uint16, g^2 + (H-1)^2 fits int32
constexpr int SD_FAR = 1 << 20;           // |position| of "no surface pixel on this side"
constexpr int32_t SD_NONE = 0x7fffffff;   // d2 to an empty surface
constexpr int SD_STRIP = 32;              // columns of a column-pass block

// The surface bits of the NPIX pixels x0 .. x0 + NPIX - 1 of row y (all inside the image): bit j = pixel x0 + j has class c and one
// of its four neighbours has not (a neighbour outside the image, or a byte >= K, has no class).
template <int NPIX>
__device__ __forceinline__ uint32_t sd_surface_bits(const uint8_t* __restrict__ map, int H, int W, int y, int x0, uint32_t c) {
    const uint8_t* row = map + (size_t)y * W + x0;
    uint32_t mid, up = 0xFFFFFFFFu, dn = 0xFFFFFFFFu;
    if constexpr (NPIX == 4) {
        mid = *reinterpret_cast<const uint32_t*>(row);
        if (y > 0) up = *reinterpret_cast<const uint32_t*>(row - W);
        if (y + 1 < H) dn = *reinterpret_cast<const uint32_t*>(row + W);
    } else {
        mid = row[0];
        if (y > 0) up = *(row - W);
        if (y + 1 < H) dn = row[W];
    }
    const uint32_t left = x0 > 0 ? (uint32_t)*(row - 1) : 255u, right = x0 + NPIX < W ? (uint32_t)row[NPIX] : 255u;
    const uint32_t lf = (mid << 8) | left, rt = (mid >> 8) | (right << (8 * (NPIX - 1)));
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < NPIX; ++j) {
        const int sh = 8 * j;
        const bool in = (mid >> sh & 0xFFu) == c;
        const bool edge = (lf >> sh & 0xFFu) != c || (rt >> sh & 0xFFu) != c || (up >> sh & 0xFFu) != c || (dn >> sh & 0xFFu) != c;
        if (in && edge) bits |= 1u << j;
    }
    return bits;
}

// Map m of the B*S sample maps followed by the B*L rater maps.
__device__ __forceinline__ const uint8_t* sd_map(const uint8_t* samples, const uint8_t* raters, long long m, long long nA, size_t HW) {
    return m < nA ? samples + (size_t)m * HW : raters + (size_t)(m - nA) * HW;
}

template <int NPIX>
__global__ __launch_bounds__(256) void k_surfdist_rows(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters, long long nA,
                                                       long long nmaps, int C, int c0, int H, int W, int32_t* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = (W + 64 * NPIX - 1) / (64 * NPIX);          // <= 16
    const long long units = nmaps * C * H;
    const size_t HW = (size_t)H * W;
    // wave-uniform trip count: every lane stays active for the ballots and shuffles
    for (long long u = (long long)blockIdx.x * 4 + wave; u < units; u += (long long)gridDim.x * 4) {
        const int y = (int)(u % H);
        const long long mc = u / H;
        const uint32_t c = (uint32_t)(c0 + (int)(mc % C));
        const uint8_t* map = sd_map(samples, raters, mc / C, nA, HW);
        // lane k: the first surface position of chunk k
        int first = 2 * SD_FAR;
        for (int k = 0; k < nchunks; ++k) {
            const int x0 = (k * 64 + lane) * NPIX;
            const uint32_t bits = x0 < W ? sd_surface_bits<NPIX>(map, H, W, y, x0, c) : 0u;
            const unsigned long long any = __ballot(bits != 0);
            if (any) {
                const int fl = __ffsll((long long)any) - 1;
                const int fp = (k * 64 + fl) * NPIX + __ffs((int)seg_readlane(bits, fl)) - 1;
                if (lane == k) first = fp;
            }
        }
        // lane k: the first surface position of the chunks right of chunk k
        int nxv = first;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_down(nxv, off);
            if (lane + off < 64) nxv = min(nxv, t);
        }
        nxv = __shfl_down(nxv, 1);
        if (lane == 63) nxv = 2 * SD_FAR;

        int32_t* out = ws + (size_t)mc * HW + (size_t)y * W;
        int pv = -SD_FAR;                                            // the last surface position of the chunks to the left
        for (int k = 0; k < nchunks; ++k) {
            const int x0 = (k * 64 + lane) * NPIX;
            const uint32_t bits = x0 < W ? sd_surface_bits<NPIX>(map, H, W, y, x0, c) : 0u;
            const unsigned long long any = __ballot(bits != 0);
            const int nx = seg_readlane(nxv, k);
            const unsigned long long lower = any & ((1ull << lane) - 1ull);
            const unsigned long long higher = lane == 63 ? 0ull : any & (~0ull << (lane + 1));
            const int ll = lower ? 63 - __clzll((long long)lower) : 0, lr = higher ? __ffsll((long long)higher) - 1 : 0;
            const uint32_t nl = __shfl(bits, ll), nr = __shfl(bits, lr);
            const int left_of_lane = lower ? (k * 64 + ll) * NPIX + 31 - __clz((int)nl) : pv;
            const int right_of_lane = higher ? (k * 64 + lr) * NPIX + __ffs((int)nr) - 1 : nx;
            if (x0 < W) {
#pragma unroll
                for (int j = 0; j < NPIX; ++j) {
                    const uint32_t lo = bits & ((2u << j) - 1u), hi = bits & (~0u << j);
                    const int lp = lo ? x0 + 31 - __clz((int)lo) : left_of_lane;
                    const int rp = hi ? x0 + __ffs((int)hi) - 1 : right_of_lane;
                    const int x = x0 + j;
                    out[x] = min(min(x - lp, rp - x), SD_GINF);
                }
            }
            if (any) {
                const int hl = 63 - __clzll((long long)any);
                pv = (k * 64 + hl) * NPIX + 31 - __clz((int)seg_readlane(bits, hl));
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_surfdist_cols(int32_t* __restrict__ ws, int H, int W) {
    extern __shared__ uint16_t sd_g[];                               // [H][SD_STRIP]
    const int strips = (W + SD_STRIP - 1) / SD_STRIP;
    const int sx = blockIdx.x % strips;
    const size_t mc = blockIdx.x / strips;
    const int col = threadIdx.x & (SD_STRIP - 1), r0 = threadIdx.x / SD_STRIP, x = sx * SD_STRIP + col;
    constexpr int ROWS = 256 / SD_STRIP;
    const bool in = x < W;
    int32_t* img = ws + mc * H * W + (in ? x : 0);
    for (int y = r0; y < H; y += ROWS) sd_g[y * SD_STRIP + col] = (uint16_t)(in ? img[(size_t)y * W] : SD_GINF);
    __syncthreads();
    if (!in) return;
    for (int y = r0; y < H; y += ROWS) {
        const int g0 = sd_g[y * SD_STRIP + col];
        int best = g0 * g0;
        for (int dy = 1; dy * dy < best && (y - dy >= 0 || y + dy < H); ++dy) {
            if (y - dy >= 0) {
                const int g = sd_g[(y - dy) * SD_STRIP + col];
                best = min(best, g * g + dy * dy);
            }
            if (y + dy < H) {
                const int g = sd_g[(y + dy) * SD_STRIP + col];
                best = min(best, g * g + dy * dy);
            }
        }
        img[(size_t)y * W] = best >= SD_GINF * SD_GINF ? SD_NONE : best;
    }
}

__device__ __forceinline__ double sd_wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int sd_wave_max(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, __shfl_xor(x, off));
    return x;
}

struct SdShared {
    unsigned hist[2][256];
    double wsum[2][4];
    int wint[3][4];
    int sel[2][2];                  // per rank: {bucket, rank inside the bucket}
};

// The bucket of `hist` that holds 0-based rank r, and r's rank inside it.
__device__ __forceinline__ void sd_pick(const unsigned* hist, long long r, int* sel) {
    long long below = 0;
    int b = 0;
    for (; b < 255; ++b) {
        const long long h = hist[b];
        if (below + h > r) break;
        below += h;
    }
    sel[0] = b;
    sel[1] = (int)(r - below);
}

__global__ __launch_bounds__(256) void k_surfdist_pairs(const int32_t* __restrict__ ws, int B, int S, int L, int C, int HW, long long q_num,
                                                        long long q_den, int32_t* __restrict__ stats, double* __restrict__ sums) {
    __shared__ SdShared sh;
    const size_t cell = blockIdx.x;
    const int ci = (int)(cell % C), j = (int)(cell / C % L), i = (int)(cell / ((size_t)C * L) % S), b = (int)(cell / ((size_t)C * L * S));
    const int32_t* dA = ws + (((size_t)b * S + i) * C + ci) * HW;
    const int32_t* dR = ws + (((size_t)B * S + (size_t)b * L + j) * C + ci) * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    int n_ar = 0, n_ra = 0, mx = 0;
    double s_ar = 0.0, s_ra = 0.0;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int a = dA[p], r = dR[p];
        if (a == 0) { ++n_ar; mx = max(mx, r); s_ar += sqrt((double)r); }
        if (r == 0) { ++n_ra; mx = max(mx, a); s_ra += sqrt((double)a); }
    }
    n_ar = seg_wave_sum(n_ar); n_ra = seg_wave_sum(n_ra); mx = sd_wave_max(mx);
    s_ar = sd_wave_sum(s_ar); s_ra = sd_wave_sum(s_ra);
    if (lane == 0) {
        sh.wint[0][wave] = n_ar; sh.wint[1][wave] = n_ra; sh.wint[2][wave] = mx;
        sh.wsum[0][wave] = s_ar; sh.wsum[1][wave] = s_ra;
    }
    __syncthreads();
    n_ar = (sh.wint[0][0] + sh.wint[0][1]) + (sh.wint[0][2] + sh.wint[0][3]);
    n_ra = (sh.wint[1][0] + sh.wint[1][1]) + (sh.wint[1][2] + sh.wint[1][3]);
    mx = max(max(sh.wint[2][0], sh.wint[2][1]), max(sh.wint[2][2], sh.wint[2][3]));
    s_ar = (sh.wsum[0][0] + sh.wsum[0][1]) + (sh.wsum[0][2] + sh.wsum[0][3]);
    s_ra = (sh.wsum[1][0] + sh.wsum[1][1]) + (sh.wsum[1][2] + sh.wsum[1][3]);

    int32_t* st = stats + cell * 5;
    double* sm = sums + cell * 2;
    if (n_ar == 0 || n_ra == 0) {                                    // block-uniform: an undefined cell
        if (threadIdx.x == 0) {
            st[0] = n_ar; st[1] = n_ra; st[2] = 0; st[3] = 0; st[4] = 0;
            sm[0] = 0.0; sm[1] = 0.0;
        }
        return;
    }
    const long long n = (long long)n_ar + n_ra, t = q_num * (n - 1);
    long long r_lo = t / q_den, r_hi = r_lo + (t % q_den != 0 ? 1 : 0);           // q_num <= q_den: r_hi <= n - 1
    int pre_lo = 0, pre_hi = 0;                                      // the digits found so far
    for (int d = mx < 256 ? 0 : mx < 65536 ? 1 : 2; d >= 0; --d) {
        const int shift = 8 * d;
        const bool split = pre_lo != pre_hi;                         // block-uniform
        sh.hist[0][threadIdx.x] = 0;
        sh.hist[1][threadIdx.x] = 0;
        __syncthreads();
        for (int p = threadIdx.x; p < HW; p += 256) {
            const int a = dA[p], r = dR[p];
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                const int v = dir == 0 ? r : a;
                if ((dir == 0 ? a : r) == 0) {
                    const int head = v >> (shift + 8), digit = v >> shift & 255;
                    if (head == pre_lo) atomicAdd(&sh.hist[0][digit], 1u);
                    if (split && head == pre_hi) atomicAdd(&sh.hist[1][digit], 1u);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) sd_pick(sh.hist[0], r_lo, sh.sel[0]);
        if (threadIdx.x == 64) sd_pick(sh.hist[split ? 1 : 0], r_hi, sh.sel[1]);
        __syncthreads();
        pre_lo = pre_lo << 8 | sh.sel[0][0]; r_lo = sh.sel[0][1];
        pre_hi = pre_hi << 8 | sh.sel[1][0]; r_hi = sh.sel[1][1];
    }
    if (threadIdx.x == 0) {
        st[0] = n_ar; st[1] = n_ra; st[2] = mx; st[3] = pre_lo; st[4] = pre_hi;
        sm[0] = s_ar; sm[1] = s_ra;
    }
}

static inline int sd_classes(int K) { return K > 1 ? K - 1 : 1; }

}  // namespace ccdm

extern "C" size_t ccdm_surfdist_workspace_bytes(int B, int S, int L, int H, int W, int K) {
    if (B <= 0 || S <= 0 || L <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return (size_t)B * ((size_t)S + L) * ccdm::sd_classes(K) * H * W * sizeof(int32_t);
}

extern "C" int ccdm_surfdist(const uint8_t* samples, const uint8_t* raters, int B, int S, int L, int H, int W, int K, int q_num, int q_den,
                             int32_t* stats, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(K >= 1 && K <= SEG_MAX_K, "surfdist: K=%d outside [1,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(S >= 1 && S <= 255, "surfdist: S=%d outside [1,255]", S);
    CCDM_REQUIRE(L >= 1 && L <= 255, "surfdist: L=%d outside [1,255]", L);
    CCDM_REQUIRE(H >= 1 && H <= SD_MAX_DIM, "surfdist: H=%d outside [1,%d]", H, SD_MAX_DIM);
    CCDM_REQUIRE(W >= 1 && W <= SD_MAX_DIM, "surfdist: W=%d outside [1,%d]", W, SD_MAX_DIM);
    CCDM_REQUIRE(q_num > 0 && q_num <= q_den, "surfdist: q_num=%d q_den=%d outside 0 < q_num <= q_den", q_num, q_den);
    CCDM_REQUIRE(B >= 0, "surfdist: B=%d", B);
    if (B == 0) return 0;
    const int C = sd_classes(K), c0 = K > 1 ? 1 : 0;
    const long long nA = (long long)B * S, nmaps = nA + (long long)B * L;
    const long long col_blocks = nmaps * C * cdiv(W, SD_STRIP), cells = nA * L * C;
    CCDM_REQUIRE(col_blocks <= 0x7fffffffLL && cells <= 0x7fffffffLL, "surfdist: B=%d images (too many blocks)", B);
    CCDM_REQUIRE(samples && raters && stats && sums, "surfdist: null pointer");
    const size_t need = ccdm_surfdist_workspace_bytes(B, S, L, H, W, K);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "surfdist: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "surfdist: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* ws = static_cast<int32_t*>(workspace);
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(raters)) & 3) == 0;
    const long long row_waves = nmaps * C * H;
    const int row_blocks = (int)((row_waves + 3) / 4 < 8192 ? (row_waves + 3) / 4 : 8192);
    if (vec) hipLaunchKernelGGL(k_surfdist_rows<4>, dim3(row_blocks), dim3(256), 0, st, samples, raters, nA, nmaps, C, c0, H, W, ws);
    else hipLaunchKernelGGL(k_surfdist_rows<1>, dim3(row_blocks), dim3(256), 0, st, samples, raters, nA, nmaps, C, c0, H, W, ws);
    CCDM_CHECK_LAUNCH("surfdist rows");
    hipLaunchKernelGGL(k_surfdist_cols, dim3((int)col_blocks), dim3(256), (size_t)H * SD_STRIP * sizeof(uint16_t), st, ws, H, W);
    CCDM_CHECK_LAUNCH("surfdist cols");
    hipLaunchKernelGGL(k_surfdist_pairs, dim3((int)cells), dim3(256), 0, st, ws, B, S, L, C, H * W, (long long)q_num, (long long)q_den, stats,
                       sums);
    CCDM_CHECK_LAUNCH("surfdist pairs");
    return 0;
}
