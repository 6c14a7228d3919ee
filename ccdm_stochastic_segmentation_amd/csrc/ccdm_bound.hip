// The variational bound on the likelihood of a held-out label map (DenoisingModel.label_bound; include/ccdm_hip.h has THE definition):
//     -log p(y | image) <= L_T + sum_t E_{x_t ~ q(x_t | x_0 = y)} l_t(y, x_t),    l_t = the reference's training loss (trainer.py:255-277).
// Two launches around a network pass whose rows sit at different noise levels (every network kernel reads its time-embedding row as
// rowmap[n] + step), each reading a device table of one 32-byte ccdm_bound_row per engine row:
//   k_bound_noise   x_t ~ Cat(cumalpha_t onehot(y) + (1 - cumalpha_t) / K): the project's Exp(1) race (race_hit_miss) on a Philox counter
//                   range of its own (0x20000000 | k / 4), keyed by (pixel, the row's global sample index, its timestep).  One thread per
//                   pixel; reads 1 byte, writes 1 byte.  Many engine rows share one label map (label_row): nothing is gathered.
//   k_bound_terms   per counted pixel KL(theta_post(x_t, onehot(y)) || max(theta_post_prob(x_t, x0), floor)) in fp32, from x0 [N,HW,K] as the
//                   engine leaves it and x_t as the uint8 index: no one-hot, no BCHW copy, no [N,K,HW] intermediate.  A block's BLK pixels
//                   move as one contiguous [pixel][class] run through LDS rows of odd pitch (stage_class_rows); a thread then walks its
//                   row twice (R first, then the terms), so nothing of a pixel's K values lives in a register array: no scratch at any K.
//                   Per pixel 4 K + 2 bytes in, 4 bytes out where the map is asked for.
//   k_bound_fold    the per-(block, row) partial sums of the launch above, folded per row in a fixed order (as ccdm_stats_fold does for the
//                   GroupNorm statistics): no float atomics, the same bits on every call.
// A block's pixels may belong to several rows (HW need not be a multiple of the block): the row is found per pixel, staging and the block
// reduction run per row segment, an idle row is neither read nor drawn for.
#include "ccdm_common.h"
#include "ccdm_sampler_common.h"

#include <algorithm>

namespace ccdm {

constexpr uint32_t BOUND_TAG = 0x20000000u;      // the epilogue's blocks have word 3 < 64, the clamp 0x80000000 | kq, the renoise 0x40000000 | kq

// a row that holds something: a timestep >= 1 and a label row inside `labels`; everything else (CCDM_BOUND_IDLE) is idle
__device__ __forceinline__ bool bound_row_runs(const ccdm_bound_row& r, const int R) { return r.t >= 1 && (unsigned)r.label_row < (unsigned)R; }

__global__ __launch_bounds__(256) void k_bound_noise(const uint8_t* __restrict__ labels, const ccdm_bound_row* __restrict__ table, const unsigned npix,
                                                     const unsigned HW, const int K, const int R, const uint32_t k0, const uint32_t k1,
                                                     uint8_t* __restrict__ xt_out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;                  // (N * HW < 2^31: the launcher checks)
    if (i >= npix) return;
    const unsigned n = i / HW, pix = i - n * HW;
    const ccdm_bound_row r = table[n];                                   // a wave inside one row: 64 loads of one address
    if (!bound_row_runs(r, R)) return;
    const int y = labels[(size_t)r.label_row * HW + pix];
    // an uncounted pixel (255, or any byte that is no class) takes no draw: a class the network can read, the same on every call
    const int x = y < K ? race_hit_miss(K, y, r.p_hit, r.p_miss, pix, r.sample, (uint32_t)r.t, BOUND_TAG, k0, k1) : (int)(pix % (unsigned)K);
    xt_out[i] = (uint8_t)x;
}

// sum over the wave's 64 lanes in a fixed order; lane 0 holds it
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

constexpr int bound_blk(const int KP) { return KP <= 32 ? 256 : 64; }
template <int KP>
constexpr int bound_pitch() { return (KP | 1) > CCDM_MAX_CLASSES ? CCDM_MAX_CLASSES : (KP | 1); }

// ws: [blocks + N][2] doubles; the partial of (block b, row n) lives at b + n (b and n both grow along the pixels, so the place is
// the pair's own; places no pair maps to are never read)
template <int KP, int BLK>
__global__ __launch_bounds__(BLK) void k_bound_terms(const float* __restrict__ x0, const uint8_t* __restrict__ xt, const uint8_t* __restrict__ labels,
                                                     const ccdm_bound_row* __restrict__ table, const float* __restrict__ cw, const unsigned npix,
                                                     const unsigned HW, const int K, const int R, const float floor, double* __restrict__ ws,
                                                     float* __restrict__ map) {
    constexpr int PITCH = bound_pitch<KP>();
    constexpr int WAVES = BLK / 64;
    __shared__ float sx[BLK * PITCH];
    __shared__ double sred[WAVES][2];
    const unsigned i0 = blockIdx.x * (unsigned)BLK;
    const int tid = threadIdx.x;
    const int nvalid = (int)std::min<unsigned>((unsigned)BLK, npix - i0);
    // the block's rows n_lo .. n_hi; row n holds the block's pixels [max(n * HW, i0), min((n + 1) * HW, i0 + nvalid)) — all uniform
    const unsigned n_lo = i0 / HW, n_hi = (i0 + (unsigned)nvalid - 1u) / HW;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        if (!bound_row_runs(table[n], R)) continue;
        const unsigned s0 = std::max(n * HW, i0) - i0, s1 = std::min((n + 1u) * HW, i0 + (unsigned)nvalid) - i0;
        stage_class_rows<BLK, PITCH, false>(sx + s0 * PITCH, x0 + (size_t)(i0 + s0) * K, nullptr, (int)(s1 - s0), (unsigned)K, tid);
    }
    __syncthreads();
    float v = 0.f, wgt = 0.f;                                            // the pixel's weighted term and its weight
    unsigned my_n = ~0u;
    if (tid < nvalid) {
        const unsigned i = i0 + (unsigned)tid;
        my_n = i / HW;
        const ccdm_bound_row r = table[my_n];
        if (bound_row_runs(r, R)) {
            const int y = labels[(size_t)r.label_row * HW + (i - my_n * HW)];
            if (y < K) {
                const int x = xt[i];
                const float* const row = sx + tid * PITCH;
                wgt = cw ? cw[y] : 1.0f;
                float l;
                if (r.alpha_t == 0.0f && r.cumalpha_tm1 == 1.0f) {
                    // t = 1, posterior_coeffs = (0, 1): p = onehot(y) and q = x0 — the decoder term, without the closed form's roundings
                    l = -logf(fmaxf(row[y], floor));
                } else {
                    const float al = r.alpha_t, cu = r.cumalpha_tm1, Kf = (float)K;
                    const float u = (1.0f - al) / Kf, b = (1.0f - cu) / Kf;
                    // A_k takes two values and theta_k four, so S = sum_k A_k and T = sum_k theta_k are written out: K equal addends one
                    // after the other round the same way every time, K / 2 ulp where these are a few
                    const float Ah = al + u, Bh = cu + b;
                    const float S = Ah + (Kf - 1.0f) * u;
                    const float T = x == y ? Ah * Bh + (Kf - 1.0f) * (u * b) : (Ah * b + u * Bh) + (Kf - 2.0f) * (u * b);
                    const float bS = b * S;
                    // pass 1: R = sum_k r_k (k ascending)
                    float Rs = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const float A = (k == x ? al : 0.0f) + u;
                        Rs += row[k] / (cu * A + bS);
                    }
                    const float bR = b * Rs;
                    // pass 2: the terms, added with a compensated (Kahan) sum — the terms have both signs and reach 27.6, and K
                    // roundings at the sum's own magnitude would be the largest error of the pixel (-ffp-contract=off keeps it)
                    // (p_k = A_k B_k / T takes four values — k is x_t or not, y or not — and so does its logarithm: formed once, picked per k)
                    const float p_mm = u * b / T, p_hm = Ah * b / T, p_mh = u * Bh / T, p_hh = Ah * Bh / T;
                    const float lp_mm = p_mm > 0.f ? logf(p_mm) : 0.f, lp_hm = p_hm > 0.f ? logf(p_hm) : 0.f;
                    const float lp_mh = p_mh > 0.f ? logf(p_mh) : 0.f, lp_hh = p_hh > 0.f ? logf(p_hh) : 0.f;
                    l = 0.f;
                    float comp = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const bool kx = k == x, ky = k == y;
                        const float A = kx ? Ah : u;
                        const float p = kx ? (ky ? p_hh : p_hm) : (ky ? p_mh : p_mm);
                        const float lp = kx ? (ky ? lp_hh : lp_hm) : (ky ? lp_mh : lp_mm);
                        const float q = A * (cu * (row[k] / (cu * A + bS)) + bR);
                        if (p > 0.f) {
                            const float term = p * (lp - logf(fmaxf(q, floor))) - comp;
                            const float s = l + term;
                            comp = (s - l) - term;
                            l = s;
                        }
                    }
                }
                v = wgt != 0.f ? wgt * l : 0.f;
            }
        }
        if (map) map[i] = v;                                             // 0 at uncounted pixels and on idle rows
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (unsigned n = n_lo; n <= n_hi; ++n) {
        const double sv = wave_sum(my_n == n ? (double)v : 0.0), sw = wave_sum(my_n == n ? (double)wgt : 0.0);
        if (lane == 0) { sred[wave][0] = sv; sred[wave][1] = sw; }
        __syncthreads();
        if (tid == 0) {
            double a = sred[0][0], c = sred[0][1];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) { a = a + sred[w][0]; c = c + sred[w][1]; }
            double* const d = ws + ((size_t)blockIdx.x + n) * 2;
            d[0] = a; d[1] = c;
        }
        __syncthreads();
    }
}

// one wave per row: lane l adds the row's blocks b_lo + l, b_lo + l + 64, ... in ascending order, then the lanes are folded
__global__ __launch_bounds__(64) void k_bound_fold(const double* __restrict__ ws, const unsigned HW, const unsigned blk, double* __restrict__ row_sum,
                                                   double* __restrict__ row_weight) {
    const unsigned n = blockIdx.x;
    const unsigned b_lo = n * HW / blk, b_hi = ((n + 1u) * HW - 1u) / blk;
    double a = 0.0, c = 0.0;
    for (unsigned b = b_lo + threadIdx.x; b <= b_hi; b += 64u) {
        const double* const s = ws + ((size_t)b + n) * 2;
        a = a + s[0]; c = c + s[1];
    }
    a = wave_sum(a); c = wave_sum(c);
    if (threadIdx.x == 0) { row_sum[n] = a; row_weight[n] = c; }
}

static int check_bound_args(const char* name, const bool pointers, const ccdm_bound_row* table, const int N, const int R, const int HW, const int K) {
    CCDM_REQUIRE(pointers, "%s: null pointer", name);
    CCDM_REQUIRE(((uintptr_t)table & 3) == 0, "%s: table not 4-byte aligned", name);
    CCDM_REQUIRE(N >= 1 && R >= 1 && HW >= 1, "%s: bad shape N=%d R=%d HW=%d", name, N, R, HW);
    CCDM_REQUIRE(K >= 1 && K <= CCDM_MAX_CLASSES, "%s: K=%d outside [1,%d]", name, K, CCDM_MAX_CLASSES);
    CCDM_REQUIRE((size_t)N * HW <= 0x7FFFFFFFull && (size_t)R * HW <= 0x7FFFFFFFull, "%s: too many pixels", name);
    return 0;
}

static int bound_blk_of(const int K) {
    int blk = 0;
    dispatch_kp<256>(K, [&](auto kp) { blk = bound_blk(decltype(kp)::value); });
    return blk;
}

}  // namespace ccdm

using namespace ccdm;

extern "C" int ccdm_bound_noise(const uint8_t* labels, const ccdm_bound_row* table, int N, int R, int HW, int K, uint64_t philox_seed,
                                uint8_t* xt_out, void* stream) {
    if (const int rc = check_bound_args("ccdm_bound_noise", labels && table && xt_out, table, N, R, HW, K)) return rc;
    const unsigned npix = (unsigned)N * (unsigned)HW;
    hipLaunchKernelGGL(k_bound_noise, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, labels, table, npix, (unsigned)HW, K, R,
                       (uint32_t)philox_seed, (uint32_t)(philox_seed >> 32), xt_out);
    CCDM_CHECK_LAUNCH("bound_noise");
    return 0;
}

extern "C" size_t ccdm_bound_terms_workspace_bytes(int N, int HW, int K) {
    if (N < 1 || HW < 1 || K < 1 || K > CCDM_MAX_CLASSES || (size_t)N * HW > 0x7FFFFFFFull) return 0;
    const size_t blk = (size_t)bound_blk_of(K);
    return (((size_t)N * HW + blk - 1) / blk + (size_t)N) * 2 * sizeof(double);
}

extern "C" int ccdm_bound_terms(const float* x0, const uint8_t* xt, const uint8_t* labels, const ccdm_bound_row* table, const float* class_weights,
                                int N, int R, int HW, int K, float floor, void* ws, double* row_sum, double* row_weight, float* map,
                                void* stream) {
    if (const int rc = check_bound_args("ccdm_bound_terms", x0 && xt && labels && table && ws && row_sum && row_weight, table, N, R, HW, K)) return rc;
    CCDM_REQUIRE(floor > 0.0f && floor < 1.0f, "ccdm_bound_terms: floor %g not in (0,1)", (double)floor);
    CCDM_REQUIRE(((uintptr_t)ws & 7) == 0, "ccdm_bound_terms: workspace not 8-byte aligned");
    const unsigned npix = (unsigned)N * (unsigned)HW;
    dispatch_kp<256>(K, [&](auto kp) {
        constexpr int KP = decltype(kp)::value, BLK = bound_blk(KP);
        hipLaunchKernelGGL((k_bound_terms<KP, BLK>), dim3((npix + BLK - 1u) / BLK), dim3(BLK), 0, (hipStream_t)stream, x0, xt, labels, table,
                           class_weights, npix, (unsigned)HW, K, R, floor, (double*)ws, map);
    });
    CCDM_CHECK_LAUNCH("bound_terms");
    hipLaunchKernelGGL(k_bound_fold, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, (const double*)ws, (unsigned)HW, (unsigned)bound_blk_of(K),
                       row_sum, row_weight);
    CCDM_CHECK_LAUNCH("bound_fold");
    return 0;
}
