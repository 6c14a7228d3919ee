// GroupNorm statistics: partials stats[n][slot][c] = (sum x, sum x^2) in fp64, written by the producers' epilogues, read by the
// consumers' prologues.  Every addition runs in a fixed order (run-to-run and build-to-build identical results): producers — per lane
// in pixel order, then lane + partner, then waves ascending; consumers — per channel its slices ascending, then the group's channels.
#pragma once
#include "ccdm_common.h"

namespace ccdm {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- producer side ----
// Every stored value is added to the lane's running sums in fp64 (v * v is exact there): var = sum x^2 / n - mean^2 cancels in
// proportion to mean^2 / var of the group, and fp32 sums left rstd errors of 1e-5 at mean/std = 100 (tests/test_gn_statistics.py).
// The lanes that hold a channel are added next, in each producer's own register layout (written out at the site: as shared helpers
// that step and the per-value sum changed the register allocation of k_conv, k_conv1x1 and k_stem), then the block's waves:
// gn_fold_waves adds channel l of the LDS rows red[row0 + w * rstride][32][2], w = 0 .. nw - 1 ascending, to (s1, s2).
__device__ __forceinline__ void gn_fold_waves(const double* red, const int row0, const int rstride, const int nw, const int l, double& s1, double& s2) {
    for (int w = 0; w < nw; ++w) { s1 += red[((w * rstride + row0) * 32 + l) * 2]; s2 += red[((w * rstride + row0) * 32 + l) * 2 + 1]; }
}

// ---- consumer side: the affine of sample n, ab[c] = (scale, shift) such that y = scale * x + shift ----
// What a consumer normalises (`Src` below): one input, or two concatenated along the channels (c < C0: the first).  A conv passes its
// ccdm_conv_args (same field names), read in place — a GnSrc copied out of it changed k_conv's register allocation; other kernels a GnSrc.
struct GnSrc {
    const double* stats0; const double* stats1;   // [N][slices][C0 | C1][2]
    int slices0, slices1, C0, C1;                 // C1 = 0: one input
    int Hin, Win;                                 // pixels per sample: the count of a channel's values
    float eps;
    const float* gamma; const float* beta;
    bool film;                                    // FiLM: h = GN(h) * (1 + scale) + shift, (scale, shift) from the embedding table
    const float* emb_table; int emb_stride, film_off;
};

// (sum, sum^2) of channel c's group: every (channel, slice) partial in ascending order in ONE running sum (not per-channel sums, then
// the group sum: another rounding), fetched 16 at a time with independent loads — one L2 round trip per 16 instead of one per partial.
template <class Src>
__device__ __forceinline__ void gn_group_sums(const Src& a, int n, int c, double& sum, double& sq) {
    const int C = a.C0 + a.C1;
    const int cpg = C / 32;
    const int c_lo = (c / cpg) * cpg, c_hi = c_lo + cpg;
    sum = 0.0; sq = 0.0;
    int cc = c_lo, s = 0;
    while (cc < c_hi) {
        f64x2 v[16];
        bool ok[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            ok[u] = cc < c_hi;
            const int ccl = ok[u] ? cc : c_hi - 1;                       // clamped: the load stays unconditional
            const bool second = ccl >= a.C0;
            const double* st = second ? a.stats1 : a.stats0;
            const int ci = second ? ccl - a.C0 : ccl, Cs = second ? a.C1 : a.C0, S = second ? a.slices1 : a.slices0;
            const int sl = ok[u] ? s : 0;
            v[u] = *reinterpret_cast<const f64x2*>(st + (((size_t)n * S + sl) * Cs + ci) * 2);
            if (++s >= S) { s = 0; ++cc; }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {                                   // fixed order: ascending (channel, slice)
            sum += ok[u] ? v[u][0] : 0.0;
            sq += ok[u] ? v[u][1] : 0.0;
        }
    }
}

// mean and 1/sqrt(var + eps) of a group from its (sum, sum^2) over cnt values.  fp64 throughout, but without the division /
// square-root expansions (three v_div sequences and a v_sqrt: ~800 cycles of a block prologue that small-spatial launches cannot
// hide): hardware reciprocal / reciprocal-square-root estimates refined by two Newton steps each — relative error < 2^-50,
// invisible after the rounding to fp32.
__device__ __forceinline__ void gn_mean_rstd64(double sum, double sq, double cnt, float eps, double& mean, double& rs) {
    double ic = __builtin_amdgcn_rcp(cnt);
    ic = ic * (2.0 - cnt * ic);
    ic = ic * (2.0 - cnt * ic);
    mean = sum * ic;
    double var = sq * ic - mean * mean;
    if (var < 0.0) var = 0.0;
    const double ve = var + (double)eps;
    rs = __builtin_amdgcn_rsq(ve);
    rs = rs * (1.5 - 0.5 * ve * rs * rs);
    rs = rs * (1.5 - 0.5 * ve * rs * rs);
}

// per-channel parameters of the affine, fetched ahead of the arithmetic (gn_params) so that a kernel can issue every small load
// before its first HBM request and do the fp64 finalisation (gn_finalize: registers only) while that request is in flight
struct GnParams { float gamma, beta, film_scale, film_shift; };
template <class Src>
__device__ __forceinline__ GnParams gn_params(const Src& a, int emb_row, int c) {
    GnParams p;
    p.gamma = a.gamma[c]; p.beta = a.beta[c]; p.film_scale = 0.f; p.film_shift = 0.f;
    if (a.film) {
        const float* row = a.emb_table + (size_t)emb_row * a.emb_stride + a.film_off;
        p.film_scale = row[c]; p.film_shift = row[a.C0 + a.C1 + c];
    }
    return p;
}
template <class Src>
__device__ __forceinline__ float2 gn_finalize(const Src& a, const GnParams& p, double sum, double sq) {
    const int C = a.C0 + a.C1;
    const int cpg = C / 32;
    double mean, rs;
    gn_mean_rstd64(sum, sq, (double)cpg * (double)a.Hin * (double)a.Win, a.eps, mean, rs);
    float sc = (float)rs * p.gamma;
    double base = p.beta;
    if (a.film) {   // h = GN(h) * (1 + scale) + shift          unet.py:254-258
        const float one_plus = 1.0f + p.film_scale;
        sc = sc * one_plus;
        base = (double)p.beta * one_plus + p.film_shift;
    }
    // the shift in fp64 from the scale as rounded, then rounded once: y = sc * x + sh is then sc * (x - mean) + base up to that one
    // rounding.  (In fp32 — sc * meanf, then beta minus that — a group of variance <= eps, rstd ~ 300, lost ~2e-5 of its normalised
    // value to the roundings at |sc * mean| ~ 10^2, tests/test_gn_statistics.py.)
    return make_float2(sc, (float)(base - (double)sc * mean));
}

// Prologue form.  gn_prefetch issues EVERY load the affine of channel c needs — gamma, beta, the FiLM row and the channel's own
// first 16 slice partials — unconditionally (addresses clamped; `dummy` = any readable device memory, read when there is no
// GroupNorm), with two or three instructions of address arithmetic per load and no branch, and waits for none of them.  The kernel
// then issues its first halo or weight request; the small loads return first (vector memory returns in order), so gn_affine_block —
// per-channel sums over the slices (ascending), exchanged through LDS, added over the group's channels (ascending), finalised in
// fp64 — runs while that request is in flight.  (A branch between the loads and their use would make the waitcnt pass drain the
// whole queue at the join; a flat-addressed load anywhere in flight does the same.)
//   GMAX (most slot groups per channel) is the caller's: a kernel whose order of additions is one running sum over all of a
// channel's slices pins GMAX = 1.
struct GnPrefetch { GnParams p; f64x2 v[16]; };
template <class Src>
__device__ __forceinline__ const char* gn_channel_row(const Src& a, int n, int c, int& S, unsigned& stride) {
    const bool second = c >= a.C0;                                       // (only with a concatenated input)
    const double* st = second ? a.stats1 : a.stats0;
    const int ci = second ? c - a.C0 : c, Cs = second ? a.C1 : a.C0;
    S = second ? a.slices1 : a.slices0;
    stride = (unsigned)Cs * 16u;
    return reinterpret_cast<const char*>(st + ((size_t)n * S * Cs + ci) * 2);
}
// Thread -> (channel, slot group).  A block has more threads than channels wherever many slices occur (32-64 channels on 256
// threads at the full-resolution stages), so the first G * C threads each take 16 slices of one channel: up to 64 slices are summed
// from ONE prefetch round.  G = min(NT / C, GMAX); threads beyond G * C idle (their loads are clamped duplicates).
struct GnLane { int c, grp, G; };
template <int GMAX, class Src>
__device__ __forceinline__ GnLane gn_lane(const Src& a, int tid, int NT) {
    static_assert(GMAX >= 1 && GMAX <= 4, "slot groups");
    const int C = a.C0 + a.C1;
    const int smax = a.slices0 > a.slices1 ? a.slices0 : a.slices1;
    const int need = smax > 16 ? (smax + 15) >> 4 : 1;                   // slot groups the slice count asks for (1 wherever <= 16 slices)
    GnLane l;
    l.G = NT >= 4 * C ? 4 : (NT >= 3 * C ? 3 : (NT >= 2 * C ? 2 : 1));
    l.G = l.G < need ? l.G : need;
    if constexpr (GMAX < 4) l.G = l.G < GMAX ? l.G : GMAX;
    l.grp = (tid >= C ? 1 : 0) + (tid >= 2 * C ? 1 : 0) + (tid >= 3 * C ? 1 : 0);
    l.c = tid - l.grp * C;
    if (l.grp >= l.G || l.c >= C) { l.grp = l.G; l.c = C - 1; }         // idle lane (grp == G marks it)
    return l;
}
template <int GMAX = 4, class Src>
__device__ __forceinline__ void gn_prefetch(const Src& a, bool has_gn, int n, int emb_row, int tid, int NT, const void* dummy, GnPrefetch& g) {
    const int C = a.C0 + a.C1;
    const GnLane l = gn_lane<GMAX>(a, tid, NT);
    const int c = l.c, grp = l.grp < l.G ? l.grp : l.G - 1;
    const float* df = static_cast<const float*>(dummy);
    const bool film = has_gn && a.film;
    const float* gam = has_gn ? a.gamma + c : df;
    const float* bet = has_gn ? a.beta + c : df;
    const float* row = film ? a.emb_table + (size_t)emb_row * a.emb_stride + a.film_off + c : df;
    g.p.gamma = *gam; g.p.beta = *bet;
    g.p.film_scale = row[0]; g.p.film_shift = row[film ? C : 0];
    int S = 1;
    unsigned stride = 0;
    const char* base = static_cast<const char*>(dummy);
    if (has_gn) base = gn_channel_row(a, n, c, S, stride);               // uniform condition, selects only
    const unsigned last = (unsigned)(S - 1) * stride, first = (unsigned)(16 * grp) * stride;
    // Few-pixel images leave 1-4 slices: 12 of 16 requests would be clamped duplicates — 1 KB per wave each through a vector-memory
    // front end that takes ~40-64 B/clk, ~800 cycles of every block's prologue ahead of its halo request.  The slice count is a kernel
    // argument (uniform), so the extra requests sit behind one scalar branch.
    const bool few = !has_gn || (a.slices0 <= 4 && a.slices1 <= 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) g.v[u] = *reinterpret_cast<const f64x2*>(base + min(first + (unsigned)u * stride, last));
    if (!few) {
#pragma unroll
        for (int u = 4; u < 16; ++u) g.v[u] = *reinterpret_cast<const f64x2*>(base + min(first + (unsigned)u * stride, last));
    } else {
#pragma unroll
        for (int u = 4; u < 16; ++u) g.v[u] = f64x2{0.0, 0.0};
    }
}
// (sum, sum^2) of channel c over the slices [16 grp, 16 grp + 16) from the prefetched values g (NULL: fetched here), ascending; the lane
// of group 0 also takes the slices beyond 16 G (more slices than one prefetch round of the block covers: blocking loads)
template <class Src>
__device__ __forceinline__ f64x2 gn_channel_sums(const Src& a, int n, int c, int grp, int G, const GnPrefetch* g) {
    int S;
    unsigned stride;
    const char* base = gn_channel_row(a, n, c, S, stride);
    f64x2 acc = {0.0, 0.0};
    const int s_first = 16 * grp;
    if (g) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {                                   // selects, not branches (x + 0.0 == x)
            acc[0] += s_first + u < S ? g->v[u][0] : 0.0;
            acc[1] += s_first + u < S ? g->v[u][1] : 0.0;
        }
    } else {
        for (int s = s_first; s < S && s < s_first + 16; ++s) acc += *reinterpret_cast<const f64x2*>(base + (unsigned)s * stride);
    }
    if (grp == 0)
        for (int s = 16 * G; s < S; ++s) acc += *reinterpret_cast<const f64x2*>(base + (unsigned)s * stride);
    return acc;
}
// the whole table ab[0..C), each entry times `mul`: call with the block's NT threads converged; `scratch` = max(C, NT) x 16 B of
// LDS not otherwise in use until the caller's next barrier.  Order of additions per group: channels ascending, per channel the slot
// groups ascending, per slot group the slices ascending (for <= 16 slices, or GMAX = 1: the plain ascending (channel, slice) order).
template <int GMAX = 4, class Src>
__device__ __forceinline__ void gn_affine_block(const Src& a, int n, int emb_row, const GnPrefetch& g, f64x2* scratch, float2* ab, int NT,
                                                float mul = 1.f) {
    const int C = a.C0 + a.C1, cpg = C / 32;
    const int tid = threadIdx.x;
    const GnLane l = gn_lane<GMAX>(a, tid, NT);
    const int G = l.G;
    auto group = [&](const int c) {
        const int c_lo = (c / cpg) * cpg;
        f64x2 acc = {0.0, 0.0};
        for (int j = 0; j < cpg; ++j)
            for (int q = 0; q < G; ++q) acc += scratch[q * C + c_lo + j];
        return acc;
    };
    auto put = [&](const int c, const float2 t) { ab[c] = make_float2(t.x * mul, t.y * mul); };
    // the lanes of the first G * C threads work from the prefetched values alone — no load here, which would be younger than the caller's
    // halo request and drag its round trip into this wait; channels beyond the block size (C > NT, then G = 1: rare) take blocking loads
    if (l.grp < G) scratch[l.grp * C + l.c] = gn_channel_sums(a, n, l.c, l.grp, G, &g);
    for (int c = tid + NT; c < C; c += NT) scratch[c] = gn_channel_sums(a, n, c, 0, 1, nullptr);
    __syncthreads();
    if (tid < C) {
        const f64x2 acc = group(tid);
        put(tid, gn_finalize(a, g.p, acc[0], acc[1]));
    }
    for (int c = tid + NT; c < C; c += NT) {
        const f64x2 acc = group(c);
        put(c, gn_finalize(a, gn_params(a, emb_row, c), acc[0], acc[1]));
    }
}

// the table without a prefetch (kernels whose prologue has nothing to overlap), from c_first on; gn_group_sums' order of additions
template <class Src>
__device__ __forceinline__ void compute_gn_affine(const Src& a, int n, int emb_row, float2* ab, int c_first = 0) {
    const int C = a.C0 + a.C1;
    for (int c = c_first + threadIdx.x; c < C; c += blockDim.x) {
        double sum, sq;
        const GnParams p = gn_params(a, emb_row, c);
        gn_group_sums(a, n, c, sum, sq);
        ab[c] = gn_finalize(a, p, sum, sq);
    }
}

}  // namespace ccdm
