// Uncertainty-quality counts of a multi-sample prediction, device part: the walk of ccdm_seg_common.h ending in histograms of the
// per-pixel uncertainty (the entropy and mutual-information maps of ccdm_vote_finalize) split by whether the prediction is wrong.
// Nothing in the reference computes these; the definition in include/ccdm_hip.h is the contract, tests/test_seg_uncertainty.py
// restates it op by op.
//
// Per output pixel of [B,H,W] whose label t < C: pred is the class the confusion kernel counts (seg_step / seg_argmax),
// wrong = (pred != t); for every map m the uncertainty u is the bilinear sample of maps[m] through the same coordinates and
// weights (seg_row / seg_pixel / seg_value on a one-channel source), t = u / ranges[m] clamped to [0, 1] (NaN -> 0),
// q = (int)(t * 65536).  From q on everything is an integer.
//   pix[m][min((q*M) >> 16, M-1)] += {1, wrong};
//   patch[m][min((Q*M) / (n*65536), M-1)] += {1, 2*e >= n} per aligned P x P patch with n >= 1 counted pixels, Q the sum of their
//   q and e the number of wrong ones.  The kernel divides ((Q*M) >> 16) / n in 32 bits: floor(floor(x / a) / b) = floor(x / (a*b))
//   for positive integers, and (Q*M) >> 16 <= 2^17.
//
// Patches.  A wave walks 64 columns x 16 rows from a row that is a multiple of 16, and P divides both: a patch never leaves its
// wave.  Each lane adds q (per map) and n | e << 16 down the rows of a patch in registers; at the patch's last row (or the last
// row of the wave's part: the image edge) the P lanes of a patch are summed by DPP (the first log2 P steps of seg_wave_sum) and
// the patch's first lane commits.  No LDS for the reduce.
//
// Histograms.  Two LDS tables per block, [U][M] each, one 64-bit word per bin: the count in the low word, the wrong / inaccurate
// count in the high word (a block counts fewer than 2^31 pixels: seg_check_block_counts).  Uncertainty is 0 over most of an
// image, so most lanes of a wave hit one bin: the lanes are grouped by equal bin (ballot and bit count, as seg_for_each_group)
// for up to UNC_GROUPS distinct bins, one LDS add per group; the lanes left over add for themselves.  At the end one 64-bit
// global add per non-zero half.  Integer atomics only: exact in any order, two identical calls are bit-identical.
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int UNC_MAX_MAPS = 4;
constexpr int UNC_MAX_BINS = 512;
constexpr int UNC_GROUPS = 4;           // distinct bins of a wave that get one LDS add each
constexpr float UNC_SCALE = 65536.0f;

struct UncArgs {
    const float* maps;                  // [U][B,h,w]
    float range[UNC_MAX_MAPS];
    int U, M, P;
};

// t = u / range, not > 0 (NaN included) -> 0, >= 1 -> 1; q = (int)(t * 65536): 0 <= q <= 65536
__device__ __forceinline__ int unc_quantise(float u, float range) {
    float t = u / range;
    t = t > 0.0f ? t : 0.0f;
    t = t >= 1.0f ? 1.0f : t;
    return (int)(t * UNC_SCALE);
}

// table[bin] += {1, hi} for every lane with `flag` set.  Wave-uniform call, all 64 lanes active.
__device__ __forceinline__ void unc_add(unsigned long long* __restrict__ table, bool flag, int bin, bool hi, int lane) {
    unsigned long long rest = __ballot(flag);
    for (int it = 0; it < UNC_GROUPS && rest; ++it) {
        const int g = seg_readlane(bin, __ffsll((long long)rest) - 1);
        const bool in_g = flag && bin == g;         // a lane served before had another bin
        const unsigned long long mask = __ballot(in_g);
        const unsigned long long add = (unsigned long long)__popcll(mask) | (unsigned long long)__popcll(__ballot(in_g && hi)) << 32;
        if (lane == 0) atomicAdd(&table[g], add);
        rest &= ~mask;
    }
    if ((rest >> lane) & 1) atomicAdd(&table[bin], 1ull | (unsigned long long)hi << 32);
}

// Sum over the P lanes of a patch (aligned groups of P = 2, 4, 8, 16 lanes), in every lane of the group.
__device__ __forceinline__ int unc_patch_sum(int x, int P) {
    x += seg_dpp<0xB1>(x);                          // quad_perm [1,0,3,2]
    if (P >= 4) x += seg_dpp<0x4E>(x);              // quad_perm [2,3,0,1]
    if (P >= 8) x += seg_dpp<0x141>(x);             // row_half_mirror
    if (P >= 16) x += seg_dpp<0x140>(x);            // row_mirror
    return x;
}

// seg_step for the maps: the same source rows and horizontal weights as the prediction's, one channel per map.
template <bool IDENT>
__device__ __forceinline__ void unc_step(float (&uA)[UNC_MAX_MAPS], float (&uB)[UNC_MAX_MAPS], int& yA, int& yB, const UncArgs& a,
                                         const SegSrc& s, const SegLane<IDENT>& l, int b, int y) {
    const size_t plane = (size_t)s.B * s.h * s.w;
    if (IDENT) {
#pragma unroll
        for (int m = 0; m < UNC_MAX_MAPS; ++m) {
            if (m < a.U) {
                float r[1];
                seg_pixel<1, 0, false>(r, a.maps + m * plane, nullptr, ((size_t)b * s.h + y) * s.w + l.ix0, 1, 1);
                uA[m] = r[0];
            }
        }
        return;
    }
    int iy0, iy1;
    float h0, h1;
    seg_coord(s.sh, y, s.h, iy0, iy1, h0, h1);
    if (iy0 != yA) {
#pragma unroll
        for (int m = 0; m < UNC_MAX_MAPS; ++m) {
            if (m < a.U) {
                if (iy0 == yB) {
                    uA[m] = uB[m];
                } else {
                    float r[1];
                    seg_row<1, 0, false>(r, a.maps + m * plane, nullptr, ((size_t)b * s.h + iy0) * s.w, l.ix0, l.ix1, l.lw0, l.lw1, 1, 1);
                    uA[m] = r[0];
                }
            }
        }
        yA = iy0;
    }
    if (iy1 != yB) {
#pragma unroll
        for (int m = 0; m < UNC_MAX_MAPS; ++m) {
            if (m < a.U) {
                if (iy1 == yA) {
                    uB[m] = uA[m];
                } else {
                    float r[1];
                    seg_row<1, 0, false>(r, a.maps + m * plane, nullptr, ((size_t)b * s.h + iy1) * s.w, l.ix0, l.ix1, l.lw0, l.lw1, 1, 1);
                    uB[m] = r[0];
                }
            }
        }
        yB = iy1;
    }
}

template <int KP, int SRC, bool V4, bool IDENT>
__global__ __launch_bounds__(256) void k_uncscore(SegSrc s, const uint8_t* __restrict__ labels, UncArgs a, unsigned long long* __restrict__ pix,
                                                  unsigned long long* __restrict__ patch) {
    extern __shared__ unsigned long long unc_lds[];
    const int C = s.C, U = a.U, M = a.M, P = a.P, UM = U * M;
    unsigned long long* hpix = unc_lds;              // [U][M]: pixels | wrong pixels << 32
    unsigned long long* hpatch = unc_lds + UM;       // [U][M]: patches | inaccurate patches << 32
    for (int e = threadIdx.x; e < 2 * UM; e += blockDim.x) unc_lds[e] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool first = (lane & (P - 1)) == 0;        // the lane that commits its patch

    for (SegTiles tiles(s.B, s.H, s.W); tiles.more(); tiles.advance()) {
        const SegTile tile = tiles.get();
        const SegLane<IDENT> ln(s, tile);
        SegLabels label(labels, s, tile);
        float A[KP], Bv[KP], uA[UNC_MAX_MAPS], uB[UNC_MAX_MAPS];
#pragma unroll
        for (int m = 0; m < UNC_MAX_MAPS; ++m) uA[m] = uB[m] = 0.0f;
        int yA = -1, yB = -1, uyA = -1, uyB = -1;
        int Q[UNC_MAX_MAPS] = {0, 0, 0, 0}, ne = 0;  // down the rows of the lane's patch: sum of q per map; n | e << 16
        // no lane leaves this loop early: the wave helpers need all 64
        for (int y = tile.y_begin; y < tile.y_end; ++y) {
            float h0, h1;
            seg_step<KP, SRC, V4, IDENT>(A, Bv, yA, yB, h0, h1, s, ln, tile.b, y);
            unc_step<IDENT>(uA, uB, uyA, uyB, a, s, ln, tile.b, y);
            const int t = label.next(y);
            const bool valid = label.counted(t, C);
            const int pred = seg_argmax<KP, IDENT>(A, Bv, h0, h1, C);
            const bool wrong = valid && pred != t;
            ne += valid ? (1 | (wrong ? 1 << 16 : 0)) : 0;
            // the patch's last row, or the last row of the wave's part (y_begin is a multiple of SEG_ROWS, which P divides)
            const bool commit = (y & (P - 1)) == P - 1 || y == tile.y_end - 1;
            int n = 0, e = 0;
            if (commit) {
                const int sum = unc_patch_sum(ne, P);
                n = sum & 0xFFFF, e = sum >> 16;
                ne = 0;
            }
#pragma unroll
            for (int m = 0; m < UNC_MAX_MAPS; ++m) {
                if (m < U) {
                    const int q = unc_quantise(seg_value<IDENT>(uA[m], uB[m], h0, h1), a.range[m]);
                    unc_add(hpix + m * M, valid, min((q * M) >> 16, M - 1), wrong, lane);
                    Q[m] += valid ? q : 0;
                    if (commit) {
                        const unsigned Qs = (unsigned)unc_patch_sum(Q[m], P);       // <= 256 * 65536
                        Q[m] = 0;
                        const bool has = first && n > 0;
                        const int bin = has ? min((int)((unsigned)(((unsigned long long)Qs * (unsigned)M) >> 16) / (unsigned)n), M - 1) : 0;
                        unc_add(hpatch + m * M, has, bin, 2 * e >= n, lane);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * UM; e += blockDim.x) {
        const unsigned long long v = unc_lds[e];
        unsigned long long* out = e < UM ? pix + 2 * (size_t)e : patch + 2 * (size_t)(e - UM);
        if (v & 0xFFFFFFFFull) atomicAdd(&out[0], v & 0xFFFFFFFFull);
        if (v >> 32) atomicAdd(&out[1], v >> 32);
    }
}

}  // namespace ccdm

extern "C" size_t ccdm_uncscore_workspace_bytes(int, int, int, int, int, int) {
    return 0;           // the per-block tables live in LDS and go straight to the outputs
}

extern "C" int ccdm_uncscore(const float* probs, int64_t pixel_stride, const uint8_t* cls, const uint8_t* labels, const float* maps,
                             const float* ranges, int B, int h, int w, int H, int W, int K, int U, int M, int P, int64_t* pix, int64_t* patch,
                             void* workspace, size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    (void)workspace;
    (void)workspace_bytes;
    if (const int rc = seg_check_src("uncscore", probs, pixel_stride, cls, h, w, K)) return rc;
    if (const int rc = seg_check_out("uncscore", B, H, W)) return rc;
    CCDM_REQUIRE(labels, "uncscore: labels is null");
    CCDM_REQUIRE(maps, "uncscore: maps is null");
    CCDM_REQUIRE(ranges, "uncscore: ranges is null");
    CCDM_REQUIRE(pix && patch, "uncscore: pix or patch is null");
    CCDM_REQUIRE(U >= 1 && U <= UNC_MAX_MAPS, "uncscore: U=%d outside [1,%d]", U, UNC_MAX_MAPS);
    CCDM_REQUIRE(M >= 2 && M <= UNC_MAX_BINS, "uncscore: M=%d outside [2,%d]", M, UNC_MAX_BINS);
    CCDM_REQUIRE(P == 2 || P == 4 || P == 8 || P == 16, "uncscore: P=%d is not 2, 4, 8 or 16", P);
    UncArgs a{maps, {1.0f, 1.0f, 1.0f, 1.0f}, U, M, P};
    for (int m = 0; m < U; ++m) {
        CCDM_REQUIRE(ranges[m] > 0.0f, "uncscore: ranges[%d]=%g is not > 0", m, (double)ranges[m]);
        a.range[m] = ranges[m];
    }
    if (B == 0) return 0;
    if (const int rc = seg_check_block_counts("uncscore", B, H, W)) return rc;
    const int grid = seg_blocks(B, H, W);
    const SegSrc s = seg_src(probs, pixel_stride, cls, B, h, w, H, W, K - 1);
    const size_t lds = sizeof(unsigned long long) * 2 * (size_t)U * M;
    seg_dispatch(s, [&](auto kp, auto src, auto v4, auto ident) {
        hipLaunchKernelGGL((k_uncscore<kp(), src(), v4(), ident()>), dim3(grid), dim3(256), lds, (hipStream_t)stream, s, labels, a,
                           reinterpret_cast<unsigned long long*>(pix), reinterpret_cast<unsigned long long*>(patch));
    });
    CCDM_CHECK_LAUNCH("uncscore");
    return 0;
}
