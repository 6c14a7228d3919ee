// LIDC lesion findings of the sample SET, device part (beyond the reference): per image and scored class the lesions the S samples
// propose together (the connected components of the pixels at least n_min samples mark), how sure the set is of each (support, peak,
// mass), and the reference lesions of the raters (components of the pixels at least m_min raters mark) with the best candidate that
// touches each.  The definition in include/ccdm_hip.h is the contract; tests/detection_util.py restates it with numpy and
// tests/test_lidc_detection.py holds it against scipy.ndimage.label.
//
// Count stage (k_findings_count): a thread takes NPIX consecutive pixels of an image (NPIX = 4: one dword per stack row when
// W % 4 == 0 and both stacks are 4-byte aligned; NPIX = 1: bytes), walks the S samples and the L raters once per scored class (the
// first class reads HBM, the others the cache) and leaves n (a uint8 plane) and the two masks (uint8, 1 inside) in the workspace.
// Label stage (k_findings_label): one workgroup of 512 threads per (image, class, mask) runs les_label of ccdm_lesions_common.h on
// the mask plane: the labelling of ccdm_lesions, its arithmetic unchanged.  The invariant parent[p] <= p and why its loops end are
// stated there.  The counts go straight to the `counts` output.
// Bit stage (k_findings_bits): which samples and which raters have the class inside which candidate.  One workgroup of 256 threads per
// (image, class, group of 8 samples or 8 raters): it walks the candidate label plane, NPIX pixels a thread, and only where a pixel
// belongs to a candidate reads the group's 8 maps there (one dword or one byte each, independent loads) and ORs the 8 bits into the
// candidate's word of an LDS table (atomicOr); the low byte of every word goes to the workspace.  The stacks are read a second time,
// out of the cache, and only under the candidates; the work of a (image, class) spreads over ceil(S/8) + ceil(L/8) workgroups.
// Table stage (k_findings_tables): one workgroup of 256 threads per (image, class), tables in LDS for min(count, cap) records a side:
//   walk 1   per pixel of a candidate: LDS atomicAdd of size, mass, ref_cov and the coordinate sums, atomicMax / atomicMin of peak and
//            the box; per pixel of a reference lesion: atomicAdd of size and cov.
//   fold     support and rater_hits are the popcounts of the candidate's bytes of the bit stage.
//   walk 2   per pixel of a candidate that lies in a reference lesion: atomicMax of support and peak into the lesion's best_*; the
//            confidence map.
//   write    every row of cand and ref up to cap, zeros from the count on.
// A label above cap is skipped wherever a table is indexed: nothing outside the tables or the arrays is touched, and the counts stay
// true.  Every loop counts up to H*W, 8, cap or a group count: none depends on data.  Integers only, atomics on integers only: exact
// in any order, two identical calls are bit-identical.  No workgroup waits on another; no global atomics.
// LDS of a table workgroup: cap * (12 + 4) words = 64 B a record: FND_MAX_CAP = 1024 records are 65,536 B, two workgroups per CU (the
// CU has 160 KB); a bit workgroup takes cap words.
#include "ccdm_lesions_common.h"

namespace ccdm {

constexpr int FND_MAX_CAP = 1024;
constexpr int FND_CAND = 12, FND_REF = 4;  // int32 per record
constexpr int FND_THREADS = 256;          // of a count, a bit and a table workgroup

__host__ __device__ static inline int fnd_groups(int S, int L) { return (S + 7) / 8 + (L + 7) / 8; }      // of 8 samples, then of 8 raters

template <int NPIX>
__device__ __forceinline__ void fnd_count(const uint8_t* __restrict__ stack, int N, size_t HW, uint32_t c, int (&n)[NPIX]) {
    for (int s = 0; s < N; ++s) {
        if constexpr (NPIX == 4) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(stack + (size_t)s * HW);
#pragma unroll
            for (int j = 0; j < 4; ++j) n[j] += (v >> (8 * j) & 0xFFu) == c ? 1 : 0;
        } else {
            n[0] += stack[(size_t)s * HW] == c ? 1 : 0;
        }
    }
}

template <int NPIX>
__global__ __launch_bounds__(FND_THREADS) void k_findings_count(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters, int S, int L,
                                                               int C, int c0, int HW, int chunks, int n_min, int m_min,
                                                               uint8_t* __restrict__ nplane,
                                                               uint8_t* __restrict__ masks) {
    const size_t b = blockIdx.x / chunks;
    const int p0 = ((int)(blockIdx.x % chunks) * FND_THREADS + threadIdx.x) * NPIX;
    if (p0 >= HW) return;                                            // (HW % NPIX == 0: the whole group is inside)
    for (int ci = 0; ci < C; ++ci) {
        const uint32_t c = (uint32_t)(c0 + ci);
        int n[NPIX] = {}, m[NPIX] = {};
        fnd_count<NPIX>(samples + b * S * HW + p0, S, (size_t)HW, c, n);
        if (L > 0) fnd_count<NPIX>(raters + b * L * HW + p0, L, (size_t)HW, c, m);
        const size_t plane = b * C + ci;
        uint8_t* np = nplane + plane * HW + p0;
        uint8_t* ma = masks + plane * 2 * HW + p0;
        uint8_t* mr = ma + HW;
        if constexpr (NPIX == 4) {
            uint32_t vn = 0, va = 0, vr = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vn |= (uint32_t)n[j] << (8 * j);
                va |= (n[j] >= n_min ? 1u : 0u) << (8 * j);
                vr |= (L > 0 && m[j] >= m_min ? 1u : 0u) << (8 * j);
            }
            *reinterpret_cast<uint32_t*>(np) = vn;
            *reinterpret_cast<uint32_t*>(ma) = va;
            *reinterpret_cast<uint32_t*>(mr) = vr;
        } else {
            np[0] = (uint8_t)n[0];
            ma[0] = n[0] >= n_min ? 1 : 0;
            mr[0] = L > 0 && m[0] >= m_min ? 1 : 0;
        }
    }
}

template <int NPIX>
__global__ __launch_bounds__(LES_THREADS) void k_findings_label(const uint8_t* __restrict__ masks, int H, int W, int conn8, int32_t* __restrict__ labels,
                                                               int32_t* __restrict__ counts) {
    extern __shared__ int fnd_label_lds[];
    const size_t plane = blockIdx.x, HW = (size_t)H * W;
    les_label<NPIX>(fnd_label_lds, masks + plane * HW, 1u, H, W, conn8, labels + plane * HW, counts + plane);
}

template <int NPIX>
__global__ __launch_bounds__(FND_THREADS) void k_findings_bits(const uint8_t* __restrict__ samples, const uint8_t* __restrict__ raters,
                                                              const int32_t* __restrict__ labels, const int32_t* __restrict__ counts, int S, int L,
                                                              int C, int c0, int HW, int cap, uint8_t* __restrict__ bits) {
    extern __shared__ unsigned fnd_bit_tab[];                        // [cap]: bit s = map 8*group + s has the class inside the candidate
    const int GS = (S + 7) / 8, G = fnd_groups(S, L);
    const size_t bc = blockIdx.x / G, b = bc / C;
    const int g = (int)(blockIdx.x % G);
    const uint32_t c = (uint32_t)(c0 + (int)(bc % C));
    const int32_t* la = labels + bc * 2 * HW;
    const int n_c = counts[bc * 2];
    const int nc = n_c < cap ? n_c : cap;                            // records held; a label above them is skipped
    if (nc == 0) return;                                             // block-uniform: the table stage reads the first nc bytes only
    const bool rater_group = g >= GS;
    const int first = 8 * (rater_group ? g - GS : g);
    const int left = (rater_group ? L : S) - first, maps = left < 8 ? left : 8;
    const uint8_t* stack = (rater_group ? raters + b * L * HW : samples + b * S * HW) + (size_t)first * HW;
    for (int l = threadIdx.x; l < nc; l += FND_THREADS) fnd_bit_tab[l] = 0;
    __syncthreads();
    for (int p0 = threadIdx.x * NPIX; p0 < HW; p0 += FND_THREADS * NPIX) {     // (HW % NPIX == 0: the whole group is inside)
        int a[NPIX];
        bool any = false;
#pragma unroll
        for (int j = 0; j < NPIX; ++j) {
            a[j] = la[p0 + j];
            any = any || (a[j] >= 1 && a[j] <= nc);
        }
        if (!any) continue;
        unsigned v[NPIX] = {};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s < maps) {
                if constexpr (NPIX == 4) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(stack + (size_t)s * HW + p0);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((w >> (8 * j) & 0xFFu) == c) v[j] |= 1u << s;
                } else {
                    if (stack[(size_t)s * HW + p0] == c) v[0] |= 1u << s;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NPIX; ++j)
            if (a[j] >= 1 && a[j] <= nc && v[j]) atomicOr(fnd_bit_tab + a[j] - 1, v[j]);
    }
    __syncthreads();
    uint8_t* out = bits + (size_t)blockIdx.x * cap;
    for (int l = threadIdx.x; l < nc; l += FND_THREADS) out[l] = (uint8_t)fnd_bit_tab[l];
}

__global__ __launch_bounds__(FND_THREADS) void k_findings_tables(const int32_t* __restrict__ labels, const uint8_t* __restrict__ nplane,
                                                                const uint8_t* __restrict__ bits, const int32_t* __restrict__ counts, int S, int L,
                                                                int H, int W, int cap, int32_t* __restrict__ cand_out, int32_t* __restrict__ ref_out,
                                                                uint8_t* __restrict__ conf_map) {
    extern __shared__ int fnd_tab[];
    const int HW = H * W, GS = (S + 7) / 8, G = fnd_groups(S, L);
    int* cand = fnd_tab;                                             // [cap][12]
    int* ref = cand + cap * FND_CAND;                                // [cap][4]
    const size_t bc = blockIdx.x;
    const int32_t* la = labels + bc * 2 * HW;
    const int32_t* lr = la + HW;
    const uint8_t* np = nplane + bc * HW;
    const int n_c = counts[bc * 2], n_r = counts[bc * 2 + 1];
    const int nc = n_c < cap ? n_c : cap, nr = n_r < cap ? n_r : cap;      // records held; a label above them is skipped

    for (int i = threadIdx.x; i < nc * FND_CAND; i += FND_THREADS) {
        const int f = i % FND_CAND;
        cand[i] = f == 6 || f == 7 ? 0x7fffffff : f == 8 || f == 9 ? -1 : 0;
    }
    for (int i = threadIdx.x; i < nr * FND_REF; i += FND_THREADS) ref[i] = 0;
    __syncthreads();

    // walk 1
    for (int p = threadIdx.x; p < HW; p += FND_THREADS) {
        const int a = la[p], r = lr[p];                              // 1 .. n_c, 1 .. n_r, or 0
        if (r >= 1 && r <= nr) {
            atomicAdd(ref + (r - 1) * FND_REF, 1);
            if (a) atomicAdd(ref + (r - 1) * FND_REF + 1, 1);
        }
        if (a < 1 || a > nc) continue;
        int* rec = cand + (a - 1) * FND_CAND;
        const int n = np[p], y = p / W, x = p - y * W;
        atomicAdd(rec + 0, 1);
        atomicMax(rec + 2, n);
        atomicAdd(rec + 3, n);
        if (r) atomicAdd(rec + 4, 1);
        atomicMin(rec + 6, y);
        atomicMin(rec + 7, x);
        atomicMax(rec + 8, y);
        atomicMax(rec + 9, x);
        atomicAdd(rec + 10, y);
        atomicAdd(rec + 11, x);
    }
    __syncthreads();

    // fold
    for (int l = threadIdx.x; l < nc; l += FND_THREADS) {
        int support = 0, hits = 0;
        for (int g = 0; g < GS; ++g) support += __popc((unsigned)bits[(bc * G + g) * cap + l]);
        for (int g = GS; g < G; ++g) hits += __popc((unsigned)bits[(bc * G + g) * cap + l]);
        cand[l * FND_CAND + 1] = support;
        cand[l * FND_CAND + 5] = hits;
    }
    __syncthreads();

    // walk 2
    for (int p = threadIdx.x; p < HW; p += FND_THREADS) {
        const int a = la[p], r = lr[p];
        int support = 0;
        if (a >= 1 && a <= nc) {
            support = cand[(a - 1) * FND_CAND + 1];
            if (r >= 1 && r <= nr) {
                atomicMax(ref + (r - 1) * FND_REF + 2, support);
                atomicMax(ref + (r - 1) * FND_REF + 3, cand[(a - 1) * FND_CAND + 2]);
            }
        }
        if (conf_map) conf_map[bc * HW + p] = (uint8_t)support;
    }
    __syncthreads();

    // write
    int32_t* co = cand_out + bc * cap * FND_CAND;
    int32_t* ro = ref_out + bc * cap * FND_REF;
    for (int i = threadIdx.x; i < cap * FND_CAND; i += FND_THREADS) co[i] = i < nc * FND_CAND ? cand[i] : 0;
    for (int i = threadIdx.x; i < cap * FND_REF; i += FND_THREADS) ro[i] = i < nr * FND_REF ? ref[i] : 0;
}

}  // namespace ccdm

extern "C" size_t ccdm_findings_workspace_bytes(int B, int S, int L, int H, int W, int K, int cap) {
    if (B <= 0 || S <= 0 || L < 0 || H <= 0 || W <= 0 || K <= 0 || cap <= 0) return 0;
    return (size_t)B * ccdm::les_classes(K) * ((size_t)11 * H * W + (size_t)ccdm::fnd_groups(S, L) * cap);
}

extern "C" int ccdm_findings(const uint8_t* samples, const uint8_t* raters, int B, int S, int L, int H, int W, int K, int connectivity,
                             int n_min, int m_min, int cap, int32_t* counts, int32_t* cand, int32_t* ref, uint8_t* conf_map, void* workspace,
                             size_t workspace_bytes, void* stream) {
    using namespace ccdm;
    CCDM_REQUIRE(K >= 1 && K <= SEG_MAX_K, "findings: K=%d outside [1,%d]", K, SEG_MAX_K);
    CCDM_REQUIRE(S >= 1 && S <= 255, "findings: S=%d outside [1,255]", S);
    CCDM_REQUIRE(L >= 0 && L <= 255, "findings: L=%d outside [0,255]", L);
    CCDM_REQUIRE(H >= 1, "findings: H=%d below 1", H);
    CCDM_REQUIRE(W >= 1, "findings: W=%d below 1", W);
    CCDM_REQUIRE((long long)H * W <= LES_MAX_PIXELS, "findings: H*W=%lld above %d", (long long)H * W, LES_MAX_PIXELS);
    CCDM_REQUIRE(connectivity == 4 || connectivity == 8, "findings: connectivity=%d (expected 4 or 8)", connectivity);
    CCDM_REQUIRE(n_min >= 1 && n_min <= S, "findings: n_min=%d outside [1,S=%d]", n_min, S);
    CCDM_REQUIRE(L == 0 || (m_min >= 1 && m_min <= L), "findings: m_min=%d outside [1,L=%d]", m_min, L);
    CCDM_REQUIRE(cap >= 1 && cap <= FND_MAX_CAP, "findings: cap=%d outside [1,%d]", cap, FND_MAX_CAP);
    CCDM_REQUIRE(B >= 0, "findings: B=%d", B);
    CCDM_REQUIRE((L == 0) == (raters == nullptr), "findings: raters %s with L=%d", raters ? "given" : "null", L);
    if (B == 0) return 0;
    const int C = les_classes(K), c0 = K > 1 ? 1 : 0, HW = H * W;
    const long long cells = (long long)B * C;
    CCDM_REQUIRE(cells * 2 <= 0x7fffffffLL && cells * fnd_groups(S, L) <= 0x7fffffffLL, "findings: B=%d images (too many blocks)", B);
    CCDM_REQUIRE(samples && counts && cand && ref, "findings: null pointer");
    const size_t need = ccdm_findings_workspace_bytes(B, S, L, H, W, K, cap);
    CCDM_REQUIRE(workspace && workspace_bytes >= need, "findings: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    CCDM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "findings: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* labels = static_cast<int32_t*>(workspace);             // [B][C][2][HW]
    uint8_t* nplane = reinterpret_cast<uint8_t*>(labels + (size_t)cells * 2 * HW);      // [B][C][HW]
    uint8_t* masks = nplane + (size_t)cells * HW;                    // [B][C][2][HW]
    uint8_t* bits = masks + (size_t)cells * 2 * HW;                  // [B][C][groups][cap]
    const int G = fnd_groups(S, L);
    const int conn8 = connectivity == 8 ? 1 : 0;
    const bool rows4 = W % 4 == 0;                                   // the planes of the workspace are then 4-byte aligned
    const bool vec = rows4 && ((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(raters)) & 3) == 0;
    const int chunks = cdiv(HW, FND_THREADS * (vec ? 4 : 1));
    CCDM_REQUIRE((long long)B * chunks <= 0x7fffffffLL, "findings: B=%d images (too many blocks)", B);
    if (vec)
        hipLaunchKernelGGL(k_findings_count<4>, dim3((unsigned)(B * chunks)), dim3(FND_THREADS), 0, st, samples, raters, S, L, C, c0, HW, chunks,
                           n_min, m_min, nplane, masks);
    else
        hipLaunchKernelGGL(k_findings_count<1>, dim3((unsigned)(B * chunks)), dim3(FND_THREADS), 0, st, samples, raters, S, L, C, c0, HW, chunks,
                           n_min, m_min, nplane, masks);
    CCDM_CHECK_LAUNCH("findings count");
    const size_t label_lds = les_label_lds(HW);
    static bool reserved[3] = {false, false, false};
    if (rows4) {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_findings_label<4>, LES_LABEL_LDS_MAX, &reserved[0], "findings label") < 0) return -1;
        hipLaunchKernelGGL(k_findings_label<4>, dim3((unsigned)(cells * 2)), dim3(LES_THREADS), label_lds, st, masks, H, W, conn8, labels, counts);
    } else {
        if (label_lds > 48 * 1024 && les_reserve_lds(k_findings_label<1>, LES_LABEL_LDS_MAX, &reserved[1], "findings label") < 0) return -1;
        hipLaunchKernelGGL(k_findings_label<1>, dim3((unsigned)(cells * 2)), dim3(LES_THREADS), label_lds, st, masks, H, W, conn8, labels, counts);
    }
    CCDM_CHECK_LAUNCH("findings label");
    if (vec)
        hipLaunchKernelGGL(k_findings_bits<4>, dim3((unsigned)(cells * G)), dim3(FND_THREADS), (size_t)cap * sizeof(unsigned), st, samples, raters, labels,
                           counts, S, L, C, c0, HW, cap, bits);
    else
        hipLaunchKernelGGL(k_findings_bits<1>, dim3((unsigned)(cells * G)), dim3(FND_THREADS), (size_t)cap * sizeof(unsigned), st, samples, raters, labels,
                           counts, S, L, C, c0, HW, cap, bits);
    CCDM_CHECK_LAUNCH("findings bits");
    const size_t table_lds = (size_t)cap * (FND_CAND + FND_REF) * sizeof(int);
    if (table_lds > 48 * 1024 && les_reserve_lds(k_findings_tables, (size_t)FND_MAX_CAP * (FND_CAND + FND_REF) * sizeof(int), &reserved[2], "findings table") < 0)
        return -1;
    hipLaunchKernelGGL(k_findings_tables, dim3((unsigned)cells), dim3(FND_THREADS), table_lds, st, labels, nplane, bits, counts, S, L, H, W, cap, cand,
                       ref, conf_map);
    CCDM_CHECK_LAUNCH("findings tables");
    return 0;
}
