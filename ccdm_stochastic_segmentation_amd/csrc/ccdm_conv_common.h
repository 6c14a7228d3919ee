// Device helpers of the conv kernels (ccdm_conv.hip and its specialisations); the GroupNorm half lives in ccdm_gn.h.
#pragma once
#include "ccdm_common.h"
#include "ccdm_gn.h"

namespace ccdm {

static constexpr float ACT_PRESCALE = 16.0f;       // F16X3 activation pre-scale (power of two)

// LDS layout of the conv kernels, shared with the host code that sizes their launches.
// Staged pixel of ck channels: F32 33 floats (odd stride: conflict-free column reads); F16X3 ck hi halfs | ck lo halfs | 16 B pad,
// e.g. 80 B = 20 dwords at 16 channels: the 16 pixels of a ds_read_b128 lane group land on 16 disjoint 4-bank slots (20*p mod 64);
// 144 B = 36 dwords at 32 channels, also conflict-free.
constexpr int PIX_F32 = 33;
constexpr int conv_pixb(int prec, int ck) { return prec == CCDM_PREC_F32 ? PIX_F32 * 4 : ck * 4 + 16; }      // bytes
constexpr int EPI_ROW = 36;                        // floats per pixel row of the epilogues' transpose buffers (16-B aligned rows)
// packed weight fragments of one (tap, k-step, n-tile): [hi|lo][64 lanes] x 16 B
constexpr int FRAG_ITEMS = 128, FRAG_BYTES = FRAG_ITEMS * 16;
// (The steps the four conv files repeat — the masked split-and-store of a staged quad, the lo*hi, hi*lo, hi*hi MFMA triple, the XCD
//  block remap, the fp64 reduce-scatter over xor 32 / 16 / 8 — stay written out at each site: as __forceinline__ helpers here they
//  changed the register allocation of k_conv and the schedule of k_conv_ks, k_upconv and k_conv1x1, profiles/r11_conv_refactor_isa.txt.)

// Load 16 bytes from global memory at (wave-uniform pointer + 32-bit per-lane byte offset).  The pointer is passed
// through readfirstlane so the compiler must keep it in scalar registers and select the saddr + voffset addressing
// form: no 64-bit vector adds, one VGPR of address per load.
typedef const __attribute__((address_space(1))) char* gptr_t;
__device__ __forceinline__ f32x4 load16_uniform_base(const char* base, unsigned voff) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    gptr_t g = reinterpret_cast<gptr_t>(((unsigned long long)hi << 32) | lo);
    return *reinterpret_cast<const __attribute__((address_space(1))) f32x4*>(g + voff);
}

// Load 16 bytes of GLOBAL memory through a pointer whose address space the compiler cannot see (rebuilt from integers / register
// lanes).  Left generic it becomes flat_load, which also counts in LGKM_CNT: the wave's next LDS wait (s_waitcnt lgkmcnt) then waits
// for this memory round trip too, and with a flat load pending the waitcnt pass can no longer count vector loads in order (vmcnt(N)
// becomes vmcnt(0)).
__device__ __forceinline__ f32x4 load16_global(const char* p) {
    return *reinterpret_cast<const __attribute__((address_space(1))) f32x4*>(reinterpret_cast<unsigned long long>(p));
}

// NT: non-temporal (streaming) store — the line is marked evict-first in L2
template <bool NT = false>
__device__ __forceinline__ void store16_uniform_base(char* base, unsigned voff, const f32x4 v) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    __attribute__((address_space(1))) char* g = reinterpret_cast<__attribute__((address_space(1))) char*>(((unsigned long long)hi << 32) | lo);
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<__attribute__((address_space(1))) f32x4*>(g + voff));
    else *reinterpret_cast<__attribute__((address_space(1))) f32x4*>(g + voff) = v;
}
// fp16 hi/lo split of two fp32 values: hi = RNE(x) packed, lo = RNE(x - hi) packed.  x - hi is one v_fma_mix_f32 (the fp16 half is
// read straight out of the packed register and widened by the instruction: fma(hi, -1, x), exactly the subtraction's single rounding),
// instead of an unpack (v_cvt_f32_f16) plus a subtract per element: 4 VALU instructions per pair instead of 7.
__device__ __forceinline__ void split2_f16(const float a, const float b, unsigned& hi, unsigned& lo) {
    float la, lb;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(la) : "v"(hi), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(lb) : "v"(hi), "v"(b));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo) : "v"(la), "v"(lb));
}

struct ConvK {   // kernel-side copy of ccdm_conv_args (+ derived)
    ccdm_conv_args a;
    int cin_pad, ntiles, slices, tiles_x, tiles_y;
    int cin_pad_skip;        // padded channels of the fused 1x1 skip segment (0: none)
    int skip_wide;           // the skip segment runs in 32-channel chunks staged core-pixels-only (wide-tile F16X3 variant, SC % 32 == 0)
    const float* wscale;     // F16X3: [ntiles*32] powers of two undoing the per-output-channel weight pre-scale
    int core_unmasked;       // every core column of every tile lies inside the image and every channel quad exists (W % TW == 0, C % CK == 0):
                             // core halo items need no per-lane padding mask, only the wave-uniform row test
};

// The launch plan of one conv call: what ccdm_conv_plan reports (include/ccdm_hip.h) plus what only the launchers need.  conv_plan
// (ccdm_conv.hip) is the one place where a launch decision is taken — kernel family, tiling, chunk width, n-tiles per block, grid —
// and launch_conv / launch_upconv / launch_conv1x1 / launch_conv_ks run what it says.  Host code: it follows no pointer of the call.
struct ConvPlan : ccdm_conv_plan_info {
    ConvGeo g;               // tile geometry of the general kernel and of the sub-pixel form
    int cin_pad, cin_pad_skip;
    size_t wscale_off;       // byte offset of the F16X3 per-channel scale table behind the packed fragments of `w`
};
int conv_plan(const ccdm_conv_args& a, ConvPlan& p);

// plain 1x1 conv (+bias +residual +statistics) of a low-resolution tensor without LDS staging (ccdm_conv1x1.hip)
bool conv1x1_eligible(const ccdm_conv_args& a, int slices);
void conv1x1_plan(const ccdm_conv_args& a, ConvPlan& p);          // p.slices: the general rule's slices on entry, this kernel's pixel blocks on return
int launch_conv1x1(const ccdm_conv_args& a, const ConvPlan& p, const float* wscale, hipStream_t s);

// 3x3 conv of a few-pixel image, K split over the waves of a block, weight fragments straight from L2 (ccdm_conv_ks.hip)
bool conv_ks_eligible(const ccdm_conv_args& a);
int conv_ks_slices(const ccdm_conv_args& a);            // statistics slices that kernel leaves (one per 8x8 tile)
bool conv_ks_describe(const ccdm_conv_args& a, ConvPlan& p);     // fills p from the plan launch_conv_ks runs; false = not for this kernel
int launch_conv_ks(const ccdm_conv_args& a, int ntiles, const float* wscale, hipStream_t s);
// Upsample + conv 3x3 in sub-pixel form at the low-resolution decoder levels: wave = phase, weight fragments straight from L2 (ccdm_upconv.hip)
bool upconv_eligible(const ccdm_conv_args& a);
void upconv_plan(const ccdm_conv_args& a, ConvPlan& p);
int launch_upconv(const ccdm_conv_args& a, const ConvPlan& p, const float* wscale, hipStream_t s);

}  // namespace ccdm
