// What the lesion kernels share: the limits, the scored classes and the layout of the workspace ccdm_lesions leaves behind.
// Users: ccdm_lesions.hip (writes the label planes and the lesion counts), ccdm_lesionmatch.hip (reads them).
#pragma once
#include "ccdm_seg_common.h"

namespace ccdm {

constexpr int LES_MAX_PIXELS = 16384;     // H*W: a map and its bookkeeping stay in the LDS of one workgroup; size and cov fit 16 bits
constexpr int LES_MAX_T = 8;              // thresholds of one call, by value in the kernel arguments
constexpr int LES_MAX_DEN = 65536;

static inline int les_classes(int K) { return K > 1 ? K - 1 : 1; }
// A conn-4 checkerboard has ceil(H*W/2) lesions, the most any mask can have: one pixel of each lesion is an independent set of the grid.
static inline int les_max_lesions(int HW) { return (HW + 1) / 2; }

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

}  // namespace ccdm
