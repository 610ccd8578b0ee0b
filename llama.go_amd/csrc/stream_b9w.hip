// csrc/stream_b9w.hip — the instantiations of k_stream_b9w (kernels_stream_b9w.h) and of k_stream_b9w_h, its form over the halves of an f16 model
// (kernels_stream_b9w_h.h), in a translation unit of their own, built with the packed fp32
// instructions turned off (Makefile, B9WFLAGS): the sums of the epilogue inlined into the kernel are issued as the single fp32 adds the source spells,
// in the order it spells them.  plan.hip (launch_stream_b9w) asks for a kernel by its row-tile and column-tile counts and launches it like any other.
// The kernel headers also define the library's non-template kernels, which plan.hip defines already: this unit compiles them under a namespace of its
// own (lh_b9w_tu instead of lh), so nothing in it collides with the library's symbols; StreamArgs has the same layout under either name.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <vector>
#define lh lh_b9w_tu
#include "kernels_stream_b9w.h"
#include "kernels_stream_b9w_h.h"

// -DB9WH_PRODUCTS=8 issues the two products of the weights' zero part as well (the fallback, had six not been byte-equal on the GPU)
#ifndef B9WH_PRODUCTS
#define B9WH_PRODUCTS 6
#endif

namespace lh {

typedef void (*StreamB9wKernel)(const StreamArgs);
template <int MAXT, int NCT>
static StreamB9wKernel b9w_kernel_of(int wdt, int* nimg, int* nprod) {
    if constexpr (!b9w_built(MAXT, NCT)) return nullptr;
    else if (wdt == 1) {                           // halves: the same (MAXT, NCT), a ring of its own depth
        constexpr int NIMGH = b9wh_nimg(MAXT, NCT, 4);
        *nimg = NIMGH; *nprod = B9WH_PRODUCTS;
        return k_stream_b9w_h<MAXT, NCT, NIMGH, B9WH_PRODUCTS>;
    } else {
        constexpr int NIMG = b9w_nimg(MAXT, NCT, 4);
        *nimg = NIMG; *nprod = 8;
        return k_stream_b9w<MAXT, NCT, NIMG, 8>;   // eight products: B9S_PRODUCTS (plan.hip)
    }
}
template <int MAXT>
static StreamB9wKernel b9w_kernel_nct(int nct, int wdt, int* nimg, int* nprod) {
    switch (nct) {
        case 5: return b9w_kernel_of<MAXT, 5>(wdt, nimg, nprod);
        case 6: return b9w_kernel_of<MAXT, 6>(wdt, nimg, nprod);
        case 7: return b9w_kernel_of<MAXT, 7>(wdt, nimg, nprod);
        case 8: return b9w_kernel_of<MAXT, 8>(wdt, nimg, nprod);
        default: return nullptr;
    }
}
// the kernel for maxt row tiles per workgroup (1, 2, 3, 4, 6, 8) next to nct column tiles (5..8) over fp32 weights (wdt 0) or halves (wdt 1), the depth of
// its ring and its product count; nullptr: not built
const void* stream_b9w_kernel(int maxt, int nct, int wdt, int* nimg, int* nprod) {
    switch (maxt) {
        case 1: return (const void*)b9w_kernel_nct<1>(nct, wdt, nimg, nprod);
        case 2: return (const void*)b9w_kernel_nct<2>(nct, wdt, nimg, nprod);
        case 3: return (const void*)b9w_kernel_nct<3>(nct, wdt, nimg, nprod);
        case 4: return (const void*)b9w_kernel_nct<4>(nct, wdt, nimg, nprod);
        case 6: return (const void*)b9w_kernel_nct<6>(nct, wdt, nimg, nprod);
        case 8: return (const void*)b9w_kernel_nct<8>(nct, wdt, nimg, nprod);
        default: return nullptr;
    }
}

}  // namespace lh
