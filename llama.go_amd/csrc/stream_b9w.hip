// csrc/stream_b9w.hip — the instantiations of k_stream_b9w (kernels_stream_b9w.h) in a translation unit of their own, built with the packed fp32
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

namespace lh {

typedef void (*StreamB9wKernel)(const StreamArgs);
template <int MAXT, int NCT>
static StreamB9wKernel b9w_kernel_of(int* nimg) {
    if constexpr (!b9w_built(MAXT, NCT)) return nullptr;
    else {
        constexpr int NIMG = b9w_nimg(MAXT, NCT, 4);
        *nimg = NIMG;
        return k_stream_b9w<MAXT, NCT, NIMG, 8>;   // eight products: B9S_PRODUCTS (plan.hip)
    }
}
template <int MAXT>
static StreamB9wKernel b9w_kernel_nct(int nct, int* nimg) {
    switch (nct) {
        case 5: return b9w_kernel_of<MAXT, 5>(nimg);
        case 6: return b9w_kernel_of<MAXT, 6>(nimg);
        case 7: return b9w_kernel_of<MAXT, 7>(nimg);
        case 8: return b9w_kernel_of<MAXT, 8>(nimg);
        default: return nullptr;
    }
}
// the kernel for maxt row tiles per workgroup (1, 2, 3, 4, 6, 8) next to nct column tiles (5..8) and the depth of its ring; nullptr: not built
const void* stream_b9w_kernel(int maxt, int nct, int* nimg) {
    switch (maxt) {
        case 1: return (const void*)b9w_kernel_nct<1>(nct, nimg);
        case 2: return (const void*)b9w_kernel_nct<2>(nct, nimg);
        case 3: return (const void*)b9w_kernel_nct<3>(nct, nimg);
        case 4: return (const void*)b9w_kernel_nct<4>(nct, nimg);
        case 6: return (const void*)b9w_kernel_nct<6>(nct, nimg);
        case 8: return (const void*)b9w_kernel_nct<8>(nct, nimg);
        default: return nullptr;
    }
}

}  // namespace lh
