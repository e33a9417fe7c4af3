// vsr_scansc_l1.hip — instantiates the K1sc kernels (shared passes over a sparse corpus, compact query block, vsr_scansc.h) for one metric.
#include "vsr_scansc.h"

namespace vsr {

hipError_t launch_scansc_l1(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_scansc_metric<M_L1>(p, n_blocks, s);
}

}  // namespace vsr
