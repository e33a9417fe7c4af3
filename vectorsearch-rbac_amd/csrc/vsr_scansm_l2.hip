// vsr_scansm_l2.hip — instantiates the K1sm kernels (shared passes over a sparse corpus, vsr_scansm.h) for one metric.
#include "vsr_scansm.h"

namespace vsr {

hipError_t launch_scansm_l2(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_scansm_metric<M_L2>(p, n_blocks, s);
}

}  // namespace vsr
