// vsr_scansm_cosine.hip — instantiates the K1sm kernels (shared passes over a sparse corpus, vsr_scansm.h) for one metric.
#include "vsr_scansm.h"

namespace vsr {

hipError_t launch_scansm_cosine(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_scansm_metric<M_COSINE>(p, n_blocks, s);
}

}  // namespace vsr
