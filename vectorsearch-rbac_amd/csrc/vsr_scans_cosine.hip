// vsr_scans_cosine.hip — instantiates the K1s scan kernels (K1 over a sparse corpus, vsr_scans.h) for one metric.
#include "vsr_scans.h"

namespace vsr {

hipError_t launch_scans_cosine(const ScanParams& p, int lpr, int qi, bool global_tab, uint32_t n_blocks, hipStream_t s)
{
    return launch_scans_metric<M_COSINE>(p, lpr, qi, global_tab, n_blocks, s);
}

}  // namespace vsr
