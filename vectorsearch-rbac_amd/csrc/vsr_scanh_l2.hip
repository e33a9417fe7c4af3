// vsr_scanh_l2.hip — instantiates the K1h scan kernels (K1 over a halfvec corpus, vsr_scan.h) for one metric.
#include "vsr_scan.h"

namespace vsr {

hipError_t launch_scanh_l2(const ScanParams& p, int dim, int qb, uint32_t n_blocks, hipStream_t s)
{
    return launch_scan_metric<M_L2, true>(p, dim, qb, n_blocks, s);
}

}  // namespace vsr
