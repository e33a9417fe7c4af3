// vsr_gemmh_l2.hip — instantiates the K2gh kernels (256-query f16 GEMM passes over a halfvec corpus's long rows, vsr_gemmh.h) for one metric.
#include "vsr_gemmh.h"

namespace vsr {

hipError_t launch_gemmh_l2(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_gemmh_metric<M_L2>(p, n_blocks, s);
}

}  // namespace vsr
