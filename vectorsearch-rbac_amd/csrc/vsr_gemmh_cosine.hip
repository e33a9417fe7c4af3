// vsr_gemmh_cosine.hip — instantiates the K2gh kernels (256-query f16 GEMM passes over a halfvec corpus's long rows, vsr_gemmh.h) for one metric.
#include "vsr_gemmh.h"

namespace vsr {

hipError_t launch_gemmh_cosine(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_gemmh_metric<M_COSINE>(p, n_blocks, s);
}

}  // namespace vsr
