// vsr_scansi_ip.hip — instantiates the K1si kernel (passes over a sparse corpus's inverted image, vsr_scansi.h) for one metric.
#include "vsr_scansi.h"

namespace vsr {

hipError_t launch_scansi_ip(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_scansi_metric<M_IP>(p, n_blocks, s);
}

}  // namespace vsr
