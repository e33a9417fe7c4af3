// vsr_mfmahw_ip.hip — instantiates the K2hw kernels (workgroup-shared f16 MFMA passes over a halfvec corpus, vsr_mfmahw.h) for one metric.
#include "vsr_mfmahw.h"

namespace vsr {

hipError_t launch_mfmahw_ip(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_mfmahw_metric<M_IP>(p, n_blocks, s);
}

}  // namespace vsr
