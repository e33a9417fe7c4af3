// vsr_mfmah_l2.hip — instantiates the K2h screening kernels (K2 over a halfvec corpus, vsr_mfmah.h) for one metric.
#include "vsr_mfmah.h"

namespace vsr {

hipError_t launch_mfmah_l2(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_mfmah_metric<M_L2>(p, n_blocks, s);
}

}  // namespace vsr
