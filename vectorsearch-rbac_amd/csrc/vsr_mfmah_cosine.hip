// vsr_mfmah_cosine.hip — instantiates the K2h screening kernels (K2 over a halfvec corpus, vsr_mfmah.h) for one metric.
#include "vsr_mfmah.h"

namespace vsr {

hipError_t launch_mfmah_cosine(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_mfmah_metric<M_COSINE>(p, n_blocks, s);
}

}  // namespace vsr
