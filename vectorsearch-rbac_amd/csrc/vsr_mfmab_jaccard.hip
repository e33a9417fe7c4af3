// vsr_mfmab_jaccard.hip — instantiates the K2b kernels (K2 over a bit corpus on the int8 matrix cores, vsr_mfmab.h) for one metric.
#include "vsr_mfmab.h"

namespace vsr {

hipError_t launch_mfmab_jaccard(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    return launch_mfmab_metric<true>(p, n_blocks, s);
}

}  // namespace vsr
