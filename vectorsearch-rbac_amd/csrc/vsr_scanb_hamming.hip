// vsr_scanb_hamming.hip — instantiates the K1b scan kernels (K1 over a bit corpus, vsr_scanb.h) for one metric.
#include "vsr_scanb.h"

namespace vsr {

hipError_t launch_scanb_hamming(const ScanParams& p, int dim, int qb, uint32_t n_blocks, hipStream_t s)
{
    return launch_scanb_metric<false>(p, dim, qb, n_blocks, s);
}

}  // namespace vsr
