// vsr_ivf_lds.h — the LDS budgets of the per-query list scans: K3i (ivf_iterative_kernel, vsr_ivf_iter.h) and K3q
// (ivf_bit_shortlist_kernel, vsr_ivf_shortlist.h).  Plain C++ with no HIP header behind it, so that the host compiler can build
// it alone (tests/test_ivf_quantized_cpu.py restates the formulas); the launchers and the kernels' carves read these.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VSR_IVF_HD __host__ __device__
#else
#define VSR_IVF_HD
#endif

namespace vsr {

constexpr uint32_t IVI_CHUNK = 512;          // appended keys between two folds (>= 2 x the 256 a workgroup step can append)
constexpr uint32_t IVI_MIN_KEPT = 512;       // the fold reads kept[SK - 1 - j], j < IVI_CHUNK

VSR_IVF_HD inline uint32_t ivf_iter_kept(uint32_t k)
{
    uint32_t sk = IVI_MIN_KEPT;
    while (sk < k) sk <<= 1;
    return sk;
}
// (bit: the view of a bit corpus -- stride4 is its chunks per row -- whose waves also keep the 64 counts of a step)
inline size_t ivf_iter_lds_bytes(uint32_t lists, uint32_t stride4, uint32_t k, bool bit = false)
{
    return (((size_t) lists * 4 + 15) & ~(size_t) 15) + (size_t) stride4 * 16 + (bit ? 2 : 1) * 4 * 64 * 4 + (size_t) (ivf_iter_kept(k) + IVI_CHUNK) * 8 + 64;
}
// K3q: lists * 4 centre keys (rounded up to 16) + the packed query (chunks x 16 bytes, chunks = ceil(bits / 128), made in LDS
// from the fp32 query) + 4 x 64 row slots + 4 x 64 counts + kept (ivf_iter_kept(shortlist) keys, <= 16 KiB) + chunk (4 KiB) +
// 64 bytes of control words.  The carve of K3i's bit form with k = shortlist: 1000 lists x 768 bits x shortlist 400 is 14 400
// bytes; the largest shape the entry point admits, 32768 lists x 64000 bits x 2048, is 161 664, inside the CU's 160 KiB (the
// launcher still refuses what would not fit)
inline size_t ivf_shortlist_lds_bytes(uint32_t lists, uint32_t chunks, uint32_t shortlist)
{
    return (((size_t) lists * 4 + 15) & ~(size_t) 15) + (size_t) chunks * 16 + 4 * 64 * 4 + 4 * 64 * 4 + (size_t) ivf_iter_kept(shortlist) * 8 +
           (size_t) IVI_CHUNK * 8 + 64;
}

}  // namespace vsr
