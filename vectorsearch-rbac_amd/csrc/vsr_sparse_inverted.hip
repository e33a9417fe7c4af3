// vsr_sparse_inverted.hip — the inverted image of a sparse corpus (what K1si walks, vsr_scansi.h), built on the GPU from the
// resident CSR rows:
//
//   1. si_key_kernel       one thread per stored entry: its row (by binary search in the row offsets), the 64-bit key
//                          (row block, index, row in block) -- a pad entry gets the row block one past the last -- and the
//                          value beside it; si_row_sums_kernel: A2 = sum a^2 and A1 = sum |a| per row, double, entry order
//   2. hipCUB radix sort   (key, value) pairs over the key's used bits: postings ordered by (block, index, row)
//   3. si_mark_kernel, an exclusive scan, si_write_kernel
//                          an entry whose (block, index) differs from its predecessor's opens a segment: bterm and boff get an
//                          element, numbered by the scan; an entry whose block differs closes the blocks before it (their end
//                          sentinel in boff, the begin of the next block's run in bbeg), also the blocks that hold no entry
//
// Layout and sizes: sparse_inverted_bytes (vsr_scansi_sizing.h).  Nothing is sized by the corpus's dimension.  Scratch: two
// (key, value) buffers, the segment flags and their scan in the idle key buffer, hipCUB's own -- about 24 bytes per stored entry,
// freed before the call returns.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "vsr_device.h"
#include "vsr_scansi_sizing.h"

namespace vsr {

constexpr int SI_KEY_BLOCK_SHIFT = SI_KEY_INDEX_BITS + (int) SI_RB_LOG2;

// the row block a key names, at most n_blocks (the pads')
__device__ __forceinline__ uint32_t si_key_block(uint64_t key, uint32_t n_blocks)
{
    const uint64_t b = key >> SI_KEY_BLOCK_SHIFT;
    return b < n_blocks ? (uint32_t) b : n_blocks;
}

__global__ __launch_bounds__(256) void si_key_kernel(const uint2* __restrict__ ent, const uint64_t* __restrict__ sp_off, uint64_t entries,
                                                     uint32_t n_rows, uint32_t n_blocks, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint64_t e = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    uint32_t lo = 0, hi = n_rows;                                             // the row: the last one whose first entry is <= e
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sp_off[mid] <= e) lo = mid; else hi = mid;
    }
    const uint2 x = ent[e];
    const bool pad = x.x == SPARSE_EMPTY || x.x >= (1u << SI_KEY_INDEX_BITS);  // (the second: cannot happen, dim <= 10^9)
    keys[e] = pad ? (uint64_t) n_blocks << SI_KEY_BLOCK_SHIFT
                  : ((uint64_t) (lo >> SI_RB_LOG2) << SI_KEY_BLOCK_SHIFT) | ((uint64_t) x.x << SI_RB_LOG2) | (lo & (SI_RB - 1u));
    vals[e] = pad ? 0u : x.y;
}

__global__ __launch_bounds__(256) void si_row_sums_kernel(const uint2* __restrict__ ent, const uint64_t* __restrict__ sp_off, uint32_t n_rows,
                                                          double* __restrict__ a)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    double a2 = 0.0, a1 = 0.0;
    for (uint64_t e = sp_off[r]; e < sp_off[r + 1]; ++e) {                    // (a pad entry's value is 0)
        const double v = (double) __uint_as_float(ent[e].y);
        a2 += v * v;
        a1 += fabs(v);
    }
    a[r] = a2;
    a[(size_t) n_rows + r] = a1;
}

// i in [0, entries]: does sorted entry i open a (block, index) segment (the one-past element: no)
__global__ __launch_bounds__(256) void si_mark_kernel(const uint64_t* __restrict__ keys, uint64_t entries, uint32_t n_blocks, uint32_t* __restrict__ flag)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > entries) return;
    bool f = false;
    if (i < entries) {
        const uint64_t k = keys[i];
        f = si_key_block(k, n_blocks) < n_blocks && (i == 0 || (keys[i - 1] >> SI_RB_LOG2) != (k >> SI_RB_LOG2));
    }
    flag[i] = f ? 1u : 0u;
}

__global__ __launch_bounds__(256) void si_write_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ pos, uint64_t entries, uint32_t n_blocks, uint2* __restrict__ post,
                                                       uint32_t* __restrict__ bterm, uint64_t* __restrict__ boff, uint32_t* __restrict__ bbeg)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > entries) return;
    const uint32_t t = pos[i];
    uint32_t cb = n_blocks;                                                    // block of entry i; the pads' and the one-past element's: n_blocks
    if (i < entries) {
        const uint64_t k = keys[i];
        cb = si_key_block(k, n_blocks);
        post[i] = make_uint2((uint32_t) k & (SI_RB - 1u), vals[i]);
        if (flag[i]) {
            bterm[t] = (uint32_t) (k >> SI_RB_LOG2) & ((1u << SI_KEY_INDEX_BITS) - 1u);
            boff[(size_t) t + cb] = i;
        }
    }
    const int64_t pb = i == 0 ? -1 : (int64_t) si_key_block(keys[i - 1], n_blocks);
    if ((int64_t) cb > pb) {                                                   // blocks [pb, cb) end here, blocks (pb, cb] begin here
        for (int64_t b = pb + 1; b <= (int64_t) cb; ++b) bbeg[b] = t;
        for (int64_t b = pb < 0 ? 0 : pb; b < (int64_t) cb; ++b) boff[(size_t) t + (size_t) b] = i;
    }
}

namespace {
struct SiMem {                                                                // the build's scratch, freed on every way out
    void* p = nullptr;
    ~SiMem() { if (p) (void) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
inline dim3 si_blocks(uint64_t n) { return dim3((uint32_t) std::max<uint64_t>(1, (n + 255) / 256)); }
}  // namespace

#define SI_CHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void) hipStreamSynchronize(s); free_out(); return e_; } } while (0)

// entries + 1 < 2^31 (hipCUB counts in int; the caller refuses more).  On an error nothing is left allocated
hipError_t build_sparse_inverted(const float4* rows, const uint64_t* sp_off, uint64_t entries, uint32_t n_rows, hipStream_t s,
                                 SparseInvertedArrays* out)
{
    SparseInvertedArrays im{};
    auto free_out = [&]() {
        void* ptrs[] = {im.post, im.bterm, im.boff, im.bbeg, im.a};
        for (void* q : ptrs)
            if (q) (void) hipFree(q);
    };
    const uint2* ent = reinterpret_cast<const uint2*>(rows);
    const uint32_t nb = (uint32_t) (((uint64_t) n_rows + SI_RB - 1) >> SI_RB_LOG2);
    im.n_blocks = nb;
    im.n_post = entries;
    int end_bit = SI_KEY_BLOCK_SHIFT;
    while (end_bit < 64 && ((uint64_t) nb >> (end_bit - SI_KEY_BLOCK_SHIFT)) != 0) ++end_bit;

    SiMem key[2], val[2], tmp;
    SI_CHK(key[0].alloc((entries + 1) * 8));
    SI_CHK(key[1].alloc((entries + 1) * 8));
    SI_CHK(val[0].alloc(entries * 4));
    SI_CHK(val[1].alloc(entries * 4));
    size_t b1 = 0, b2 = 0;
    {
        hipcub::DoubleBuffer<uint64_t> k(nullptr, nullptr);
        hipcub::DoubleBuffer<uint32_t> v(nullptr, nullptr);
        SI_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k, v, (int) entries, 0, end_bit, s));
        SI_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const uint32_t*) nullptr, (uint32_t*) nullptr, (int) (entries + 1), s));
    }
    const size_t tmp_bytes = std::max(b1, b2);
    SI_CHK(tmp.alloc(tmp_bytes));
    SI_CHK(hipMalloc(reinterpret_cast<void**>(&im.post), std::max<size_t>(entries * 8, 256)));
    SI_CHK(hipMalloc(reinterpret_cast<void**>(&im.bbeg), ((size_t) nb + 1) * 4));
    SI_CHK(hipMalloc(reinterpret_cast<void**>(&im.a), std::max<size_t>((size_t) n_rows * 16, 256)));

    hipcub::DoubleBuffer<uint64_t> k(key[0].as<uint64_t>(), key[1].as<uint64_t>());
    hipcub::DoubleBuffer<uint32_t> v(val[0].as<uint32_t>(), val[1].as<uint32_t>());
    if (entries > 0) {
        hipLaunchKernelGGL(si_key_kernel, si_blocks(entries), dim3(256), 0, s, ent, sp_off, entries, n_rows, nb, k.Current(), v.Current());
        SI_CHK(hipGetLastError());
        size_t tb = tmp_bytes;
        SI_CHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k, v, (int) entries, 0, end_bit, s));
    }
    if (n_rows > 0) {
        hipLaunchKernelGGL(si_row_sums_kernel, si_blocks(n_rows), dim3(256), 0, s, ent, sp_off, n_rows, im.a);
        SI_CHK(hipGetLastError());
    }
    // the idle key buffer holds the flags and their scan: 2 x (entries + 1) words
    uint32_t* flag = reinterpret_cast<uint32_t*>(k.Alternate());
    uint32_t* pos = flag + (entries + 1);
    hipLaunchKernelGGL(si_mark_kernel, si_blocks(entries + 1), dim3(256), 0, s, (const uint64_t*) k.Current(), entries, nb, flag);
    SI_CHK(hipGetLastError());
    size_t tb = tmp_bytes;
    SI_CHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, (const uint32_t*) flag, pos, (int) (entries + 1), s));
    uint32_t n_terms = 0;
    SI_CHK(hipMemcpyAsync(&n_terms, pos + entries, 4, hipMemcpyDeviceToHost, s));
    SI_CHK(hipStreamSynchronize(s));
    im.n_terms = n_terms;
    SI_CHK(hipMalloc(reinterpret_cast<void**>(&im.bterm), std::max<size_t>((size_t) n_terms * 4, 256)));
    SI_CHK(hipMalloc(reinterpret_cast<void**>(&im.boff), std::max<size_t>(((size_t) n_terms + nb) * 8, 256)));
    hipLaunchKernelGGL(si_write_kernel, si_blocks(entries + 1), dim3(256), 0, s, (const uint64_t*) k.Current(), (const uint32_t*) v.Current(),
                       (const uint32_t*) flag, (const uint32_t*) pos, entries, nb, im.post, im.bterm, im.boff, im.bbeg);
    SI_CHK(hipGetLastError());
    SI_CHK(hipStreamSynchronize(s));                                           // the scratch goes away with this frame
    *out = im;
    return hipSuccess;
}

#undef SI_CHK

}  // namespace vsr
