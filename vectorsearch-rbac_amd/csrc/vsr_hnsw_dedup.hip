// vsr_hnsw_dedup.hip — the pre-pass of a merging HNSW build (VSR_HNSW_BUILD_MERGE_DUPLICATES): byte-identical rows become
// one element with up to 10 heap TIDs, as pgvector's HnswFindDuplicateInMemory does for the rows it happens to meet
// (hnswbuild.c:309-355).  Here the grouping is exhaustive:
//
//   1. hnsw_row_hash_kernel     64-bit hash of every unresolved row's bit patterns (one pass, coalesced 16-byte loads)
//   2. hipCUB radix sort        (hash, row) pairs; stable, and the unresolved rows enter in ascending order, so rows ascend
//                               inside a run of equal hashes and the run's first row is its lowest
//   3. hnsw_dup_resolve_kernel  a row joins its run head's group only when all its bytes equal the head's.  Rows that differ
//                               from their run head (a hash collision) stay unresolved and go round again under the next
//                               seed.  Identical rows hash alike under every seed, so they always meet in one run: a
//                               collision neither merges different rows nor splits a group, and a group's head is its lowest
//                               row.  Every round resolves at least the run heads, so the loop ends.
//   4. hnsw_elem_mark_kernel, an exclusive scan, hnsw_elem_table_kernel
//                               rows sorted by (head, row): a row's member index inside its group, an element per 10
//                               members, elements numbered by their first member's row.
//
// With 64 hash bits round 2 essentially never runs; VSR_HNSW_DEDUP_HASH_BITS (development / tests) keeps fewer bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "vsr_hnsw_build.h"

namespace vsr {

__device__ __forceinline__ uint64_t dd_mix64(uint64_t x)                     // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27; x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}

// Both row kernels give a row to 2^lpr_shift lanes (8 .. 64: several rows per wave for d <= 32 .. 128, a wave per row
// beyond), lane `sub` of a row reading its 16-byte chunks sub, sub + lanes, ...: consecutive lanes, consecutive chunks.
__global__ __launch_bounds__(256) void hnsw_row_hash_kernel(const float4* __restrict__ rows, uint32_t stride4, const int32_t* __restrict__ list,
                                                            uint32_t count, uint32_t lpr_shift, uint64_t seed, uint64_t mask,
                                                            uint64_t* __restrict__ keys)
{
    const uint64_t gt = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    const uint32_t lpr = 1u << lpr_shift, sub = (uint32_t) gt & (lpr - 1u);
    const uint64_t i = gt >> lpr_shift;
    const bool live = i < count;
    uint64_t h = 0;
    if (live) {
        const uint4* r = reinterpret_cast<const uint4*>(rows + (size_t) list[i] * stride4);
        for (uint32_t ch = sub; ch < stride4; ch += lpr) {
            const uint4 v = r[ch];
            const uint64_t a = (uint64_t) v.x | ((uint64_t) v.y << 32), b = (uint64_t) v.z | ((uint64_t) v.w << 32);
            h += dd_mix64(dd_mix64(a + seed + (uint64_t) ch * 0x9E3779B97F4A7C15ULL) ^ b);      // keyed by the chunk's place
        }
    }
    for (uint32_t mm = lpr >> 1; mm >= 1; mm >>= 1) h += (uint64_t) __shfl_xor((unsigned long long) h, (int) mm);
    if (live && sub == 0) keys[i] = dd_mix64(h ^ seed) & mask;
}

// first index in [0, i] whose key equals keys[i] (keys ascending)
template <class K>
__device__ __forceinline__ uint32_t dd_run_start(const K* keys, uint32_t i)
{
    const K key = keys[i];
    uint32_t lo = 0, hi = i;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void hnsw_dup_resolve_kernel(const float4* __restrict__ rows, uint32_t stride4, const uint64_t* __restrict__ keys,
                                                               const int32_t* __restrict__ list, uint32_t count, uint32_t lpr_shift,
                                                               int32_t* __restrict__ head, uint8_t* __restrict__ unresolved)
{
    const uint64_t gt = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    const uint32_t lpr = 1u << lpr_shift, sub = (uint32_t) gt & (lpr - 1u);
    const uint64_t i = gt >> lpr_shift;
    const bool live = i < count;
    bool diff = false;
    int32_t r = 0, hr = 0;
    if (live) {
        r = list[i];
        hr = list[dd_run_start(keys, (uint32_t) i)];
        if (r != hr) {
            const uint4* a = reinterpret_cast<const uint4*>(rows + (size_t) r * stride4);
            const uint4* b = reinterpret_cast<const uint4*>(rows + (size_t) hr * stride4);
            for (uint32_t ch = sub; ch < stride4; ch += lpr) {
                const uint4 x = a[ch], y = b[ch];
                diff |= ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0u;
            }
        }
    }
    const uint64_t bal = __ballot(diff);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mine = lpr == 64u ? ~0ull : (((1ull << lpr) - 1ull) << (lane & ~(lpr - 1u)));
    if (live && sub == 0 && (bal & mine) == 0ull) {
        head[r] = hr;
        unresolved[r] = 0;
    }
}

__global__ __launch_bounds__(256) void hnsw_iota_kernel(int32_t* out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t) i;
}

// rows sorted by (head, row): member index of each inside its group; a row that opens a chunk of 10 opens an element
__global__ __launch_bounds__(256) void hnsw_elem_mark_kernel(const uint32_t* __restrict__ head_s, const int32_t* __restrict__ row_s, uint32_t n,
                                                             int32_t* __restrict__ member, int32_t* __restrict__ is_head)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t mem = i - dd_run_start(head_s, i);
    member[i] = (int32_t) mem;
    is_head[row_s[i]] = mem % HB_TIDS == 0 ? 1 : 0;
}

// eidx = exclusive scan of is_head over rows: the element a chunk's first row opens
__global__ __launch_bounds__(256) void hnsw_elem_table_kernel(const uint32_t* __restrict__ head_s, const int32_t* __restrict__ row_s,
                                                              const int32_t* __restrict__ member, const int32_t* __restrict__ eidx,
                                                              const int32_t* __restrict__ row_level, uint32_t n, int32_t* __restrict__ elem_row,
                                                              int32_t* __restrict__ tid_count, int32_t* __restrict__ tids,
                                                              int32_t* __restrict__ level)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = (uint32_t) member[i] % HB_TIDS;
    const int32_t e = eidx[row_s[i - slot]], r = row_s[i];
    tids[(size_t) e * HB_TIDS + slot] = r;
    if (slot != 0) return;
    elem_row[e] = r;
    level[e] = row_level[r];
    int32_t cnt = 1;
    while (cnt < HB_TIDS && i + (uint32_t) cnt < n && head_s[i + (uint32_t) cnt] == head_s[i]) ++cnt;
    tid_count[e] = cnt;
}

}  // namespace vsr

using namespace vsr;

namespace {
struct DevMem {                                                              // the pre-pass's scratch, freed on every way out
    void* p = nullptr;
    ~DevMem() { if (p) (void) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct Events {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    ~Events() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};
}  // namespace

#define DD_CHK(call)                          \
    do {                                      \
        hipError_t e_ = (call);               \
        if (e_ != hipSuccess) return e_;      \
    } while (0)

hipError_t vsr_hnsw_dedup_elements(const float4* rows, uint32_t n, uint32_t stride4, int hash_bits, const int32_t* d_row_level,
                                   HnswElemTable* out, HnswDedupTimes* times, hipStream_t s)
{
    *out = HnswElemTable{};
    if (n == 0) return hipSuccess;
    uint32_t lpr_shift = 3;                                                   // 8 lanes cover d <= 32
    while (lpr_shift < 6 && (1u << lpr_shift) < stride4) ++lpr_shift;
    const uint64_t mask = hash_bits >= 64 ? ~0ull : ((1ull << hash_bits) - 1ull);
    int id_bits = 1;
    while (id_bits < 32 && (1ull << id_bits) < (uint64_t) n) ++id_bits;

    DevMem key[2], list[2], head, unres, cnt, tmp, member, is_head, eidx;
    for (int b = 0; b < 2; ++b) {
        DD_CHK(key[b].alloc((size_t) n * 8));
        DD_CHK(list[b].alloc((size_t) n * 4));
    }
    DD_CHK(head.alloc((size_t) n * 4));
    DD_CHK(unres.alloc(n));
    DD_CHK(cnt.alloc(64));
    DD_CHK(member.alloc((size_t) n * 4));
    DD_CHK(is_head.alloc((size_t) n * 4));
    DD_CHK(eidx.alloc((size_t) n * 4));
    size_t tmp_bytes = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    {
        hipcub::DoubleBuffer<uint64_t> k64(nullptr, nullptr);
        hipcub::DoubleBuffer<uint32_t> k32(nullptr, nullptr);
        hipcub::DoubleBuffer<int32_t> v(nullptr, nullptr);
        DD_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k64, v, (int) n, 0, hash_bits, s));
        DD_CHK(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, k32, v, (int) n, 0, id_bits, s));
        DD_CHK(hipcub::DeviceSelect::Flagged(nullptr, b3, hipcub::CountingInputIterator<int32_t>(0), (const uint8_t*) nullptr, (int32_t*) nullptr,
                                             (uint32_t*) nullptr, (int) n, s));
        DD_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, b4, (const int32_t*) nullptr, (int32_t*) nullptr, (int) n, s));
        tmp_bytes = std::max({b1, b2, b3, b4});
    }
    DD_CHK(tmp.alloc(tmp_bytes));
    Events ev;
    if (times) {
        *times = HnswDedupTimes{};
        for (hipEvent_t& e : ev.ev) DD_CHK(hipEventCreate(&e));
        ev.on = true;
    }
    auto mark = [&](int i) -> hipError_t { return ev.on ? hipEventRecord(ev.ev[i], s) : hipSuccess; };
    auto blocks_of = [&](uint64_t items) { return dim3((unsigned) ((items + 255) / 256)); };

    // ---- groups: head[r] = the lowest row with r's bytes ----
    DD_CHK(hipMemsetAsync(unres.p, 1, n, s));
    for (uint32_t round = 0;; ++round) {
        // the unresolved rows, ascending
        DD_CHK(mark(0));
        size_t tb = tmp_bytes;
        DD_CHK(hipcub::DeviceSelect::Flagged(tmp.p, tb, hipcub::CountingInputIterator<int32_t>(0), unres.as<const uint8_t>(), list[0].as<int32_t>(),
                                             cnt.as<uint32_t>(), (int) n, s));
        uint32_t left = 0;
        DD_CHK(hipMemcpyAsync(&left, cnt.p, 4, hipMemcpyDeviceToHost, s));
        DD_CHK(hipStreamSynchronize(s));
        if (ev.on && round > 0) {
            float ms[3] = {0, 0, 0};
            for (int j = 0; j < 3; ++j) DD_CHK(hipEventElapsedTime(&ms[j], ev.ev[j + 1], j == 2 ? ev.ev[0] : ev.ev[j + 2]));
            times->hash_ms += ms[0];
            times->sort_ms += ms[1];
            times->resolve_ms += ms[2];
        }
        if (left == 0) break;
        if (times) times->rounds = (int) round + 1;
        const uint64_t seed = 0x9E3779B97F4A7C15ULL * (round + 1);
        DD_CHK(mark(1));
        hipLaunchKernelGGL(hnsw_row_hash_kernel, blocks_of((uint64_t) left << lpr_shift), dim3(256), 0, s, rows, stride4, list[0].as<const int32_t>(),
                           left, lpr_shift, seed, mask, key[0].as<uint64_t>());
        DD_CHK(hipGetLastError());
        DD_CHK(mark(2));
        hipcub::DoubleBuffer<uint64_t> k(key[0].as<uint64_t>(), key[1].as<uint64_t>());
        hipcub::DoubleBuffer<int32_t> v(list[0].as<int32_t>(), list[1].as<int32_t>());
        tb = tmp_bytes;
        DD_CHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k, v, (int) left, 0, hash_bits, s));
        DD_CHK(mark(3));
        hipLaunchKernelGGL(hnsw_dup_resolve_kernel, blocks_of((uint64_t) left << lpr_shift), dim3(256), 0, s, rows, stride4,
                           (const uint64_t*) k.Current(), (const int32_t*) v.Current(), left, lpr_shift, head.as<int32_t>(), unres.as<uint8_t>());
        DD_CHK(hipGetLastError());
    }

    // ---- elements: rows by (head, row), 10 members each ----
    DD_CHK(mark(1));
    hipLaunchKernelGGL(hnsw_iota_kernel, blocks_of(n), dim3(256), 0, s, list[0].as<int32_t>(), n);
    DD_CHK(hipGetLastError());
    DD_CHK(hipMemcpyAsync(key[0].p, head.p, (size_t) n * 4, hipMemcpyDeviceToDevice, s));
    hipcub::DoubleBuffer<uint32_t> k(key[0].as<uint32_t>(), key[1].as<uint32_t>());
    hipcub::DoubleBuffer<int32_t> v(list[0].as<int32_t>(), list[1].as<int32_t>());
    size_t tb = tmp_bytes;
    DD_CHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k, v, (int) n, 0, id_bits, s));
    const uint32_t* head_s = k.Current();
    const int32_t* row_s = v.Current();
    hipLaunchKernelGGL(hnsw_elem_mark_kernel, blocks_of(n), dim3(256), 0, s, head_s, row_s, n, member.as<int32_t>(), is_head.as<int32_t>());
    DD_CHK(hipGetLastError());
    tb = tmp_bytes;
    DD_CHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, is_head.as<const int32_t>(), eidx.as<int32_t>(), (int) n, s));
    int32_t last[2] = {0, 0};
    DD_CHK(hipMemcpyAsync(&last[0], eidx.as<int32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s));
    DD_CHK(hipMemcpyAsync(&last[1], is_head.as<int32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s));
    DD_CHK(hipStreamSynchronize(s));
    const int32_t n_elem = last[0] + last[1];
    HnswElemTable t{};
    t.n_elem = n_elem;
    hipError_t e = hipMalloc(&t.elem_row, (size_t) n_elem * 4);
    if (e == hipSuccess) e = hipMalloc(&t.tid_count, (size_t) n_elem * 4);
    if (e == hipSuccess) e = hipMalloc(&t.tids, (size_t) n_elem * HB_TIDS * 4);
    if (e == hipSuccess) e = hipMalloc(&t.level, (size_t) n_elem * 4);
    if (e == hipSuccess) e = hipMemsetAsync(t.tids, 0xFF, (size_t) n_elem * HB_TIDS * 4, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hnsw_elem_table_kernel, blocks_of(n), dim3(256), 0, s, head_s, row_s, member.as<const int32_t>(), eidx.as<const int32_t>(),
                           d_row_level, n, t.elem_row, t.tid_count, t.tids, t.level);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mark(2);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                         // the scratch goes away with this frame
    if (e == hipSuccess && ev.on) e = hipEventElapsedTime(&times->table_ms, ev.ev[1], ev.ev[2]);
    if (e != hipSuccess) {
        void* ptrs[] = {t.elem_row, t.tid_count, t.tids, t.level};
        for (void* q : ptrs)
            if (q) (void) hipFree(q);
        return e;
    }
    *out = t;
    return hipSuccess;
}
