// vsr_hnsw_forest_search.h -- searching a FOREST of HNSW graphs over one corpus (vsr_hnsw_forest_search*, vsr_hnsw_rt.hip): the
// graphs of a query's partitions in one search launch, their results merged on the GPU in one merge launch.
//
// A TASK is a (query, graph) pair: query i owns tasks q_off[i] .. q_off[i + 1] of q_graph.  The search launch is K4's own body
// (hnsw_search_body<false, ROWS, true>, vsr_hnsw.h) with one wave per task: the walk, the admission rule, the order of the TIDs and
// the first k are those of vsr_hnsw_search on that graph, so a task's list holds exactly the rows that call returns, as keys
// make_key(rank value, internal row).  The merge launch gives a query the first k distinct keys of its tasks' lists in key order:
// internal rows are in (document_id, block_id) order, so that is the project's tie rule, and a row several partitions hold carries
// the same fp32 sum in each (the same body sums it in the same lane mapping), so its repeats are equal keys and sort side by side.
//
// The first part of this file is plain C++ with no HIP call -- the checks of the task table and the merge's pass plan --
// and tests/test_hnsw_forest_search_cpu.py compiles it alone with the host compiler; the kernels follow under __HIPCC__.
//
// The merge of one query (one wave): a running list of at most k sorted, repeat-free keys at the front of C key slots of LDS.  A pass
// appends as many whole task lists (k slots each, KEY_EMPTY past a list's count) as fit behind the running list, sorts the lot with
// the bitonic network of the iterative scan's take(), drops equal neighbours and empty slots by ballot compaction and keeps k.  The
// first k of a union are the first k of (the first k of one part, united with the rest), so the number of passes -- the capacity C --
// does not change the result.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#if defined(__HIPCC__)
#define VSR_FOREST_HD __host__ __device__
#else
#define VSR_FOREST_HD
#endif

namespace vsr {

constexpr uint32_t HFS_MERGE_KEYS_MAX = 16384;       // key slots of the merge's LDS at most: 128 KB of the CU's 160
constexpr uint32_t HFS_MERGE_KEYS_DEFAULT = 2048;    // 16 KB per merge wave ("Forest search")

// the smallest legal capacity for k: the smallest power of two >= 2 k (the running list and one task list)
inline uint32_t hnsw_merge_keys_min(uint32_t k)
{
    uint32_t c = 2;
    while (c < 2 * k) c <<= 1;
    return c;
}

// VSR_HNSW_FOREST_MERGE_KEYS: a power of two from hnsw_merge_keys_min(k) to HFS_MERGE_KEYS_MAX
inline bool hnsw_merge_keys_ok(uint32_t k, uint64_t c)
{
    return c >= hnsw_merge_keys_min(k) && c <= HFS_MERGE_KEYS_MAX && (c & (c - 1)) == 0;
}

// the capacity of a call that sets none: the default, raised to the smallest legal one for a large k
inline uint32_t hnsw_merge_keys_default(uint32_t k)
{
    const uint32_t lo = hnsw_merge_keys_min(k);
    return lo > HFS_MERGE_KEYS_DEFAULT ? lo : HFS_MERGE_KEYS_DEFAULT;
}

// whole lists of k slots a pass takes: all of C in the first pass, C less the running list's k slots afterwards (>= 1: C >= 2 k)
VSR_FOREST_HD inline uint32_t hnsw_merge_pass_lists(uint32_t k, uint32_t c, bool first) { return first ? c / k : (c - k) / k; }

struct HnswMergePass {
    uint32_t first_list = 0, n_lists = 0;
    uint32_t keys = 0;                       // slots the pass sorts: the running list's k (not in the first pass) + k per list
};

// which of a query's n_lists task lists go into which pass (what hnsw_forest_merge_kernel walks)
inline std::vector<HnswMergePass> hnsw_merge_pass_plan(uint32_t k, uint32_t c, uint32_t n_lists)
{
    std::vector<HnswMergePass> plan;
    for (uint32_t t = 0; t < n_lists;) {
        const bool first = plan.empty();
        uint32_t n = hnsw_merge_pass_lists(k, c, first);
        if (n > n_lists - t) n = n_lists - t;
        plan.push_back({t, n, (first ? 0u : k) + n * k});
        t += n;
    }
    return plan;
}

// The task table of a call: q_off[nq + 1] non-decreasing from 0, every graph id of q_graph[q_off[nq]] within [0, n_indexes), at most
// 2^31 - 1 tasks.  Returns true, or false with the reason in msg.
inline bool hnsw_forest_check_tasks(int nq, const int64_t* q_off, const int32_t* q_graph, int n_indexes, char* msg, size_t msg_len)
{
    if (nq < 0) return snprintf(msg, msg_len, "nq is %d", nq), false;
    if (!q_off) return snprintf(msg, msg_len, "q_off is NULL"), false;
    if (q_off[0] != 0) return snprintf(msg, msg_len, "q_off[0] is %lld, not 0", (long long) q_off[0]), false;
    for (int i = 0; i < nq; ++i)
        if (q_off[i + 1] < q_off[i]) return snprintf(msg, msg_len, "q_off decreases at query %d", i), false;
    const int64_t n_tasks = q_off[nq];
    if (n_tasks > 0x7FFFFFFFll) return snprintf(msg, msg_len, "%lld tasks are more than 2^31 - 1", (long long) n_tasks), false;
    if (n_tasks > 0 && !q_graph) return snprintf(msg, msg_len, "q_graph is NULL"), false;
    for (int64_t t = 0; t < n_tasks; ++t)
        if (q_graph[t] < 0 || q_graph[t] >= n_indexes)
            return snprintf(msg, msg_len, "task %lld names graph %d of a forest of %d", (long long) t, (int) q_graph[t], n_indexes), false;
    return true;
}

}  // namespace vsr

#if defined(__HIPCC__)
#include "vsr_hnsw.h"

namespace vsr {

// K4 / K4h / K4b over a forest: one wave per task, up to four tasks per workgroup (HnswParams::nq counts tasks)
__global__ __launch_bounds__(256) void hnsw_forest_search_kernel(const HnswParams p, const HnswForestTasks ft)
{
    hnsw_search_body<false, ROWS_F32, true>(p, ft);
}
__global__ __launch_bounds__(256) void hnsw_half_forest_search_kernel(const HnswParams p, const HnswForestTasks ft)
{
    hnsw_search_body<false, ROWS_HALF, true>(p, ft);
}
__global__ __launch_bounds__(256) void hnsw_bit_forest_search_kernel(const HnswParams p, const HnswForestTasks ft)
{
    hnsw_search_body<false, ROWS_BIT, true>(p, ft);
}

inline hipError_t launch_hnsw_forest(RowFormat f, const HnswParams& p, const HnswForestTasks& ft, hipStream_t s)
{
    if (p.nq == 0) return hipSuccess;
    const size_t lds = (size_t) p.lds_per_query * p.qpb;
    if (lds > HN_LDS_BUDGET || p.qpb < 1 || p.qpb > 4 || !p.out_keys || !p.out_count || !p.out_status) return hipErrorInvalidValue;
    const auto kernel = f == RowFormat::BIT ? hnsw_bit_forest_search_kernel : f == RowFormat::HALF ? hnsw_half_forest_search_kernel
                        : f == RowFormat::F32 ? hnsw_forest_search_kernel : nullptr;
    if (!kernel) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((p.nq + p.qpb - 1) / p.qpb), dim3(64 * p.qpb), lds, s, p, ft);
    return hipGetLastError();
}

struct HnswForestMergeParams {
    const int64_t*  q_off = nullptr;         // [nq + 1] (device)
    const uint64_t* task_keys = nullptr;     // [tasks][k]
    const int32_t*  task_status = nullptr;   // [tasks] 1: the task has no result, and so has its query (count -1)
    uint32_t        nq = 0, k = 0, cap = 0;  // cap: C, the key slots of the wave's LDS
    int             rows = ROWS_F32;         // HnswRows of the forest and the metric of the call: what a distance is reported as
    int             metric = 0;
    const int64_t*  block_ids = nullptr; const int32_t* doc_ids = nullptr; const int64_t* orig_rows = nullptr;
    int64_t* out_block = nullptr; int32_t* out_doc = nullptr; int64_t* out_row = nullptr; float* out_dist = nullptr; int32_t* out_count = nullptr;
};

// one wave (one workgroup) per query; dynamic LDS: cap keys
__global__ __launch_bounds__(64) void hnsw_forest_merge_kernel(const HnswForestMergeParams p)
{
    extern __shared__ __align__(16) unsigned char smem_all[];
    uint64_t* L = reinterpret_cast<uint64_t*>(smem_all);
    const uint32_t lane = threadIdx.x;
    const uint32_t qi = blockIdx.x;
    if (qi >= p.nq) return;
    const uint32_t t0 = (uint32_t) p.q_off[qi], t1 = (uint32_t) p.q_off[qi + 1];
    bool bad = false;
    for (uint32_t t = t0 + lane; t < t1; t += 64) bad |= p.task_status[t] != 0;
    const bool failed = __ballot(bad) != 0ull;
    const uint64_t below_me = (1ull << lane) - 1ull;
    uint32_t run = 0;                                                        // the running list: L[0, run), sorted, repeat-free
    for (uint32_t t = t0; t < t1 && !failed;) {
        uint32_t n = hnsw_merge_pass_lists(p.k, p.cap, t == t0);
        if (n > t1 - t) n = t1 - t;
        const uint32_t add = n * p.k;                                        // (<= cap - run: run <= k, and run = 0 in the first pass)
        const uint64_t* src = p.task_keys + (size_t) t * p.k;               // a query's lists are contiguous
        for (uint32_t i = lane; i < add; i += 64) L[run + i] = src[i];
        const uint32_t count = run + add;
        wave_sync();
        // bitonic sort of L[0, count): positions >= count act as +inf and are never touched (take(), vsr_hnsw.h)
        uint32_t n2 = 1, lg = 0;
        while (n2 < count) { n2 <<= 1; ++lg; }
        for (uint32_t ls = 1; ls <= lg; ++ls) {
            const uint32_t size = 1u << ls, half = size >> 1;
            for (uint32_t tt = lane; tt < n2 / 2; tt += 64) {                // flip: i against its mirror in the block
                const uint32_t i = ((tt >> (ls - 1)) << ls) + (tt & (half - 1)), j = i ^ (size - 1);
                if (j < count) {
                    const uint64_t a = L[i], b = L[j];
                    if (a > b) { L[i] = b; L[j] = a; }
                }
            }
            wave_sync();
            for (uint32_t ld = ls - 1; ld >= 1; --ld) {
                const uint32_t stride = 1u << (ld - 1);
                for (uint32_t tt = lane; tt < n2 / 2; tt += 64) {
                    const uint32_t i = ((tt >> (ld - 1)) << ld) + (tt & (stride - 1)), j = i + stride;
                    if (j < count) {
                        const uint64_t a = L[i], b = L[j];
                        if (a > b) { L[i] = b; L[j] = a; }
                    }
                }
                wave_sync();
            }
        }
        // keep a key that is real and differs from the one before it; the kept keys move to the front in order.  A write lands at or
        // before the position it was read from, and position base - 1 is written before chunk `base` reads it only while nothing has
        // been dropped, with the value it held
        uint32_t kept = 0;
        for (uint32_t base = 0; base < count && kept < p.k; base += 64) {
            const uint32_t i = base + lane;
            const uint64_t key = i < count ? L[i] : KEY_EMPTY;
            const uint64_t before = i > 0 && i < count ? L[i - 1] : KEY_EMPTY;
            const bool keep = key != KEY_EMPTY && (i == 0 || key != before);
            const uint64_t km = __ballot(keep);
            wave_sync();
            const uint32_t at = kept + (uint32_t) __popcll(km & below_me);
            if (keep && at < p.k) L[at] = key;
            kept += (uint32_t) __popcll(km);
            wave_sync();
        }
        run = kept < p.k ? kept : p.k;
        t += n;
    }
    for (uint32_t i = lane; i < p.k; i += 64) {
        const size_t o = (size_t) qi * p.k + i;
        if (i < run) {
            const uint64_t key = L[i];
            const uint32_t row = (uint32_t) key;
            p.out_block[o] = p.block_ids[row];
            if (p.out_doc) p.out_doc[o] = p.doc_ids[row];
            if (p.out_row) p.out_row[o] = p.orig_rows[row];
            p.out_dist[o] = hnsw_reported_distance(p.rows, p.metric, mono_to_float((uint32_t) (key >> 32)));
        } else {
            p.out_block[o] = -1;
            if (p.out_doc) p.out_doc[o] = -1;
            if (p.out_row) p.out_row[o] = -1;
            p.out_dist[o] = __builtin_inff();
        }
    }
    if (lane == 0) p.out_count[qi] = failed ? -1 : (int32_t) run;
}

inline hipError_t launch_hnsw_forest_merge(const HnswForestMergeParams& p, hipStream_t s)
{
    if (p.nq == 0) return hipSuccess;
    if (!hnsw_merge_keys_ok(p.k, p.cap)) return hipErrorInvalidValue;
    const size_t lds = (size_t) p.cap * sizeof(uint64_t);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_forest_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hnsw_forest_merge_kernel, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

}  // namespace vsr
#endif
