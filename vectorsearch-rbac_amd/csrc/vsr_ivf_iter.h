// vsr_ivf_iter.h — K3i: pgvector's IVFFlat iterative index scan (ivfflat.iterative_scan = relaxed_order with
// ivfflat.max_probes; ivfscan.c:112-176 GetScanItems, :249-272 the maxProbes set-up, :375-381 the refill loop), the part
// past the first batch, for all queries of a call in ONE launch.  Compiled by vsr_ivf.hip.
//
// Batch 0 (the `probes` nearest lists) is vsr_ivf_search itself and has already written the outputs.  This kernel takes one
// 256-thread workgroup per query and
//   * leaves at once when batch 0 found k rows or there is no list past it (out_probes = P);
//   * orders the centres exactly as ivf_probe_kernel does (ivf_center_key / ivf_extract_nearest, vsr_exact.h), the 32-bit
//     monotone keys in LDS; the first P extractions are batch 0's lists and are only marked taken; later lists are extracted
//     one at a time as their batch is scanned, so a query that stops after two batches never orders the rest;
//   * scans a list as a contiguous range of the list-ordered view, 64 rows per wave step: one permission word of the query's
//     view-order bitmap per step (steps are aligned to the words; rows of the step outside the list are masked), the
//     permitted rows compacted by a ballot, and only those rows read: half a wave per row, 4 rows per half-wave in flight,
//     the operator arithmetic of the exact re-rank (halfwave_row_sums, vsr_exact.h);
//   * keeps the (k - have) smallest keys of the batch -- key = make_key(value, base row), so equal values order by
//     (document_id, block_id) -- sorted in LDS, and appends them at position `have` of the query's outputs;
//   * goes on, batch after batch, while fewer than k rows are out and lists remain (an empty batch does not stop it).
//
// Selection: `kept` = SK sorted keys (SK = max(512, 2^ceil(log2 need)) <= 2048: 16 KiB), `chunk` = 512 appended keys.  Waves
// append keys below the running threshold; a workgroup step appends at most 256, and before a step could overflow the chunk
// it is sorted and folded into `kept` (kept[SK-1-j] = min(kept[SK-1-j], chunk[j]): the SK smallest of both, then sorted
// again) and the threshold becomes kept[need - 1].
//
// LDS (all dynamic, every carve a multiple of 16): lists * 4 centre keys (<= 128 KiB) + padded query (stride4 * 16) +
// 4 x 64 row slots + kept (<= 16 KiB) + chunk (4 KiB) + 64 bytes of control words: <= 160 KiB for rows of up to ~2700 floats
// at the reloption's 32768 lists (ivfflat indexes at most 2000 dimensions); the launcher refuses what does not fit.
//
// Bounds: a list id outside [0, lists), a list range outside the view's rows, or a base row outside the corpus ends that
// query's scan with what it has; none of them becomes an address.
#pragma once
#include "vsr_device.h"
#include "vsr_exact.h"
#include "vsr_bitops.h"
#include "vsr_topk.h"
#include "vsr_ivf_lds.h"     // IVI_CHUNK, ivf_iter_kept, ivf_iter_lds_bytes

namespace vsr {

struct IvfIterParams {
    const float*           queries;          // [nq][q_stride] (device); rows_bit: packed bit strings, q_stride BYTES apart
    uint32_t               q_stride;
    uint32_t               dim;
    const void*            centers_t;        // [dim][lists]: fp32, or binary16 when rows_half (K3h); rows_bit: packed, [words][lists]
    uint32_t               lists;
    int                    center_metric;    // M_L2, or M_IP for the inner-product and cosine opclasses
    int                    metric;           // the operator the rows rank by
    uint32_t               probes;           // P = min(probes, lists)
    uint32_t               max_lists;        // M = min(max(max_probes, probes), lists)
    uint32_t               k;
    const uint32_t*        list_start;       // [lists + 1] offsets into the view
    const float4*          rows;             // the view's rows, [n_rows][stride4], zero padded
    uint32_t               rows_half;        // 1: the view of a halfvec corpus, [n_rows][stride4 / 2] chunks of 8 binary16 values
    uint32_t               rows_bit;         // 1: the view of a bit corpus (K3b), [n_rows][stride4] chunks of packed bits, pad bits clear
    uint32_t               stride4;
    uint32_t               n_rows;
    const uint32_t*        rank;             // view row -> base row (what keys carry)
    const uint64_t* const* bitmaps;          // [nq] the query's permission bits in view order; nullptr entry: every row
    const int64_t*         block_ids;        // identity arrays of the base corpus
    const int32_t*         doc_ids;
    const int64_t*         orig_rows;
    int64_t*               out_block;        // [nq][k], already holding batch 0
    int32_t*               out_doc;          // may be nullptr
    int64_t*               out_row;          // may be nullptr
    float*                 out_dist;
    int32_t*               out_count;        // [nq] in: batch 0's count; out: the scan's
    int32_t*               out_probes;       // [nq] lists scanned, whole batches; may be nullptr
};

#ifdef __HIPCC__
struct IvfIterCtrl {                         // 64 bytes
    uint64_t tau;                            // keys >= tau cannot enter the batch's result
    uint64_t s_best[4];
    uint32_t count;                          // keys in the chunk
    uint32_t bad;                            // an index out of bounds was met: the scan ends
    uint32_t pad[4];
};

// sort the chunk, fold it into kept (the SK smallest of both survive), sort kept, lower tau.  All 256 threads; the
// caller's barrier orders every append before it.  Ends with a barrier.
__device__ __forceinline__ void ivf_iter_fold(uint64_t* kept, uint32_t sk, uint64_t* chunk, IvfIterCtrl* ctrl, uint32_t need, int tid)
{
    const uint32_t n = ctrl->count < IVI_CHUNK ? ctrl->count : IVI_CHUNK;
    __syncthreads();                                                       // every thread has read count
    if (n == 0) return;
    for (uint32_t i = n + tid; i < IVI_CHUNK; i += 256) chunk[i] = KEY_EMPTY;
    __syncthreads();
    bitonic_sort_lds<256>(chunk, IVI_CHUNK, tid);
    for (uint32_t j = tid; j < IVI_CHUNK; j += 256) {
        const uint64_t a = kept[sk - 1 - j], b = chunk[j];
        kept[sk - 1 - j] = b < a ? b : a;
    }
    __syncthreads();
    bitonic_sort_lds<256>(kept, sk, tid);
    if (tid == 0) {
        ctrl->count = 0;
        ctrl->tau = kept[need - 1];                                        // KEY_EMPTY until `need` keys exist
    }
    __syncthreads();
}

// The permitted rows of one workgroup step -- the 256 view rows from `base` (a multiple of 64), one word of the bitmap per
// wave -- of the list [s0, s1): this wave's word into m, the workgroup's count returned (the same in every thread).  Shared
// with K3q (vsr_ivf_shortlist.h).
__device__ __forceinline__ uint32_t ivf_iter_step_masks(uint32_t base, uint32_t s0, uint32_t s1, const uint64_t* bm, int wave, uint64_t& m)
{
    uint32_t step_n = 0;
    m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t w0 = base + (uint32_t) w * 64;
        uint64_t mw = 0;
        if (w0 < s1) {
            const uint32_t lo = s0 > w0 ? s0 - w0 : 0u;        // < 64: w0 >= s0 & ~63
            const uint32_t hi = s1 - w0 < 64u ? s1 - w0 : 64u;
            mw = (hi == 64u ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
            if (bm) mw &= bm[w0 >> 6];                         // w0 < s1 <= n_rows: inside the bitmap
        }
        step_n += (uint32_t) __popcll(mw);
        if (w == wave) m = mw;
    }
    return step_n;
}

// A wave's step over a bit view: the n_ok (>= 1, wave-uniform) compacted view rows of rowsel are gathered by lane groups and
// counted against the packed query in LDS (bit_graph_distances, vsr_bitops.h), 64 counts into `counts`; lane j makes the key of
// row j -- make_key((float) count, base row), the value the count as fp32, as K1b's -- and keys below tau are appended to the
// chunk.  A base row outside the corpus sets ctrl->bad and becomes neither a key nor an address.  Shared by K3i's bit form and K3q.
__device__ __forceinline__ void ivf_iter_bit_rows(const uint4* rows16, uint32_t stride4, const uint4* qs, uint32_t* rowsel, uint32_t n_ok,
                                                  float* counts, const uint32_t* rank, uint32_t n_rows, uint64_t tau,
                                                  IvfIterCtrl* ctrl, uint64_t* chunk, int lane)
{
    const uint32_t G = bit_graph_lanes(stride4), gl = (uint32_t) lane & (G - 1u);
    const uint4 qreg = gl < stride4 ? qs[gl] : make_uint4(0u, 0u, 0u, 0u);
    // rowsel[j] < s1 <= n_rows < 2^31 (launcher): a row id of the view as the gather takes it
    bit_graph_distances<false>(rows16, stride4, G, nullptr, nullptr, qs, qreg, 0.0f, reinterpret_cast<const int32_t*>(rowsel), (int) n_ok,
                               counts, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const bool mine = (uint32_t) lane < n_ok;
    const uint32_t br = mine ? rank[rowsel[lane]] : 0u;
    const bool in_range = br < n_rows;
    if (mine && !in_range) ctrl->bad = 1;              // never a key, never an address
    const uint64_t key = make_key(mine ? counts[lane] : 0.0f, br);
    const bool pass = mine && in_range && key < tau;
    const uint64_t pm = __ballot(pass);
    if (pm) {
        const int leader = __ffsll((unsigned long long) pm) - 1;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(&ctrl->count, (uint32_t) __popcll(pm));
        at = (uint32_t) __shfl((int) at, leader) + (uint32_t) __popcll(pm & ((1ull << lane) - 1ull));
        if (pass && at < IVI_CHUNK) chunk[at] = key;
    }
}

// HALF (K3h): rows and centres are binary16.  The query is rounded to binary16 as it is loaded (`$1::halfvec`) and kept in LDS
// widened, as fp32 -- the LDS formula does not change -- so the row sums (halfwave_row_sums<U, true>), cosine's |q|^2 and the
// centre keys (IVF_HALF_Q32, from the query in global memory, rounded the same way) all see the same values.
//
// IVI_BIT (K3b, bit_hamming_ops): rows, centres and the query are packed bits.  The query goes into LDS byte by byte (device
// queries need no alignment) with the pad bits and the rest of its stride4 chunks cleared; the centre keys are IVF_BIT's Hamming
// counts of that LDS image -- the probe's key of the same pair; a step's permitted rows are gathered by lane groups and counted
// by bit_graph_distances (vsr_bitops.h), 64 counts per wave step into LDS, and lane j makes the key of row j: the value is the
// count as fp32, as K1b's.  Selection, folding, bounds checks and out_probes are the code below, unchanged.
enum { IVI_F32 = 0, IVI_HALF = 1, IVI_BIT = 2 };

template <int FORM>
__global__ __launch_bounds__(256) void ivf_iterative_kernel(const IvfIterParams p)
{
    constexpr bool HALF = FORM == IVI_HALF, BIT = FORM == IVI_BIT;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t qi = blockIdx.x;
    const uint32_t P = p.probes, M = p.max_lists, k = p.k;
    const int32_t c0 = p.out_count[qi];
    if (c0 < 0 || (uint32_t) c0 >= k || M <= P) {                          // (uniform: the whole workgroup leaves)
        if (tid == 0 && p.out_probes) p.out_probes[qi] = (int32_t) P;
        return;
    }
    const uint32_t sk = ivf_iter_kept(k);
    size_t off = ((size_t) p.lists * 4 + 15) & ~(size_t) 15;
    uint32_t* ckeys = reinterpret_cast<uint32_t*>(smem);                  // [lists]; 0xFFFFFFFF = taken
    float4* q4 = reinterpret_cast<float4*>(smem + off);                   // [stride4] the query, zero padded
    off += (size_t) p.stride4 * 16;
    uint32_t* rowsel = reinterpret_cast<uint32_t*>(smem + off) + wave * 64;   // this wave's compacted rows of a step
    off += 4 * 64 * 4;
    float* counts = reinterpret_cast<float*>(smem + off) + wave * 64;        // BIT: this wave's Hamming counts of a step
    if (BIT) off += 4 * 64 * 4;
    uint64_t* kept = reinterpret_cast<uint64_t*>(smem + off);             // [sk]
    off += (size_t) sk * 8;
    uint64_t* chunk = reinterpret_cast<uint64_t*>(smem + off);            // [IVI_CHUNK]
    off += (size_t) IVI_CHUNK * 8;
    IvfIterCtrl* ctrl = reinterpret_cast<IvfIterCtrl*>(smem + off);

    if constexpr (BIT) {
        const uint8_t* qb = reinterpret_cast<const uint8_t*>(p.queries) + (size_t) qi * p.q_stride;
        uint8_t* ql = reinterpret_cast<uint8_t*>(q4);
        const uint32_t src_bytes = (p.dim + 7u) / 8u;
        for (uint32_t j = tid; j < p.stride4 * 16; j += 256) {
            uint32_t v = 0;
            if (j < src_bytes) {
                const uint32_t live = p.dim - j * 8u;                        // >= 1: the valid bits of byte j from its top
                v = (uint32_t) qb[j] & (live >= 8u ? 0xFFu : (0xFF00u >> live) & 0xFFu);
            }
            ql[j] = (uint8_t) v;
        }
        __syncthreads();                                                   // the centre keys read the whole query
        for (int c = tid; c < (int) p.lists; c += 256)
            ckeys[c] = ivf_center_key<IVF_BIT>(p.centers_t, (int) p.lists, (int) ((p.dim + 31u) / 32u), c, q4, p.center_metric);
    } else {
        const float* qg = p.queries + (size_t) qi * p.q_stride;
        float* qf = reinterpret_cast<float*>(q4);
        for (uint32_t j = tid; j < p.stride4 * 4; j += 256) qf[j] = j < p.dim ? (HALF ? (float) (_Float16) qg[j] : qg[j]) : 0.0f;
        for (int c = tid; c < (int) p.lists; c += 256)
            ckeys[c] = ivf_center_key<HALF ? IVF_HALF_Q32 : IVF_F32>(p.centers_t, (int) p.lists, (int) p.dim, c, qg, p.center_metric);
    }
    if (tid == 0) ctrl->bad = 0;
    __syncthreads();
    const float qn = p.metric == M_COSINE ? wave_query_norm2(q4, p.stride4, lane) : 0.0f;
    for (uint32_t j = 0; j < P; ++j) (void) ivf_extract_nearest(ckeys, (int) p.lists, ctrl->s_best, tid);   // batch 0's lists

    const uint64_t* bm = p.bitmaps ? p.bitmaps[qi] : nullptr;
    const int half = lane >> 5, hl = lane & 31;
    constexpr int U = 4;                                                   // rows in flight per half-wave
    uint32_t have = (uint32_t) c0, list_index = P;
    bool stop = false;
    while (!stop && have < k && list_index < M) {
        const uint32_t need = k - have;
        const uint32_t batch_end = list_index + P < M ? list_index + P : M;
        for (uint32_t i = tid; i < sk; i += 256) kept[i] = KEY_EMPTY;
        if (tid == 0) {
            ctrl->count = 0;
            ctrl->tau = KEY_EMPTY;
        }
        uint32_t ub = 0;                                                   // upper bound of ctrl->count, the same in every thread
        __syncthreads();
        for (; list_index < batch_end && !stop; ++list_index) {
            const uint64_t b = ivf_extract_nearest(ckeys, (int) p.lists, ctrl->s_best, tid);    // ends with a barrier
            const uint32_t bad = ctrl->bad;
            __syncthreads();                                               // nobody scans (and sets it) before everyone has read it
            const uint32_t l = (uint32_t) b;
            if (bad || b == KEY_EMPTY || l >= p.lists) { stop = true; break; }    // (M <= lists: no list left cannot happen)
            const uint32_t s0 = p.list_start[l], s1 = p.list_start[l + 1];
            if (s0 > s1 || s1 > p.n_rows) { stop = true; break; }
            // workgroup steps of 256 view rows (64 per wave) from the 64-row boundary at or below s0: a wave's step is one
            // word of the bitmap, the rows of the word outside the list masked out
            for (uint32_t base = s0 & ~63u; base < s1; base += 256) {
                uint64_t m;                                                // this wave's permitted rows of the step
                const uint32_t step_n = ivf_iter_step_masks(base, s0, s1, bm, wave, m);   // ... and the workgroup's count of them
                if (ub + step_n > IVI_CHUNK) {                             // (uniform) the chunk could overflow: fold it first
                    __syncthreads();                                       // every append so far is in the chunk
                    ivf_iter_fold(kept, sk, chunk, ctrl, need, tid);
                    ub = 0;
                }
                ub += step_n;
                const bool ok = (m >> lane) & 1ull;                        // ballot-style compaction of the permitted rows
                const uint32_t n_ok = (uint32_t) __popcll(m);
                if (ok) rowsel[__popcll(m & ((1ull << lane) - 1ull))] = base + (uint32_t) wave * 64 + (uint32_t) lane;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint64_t tau = lds_peek(&ctrl->tau);                 // a stale (larger) tau only admits extra keys
                if constexpr (BIT) {
                    if (n_ok)                                              // (wave-uniform)
                        ivf_iter_bit_rows(reinterpret_cast<const uint4*>(p.rows), p.stride4, reinterpret_cast<const uint4*>(q4), rowsel, n_ok,
                                          counts, p.rank, p.n_rows, tau, ctrl, chunk, lane);
                }
                for (uint32_t j0 = 0; !BIT && j0 < n_ok; j0 += 2 * U) {          // fp32 / binary16 rows
                    uint32_t row[U];
                    float s[U], nx[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t j = j0 + 2 * u + half;
                        row[u] = j < n_ok ? rowsel[j] : s0;                // an empty slot reads a row of the list and is dropped
                    }
                    halfwave_row_sums<U, HALF>(p.rows, p.stride4, q4, p.metric, row, hl, s, nx);     // vsr_exact.h
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t j = j0 + 2 * u + half;
                        const bool mine = hl == 0 && j < n_ok;
                        const uint32_t br = mine ? p.rank[row[u]] : 0u;    // row[u] < s1 <= n_rows
                        const bool in_range = br < p.n_rows;
                        if (mine && !in_range) ctrl->bad = 1;              // never a key, never an address
                        const uint64_t key = make_key(exact_rank_value(p.metric, s[u], nx[u], qn), br);
                        const bool pass = mine && in_range && key < tau;
                        const uint64_t pm = __ballot(pass);
                        if (pm) {
                            const int leader = __ffsll((unsigned long long) pm) - 1;
                            uint32_t at = 0;
                            if (lane == leader) at = atomicAdd(&ctrl->count, (uint32_t) __popcll(pm));
                            at = (uint32_t) __shfl((int) at, leader) + (uint32_t) __popcll(pm & ((1ull << lane) - 1ull));
                            if (pass && at < IVI_CHUNK) chunk[at] = key;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // rowsel is rewritten by the next step
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();                                                   // every append of the batch is in the chunk
        if (ctrl->bad) stop = true;                                        // (not written again before the next batch's steps)
        ivf_iter_fold(kept, sk, chunk, ctrl, need, tid);
        // the batch's rows, sorted, behind what is already out
        uint32_t lo = 0, hi = need;                                        // real keys among kept[0 .. need)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (kept[mid] != KEY_EMPTY) lo = mid + 1; else hi = mid;
        }
        const uint32_t got = lo;
        const size_t o = (size_t) qi * k + have;
        for (uint32_t i = tid; i < got; i += 256) {
            const uint64_t key = kept[i];
            const uint32_t br = (uint32_t) key;                            // < n_rows: checked before it became a key
            p.out_block[o + i] = p.block_ids[br];
            if (p.out_doc) p.out_doc[o + i] = p.doc_ids[br];
            if (p.out_row) p.out_row[o + i] = p.orig_rows[br];
            p.out_dist[o + i] = output_distance(p.metric, mono_to_float((uint32_t) (key >> 32)));
        }
        have += got;
        __syncthreads();                                                   // kept is cleared by the next batch
    }
    if (tid == 0) {
        p.out_count[qi] = (int32_t) have;
        if (p.out_probes) p.out_probes[qi] = (int32_t) list_index;
    }
}
#endif

hipError_t launch_ivf_iterative(const IvfIterParams& p, uint32_t nq, hipStream_t s);

}  // namespace vsr
