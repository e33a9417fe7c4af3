// vsr_ivf_shortlist.h — K3q: stage 1 of the two-stage search through the bit IVFFlat index (vsr_ivf_search_quantized*): the
// Hamming shortlist of binary_quantize(q) from the lists of a vsr_ivf_load_bit index, for all queries of a call in ONE launch
// that starts at the first list.  Compiled by vsr_ivf.hip; stage 2 is quantized_rerank (vsr_shortlist.h).
//
// One 256-thread workgroup per query, K3i's bit form (ivf_iterative_kernel<IVI_BIT>, vsr_ivf_iter.h) with three differences:
//   * the packed query is made in LDS from the fp32 query: element e is read by one lane (a 4-byte load: the queries need no
//     more alignment than a float's), a wave's ballot of `q[e] > 0` -- NaN, 0 and -0.0 give 0, as binary_quantize -- is 64 bits
//     of the string, and reversing the bits inside each byte gives varbit order; elements at or past dim vote 0, so the pad bits
//     and the rest of the last chunk are clear.  No quantize launch, no staged query;
//   * no list is extracted beforehand and nothing is read from the outputs: batch 0 is scanned like every other batch;
//   * the output is keys alone: s1_keys[qi][have + i] = the batch's i-th key with the corpus's row_offset added to its row --
//     what quantized_rerank takes -- and KEY_EMPTY from the end of the scan to the end of the row.
// The centre order (ivf_center_key<IVF_BIT>, ivf_extract_nearest), the 64-row word-aligned step under the view-order bitmap
// (ivf_iter_step_masks), the gather and keys of a step (ivf_iter_bit_rows), selection (ivf_iter_fold) and the bounds rules -- a
// list id, list range or base row out of range ends that query's scan and never becomes an address -- are K3i's own code.
//
// Batches of P lists in (Hamming count, list id) centre order; a batch contributes its (shortlist - have) smallest
// ((float) Hamming, document_id, block_id) keys; the scan stops at `shortlist` rows or at M lists: the answer of
// vsr_ivf_search_bit_iterative at k = shortlist (M = P: vsr_ivf_search_bit's).
//
// LDS: ivf_shortlist_lds_bytes (vsr_ivf_lds.h).
#pragma once
#include "vsr_ivf_iter.h"

namespace vsr {

struct IvfShortlistParams {
    const float*           queries;          // [nq][dim] fp32 (device), 4-byte aligned
    uint32_t               dim;              // elements of a query = bits of a row
    const void*            centers_t;        // packed centres, [words][lists]
    uint32_t               lists;
    uint32_t               probes;           // P = min(probes, lists)
    uint32_t               max_lists;        // M = min(max(max_probes, probes), lists); iterative scan off: P
    uint32_t               shortlist;
    const uint32_t*        list_start;       // [lists + 1] offsets into the view
    const uint4*           rows;             // the view's rows, [n_rows][stride4] chunks of packed bits, pad bits clear
    uint32_t               stride4;
    uint32_t               n_rows;
    const uint32_t*        rank;             // view row -> base row
    const uint64_t* const* bitmaps;          // [nq] the query's permission bits in view order; nullptr entry: every row
    uint32_t               row_offset;       // the bit corpus's: added to the base rows the keys carry
    uint64_t*              s1_keys;          // [nq][shortlist]
    int32_t*               out_count;        // [nq] rows in the shortlist
    int32_t*               out_probes;       // [nq] lists scanned, whole batches; may be nullptr
};

#ifdef __HIPCC__
__global__ __launch_bounds__(256) void ivf_bit_shortlist_kernel(const IvfShortlistParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t qi = blockIdx.x;
    const uint32_t P = p.probes, M = p.max_lists, k = p.shortlist;
    const uint32_t sk = ivf_iter_kept(k);
    size_t off = ((size_t) p.lists * 4 + 15) & ~(size_t) 15;
    uint32_t* ckeys = reinterpret_cast<uint32_t*>(smem);                  // [lists]; 0xFFFFFFFF = taken
    uint4* q4 = reinterpret_cast<uint4*>(smem + off);                     // [stride4] the packed query
    off += (size_t) p.stride4 * 16;
    uint32_t* rowsel = reinterpret_cast<uint32_t*>(smem + off) + wave * 64;   // this wave's compacted rows of a step
    off += 4 * 64 * 4;
    float* counts = reinterpret_cast<float*>(smem + off) + wave * 64;        // this wave's Hamming counts of a step
    off += 4 * 64 * 4;
    uint64_t* kept = reinterpret_cast<uint64_t*>(smem + off);             // [sk]
    off += (size_t) sk * 8;
    uint64_t* chunk = reinterpret_cast<uint64_t*>(smem + off);            // [IVI_CHUNK]
    off += (size_t) IVI_CHUNK * 8;
    IvfIterCtrl* ctrl = reinterpret_cast<IvfIterCtrl*>(smem + off);

    {
        const float* qg = p.queries + (size_t) qi * p.dim;
        uint64_t* ql = reinterpret_cast<uint64_t*>(q4);
        for (uint32_t e0 = (uint32_t) wave * 64; e0 < p.stride4 * 128; e0 += 256) {      // (wave-uniform trip count)
            const uint32_t e = e0 + (uint32_t) lane;
            const bool set = e < p.dim && qg[e] > 0.0f;
            const uint64_t v = __ballot(set);                              // bit i: element e0 + i
            // element e0 + i -> bit 7 - i % 8 of byte i / 8: all 64 bits reversed, then the bytes put back in order
            if (lane == 0) ql[e0 >> 6] = __builtin_bswap64(__builtin_bitreverse64(v));
        }
    }
    if (tid == 0) ctrl->bad = 0;
    __syncthreads();                                                       // the centre keys read the whole query
    for (int c = tid; c < (int) p.lists; c += 256)
        ckeys[c] = ivf_center_key<IVF_BIT>(p.centers_t, (int) p.lists, (int) ((p.dim + 31u) / 32u), c, q4, 0);
    __syncthreads();

    const uint64_t* bm = p.bitmaps ? p.bitmaps[qi] : nullptr;
    uint32_t have = 0, list_index = 0;
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
            for (uint32_t base = s0 & ~63u; base < s1; base += 256) {      // K3i's step: a wave takes one word of the bitmap
                uint64_t m;
                const uint32_t step_n = ivf_iter_step_masks(base, s0, s1, bm, wave, m);
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
                if (n_ok)                                                  // (wave-uniform)
                    ivf_iter_bit_rows(p.rows, p.stride4, q4, rowsel, n_ok, counts, p.rank, p.n_rows, tau, ctrl, chunk, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // rowsel is rewritten by the next step
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();                                                   // every append of the batch is in the chunk
        if (ctrl->bad) stop = true;                                        // (not written again before the next batch's steps)
        ivf_iter_fold(kept, sk, chunk, ctrl, need, tid);
        uint32_t lo = 0, hi = need;                                        // real keys among kept[0 .. need)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (kept[mid] != KEY_EMPTY) lo = mid + 1; else hi = mid;
        }
        const uint32_t got = lo;
        // the batch's keys, sorted, behind what is already out (row + row_offset < 2^32: the corpus load's limit)
        for (uint32_t i = tid; i < got; i += 256) p.s1_keys[(size_t) qi * k + have + i] = kept[i] + p.row_offset;
        have += got;
        __syncthreads();                                                   // kept is cleared by the next batch
    }
    for (uint32_t i = have + tid; i < k; i += 256) p.s1_keys[(size_t) qi * k + i] = KEY_EMPTY;
    if (tid == 0) {
        p.out_count[qi] = (int32_t) have;
        if (p.out_probes) p.out_probes[qi] = (int32_t) list_index;
    }
}
#endif

hipError_t launch_ivf_bit_shortlist(const IvfShortlistParams& p, uint32_t nq, hipStream_t s);

}  // namespace vsr
