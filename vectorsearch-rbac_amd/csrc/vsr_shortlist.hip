// vsr_shortlist.hip — the exact re-rank of a Hamming shortlist (stage 2 of vsr_search_quantized*, see vsr_shortlist.h).
//
// shortlist_rerank_kernel<HALF>: nq x ceil(shortlist / 256) workgroups, a query's side by side.  A workgroup takes 256 consecutive entries of one
// query's stage-1 list, so a one-query call still spreads its up to 2048 row gathers over 8 CUs.  It stages the query
// itself -- zero-padded to the source's row stride in LDS, through binary16 for a halfvec source, |q|^2 for cosine -- and
// then runs K5r's inner loop: half a wave per row, 4 rows in flight per half-wave, halfwave_row_sums and exact_rank_value
// of vsr_exact.h.  Sharing that code is what makes a distance of the two-stage search the bits the exact search reports
// for the same row (K5r, K1h).  Every row index comes out of a device buffer and is bounded before it is used.
//
// shortlist_emit_kernel: one workgroup per query sorts the <= 2048 re-rank keys (bitonic, 16 KB of LDS) and writes the
// first k in the layout of every other search.
#include "vsr_shortlist.h"
#include "vsr_exact.h"

namespace vsr {

template <bool HALF>
__global__ __launch_bounds__(256) void shortlist_rerank_kernel(const ShortlistParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float* qf = reinterpret_cast<float*>(smem);                            // [stride4 * 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t chunks = (p.shortlist + SL_CHUNK - 1) / SL_CHUNK;
    const uint32_t qi = blockIdx.x / chunks, base = (blockIdx.x - qi * chunks) * SL_CHUNK;   // base < shortlist
    const uint64_t* list = p.s1_keys + (size_t) qi * p.shortlist;
    uint64_t* out = p.rr_keys + (size_t) qi * p.shortlist;
    // the list is ascending with its empty entries last: a chunk that starts empty is empty (a filter admitting few rows)
    if (list[base] == KEY_EMPTY) {
        for (uint32_t c = base + (uint32_t) tid; c < base + SL_CHUNK && c < p.shortlist; c += 256) out[c] = KEY_EMPTY;
        return;                                                            // workgroup-uniform
    }
    const float* src = p.q_src + (size_t) qi * p.dim;
    for (uint32_t j = (uint32_t) tid; j < p.stride4 * 4u; j += 256) {
        const float v = j < p.dim ? src[j] : 0.0f;
        qf[j] = HALF ? (float) (_Float16) v : v;                           // what `$1::halfvec` holds, as K1h and K5r see it
    }
    __syncthreads();
    const float4* q = reinterpret_cast<const float4*>(qf);
    const float qn = wave_query_norm2(q, p.stride4, lane);

    const int half = lane >> 5, hl = lane & 31;
    constexpr int U = 4;                                                   // candidates in flight per half-wave
    for (uint32_t c0 = (uint32_t) wave * 2 * U; c0 < SL_CHUNK; c0 += 4 * 2 * U) {
        uint64_t sk[U];
        uint32_t row[U];
        float s[U], nx[U];
        bool any = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t c = base + c0 + 2 * u + half;
            sk[u] = c < p.shortlist ? list[c] : KEY_EMPTY;
            const uint32_t r = (uint32_t) sk[u] - p.s1_row_offset;
            if (sk[u] != KEY_EMPTY && r >= p.n_rows) {                     // cannot happen; never gather past the corpus
                if (hl == 0) atomicOr(p.err, 1u);
                sk[u] = KEY_EMPTY;
            }
            row[u] = sk[u] == KEY_EMPTY ? 0u : r;                          // an empty slot reads row 0 and is dropped below
            any = any || sk[u] != KEY_EMPTY;
        }
        if (__ballot(any) != 0)                                            // wave-uniform: the tail of a short list gathers nothing
            halfwave_row_sums<U, HALF>(p.rows, p.stride4, q, p.metric, row, hl, s, nx);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t c = base + c0 + 2 * u + half;
            uint64_t key = KEY_EMPTY;
            if (sk[u] != KEY_EMPTY) key = make_key(exact_rank_value(p.metric, s[u], nx[u], qn), row[u]);
            if (hl == 0 && c < p.shortlist) out[c] = key;
        }
    }
}

__global__ __launch_bounds__(256) void shortlist_emit_kernel(const ShortlistParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                    // [np2]
    __shared__ uint32_t s_count;
    const int tid = threadIdx.x;
    const uint32_t qi = blockIdx.x;
    const uint64_t* rr = p.rr_keys + (size_t) qi * p.shortlist;
    const uint32_t np2 = next_pow2(p.shortlist);
    if (tid == 0) s_count = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t c = (uint32_t) tid; c < np2; c += 256) {
        const uint64_t key = c < p.shortlist ? rr[c] : KEY_EMPTY;
        keys[c] = key;
        mine += key != KEY_EMPTY ? 1u : 0u;
    }
    for (int m = 32; m >= 1; m >>= 1) mine += (uint32_t) __shfl_xor((int) mine, m);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    bitonic_sort_lds<256>(keys, np2, tid);                                 // ends with a barrier
    const uint32_t m = s_count < p.k ? s_count : p.k;
    const size_t o = (size_t) qi * p.k;
    for (uint32_t i = (uint32_t) tid; i < p.k; i += 256) {
        if (i < m) {
            const uint64_t key = keys[i];
            const uint32_t row = (uint32_t) key;                           // < n_rows: shortlist_rerank_kernel bounded it
            p.out_block[o + i] = p.block_ids[row];
            if (p.out_doc) p.out_doc[o + i] = p.doc_ids[row];
            if (p.out_row) p.out_row[o + i] = p.orig_rows[row];
            p.out_dist[o + i] = output_distance(p.metric, mono_to_float((uint32_t) (key >> 32)));
            if (p.out_keys) p.out_keys[o + i] = (key & 0xFFFFFFFF00000000ull) | (uint64_t) (row + p.row_offset);
        } else {
            p.out_block[o + i] = -1;
            if (p.out_doc) p.out_doc[o + i] = -1;
            if (p.out_row) p.out_row[o + i] = -1;
            p.out_dist[o + i] = __builtin_inff();
            if (p.out_keys) p.out_keys[o + i] = KEY_EMPTY;
        }
    }
    if (tid == 0) p.out_count[qi] = (int32_t) m;
}

hipError_t launch_shortlist_rerank(const ShortlistParams& p, RowFormat src, uint32_t nq, hipStream_t s)
{
    if (nq == 0) return hipSuccess;
    if (p.shortlist < 1 || p.shortlist > (uint32_t) MAX_K) return hipErrorInvalidValue;
    const dim3 grid(nq * ((p.shortlist + SL_CHUNK - 1) / SL_CHUNK));      // nq <= 2^31 / 8
    const size_t lds = shortlist_rerank_lds(p.stride4);                    // <= 64000 bytes (16000 dimensions)
    if (src == RowFormat::HALF) hipLaunchKernelGGL(shortlist_rerank_kernel<true>, grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(shortlist_rerank_kernel<false>, grid, dim3(256), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_shortlist_emit(const ShortlistParams& p, uint32_t nq, hipStream_t s)
{
    if (nq == 0) return hipSuccess;
    if (p.shortlist < 1 || p.shortlist > (uint32_t) MAX_K || p.k > p.shortlist) return hipErrorInvalidValue;
    uint32_t np2 = 2;
    while (np2 < p.shortlist) np2 <<= 1;
    hipLaunchKernelGGL(shortlist_emit_kernel, dim3(nq), dim3(256), (size_t) np2 * sizeof(uint64_t), s, p);
    return hipGetLastError();
}

}  // namespace vsr
