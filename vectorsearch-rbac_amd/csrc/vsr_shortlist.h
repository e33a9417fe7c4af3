// vsr_shortlist.h — stage 2 of the two-stage search (vsr_search_quantized*): the exact re-rank of a Hamming shortlist.
// Stage 1 is K1b over the bit corpus with k = shortlist (vsr_search.hip), or K4b over its Hamming graph (vsr_hnsw_rt.hip:
// vsr_hnsw_search_quantized*); its keys (KEY_EMPTY padded: every real key before the first empty one) name the rows whose
// SOURCE image -- fp32 or halfvec -- is gathered here.  Kernels: vsr_shortlist.hip.
#pragma once
#include "vsr_device.h"

namespace vsr {

constexpr uint32_t SL_CHUNK = 256;         // shortlist entries one re-rank workgroup takes (8 half-waves x 4 rows x 8 rounds)

struct ShortlistParams {
    // ---- shortlist_rerank_kernel: nq x ceil(shortlist / SL_CHUNK) workgroups ----
    const uint64_t* s1_keys;       // [nq][shortlist] stage-1 keys: Hamming << 32 | (internal row + s1_row_offset)
    uint32_t        shortlist;
    uint32_t        s1_row_offset; // the bits corpus's row_offset (its keys carry it)
    const float*    q_src;         // [nq][dim] fp32 queries as the caller gave them (4-byte aligned)
    uint32_t        dim;
    const float4*   rows;          // the source corpus's rows (HALF: stride4 / 2 16-byte chunks of 8 halves per row)
    uint32_t        stride4;       // float4 per padded query
    uint32_t        n_rows;        // rows of the source corpus: a key naming a row at or past it is never dereferenced
    int             metric;        // M_L2 / M_IP / M_COSINE
    uint64_t*       rr_keys;       // [nq][shortlist] <- mono_bits(exact rank value) << 32 | internal row; KEY_EMPTY: no candidate
    uint32_t*       err;           // the session's bounds-guard word (bit 0: row index out of range)
    // ---- shortlist_emit_kernel: nq workgroups ----
    uint32_t        k;
    uint32_t        row_offset;    // added to internal rows in out_keys
    const int64_t*  block_ids;
    const int32_t*  doc_ids;
    const int64_t*  orig_rows;
    int64_t*        out_block;
    int32_t*        out_doc;       // may be nullptr
    int64_t*        out_row;       // may be nullptr
    float*          out_dist;
    uint64_t*       out_keys;      // may be nullptr
    int32_t*        out_count;
};

inline size_t shortlist_rerank_lds(uint32_t stride4) { return (size_t) stride4 * 16; }   // the padded query
hipError_t launch_shortlist_rerank(const ShortlistParams& p, RowFormat src, uint32_t nq, hipStream_t s);   // src: the source rows, F32 or HALF
hipError_t launch_shortlist_emit(const ShortlistParams& p, uint32_t nq, hipStream_t s);

}  // namespace vsr
