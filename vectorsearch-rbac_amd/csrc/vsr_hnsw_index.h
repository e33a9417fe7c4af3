// vsr_hnsw_index.h -- the HNSW index object and what the two host units of the HNSW runtime share: vsr_hnsw_rt.hip (the index
// object, load, export, every search) and vsr_hnsw_build_rt.hip (build, extend, partition build, vacuum).  No device code.
#pragma once
#include "vsr_runtime.h"

// ---- K4: HNSW graph search (hnswscan.c:15-45, hnswutils.c:813-976) over a graph built elsewhere
struct vsr_hnsw {
    vsr_corpus* corpus = nullptr;
    int32_t n_elem = 0, entry = -1, entry_level = -1, m = 0, max_level = 1, n_upper = 0;
    int32_t *d_elem_row = nullptr, *d_level = nullptr, *d_nbr0 = nullptr, *d_up_slot = nullptr, *d_up_nbr = nullptr,
            *d_tid_count = nullptr, *d_tids = nullptr;
    std::map<uint64_t, uint64_t*> bitmaps;           // filters (by vsr_filter::id) without a full bitmap of their own, as one
    DevBuf d_q, d_vis, d_out, d_bm, d_disc;
    DevBuf d_qb;                                     // bit index: [staged queries | their popcounts | the staging kernel's flag and seed words]
    RowFormat format = RowFormat::F32;               // the corpus's rows: F32 (K4), HALF (vsr_hnsw_load_half / vsr_hnsw_build_half: K4h) or BIT (K4b)
    int bit_metric = 0;                              // BIT only: the opclass, VSR_METRIC_HAMMING / VSR_METRIC_JACCARD (fixed when the index
                                                     // is made: the graph is built for one distance)
    PinBuf h_out, h_bm;
    int last_mode = -1;                              // visited form of the last launch (HnswVisited)
    int predicate_aware = 0;                         // vsr_hnsw_set_predicate_aware
    int32_t vacuum_spilled = 0;                      // vsr_hnsw_vacuum: repairs run in the global-memory form; 0 for any other index
    int64_t vacuum_ws_bytes = 0;                     // and the bytes of the workspace pool they ran in
    int made_here = 0;                               // 1: this library made the graph (build, build_partitions, extend, vacuum, and
                                                     // extend_partitions for a graph that took rows or whose prior had the flag), so its
                                                     // lists are valid by construction and may be written through; 0: the arrays came from
                                                     // a caller (vsr_hnsw_load*), checked for searching only -- a plain copy of such an index
                                                     // (extend_partitions, no new rows) stays 0
};

namespace vsr {

// the caller's graph: the arrays vsr_hnsw_load takes, as they arrive.  Filled once in each entry point, never owned
struct HnswGraphView {
    int m = 0;
    int32_t n_elem = 0, entry = -1;
    const int32_t *level = nullptr, *nbr0 = nullptr, *tid_count = nullptr;
    const int64_t* tids = nullptr;                   // [n_elem][10] caller row indices
    const int32_t *up_slot = nullptr, *up_nbr = nullptr;
    int32_t n_upper = 0, max_level = 1;
};

// an index under construction: letting go of it frees its device arrays (vsr_hnsw_free waits for the stream first)
struct HnswFree { void operator()(vsr_hnsw* h) const { (void) vsr_hnsw_free(h); } };
using HnswOwner = std::unique_ptr<vsr_hnsw, HnswFree>;

// a new index over c, not registered yet.  metric: the opclass, kept for a BIT index
inline HnswOwner hnsw_new_index(vsr_corpus* c, RowFormat expect, int metric, int m)
{
    HnswOwner h(new vsr_hnsw());
    h->corpus = c;
    h->format = expect;
    h->bit_metric = expect == RowFormat::BIT ? metric : 0;
    h->m = m;
    return h;
}
// the finished index joins its corpus (vsr_hnsw_free takes it out) and becomes the caller's.  made: vsr_hnsw::made_here
inline vsr_hnsw* hnsw_register(HnswOwner h, int made = 0)
{
    h->made_here = made;
    h->corpus->hnsw_indexes.push_back(h.get());
    return h.release();
}
// caller row -> internal row
inline std::vector<int32_t> hnsw_row_map(const vsr_corpus* c)
{
    std::vector<int32_t> inv((size_t) std::max<int64_t>(c->n, 1), -1);
    for (int64_t r = 0; r < c->n; ++r) inv[(size_t) c->h_orig[(size_t) r]] = (int32_t) r;
    return inv;
}

// vsr_hnsw_rt.hip.  hnsw_load: vsr_hnsw_load (expect = F32), vsr_hnsw_load_half (HALF), vsr_hnsw_load_bit (BIT; bit_metric: the
// opclass) and vsr_hnsw_load_sparse (SPARSE): `expect` is the corpus format the entry point is for
int hnsw_load(vsr_corpus* c, RowFormat expect, int bit_metric, const HnswGraphView& g, vsr_hnsw** out, const char* who);
int upload_i32(int32_t** d, const int32_t* src, size_t count);               // a graph array into device memory of its own
// what a bit / halfvec / sparsevec entry point asks of its corpus and opclass (who: the entry point)
int hnsw_bit_opclass(const vsr_corpus* c, int metric, const char* who);
int hnsw_half_opclass(const vsr_corpus* c, const char* who);
int hnsw_sparse_opclass(const vsr_corpus* c, const char* who);
int hnsw_opclass(const vsr_corpus* c, RowFormat expect, int metric, const char* who);   // the one of the three that `expect` asks for
static const char* const HNSW_HALF_ENTRY =
    "the graph of a halfvec corpus is loaded with vsr_hnsw_load_half and built with vsr_hnsw_build_half (the halfvec_l2_ops / halfvec_ip_ops / "
    "halfvec_cosine_ops opclasses)";

}  // namespace vsr
