// vsr_hnsw_rt.hip — K4 / K4b / K4h / K4s: the HNSW index object (free, load, export, info) and every search over it: fp32 corpora
// (vsr_hnsw_*), bit corpora (vsr_hnsw_*_bit, vsr_hnsw_search_quantized*), halfvec corpora (vsr_hnsw_load_half, searched by the
// float entry points) and sparse corpora, and the forest entry points that search many indexes of one corpus as a set
// (vsr_hnsw_forest_*).  The only unit that compiles vsr_hnsw.h's and vsr_hnsw_forest_search.h's kernels; what makes a graph on
// the GPU (build, extend, partitions, vacuum) is vsr_hnsw_build_rt.hip, over the index object of vsr_hnsw_index.h.
#include "vsr_hnsw_index.h"
#include "vsr_hnsw.h"
#include "vsr_hnsw_forest_search.h"
#include "vsr_shortlist.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

extern "C" int vsr_hnsw_free(vsr_hnsw* h)
{
    if (!h) return VSR_OK;
    if (h->corpus) {
        (void) hipSetDevice(h->corpus->ctx->device);
        (void) hipStreamSynchronize(h->corpus->ctx->stream);
    }
    if (h->corpus) {
        auto& reg = h->corpus->hnsw_indexes;
        reg.erase(std::remove(reg.begin(), reg.end(), h), reg.end());
    }
    void* ptrs[] = {h->d_elem_row, h->d_level, h->d_nbr0, h->d_up_slot, h->d_up_nbr, h->d_tid_count, h->d_tids};
    for (void* p : ptrs)
        if (p) (void) hipFree(p);
    for (auto& kv : h->bitmaps)
        if (kv.second) (void) hipFree(kv.second);
    delete h;
    return VSR_OK;
}

// ---- what vsr_hnsw_index.h declares for both host units
int vsr::upload_i32(int32_t** d, const int32_t* src, size_t count)
{
    HIPCHK(hipMalloc(d, std::max<size_t>(4, count * sizeof(int32_t))));
    if (count) HIPCHK(hipMemcpy(*d, src, count * sizeof(int32_t), hipMemcpyHostToDevice));
    return VSR_OK;
}

int vsr::hnsw_bit_opclass(const vsr_corpus* c, int metric, const char* who)
{
    if (c->format != RowFormat::BIT) return fail(VSR_ERR_INVALID, "%s: the corpus is not a bit corpus", who);
    if (metric != VSR_METRIC_HAMMING && metric != VSR_METRIC_JACCARD)
        return fail(VSR_ERR_INVALID, "%s: metric %d is not an operator class of bit (4: bit_hamming_ops, 5: bit_jaccard_ops)", who, metric);
    return VSR_OK;
}

int vsr::hnsw_half_opclass(const vsr_corpus* c, const char* who)
{
    if (c->format != RowFormat::HALF) return fail(VSR_ERR_INVALID, "%s: the corpus is not a halfvec corpus", who);
    if (c->dim > 4000)           /* HNSW_MAX_DIM * 2, hnswutils.c:1390 */
        return fail(VSR_ERR_UNSUPPORTED, "%s: column cannot have more than 4000 dimensions for hnsw index", who);
    return VSR_OK;
}

// (checkValue of the sparsevec opclasses, hnswutils.c:1352-1361)
int vsr::hnsw_sparse_opclass(const vsr_corpus* c, const char* who)
{
    if (c->format != RowFormat::SPARSE) return fail(VSR_ERR_INVALID, "%s: the corpus is not a sparse corpus", who);
    if (c->sp_max_nnz > (uint32_t) HNSW_SPARSE_MAX_NNZ)
        return fail(VSR_ERR_UNSUPPORTED, "sparsevec cannot have more than %d non-zero elements for hnsw index", HNSW_SPARSE_MAX_NNZ);
    return VSR_OK;
}

int vsr::hnsw_opclass(const vsr_corpus* c, RowFormat expect, int metric, const char* who)
{
    if (expect == RowFormat::BIT) return hnsw_bit_opclass(c, metric, who);
    if (expect == RowFormat::HALF) return hnsw_half_opclass(c, who);
    if (expect == RowFormat::SPARSE) return hnsw_sparse_opclass(c, who);
    return VSR_OK;
}

int vsr::hnsw_load(vsr_corpus* c, RowFormat expect, int bit_metric, const HnswGraphView& g, vsr_hnsw** out, const char* who)
{
    const int m = g.m;
    const int32_t n_elem = g.n_elem, entry = g.entry, n_upper = g.n_upper, max_level = g.max_level;
    const int32_t *level = g.level, *nbr0 = g.nbr0, *tid_count = g.tid_count, *up_slot = g.up_slot, *up_nbr = g.up_nbr;
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (c->base) return fail(VSR_ERR_INVALID, "%s: the corpus is a view", who);
    if (const int rc = hnsw_opclass(c, expect, bit_metric, who)) return rc;
    if (c->format == RowFormat::HALF && expect != RowFormat::HALF) return fail(VSR_ERR_UNSUPPORTED, "%s: %s", who, HNSW_HALF_ENTRY);
    // (stale since K4s: the graph of a sparse corpus is loaded with vsr_hnsw_load_sparse; the text is pinned by tests)
    if (c->format == RowFormat::SPARSE && expect != RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)", who);
    if (c->format == RowFormat::BIT && expect != RowFormat::BIT)
        return fail(VSR_ERR_UNSUPPORTED, "%s: the graph of a bit corpus is loaded with vsr_hnsw_load_bit (the bit_hamming_ops / bit_jaccard_ops opclasses)", who);
    if (m < 2 || m > 100)        /* reloption m: 2 .. HNSW_MAX_M (hnsw.h:36-40) */
        return fail(VSR_ERR_UNSUPPORTED, "%s: m must be between 2 and 100 (got %d)", who, m);
    if (n_elem < 0 || (n_elem > 0 && (!level || !nbr0 || !tid_count || !g.tids || !up_slot)) || max_level < 1 || n_upper < 0 ||
        (n_upper > 0 && !up_nbr) || entry >= n_elem)
        return fail(VSR_ERR_INVALID, "%s: bad graph arrays", who);
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    HnswOwner h = hnsw_new_index(c, expect, bit_metric, m);
    h->n_elem = n_elem;
    h->entry = n_elem > 0 ? entry : -1;
    h->max_level = max_level;
    h->n_upper = n_upper;
    // heap TIDs arrive as caller row indices; the kernels work on internal rows
    const std::vector<int32_t> inv = hnsw_row_map(c);
    std::vector<int32_t> itids((size_t) std::max(n_elem, 1) * 10, -1), erow((size_t) std::max(n_elem, 1), 0);
    for (int32_t e = 0; e < n_elem; ++e) {
        if (tid_count[e] < 1 || tid_count[e] > 10 || level[e] < 0 || level[e] > max_level)
            return fail(VSR_ERR_INVALID, "%s: element %d has %d heap TIDs / level %d", who, e, tid_count[e], level[e]);
        for (int t = 0; t < tid_count[e]; ++t) {
            const int64_t row = g.tids[(size_t) e * 10 + t];
            if (row < 0 || row >= c->n) return fail(VSR_ERR_INVALID, "%s: element %d points at row %lld", who, e, (long long) row);
            itids[(size_t) e * 10 + t] = inv[(size_t) row];
        }
        erow[(size_t) e] = itids[(size_t) e * 10];
        for (int j = 0; j < 2 * m; ++j)
            if (nbr0[(size_t) e * 2 * m + j] >= n_elem) return fail(VSR_ERR_INVALID, "%s: neighbour out of range", who);
    }
    h->entry_level = h->entry >= 0 ? level[h->entry] : -1;
    auto& up = upload_i32;
    int rc;
    if ((rc = up(&h->d_elem_row, erow.data(), (size_t) n_elem)) || (rc = up(&h->d_level, level, (size_t) n_elem)) ||
        (rc = up(&h->d_nbr0, nbr0, (size_t) n_elem * 2 * m)) || (rc = up(&h->d_up_slot, up_slot, (size_t) n_elem)) ||
        (rc = up(&h->d_up_nbr, up_nbr, (size_t) n_upper * max_level * m)) || (rc = up(&h->d_tid_count, tid_count, (size_t) n_elem)) ||
        (rc = up(&h->d_tids, itids.data(), (size_t) n_elem * 10)))
        return rc;
    *out = hnsw_register(std::move(h));
    return VSR_OK;
}

extern "C" int vsr_hnsw_load(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                             const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                             int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
    return hnsw_load(c, RowFormat::F32, 0, g, out, "vsr_hnsw_load");
}

extern "C" int vsr_hnsw_load_bit(vsr_corpus* c, int metric, int m, int32_t n_elem, int32_t entry, const int32_t* level,
                                 const int32_t* nbr0, const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot,
                                 const int32_t* up_nbr, int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "vsr_hnsw_load_bit: NULL argument");
    *out = nullptr;
    int rc = hnsw_bit_opclass(c, metric, "vsr_hnsw_load_bit");
    if (rc) return rc;
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
    return hnsw_load(c, RowFormat::BIT, metric, g, out, "vsr_hnsw_load_bit");
}

extern "C" int vsr_hnsw_load_half(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                                  const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                                  int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
    return hnsw_load(c, RowFormat::HALF, 0, g, out, "vsr_hnsw_load_half");
}

extern "C" int vsr_hnsw_load_sparse(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                                    const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                                    int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
    return hnsw_load(c, RowFormat::SPARSE, 0, g, out, "vsr_hnsw_load_sparse");
}


// device memory of the graph arrays of an index (the corpus is counted by vsr_corpus_device_bytes); any index.  The row format
// of the corpus does not enter: an index over halfvec rows and one over their fp32 image loaded from the same arrays agree
extern "C" int64_t vsr_hnsw_device_bytes(const vsr_hnsw* h)
{
    if (!h) return 0;
    const size_t ne = (size_t) std::max(h->n_elem, 0);
    const size_t words = ne * 4 /* elem_row, level, up_slot, tid_count */ + ne * 2 * (size_t) h->m + ne * 10 +
                         (size_t) h->n_upper * (size_t) h->max_level * (size_t) h->m;
    return (int64_t) (words * sizeof(int32_t));
}

// the arrays vsr_hnsw_load takes, back from any index (loaded or built): shapes first, then the arrays into host memory
extern "C" int vsr_hnsw_export_shape(const vsr_hnsw* h, int32_t* m, int32_t* n_elem, int32_t* entry, int32_t* n_upper, int32_t* max_level)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_export_shape: index is NULL");
    if (m) *m = h->m;
    if (n_elem) *n_elem = h->n_elem;
    if (entry) *entry = h->entry;
    if (n_upper) *n_upper = h->n_upper;
    if (max_level) *max_level = h->max_level;
    return VSR_OK;
}

extern "C" int vsr_hnsw_export(const vsr_hnsw* h, int32_t* level, int32_t* nbr0, int32_t* tid_count, int64_t* tids, int32_t* up_slot,
                               int32_t* up_nbr)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_export: index is NULL");
    if (!level || !nbr0 || !tid_count || !tids || !up_slot || (h->n_upper > 0 && !up_nbr))
        return fail(VSR_ERR_INVALID, "vsr_hnsw_export: an output array is NULL");
    const vsr_corpus* c = h->corpus;
    HIPCHK(hipSetDevice(c->ctx->device));
    HIPCHK(hipStreamSynchronize(c->ctx->stream));
    const size_t ne = (size_t) h->n_elem;
    if (ne == 0) return VSR_OK;
    HIPCHK(hipMemcpy(level, h->d_level, ne * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nbr0, h->d_nbr0, ne * 2 * h->m * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tid_count, h->d_tid_count, ne * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(up_slot, h->d_up_slot, ne * 4, hipMemcpyDeviceToHost));
    if (h->n_upper > 0) HIPCHK(hipMemcpy(up_nbr, h->d_up_nbr, (size_t) h->n_upper * h->max_level * h->m * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> itids(ne * 10);
    HIPCHK(hipMemcpy(itids.data(), h->d_tids, ne * 10 * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ne * 10; ++i)                                      // internal rows -> the caller's row indices
        tids[i] = itids[i] >= 0 && (i % 10) < (size_t) tid_count[i / 10] ? c->h_orig[(size_t) itids[i]] : -1;
    return VSR_OK;
}

// what a build left: elements, entry point, its level, the highest level (for reports and tests)
extern "C" int vsr_hnsw_set_predicate_aware(vsr_hnsw* h, int on)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_set_predicate_aware: index is NULL");
    h->predicate_aware = on ? 1 : 0;
    return VSR_OK;
}

extern "C" int vsr_hnsw_info(const vsr_hnsw* h, int32_t* n_elem, int32_t* entry, int32_t* entry_level, int32_t* max_level)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_info: index is NULL");
    if (n_elem) *n_elem = h->n_elem;
    if (entry) *entry = h->entry;
    if (entry_level) *entry_level = h->entry_level;
    if (max_level) *max_level = h->max_level;
    return VSR_OK;
}

void vsr::purge_hnsw_caches(vsr_corpus* c, const vsr_filter* f)
{
    for (vsr_hnsw* h : c->hnsw_indexes) {
        for (auto it = h->bitmaps.begin(); it != h->bitmaps.end();) {
            if (!f || it->first == f->id) {
                if (it->second) (void) hipFree(it->second);
                it = h->bitmaps.erase(it);
            } else
                ++it;
        }
    }
}

// the rows a filter admits as a bitmap over internal rows
static int hnsw_filter_bitmap(vsr_hnsw* h, const vsr_filter* f, const uint64_t** out)
{
    vsr_corpus* c = h->corpus;
    if (f->mode == VSR_FILTER_BITMAP && f->d_bitmap) {       // role / byte-mask filters in post-filter mode: already one
        *out = f->d_bitmap;
        return VSR_OK;
    }
    auto it = h->bitmaps.find(f->id);
    if (it == h->bitmaps.end()) {
        uint64_t* d = nullptr;
        const size_t words = bitmap_words(c->n);
        HIPCHK(hipMalloc(&d, words * sizeof(uint64_t)));
        HIPCHK(hipMemsetAsync(d, 0, words * sizeof(uint64_t), c->ctx->stream));
        HIPCHK(launch_view_bitmap(nullptr, (uint32_t) c->n, f->d_tiles, f->n_tiles, f->d_bitmap, d, c->ctx->stream));
        it = h->bitmaps.emplace(f->id, d).first;
    }
    *out = it->second;
    return VSR_OK;
}

// the iterative kernel's settings for one launch (hnsw_launch: nullptr = the plain search)
struct HnswIterLaunch {
    int mode;
    int64_t max_scan;
    uint32_t cap_d;
};

// The queries of a launch in device memory: rows of `stride` floats.  A bit index: the STAGED bit strings (hnsw_stage_bits),
// stride / 4 16-byte chunks each, and their popcounts.
// A sparse index: the STAGED tables (hnsw_stage_sparse) of sp_slots slots each and their double totals; q is not read.
struct HnswQueries {
    const float* q;
    uint32_t     stride;
    const float* pop;
    const uint2*  sp_tab = nullptr;
    const double* sp_qtot = nullptr;
    uint32_t      sp_slots = 0;
    HnswQueries from_query(size_t q0) const
    {
        return {q ? q + q0 * stride : nullptr, stride, pop ? pop + q0 : nullptr, sp_tab ? sp_tab + q0 * sp_slots : nullptr,
                sp_qtot ? sp_qtot + 2 * q0 : nullptr, sp_slots};
    }
};

// the queries of a sparse entry point as the caller holds them: CSR arrays in host or in device memory, and the longest of them
struct SparseCsr {
    const int64_t* indptr;
    const int32_t* indices;
    const float*   values;
    uint32_t       max_nnz;
};

// The parameter block of one launch over the index's graph: rows, queries, the graph arrays, the LDS plan (VSR_HNSW_VISITED applies)
// and, where the plan asks for them, the global visited words of the launch's nq waves (cleared on the stream).  Results, status and
// the guard word are the caller's to set.  (vsr_hnsw_forest_search*: h is the forest's own index object, whose n_elem is the
// largest of the forest and whose graph arrays every wave replaces by its graph's, and nq counts tasks.)
static int hnsw_params(vsr_hnsw* h, vsr_ctx* ctx, const HnswQueries& qs, int nq, int k, int ef, int metric, const uint64_t* const* d_bm,
                       bool force_global, const HnswIterLaunch* iter, HnswParams& p)
{
    vsr_corpus* c = h->corpus;
    p.rows = c->d_rows;
    p.stride4 = format_row_chunks(h->format, c->dim);       // 16-byte chunks per row
    p.metric = metric;
    p.queries = qs.q;
    p.q_stride = qs.stride;
    if (h->format == RowFormat::BIT) {
        p.metric = h->bit_metric == VSR_METRIC_JACCARD ? M_JACCARD : M_HAMMING;
        p.row_pop = c->d_norm2;
        p.q_pop = qs.pop;
        p.key_row_offset = (uint32_t) c->row_offset;
    }
    if (h->format == RowFormat::HALF) p.q_chunks = p.stride4 > 64u ? p.stride4 : 0u;   // K4h: rows past 64 chunks keep the query in LDS
    if (h->format == RowFormat::SPARSE) {                   // K4s
        p.sp_off = c->d_sp_off;
        p.sp_tab = qs.sp_tab;
        p.sp_qtot = qs.sp_qtot;
        p.sp_slots = qs.sp_slots;
        p.sp_lanes = (uint32_t) c->shape.lpr;
    }
    p.dim = (uint32_t) c->dim;
    p.nq = (uint32_t) nq;
    p.n_elem = (uint32_t) h->n_elem;
    p.entry = h->entry;
    p.entry_level = h->entry_level;
    p.m = (uint32_t) h->m;
    p.max_level = (uint32_t) h->max_level;
    p.elem_row = h->d_elem_row;
    p.nbr0 = h->d_nbr0;
    p.up_slot = h->d_up_slot;
    p.up_nbr = h->d_up_nbr;
    p.level = h->d_level;
    p.tid_count = h->d_tid_count;
    p.tids = h->d_tids;
    p.bitmaps = d_bm;
    p.predicate_aware = h->predicate_aware;
    p.ef = (uint32_t) ef;
    p.k = (uint32_t) k;
    p.caps = (uint32_t) (2 * ef + 2 * h->m + 64);
    // K4s: the wave keeps its query's table in LDS (sp_slots / 2 chunks in front of the visited set) when the table fits beside S at
    // one query per workgroup; otherwise the table is read where staging wrote it (K1s's GLOBAL_TAB choice)
    auto sparse_table = [&]() {
        if (h->format != RowFormat::SPARSE) return;
        p.q_chunks = p.sp_slots / 2u;
        if (hnsw_lds_fixed(p.caps, p.q_chunks) + (iter ? (size_t) HN_HIST * 4 : 0) > HN_LDS_BUDGET) p.q_chunks = 0u;
    };
    sparse_table();
    if (iter) {                                             // (the LDS hash is sized by ef, not by the scan: never used here)
        const char* env = getenv("VSR_HNSW_VISITED");
        const bool glob = force_global || (env && !strcmp(env, "global"));
        if (!hnsw_plan_iterative(p, glob)) {
            p.caps = (uint32_t) (ef + 2 * h->m + 64);
            sparse_table();
            if (!hnsw_plan_iterative(p, glob))
                return fail(VSR_ERR_UNSUPPORTED, "vsr_hnsw_search_iterative: ef_search = %d does not fit the LDS", ef);
        }
        int rc = h->d_disc.reserve((size_t) nq * iter->cap_d * sizeof(uint64_t));
        if (rc) return rc;
        p.iter_mode = iter->mode;
        p.max_scan = iter->max_scan;
        p.disc = h->d_disc.as<uint64_t>();
        p.cap_d = iter->cap_d;
    } else if (!hnsw_plan(p, force_global)) {               // S does not fit beside anything: a shorter tail behind W
        p.caps = (uint32_t) (ef + 2 * h->m + 64);
        sparse_table();
        if (!hnsw_plan(p, force_global)) return fail(VSR_ERR_UNSUPPORTED, "vsr_hnsw_search: ef_search = %d does not fit the LDS", ef);
    }
    // development / tests: VSR_HNSW_VISITED=hash[:slots] forces the LDS hash table (with `slots` entries, a power of two) on a
    // graph small enough for the LDS bitmap, so that the table and its overflow re-run can be exercised on small graphs
    if (!force_global && !iter) {
        const char* env = getenv("VSR_HNSW_VISITED");
        if (env && !strncmp(env, "hash", 4)) {
            uint32_t slots = env[4] == ':' ? (uint32_t) atoi(env + 5) : 4096u;
            while (slots & (slots - 1)) slots &= slots - 1;
            slots = std::max(64u, slots);
            const size_t fixed = hnsw_lds_fixed(p.caps, p.q_chunks);
            if (fixed + (size_t) slots * 4 <= HN_LDS_BUDGET) {
                p.vis_mode = VIS_LDS_HASH;
                p.vis_words = slots;
                p.lds_per_query = (uint32_t) ((fixed + (size_t) slots * 4 + 15) & ~(size_t) 15);
                p.qpb = 1;
            }
        } else if (env && !strcmp(env, "global")) {
            (void) hnsw_plan(p, true);
        }
    }
    if (p.vis_mode == VIS_GLOBAL) {
        int rc = h->d_vis.reserve((size_t) nq * p.vis_words * 4);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->d_vis.p, 0, (size_t) nq * p.vis_words * 4, ctx->stream));
        p.visited = h->d_vis.as<uint32_t>();
    }
    return VSR_OK;
}

// One launch over queries resident in device memory, results into device arrays (out.keys: a bit index only, the raw keys of
// the results); bitmaps: one device pointer per query (d_bm, may be nullptr).  d_status / d_vis are optional device arrays
// (iterative: T).  The kernel is K4b when the index is over a bit corpus, K4h when it is over a halfvec corpus.
static int hnsw_launch(vsr_hnsw* h, vsr_ctx* ctx, const HnswQueries& qs, int nq, int k, int ef, int metric,
                       const uint64_t* const* d_bm, bool force_global, const Outputs& out, int64_t* d_vis, int32_t* d_status,
                       const HnswIterLaunch* iter = nullptr)
{
    vsr_corpus* c = h->corpus;
    HnswParams p{};
    int rc = hnsw_params(h, ctx, qs, nq, k, ef, metric, d_bm, force_global, iter, p);
    if (rc) return rc;
    if (h->format == RowFormat::BIT) p.out_keys = out.keys;
    set_results(p, c, out);
    p.out_visited = d_vis;
    p.out_status = d_status;
    p.err = ctx->err_word();
    HIPCHK(launch_hnsw(h->format, iter != nullptr, p, ctx->stream));
    h->last_mode = p.vis_mode;
    return VSR_OK;
}

static const char* bit_metric_name(int metric) { return metric == VSR_METRIC_JACCARD ? "Jaccard (5, bit_jaccard_ops)" : "Hamming (4, bit_hamming_ops)"; }

// entry: the queries the entry point takes -- BIT: a vsr_hnsw_search_bit* one (a bit index, `dim` bits, the index's own metric); F32
// otherwise
static int hnsw_check(vsr_hnsw* h, const void* queries, int nq, int dim, int k, int ef, int metric, const vsr_filter* const* filters,
                      const char* who, RowFormat entry)
{
    if (!h) return fail(VSR_ERR_INVALID, "%s: index is NULL", who);
    const bool bit_index = h->format == RowFormat::BIT, sparse_index = h->format == RowFormat::SPARSE;
    if (entry == RowFormat::SPARSE && !sparse_index)
        return fail(VSR_ERR_INVALID, "%s: the index is not over a sparse corpus (it is searched with vsr_hnsw_search* or vsr_hnsw_search_bit*)", who);
    if (entry != RowFormat::SPARSE && sparse_index)
        return fail(VSR_ERR_UNSUPPORTED,
                    "%s: the index is over a sparsevec corpus: it is searched with vsr_hnsw_search_sparse* (vsr_hnsw_search_sparse, "
                    "vsr_hnsw_search_sparse_device, vsr_hnsw_search_sparse_iterative, vsr_hnsw_search_sparse_iterative_device)", who);
    if (entry == RowFormat::BIT && !bit_index)
        return fail(VSR_ERR_INVALID, "%s: the index is not over a bit corpus (it is searched with vsr_hnsw_search*)", who);
    if (entry != RowFormat::BIT && bit_index)
        return fail(VSR_ERR_UNSUPPORTED, "%s: the index is over a bit corpus: it is searched with vsr_hnsw_search_bit* (<~> / <%%>)", who);
    int rc = check_search_args(h->corpus, queries, nq, dim, k, metric, filters, who, entry);
    if (rc) return rc;
    if (bit_index && metric != h->bit_metric)               // an index belongs to one opclass: the metric only catches misuse
        return fail(VSR_ERR_INVALID, "%s: the index was made for %s, the search asks for %s", who, bit_metric_name(h->bit_metric),
                    bit_metric_name(metric));
    if (metric == VSR_METRIC_L1 && !sparse_index)           // (sparsevec_l1_ops is the one L1 opclass of hnsw)
        return fail(VSR_ERR_UNSUPPORTED, "%s: L1 graphs are not supported", who);
    if (ef < 1 || ef > 5000)      /* hnsw.ef_search: 1 .. HNSW_MAX_EF_SEARCH (hnsw.c:86-89, hnsw.h:44) */
        return fail(VSR_ERR_INVALID, "%s: ef_search must be between 1 and 5000 (got %d)", who, ef);
    return VSR_OK;
}

// The host entry points over halfvec rows refuse what `$1::halfvec` refuses (halfutils.h:146-261: a finite value that rounds
// to +-Inf), as vsr_search does; the device entry points do not look.  (Also the IVFFlat entry points': vsr_ivf.hip.)
int vsr::half_query_range(const void* queries, int nq, int dim)
{
    const float* q = static_cast<const float*>(queries);
    const size_t total = (size_t) nq * (size_t) dim;
    for (size_t i = 0; i < total; ++i)
        if (std::isfinite(q[i]) && std::fabs(q[i]) >= 65520.0f)
            return fail(VSR_ERR_INVALID, "\"%.9g\" is out of range for type halfvec", (double) q[i]);
    return VSR_OK;
}

// Query staging of a bit index: nq packed strings of (dim + 7) / 8 bytes at d_src (any alignment) -> 16-byte chunks with the
// pad bits cleared, and their popcounts, in h->d_qb (stage_bit_kernel, vsr_bit.hip: the staging of vsr_search_bit).  One launch
// on the context's stream.
static int hnsw_stage_bits(vsr_hnsw* h, vsr_ctx* ctx, const uint8_t* d_src, int nq, HnswQueries& qs)
{
    const vsr_corpus* c = h->corpus;
    const size_t slot = (size_t) c->stride4 * 16;
    const size_t o_pop = align_up((size_t) nq * slot, 256), o_flags = align_up(o_pop + (size_t) nq * 4, 256),
                 o_tau = align_up(o_flags + (size_t) nq * 4, 256), total = o_tau + (size_t) nq * 8;
    int rc = h->d_qb.reserve(total);
    if (rc) return rc;
    char* w = h->d_qb.as<char>();
    StageParams st{};
    st.q_src = reinterpret_cast<const float*>(d_src);
    st.q_stride = (uint32_t) ((c->dim + 7) / 8);            // bytes
    st.q_dst = reinterpret_cast<float*>(w);
    st.dim = (uint32_t) c->dim;
    st.qfloats = c->stride4 * 4u;
    st.nq = (uint32_t) nq;
    st.q_bits = 1u;
    st.q_norm2 = reinterpret_cast<float*>(w + o_pop);
    st.flags = reinterpret_cast<int32_t*>(w + o_flags);     // (the staging kernel clears a flag and a seed word per query: unused here)
    st.tau = reinterpret_cast<uint64_t*>(w + o_tau);
    HIPCHK(launch_stage_bit(st, ctx->stream));
    qs = {reinterpret_cast<const float*>(w), c->stride4 * 4u, reinterpret_cast<const float*>(w + o_pop)};
    return VSR_OK;
}

// Query staging of a sparse index: nq queries as CSR arrays in device memory -> one open-addressing table of `slots` (index, value)
// slots per query (slots: a power of two >= 2 x max_nnz, the same for every query of the call), their double totals Q2 / Q1 and
// |q|^2, in h->d_qb (stage_sparse_kernel, vsr_sparse.hip: the staging of vsr_search_sparse).  A query longer than max_nnz becomes an
// empty table and sets SPARSE_ERR_QUERY in the session's guard word.  One launch on the context's stream.
static int hnsw_stage_sparse(vsr_hnsw* h, vsr_ctx* ctx, const SparseCsr& d, int nq, HnswQueries& qs)
{
    const vsr_corpus* c = h->corpus;
    const uint32_t slots = sparse_slots_for_nnz(d.max_nnz);
    const size_t o_tot = align_up((size_t) nq * slots * sizeof(uint2), 256), o_norm = align_up(o_tot + (size_t) nq * 2 * sizeof(double), 256),
                 o_flags = align_up(o_norm + (size_t) nq * 4, 256), o_tau = align_up(o_flags + (size_t) nq * 4, 256),
                 total = o_tau + (size_t) nq * 8;
    int rc = h->d_qb.reserve(total);
    if (rc) return rc;
    char* w = h->d_qb.as<char>();
    SparseStageParams st{};
    st.indptr = d.indptr;
    st.indices = d.indices;
    st.values = d.values;
    st.nq = (uint32_t) nq;
    st.dim = (uint32_t) c->dim;
    st.max_nnz = d.max_nnz;
    st.slots = slots;
    st.shift = 32u - (uint32_t) __builtin_ctz(slots);
    st.tab = reinterpret_cast<uint2*>(w);
    st.qtot = reinterpret_cast<double*>(w + o_tot);
    st.q_norm2 = reinterpret_cast<float*>(w + o_norm);
    st.flags = reinterpret_cast<int32_t*>(w + o_flags);     // (the staging kernel clears a flag and a seed word per query: unused here)
    st.tau = reinterpret_cast<uint64_t*>(w + o_tau);
    st.err = ctx->err_word();
    HIPCHK(launch_stage_sparse(st, ctx->stream));
    qs = {nullptr, 0u, nullptr, reinterpret_cast<const uint2*>(w), reinterpret_cast<const double*>(w + o_tot), slots};
    return VSR_OK;
}

// per-query permission bitmaps as a device array of pointers (nullptr entries: no filter); any_filter = false: none at all
static int hnsw_bitmaps(vsr_hnsw* h, vsr_ctx* ctx, const vsr_filter* const* filters, int n, bool& any_filter)
{
    any_filter = false;
    std::vector<const uint64_t*> bms((size_t) n, nullptr);
    int rc;
    for (int i = 0; i < n; ++i)
        if (filters && filters[i]) {
            if ((rc = hnsw_filter_bitmap(h, filters[i], &bms[(size_t) i]))) return rc;
            any_filter = true;
        }
    if (!any_filter) return VSR_OK;
    if ((rc = h->d_bm.reserve((size_t) n * sizeof(uint64_t*)))) return rc;
    if ((rc = h->h_bm.reserve((size_t) n * sizeof(uint64_t*)))) return rc;
    memcpy(h->h_bm.p, bms.data(), (size_t) n * sizeof(uint64_t*));
    HIPCHK(hipMemcpyAsync(h->d_bm.p, h->h_bm.p, (size_t) n * sizeof(uint64_t*), hipMemcpyHostToDevice, ctx->stream));
    return VSR_OK;
}

// a device entry point's optional document array: the kernels always write one
static int hnsw_doc_scratch(vsr_hnsw* h, int nq, int k, int32_t*& d_doc)
{
    if (d_doc) return VSR_OK;
    int rc = h->d_out.reserve((size_t) nq * k * sizeof(int32_t));
    if (rc) return rc;
    d_doc = h->d_out.as<int32_t>();
    return VSR_OK;
}

// The queries of a search entry point, fp32 or bit.  Float: rows of `dim` floats.  Bit: packed strings of (dim + 7) / 8 bytes,
// staged (hnsw_stage_bits) in front of every launch.
struct HnswEntry {
    const char* who;
    RowFormat   queries;                                    // F32, BIT or SPARSE (then the query pointer addresses a SparseCsr)
    size_t bytes(int dim) const { return format_query_bytes(queries, dim); }
    // queries resident at d_q -> what hnsw_launch takes (bit, sparse: one staging launch on the stream)
    int resident(vsr_hnsw* h, vsr_ctx* ctx, const void* d_q, int nq, int dim, HnswQueries& qs) const
    {
        if (queries == RowFormat::SPARSE) return hnsw_stage_sparse(h, ctx, *static_cast<const SparseCsr*>(d_q), nq, qs);
        qs = {static_cast<const float*>(d_q), (uint32_t) dim, nullptr};
        return queries == RowFormat::BIT ? hnsw_stage_bits(h, ctx, static_cast<const uint8_t*>(d_q), nq, qs) : VSR_OK;
    }
};

// vsr_hnsw_search_device / vsr_hnsw_search_bit_device: (bit: query staging plus) ONE search launch, no synchronisation
static int hnsw_search_device(const HnswEntry& en, vsr_hnsw* h, const void* d_queries, int nq, int dim, int k, int ef, int metric,
                              const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist,
                              int32_t* d_cnt, int64_t* d_visited)
{
    int rc = hnsw_check(h, d_queries, nq, dim, k, ef, metric, filters, en.who, en.queries);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = hnsw_doc_scratch(h, nq, k, d_doc))) return rc;
    bool any_filter = false;
    if (h->h_bm.p) HIPCHK(hipStreamSynchronize(ctx->stream));            // the pinned pointer block of the previous call
    if ((rc = hnsw_bitmaps(h, ctx, filters, nq, any_filter))) return rc;
    HnswQueries qs;
    if ((rc = en.resident(h, ctx, d_queries, nq, dim, qs))) return rc;
    return hnsw_launch(h, ctx, qs, nq, k, ef, metric, any_filter ? h->d_bm.as<const uint64_t*>() : nullptr, false,
                       {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr}, d_visited, nullptr);
}

extern "C" int vsr_hnsw_search_device(vsr_hnsw* h, const float* d_queries, int nq, int dim, int k, int ef, int metric,
                                      const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                      float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    return hnsw_search_device({"vsr_hnsw_search_device", RowFormat::F32}, h, d_queries, nq, dim, k, ef, metric, filters, d_blk, d_doc, d_row, d_dist,
                              d_cnt, d_visited);
}

extern "C" int vsr_hnsw_search_bit_device(vsr_hnsw* h, const uint8_t* d_queries, int nq, int dim, int k, int ef, int metric,
                                          const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                          float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    return hnsw_search_device({"vsr_hnsw_search_bit_device", RowFormat::BIT}, h, d_queries, nq, dim, k, ef, metric, filters, d_blk, d_doc, d_row,
                              d_dist, d_cnt, d_visited);
}

// The host form of a K4 search.  `launch(d_q, n, filters, tier, results, d_extra, d_status)` runs n device-resident queries
// (qbytes bytes each, as the caller holds them) at re-run tier 0 or 1; the whole call is one launch and one copy back, then
// ONE re-run, a tier up, of the queries whose status word says their first result is not valid (rare; big graphs or long
// scans only), patched into the caller's arrays.
template <class Launch>
static int hnsw_host_search(vsr_hnsw* h, const void* queries, size_t qbytes, int nq, int k, const vsr_filter* const* filters,
                            const Outputs& out, int64_t* out_extra, Launch launch)
{
    vsr_ctx* ctx = h->corpus->ctx;
    const ResultBlock rb(nq, k, true);
    int rc;
    if ((rc = h->d_q.reserve((size_t) nq * qbytes))) return rc;
    if ((rc = h->d_out.reserve(rb.total))) return rc;
    if ((rc = h->h_out.reserve(rb.total))) return rc;
    char* d = h->d_out.as<char>();
    char* hh = h->h_out.as<char>();
    auto run = [&](const void* qs, int n, const vsr_filter* const* fs, int tier) -> int {
        HIPCHK(hipMemcpyAsync(h->d_q.p, qs, (size_t) n * qbytes, hipMemcpyHostToDevice, ctx->stream));
        int r = launch(h->d_q.p, n, fs, tier, rb.arrays(d), rb.column<int64_t>(d, rb.o_extra), rb.column<int32_t>(d, rb.o_status));
        if (r) return r;
        HIPCHK(hipMemcpyAsync(hh, d, rb.total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    };
    if ((rc = run(queries, nq, filters, 0))) return rc;
    rb.copy_out_all(hh, out, out_extra);
    const std::vector<int> redo = rb.flagged(hh, (size_t) nq);
    if (redo.empty()) return VSR_OK;
    std::vector<char> q2(redo.size() * qbytes);
    std::vector<const vsr_filter*> f2(redo.size(), nullptr);
    for (size_t j = 0; j < redo.size(); ++j) {
        memcpy(&q2[j * qbytes], static_cast<const char*>(queries) + (size_t) redo[j] * qbytes, qbytes);
        if (filters) f2[j] = filters[redo[j]];
    }
    if ((rc = run(q2.data(), (int) redo.size(), f2.data(), 1))) return rc;
    for (size_t j = 0; j < redo.size(); ++j) rb.patch_one(hh, j, (size_t) redo[j], out, out_extra);
    return VSR_OK;
}

// hnsw_host_search over CSR queries in host memory (validated by the entry point): the three arrays travel to h->d_q, `launch`
// takes a SparseCsr of device pointers; the re-run's queries are the flagged ones gathered into a CSR triple of their own.
template <class Launch>
static int hnsw_host_search_sparse(vsr_hnsw* h, const SparseCsr& q, int nq, int k, const vsr_filter* const* filters, const Outputs& out,
                                   int64_t* out_extra, Launch launch)
{
    vsr_ctx* ctx = h->corpus->ctx;
    const ResultBlock rb(nq, k, true);
    int rc;
    if ((rc = h->d_out.reserve(rb.total))) return rc;
    if ((rc = h->h_out.reserve(rb.total))) return rc;
    char* d = h->d_out.as<char>();
    char* hh = h->h_out.as<char>();
    // ptr: n + 1 offsets starting at 0; idx / val: the entries they address
    auto run = [&](const int64_t* ptr, const int32_t* idx, const float* val, int n, const vsr_filter* const* fs, int tier) -> int {
        const size_t nnz = (size_t) ptr[n];
        const size_t o_idx = align_up(((size_t) n + 1) * 8, 256), o_val = align_up(o_idx + nnz * 4, 256), total = o_val + nnz * 4;
        int r = h->d_q.reserve(total);
        if (r) return r;
        char* dq = h->d_q.as<char>();
        HIPCHK(hipMemcpyAsync(dq, ptr, ((size_t) n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (nnz) {
            HIPCHK(hipMemcpyAsync(dq + o_idx, idx, nnz * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(dq + o_val, val, nnz * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        const SparseCsr dev{reinterpret_cast<const int64_t*>(dq), reinterpret_cast<const int32_t*>(dq + o_idx),
                            reinterpret_cast<const float*>(dq + o_val), q.max_nnz};
        r = launch(&dev, n, fs, tier, rb.arrays(d), rb.column<int64_t>(d, rb.o_extra), rb.column<int32_t>(d, rb.o_status));
        if (r) return r;
        HIPCHK(hipMemcpyAsync(hh, d, rb.total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    };
    std::vector<int64_t> ptr((size_t) nq + 1);
    for (int i = 0; i <= nq; ++i) ptr[(size_t) i] = q.indptr[i] - q.indptr[0];
    if ((rc = run(ptr.data(), q.indices + q.indptr[0], q.values + q.indptr[0], nq, filters, 0))) return rc;
    rb.copy_out_all(hh, out, out_extra);
    const std::vector<int> redo = rb.flagged(hh, (size_t) nq);
    if (redo.empty()) return VSR_OK;
    std::vector<int64_t> ptr2(redo.size() + 1, 0);
    std::vector<int32_t> idx2;
    std::vector<float> val2;
    std::vector<const vsr_filter*> f2(redo.size(), nullptr);
    for (size_t j = 0; j < redo.size(); ++j) {
        const int64_t b = q.indptr[redo[j]], e = q.indptr[redo[j] + 1];
        idx2.insert(idx2.end(), q.indices + b, q.indices + e);
        val2.insert(val2.end(), q.values + b, q.values + e);
        ptr2[j + 1] = ptr2[j] + (e - b);
        if (filters) f2[j] = filters[redo[j]];
    }
    if ((rc = run(ptr2.data(), idx2.data(), val2.data(), (int) redo.size(), f2.data(), 1))) return rc;
    for (size_t j = 0; j < redo.size(); ++j) rb.patch_one(hh, j, (size_t) redo[j], out, out_extra);
    return VSR_OK;
}

// vsr_hnsw_search / vsr_hnsw_search_bit / vsr_hnsw_search_sparse (then `queries` addresses a SparseCsr of host arrays)
static int hnsw_search_host(const HnswEntry& en, vsr_hnsw* h, const void* queries, int nq, int dim, int k, int ef, int metric,
                            const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row, float* out_dist,
                            int32_t* out_cnt, int64_t* out_visited)
{
    int rc = hnsw_check(h, queries, nq, dim, k, ef, metric, filters, en.who, en.queries);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    if (h->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    // tier 1: queries whose LDS visited table overflowed (big graphs only) are re-run with the global bitmap
    const auto launch = [&](const void* d_q, int n, const vsr_filter* const* fs, int tier, const Outputs& res, int64_t* d_vis,
                            int32_t* d_status) -> int {
        bool any_filter = false;
        int r = hnsw_bitmaps(h, ctx, fs, n, any_filter);
        if (r) return r;
        HnswQueries qs;
        if ((r = en.resident(h, ctx, d_q, n, dim, qs))) return r;
        return hnsw_launch(h, ctx, qs, n, k, ef, metric, any_filter ? h->d_bm.as<const uint64_t*>() : nullptr, tier == 1, res, d_vis, d_status);
    };
    const Outputs out{out_blk, out_doc, out_row, out_dist, out_cnt, nullptr};
    if (en.queries == RowFormat::SPARSE)
        return hnsw_host_search_sparse(h, *static_cast<const SparseCsr*>(queries), nq, k, filters, out, out_visited, launch);
    return hnsw_host_search(h, queries, en.bytes(dim), nq, k, filters, out, out_visited, launch);
}

extern "C" int vsr_hnsw_search(vsr_hnsw* h, const float* queries, int nq, int dim, int k, int ef, int metric,
                               const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                               float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    return hnsw_search_host({"vsr_hnsw_search", RowFormat::F32}, h, queries, nq, dim, k, ef, metric, filters, out_blk, out_doc, out_row, out_dist,
                            out_cnt, out_visited);
}

extern "C" int vsr_hnsw_search_bit(vsr_hnsw* h, const uint8_t* queries, int nq, int dim, int k, int ef, int metric,
                                   const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                                   float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    return hnsw_search_host({"vsr_hnsw_search_bit", RowFormat::BIT}, h, queries, nq, dim, k, ef, metric, filters, out_blk, out_doc, out_row, out_dist,
                            out_cnt, out_visited);
}

// ---- iterative index scans (hnsw.iterative_scan, hnsw.max_scan_tuples; vsr_hnsw.h's header comment) ----------------
constexpr size_t HN_ITER_WORKSPACE = (size_t) 1 << 30;      // per launch: D + global visited bitmaps of its queries

static int hnsw_iter_check(vsr_hnsw* h, const void* queries, int nq, int dim, int k, int ef, int metric,
                           const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, const HnswEntry& en)
{
    const char* who = en.who;
    int rc = hnsw_check(h, queries, nq, dim, k, ef, metric, filters, who, en.queries);
    if (rc) return rc;
    if (mode < VSR_HNSW_ITERATIVE_OFF || mode > VSR_HNSW_ITERATIVE_STRICT) return fail(VSR_ERR_INVALID, "%s: iterative scan mode %d", who, mode);
    if (max_scan_tuples < 1 || max_scan_tuples > INT_MAX)   /* hnsw.max_scan_tuples: 1 .. INT_MAX (hnsw.c:95-97) */
        return fail(VSR_ERR_INVALID, "%s: max_scan_tuples must be between 1 and %d (got %lld)", who, INT_MAX, (long long) max_scan_tuples);
    if (mode != VSR_HNSW_ITERATIVE_OFF && h->predicate_aware)
        return fail(VSR_ERR_UNSUPPORTED, "%s: iterative scans of the predicate-aware walk are not supported", who);
    return VSR_OK;
}

// D's capacity: max_scan_tuples plus what one more round may visit beyond it (|D| <= T), at most every element.
// VSR_HNSW_DISCARD_CAP=n (development / tests) forces n, so that the overflow re-run can be exercised on small graphs
static uint32_t hnsw_discard_cap(const vsr_hnsw* h, int ef, int64_t max_scan_tuples)
{
    const int64_t slack = (int64_t) 4 * h->m * ef + 4096;    // (a round visits ~20 x ef elements at m = 16)
    int64_t cap = std::min<int64_t>(h->n_elem, max_scan_tuples + slack);
    if (const char* env = getenv("VSR_HNSW_DISCARD_CAP")) {
        const long long forced = atoll(env);
        if (forced > 0) cap = std::min<int64_t>(h->n_elem, forced);
    }
    return (uint32_t) std::max<int64_t>(cap, 1);
}

// the iterative kernel over queries resident on the device, one launch per chunk of queries whose workspace stays under
// HN_ITER_WORKSPACE, on the context's stream without synchronisation
static int hnsw_iter_run(vsr_hnsw* h, const HnswQueries& qs, int nq, int k, int ef, int metric, const vsr_filter* const* filters,
                         int mode, int64_t max_scan_tuples, uint32_t cap_d, const Outputs& out, int64_t* d_tuples, int32_t* d_status)
{
    vsr_ctx* ctx = h->corpus->ctx;
    bool any_filter = false;
    int rc;
    if (h->h_bm.p) HIPCHK(hipStreamSynchronize(ctx->stream));            // the pinned pointer block of the previous call
    if ((rc = hnsw_bitmaps(h, ctx, filters, nq, any_filter))) return rc;
    const size_t per_query = (size_t) cap_d * 8 + (((size_t) h->n_elem + 31) / 32) * 4;
    const int chunk = (int) std::max<size_t>(1, std::min<size_t>((size_t) nq, HN_ITER_WORKSPACE / per_query));
    const HnswIterLaunch it{mode, max_scan_tuples, cap_d};
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int n = std::min(chunk, nq - q0);
        if ((rc = hnsw_launch(h, ctx, qs.from_query((size_t) q0), n, k, ef, metric,
                              any_filter ? h->d_bm.as<const uint64_t*>() + q0 : nullptr, false, out.from_query((size_t) q0, k),
                              d_tuples ? d_tuples + q0 : nullptr, d_status ? d_status + q0 : nullptr, &it)))
            return rc;
    }
    return VSR_OK;
}

// vsr_hnsw_search_iterative_device / vsr_hnsw_search_bit_iterative_device
static int hnsw_iterative_device(const HnswEntry& en, vsr_hnsw* h, const void* d_queries, int nq, int dim, int k, int ef, int metric,
                                 const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, int64_t* d_blk, int32_t* d_doc,
                                 int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_tuples)
{
    int rc = hnsw_iter_check(h, d_queries, nq, dim, k, ef, metric, filters, mode, max_scan_tuples, en);
    if (rc) return rc;
    if (mode == VSR_HNSW_ITERATIVE_OFF)
        return hnsw_search_device(en, h, d_queries, nq, dim, k, ef, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_tuples);
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = hnsw_doc_scratch(h, nq, k, d_doc))) return rc;
    HnswQueries qs;
    if ((rc = en.resident(h, ctx, d_queries, nq, dim, qs))) return rc;
    return hnsw_iter_run(h, qs, nq, k, ef, metric, filters, mode, max_scan_tuples, hnsw_discard_cap(h, ef, max_scan_tuples),
                         {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr}, d_tuples, nullptr);
}

extern "C" int vsr_hnsw_search_iterative_device(vsr_hnsw* h, const float* d_queries, int nq, int dim, int k, int ef, int metric,
                                                const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                                int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                                int64_t* d_tuples)
{
    return hnsw_iterative_device({"vsr_hnsw_search_iterative_device", RowFormat::F32}, h, d_queries, nq, dim, k, ef, metric, filters, mode,
                                 max_scan_tuples, d_blk, d_doc, d_row, d_dist, d_cnt, d_tuples);
}

extern "C" int vsr_hnsw_search_bit_iterative_device(vsr_hnsw* h, const uint8_t* d_queries, int nq, int dim, int k, int ef, int metric,
                                                    const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                                    int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                                    int64_t* d_tuples)
{
    return hnsw_iterative_device({"vsr_hnsw_search_bit_iterative_device", RowFormat::BIT}, h, d_queries, nq, dim, k, ef, metric, filters, mode,
                                 max_scan_tuples, d_blk, d_doc, d_row, d_dist, d_cnt, d_tuples);
}

// vsr_hnsw_search_iterative / vsr_hnsw_search_bit_iterative
static int hnsw_iterative_host(const HnswEntry& en, vsr_hnsw* h, const void* queries, int nq, int dim, int k, int ef, int metric,
                               const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, int64_t* out_blk, int32_t* out_doc,
                               int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_tuples)
{
    int rc = hnsw_iter_check(h, queries, nq, dim, k, ef, metric, filters, mode, max_scan_tuples, en);
    if (rc) return rc;
    if (mode == VSR_HNSW_ITERATIVE_OFF)                      // hnsw.iterative_scan = off: the plain search, T = the visited count
        return hnsw_search_host(en, h, queries, nq, dim, k, ef, metric, filters, out_blk, out_doc, out_row, out_dist, out_cnt, out_tuples);
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    if (h->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    // tier 1: queries whose D overflowed, again with room for every element (an element is in at most one of D, W, emitted)
    const uint32_t cap_d[2] = {hnsw_discard_cap(h, ef, max_scan_tuples), (uint32_t) std::max(h->n_elem, 1)};
    const auto launch = [&](const void* d_q, int n, const vsr_filter* const* fs, int tier, const Outputs& res, int64_t* d_tup,
                            int32_t* d_status) -> int {
        HnswQueries qs;
        int r = en.resident(h, ctx, d_q, n, dim, qs);
        if (r) return r;
        return hnsw_iter_run(h, qs, n, k, ef, metric, fs, mode, max_scan_tuples, cap_d[tier], res, d_tup, d_status);
    };
    const Outputs out{out_blk, out_doc, out_row, out_dist, out_cnt, nullptr};
    if (en.queries == RowFormat::SPARSE)
        return hnsw_host_search_sparse(h, *static_cast<const SparseCsr*>(queries), nq, k, filters, out, out_tuples, launch);
    return hnsw_host_search(h, queries, en.bytes(dim), nq, k, filters, out, out_tuples, launch);
}

extern "C" int vsr_hnsw_search_iterative(vsr_hnsw* h, const float* queries, int nq, int dim, int k, int ef, int metric,
                                         const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, int64_t* out_blk,
                                         int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_tuples)
{
    return hnsw_iterative_host({"vsr_hnsw_search_iterative", RowFormat::F32}, h, queries, nq, dim, k, ef, metric, filters, mode, max_scan_tuples,
                               out_blk, out_doc, out_row, out_dist, out_cnt, out_tuples);
}

extern "C" int vsr_hnsw_search_bit_iterative(vsr_hnsw* h, const uint8_t* queries, int nq, int dim, int k, int ef, int metric,
                                             const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, int64_t* out_blk,
                                             int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_tuples)
{
    return hnsw_iterative_host({"vsr_hnsw_search_bit_iterative", RowFormat::BIT}, h, queries, nq, dim, k, ef, metric, filters, mode, max_scan_tuples,
                               out_blk, out_doc, out_row, out_dist, out_cnt, out_tuples);
}

// ---- K4s: the entry points of an index over a sparse corpus.  Queries are CSR; the metric is given per call, L2 .. L1 -----------
// a host entry point's queries, validated as vsr_search_sparse validates them
static int hnsw_sparse_host_queries(const char* who, vsr_hnsw* h, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values,
                                    int nq, int dim, int k, int metric, const vsr_filter* const* filters, SparseCsr& out)
{
    if (!h) return fail(VSR_ERR_INVALID, "%s: index is NULL", who);
    if (h->format != RowFormat::SPARSE)
        return fail(VSR_ERR_INVALID, "%s: the index is not over a sparse corpus (it is searched with vsr_hnsw_search* or vsr_hnsw_search_bit*)", who);
    int rc = check_search_args(h->corpus, q_indptr, nq, dim, k, metric, filters, who, RowFormat::SPARSE);
    if (rc) return rc;
    uint32_t max_nnz = 0;
    if ((rc = check_sparse_rows(who, q_indptr, q_indices, q_values, nq, dim, &max_nnz))) return rc;
    out = {q_indptr, q_indices, q_values, max_nnz};
    return VSR_OK;
}

// a device entry point's queries: nothing is read here; max_query_nnz sizes the tables (a longer query: an empty table and the guard bit)
static int hnsw_sparse_device_queries(const char* who, vsr_hnsw* h, const int64_t* d_indptr, const int32_t* d_indices, const float* d_values,
                                      int nq, int max_query_nnz, SparseCsr& out)
{
    if (!h) return fail(VSR_ERR_INVALID, "%s: index is NULL", who);
    if (nq < 0 || (nq > 0 && !d_indptr)) return fail(VSR_ERR_INVALID, "%s: queries is NULL", who);
    if (max_query_nnz < 0 || max_query_nnz > SPARSE_MAX_NNZ)
        return fail(VSR_ERR_INVALID, "%s: max_query_nnz must be between 0 and %d (got %d)", who, SPARSE_MAX_NNZ, max_query_nnz);
    if (nq > 0 && max_query_nnz > 0 && (!d_indices || !d_values)) return fail(VSR_ERR_INVALID, "%s: queries is NULL", who);
    out = {d_indptr, d_indices, d_values, (uint32_t) max_query_nnz};
    return VSR_OK;
}

extern "C" int vsr_hnsw_search_sparse(vsr_hnsw* h, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq, int dim,
                                      int k, int ef, int metric, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                                      int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    const char* who = "vsr_hnsw_search_sparse";
    SparseCsr q{};
    int rc = hnsw_sparse_host_queries(who, h, q_indptr, q_indices, q_values, nq, dim, k, metric, filters, q);
    if (rc) return rc;
    return hnsw_search_host({who, RowFormat::SPARSE}, h, &q, nq, dim, k, ef, metric, filters, out_blk, out_doc, out_row, out_dist, out_cnt,
                            out_visited);
}

extern "C" int vsr_hnsw_search_sparse_device(vsr_hnsw* h, const int64_t* d_indptr, const int32_t* d_indices, const float* d_values, int nq,
                                             int dim, int max_query_nnz, int k, int ef, int metric, const vsr_filter* const* filters,
                                             int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    const char* who = "vsr_hnsw_search_sparse_device";
    SparseCsr q{};
    int rc = hnsw_sparse_device_queries(who, h, d_indptr, d_indices, d_values, nq, max_query_nnz, q);
    if (rc) return rc;
    return hnsw_search_device({who, RowFormat::SPARSE}, h, &q, nq, dim, k, ef, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_visited);
}

extern "C" int vsr_hnsw_search_sparse_iterative(vsr_hnsw* h, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq,
                                                int dim, int k, int ef, int metric, const vsr_filter* const* filters, int mode,
                                                int64_t max_scan_tuples, int64_t* out_blk, int32_t* out_doc, int64_t* out_row, float* out_dist,
                                                int32_t* out_cnt, int64_t* out_tuples)
{
    const char* who = "vsr_hnsw_search_sparse_iterative";
    SparseCsr q{};
    int rc = hnsw_sparse_host_queries(who, h, q_indptr, q_indices, q_values, nq, dim, k, metric, filters, q);
    if (rc) return rc;
    return hnsw_iterative_host({who, RowFormat::SPARSE}, h, &q, nq, dim, k, ef, metric, filters, mode, max_scan_tuples, out_blk, out_doc, out_row,
                               out_dist, out_cnt, out_tuples);
}

extern "C" int vsr_hnsw_search_sparse_iterative_device(vsr_hnsw* h, const int64_t* d_indptr, const int32_t* d_indices, const float* d_values,
                                                       int nq, int dim, int max_query_nnz, int k, int ef, int metric,
                                                       const vsr_filter* const* filters, int mode, int64_t max_scan_tuples, int64_t* d_blk,
                                                       int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_tuples)
{
    const char* who = "vsr_hnsw_search_sparse_iterative_device";
    SparseCsr q{};
    int rc = hnsw_sparse_device_queries(who, h, d_indptr, d_indices, d_values, nq, max_query_nnz, q);
    if (rc) return rc;
    return hnsw_iterative_device({who, RowFormat::SPARSE}, h, &q, nq, dim, k, ef, metric, filters, mode, max_scan_tuples, d_blk, d_doc, d_row,
                                 d_dist, d_cnt, d_tuples);
}

// ---- indexed two-stage search: the Hamming shortlist from the bit graph (K4b), the exact re-rank on the source rows ----
// vsr_search_quantized with stage 1 replaced by the index: binary_quantize of the queries -> query staging -> ONE K4b launch
// with k = shortlist whose epilogue writes the stage-1 keys -> the re-rank and emit launches of vsr_shortlist.h
// (quantized_rerank, vsr_search.hip).  Everything on the bit corpus context's stream, no host round trip.  d_status: optional
// [nq] status words of stage 1 (1: the LDS visited table overflowed; that query's shortlist is empty).
static int hnsw_quantized_impl(vsr_corpus* src, vsr_hnsw* h, const float* h_queries, const float* d_queries, int nq, int dim, int k,
                               int shortlist, int ef, int metric, const vsr_filter* const* filters, bool force_global,
                               const Outputs& out, int32_t* d_status)
{
    vsr_corpus* bits = h->corpus;
    vsr_ctx* ctx = bits->ctx;
    const size_t ns = (size_t) nq * (size_t) shortlist, qbytes = (size_t) (dim + 7) / 8;
    // scratch: [fp32 queries of a host call | bit queries | stage-1 keys | stage-1 block ids, then the re-rank keys | doc | dist | counts]
    const size_t o_q = 0, o_qb = align_up(o_q + (h_queries ? (size_t) nq * dim * sizeof(float) : 0), 256),
                 o_key = align_up(o_qb + (size_t) nq * qbytes, 256), o_blk = align_up(o_key + ns * 8, 256),
                 o_doc = align_up(o_blk + ns * 8, 256), o_dist = align_up(o_doc + ns * 4, 256),
                 o_cnt = align_up(o_dist + ns * 4, 256), total = align_up(o_cnt + (size_t) nq * 4, 256);
    int rc = ctx->d_short.reserve(total);
    if (rc) return rc;
    char* w = ctx->d_short.as<char>();
    if (h_queries) {
        HIPCHK(hipMemcpyAsync(w + o_q, h_queries, (size_t) nq * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        d_queries = reinterpret_cast<const float*>(w + o_q);
    }
    uint8_t* d_qb = reinterpret_cast<uint8_t*>(w + o_qb);
    uint64_t* s1_keys = reinterpret_cast<uint64_t*>(w + o_key);
    HIPCHK(launch_binary_quantize(d_queries, 0, (uint64_t) nq, (uint32_t) dim, (uint32_t) dim, d_qb, (uint32_t) qbytes, ctx->stream));
    bool any_filter = false;
    if (h->h_bm.p) HIPCHK(hipStreamSynchronize(ctx->stream));            // the pinned pointer block of the previous call
    if ((rc = hnsw_bitmaps(h, ctx, filters, nq, any_filter))) return rc;
    HnswQueries qs;
    if ((rc = hnsw_stage_bits(h, ctx, d_qb, nq, qs))) return rc;
    const Outputs s1{reinterpret_cast<int64_t*>(w + o_blk), reinterpret_cast<int32_t*>(w + o_doc), nullptr,
                     reinterpret_cast<float*>(w + o_dist), reinterpret_cast<int32_t*>(w + o_cnt), s1_keys};
    if ((rc = hnsw_launch(h, ctx, qs, nq, shortlist, ef, VSR_METRIC_HAMMING, any_filter ? h->d_bm.as<const uint64_t*>() : nullptr,
                          force_global, s1, nullptr, d_status)))
        return rc;
    return quantized_rerank(ctx, src, s1_keys, (uint32_t) bits->row_offset, reinterpret_cast<uint64_t*>(w + o_blk), d_queries, nq, dim, k,
                            shortlist, metric, out);
}

static int hnsw_quantized_check(vsr_corpus* src, vsr_hnsw* h, const void* queries, int nq, int dim, int k, int shortlist, int ef,
                                int metric, const vsr_filter* const* filters, const char* who)
{
    if (!h) return fail(VSR_ERR_INVALID, "%s: index is NULL", who);
    int rc = check_quantized_args(nullptr, src, h->corpus, queries, nq, dim, k, shortlist, metric, filters, who);
    if (rc) return rc;
    if (h->format != RowFormat::BIT || h->bit_metric != VSR_METRIC_HAMMING)
        return fail(VSR_ERR_INVALID, "%s: the index was made for %s: the shortlist of binary_quantize needs a Hamming index", who,
                    h->format == RowFormat::BIT ? bit_metric_name(h->bit_metric) : "a corpus that is not a bit corpus");
    if (ef < 1 || ef > 5000) return fail(VSR_ERR_INVALID, "%s: ef_search must be between 1 and 5000 (got %d)", who, ef);
    return VSR_OK;
}

extern "C" int vsr_hnsw_search_quantized_device(vsr_corpus* src, vsr_hnsw* h, const float* d_queries, int nq, int dim, int k,
                                                int shortlist, int ef, int metric, const vsr_filter* const* filters, int64_t* d_blk,
                                                int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    const char* who = "vsr_hnsw_search_quantized_device";
    int rc = hnsw_quantized_check(src, h, d_queries, nq, dim, k, shortlist, ef, metric, filters, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    HIPCHK(hipSetDevice(h->corpus->ctx->device));
    return hnsw_quantized_impl(src, h, nullptr, d_queries, nq, dim, k, shortlist, ef, metric, filters, false,
                               {d_blk, d_doc, d_row, d_dist, d_cnt, d_keys}, nullptr);
}

extern "C" int vsr_hnsw_search_quantized(vsr_corpus* src, vsr_hnsw* h, const float* queries, int nq, int dim, int k, int shortlist,
                                         int ef, int metric, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                                         int64_t* out_row, float* out_dist, int32_t* out_cnt)
{
    const char* who = "vsr_hnsw_search_quantized";
    int rc = hnsw_quantized_check(src, h, queries, nq, dim, k, shortlist, ef, metric, filters, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    if (src->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;   // `$1::halfvec`, as vsr_search refuses it
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const ResultBlock rb(nq, k, false);                     // results and stage 1's status words: one packed copy back, one wait
    if ((rc = h->d_out.reserve(rb.total))) return rc;
    if ((rc = h->h_out.reserve(rb.total))) return rc;
    char* d = h->d_out.as<char>();
    char* hh = h->h_out.as<char>();
    // tier 1: a query's LDS visited table overflowed (big graphs only): the call again with the global bitmap
    for (int tier = 0; tier < 2; ++tier) {
        if ((rc = hnsw_quantized_impl(src, h, queries, nullptr, nq, dim, k, shortlist, ef, metric, filters, tier == 1, rb.arrays(d),
                                      rb.column<int32_t>(d, rb.o_status))))
            return rc;
        HIPCHK(hipMemcpyAsync(hh, d, rb.total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (rb.flagged(hh, (size_t) nq).empty()) break;
    }
    rb.copy_out_all(hh, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    return VSR_OK;
}

// ---- forest search: the partition graphs of a query in one search launch, merged on the GPU (vsr_hnsw_forest_search.h) ----
struct vsr_hnsw_forest {
    // The forest's own index object: no graph, registered with the corpus like any index.  It carries what the single-index entry
    // points keep per index -- the row format and opclass the argument checks read, the shared m, the largest n_elem (the LDS plan), the
    // forest's predicate-aware flag, the filter bitmaps, staged queries, visited words and result blocks of a call.  nullptr: an empty forest
    vsr_hnsw* host = nullptr;
    std::vector<vsr_hnsw*> indexes;
    DevBuf d_graphs;                                 // one HnswGraphDesc per index
    DevBuf d_tasks;                                  // a call's task table, task keys, counts, status words and visited counts
    PinBuf h_tasks;
};

extern "C" int vsr_hnsw_forest_free(vsr_hnsw_forest* f)
{
    if (!f) return VSR_OK;
    if (f->host) {
        (void) hipSetDevice(f->host->corpus->ctx->device);
        (void) vsr_hnsw_free(f->host);               // waits for the stream
    }
    delete f;
    return VSR_OK;
}

extern "C" int vsr_hnsw_forest_open(vsr_hnsw* const* indexes, int n_indexes, vsr_hnsw_forest** out)
{
    const char* who = "vsr_hnsw_forest_open";
    if (!out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (n_indexes < 0 || (n_indexes > 0 && !indexes)) return fail(VSR_ERR_INVALID, "%s: %d indexes at %p", who, n_indexes, (const void*) indexes);
    std::unique_ptr<vsr_hnsw_forest, int (*)(vsr_hnsw_forest*)> f(new vsr_hnsw_forest, vsr_hnsw_forest_free);
    if (n_indexes == 0) {
        *out = f.release();
        return VSR_OK;
    }
    for (int g = 0; g < n_indexes; ++g) {
        const vsr_hnsw* h = indexes[g];
        const vsr_hnsw* h0 = indexes[0];
        if (!h) return fail(VSR_ERR_INVALID, "%s: index %d is NULL", who, g);
        if (h->format == RowFormat::SPARSE)
            return fail(VSR_ERR_UNSUPPORTED, "%s: index %d is over a sparsevec corpus: a forest is searched over vector, halfvec or bit rows", who, g);
        if (h->format != h0->format)
            return fail(VSR_ERR_INVALID, "%s: index %d is over %s rows, index 0 over %s rows", who, g, format_name(h->format), format_name(h0->format));
        if (h->corpus != h0->corpus) return fail(VSR_ERR_INVALID, "%s: index %d is over another corpus than index 0", who, g);
        if (h->m != h0->m) return fail(VSR_ERR_INVALID, "%s: index %d has m = %d, index 0 has m = %d", who, g, h->m, h0->m);
        if (h->format == RowFormat::BIT && h->bit_metric != h0->bit_metric)
            return fail(VSR_ERR_INVALID, "%s: index %d was made for %s, index 0 for %s", who, g, bit_metric_name(h->bit_metric),
                        bit_metric_name(h0->bit_metric));
    }
    vsr_corpus* c = indexes[0]->corpus;
    HIPCHK(hipSetDevice(c->ctx->device));
    HnswOwner host = hnsw_new_index(c, indexes[0]->format, indexes[0]->bit_metric, indexes[0]->m);
    std::vector<HnswGraphDesc> desc((size_t) n_indexes);
    for (int g = 0; g < n_indexes; ++g) {
        const vsr_hnsw* h = indexes[g];
        HnswGraphDesc& d = desc[(size_t) g];
        d.n_elem = (uint32_t) h->n_elem;
        d.entry = h->entry;
        d.entry_level = h->entry_level;
        d.max_level = (uint32_t) h->max_level;
        d.elem_row = h->d_elem_row;
        d.nbr0 = h->d_nbr0;
        d.up_slot = h->d_up_slot;
        d.up_nbr = h->d_up_nbr;
        d.level = h->d_level;
        d.tid_count = h->d_tid_count;
        d.tids = h->d_tids;
        host->n_elem = std::max(host->n_elem, h->n_elem);
    }
    int rc = f->d_graphs.reserve(desc.size() * sizeof(HnswGraphDesc));
    if (rc) return rc;
    HIPCHK(hipMemcpy(f->d_graphs.p, desc.data(), desc.size() * sizeof(HnswGraphDesc), hipMemcpyHostToDevice));
    f->indexes.assign(indexes, indexes + n_indexes);
    f->host = hnsw_register(std::move(host));
    *out = f.release();
    return VSR_OK;
}

extern "C" int vsr_hnsw_forest_set_predicate_aware(vsr_hnsw_forest* f, int on)
{
    if (!f) return fail(VSR_ERR_INVALID, "vsr_hnsw_forest_set_predicate_aware: forest is NULL");
    if (f->host) f->host->predicate_aware = on ? 1 : 0;
    return VSR_OK;
}

// where a call's task arrays live in d_tasks; h_tasks mirrors the sections in front of o_keys (the upload, and a re-run's lists)
struct ForestLayout {
    size_t o_off, o_tq, o_tg, upload, o_redo, sec, o_keys, o_cnt, o_status, o_vis, total;
    ForestLayout(int nq, size_t n_tasks, int k)
    {
        o_off = 0;
        o_tq = align_up(((size_t) nq + 1) * 8, 256);
        o_tg = align_up(o_tq + n_tasks * 4, 256);
        upload = align_up(o_tg + n_tasks * 4, 256);
        o_redo = upload;                                                     // a re-run's [query | graph | slot], `sec` bytes each
        sec = align_up(n_tasks * 4, 256);
        o_keys = o_redo + 3 * sec;
        o_cnt = align_up(o_keys + n_tasks * (size_t) k * 8, 256);
        o_status = align_up(o_cnt + n_tasks * 4, 256);
        o_vis = align_up(o_status + n_tasks * 4, 256);                       // (status and visited: one copy back)
        total = align_up(o_vis + n_tasks * 8, 256);
    }
};

// VSR_HNSW_FOREST_MERGE_KEYS (read at every call)
static int forest_merge_keys(const char* who, int k, uint32_t* cap)
{
    *cap = hnsw_merge_keys_default((uint32_t) k);
    const char* env = getenv("VSR_HNSW_FOREST_MERGE_KEYS");
    if (!env) return VSR_OK;
    char* end = nullptr;
    const unsigned long long v = strtoull(env, &end, 10);
    if (!*env || *end || env[0] == '-' || !hnsw_merge_keys_ok((uint32_t) k, v))
        return fail(VSR_ERR_INVALID, "%s: VSR_HNSW_FOREST_MERGE_KEYS must be a power of two from %u (the smallest >= 2 k) to %u (got \"%s\")", who,
                    hnsw_merge_keys_min((uint32_t) k), HFS_MERGE_KEYS_MAX, env);
    *cap = (uint32_t) v;
    return VSR_OK;
}

// the search launch over n tasks listed at d_tq / d_tg (d_slot: a re-run's output slots, else nullptr)
static int forest_search_launch(vsr_hnsw_forest* f, vsr_ctx* ctx, const HnswQueries& qs, bool any_filter, int n, const int32_t* d_tq,
                                const int32_t* d_tg, const int32_t* d_slot, bool force_global, int k, int ef, int metric, const ForestLayout& lay,
                                int64_t* d_visited)
{
    if (n == 0) return VSR_OK;
    vsr_hnsw* h = f->host;
    char* w = f->d_tasks.as<char>();
    HnswParams p{};
    int rc = hnsw_params(h, ctx, qs, n, k, ef, metric, any_filter ? h->d_bm.as<const uint64_t*>() : nullptr, force_global, nullptr, p);
    if (rc) return rc;
    p.key_row_offset = 0;
    p.out_keys = reinterpret_cast<uint64_t*>(w + lay.o_keys);
    p.out_count = reinterpret_cast<int32_t*>(w + lay.o_cnt);
    p.out_status = reinterpret_cast<int32_t*>(w + lay.o_status);
    p.out_visited = d_visited;
    p.err = ctx->err_word();
    HnswForestTasks ft{};
    ft.graphs = f->d_graphs.as<const HnswGraphDesc>();
    ft.task_query = d_tq;
    ft.task_graph = d_tg;
    ft.task_slot = d_slot;
    HIPCHK(launch_hnsw_forest(h->format, p, ft, ctx->stream));
    h->last_mode = p.vis_mode;
    return VSR_OK;
}

static int forest_merge_launch(vsr_hnsw_forest* f, vsr_ctx* ctx, int nq, int k, uint32_t cap, int metric, const ForestLayout& lay, const Outputs& out)
{
    const vsr_hnsw* h = f->host;
    char* w = f->d_tasks.as<char>();
    HnswForestMergeParams mp{};
    mp.q_off = reinterpret_cast<const int64_t*>(w + lay.o_off);
    mp.task_keys = reinterpret_cast<const uint64_t*>(w + lay.o_keys);
    mp.task_status = reinterpret_cast<const int32_t*>(w + lay.o_status);
    mp.nq = (uint32_t) nq;
    mp.k = (uint32_t) k;
    mp.cap = cap;
    mp.rows = h->format == RowFormat::BIT ? ROWS_BIT : h->format == RowFormat::HALF ? ROWS_HALF : ROWS_F32;
    mp.metric = metric;
    set_results(mp, h->corpus, out);
    HIPCHK(launch_hnsw_forest_merge(mp, ctx->stream));
    return VSR_OK;
}

// What every forest entry point checks; *n_tasks: the call's tasks, *cap: the merge's capacity
static int forest_check(const HnswEntry& en, vsr_hnsw_forest* f, const void* queries, int nq, int dim, int k, int ef, int metric, const int64_t* q_off,
                        const int32_t* q_graph, const vsr_filter* const* filters, size_t* n_tasks, uint32_t* cap)
{
    if (!f) return fail(VSR_ERR_INVALID, "%s: forest is NULL", en.who);
    int rc;
    if (f->host) {
        if ((rc = hnsw_check(f->host, queries, nq, dim, k, ef, metric, filters, en.who, en.queries))) return rc;
    } else if (nq < 0 || k < 1 || k > VSR_MAX_K)
        return fail(VSR_ERR_INVALID, "%s: nq = %d, k = %d", en.who, nq, k);
    char msg[160];
    if (!hnsw_forest_check_tasks(nq, q_off, q_graph, (int) f->indexes.size(), msg, sizeof msg)) return fail(VSR_ERR_INVALID, "%s: %s", en.who, msg);
    *n_tasks = (size_t) q_off[nq];
    return forest_merge_keys(en.who, k, cap);
}

// queries resident at d_q: the task table's upload, the filters' bitmaps, (bit: the staging launch,) the search launch, the merge launch
static int forest_enqueue(const HnswEntry& en, vsr_hnsw_forest* f, const void* d_q, int nq, int dim, int k, int ef, int metric, uint32_t cap,
                          const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, const ForestLayout& lay,
                          const Outputs& out, int64_t* d_visited, HnswQueries& qs, bool& any_filter)
{
    vsr_hnsw* h = f->host;
    vsr_ctx* ctx = h->corpus->ctx;
    const size_t n_tasks = (size_t) q_off[nq];
    int rc;
    if (h->h_bm.p || f->h_tasks.p) HIPCHK(hipStreamSynchronize(ctx->stream));  // the pinned blocks of the previous call
    if ((rc = f->d_tasks.reserve(lay.total))) return rc;
    if ((rc = f->h_tasks.reserve(lay.o_keys))) return rc;
    char* hp = f->h_tasks.as<char>();
    char* w = f->d_tasks.as<char>();
    memcpy(hp + lay.o_off, q_off, ((size_t) nq + 1) * 8);
    int32_t* tq = reinterpret_cast<int32_t*>(hp + lay.o_tq);
    for (int i = 0; i < nq; ++i)
        for (int64_t t = q_off[i]; t < q_off[i + 1]; ++t) tq[t] = i;
    if (n_tasks) memcpy(hp + lay.o_tg, q_graph, n_tasks * 4);
    HIPCHK(hipMemcpyAsync(w, hp, lay.upload, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = hnsw_bitmaps(h, ctx, filters, nq, any_filter))) return rc;
    if ((rc = en.resident(h, ctx, d_q, nq, dim, qs))) return rc;               // (bit: every QUERY staged once)
    if ((rc = forest_search_launch(f, ctx, qs, any_filter, (int) n_tasks, reinterpret_cast<const int32_t*>(w + lay.o_tq),
                                   reinterpret_cast<const int32_t*>(w + lay.o_tg), nullptr, false, k, ef, metric, lay, d_visited)))
        return rc;
    return forest_merge_launch(f, ctx, nq, k, cap, metric, lay, out);
}

// vsr_hnsw_forest_search_device / _bit_device: no synchronisation beyond the pinned blocks' reuse
static int forest_search_device(const HnswEntry& en, vsr_hnsw_forest* f, const void* d_queries, int nq, int dim, int k, int ef, int metric,
                                const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc,
                                int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    size_t n_tasks = 0;
    uint32_t cap = 0;
    int rc = forest_check(en, f, d_queries, nq, dim, k, ef, metric, q_off, q_graph, filters, &n_tasks, &cap);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    if (!f->host) return fail(VSR_ERR_INVALID, "%s: an empty forest has no corpus, and so no stream to enqueue on (the host form answers)", en.who);
    HIPCHK(hipSetDevice(f->host->corpus->ctx->device));
    const ForestLayout lay(nq, n_tasks, k);
    HnswQueries qs;
    bool any_filter = false;
    return forest_enqueue(en, f, d_queries, nq, dim, k, ef, metric, cap, q_off, q_graph, filters, lay, {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr},
                          d_visited, qs, any_filter);
}

// vsr_hnsw_forest_search / _bit: the device form over an upload of the queries, one copy back; the tasks whose LDS visited table
// overflowed are run again with the global bitmap into their own slots, and every query is merged again
static int forest_search_host(const HnswEntry& en, vsr_hnsw_forest* f, const void* queries, int nq, int dim, int k, int ef, int metric,
                              const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                              int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    size_t n_tasks = 0;
    uint32_t cap = 0;
    int rc = forest_check(en, f, queries, nq, dim, k, ef, metric, q_off, q_graph, filters, &n_tasks, &cap);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", en.who);
    if (!f->host) {                                                          // an empty forest: no query has a task
        for (size_t o = 0; o < (size_t) nq * k; ++o) {
            out_blk[o] = -1;
            if (out_doc) out_doc[o] = -1;
            if (out_row) out_row[o] = -1;
            out_dist[o] = INFINITY;
        }
        std::fill(out_cnt, out_cnt + nq, 0);
        return VSR_OK;
    }
    vsr_hnsw* h = f->host;
    if (h->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;
    vsr_ctx* ctx = h->corpus->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const ForestLayout lay(nq, n_tasks, k);
    const ResultBlock rb(nq, k, false);
    const size_t qbytes = en.bytes(dim), tail = lay.total - lay.o_status;     // [status | visited] of the tasks behind the results
    if ((rc = h->d_q.reserve((size_t) nq * qbytes))) return rc;
    if ((rc = h->d_out.reserve(rb.total))) return rc;
    if ((rc = h->h_out.reserve(rb.total + tail))) return rc;
    char* d = h->d_out.as<char>();
    char* hh = h->h_out.as<char>();
    HIPCHK(hipMemcpyAsync(h->d_q.p, queries, (size_t) nq * qbytes, hipMemcpyHostToDevice, ctx->stream));
    HnswQueries qs;
    bool any_filter = false;
    if ((rc = f->d_tasks.reserve(lay.total))) return rc;                       // (forest_enqueue's own reservation then keeps the block)
    char* w = f->d_tasks.as<char>();
    int64_t* d_visited = reinterpret_cast<int64_t*>(w + lay.o_vis);
    if ((rc = forest_enqueue(en, f, h->d_q.p, nq, dim, k, ef, metric, cap, q_off, q_graph, filters, lay, rb.arrays(d), d_visited, qs, any_filter)))
        return rc;
    const auto fetch = [&]() -> int {
        HIPCHK(hipMemcpyAsync(hh, d, rb.total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(hh + rb.total, w + lay.o_status, tail, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    };
    if ((rc = fetch())) return rc;
    const int32_t* status = reinterpret_cast<const int32_t*>(hh + rb.total);
    std::vector<int32_t> redo;
    for (size_t t = 0; t < n_tasks; ++t)
        if (status[t]) redo.push_back((int32_t) t);
    if (!redo.empty()) {
        const size_t nr = redo.size(), sec4 = lay.sec / 4;
        char* hp = f->h_tasks.as<char>();
        const int32_t* tq = reinterpret_cast<const int32_t*>(hp + lay.o_tq);
        int32_t* hr = reinterpret_cast<int32_t*>(hp + lay.o_redo);
        for (size_t j = 0; j < nr; ++j) {
            hr[j] = tq[redo[j]];
            hr[sec4 + j] = q_graph[redo[j]];
            hr[2 * sec4 + j] = redo[j];
        }
        HIPCHK(hipMemcpyAsync(w + lay.o_redo, hr, 3 * lay.sec, hipMemcpyHostToDevice, ctx->stream));
        const int32_t* dr = reinterpret_cast<const int32_t*>(w + lay.o_redo);
        if ((rc = forest_search_launch(f, ctx, qs, any_filter, (int) nr, dr, dr + sec4, dr + 2 * sec4, true, k, ef, metric, lay, d_visited)))
            return rc;
        // q_off went with the first upload and is still in place
        if ((rc = forest_merge_launch(f, ctx, nq, k, cap, metric, lay, rb.arrays(d)))) return rc;
        if ((rc = fetch())) return rc;
    }
    rb.copy_out_all(hh, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    if (out_visited && n_tasks) memcpy(out_visited, hh + rb.total + (lay.o_vis - lay.o_status), n_tasks * 8);
    return VSR_OK;
}

extern "C" int vsr_hnsw_forest_search(vsr_hnsw_forest* f, const float* queries, int nq, int dim, int k, int ef, int metric, const int64_t* q_off,
                                      const int32_t* q_graph, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                                      int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    return forest_search_host({"vsr_hnsw_forest_search", RowFormat::F32}, f, queries, nq, dim, k, ef, metric, q_off, q_graph, filters, out_blk,
                              out_doc, out_row, out_dist, out_cnt, out_visited);
}

extern "C" int vsr_hnsw_forest_search_bit(vsr_hnsw_forest* f, const uint8_t* queries, int nq, int dim, int k, int ef, int metric,
                                          const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, int64_t* out_blk,
                                          int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int64_t* out_visited)
{
    return forest_search_host({"vsr_hnsw_forest_search_bit", RowFormat::BIT}, f, queries, nq, dim, k, ef, metric, q_off, q_graph, filters, out_blk,
                              out_doc, out_row, out_dist, out_cnt, out_visited);
}

extern "C" int vsr_hnsw_forest_search_device(vsr_hnsw_forest* f, const float* d_queries, int nq, int dim, int k, int ef, int metric,
                                             const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, int64_t* d_blk,
                                             int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    return forest_search_device({"vsr_hnsw_forest_search_device", RowFormat::F32}, f, d_queries, nq, dim, k, ef, metric, q_off, q_graph, filters,
                                d_blk, d_doc, d_row, d_dist, d_cnt, d_visited);
}

extern "C" int vsr_hnsw_forest_search_bit_device(vsr_hnsw_forest* f, const uint8_t* d_queries, int nq, int dim, int k, int ef, int metric,
                                                 const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters, int64_t* d_blk,
                                                 int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, int64_t* d_visited)
{
    return forest_search_device({"vsr_hnsw_forest_search_bit_device", RowFormat::BIT}, f, d_queries, nq, dim, k, ef, metric, q_off, q_graph, filters,
                                d_blk, d_doc, d_row, d_dist, d_cnt, d_visited);
}
