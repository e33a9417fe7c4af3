// vsr_hnsw_rt.hip — K4 / K4b / K4h: HNSW graph load / build / search entry points, over fp32 corpora (vsr_hnsw_*), bit corpora
// (vsr_hnsw_*_bit, vsr_hnsw_search_quantized*) and halfvec corpora (vsr_hnsw_load_half / vsr_hnsw_build_half, searched by the
// float entry points), and the forest entry points that search many indexes of one corpus as a set (vsr_hnsw_forest_*).  The only
// unit that compiles vsr_hnsw.h's and vsr_hnsw_forest_search.h's kernels.
#include "vsr_runtime.h"
#include "vsr_hnsw.h"
#include "vsr_hnsw_build.h"
#include "vsr_hnsw_forest.h"
#include "vsr_hnsw_forest_search.h"
#include "vsr_shortlist.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

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
};

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

static int upload_i32(int32_t** d, const int32_t* src, size_t count)          // a graph array into device memory of its own
{
    HIPCHK(hipMalloc(d, std::max<size_t>(4, count * sizeof(int32_t))));
    if (count) HIPCHK(hipMemcpy(*d, src, count * sizeof(int32_t), hipMemcpyHostToDevice));
    return VSR_OK;
}

// what a bit entry point asks of its corpus and opclass (who: the entry point)
static int hnsw_bit_opclass(const vsr_corpus* c, int metric, const char* who)
{
    if (c->format != RowFormat::BIT) return fail(VSR_ERR_INVALID, "%s: the corpus is not a bit corpus", who);
    if (metric != VSR_METRIC_HAMMING && metric != VSR_METRIC_JACCARD)
        return fail(VSR_ERR_INVALID, "%s: metric %d is not an operator class of bit (4: bit_hamming_ops, 5: bit_jaccard_ops)", who, metric);
    return VSR_OK;
}

// what a halfvec entry point asks of its corpus (who: the entry point)
static int hnsw_half_opclass(const vsr_corpus* c, const char* who)
{
    if (c->format != RowFormat::HALF) return fail(VSR_ERR_INVALID, "%s: the corpus is not a halfvec corpus", who);
    if (c->dim > 4000)           /* HNSW_MAX_DIM * 2, hnswutils.c:1390 */
        return fail(VSR_ERR_UNSUPPORTED, "%s: column cannot have more than 4000 dimensions for hnsw index", who);
    return VSR_OK;
}
static const char* const HNSW_HALF_ENTRY =
    "the graph of a halfvec corpus is loaded with vsr_hnsw_load_half and built with vsr_hnsw_build_half (the halfvec_l2_ops / halfvec_ip_ops / "
    "halfvec_cosine_ops opclasses)";

// what a sparsevec entry point asks of its corpus (who: the entry point): checkValue of the sparsevec opclasses, hnswutils.c:1352-1361
static int hnsw_sparse_opclass(const vsr_corpus* c, const char* who)
{
    if (c->format != RowFormat::SPARSE) return fail(VSR_ERR_INVALID, "%s: the corpus is not a sparse corpus", who);
    if (c->sp_max_nnz > (uint32_t) HNSW_SPARSE_MAX_NNZ)
        return fail(VSR_ERR_UNSUPPORTED, "sparsevec cannot have more than %d non-zero elements for hnsw index", HNSW_SPARSE_MAX_NNZ);
    return VSR_OK;
}

// vsr_hnsw_load (expect = F32), vsr_hnsw_load_half (HALF), vsr_hnsw_load_bit (BIT; bit_metric: the opclass) and
// vsr_hnsw_load_sparse (SPARSE): `expect` is the corpus format the entry point is for
static int hnsw_load(vsr_corpus* c, RowFormat expect, int bit_metric, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                     const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                     int32_t n_upper, int32_t max_level, vsr_hnsw** out, const char* who)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (c->base) return fail(VSR_ERR_INVALID, "%s: the corpus is a view", who);
    if (expect == RowFormat::BIT) {
        int rc = hnsw_bit_opclass(c, bit_metric, who);
        if (rc) return rc;
    }
    if (expect == RowFormat::HALF) {
        int rc = hnsw_half_opclass(c, who);
        if (rc) return rc;
    }
    if (expect == RowFormat::SPARSE) {
        int rc = hnsw_sparse_opclass(c, who);
        if (rc) return rc;
    }
    if (c->format == RowFormat::HALF && expect != RowFormat::HALF) return fail(VSR_ERR_UNSUPPORTED, "%s: %s", who, HNSW_HALF_ENTRY);
    // (stale since K4s: the graph of a sparse corpus is loaded with vsr_hnsw_load_sparse; the text is pinned by tests)
    if (c->format == RowFormat::SPARSE && expect != RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)", who);
    if (c->format == RowFormat::BIT && expect != RowFormat::BIT)
        return fail(VSR_ERR_UNSUPPORTED, "%s: the graph of a bit corpus is loaded with vsr_hnsw_load_bit (the bit_hamming_ops / bit_jaccard_ops opclasses)", who);
    if (m < 2 || m > 100)        /* reloption m: 2 .. HNSW_MAX_M (hnsw.h:36-40) */
        return fail(VSR_ERR_UNSUPPORTED, "%s: m must be between 2 and 100 (got %d)", who, m);
    if (n_elem < 0 || (n_elem > 0 && (!level || !nbr0 || !tid_count || !tids || !up_slot)) || max_level < 1 || n_upper < 0 ||
        (n_upper > 0 && !up_nbr) || entry >= n_elem)
        return fail(VSR_ERR_INVALID, "%s: bad graph arrays", who);
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<vsr_hnsw> h(new vsr_hnsw());
    h->corpus = c;
    h->format = expect;
    h->bit_metric = bit_metric;
    h->n_elem = n_elem;
    h->entry = n_elem > 0 ? entry : -1;
    h->m = m;
    h->max_level = max_level;
    h->n_upper = n_upper;
    // heap TIDs arrive as caller row indices; the kernels work on internal rows
    std::vector<int32_t> inv((size_t) std::max<int64_t>(c->n, 1), -1);
    for (int64_t r = 0; r < c->n; ++r) inv[(size_t) c->h_orig[(size_t) r]] = (int32_t) r;
    std::vector<int32_t> itids((size_t) std::max(n_elem, 1) * 10, -1), erow((size_t) std::max(n_elem, 1), 0);
    for (int32_t e = 0; e < n_elem; ++e) {
        if (tid_count[e] < 1 || tid_count[e] > 10 || level[e] < 0 || level[e] > max_level)
            return fail(VSR_ERR_INVALID, "%s: element %d has %d heap TIDs / level %d", who, e, tid_count[e], level[e]);
        for (int t = 0; t < tid_count[e]; ++t) {
            const int64_t row = tids[(size_t) e * 10 + t];
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
        (rc = up(&h->d_tids, itids.data(), (size_t) n_elem * 10))) {
        vsr_hnsw_free(h.release());
        return rc;
    }
    c->hnsw_indexes.push_back(h.get());
    *out = h.release();
    return VSR_OK;
}

extern "C" int vsr_hnsw_load(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                             const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                             int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    return hnsw_load(c, RowFormat::F32, 0, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, out, "vsr_hnsw_load");
}

extern "C" int vsr_hnsw_load_bit(vsr_corpus* c, int metric, int m, int32_t n_elem, int32_t entry, const int32_t* level,
                                 const int32_t* nbr0, const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot,
                                 const int32_t* up_nbr, int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "vsr_hnsw_load_bit: NULL argument");
    *out = nullptr;
    int rc = hnsw_bit_opclass(c, metric, "vsr_hnsw_load_bit");
    if (rc) return rc;
    return hnsw_load(c, RowFormat::BIT, metric, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, out, "vsr_hnsw_load_bit");
}

extern "C" int vsr_hnsw_load_half(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                                  const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                                  int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    return hnsw_load(c, RowFormat::HALF, 0, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, out, "vsr_hnsw_load_half");
}

extern "C" int vsr_hnsw_load_sparse(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                                    const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                                    int32_t n_upper, int32_t max_level, vsr_hnsw** out)
{
    return hnsw_load(c, RowFormat::SPARSE, 0, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, out, "vsr_hnsw_load_sparse");
}

// per-wave LDS of the build's search kernel (hnsw_build_search_kernel's carve-up) with `slots` visited-table entries and, a sparse
// build, the wave's left-hand table of sp_slots (index, value) slots behind them
static size_t hnsw_build_lds_per_wave(uint32_t caps, uint32_t slots, uint32_t sp_slots = 0)
{
    return (((size_t) caps * 8 + ((caps + 15) & ~15u) + (size_t) HB_NBR * 12 + (size_t) caps * 4 + (size_t) slots * 4 + 15) & ~(size_t) 15) +
           (size_t) sp_slots * 8;
}
// slots of a sparse build's left-hand tables: sized once from the corpus's largest row (<= 1000 non-zeros: <= 2048 slots, 16 KB)
static uint32_t hnsw_build_sparse_slots(const vsr_corpus* c, RowFormat expect)
{
    return c && expect == RowFormat::SPARSE && c->format == RowFormat::SPARSE ? sparse_slots_for_nnz(c->sp_max_nnz) : 0u;
}

// CREATE INDEX ... USING hnsw on the GPU (vsr_hnsw_build.hip): batched insertion over the corpus's rows, levels from a seeded
// xorshift64* stream drawn once per row.  flags = 0: element e = internal row e.  VSR_HNSW_BUILD_MERGE_DUPLICATES: the
// elements come from vsr_hnsw_dedup.hip's table.  Returns a loaded index, as vsr_hnsw_load would from the same graph.
// expect: the corpus format the entry point is for -- BIT (vsr_hnsw_build_bit; metric is the opclass), HALF (vsr_hnsw_build_half) or
// F32; the kernels take that row format.
// One attempt with a visited table of *slots entries (0: the default for m and ef_construction, written back).  *guard: the
// build's guard-word bits (HB_ERR_VISITED / HB_ERR_RECORDS / HB_ERR_CANDIDATES) when a kernel set one (caps: entries of the sorted
// candidate array, at least ef_construction + 2 m); the partial index is then freed, the bits
// are cleared from the session's word, *out stays NULL and the return value is VSR_OK: hnsw_build decides what follows.
//
// prior (vsr_hnsw_extend; nullptr: a build): the graph the batches are inserted into.  A build is the extension of nothing: no
// prior elements, no draws skipped, the schedule from done = 0, distances all zero.  Everything an attempt changes is a device copy,
// so a restart begins again from the caller's arrays.
struct HnswPrior {
    int32_t n_elem = 0, entry = -1, n_upper = 0, max_level = 1;
    const int32_t *level = nullptr, *nbr0 = nullptr, *tid_count = nullptr, *up_slot = nullptr, *up_nbr = nullptr;   // the caller's arrays, checked
    std::vector<int32_t> itids;              // [n_elem][10] heap TIDs as internal rows, -1 padded
    std::vector<int32_t> elem_row;           // [n_elem + n_new] element -> internal row: first TIDs, then the rows no TID names, ascending
    std::vector<int32_t> up_owner;           // [n_upper] upper slot -> its element, -1: no element names the slot
    int64_t n0 = 0, n_new = 0;               // rows the prior graph covers (level draws to skip) / rows to insert
    bool identity = true;                    // element e is internal row e throughout: the direct kernels serve
};

// The build's levels: level = floor(-ln(u) * ml), ml = 1 / ln(m) (hnswutils.c:243), capped like HnswGetMaxLevel (hnsw.h:89), u from a
// seeded xorshift64* stream (the serial CPU restatement draws the same stream).  One draw per inserted row
struct HnswLevelStream {
    uint64_t rs;
    double ml;
    int cap;
    HnswLevelStream(uint64_t seed, int m) : rs(seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL), ml(1.0 / std::log((double) m))
    {
        cap = std::min((8192 - 24 - 8 - 4 - 4) / 6 / m - 2, 255);
        if (!rs) rs = 1;
        (void) next();
    }
    uint64_t next()
    {
        uint64_t x = rs;
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        rs = x;
        return x * 0x2545F4914F6CDD1DULL;
    }
    int32_t level()
    {
        const double u = (double) (next() >> 11) * (1.0 / 9007199254740992.0);
        return std::min((int) (-std::log(u) * ml), cap);
    }
};

// what every build entry point asks of its corpus and arguments, in the order and words the build has always used
static int hnsw_build_check(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint32_t flags, vsr_hnsw** out, const char* who)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (expect == RowFormat::BIT) {
        int rc = hnsw_bit_opclass(c, metric, who);
        if (rc) return rc;
    }
    if (expect == RowFormat::HALF) {
        int rc = hnsw_half_opclass(c, who);
        if (rc) return rc;
    }
    if (expect == RowFormat::SPARSE) {
        int rc = hnsw_sparse_opclass(c, who);
        if (rc) return rc;
    }
    if (flags & ~(uint32_t) VSR_HNSW_BUILD_MERGE_DUPLICATES) return fail(VSR_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (expect == RowFormat::SPARSE && (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES))
        return fail(VSR_ERR_UNSUPPORTED, "%s: VSR_HNSW_BUILD_MERGE_DUPLICATES is not supported over a sparse corpus (the pre-pass compares fixed-stride rows)", who);
    if (c->base) return fail(VSR_ERR_INVALID, "%s: the corpus is a view", who);
    if (c->format == RowFormat::HALF && expect != RowFormat::HALF) return fail(VSR_ERR_UNSUPPORTED, "%s: %s", who, HNSW_HALF_ENTRY);
    // (stale since K4s: the graph of a sparse corpus is built with vsr_hnsw_build_sparse; the text is pinned by tests)
    if (c->format == RowFormat::SPARSE && expect != RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)", who);
    if (c->format == RowFormat::BIT && expect != RowFormat::BIT)
        return fail(VSR_ERR_UNSUPPORTED, "%s: the graph of a bit corpus is built with vsr_hnsw_build_bit (the bit_hamming_ops / bit_jaccard_ops opclasses)", who);
    if (m < 2 || m > 100) return fail(VSR_ERR_UNSUPPORTED, "%s: m must be between 2 and 100 (got %d)", who, m);
    if (ef_construction < 4 || ef_construction > 1000 || ef_construction < 2 * m)      /* hnsw.c:62-63, hnswbuild.c:677-679 */
        return fail(VSR_ERR_UNSUPPORTED, "%s: ef_construction must be between 4 and 1000 and at least 2 * m (got %d)", who, ef_construction);
    if (expect == RowFormat::SPARSE && (metric < VSR_METRIC_L2 || metric > VSR_METRIC_L1))
        return fail(VSR_ERR_INVALID, "%s: metric %d is not an operator class of sparsevec (0: sparsevec_l2_ops, 1: sparsevec_ip_ops, 2: sparsevec_cosine_ops, 3: sparsevec_l1_ops)", who, metric);
    if (expect != RowFormat::BIT && expect != RowFormat::SPARSE && metric != VSR_METRIC_L2 && metric != VSR_METRIC_IP && metric != VSR_METRIC_COSINE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: L2, inner product and cosine operator classes only", who);
    return VSR_OK;
}

static int hnsw_build_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out,
                           const char* who, uint32_t* slots_io, uint32_t caps, uint32_t* guard, const HnswPrior* prior = nullptr)
{
    {
        const int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, out, who);
        if (rc) return rc;
    }
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (n > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many rows", who);
    const bool merge = !prior && (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES) != 0 && n > 0;
    const int64_t n_prior = prior ? prior->n_elem : 0;                        // elements that are there already
    const int64_t n_new = prior ? prior->n_new : n;                           // rows to insert, one element each unless merging
    if (n_prior + n_new > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);
    const uint32_t row_chunks = format_row_chunks(expect, c->dim);
    std::unique_ptr<vsr_hnsw> h(new vsr_hnsw());
    h->corpus = c;
    h->format = expect;
    h->bit_metric = expect == RowFormat::BIT ? metric : 0;
    h->m = m;
    HnswLevelStream draws(seed, m);
    // per element: the prior graph's levels, then one draw per inserted row (merging: per row, then per element).  The i-th
    // inserted row takes draw n0 + i, so a prefix build extended with the build's seed draws what the one-shot build draws
    std::vector<int32_t> level((size_t) std::max<int64_t>(n_prior + n_new, 1), 0);
    if (n_prior > 0) std::copy(prior->level, prior->level + n_prior, level.begin());
    for (int64_t r = 0; r < (prior ? prior->n0 : 0); ++r) (void) draws.next();
    for (int64_t r = 0; r < n_new; ++r) level[(size_t) (n_prior + r)] = draws.level();
    float *d_dist0 = nullptr, *d_up_dist = nullptr;
    uint64_t *d_key[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr};
    uint32_t* d_cnt = nullptr;
    void* d_tmp = nullptr;
    int32_t *d_row_level = nullptr, *d_up_owner = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};                                    // VSR_HNSW_EXTEND_TIMING: around the edge-distance launch
    auto cleanup = [&]() {
        for (hipEvent_t e : ev)
            if (e) (void) hipEventDestroy(e);
        void* ptrs[] = {d_dist0, d_up_dist, d_key[0], d_key[1], d_val[0], d_val[1], d_cnt, d_tmp, d_row_level, d_up_owner};
        for (void* q : ptrs)
            if (q) (void) hipFree(q);
    };
    auto bail = [&](int rc) {
        cleanup();
        vsr_hnsw_free(h.release());
        return rc;
    };
#define HB_CHK(call)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return bail(fail(VSR_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)));          \
    } while (0)
    int64_t ne = n_prior + n_new;                                             // elements
    if (merge) {
        // development / tests: VSR_HNSW_DEDUP_HASH_BITS=b keeps the low b bits of the row hash (the collision path on a small
        // corpus); VSR_HNSW_DEDUP_TIMING=1 prints the pre-pass's device-event times to stderr.  Both read at every call
        int hash_bits = 64;
        if (const char* env = getenv("VSR_HNSW_DEDUP_HASH_BITS")) hash_bits = std::max(1, std::min(64, atoi(env)));
        const char* tenv = getenv("VSR_HNSW_DEDUP_TIMING");
        const bool timing = tenv && atoi(tenv) > 0;
        HnswDedupTimes times;
        HnswElemTable t;
        HB_CHK(hipMalloc(&d_row_level, (size_t) n * 4));
        HB_CHK(hipMemcpyAsync(d_row_level, level.data(), (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
        HB_CHK(vsr_hnsw_dedup_elements(c->d_rows, (uint32_t) n, row_chunks, hash_bits, d_row_level, &t, timing ? &times : nullptr, ctx->stream));
        h->d_elem_row = t.elem_row;
        h->d_tid_count = t.tid_count;
        h->d_tids = t.tids;
        h->d_level = t.level;
        ne = t.n_elem;
        HB_CHK(hipMemcpy(level.data(), t.level, (size_t) ne * 4, hipMemcpyDeviceToHost));
        if (timing)
            fprintf(stderr, "vsr_hnsw_dedup: rows=%lld elements=%lld rounds=%d hash_ms=%.4f sort_ms=%.4f resolve_ms=%.4f table_ms=%.4f\n",
                    (long long) n, (long long) ne, times.rounds, times.hash_ms, times.sort_ms, times.resolve_ms, times.table_ms);
    }
    h->n_elem = (int32_t) ne;
    const size_t alloc = (size_t) std::max<int64_t>(ne, 1);
    // prior elements keep their upper slots; new upper elements take the next ones in element order
    std::vector<int32_t> up_slot(alloc, -1);
    int32_t max_level = prior ? prior->max_level : 1, n_upper = prior ? prior->n_upper : 0;
    if (n_prior > 0) std::copy(prior->up_slot, prior->up_slot + n_prior, up_slot.begin());
    for (int64_t e = n_prior; e < ne; ++e)
        if (level[(size_t) e] >= 1) {
            up_slot[(size_t) e] = n_upper++;
            max_level = std::max(max_level, level[(size_t) e]);
        }
    h->max_level = max_level;
    h->n_upper = n_upper;
    const size_t up_words = (size_t) std::max(n_upper, 1) * max_level * m;
    if (!merge) {
        HB_CHK(hipMalloc(&h->d_level, alloc * 4));
        HB_CHK(hipMemcpy(h->d_level, level.data(), alloc * 4, hipMemcpyHostToDevice));
    }
    HB_CHK(hipMalloc(&h->d_up_slot, alloc * 4));
    HB_CHK(hipMalloc(&h->d_nbr0, alloc * 2 * m * 4));
    HB_CHK(hipMalloc(&h->d_up_nbr, up_words * 4));
    HB_CHK(hipMalloc(&d_dist0, alloc * 2 * m * 4));
    HB_CHK(hipMalloc(&d_up_dist, up_words * 4));
    HB_CHK(hipMemcpy(h->d_up_slot, up_slot.data(), alloc * 4, hipMemcpyHostToDevice));
    HB_CHK(hipMemsetAsync(h->d_nbr0, 0xFF, alloc * 2 * m * 4, ctx->stream));
    HB_CHK(hipMemsetAsync(h->d_up_nbr, 0xFF, up_words * 4, ctx->stream));
    HB_CHK(hipMemsetAsync(d_dist0, 0, alloc * 2 * m * 4, ctx->stream));
    HB_CHK(hipMemsetAsync(d_up_dist, 0, up_words * 4, ctx->stream));
    // the prior graph's lists, behind the memsets on the same stream; the upper arrays at this graph's max_level (a new element
    // above the prior top re-strides them).  The host arrays outlive the stream's work: it is synchronised below and in bail
    std::vector<int32_t> prior_up;
    if (n_prior > 0) {
        HB_CHK(hipMemcpyAsync(h->d_nbr0, prior->nbr0, (size_t) n_prior * 2 * m * 4, hipMemcpyHostToDevice, ctx->stream));
        if (prior->n_upper > 0) {
            const int32_t* src = prior->up_nbr;
            if (max_level != prior->max_level) {
                prior_up.assign((size_t) prior->n_upper * max_level * m, -1);
                for (int32_t s = 0; s < prior->n_upper; ++s)
                    std::copy(src + (size_t) s * prior->max_level * m, src + (size_t) (s + 1) * prior->max_level * m,
                              prior_up.begin() + (size_t) s * max_level * m);
                src = prior_up.data();
            }
            HB_CHK(hipMemcpyAsync(h->d_up_nbr, src, (size_t) prior->n_upper * max_level * m * 4, hipMemcpyHostToDevice, ctx->stream));
            HB_CHK(hipMalloc(&d_up_owner, (size_t) prior->n_upper * 4));
            HB_CHK(hipMemcpyAsync(d_up_owner, prior->up_owner.data(), (size_t) prior->n_upper * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (!prior->identity) {
            const int rc = upload_i32(&h->d_elem_row, prior->elem_row.data(), (size_t) ne);
            if (rc) return bail(rc);
        }
    }

    HnswBuildParams bp{};
    bp.rows = c->d_rows;
    bp.stride4 = row_chunks;
    bp.metric = metric == VSR_METRIC_L2 ? M_L2 : M_IP;
    bp.halves = expect == RowFormat::HALF ? 1 : 0;
    if (expect == RowFormat::BIT) {
        bp.bits = 1;
        bp.metric = metric == VSR_METRIC_JACCARD ? M_JACCARD : M_HAMMING;
        bp.row_pop = c->d_norm2;
    }
    if (expect == RowFormat::SPARSE) {
        bp.sparse = 1;
        bp.stride4 = 1;                                       // rows + r names row r (vsr_hnsw_build.h)
        bp.metric = metric == VSR_METRIC_L2 ? M_L2 : metric == VSR_METRIC_L1 ? M_L1 : M_IP;
        bp.sp_off = c->d_sp_off;
        bp.sp_slots = hnsw_build_sparse_slots(c, expect);
        bp.sp_lanes = (uint32_t) c->shape.lpr;
    }
    bp.m = (uint32_t) m;
    bp.efc = (uint32_t) ef_construction;
    bp.max_level = (uint32_t) max_level;
    bp.nbr0 = h->d_nbr0;
    bp.dist0 = d_dist0;
    bp.up_slot = h->d_up_slot;
    bp.up_nbr = h->d_up_nbr;
    bp.up_dist = d_up_dist;
    bp.level = h->d_level;
    bp.elem_row = h->d_elem_row;                                              // the merging build's table / an extension whose elements are
                                                                              // not its rows in order; nullptr: element e is row e
    bp.caps = std::max(caps, (uint32_t) (ef_construction + 2 * m));
    uint32_t slots = *slots_io;
    if (slots == 0) {
        slots = 4096;
        while (slots < (uint32_t) ef_construction * 2u * (uint32_t) m * 2u && slots < 32768u) slots <<= 1;
        *slots_io = slots;
    }
    bp.hash_slots = slots;
    const size_t per = hnsw_build_lds_per_wave(bp.caps, slots, bp.sp_slots);
    if (per > HN_LDS_BUDGET) return bail(fail(VSR_ERR_UNSUPPORTED, "%s: ef_construction = %d with m = %d does not fit the LDS", who, ef_construction, m));
    bp.lds_per_wave = (uint32_t) per;
    bp.wpb = (uint32_t) std::min<size_t>(4, HN_LDS_BUDGET / per);
    bp.err = ctx->err_word();
    // the schedule: a batch never exceeds 1/8 of the graph it is inserted into (its elements do not see each other).  An element
    // of level l emits at most 2m + l * m reverse edges, so a batch's record slots are known here: the sort and the link
    // launch cover those, not the largest batch's
    struct Batch { uint32_t first, count, rec_cap; };
    std::vector<Batch> batches;
    uint32_t rec_cap_max = 1;
    size_t tmp_bytes = 0;
    for (int64_t done = n_prior; done < ne;) {
        const int64_t b = std::max<int64_t>(1, std::min<int64_t>({done / 8, (int64_t) HB_BATCH_MAX, ne - done}));
        uint64_t cap = 0;
        for (int64_t e = done; e < done + b; ++e) cap += (uint64_t) (2 * m + level[(size_t) e] * m);
        if (cap > 0x7FFFFFFFull) return bail(fail(VSR_ERR_UNSUPPORTED, "%s: a batch of %lld elements with m = %d has too many reverse edges", who, (long long) b, m));
        batches.push_back({(uint32_t) done, (uint32_t) b, (uint32_t) cap});
        rec_cap_max = std::max(rec_cap_max, (uint32_t) cap);
        done += b;
    }
    {
        std::vector<uint32_t> caps;                                           // the sort's scratch: the most any batch's size asks for
        for (const Batch& bt : batches) caps.push_back(bt.rec_cap);
        std::sort(caps.begin(), caps.end());
        caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
        for (uint32_t cap : caps) tmp_bytes = std::max(tmp_bytes, vsr_hnsw_build_sort_bytes(cap));
    }
    HB_CHK(hipMalloc(&d_key[0], (size_t) rec_cap_max * 8));
    HB_CHK(hipMalloc(&d_key[1], (size_t) rec_cap_max * 8));
    HB_CHK(hipMalloc(&d_val[0], (size_t) rec_cap_max * 8));
    HB_CHK(hipMalloc(&d_val[1], (size_t) rec_cap_max * 8));
    HB_CHK(hipMalloc(&d_cnt, 64));
    HB_CHK(hipMalloc(&d_tmp, std::max<size_t>(tmp_bytes, 256)));
    bp.rec_count = d_cnt;

    int32_t entry = -1, entry_level = -1;
    const char* tenv = getenv("VSR_HNSW_EXTEND_TIMING");                      // development: 1 prints the edge-distance launch's device time
    const bool edge_timing = n_prior > 0 && tenv && atoi(tenv) > 0;
    if (n_prior > 0) {
        // the one piece of build state the arrays do not carry: the distance of every edge, which the link kernel's re-selection reads
        entry = prior->entry;
        entry_level = level[(size_t) entry];
        if (edge_timing) {
            HB_CHK(hipEventCreate(&ev[0]));
            HB_CHK(hipEventCreate(&ev[1]));
            HB_CHK(hipEventRecord(ev[0], ctx->stream));
        }
        HB_CHK(vsr_hnsw_edge_distances(bp, (uint32_t) n_prior, d_up_owner, (uint32_t) prior->n_upper, ctx->stream));
        if (edge_timing) HB_CHK(hipEventRecord(ev[1], ctx->stream));
    }
    for (const Batch& bt : batches) {
        bp.entry = entry;
        bp.entry_level = entry_level;
        bp.first = bt.first;
        bp.count = bt.count;
        bp.rec_cap = bt.rec_cap;
        bp.rec_key = d_key[0];
        bp.rec_val = d_val[0];
        HB_CHK(vsr_hnsw_build_batch(bp, d_tmp, tmp_bytes, d_key[1], d_val[1], ctx->stream));
        for (uint32_t e = bt.first; e < bt.first + bt.count; ++e)   // HnswUpdateGraphInMemory: a higher element becomes the entry point
            if (entry < 0 || level[(size_t) e] > entry_level) {
                entry = (int32_t) e;
                entry_level = level[(size_t) e];
            }
    }
    HB_CHK(hipStreamSynchronize(ctx->stream));
    if (edge_timing) {
        float ms = 0.0f;
        HB_CHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "vsr_hnsw_extend: prior_elements=%lld new_elements=%lld batches=%zu edge_dist_ms=%.4f\n", (long long) n_prior,
                (long long) (ne - n_prior), batches.size(), ms);
    }
    // no silent degradation: a full visited table made a search stop early, records past rec_cap were dropped.  The bits are
    // this build's: they leave the session's guard word here, so that a later vsr_screening_check is not poisoned
    uint32_t word = 0;
    HB_CHK(hipMemcpy(&word, bp.err, sizeof word, hipMemcpyDeviceToHost));
    if (word & (HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES)) {
        *guard = word & (HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES);
        word &= ~(HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES);
        HB_CHK(hipMemcpy(bp.err, &word, sizeof word, hipMemcpyHostToDevice));
        return bail(VSR_OK);
    }
#undef HB_CHK
    cleanup();
    h->entry = ne > 0 ? entry : -1;
    h->entry_level = ne > 0 ? entry_level : -1;
    if (!merge) {
        // an inserted element holds its row alone (a build: element e is internal row e); prior elements keep their TID lists
        std::vector<int32_t> erow(alloc, 0), tcount(alloc, 1), itids(alloc * 10, -1);
        if (n_prior > 0) {
            std::copy(prior->tid_count, prior->tid_count + n_prior, tcount.begin());
            std::copy(prior->itids.begin(), prior->itids.begin() + (size_t) n_prior * 10, itids.begin());
        }
        for (int64_t e = 0; e < ne; ++e) {
            erow[(size_t) e] = prior ? prior->elem_row[(size_t) e] : (int32_t) e;
            if (e >= n_prior) itids[(size_t) e * 10] = erow[(size_t) e];
        }
        auto& up = upload_i32;
        int rc = VSR_OK;
        if ((!h->d_elem_row && (rc = up(&h->d_elem_row, erow.data(), alloc))) || (rc = up(&h->d_tid_count, tcount.data(), alloc)) ||
            (rc = up(&h->d_tids, itids.data(), alloc * 10))) {
            vsr_hnsw_free(h.release());
            return rc;
        }
    }
    c->hnsw_indexes.push_back(h.get());
    *out = h.release();
    return VSR_OK;
}

// The build never returns a thinner graph than it was asked for: when a layer search filled its visited table the build is
// run again with a table twice as large, as long as one fits the LDS; dropped reverse edges are an error.
// VSR_HNSW_BUILD_VISITED_SLOTS=n (development / tests; a power of two, 256 .. 32768; read at every call) sets the INITIAL table
// size, so that the restart can be exercised on a small corpus.
// A sparse build also restarts, with a candidate array twice as long, when a layer search lost an unexpanded candidate as near as
// the furthest of W (HB_ERR_CANDIDATES, vsr_hnsw_build.hip): pgvector's candidate heap has no bound, and rows without a common
// index all have inner product 0, so such ties outgrow ef_construction + 2 m entries.
static int hnsw_env_visited_slots(const char* who, uint32_t* slots)           // VSR_HNSW_BUILD_VISITED_SLOTS; unset: *slots stays
{
    if (const char* env = getenv("VSR_HNSW_BUILD_VISITED_SLOTS")) {
        char* end = nullptr;
        const long v = strtol(env, &end, 10);
        if (end == env || *end != '\0' || v < 256 || v > 32768 || (v & (v - 1)) != 0)
            return fail(VSR_ERR_INVALID, "%s: VSR_HNSW_BUILD_VISITED_SLOTS must be a power of two from 256 to 32768 (got \"%s\")", who, env);
        *slots = (uint32_t) v;
    }
    return VSR_OK;
}

static int hnsw_build(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out,
                      const char* who, const HnswPrior* prior = nullptr)
{
    uint32_t slots = 0;
    if (const int rc = hnsw_env_visited_slots(who, &slots)) {
        if (out) *out = nullptr;
        return rc;
    }
    uint32_t caps = (uint32_t) (ef_construction + 2 * m);
    for (;;) {
        uint32_t guard = 0;
        const int rc = hnsw_build_once(c, expect, m, ef_construction, metric, seed, flags, out, who, &slots, caps, &guard, prior);
        if (rc != VSR_OK || guard == 0) return rc;
        if (guard & HB_ERR_RECORDS)
            return fail(VSR_ERR_UNSUPPORTED, "%s: reverse edges were dropped at ef_construction = %d with m = %d: the graph would be incomplete", who,
                        ef_construction, m);
        if (guard & HB_ERR_CANDIDATES) {
            if (hnsw_build_lds_per_wave(caps * 2u, slots, hnsw_build_sparse_slots(c, expect)) > HN_LDS_BUDGET)
                return fail(VSR_ERR_UNSUPPORTED,
                            "%s: a layer search at ef_construction = %d with m = %d holds more than %u candidates of equal distance and no longer "
                            "candidate array fits the LDS", who, ef_construction, m, caps);
            caps *= 2u;
            if (!(guard & HB_ERR_VISITED)) continue;
        }
        // HB_ERR_VISITED
        if (slots >= 32768u || hnsw_build_lds_per_wave(caps, slots * 2u, hnsw_build_sparse_slots(c, expect)) > HN_LDS_BUDGET)
            return fail(VSR_ERR_UNSUPPORTED,
                        "%s: a layer search at ef_construction = %d with m = %d fills its visited table of %u entries and no larger one fits the LDS",
                        who, ef_construction, m, slots);
        slots *= 2u;
    }
}

extern "C" int vsr_hnsw_build(vsr_corpus* c, int m, int ef_construction, int metric, uint64_t seed, vsr_hnsw** out)
{
    return hnsw_build(c, RowFormat::F32, m, ef_construction, metric, seed, 0u, out, "vsr_hnsw_build");
}

extern "C" int vsr_hnsw_build_ex(vsr_corpus* c, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    return hnsw_build(c, RowFormat::F32, m, ef_construction, metric, seed, flags, out, "vsr_hnsw_build_ex");
}

extern "C" int vsr_hnsw_build_bit(vsr_corpus* c, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    return hnsw_build(c, RowFormat::BIT, m, ef_construction, metric, seed, flags, out, "vsr_hnsw_build_bit");
}

extern "C" int vsr_hnsw_build_half(vsr_corpus* c, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    return hnsw_build(c, RowFormat::HALF, m, ef_construction, metric, seed, flags, out, "vsr_hnsw_build_half");
}

extern "C" int vsr_hnsw_build_sparse(vsr_corpus* c, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    return hnsw_build(c, RowFormat::SPARSE, m, ef_construction, metric, seed, flags, out, "vsr_hnsw_build_sparse");
}

// ---- vsr_hnsw_build_partitions: the graphs of many row subsets in one global element space (vsr_hnsw_forest.h has the schedule,
// vsr_hnsw_build.hip the forest form of the search kernel and the split launch)
static_assert(HF_BATCH_MAX == HB_BATCH_MAX, "the forest's schedule is the build's");

// what the host pass leaves for every attempt: the partitions as runs of one element space
struct HnswForest {
    int n_parts = 0;
    std::vector<int64_t> base;               // [n_parts + 1] partition g owns elements base[g] .. base[g + 1] - 1
    std::vector<int32_t> elem_row;           // [total] element -> internal row: a partition's rows in ascending internal order
    std::vector<int32_t> level;              // [total] the build's level stream, started afresh for every partition
    std::vector<int32_t> up_slot;            // [total] upper slots in global element order, -1 for level 0
    std::vector<int32_t> slot_base, n_upper, max_level;   // [n_parts] a graph's first slot, its slots, its own max_level (>= 1)
    int32_t g_upper = 0, g_max_level = 1;    // all slots / the stride of the global upper arrays
    HnswForestPlan plan;
};

// One attempt with `slots` visited-table entries; *guard: as hnsw_build_once.  On success out[g] holds every index, registered
static int hnsw_forest_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswForest& fo, uint32_t* slots_io,
                            uint32_t* guard, vsr_hnsw** out, const char* who)
{
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t total = (size_t) fo.base[(size_t) fo.n_parts];
    const uint32_t row_chunks = format_row_chunks(expect, c->dim);
    std::vector<std::unique_ptr<vsr_hnsw>> made((size_t) fo.n_parts);
    std::vector<void*> scratch;                                               // every device allocation of the attempt but the indexes'
    auto cleanup = [&]() {
        for (void* q : scratch)
            if (q) (void) hipFree(q);
        scratch.clear();
    };
    auto bail = [&](int rc) {
        (void) hipStreamSynchronize(ctx->stream);
        cleanup();
        for (auto& h : made)
            if (h) vsr_hnsw_free(h.release());                                // (not registered yet: corpus stays nullptr until the end)
        return rc;
    };
#define HF_CHK(call)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return bail(fail(VSR_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)));          \
    } while (0)
    auto dev = [&](void** p, size_t bytes) -> hipError_t {
        const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 4));
        if (e == hipSuccess) scratch.push_back(*p);
        return e;
    };
    // every index and its arrays first: an allocation that fails costs no GPU work.  An empty partition: what hnsw_load makes of n_elem = 0
    std::vector<HnswForestGraph> graphs;
    for (int g = 0; g < fo.n_parts; ++g) {
        std::unique_ptr<vsr_hnsw> h(new vsr_hnsw());
        const size_t ne = (size_t) (fo.base[(size_t) g + 1] - fo.base[(size_t) g]);
        h->format = expect;
        h->bit_metric = expect == RowFormat::BIT ? metric : 0;
        h->m = m;
        h->n_elem = (int32_t) ne;
        h->max_level = fo.max_level[(size_t) g];
        h->n_upper = fo.n_upper[(size_t) g];
        const int32_t e = fo.plan.final_entry[(size_t) g];
        h->entry = e >= 0 ? (int32_t) (e - fo.base[(size_t) g]) : -1;
        h->entry_level = e >= 0 ? fo.level[(size_t) e] : -1;
        made[(size_t) g] = std::move(h);
        vsr_hnsw* hh = made[(size_t) g].get();
        const size_t counts[7] = {ne, ne, ne * 2 * m, ne, (size_t) hh->n_upper * hh->max_level * m, ne, ne * 10};
        int32_t** ptrs[7] = {&hh->d_elem_row, &hh->d_level, &hh->d_nbr0, &hh->d_up_slot, &hh->d_up_nbr, &hh->d_tid_count, &hh->d_tids};
        for (int i = 0; i < 7; ++i) HF_CHK(hipMalloc(ptrs[i], std::max<size_t>(4, counts[i] * sizeof(int32_t))));
        if (ne == 0) continue;
        HnswForestGraph fg{};
        fg.level = hh->d_level;
        fg.elem_row = hh->d_elem_row;
        fg.nbr0 = hh->d_nbr0;
        fg.up_slot = hh->d_up_slot;
        fg.up_nbr = hh->d_up_nbr;
        fg.tid_count = hh->d_tid_count;
        fg.tids = hh->d_tids;
        fg.base = (int32_t) fo.base[(size_t) g];
        fg.n_elem = (int32_t) ne;
        fg.slot_base = fo.slot_base[(size_t) g];
        fg.max_level = hh->max_level;
        graphs.push_back(fg);
    }
    if (total > 0) {
        int32_t *d_level = nullptr, *d_elem_row = nullptr, *d_up_slot = nullptr, *d_nbr0 = nullptr, *d_up_nbr = nullptr, *d_plan = nullptr;
        float *d_dist0 = nullptr, *d_up_dist = nullptr;
        uint64_t *d_key[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr};
        uint32_t* d_cnt = nullptr;
        void* d_tmp = nullptr;
        HnswForestGraph* d_graphs = nullptr;
        const size_t up_words = (size_t) std::max(fo.g_upper, 1) * fo.g_max_level * m;
        HF_CHK(dev((void**) &d_level, total * 4));
        HF_CHK(dev((void**) &d_elem_row, total * 4));
        HF_CHK(dev((void**) &d_up_slot, total * 4));
        HF_CHK(dev((void**) &d_nbr0, total * 2 * m * 4));
        HF_CHK(dev((void**) &d_dist0, total * 2 * m * 4));
        HF_CHK(dev((void**) &d_up_nbr, up_words * 4));
        HF_CHK(dev((void**) &d_up_dist, up_words * 4));
        HF_CHK(dev((void**) &d_plan, total * 3 * 4));                         // the rounds' elements | entry points | their levels
        HF_CHK(dev((void**) &d_graphs, graphs.size() * sizeof(HnswForestGraph)));
        HF_CHK(hipMemcpy(d_level, fo.level.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_elem_row, fo.elem_row.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_up_slot, fo.up_slot.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_plan, fo.plan.elems.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_plan + total, fo.plan.entry.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_plan + 2 * total, fo.plan.entry_level.data(), total * 4, hipMemcpyHostToDevice));
        HF_CHK(hipMemcpy(d_graphs, graphs.data(), graphs.size() * sizeof(HnswForestGraph), hipMemcpyHostToDevice));
        HF_CHK(hipMemsetAsync(d_nbr0, 0xFF, total * 2 * m * 4, ctx->stream));
        HF_CHK(hipMemsetAsync(d_up_nbr, 0xFF, up_words * 4, ctx->stream));
        HF_CHK(hipMemsetAsync(d_dist0, 0, total * 2 * m * 4, ctx->stream));
        HF_CHK(hipMemsetAsync(d_up_dist, 0, up_words * 4, ctx->stream));

        HnswBuildParams bp{};
        bp.rows = c->d_rows;
        bp.stride4 = row_chunks;
        bp.metric = metric == VSR_METRIC_L2 ? M_L2 : M_IP;
        bp.halves = expect == RowFormat::HALF ? 1 : 0;
        if (expect == RowFormat::BIT) {
            bp.bits = 1;
            bp.metric = metric == VSR_METRIC_JACCARD ? M_JACCARD : M_HAMMING;
            bp.row_pop = c->d_norm2;
        }
        bp.m = (uint32_t) m;
        bp.efc = (uint32_t) ef_construction;
        bp.max_level = (uint32_t) fo.g_max_level;
        bp.nbr0 = d_nbr0;
        bp.dist0 = d_dist0;
        bp.up_slot = d_up_slot;
        bp.up_nbr = d_up_nbr;
        bp.up_dist = d_up_dist;
        bp.level = d_level;
        bp.elem_row = d_elem_row;
        bp.caps = (uint32_t) (ef_construction + 2 * m);
        uint32_t slots = *slots_io;
        if (slots == 0) {                                                     // the build's default
            slots = 4096;
            while (slots < (uint32_t) ef_construction * 2u * (uint32_t) m * 2u && slots < 32768u) slots <<= 1;
            *slots_io = slots;
        }
        bp.hash_slots = slots;
        const size_t per = hnsw_build_lds_per_wave(bp.caps, slots);
        if (per > HN_LDS_BUDGET) return bail(fail(VSR_ERR_UNSUPPORTED, "%s: ef_construction = %d with m = %d does not fit the LDS", who, ef_construction, m));
        bp.lds_per_wave = (uint32_t) per;
        bp.wpb = (uint32_t) std::min<size_t>(4, HN_LDS_BUDGET / per);
        bp.err = ctx->err_word();
        uint32_t rec_cap_max = 1;
        size_t tmp_bytes = 0;
        {
            std::vector<uint32_t> caps;                                       // the sort's scratch: the most any round's size asks for
            for (const HnswForestRound& r : fo.plan.rounds) caps.push_back(r.rec_cap);
            std::sort(caps.begin(), caps.end());
            caps.erase(std::unique(caps.begin(), caps.end()), caps.end());
            for (uint32_t cap : caps) tmp_bytes = std::max(tmp_bytes, vsr_hnsw_build_sort_bytes(cap));
            if (!caps.empty()) rec_cap_max = std::max(rec_cap_max, caps.back());
        }
        for (int i = 0; i < 2; ++i) {
            HF_CHK(dev((void**) &d_key[i], (size_t) rec_cap_max * 8));
            HF_CHK(dev((void**) &d_val[i], (size_t) rec_cap_max * 8));
        }
        HF_CHK(dev((void**) &d_cnt, 64));
        HF_CHK(dev(&d_tmp, std::max<size_t>(tmp_bytes, 256)));
        bp.rec_count = d_cnt;
        for (const HnswForestRound& r : fo.plan.rounds) {
            HnswForestParams fp{};
            fp.elems = d_plan + r.first_slot;
            fp.entry = d_plan + total + r.first_slot;
            fp.entry_level = d_plan + 2 * total + r.first_slot;
            bp.count = r.count;
            bp.rec_cap = r.rec_cap;
            bp.rec_key = d_key[0];
            bp.rec_val = d_val[0];
            HF_CHK(vsr_hnsw_forest_round(bp, fp, d_tmp, tmp_bytes, d_key[1], d_val[1], ctx->stream));
        }
        HF_CHK(vsr_hnsw_forest_split(bp, d_graphs, (uint32_t) graphs.size(), (uint32_t) total, ctx->stream));
        HF_CHK(hipStreamSynchronize(ctx->stream));
        // the build's rule: never a thinner graph.  The bits are this call's and leave the session's guard word here
        uint32_t word = 0;
        HF_CHK(hipMemcpy(&word, bp.err, sizeof word, hipMemcpyDeviceToHost));
        if (word & (HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES)) {
            *guard = word & (HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES);
            word &= ~(HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES);
            HF_CHK(hipMemcpy(bp.err, &word, sizeof word, hipMemcpyHostToDevice));
            return bail(VSR_OK);
        }
    }
#undef HF_CHK
    cleanup();
    for (int g = 0; g < fo.n_parts; ++g) {
        made[(size_t) g]->corpus = c;
        c->hnsw_indexes.push_back(made[(size_t) g].get());
        out[g] = made[(size_t) g].release();
    }
    return VSR_OK;
}

extern "C" int vsr_hnsw_build_partitions(vsr_corpus* c, int n_parts, const int64_t* part_off, const int64_t* part_rows, int m, int ef_construction,
                                         int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    const char* who = "vsr_hnsw_build_partitions";
    if (out)
        for (int g = 0; g < n_parts; ++g) out[g] = nullptr;
    if (!c || n_parts < 0 || (n_parts > 0 && (!out || !part_off))) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    const RowFormat expect = c->format;
    if (expect == RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED,
                    "%s: a sparsevec corpus is not supported (the sparse build has no element -> row form): build every partition's graph with "
                    "vsr_hnsw_build_sparse over a corpus of its rows", who);
    if (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES)
        return fail(VSR_ERR_UNSUPPORTED, "%s: VSR_HNSW_BUILD_MERGE_DUPLICATES is not supported (every element of a partition graph is one row)", who);
    {
        vsr_hnsw* none = nullptr;
        const int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, &none, who);
        if (rc) return rc;
    }
    uint32_t cap = HB_BATCH_MAX;
    if (const char* env = getenv("VSR_HNSW_FOREST_BATCH")) {
        char* end = nullptr;
        const long v = strtol(env, &end, 10);
        if (end == env || *end != '\0' || v < 1 || v > (long) HB_BATCH_MAX)
            return fail(VSR_ERR_INVALID, "%s: VSR_HNSW_FOREST_BATCH must be a number from 1 to %u (got \"%s\")", who, HB_BATCH_MAX, env);
        cap = (uint32_t) v;
    }
    uint32_t slots = 0;
    if (const int rc = hnsw_env_visited_slots(who, &slots)) return rc;
    if (n_parts == 0) return VSR_OK;
    if (part_off[0] != 0) return fail(VSR_ERR_INVALID, "%s: part_off[0] is %lld, not 0", who, (long long) part_off[0]);
    for (int g = 0; g < n_parts; ++g)
        if (part_off[g + 1] < part_off[g])
            return fail(VSR_ERR_INVALID, "%s: part_off does not ascend at partition %d (%lld after %lld)", who, g, (long long) part_off[g + 1],
                        (long long) part_off[g]);
    const int64_t total = part_off[n_parts];
    if (total > 0 && !part_rows) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    if (total > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);

    HnswForest fo;
    fo.n_parts = n_parts;
    fo.base.assign(part_off, part_off + n_parts + 1);
    fo.elem_row.resize((size_t) total);
    {
        // caller rows -> internal rows; within a partition every row once (seen[row] = the partition that named it last, + 1)
        std::vector<int32_t> inv((size_t) std::max<int64_t>(c->n, 1), -1), seen((size_t) std::max<int64_t>(c->n, 1), 0);
        for (int64_t r = 0; r < c->n; ++r) inv[(size_t) c->h_orig[(size_t) r]] = (int32_t) r;
        for (int g = 0; g < n_parts; ++g) {
            for (int64_t i = part_off[g]; i < part_off[g + 1]; ++i) {
                const int64_t row = part_rows[i];
                if (row < 0 || row >= c->n)
                    return fail(VSR_ERR_INVALID, "%s: partition %d, position %lld: row %lld is outside [0, %lld)", who, g, (long long) (i - part_off[g]),
                                (long long) row, (long long) c->n);
                if (seen[(size_t) row] == g + 1)
                    return fail(VSR_ERR_INVALID, "%s: partition %d, position %lld: row %lld is named twice", who, g, (long long) (i - part_off[g]),
                                (long long) row);
                seen[(size_t) row] = g + 1;
                fo.elem_row[(size_t) i] = inv[(size_t) row];
            }
            std::sort(fo.elem_row.begin() + part_off[g], fo.elem_row.begin() + part_off[g + 1]);   // the build's insertion order
        }
    }
    // levels: the build's stream, drawn once as far as the largest partition needs and read from its start by each
    {
        int64_t longest = 0;
        for (int g = 0; g < n_parts; ++g) longest = std::max(longest, part_off[g + 1] - part_off[g]);
        HnswLevelStream stream(seed, m);
        std::vector<int32_t> draws((size_t) longest);
        for (int32_t& d : draws) d = stream.level();
        fo.level.resize((size_t) total);
        for (int g = 0; g < n_parts; ++g) std::copy(draws.begin(), draws.begin() + (part_off[g + 1] - part_off[g]), fo.level.begin() + part_off[g]);
    }
    fo.up_slot.assign((size_t) total, -1);
    fo.slot_base.assign((size_t) n_parts, 0);
    fo.n_upper.assign((size_t) n_parts, 0);
    fo.max_level.assign((size_t) n_parts, 1);
    for (int g = 0; g < n_parts; ++g) {
        fo.slot_base[(size_t) g] = fo.g_upper;
        for (int64_t e = part_off[g]; e < part_off[g + 1]; ++e)
            if (fo.level[(size_t) e] >= 1) {
                fo.up_slot[(size_t) e] = fo.g_upper++;
                fo.max_level[(size_t) g] = std::max(fo.max_level[(size_t) g], fo.level[(size_t) e]);
            }
        fo.n_upper[(size_t) g] = fo.g_upper - fo.slot_base[(size_t) g];
        fo.g_max_level = std::max(fo.g_max_level, fo.max_level[(size_t) g]);
    }
    if (!hnsw_forest_plan(n_parts, fo.base.data(), fo.level.data(), m, cap, fo.plan))
        return fail(VSR_ERR_UNSUPPORTED, "%s: a round with m = %d has too many reverse edges", who, m);
    for (;;) {
        uint32_t guard = 0;
        const int rc = hnsw_forest_once(c, expect, m, ef_construction, metric, fo, &slots, &guard, out, who);
        if (rc != VSR_OK || guard == 0) return rc;
        if (guard & HB_ERR_RECORDS)
            return fail(VSR_ERR_UNSUPPORTED, "%s: reverse edges were dropped at ef_construction = %d with m = %d: the graph would be incomplete", who,
                        ef_construction, m);
        // HB_ERR_VISITED, in any graph: the whole call again, as hnsw_build
        if (slots >= 32768u || hnsw_build_lds_per_wave((uint32_t) (ef_construction + 2 * m), slots * 2u) > HN_LDS_BUDGET)
            return fail(VSR_ERR_UNSUPPORTED,
                        "%s: a layer search at ef_construction = %d with m = %d fills its visited table of %u entries and no larger one fits the LDS",
                        who, ef_construction, m, slots);
        slots *= 2u;
    }
}

// vsr_hnsw_extend's host pass over the caller's graph, before anything is uploaded.  The extension WRITES through these lists
// (phase 2 updates the lists of old elements, the edge-distance launch gathers rows through every id), so it asks more than
// hnsw_load: ids in [-1, n_elem), packed lists, a neighbour on layer lc living on layer lc (else its up_slot is -1 and the
// reverse-edge pass would write out of bounds), upper slots distinct exactly where level >= 1, the entry on the top level, no row
// under two TIDs.  Leaves in pr what hnsw_build_once needs: TIDs as internal rows, element -> row with the rows no TID names
// appended in ascending internal order (the build's insertion order), slot -> element.
static int hnsw_extend_prepare(const vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                               const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr, int32_t n_upper,
                               int32_t max_level, HnswPrior& pr, const char* who)
{
    if (c->n > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many rows", who);
    if (n_elem < 0 || (n_elem > 0 && (!level || !nbr0 || !tid_count || !tids || !up_slot || entry < 0)) || max_level < 1 || n_upper < 0 ||
        (n_upper > 0 && !up_nbr) || entry >= n_elem)
        return fail(VSR_ERR_INVALID, "%s: bad graph arrays", who);
    pr.n_elem = n_elem;
    pr.entry = n_elem > 0 ? entry : -1;
    pr.n_upper = n_elem > 0 ? n_upper : 0;
    pr.max_level = n_elem > 0 ? max_level : 1;
    pr.level = level; pr.nbr0 = nbr0; pr.tid_count = tid_count; pr.up_slot = up_slot; pr.up_nbr = up_nbr;
    const size_t rows = (size_t) c->n;
    std::vector<int32_t> inv(std::max<size_t>(rows, 1), -1);
    for (size_t r = 0; r < rows; ++r) inv[(size_t) c->h_orig[r]] = (int32_t) r;
    std::vector<uint8_t> covered(std::max<size_t>(rows, 1), 0);
    pr.itids.assign((size_t) std::max(n_elem, 1) * 10, -1);
    pr.up_owner.assign((size_t) std::max(pr.n_upper, 1), -1);
    int32_t top = 0;
    for (int32_t e = 0; e < n_elem; ++e) {
        if (tid_count[e] < 1 || tid_count[e] > 10 || level[e] < 0 || level[e] > max_level)
            return fail(VSR_ERR_INVALID, "%s: element %d has %d heap TIDs / level %d", who, e, tid_count[e], level[e]);
        for (int t = 0; t < tid_count[e]; ++t) {
            const int64_t row = tids[(size_t) e * 10 + t];
            if (row < 0 || row >= c->n) return fail(VSR_ERR_INVALID, "%s: element %d points at row %lld", who, e, (long long) row);
            const int32_t r = inv[(size_t) row];
            if (covered[(size_t) r]) return fail(VSR_ERR_INVALID, "%s: element %d names row %lld, which another heap TID names already", who, e, (long long) row);
            covered[(size_t) r] = 1;
            pr.itids[(size_t) e * 10 + t] = r;
        }
        pr.n0 += tid_count[e];
        const int32_t s = up_slot[e];
        if (level[e] >= 1) {
            if (s < 0 || s >= n_upper) return fail(VSR_ERR_INVALID, "%s: element %d of level %d has upper slot %d, outside [0, %d)", who, e, level[e], s, n_upper);
            if (pr.up_owner[(size_t) s] >= 0)
                return fail(VSR_ERR_INVALID, "%s: element %d shares upper slot %d with element %d", who, e, s, pr.up_owner[(size_t) s]);
            pr.up_owner[(size_t) s] = e;
        } else if (s != -1)
            return fail(VSR_ERR_INVALID, "%s: element %d of level 0 has upper slot %d (must be -1)", who, e, s);
        top = std::max(top, level[e]);
    }
    if (n_elem > 0 && level[entry] != top)
        return fail(VSR_ERR_INVALID, "%s: entry element %d has level %d, below the highest level %d", who, entry, level[entry], top);
    for (int32_t e = 0; e < n_elem; ++e)
        for (int lc = 0; lc <= level[e]; ++lc) {
            const int lm = lc == 0 ? 2 * m : m;
            const int32_t* nl = lc == 0 ? nbr0 + (size_t) e * 2 * m : up_nbr + ((size_t) up_slot[e] * max_level + (size_t) (lc - 1)) * m;
            bool gap = false;
            for (int j = 0; j < lm; ++j) {
                const int32_t id = nl[j];
                if (id < -1 || id >= n_elem)
                    return fail(VSR_ERR_INVALID, "%s: element %d lists neighbour %d on layer %d, outside [-1, %d)", who, e, id, lc, n_elem);
                if (id < 0) { gap = true; continue; }
                if (gap) return fail(VSR_ERR_INVALID, "%s: element %d: the layer %d list is not packed (neighbour %d follows a -1)", who, e, lc, id);
                if (level[id] < lc)
                    return fail(VSR_ERR_INVALID, "%s: element %d lists neighbour %d on layer %d, above that element's level %d", who, e, id, lc, level[id]);
            }
        }
    pr.n_new = c->n - pr.n0;
    pr.elem_row.assign((size_t) std::max<int64_t>(n_elem + pr.n_new, 1), 0);
    for (int32_t e = 0; e < n_elem; ++e) pr.elem_row[(size_t) e] = pr.itids[(size_t) e * 10];
    size_t at = (size_t) n_elem;
    for (size_t r = 0; r < rows; ++r)
        if (!covered[r]) pr.elem_row[at++] = (int32_t) r;
    pr.identity = true;
    for (size_t e = 0; e < (size_t) (n_elem + pr.n_new); ++e) pr.identity = pr.identity && pr.elem_row[e] == (int32_t) e;
    return VSR_OK;
}

// INSERT into a table that has an hnsw index (hnswinsert.c), for a batch of rows: the arrays vsr_hnsw_load takes, over a corpus
// that holds the rows they were built on plus new ones; the new rows go in by the build's own batches (hnsw_build_once with a prior).
extern "C" int vsr_hnsw_extend(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                               const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr, int32_t n_upper,
                               int32_t max_level, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    const char* who = "vsr_hnsw_extend";
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (c->format == RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED,
                    "%s: the graph of a sparsevec corpus cannot be extended yet (the sparse build has no element -> row form): rebuild it with "
                    "vsr_hnsw_build_sparse", who);
    const RowFormat expect = c->format;
    int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, out, who);
    if (rc) return rc;
    if (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES)
        return fail(VSR_ERR_UNSUPPORTED, "%s: VSR_HNSW_BUILD_MERGE_DUPLICATES is not supported: an inserted row is never folded into an existing element", who);
    HnswPrior pr;
    rc = hnsw_extend_prepare(c, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, pr, who);
    if (rc) return rc;
    if (pr.n_new == 0)                                                        // nothing to insert: the graph as it is
        return hnsw_load(c, expect, expect == RowFormat::BIT ? metric : 0, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper,
                         max_level, out, who);
    return hnsw_build(c, expect, m, ef_construction, metric, seed, 0u, out, who, &pr);
}

// ---- VACUUM (hnswvacuum.c): delete rows from a graph, repair it on the GPU, squeeze the deleted elements out.
// pass 1 on the host: the surviving TIDs, which elements live, the highest live element other than the entry (RemoveHeapTids'
// scan: strict >, so the lowest id of the top level)
struct HnswVacuumPlan {
    std::vector<int32_t> live;               // [n_elem] 1: a heap TID is left
    std::vector<int32_t> tcount, itids;      // the surviving TIDs (internal rows), in their old order, moved to the front; -1 padded
    int32_t highest = -1, n_live = 0;
    int64_t removed = 0, kept = 0;
    bool identity = true;                    // element e is internal row e for every prior element: the direct kernels serve
};

// per-wave LDS of the repair's search kernel (hb_search_body, VAC): S and the flags, the three HB_NBR arrays, the visited table; the
// selection's scratch lies over the table, so an entry of S costs 9 bytes and a graph's whole working set can be thousands long
static size_t hnsw_vacuum_lds_per_wave(uint32_t caps, uint32_t slots)
{
    return ((size_t) caps * 8 + ((caps + 15) & ~15u) + (size_t) HB_NBR * 12 + (size_t) slots * 4 + 15) & ~(size_t) 15;
}

// how an attempt treats a repair that outgrows the LDS arrays (hnsw_vacuum_search_spill_kernel, vsr_hnsw_build.hip)
enum { HV_SPILL_NONE = 0,                    // the guard bits: the caller's ladders
       HV_SPILL_MIXED = 1,                   // such a repair is listed and redone in the global-memory form
       HV_SPILL_ALL = 2 };                   // every repair runs in that form (VSR_HNSW_VACUUM_SPILL=all)
constexpr uint32_t HV_SPILL_WAVES = 1024;    // cap of the workspace pool: four waves a CU
struct HnswVacuumSpill {
    int      mode = HV_SPILL_NONE;
    size_t   lds_budget = HN_LDS_BUDGET;     // VSR_HNSW_VACUUM_LDS
    uint32_t waves = HV_SPILL_WAVES;         // VSR_HNSW_VACUUM_SPILL_WAVES
};

// One attempt with `slots` visited-table entries and `caps` candidate entries, from the caller's arrays.  *guard: as hnsw_build_once
static int hnsw_vacuum_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswPrior& pr, const HnswVacuumPlan& pl,
                            uint32_t slots, uint32_t caps, uint32_t batch_max, const HnswVacuumSpill& sp, uint32_t* guard,
                            vsr_hnsw_vacuum_stats* st, int32_t* out_elem_map, vsr_hnsw** out, const char* who)
{
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t ne = (size_t) pr.n_elem, lm0 = (size_t) 2 * m;
    const int32_t max_level = pr.max_level;
    const size_t up_words = (size_t) std::max(pr.n_upper, 1) * max_level * m;
    const uint32_t row_chunks = format_row_chunks(expect, c->dim);
    std::vector<void*> work;                                                  // everything but the result's arrays
    std::unique_ptr<vsr_hnsw> h(new vsr_hnsw());
    h->corpus = c;
    h->format = expect;
    h->bit_metric = expect == RowFormat::BIT ? metric : 0;
    h->m = m;
    auto bail = [&](int rc) {
        (void) hipStreamSynchronize(ctx->stream);
        for (void* q : work) (void) hipFree(q);
        vsr_hnsw_free(h.release());
        return rc;
    };
#define HV_CHK(call)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return bail(fail(VSR_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)));          \
    } while (0)
#define HV_ALLOC(ptr, bytes)                                                                                 \
    do {                                                                                                     \
        void* q_ = nullptr;                                                                                  \
        HV_CHK(hipMalloc(&q_, std::max<size_t>((bytes), 16)));                                               \
        work.push_back(q_);                                                                                  \
        (ptr) = static_cast<std::remove_reference_t<decltype(ptr)>>(q_);                                     \
    } while (0)
    int32_t *w_level, *w_nbr0, *w_up_slot, *w_up_nbr, *w_live, *w_elem_row = nullptr, *w_up_owner, *w_list, *w_num, *w_map, *w_slot_map, *w_stage_n;
    float *w_dist0, *w_up_dist, *w_stage_d;
    uint8_t* w_flag;
    HV_ALLOC(w_level, ne * 4);
    HV_ALLOC(w_nbr0, ne * lm0 * 4);
    HV_ALLOC(w_up_slot, ne * 4);
    HV_ALLOC(w_up_nbr, up_words * 4);
    HV_ALLOC(w_dist0, ne * lm0 * 4);
    HV_ALLOC(w_up_dist, up_words * 4);
    HV_ALLOC(w_live, ne * 4);
    HV_ALLOC(w_up_owner, (size_t) std::max(pr.n_upper, 1) * 4);
    HV_ALLOC(w_list, ne * 4);
    HV_ALLOC(w_num, 16);                                                      // [0]: the repair list's length; [1], [2]: batches of one
    HV_ALLOC(w_map, ne * 4);
    HV_ALLOC(w_slot_map, (size_t) std::max(pr.n_upper, 1) * 4);
    HV_ALLOC(w_flag, ne);
    HV_CHK(hipMemsetAsync(w_up_nbr, 0xFF, up_words * 4, ctx->stream));
    HV_CHK(hipMemsetAsync(w_dist0, 0, ne * lm0 * 4, ctx->stream));
    HV_CHK(hipMemsetAsync(w_up_dist, 0, up_words * 4, ctx->stream));
    HV_CHK(hipStreamSynchronize(ctx->stream));                                // the copies below are not on the stream
    HV_CHK(hipMemcpy(w_level, pr.level, ne * 4, hipMemcpyHostToDevice));
    HV_CHK(hipMemcpy(w_nbr0, pr.nbr0, ne * lm0 * 4, hipMemcpyHostToDevice));
    HV_CHK(hipMemcpy(w_up_slot, pr.up_slot, ne * 4, hipMemcpyHostToDevice));
    if (pr.n_upper > 0) {
        HV_CHK(hipMemcpy(w_up_nbr, pr.up_nbr, (size_t) pr.n_upper * max_level * m * 4, hipMemcpyHostToDevice));
        HV_CHK(hipMemcpy(w_up_owner, pr.up_owner.data(), (size_t) pr.n_upper * 4, hipMemcpyHostToDevice));
    }
    HV_CHK(hipMemcpy(w_live, pl.live.data(), ne * 4, hipMemcpyHostToDevice));
    if (!pl.identity) {                                                       // a deleted element keeps its row for the whole repair
        HV_ALLOC(w_elem_row, ne * 4);
        HV_CHK(hipMemcpy(w_elem_row, pr.elem_row.data(), ne * 4, hipMemcpyHostToDevice));
    }

    HnswBuildParams bp{};
    bp.rows = c->d_rows;
    bp.stride4 = row_chunks;
    bp.metric = metric == VSR_METRIC_L2 ? M_L2 : M_IP;
    bp.halves = expect == RowFormat::HALF ? 1 : 0;
    if (expect == RowFormat::BIT) {
        bp.bits = 1;
        bp.metric = metric == VSR_METRIC_JACCARD ? M_JACCARD : M_HAMMING;
        bp.row_pop = c->d_norm2;
    }
    bp.m = (uint32_t) m;
    bp.efc = (uint32_t) ef_construction + 1u;                                 // the repaired element counts towards its own beam
    bp.max_level = (uint32_t) max_level;
    bp.nbr0 = w_nbr0;
    bp.dist0 = w_dist0;
    bp.up_slot = w_up_slot;
    bp.up_nbr = w_up_nbr;
    bp.up_dist = w_up_dist;
    bp.level = w_level;
    bp.elem_row = w_elem_row;
    bp.caps = caps;
    bp.hash_slots = slots;
    const size_t per = hnsw_vacuum_lds_per_wave(caps, slots);
    if (per > sp.lds_budget)
        return bail(fail(VSR_ERR_UNSUPPORTED, "%s: %u candidates with a visited table of %u entries do not fit the LDS", who, caps, slots));
    bp.lds_per_wave = (uint32_t) per;
    bp.wpb = (uint32_t) std::min<size_t>(4, sp.lds_budget / per);
    bp.err = ctx->err_word();

    HnswVacuumParams vp{};
    const uint32_t stride = (uint32_t) (2 * m + max_level * m);
    const uint64_t most = std::min<uint64_t>(batch_max, (uint64_t) std::max(pl.n_live, 1));
    if (most * stride > 0x7FFFFFFFull) return bail(fail(VSR_ERR_UNSUPPORTED, "%s: a batch of %llu elements with m = %d has too many reverse edges", who, (unsigned long long) most, m));
    const uint32_t rec_cap_max = (uint32_t) (most * stride);
    uint64_t *d_key[2], *d_val[2];
    uint32_t* d_cnt;
    void* d_tmp;
    const size_t tmp_bytes = std::max<size_t>({vsr_hnsw_build_sort_bytes(rec_cap_max), vsr_hnsw_build_sort_bytes(stride), vsr_hnsw_vacuum_tmp_bytes((uint32_t) ne), 256});
    HV_ALLOC(d_key[0], (size_t) rec_cap_max * 8);
    HV_ALLOC(d_key[1], (size_t) rec_cap_max * 8);
    HV_ALLOC(d_val[0], (size_t) rec_cap_max * 8);
    HV_ALLOC(d_val[1], (size_t) rec_cap_max * 8);
    HV_ALLOC(d_cnt, 64);
    HV_ALLOC(d_tmp, tmp_bytes);
    HV_ALLOC(w_stage_n, (size_t) rec_cap_max * 4);
    HV_ALLOC(w_stage_d, (size_t) rec_cap_max * 4);
    bp.rec_count = d_cnt;
    vp.live = w_live;
    vp.stage_nbr = w_stage_n;
    vp.stage_dist = w_stage_d;
    vp.stage_stride = stride;
    // the spill form's pool: one workspace a wave, as many as the largest batch has repairs, a quarter of the free device memory
    // holds and the cap allows -- at least one, whose hipMalloc is then what can fail
    int64_t ws_total = 0;
    if (sp.mode != HV_SPILL_NONE) {
        const size_t ws_bytes = hnsw_vacuum_spill_ws_bytes((uint32_t) ne);
        size_t free_b = 0, total_b = 0;
        HV_CHK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t pool = std::max<uint64_t>(1, std::min<uint64_t>({most, (uint64_t) sp.waves, (uint64_t) (free_b / 4 / ws_bytes)}));
        uint32_t* w_spill;
        HV_ALLOC(w_spill, 16);                                                // [0]: the batch's spill count, [1]: the call's total
        HV_CHK(hipMemsetAsync(w_spill, 0, 16, ctx->stream));
        HV_ALLOC(vp.spill_ws, (size_t) pool * ws_bytes);
        vp.spill_ws_bytes = ws_bytes;
        vp.spill_pool = (uint32_t) pool;
        vp.spill_n = (uint32_t) ne;
        vp.spill_total = w_spill + 1;
        if (sp.mode == HV_SPILL_ALL) {
            vp.spill_all = 1;
        } else {
            vp.spill_count = w_spill;
            HV_ALLOC(vp.spill_list, (size_t) most * 4);
        }
        ws_total = (int64_t) (pool * ws_bytes);
    }

    HV_CHK(vsr_hnsw_edge_distances(bp, (uint32_t) ne, w_up_owner, (uint32_t) pr.n_upper, ctx->stream));
    int32_t nrep = 0, nbatch = 0;
    // one repair batch: `count` elements at d_elems, searched from element `from` (-1: nobody is left, the lists become empty)
    auto run_batch = [&](const int32_t* d_elems, uint32_t count, uint32_t rec_cap, int32_t from) -> hipError_t {
        bp.entry = from;
        bp.entry_level = from >= 0 ? pr.level[from] : -1;
        bp.first = 0;
        bp.count = count;
        bp.rec_cap = rec_cap;
        bp.rec_key = d_key[0];
        bp.rec_val = d_val[0];
        vp.elems = d_elems;
        nrep += (int32_t) count;
        ++nbatch;
        return vsr_hnsw_vacuum_batch(bp, vp, d_tmp, tmp_bytes, d_key[1], d_val[1], ctx->stream);
    };
    auto rec_cap_of = [&](int32_t e) { return (uint32_t) (2 * m + pr.level[e] * m); };
    // NeedsUpdated of one element, on the graph as the stream leaves it
    auto needs = [&](int32_t e, bool* yes) -> hipError_t {
        hipError_t e_ = vsr_hnsw_vacuum_mark(bp, w_live, (uint32_t) ne, -1, w_flag, nullptr, nullptr, d_tmp, tmp_bytes, ctx->stream);
        if (e_ != hipSuccess) return e_;
        if ((e_ = hipStreamSynchronize(ctx->stream)) != hipSuccess) return e_;
        uint8_t f = 0;
        e_ = hipMemcpy(&f, w_flag + e, 1, hipMemcpyDeviceToHost);
        *yes = f != 0;
        return e_;
    };
    // the entry phase (RepairGraphEntryPoint), batches of one
    int32_t entry = pr.entry;
    const int32_t hp = pl.highest;
    const int32_t ones[2] = {hp, entry};
    HV_CHK(hipMemcpy(w_num + 1, ones, sizeof ones, hipMemcpyHostToDevice));
    if (hp >= 0) {
        bool yes = false;
        HV_CHK(needs(hp, &yes));
        if (yes) HV_CHK(run_batch(w_num + 1, 1, rec_cap_of(hp), entry));      // from the entry as it is, deleted or not
    }
    if (pl.live[(size_t) entry] == 0) {
        entry = hp;
    } else {
        bool yes = false;
        HV_CHK(needs(entry, &yes));
        if (yes) HV_CHK(run_batch(w_num + 2, 1, rec_cap_of(entry), hp));
    }
    // the main phase: the repair list once, after the entry phase
    HV_CHK(vsr_hnsw_vacuum_mark(bp, w_live, (uint32_t) ne, entry, w_flag, w_list, w_num, d_tmp, tmp_bytes, ctx->stream));
    HV_CHK(hipStreamSynchronize(ctx->stream));
    int32_t n_list = 0;
    HV_CHK(hipMemcpy(&n_list, w_num, 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> list((size_t) std::max(n_list, 1));
    if (n_list > 0) HV_CHK(hipMemcpy(list.data(), w_list, (size_t) n_list * 4, hipMemcpyDeviceToHost));
    // the guard word after the entry phase and after every batch: an attempt whose arrays are too short ends where that shows
    uint32_t word = 0;
    const uint32_t guard_bits = HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES;
    HV_CHK(hipMemcpy(&word, bp.err, sizeof word, hipMemcpyDeviceToHost));
    for (int32_t at = 0; at < n_list && !(word & guard_bits);) {
        const uint32_t b = (uint32_t) std::min<int64_t>(batch_max, n_list - at);
        uint64_t cap = 0;
        for (uint32_t i = 0; i < b; ++i) cap += rec_cap_of(list[(size_t) at + i]);
        HV_CHK(run_batch(w_list + at, b, (uint32_t) cap, entry));             // (cap <= rec_cap_max: b <= most, a level <= max_level)
        at += (int32_t) b;
        HV_CHK(hipStreamSynchronize(ctx->stream));
        HV_CHK(hipMemcpy(&word, bp.err, sizeof word, hipMemcpyDeviceToHost));
    }
    if (word & guard_bits) {
        *guard = word & guard_bits;
        word &= ~guard_bits;
        HV_CHK(hipMemcpy(bp.err, &word, sizeof word, hipMemcpyHostToDevice));
        return bail(VSR_OK);
    }

    // pass 3: the compacted index.  Elements in ascending old id, upper slots in ascending old slot, the upper arrays at the new top
    std::vector<int32_t> map(ne, -1), slot_map((size_t) std::max(pr.n_upper, 1), -1);
    int32_t n_new = 0, n_upper_new = 0;
    for (size_t e = 0; e < ne; ++e)
        if (pl.live[e]) map[e] = n_new++;
    for (int32_t s = 0; s < pr.n_upper; ++s)
        if (pr.up_owner[(size_t) s] >= 0 && pl.live[(size_t) pr.up_owner[(size_t) s]]) slot_map[(size_t) s] = n_upper_new++;
    const int32_t new_max_level = std::max(1, pr.level[entry]);
    const size_t nn = (size_t) n_new, new_up_words = (size_t) std::max(n_upper_new, 1) * new_max_level * m;
    std::vector<int32_t> level(nn), up_slot(nn), tcount(nn), erow(nn), itids(nn * 10);
    for (size_t e = 0; e < ne; ++e) {
        if (!pl.live[e]) continue;
        const size_t k = (size_t) map[e];
        level[k] = pr.level[e];
        up_slot[k] = pr.up_slot[e] >= 0 ? slot_map[(size_t) pr.up_slot[e]] : -1;
        tcount[k] = pl.tcount[e];
        std::copy(pl.itids.begin() + e * 10, pl.itids.begin() + (e + 1) * 10, itids.begin() + k * 10);
        erow[k] = itids[k * 10];
    }
    h->n_elem = n_new;
    h->entry = map[(size_t) entry];
    h->entry_level = pr.level[entry];
    h->max_level = new_max_level;
    h->n_upper = n_upper_new;
    HV_CHK(hipMemcpy(w_slot_map, slot_map.data(), slot_map.size() * 4, hipMemcpyHostToDevice));
    HV_CHK(hipMalloc(&h->d_nbr0, std::max<size_t>(nn * lm0 * 4, 4)));
    HV_CHK(hipMalloc(&h->d_up_nbr, new_up_words * 4));
    HV_CHK(hipMemsetAsync(h->d_nbr0, 0xFF, std::max<size_t>(nn * lm0 * 4, 4), ctx->stream));
    HV_CHK(hipMemsetAsync(h->d_up_nbr, 0xFF, new_up_words * 4, ctx->stream));
    HV_CHK(vsr_hnsw_vacuum_renumber(bp, w_live, w_map, w_slot_map, (uint32_t) ne, h->d_nbr0, h->d_up_nbr, (uint32_t) new_max_level, d_tmp, tmp_bytes,
                                    ctx->stream));
    HV_CHK(hipStreamSynchronize(ctx->stream));
    HV_CHK(hipMemcpy(&word, bp.err, sizeof word, hipMemcpyDeviceToHost));
    if (word & guard_bits) {                                                  // (HB_ERR_RECORDS: a live list still named a deleted element)
        *guard = word & guard_bits;
        word &= ~guard_bits;
        HV_CHK(hipMemcpy(bp.err, &word, sizeof word, hipMemcpyHostToDevice));
        return bail(VSR_OK);
    }
    if (vp.spill_total) {
        uint32_t spilled = 0;
        HV_CHK(hipMemcpy(&spilled, vp.spill_total, sizeof spilled, hipMemcpyDeviceToHost));
        h->vacuum_spilled = (int32_t) spilled;
        h->vacuum_ws_bytes = ws_total;
    }
    // the device's scan and the host's must agree: the lists were renumbered by the one, the other arrays by the other
    std::vector<int32_t> dmap(ne);
    HV_CHK(hipMemcpy(dmap.data(), w_map, ne * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < ne; ++e)
        if (pl.live[e] && dmap[e] != map[e]) return bail(fail(VSR_ERR_HIP, "%s: the element scan disagrees at element %zu", who, e));
#undef HV_ALLOC
#undef HV_CHK
    for (void* q : work) (void) hipFree(q);
    work.clear();
    auto& up = upload_i32;
    int rc = VSR_OK;
    if ((rc = up(&h->d_elem_row, erow.data(), nn)) || (rc = up(&h->d_level, level.data(), nn)) || (rc = up(&h->d_up_slot, up_slot.data(), nn)) ||
        (rc = up(&h->d_tid_count, tcount.data(), nn)) || (rc = up(&h->d_tids, itids.data(), nn * 10))) {
        vsr_hnsw_free(h.release());
        return rc;
    }
    if (out_elem_map) std::copy(map.begin(), map.end(), out_elem_map);
    if (st) {
        st->elements_repaired = nrep;
        st->batches = nbatch;
    }
    c->hnsw_indexes.push_back(h.get());
    *out = h.release();
    return VSR_OK;
}

// VACUUM of an index after DELETE (include/vsrbac.h).  The ladders are the build's: a visited table twice as large, a candidate
// array twice as long (or the longest that fits), every attempt from the caller's arrays; where a ladder ends, one more attempt
// in mixed form, whose overflowing repairs are redone in global memory (HnswVacuumSpill).  Read at every call (development / tests):
// VSR_HNSW_VACUUM_CAPS=n, the INITIAL candidate entries (ef_construction + 1 ..), VSR_HNSW_VACUUM_BATCH=n, the batch maximum
// (1 .. 4096), and VSR_HNSW_BUILD_VISITED_SLOTS as for the build.
extern "C" int vsr_hnsw_vacuum(vsr_corpus* c, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                               const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr, int32_t n_upper,
                               int32_t max_level, int ef_construction, int metric, const int64_t* dead_rows, int64_t n_dead, uint32_t flags,
                               int32_t* out_elem_map, vsr_hnsw_vacuum_stats* out_stats, vsr_hnsw** out)
{
    const char* who = "vsr_hnsw_vacuum";
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (c->format == RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED,
                    "%s: the graph of a sparsevec corpus cannot be vacuumed yet (the sparse build has no element -> row form): rebuild it with "
                    "vsr_hnsw_build_sparse over the live rows", who);
    if (flags != 0) return fail(VSR_ERR_INVALID, "%s: flags must be 0 (got 0x%x)", who, flags);
    const RowFormat expect = c->format;
    int rc = hnsw_build_check(c, expect, m, ef_construction, metric, 0u, out, who);
    if (rc) return rc;
    if (n_dead < 0 || (n_dead > 0 && !dead_rows)) return fail(VSR_ERR_INVALID, "%s: bad dead_rows", who);
    for (int64_t i = 0; i < n_dead; ++i)
        if (dead_rows[i] < 0 || dead_rows[i] >= c->n)
            return fail(VSR_ERR_INVALID, "%s: dead row %lld is outside [0, %lld)", who, (long long) dead_rows[i], (long long) c->n);
    HnswPrior pr;
    rc = hnsw_extend_prepare(c, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, pr, who);
    if (rc) return rc;
    vsr_hnsw_vacuum_stats st{};
    const int bit_metric = expect == RowFormat::BIT ? metric : 0;
    if (n_dead == 0 || n_elem == 0) {                                         // nothing to delete: the graph as it is
        st.tuples_kept = pr.n0;
        for (int32_t e = 0; out_elem_map && e < n_elem; ++e) out_elem_map[e] = e;
        if (out_stats) *out_stats = st;
        return hnsw_load(c, expect, bit_metric, m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level, out, who);
    }
    // pass 1
    const size_t ne = (size_t) n_elem;
    HnswVacuumPlan pl;
    {
        std::vector<int32_t> inv((size_t) c->n, -1);
        for (int64_t r = 0; r < c->n; ++r) inv[(size_t) c->h_orig[(size_t) r]] = (int32_t) r;
        std::vector<uint8_t> dead((size_t) c->n, 0);
        for (int64_t i = 0; i < n_dead; ++i) dead[(size_t) inv[(size_t) dead_rows[i]]] = 1;
        pl.live.assign(ne, 0);
        pl.tcount.assign(ne, 0);
        pl.itids.assign(ne * 10, -1);
        int32_t hl = -1;
        for (size_t e = 0; e < ne; ++e) {
            int k = 0;
            for (int t = 0; t < tid_count[e]; ++t) {
                const int32_t r = pr.itids[e * 10 + (size_t) t];
                if (!dead[(size_t) r]) pl.itids[e * 10 + (size_t) k++] = r;
            }
            pl.tcount[e] = k;
            pl.removed += tid_count[e] - k;
            pl.kept += k;
            pl.live[e] = k > 0;
            pl.n_live += k > 0;
            pl.identity = pl.identity && pr.elem_row[e] == (int32_t) e;
            if (k > 0 && (int32_t) e != entry && level[e] > hl) {
                pl.highest = (int32_t) e;
                hl = level[e];
            }
        }
    }
    st.tuples_removed = pl.removed;
    st.tuples_kept = pl.kept;
    st.elements_removed = n_elem - pl.n_live;
    if (pl.n_live == 0) {                                                     // everything is deleted: the empty index
        for (int32_t e = 0; out_elem_map && e < n_elem; ++e) out_elem_map[e] = -1;
        if (out_stats) *out_stats = st;
        return hnsw_load(c, expect, bit_metric, m, 0, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, out, who);
    }
    // the knobs and the initial sizes.  Candidates: what the build holds, ef_construction + 1 + 2 m, over the live share, since
    // W holds every deleted element met on the way to ef live ones; the result does not depend on it (HB_ERR_CANDIDATES)
    uint32_t slots = 0;
    if ((rc = hnsw_env_visited_slots(who, &slots))) return rc;
    const bool slots_given = slots != 0;
    if (slots == 0) {
        slots = 4096;
        while (slots < (uint32_t) ef_construction * 2u * (uint32_t) m * 2u && slots < 32768u) slots <<= 1;
    }
    auto env_int = [&](const char* name, long lo, long hi, long* v) -> int {
        const char* env = getenv(name);
        if (!env) return VSR_OK;
        char* end = nullptr;
        const long x = strtol(env, &end, 10);
        if (end == env || *end != '\0' || x < lo || x > hi) return fail(VSR_ERR_INVALID, "%s: %s must be between %ld and %ld (got \"%s\")", who, name, lo, hi, env);
        *v = x;
        return VSR_OK;
    };
    // the longest candidate array that fits beside `s` visited slots (hnsw_vacuum_lds_per_wave: 9 bytes an entry), a multiple of 16
    const uint32_t caps_min = (uint32_t) ef_construction + 1u;
    // the spill knobs.  VSR_HNSW_VACUUM_SPILL: unset / 1: a repair that outgrows the largest arrays the LDS holds is redone in the
    // global-memory form (one mixed attempt where the ladders end); 0: never, the refusals as they were; all: every repair in that
    // form from the first attempt.  VSR_HNSW_VACUUM_LDS=bytes: the LDS the sizing and the ladders believe in;
    // VSR_HNSW_VACUUM_SPILL_WAVES=n: the cap of the workspace pool
    HnswVacuumSpill sp;
    int spill = 1;
    if (const char* env = getenv("VSR_HNSW_VACUUM_SPILL")) {
        if (!strcmp(env, "0")) spill = 0;
        else if (!strcmp(env, "1")) spill = 1;
        else if (!strcmp(env, "all")) spill = 2;
        else return fail(VSR_ERR_INVALID, "%s: VSR_HNSW_VACUUM_SPILL must be 0, 1 or all (got \"%s\")", who, env);
    }
    long lds = 0, waves = HV_SPILL_WAVES;
    if ((rc = env_int("VSR_HNSW_VACUUM_LDS", (long) hnsw_vacuum_lds_per_wave(caps_min, 256), (long) HN_LDS_BUDGET, &lds))) return rc;
    if ((rc = env_int("VSR_HNSW_VACUUM_SPILL_WAVES", 1, 1L << 20, &waves))) return rc;
    if (lds > 0) sp.lds_budget = (size_t) lds;
    sp.waves = (uint32_t) waves;
    const size_t budget = sp.lds_budget;
    // a budget that was given may be below the default table: the largest table beside which caps_min candidates still fit
    while (lds > 0 && !slots_given && slots > 256u && hnsw_vacuum_lds_per_wave(caps_min, slots) > budget) slots /= 2u;
    auto caps_fit = [&](uint32_t s) -> uint32_t {
        const size_t fixed = (size_t) HB_NBR * 12 + (size_t) s * 4 + 64;
        return budget > fixed ? (uint32_t) ((budget - fixed) / 9) & ~15u : 0u;
    };
    long v = 0;
    if ((rc = env_int("VSR_HNSW_VACUUM_CAPS", (long) caps_min, 1L << 20, &v))) return rc;
    uint32_t caps;
    if (v > 0) {
        caps = (uint32_t) v;
    } else {
        const uint64_t base = (uint64_t) ef_construction + 1u + 2u * (uint64_t) m;
        const uint64_t want = std::min<uint64_t>((base * (uint64_t) n_elem + (uint64_t) pl.n_live - 1) / (uint64_t) pl.n_live, (uint64_t) n_elem);
        caps = (uint32_t) std::max<uint64_t>(base, std::min<uint64_t>((want + 15) & ~15ull, caps_fit(slots)));
        if (lds > 0 && hnsw_vacuum_lds_per_wave(caps, slots) > budget) caps = std::max(caps_min, caps_fit(slots));   // (a given budget below `base`)
    }
    // every candidate was visited first, so a table that fills at 3/4 should hold what the candidate array is sized for
    while (!slots_given && v == 0 && slots < 32768u && (uint64_t) slots * 3u < (uint64_t) caps * 4u && hnsw_vacuum_lds_per_wave(caps, slots * 2u) <= budget)
        slots *= 2u;
    long batch = HB_BATCH_MAX;
    if ((rc = env_int("VSR_HNSW_VACUUM_BATCH", 1, (long) HB_BATCH_MAX, &batch))) return rc;
    // where a ladder ends with spilling on, ONE more attempt at the sizes it has, in mixed form: the repairs that fit stay on the
    // LDS kernel, the others are redone in the global-memory form, which cannot overflow
    sp.mode = spill == 2 ? HV_SPILL_ALL : HV_SPILL_NONE;
    auto go_mixed = [&]() -> bool {
        if (spill != 1 || sp.mode != HV_SPILL_NONE) return false;
        sp.mode = HV_SPILL_MIXED;
        return true;
    };
    for (;;) {
        uint32_t guard = 0;
        ++st.attempts;
        rc = hnsw_vacuum_once(c, expect, m, ef_construction, metric, pr, pl, slots, caps, (uint32_t) batch, sp, &guard, &st, out_elem_map, out, who);
        if (rc != VSR_OK || guard == 0) {
            if (rc == VSR_OK && out_stats) *out_stats = st;
            return rc;
        }
        if (guard & HB_ERR_RECORDS)
            return fail(VSR_ERR_UNSUPPORTED, "%s: the repair at ef_construction = %d with m = %d dropped reverse edges or left a list that names a "
                        "deleted element: the graph would be incomplete", who, ef_construction, m);
        const char* rebuild = "a graph this dead is to be rebuilt over its live rows (vsr_hnsw_build*)";
        if (guard & HB_ERR_CANDIDATES) {
            const uint32_t next = std::min(caps * 2u, caps_fit(slots));
            if (next <= caps || hnsw_vacuum_lds_per_wave(next, slots) > budget) {
                if (go_mixed()) continue;
                return fail(VSR_ERR_UNSUPPORTED, "%s: a layer search of the repair holds more than %u candidates (%d of %d elements live) and no longer "
                            "candidate array fits the LDS: %s", who, caps, pl.n_live, n_elem, rebuild);
            }
            caps = next;
            if (!(guard & HB_ERR_VISITED)) continue;
        }
        if (slots >= 32768u || hnsw_vacuum_lds_per_wave(caps, slots * 2u) > budget) {
            if (go_mixed()) continue;
            return fail(VSR_ERR_UNSUPPORTED, "%s: a layer search of the repair fills its visited table of %u entries (%d of %d elements live) and no "
                        "larger one fits the LDS: %s", who, slots, pl.n_live, n_elem, rebuild);
        }
        slots *= 2u;
    }
}

extern "C" int vsr_hnsw_vacuum_spill_info(const vsr_hnsw* h, int32_t* spilled_repairs, int64_t* workspace_bytes)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_vacuum_spill_info: index is NULL");
    if (spilled_repairs) *spilled_repairs = h->vacuum_spilled;
    if (workspace_bytes) *workspace_bytes = h->vacuum_ws_bytes;
    return VSR_OK;
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
    std::unique_ptr<vsr_hnsw> host(new vsr_hnsw);
    host->format = indexes[0]->format;
    host->bit_metric = indexes[0]->bit_metric;
    host->m = indexes[0]->m;
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
    host->corpus = c;
    c->hnsw_indexes.push_back(host.get());
    f->host = host.release();
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
