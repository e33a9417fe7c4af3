// vsr_hnsw_build_rt.hip — the host side of everything that makes an HNSW graph on the GPU: vsr_hnsw_build / _ex / _bit / _half /
// _sparse, vsr_hnsw_extend, vsr_hnsw_build_partitions, vsr_hnsw_extend_partitions and vsr_hnsw_vacuum.  No device code: the kernels are in vsr_hnsw_build.hip
// and vsr_hnsw_dedup.hip, what is decided without a GPU in vsr_hnsw_sizing.h and vsr_hnsw_forest.h, the index object and its load
// in vsr_hnsw_index.h / vsr_hnsw_rt.hip.  Every call is attempts under a ladder: an attempt (hnsw_build_once, hnsw_forest_once,
// hnsw_vacuum_once) runs the whole call from the caller's arrays with `slots` visited-table entries and `caps` candidates; when a
// kernel set a guard-word bit its result is thrown away and hnsw_ladder_step says with which sizes to try again, or that none fit.
#include "vsr_hnsw_index.h"
#include "vsr_hnsw_build.h"
#include "vsr_hnsw_forest.h"
#include "vsr_bitops.h"

#include <cstdio>
#include <cstdlib>

// ---- the attempt scaffold
// An attempt's device scratch and events.  Everything an attempt changes is a device copy, so a failed attempt only has to let go:
// the destructor waits for the stream (kernels and asynchronous copies may still read the scratch and the host arrays declared
// before the attempt) and then frees.  The index under construction is an HnswOwner declared BEFORE the attempt, so it goes after.
struct HnswAttempt {
    vsr_ctx* ctx;
    const char* who;
    std::vector<void*> scratch;
    std::vector<hipEvent_t> events;
    HnswAttempt(vsr_ctx* ctx_, const char* who_) : ctx(ctx_), who(who_) {}
    HnswAttempt(const HnswAttempt&) = delete;
    HnswAttempt& operator=(const HnswAttempt&) = delete;
    ~HnswAttempt()
    {
        if (scratch.empty() && events.empty()) return;
        (void) hipStreamSynchronize(ctx->stream);
        free_all();
    }
    template <class T> hipError_t alloc(T** p, size_t count)
    {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 16));
        if (e == hipSuccess) scratch.push_back(q);
        *p = static_cast<T*>(q);
        return e;
    }
    template <class T> hipError_t upload(T** p, const T* src, size_t count)   // alloc, then a copy that is not on the stream
    {
        const hipError_t e = alloc(p, count);
        return e != hipSuccess || !count ? e : hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t event(hipEvent_t* ev)
    {
        const hipError_t e = hipEventCreate(ev);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    void free_all()                                                           // the success path: the stream has been waited for
    {
        for (hipEvent_t e : events) (void) hipEventDestroy(e);
        for (void* q : scratch) (void) hipFree(q);
        events.clear();
        scratch.clear();
    }
    int check(hipError_t e) const { return e == hipSuccess ? VSR_OK : fail(VSR_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
};
// the one checked-call path of an attempt `at`: a HIP error ends the function, whose destructors clean up
#define HNSW_TRY(call)                                                                                       \
    do {                                                                                                     \
        if (const int rc_ = at.check(call)) return rc_;                                                      \
    } while (0)

// slots of a sparse build's left-hand tables: sized once from the corpus's largest row (<= 1000 non-zeros: <= 2048 slots, 16 KB)
static uint32_t hnsw_build_sparse_slots(const vsr_corpus* c, RowFormat expect)
{
    return c && expect == RowFormat::SPARSE && c->format == RowFormat::SPARSE ? sparse_slots_for_nnz(c->sp_max_nnz) : 0u;
}

// the row-format part of the kernels' parameters: how the rows of c are read and which distance `metric` is on them
static void hnsw_row_params(HnswBuildParams& bp, const vsr_corpus* c, RowFormat expect, int metric)
{
    bp.rows = c->d_rows;
    bp.stride4 = format_row_chunks(expect, c->dim);
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
}

// the search kernel's LDS for bp.caps candidates and bp.hash_slots visited slots; false: they do not fit the ladder's budget
static bool hnsw_lds_params(HnswBuildParams& bp, const HnswLadder& l)
{
    const size_t per = l.lds(bp.caps, bp.hash_slots);
    if (per > l.budget) return false;
    bp.lds_per_wave = (uint32_t) per;
    bp.wpb = hnsw_build_wpb(l.budget, per);
    return true;
}

// the reverse edges' records and the sort's scratch, for launches of the given record capacities: the largest batch's slots, the
// most any batch's size asks of the sort (at least tmp_floor bytes, for whoever else works in tmp)
struct HnswRecScratch {
    uint64_t *key[2] = {nullptr, nullptr}, *val[2] = {nullptr, nullptr};
    uint32_t* cnt = nullptr;
    unsigned char* tmp = nullptr;
    size_t tmp_bytes = 0;
    uint32_t rec_cap_max = 1;
};
static hipError_t hnsw_rec_scratch(HnswAttempt& at, std::vector<uint32_t> rec_caps, size_t tmp_floor, HnswRecScratch* rs)
{
    std::sort(rec_caps.begin(), rec_caps.end());
    rec_caps.erase(std::unique(rec_caps.begin(), rec_caps.end()), rec_caps.end());
    rs->tmp_bytes = tmp_floor;
    for (uint32_t cap : rec_caps) rs->tmp_bytes = std::max(rs->tmp_bytes, vsr_hnsw_build_sort_bytes(cap));
    if (!rec_caps.empty()) rs->rec_cap_max = std::max(rs->rec_cap_max, rec_caps.back());
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = at.alloc(&rs->key[i], (size_t) rs->rec_cap_max);
        if (e == hipSuccess) e = at.alloc(&rs->val[i], (size_t) rs->rec_cap_max);
    }
    if (e == hipSuccess) e = at.alloc(&rs->cnt, 16);
    if (e == hipSuccess) e = at.alloc(&rs->tmp, std::max<size_t>(rs->tmp_bytes, 256));
    return e;
}

// no silent degradation: a full visited table made a search stop early, records past rec_cap were dropped.  The bits are this
// call's: *guard takes them and they leave the session's word here, so that a later vsr_screening_check is not poisoned
static hipError_t hnsw_take_guard(uint32_t* err, uint32_t* guard)
{
    uint32_t word = 0;
    const hipError_t e = hipMemcpy(&word, err, sizeof word, hipMemcpyDeviceToHost);
    if (e != hipSuccess || !(word & HB_ERR_BITS)) return e;
    *guard = word & HB_ERR_BITS;
    word &= ~HB_ERR_BITS;
    return hipMemcpy(err, &word, sizeof word, hipMemcpyHostToDevice);
}

// an integer environment knob (development / tests; read at every call).  Unset: *v stays.  Anything but a number in lo .. hi
// (pow2: a power of two) is refused in the knob's own words, "must be <from> lo <to> hi"
static int hnsw_env_int(const char* who, const char* name, long lo, long hi, bool pow2, const char* from, const char* to, long* v)
{
    const char* env = getenv(name);
    if (!env) return VSR_OK;
    char* end = nullptr;
    const long x = strtol(env, &end, 10);
    if (end == env || *end != '\0' || x < lo || x > hi || (pow2 && (x & (x - 1)) != 0))
        return fail(VSR_ERR_INVALID, "%s: %s must be %s %ld %s %ld (got \"%s\")", who, name, from, lo, to, hi, env);
    *v = x;
    return VSR_OK;
}
// VSR_HNSW_BUILD_VISITED_SLOTS=n: the INITIAL visited table, so that the restart can be exercised on a small corpus.  Unset: 0
static int hnsw_env_visited_slots(const char* who, uint32_t* slots)
{
    long v = 0;
    const int rc = hnsw_env_int(who, "VSR_HNSW_BUILD_VISITED_SLOTS", 256, (long) HB_SLOTS_MAX, true, "a power of two from", "to", &v);
    *slots = (uint32_t) v;
    return rc;
}

// ---- CREATE INDEX ... USING hnsw on the GPU (vsr_hnsw_build.hip): batched insertion over the corpus's rows, levels from a seeded
// xorshift64* stream drawn once per row.  flags = 0: element e = internal row e.  VSR_HNSW_BUILD_MERGE_DUPLICATES: the
// elements come from vsr_hnsw_dedup.hip's table.  Returns a loaded index, as vsr_hnsw_load would from the same graph.
// expect: the corpus format the entry point is for -- BIT (vsr_hnsw_build_bit; metric is the opclass), HALF (vsr_hnsw_build_half),
// SPARSE (vsr_hnsw_build_sparse) or F32; the kernels take that row format.
//
// prior (vsr_hnsw_extend, vsr_hnsw_vacuum; nullptr: a build): the caller's graph, checked.  A build is the extension of nothing: no
// prior elements, no draws skipped, the schedule from done = 0, distances all zero.
struct HnswPrior {
    int32_t n_elem = 0, entry = -1, n_upper = 0, max_level = 1;
    const int32_t *level = nullptr, *nbr0 = nullptr, *tid_count = nullptr, *up_slot = nullptr, *up_nbr = nullptr;   // the caller's arrays, checked
    std::vector<int32_t> itids;              // [n_elem][10] heap TIDs as internal rows, -1 padded
    std::vector<int32_t> elem_row;           // [n_elem + n_new] element -> internal row: first TIDs, then the rows no TID names, ascending
    std::vector<int32_t> up_owner;           // [n_upper] upper slot -> its element, -1: no element names the slot
    int64_t n0 = 0, n_new = 0;               // rows the prior graph covers (level draws to skip) / rows to insert
    bool identity = true;                    // element e is internal row e throughout: the direct kernels serve
};

// what every build entry point asks of its corpus and arguments, in the order and words the build has always used
static int hnsw_build_check(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint32_t flags, vsr_hnsw** out, const char* who)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (const int rc = hnsw_opclass(c, expect, metric, who)) return rc;
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

// One attempt with a visited table of *slots_io entries (0: the default for m and ef_construction, written back) and a candidate
// array of `caps` (at least ef_construction + 2 m).  *guard: the guard-word bits a kernel set; *out then stays NULL and the return
// value is VSR_OK: hnsw_build decides what follows.  Its own: the prior graph's upload and the batch loop
static int hnsw_build_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out,
                           const char* who, uint32_t* slots_io, uint32_t caps, uint32_t* guard, const HnswPrior* prior = nullptr)
{
    if (const int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, out, who)) return rc;
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (n > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many rows", who);
    const bool merge = !prior && (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES) != 0 && n > 0;
    const int64_t n_prior = prior ? prior->n_elem : 0;                        // elements that are there already
    const int64_t n_new = prior ? prior->n_new : n;                           // rows to insert, one element each unless merging
    if (n_prior + n_new > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);
    HnswOwner h = hnsw_new_index(c, expect, metric, m);
    // per element: the prior graph's levels, then one draw per inserted row (merging: per row, then per element).  The i-th
    // inserted row takes draw n0 + i, so a prefix build extended with the build's seed draws what the one-shot build draws.
    // (level and prior_up feed asynchronous copies: they are declared before the attempt, which waits for the stream before they die)
    std::vector<int32_t> level((size_t) std::max<int64_t>(n_prior + n_new, 1), 0), prior_up;
    HnswAttempt at(ctx, who);
    HnswLevelStream draws(seed, m);
    if (n_prior > 0) std::copy(prior->level, prior->level + n_prior, level.begin());
    for (int64_t r = 0; r < (prior ? prior->n0 : 0); ++r) (void) draws.next();
    for (int64_t r = 0; r < n_new; ++r) level[(size_t) (n_prior + r)] = draws.level();
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
        int32_t* d_row_level = nullptr;
        HNSW_TRY(at.alloc(&d_row_level, (size_t) n));
        HNSW_TRY(hipMemcpyAsync(d_row_level, level.data(), (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
        HNSW_TRY(vsr_hnsw_dedup_elements(c->d_rows, (uint32_t) n, format_row_chunks(expect, c->dim), hash_bits, d_row_level, &t,
                                         timing ? &times : nullptr, ctx->stream));
        h->d_elem_row = t.elem_row;
        h->d_tid_count = t.tid_count;
        h->d_tids = t.tids;
        h->d_level = t.level;
        ne = t.n_elem;
        HNSW_TRY(hipMemcpy(level.data(), t.level, (size_t) ne * 4, hipMemcpyDeviceToHost));
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
    float *d_dist0 = nullptr, *d_up_dist = nullptr;
    int32_t* d_up_owner = nullptr;
    if (!merge) {
        HNSW_TRY(hipMalloc(&h->d_level, alloc * 4));
        HNSW_TRY(hipMemcpy(h->d_level, level.data(), alloc * 4, hipMemcpyHostToDevice));
    }
    HNSW_TRY(hipMalloc(&h->d_up_slot, alloc * 4));
    HNSW_TRY(hipMalloc(&h->d_nbr0, alloc * 2 * m * 4));
    HNSW_TRY(hipMalloc(&h->d_up_nbr, up_words * 4));
    HNSW_TRY(at.alloc(&d_dist0, alloc * 2 * m));
    HNSW_TRY(at.alloc(&d_up_dist, up_words));
    HNSW_TRY(hipMemcpy(h->d_up_slot, up_slot.data(), alloc * 4, hipMemcpyHostToDevice));
    HNSW_TRY(hipMemsetAsync(h->d_nbr0, 0xFF, alloc * 2 * m * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(h->d_up_nbr, 0xFF, up_words * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(d_dist0, 0, alloc * 2 * m * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(d_up_dist, 0, up_words * 4, ctx->stream));
    // the prior graph's lists, behind the memsets on the same stream; the upper arrays at this graph's max_level (a new element
    // above the prior top re-strides them)
    if (n_prior > 0) {
        HNSW_TRY(hipMemcpyAsync(h->d_nbr0, prior->nbr0, (size_t) n_prior * 2 * m * 4, hipMemcpyHostToDevice, ctx->stream));
        if (prior->n_upper > 0) {
            const int32_t* src = prior->up_nbr;
            if (max_level != prior->max_level) {
                prior_up.assign((size_t) prior->n_upper * max_level * m, -1);
                for (int32_t s = 0; s < prior->n_upper; ++s)
                    std::copy(src + (size_t) s * prior->max_level * m, src + (size_t) (s + 1) * prior->max_level * m,
                              prior_up.begin() + (size_t) s * max_level * m);
                src = prior_up.data();
            }
            HNSW_TRY(hipMemcpyAsync(h->d_up_nbr, src, (size_t) prior->n_upper * max_level * m * 4, hipMemcpyHostToDevice, ctx->stream));
            HNSW_TRY(at.alloc(&d_up_owner, (size_t) prior->n_upper));
            HNSW_TRY(hipMemcpyAsync(d_up_owner, prior->up_owner.data(), (size_t) prior->n_upper * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (!prior->identity) {
            const int rc = upload_i32(&h->d_elem_row, prior->elem_row.data(), (size_t) ne);
            if (rc) return rc;
        }
    }

    HnswBuildParams bp{};
    hnsw_row_params(bp, c, expect, metric);
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
    if (*slots_io == 0) *slots_io = hnsw_default_visited_slots(ef_construction, m);
    bp.hash_slots = *slots_io;
    const HnswLadder ladder{false, bp.sp_slots};
    if (!hnsw_lds_params(bp, ladder)) return fail(VSR_ERR_UNSUPPORTED, "%s: ef_construction = %d with m = %d does not fit the LDS", who, ef_construction, m);
    bp.err = ctx->err_word();
    // the schedule (hnsw_build_batch); a batch's record slots are known here, so the sort and the link launch cover those, not the
    // largest batch's
    struct Batch { uint32_t first, count, rec_cap; };
    std::vector<Batch> batches;
    std::vector<uint32_t> rec_caps;
    for (int64_t done = n_prior; done < ne;) {
        const int64_t b = hnsw_build_batch(done, ne);
        uint64_t cap = 0;
        for (int64_t e = done; e < done + b; ++e) cap += hnsw_rec_cap(m, level[(size_t) e]);
        if (cap > 0x7FFFFFFFull) return fail(VSR_ERR_UNSUPPORTED, "%s: a batch of %lld elements with m = %d has too many reverse edges", who, (long long) b, m);
        batches.push_back({(uint32_t) done, (uint32_t) b, (uint32_t) cap});
        rec_caps.push_back((uint32_t) cap);
        done += b;
    }
    HnswRecScratch rs;
    HNSW_TRY(hnsw_rec_scratch(at, rec_caps, 0, &rs));
    bp.rec_count = rs.cnt;

    int32_t entry = -1, entry_level = -1;
    const char* tenv = getenv("VSR_HNSW_EXTEND_TIMING");                      // development: 1 prints the edge-distance launch's device time
    const bool edge_timing = n_prior > 0 && tenv && atoi(tenv) > 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (n_prior > 0) {
        // the one piece of build state the arrays do not carry: the distance of every edge, which the link kernel's re-selection reads
        entry = prior->entry;
        entry_level = level[(size_t) entry];
        if (edge_timing) {
            HNSW_TRY(at.event(&ev[0]));
            HNSW_TRY(at.event(&ev[1]));
            HNSW_TRY(hipEventRecord(ev[0], ctx->stream));
        }
        HNSW_TRY(vsr_hnsw_edge_distances(bp, (uint32_t) n_prior, d_up_owner, (uint32_t) prior->n_upper, ctx->stream));
        if (edge_timing) HNSW_TRY(hipEventRecord(ev[1], ctx->stream));
    }
    for (const Batch& bt : batches) {
        bp.entry = entry;
        bp.entry_level = entry_level;
        bp.first = bt.first;
        bp.count = bt.count;
        bp.rec_cap = bt.rec_cap;
        bp.rec_key = rs.key[0];
        bp.rec_val = rs.val[0];
        HNSW_TRY(vsr_hnsw_build_batch(bp, rs.tmp, rs.tmp_bytes, rs.key[1], rs.val[1], ctx->stream));
        for (uint32_t e = bt.first; e < bt.first + bt.count; ++e)   // HnswUpdateGraphInMemory: a higher element becomes the entry point
            if (entry < 0 || level[(size_t) e] > entry_level) {
                entry = (int32_t) e;
                entry_level = level[(size_t) e];
            }
    }
    HNSW_TRY(hipStreamSynchronize(ctx->stream));
    if (edge_timing) {
        float ms = 0.0f;
        HNSW_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "vsr_hnsw_extend: prior_elements=%lld new_elements=%lld batches=%zu edge_dist_ms=%.4f\n", (long long) n_prior,
                (long long) (ne - n_prior), batches.size(), ms);
    }
    HNSW_TRY(hnsw_take_guard(bp.err, guard));
    if (*guard) return VSR_OK;                                                // the partial index goes with h
    at.free_all();
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
        int rc = VSR_OK;
        if ((!h->d_elem_row && (rc = upload_i32(&h->d_elem_row, erow.data(), alloc))) || (rc = upload_i32(&h->d_tid_count, tcount.data(), alloc)) ||
            (rc = upload_i32(&h->d_tids, itids.data(), alloc * 10)))
            return rc;
    }
    *out = hnsw_register(std::move(h), 1);
    return VSR_OK;
}

// The build never returns a thinner graph than it was asked for: when a layer search filled its visited table the build is
// run again with a table twice as large, as long as one fits the LDS; dropped reverse edges are an error.
// A sparse build also restarts, with a candidate array twice as long, when a layer search lost an unexpanded candidate as near as
// the furthest of W (HB_ERR_CANDIDATES, vsr_hnsw_build.hip): pgvector's candidate heap has no bound, and rows without a common
// index all have inner product 0, so such ties outgrow ef_construction + 2 m entries.
static int hnsw_build(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out,
                      const char* who, const HnswPrior* prior = nullptr)
{
    uint32_t slots = 0;
    if (const int rc = hnsw_env_visited_slots(who, &slots)) {
        if (out) *out = nullptr;
        return rc;
    }
    uint32_t caps = (uint32_t) (ef_construction + 2 * m);
    const HnswLadder ladder{false, hnsw_build_sparse_slots(c, expect)};
    for (;;) {
        uint32_t guard = 0;
        const int rc = hnsw_build_once(c, expect, m, ef_construction, metric, seed, flags, out, who, &slots, caps, &guard, prior);
        if (rc != VSR_OK || guard == 0) return rc;
        switch (hnsw_ladder_step(ladder, guard, &caps, &slots)) {
        case HB_LADDER_ON: break;
        case HB_LADDER_RECORDS:
            return fail(VSR_ERR_UNSUPPORTED, "%s: reverse edges were dropped at ef_construction = %d with m = %d: the graph would be incomplete", who,
                        ef_construction, m);
        case HB_LADDER_CANDIDATES:
            return fail(VSR_ERR_UNSUPPORTED,
                        "%s: a layer search at ef_construction = %d with m = %d holds more than %u candidates of equal distance and no longer "
                        "candidate array fits the LDS", who, ef_construction, m, caps);
        case HB_LADDER_VISITED:
            return fail(VSR_ERR_UNSUPPORTED,
                        "%s: a layer search at ef_construction = %d with m = %d fills its visited table of %u entries and no larger one fits the LDS",
                        who, ef_construction, m, slots);
        }
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

// the seven device arrays of an index under construction, sized by its n_elem, n_upper, max_level and m (at least 4 bytes each)
static int hnsw_index_arrays(HnswAttempt& at, vsr_hnsw* hh, size_t counts[7] = nullptr)
{
    const size_t ne = (size_t) hh->n_elem, m = (size_t) hh->m;
    const size_t want[7] = {ne, ne, ne * 2 * m, ne, (size_t) hh->n_upper * hh->max_level * m, ne, ne * 10};
    int32_t** ptrs[7] = {&hh->d_elem_row, &hh->d_level, &hh->d_nbr0, &hh->d_up_slot, &hh->d_up_nbr, &hh->d_tid_count, &hh->d_tids};
    for (int i = 0; i < 7; ++i) {
        HNSW_TRY(hipMalloc(ptrs[i], std::max<size_t>(4, want[i] * sizeof(int32_t))));
        if (counts) counts[i] = want[i];
    }
    return VSR_OK;
}

// the global element space of one attempt of a partition call (build or extend): the build arrays over all graphs, the plan's slot
// arrays, the reverse edges' scratch and the kernels' parameters.  All of it is the attempt's scratch
struct HnswForestSpace {
    int32_t *level = nullptr, *elem_row = nullptr, *up_slot = nullptr, *nbr0 = nullptr, *up_nbr = nullptr;
    int32_t* plan = nullptr;                 // [3][slots] the rounds' elements | entry points | their levels
    float *dist0 = nullptr, *up_dist = nullptr;
    size_t total = 0, slots = 0, up_slots = 1, up_words = 0;
    HnswBuildParams bp{};
    HnswRecScratch rs;
};
// allocates and fills the space of fo with *slots_io visited-table entries (0: the build's default, written back): the host's per-element
// arrays uploaded, lists -1, distances 0 (behind the uploads, on the stream)
static int hnsw_forest_space(HnswAttempt& at, vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswForest& fo,
                             uint32_t* slots_io, HnswForestSpace& sp)
{
    vsr_ctx* ctx = c->ctx;
    const size_t total = sp.total = (size_t) fo.base.back(), slots = sp.slots = fo.plan.elems.size();
    sp.up_slots = (size_t) std::max(fo.g_upper, 1);
    sp.up_words = sp.up_slots * fo.g_max_level * m;
    HNSW_TRY(at.upload(&sp.level, fo.level.data(), total));
    HNSW_TRY(at.upload(&sp.elem_row, fo.elem_row.data(), total));
    HNSW_TRY(at.upload(&sp.up_slot, fo.up_slot.data(), total));
    HNSW_TRY(at.alloc(&sp.nbr0, total * 2 * m));
    HNSW_TRY(at.alloc(&sp.dist0, total * 2 * m));
    HNSW_TRY(at.alloc(&sp.up_nbr, sp.up_words));
    HNSW_TRY(at.alloc(&sp.up_dist, sp.up_words));
    HNSW_TRY(at.alloc(&sp.plan, slots * 3));
    HNSW_TRY(hipMemcpy(sp.plan, fo.plan.elems.data(), slots * 4, hipMemcpyHostToDevice));
    HNSW_TRY(hipMemcpy(sp.plan + slots, fo.plan.entry.data(), slots * 4, hipMemcpyHostToDevice));
    HNSW_TRY(hipMemcpy(sp.plan + 2 * slots, fo.plan.entry_level.data(), slots * 4, hipMemcpyHostToDevice));
    HNSW_TRY(hipMemsetAsync(sp.nbr0, 0xFF, total * 2 * m * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(sp.up_nbr, 0xFF, sp.up_words * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(sp.dist0, 0, total * 2 * m * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(sp.up_dist, 0, sp.up_words * 4, ctx->stream));

    HnswBuildParams& bp = sp.bp;
    hnsw_row_params(bp, c, expect, metric);
    bp.m = (uint32_t) m;
    bp.efc = (uint32_t) ef_construction;
    bp.max_level = (uint32_t) fo.g_max_level;
    bp.nbr0 = sp.nbr0;
    bp.dist0 = sp.dist0;
    bp.up_slot = sp.up_slot;
    bp.up_nbr = sp.up_nbr;
    bp.up_dist = sp.up_dist;
    bp.level = sp.level;
    bp.elem_row = sp.elem_row;
    bp.caps = (uint32_t) (ef_construction + 2 * m);
    if (*slots_io == 0) *slots_io = hnsw_default_visited_slots(ef_construction, m);   // the build's default
    bp.hash_slots = *slots_io;
    if (!hnsw_lds_params(bp, HnswLadder{}))
        return fail(VSR_ERR_UNSUPPORTED, "%s: ef_construction = %d with m = %d does not fit the LDS", at.who, ef_construction, m);
    bp.err = ctx->err_word();
    std::vector<uint32_t> rec_caps;
    for (const HnswForestRound& r : fo.plan.rounds) rec_caps.push_back(r.rec_cap);
    HNSW_TRY(hnsw_rec_scratch(at, rec_caps, 0, &sp.rs));
    bp.rec_count = sp.rs.cnt;
    return VSR_OK;
}
// the rounds of fo.plan over sp, on the stream
static int hnsw_forest_rounds(HnswAttempt& at, const HnswForest& fo, HnswForestSpace& sp)
{
    for (const HnswForestRound& r : fo.plan.rounds) {
        HnswForestParams fp{};
        fp.elems = sp.plan + r.first_slot;
        fp.entry = sp.plan + sp.slots + r.first_slot;
        fp.entry_level = sp.plan + 2 * sp.slots + r.first_slot;
        sp.bp.count = r.count;
        sp.bp.rec_cap = r.rec_cap;
        sp.bp.rec_key = sp.rs.key[0];
        sp.bp.rec_val = sp.rs.val[0];
        HNSW_TRY(vsr_hnsw_forest_round(sp.bp, fp, sp.rs.tmp, sp.rs.tmp_bytes, sp.rs.key[1], sp.rs.val[1], at.ctx->stream));
    }
    return VSR_OK;
}

// One attempt with *slots_io visited-table entries; *guard: as hnsw_build_once.  On success out[g] holds every index, registered.
// Its own: the per-graph arrays and the split
static int hnsw_forest_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswForest& fo, uint32_t* slots_io,
                            uint32_t* guard, vsr_hnsw** out, const char* who)
{
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t total = (size_t) fo.base[(size_t) fo.n_parts];
    std::vector<HnswOwner> made((size_t) fo.n_parts);
    HnswAttempt at(ctx, who);                                                 // every device allocation of the attempt but the indexes'
    // every index and its arrays first: an allocation that fails costs no GPU work.  An empty partition: what hnsw_load makes of n_elem = 0
    std::vector<HnswForestGraph> graphs;
    for (int g = 0; g < fo.n_parts; ++g) {
        made[(size_t) g] = hnsw_new_index(c, expect, metric, m);
        vsr_hnsw* hh = made[(size_t) g].get();
        const size_t ne = (size_t) (fo.base[(size_t) g + 1] - fo.base[(size_t) g]);
        hh->n_elem = (int32_t) ne;
        hh->max_level = fo.max_level[(size_t) g];
        hh->n_upper = fo.n_upper[(size_t) g];
        const int32_t e = fo.plan.final_entry[(size_t) g];
        hh->entry = e >= 0 ? (int32_t) (e - fo.base[(size_t) g]) : -1;
        hh->entry_level = e >= 0 ? fo.level[(size_t) e] : -1;
        if (const int rc = hnsw_index_arrays(at, hh)) return rc;
        if (ne > 0)
            graphs.push_back({hh->d_level, hh->d_elem_row, hh->d_nbr0, hh->d_up_slot, hh->d_up_nbr, hh->d_tid_count, hh->d_tids,
                              (int32_t) fo.base[(size_t) g], (int32_t) ne, fo.slot_base[(size_t) g], hh->max_level});
    }
    if (total > 0) {
        HnswForestSpace sp;
        HnswForestGraph* d_graphs = nullptr;
        if (const int rc = hnsw_forest_space(at, c, expect, m, ef_construction, metric, fo, slots_io, sp)) return rc;
        HNSW_TRY(at.upload(&d_graphs, graphs.data(), graphs.size()));
        if (const int rc = hnsw_forest_rounds(at, fo, sp)) return rc;
        HNSW_TRY(vsr_hnsw_forest_split(sp.bp, d_graphs, (uint32_t) graphs.size(), (uint32_t) total, ctx->stream));
        HNSW_TRY(hipStreamSynchronize(ctx->stream));
        HNSW_TRY(hnsw_take_guard(sp.bp.err, guard));                          // the build's rule: never a thinner graph
        if (*guard) return VSR_OK;
    }
    at.free_all();
    for (int g = 0; g < fo.n_parts; ++g) out[g] = hnsw_register(std::move(made[(size_t) g]), 1);
    return VSR_OK;
}

// the partitions' row lists as both partition calls take them: `off` ascends from 0, a row is inside the corpus and named once within
// its partition (seen[row] = the partition that named it last, + 1).  Leaves in `internal` the internal rows, every partition's
// ascending: the build's insertion order.  off_name: what the caller's header calls `off`
static int hnsw_partition_rows(const vsr_corpus* c, int n_parts, const int64_t* off, const int64_t* rows, const char* off_name, const char* who,
                               std::vector<int32_t>& internal)
{
    if (off[0] != 0) return fail(VSR_ERR_INVALID, "%s: %s[0] is %lld, not 0", who, off_name, (long long) off[0]);
    for (int g = 0; g < n_parts; ++g)
        if (off[g + 1] < off[g])
            return fail(VSR_ERR_INVALID, "%s: %s does not ascend at partition %d (%lld after %lld)", who, off_name, g, (long long) off[g + 1],
                        (long long) off[g]);
    const int64_t total = off[n_parts];
    if (total > 0 && !rows) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    if (total > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);
    internal.resize((size_t) total);
    const std::vector<int32_t> inv = hnsw_row_map(c);
    std::vector<int32_t> seen((size_t) std::max<int64_t>(c->n, 1), 0);
    for (int g = 0; g < n_parts; ++g) {
        for (int64_t i = off[g]; i < off[g + 1]; ++i) {
            const int64_t row = rows[i];
            if (row < 0 || row >= c->n)
                return fail(VSR_ERR_INVALID, "%s: partition %d, position %lld: row %lld is outside [0, %lld)", who, g, (long long) (i - off[g]),
                            (long long) row, (long long) c->n);
            if (seen[(size_t) row] == g + 1)
                return fail(VSR_ERR_INVALID, "%s: partition %d, position %lld: row %lld is named twice", who, g, (long long) (i - off[g]),
                            (long long) row);
            seen[(size_t) row] = g + 1;
            internal[(size_t) i] = inv[(size_t) row];
        }
        std::sort(internal.begin() + off[g], internal.begin() + off[g + 1]);
    }
    return VSR_OK;
}

// the attempts of a partition call under the visited-table ladder: once(&slots, &guard) runs the whole call.  Dropped records apart,
// a bit in any graph is the visited table's: the whole call again with twice the slots, as hnsw_build
template <class Once>
static int hnsw_forest_ladder(int m, int ef_construction, uint32_t slots, const char* who, Once once)
{
    uint32_t caps = (uint32_t) (ef_construction + 2 * m);
    for (;;) {
        uint32_t guard = 0;
        const int rc = once(&slots, &guard);
        if (rc != VSR_OK || guard == 0) return rc;
        switch (hnsw_ladder_step(HnswLadder{}, (guard & HB_ERR_RECORDS) | HB_ERR_VISITED, &caps, &slots)) {
        case HB_LADDER_RECORDS:
            return fail(VSR_ERR_UNSUPPORTED, "%s: reverse edges were dropped at ef_construction = %d with m = %d: the graph would be incomplete", who,
                        ef_construction, m);
        case HB_LADDER_VISITED:
            return fail(VSR_ERR_UNSUPPORTED,
                        "%s: a layer search at ef_construction = %d with m = %d fills its visited table of %u entries and no larger one fits the LDS",
                        who, ef_construction, m, slots);
        default: break;
        }
    }
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
    vsr_hnsw* none = nullptr;
    if (const int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, &none, who)) return rc;
    long cap = HB_BATCH_MAX;                                                  // VSR_HNSW_FOREST_BATCH: a round's elements (vsr_hnsw_forest.h)
    if (const int rc = hnsw_env_int(who, "VSR_HNSW_FOREST_BATCH", 1, (long) HB_BATCH_MAX, false, "a number from", "to", &cap)) return rc;
    uint32_t slots = 0;
    if (const int rc = hnsw_env_visited_slots(who, &slots)) return rc;
    if (n_parts == 0) return VSR_OK;
    HnswForest fo;
    fo.n_parts = n_parts;
    if (const int rc = hnsw_partition_rows(c, n_parts, part_off, part_rows, "part_off", who, fo.elem_row)) return rc;
    const int64_t total = part_off[n_parts];
    fo.base.assign(part_off, part_off + n_parts + 1);
    // levels: the build's stream, drawn once as far as the largest partition needs and read from its start by each
    int64_t longest = 0;
    for (int g = 0; g < n_parts; ++g) longest = std::max(longest, part_off[g + 1] - part_off[g]);
    HnswLevelStream stream(seed, m);
    std::vector<int32_t> draws((size_t) longest);
    for (int32_t& d : draws) d = stream.level();
    fo.level.resize((size_t) total);
    for (int g = 0; g < n_parts; ++g) std::copy(draws.begin(), draws.begin() + (part_off[g + 1] - part_off[g]), fo.level.begin() + part_off[g]);
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
    if (!hnsw_forest_plan(n_parts, fo.base.data(), fo.level.data(), m, (uint32_t) cap, fo.plan))
        return fail(VSR_ERR_UNSUPPORTED, "%s: a round with m = %d has too many reverse edges", who, m);
    return hnsw_forest_ladder(m, ef_construction, slots, who, [&](uint32_t* slots_io, uint32_t* guard) {
        return hnsw_forest_once(c, expect, m, ef_construction, metric, fo, slots_io, guard, out, who);
    });
}

// ---- vsr_hnsw_extend's host pass over the caller's graph, before anything is uploaded.  The extension WRITES through these lists
// (phase 2 updates the lists of old elements, the edge-distance launch gathers rows through every id), so it asks more than
// hnsw_load: ids in [-1, n_elem), packed lists, a neighbour on layer lc living on layer lc (else its up_slot is -1 and the
// reverse-edge pass would write out of bounds), upper slots distinct exactly where level >= 1, the entry on the top level, no row
// under two TIDs.  Leaves in pr what hnsw_build_once needs: TIDs as internal rows, element -> row with the rows no TID names
// appended in ascending internal order (the build's insertion order), slot -> element.
static int hnsw_extend_prepare(const vsr_corpus* c, const HnswGraphView& g, HnswPrior& pr, const char* who)
{
    const int m = g.m;
    const int32_t n_elem = g.n_elem, entry = g.entry, n_upper = g.n_upper, max_level = g.max_level;
    const int32_t *level = g.level, *nbr0 = g.nbr0, *tid_count = g.tid_count, *up_slot = g.up_slot, *up_nbr = g.up_nbr;
    if (c->n > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many rows", who);
    if (n_elem < 0 || (n_elem > 0 && (!level || !nbr0 || !tid_count || !g.tids || !up_slot || entry < 0)) || max_level < 1 || n_upper < 0 ||
        (n_upper > 0 && !up_nbr) || entry >= n_elem)
        return fail(VSR_ERR_INVALID, "%s: bad graph arrays", who);
    pr.n_elem = n_elem;
    pr.entry = n_elem > 0 ? entry : -1;
    pr.n_upper = n_elem > 0 ? n_upper : 0;
    pr.max_level = n_elem > 0 ? max_level : 1;
    pr.level = level; pr.nbr0 = nbr0; pr.tid_count = tid_count; pr.up_slot = up_slot; pr.up_nbr = up_nbr;
    const size_t rows = (size_t) c->n;
    const std::vector<int32_t> inv = hnsw_row_map(c);
    std::vector<uint8_t> covered(std::max<size_t>(rows, 1), 0);
    pr.itids.assign((size_t) std::max(n_elem, 1) * 10, -1);
    pr.up_owner.assign((size_t) std::max(pr.n_upper, 1), -1);
    int32_t top = 0;
    for (int32_t e = 0; e < n_elem; ++e) {
        if (tid_count[e] < 1 || tid_count[e] > 10 || level[e] < 0 || level[e] > max_level)
            return fail(VSR_ERR_INVALID, "%s: element %d has %d heap TIDs / level %d", who, e, tid_count[e], level[e]);
        for (int t = 0; t < tid_count[e]; ++t) {
            const int64_t row = g.tids[(size_t) e * 10 + t];
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
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
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
    rc = hnsw_extend_prepare(c, g, pr, who);
    if (rc) return rc;
    if (pr.n_new == 0) return hnsw_load(c, expect, expect == RowFormat::BIT ? metric : 0, g, out, who);   // nothing to insert: the graph as it is
    return hnsw_build(c, expect, m, ef_construction, metric, seed, 0u, out, who, &pr);
}

// ---- vsr_hnsw_extend_partitions: vsr_hnsw_extend for many graphs over one corpus.  The graphs that take rows are joined on the device
// into the global element space of vsr_hnsw_build_partitions (hnsw_forest_join_kernel), every graph's batches run in shared rounds from
// done = its prior n_elem (hnsw_forest_plan_from), and the split writes every graph's own arrays with the prior TID lists carried over

// what the host pass leaves for every attempt
struct HnswForestExtend {
    int n_parts = 0;
    std::vector<const vsr_hnsw*> prior;      // [n_parts] nullptr: no prior graph (NULL, or n_elem = 0)
    std::vector<int> active;                 // the partitions that take rows, ascending: graph i of the element space is active[i]
    std::vector<int64_t> n_prior;            // [active] its prior elements
    HnswForest fo;                           // the element space of the active graphs (fo.n_parts of them): graph i owns base[i] .. base[i + 1]
                                             // - 1, prior elements first; elem_row / level / up_slot hold the new elements' entries, a prior
                                             // element's are the join kernel's
};

// an index like h in arrays of its own (a partition that takes no rows); copies on the stream
static int hnsw_clone_into(HnswAttempt& at, vsr_hnsw* to, const vsr_hnsw* h)
{
    if (h && h->n_elem > 0) {
        to->n_elem = h->n_elem;
        to->entry = h->entry;
        to->entry_level = h->entry_level;
        to->max_level = h->max_level;
        to->n_upper = h->n_upper;
    }
    size_t counts[7];
    if (const int rc = hnsw_index_arrays(at, to, counts)) return rc;
    if (to->n_elem == 0) return VSR_OK;
    int32_t* const ptrs[7] = {to->d_elem_row, to->d_level, to->d_nbr0, to->d_up_slot, to->d_up_nbr, to->d_tid_count, to->d_tids};
    const int32_t* const from[7] = {h->d_elem_row, h->d_level, h->d_nbr0, h->d_up_slot, h->d_up_nbr, h->d_tid_count, h->d_tids};
    for (int i = 0; i < 7; ++i)
        if (counts[i] > 0) HNSW_TRY(hipMemcpyAsync(ptrs[i], from[i], counts[i] * sizeof(int32_t), hipMemcpyDeviceToDevice, at.ctx->stream));
    return VSR_OK;
}

// One attempt with *slots_io visited-table entries; *guard: as hnsw_build_once.  On success out[g] holds every index, registered.
static int hnsw_forest_extend_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswForestExtend& fx,
                                   uint32_t* slots_io, uint32_t* guard, vsr_hnsw** out, const char* who)
{
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const HnswForest& fo = fx.fo;
    const size_t n_graphs = fx.active.size(), total = (size_t) fo.base[n_graphs];
    std::vector<HnswOwner> made((size_t) fx.n_parts);
    std::vector<int> made_here((size_t) fx.n_parts, 1);
    HnswAttempt at(ctx, who);
    std::vector<HnswForestGraph> graphs;
    std::vector<HnswForestPrior> priors;
    size_t next = 0;                                                          // the next active partition
    for (int g = 0; g < fx.n_parts; ++g) {
        made[(size_t) g] = hnsw_new_index(c, expect, metric, m);
        vsr_hnsw* hh = made[(size_t) g].get();
        const vsr_hnsw* pr = fx.prior[(size_t) g];
        if (next >= n_graphs || fx.active[next] != g) {
            // nothing to insert: the prior graph as it is, unread -- so the copy is worth what the prior was worth (an empty one: nothing to doubt)
            if (const int rc = hnsw_clone_into(at, hh, pr)) return rc;
            made_here[(size_t) g] = pr ? pr->made_here : 1;
            continue;
        }
        const size_t i = next++, ne = (size_t) (fo.base[i + 1] - fo.base[i]);
        hh->n_elem = (int32_t) ne;
        hh->max_level = fo.max_level[i];
        hh->n_upper = fo.n_upper[i];
        const int32_t e = fo.plan.final_entry[i];
        hh->entry = (int32_t) (e - fo.base[i]);
        hh->entry_level = e >= fo.base[i] + fx.n_prior[i] ? fo.level[(size_t) e] : pr->entry_level;   // a new element took over / the prior entry stays
        if (const int rc = hnsw_index_arrays(at, hh)) return rc;
        graphs.push_back({hh->d_level, hh->d_elem_row, hh->d_nbr0, hh->d_up_slot, hh->d_up_nbr, hh->d_tid_count, hh->d_tids, (int32_t) fo.base[i],
                          (int32_t) ne, fo.slot_base[i], hh->max_level});
        HnswForestPrior fp{};
        if (pr) {
            fp.level = pr->d_level; fp.elem_row = pr->d_elem_row; fp.nbr0 = pr->d_nbr0; fp.up_slot = pr->d_up_slot; fp.up_nbr = pr->d_up_nbr;
            fp.tid_count = pr->d_tid_count; fp.tids = pr->d_tids;
            fp.n_elem = pr->n_elem; fp.n_upper = pr->n_upper; fp.max_level = pr->max_level;
        }
        priors.push_back(fp);
    }
    if (total > 0) {
        HnswForestSpace sp;
        int32_t* d_up_owner = nullptr;
        HnswForestGraph* d_graphs = nullptr;
        HnswForestPrior* d_priors = nullptr;
        unsigned long long* d_words = nullptr;                                // [0]: HnswForestJoin::held; [1]: bad (its low word)
        if (const int rc = hnsw_forest_space(at, c, expect, m, ef_construction, metric, fo, slots_io, sp)) return rc;
        HNSW_TRY(at.upload(&d_graphs, graphs.data(), graphs.size()));
        HNSW_TRY(at.upload(&d_priors, priors.data(), priors.size()));
        const unsigned long long words[2] = {~0ull, ~0ull};
        HNSW_TRY(at.upload(&d_words, words, 2));
        HNSW_TRY(at.alloc(&d_up_owner, sp.up_slots));
        HNSW_TRY(hipMemsetAsync(d_up_owner, 0xFF, sp.up_slots * 4, ctx->stream));

        // the prior graphs into the element space; what they say is read before anything is written through them
        HnswForestJoin jn{};
        jn.level = sp.level;
        jn.elem_row = sp.elem_row;
        jn.up_slot = sp.up_slot;
        jn.up_owner = d_up_owner;
        jn.n_rows = (uint32_t) c->n;
        jn.held = d_words;
        jn.bad = reinterpret_cast<uint32_t*>(d_words + 1);
        HNSW_TRY(vsr_hnsw_forest_join(sp.bp, jn, d_graphs, d_priors, (uint32_t) graphs.size(), (uint32_t) total, ctx->stream));
        HNSW_TRY(hipStreamSynchronize(ctx->stream));
        unsigned long long got[2] = {~0ull, ~0ull};
        HNSW_TRY(hipMemcpy(got, d_words, sizeof got, hipMemcpyDeviceToHost));
        if ((uint32_t) got[1] != 0xFFFFFFFFu) {
            const size_t i = (size_t) (uint32_t) got[1];
            return fail(VSR_ERR_INVALID, "%s: partition %d: the prior index holds a level, row, upper slot or neighbour outside its range", who,
                        i < n_graphs ? fx.active[i] : -1);
        }
        if (got[0] != ~0ull) {
            const size_t i = (size_t) (got[0] >> 32), r = (size_t) (got[0] & 0xFFFFFFFFull);
            if (i < n_graphs && r < (size_t) c->n)
                return fail(VSR_ERR_INVALID, "%s: partition %d: new row %lld is under a heap TID of the prior graph already", who, fx.active[i],
                            (long long) c->h_orig[r]);
            return fail(VSR_ERR_INVALID, "%s: a new row is under a heap TID of a prior graph already", who);
        }
        // the distance of every prior edge (the new elements' lists are empty and return at once), then the rounds
        HNSW_TRY(vsr_hnsw_edge_distances(sp.bp, (uint32_t) total, d_up_owner, (uint32_t) fo.g_upper, ctx->stream));
        if (const int rc = hnsw_forest_rounds(at, fo, sp)) return rc;
        HNSW_TRY(vsr_hnsw_forest_split_carry(sp.bp, d_graphs, d_priors, (uint32_t) graphs.size(), (uint32_t) total, ctx->stream));
    }
    HNSW_TRY(hipStreamSynchronize(ctx->stream));
    if (total > 0) {
        HNSW_TRY(hnsw_take_guard(ctx->err_word(), guard));                    // the build's rule: never a thinner graph
        if (*guard) return VSR_OK;
    }
    at.free_all();
    for (int g = 0; g < fx.n_parts; ++g) out[g] = hnsw_register(std::move(made[(size_t) g]), made_here[(size_t) g]);
    return VSR_OK;
}

// a prior index this library did not make: its arrays to the host and through vsr_hnsw_extend's checks, before anything is launched
static int hnsw_forest_check_prior(const vsr_corpus* c, const vsr_hnsw* h, int g, const char* who)
{
    const size_t ne = (size_t) h->n_elem, m = (size_t) h->m, up = (size_t) std::max(h->n_upper, 0) * (size_t) std::max(h->max_level, 1) * m;
    std::vector<int32_t> level(ne), nbr0(ne * 2 * m), tid_count(ne), up_slot(ne), up_nbr(std::max<size_t>(up, 1)), itids(ne * 10);
    std::vector<int64_t> tids(ne * 10, -1);
    HIPCHK(hipMemcpy(level.data(), h->d_level, ne * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nbr0.data(), h->d_nbr0, ne * 2 * m * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tid_count.data(), h->d_tid_count, ne * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(up_slot.data(), h->d_up_slot, ne * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(itids.data(), h->d_tids, ne * 10 * 4, hipMemcpyDeviceToHost));
    if (up > 0) HIPCHK(hipMemcpy(up_nbr.data(), h->d_up_nbr, up * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ne * 10; ++i)                                      // internal rows -> the caller's row indices
        if (itids[i] >= 0 && (int64_t) itids[i] < c->n) tids[i] = c->h_orig[(size_t) itids[i]];
    char name[96];
    snprintf(name, sizeof name, "%s: partition %d: the prior index", who, g);
    const HnswGraphView view{h->m, h->n_elem, h->entry, level.data(), nbr0.data(), tid_count.data(), tids.data(), up_slot.data(),
                             up_nbr.data(), h->n_upper, h->max_level};
    HnswPrior pr;
    return hnsw_extend_prepare(c, view, pr, name);
}

extern "C" int vsr_hnsw_extend_partitions(vsr_corpus* c, int n_parts, vsr_hnsw* const* prior, const int64_t* new_off, const int64_t* new_rows,
                                          int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out)
{
    const char* who = "vsr_hnsw_extend_partitions";
    if (out)
        for (int g = 0; g < n_parts; ++g) out[g] = nullptr;
    if (!c || n_parts < 0 || (n_parts > 0 && (!out || !new_off || !prior))) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    const RowFormat expect = c->format;
    if (expect == RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED,
                    "%s: a sparsevec corpus is not supported (the sparse build has no element -> row form): rebuild every partition's graph with "
                    "vsr_hnsw_build_sparse over a corpus of its rows", who);
    if (flags & VSR_HNSW_BUILD_MERGE_DUPLICATES)
        return fail(VSR_ERR_UNSUPPORTED, "%s: VSR_HNSW_BUILD_MERGE_DUPLICATES is not supported: an inserted row is never folded into an existing element", who);
    if (flags) return fail(VSR_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (c->base) return fail(VSR_ERR_INVALID, "%s: the corpus is a view", who);
    long cap = HB_BATCH_MAX;
    if (const int rc = hnsw_env_int(who, "VSR_HNSW_FOREST_BATCH", 1, (long) HB_BATCH_MAX, false, "a number from", "to", &cap)) return rc;
    uint32_t slots = 0;
    if (const int rc = hnsw_env_visited_slots(who, &slots)) return rc;
    if (n_parts == 0) return VSR_OK;
    // m is the priors': the call has no m of its own, so at least one prior index must be there to say it
    int m = 0;
    for (int g = 0; g < n_parts; ++g) {
        const vsr_hnsw* h = prior[g];
        if (!h) continue;
        if (h->corpus != c) return fail(VSR_ERR_INVALID, "%s: partition %d: the prior index is over another corpus", who, g);
        if (h->format != expect) return fail(VSR_ERR_INVALID, "%s: partition %d: the prior index is of another row format than the corpus", who, g);
        if (m == 0) m = h->m;
        if (h->m != m) return fail(VSR_ERR_INVALID, "%s: partition %d: the prior index has m = %d, the ones before it m = %d", who, g, h->m, m);
        if (expect == RowFormat::BIT && h->bit_metric != metric)
            return fail(VSR_ERR_INVALID, "%s: partition %d: the prior index's opclass is metric %d, not %d", who, g, h->bit_metric, metric);
    }
    if (m == 0)
        return fail(VSR_ERR_INVALID, "%s: every prior index is NULL, so m is not known: build the graphs with vsr_hnsw_build_partitions", who);
    vsr_hnsw* none = nullptr;
    if (const int rc = hnsw_build_check(c, expect, m, ef_construction, metric, flags, &none, who)) return rc;
    if (c->n > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);
    std::vector<int32_t> fresh;                                               // the new rows as internal rows, a partition's ascending
    if (const int rc = hnsw_partition_rows(c, n_parts, new_off, new_rows, "new_off", who, fresh)) return rc;
    HIPCHK(hipSetDevice(c->ctx->device));
    // per prior index, once however many partitions name it: the checks of one this library did not make, and n0, its heap TIDs
    HnswForestExtend fx;
    fx.n_parts = n_parts;
    HnswForest& fo = fx.fo;
    fx.prior.assign((size_t) n_parts, nullptr);
    std::map<const vsr_hnsw*, int64_t> n0_of;
    std::vector<int32_t> counts;
    int64_t most_draws = 0;
    for (int g = 0; g < n_parts; ++g) {
        const vsr_hnsw* h = prior[g];
        if (!h || h->n_elem <= 0) continue;
        fx.prior[(size_t) g] = h;
        const int64_t n_new = new_off[g + 1] - new_off[g];
        if (n_new == 0) continue;                                             // copied as it is: nothing is written through it
        auto it = n0_of.find(h);
        if (it == n0_of.end()) {
            if (!h->made_here)
                if (const int rc = hnsw_forest_check_prior(c, h, g, who)) return rc;
            counts.resize((size_t) h->n_elem);
            HIPCHK(hipMemcpy(counts.data(), h->d_tid_count, (size_t) h->n_elem * 4, hipMemcpyDeviceToHost));
            int64_t n0 = 0;
            for (int32_t t : counts) n0 += std::min(std::max(t, 0), (int32_t) HB_TIDS);
            it = n0_of.emplace(h, n0).first;
        }
        most_draws = std::max(most_draws, it->second + n_new);
    }
    for (int g = 0; g < n_parts; ++g)
        if (!fx.prior[(size_t) g]) most_draws = std::max(most_draws, new_off[g + 1] - new_off[g]);
    // levels: the build's stream, drawn once as far as any partition reaches; the i-th new row of a graph takes draw n0 + i
    HnswLevelStream stream(seed, m);
    std::vector<int32_t> draws((size_t) most_draws);
    for (int32_t& d : draws) d = stream.level();

    fo.base.assign(1, 0);
    std::vector<int64_t> start_done;
    std::vector<int32_t> start_entry, start_entry_level;
    for (int g = 0; g < n_parts; ++g) {
        const int64_t n_new = new_off[g + 1] - new_off[g];
        if (n_new == 0) continue;
        const vsr_hnsw* h = fx.prior[(size_t) g];
        const int64_t np = h ? h->n_elem : 0, b = fo.base.back();
        if (b + np + n_new > 0x7FFFFFF0ll) return fail(VSR_ERR_UNSUPPORTED, "%s: too many elements", who);
        if (h && (h->entry < 0 || h->entry >= h->n_elem || h->max_level < 1 || h->n_upper < 0))
            return fail(VSR_ERR_INVALID, "%s: partition %d: bad graph arrays", who, g);
        fx.active.push_back(g);
        fx.n_prior.push_back(np);
        fo.base.push_back(b + np + n_new);
        start_done.push_back(np);
        start_entry.push_back(h ? (int32_t) (b + h->entry) : -1);
        start_entry_level.push_back(h ? h->entry_level : -1);
        fo.elem_row.resize((size_t) (b + np + n_new), 0);
        fo.level.resize((size_t) (b + np + n_new), 0);
        fo.up_slot.resize((size_t) (b + np + n_new), -1);
        int32_t n_upper = h ? h->n_upper : 0, max_level = h ? h->max_level : 1;
        fo.slot_base.push_back(fo.g_upper);
        const int64_t n0 = h ? n0_of[h] : 0;
        for (int64_t i = 0; i < n_new; ++i) {
            const size_t e = (size_t) (b + np + i);
            fo.elem_row[e] = fresh[(size_t) (new_off[g] + i)];
            fo.level[e] = draws[(size_t) (n0 + i)];
            if (fo.level[e] >= 1) {
                fo.up_slot[e] = fo.g_upper + n_upper++;                       // new upper slots continue after the prior ones
                max_level = std::max(max_level, fo.level[e]);
            }
        }
        fo.n_upper.push_back(n_upper);
        fo.max_level.push_back(max_level);
        fo.g_upper += n_upper;
        fo.g_max_level = std::max(fo.g_max_level, max_level);
    }
    fo.n_parts = (int) fx.active.size();
    if (!hnsw_forest_plan_from((int) fx.active.size(), fo.base.data(), fo.level.data(), m, (uint32_t) cap, start_done.data(), start_entry.data(),
                               start_entry_level.data(), fo.plan))
        return fail(VSR_ERR_UNSUPPORTED, "%s: a round with m = %d has too many reverse edges", who, m);
    // every attempt starts again from the priors, which no attempt has changed
    return hnsw_forest_ladder(m, ef_construction, slots, who, [&](uint32_t* slots_io, uint32_t* guard) {
        return hnsw_forest_extend_once(c, expect, m, ef_construction, metric, fx, slots_io, guard, out, who);
    });
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

// One attempt with `slots` visited-table entries and `caps` candidate entries, from the caller's arrays.  *guard: as hnsw_build_once.
// Its own: the entry phase, the repair list and the compaction
static int hnsw_vacuum_once(vsr_corpus* c, RowFormat expect, int m, int ef_construction, int metric, const HnswPrior& pr, const HnswVacuumPlan& pl,
                            uint32_t slots, uint32_t caps, uint32_t batch_max, const HnswVacuumSpill& sp, uint32_t* guard,
                            vsr_hnsw_vacuum_stats* st, int32_t* out_elem_map, vsr_hnsw** out, const char* who)
{
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t ne = (size_t) pr.n_elem, lm0 = (size_t) 2 * m;
    const int32_t max_level = pr.max_level;
    const size_t n_up = (size_t) std::max(pr.n_upper, 1), up_words = n_up * max_level * m;
    HnswOwner h = hnsw_new_index(c, expect, metric, m);
    HnswAttempt at(ctx, who);                                                 // everything but the result's arrays
    int32_t *w_level, *w_nbr0, *w_up_slot, *w_up_nbr, *w_live, *w_elem_row = nullptr, *w_up_owner, *w_list, *w_num, *w_map, *w_slot_map, *w_stage_n;
    float *w_dist0, *w_up_dist, *w_stage_d;
    uint8_t* w_flag;
    HNSW_TRY(at.upload(&w_level, pr.level, ne));
    HNSW_TRY(at.upload(&w_nbr0, pr.nbr0, ne * lm0));
    HNSW_TRY(at.upload(&w_up_slot, pr.up_slot, ne));
    HNSW_TRY(at.upload(&w_live, pl.live.data(), ne));
    if (!pl.identity) HNSW_TRY(at.upload(&w_elem_row, pr.elem_row.data(), ne));   // a deleted element keeps its row for the whole repair
    HNSW_TRY(at.alloc(&w_up_nbr, up_words));
    HNSW_TRY(at.alloc(&w_dist0, ne * lm0));
    HNSW_TRY(at.alloc(&w_up_dist, up_words));
    HNSW_TRY(at.alloc(&w_up_owner, n_up));
    HNSW_TRY(at.alloc(&w_list, ne));
    HNSW_TRY(at.alloc(&w_num, 4));                                            // [0]: the repair list's length; [1], [2]: batches of one
    HNSW_TRY(at.alloc(&w_map, ne));
    HNSW_TRY(at.alloc(&w_slot_map, n_up));
    HNSW_TRY(at.alloc(&w_flag, ne));
    HNSW_TRY(hipMemsetAsync(w_up_nbr, 0xFF, up_words * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(w_dist0, 0, ne * lm0 * 4, ctx->stream));
    HNSW_TRY(hipMemsetAsync(w_up_dist, 0, up_words * 4, ctx->stream));
    HNSW_TRY(hipStreamSynchronize(ctx->stream));                              // the copies below are not on the stream
    if (pr.n_upper > 0) {
        HNSW_TRY(hipMemcpy(w_up_nbr, pr.up_nbr, (size_t) pr.n_upper * max_level * m * 4, hipMemcpyHostToDevice));
        HNSW_TRY(hipMemcpy(w_up_owner, pr.up_owner.data(), (size_t) pr.n_upper * 4, hipMemcpyHostToDevice));
    }

    HnswBuildParams bp{};
    hnsw_row_params(bp, c, expect, metric);
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
    const HnswLadder ladder{true, 0, sp.lds_budget};
    if (!hnsw_lds_params(bp, ladder)) return fail(VSR_ERR_UNSUPPORTED, "%s: %u candidates with a visited table of %u entries do not fit the LDS", who, caps, slots);
    bp.err = ctx->err_word();

    HnswVacuumParams vp{};
    const uint32_t stride = (uint32_t) hnsw_rec_cap(m, max_level);
    const uint64_t most = std::min<uint64_t>(batch_max, (uint64_t) std::max(pl.n_live, 1));
    if (most * stride > 0x7FFFFFFFull) return fail(VSR_ERR_UNSUPPORTED, "%s: a batch of %llu elements with m = %d has too many reverse edges", who, (unsigned long long) most, m);
    HnswRecScratch rs;                                                        // tmp also serves the compaction and the scans
    HNSW_TRY(hnsw_rec_scratch(at, {(uint32_t) (most * stride), stride}, std::max<size_t>(vsr_hnsw_vacuum_tmp_bytes((uint32_t) ne), 256), &rs));
    HNSW_TRY(at.alloc(&w_stage_n, (size_t) rs.rec_cap_max));
    HNSW_TRY(at.alloc(&w_stage_d, (size_t) rs.rec_cap_max));
    bp.rec_count = rs.cnt;
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
        HNSW_TRY(hipMemGetInfo(&free_b, &total_b));
        const uint64_t pool = std::max<uint64_t>(1, std::min<uint64_t>({most, (uint64_t) sp.waves, (uint64_t) (free_b / 4 / ws_bytes)}));
        uint32_t* w_spill;
        HNSW_TRY(at.alloc(&w_spill, 4));                                      // [0]: the batch's spill count, [1]: the call's total
        HNSW_TRY(hipMemsetAsync(w_spill, 0, 16, ctx->stream));
        HNSW_TRY(at.alloc(&vp.spill_ws, (size_t) pool * ws_bytes));
        vp.spill_ws_bytes = ws_bytes;
        vp.spill_pool = (uint32_t) pool;
        vp.spill_n = (uint32_t) ne;
        vp.spill_total = w_spill + 1;
        if (sp.mode == HV_SPILL_ALL) {
            vp.spill_all = 1;
        } else {
            vp.spill_count = w_spill;
            HNSW_TRY(at.alloc(&vp.spill_list, (size_t) most));
        }
        ws_total = (int64_t) (pool * ws_bytes);
    }

    HNSW_TRY(vsr_hnsw_edge_distances(bp, (uint32_t) ne, w_up_owner, (uint32_t) pr.n_upper, ctx->stream));
    int32_t nrep = 0, nbatch = 0;
    // one repair batch: `count` elements at d_elems, searched from element `from` (-1: nobody is left, the lists become empty)
    auto run_batch = [&](const int32_t* d_elems, uint32_t count, uint32_t rec_cap, int32_t from) -> hipError_t {
        bp.entry = from;
        bp.entry_level = from >= 0 ? pr.level[from] : -1;
        bp.first = 0;
        bp.count = count;
        bp.rec_cap = rec_cap;
        bp.rec_key = rs.key[0];
        bp.rec_val = rs.val[0];
        vp.elems = d_elems;
        nrep += (int32_t) count;
        ++nbatch;
        return vsr_hnsw_vacuum_batch(bp, vp, rs.tmp, rs.tmp_bytes, rs.key[1], rs.val[1], ctx->stream);
    };
    auto rec_cap_of = [&](int32_t e) { return (uint32_t) hnsw_rec_cap(m, pr.level[e]); };
    // NeedsUpdated of one element, on the graph as the stream leaves it
    auto needs = [&](int32_t e, bool* yes) -> hipError_t {
        hipError_t e_ = vsr_hnsw_vacuum_mark(bp, w_live, (uint32_t) ne, -1, w_flag, nullptr, nullptr, rs.tmp, rs.tmp_bytes, ctx->stream);
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
    HNSW_TRY(hipMemcpy(w_num + 1, ones, sizeof ones, hipMemcpyHostToDevice));
    if (hp >= 0) {
        bool yes = false;
        HNSW_TRY(needs(hp, &yes));
        if (yes) HNSW_TRY(run_batch(w_num + 1, 1, rec_cap_of(hp), entry));    // from the entry as it is, deleted or not
    }
    if (pl.live[(size_t) entry] == 0) {
        entry = hp;
    } else {
        bool yes = false;
        HNSW_TRY(needs(entry, &yes));
        if (yes) HNSW_TRY(run_batch(w_num + 2, 1, rec_cap_of(entry), hp));
    }
    // the main phase: the repair list once, after the entry phase
    HNSW_TRY(vsr_hnsw_vacuum_mark(bp, w_live, (uint32_t) ne, entry, w_flag, w_list, w_num, rs.tmp, rs.tmp_bytes, ctx->stream));
    HNSW_TRY(hipStreamSynchronize(ctx->stream));
    int32_t n_list = 0;
    HNSW_TRY(hipMemcpy(&n_list, w_num, 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> list((size_t) std::max(n_list, 1));
    if (n_list > 0) HNSW_TRY(hipMemcpy(list.data(), w_list, (size_t) n_list * 4, hipMemcpyDeviceToHost));
    // the guard word after the entry phase and after every batch: an attempt whose arrays are too short ends where that shows
    HNSW_TRY(hnsw_take_guard(bp.err, guard));
    for (int32_t done = 0; done < n_list && !*guard;) {
        const uint32_t b = (uint32_t) std::min<int64_t>(batch_max, n_list - done);
        uint64_t cap = 0;
        for (uint32_t i = 0; i < b; ++i) cap += rec_cap_of(list[(size_t) done + i]);
        HNSW_TRY(run_batch(w_list + done, b, (uint32_t) cap, entry));         // (cap <= rec_cap_max: b <= most, a level <= max_level)
        done += (int32_t) b;
        HNSW_TRY(hipStreamSynchronize(ctx->stream));
        HNSW_TRY(hnsw_take_guard(bp.err, guard));
    }
    if (*guard) return VSR_OK;

    // pass 3: the compacted index.  Elements in ascending old id, upper slots in ascending old slot, the upper arrays at the new top
    std::vector<int32_t> map(ne, -1), slot_map(n_up, -1);
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
    HNSW_TRY(hipMemcpy(w_slot_map, slot_map.data(), slot_map.size() * 4, hipMemcpyHostToDevice));
    HNSW_TRY(hipMalloc(&h->d_nbr0, std::max<size_t>(nn * lm0 * 4, 4)));
    HNSW_TRY(hipMalloc(&h->d_up_nbr, new_up_words * 4));
    HNSW_TRY(hipMemsetAsync(h->d_nbr0, 0xFF, std::max<size_t>(nn * lm0 * 4, 4), ctx->stream));
    HNSW_TRY(hipMemsetAsync(h->d_up_nbr, 0xFF, new_up_words * 4, ctx->stream));
    HNSW_TRY(vsr_hnsw_vacuum_renumber(bp, w_live, w_map, w_slot_map, (uint32_t) ne, h->d_nbr0, h->d_up_nbr, (uint32_t) new_max_level, rs.tmp,
                                      rs.tmp_bytes, ctx->stream));
    HNSW_TRY(hipStreamSynchronize(ctx->stream));
    HNSW_TRY(hnsw_take_guard(bp.err, guard));                                 // (HB_ERR_RECORDS: a live list still named a deleted element)
    if (*guard) return VSR_OK;
    if (vp.spill_total) {
        uint32_t spilled = 0;
        HNSW_TRY(hipMemcpy(&spilled, vp.spill_total, sizeof spilled, hipMemcpyDeviceToHost));
        h->vacuum_spilled = (int32_t) spilled;
        h->vacuum_ws_bytes = ws_total;
    }
    // the device's scan and the host's must agree: the lists were renumbered by the one, the other arrays by the other
    std::vector<int32_t> dmap(ne);
    HNSW_TRY(hipMemcpy(dmap.data(), w_map, ne * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < ne; ++e)
        if (pl.live[e] && dmap[e] != map[e]) return fail(VSR_ERR_HIP, "%s: the element scan disagrees at element %zu", who, e);
    at.free_all();
    int rc = VSR_OK;
    if ((rc = upload_i32(&h->d_elem_row, erow.data(), nn)) || (rc = upload_i32(&h->d_level, level.data(), nn)) ||
        (rc = upload_i32(&h->d_up_slot, up_slot.data(), nn)) || (rc = upload_i32(&h->d_tid_count, tcount.data(), nn)) ||
        (rc = upload_i32(&h->d_tids, itids.data(), nn * 10)))
        return rc;
    if (out_elem_map) std::copy(map.begin(), map.end(), out_elem_map);
    if (st) {
        st->elements_repaired = nrep;
        st->batches = nbatch;
    }
    *out = hnsw_register(std::move(h), 1);
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
    const HnswGraphView g{m, n_elem, entry, level, nbr0, tid_count, tids, up_slot, up_nbr, n_upper, max_level};
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
    rc = hnsw_extend_prepare(c, g, pr, who);
    if (rc) return rc;
    vsr_hnsw_vacuum_stats st{};
    const int bit_metric = expect == RowFormat::BIT ? metric : 0;
    if (n_dead == 0 || n_elem == 0) {                                         // nothing to delete: the graph as it is
        st.tuples_kept = pr.n0;
        for (int32_t e = 0; out_elem_map && e < n_elem; ++e) out_elem_map[e] = e;
        if (out_stats) *out_stats = st;
        return hnsw_load(c, expect, bit_metric, g, out, who);
    }
    // pass 1
    const size_t ne = (size_t) n_elem;
    HnswVacuumPlan pl;
    {
        const std::vector<int32_t> inv = hnsw_row_map(c);
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
        return hnsw_load(c, expect, bit_metric, HnswGraphView{m}, out, who);
    }
    // the knobs and the initial sizes.  Candidates: what the build holds, ef_construction + 1 + 2 m, over the live share, since
    // W holds every deleted element met on the way to ef live ones; the result does not depend on it (HB_ERR_CANDIDATES)
    uint32_t slots = 0;
    if ((rc = hnsw_env_visited_slots(who, &slots))) return rc;
    const bool slots_given = slots != 0;
    if (slots == 0) slots = hnsw_default_visited_slots(ef_construction, m);
    auto env_int = [&](const char* name, long lo, long hi, long* v) { return hnsw_env_int(who, name, lo, hi, false, "between", "and", v); };
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
    long v = 0;
    if ((rc = env_int("VSR_HNSW_VACUUM_CAPS", (long) caps_min, 1L << 20, &v))) return rc;
    uint32_t caps;
    if (v > 0) {
        caps = (uint32_t) v;
    } else {
        const uint64_t base = (uint64_t) ef_construction + 1u + 2u * (uint64_t) m;
        const uint64_t want = std::min<uint64_t>((base * (uint64_t) n_elem + (uint64_t) pl.n_live - 1) / (uint64_t) pl.n_live, (uint64_t) n_elem);
        caps = (uint32_t) std::max<uint64_t>(base, std::min<uint64_t>((want + 15) & ~15ull, hnsw_vacuum_caps_fit(budget, slots)));
        if (lds > 0 && hnsw_vacuum_lds_per_wave(caps, slots) > budget) caps = std::max(caps_min, hnsw_vacuum_caps_fit(budget, slots));   // (a given budget below `base`)
    }
    // every candidate was visited first, so a table that fills at 3/4 should hold what the candidate array is sized for
    while (!slots_given && v == 0 && slots < HB_SLOTS_MAX && (uint64_t) slots * 3u < (uint64_t) caps * 4u && hnsw_vacuum_lds_per_wave(caps, slots * 2u) <= budget)
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
    const char* rebuild = "a graph this dead is to be rebuilt over its live rows (vsr_hnsw_build*)";
    HnswLadder ladder{true, 0, budget};
    for (;;) {
        uint32_t guard = 0;
        ++st.attempts;
        rc = hnsw_vacuum_once(c, expect, m, ef_construction, metric, pr, pl, slots, caps, (uint32_t) batch, sp, &guard, &st, out_elem_map, out, who);
        if (rc != VSR_OK || guard == 0) {
            if (rc == VSR_OK && out_stats) *out_stats = st;
            return rc;
        }
        ladder.caps_ceiling = hnsw_vacuum_caps_fit(budget, slots);
        switch (hnsw_ladder_step(ladder, guard, &caps, &slots)) {
        case HB_LADDER_ON: break;
        case HB_LADDER_RECORDS:
            return fail(VSR_ERR_UNSUPPORTED, "%s: the repair at ef_construction = %d with m = %d dropped reverse edges or left a list that names a "
                        "deleted element: the graph would be incomplete", who, ef_construction, m);
        case HB_LADDER_CANDIDATES:
            if (go_mixed()) break;
            return fail(VSR_ERR_UNSUPPORTED, "%s: a layer search of the repair holds more than %u candidates (%d of %d elements live) and no longer "
                        "candidate array fits the LDS: %s", who, caps, pl.n_live, n_elem, rebuild);
        case HB_LADDER_VISITED:
            if (go_mixed()) break;
            return fail(VSR_ERR_UNSUPPORTED, "%s: a layer search of the repair fills its visited table of %u entries (%d of %d elements live) and no "
                        "larger one fits the LDS: %s", who, slots, pl.n_live, n_elem, rebuild);
        }
    }
}

extern "C" int vsr_hnsw_vacuum_spill_info(const vsr_hnsw* h, int32_t* spilled_repairs, int64_t* workspace_bytes)
{
    if (!h) return fail(VSR_ERR_INVALID, "vsr_hnsw_vacuum_spill_info: index is NULL");
    if (spilled_repairs) *spilled_repairs = h->vacuum_spilled;
    if (workspace_bytes) *workspace_bytes = h->vacuum_ws_bytes;
    return VSR_OK;
}
