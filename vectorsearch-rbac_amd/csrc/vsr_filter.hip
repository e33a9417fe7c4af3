// vsr_filter.hip — who may see which rows: the RBAC tables of a corpus, row ranges as tiles and bitmaps, permission classes,
// and every vsr_filter_* entry point.
#include "vsr_runtime.h"

// index-side caches derived from filters: drop what belongs to `f` (nullptr: everything)
static void purge_index_caches(vsr_corpus* c, const vsr_filter* f)
{
    purge_ivf_caches(c, f);
    purge_hnsw_caches(c, f);
}

// ---- RBAC
void vsr::drop_cached_filters(vsr_corpus* c)
{
    purge_index_caches(c, nullptr);                  // the indexes' view-order bitmaps and probe parts of every filter
    c->class_view.reset();                           // (its order is the classes')
    for (vsr_filter* f : c->class_filters) free_filter(f);
    c->class_filters.clear();
    for (vsr_filter* f : c->class_bitmap_filters) free_filter(f);
    c->class_bitmap_filters.clear();
    c->class_sig.clear();
    c->doc_class.clear();
    for (auto& kv : c->cache) free_filter(kv.second);
    c->cache.clear();
}

static void build_class_view(vsr_corpus* c);

extern "C" int vsr_rbac_load(vsr_corpus* c, const int32_t* ur_user, const int32_t* ur_role, int64_t n_ur,
                             const int32_t* pa_role, const int32_t* pa_doc, int64_t n_pa)
{
    if (!c) return fail(VSR_ERR_INVALID, "vsr_rbac_load: corpus is NULL");
    if ((n_ur > 0 && (!ur_user || !ur_role)) || (n_pa > 0 && (!pa_role || !pa_doc)) || n_ur < 0 || n_pa < 0)
        return fail(VSR_ERR_INVALID, "vsr_rbac_load: NULL table");
    HIPCHK(hipSetDevice(c->ctx->device));
    HIPCHK(hipStreamSynchronize(c->ctx->stream));
    drop_cached_filters(c);

    c->roles.clear();
    for (int64_t i = 0; i < n_ur; ++i) c->roles.push_back(ur_role[i]);
    for (int64_t i = 0; i < n_pa; ++i) c->roles.push_back(pa_role[i]);
    std::sort(c->roles.begin(), c->roles.end());
    c->roles.erase(std::unique(c->roles.begin(), c->roles.end()), c->roles.end());
    c->words = (uint32_t) std::max<size_t>(1, (c->roles.size() + 63) / 64);

    c->user_roles.clear();
    for (int64_t i = 0; i < n_ur; ++i) c->user_roles[ur_user[i]].push_back(ur_role[i]);
    for (auto& kv : c->user_roles) {
        std::sort(kv.second.begin(), kv.second.end());
        kv.second.erase(std::unique(kv.second.begin(), kv.second.end()), kv.second.end());
    }

    c->doc_mask.assign(c->docs.size() * c->words, 0);
    for (int64_t i = 0; i < n_pa; ++i) {
        auto d = std::lower_bound(c->docs.begin(), c->docs.end(), pa_doc[i]);
        if (d == c->docs.end() || *d != pa_doc[i]) continue;     // permission on a document with no rows here
        const size_t di = (size_t) (d - c->docs.begin());
        const size_t ri = (size_t) (std::lower_bound(c->roles.begin(), c->roles.end(), pa_role[i]) - c->roles.begin());
        c->doc_mask[di * c->words + ri / 64] |= 1ull << (ri % 64);
    }
    if (c->d_doc_mask) (void) hipFree(c->d_doc_mask);
    c->d_doc_mask = nullptr;
    const size_t bytes = std::max<size_t>(8, c->doc_mask.size() * sizeof(uint64_t));
    HIPCHK(hipMalloc(&c->d_doc_mask, bytes));
    if (!c->doc_mask.empty())
        HIPCHK(hipMemcpy(c->d_doc_mask, c->doc_mask.data(), c->doc_mask.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    // permission classes = distinct role signatures of the documents
    {
        std::map<std::vector<uint64_t>, uint32_t> ids;
        c->doc_class.assign(c->docs.size(), 0);
        std::vector<uint64_t> sig(c->words);
        for (size_t di = 0; di < c->docs.size(); ++di) {
            std::copy(c->doc_mask.begin() + (long) (di * c->words), c->doc_mask.begin() + (long) ((di + 1) * c->words), sig.begin());
            auto it = ids.find(sig);
            if (it == ids.end()) {
                it = ids.emplace(sig, (uint32_t) c->class_sig.size()).first;
                c->class_sig.push_back(sig);
            }
            c->doc_class[di] = it->second;
        }
        c->class_filters.assign(c->class_sig.size(), nullptr);
        c->class_bitmap_filters.assign(c->class_sig.size(), nullptr);
        if (c->d_doc_class) (void) hipFree(c->d_doc_class);
        c->d_doc_class = nullptr;
        HIPCHK(hipMalloc(&c->d_doc_class, std::max<size_t>(4, c->doc_class.size() * sizeof(uint32_t))));
        if (!c->doc_class.empty())
            HIPCHK(hipMemcpy(c->d_doc_class, c->doc_class.data(), c->doc_class.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    c->rbac = true;
    build_class_view(c);
    return VSR_OK;
}

// ---- filters
int vsr::upload_tiles(vsr_filter* f, const std::vector<uint2>& tiles)
{
    f->n_tiles = (uint32_t) tiles.size();
    if (tiles.empty()) return VSR_OK;
    HIPCHK(hipMalloc(&f->d_tiles, tiles.size() * sizeof(uint2)));
    HIPCHK(hipMemcpy(f->d_tiles, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return VSR_OK;
}

// contiguous permitted row ranges -> the RW-aligned row windows that hold at least one permitted row
// (bitmap mode: the per-row bits decide inside each window; windows without a set bit are never visited)
static int64_t ranges_to_aligned_tiles(const std::vector<std::pair<uint32_t, uint32_t>>& ranges, int rw, int64_t n,
                                       std::vector<uint2>& tiles)
{
    int64_t rows = 0;
    int64_t last = -1;
    for (auto& r : ranges)
        for (int64_t t = r.first / rw; t <= (int64_t) (r.second - 1) / rw; ++t) {
            if (t == last) continue;
            last = t;
            const uint32_t s = (uint32_t) (t * rw);
            const uint32_t cnt = (uint32_t) std::min<int64_t>(rw, n - (int64_t) s);
            tiles.push_back(make_uint2(s, cnt));
            rows += cnt;
        }
    return rows;
}

// contiguous permitted row ranges -> tiles of <= RW rows
void vsr::ranges_to_tiles(const std::vector<std::pair<uint32_t, uint32_t>>& ranges, int rw, std::vector<uint2>& tiles)
{
    for (auto& r : ranges)
        for (uint32_t s = r.first; s < r.second; s += (uint32_t) rw)
            tiles.push_back(make_uint2(s, std::min<uint32_t>((uint32_t) rw, r.second - s)));
}

static int alloc_bitmap(vsr_filter* f)
{
    const size_t bytes = bitmap_words(f->corpus->n) * sizeof(uint64_t);
    HIPCHK(hipMalloc(&f->d_bitmap, bytes));
    HIPCHK(hipMemsetAsync(f->d_bitmap, 0, bytes, f->corpus->ctx->stream));
    f->owns_bitmap = true;
    return VSR_OK;
}

FilterPtr vsr::new_filter(vsr_corpus* c, int mode, bool cached)
{
    FilterPtr f(new vsr_filter(), free_filter);
    f->corpus = c;
    f->mode = mode;
    f->cached = cached;
    return f;
}

void vsr::free_filter(vsr_filter* f)
{
    if (!f) return;
    if (f->d_tiles) (void) hipFree(f->d_tiles);
    if (f->d_bitmap && f->owns_bitmap) (void) hipFree(f->d_bitmap);
    delete f;
}

static std::vector<uint64_t> role_mask(const vsr_corpus* c, const std::vector<int32_t>& roles)
{
    std::vector<uint64_t> m(c->words, 0);
    for (int32_t r : roles) {
        auto it = std::lower_bound(c->roles.begin(), c->roles.end(), r);
        if (it == c->roles.end() || *it != r) continue;
        const size_t ri = (size_t) (it - c->roles.begin());
        m[ri / 64] |= 1ull << (ri % 64);
    }
    return m;
}

static const std::vector<int32_t>& roles_of_user(const vsr_corpus* c, int32_t user_id)
{
    static const std::vector<int32_t> none;                // unknown user: sees nothing
    auto it = c->user_roles.find(user_id);
    return it == c->user_roles.end() ? none : it->second;
}

static bool doc_allowed(const vsr_corpus* c, size_t di, const std::vector<uint64_t>& m)
{
    for (uint32_t w = 0; w < c->words; ++w)
        if (c->doc_mask[di * c->words + w] & m[w]) return true;
    return false;
}

using Ranges = std::vector<std::pair<uint32_t, uint32_t>>;

static void append_range(Ranges& ranges, uint32_t s, uint32_t e)       // [s, e), merged with the last range where they touch
{
    if (!ranges.empty() && ranges.back().second == s) ranges.back().second = e;
    else ranges.emplace_back(s, e);
}

// the rows of one permission class as contiguous ranges; returns their number
static int64_t class_ranges(const vsr_corpus* c, uint32_t cls, Ranges& ranges)
{
    int64_t rows = 0;
    for (size_t di = 0; di < c->docs.size(); ++di) {
        if (c->doc_class[di] != cls) continue;
        rows += c->doc_row_start[di + 1] - c->doc_row_start[di];
        append_range(ranges, c->doc_row_start[di], c->doc_row_start[di + 1]);
    }
    return rows;
}

static int upload_ranges(vsr_filter* f, const Ranges& ranges)            // as tiles of <= RW rows
{
    std::vector<uint2> tiles;
    ranges_to_tiles(ranges, f->corpus->shape.rw, tiles);
    return upload_tiles(f, tiles);
}

// ... as the RW-aligned windows that hold at least one of the rows (bitmap mode); sets the filter's scanned rows
static int upload_aligned_ranges(vsr_filter* f, const Ranges& ranges)
{
    std::vector<uint2> tiles;
    f->scanned_rows = ranges_to_aligned_tiles(ranges, f->corpus->shape.rw, f->corpus->n, tiles);
    return upload_tiles(f, tiles);
}

constexpr size_t MAX_CLASSES = 4096;        // beyond this (e.g. random RBAC: a signature per document) filters stay whole
constexpr size_t MAX_PARTS = 64;

// The class view of the int8 planes (ClassView, vsr_runtime.h), rebuilt whenever the classes are (vsr_rbac_load).  The
// corpus simply has none when it does not apply or cannot be allocated: every call is then planned on the base planes.
// The int8 planes and their norms once more (classes padded to 64 rows) plus 4.5 bytes per row of rank and tile list
// (10M x 128: 1.4 GB).
static void build_class_view(vsr_corpus* c)
{
    c->class_view.reset();
    vsr_ctx* ctx = c->ctx;
    const size_t n_cls = c->class_sig.size();
    if (!c->d_scr8 || !c->d_norm2_8 || c->base || ctx->no_class_view || c->shape.rw != 16 || c->n == 0 || n_cls == 0 ||
        n_cls > MAX_CLASSES)
        return;
    std::unique_ptr<ClassView> v(new ClassView());
    v->start.assign(n_cls, 0);
    v->rows.assign(n_cls, 0);
    for (size_t di = 0; di < c->docs.size(); ++di) v->rows[c->doc_class[di]] += c->doc_row_start[di + 1] - c->doc_row_start[di];
    uint64_t total = 0;
    for (size_t cls = 0; cls < n_cls; ++cls) {
        v->start[cls] = (uint32_t) total;
        total += align_up(v->rows[cls], 64);
        if (total >= 0xFFFFFF00ull) return;
    }
    v->n_rows = (uint32_t) total;
    // view row -> base row: documents in base order, each appended to its class; pads stay ~0u for the gather kernel
    std::vector<uint32_t> rank((size_t) total, 0xFFFFFFFFu), at(v->start);
    for (size_t di = 0; di < c->docs.size(); ++di) {
        uint32_t& p = at[c->doc_class[di]];
        for (uint32_t r = c->doc_row_start[di]; r < c->doc_row_start[di + 1]; ++r) rank[p++] = r;
    }
    // identity tile list; a tile counts only the rows of its class (the last one of a class fewer than 16, pad tiles none)
    std::vector<uint2> tiles((size_t) (total / 16));
    for (size_t cls = 0; cls < n_cls; ++cls)
        for (uint32_t o = 0; o < (uint32_t) align_up(v->rows[cls], 64); o += 16)
            tiles[(v->start[cls] + o) / 16] = make_uint2(v->start[cls] + o, o < v->rows[cls] ? std::min(16u, v->rows[cls] - o) : 0u);
    const size_t scr_bytes = ((size_t) total + 32) * 128, norm_bytes = ((size_t) total + 64) * sizeof(float);
    bool ok = hipSetDevice(ctx->device) == hipSuccess;
    ok = ok && hipMalloc(&v->d_scr8, scr_bytes) == hipSuccess;
    ok = ok && hipMalloc(&v->d_norm2_8, norm_bytes) == hipSuccess;
    ok = ok && hipMalloc(&v->d_rank, (size_t) total * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(&v->d_tiles, tiles.size() * sizeof(uint2)) == hipSuccess;
    ok = ok && hipMalloc(&v->d_walk_pos, 64) == hipSuccess;
    ok = ok && hipMemsetAsync(v->d_walk_pos, 0, 64, ctx->stream) == hipSuccess;
    ok = ok && hipMemcpy(v->d_rank, rank.data(), (size_t) total * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(v->d_tiles, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemsetAsync(reinterpret_cast<char*>(v->d_scr8) + (size_t) total * 128, 0, 32 * 128, ctx->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(v->d_norm2_8 + total, 0xFF, 64 * sizeof(float), ctx->stream) == hipSuccess;     // (NaN)
    ok = ok && launch_gather_class_view(c->d_scr8, c->d_norm2_8, v->d_rank, v->n_rows, v->d_scr8, v->d_norm2_8, ctx->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        (void) hipGetLastError();                    // (out of memory: not an error of the load)
        return;
    }
    c->class_view = std::move(v);
}

// the rows of one permission class as a RANGES filter (built once, owned by the corpus)
static int class_filter(vsr_corpus* c, uint32_t cls, vsr_filter** out)
{
    if (c->class_filters[cls]) {
        *out = c->class_filters[cls];
        return VSR_OK;
    }
    FilterPtr f = new_filter(c, VSR_FILTER_RANGES, true);
    Ranges ranges;
    const int64_t rows = class_ranges(c, cls, ranges);
    int rc = upload_ranges(f.get(), ranges);
    if (rc) return rc;
    f->allowed_rows = f->scanned_rows = rows;
    f->view_class = (int32_t) cls;
    c->class_filters[cls] = f.release();
    *out = c->class_filters[cls];
    return VSR_OK;
}


// the rows of one permission class in post-filter form: the RW-aligned windows that hold at least one of its rows and the
// class's own permission bitmap, tested per row in the distance loop (built once, owned by the corpus)
static int class_bitmap_filter(vsr_corpus* c, uint32_t cls, vsr_filter** out)
{
    if (c->class_bitmap_filters[cls]) {
        *out = c->class_bitmap_filters[cls];
        return VSR_OK;
    }
    FilterPtr f = new_filter(c, VSR_FILTER_BITMAP, true);
    Ranges ranges;
    const int64_t rows = class_ranges(c, cls, ranges);
    int rc = alloc_bitmap(f.get());
    if (rc) return rc;
    HIPCHK(launch_build_class_bitmap(c->d_row_docidx, (uint32_t) c->n, c->d_doc_class, cls, f->d_bitmap, c->ctx->stream));
    if ((rc = upload_aligned_ranges(f.get(), ranges))) return rc;
    HIPCHK(hipStreamSynchronize(c->ctx->stream));
    f->allowed_rows = rows;
    c->class_bitmap_filters[cls] = f.release();
    *out = c->class_bitmap_filters[cls];
    return VSR_OK;
}

// f->parts <- the non-empty classes a role mask sees, each as the filter `make` builds of it (none when there are too
// many classes or parts to pay, or fewer than two parts)
static int class_parts(vsr_corpus* c, const std::vector<uint64_t>& m, int (*make)(vsr_corpus*, uint32_t, vsr_filter**), vsr_filter* f)
{
    if (c->class_sig.size() > MAX_CLASSES) return VSR_OK;
    for (uint32_t cls = 0; cls < (uint32_t) c->class_sig.size(); ++cls) {
        bool hit = false;
        for (uint32_t w = 0; w < c->words; ++w) hit |= (c->class_sig[cls][w] & m[w]) != 0;
        if (!hit) continue;
        vsr_filter* part = nullptr;
        int rc = make(c, cls, &part);
        if (rc) return rc;
        if (part->n_tiles) f->parts.push_back(part);
    }
    if (f->parts.size() == 1 && f->mode == VSR_FILTER_RANGES && !f->d_bitmap) f->view_class = f->parts[0]->view_class;   // its rows are that class
    if (f->parts.size() > MAX_PARTS || f->parts.size() < 2) f->parts.clear();
    return VSR_OK;
}

static int build_role_filter(vsr_corpus* c, const std::vector<int32_t>& roles, int mode, vsr_filter** out)
{
    FilterPtr f = new_filter(c, mode, false);
    const std::vector<uint64_t> m = role_mask(c, roles);
    Ranges ranges;
    int64_t allowed = 0;
    for (size_t di = 0; di < c->docs.size(); ++di) {
        if (!doc_allowed(c, di, m)) continue;
        const uint32_t s = c->doc_row_start[di], e = c->doc_row_start[di + 1];
        allowed += e - s;
        append_range(ranges, s, e);
    }
    f->allowed_rows = allowed;
    if (mode == VSR_FILTER_RANGES) {
        int rc = upload_ranges(f.get(), ranges);
        if (rc) return rc;
        f->scanned_rows = allowed;
        // the same row set as a union of permission classes (used when many queries are searched together)
        if ((rc = class_parts(c, m, class_filter, f.get()))) return rc;
    } else {
        int rc = alloc_bitmap(f.get());
        if (rc) return rc;
        vsr_ctx* ctx = c->ctx;
        rc = ctx->d_misc.reserve(c->words * sizeof(uint64_t));
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->d_misc.p, m.data(), c->words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_build_bitmap(c->d_row_docidx, (uint32_t) c->n, c->d_doc_mask, c->words,
                                   ctx->d_misc.as<uint64_t>(), f->d_bitmap, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));      // m is a stack-owned host buffer
        if ((rc = upload_aligned_ranges(f.get(), ranges))) return rc;
        // the same row set class by class, each class with its own bitmap: queries of different roles then share the
        // classes they have in common exactly as in pre-filter mode (the bit test per row stays in the distance loop)
        if ((rc = class_parts(c, m, class_bitmap_filter, f.get()))) return rc;
    }
    *out = f.release();
    return VSR_OK;
}

extern "C" int vsr_filter_for_roles(vsr_corpus* c, const int32_t* role_ids, int n_roles, int mode, vsr_filter** out)
{
    if (!c || !out || n_roles < 0 || (n_roles > 0 && !role_ids)) return fail(VSR_ERR_INVALID, "vsr_filter_for_roles: bad argument");
    *out = nullptr;
    if (mode != VSR_FILTER_RANGES && mode != VSR_FILTER_BITMAP) return fail(VSR_ERR_INVALID, "vsr_filter_for_roles: mode %d", mode);
    if (!c->rbac) return fail(VSR_ERR_NO_RBAC, "vsr_filter_for_roles: call vsr_rbac_load first");
    HIPCHK(hipSetDevice(c->ctx->device));
    std::vector<int32_t> roles(role_ids, role_ids + n_roles);
    std::sort(roles.begin(), roles.end());
    roles.erase(std::unique(roles.begin(), roles.end()), roles.end());
    auto key = std::make_pair(mode, roles);
    auto it = c->cache.find(key);
    if (it != c->cache.end()) {
        *out = it->second;
        return VSR_OK;
    }
    vsr_filter* f = nullptr;
    int rc = build_role_filter(c, roles, mode, &f);
    if (rc) return rc;
    f->cached = true;
    c->cache[key] = f;
    *out = f;
    return VSR_OK;
}

extern "C" int vsr_filter_for_user(vsr_corpus* c, int32_t user_id, int mode, vsr_filter** out)
{
    if (!c || !out) return fail(VSR_ERR_INVALID, "vsr_filter_for_user: NULL argument");
    if (!c->rbac) return fail(VSR_ERR_NO_RBAC, "vsr_filter_for_user: call vsr_rbac_load first");
    const std::vector<int32_t>& roles = roles_of_user(c, user_id);
    return vsr_filter_for_roles(c, roles.data(), (int) roles.size(), mode, out);
}

extern "C" int vsr_filter_from_bytemask(vsr_corpus* c, const uint8_t* allowed, int mode, vsr_filter** out)
{
    if (!c || !out || (!allowed && c->n > 0)) return fail(VSR_ERR_INVALID, "vsr_filter_from_bytemask: NULL argument");
    *out = nullptr;
    if (mode != VSR_FILTER_RANGES && mode != VSR_FILTER_BITMAP) return fail(VSR_ERR_INVALID, "vsr_filter_from_bytemask: mode %d", mode);
    HIPCHK(hipSetDevice(c->ctx->device));
    FilterPtr f = new_filter(c, mode, false);
    int64_t cnt = 0;
    for (int64_t i = 0; i < c->n; ++i) cnt += allowed[i] != 0;
    f->allowed_rows = cnt;
    Ranges ranges;
    for (int64_t i = 0; i < c->n; ++i) {
        if (!allowed[c->h_orig[(size_t) i]]) continue;
        append_range(ranges, (uint32_t) i, (uint32_t) i + 1);
    }
    if (mode == VSR_FILTER_RANGES) {
        int rc = upload_ranges(f.get(), ranges);
        if (rc) return rc;
        f->scanned_rows = cnt;
    } else {
        int rc = alloc_bitmap(f.get());
        if (rc) return rc;
        vsr_ctx* ctx = c->ctx;
        rc = ctx->d_misc.reserve((size_t) std::max<int64_t>(c->n, 1));
        if (rc) return rc;
        if (c->n > 0) {
            HIPCHK(hipMemcpyAsync(ctx->d_misc.p, allowed, (size_t) c->n, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(launch_pack_bytemask(ctx->d_misc.as<uint8_t>(), c->d_orig, (uint32_t) c->n, f->d_bitmap, ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if ((rc = upload_aligned_ranges(f.get(), ranges))) return rc;
    }
    *out = f.release();
    return VSR_OK;
}

extern "C" int vsr_filter_from_documents(vsr_corpus* c, const int32_t* doc_ids, int64_t n_docs, int32_t user_id,
                                         vsr_filter** out)
{
    if (!c || !out || n_docs < 0 || (n_docs > 0 && !doc_ids)) return fail(VSR_ERR_INVALID, "vsr_filter_from_documents: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->ctx->device));
    FilterPtr f = new_filter(c, VSR_FILTER_RANGES, false);
    std::vector<int32_t> want(doc_ids, doc_ids + n_docs);
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    std::vector<uint64_t> um;
    if (user_id >= 0) {
        if (!c->rbac) return fail(VSR_ERR_NO_RBAC, "vsr_filter_from_documents: call vsr_rbac_load first");
        um = role_mask(c, roles_of_user(c, user_id));
    }
    Ranges ranges;
    int64_t scanned = 0, allowed = 0;
    for (int32_t d : want) {
        auto it = std::lower_bound(c->docs.begin(), c->docs.end(), d);
        if (it == c->docs.end() || *it != d) continue;
        const size_t di = (size_t) (it - c->docs.begin());
        const uint32_t s = c->doc_row_start[di], e = c->doc_row_start[di + 1];
        scanned += e - s;
        if (user_id < 0 || doc_allowed(c, di, um)) allowed += e - s;
        append_range(ranges, s, e);
    }
    int rc = upload_ranges(f.get(), ranges);
    if (rc) return rc;
    f->allowed_rows = allowed;
    f->scanned_rows = scanned;
    if (user_id >= 0) {
        // impure partition: the user's permission bitmap rides along with the partition's tiles
        vsr_filter* ub = nullptr;
        rc = vsr_filter_for_user(c, user_id, VSR_FILTER_BITMAP, &ub);
        if (rc) return rc;
        f->d_bitmap = ub->d_bitmap;
        f->owns_bitmap = false;
    }
    *out = f.release();
    return VSR_OK;
}

extern "C" int vsr_filter_free(vsr_filter* f)
{
    if (!f || f->cached) return VSR_OK;    // cached filters belong to the corpus
    (void) hipSetDevice(f->corpus->ctx->device);
    (void) hipStreamSynchronize(f->corpus->ctx->stream);
    purge_index_caches(f->corpus, f);
    free_filter(f);
    return VSR_OK;
}

extern "C" int64_t vsr_filter_allowed_rows(const vsr_filter* f) { return f ? f->allowed_rows : 0; }
extern "C" int64_t vsr_filter_scanned_rows(const vsr_filter* f) { return f ? f->scanned_rows : 0; }
