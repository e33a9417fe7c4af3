// vsr_runtime.hip — host side of libvsrbac: the C ABI of include/vsrbac.h over the gfx950 kernels.  This unit: errors, the
// context and its knobs, statistics and profiling events, corpus load / free, the pair / vector functions and the multi-GPU
// merge entry points.  No CPU compute path: every search / distance entry point launches HIP kernels or fails.
#include "vsr_runtime.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <numeric>

// ---- errors
static thread_local std::string g_last_error;

int vsr::fail(int status, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

// helpers of the other translation units of the library (vsr_kmeans.hip)
int vsr_kmeans_fail(const char* what, const char* why, bool oom)
{
    return fail(oom ? VSR_ERR_OOM : VSR_ERR_HIP, "%s: %s", what, why);
}

// ---- context
extern "C" int vsr_abi_version(void) { return VSR_ABI_VERSION; }

extern "C" const char* vsr_last_error(void) { return g_last_error.c_str(); }

extern "C" const char* vsr_status_string(int s)
{
    switch (s) {
    case VSR_OK: return "ok";
    case VSR_ERR_INVALID: return "invalid argument";
    case VSR_ERR_DIM_MISMATCH: return "different vector dimensions";
    case VSR_ERR_NO_DEVICE: return "no usable gfx950 device";
    case VSR_ERR_HIP: return "HIP error";
    case VSR_ERR_OOM: return "out of device memory";
    case VSR_ERR_UNSUPPORTED: return "unsupported";
    case VSR_ERR_NO_RBAC: return "RBAC tables not loaded";
    default: return "unknown";
    }
}

extern "C" int vsr_open(int device, vsr_ctx** out)
{
    if (!out) return fail(VSR_ERR_INVALID, "vsr_open: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(VSR_ERR_NO_DEVICE, "vsr_open: no HIP device (%s); libvsrbac has no CPU path",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(VSR_ERR_INVALID, "vsr_open: device %d of %d", device, count);
    std::unique_ptr<vsr_ctx> ctx(new vsr_ctx());
    ctx->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipGetDeviceProperties(&ctx->prop, device));
    if (strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VSR_ERR_NO_DEVICE, "vsr_open: device %d is %s; this library is built for gfx950 only", device,
                    ctx->prop.gcnArchName);
    HIPCHK(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    HIPCHK(hipEventCreateWithFlags(&ctx->desc_done, hipEventDisableTiming));
    HIPCHK(hipMalloc(&ctx->d_flag_total, 64));
    HIPCHK(hipMemset(ctx->d_flag_total, 0, 64));
    HIPCHK(hipMemset(const_cast<uint64_t*>(ctx->ones_word()), 0xFF, 8));
    const char* env;
    if ((env = getenv("VSR_BLOCK_BUDGET"))) ctx->block_budget = atoi(env);
    if ((env = getenv("VSR_FUSED_FAN"))) ctx->fused_fan = atoi(env);
    if ((env = getenv("VSR_SCAN_LANE"))) ctx->scan_lane = atoi(env) != 0;
    if ((env = getenv("VSR_FUSED_DBG"))) ctx->fused_dbg = atoi(env) != 0;
    if ((env = getenv("VSR_MIN_ROWS_PER_BLOCK"))) ctx->min_rows_per_block = std::max(1, atoi(env));
    if ((env = getenv("VSR_MAX_QB"))) { ctx->max_qb = std::max(1, atoi(env)); ctx->max_qb_set = true; }
    if ((env = getenv("VSR_NO_MQ"))) ctx->no_mq = atoi(env) != 0;
    if ((env = getenv("VSR_NO_WIDE"))) ctx->no_wide = atoi(env) != 0;
    if ((env = getenv("VSR_NO_GEMM"))) ctx->no_gemm = atoi(env) != 0;
    if ((env = getenv("VSR_NO_HALF_MFMA"))) ctx->no_half_mfma = atoi(env) != 0;
    if ((env = getenv("VSR_K2I"))) ctx->no_k2i = atoi(env) == 0;
    if ((env = getenv("VSR_FORCE_EPI"))) ctx->force_epi = atoi(env) != 0;
    if ((env = getenv("VSR_K2I_WIDE"))) ctx->k2i_wide = atoi(env) != 0;
    if ((env = getenv("VSR_NO_SCAN8"))) ctx->no_scan8 = atoi(env) != 0;
    if ((env = getenv("VSR_NO_K2I_SAMPLE"))) ctx->k2i_sample = atoi(env) == 0;
    if ((env = getenv("VSR_NO_CLASSES"))) ctx->no_classes = atoi(env) != 0;
    if ((env = getenv("VSR_NO_CLASS_VIEW"))) ctx->no_class_view = atoi(env) != 0;
    if ((env = getenv("VSR_DEBUG"))) ctx->debug = (uint32_t) atoi(env);
    if ((env = getenv("VSR_NO_SEED"))) ctx->seeding = atoi(env) == 0;
    if ((env = getenv("VSR_NO_FUSED"))) ctx->no_fused = atoi(env) != 0;
    if ((env = getenv("VSR_NO_XCD_MAP"))) ctx->no_xcd_map = atoi(env) != 0;
    if ((env = getenv("VSR_MIN_SHARED_ROWS"))) ctx->min_shared_rows = std::max(64, atoi(env));
    if ((env = getenv("VSR_SEED_MIN_PASS"))) ctx->seed_min_pass_rows = atoll(env);
    if ((env = getenv("VSR_SAMPLE_STRIDE"))) {
        ctx->sample_stride = (uint32_t) std::min(512, std::max(2, atoi(env)));
        ctx->sample_stride_set = true;
    }
    if ((env = getenv("VSR_SAMPLE_REG"))) ctx->sample_reg = atoi(env) != 0;
    if ((env = getenv("VSR_SELECT_WAVE"))) ctx->select_wave = atoi(env) != 0;
    if ((env = getenv("VSR_SAMPLE_ROUNDS"))) ctx->sample_rounds = (uint32_t) std::min(4, std::max(1, atoi(env)));
    if ((env = getenv("VSR_SEED_STRIDE"))) ctx->seed_stride = (uint32_t) std::max(2, atoi(env));
    if ((env = getenv("VSR_SEED_DIV"))) ctx->seed_block_div = (uint32_t) std::max(1, atoi(env));
    if ((env = getenv("VSR_NO_SCREENING"))) ctx->screening = atoi(env) == 0;
    static std::atomic<uint32_t> g_ctx_ordinal{0};
    ctx->ordinal = g_ctx_ordinal.fetch_add(1, std::memory_order_relaxed);
    if ((env = getenv("VSR_WALK_ALIGN"))) ctx->walk_align = atoi(env) != 0;
    if ((env = getenv("VSR_WALK_POS"))) {
        ctx->walk_pos = (uint32_t) std::min<unsigned long long>(strtoull(env, nullptr, 0), 0xFFFFFFFFull);
        ctx->walk_pos_set = true;
    }
    if ((env = getenv("VSR_WALK_ROT"))) {
        ctx->walk_spread = strcmp(env, "spread") == 0;
        ctx->walk_rot_set = !ctx->walk_spread;
        ctx->walk_rot = ctx->walk_spread ? 0 : strtoull(env, nullptr, 0);
    }
    *out = ctx.release();
    return VSR_OK;
}

int vsr_ctx_device(const vsr_ctx* ctx, hipStream_t* stream)
{
    if (stream) *stream = ctx->stream;
    return ctx->device;
}

extern "C" int vsr_close(vsr_ctx* ctx)
{
    if (!ctx) return VSR_OK;
    (void) hipSetDevice(ctx->device);
    (void) hipStreamSynchronize(ctx->stream);
    delete ctx;
    return VSR_OK;
}

extern "C" int vsr_set_stream(vsr_ctx* ctx, void* s)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_set_stream: ctx is NULL");
    ctx->stream = s ? reinterpret_cast<hipStream_t>(s) : ctx->own_stream;
    return VSR_OK;
}

extern "C" int vsr_synchronize(vsr_ctx* ctx)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_synchronize: ctx is NULL");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

extern "C" int vsr_device_info(vsr_ctx* ctx, char* name, int name_len, int* cus, int64_t* hbm)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_device_info: ctx is NULL");
    if (name && name_len > 0)      // some boxes report an empty marketing name: say what the architecture implies
        snprintf(name, (size_t) name_len, "%s (%s)", ctx->prop.name[0] ? ctx->prop.name : "AMD Instinct (CDNA4)",
                 ctx->prop.gcnArchName);
    if (cus) *cus = ctx->prop.multiProcessorCount;
    if (hbm) *hbm = (int64_t) ctx->prop.totalGlobalMem;
    return VSR_OK;
}

extern "C" int vsr_tune(vsr_ctx* ctx, int block_budget, int min_rows_per_block, int max_qb)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_tune: ctx is NULL");
    if (block_budget >= 0) ctx->block_budget = block_budget;
    if (min_rows_per_block > 0) ctx->min_rows_per_block = min_rows_per_block;
    if (max_qb > 0) { ctx->max_qb = max_qb; ctx->max_qb_set = true; }
    return VSR_OK;
}

// ---- measurement
static void drain_events(vsr_ctx* ctx)
{
    for (auto& ep : ctx->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(ep.b) == hipSuccess && hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
            if (ep.kind == 5) {
                ctx->stats.search_ms += ms;
            } else if (ep.kind >= 3) {
                ctx->extra_ms[ep.kind - 3] += ms;
            } else if (ep.kind < 2) {
                ctx->stats.scan_ms[ep.kind] += ms;
                ctx->stats.scan_launches[ep.kind]++;
            } else {
                ctx->stats.select_ms += ms;
                ctx->stats.select_launches++;
            }
        }
        ctx->event_pool.push_back(ep.a);
        ctx->event_pool.push_back(ep.b);
    }
    ctx->pending.clear();
}

extern "C" int vsr_profiling(vsr_ctx* ctx, int enable)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_profiling: ctx is NULL");
    ctx->profiling = enable < 0 ? 0 : enable;
    return VSR_OK;
}

extern "C" int vsr_stats_get(vsr_ctx* ctx, vsr_stats* out)
{
    if (!ctx || !out) return fail(VSR_ERR_INVALID, "vsr_stats_get: NULL argument");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    drain_events(ctx);
    *out = ctx->stats;
    if (ctx->debug) {              // VSR_DEBUG=1: host-side timing of the searches since the last call (stderr)
        fprintf(stderr, "[vsr debug] sample_scan_ms=%.3f seed_select_ms=%.3f\n", ctx->extra_ms[0], ctx->extra_ms[1]);
        ctx->extra_ms[0] = ctx->extra_ms[1] = 0;
        if (ctx->host_calls)
            fprintf(stderr, "[vsr debug] host per search: plan %.1f us, staging wait %.1f us, total %.1f us (%ld calls)\n",
                    ctx->host_us[0] / ctx->host_calls, ctx->host_us[1] / ctx->host_calls, ctx->host_us[2] / ctx->host_calls,
                    ctx->host_calls);
        ctx->host_us[0] = ctx->host_us[1] = ctx->host_us[2] = 0;
        ctx->host_calls = 0;
    }
    return VSR_OK;
}

extern "C" int vsr_stats_reset(vsr_ctx* ctx)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_stats_reset: ctx is NULL");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    drain_events(ctx);
    ctx->stats = vsr_stats{};
    return VSR_OK;
}

// ---- corpus
extern "C" int vsr_corpus_free(vsr_corpus* c)
{
    if (!c) return VSR_OK;
    (void) hipSetDevice(c->ctx->device);
    (void) hipStreamSynchronize(c->ctx->stream);
    delete c;
    return VSR_OK;
}

vsr_corpus::~vsr_corpus()
{
    if (scan_stream) { (void) hipStreamSynchronize(scan_stream); (void) hipStreamDestroy(scan_stream); }
    drop_cached_filters(this);
    void* ptrs[] = {d_rows, d_sp_off, d_scr, d_scr_c, d_scr8, d_norm2_8, d_all_tiles, d_doc_class, d_rank, d_norm2, d_norm2_max, d_block, d_doc, d_orig, d_row_docidx, d_doc_mask};
    for (void* p : ptrs)
        if (p) (void) hipFree(p);
}

extern "C" int64_t vsr_corpus_rows(const vsr_corpus* c) { return c ? c->n : 0; }
extern "C" int vsr_corpus_dim(const vsr_corpus* c) { return c ? c->dim : 0; }

// vsr_corpus_load (ELEM = float), vsr_corpus_load_half (ELEM = uint16_t, binary16 bit patterns) and vsr_corpus_load_bit
// (ELEM = uint8_t, ceil(dim / 8) bytes of packed bits): the same identity arrays and row order; a halfvec corpus keeps its rows
// as they came -- 2 bytes per element -- plus |row|^2, a bit corpus its bytes (pad bits cleared) plus the rows' popcounts,
// nothing else
template <class ELEM>
static int corpus_load(vsr_ctx* ctx, const ELEM* rows, int64_t n, int dim, const int64_t* block_ids, const int32_t* doc_ids,
                       int64_t row_offset, vsr_corpus** out, const char* who)
{
    constexpr bool HALF = sizeof(ELEM) == 2;
    constexpr bool BIT = sizeof(ELEM) == 1;
    constexpr int PER16 = 16 / (int) sizeof(ELEM);          // elements per 16-byte chunk (bit corpus: bytes)
    if (!ctx || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (n < 0 || (n > 0 && !rows)) return fail(VSR_ERR_INVALID, "%s: rows is NULL", who);
    if (BIT && (dim < 1 || dim > 64000))   // HNSW_MAX_DIM * 32, the widest bit column an index takes (hnswutils.c:1403)
        return fail(VSR_ERR_INVALID, "%s: bit must have between 1 and 64000 dimensions (got %d)", who, dim);
    if (!BIT && (dim < 1 || dim > 16000))  // VECTOR_MAX_DIM, pgvector/src/vector.h:4; HALFVEC_MAX_DIM, halfvec.h
        return fail(VSR_ERR_INVALID, "%s: %s must have between 1 and 16000 dimensions (got %d)", who, HALF ? "halfvec" : "vector", dim);
    if (n + row_offset >= 0xFFFFFFFFll) return fail(VSR_ERR_UNSUPPORTED, "%s: more than 2^32-2 rows per shard", who);
    HIPCHK(hipSetDevice(ctx->device));

    std::unique_ptr<vsr_corpus> c(new vsr_corpus());
    c->ctx = ctx;
    c->n = n;
    c->dim = dim;
    c->format = BIT ? RowFormat::BIT : HALF ? RowFormat::HALF : RowFormat::F32;
    const int in_elems = BIT ? (dim + 7) / 8 : dim;         // elements per row as the caller holds them
    const uint32_t row_chunks = format_row_chunks(c->format, dim);
    c->stride4 = HALF ? 2 * row_chunks : row_chunks;
    c->row_offset = row_offset;
    c->shape = scan_shape(c->format, dim);

    // internal order: (document_id, block_id); identity when the input is already sorted that way
    std::vector<int64_t> perm((size_t) n);
    std::iota(perm.begin(), perm.end(), (int64_t) 0);
    auto doc_of = [&](int64_t r) { return doc_ids ? doc_ids[r] : 0; };
    auto blk_of = [&](int64_t r) { return block_ids ? block_ids[r] : r; };
    bool sorted = true;
    for (int64_t i = 1; i < n && sorted; ++i) {
        const int32_t da = doc_of(i - 1), db = doc_of(i);
        if (da > db || (da == db && blk_of(i - 1) > blk_of(i))) sorted = false;
    }
    if (!sorted)
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
            const int32_t da = doc_of(a), db = doc_of(b);
            if (da != db) return da < db;
            return blk_of(a) < blk_of(b);
        });
    c->h_orig = perm;

    std::vector<int32_t> h_doc((size_t) n);
    std::vector<int64_t> h_blk((size_t) n);
    std::vector<uint32_t> h_docidx((size_t) n);
    for (int64_t i = 0; i < n; ++i) {
        h_doc[(size_t) i] = doc_of(perm[(size_t) i]);
        h_blk[(size_t) i] = blk_of(perm[(size_t) i]);
        if (i == 0 || h_doc[(size_t) i] != h_doc[(size_t) i - 1]) {
            c->docs.push_back(h_doc[(size_t) i]);
            c->doc_row_start.push_back((uint32_t) i);
        }
        h_docidx[(size_t) i] = (uint32_t) (c->docs.size() - 1);
    }
    c->doc_row_start.push_back((uint32_t) n);

    const size_t row_bytes = (size_t) row_chunks * 16;
    const size_t alloc_rows = (size_t) std::max<int64_t>(n, 1);
    HIPCHK(hipMalloc(&c->d_rows, alloc_rows * row_bytes + 1024));
    HIPCHK(hipMalloc(&c->d_norm2, alloc_rows * sizeof(float)));
    if (!BIT) {
        HIPCHK(hipMalloc(&c->d_norm2_max, 64));
        HIPCHK(hipMemset(c->d_norm2_max, 0, 64));
    }
    HIPCHK(hipMalloc(&c->d_block, alloc_rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_doc, alloc_rows * sizeof(int32_t)));
    HIPCHK(hipMalloc(&c->d_orig, alloc_rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_row_docidx, alloc_rows * sizeof(uint32_t)));

    if (n > 0) {
        if (sorted && in_elems % PER16 == 0 && !(BIT && dim % 8)) {
            HIPCHK(hipMemcpy(c->d_rows, rows, (size_t) n * row_bytes, hipMemcpyHostToDevice));
        } else {
            // permute + zero-pad through a bounded host staging buffer
            const size_t chunk_rows = std::max<size_t>(1, (64u << 20) / row_bytes);
            const size_t row_elems = (size_t) row_chunks * PER16;
            std::vector<ELEM> stage(chunk_rows * row_elems);
            for (int64_t base = 0; base < n; base += (int64_t) chunk_rows) {
                const int64_t m = std::min<int64_t>((int64_t) chunk_rows, n - base);
                std::fill(stage.begin(), stage.begin() + (size_t) m * row_elems, ELEM(0));
                for (int64_t i = 0; i < m; ++i) {
                    memcpy(&stage[(size_t) i * row_elems], rows + (size_t) perm[(size_t) (base + i)] * in_elems,
                           (size_t) in_elems * sizeof(ELEM));
                    // varbit guarantees zero pad bits and pgvector relies on it; this library clears them
                    if constexpr (BIT)
                        if (dim % 8) stage[(size_t) i * row_elems + (size_t) in_elems - 1] &= (ELEM) (0xFF00u >> (dim % 8));
                }
                HIPCHK(hipMemcpy(reinterpret_cast<char*>(c->d_rows) + (size_t) base * row_bytes, stage.data(),
                                 (size_t) m * row_bytes, hipMemcpyHostToDevice));
            }
        }
        HIPCHK(hipMemcpy(c->d_block, h_blk.data(), (size_t) n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_doc, h_doc.data(), (size_t) n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_orig, perm.data(), (size_t) n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_row_docidx, h_docidx.data(), (size_t) n * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (BIT) {                                          // the rows' popcounts (Jaccard), exact in fp32; nothing else
            HIPCHK(launch_row_popcounts(reinterpret_cast<const uint4*>(c->d_rows), (uint32_t) n, row_chunks, c->d_norm2, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            *out = c.release();
            return VSR_OK;
        }
        if (HALF) {
            // the rows are the corpus and their own screening plane (K2h): no fp32 image, no planes.  As below, a corpus
            // holding NaN / Inf (or norms that overflow) stays on the exact kernel, K1h
            HIPCHK(launch_row_norms_half(reinterpret_cast<const uint4*>(c->d_rows), (uint32_t) n, row_chunks, c->d_norm2, ctx->stream));
            HIPCHK(launch_norm_max(c->d_norm2, (uint32_t) n, c->d_norm2_max, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            float nmax = 0.0f;
            HIPCHK(hipMemcpy(&nmax, c->d_norm2_max, sizeof(float), hipMemcpyDeviceToHost));
            c->k2_safe = std::isfinite(nmax);
            *out = c.release();
            return VSR_OK;
        }
        HIPCHK(launch_row_norms(c->d_rows, (uint32_t) n, c->stride4, c->d_norm2, ctx->stream));
        HIPCHK(launch_norm_max(c->d_norm2, (uint32_t) n, c->d_norm2_max, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        // K2 multiplies the zero padding of its query fragments with row data and needs a finite error bound: a corpus
        // holding NaN / Inf (pgvector rejects those on input, vector.c:101-113) or overflowing norms stays on K1 / K1m
        float nmax = 0.0f;
        HIPCHK(hipMemcpy(&nmax, c->d_norm2_max, sizeof(float), hipMemcpyDeviceToHost));
        c->k2_safe = std::isfinite(nmax);
        // K2w multiplies bf16 hi / mid planes of the rows on the matrix cores (16x the fp32 MFMA rate); the planes are a
        // second, equally large image of the corpus, built once here (288 GB of HBM: the SIFT10M planes are 5 GB)
        if (c->k2_safe && mfmaw_supported(c->stride4) && !getenv("VSR_NO_PLANES")) {
            uint32_t* d_any = reinterpret_cast<uint32_t*>(c->d_norm2_max) + 8;      // spare word of the 64-byte block
            HIPCHK(launch_check_bf16_exact(c->d_rows, (uint32_t) n, c->stride4, d_any, ctx->stream));
            uint32_t any = 1;
            HIPCHK(hipMemcpyAsync(&any, d_any, sizeof any, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            c->scr_has_mid = any != 0 || getenv("VSR_NO_HIONLY") != nullptr;
            c->pstride4 = plane_stride4(dim, !c->scr_has_mid);
            HIPCHK(hipMalloc(&c->d_scr, alloc_rows * (size_t) c->pstride4 * 16 + 1024));
            HIPCHK(launch_split_planes(c->d_rows, (uint32_t) n, c->stride4, c->d_scr, c->pstride4, !c->scr_has_mid, ctx->stream));
            std::vector<uint2> all;
            ranges_to_tiles({{0u, (uint32_t) n}}, c->shape.rw, all);
            HIPCHK(hipMalloc(&c->d_all_tiles, all.size() * sizeof(uint2)));
            HIPCHK(hipMemcpy(c->d_all_tiles, all.data(), all.size() * sizeof(uint2), hipMemcpyHostToDevice));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            // long rows (the 768-d configurations) also get the COARSE planes of K2g: hi = bf16(x) alone, half the bytes of
            // the hi + mid planes and one product per element; wide passes (> 128 queries per filter part) screen on them
            if (mfmaw_qmax(c->pstride4, !c->scr_has_mid) > 64 && !getenv("VSR_NO_COARSE")) {
                c->cstride4 = coarse_stride4(dim);
                HIPCHK(hipMalloc(&c->d_scr_c, coarse_plane_u4((uint64_t) alloc_rows, c->cstride4) * 16 + 1024));
                HIPCHK(launch_split_coarse(c->d_rows, (uint32_t) n, c->stride4, c->d_scr_c, c->cstride4, ctx->stream));
                HIPCHK(hipStreamSynchronize(ctx->stream));
            }
            // SIFT-like corpora (every element an integer 0..255, d <= 128) also get int8 planes: a quarter of the fp32
            // bytes per row and v_mfma_i32_16x16x64_i8; used for L2 searches whose queries are such integers too
            if (!c->scr_has_mid && dim <= 128 && !getenv("VSR_NO_INT8")) {
                HIPCHK(hipMemsetAsync(d_any, 0, sizeof(uint32_t), ctx->stream));
                HIPCHK(launch_check_u8_exact(c->d_rows, (uint32_t) n, c->stride4, d_any, ctx->stream));
                HIPCHK(hipMemcpyAsync(&any, d_any, sizeof any, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(hipStreamSynchronize(ctx->stream));
                if (any == 0) {
                    // (K2i streams whole 16-row list tiles: a tile that starts at the last row reads 15 rows / norms past it)
                    HIPCHK(hipMalloc(&c->d_scr8, alloc_rows * (size_t) 128 + 4096));
                    HIPCHK(hipMalloc(&c->d_norm2_8, (alloc_rows + 64) * sizeof(float)));
                    HIPCHK(launch_split_planes8(c->d_rows, (uint32_t) n, c->stride4, (uint32_t) dim, c->d_scr8, c->d_norm2_8, ctx->stream));
                    HIPCHK(hipStreamSynchronize(ctx->stream));
                }
            }
        }
    }
    *out = c.release();
    return VSR_OK;
}

extern "C" int vsr_corpus_load(vsr_ctx* ctx, const float* rows, int64_t n, int dim, const int64_t* block_ids,
                               const int32_t* doc_ids, int64_t row_offset, vsr_corpus** out)
{
    return corpus_load(ctx, rows, n, dim, block_ids, doc_ids, row_offset, out, "vsr_corpus_load");
}

extern "C" int vsr_corpus_load_half(vsr_ctx* ctx, const uint16_t* rows, int64_t n, int dim, const int64_t* block_ids,
                                    const int32_t* doc_ids, int64_t row_offset, vsr_corpus** out)
{
    return corpus_load(ctx, rows, n, dim, block_ids, doc_ids, row_offset, out, "vsr_corpus_load_half");
}

extern "C" int vsr_corpus_is_half(const vsr_corpus* c) { return c && c->format == RowFormat::HALF ? 1 : 0; }

extern "C" int vsr_corpus_load_bit(vsr_ctx* ctx, const uint8_t* rows, int64_t n, int dim, const int64_t* block_ids,
                                   const int32_t* doc_ids, int64_t row_offset, vsr_corpus** out)
{
    return corpus_load(ctx, rows, n, dim, block_ids, doc_ids, row_offset, out, "vsr_corpus_load_bit");
}

extern "C" int vsr_corpus_is_bit(const vsr_corpus* c) { return c && c->format == RowFormat::BIT ? 1 : 0; }

// ---- sparse corpora (pgvector's sparsevec) ----
int vsr::check_sparse_rows(const char* who, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n, int dim,
                           uint32_t* max_nnz)
{
    if (max_nnz) *max_nnz = 0;
    // CheckDim, sparsevec.c:53-65
    if (dim < 1) return fail(VSR_ERR_INVALID, "sparsevec must have at least 1 dimension");
    if (dim > SPARSE_MAX_DIM) return fail(VSR_ERR_INVALID, "sparsevec cannot have more than %d dimensions", SPARSE_MAX_DIM);
    if (n < 0 || (n > 0 && !indptr)) return fail(VSR_ERR_INVALID, "%s: indptr is NULL", who);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t beg = indptr[r], nnz = indptr[r + 1] - beg;
        // CheckNnz, :70-87
        if (nnz < 0 || beg < 0) return fail(VSR_ERR_INVALID, "sparsevec cannot have negative number of elements");
        if (nnz > SPARSE_MAX_NNZ) return fail(VSR_ERR_INVALID, "sparsevec cannot have more than %d non-zero elements", SPARSE_MAX_NNZ);
        if (nnz > dim) return fail(VSR_ERR_INVALID, "sparsevec cannot have more elements than dimensions");
        if (nnz > 0 && (!indices || !values)) return fail(VSR_ERR_INVALID, "%s: indices / values is NULL", who);
        for (int64_t i = 0; i < nnz; ++i) {                  // CheckIndex, :92-116
            const int32_t index = indices[beg + i];
            if (index < 0 || index >= dim) return fail(VSR_ERR_INVALID, "sparsevec index out of bounds");
            if (i > 0 && index < indices[beg + i - 1]) return fail(VSR_ERR_INVALID, "sparsevec indices must be in ascending order");
            if (i > 0 && index == indices[beg + i - 1]) return fail(VSR_ERR_INVALID, "sparsevec indices must not contain duplicates");
        }
        for (int64_t i = 0; i < nnz; ++i) {                  // CheckElement, :121-133; sparsevec_recv, :527-536
            const float v = values[beg + i];
            if (std::isnan(v)) return fail(VSR_ERR_INVALID, "NaN not allowed in sparsevec");
            if (std::isinf(v)) return fail(VSR_ERR_INVALID, "infinite value not allowed in sparsevec");
            if (v == 0) return fail(VSR_ERR_INVALID, "binary representation of sparsevec cannot contain zero values");
        }
        if (max_nnz && (uint32_t) nnz > *max_nnz) *max_nnz = (uint32_t) nnz;
    }
    return VSR_OK;
}

extern "C" int vsr_corpus_load_sparse(vsr_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                                      int dim, const int64_t* block_ids, const int32_t* doc_ids, int64_t row_offset, vsr_corpus** out)
{
    const char* who = "vsr_corpus_load_sparse";
    if (!ctx || !out) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    int rc = check_sparse_rows(who, indptr, indices, values, n, dim, nullptr);
    if (rc) return rc;
    if (n + row_offset >= 0xFFFFFFFFll) return fail(VSR_ERR_UNSUPPORTED, "%s: more than 2^32-2 rows per shard", who);
    HIPCHK(hipSetDevice(ctx->device));

    std::unique_ptr<vsr_corpus> c(new vsr_corpus());
    c->ctx = ctx;
    c->n = n;
    c->dim = dim;
    c->format = RowFormat::SPARSE;
    c->stride4 = 0;
    c->row_offset = row_offset;

    // internal order: (document_id, block_id), as corpus_load
    std::vector<int64_t> perm((size_t) n);
    std::iota(perm.begin(), perm.end(), (int64_t) 0);
    auto doc_of = [&](int64_t r) { return doc_ids ? doc_ids[r] : 0; };
    auto blk_of = [&](int64_t r) { return block_ids ? block_ids[r] : r; };
    bool sorted = true;
    for (int64_t i = 1; i < n && sorted; ++i) {
        const int32_t da = doc_of(i - 1), db = doc_of(i);
        if (da > db || (da == db && blk_of(i - 1) > blk_of(i))) sorted = false;
    }
    if (!sorted)
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
            const int32_t da = doc_of(a), db = doc_of(b);
            if (da != db) return da < db;
            return blk_of(a) < blk_of(b);
        });
    c->h_orig = perm;
    std::vector<int32_t> h_doc((size_t) n);
    std::vector<int64_t> h_blk((size_t) n);
    std::vector<uint32_t> h_docidx((size_t) n);
    for (int64_t i = 0; i < n; ++i) {
        h_doc[(size_t) i] = doc_of(perm[(size_t) i]);
        h_blk[(size_t) i] = blk_of(perm[(size_t) i]);
        if (i == 0 || h_doc[(size_t) i] != h_doc[(size_t) i - 1]) {
            c->docs.push_back(h_doc[(size_t) i]);
            c->doc_row_start.push_back((uint32_t) i);
        }
        h_docidx[(size_t) i] = (uint32_t) (c->docs.size() - 1);
    }
    c->doc_row_start.push_back((uint32_t) n);

    // the rows in internal order: offsets (every row an even number of entries), |row|^2 as sparsevec_cosine_distance sums it
    // (fp32, in order, :964-966)
    std::vector<uint64_t> off((size_t) n + 1, 0);
    std::vector<float> norm2((size_t) n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = perm[(size_t) i], nnz = indptr[r + 1] - indptr[r];
        off[(size_t) i + 1] = off[(size_t) i] + (uint64_t) ((nnz + 1) / 2 * 2);
        c->sp_max_nnz = std::max(c->sp_max_nnz, (uint32_t) nnz);
        float na = 0.0f;
        for (int64_t e = 0; e < nnz; ++e) {
            const float v = values[indptr[r] + e];
            const float sq = v * v;
            na = na + sq;
        }
        norm2[(size_t) i] = na;
    }
    c->sp_entries = off[(size_t) n];
    const double mean = n > 0 ? (double) c->sp_entries / (double) n : 0.0;
    const int lpr = sparse_lpr_for_mean_nnz(mean);
    c->shape = KernelShape{lpr, 0, lpr, 64};

    const size_t alloc_rows = (size_t) std::max<int64_t>(n, 1);
    HIPCHK(hipMalloc(&c->d_rows, (size_t) c->sp_entries * 8 + 1024));
    HIPCHK(hipMalloc(&c->d_sp_off, (alloc_rows + 1) * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&c->d_norm2, alloc_rows * sizeof(float)));
    HIPCHK(hipMalloc(&c->d_block, alloc_rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_doc, alloc_rows * sizeof(int32_t)));
    HIPCHK(hipMalloc(&c->d_orig, alloc_rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_row_docidx, alloc_rows * sizeof(uint32_t)));
    if (n > 0) {
        // interleave through a bounded host staging buffer (whole rows per piece)
        const size_t piece = (size_t) 8 << 20;               // entries
        std::vector<uint2> stage;
        for (int64_t i0 = 0; i0 < n;) {
            int64_t i1 = i0 + 1;
            while (i1 < n && off[(size_t) i1 + 1] - off[(size_t) i0] <= piece) ++i1;
            stage.assign((size_t) (off[(size_t) i1] - off[(size_t) i0]), make_uint2(SPARSE_EMPTY, 0u));
            for (int64_t i = i0; i < i1; ++i) {
                const int64_t r = perm[(size_t) i], nnz = indptr[r + 1] - indptr[r];
                uint2* dst = stage.data() + (off[(size_t) i] - off[(size_t) i0]);
                for (int64_t e = 0; e < nnz; ++e) {
                    uint32_t bits;
                    memcpy(&bits, &values[indptr[r] + e], 4);
                    dst[e] = make_uint2((uint32_t) indices[indptr[r] + e], bits);
                }
            }
            if (!stage.empty())
                HIPCHK(hipMemcpy(reinterpret_cast<uint2*>(c->d_rows) + off[(size_t) i0], stage.data(), stage.size() * sizeof(uint2),
                                 hipMemcpyHostToDevice));
            i0 = i1;
        }
        HIPCHK(hipMemcpy(c->d_norm2, norm2.data(), (size_t) n * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_block, h_blk.data(), (size_t) n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_doc, h_doc.data(), (size_t) n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_orig, perm.data(), (size_t) n * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_row_docidx, h_docidx.data(), (size_t) n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(c->d_sp_off, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    *out = c.release();
    return VSR_OK;
}

extern "C" int vsr_corpus_is_sparse(const vsr_corpus* c) { return c && c->format == RowFormat::SPARSE ? 1 : 0; }

// sparsevec.c:803-1037 for n explicit pairs (host CSR triples)
extern "C" int vsr_sparse_pair_distances(vsr_ctx* ctx, int metric, const int64_t* a_indptr, const int32_t* a_indices,
                                         const float* a_values, const int64_t* b_indptr, const int32_t* b_indices,
                                         const float* b_values, int64_t n_pairs, int dim_a, int dim_b, double* out)
{
    const char* who = "vsr_sparse_pair_distances";
    if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!a_indptr || !b_indptr || !out))) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    int rc = check_sparse_rows(who, a_indptr, a_indices, a_values, n_pairs, dim_a, nullptr);
    if (rc) return rc;
    if ((rc = check_sparse_rows(who, b_indptr, b_indices, b_values, n_pairs, dim_b, nullptr))) return rc;
    if (dim_a != dim_b) return fail(VSR_ERR_DIM_MISMATCH, "different sparsevec dimensions %d and %d", dim_a, dim_b);   // CheckDims
    if (metric < VSR_METRIC_L2 || metric > VSR_METRIC_L1) return fail(VSR_ERR_INVALID, "%s: metric %d", who, metric);
    if (n_pairs == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    // the pairs' entries, rebased to 0
    const int64_t a0 = a_indptr[0], b0 = b_indptr[0];
    const size_t a_nnz = (size_t) (a_indptr[n_pairs] - a0), b_nnz = (size_t) (b_indptr[n_pairs] - b0);
    std::vector<int64_t> ptr(2 * ((size_t) n_pairs + 1));
    for (int64_t i = 0; i <= n_pairs; ++i) {
        ptr[(size_t) i] = a_indptr[i] - a0;
        ptr[(size_t) n_pairs + 1 + (size_t) i] = b_indptr[i] - b0;
    }
    const size_t ptr_bytes = ptr.size() * sizeof(int64_t);
    const size_t o_ai = align_up(ptr_bytes, 256), o_av = align_up(o_ai + a_nnz * 4, 256), o_bi = align_up(o_av + a_nnz * 4, 256),
                 o_bv = align_up(o_bi + b_nnz * 4, 256), o_out = align_up(o_bv + b_nnz * 4, 256);
    if ((rc = ctx->d_misc.reserve(o_out + (size_t) n_pairs * sizeof(double)))) return rc;
    char* d = ctx->d_misc.as<char>();
    HIPCHK(hipMemcpyAsync(d, ptr.data(), ptr_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (a_nnz) {
        HIPCHK(hipMemcpyAsync(d + o_ai, a_indices + a0, a_nnz * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d + o_av, a_values + a0, a_nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (b_nnz) {
        HIPCHK(hipMemcpyAsync(d + o_bi, b_indices + b0, b_nnz * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d + o_bv, b_values + b0, b_nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (ptr is a local: the copy must have left it)
    const int64_t* d_ptr = reinterpret_cast<const int64_t*>(d);
    HIPCHK(launch_sparse_pair_distances(d_ptr, reinterpret_cast<const int32_t*>(d + o_ai), reinterpret_cast<const float*>(d + o_av),
                                        d_ptr + n_pairs + 1, reinterpret_cast<const int32_t*>(d + o_bi),
                                        reinterpret_cast<const float*>(d + o_bv), n_pairs, metric, reinterpret_cast<double*>(d + o_out),
                                        ctx->stream));
    HIPCHK(hipMemcpyAsync(out, d + o_out, (size_t) n_pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

// sparsevec_l2_norm (out_norm) or sparsevec_l2_normalize (out_values, out_zeros) of n CSR rows: only the offsets and the values enter
static int sparse_norm_fn(vsr_ctx* ctx, const int64_t* indptr, const float* values, int64_t n, double* out_norm, float* out_values,
                          int64_t* out_zeros, bool normalize, const char* who)
{
    if (!ctx || n < 0 || (n > 0 && !indptr) || (n > 0 && !normalize && !out_norm)) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    if (out_zeros) *out_zeros = 0;
    if (n == 0) return VSR_OK;
    const int64_t b0 = indptr[0];
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i] || indptr[i] < 0) return fail(VSR_ERR_INVALID, "sparsevec cannot have negative number of elements");
    const size_t nnz = (size_t) (indptr[n] - b0);
    if (nnz > 0 && (!values || (normalize && !out_values))) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int64_t> ptr((size_t) n + 1);
    for (int64_t i = 0; i <= n; ++i) ptr[(size_t) i] = indptr[i] - b0;
    const size_t o_val = align_up(ptr.size() * 8, 256), o_norm = align_up(o_val + nnz * 4, 256), o_out = align_up(o_norm + (size_t) n * 8, 256),
                 o_flag = align_up(o_out + nnz * 4, 256);
    int rc = ctx->d_misc.reserve(o_flag + 64);
    if (rc) return rc;
    char* d = ctx->d_misc.as<char>();
    HIPCHK(hipMemcpyAsync(d, ptr.data(), ptr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nnz) HIPCHK(hipMemcpyAsync(d + o_val, values + b0, nnz * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d + o_flag, 0, 16, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (ptr is a local: the copy must have left it)
    HIPCHK(launch_sparse_norms(reinterpret_cast<const int64_t*>(d), reinterpret_cast<const float*>(d + o_val), n,
                               reinterpret_cast<double*>(d + o_norm), normalize ? reinterpret_cast<float*>(d + o_out) : nullptr,
                               reinterpret_cast<int*>(d + o_flag), reinterpret_cast<unsigned long long*>(d + o_flag + 8), ctx->stream));
    struct { int overflow; int pad; unsigned long long zeros; } flag = {0, 0, 0};
    if (out_norm) HIPCHK(hipMemcpyAsync(out_norm, d + o_norm, (size_t) n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (normalize && nnz) HIPCHK(hipMemcpyAsync(out_values, d + o_out, nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&flag, d + o_flag, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (flag.overflow) return fail(VSR_ERR_INVALID, "value out of range: overflow");     // float_overflow_error(), sparsevec.c:1088
    if (out_zeros) *out_zeros = (int64_t) flag.zeros;
    return VSR_OK;
}

extern "C" int vsr_sparse_norms(vsr_ctx* ctx, const int64_t* indptr, const float* values, int64_t n, double* out)
{
    return sparse_norm_fn(ctx, indptr, values, n, out, nullptr, nullptr, false, "vsr_sparse_norms");
}

extern "C" int vsr_sparse_l2_normalize(vsr_ctx* ctx, const int64_t* indptr, const float* values, int64_t n, float* out_values,
                                       int64_t* out_zeros)
{
    return sparse_norm_fn(ctx, indptr, values, n, nullptr, out_values, out_zeros, true, "vsr_sparse_l2_normalize");
}

// binary_quantize over the resident rows: a bit corpus with the source's context, row identity and internal order.  RBAC
// tables are not inherited (filters belong to one corpus): the caller runs vsr_rbac_load on the new corpus.
extern "C" int vsr_corpus_binary_quantize(vsr_corpus* src, vsr_corpus** out)
{
    if (!src || !out) return fail(VSR_ERR_INVALID, "vsr_corpus_binary_quantize: NULL argument");
    *out = nullptr;
    if (src->format == RowFormat::BIT) return fail(VSR_ERR_INVALID, "vsr_corpus_binary_quantize: the corpus is a bit corpus already");
    if (src->format == RowFormat::SPARSE) return fail(VSR_ERR_UNSUPPORTED, "vsr_corpus_binary_quantize: a sparsevec corpus has no binary_quantize (pgvector defines none)");
    if (src->base) return fail(VSR_ERR_INVALID, "vsr_corpus_binary_quantize: this corpus is an index view");
    vsr_ctx* ctx = src->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<vsr_corpus> c(new vsr_corpus());
    c->ctx = ctx;
    c->n = src->n;
    c->dim = src->dim;
    c->format = RowFormat::BIT;
    c->quantized_from = src->serial;
    const uint32_t row_chunks = format_row_chunks(RowFormat::BIT, src->dim);
    c->stride4 = row_chunks;
    c->row_offset = src->row_offset;
    c->shape = scan_shape(RowFormat::BIT, src->dim);
    c->h_orig = src->h_orig;
    c->docs = src->docs;
    c->doc_row_start = src->doc_row_start;
    const size_t rows = (size_t) std::max<int64_t>(src->n, 1), n = (size_t) src->n;
    HIPCHK(hipMalloc(&c->d_rows, rows * row_chunks * 16 + 1024));
    HIPCHK(hipMalloc(&c->d_norm2, rows * sizeof(float)));
    HIPCHK(hipMalloc(&c->d_block, rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_doc, rows * sizeof(int32_t)));
    HIPCHK(hipMalloc(&c->d_orig, rows * sizeof(int64_t)));
    HIPCHK(hipMalloc(&c->d_row_docidx, rows * sizeof(uint32_t)));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(c->d_block, src->d_block, n * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(c->d_doc, src->d_doc, n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(c->d_orig, src->d_orig, n * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(c->d_row_docidx, src->d_row_docidx, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        // (both kinds of source row hold stride4 * 4 elements: fp32 rows stride4 float4, half rows stride4 / 2 chunks of 8)
        HIPCHK(launch_binary_quantize(src->d_rows, src->format == RowFormat::HALF ? 1 : 0, (uint64_t) n, (uint32_t) src->dim, src->stride4 * 4u,
                                      reinterpret_cast<uint8_t*>(c->d_rows), row_chunks * 16u, ctx->stream));
        HIPCHK(launch_row_popcounts(reinterpret_cast<const uint4*>(c->d_rows), (uint32_t) n, row_chunks, c->d_norm2, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    *out = c.release();
    return VSR_OK;
}

// binary_quantize (vector.c:941-968) for n host vectors -> n x ceil(dim / 8) bytes
extern "C" int vsr_binary_quantize(vsr_ctx* ctx, const float* a, int64_t n, int dim, uint8_t* out)
{
    if (!ctx || n < 0 || (n > 0 && (!a || !out))) return fail(VSR_ERR_INVALID, "vsr_binary_quantize: NULL argument");
    if (dim < 1) return fail(VSR_ERR_INVALID, "vsr_binary_quantize: dim %d", dim);
    if (n == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t a_bytes = (size_t) n * dim * sizeof(float), o_bytes = (size_t) n * (size_t) ((dim + 7) / 8);
    const size_t o_out = align_up(a_bytes, 256);
    int rc = ctx->d_misc.reserve(o_out + o_bytes);
    if (rc) return rc;
    char* d = ctx->d_misc.as<char>();
    HIPCHK(hipMemcpyAsync(d, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_binary_quantize(d, 0, (uint64_t) n, (uint32_t) dim, (uint32_t) dim, reinterpret_cast<uint8_t*>(d + o_out),
                                  (uint32_t) ((dim + 7) / 8), ctx->stream));
    HIPCHK(hipMemcpyAsync(out, d + o_out, o_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

// hamming_distance / jaccard_distance for n explicit pairs (bitvec.c:46-77); dim 0 is a valid bit string
extern "C" int vsr_bit_pair_distances(vsr_ctx* ctx, int metric, const uint8_t* a, const uint8_t* b, int64_t n_pairs, int dim_a,
                                      int dim_b, int b_broadcast, double* out)
{
    if (!ctx || n_pairs < 0 || (n_pairs > 0 && !out)) return fail(VSR_ERR_INVALID, "vsr_bit_pair_distances: NULL argument");
    if (dim_a < 0 || dim_b < 0) return fail(VSR_ERR_INVALID, "vsr_bit_pair_distances: negative bit length");
    if (dim_a != dim_b) return fail(VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u", (unsigned) dim_a, (unsigned) dim_b);   // CheckDims, bitvec.c:32-39
    if (dim_a > 0 && n_pairs > 0 && (!a || !b)) return fail(VSR_ERR_INVALID, "vsr_bit_pair_distances: NULL argument");
    if (metric != VSR_METRIC_HAMMING && metric != VSR_METRIC_JACCARD) return fail(VSR_ERR_INVALID, "vsr_bit_pair_distances: metric %d", metric);
    if (n_pairs == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t) ((dim_a + 7) / 8);
    const size_t a_bytes = (size_t) n_pairs * bytes, b_bytes = (size_t) (b_broadcast ? 1 : n_pairs) * bytes;
    const size_t o_b = align_up(a_bytes, 256), o_out = align_up(o_b + b_bytes, 256);
    int rc = ctx->d_misc.reserve(o_out + (size_t) n_pairs * sizeof(double));
    if (rc) return rc;
    char* d = ctx->d_misc.as<char>();
    if (a_bytes) HIPCHK(hipMemcpyAsync(d, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (b_bytes) HIPCHK(hipMemcpyAsync(d + o_b, b, b_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_bit_pair_distances(reinterpret_cast<uint8_t*>(d), reinterpret_cast<uint8_t*>(d + o_b), n_pairs, dim_a, b_broadcast,
                                     metric, reinterpret_cast<double*>(d + o_out), ctx->stream));
    HIPCHK(hipMemcpyAsync(out, d + o_out, (size_t) n_pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

// rows, norms and every screening plane as allocated at load (a view's own image: its base is another corpus)
extern "C" int64_t vsr_corpus_device_bytes(const vsr_corpus* c)
{
    if (!c) return 0;
    const size_t rows = (size_t) std::max<int64_t>(c->n, 1);
    if (c->format == RowFormat::SPARSE)                      // entries, row offsets, |row|^2
        return (int64_t) ((size_t) c->sp_entries * 8 + 1024 + (rows + 1) * sizeof(uint64_t) + rows * sizeof(float));
    size_t b = rows * format_row_chunks(c->format, c->dim) * 16 + 1024 + rows * sizeof(float);   // d_rows, d_norm2
    if (c->d_norm2_max) b += 64;
    if (c->d_scr) b += rows * (size_t) c->pstride4 * 16 + 1024;
    if (c->d_scr_c) b += coarse_plane_u4((uint64_t) rows, c->cstride4) * 16 + 1024;
    if (c->d_scr8) b += rows * (size_t) 128 + 4096;
    if (c->d_norm2_8) b += (rows + 64) * sizeof(float);
    if (c->class_view) b += c->class_view->bytes();         // (built by vsr_rbac_load, not at load)
    return (int64_t) b;
}

extern "C" int vsr_last_scan_kernel(vsr_ctx* ctx, char* name, int name_len)
{
    if (!ctx || !name || name_len < 1) return fail(VSR_ERR_INVALID, "vsr_last_scan_kernel: bad argument");
    snprintf(name, (size_t) name_len, "%s", ctx->last_kernel.c_str());
    return VSR_OK;
}

extern "C" int vsr_set_query_hint(vsr_ctx* ctx, int u8_queries)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_set_query_hint: ctx is NULL");
    ctx->hint_u8 = u8_queries != 0;
    if (ctx->hint_u8) {                                     // a fresh promise: forget earlier violations
        ctx->q8_ok = true;
        if (ctx->h_q8.p) *reinterpret_cast<volatile uint32_t*>(ctx->h_q8.p) = 0;
    }
    return VSR_OK;
}

extern "C" int vsr_set_screening(vsr_ctx* ctx, int enable)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_set_screening: ctx is NULL");
    ctx->screening = enable != 0;
    return VSR_OK;
}

extern "C" int vsr_screening_check(vsr_ctx* ctx, int64_t* flagged_total, int32_t* flags_last_call, int nq)
{
    if (!ctx) return fail(VSR_ERR_INVALID, "vsr_screening_check: ctx is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int32_t words[8] = {0};
    HIPCHK(hipMemcpy(words, ctx->d_flag_total, sizeof words, hipMemcpyDeviceToHost));
    const int32_t total = words[0];
    if (words[4] != 0)
        return fail(VSR_ERR_HIP, "internal bounds guard tripped in a scan kernel (bits %d): results are not valid", words[4]);
    if (flagged_total) *flagged_total = total;
    if (flags_last_call && nq > 0) {
        if (!ctx->d_flags.p || ctx->d_flags.cap < (size_t) nq * sizeof(int32_t))
            memset(flags_last_call, 0, (size_t) nq * sizeof(int32_t));
        else
            HIPCHK(hipMemcpy(flags_last_call, ctx->d_flags.p, (size_t) nq * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return VSR_OK;
}

extern "C" int vsr_merge_topk_device(vsr_ctx* ctx, const uint64_t* d_keys, const int64_t* d_blk, const int32_t* d_doc,
                                     const float* d_dist, int n_parts, int nq, int k, int64_t* o_blk, int32_t* o_doc,
                                     float* o_dist, uint64_t* o_keys, int32_t* o_cnt)
{
    if (!ctx || !d_keys || !d_blk || !d_doc || !d_dist || !o_blk || !o_doc || !o_dist || !o_cnt)
        return fail(VSR_ERR_INVALID, "vsr_merge_topk_device: NULL argument");
    if (n_parts < 1 || nq < 0 || k < 1) return fail(VSR_ERR_INVALID, "vsr_merge_topk_device: bad sizes");
    if (nq == 0) return VSR_OK;
    if ((int64_t) n_parts * k > 8192) return fail(VSR_ERR_UNSUPPORTED, "vsr_merge_topk_device: n_parts * k > 8192");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_merge_lists(d_keys, d_blk, d_doc, d_dist, (uint32_t) n_parts, (uint32_t) nq, (uint32_t) k, 0, o_blk,
                              o_doc, o_dist, o_keys, o_cnt, ctx->stream));
    return VSR_OK;
}

extern "C" int64_t vsr_packed_result_bytes(int nq, int k)
{
    return nq < 0 || k < 1 ? 0 : (int64_t) nq * k * 24;
}

extern "C" int vsr_merge_topk_packed_device(vsr_ctx* ctx, const void* d_packed, int n_parts, int nq, int k,
                                            int64_t* o_blk, int32_t* o_doc, float* o_dist, uint64_t* o_keys, int32_t* o_cnt)
{
    if (!ctx || !d_packed || !o_blk || !o_doc || !o_dist || !o_cnt) return fail(VSR_ERR_INVALID, "vsr_merge_topk_packed_device: NULL argument");
    if (n_parts < 1 || nq < 0 || k < 1) return fail(VSR_ERR_INVALID, "vsr_merge_topk_packed_device: bad sizes");
    if (nq == 0) return VSR_OK;
    if ((int64_t) n_parts * k > 8192) return fail(VSR_ERR_UNSUPPORTED, "vsr_merge_topk_packed_device: n_parts * k > 8192");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nk = (size_t) nq * k;
    const char* base = reinterpret_cast<const char*>(d_packed);
    HIPCHK(launch_merge_lists(reinterpret_cast<const uint64_t*>(base), reinterpret_cast<const int64_t*>(base + nk * 8),
                              reinterpret_cast<const int32_t*>(base + nk * 16), reinterpret_cast<const float*>(base + nk * 20),
                              (uint32_t) n_parts, (uint32_t) nq, (uint32_t) k, nk * 24, o_blk, o_doc, o_dist, o_keys, o_cnt,
                              ctx->stream));
    return VSR_OK;
}

extern "C" int vsr_pair_distances(vsr_ctx* ctx, int metric, const float* a, const float* b, int64_t n_pairs, int dim_a,
                                  int dim_b, int b_broadcast, double* out)
{
    if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!a || !b || !out))) return fail(VSR_ERR_INVALID, "vsr_pair_distances: NULL argument");
    if (dim_a != dim_b) return fail(VSR_ERR_DIM_MISMATCH, "different vector dimensions %d and %d", dim_a, dim_b);
    if (dim_a < 1) return fail(VSR_ERR_INVALID, "vsr_pair_distances: dim %d", dim_a);
    if (metric < VSR_METRIC_L2 || metric > VSR_METRIC_L1) return fail(VSR_ERR_INVALID, "vsr_pair_distances: metric %d", metric);
    if (n_pairs == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t a_bytes = (size_t) n_pairs * dim_a * sizeof(float);
    const size_t b_bytes = (size_t) (b_broadcast ? 1 : n_pairs) * dim_a * sizeof(float);
    const size_t o_a = 0, o_b = align_up(a_bytes, 256), o_out = align_up(o_b + b_bytes, 256);
    int rc = ctx->d_misc.reserve(o_out + (size_t) n_pairs * sizeof(double));
    if (rc) return rc;
    char* d = ctx->d_misc.as<char>();
    HIPCHK(hipMemcpyAsync(d + o_a, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d + o_b, b, b_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_pair_distances(reinterpret_cast<float*>(d + o_a), reinterpret_cast<float*>(d + o_b), n_pairs, dim_a,
                                 b_broadcast, metric, reinterpret_cast<double*>(d + o_out), ctx->stream));
    HIPCHK(hipMemcpyAsync(out, d + o_out, (size_t) n_pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

// ---- opclass support functions, batched (vector.c:692-711, 756-808)
static int vector_fn(vsr_ctx* ctx, int mode, const float* a, const float* b, int64_t n, int dim_a, int dim_b, int b_broadcast,
                     double* out_d, float* out_f, const char* who)
{
    if (!ctx || n < 0 || (n > 0 && (!a || (mode == 2 && !b) || (mode == 1 ? !out_f : !out_d))))
        return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    if (mode == 2 && dim_a != dim_b) return fail(VSR_ERR_DIM_MISMATCH, "different vector dimensions %d and %d", dim_a, dim_b);
    if (dim_a < 1) return fail(VSR_ERR_INVALID, "%s: dim %d", who, dim_a);
    if (n == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t a_bytes = (size_t) n * dim_a * sizeof(float);
    const size_t b_bytes = mode == 2 ? (size_t) (b_broadcast ? 1 : n) * dim_a * sizeof(float) : 0;
    const size_t o_bytes = mode == 1 ? a_bytes : (size_t) n * sizeof(double);
    const size_t o_b = align_up(a_bytes, 256), o_out = align_up(o_b + b_bytes, 256), o_flag = align_up(o_out + o_bytes, 256);
    int rc = ctx->d_misc.reserve(o_flag + 64);
    if (rc) return rc;
    char* d = ctx->d_misc.as<char>();
    HIPCHK(hipMemcpyAsync(d, a, a_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (b_bytes) HIPCHK(hipMemcpyAsync(d + o_b, b, b_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d + o_flag, 0, 4, ctx->stream));
    HIPCHK(launch_vector_fn(mode, reinterpret_cast<float*>(d), reinterpret_cast<float*>(d + o_b), n, dim_a, b_broadcast,
                            reinterpret_cast<double*>(d + o_out), reinterpret_cast<float*>(d + o_out),
                            reinterpret_cast<int*>(d + o_flag), ctx->stream));
    int overflow = 0;
    HIPCHK(hipMemcpyAsync(mode == 1 ? (void*) out_f : (void*) out_d, d + o_out, o_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&overflow, d + o_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (overflow) return fail(VSR_ERR_INVALID, "value out of range: overflow");        // float_overflow_error(), vector.c:803
    return VSR_OK;
}

extern "C" int vsr_vector_norms(vsr_ctx* ctx, const float* a, int64_t n, int dim, double* out)
{
    return vector_fn(ctx, 0, a, nullptr, n, dim, dim, 0, out, nullptr, "vsr_vector_norms");
}

extern "C" int vsr_l2_normalize(vsr_ctx* ctx, const float* a, int64_t n, int dim, float* out)
{
    return vector_fn(ctx, 1, a, nullptr, n, dim, dim, 0, nullptr, out, "vsr_l2_normalize");
}

extern "C" int vsr_spherical_distances(vsr_ctx* ctx, const float* a, const float* b, int64_t n, int dim_a, int dim_b,
                                       int b_broadcast, double* out)
{
    return vector_fn(ctx, 2, a, b, n, dim_a, dim_b, b_broadcast, out, nullptr, "vsr_spherical_distances");
}
