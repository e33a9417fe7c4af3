// vsr_ivf.hip — K3: IVFFlat over a list-ordered view of the corpus (probe, per-list filter parts, assignment).
// K3h: the same over a halfvec corpus (the _half entry points): binary16 rows in the view, binary16 centres, nothing widened.
// K3b: the same over a bit corpus (the _bit entry points, bit_hamming_ops): packed rows in the view, packed centres, K1b scans.
#include "vsr_runtime.h"
#include "vsr_ivf_iter.h"
#include "vsr_ivf_shortlist.h"

#include <cmath>

namespace vsr {
hipError_t launch_ivf_iterative(const IvfIterParams& p, uint32_t nq, hipStream_t s)
{
    if (nq == 0) return hipSuccess;
    if (p.rows_bit) {                                      // K3b: its own kernel, its own LDS formula (chunks per row, the waves' counts)
        const size_t lds = ivf_iter_lds_bytes(p.lists, p.stride4, p.k, true);
        // (the lane-group gather of vsr_bitops.h takes row ids as int32)
        if (lds > 160 * 1024 || p.k < 1 || p.k > (uint32_t) MAX_K || p.n_rows > 0x7FFFFE00u) return hipErrorInvalidValue;
        auto* kernel = ivf_iterative_kernel<IVI_BIT>;
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, dim3(nq), dim3(256), lds, s, p);
        return hipGetLastError();
    }
    const size_t lds = ivf_iter_lds_bytes(p.lists, p.stride4, p.k);
    // 160 KiB of LDS per CU; view rows are addressed in 32 bits with a step of 256 to spare
    if (lds > 160 * 1024 || p.k < 1 || p.k > (uint32_t) MAX_K || p.n_rows > 0xFFFFFE00u) return hipErrorInvalidValue;
    auto* kernel = p.rows_half ? ivf_iterative_kernel<IVI_HALF> : ivf_iterative_kernel<IVI_F32>;
    if (lds > 64 * 1024) {                                 // (per instantiation: each is a kernel of its own)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(nq), dim3(256), lds, s, p);
    return hipGetLastError();
}

// K3q (vsr_ivf_shortlist.h): one workgroup per query; what does not fit the CU's LDS is refused, as above
hipError_t launch_ivf_bit_shortlist(const IvfShortlistParams& p, uint32_t nq, hipStream_t s)
{
    if (nq == 0) return hipSuccess;
    const size_t lds = ivf_shortlist_lds_bytes(p.lists, p.stride4, p.shortlist);
    if (lds > 160 * 1024 || p.shortlist < 1 || p.shortlist > (uint32_t) MAX_K || p.n_rows > 0x7FFFFE00u) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_bit_shortlist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ivf_bit_shortlist_kernel, dim3(nq), dim3(256), lds, s, p);
    return hipGetLastError();
}
}  // namespace vsr

// ---- K3: IVFFlat list probe (ivfscan.c:36-176, 339-389) over a list-ordered view of the corpus
// [lists][dim] -> [dim][lists]: the layout ivf_probe_kernel reads (vsr_kernels.hip)
// (T = float, or uint16_t: the binary16 centres of a halfvec index)
template <class T> static std::vector<T> transpose_centers(const T* centers, int lists, int dim)
{
    std::vector<T> t((size_t) lists * dim);
    for (int c = 0; c < lists; ++c)
        for (int j = 0; j < dim; ++j) t[(size_t) j * lists + c] = centers[(size_t) c * dim + j];
    return t;
}

struct vsr_ivf {
    vsr_corpus* main = nullptr;
    vsr_corpus* view = nullptr;                      // list-ordered rows; view->base = main
    int         lists = 0;
    void*       d_centers = nullptr;                 // [dim][lists] fp32; binary16 when the view's rows are (vsr_ivf_load_half, K3h);
                                                     // [words][lists] packed bits over a bit corpus (vsr_ivf_load_bit, K3b)
    std::vector<uint32_t> list_start;                // lists + 1 offsets into the view
    std::vector<vsr_filter*> list_filters;           // one RANGES filter per list (tiles over the view)
    struct ViewBitmap { uint64_t* d = nullptr; std::vector<uint64_t> h; };
    std::map<uint64_t, ViewBitmap> view_bitmaps;                          // a base filter (by vsr_filter::id) as a bitmap in view order
    std::map<std::pair<uint64_t, int>, vsr_filter*> parts;                // (base filter id, list) -> part of a probe
    DevBuf d_q, d_probe;
    DevBuf d_qwords;                                 // bit index: the probe's queries as whole words, pad bits clear
    uint32_t* d_list_start = nullptr;                // list_start on the device (the iterative scan walks lists there)
    PinBuf h_vb;                                     // iterative scan: per query, its view bitmap's device address
    DevBuf d_res;                                    // iterative scan, host form: the results before they go back
    // vsr_ivf_search_quantized*: the per-query view-bitmap addresses on their way into the context's scratch.  The kernel reads the
    // scratch copy; the event guards the pinned block against the next call's rewrite until that copy has run
    PinBuf h_vbq;
    hipEvent_t vbq_done = nullptr;
    bool vbq_pending = false;
};

static bool ivf_half(const vsr_ivf* ivf) { return ivf->view->format == RowFormat::HALF; }
static bool ivf_bit(const vsr_ivf* ivf) { return ivf->view->format == RowFormat::BIT; }

// K3b: the centres of a bit index as the bit centre key reads them (IVF_BIT, vsr_exact.h): [words][lists] 32-bit words of packed
// bits, word w of every list contiguous; the caller's pad bits are cleared on the way
static uint32_t bit_words(int dim) { return ((uint32_t) dim + 31u) / 32u; }
static std::vector<uint32_t> pack_bit_centers(const uint8_t* centers, int lists, int dim)
{
    const size_t words = bit_words(dim), bytes = ((size_t) dim + 7) / 8;
    const uint8_t last = (dim & 7) ? (uint8_t) (0xFF00u >> (dim & 7)) : (uint8_t) 0xFF;
    std::vector<uint32_t> t(words * (size_t) lists, 0u), one(words);
    for (int c = 0; c < lists; ++c) {
        std::fill(one.begin(), one.end(), 0u);
        uint8_t* b = reinterpret_cast<uint8_t*>(one.data());
        memcpy(b, centers + (size_t) c * bytes, bytes);
        b[bytes - 1] &= last;
        for (size_t w = 0; w < words; ++w) t[w * lists + c] = one[w];
    }
    return t;
}

extern "C" int vsr_ivf_free(vsr_ivf* ivf)
{
    if (!ivf) return VSR_OK;
    if (ivf->main) {
        (void) hipSetDevice(ivf->main->ctx->device);
        (void) hipStreamSynchronize(ivf->main->ctx->stream);
    }
    if (ivf->main) {
        auto& reg = ivf->main->ivf_indexes;
        reg.erase(std::remove(reg.begin(), reg.end(), ivf), reg.end());
    }
    for (auto& kv : ivf->parts) delete kv.second;    // tiles / bitmaps are borrowed
    for (auto& kv : ivf->view_bitmaps)
        if (kv.second.d) (void) hipFree(kv.second.d);
    for (vsr_filter* f : ivf->list_filters) free_filter(f);
    if (ivf->d_centers) (void) hipFree(ivf->d_centers);
    if (ivf->d_list_start) (void) hipFree(ivf->d_list_start);
    ivf->h_vb.release();
    ivf->h_vbq.release();
    if (ivf->vbq_done) (void) hipEventDestroy(ivf->vbq_done);
    ivf->d_res.release();
    ivf->d_q.release();
    ivf->d_qwords.release();
    ivf->d_probe.release();
    delete ivf->view;                                // frees the view's own arrays only
    delete ivf;
    return VSR_OK;
}

// what vsr_ivf_load / vsr_ivf_assign (expect = F32), their _half forms (HALF) and their _bit forms (BIT, K3b) refuse alike
static int ivf_check_corpus(const vsr_corpus* c, RowFormat expect, int lists, const char* who)
{
    if (c->base) return fail(VSR_ERR_INVALID, "%s: the corpus is a view", who);
    if (expect == RowFormat::HALF && c->format != RowFormat::HALF) return fail(VSR_ERR_INVALID, "%s: the corpus is not a halfvec corpus", who);
    if (expect == RowFormat::BIT && c->format != RowFormat::BIT) return fail(VSR_ERR_INVALID, "%s: the corpus is not a bit corpus", who);
    if (expect == RowFormat::BIT) {
        if (lists < 1 || lists > 32768) return fail(VSR_ERR_UNSUPPORTED, "%s: lists must be between 1 and 32768 (got %d)", who, lists);
        return VSR_OK;
    }
    if (c->format == RowFormat::HALF && expect != RowFormat::HALF)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a halfvec corpus is indexed with vsr_ivf_kmeans_half / vsr_ivf_assign_half / vsr_ivf_load_half "
                    "(the halfvec_*_ops opclasses)", who);
    if (c->format == RowFormat::SPARSE) return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)", who);
    if (c->format == RowFormat::BIT) return fail(VSR_ERR_UNSUPPORTED, "%s: a bit corpus has no index path yet (the bit_hamming_ops / bit_jaccard_ops opclasses)", who);
    if (lists < 1 || lists > 32768)      /* reloption lists: 1 .. IVFFLAT_MAX_LISTS (ivfflat.h:42-44) */
        return fail(VSR_ERR_UNSUPPORTED, "%s: lists must be between 1 and 32768 (got %d)", who, lists);
    return VSR_OK;
}

// vsr_ivf_load (T = float) and vsr_ivf_load_half (T = uint16_t: binary16 centres over a halfvec corpus, K3h).  The half view
// holds the rows as the corpus does, stride4 / 2 chunks of 8 binary16 values, and no planes: nothing is widened.
// vsr_ivf_load_bit (T = uint8_t, K3b): packed centres over a bit corpus.  The view holds the packed rows (stride4 chunks), their
// popcounts (d_norm2) and the rank map; no planes, no class view; the centres are resident packed and transposed by word.
template <class T> constexpr RowFormat ivf_format()
{
    return std::is_same<T, uint8_t>::value ? RowFormat::BIT : std::is_same<T, uint16_t>::value ? RowFormat::HALF : RowFormat::F32;
}

template <class T>
static int ivf_load(vsr_corpus* c, const T* centers, int lists, const int32_t* row_list, vsr_ivf** out, const char* who)
{
    constexpr RowFormat FMT = ivf_format<T>();
    if (!c || !out || !centers || (c->n > 0 && !row_list)) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    int rc = ivf_check_corpus(c, FMT, lists, who);
    if (rc) return rc;
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    for (int64_t i = 0; i < n; ++i)
        if (row_list[i] < 0 || row_list[i] >= lists) return fail(VSR_ERR_INVALID, "%s: row %lld has list %d", who, (long long) i, row_list[i]);
    std::unique_ptr<vsr_ivf> ivf(new vsr_ivf());
    ivf->main = c;
    ivf->lists = lists;
    // view order: by list, then by base row (= (document_id, block_id) order inside a list)
    std::vector<uint32_t> count((size_t) lists + 1, 0);
    for (int64_t r = 0; r < n; ++r) count[(size_t) row_list[c->h_orig[(size_t) r]] + 1]++;
    for (int l = 0; l < lists; ++l) count[(size_t) l + 1] += count[(size_t) l];
    ivf->list_start = count;
    std::vector<uint32_t> rank((size_t) std::max<int64_t>(n, 1));
    {
        std::vector<uint32_t> cur(count.begin(), count.end() - 1);
        for (int64_t r = 0; r < n; ++r) rank[cur[(size_t) row_list[c->h_orig[(size_t) r]]]++] = (uint32_t) r;
    }
    std::unique_ptr<vsr_corpus> v(new vsr_corpus());
    v->ctx = ctx;
    v->n = n;
    v->dim = c->dim;
    v->stride4 = c->stride4;
    v->row_offset = c->row_offset;
    v->shape = c->shape;
    v->base = c;
    v->k2_safe = c->k2_safe;
    v->format = FMT;
    const uint32_t row_chunks = format_row_chunks(FMT, c->dim);   // (the gather moves 16-byte chunks, whatever they hold)
    const size_t alloc_rows = (size_t) std::max<int64_t>(n, 1), row_bytes = (size_t) row_chunks * 16;
    HIPCHK(hipMalloc(&v->d_rank, alloc_rows * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(v->d_rank, rank.data(), alloc_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&v->d_rows, alloc_rows * row_bytes + 1024));
    HIPCHK(hipMalloc(&v->d_norm2, alloc_rows * sizeof(float)));
    HIPCHK(launch_gather_rows(c->d_rows, c->d_norm2, v->d_rank, (uint32_t) n, row_chunks, v->d_rows, v->d_norm2, ctx->stream));
    if (c->d_scr) {                                  // the view's own screening planes, in its order
        v->scr_has_mid = c->scr_has_mid;
        v->pstride4 = c->pstride4;
        HIPCHK(hipMalloc(&v->d_scr, alloc_rows * (size_t) v->pstride4 * 16 + 1024));
        HIPCHK(launch_split_planes(v->d_rows, (uint32_t) n, v->stride4, v->d_scr, v->pstride4, !v->scr_has_mid, ctx->stream));
        std::vector<uint2> all;
        ranges_to_tiles({{0u, (uint32_t) n}}, v->shape.rw, all);
        HIPCHK(hipMalloc(&v->d_all_tiles, std::max<size_t>(8, all.size() * sizeof(uint2))));
        if (!all.empty()) HIPCHK(hipMemcpy(v->d_all_tiles, all.data(), all.size() * sizeof(uint2), hipMemcpyHostToDevice));
    }
    if constexpr (FMT == RowFormat::BIT) {
        const std::vector<uint32_t> ct = pack_bit_centers(centers, lists, c->dim);
        HIPCHK(hipMalloc(&ivf->d_centers, ct.size() * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(ivf->d_centers, ct.data(), ct.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    } else {                                                // transposed for the probe kernel: element j of every list contiguous
        HIPCHK(hipMalloc(&ivf->d_centers, (size_t) lists * c->dim * sizeof(T)));
        std::vector<T> ct = transpose_centers(centers, lists, c->dim);
        HIPCHK(hipMemcpy(ivf->d_centers, ct.data(), ct.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&ivf->d_list_start, ((size_t) lists + 1) * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(ivf->d_list_start, ivf->list_start.data(), ((size_t) lists + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ivf->view = v.release();
    ivf->list_filters.assign((size_t) lists, nullptr);
    for (int l = 0; l < lists; ++l) {
        FilterPtr f = new_filter(ivf->view, VSR_FILTER_RANGES, true);
        std::vector<uint2> tiles;
        const uint32_t s0 = ivf->list_start[(size_t) l], s1 = ivf->list_start[(size_t) l + 1];
        if (s1 > s0) ranges_to_tiles({{s0, s1}}, ivf->view->shape.rw, tiles);
        int rc = upload_tiles(f.get(), tiles);
        if (rc) { vsr_ivf_free(ivf.release()); return rc; }
        f->allowed_rows = f->scanned_rows = s1 - s0;
        ivf->list_filters[(size_t) l] = f.release();
    }
    c->ivf_indexes.push_back(ivf.get());
    *out = ivf.release();
    return VSR_OK;
}

extern "C" int vsr_ivf_load(vsr_corpus* c, const float* centers, int lists, const int32_t* row_list, vsr_ivf** out)
{
    return ivf_load(c, centers, lists, row_list, out, "vsr_ivf_load");
}

extern "C" int vsr_ivf_load_half(vsr_corpus* c, const uint16_t* centers, int lists, const int32_t* row_list, vsr_ivf** out)
{
    return ivf_load(c, centers, lists, row_list, out, "vsr_ivf_load_half");
}

extern "C" int vsr_ivf_load_bit(vsr_corpus* c, const uint8_t* centers, int lists, const int32_t* row_list, vsr_ivf** out)
{
    return ivf_load(c, centers, lists, row_list, out, "vsr_ivf_load_bit");
}

// the view's rows, norms (bit index: popcounts) and rank, the centres (bit index: packed) and the list offsets (cached per-filter bitmaps and tile lists are not counted)
extern "C" int64_t vsr_ivf_device_bytes(const vsr_ivf* ivf)
{
    if (!ivf) return 0;
    const vsr_corpus* v = ivf->view;
    const size_t rows = (size_t) std::max<int64_t>(v->n, 1);
    size_t b = rows * format_row_chunks(v->format, v->dim) * 16 + 1024 + rows * sizeof(float) + rows * sizeof(uint32_t);
    if (v->d_scr) b += rows * (size_t) v->pstride4 * 16 + 1024;
    b += ivf_bit(ivf) ? (size_t) ivf->lists * bit_words(v->dim) * 4 : (size_t) ivf->lists * v->dim * (ivf_half(ivf) ? 2 : 4);
    b += ((size_t) ivf->lists + 1) * sizeof(uint32_t);
    return (int64_t) b;
}

void vsr::purge_ivf_caches(vsr_corpus* c, const vsr_filter* f)
{
    for (vsr_ivf* ivf : c->ivf_indexes) {
        for (auto it = ivf->parts.begin(); it != ivf->parts.end();) {
            if (!f || it->first.first == f->id) {
                delete it->second;                           // tiles / bitmap are borrowed
                it = ivf->parts.erase(it);
            } else
                ++it;
        }
        for (auto it = ivf->view_bitmaps.begin(); it != ivf->view_bitmaps.end();) {
            if (!f || it->first == f->id) {
                if (it->second.d) (void) hipFree(it->second.d);
                it = ivf->view_bitmaps.erase(it);
            } else
                ++it;
        }
    }
}

// a filter of the base corpus as permission bits in view order (device and host copies), built on first use
static int ivf_view_bitmap(vsr_ivf* ivf, const vsr_filter* bf, vsr_ivf::ViewBitmap** out)
{
    vsr_corpus* v = ivf->view;
    vsr_ctx* ctx = v->ctx;
    auto& vb = ivf->view_bitmaps[bf->id];
    if (!vb.d) {
        const size_t words = bitmap_words(v->n);
        HIPCHK(hipMalloc(&vb.d, words * sizeof(uint64_t)));
        HIPCHK(hipMemsetAsync(vb.d, 0, words * sizeof(uint64_t), ctx->stream));
        HIPCHK(launch_view_bitmap(v->d_rank, (uint32_t) v->n, bf->d_tiles, bf->n_tiles, bf->d_bitmap, vb.d, ctx->stream));
        vb.h.resize(words);
        HIPCHK(hipMemcpyAsync(vb.h.data(), vb.d, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    *out = &vb;
    return VSR_OK;
}

// (base filter, list) as a filter of the view: the list's tiles and the base filter's bitmap in view order
static int ivf_part(vsr_ivf* ivf, const vsr_filter* bf, int list, vsr_filter** out)
{
    if (!bf) {
        *out = ivf->list_filters[(size_t) list];
        return VSR_OK;
    }
    auto key = std::make_pair(bf->id, list);
    auto it = ivf->parts.find(key);
    if (it != ivf->parts.end()) {
        *out = it->second;
        return VSR_OK;
    }
    vsr_corpus* v = ivf->view;
    vsr_ivf::ViewBitmap* vbp = nullptr;
    int rc = ivf_view_bitmap(ivf, bf, &vbp);
    if (rc) return rc;
    vsr_ivf::ViewBitmap& vb = *vbp;
    const vsr_filter* lf = ivf->list_filters[(size_t) list];
    std::unique_ptr<vsr_filter> f(new vsr_filter());
    f->corpus = v;
    f->mode = VSR_FILTER_BITMAP;
    f->cached = true;
    f->d_tiles = lf->d_tiles;
    f->n_tiles = lf->n_tiles;
    f->d_bitmap = vb.d;
    f->owns_bitmap = false;
    f->scanned_rows = lf->scanned_rows;
    int64_t allowed = 0;
    for (uint32_t p = ivf->list_start[(size_t) list]; p < ivf->list_start[(size_t) list + 1]; ++p)
        allowed += (vb.h[p >> 6] >> (p & 63)) & 1ull;
    f->allowed_rows = allowed;
    *out = ivf->parts[key] = f.release();
    return VSR_OK;
}

// the probe launch on device-resident queries; the probed list ids (nq x probes) back to the host, synchronised
// (bit index: d_queries are packed bit strings; they are staged as whole words with the pad bits clear, the centre key's query side)
static int ivf_probe_lists(vsr_ivf* ivf, const void* d_queries, int nq, int dim, int probes, int metric, int32_t* out_lists)
{
    vsr_ctx* ctx = ivf->main->ctx;
    int rc;
    if ((rc = ivf->d_probe.reserve((size_t) nq * probes * sizeof(int32_t)))) return rc;
    if (ivf_bit(ivf)) {
        const uint32_t words = bit_words(dim), q_bytes = (uint32_t) format_query_bytes(RowFormat::BIT, dim);
        if ((rc = ivf->d_qwords.reserve((size_t) nq * words * 4))) return rc;
        HIPCHK(launch_pack_bits(static_cast<const uint8_t*>(d_queries), q_bytes, (uint32_t) nq, (uint32_t) dim, ivf->d_qwords.as<uint8_t>(),
                                words * 4, ctx->stream));
        HIPCHK(launch_ivf_probe(ivf->d_qwords.p, words, (uint32_t) nq, ivf->d_centers, (int) words, ivf->lists, probes, 0,
                                ivf->d_probe.as<int32_t>(), ctx->stream, IVF_BIT));
        HIPCHK(hipMemcpyAsync(out_lists, ivf->d_probe.p, (size_t) nq * probes * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    }
    // cosine opclass: the caller passes normalised queries and the index distance is the negative inner product
    // (vector.sql:323-327)
    HIPCHK(launch_ivf_probe(d_queries, (uint32_t) dim, (uint32_t) nq, ivf->d_centers, dim, ivf->lists, probes,
                            metric == VSR_METRIC_L2 ? M_L2 : M_IP, ivf->d_probe.as<int32_t>(), ctx->stream,
                            ivf_half(ivf) ? IVF_HALF_Q32 : IVF_F32));
    HIPCHK(hipMemcpyAsync(out_lists, ivf->d_probe.p, (size_t) nq * probes * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VSR_OK;
}

// GetScanLists + the per-query filters of GetScanItems: the probe launch on device-resident queries, the probed list
// ids back to the host (nq x probes x 4 bytes: the planner that groups queries by list is host code), one parts-only
// filter of the view per query.
static int ivf_plan(vsr_ivf* ivf, const void* d_queries, int nq, int dim, int probes, int metric,
                    const vsr_filter* const* filters, std::vector<std::unique_ptr<vsr_filter>>& owned,
                    std::vector<const vsr_filter*>& fl)
{
    int rc;
    std::vector<int32_t> probe((size_t) nq * probes);
    if ((rc = ivf_probe_lists(ivf, d_queries, nq, dim, probes, metric, probe.data()))) return rc;
    owned.resize((size_t) nq);
    fl.assign((size_t) nq, nullptr);
    for (int q = 0; q < nq; ++q) {
        std::unique_ptr<vsr_filter> f(new vsr_filter());
        f->corpus = ivf->view;
        f->mode = VSR_FILTER_RANGES;
        f->parts_only = true;
        for (int j = 0; j < probes; ++j) {
            const int32_t l = probe[(size_t) q * probes + j];
            if (l < 0) continue;
            vsr_filter* part = nullptr;
            if ((rc = ivf_part(ivf, filters ? filters[q] : nullptr, l, &part))) return rc;
            if (part->n_tiles == 0) continue;
            f->parts.push_back(part);
            f->allowed_rows += part->allowed_rows;
            f->scanned_rows += part->scanned_rows;
        }
        fl[(size_t) q] = f.get();
        owned[(size_t) q] = std::move(f);
    }
    return VSR_OK;
}

// entry: what the entry point's queries are -- F32 (vsr_ivf_search*: an fp32 or a halfvec index) or BIT (vsr_ivf_search_bit*: a bit index)
static int ivf_check_entry(const vsr_ivf* ivf, RowFormat entry, const char* who)
{
    if (!ivf) return fail(VSR_ERR_INVALID, "%s: index is NULL", who);
    if (entry == RowFormat::BIT && !ivf_bit(ivf))
        return fail(VSR_ERR_INVALID, "%s: the index is not over a bit corpus (it is searched with vsr_ivf_search*)", who);
    if (entry != RowFormat::BIT && ivf_bit(ivf))
        return fail(VSR_ERR_UNSUPPORTED, "%s: the index is over a bit corpus: it is searched with vsr_ivf_search_bit* (<~>)", who);
    return VSR_OK;
}

static int ivf_check_probes(int probes, const char* who)
{
    if (probes < 1) return fail(VSR_ERR_INVALID, "%s: probes must be >= 1 (got %d)", who, probes);   /* ivfflat.c:41-45 */
    return VSR_OK;
}

// the two arguments of the iterative forms (GUC ranges: ivfflat.c:20-51)
static int ivf_check_iterative(int mode, int max_probes, const char* who)
{
    if (mode != VSR_IVF_ITERATIVE_OFF && mode != VSR_IVF_ITERATIVE_RELAXED)
        return fail(VSR_ERR_INVALID, "%s: iterative scan mode %d (ivfflat has off and relaxed_order)", who, mode);
    if (max_probes < 1 || max_probes > 32768)
        return fail(VSR_ERR_INVALID, "%s: max_probes must be between 1 and 32768 (got %d)", who, max_probes);
    return VSR_OK;
}

static int ivf_check(vsr_ivf* ivf, RowFormat entry, const void* queries, int nq, int dim, int k, int& probes, int metric,
                     const vsr_filter* const* filters, const void* o1, const void* o2, const void* o3, const char* who)
{
    int rc = ivf_check_entry(ivf, entry, who);
    if (rc) return rc;
    if ((rc = check_search_args(ivf->main, queries, nq, dim, k, metric, filters, who, entry))) return rc;
    if (metric == VSR_METRIC_JACCARD) return fail(VSR_ERR_UNSUPPORTED, "%s: ivfflat has no bit_jaccard_ops operator class", who);
    if (metric == VSR_METRIC_L1) return fail(VSR_ERR_UNSUPPORTED, "%s: ivfflat has no L1 operator class", who);
    if ((rc = ivf_check_probes(probes, who))) return rc;
    if (nq > 0 && (!o1 || !o2 || !o3)) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    probes = std::min(probes, ivf->lists);
    return VSR_OK;
}

// ... and the two arguments of the iterative form
static int ivf_check(vsr_ivf* ivf, RowFormat entry, const void* queries, int nq, int dim, int k, int& probes, int metric,
                     const vsr_filter* const* filters, int mode, int max_probes, const void* o1, const void* o2, const void* o3,
                     const char* who)
{
    int rc = ivf_check(ivf, entry, queries, nq, dim, k, probes, metric, filters, o1, o2, o3, who);
    if (rc) return rc;
    return ivf_check_iterative(mode, max_probes, who);
}

// vsr_ivf_search (entry = F32) and vsr_ivf_search_bit (BIT: packed queries)
static int ivf_search(vsr_ivf* ivf, RowFormat entry, const void* queries, int nq, int dim, int k, int probes, int metric,
                      const vsr_filter* const* filters, const Outputs& out, const char* who)
{
    int rc = ivf_check(ivf, entry, queries, nq, dim, k, probes, metric, filters, out.blk, out.dist, out.cnt, who);
    if (rc || nq == 0) return rc;
    if (ivf_half(ivf) && (rc = half_query_range(queries, nq, dim))) return rc;   // `$1::halfvec`, as vsr_search refuses it
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t q_bytes = (size_t) nq * format_query_bytes(ivf->view->format, dim);
    if ((rc = ivf->d_q.reserve(q_bytes))) return rc;
    HIPCHK(hipMemcpyAsync(ivf->d_q.p, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    std::vector<std::unique_ptr<vsr_filter>> owned;
    std::vector<const vsr_filter*> fl;
    if ((rc = ivf_plan(ivf, ivf->d_q.p, nq, dim, probes, metric, filters, owned, fl))) return rc;
    return host_search(ivf->view, queries, nq, dim, k, metric, fl.data(), out);
}

extern "C" int vsr_ivf_search(vsr_ivf* ivf, const float* queries, int nq, int dim, int k, int probes, int metric,
                              const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                              float* out_dist, int32_t* out_cnt)
{
    return ivf_search(ivf, RowFormat::F32, queries, nq, dim, k, probes, metric, filters, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr},
                      "vsr_ivf_search");
}

extern "C" int vsr_ivf_search_bit(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int k, int probes, int metric,
                                  const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                                  float* out_dist, int32_t* out_cnt)
{
    return ivf_search(ivf, RowFormat::BIT, queries, nq, dim, k, probes, metric, filters, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr},
                      "vsr_ivf_search_bit");
}

// the search over the view with queries and results on the device, every query exact at the return.  A bit view goes through the
// search path of vsr_search_bit_device (K1b: exact by construction, nothing to re-run) and is then waited for.
static int ivf_view_search_device(vsr_ivf* ivf, const void* d_queries, int nq, int dim, int k, int metric, const vsr_filter* const* fl,
                                  const Outputs& o)
{
    if (!ivf_bit(ivf))
        return vsr_search_device_exact(nullptr, ivf->view, static_cast<const float*>(d_queries), nq, dim, k, metric, fl, o.blk, o.doc, o.row,
                                       o.dist, o.cnt, nullptr, nullptr);
    int rc = device_search(ivf->view, d_queries, nq, dim, k, metric, fl, o);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ivf->main->ctx->stream));
    return VSR_OK;
}

// The same with queries and results resident on the device.  Returns when every query is proven exact over its lists
// (vsr_search_device_exact's contract); only the probed list ids cross PCIe.
static int ivf_search_device(vsr_ivf* ivf, RowFormat entry, const void* d_queries, int nq, int dim, int k, int probes, int metric,
                             const vsr_filter* const* filters, const Outputs& o, const char* who)
{
    int rc = ivf_check(ivf, entry, d_queries, nq, dim, k, probes, metric, filters, o.blk, o.dist, o.cnt, who);
    if (rc || nq == 0) return rc;
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<std::unique_ptr<vsr_filter>> owned;
    std::vector<const vsr_filter*> fl;
    if ((rc = ivf_plan(ivf, d_queries, nq, dim, probes, metric, filters, owned, fl))) return rc;
    return ivf_view_search_device(ivf, d_queries, nq, dim, k, metric, fl.data(), o);
}

extern "C" int vsr_ivf_search_device(vsr_ivf* ivf, const float* d_queries, int nq, int dim, int k, int probes, int metric,
                                     const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                     float* d_dist, int32_t* d_cnt)
{
    return ivf_search_device(ivf, RowFormat::F32, d_queries, nq, dim, k, probes, metric, filters, {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr},
                             "vsr_ivf_search_device");
}

extern "C" int vsr_ivf_search_bit_device(vsr_ivf* ivf, const uint8_t* d_queries, int nq, int dim, int k, int probes, int metric,
                                         const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                         float* d_dist, int32_t* d_cnt)
{
    return ivf_search_device(ivf, RowFormat::BIT, d_queries, nq, dim, k, probes, metric, filters, {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr},
                             "vsr_ivf_search_bit_device");
}

// ---- iterative index scans (ivfflat.iterative_scan = relaxed_order, ivfflat.max_probes) ----
static int fill_probes(vsr_ctx* ctx, int32_t* d_probes, int nq, int value)
{
    if (d_probes) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_probes), value, (size_t) nq, ctx->stream));
    return VSR_OK;
}

static int ivf_iterative_device(vsr_ivf* ivf, RowFormat entry, const void* d_queries, int nq, int dim, int k, int probes,
                                int metric, const vsr_filter* const* filters, int mode, int max_probes,
                                int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                int32_t* d_probes, const char* who)
{
    int rc = ivf_check(ivf, entry, d_queries, nq, dim, k, probes, metric, filters, mode, max_probes, d_blk, d_dist, d_cnt, who);
    if (rc || nq == 0) return rc;
    vsr_ctx* ctx = ivf->main->ctx;
    vsr_corpus* v = ivf->view;
    HIPCHK(hipSetDevice(ctx->device));
    // batch 0 = the scan without iteration: the shared matrix-core passes over the `probes` nearest lists, outputs written
    std::vector<std::unique_ptr<vsr_filter>> owned;
    std::vector<const vsr_filter*> fl;
    if ((rc = ivf_plan(ivf, d_queries, nq, dim, probes, metric, filters, owned, fl))) return rc;
    if ((rc = ivf_view_search_device(ivf, d_queries, nq, dim, k, metric, fl.data(), {d_blk, d_doc, d_row, d_dist, d_cnt, nullptr}))) return rc;
    const int max_lists = std::min(std::max(max_probes, probes), ivf->lists);
    if (mode == VSR_IVF_ITERATIVE_OFF || max_lists <= probes) {            // pgvector ignores max_probes when the scan is off
        if ((rc = fill_probes(ctx, d_probes, nq, probes))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    }
    // every later batch in one launch; nothing comes back to the host in between.  Per query the address of its
    // permission bits in view order (the bitmap exists even when batch 0's lists were all empty)
    if ((rc = ivf->h_vb.reserve((size_t) nq * sizeof(uint64_t*)))) return rc;
    const uint64_t** vbs = ivf->h_vb.as<const uint64_t*>();
    for (int q = 0; q < nq; ++q) {
        vbs[q] = nullptr;
        if (filters && filters[q]) {
            vsr_ivf::ViewBitmap* vb = nullptr;
            if ((rc = ivf_view_bitmap(ivf, filters[q], &vb))) return rc;
            vbs[q] = vb->d;
        }
    }
    IvfIterParams p{};
    p.queries = static_cast<const float*>(d_queries);
    p.q_stride = ivf_bit(ivf) ? (uint32_t) format_query_bytes(RowFormat::BIT, dim) : (uint32_t) dim;   // (bit index: bytes)
    p.dim = (uint32_t) dim;
    p.centers_t = ivf->d_centers;
    p.lists = (uint32_t) ivf->lists;
    p.center_metric = metric == VSR_METRIC_L2 ? M_L2 : M_IP;              // as the probe: cosine opclass = negative inner product
    p.metric = metric;
    p.probes = (uint32_t) probes;
    p.max_lists = (uint32_t) max_lists;
    p.k = (uint32_t) k;
    p.list_start = ivf->d_list_start;
    p.rows = v->d_rows;
    p.rows_half = ivf_half(ivf) ? 1u : 0u;
    p.rows_bit = ivf_bit(ivf) ? 1u : 0u;
    p.stride4 = v->stride4;
    p.n_rows = (uint32_t) v->n;
    p.rank = v->d_rank;
    p.bitmaps = reinterpret_cast<const uint64_t* const*>(ivf->h_vb.dp);
    set_results(p, ivf->main, Outputs{d_blk, d_doc, d_row, d_dist, d_cnt, nullptr});
    p.out_probes = d_probes;
    hipError_t e = launch_ivf_iterative(p, (uint32_t) nq, ctx->stream);
    if (e == hipErrorInvalidValue)
        return fail(VSR_ERR_UNSUPPORTED, "vsr_ivf_search_iterative: %d lists x %d dimensions x k = %d need more than the 160 KiB of LDS",
                    ivf->lists, dim, k);
    HIPCHK(e);
    HIPCHK(hipStreamSynchronize(ctx->stream));                             // (h_vb is reused by the next call)
    return VSR_OK;
}

extern "C" int vsr_ivf_search_iterative_device(vsr_ivf* ivf, const float* d_queries, int nq, int dim, int k, int probes,
                                               int metric, const vsr_filter* const* filters, int mode, int max_probes,
                                               int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                               int32_t* d_probes)
{
    return ivf_iterative_device(ivf, RowFormat::F32, d_queries, nq, dim, k, probes, metric, filters, mode, max_probes, d_blk, d_doc, d_row,
                                d_dist, d_cnt, d_probes, "vsr_ivf_search_iterative_device");
}

extern "C" int vsr_ivf_search_bit_iterative_device(vsr_ivf* ivf, const uint8_t* d_queries, int nq, int dim, int k, int probes,
                                                   int metric, const vsr_filter* const* filters, int mode, int max_probes,
                                                   int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                                   int32_t* d_probes)
{
    return ivf_iterative_device(ivf, RowFormat::BIT, d_queries, nq, dim, k, probes, metric, filters, mode, max_probes, d_blk, d_doc, d_row,
                                d_dist, d_cnt, d_probes, "vsr_ivf_search_bit_iterative_device");
}

static int ivf_iterative(vsr_ivf* ivf, RowFormat entry, const void* queries, int nq, int dim, int k, int probes, int metric,
                         const vsr_filter* const* filters, int mode, int max_probes, int64_t* out_blk,
                         int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int32_t* out_probes, const char* who)
{
    int rc = ivf_check(ivf, entry, queries, nq, dim, k, probes, metric, filters, mode, max_probes, out_blk, out_dist, out_cnt, who);
    if (rc || nq == 0) return rc;
    if (mode == VSR_IVF_ITERATIVE_OFF || std::min(std::max(max_probes, probes), ivf->lists) <= probes) {
        if ((rc = ivf_search(ivf, entry, queries, nq, dim, k, probes, metric, filters, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, who)))
            return rc;
        if (out_probes) std::fill(out_probes, out_probes + nq, (int32_t) probes);
        return VSR_OK;
    }
    if (ivf_half(ivf) && (rc = half_query_range(queries, nq, dim))) return rc;
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    // queries up, the device form, results down
    const ResultBlock rb(nq, k, true);                                     // (extra column: the lists scanned)
    const size_t q_bytes = (size_t) nq * format_query_bytes(ivf->view->format, dim);
    if ((rc = ivf->d_q.reserve(q_bytes))) return rc;
    if ((rc = ivf->d_res.reserve(rb.total))) return rc;
    HIPCHK(hipMemcpyAsync(ivf->d_q.p, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    char* d = ivf->d_res.as<char>();
    const Outputs o = rb.arrays(d);
    int32_t* d_probes = rb.column<int32_t>(d, rb.o_extra);
    if ((rc = ivf_iterative_device(ivf, entry, ivf->d_q.p, nq, dim, k, probes, metric, filters, mode, max_probes, o.blk, o.doc, o.row, o.dist,
                                   o.cnt, d_probes, who)))
        return rc;
    std::vector<char> h(rb.o_status);
    HIPCHK(hipMemcpy(h.data(), d, rb.o_status, hipMemcpyDeviceToHost));
    rb.copy_out_all(h.data(), {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    if (out_probes) memcpy(out_probes, rb.column<int32_t>(h.data(), rb.o_extra), (size_t) nq * sizeof(int32_t));
    return VSR_OK;
}

extern "C" int vsr_ivf_search_iterative(vsr_ivf* ivf, const float* queries, int nq, int dim, int k, int probes, int metric,
                                        const vsr_filter* const* filters, int mode, int max_probes, int64_t* out_blk,
                                        int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int32_t* out_probes)
{
    return ivf_iterative(ivf, RowFormat::F32, queries, nq, dim, k, probes, metric, filters, mode, max_probes, out_blk, out_doc, out_row,
                         out_dist, out_cnt, out_probes, "vsr_ivf_search_iterative");
}

extern "C" int vsr_ivf_search_bit_iterative(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int k, int probes, int metric,
                                            const vsr_filter* const* filters, int mode, int max_probes, int64_t* out_blk,
                                            int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt, int32_t* out_probes)
{
    return ivf_iterative(ivf, RowFormat::BIT, queries, nq, dim, k, probes, metric, filters, mode, max_probes, out_blk, out_doc, out_row,
                         out_dist, out_cnt, out_probes, "vsr_ivf_search_bit_iterative");
}

// ---- two-stage search through the bit index: the Hamming shortlist from the lists (K3q), the exact re-rank on the source rows ----
// vsr_search_quantized with stage 1 replaced by the index, everything on the bit corpus context's stream with no host round trip:
// the per-query table of view-order bitmap addresses (a stream-ordered copy into the context's scratch: the kernel never reads
// the pinned block, which the next call rewrites) -> ONE K3q launch, which quantizes the queries itself and starts at the first
// list -> the re-rank and emit launches of vsr_shortlist.h (quantized_rerank, vsr_search.hip).  Exactly one of h_queries /
// d_queries is set; `out` and d_probes address device memory either way.
static int ivf_quantized_impl(vsr_corpus* src, vsr_ivf* ivf, const float* h_queries, const float* d_queries, int nq, int dim, int k,
                              int shortlist, int probes, int metric, const vsr_filter* const* filters, int mode, int max_probes,
                              const Outputs& out, int32_t* d_probes, const char* who)
{
    vsr_corpus* bits = ivf->main;
    vsr_corpus* v = ivf->view;
    vsr_ctx* ctx = bits->ctx;
    int rc;
    const size_t ns = (size_t) nq * (size_t) shortlist;
    // scratch: [fp32 queries of a host call | bitmap addresses | stage-1 keys | re-rank keys | stage-1 counts]
    const size_t o_q = 0, o_vb = align_up(o_q + (h_queries ? (size_t) nq * dim * sizeof(float) : 0), 256),
                 o_key = align_up(o_vb + (size_t) nq * sizeof(uint64_t*), 256), o_rr = align_up(o_key + ns * 8, 256),
                 o_cnt = align_up(o_rr + ns * 8, 256), total = align_up(o_cnt + (size_t) nq * 4, 256);
    if ((rc = ctx->d_short.reserve(total))) return rc;
    char* w = ctx->d_short.as<char>();
    if (h_queries) {
        HIPCHK(hipMemcpyAsync(w + o_q, h_queries, (size_t) nq * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        d_queries = reinterpret_cast<const float*>(w + o_q);
    }
    bool any_filter = false;
    if (filters)
        for (int q = 0; q < nq && !any_filter; ++q) any_filter = filters[q] != nullptr;
    if (any_filter) {
        if (ivf->vbq_pending) {                                            // the previous call's copy still owns the pinned block
            HIPCHK(hipEventSynchronize(ivf->vbq_done));
            ivf->vbq_pending = false;
        }
        if (!ivf->vbq_done) HIPCHK(hipEventCreateWithFlags(&ivf->vbq_done, hipEventDisableTiming));
        if ((rc = ivf->h_vbq.reserve((size_t) nq * sizeof(uint64_t*)))) return rc;
        const uint64_t** vbs = ivf->h_vbq.as<const uint64_t*>();
        for (int q = 0; q < nq; ++q) {
            vbs[q] = nullptr;
            if (filters[q]) {
                vsr_ivf::ViewBitmap* vb = nullptr;
                if ((rc = ivf_view_bitmap(ivf, filters[q], &vb))) return rc;    // (built, and waited for, on a filter's first use)
                vbs[q] = vb->d;
            }
        }
        HIPCHK(hipMemcpyAsync(w + o_vb, vbs, (size_t) nq * sizeof(uint64_t*), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipEventRecord(ivf->vbq_done, ctx->stream));
        ivf->vbq_pending = true;
    }
    uint64_t* s1_keys = reinterpret_cast<uint64_t*>(w + o_key);
    IvfShortlistParams p{};
    p.queries = d_queries;
    p.dim = (uint32_t) dim;
    p.centers_t = ivf->d_centers;
    p.lists = (uint32_t) ivf->lists;
    p.probes = (uint32_t) probes;
    // pgvector ignores max_probes when the scan is off
    p.max_lists = (uint32_t) (mode == VSR_IVF_ITERATIVE_OFF ? probes : std::min(std::max(max_probes, probes), ivf->lists));
    p.shortlist = (uint32_t) shortlist;
    p.list_start = ivf->d_list_start;
    p.rows = reinterpret_cast<const uint4*>(v->d_rows);
    p.stride4 = v->stride4;
    p.n_rows = (uint32_t) v->n;
    p.rank = v->d_rank;
    p.bitmaps = any_filter ? reinterpret_cast<const uint64_t* const*>(w + o_vb) : nullptr;
    p.row_offset = (uint32_t) bits->row_offset;
    p.s1_keys = s1_keys;
    p.out_count = reinterpret_cast<int32_t*>(w + o_cnt);
    p.out_probes = d_probes;
    hipError_t e = launch_ivf_bit_shortlist(p, (uint32_t) nq, ctx->stream);
    if (e == hipErrorInvalidValue)
        return fail(VSR_ERR_UNSUPPORTED, "%s: %d lists x %d bits x shortlist = %d need more than the 160 KiB of LDS", who, ivf->lists, dim, shortlist);
    HIPCHK(e);
    ctx->last_kernel = "ivf_bit_shortlist_kernel";
    return quantized_rerank(ctx, src, s1_keys, (uint32_t) bits->row_offset, reinterpret_cast<uint64_t*>(w + o_rr), d_queries, nq, dim, k,
                            shortlist, metric, out);
}

static int ivf_quantized_check(vsr_corpus* src, vsr_ivf* ivf, const void* queries, int nq, int dim, int k, int shortlist, int& probes,
                               int metric, const vsr_filter* const* filters, int mode, int max_probes, const char* who)
{
    int rc = ivf_check_entry(ivf, RowFormat::BIT, who);
    if (rc) return rc;
    if ((rc = check_quantized_args(nullptr, src, ivf->main, queries, nq, dim, k, shortlist, metric, filters, who))) return rc;
    if ((rc = ivf_check_probes(probes, who))) return rc;
    if ((rc = ivf_check_iterative(mode, max_probes, who))) return rc;
    probes = std::min(probes, ivf->lists);
    return VSR_OK;
}

extern "C" int vsr_ivf_search_quantized_device(vsr_corpus* src, vsr_ivf* ivf, const float* d_queries, int nq, int dim, int k,
                                               int shortlist, int probes, int metric, const vsr_filter* const* filters, int mode,
                                               int max_probes, int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist,
                                               int32_t* d_cnt, int32_t* d_probes, uint64_t* d_keys)
{
    const char* who = "vsr_ivf_search_quantized_device";
    int rc = ivf_quantized_check(src, ivf, d_queries, nq, dim, k, shortlist, probes, metric, filters, mode, max_probes, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    HIPCHK(hipSetDevice(ivf->main->ctx->device));
    return ivf_quantized_impl(src, ivf, nullptr, d_queries, nq, dim, k, shortlist, probes, metric, filters, mode, max_probes,
                              {d_blk, d_doc, d_row, d_dist, d_cnt, d_keys}, d_probes, who);
}

extern "C" int vsr_ivf_search_quantized(vsr_corpus* src, vsr_ivf* ivf, const float* queries, int nq, int dim, int k, int shortlist,
                                        int probes, int metric, const vsr_filter* const* filters, int mode, int max_probes,
                                        int64_t* out_blk, int32_t* out_doc, int64_t* out_row, float* out_dist, int32_t* out_cnt,
                                        int32_t* out_probes)
{
    const char* who = "vsr_ivf_search_quantized";
    int rc = ivf_quantized_check(src, ivf, queries, nq, dim, k, shortlist, probes, metric, filters, mode, max_probes, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    if (src->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;   // `$1::halfvec`, as vsr_search refuses it
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    // queries up, the device form's launches, results down: one packed copy back, one wait
    const ResultBlock rb(nq, k, true);                                     // (extra column: the lists scanned)
    if ((rc = ctx->d_out.reserve(rb.o_status))) return rc;
    if ((rc = ctx->h_out.reserve(rb.total))) return rc;
    char* d = ctx->d_out.as<char>();
    char* h = ctx->h_out.as<char>();
    int32_t* d_probes = rb.column<int32_t>(d, rb.o_extra);
    if ((rc = ivf_quantized_impl(src, ivf, queries, nullptr, nq, dim, k, shortlist, probes, metric, filters, mode, max_probes, rb.arrays(d),
                                 d_probes, who)))
        return rc;
    HIPCHK(hipMemcpyAsync(h, d, rb.o_status, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rb.copy_out_all(h, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    if (out_probes) memcpy(out_probes, rb.column<int32_t>(h, rb.o_extra), (size_t) nq * sizeof(int32_t));
    return VSR_OK;
}

extern "C" int vsr_ivf_probe(vsr_ivf* ivf, const float* queries, int nq, int dim, int probes, int metric, int32_t* out_lists)
{
    if (!ivf || !queries || !out_lists || nq < 0) return fail(VSR_ERR_INVALID, "vsr_ivf_probe: NULL argument");
    int rc = ivf_check_entry(ivf, RowFormat::F32, "vsr_ivf_probe");
    if (rc) return rc;
    if (dim != ivf->main->dim)
        return fail(VSR_ERR_DIM_MISMATCH, "different %s dimensions %d and %d", format_name(ivf->main->format), ivf->main->dim, dim);
    if (probes < 1) return fail(VSR_ERR_INVALID, "vsr_ivf_probe: probes must be >= 1 (got %d)", probes);
    if (nq == 0) return VSR_OK;
    if (ivf_half(ivf)) {
        int rr = half_query_range(queries, nq, dim);
        if (rr) return rr;
    }
    probes = std::min(probes, ivf->lists);
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ivf->d_q.reserve((size_t) nq * dim * sizeof(float)))) return rc;
    HIPCHK(hipMemcpyAsync(ivf->d_q.p, queries, (size_t) nq * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return ivf_probe_lists(ivf, ivf->d_q.as<float>(), nq, dim, probes, metric, out_lists);
}

extern "C" int vsr_ivf_probe_bit(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int probes, int32_t* out_lists)
{
    if (!ivf || !queries || !out_lists || nq < 0) return fail(VSR_ERR_INVALID, "vsr_ivf_probe_bit: NULL argument");
    int rc = ivf_check_entry(ivf, RowFormat::BIT, "vsr_ivf_probe_bit");
    if (rc) return rc;
    if (dim != ivf->main->dim)                              // CheckDims, bitvec.c:32-39: the column's length first
        return fail(VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u", (unsigned) ivf->main->dim, (unsigned) dim);
    if (probes < 1) return fail(VSR_ERR_INVALID, "vsr_ivf_probe_bit: probes must be >= 1 (got %d)", probes);
    if (nq == 0) return VSR_OK;
    probes = std::min(probes, ivf->lists);
    vsr_ctx* ctx = ivf->main->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t q_bytes = (size_t) nq * format_query_bytes(RowFormat::BIT, dim);
    if ((rc = ivf->d_q.reserve(q_bytes))) return rc;
    HIPCHK(hipMemcpyAsync(ivf->d_q.p, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    return ivf_probe_lists(ivf, ivf->d_q.p, nq, dim, probes, VSR_METRIC_HAMMING, out_lists);
}

// Index build, the part that touches every row (ivfbuild.c:141-227: InsertTuple finds the nearest list of each heap
// row): all corpus rows against the centres, in the index's arithmetic, on the GPU.  The k-means that produces the
// centres from the sampled rows (ivfbuild.c:404-445 ComputeCenters, ivfkmeans.c) is vsr_ivf_kmeans (vsr_kmeans.hip).
// (T = uint16_t, vsr_ivf_assign_half: binary16 centres against the binary16 rows where they lie -- a stored row holds stride4 * 4
// elements in either format -- and no widened copy of the corpus.)
// (T = uint8_t, vsr_ivf_assign_bit, K3b: packed centres against the packed rows where they lie, by the Hamming count -- the key the
// probe gives the same pair; metric is not read.)
template <class T>
static int ivf_assign(vsr_corpus* c, const T* centers, int lists, int metric, int32_t* out_row_list, const char* who)
{
    constexpr RowFormat FMT = ivf_format<T>();
    if (!c || !centers || (c->n > 0 && !out_row_list)) return fail(VSR_ERR_INVALID, "%s: NULL argument", who);
    int rc = ivf_check_corpus(c, FMT, lists, who);
    if (rc) return rc;
    if (FMT != RowFormat::BIT && metric != VSR_METRIC_L2 && metric != VSR_METRIC_IP && metric != VSR_METRIC_COSINE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: metric %d has no ivfflat opclass", who, metric);
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (n == 0) return VSR_OK;
    DevBuf d_centers, d_out;
    if ((rc = d_out.reserve((size_t) n * sizeof(int32_t)))) return rc;
    std::vector<T> ct;                                                        // (outlive the copy: synchronised below)
    std::vector<uint32_t> ctb;
    if constexpr (FMT == RowFormat::BIT) {
        ctb = pack_bit_centers(centers, lists, c->dim);
        if ((rc = d_centers.reserve(ctb.size() * sizeof(uint32_t)))) return rc;
        HIPCHK(hipMemcpyAsync(d_centers.p, ctb.data(), ctb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        // a stored row is stride4 chunks = stride4 * 4 words, zero behind the bits: the first `words` of them are the key's query side
        HIPCHK(launch_ivf_probe(c->d_rows, (uint32_t) c->stride4 * 4, (uint32_t) n, d_centers.p, (int) bit_words(c->dim), lists, 1, 0,
                                d_out.as<int32_t>(), ctx->stream, IVF_BIT));
    } else {
        if ((rc = d_centers.reserve((size_t) lists * c->dim * sizeof(T)))) return rc;
        ct = transpose_centers(centers, lists, c->dim);
        HIPCHK(hipMemcpyAsync(d_centers.p, ct.data(), ct.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        // cosine opclass: rows and centres are compared by the negative inner product (spherical k-means, vector.sql:323-327)
        HIPCHK(launch_ivf_probe(c->d_rows, (uint32_t) c->stride4 * 4, (uint32_t) n, d_centers.p, c->dim, lists, 1,
                                metric == VSR_METRIC_L2 ? M_L2 : M_IP, d_out.as<int32_t>(), ctx->stream, FMT == RowFormat::HALF ? IVF_HALF_ROW : IVF_F32));
    }
    std::vector<int32_t> by_internal((size_t) n);
    HIPCHK(hipMemcpyAsync(by_internal.data(), d_out.p, (size_t) n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < n; ++r) out_row_list[c->h_orig[(size_t) r]] = by_internal[(size_t) r];     // caller's row order
    return VSR_OK;
}

extern "C" int vsr_ivf_assign(vsr_corpus* c, const float* centers, int lists, int metric, int32_t* out_row_list)
{
    return ivf_assign(c, centers, lists, metric, out_row_list, "vsr_ivf_assign");
}

extern "C" int vsr_ivf_assign_half(vsr_corpus* c, const uint16_t* centers, int lists, int metric, int32_t* out_row_list)
{
    return ivf_assign(c, centers, lists, metric, out_row_list, "vsr_ivf_assign_half");
}

extern "C" int vsr_ivf_assign_bit(vsr_corpus* c, const uint8_t* centers, int lists, int32_t* out_row_list)
{
    return ivf_assign(c, centers, lists, VSR_METRIC_HAMMING, out_row_list, "vsr_ivf_assign_bit");
}
