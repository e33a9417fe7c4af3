// vsr_runtime.h — what the host-side translation units of libvsrbac share (internal, not the C ABI): the error plumbing,
// the grow-only buffers, the context / filter / corpus objects and the few functions one unit calls in another
// (README.md lists the units).
#pragma once
#include "../../include/vsrbac.h"
#include "vsr_device.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace vsr {

int fail(int status, const char* fmt, ...);      // sets vsr_last_error of the calling thread, returns status

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return vsr::fail(e_ == hipErrorOutOfMemory ? VSR_ERR_OOM : VSR_ERR_HIP, "%s: %s", #expr, \
                             hipGetErrorString(e_));                                               \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// small RAII buffers (grow-only workspaces): device memory, or pinned host memory mapped into the device
template <bool PINNED> struct Buf {
    void*  p = nullptr;
    void*  dp = nullptr;           // the same memory as the device sees it (kernels read the pinned staging block directly)
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return VSR_OK;
        const bool regrow = p != nullptr;
        release();
        // a quarter of slack the first time; a buffer that had to grow once doubles: hipFree / hipMalloc synchronise the device,
        // and a serving process whose batches differ by a few per cent should stop paying that after its first few calls
        size_t want = std::max(bytes, (size_t) 4096);
        want += regrow ? want : want / 4;
        if (PINNED) {
            HIPCHK(hipHostMalloc(&p, want, hipHostMallocMapped));
            HIPCHK(hipHostGetDevicePointer(&dp, p, 0));
        } else {
            HIPCHK(hipMalloc(&p, want));
            dp = p;
        }
        cap = want;
        return VSR_OK;
    }
    void release()
    {
        if (p) (void) (PINNED ? hipHostFree(p) : hipFree(p));
        p = dp = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
using DevBuf = Buf<false>;
using PinBuf = Buf<true>;

inline std::atomic<uint64_t> g_filter_id{0};
inline std::atomic<uint64_t> g_corpus_serial{0};

}  // namespace vsr

using namespace vsr;               // (internal header: every unit that includes it is part of the library's host side)

struct EventPair {
    hipEvent_t a, b;
    int kind;   // 0 = scan (1 query/pass), 1 = scan (shared pass), 2 = select, 3 = sample scan, 4 = seed select, 5 = whole search
};

struct vsr_ctx {
    int             device = 0;
    hipStream_t     stream = nullptr;
    hipStream_t     own_stream = nullptr;
    hipDeviceProp_t prop;
    // workspaces
    DevBuf d_desc;       // queries (padded) + q norms + scan groups + select queries, one upload
    DevBuf d_partial;
    DevBuf d_cand;       // K1m / K2 candidate buffers
    DevBuf d_flags;      // per-query screening flags of the last call
    DevBuf d_tau;        // seeded thresholds (sample pass)
    DevBuf d_samp;       // K2w: per-query sample buffers
    DevBuf d_qcnt;       // K2w: [candidate counts | sample counts]
    bool   hint_u8 = false;       // vsr_set_query_hint: the caller's DEVICE-resident queries are integers 0..255
    bool   int8_this_call = false;   // search_impl -> make_plan: the queries of this call qualify for the int8 planes
    uint32_t sparse_slots = 2;       // ... (sparse corpus) slots of this call's query tables: sizes the passes (scan_qmax_sparse)
    bool   q8_ok = true;          // ... and every hinted query so far really was (else the hint is dropped)
    PinBuf h_q8;                  // one word the staging kernel sets when a query is not (read without synchronising)
    bool   no_fused = false;      // VSR_NO_FUSED: nq == 1 takes the general path (staging, K1, K5)
    bool   seeding = true;        // seed thresholds of big shared passes from a 1/32 sample pass
    int64_t seed_min_rows = 2000000;
    uint32_t sample_stride = 16;  // K2w sample launch: every 16th tile of a workgroup (VSR_SAMPLE_STRIDE)
    bool   sample_stride_set = false;   // ... given explicitly: the planner's own choice for int8 class-view plans (every 32nd) stands back
    // threshold seeding of the K2 / K1m shared passes (vsr_search.hip): the sample pass visits every seed_stride-th tile with
    // 1/seed_block_div of the workgroups (measured on MI355X: 256 / 1 is the cheapest sample that still seeds tightly)
    uint32_t seed_stride = 256;   // VSR_SEED_STRIDE
    uint32_t seed_block_div = 1;  // VSR_SEED_DIV
    int64_t seed_min_pass_rows = 2048;   // average rows per pass below which the warm-up it removes is too small to pay
    // 64 bytes of device words: [0] running count of flagged queries; byte 16: the kernels' bounds-guard word (checked by
    // vsr_screening_check); byte 32: one all-ones 64-bit word, the "bitmap" of passes without a permission bitmap; byte 48: the
    // session's walk rotation (walk_rot_word)
    int32_t* d_flag_total = nullptr;
    uint32_t* err_word() const { return reinterpret_cast<uint32_t*>(d_flag_total) + 4; }
    const uint64_t* ones_word() const { return reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(d_flag_total) + 32); }
    bool   screening = true;      // allow K2 (MFMA screening + exact re-rank) for shared passes
    int64_t flagged_seen = 0;
    DevBuf d_out;        // host-API outputs
    DevBuf d_misc;
    DevBuf d_dbg;                 // VSR_FUSED_DBG: timestamps of the one-query launch
    PinBuf h_dbg;
    DevBuf d_done;                // nq == 1 fused path: arrival counters of the in-kernel merge tree (zero between calls)
    DevBuf d_redo;                // vsr_search_device_exact: queries and results of the flagged queries
    DevBuf d_short;               // vsr_search_quantized*: bit queries, the stage-1 answer, the re-rank keys
    PinBuf h_desc;
    PinBuf h_out;
    hipEvent_t desc_done = nullptr;   // staging buffer reuse guard
    bool desc_pending = false;
    // measurement
    int profiling = 0;             // 0 off, 1 HIP events around every launch class, 2 around the main scan launch only
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> event_pool;
    vsr_stats stats{};
    // knobs
    int block_budget = 0;          // 0 = 4 * CUs
    bool fused_dbg = false;        // VSR_FUSED_DBG=1
    bool scan_lane = false;        // VSR_SCAN_LANE=1
    hipEvent_t lane_in = nullptr, lane_out = nullptr;
    int fused_fan = 0;             // VSR_FUSED_FAN: lists per first-level merge of the one-query launch (0: the planner's rule)
    int min_rows_per_block = 256;
    int min_shared_rows = 2048;    // rows per workgroup of a shared pass (VSR_MIN_SHARED_ROWS)
    int max_qb = 16;               // queries per shared pass.  32 (two MFMA query groups) does not pay at d = 128; the planner
                                   // picks it by itself for long rows when the query groups fill it (make_plan)
    uint32_t debug = 0;            // VSR_DEBUG != 0: vsr_stats_get prints host-side timings (measurement only)
    double extra_ms[2] = {0, 0};   // sample scan, seed select (profiling only)
    double host_us[3] = {0, 0, 0}; // VSR_DEBUG: host time in make_plan / waiting for the staging buffer / whole search_impl
    long   host_calls = 0;
    std::string last_kernel;       // main scan kernel of the last search (vsr_last_scan_kernel); int8 K2w plans: " + sample <kernel>" appended
    bool no_classes = false;       // VSR_NO_CLASSES=1: scan role partitions whole (A/B measurements)
    bool max_qb_set = false;       // VSR_MAX_QB / vsr_tune chose the queries per pass: the planner does not override it
    bool no_xcd_map = false;       // VSR_NO_XCD_MAP=1: workgroups in pass order instead of XCD-aware bundles (A/B)
    bool no_mq = false;            // VSR_NO_MQ=1: keep shared passes on K1 (A/B measurements)
    bool no_wide = false;          // VSR_NO_WIDE=1: shared passes on K2 (wave-private tiles) instead of K2w (A/B)
    bool no_gemm = false;          // VSR_NO_GEMM=1: wide passes over long rows on K2w instead of K2g (A/B)
    bool no_half_mfma = false;     // VSR_NO_HALF_MFMA=1: shared passes over a halfvec corpus on K1h instead of K2h (A/B)
    bool no_k2i = true;            // VSR_K2I=1: the int8 main launch as K2i's per-wave streams instead of K2w's workgroup tiles (A/B;
                                   // measured on the headline step: K2w 0.342 ms, K2i 0.366 ms -- K2w stays the default)
    bool last_k2i = false;         // the last main launch was eligible for K2i
    uint32_t sample_rounds = 1;    // VSR_SAMPLE_ROUNDS=1..4: resident rounds of workgroups the K2w-family sample launch is cut into (A/B)
    bool sample_reg = true;        // VSR_SAMPLE_REG=0: the int8 sample pass of a class-view plan on K2i's streams instead of K2r's registers (A/B)
    bool select_wave = true;       // VSR_SELECT_WAVE=0: seed and final selection of an int8 (exact_screen) plan on seed_select_kernel /
                                   // select_rerank_kernel instead of the one-wave-per-query kernels (A/B, tests)
    bool k2i_sample = true;        // VSR_NO_K2I_SAMPLE=1: the int8 sample pass on K2w's kernel instead of K2i's streams (A/B)
    bool no_scan8 = false;         // VSR_NO_SCAN8=1: one-query calls on the fp32 rows even when the int8 planes apply (A/B)
    bool k2i_wide = false;         // VSR_K2I_WIDE=1 (with VSR_K2I=1): 128-column passes on K2i
    int  force_epi = -1;           // VSR_FORCE_EPI=0|1: the main launch's survivor handling regardless of the estimate (tests)
    bool no_class_view = false;    // VSR_NO_CLASS_VIEW=1: role pre-filters scan the base-order int8 planes, never the class view (A/B)
    // walk alignment of the DENSE int8 main launches of class-view plans (WalkHint, vsr_device.h)
    bool walk_align = true;        // VSR_WALK_ALIGN=0: no rotation, no position word, passes in first-seen order (A/B: the code before it)
    bool walk_pos_set = false, walk_rot_set = false, walk_spread = false;
    uint32_t walk_pos = 0;         // VSR_WALK_POS=<n>: the seed selection translates n instead of the position word (tests)
    uint64_t walk_rot = 0;         // VSR_WALK_ROT=<n>: rot = (8 n) mod n_launch, bypassing the word (tests);
                                   // VSR_WALK_ROT=spread: the i-th context of the process starts i/3 of the map in (A/B: misaligned on purpose)
    uint32_t ordinal = 0;          // this context is the process's ordinal-th
    uint32_t* walk_rot_word() const { return reinterpret_cast<uint32_t*>(d_flag_total) + 12; }   // byte 48 of d_flag_total's block
    int  screen_level = 2;         // search_impl -> make_plan: 2 = every screening tier, 1 = no coarse tier (K2g), 0 = exact only
    bool last_coarse = false;      // the last search screened on the coarse planes: its flagged queries go to the fine tier first

    ~vsr_ctx()                     // also runs on vsr_open's error returns: nothing allocated so far is leaked
    {
        for (auto& ep : pending) {
            (void) hipEventDestroy(ep.a);
            (void) hipEventDestroy(ep.b);
        }
        for (auto ev : event_pool) (void) hipEventDestroy(ev);
        // (every DevBuf / PinBuf member releases itself: ~Buf)
        if (desc_done) (void) hipEventDestroy(desc_done);
        if (d_flag_total) (void) hipFree(d_flag_total);
        if (lane_in) (void) hipEventDestroy(lane_in);
        if (lane_out) (void) hipEventDestroy(lane_out);
        if (own_stream) (void) hipStreamDestroy(own_stream);
    }
};


struct vsr_filter {
    // never reused, unlike the address: what the index-side caches (vsr_ivf::parts / view_bitmaps, vsr_hnsw::bitmaps) are
    // keyed by, so that a filter allocated where a freed one used to live can never inherit that filter's permissions
    const uint64_t id = g_filter_id.fetch_add(1, std::memory_order_relaxed) + 1;
    vsr_corpus* corpus = nullptr;
    int         mode = VSR_FILTER_RANGES;
    bool        cached = false;
    uint2*      d_tiles = nullptr;     // RANGES
    uint32_t    n_tiles = 0;
    uint64_t*   d_bitmap = nullptr;    // BITMAP (or impure partition: tiles + bitmap)
    bool        owns_bitmap = false;
    int64_t     allowed_rows = 0;
    int64_t     scanned_rows = 0;
    // pre-filter of a role set = union of disjoint permission classes (documents with the same role signature);
    // the planner scans class by class so that queries of different roles share the classes they have in common
    std::vector<vsr_filter*> parts;
    bool parts_only = false;               // the filter has no tile list of its own: always scanned part by part (IVF probes)
    int32_t view_class = -1;               // RANGES filter whose rows are exactly one permission class (a corpus's class filter, or
                                           // a role filter that sees a single class): that class, for the class view (ClassView)
    // planner scratch (one planner per context at a time): group id of this filter in the plan being built
    mutable uint64_t plan_epoch = 0;
    mutable uint32_t plan_group = 0;
};

// Class view: a second, derived copy of the int8 planes in permission-class order (vsr_filter.hip: build_class_view).
// Class after class, rows inside a class in base order, every class starting at a multiple of 64 rows; pad rows are zero
// planes with |row|^2 = NaN and no tile ever counts them.  A call whose passes are all whole classes scans a class as ONE
// contiguous run of full 16-row tiles instead of one short range per document (make_plan, search_wide); candidate keys
// carry base rows through `rank`, as the IVFFlat views' do.  Built by vsr_rbac_load, dropped with the classes.
struct ClassView {
    uint4*    d_scr8 = nullptr;          // [n_rows + 32][8] int8 planes (whole tiles may be read past the last row)
    float*    d_norm2_8 = nullptr;       // [n_rows + 64]
    uint32_t* d_rank = nullptr;          // [n_rows] view row -> base row (pads: 0, never emitted)
    uint2*    d_tiles = nullptr;         // [n_rows / 16] (16 t, rows of the class that tile t holds: 16, fewer at a class's end, 0)
    uint32_t* d_walk_pos = nullptr;      // one word, zero at creation: first view row >> 6 of the DENSE main workgroup that started
                                         // last, whichever session launched it (walk alignment: WalkHint, vsr_device.h)
    uint32_t  n_rows = 0;                // with the pads: a multiple of 64
    std::vector<uint32_t> start, rows;   // per class: first view row, row count
    size_t bytes() const { return ((size_t) n_rows + 32) * 128 + ((size_t) n_rows + 64) * 4 + (size_t) n_rows * 4 + (size_t) n_rows / 16 * 8; }
    ~ClassView()
    {
        void* ptrs[] = {d_scr8, d_norm2_8, d_rank, d_tiles, d_walk_pos};
        for (void* p : ptrs)
            if (p) (void) hipFree(p);
    }
};

struct vsr_corpus {
    vsr_ctx*    ctx = nullptr;
    // identity of this corpus among all the process ever created: never reused, unlike the address.  A quantized corpus
    // records its source's, which is how vsr_search_quantized* knows that the two hold the same rows in the same order
    const uint64_t serial = g_corpus_serial.fetch_add(1, std::memory_order_relaxed) + 1;
    uint64_t    quantized_from = 0;      // vsr_corpus_binary_quantize: the source's serial; 0: not a quantized corpus
    // the corpus's scan lane (VSR_SCAN_LANE=1): the main scan launches of ALL sessions over this corpus queue up on this one
    // stream, so two of them never share the GPU (their short kernels still run beside the other sessions' scans)
    mutable hipStream_t scan_stream = nullptr;
    int64_t     n = 0;
    int         dim = 0;
    uint32_t    stride4 = 0;             // float4 per padded row (halfvec corpus: per padded QUERY, dim rounded up to 8 floats)
    // What d_rows holds (RowFormat, vsr_device.h; format_row_chunks 16-byte chunks per row):
    // HALF (vsr_corpus_load_half): chunks of 8 binary16 values, no fp32 image, no screening planes; K1h, or K2h on the rows themselves
    // BIT (vsr_corpus_load_bit, vsr_corpus_binary_quantize): dim counts BITS, chunks of packed bits (pad bits zero), d_norm2 the
    //   rows' popcounts; no norms-max, no planes, no class view; exact kernel only (K1b)
    // SPARSE (vsr_corpus_load_sparse): sp_entries interleaved (index, value) entries of 8 bytes, d_sp_off the rows' first entries
    //   (n + 1 of them, all even), d_norm2 the rows' |row|^2; stride4 = 0, shape = {LPR by the mean entry count, 0, LPR, 64}; no
    //   planes, no class view; exact kernel only (K1s)
    RowFormat   format = RowFormat::F32;
    uint64_t*   d_sp_off = nullptr;
    uint64_t    sp_entries = 0;          // stored entries, pad entries included
    uint32_t    sp_max_nnz = 0;          // non-zeros of the longest row (the HNSW entry points take at most HNSW_MAX_NNZ = 1000)
    int64_t     row_offset = 0;
    KernelShape shape{};
    float4*     d_rows = nullptr;
    float*      d_norm2 = nullptr;
    uint4*      d_scr = nullptr;         // K2w screening planes (bf16 hi / mid split of the rows), nullptr: not built
    // list-ordered VIEW of another corpus (IVFFlat, vsr_ivf_load): rows / norms / planes / tile lists are the view's own,
    // in list order; identity arrays, RBAC tables and the fp32 rows the exact re-rank gathers stay in `base`, and keys carry
    // base rows through d_rank (physical row -> base row)
    vsr_corpus* base = nullptr;
    uint32_t*   d_rank = nullptr;
    uint2*      d_all_tiles = nullptr;   // identity tile list (K2w always walks an explicit list: unfiltered passes use this)
    uint32_t    pstride4 = 0;            // 16-byte chunks per plane row
    bool        scr_has_mid = true;      // false: every element is exactly a bf16 value (e.g. SIFT's 0..255 integers)
    uint4*      d_scr_c = nullptr;       // K2g coarse planes (hi = bf16(x) only, rows padded to whole 64-element K-steps): long rows
    uint32_t    cstride4 = 0;            // 16-byte chunks per coarse plane row
    uint4*      d_scr8 = nullptr;        // int8 planes (x - 128, 128 bytes per row): corpus of integers 0..255, d <= 128; L2 only
    float*      d_norm2_8 = nullptr;     // sum (x - 128)^2 per row
    float*      d_norm2_max = nullptr;   // max |row|^2 (error bound of K2 screening); +Inf if any |row|^2 is not finite
    bool        k2_safe = true;          // false: some |row|^2 is Inf / NaN (non-finite or huge elements) -> exact kernels only
    int64_t*    d_block = nullptr;
    int32_t*    d_doc = nullptr;
    int64_t*    d_orig = nullptr;
    uint32_t*   d_row_docidx = nullptr;
    // host-side identity (internal order)
    std::vector<int64_t> h_orig;
    std::vector<int32_t> docs;            // sorted unique document ids
    std::vector<uint32_t> doc_row_start;  // docs.size() + 1
    // RBAC
    bool rbac = false;
    std::vector<int32_t> roles;           // sorted unique role ids
    uint32_t words = 0;
    std::vector<uint64_t> doc_mask;       // docs.size() * words
    uint64_t* d_doc_mask = nullptr;
    std::unordered_map<int32_t, std::vector<int32_t>> user_roles;
    std::map<std::pair<int, std::vector<int32_t>>, vsr_filter*> cache;
    // permission classes: documents grouped by identical role signature (doc_mask row)
    std::vector<uint32_t> doc_class;                 // per document
    std::vector<std::vector<uint64_t>> class_sig;    // per class
    std::vector<vsr_filter*> class_filters;          // per class, built on first use (RANGES, owned by the corpus)
    std::vector<vsr_filter*> class_bitmap_filters;   // per class, BITMAP mode: aligned windows + the class's own bitmap
    uint32_t* d_doc_class = nullptr;                 // class of every document (device copy of doc_class)
    std::unique_ptr<ClassView> class_view;           // the int8 planes in class order; none: no int8 planes, too many classes,
                                                     // VSR_NO_CLASS_VIEW, or no memory for it
    // indexes loaded over this corpus: a filter that dies (vsr_filter_free, vsr_rbac_load) is purged from their caches
    std::vector<struct vsr_ivf*>  ivf_indexes;
    std::vector<struct vsr_hnsw*> hnsw_indexes;

    ~vsr_corpus();                 // frees the device arrays and cached filters (also on vsr_corpus_load's error returns)
};

namespace vsr {

inline int64_t allowed_rows(const vsr_corpus* c, const vsr_filter* f) { return f ? f->allowed_rows : c->n; }
// the filter's count of permitted rows is exact knowledge about the rows its tiles cover (no bitmap thins them out)
inline bool exact_count(const vsr_filter* f) { return !f || f->allowed_rows == f->scanned_rows; }

// The result arrays of a search, [nq][k] each (cnt: [nq]), in device or host memory.  row / keys may be nullptr (doc too
// where an entry point allows it): that column is then not written.
struct Outputs {
    int64_t* blk; int32_t* doc; int64_t* row; float* dist; int32_t* cnt; uint64_t* keys;
    Outputs from_query(size_t q0, int k) const     // the same arrays from query q0 on
    {
        const size_t ok = q0 * (size_t) k;
        return {blk + ok, doc ? doc + ok : nullptr, row ? row + ok : nullptr, dist + ok, cnt + q0, keys ? keys + ok : nullptr};
    }
};

// identity arrays of the corpus and the caller's result arrays, into any parameter block that carries them
// (FusedTail, SelectParams, RerankParams, HnswParams)
template <class P> inline void set_results(P& p, const vsr_corpus* idc, const Outputs& o)
{
    p.block_ids = idc->d_block;
    p.doc_ids = idc->d_doc;
    p.orig_rows = idc->d_orig;
    p.out_block = o.blk;
    p.out_doc = o.doc;
    p.out_row = o.row;
    p.out_dist = o.dist;
    p.out_count = o.cnt;
}
// ... and, for the brute-force search's blocks, the raw keys and the shard offset they carry
template <class P> inline void set_keyed_results(P& p, const vsr_corpus* idc, const Outputs& o)
{
    set_results(p, idc, o);
    p.out_keys = o.keys;
    p.row_offset = (uint32_t) idc->row_offset;
}

// One block that carries the results of nq queries between device and host: [blk | row | doc | dist | cnt | extra | status],
// every section 256-byte aligned.  `extra` is an optional 8-byte column per query (HNSW: visited elements / scanned
// tuples); `status` is a 4-byte column per query (screening flags, K4 overflow status) behind the results proper.
struct ResultBlock {
    int    nq, k;
    size_t o_blk, o_row, o_doc, o_dist, o_cnt, o_extra, o_status;
    size_t total;                                    // with the status column; results alone: o_status
    ResultBlock(int nq_, int k_, bool extra) : nq(nq_), k(k_)
    {
        const size_t nk = (size_t) nq * k;
        o_blk = 0;
        o_row = align_up(o_blk + nk * 8, 256);
        o_doc = align_up(o_row + nk * 8, 256);
        o_dist = align_up(o_doc + nk * 4, 256);
        o_cnt = align_up(o_dist + nk * 4, 256);
        o_extra = align_up(o_cnt + (size_t) nq * 4, 256);
        o_status = extra ? align_up(o_extra + (size_t) nq * 8, 256) : o_extra;
        total = align_up(o_status + (size_t) nq * 4, 256);
    }
    Outputs arrays(char* b) const
    {
        return {reinterpret_cast<int64_t*>(b + o_blk), reinterpret_cast<int32_t*>(b + o_doc), reinterpret_cast<int64_t*>(b + o_row),
                reinterpret_cast<float*>(b + o_dist), reinterpret_cast<int32_t*>(b + o_cnt), nullptr};
    }
    template <class T> T* column(char* b, size_t off) const { return reinterpret_cast<T*>(b + off); }
    // results of queries [j, j + n) of the block `h` (host memory) into queries [dst, dst + n) of the caller's arrays
    void copy_out(char* h, size_t j, size_t n, size_t dst, const Outputs& out, int64_t* out_extra) const
    {
        const Outputs in = arrays(h).from_query(j, k), to = out.from_query(dst, k);
        const size_t nk = n * (size_t) k;
        memcpy(to.blk, in.blk, nk * 8);
        if (to.row) memcpy(to.row, in.row, nk * 8);
        if (to.doc) memcpy(to.doc, in.doc, nk * 4);
        memcpy(to.dist, in.dist, nk * 4);
        memcpy(to.cnt, in.cnt, n * 4);
        if (out_extra) memcpy(out_extra + dst, column<int64_t>(h, o_extra) + j, n * 8);
    }
    void copy_out_all(char* h, const Outputs& out, int64_t* out_extra) const { copy_out(h, 0, (size_t) nq, 0, out, out_extra); }
    void patch_one(char* h, size_t j, size_t dst, const Outputs& out, int64_t* out_extra) const { copy_out(h, j, 1, dst, out, out_extra); }
    // the queries of the first n whose status word is set
    std::vector<int> flagged(char* h, size_t n) const
    {
        std::vector<int> redo;
        for (size_t i = 0; i < n; ++i)
            if (column<int32_t>(h, o_status)[i]) redo.push_back((int) i);
        return redo;
    }
};

// the queries (rows of dim floats, host memory) and filters of the queries listed in `redo`, packed for a re-run
inline void gather_subset(const float* queries, int dim, const vsr_filter* const* filters, const std::vector<int>& redo,
                          std::vector<float>& q2, std::vector<const vsr_filter*>& f2)
{
    q2.resize(redo.size() * (size_t) dim);
    f2.assign(redo.size(), nullptr);
    for (size_t j = 0; j < redo.size(); ++j) {
        memcpy(&q2[j * (size_t) dim], queries + (size_t) redo[j] * dim, (size_t) dim * sizeof(float));
        if (filters) f2[j] = filters[redo[j]];
    }
}

// ---- functions one unit calls in another ----
// vsr_filter.hip
void   drop_cached_filters(vsr_corpus* c);
void   free_filter(vsr_filter* f);
using FilterPtr = std::unique_ptr<vsr_filter, void (*)(vsr_filter*)>;
FilterPtr new_filter(vsr_corpus* c, int mode, bool cached);        // (cached: owned by the corpus or an index, not by the caller)
int    upload_tiles(vsr_filter* f, const std::vector<uint2>& tiles);
void   ranges_to_tiles(const std::vector<std::pair<uint32_t, uint32_t>>& ranges, int rw, std::vector<uint2>& tiles);
inline size_t bitmap_words(int64_t n) { return (size_t) ((n + 63) / 64) + 2; }   // + pad for the 2-word window
// vsr_ivf.hip, vsr_hnsw_rt.hip: a filter of the corpus is about to die (vsr_filter_free) or all of them are (f == nullptr:
// vsr_rbac_load, corpus teardown): the indexes forget what they derived from it.  The caller has synchronised the stream.
void   purge_ivf_caches(vsr_corpus* c, const vsr_filter* f);
void   purge_hnsw_caches(vsr_corpus* c, const vsr_filter* f);
// vsr_hnsw_rt.hip: host queries bound for halfvec rows: a finite element that rounds to +-Inf in binary16 is refused (`$1::halfvec`)
int    half_query_range(const void* queries, int nq, int dim);
// vsr_search.hip
// entry: the queries the calling entry point takes -- F32 (fp32 vectors: a vector or a halfvec corpus, metrics 0 .. 3), BIT (a
// vsr_search_bit* / vsr_hnsw_search_bit* entry point: bit corpus, metrics 4 / 5) or SPARSE (vsr_search_sparse*: sparse corpus,
// metrics 0 .. 3).  A bit or a sparse corpus is refused to every other entry point
int    check_search_args(const vsr_corpus* c, const void* queries, int nq, int dim, int k, int metric,
                         const vsr_filter* const* filters, const char* who, RowFormat entry = RowFormat::F32);
// vsr_runtime.hip: n sparsevec values as CSR, checked as sparsevec_recv checks one (sparsevec.c:53-133, 493-539); max_nnz (may be
// nullptr) receives the longest row's entry count
int    check_sparse_rows(const char* who, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n, int dim,
                         uint32_t* max_nnz);
// queries: format_query_bytes(c->format, dim) bytes each
int    host_search(vsr_corpus* c, const void* queries, int nq, int dim, int k, int metric, const vsr_filter* const* filters,
                   const Outputs& out);
// the same with queries and results on the device, enqueued and not waited for; a bit corpus or a view of one: nothing flags
int    device_search(vsr_corpus* c, const void* d_queries, int nq, int dim, int k, int metric, const vsr_filter* const* filters,
                     const Outputs& out);
// the two-stage searches (vsr_search_quantized*, and vsr_hnsw_search_quantized* in vsr_hnsw_rt.hip): the argument checks they share
// (session may be nullptr) and stage 2, the exact re-rank of stage-1 keys on the source rows
int    check_quantized_args(const vsr_ctx* session, const vsr_corpus* src, const vsr_corpus* bits, const void* queries, int nq,
                            int dim, int k, int shortlist, int metric, const vsr_filter* const* filters, const char* who);
int    quantized_rerank(vsr_ctx* ctx, vsr_corpus* src, const uint64_t* s1_keys, uint32_t s1_row_offset, uint64_t* rr_keys,
                        const float* d_queries, int nq, int dim, int k, int shortlist, int metric, const Outputs& out);

}  // namespace vsr
