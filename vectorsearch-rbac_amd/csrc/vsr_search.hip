// vsr_search.hip — the brute-force search: the three launch sequences a plan resolves to (K2w / K2g wide passes, the
// one-query fused launch, the general K1 / K1m / K2 path), the vsr_search* entry points and their flag re-run ladders, and the
// two-stage search (vsr_search_quantized*: K1b shortlist, then the exact re-rank of vsr_shortlist.h).
#include "vsr_plan.h"
#include "vsr_shortlist.h"

#include <chrono>
#include <cmath>
#include <cstdio>

namespace {

using Clock = std::chrono::steady_clock;
double us_since(Clock::time_point t0) { return std::chrono::duration<double, std::micro>(Clock::now() - t0).count(); }

// ---- timed launches ----------------------------------------------------------------------------------------------
// HIP events around one class of launches (vsr_profiling; EventPair::kind).  Records the first event on the stream where it
// is created, stop() records the second and queues the pair for drain_events.  The main scan launch (kinds 0, 1) is timed
// at any profiling level, everything else (2 .. 5) at level 1 only; unarmed, neither does anything.
struct Timed {
    vsr_ctx*    ctx;
    hipStream_t stream;
    int         kind;
    hipEvent_t  a = nullptr, b = nullptr;
    hipError_t  err = hipSuccess;
    static hipEvent_t take_event(vsr_ctx* ctx)
    {
        if (!ctx->event_pool.empty()) {
            hipEvent_t e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void) hipEventCreate(&e);
        return e;
    }
    Timed(vsr_ctx* ctx_, int kind_, hipStream_t stream_) : ctx(ctx_), stream(stream_), kind(kind_)
    {
        if (kind < 2 ? ctx->profiling == 0 : ctx->profiling != 1) return;
        a = take_event(ctx);
        b = take_event(ctx);
        err = hipEventRecord(a, stream);
    }
    hipError_t stop()                                       // (reports a failed record of either event)
    {
        if (a && err == hipSuccess) err = hipEventRecord(b, stream);
        if (a && err == hipSuccess) ctx->pending.push_back({a, b, kind});
        return err;
    }
};
#define RCCHK(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// the queries of a sparse search
struct SparseQueries {                                      // nq queries as CSR
    const int64_t* indptr; const int32_t* indices; const float* values;
    bool     host;                                          // the arrays are host memory (validated; copied through the pinned block)
    uint32_t max_nnz;                                       // the longest query: sizes the tables
};

// ---- staging block -----------------------------------------------------------------------------------------------
// The per-batch block in device memory, sections appended in order, each 256-byte aligned: [what the staging kernel
// computes: padded queries, |q|^2, query planes || what the host writes (and the pinned block holds): the plan's descriptors]
struct Staging {
    struct Section { size_t off, bytes; const void* src; };
    Section sec[16];
    int     n = 0;
    size_t  total = 0;
    size_t add(size_t bytes, const void* src = nullptr)     // src: host data copied by fill() (nullptr: device-only section)
    {
        const size_t off = total;
        sec[n++] = {off, bytes, src};
        total = align_up(off + bytes, 256);
        return off;
    }
    template <class T> size_t add(const std::vector<T>& v) { return add(v.size() * sizeof(T), v.data()); }
    void fill(char* host_image, size_t first_off) const     // host_image: the pinned copy of [first_off, total)
    {
        for (int i = 0; i < n; ++i)
            if (sec[i].src) memcpy(host_image + (sec[i].off - first_off), sec[i].src, sec[i].bytes);
    }
};

// the previous batch's staging kernel may still own the pinned block
int wait_for_staging_block(vsr_ctx* ctx)
{
    if (!ctx->desc_pending) return VSR_OK;
    const auto w0 = Clock::now();
    HIPCHK(hipEventSynchronize(ctx->desc_done));
    ctx->desc_pending = false;
    const double waited = us_since(w0);
    ctx->host_us[1] += waited;
    ctx->stats.host_wait_ms += waited * 1e-3;
    return VSR_OK;
}

// Writes the host's part of the staging block (sections from off_g on, and the queries of a host call, padded to the row
// stride) into the pinned block and fills the staging kernel's common arguments.  ONE staging kernel instead of an SDMA
// copy + gather + norm + two fills: it pulls the descriptor block out of the pinned host buffer, pads the queries to the row
// stride (from the caller's device buffer, or from the staged host copy), computes |q|^2 with the arithmetic of the row
// norms, clears the per-query flags and seeds.  The queries' section is the block's first, |q|^2 lies at off_qn.
// (fmt, the corpus's: BIT queries are packed bit strings, `dim` bits = ceil(dim / 8) bytes per query, padded to qfloats * 4 bytes)
int stage_host_part(vsr_ctx* ctx, const Staging& sb, size_t off_qn, size_t off_g, RowFormat fmt, const void* h_queries, const void* d_queries,
                    int nq, int dim, size_t qfloats, StageParams& st)
{
    const size_t h_q_bytes = h_queries ? align_up((size_t) nq * qfloats * sizeof(float), 256) : 0;
    const size_t src_bytes = format_query_bytes(fmt, dim);
    RCCHK(wait_for_staging_block(ctx));
    RCCHK(ctx->h_desc.reserve(h_q_bytes + (sb.total - off_g)));
    RCCHK(ctx->d_desc.reserve(sb.total));
    RCCHK(ctx->d_flags.reserve((size_t) nq * sizeof(int32_t)));
    RCCHK(ctx->d_tau.reserve((size_t) nq * sizeof(uint64_t)));
    char* hs = ctx->h_desc.as<char>();
    char* ds = ctx->d_desc.as<char>();
    if (h_queries) {
        const size_t slot_bytes = qfloats * sizeof(float);
        for (int s = 0; s < nq; ++s) {
            char* dst = hs + (size_t) s * slot_bytes;
            memcpy(dst, static_cast<const char*>(h_queries) + (size_t) s * src_bytes, src_bytes);
            memset(dst + src_bytes, 0, slot_bytes - src_bytes);
        }
    }
    sb.fill(hs + h_q_bytes, off_g);
    const char* hd = reinterpret_cast<const char*>(ctx->h_desc.dp);
    st.src16 = reinterpret_cast<const uint4*>(hd + h_q_bytes);
    st.dst16 = reinterpret_cast<uint4*>(ds + off_g);
    st.n16 = (uint32_t) ((sb.total - off_g) / 16);
    st.q_src = d_queries ? static_cast<const float*>(d_queries) : reinterpret_cast<const float*>(hd);
    st.q_stride = d_queries ? (uint32_t) dim : (uint32_t) qfloats;
    if (fmt == RowFormat::BIT) {                                           // byte strides; stage_bit_kernel clears the pad bits and counts the ones
        st.q_stride = d_queries ? (uint32_t) src_bytes : (uint32_t) (qfloats * sizeof(float));
        st.q_bits = 1u;
    }
    st.q_dst = reinterpret_cast<float*>(ds);
    st.dim = (uint32_t) dim;
    st.qfloats = (uint32_t) qfloats;
    st.nq = (uint32_t) nq;
    st.q_norm2 = reinterpret_cast<float*>(ds + off_qn);
    st.flags = ctx->d_flags.as<int32_t>();
    st.tau = ctx->d_tau.as<uint64_t>();
    return VSR_OK;
}

// ... of a sparse search: the host's part as above; a host call's CSR arrays travel in front of it in the pinned block.  The
// staging block's first section is the queries' tables, `off_qt` their double totals, `off_qn` their fp32 |q|^2.
int stage_sparse(vsr_ctx* ctx, const Staging& sb, size_t off_qt, size_t off_qn, size_t off_g, const SparseQueries& sq, int nq, int dim,
                 uint32_t slots)
{
    const size_t nnz = sq.host ? (size_t) (sq.indptr[nq] - sq.indptr[0]) : 0;
    const size_t h_ptr = 0, h_idx = align_up(h_ptr + ((size_t) nq + 1) * 8, 256), h_val = align_up(h_idx + nnz * 4, 256),
                 h_q_bytes = sq.host ? align_up(h_val + nnz * 4, 256) : 0;
    RCCHK(wait_for_staging_block(ctx));
    RCCHK(ctx->h_desc.reserve(h_q_bytes + (sb.total - off_g)));
    RCCHK(ctx->d_desc.reserve(sb.total));
    RCCHK(ctx->d_flags.reserve((size_t) nq * sizeof(int32_t)));
    RCCHK(ctx->d_tau.reserve((size_t) nq * sizeof(uint64_t)));
    char* hs = ctx->h_desc.as<char>();
    char* ds = ctx->d_desc.as<char>();
    const char* hd = reinterpret_cast<const char*>(ctx->h_desc.dp);
    SparseStageParams st{};
    if (sq.host) {
        int64_t* ptr = reinterpret_cast<int64_t*>(hs + h_ptr);
        for (int i = 0; i <= nq; ++i) ptr[i] = sq.indptr[i] - sq.indptr[0];
        if (nnz) {
            memcpy(hs + h_idx, sq.indices + sq.indptr[0], nnz * 4);
            memcpy(hs + h_val, sq.values + sq.indptr[0], nnz * 4);
        }
        st.indptr = reinterpret_cast<const int64_t*>(hd + h_ptr);
        st.indices = reinterpret_cast<const int32_t*>(hd + h_idx);
        st.values = reinterpret_cast<const float*>(hd + h_val);
    } else {
        st.indptr = sq.indptr;
        st.indices = sq.indices;
        st.values = sq.values;
    }
    sb.fill(hs + h_q_bytes, off_g);
    st.src16 = reinterpret_cast<const uint4*>(hd + h_q_bytes);
    st.dst16 = reinterpret_cast<uint4*>(ds + off_g);
    st.n16 = (uint32_t) ((sb.total - off_g) / 16);
    st.nq = (uint32_t) nq;
    st.dim = (uint32_t) dim;
    st.max_nnz = sq.max_nnz;
    st.slots = slots;
    st.shift = 32u - (uint32_t) __builtin_ctz(slots);
    st.tab = reinterpret_cast<uint2*>(ds);
    st.qtot = reinterpret_cast<double*>(ds + off_qt);
    st.q_norm2 = reinterpret_cast<float*>(ds + off_qn);
    st.flags = ctx->d_flags.as<int32_t>();
    st.tau = ctx->d_tau.as<uint64_t>();
    st.err = ctx->err_word();
    HIPCHK(launch_stage_sparse(st, ctx->stream));
    HIPCHK(hipEventRecord(ctx->desc_done, ctx->stream));
    ctx->desc_pending = true;
    return VSR_OK;
}

int launch_staging(vsr_ctx* ctx, const StageParams& st)
{
    HIPCHK(st.q_bits ? launch_stage_bit(st, ctx->stream) : launch_stage(st, ctx->stream));
    HIPCHK(hipEventRecord(ctx->desc_done, ctx->stream));
    ctx->desc_pending = true;
    return VSR_OK;
}

// the pinned word the kernels set when a query breaks the caller's u8 promise (allocated on first use)
int ensure_q8_word(vsr_ctx* ctx)
{
    if (ctx->h_q8.p) return VSR_OK;
    RCCHK(ctx->h_q8.reserve(64));
    memset(ctx->h_q8.p, 0, 64);
    return VSR_OK;
}

// ---- parameter blocks --------------------------------------------------------------------------------------------
// what every scan launch over corpus `c` has in common
ScanParams scan_params(const vsr_ctx* ctx, const vsr_corpus* c, uint32_t kp, uint32_t qmax)
{
    ScanParams sp{};
    sp.rows = c->d_rows;
    sp.norm2 = c->d_norm2;
    sp.n_rows = (uint32_t) c->n;
    sp.stride4 = c->stride4;
    sp.kp = sp.k = kp;
    sp.qmax = qmax;
    sp.rw = (uint32_t) c->shape.rw;
    sp.err = ctx->err_word();
    sp.ones = ctx->ones_word();
    sp.rank = c->d_rank;
    sp.sample_stride = 1;
    return sp;
}

// ... and every exact re-rank (K5r) of screening survivors; `ds` is the staging block, whose first section is the queries
RerankParams rerank_params(const vsr_ctx* ctx, const vsr_corpus* c, const char* ds, size_t off_sq, uint32_t kp, int k, int metric,
                           const Outputs& out)
{
    const vsr_corpus* idc = c->base ? c->base : c;          // identity arrays and re-rank rows (c may be a list-ordered view)
    RerankParams rr{};
    rr.queries = reinterpret_cast<const SelectQuery*>(ds + off_sq);
    rr.rows = idc->d_rows;
    rr.rows_half = c->format == RowFormat::HALF ? 1u : 0u;
    rr.stride4 = c->stride4;
    rr.queries_f = reinterpret_cast<const float*>(ds);
    rr.kp = kp;
    rr.k = (uint32_t) k;
    rr.metric = metric;
    rr.dim = c->dim;
    rr.norm2_max = idc->d_norm2_max;
    set_keyed_results(rr, idc, out);
    rr.out_flags = ctx->d_flags.as<int32_t>();
    rr.flagged_total = ctx->d_flag_total;
    return rr;
}

void count_scan(vsr_ctx* ctx, const Plan& plan, int cls)    // cls: 0 = one query per pass, 1 = shared passes
{
    ctx->stats.scan_bytes[cls] += plan.scan_bytes;
    ctx->stats.scan_rows[cls] += plan.scan_rows;
    ctx->stats.scan_pairs[cls] += plan.scan_pairs;
    ctx->stats.unique_rows[cls] += plan.unique_rows;
}

// one search call as the launch sequences see it.  d_queries == nullptr: queries come from `h_queries`.  The corpus's format says
// what the query pointers address: fp32 vectors, or (BIT) packed bit strings, format_query_bytes each; SPARSE: `sparse` is set
// and the query pointers are not used
struct Call { const void *h_queries, *d_queries; int nq, dim, k, metric; Outputs out; const SparseQueries* sparse = nullptr; };

// ---- K2w / K2g ---------------------------------------------------------------------------------------------------
// K2w launch sequence (plan.k2w): staging -> sample pass -> threshold seeds -> main pass -> select + exact re-rank.
// Five launches, one candidate buffer per query, no partial lists (see vsr_mfmaw.h).
int search_wide(vsr_ctx* ctx, vsr_corpus* c, const Plan& plan, const Call& q)
{
    const uint32_t kp = plan.keep;
    const int nq = q.nq, metric = q.metric;
    const size_t qfloats = (size_t) c->stride4 * 4;
    const size_t q_pstride = c->scr_has_mid ? c->pstride4 : 2 * (size_t) c->pstride4;    // query planes keep hi and mid
    Staging sb;
    sb.add((size_t) nq * qfloats * sizeof(float));                                        // queries
    const size_t off_qn = sb.add((size_t) nq * sizeof(float));
    const size_t off_qp = sb.add((size_t) nq * q_pstride * 16);
    const size_t off_qc = sb.add(plan.k2g ? coarse_plane_u4((uint64_t) nq, c->cstride4) * 16 : 0);   // K2g: coarse query planes
    const size_t off_q8 = sb.add(plan.int8 ? (size_t) nq * 128 : 0);                      // int8 query planes, |q-128|^2, validity
    const size_t off_qn8 = sb.add(plan.int8 ? (size_t) nq * sizeof(float) : 0);
    const size_t off_qb = sb.add(plan.int8 ? (size_t) nq * sizeof(uint32_t) : 0);
    const size_t off_g = sb.add(plan.groups);                                              // copied from here on
    const size_t off_gs = sb.add(plan.groups_s);
    const size_t off_qs = sb.add(plan.q_slots);
    const size_t off_sq = sb.add(plan.selq);
    const size_t off_bm = sb.add(plan.block_map);
    const size_t off_wt = sb.add(plan.walk_table);

    StageParams st{};
    RCCHK(stage_host_part(ctx, sb, off_qn, off_g, c->format, q.h_queries, q.d_queries, nq, q.dim, qfloats, st));
    RCCHK(ctx->d_cand.reserve((size_t) nq * GQ_CAP * sizeof(uint64_t)));
    RCCHK(ctx->d_samp.reserve((size_t) nq * GQ_SAMPLE_CAP * sizeof(uint64_t)));
    RCCHK(ctx->d_qcnt.reserve((size_t) 2 * nq * sizeof(uint32_t)));
    char* ds = ctx->d_desc.as<char>();

    Timed whole(ctx, 5, ctx->stream);                       // the whole search on the device
    uint32_t* qcnt = ctx->d_qcnt.as<uint32_t>();
    uint32_t* scnt = qcnt + nq;
    st.q_scr = reinterpret_cast<uint4*>(ds + off_qp);
    st.pstride4 = c->pstride4;
    st.plane_ho = c->scr_has_mid ? 0u : 1u;
    st.qcnt = qcnt;
    st.scnt = scnt;
    if (plan.k2g) {
        st.q_scr = nullptr;                                 // only the coarse planes are read
        st.q_scr_c = reinterpret_cast<uint4*>(ds + off_qc);
        st.cstride4 = c->cstride4;
    }
    if (plan.int8) {
        RCCHK(ensure_q8_word(ctx));
        st.q_scr8 = reinterpret_cast<uint4*>(ds + off_q8);
        st.q_norm2_8 = reinterpret_cast<float*>(ds + off_qn8);
        st.q8_bad = reinterpret_cast<uint32_t*>(ds + off_qb);
        st.q8_bad_host = reinterpret_cast<uint32_t*>(ctx->h_q8.dp);
    }
    RCCHK(launch_staging(ctx, st));

    ScanParams sp = scan_params(ctx, c, kp, plan.qmax);
    sp.queries = reinterpret_cast<const float*>(ds);
    sp.q_norm2 = reinterpret_cast<const float*>(ds + off_qn);
    sp.scr = c->d_scr;
    sp.q_scr = reinterpret_cast<const uint4*>(ds + off_qp);
    sp.pstride4 = c->pstride4;
    sp.plane_ho = c->scr_has_mid ? 0u : 1u;
    if (plan.int8) {                                        // same kernel, int8 planes: 8 chunks per row, their own norms
        sp.norm2 = c->d_norm2_8;
        sp.q_norm2 = reinterpret_cast<const float*>(ds + off_qn8);
        sp.scr = c->d_scr8;
        sp.q_scr = reinterpret_cast<const uint4*>(ds + off_q8);
        sp.pstride4 = 8;
        sp.plane_ho = 2u;
        if (plan.class_view) {                              // the same planes in class order; keys carry base rows through rank
            const ClassView* v = c->class_view.get();
            sp.scr = v->d_scr8;
            sp.norm2 = v->d_norm2_8;
            sp.rank = v->d_rank;
            sp.n_rows = v->n_rows;
        }
    }
    if (plan.k2g) {
        sp.scr_c = c->d_scr_c;
        sp.q_scr_c = reinterpret_cast<const uint4*>(ds + off_qc);
        sp.cstride4 = c->cstride4;
    }
    auto launch_pass = [&](uint32_t blocks, hipStream_t s) { return plan.k2g ? launch_gemm(sp, metric, blocks, s) : launch_mfmaw(sp, metric, blocks, s); };
    sp.q_slots = reinterpret_cast<const uint32_t*>(ds + off_qs);

    // int8 planes (exact_screen): seed and final selection as one wave per query, resident beside the main launches
    const bool wave_select = plan.int8 && ctx->select_wave;
    if (plan.n_blocks) {
        // ---- sample pass: every sample_stride-th tile, open threshold, into the queries' sample buffers ----
        Timed sample(ctx, 3, ctx->stream);                  // sample pass + seed select together
        sp.groups = reinterpret_cast<const ScanGroup*>(ds + off_gs);
        sp.n_groups = (uint32_t) plan.groups_s.size();
        sp.sample_stride = plan.sample_stride;
        sp.tau_init = nullptr;
        sp.block_map = nullptr;
        sp.qcand = ctx->d_samp.as<uint64_t>();
        sp.qcnt = scnt;
        sp.capq = GQ_SAMPLE_CAP;
        sp.k2i = plan.k2r_sample ? 4u : plan.k2i_sample ? 2u : 0u;   // (bit 2: the sample launch on K2r; bit 1: on K2i; bit 0: the main launch)
        HIPCHK(launch_pass(plan.n_blocks_s, ctx->stream));
        // walk alignment: the seed selection also turns the view's position word into this session's rotation of the main launch
        WalkHint walk{};
        if (plan.walk) {
            const uint32_t n_rows8 = plan.n_launch / 8;     // rotations are whole rows of 8 slots: one per XCD
            walk.rot = ctx->walk_rot_word();
            walk.pos = c->class_view->d_walk_pos;
            walk.table = reinterpret_cast<const uint32_t*>(ds + off_wt);
            walk.n_pos = plan.walk_n_pos;
            walk.shift = plan.walk_shift;
            walk.n_launch = plan.n_launch;
            if (ctx->walk_rot_set || ctx->walk_spread) {
                walk.mode = 2u;
                walk.value = 8u * (uint32_t) (ctx->walk_spread ? (uint64_t) (ctx->ordinal % 3u) * n_rows8 / 3u : ctx->walk_rot % n_rows8);
            } else if (ctx->walk_pos_set) {
                walk.mode = 1u;
                walk.value = ctx->walk_pos;
            }
        }
        HIPCHK((wave_select ? launch_seed_select_wave : launch_seed_select)(ctx->d_samp.as<uint64_t>(), scnt, GQ_SAMPLE_CAP, plan.kp_frac,
                                                                            ctx->d_tau.as<uint64_t>(), (uint32_t) nq, ctx->stream, walk));
        HIPCHK(sample.stop());
        // ---- main pass ----
        hipStream_t main_stream = ctx->stream;
        if (ctx->scan_lane) {                               // the main launch goes to the corpus's lane, behind this batch's seeds
            if (!c->scan_stream) HIPCHK(hipStreamCreateWithFlags(&c->scan_stream, hipStreamNonBlocking));
            if (!ctx->lane_in) {
                HIPCHK(hipEventCreateWithFlags(&ctx->lane_in, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&ctx->lane_out, hipEventDisableTiming));
            }
            HIPCHK(hipEventRecord(ctx->lane_in, ctx->stream));
            HIPCHK(hipStreamWaitEvent(c->scan_stream, ctx->lane_in, 0));
            main_stream = c->scan_stream;
        }
        Timed main(ctx, 1, main_stream);
        sp.groups = reinterpret_cast<const ScanGroup*>(ds + off_g);
        sp.n_groups = (uint32_t) plan.groups.size();
        sp.sample_stride = 1;
        sp.epi = survivors_per_wave_tile(plan, nq) <= MASK_EPI_SURVIVORS ? 1u : 0u;
        if (ctx->force_epi >= 0) sp.epi = (uint32_t) ctx->force_epi;
        if (plan.int8 && plan.qmax > 64) sp.epi = 1u;       // 128-column passes exist on K2i only (its parking area takes bursts)
        sp.k2i = plan.int8 && !plan.k2g && sp.epi == 1 && !ctx->no_k2i && sp.rw == 16 && sp.qmax <= 128 ? 1u : 0u;
        ctx->last_k2i = sp.k2i != 0;
        sp.dense = plan.class_view && VSR_MW_DENSE ? 1u : 0u;   // (the sample launch: K2r, vsr_i8r.h, when the plan chose it)
        sp.tau_init = ctx->d_tau.as<uint64_t>();
        sp.qcand = ctx->d_cand.as<uint64_t>();
        sp.qcnt = qcnt;
        sp.capq = GQ_CAP;
        if (!plan.block_map.empty() && !ctx->no_xcd_map) sp.block_map = reinterpret_cast<const uint2*>(ds + off_bm);
        if (plan.walk && sp.block_map && sp.dense) {        // (the sample launch above knows neither word)
            sp.walk_rot = walk.rot;
            sp.walk_pos = c->class_view->d_walk_pos;
        }
        HIPCHK(launch_pass(sp.block_map ? plan.n_launch : plan.n_blocks, main_stream));
        HIPCHK(main.stop());
        if (ctx->scan_lane) {                               // the selection waits for the lane
            HIPCHK(hipEventRecord(ctx->lane_out, main_stream));
            HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->lane_out, 0));
        }
        ctx->last_kernel = scan_kernel_name(plan, c, metric, ctx->last_k2i);
        if (plan.k2r_sample)
            ctx->last_kernel += " + sample vsr::i8_sample_reg_kernel<NQG=4> (K2r, stride " + std::to_string(plan.sample_stride) + ")";
        else if (plan.k2i_sample) ctx->last_kernel += " + sample vsr::i8_stream_kernel<NQG=4, SAMPLE=true>";
        else if (plan.int8) ctx->last_kernel += " + sample vsr::mfma_wide_kernel<L2, NCH=1, SAMPLE=true, PL=int8>";
        count_scan(ctx, plan, 1);
    }

    Timed select(ctx, 2, ctx->stream);
    RerankParams rr = rerank_params(ctx, c, ds, off_sq, kp, q.k, metric, q.out);
    rr.qcand = ctx->d_cand.as<uint64_t>();
    rr.qcnt = qcnt;
    rr.capq = GQ_CAP;
    rr.err_g = plan.k2g ? coarse_err_g(c->dim) : plane_err_g(c->dim);
    rr.err_tight = plan.k2g ? 1u : 0u;
    rr.qbad = plan.int8 ? reinterpret_cast<const uint32_t*>(ds + off_qb) : nullptr;
    rr.exact_screen = plan.int8 ? 1u : 0u;
    rr.seeded = 1;
    rr.tau_init = ctx->d_tau.as<uint64_t>();
    HIPCHK((wave_select ? launch_select_emit_wave : launch_select_rerank)(rr, (uint32_t) nq, ctx->stream));
    if (plan.n_blocks) ctx->last_kernel += wave_select ? " + select vsr::select_emit_wave_kernel" : " + select vsr::select_rerank_kernel";
    HIPCHK(select.stop());
    HIPCHK(whole.stop());
    ctx->stats.queries += nq;
    return VSR_OK;
}

// ---- one query, one pass -----------------------------------------------------------------------------------------
// The whole search in ONE launch (FusedTail, vsr_device.h).  Conditions: the query already lies in device memory in the row
// layout (d a multiple of 4, of 8 over a halfvec corpus: no padding to add), no |q|^2 needed (not cosine), one plain pass on K1, k small enough for the
// workgroup's LDS top-k buffer.  Returns the workgroups per first-level merge, 0: the call takes the general path.
uint32_t fused_fan(const vsr_ctx* ctx, const vsr_corpus* c, const Plan& plan, const Call& q)
{
    // (K1h rounds the query to binary16 itself as it enters LDS: no staging kernel needed for that either)
    if (c->format == RowFormat::BIT || c->format == RowFormat::SPARSE) return 0;   // K1b / K1s do not instantiate the in-kernel merge: staging + scan + K5
    if (!(q.nq == 1 && !ctx->no_fused && plan.groups.size() == 1 && plan.qi == 1 && !plan.k2 && !plan.mq && q.dim % (c->format == RowFormat::HALF ? 8 : 4) == 0 &&
          q.metric != VSR_METRIC_COSINE && plan.groups[0].n_blocks <= 64u * 64u && ctx->profiling != 1))
        return 0;
    const uint32_t kp = plan.keep;
    const uint32_t per_merge = kp ? 8192u / kp : 0u;        // lists one merge takes (16 keys per thread, vsr_scan.h)
    uint32_t fan = per_merge ? std::max<uint32_t>(16, (plan.groups[0].n_blocks + per_merge - 1) / per_merge) : 0u;
    if (ctx->fused_fan >= 16 && per_merge >= 16) fan = std::min<uint32_t>((uint32_t) ctx->fused_fan, per_merge);   // development knob (>= 16: d_done holds 256 group counters)
    return kp <= 512 && fan && fan <= per_merge ? fan : 0u;
}

int search_fused(vsr_ctx* ctx, vsr_corpus* c, const Plan& plan, const Call& q, uint32_t fan)
{
    const uint32_t kp = plan.keep;
    const int dim = q.dim, metric = q.metric;
    const vsr_corpus* idc = c->base ? c->base : c;          // identity arrays (c may be a list-ordered view)
    const ScanGroup& g = plan.groups[0];
    const uint32_t n_g = (g.n_blocks + fan - 1) / fan;
    RCCHK(ctx->d_partial.reserve((size_t) (g.n_blocks + n_g) * kp * sizeof(uint64_t)));
    RCCHK(ctx->d_flags.reserve(sizeof(int32_t)));
    if (!ctx->d_done.p) {
        RCCHK(ctx->d_done.reserve((size_t) (1 + 4096 / 16 + 64) * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(ctx->d_done.p, 0, ctx->d_done.cap, ctx->stream));
    }
    const float* q_dev = static_cast<const float*>(q.d_queries);   // (F32 or HALF corpus: fused_fan)
    if (!q_dev) {
        // host query: the kernel reads it straight out of the pinned staging block (512 bytes, cached after the
        // first workgroup), which the previous call's kernel must have left
        RCCHK(wait_for_staging_block(ctx));
        RCCHK(ctx->h_desc.reserve((size_t) c->stride4 * 4 * sizeof(float)));
        memcpy(ctx->h_desc.p, q.h_queries, (size_t) dim * sizeof(float));
        q_dev = reinterpret_cast<const float*>(ctx->h_desc.dp);
    }
    ScanParams sp = scan_params(ctx, c, kp, 1);
    sp.queries = q_dev;
    sp.partial = ctx->d_partial.as<uint64_t>();
    sp.cap = std::max<uint32_t>(4096, scan_cap_for_rw((int) kp, c->shape.rw));   // the merge's LDS layout (vsr_scan.h, FUSED_*)
    sp.n_groups = 1;
    sp.fused.enable = 1;
    sp.fused.fan = fan;
    sp.fused.group = g;
    sp.fused.group.block_begin = 0;
    sp.fused.group.partial_begin = 0;
    sp.fused.done = ctx->d_done.as<uint32_t>();
    set_keyed_results(sp.fused, idc, q.out);
    sp.fused.out_flag = ctx->d_flags.as<int32_t>();
    sp.fused.metric = metric;
    if (ctx->fused_dbg) {                                   // development: timestamps of the finishing workgroup, printed by the next call
        if (!ctx->d_dbg.p) {
            RCCHK(ctx->d_dbg.reserve(64));
            RCCHK(ctx->h_dbg.reserve(64));
        } else {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            const uint64_t* t = ctx->h_dbg.as<uint64_t>();
            HIPCHK(hipMemcpy(ctx->h_dbg.p, ctx->d_dbg.p, 64, hipMemcpyDeviceToHost));
            fprintf(stderr, "fused_dbg us: scan %.1f compact+publish %.1f wait %.1f merge1 %.1f publish+wait %.1f merge2 %.1f tail %.1f total %.1f\n",
                    (t[1] - t[0]) / 100.0, (t[2] - t[1]) / 100.0, t[3] ? (t[3] - t[2]) / 100.0 : 0.0, t[3] ? (t[4] - t[3]) / 100.0 : 0.0,
                    (t[5] - (t[4] ? t[4] : t[2])) / 100.0, (t[6] - t[5]) / 100.0, (t[7] - t[6]) / 100.0, (t[7] - t[0]) / 100.0);
        }
        sp.fused.dbg = ctx->d_dbg.as<uint64_t>();
    }
    Timed main(ctx, 0, ctx->stream);
    // SIFT-like corpus and query (u8-exact, L2): the same launch over the int8 planes -- a quarter of the bytes per
    // row, identical distances (vsr_scan.h, scan8_fused_kernel)
    const bool scan8 = c->d_scr8 && !c->base && metric == VSR_METRIC_L2 && ctx->int8_this_call && c->shape.rw == 16 &&
                       !ctx->no_scan8;
    if (scan8) {
        RCCHK(ensure_q8_word(ctx));
        sp.scr = c->d_scr8;
        sp.norm2 = c->d_norm2_8;
        sp.pstride4 = 8;
        sp.plane_ho = 2u;
        sp.fused.flag_total = ctx->d_flag_total;
        HIPCHK(launch_scan8_fused(sp, (uint32_t) dim, reinterpret_cast<uint32_t*>(ctx->h_q8.dp), g.n_blocks, ctx->stream));
    } else
        HIPCHK(launch_scan(c->format, sp, metric, c->dim, 1, g.n_blocks, ctx->stream));
    if (!q.d_queries) {
        HIPCHK(hipEventRecord(ctx->desc_done, ctx->stream));
        ctx->desc_pending = true;
    }
    HIPCHK(main.stop());
    ctx->last_kernel = scan8 ? std::string("vsr::scan8_fused_kernel (K1 on the int8 planes) + in-kernel merge")
                             : scan_kernel_name(plan, c, metric) + " + in-kernel merge";
    count_scan(ctx, plan, 0);
    ctx->stats.queries += 1;
    return VSR_OK;
}

// ---- the general path: K1 / K1m / K2 scan into partial lists, K5 select (and K5r re-rank) -----------------------
constexpr uint32_t SEED_LIST = 64;                          // keys a sample-pass workgroup publishes per query (one tile: no selection)

// Threshold seeding: a 1/seed_stride sample pass of the same launch, then the m-th best sampled candidate of each query
// becomes the initial threshold of the main pass (all rows at or before it stay eligible; a query whose seed turns out
// too tight is flagged by K5 / K5r and re-run unseeded).  m = seed_rank of the sample's fraction makes a too-tight seed
// a ~1e-8 event (and a detected one).  The m-th best of the whole sample only involves the m best of every sample list, so
// those lists are short.  Every sample workgroup visits at least one 64-row tile, so a pass cut into many workgroups is
// sampled more densely than 1 / seed_stride: lambda uses the densest pass's fraction (a larger m only loosens the seed).
// (Not vsr_plan.hip's densest_fraction: this launch's workgroups sample one 64-row tile each however long their range.)
uint32_t legacy_seed_rank(const vsr_ctx* ctx, const vsr_corpus* c, const Plan& plan)
{
    double frac = 1.0 / ctx->seed_stride;
    for (const ScanGroup& g : plan.groups_s) {
        const double rows = (double) g.n_tiles * c->shape.rw;
        if (rows > 0) frac = std::max(frac, std::min(1.0, 64.0 * g.n_blocks / rows));
    }
    return seed_rank(plan.keep, frac);
}

int search_general(vsr_ctx* ctx, vsr_corpus* c, const Plan& plan, const Call& q, bool allow_screening)
{
    const uint32_t kp = plan.keep;
    const int nq = q.nq, metric = q.metric;
    const vsr_corpus* idc = c->base ? c->base : c;          // identity arrays and re-rank rows (c may be a list-ordered view)
    const size_t qfloats = (size_t) c->stride4 * 4;
    Staging sb;
    const bool sparse = c->format == RowFormat::SPARSE, half = c->format == RowFormat::HALF;
    const uint32_t sp_slots = sparse ? ctx->sparse_slots : 0u;
    sb.add(sparse ? (size_t) nq * sp_slots * sizeof(uint2) : (size_t) nq * qfloats * sizeof(float));   // queries (sparse: their tables)
    const size_t off_qn = sb.add((size_t) nq * sizeof(float));
    const size_t off_qt = sb.add(sparse ? (size_t) nq * 2 * sizeof(double) : 0);   // K1s: sum q^2, sum |q| in double
    const bool k2h = plan.k2 && half;                       // K2h: the queries also as binary16, its B fragments
    const size_t off_qh = sb.add(k2h ? (size_t) nq * qfloats * sizeof(uint16_t) : 0);
    const size_t off_g = sb.add(plan.groups);               // copied from here on
    const size_t off_gs = sb.add(plan.groups_s);
    const size_t off_qs = sb.add(plan.q_slots);
    const size_t off_s1 = sb.add(plan.sel1);
    const size_t off_sq = sb.add(plan.selq);
    const size_t off_sd = sb.add(plan.seedq);
    const size_t off_li = sb.add(plan.list_ids);
    const size_t off_bm = sb.add(plan.block_map);

    StageParams st{};                                       // (no query planes, no K2w counters on this path)
    if (!sparse) {
        RCCHK(stage_host_part(ctx, sb, off_qn, off_g, c->format, q.h_queries, q.d_queries, nq, q.dim, qfloats, st));
        st.q_half = half ? 1u : 0u;
        if (k2h) st.q_h16 = reinterpret_cast<_Float16*>(ctx->d_desc.as<char>() + off_qh);
    }
    RCCHK(ctx->d_partial.reserve(std::max<size_t>(8, (size_t) plan.n_partial * kp * sizeof(uint64_t))));
    Timed whole(ctx, 5, ctx->stream);                       // the whole search on the device
    if (sparse) RCCHK(stage_sparse(ctx, sb, off_qt, off_qn, off_g, *q.sparse, nq, q.dim, sp_slots));
    else RCCHK(launch_staging(ctx, st));
    char* ds = ctx->d_desc.as<char>();

    ScanParams sp = scan_params(ctx, c, kp, plan.qmax);
    sp.queries = reinterpret_cast<const float*>(ds);
    sp.q_norm2 = reinterpret_cast<const float*>(ds + off_qn);
    if (k2h) sp.q_scr = reinterpret_cast<const uint4*>(ds + off_qh);
    if (sparse) {
        sp.sp_off = c->d_sp_off;
        sp.sp_tab = reinterpret_cast<const uint2*>(ds);
        sp.sp_slots = sp_slots;
        sp.sp_qtot = reinterpret_cast<const double*>(ds + off_qt);
    }
    sp.partial = ctx->d_partial.as<uint64_t>();
    sp.cap = plan.k2 ? mfma_cap_for_k(kp) : scan_cap_for_rw((int) kp, c->shape.rw);
    if (plan.mq || plan.k2) {
        RCCHK(ctx->d_cand.reserve(std::max<size_t>(8, (size_t) plan.n_scan_lists * cand_pitch(sp.cap) * sizeof(uint64_t))));
        sp.cand = ctx->d_cand.as<uint64_t>();
    }
    sp.groups = reinterpret_cast<const ScanGroup*>(ds + off_g);
    sp.n_groups = (uint32_t) plan.groups.size();
    sp.q_slots = reinterpret_cast<const uint32_t*>(ds + off_qs);

    SelectParams sel{};
    sel.partial = ctx->d_partial.as<uint64_t>();
    sel.list_ids = reinterpret_cast<const uint32_t*>(ds + off_li);
    sel.kp = kp;
    // short candidate streams (<= 16k keys per query) merge faster with small workgroups
    uint32_t max_lists = 1;
    for (auto& s : plan.selq) max_lists = std::max(max_lists, s.n_lists);
    for (auto& s : plan.sel1) max_lists = std::max(max_lists, s.n_lists);
    uint32_t max_seed_lists = 1;
    for (auto& s : plan.seedq) max_seed_lists = std::max(max_seed_lists, s.n_lists);
    if (!plan.sel_wave) max_lists = std::max(max_lists, max_seed_lists);
    const int sel_threads = plan.sel_wave ? 64 : (uint64_t) max_lists * kp <= 16384 ? 256 : 1024;
    sel.cap = plan.sel_wave ? std::max<uint32_t>(1024, max_lists * kp) : select_cap(kp, sel_threads);   // wave: key capacity
    sel.metric = metric;
    set_keyed_results(sel, idc, q.out);
    sel.out_flags = ctx->d_flags.as<int32_t>();
    sel.flagged_total = ctx->d_flag_total;

    const uint32_t seed_m = legacy_seed_rank(ctx, c, plan);
    const bool seed = allow_screening && ctx->screening && ctx->seeding && (plan.k2 || plan.mq) && plan.n_blocks > 0 &&
                      seed_m <= SEED_LIST && kp >= SEED_LIST &&
                      plan.scan_rows >= ctx->seed_min_rows &&
                      plan.scan_rows / (int64_t) std::max<size_t>(1, plan.groups.size()) >= ctx->seed_min_pass_rows;
    if (seed) {
        sp.sample_stride = ctx->seed_stride;
        sp.groups = reinterpret_cast<const ScanGroup*>(ds + off_gs);
        sp.n_groups = (uint32_t) plan.groups_s.size();
        Timed sample(ctx, 3, ctx->stream);
        sp.kp = sp.k = SEED_LIST;
        if (k2h) HIPCHK(launch_mfmah(sp, metric, plan.n_blocks_s, ctx->stream));
        else if (plan.k2) HIPCHK(launch_mfma(sp, metric, plan.n_blocks_s, ctx->stream));
        else HIPCHK(launch_mq(sp, metric, plan.n_blocks_s, ctx->stream));
        sp.kp = sp.k = kp;
        HIPCHK(sample.stop());
        Timed seeds_t(ctx, 4, ctx->stream);
        sp.groups = reinterpret_cast<const ScanGroup*>(ds + off_g);
        sp.n_groups = (uint32_t) plan.groups.size();
        SelectParams seeds = sel;
        seeds.kp = SEED_LIST;
        seeds.k = seed_m;
        if (plan.sel_wave) seeds.cap = std::max<uint32_t>(1024, max_seed_lists * SEED_LIST);   // <= 64 lists (planner)
        seeds.tau_out = ctx->d_tau.as<uint64_t>();
        seeds.queries = reinterpret_cast<const SelectQuery*>(ds + off_sd);
        HIPCHK(launch_select(seeds, (uint32_t) plan.seedq.size(), sel_threads, ctx->stream));
        HIPCHK(seeds_t.stop());
        sp.sample_stride = 1;
        sp.tau_init = ctx->d_tau.as<uint64_t>();
        sel.seeded = 1;
    }

    const int cls = plan.qi == 4 ? 1 : 0;
    if (plan.n_blocks) {
        Timed main(ctx, cls, ctx->stream);
        if (!plan.block_map.empty() && !ctx->no_xcd_map) sp.block_map = reinterpret_cast<const uint2*>(ds + off_bm);
        const uint32_t launch_blocks = sp.block_map ? plan.n_launch : plan.n_blocks;
        if (k2h) HIPCHK(launch_mfmah(sp, metric, launch_blocks, ctx->stream));
        else if (plan.k2) HIPCHK(launch_mfma(sp, metric, launch_blocks, ctx->stream));
        else if (plan.mq) HIPCHK(launch_mq(sp, metric, launch_blocks, ctx->stream));
        else HIPCHK(launch_scan(c->format, sp, metric, c->dim, plan.qi, plan.n_blocks, ctx->stream, c->shape.lpr, plan.sparse_global));
        HIPCHK(main.stop());
        ctx->last_kernel = scan_kernel_name(plan, c, metric);
        count_scan(ctx, plan, cls);
    }

    sel.k = kp;
    Timed select(ctx, 2, ctx->stream);
    if (!plan.sel1.empty()) {
        sel.queries = reinterpret_cast<const SelectQuery*>(ds + off_s1);
        HIPCHK(launch_select(sel, (uint32_t) plan.sel1.size(), sel_threads, ctx->stream));
    }
    sel.queries = reinterpret_cast<const SelectQuery*>(ds + off_sq);
    HIPCHK(launch_select(sel, (uint32_t) nq, sel_threads, ctx->stream));
    if (plan.k2) {
        RerankParams rr = rerank_params(ctx, c, ds, off_sq, kp, q.k, metric, q.out);
        rr.lists = ctx->d_partial.as<uint64_t>() + (size_t) plan.rerank_base * kp;
        rr.err_g = half ? half_err_g(c->dim) : k2_err_g(c->dim);   // K2h's / K2's fp32 accumulation (vsr_bounds.h)
        rr.seeded = seed ? 1 : 0;
        rr.tau_init = seed ? ctx->d_tau.as<uint64_t>() : nullptr;
        HIPCHK(launch_rerank(rr, (uint32_t) nq, ctx->stream));
    }
    HIPCHK(select.stop());
    HIPCHK(whole.stop());
    ctx->stats.queries += nq;
    return VSR_OK;
}

// int8 planes (SIFT-like corpora): host queries are checked here; device-resident queries only under the caller's
// hint (vsr_set_query_hint), validated by the staging kernel -- a violating query is flagged, and the hint is dropped
// once the kernel's pinned word shows one (read without synchronising: at worst a batch late)
bool queries_are_u8(vsr_ctx* ctx, const vsr_corpus* c, const Call& q, bool allow_screening)
{
    if (ctx->q8_ok && ctx->h_q8.p && *reinterpret_cast<volatile uint32_t*>(ctx->h_q8.p)) ctx->q8_ok = false;
    if (!(c->d_scr8 && q.metric == VSR_METRIC_L2 && allow_screening)) return false;
    if (!q.h_queries) return ctx->hint_u8 && ctx->q8_ok;
    bool ok = true;
    const float* hq = static_cast<const float*>(q.h_queries);   // (int8 planes: an F32 corpus)
    const size_t total = (size_t) q.nq * q.dim;
    for (size_t i = 0; i < total && ok; ++i) {
        const float v = hq[i];
        ok = v >= 0.0f && v <= 255.0f && v == floorf(v);
    }
    return ok;
}

// Shared by the host and device entry points.
// `ctx` is the session the search runs in (stream, workspaces, counters): the corpus's own context, or another context
// of the same device (vsr_search_device_on) so that two batches over one corpus can be in flight at once.
// level: 2 = every screening tier (coarse planes for wide passes over long rows, K2g), 1 = fine planes only (K2w / K2),
// 0 = exact kernels only.  A query flagged at one level is re-run at the next lower one (host_search,
// vsr_search_device_exact).
int search_impl(vsr_ctx* ctx, vsr_corpus* c, const Call& q, const vsr_filter* const* filters, int level)
{
    const bool allow_screening = level >= 1;
    ctx->screen_level = level;
    const auto h0 = Clock::now();
    ctx->int8_this_call = queries_are_u8(ctx, c, q, allow_screening);
    if (q.sparse) ctx->sparse_slots = sparse_slots_for_nnz(q.sparse->max_nnz);
    static thread_local Plan plan;
    if (!make_plan(ctx, c, q.nq, q.k, q.metric, allow_screening, true, true, filters, plan)) {
        // K2g could not be seeded safely: K2w; K2w neither: legacy shared passes
        if (!plan.k2g || !make_plan(ctx, c, q.nq, q.k, q.metric, allow_screening, true, false, filters, plan))
            (void) make_plan(ctx, c, q.nq, q.k, q.metric, allow_screening, false, false, filters, plan);
    }
    ctx->last_coarse = plan.k2g;
    ctx->host_us[0] += us_since(h0);
    const uint32_t fan = plan.k2w ? 0u : fused_fan(ctx, c, plan, q);
    const int rc = plan.k2w ? search_wide(ctx, c, plan, q) : fan ? search_fused(ctx, c, plan, q, fan) : search_general(ctx, c, plan, q, allow_screening);
    const double spent = us_since(h0);
    ctx->host_us[2] += spent;
    ctx->stats.host_ms += spent * 1e-3;
    ctx->host_calls++;
    return rc;
}

}  // namespace

int vsr::check_search_args(const vsr_corpus* c, const void* queries, int nq, int dim, int k, int metric,
                           const vsr_filter* const* filters, const char* who, RowFormat entry)
{
    if (!c) return fail(VSR_ERR_INVALID, "%s: corpus is NULL", who);
    const bool bit = c->format == RowFormat::BIT, sparse = c->format == RowFormat::SPARSE;
    if (entry == RowFormat::SPARSE && !sparse) return fail(VSR_ERR_INVALID, "%s: the corpus is not a sparse corpus", who);
    if (sparse && entry != RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus is searched with vsr_search_sparse* (<->, <#>, <=>, <+>) and has no index path yet", who);
    if (entry == RowFormat::BIT && !bit) return fail(VSR_ERR_INVALID, "%s: the corpus is not a bit corpus", who);
    if (bit && entry != RowFormat::BIT)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a bit corpus is searched with vsr_search_bit* (<~> / <%%>), its graphs with vsr_hnsw_search_bit*", who);
    if (nq < 0 || (nq > 0 && !queries)) return fail(VSR_ERR_INVALID, "%s: queries is NULL", who);
    if (dim != c->dim && sparse)                            // CheckDims, sparsevec.c
        return fail(VSR_ERR_DIM_MISMATCH, "different sparsevec dimensions %d and %d", c->dim, dim);
    if (dim != c->dim && bit)                               // CheckDims, bitvec.c:32-39: the column's length first
        return fail(VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u", (unsigned) c->dim, (unsigned) dim);
    if (dim != c->dim)                                      // CheckDims: vector.c:60-67, halfvec.c:60-67
        return fail(VSR_ERR_DIM_MISMATCH, "different %s dimensions %d and %d", format_name(c->format), c->dim, dim);
    if (k < 1) return fail(VSR_ERR_INVALID, "%s: k must be >= 1 (got %d)", who, k);
    if (k > VSR_MAX_K) return fail(VSR_ERR_UNSUPPORTED, "%s: k = %d exceeds VSR_MAX_K = %d", who, k, VSR_MAX_K);
    if (entry == RowFormat::BIT ? metric != VSR_METRIC_HAMMING && metric != VSR_METRIC_JACCARD : metric < VSR_METRIC_L2 || metric > VSR_METRIC_L1)
        return fail(VSR_ERR_INVALID, "%s: metric %d", who, metric);
    if (filters)
        for (int i = 0; i < nq; ++i)
            if (filters[i] && filters[i]->corpus != c) return fail(VSR_ERR_INVALID, "%s: filter %d belongs to another corpus", who, i);
    return VSR_OK;
}

// vsr_search_device_on (entry = F32) and vsr_search_bit_device_on (BIT: d_queries addresses packed bit strings)
static int search_device_on(vsr_ctx* session, vsr_corpus* c, RowFormat entry, const void* d_queries, int nq, int dim, int k, int metric,
                            const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist,
                            int32_t* d_cnt, uint64_t* d_keys)
{
    int rc = check_search_args(c, d_queries, nq, dim, k, metric, filters, entry == RowFormat::BIT ? "vsr_search_bit_device" : "vsr_search_device", entry);
    if (rc) return rc;
    vsr_ctx* ctx = session ? session : c->ctx;
    if (ctx->device != c->ctx->device) return fail(VSR_ERR_INVALID, "vsr_search_device_on: session and corpus are on different devices");
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "vsr_search_device: output is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    if (!d_doc) {
        if ((rc = ctx->d_misc.reserve((size_t) nq * k * sizeof(int32_t)))) return rc;
        d_doc = ctx->d_misc.as<int32_t>();
    }
    return search_impl(ctx, c, {nullptr, d_queries, nq, dim, k, metric, {d_blk, d_doc, d_row, d_dist, d_cnt, d_keys}}, filters, 2);
}

extern "C" int vsr_search_device_on(vsr_ctx* session, vsr_corpus* c, const float* d_queries, int nq, int dim, int k,
                                    int metric, const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc,
                                    int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return search_device_on(session, c, RowFormat::F32, d_queries, nq, dim, k, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_bit_device_on(vsr_ctx* session, vsr_corpus* c, const uint8_t* d_queries, int nq, int dim, int k,
                                        int metric, const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc,
                                        int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return search_device_on(session, c, RowFormat::BIT, d_queries, nq, dim, k, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_bit_device(vsr_corpus* c, const uint8_t* d_queries, int nq, int dim, int k, int metric,
                                     const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                     float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return vsr_search_bit_device_on(nullptr, c, d_queries, nq, dim, k, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_device(vsr_corpus* c, const float* d_queries, int nq, int dim, int k, int metric,
                                 const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                 float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return vsr_search_device_on(nullptr, c, d_queries, nq, dim, k, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt,
                                d_keys);
}

// The search of vsr_search_bit_device over a corpus or a list-ordered view of one (vsr_ivf_search_bit_device, K3b), arguments
// already checked by the caller: enqueued on the corpus context's stream, not waited for.  Bit corpora only: K1b is exact by
// construction, so there is nothing to flag or re-run (fp32 / halfvec views: vsr_search_device_exact).
int vsr::device_search(vsr_corpus* c, const void* d_queries, int nq, int dim, int k, int metric, const vsr_filter* const* filters,
                       const Outputs& out)
{
    vsr_ctx* ctx = c->ctx;
    if (nq == 0) return VSR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Outputs o = out;
    if (!o.doc) {
        int rc = ctx->d_misc.reserve((size_t) nq * k * sizeof(int32_t));
        if (rc) return rc;
        o.doc = ctx->d_misc.as<int32_t>();
    }
    return search_impl(ctx, c, {nullptr, d_queries, nq, dim, k, metric, o}, filters, 2);
}

// The device API for callers that cannot tolerate an unproven row: search, wait, re-run what was flagged, patch.
extern "C" int vsr_search_device_exact(vsr_ctx* session, vsr_corpus* c, const float* d_queries, int nq, int dim, int k,
                                       int metric, const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc,
                                       int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys, int32_t* n_rerun)
{
    if (n_rerun) *n_rerun = 0;
    int rc = vsr_search_device_on(session, c, d_queries, nq, dim, k, metric, filters, d_blk, d_doc, d_row, d_dist, d_cnt, d_keys);
    if (rc || nq == 0) return rc;
    vsr_ctx* ctx = session ? session : c->ctx;
    std::vector<int32_t> flags((size_t) nq, 0);
    HIPCHK(hipMemcpyAsync(flags.data(), ctx->d_flags.p, (size_t) nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<int> redo;
    for (int i = 0; i < nq; ++i)
        if (flags[(size_t) i]) redo.push_back(i);
    if (redo.empty()) return VSR_OK;
    ctx->flagged_seen += (int64_t) redo.size();
    if (n_rerun) *n_rerun = (int32_t) redo.size();
    // flagged on the coarse planes: the fine planes next; flagged there (or no coarse tier involved): the exact kernels
    for (int level = ctx->last_coarse ? 1 : 0; level >= 0 && !redo.empty(); --level) {
        const size_t nr = redo.size(), nk = nr * (size_t) k;
        // workspace: [queries | block | row | doc | dist | keys | counts] of the flagged queries
        const size_t o_q = 0, o_blk = align_up(o_q + nr * (size_t) dim * 4, 256), o_row = align_up(o_blk + nk * 8, 256),
                     o_doc = align_up(o_row + nk * 8, 256), o_dist = align_up(o_doc + nk * 4, 256),
                     o_key = align_up(o_dist + nk * 4, 256), o_cnt = align_up(o_key + nk * 8, 256),
                     total = align_up(o_cnt + nr * 4, 256);
        if ((rc = ctx->d_redo.reserve(total))) return rc;
        char* w = ctx->d_redo.as<char>();
        const Outputs redone{reinterpret_cast<int64_t*>(w + o_blk), reinterpret_cast<int32_t*>(w + o_doc),
                             reinterpret_cast<int64_t*>(w + o_row), reinterpret_cast<float*>(w + o_dist),
                             reinterpret_cast<int32_t*>(w + o_cnt), reinterpret_cast<uint64_t*>(w + o_key)};
        std::vector<const vsr_filter*> f2(nr, nullptr);
        for (size_t j = 0; j < nr; ++j) {
            HIPCHK(hipMemcpyAsync(w + o_q + j * (size_t) dim * 4, d_queries + (size_t) redo[j] * dim, (size_t) dim * 4,
                                  hipMemcpyDeviceToDevice, ctx->stream));
            if (filters) f2[j] = filters[redo[j]];
        }
        rc = search_impl(ctx, c, {nullptr, w + o_q, (int) nr, dim, k, metric, redone}, f2.data(), level);
        if (rc) return rc;
        const Outputs all{d_blk, d_doc, d_row, d_dist, d_cnt, d_keys};
        for (size_t j = 0; j < nr; ++j) {
            const Outputs from = redone.from_query(j, k), to = all.from_query((size_t) redo[j], k);
            auto patch = [&](void* dst, const void* src, size_t bytes) {
                return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
            };
            HIPCHK(patch(to.blk, from.blk, (size_t) k * 8));
            if (to.row) HIPCHK(patch(to.row, from.row, (size_t) k * 8));
            if (to.doc) HIPCHK(patch(to.doc, from.doc, (size_t) k * 4));
            HIPCHK(patch(to.dist, from.dist, (size_t) k * 4));
            if (to.keys) HIPCHK(patch(to.keys, from.keys, (size_t) k * 8));
            HIPCHK(patch(to.cnt, from.cnt, 4));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(flags.data(), ctx->d_flags.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<int> still;
        for (size_t j = 0; j < nr; ++j)
            if (flags[j]) still.push_back(redo[j]);
        // the exact path never flags; anything else is a library fault and must not be published
        if (level == 0 && !still.empty())
            return fail(VSR_ERR_HIP, "vsr_search_device_exact: query %d still flagged after the exact re-run", still[0]);
        redo.swap(still);
    }
    return VSR_OK;
}

// Host-buffer search on a corpus or on a list-ordered view of one: the search, then the re-run of the (rare) flagged
// queries one tier down -- coarse planes -> fine planes -> exact kernels.
int vsr::host_search(vsr_corpus* c, const void* queries, int nq, int dim, int k, int metric, const vsr_filter* const* filters,
                     const Outputs& out)
{
    int rc;
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    // [results | flags] in pinned memory.  Small results (the harness's one query per call) are written there by the kernels
    // themselves -- the block is mapped into the device's address space -- so a call is its launches, a 4-byte-per-query copy of
    // the flags and ONE wait; larger ones go through device memory and one packed copy.
    const ResultBlock rb(nq, k, false);
    const size_t results = rb.o_status;
    const bool direct = results <= 64 * 1024;
    if (!direct && (rc = ctx->d_out.reserve(results))) return rc;
    if ((rc = ctx->h_out.reserve(rb.total))) return rc;
    char* d = direct ? static_cast<char*>(ctx->h_out.dp) : ctx->d_out.as<char>();
    char* h = ctx->h_out.as<char>();
    auto run = [&](const void* qs, int n, const vsr_filter* const* fs, int level) -> int {
        int r = search_impl(ctx, c, {qs, nullptr, n, dim, k, metric, rb.arrays(d)}, fs, level);
        if (r) return r;
        if (!direct) HIPCHK(hipMemcpyAsync(h, d, results, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(h + rb.o_status, ctx->d_flags.p, (size_t) n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return VSR_OK;
    };
    if ((rc = run(queries, nq, filters, 2))) return rc;
    rb.copy_out_all(h, out, nullptr);
    std::vector<int> redo = rb.flagged(h, (size_t) nq);
    if (!redo.empty()) ctx->flagged_seen += (int64_t) redo.size();
    std::vector<float> q2;
    std::vector<const vsr_filter*> f2;
    for (int level = ctx->last_coarse ? 1 : 0; level >= 0 && !redo.empty(); --level) {
        gather_subset(static_cast<const float*>(queries), dim, filters, redo, q2, f2);   // (only screening flags: fp32 queries)
        if ((rc = run(q2.data(), (int) redo.size(), f2.data(), level))) return rc;
        std::vector<int> still;
        for (size_t j = 0; j < redo.size(); ++j) {
            if (rb.column<int32_t>(h, rb.o_status)[j] && level > 0) still.push_back(redo[j]);    // unproven again: one more tier down
            else rb.patch_one(h, j, (size_t) redo[j], out, nullptr);
        }
        redo.swap(still);
    }
    return VSR_OK;
}

extern "C" int vsr_search(vsr_corpus* c, const float* queries, int nq, int dim, int k, int metric,
                          const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                          float* out_dist, int32_t* out_cnt)
{
    int rc = check_search_args(c, queries, nq, dim, k, metric, filters, "vsr_search");
    if (rc) return rc;
    if (c->base) return fail(VSR_ERR_INVALID, "vsr_search: this corpus is an index view; use the index's search function");
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "vsr_search: output is NULL");
    // `$1::halfvec`: a finite element that rounds to +-Inf is an error (halfvec_in, halfvec.c:224-230); 65520 is the smallest
    // magnitude that does.  (The device entry points do not look: the element becomes +-Inf.)
    if (c->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;
    return host_search(c, queries, nq, dim, k, metric, filters, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr});
}

// ORDER BY col <~> $1 / col <%> $1 LIMIT k over a bit corpus.  Exact by construction: nothing flags, nothing is re-run.
extern "C" int vsr_search_bit(vsr_corpus* c, const uint8_t* queries, int nq, int dim, int k, int metric,
                              const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc, int64_t* out_row,
                              float* out_dist, int32_t* out_cnt)
{
    int rc = check_search_args(c, queries, nq, dim, k, metric, filters, "vsr_search_bit", RowFormat::BIT);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "vsr_search_bit: output is NULL");
    return host_search(c, queries, nq, dim, k, metric, filters, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr});
}

// ORDER BY col <op> $1 LIMIT k over a sparse corpus (sparsevec.c:803-1037).  Exact by construction: nothing flags.
static int search_sparse_device_on(vsr_ctx* session, vsr_corpus* c, const int64_t* d_indptr, const int32_t* d_indices, const float* d_values,
                                   int nq, int dim, int max_query_nnz, int k, int metric, const vsr_filter* const* filters, int64_t* d_blk,
                                   int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    const char* who = "vsr_search_sparse_device";
    int rc = check_search_args(c, d_indptr, nq, dim, k, metric, filters, who, RowFormat::SPARSE);
    if (rc) return rc;
    if (max_query_nnz < 0 || max_query_nnz > SPARSE_MAX_NNZ)
        return fail(VSR_ERR_INVALID, "%s: max_query_nnz must be between 0 and %d (got %d)", who, SPARSE_MAX_NNZ, max_query_nnz);
    if (nq > 0 && max_query_nnz > 0 && (!d_indices || !d_values)) return fail(VSR_ERR_INVALID, "%s: queries is NULL", who);
    vsr_ctx* ctx = session ? session : c->ctx;
    if (ctx->device != c->ctx->device) return fail(VSR_ERR_INVALID, "vsr_search_sparse_device_on: session and corpus are on different devices");
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    HIPCHK(hipSetDevice(ctx->device));
    if (!d_doc) {
        if ((rc = ctx->d_misc.reserve((size_t) nq * k * sizeof(int32_t)))) return rc;
        d_doc = ctx->d_misc.as<int32_t>();
    }
    const SparseQueries sq{d_indptr, d_indices, d_values, false, (uint32_t) max_query_nnz};
    return search_impl(ctx, c, {nullptr, nullptr, nq, dim, k, metric, {d_blk, d_doc, d_row, d_dist, d_cnt, d_keys}, &sq}, filters, 0);
}

extern "C" int vsr_search_sparse_device_on(vsr_ctx* session, vsr_corpus* c, const int64_t* d_indptr, const int32_t* d_indices,
                                           const float* d_values, int nq, int dim, int max_query_nnz, int k, int metric,
                                           const vsr_filter* const* filters, int64_t* d_blk, int32_t* d_doc, int64_t* d_row,
                                           float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return search_sparse_device_on(session, c, d_indptr, d_indices, d_values, nq, dim, max_query_nnz, k, metric, filters, d_blk, d_doc,
                                   d_row, d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_sparse_device(vsr_corpus* c, const int64_t* d_indptr, const int32_t* d_indices, const float* d_values, int nq,
                                        int dim, int max_query_nnz, int k, int metric, const vsr_filter* const* filters, int64_t* d_blk,
                                        int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return search_sparse_device_on(nullptr, c, d_indptr, d_indices, d_values, nq, dim, max_query_nnz, k, metric, filters, d_blk, d_doc,
                                   d_row, d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_sparse(vsr_corpus* c, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq, int dim,
                                 int k, int metric, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                                 int64_t* out_row, float* out_dist, int32_t* out_cnt)
{
    const char* who = "vsr_search_sparse";
    int rc = check_search_args(c, q_indptr, nq, dim, k, metric, filters, who, RowFormat::SPARSE);
    if (rc) return rc;
    uint32_t max_nnz = 0;
    if ((rc = check_sparse_rows(who, q_indptr, q_indices, q_values, nq, dim, &max_nnz))) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    vsr_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const ResultBlock rb(nq, k, false);                     // results in device memory, one packed copy back, one wait
    if ((rc = ctx->d_out.reserve(rb.o_status))) return rc;
    if ((rc = ctx->h_out.reserve(rb.total))) return rc;
    char* d = ctx->d_out.as<char>();
    char* h = ctx->h_out.as<char>();
    const SparseQueries sq{q_indptr, q_indices, q_values, true, max_nnz};
    if ((rc = search_impl(ctx, c, {nullptr, nullptr, nq, dim, k, metric, rb.arrays(d), &sq}, filters, 0))) return rc;
    HIPCHK(hipMemcpyAsync(h, d, rb.o_status, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rb.copy_out_all(h, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    return VSR_OK;
}

// ---- two-stage search: Hamming shortlist on the bits (K1b), exact re-rank on the source rows ------------------------
// What the three vsr_search_quantized* entry points share.  Exactly one of h_queries / d_queries is set; `out` addresses
// device memory either way (the host entry point hands in its result block).  Everything is enqueued on ctx->stream:
//   binary_quantize of the queries -> stage 1 = the internal search over `bits` with k = shortlist, its keys into the
//   session's scratch -> shortlist_rerank_kernel over the source rows -> shortlist_emit_kernel.
int vsr::check_quantized_args(const vsr_ctx* session, const vsr_corpus* src, const vsr_corpus* bits, const void* queries, int nq,
                                int dim, int k, int shortlist, int metric, const vsr_filter* const* filters, const char* who)
{
    if (!src || !bits) return fail(VSR_ERR_INVALID, "%s: corpus is NULL", who);
    if (src->format == RowFormat::SPARSE || bits->format == RowFormat::SPARSE)
        return fail(VSR_ERR_UNSUPPORTED, "%s: a sparsevec corpus has no two-stage search (pgvector defines no binary_quantize for sparsevec)", who);
    if (src->format == RowFormat::BIT) return fail(VSR_ERR_INVALID, "%s: the source corpus is a bit corpus (the re-rank needs the fp32 or halfvec rows)", who);
    if (src->base) return fail(VSR_ERR_INVALID, "%s: the source corpus is an index view", who);
    if (bits->format != RowFormat::BIT) return fail(VSR_ERR_INVALID, "%s: the bits corpus is not a bit corpus", who);
    if (bits->quantized_from != src->serial) {
        char from[64] = "it was loaded with vsr_corpus_load_bit";
        if (bits->quantized_from) snprintf(from, sizeof from, "it was made from corpus #%llu", (unsigned long long) bits->quantized_from);
        return fail(VSR_ERR_INVALID, "%s: bits corpus #%llu (%lld rows of %d bits) was not made from source corpus #%llu (%s, %lld rows "
                    "of %d dimensions) by vsr_corpus_binary_quantize: %s", who, (unsigned long long) bits->serial, (long long) bits->n,
                    bits->dim, (unsigned long long) src->serial, format_name(src->format), (long long) src->n, src->dim, from);
    }
    if (nq < 0 || (nq > 0 && !queries)) return fail(VSR_ERR_INVALID, "%s: queries is NULL", who);
    if (dim != src->dim)                                    // CheckDims: vector.c:60-67, halfvec.c:60-67
        return fail(VSR_ERR_DIM_MISMATCH, "different %s dimensions %d and %d", format_name(src->format), src->dim, dim);
    if (k < 1) return fail(VSR_ERR_INVALID, "%s: k must be >= 1 (got %d)", who, k);
    if (shortlist < k) return fail(VSR_ERR_INVALID, "%s: shortlist = %d is shorter than k = %d", who, shortlist, k);
    if (shortlist > VSR_MAX_K) return fail(VSR_ERR_INVALID, "%s: shortlist = %d exceeds VSR_MAX_K = %d", who, shortlist, VSR_MAX_K);
    if (metric == VSR_METRIC_L1) return fail(VSR_ERR_UNSUPPORTED, "%s: the re-rank has no L1 form (metric 3)", who);
    if (metric < VSR_METRIC_L2 || metric > VSR_METRIC_L1) return fail(VSR_ERR_INVALID, "%s: metric %d", who, metric);
    if (filters)
        for (int i = 0; i < nq; ++i)
            if (filters[i] && filters[i]->corpus != bits)
                return fail(VSR_ERR_INVALID, "%s: filter %d belongs to another corpus (the bits corpus is the one scanned: it owns the filters)", who, i);
    if (src->ctx->device != bits->ctx->device || (session && session->device != bits->ctx->device))
        return fail(VSR_ERR_INVALID, "%s: session and corpora are on different devices", who);
    return VSR_OK;
}

static int search_quantized_impl(vsr_ctx* ctx, vsr_corpus* src, vsr_corpus* bits, const float* h_queries, const float* d_queries,
                                 int nq, int dim, int k, int shortlist, int metric, const vsr_filter* const* filters, const Outputs& out)
{
    const size_t ns = (size_t) nq * (size_t) shortlist, qbytes = (size_t) (dim + 7) / 8;
    // scratch: [fp32 queries of a host call | bit queries | stage-1 keys | stage-1 block ids, then the re-rank keys | doc | dist | counts]
    // (nobody reads stage 1's id columns: the re-rank keys take the block ids' place once stage 1 has run)
    const size_t o_q = 0, o_qb = align_up(o_q + (h_queries ? (size_t) nq * dim * sizeof(float) : 0), 256),
                 o_key = align_up(o_qb + (size_t) nq * qbytes, 256), o_blk = align_up(o_key + ns * 8, 256),
                 o_doc = align_up(o_blk + ns * 8, 256), o_dist = align_up(o_doc + ns * 4, 256),
                 o_cnt = align_up(o_dist + ns * 4, 256), total = align_up(o_cnt + (size_t) nq * 4, 256);
    RCCHK(ctx->d_short.reserve(total));
    char* w = ctx->d_short.as<char>();
    if (h_queries) {
        HIPCHK(hipMemcpyAsync(w + o_q, h_queries, (size_t) nq * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        d_queries = reinterpret_cast<const float*>(w + o_q);
    }
    uint8_t* d_qb = reinterpret_cast<uint8_t*>(w + o_qb);
    uint64_t* s1_keys = reinterpret_cast<uint64_t*>(w + o_key);
    HIPCHK(launch_binary_quantize(d_queries, 0, (uint64_t) nq, (uint32_t) dim, (uint32_t) dim, d_qb, (uint32_t) qbytes, ctx->stream));
    const Outputs s1{reinterpret_cast<int64_t*>(w + o_blk), reinterpret_cast<int32_t*>(w + o_doc), nullptr,
                     reinterpret_cast<float*>(w + o_dist), reinterpret_cast<int32_t*>(w + o_cnt), s1_keys};
    RCCHK(search_impl(ctx, bits, {nullptr, d_qb, nq, dim, shortlist, VSR_METRIC_HAMMING, s1}, filters, 2));
    return quantized_rerank(ctx, src, s1_keys, (uint32_t) bits->row_offset, reinterpret_cast<uint64_t*>(w + o_blk), d_queries, nq, dim, k,
                            shortlist, metric, out);
}

// Stage 2 of a two-stage search, whoever made the shortlist (K1b here, the bit graph in vsr_hnsw_rt.hip): the re-rank and emit
// launches of vsr_shortlist.h on ctx->stream.  s1_keys: [nq][shortlist] stage-1 keys, ascending with KEY_EMPTY last, whose rows carry
// s1_row_offset; rr_keys: [nq][shortlist] scratch; d_queries: the fp32 queries in device memory.
int vsr::quantized_rerank(vsr_ctx* ctx, vsr_corpus* src, const uint64_t* s1_keys, uint32_t s1_row_offset, uint64_t* rr_keys,
                          const float* d_queries, int nq, int dim, int k, int shortlist, int metric, const Outputs& out)
{
    ShortlistParams sl{};
    sl.s1_keys = s1_keys;
    sl.shortlist = (uint32_t) shortlist;
    sl.s1_row_offset = s1_row_offset;
    sl.q_src = d_queries;
    sl.dim = (uint32_t) dim;
    sl.rows = src->d_rows;
    sl.stride4 = src->stride4;
    sl.n_rows = (uint32_t) src->n;
    sl.metric = metric;
    sl.rr_keys = rr_keys;
    sl.err = ctx->err_word();
    sl.k = (uint32_t) k;
    sl.row_offset = (uint32_t) src->row_offset;
    sl.block_ids = src->d_block;
    sl.doc_ids = src->d_doc;
    sl.orig_rows = src->d_orig;
    sl.out_block = out.blk;
    sl.out_doc = out.doc;
    sl.out_row = out.row;
    sl.out_dist = out.dist;
    sl.out_keys = out.keys;
    sl.out_count = out.cnt;
    Timed rerank(ctx, 2, ctx->stream);                      // counted with the selections
    HIPCHK(launch_shortlist_rerank(sl, src->format, (uint32_t) nq, ctx->stream));
    HIPCHK(launch_shortlist_emit(sl, (uint32_t) nq, ctx->stream));
    HIPCHK(rerank.stop());
    ctx->last_kernel += " + shortlist re-rank";
    return VSR_OK;
}

extern "C" int vsr_search_quantized_device_on(vsr_ctx* session, vsr_corpus* src, vsr_corpus* bits, const float* d_queries, int nq,
                                              int dim, int k, int shortlist, int metric, const vsr_filter* const* filters,
                                              int64_t* d_blk, int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt,
                                              uint64_t* d_keys)
{
    const char* who = "vsr_search_quantized_device";
    int rc = check_quantized_args(session, src, bits, d_queries, nq, dim, k, shortlist, metric, filters, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!d_blk || !d_dist || !d_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    vsr_ctx* ctx = session ? session : bits->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    return search_quantized_impl(ctx, src, bits, nullptr, d_queries, nq, dim, k, shortlist, metric, filters,
                                 {d_blk, d_doc, d_row, d_dist, d_cnt, d_keys});
}

extern "C" int vsr_search_quantized_device(vsr_corpus* src, vsr_corpus* bits, const float* d_queries, int nq, int dim, int k,
                                           int shortlist, int metric, const vsr_filter* const* filters, int64_t* d_blk,
                                           int32_t* d_doc, int64_t* d_row, float* d_dist, int32_t* d_cnt, uint64_t* d_keys)
{
    return vsr_search_quantized_device_on(nullptr, src, bits, d_queries, nq, dim, k, shortlist, metric, filters, d_blk, d_doc, d_row,
                                          d_dist, d_cnt, d_keys);
}

extern "C" int vsr_search_quantized(vsr_corpus* src, vsr_corpus* bits, const float* queries, int nq, int dim, int k, int shortlist,
                                    int metric, const vsr_filter* const* filters, int64_t* out_blk, int32_t* out_doc,
                                    int64_t* out_row, float* out_dist, int32_t* out_cnt)
{
    const char* who = "vsr_search_quantized";
    int rc = check_quantized_args(nullptr, src, bits, queries, nq, dim, k, shortlist, metric, filters, who);
    if (rc) return rc;
    if (nq == 0) return VSR_OK;
    if (!out_blk || !out_dist || !out_cnt) return fail(VSR_ERR_INVALID, "%s: output is NULL", who);
    if (src->format == RowFormat::HALF && (rc = half_query_range(queries, nq, dim))) return rc;   // `$1::halfvec`, as vsr_search refuses it
    vsr_ctx* ctx = bits->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const ResultBlock rb(nq, k, false);                     // results in device memory, one packed copy back, one wait
    if ((rc = ctx->d_out.reserve(rb.o_status))) return rc;
    if ((rc = ctx->h_out.reserve(rb.total))) return rc;
    char* d = ctx->d_out.as<char>();
    char* h = ctx->h_out.as<char>();
    if ((rc = search_quantized_impl(ctx, src, bits, queries, nullptr, nq, dim, k, shortlist, metric, filters, rb.arrays(d)))) return rc;
    HIPCHK(hipMemcpyAsync(h, d, rb.o_status, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rb.copy_out_all(h, {out_blk, out_doc, out_row, out_dist, out_cnt, nullptr}, nullptr);
    return VSR_OK;
}
