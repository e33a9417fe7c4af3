// vsr_plan.hip — the batch planner: queries -> passes over filter parts -> workgroups (vsr_plan.h).
// On purpose this unit makes NO HIP runtime call and includes no kernel header.  It reads the context's knobs, the corpus's
// shape facts and the filters' row counts and device pointers (as opaque values), takes the capacity formulas from
// vsr_device.h, and writes a Plan: plain host arithmetic, so a plan can be reasoned about -- or unit-tested -- without a GPU.
// It runs once per batch on the critical path of a sub-millisecond step: the scratch vectors live in one thread-local
// PlanScratch and keep their capacity, so a warm planner allocates nothing.
#include "vsr_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace {

struct PlanIn {                              // what one make_plan call is asked
    const vsr_ctx*           ctx;
    const vsr_corpus*        c;
    int                      nq, k, metric;
    const vsr_filter* const* filters;
    bool                     thin_sample;    // make_plan's first attempt: an int8 class-view plan may sample at VIEW_SAMPLE_STRIDE
    const vsr_filter* filter(uint32_t q) const { return filters ? filters[q] : nullptr; }
};

// The sample stride of int8 class-view plans whose sample launch is K2r.  The context's stride (16) dates from plans that
// re-ranked every admitted row; on these plans a candidate costs an LDS park, a share of a column atomic and an 8-byte key,
// and the seed admits (kp f + 6 sqrt(kp f) + 4) / f rows per query: 404 at f = 1/16, 568 at 1/32, 836 at 1/64 (kp = 100).
// Measured on the headline step (profiles/r7): 32 beats 16 by more than the session's spread, 64 loses.
constexpr uint32_t VIEW_SAMPLE_STRIDE = 32;

struct PassItem { const vsr_filter* part; uint32_t slot; };     // part: atomic filter scanned (nullptr = whole corpus)
struct Pass {
    const vsr_filter* f; uint32_t q_off, q_count; int64_t rows; uint32_t n_tiles; int64_t cost;
    const uint2* vtiles;                     // class view: the class's slice of the view's tile list (nullptr: the part's own list)
};

constexpr uint32_t XCDS = 8;

struct PlanScratch {
    std::vector<PassItem> raw, items;        // (part, query) items in query order / grouped by part
    std::vector<uint32_t> gid;               // group of raw[i]
    std::vector<uint32_t> gend;              // per group: item count, then (after the scatter) the end offset of its items
    std::vector<const vsr_filter*> gpart;    // per group: its filter part
    std::vector<Pass>     passes;
    std::vector<uint32_t> loff, lcur, lids, lids_s, lcnt_s, level2;   // partial lists per query as CSR; K5 level-2 lists
    std::vector<double>   gdens_s;           // per sample group: permitted fraction of the rows its tiles cover
    std::vector<double>   est;               // per query: sample entries it can expect
    std::vector<uint2>    lane[XCDS];
};

struct Width {                               // what the kernel family and pass width stage decides
    bool     mq_ok, k2_ok, k2w_ok, k2g, i8wide;
    int      wq;                             // K2w / K2g: query columns of a workgroup
    int      qmax;                           // queries per pass
    uint32_t keep, keep_c;                   // screening survivors kept per query: fine planes, coarse planes
};

struct LaunchSize {
    int64_t  budget;                         // workgroups of the main launch, before the per-pass limits
    int64_t  total_cost;
    uint32_t seed_div;                       // the sample launch gets 1/seed_div of a pass's workgroups
};

// ---- stage 1: (filter part, query slot) items grouped by part ---------------------------------------------------
// A filter that is a union of permission classes (vsr_filter::parts) is scanned class by class, so that every query whose
// role sees a class shares that class's pass: the corpus is then read at most ceil(queries of the class / qmax) times per
// class instead of once per role partition.  Group ids in first-seen order, then a counting sort (stable, so the slots of
// a part stay ascending).  No comparison sort, no per-query allocation.  Returns the distinct parts' rows.
int64_t group_items(const PlanIn& in, PlanScratch& s)
{
    // plan marks live in the (shared) filters, so the epoch must be unique across host threads: a corpus handed from one
    // thread to another must never meet a stale mark that equals the new thread's counter
    static std::atomic<uint64_t> g_epoch{0};
    const uint64_t epoch = g_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
    s.raw.clear(); s.gid.clear(); s.gend.clear(); s.gpart.clear();
    const bool decompose = in.nq >= 32 && !in.ctx->no_classes;
    uint32_t null_group = 0xFFFFFFFFu;
    auto add = [&](const vsr_filter* f, uint32_t q) {
        uint32_t g;
        if (!f) {
            if (null_group == 0xFFFFFFFFu) {
                null_group = (uint32_t) s.gpart.size();
                s.gpart.push_back(nullptr);
                s.gend.push_back(0);
            }
            g = null_group;
        } else {
            if (f->plan_epoch != epoch) {
                f->plan_epoch = epoch;
                f->plan_group = (uint32_t) s.gpart.size();
                s.gpart.push_back(f);
                s.gend.push_back(0);
            }
            g = f->plan_group;
        }
        s.raw.push_back({f, q});
        s.gid.push_back(g);
        s.gend[g]++;
    };
    for (uint32_t q = 0; q < (uint32_t) in.nq; ++q) {
        const vsr_filter* f = in.filter(q);
        if (f && !f->parts.empty() && (decompose || f->parts_only))
            for (const vsr_filter* part : f->parts) add(part, q);
        else
            add(f, q);
    }
    uint32_t run = 0;
    for (auto& cnt : s.gend) { const uint32_t n = cnt; cnt = run; run += n; }     // counts -> start offsets
    s.items.resize(s.raw.size());
    for (size_t i = 0; i < s.raw.size(); ++i) s.items[s.gend[s.gid[i]]++] = s.raw[i];   // ... -> end offsets

    int64_t unique_rows = 0;
    for (const vsr_filter* part : s.gpart) unique_rows += part ? part->scanned_rows : in.c->n;
    return std::min<int64_t>(unique_rows, in.c->n);
}

// ---- stage 2: kernel family and pass width ----------------------------------------------------------------------
// Is the sum of num(cnt) over the parts at least nine tenths of the sum of den(cnt), cnt = a part's (part, query) items?
template <class Num, class Den> bool nine_tenths(const std::vector<uint32_t>& gend, Num num, Den den, bool if_none)
{
    uint64_t n = 0, d = 0;
    for (size_t g = 0; g < gend.size(); ++g) {
        const uint32_t cnt = gend[g] - (g ? gend[g - 1] : 0u);
        n += num(cnt);
        d += den(cnt);
    }
    return d ? n * 10 >= d * 9 : if_none;
}
// ... of all items, those in parts seen by more than `over` queries
bool mostly_in_parts_over(const std::vector<uint32_t>& gend, uint32_t over, bool if_none)
{
    return nine_tenths(gend, [over](uint32_t cnt) { return cnt > over ? cnt : 0u; }, [](uint32_t cnt) { return cnt; }, if_none);
}

Width choose_width(const PlanIn& in, const std::vector<uint32_t>& gend, bool allow_screening, bool allow_wide, bool allow_gemm)
{
    const vsr_ctx* ctx = in.ctx;
    const vsr_corpus* c = in.c;
    Width w{};
    // (a halfvec corpus has fp16 rows only: K1h or, under K2's gates, K2h -- K2 on the f16 matrix cores, vsr_mfmah.h; never
    // K1m, which reads fp32 rows, nor K2w / K2g / int8, which read planes it does not have)
    // (a bit corpus has packed bits only and an exact integer kernel, K1b: as with screening off, nothing else applies)
    // (a sparse corpus has CSR rows only and an exact kernel, K1s: planned like a bit corpus; the call's table size bounds the pass)
    const bool f32 = c->format == RowFormat::F32, half = c->format == RowFormat::HALF;
    w.mq_ok = f32 && mq_supported(c->dim) && mq_qmax(c->dim) >= 4 && !ctx->no_mq;
    // K2 / K2w: matrix-core screening keeps 2k (>= 32) candidates per query, K5r re-ranks them exactly
    w.keep = (uint32_t) std::max(2 * in.k, 32);
    const bool k2_any = (f32 || (half && !ctx->no_half_mfma)) && allow_screening && ctx->screening && c->k2_safe && in.metric != VSR_METRIC_L1 &&
                        mq_supported(c->dim) && ctx->max_qb >= 16;
    w.k2w_ok = k2_any && f32 && allow_wide && c->d_scr && w.keep <= GQ_MAX_KP && !ctx->no_wide && ctx->seeding;
    w.k2_ok = w.k2w_ok || (k2_any && mfma_cap_for_k(w.keep) <= 8192 && mfma_lds_bytes(c->stride4) <= 150 * 1024);
    w.wq = mfmaw_qmax(c->pstride4, !c->scr_has_mid);
    // K2g (coarse planes, 256-query passes): when nearly all (part, query) items sit in parts seen by more than 128
    // queries -- unfiltered batches, a few big partitions -- and the coarser screen's larger survivor list fits
    w.keep_c = (uint32_t) std::max(4 * in.k, 128);
    w.k2g = w.k2w_ok && allow_gemm && c->d_scr_c && !ctx->no_gemm && ctx->screen_level >= 2 && w.keep_c <= GQ_MAX_KP && !ctx->max_qb_set;
    w.k2g = w.k2g && mostly_in_parts_over(gend, 128, false);
    if (w.k2g) w.wq = (int) GM_QMAX;
    // int8 planes on K2i: every wave holds the B fragments of the whole pass, and 128 columns fit its registers -- a class seen
    // by 330 queries is streamed 3 times instead of 6.  The sample launch (K2w's kernel: 64 columns) gets such a pass as two.
    // (measured on the headline step: 12 % fewer pass rows, but the 8-group instantiation -- 223 VGPRs, its candidate masks
    // spilled to lanes -- is slower per row: 0.43 ms against 0.357 ms for 64-column passes.  Opt-in: VSR_K2I_WIDE=1.)
    w.i8wide = w.k2w_ok && !w.k2g && c->d_scr8 && in.metric == VSR_METRIC_L2 && ctx->int8_this_call && !ctx->no_k2i &&
               ctx->k2i_wide && c->shape.rw == 16 && !ctx->max_qb_set;
    if (w.i8wide) w.wq = 128;
    // long rows: 128-query passes (two groups per wave: a heavier kernel that also fetches the second group's fragments
    // where a pass has none) pay when nearly all (part, query) items sit in parts seen by more than 64 queries --
    // unfiltered batches: 1M x 768 x 1000 queries 9.9 -> 7.9 ms; a role mix (1000 users over 100 roles) would lose:
    // 1.10 -> 1.39 ms
    if (w.wq > 64 && !w.k2g && !w.i8wide && !mostly_in_parts_over(gend, 64, true)) w.wq = 64;
    const int legacy_qb = ctx->max_qb_set ? ctx->max_qb : 16;
    if (w.k2w_ok) w.qmax = ctx->max_qb_set ? std::min(ctx->max_qb, w.wq) : w.wq;
    else if (w.k2_ok) w.qmax = std::min(legacy_qb, mfma_qmax(c->stride4));
    else if (w.mq_ok) w.qmax = std::min(legacy_qb, mq_qmax(c->dim));
    else
        switch (c->format) {
        case RowFormat::SPARSE: w.qmax = std::min(legacy_qb, scan_qmax_sparse(ctx->sparse_slots, in.k)); break;
        default:                w.qmax = std::min(legacy_qb, scan_qmax(c->format, c->dim, in.k));
        }
    if (w.k2_ok && !w.k2w_ok && !ctx->max_qb_set && w.qmax >= 16 && c->stride4 > 64) {
        // long rows (d > 256): a pass costs mostly its row bytes, so two 16-query MFMA groups per pass (half the passes)
        // pay off -- but only when the query groups fill them (an unfiltered 1000-query batch: 17 % less time at
        // d = 768; role partitions with ~25 queries per class: 2.7x more, the second group would be mostly padding)
        const bool filled = nine_tenths(gend, [](uint32_t cnt) { return cnt; },                 // items per 32-query slots
                                        [](uint32_t cnt) { return (uint64_t) (cnt + 31) / 32 * 32; }, false);
        if (filled) w.qmax = std::min(32, mfma_qmax(c->stride4));
    }
    w.qmax = w.k2w_ok ? std::max(16, w.qmax / 16 * 16) : w.qmax >= 4 ? w.qmax / 4 * 4 : 1;
    return w;
}

// ---- stage 3: parts -> passes of at most qmax queries (their slots appended to q_slots); returns the widest's count ----
uint32_t cut_passes(const PlanIn& in, const Width& w, const std::vector<PassItem>& items, std::vector<Pass>& passes,
                    std::vector<uint32_t>& q_slots)
{
    const vsr_corpus* c = in.c;
    passes.clear();
    uint32_t widest = 1;
    for (size_t s = 0; s < items.size();) {
        size_t e = s;
        while (e < items.size() && items[e].part == items[s].part) ++e;
        const vsr_filter* f = items[s].part;
        // K2w: a part seen by more queries than one pass holds is cut into equal passes (330 queries -> 3 x 110, not
        // 128 + 128 + 74), each a whole number of 16-query MFMA groups
        size_t per = (size_t) w.qmax;
        if (w.k2w_ok && e - s > (size_t) w.qmax) {
            const size_t n_pass = (e - s + (size_t) w.qmax - 1) / (size_t) w.qmax;
            per = std::min<size_t>((size_t) w.qmax, ((e - s + n_pass - 1) / n_pass + 15) / 16 * 16);
        }
        for (size_t b = s; b < e;) {
            const uint32_t cnt = (uint32_t) std::min<size_t>(e - b, per);
            Pass pd;
            pd.f = f;
            pd.q_off = (uint32_t) q_slots.size();
            pd.q_count = cnt;
            pd.rows = f ? f->scanned_rows : c->n;
            pd.n_tiles = f ? f->n_tiles : (uint32_t) ((c->n + c->shape.rw - 1) / c->shape.rw);
            pd.vtiles = nullptr;
            // relative cost of a row of this pass: K2w passes are bound by the row stream up to ~3 query groups and by
            // the matrix pipe beyond (a 64-row tile costs 4 * groups * d/4 MFMAs), so fat passes get more workgroups
            const int64_t groups = (cnt + 15) / 16;
            pd.cost = std::max<int64_t>(pd.rows, 1) * (w.k2w_ok ? std::max<int64_t>(32, 10 * groups) : 32);
            for (uint32_t i = 0; i < cnt; ++i) q_slots.push_back(items[b + i].slot);
            passes.push_back(pd);
            widest = std::max(widest, cnt);
            b += cnt;
        }
        s = e;
    }
    return widest;
}

// one launch: the shared-pass kernels as soon as any pass carries more than one query
void set_family(const PlanIn& in, const Width& w, uint32_t widest, Plan& plan)
{
    plan.qi = widest > 1 ? 4 : 1;
    plan.qmax = plan.qi == 1 ? 1 : (widest + 3) / 4 * 4;
    plan.k2 = plan.qi == 4 && w.k2_ok;
    plan.k2w = plan.k2 && w.k2w_ok;
    plan.mq = plan.qi == 4 && w.mq_ok && !plan.k2;
    plan.keep = plan.k2 ? w.keep : (uint32_t) in.k;
    // K1s: a table that does not fit LDS beside one candidate list is read from global memory, and then qmax = QI
    plan.sparse_global = in.c->format == RowFormat::SPARSE && !scan_sparse_table_in_lds(in.ctx->sparse_slots, in.k);
    if (plan.k2w) plan.qmax = (uint32_t) w.wq;              // query slots per workgroup: one (long rows: two) 16-query groups per wave
    else if (plan.k2) plan.qmax = plan.qmax > 16 ? 32 : 16;
    plan.int8 = plan.k2w && in.c->d_scr8 && in.metric == VSR_METRIC_L2 && in.ctx->int8_this_call;
    if (plan.int8) plan.keep = (uint32_t) std::max(in.k, 32);  // exact screening: no second half of survivors to re-rank
    plan.k2g = plan.k2w && w.k2g && !plan.int8;
    if (plan.k2g) plan.keep = w.keep_c;                     // coarse screening: a wider survivor list for the exact re-rank
}

// ---- stage 3b: the class view ------------------------------------------------------------------------------------
// A call scans the corpus's class view (ClassView, vsr_runtime.h) when it screens on the int8 planes with K2w and EVERY pass's
// part is one whole permission class: a class filter of the corpus, or a role filter that sees a single class (RANGES, no
// bitmap, every scanned row permitted).  All or nothing: one unfiltered query, BITMAP part or ad-hoc filter and the call is
// planned on the base planes exactly as before.  A pass's tile list becomes its class's slice of the view's identity list,
// ceil(rows / 16) tiles without a dead slot except in the last; its rows -- and every count made of them -- stay rows.
bool take_class_view(const PlanIn& in, const Plan& plan, std::vector<Pass>& passes)
{
    const ClassView* v = in.c->class_view.get();
    if (!v || in.ctx->no_class_view || !plan.int8 || plan.k2g) return false;
    bool any = false;
    for (const Pass& p : passes) {
        const vsr_filter* f = p.f;
        if (f && f->scanned_rows == 0) continue;            // (a role that sees nothing: never launched)
        if (!f || f->view_class < 0 || (size_t) f->view_class >= v->rows.size() || f->mode != VSR_FILTER_RANGES || f->d_bitmap ||
            f->allowed_rows != f->scanned_rows || f->scanned_rows != (int64_t) v->rows[(size_t) f->view_class])
            return false;
        any = true;
    }
    if (!any) return false;
    for (Pass& p : passes) {
        if (!p.f || p.f->scanned_rows == 0) continue;
        const size_t cls = (size_t) p.f->view_class;
        p.vtiles = v->d_tiles + v->start[cls] / 16;
        p.n_tiles = (v->rows[cls] + 15) / 16;
    }
    return true;
}

// ---- stage 3c: walk alignment (WalkHint, vsr_device.h) -------------------------------------------------------------
// ONE canonical walk order: the passes of a class-view plan in ascending view position, so that every launch over a corpus
// visits the classes in the same order whichever query of the batch named a class first (cut_passes emits parts in first-seen
// order).  The passes of one class stay adjacent and in their order (q_off ascends with it).  Results do not depend on it.
#ifndef VSR_WALK_SLICES
#define VSR_WALK_SLICES 512        // slices of the view in a plan's walk table (2 KB of the staging block)
#endif
#ifndef VSR_WALK_LEAD
#define VSR_WALK_LEAD 8            // rows of 8 dispatch slots a launch starts ahead of (< 0: behind) the published position: the word is
#endif                             // a seed selection and a launch old when the first workgroups start.  Measured on the headline step
                                   // (profiles/r8): +8 beats 0 in five adjacent pairs of five, -8 equals 0; variant libraries only

bool takes_walk(const vsr_ctx* ctx, const Plan& plan)
{
    return plan.class_view && ctx->walk_align && !ctx->no_xcd_map && ctx->no_k2i && VSR_MW_DENSE;
}

void order_walk(const ClassView* v, std::vector<Pass>& passes)
{
    auto key = [v](const Pass& p) { return p.f && p.f->scanned_rows > 0 ? v->start[(size_t) p.f->view_class] : 0xFFFFFFFFu; };
    auto before = [&](const Pass& a, const Pass& b) { return key(a) != key(b) ? key(a) < key(b) : a.q_off < b.q_off; };
    if (!std::is_sorted(passes.begin(), passes.end(), before)) std::sort(passes.begin(), passes.end(), before);
}

// The table of a plan: slice s of the view (positions s << shift ..., a position = 64 rows) -> the first row of 8 dispatch
// slots at which the mapped launch has a workgroup reaching past the slice's first row.  A row in a class this batch does
// not scan maps to the next class it does scan; rows behind the last scanned class map to slot 0.
void build_walk_table(const ClassView* v, Plan& plan)
{
    plan.walk_n_pos = v->n_rows >> 6;
    plan.walk_shift = 0;
    while (((plan.walk_n_pos - 1) >> plan.walk_shift) + 1 > (uint32_t) VSR_WALK_SLICES) ++plan.walk_shift;
    const uint32_t n_slices = ((plan.walk_n_pos - 1) >> plan.walk_shift) + 1;
    plan.walk_table.assign(n_slices, 0u);
    const uint32_t n_t = plan.n_launch / XCDS;
    const uint32_t lead = (uint32_t) (((int64_t) VSR_WALK_LEAD % (int64_t) n_t + (int64_t) n_t) % (int64_t) n_t);
    uint64_t reach = 0;                                     // first view row no workgroup of slots [0, 8 t + 8) reaches
    for (uint32_t t = 0, s = 0; t < n_t && s < n_slices; ++t) {
        for (uint32_t l = 0; l < XCDS; ++l) {
            const uint2 m = plan.block_map[(size_t) t * XCDS + l];
            if (m.x == 0xFFFFFFFFu) continue;
            const ScanGroup& g = plan.groups[m.x];
            const uint64_t first = (uint64_t) (g.tiles - v->d_tiles) * 16;
            reach = std::max(reach, first + 16 * ((uint64_t) g.n_tiles * (m.y + 1) / g.n_blocks));
        }
        for (; s < n_slices && ((uint64_t) s << (plan.walk_shift + 6)) < reach; ++s) plan.walk_table[s] = (t + lead) % n_t * XCDS;
    }
}

// The stride the plan's sampling starts from: VIEW_SAMPLE_STRIDE for an int8 class-view plan that can sample on K2r (the
// first planning attempt only: make_plan), else the context's.  An explicit VSR_SAMPLE_STRIDE always wins.
uint32_t first_stride(const PlanIn& in, const Plan& plan)
{
    const vsr_ctx* ctx = in.ctx;
    const bool thin = in.thin_sample && !ctx->sample_stride_set && plan.int8 && plan.class_view && ctx->k2i_sample && ctx->sample_reg &&
                      in.c->shape.rw == 16 && ctx->sample_stride < VIEW_SAMPLE_STRIDE;
    return thin ? VIEW_SAMPLE_STRIDE : ctx->sample_stride;
}

// ---- stage 4: workgroups of the launch ---------------------------------------------------------------------------
// Workgroups per launch: 4 per CU (two resident at a time), and for big shared-pass launches one per ~13k scanned
// rows up to 16 per CU -- finer blocks even out the passes' very different lengths over the chip (10M rows, 1000
// queries: main launch alone 2.38 -> 2.12 ms with 8 per CU).  The sample launch then keeps ~2 workgroups per CU.
LaunchSize size_launch(const PlanIn& in, const Plan& plan, const std::vector<Pass>& passes)
{
    const vsr_ctx* ctx = in.ctx;
    int64_t total_rows = 0;
    LaunchSize ls{};
    for (auto& p : passes) {
        total_rows += std::max<int64_t>(p.rows, 1);
        ls.total_cost += p.cost;
    }
    const int64_t cus = ctx->prop.multiProcessorCount;
    // (one query per call: 2 per CU -- one resident round -- halves the lists the in-kernel merge tree has to combine:
    // 0.094 -> 0.079 ms per call on SIFT10M role partitions)
    ls.budget = ctx->block_budget > 0 ? ctx->block_budget : in.nq == 1 ? 2 * cus : 4 * cus;
    ls.seed_div = ctx->seed_block_div;
    if (ctx->block_budget <= 0 && plan.qi == 4) {
        // K2w keeps 3 workgroups per CU resident and its passes differ a lot in cost per row: ~4 rounds of workgroups
        // even them out (10M rows, 1000 queries: main launch alone 0.97 -> 0.75 ms from 4 to 12 per CU)
        // (K2g: one 8-wave workgroup per CU; ~3 rounds, at least ~8 of its 256-row tiles per workgroup)
        const int64_t want = plan.k2g ? std::min<int64_t>(total_rows / 2048, 3 * cus)
                           : plan.k2w ? std::min<int64_t>(total_rows / 4096, 12 * cus) : std::min<int64_t>(total_rows / 13000, 16 * cus);
        if (want > ls.budget) {
            ls.budget = want;
            ls.seed_div = std::max<uint32_t>(ls.seed_div, (uint32_t) (ls.budget / (2 * cus)));
        }
    }
    if (plan.k2w) {
        // the sample launch visits every ss-th tile: a workgroup of it is all prologue and memory latency, so it gets ONE
        // resident round of workgroups (each then walks ~12 tiles instead of three rounds walking 4: 72 -> ~45 us on the
        // 10M-row corpus); launches that fit one round anyway (a shard) keep the main launch's workgroups
        const int64_t slots = (plan.k2g ? 1 : plan.int8 ? 4 : 3) * cus * ctx->sample_rounds;   // (VSR_SAMPLE_ROUNDS: measurements only)
        ls.seed_div = (uint32_t) std::max<int64_t>(1, (ls.budget + slots - 1) / slots);
        // a thinner sample: fewer, not shorter, workgroups -- each still walks about as many stages of a longer range
        ls.seed_div = ls.seed_div * first_stride(in, plan) / ctx->sample_stride;
    }
    return ls;
}

// ---- stage 5: ScanGroups of the main and the sample launch; partial lists per query counted into loff[slot + 1] ----
void emit_groups(const PlanIn& in, bool i8wide, const LaunchSize& ls, PlanScratch& s, Plan& plan)
{
    const vsr_ctx* ctx = in.ctx;
    const vsr_corpus* c = in.c;
    s.gdens_s.clear();
    s.loff.assign((size_t) in.nq + 1, 0);
    for (auto& p : s.passes) {
        if (p.n_tiles == 0 || p.rows == 0) continue;       // empty filter part: nothing to scan
        int64_t nb = (int64_t) (((__int128) p.cost * ls.budget + ls.total_cost - 1) / ls.total_cost);
        const int64_t min_rows = p.q_count > 1 ? std::max<int64_t>(ctx->min_rows_per_block, ctx->min_shared_rows) : ctx->min_rows_per_block;
        nb = std::min<int64_t>(nb, std::max<int64_t>(1, p.rows / min_rows));   // shared passes need rows to prune on
        nb = std::min<int64_t>(nb, std::max<uint32_t>(1, p.n_tiles));
        nb = std::max<int64_t>(nb, 1);
        ScanGroup g;
        g.tiles = p.vtiles ? p.vtiles : p.f ? p.f->d_tiles : plan.k2w ? c->d_all_tiles : nullptr;
        g.bitmap = p.f ? p.f->d_bitmap : nullptr;
        g.n_tiles = p.n_tiles;
        g.q_begin = p.q_off;
        g.q_count = p.q_count;
        g.block_begin = plan.n_blocks;
        g.n_blocks = (uint32_t) nb;
        g.partial_begin = plan.n_partial;
        plan.groups.push_back(g);
        const double dens = p.f && p.f->scanned_rows > 0 ? (double) p.f->allowed_rows / (double) p.f->scanned_rows : 1.0;
        ScanGroup gs = g;                                   // the same pass in the sample launch (buffers alias:
        gs.n_blocks = (uint32_t) std::max<int64_t>(1, nb / ls.seed_div);      // it finishes before the main launch)
        gs.block_begin = plan.n_blocks_s;
        gs.partial_begin = plan.n_partial_s;
        if (i8wide && p.q_count > 64) {                     // a 128-column pass: two sample groups of at most 64 columns
            ScanGroup g1 = gs;
            g1.q_count = (p.q_count / 2 + 15) / 16 * 16;
            plan.groups_s.push_back(g1);
            s.gdens_s.push_back(dens);
            plan.n_blocks_s += g1.n_blocks;
            plan.n_partial_s += g1.n_blocks * g1.q_count;
            gs.q_begin += g1.q_count;
            gs.q_count = p.q_count - g1.q_count;
            gs.block_begin = plan.n_blocks_s;
            gs.partial_begin = plan.n_partial_s;
            plan.n_partial_s -= gs.n_blocks * p.q_count - gs.n_blocks * gs.q_count;   // (the common accounting below adds the whole pass)
        }
        plan.groups_s.push_back(gs);
        s.gdens_s.push_back(dens);
        for (uint32_t qi = 0; qi < p.q_count; ++qi) s.loff[plan.q_slots[p.q_off + qi] + 1] += g.n_blocks;
        plan.n_blocks += g.n_blocks;
        plan.n_partial += g.n_blocks * p.q_count;
        plan.n_blocks_s += gs.n_blocks;
        plan.n_partial_s += gs.n_blocks * p.q_count;
        plan.scan_rows += p.rows;
        plan.scan_pairs += p.rows * (int64_t) p.q_count;
        // (sparse corpus: 8 bytes per stored entry -- a filter part's rows at the corpus's mean entry count)
        const int64_t rows_bytes = c->format == RowFormat::SPARSE
                                       ? (int64_t) ((__int128) p.rows * (__int128) c->sp_entries * 8 / std::max<int64_t>(c->n, 1))
                                       : p.rows * format_row_bytes(c->format, c->dim);
        plan.scan_bytes += rows_bytes + (g.bitmap ? (p.rows + 7) / 8 : 0) + (int64_t) p.q_count * in.k * 12 +
                           (plan.k2 ? p.rows * 4 : 0);     // K2 also reads |row|^2
    }
    plan.n_scan_lists = plan.n_partial;
    plan.n_launch = plan.n_blocks;
}

// ---- stage 6: XCD-aware workgroup order -------------------------------------------------------------------------
// Consecutive passes over the same rows (one permission class scanned for several query groups) are split into the same
// block ranges; block j of all of them forms a bundle that should run on ONE XCD at the same time, so that the rows are
// fetched over the fabric once and re-read from that XCD's L2.  Workgroups are dealt round-robin over the 8 XCDs
// (id % 8 = one XCD, MI355X_MICROARCH.md): lane l owns the ids l, l+8, l+16, ...; every bundle is appended whole to the
// currently shortest lane.
void map_blocks_to_xcds(std::vector<uint2> (&lane)[XCDS], Plan& plan)
{
    for (auto& l : lane) l.clear();
    size_t gi = 0;
    while (gi < plan.groups.size()) {
        size_t ge = gi + 1;
        while (ge < plan.groups.size() && plan.groups[ge].tiles == plan.groups[gi].tiles &&
               plan.groups[ge].bitmap == plan.groups[gi].bitmap && plan.groups[ge].n_tiles == plan.groups[gi].n_tiles &&
               plan.groups[ge].n_blocks == plan.groups[gi].n_blocks)
            ++ge;
        for (uint32_t j = 0; j < plan.groups[gi].n_blocks; ++j) {
            uint32_t best = 0;
            for (uint32_t l = 1; l < XCDS; ++l)
                if (lane[l].size() < lane[best].size()) best = l;
            for (size_t g2 = gi; g2 < ge; ++g2) lane[best].push_back(make_uint2((uint32_t) g2, j));
        }
        gi = ge;
    }
    size_t longest = 0;
    for (auto& l : lane) longest = std::max(longest, l.size());
    plan.block_map.assign(longest * XCDS, make_uint2(0xFFFFFFFFu, 0u));
    for (uint32_t l = 0; l < XCDS; ++l)
        for (size_t t = 0; t < lane[l].size(); ++t) plan.block_map[t * XCDS + l] = lane[l][t];
    plan.n_launch = (uint32_t) plan.block_map.size();
}

// ---- stage 7: K2w / K2g / K2i sampling and seed rank ------------------------------------------------------------
// of the t tiles of `tile_rows` rows in a group: those a launch samples whose workgroups visit every ss-th tile of theirs
double sampled_tiles(const ScanGroup& g, int rw, double tile_rows, double ss, double& t)
{
    t = std::ceil((double) g.n_tiles * rw / tile_rows);
    const double per_block = std::ceil(t / g.n_blocks);
    return std::min(t, g.n_blocks * std::ceil(per_block / ss));
}

// the sampling fraction of the most densely sampled group (>= 1 / ss: every workgroup samples at least one tile)
double densest_fraction(const std::vector<ScanGroup>& groups, int rw, double tile_rows, double ss)
{
    double frac = 1.0 / ss;
    for (const ScanGroup& g : groups) {
        double t;
        const double sampled = sampled_tiles(g, rw, tile_rows, ss, t);
        if (t > 0) frac = std::max(frac, sampled / t);
    }
    return frac;
}

// The int8 sample pass as per-wave streams (vsr_i8s.h, SAMPLE): stages of 32 rows, every ss-th stage of a workgroup's
// range; each of the <= 4 waves that get a stage keeps 4 lanes' minima per query column over its whole stream.
// Fewer entries than K2w's per-tile minima, so the plan takes it only when every query's sample stays thick enough.
bool try_k2i_sample(const PlanIn& in, PlanScratch& s, Plan& plan)
{
    const vsr_corpus* c = in.c;
    const uint32_t stride = first_stride(in, plan);
    const double ss = stride;
    const double frac = densest_fraction(plan.groups_s, c->shape.rw, 32.0, ss);
    const uint32_t seed_m = seed_rank(plan.keep, frac);
    s.est.assign((size_t) in.nq, 0.0);
    for (size_t gi = 0; gi < plan.groups_s.size(); ++gi) {
        const ScanGroup& gs = plan.groups_s[gi];
        const double t32 = std::ceil((double) gs.n_tiles * c->shape.rw / 32.0);
        const double per_block = std::floor(t32 / gs.n_blocks);                  // (the shortest block of the group)
        const double st = std::max(1.0, std::ceil(per_block / ss));              // stages a workgroup samples
        const double waves = std::min(4.0, st);
        const double rows_per_entry = st / waves * 8.0;                          // 2 row blocks x 4 rows per lane and stage
        const double p_entry = std::min(1.0, s.gdens_s[gi] * rows_per_entry);
        for (uint32_t qi = 0; qi < gs.q_count; ++qi) s.est[plan.q_slots[gs.q_begin + qi]] += gs.n_blocks * waves * 4.0 * p_entry;
    }
    bool thick = seed_m <= GQ_SAMPLE_CAP / 4;
    for (uint32_t q = 0; q < (uint32_t) in.nq && thick; ++q) {
        const vsr_filter* f = in.filter(q);
        if (allowed_rows(c, f) > (int64_t) GQ_CAP && s.est[q] < (exact_count(f) ? 1.5 * seed_m + 16.0 : 2.5 * seed_m)) thick = false;
    }
    if (!thick) return false;
    plan.k2i_sample = true;
    plan.sample_stride = stride;
    plan.kp_frac = (float) seed_lambda(plan.keep, frac);
    for (ScanGroup& gs : plan.groups_s) gs.partial_begin = 0u;
    return true;
}

// The K2w / K2g sample launch at `stride`: sets the plan's stride and seed fraction and the sample groups' `fine` flags.
// Returns whether every query that needs a seed can get one; soft_thin: some query that fits its candidate buffer, but
// has more than a few thousand rows, would run with an open threshold.
bool evaluate_stride(const PlanIn& in, uint32_t stride, PlanScratch& s, Plan& plan, bool& soft_thin)
{
    const vsr_corpus* c = in.c;
    const double tile_rows = plan.k2g ? 256.0 : 64.0;       // rows per workgroup tile of the kernel
    plan.sample_stride = stride;
    const double ss = stride;
    const double frac = densest_fraction(plan.groups_s, c->shape.rw, tile_rows, ss);
    const uint32_t seed_m = seed_rank(plan.keep, frac);
    plan.kp_frac = (float) seed_lambda(plan.keep, frac);
    bool good = seed_m <= GQ_SAMPLE_CAP / 4;
    // fine passes: any query whose per-column minima (one per 64 rows of a sampled tile; K2g: one per 128) would be
    // fewer than 4 m: one minimum per lane instead (4 x as many)
    s.est.assign((size_t) in.nq, 0.0);
    for (size_t gi = 0; gi < plan.groups_s.size(); ++gi) {
        ScanGroup& gs = plan.groups_s[gi];
        bool fine = false;
        for (uint32_t qi = 0; qi < gs.q_count; ++qi) {
            const double allowed = (double) allowed_rows(c, in.filter(plan.q_slots[gs.q_begin + qi]));
            fine |= allowed / ((plan.k2g ? 128.0 : 64.0) * ss) < 4.0 * seed_m;
        }
        gs.partial_begin = fine ? 1u : 0u;                     // (K2w / K2g have no partial lists: the field carries the flag)
        double t64;
        const double sampled = sampled_tiles(gs, c->shape.rw, tile_rows, ss, t64);
        const uint32_t ngt = (gs.q_count + 15) / 16;
        const double waves_per_col = plan.k2g ? 2.0 : ngt == 1 ? 4.0 : ngt == 2 ? 2.0 : 1.0;     // row split (vsr_mfmaw.h)
        const double entries_per_tile = waves_per_col * (fine ? 4.0 : 1.0);
        const double rows_per_entry = tile_rows / entries_per_tile;
        const double p_entry = std::min(1.0, s.gdens_s[gi] * rows_per_entry);    // a bitmap may leave an entry without rows
        for (uint32_t qi = 0; qi < gs.q_count; ++qi) s.est[plan.q_slots[gs.q_begin + qi]] += sampled * entries_per_tile * p_entry;
    }
    soft_thin = false;
    for (uint32_t q = 0; q < (uint32_t) in.nq; ++q) {
        const vsr_filter* f = in.filter(q);
        const int64_t allowed = allowed_rows(c, f);
        // the sample must be thick enough to reach rank m (with a margin where a bitmap makes the count random),
        // unless all of the query's rows fit its buffer anyway
        const bool thin = s.est[q] < (exact_count(f) ? 1.25 * seed_m + 8.0 : 2.0 * seed_m);
        if (allowed > (int64_t) GQ_CAP && thin) good = false;
        if (allowed > (int64_t) (8 * plan.keep) && allowed > 2048 && thin) soft_thin = true;
    }
    return good;
}

// K2w keeps one candidate buffer per query: no partial lists, no K5 items.  What the plan still owes is the
// threshold seeding.  The sample launch runs the same workgroups over every ss-th tile of theirs (at least one
// each), so every pass is sampled at a fraction f >= 1/ss of its rows, and keeps per query only minima: one
// entry per query column and wave-tile, or one per lane where a query's sample would otherwise be too thin
// (`fine` passes).  The seed is the m-th smallest entry of a query (seed_rank) for the most densely sampled pass,
// so it ranks behind the kp-th row and admits about m / f rows of the query:
// kp + 6 sqrt(kp / f) + 4 / f (~600 at f = 1/16, kp = 200).  Dropping sample entries (minima, buffer
// overflow) can only raise the m-th smallest, i.e. loosen the seed.  A query whose sample cannot reach rank m
// gets an open threshold; that is only safe when all of its rows fit its candidate buffer (GQ_CAP).
// Returns false when some query can get neither.
bool plan_wide_sampling(const PlanIn& in, PlanScratch& s, Plan& plan)
{
    bool ok = plan.int8 && in.ctx->k2i_sample && in.c->shape.rw == 16 && try_k2i_sample(in, s, plan);
    // (the thinner sample of a class-view plan is K2r's or nobody's: make_plan plans the call again at the context's stride)
    if (!ok && first_stride(in, plan) != in.ctx->sample_stride) return false;
    // A sample too thin for some query at the configured stride is taken more densely (8, 4, 2) before the plan is given up:
    // K2g's 256-row tiles on a small corpus, and K2w over many small parts (IVFFlat lists: probes x ~1000 rows per query
    // used to fall back to the legacy kernels as soon as one query's lists added up to more than its candidate buffer).
    // Among the strides that make a valid plan the first one is preferred that also seeds every query with more than a
    // few thousand rows: a query that fits its buffer may run with an open threshold, but then EVERY one of its rows is a
    // candidate (IVFFlat, 4 probes of ~1000 rows: 4000 appended keys per query, slower than 10 probes with seeds).
    uint32_t first_ok = 0, chosen = 0;
    for (uint32_t stride = in.ctx->sample_stride; !ok && !chosen && stride >= 2; stride /= 2) {
        bool soft = false;
        if (evaluate_stride(in, stride, s, plan, soft)) {
            if (!first_ok) first_ok = stride;
            if (!soft) chosen = stride;
        }
    }
    if (!ok && (chosen || first_ok)) {
        bool soft = false;
        ok = evaluate_stride(in, chosen ? chosen : first_ok, s, plan, soft);   // (leaves the plan at that stride)
    }
    plan.selq.resize((size_t) in.nq);
    for (uint32_t q = 0; q < (uint32_t) in.nq; ++q) {
        SelectQuery sq;
        sq.ids_begin = 0;
        sq.n_lists = 0;
        sq.out_slot = q;
        sq.dst_list = SEL_FINAL;
        sq.allowed = (uint32_t) std::min<int64_t>(allowed_rows(in.c, in.filter(q)), 0xFFFFFFFFll);
        sq.pad = 0;
        plan.selq[q] = sq;
    }
    return ok;
}

// ---- stage 8: partial lists per query (CSR) and K5 select items -------------------------------------------------
void build_select_items(const PlanIn& in, uint32_t seed_div, PlanScratch& s, Plan& plan)
{
    const int nq = in.nq;
    auto &loff = s.loff, &lcur = s.lcur, &lids = s.lids, &lids_s = s.lids_s, &lcnt_s = s.lcnt_s, &level2 = s.level2;
    for (int q = 0; q < nq; ++q) loff[(size_t) q + 1] += loff[(size_t) q];
    lcur.assign(loff.begin(), loff.end() - 1);
    lids.resize(loff[(size_t) nq]);
    const bool same_blocks = seed_div == 1;                // sample lists mirror the main lists one to one
    if (!same_blocks) lids_s.resize(loff[(size_t) nq]);
    lcnt_s.assign((size_t) nq, 0);
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const ScanGroup& g = plan.groups[gi];
        const ScanGroup& gs = plan.groups_s[gi];
        for (uint32_t qi = 0; qi < g.q_count; ++qi) {
            const uint32_t slot = plan.q_slots[g.q_begin + qi];
            uint32_t at = lcur[slot];
            for (uint32_t b = 0; b < g.n_blocks; ++b) lids[at + b] = g.partial_begin + qi * g.n_blocks + b;
            if (!same_blocks) {
                // the sample pass has at most as many lists: kept left-packed in the same CSR range
                uint32_t as = loff[slot] + lcnt_s[slot];
                for (uint32_t b = 0; b < gs.n_blocks; ++b) lids_s[as + b] = gs.partial_begin + qi * gs.n_blocks + b;
                lcnt_s[slot] += gs.n_blocks;
            }
            lcur[slot] = at + g.n_blocks;
        }
    }

    // K5 items.  Queries with many partial lists get a first level of fan-in-list merges.  When every query fits two
    // levels of the wave-per-query selection (<= 4096 keys per item) that kernel and its smaller fan-in are used.
    uint32_t most_lists = 0;
    for (int q = 0; q < nq; ++q) most_lists = std::max(most_lists, loff[(size_t) q + 1] - loff[(size_t) q]);
    const uint32_t wave_fanin = select_wave_fanin(plan.keep);
    plan.sel_wave = wave_fanin > 0 && (uint64_t) most_lists <= (uint64_t) wave_fanin * wave_fanin;
    const uint32_t fanin = plan.sel_wave ? wave_fanin : SEL_FANIN;
    plan.selq.resize((size_t) nq);
    plan.seedq.resize((size_t) nq);
    plan.list_ids.reserve(lids.size() * 2 + 64);
    for (uint32_t q = 0; q < (uint32_t) nq; ++q) {
        const uint32_t allowed = (uint32_t) std::min<int64_t>(allowed_rows(in.c, in.filter(q)), 0xFFFFFFFFll);
        const uint32_t* ls = lids.data() + loff[q];
        uint32_t n_ls = loff[q + 1] - loff[q];
        if (n_ls > fanin) {
            level2.clear();
            for (uint32_t j = 0; j < n_ls; j += fanin) {
                SelectQuery s1;
                s1.ids_begin = (uint32_t) plan.list_ids.size();
                s1.n_lists = std::min<uint32_t>(fanin, n_ls - j);
                s1.out_slot = 0;
                s1.dst_list = plan.n_partial;
                s1.allowed = 0;
                s1.pad = 0;
                plan.list_ids.insert(plan.list_ids.end(), ls + j, ls + j + s1.n_lists);
                plan.sel1.push_back(s1);
                level2.push_back(plan.n_partial++);
            }
            ls = level2.data();
            n_ls = (uint32_t) level2.size();
        }
        SelectQuery sq;
        sq.ids_begin = (uint32_t) plan.list_ids.size();
        sq.n_lists = n_ls;
        sq.out_slot = q;
        sq.dst_list = SEL_FINAL;
        sq.allowed = allowed;
        sq.pad = 0;
        plan.list_ids.insert(plan.list_ids.end(), ls, ls + n_ls);
        plan.selq[q] = sq;
        SelectQuery sd = sq;                                // seed item: the sample pass's lists of the same query
        sd.ids_begin = (uint32_t) plan.list_ids.size();
        sd.dst_list = SEL_SEED;
        const uint32_t* sl = same_blocks ? lids.data() + loff[q] : lids_s.data() + loff[q];
        sd.n_lists = same_blocks ? loff[q + 1] - loff[q] : lcnt_s[q];     // same_blocks: identical list numbering
        if (plan.sel_wave && sd.n_lists > 64) sd.n_lists = 64;            // a subset of the sample only loosens the seed
        plan.list_ids.insert(plan.list_ids.end(), sl, sl + sd.n_lists);
        plan.seedq[q] = sd;
    }
    if (plan.k2) {          // the final K5 of every query writes its kp screening survivors as list rerank_base + slot
        plan.rerank_base = plan.n_partial;
        for (size_t i = 0; i < plan.selq.size(); ++i) plan.selq[i].dst_list = plan.rerank_base + (uint32_t) i;
        plan.n_partial += (uint32_t) plan.selq.size();
    }
}

}  // namespace

uint32_t vsr::seed_rank(uint32_t kp, double frac)
{
    const double lambda = seed_lambda(kp, frac);
    return (uint32_t) std::ceil(lambda + 6.0 * std::sqrt(lambda)) + 4;
}

bool vsr::make_plan(const vsr_ctx* ctx, const vsr_corpus* c, int nq, int k, int metric, bool allow_screening, bool allow_wide,
                    bool allow_gemm, const vsr_filter* const* filters, Plan& plan)
{
    static thread_local PlanScratch s;
    // An int8 class-view plan is first planned with the thinner sample (VIEW_SAMPLE_STRIDE: sample workgroups and seed rank
    // follow from the stride, so the whole plan does).  It stands when everything that protects a seed holds at that stride --
    // try_k2i_sample's thickness and buffer-capacity checks for every query, K2r as the sample kernel -- and the main launch
    // keeps the mask epilogue under the looser seeds.  Otherwise (a query whose sample gets too thin, a small corpus) the call
    // is planned again exactly as before: the context's stride, stepped down by plan_wide_sampling until the checks hold.
    for (int attempt = 0; attempt < 2; ++attempt) {
        const PlanIn in{ctx, c, nq, k, metric, filters, attempt == 0};
        plan.reset();
        plan.unique_rows = group_items(in, s);
        const Width w = choose_width(in, s.gend, allow_screening, allow_wide, allow_gemm);
        const uint32_t widest = cut_passes(in, w, s.items, s.passes, plan.q_slots);
        set_family(in, w, widest, plan);
        plan.class_view = take_class_view(in, plan, s.passes);
        plan.walk = takes_walk(ctx, plan);
        if (plan.walk) order_walk(c->class_view.get(), s.passes);
        const bool thin = first_stride(in, plan) != ctx->sample_stride;
        const LaunchSize ls = size_launch(in, plan, s.passes);
        emit_groups(in, w.i8wide, ls, s, plan);
        if (plan.k2 || plan.mq) map_blocks_to_xcds(s.lane, plan);
        plan.walk = plan.walk && !plan.block_map.empty();
        if (plan.walk) build_walk_table(c->class_view.get(), plan);
        if (plan.k2w) {
            const bool ok = plan_wide_sampling(in, s, plan);
            plan.k2r_sample = ok && plan.class_view && plan.k2i_sample && ctx->sample_reg;   // same geometry, same entries (vsr_i8r.h)
            if (thin && !(plan.k2r_sample && survivors_per_wave_tile(plan, nq) <= MASK_EPI_SURVIVORS)) continue;
            return ok;
        }
        build_select_items(in, ls.seed_div, s, plan);
        return true;
    }
    return false;                                              // (not reached: the second attempt never samples thin)
}

std::string vsr::scan_kernel_name(const Plan& plan, const vsr_corpus* c, int metric, bool k2i)
{
    static const char* mname[] = {"L2", "IP", "COSINE", "L1", "HAMMING", "JACCARD"};
    char buf[160];
    const uint32_t nstage = (c->stride4 + 15) / 16;
    if (plan.k2g)
        snprintf(buf, sizeof buf, "vsr::gemm_screen_kernel<%s, SAMPLE=false> (K2g, bf16 coarse planes)", mname[metric]);
    else if (plan.k2w && plan.int8 && k2i)
        snprintf(buf, sizeof buf, "vsr::i8_stream_kernel<NQG=4> (K2i, int8 planes, %s)", mname[metric]);
    else if (plan.k2w && plan.int8)
        snprintf(buf, sizeof buf, "vsr::mfma_wide_kernel<%s, NCH=1, SAMPLE=false, PL=int8> (K2w, int8 planes)", mname[metric]);
    else if (plan.k2w)
        snprintf(buf, sizeof buf, "vsr::mfma_wide_kernel<%s, NCH=%u, SAMPLE=false, HO=%s> (K2w, bf16 %s planes)", mname[metric],
                 c->pstride4 / 16, c->scr_has_mid ? "false" : "true", c->scr_has_mid ? "hi+mid" : "hi-only");
    else if (plan.k2 && c->format == RowFormat::HALF) {
        const uint32_t hstage = (c->stride4 / 2 + 15) / 16;    // launch_mfmah_metric's choice
        const int ng = plan.qmax > 16 ? 2 : 1;
        snprintf(buf, sizeof buf, "vsr::mfmah_scan_kernel<%s, NSTR=%u, SAMPLE=false, NG=%d> (K2h, half rows)", mname[metric],
                 hstage <= 2 ? hstage : hstage <= 4 && ng == 1 ? 4u : 0u, ng);
    } else if (plan.k2)
        snprintf(buf, sizeof buf, "vsr::mfma_scan_kernel<%s, NSTR=%d, SAMPLE=false, NG=%d> (K2)", mname[metric],
                 nstage > 4 ? 0 : 4, plan.qmax > 16 ? 2 : 1);
    else if (plan.mq)
        snprintf(buf, sizeof buf, "vsr::mq_scan_kernel<%s, SAMPLE=false> (K1m)", mname[metric]);
    else
        switch (c->format) {
        case RowFormat::SPARSE:
            snprintf(buf, sizeof buf, "vsr::scans_kernel<%s, LPR=%d, QI=%d, TAB=%s> (K1s, sparse rows)", mname[metric], c->shape.lpr, plan.qi,
                     plan.sparse_global ? "global" : "lds");
            break;
        case RowFormat::BIT:
            snprintf(buf, sizeof buf, "vsr::scanb_kernel<%s, LPR=%d, C=%d, R=%d, QI=%d> (K1b, bit rows)", mname[metric], c->shape.lpr,
                     c->shape.c, c->shape.r, plan.qi);
            break;
        default:
            snprintf(buf, sizeof buf, "vsr::scan_kernel<%s, LPR=%d, C=%d, R=%d, QI=%d%s", mname[metric], c->shape.lpr, c->shape.c,
                     c->shape.r, plan.qi, c->format == RowFormat::HALF ? ", HALF=true> (K1h, half rows)" : "> (K1)");
        }
    std::string name = buf;
    if (plan.class_view) name.insert(name.rfind(')'), ", class view");
    if (plan.walk) name.insert(name.rfind(')'), ", walk-aligned over " + std::to_string(plan.n_launch) + " slots");
    return name;
}
