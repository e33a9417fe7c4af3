// vsr_plan.h — the plan of one search batch: which passes scan which filter parts for which queries, on which kernel family,
// in how many workgroups, seeded and merged how.  Written by make_plan (vsr_plan.hip), read by vsr_search.hip.
#pragma once
#include <cmath>
#include "vsr_runtime.h"

namespace vsr {

constexpr uint32_t SEL_FANIN = 64;           // partial lists one K5 workgroup merges; more -> two levels

// Plan's plain fields.  Plan::reset() clears them all at once by assigning PlanScalars{}: a field added here starts
// every batch at its initialiser, whether or not anyone remembers reset().
struct PlanScalars {
    uint32_t n_blocks = 0;
    int      qi = 1;              // K1 sub-batch width (1 or 4)
    bool     mq = false;          // shared passes run on K1m (vsr_mq.h)
    bool     k2 = false;          // shared passes run on K2 / K2w (MFMA screening) + K5r
    bool     k2w = false;         // ... on K2w: workgroup-shared row tiles, up to 128 queries per pass (vsr_mfmaw.h)
    bool     int8 = false;        // ... on the corpus's int8 planes (L2, integer 0..255 rows and queries)
    bool     class_view = false;  // ... on the corpus's class view of the int8 planes (every pass a whole permission class)
    bool     walk = false;        // ... with the main launch's block_map rotated to where the launches in flight are reading (walk_table)
    uint32_t walk_n_pos = 0;      // 64-row units of the view
    uint32_t walk_shift = 0;      // walk_table's slice of a position p: p >> walk_shift
    bool     k2g = false;         // ... on K2g: long rows, 256-query passes, coarse planes (vsr_gemm.h); implies k2w
    bool     sparse_global = false;   // K1s (sparse corpus): the query tables stay in global memory (vsr_scans.h, GLOBAL_TAB)
    uint32_t keep = 0;            // partial list length kp (K2: 2k screening survivors; else k)
    uint32_t rerank_base = 0;     // K2: first partial list holding the per-query screening survivors
    uint32_t n_scan_lists = 0;
    uint32_t qmax = 1;            // query slots per workgroup
    bool     k2i_sample = false;  // int8 planes: the sample pass runs as K2i's per-wave streams (vsr_i8s.h, SAMPLE)
    bool     k2r_sample = false;  // ... of a class-view plan: the same sample from the register-fed kernel (K2r, vsr_i8r.h)
    uint32_t n_blocks_s = 0;
    uint32_t n_partial_s = 0;
    uint32_t n_partial = 0;       // scan partial lists + level-1 K5 outputs (+ K2 survivor lists)
    bool     sel_wave = false;    // K5 items are small enough for the one-wave-per-query radix select
    uint32_t n_launch = 0;        // workgroups of the main launch (= block_map.size() when mapped)
    int64_t  scan_rows = 0;
    int64_t  scan_bytes = 0;
    float    kp_frac = 0;         // K2w: kp * sampling fraction of the densest pass (expected top-kp rows in a sample)
    uint32_t sample_stride = 1;   // K2w: the sample launch visits every sample_stride-th tile of a workgroup
    int64_t  scan_pairs = 0;      // sum over passes of rows * queries
    int64_t  unique_rows = 0;     // distinct filter parts' rows (capped at the corpus size)
};

struct Plan : PlanScalars {
    // slot i = caller query i; passes address their queries through q_slots
    std::vector<uint32_t>    q_slots;        // per pass: the slots of its queries, concatenated
    std::vector<ScanGroup>   groups;         // one K1 / K1m / K2 launch
    std::vector<uint32_t>    list_ids;       // K5 indirection: per query the indices of its partial lists
    std::vector<SelectQuery> sel1;           // level-1 K5 items (only for queries with many partial lists)
    std::vector<SelectQuery> selq;           // final K5 item per query (slot order)
    std::vector<ScanGroup>   groups_s;       // sample pass (threshold seeding): same passes, fewer workgroups
    std::vector<SelectQuery> seedq;          // per query: merge the sample pass's lists into a seed threshold
    std::vector<uint2>       block_map;      // shared-pass launches: workgroup -> (group, block), XCD-aware (vsr_plan.hip)
    std::vector<uint32_t>    walk_table;     // walk: position slice -> slot (a multiple of 8) at which block_map reaches its rows (WalkHint)

    void reset()                             // keeps the vectors' capacity: one plan per batch, no allocation once warm
    {
        static_cast<PlanScalars&>(*this) = PlanScalars{};
        q_slots.clear(); groups.clear(); list_ids.clear(); sel1.clear(); selq.clear(); groups_s.clear(); seedq.clear(); block_map.clear();
        walk_table.clear();
    }
};

// Queries -> passes -> workgroups.  Returns false when the K2w / K2g plan it built cannot be seeded safely (the caller then
// plans again with allow_gemm, then allow_wide, set to false).  Resets `plan` first.
bool make_plan(const vsr_ctx* ctx, const vsr_corpus* c, int nq, int k, int metric, bool allow_screening, bool allow_wide,
               bool allow_gemm, const vsr_filter* const* filters, Plan& plan);

// The rank of the sample's entry that becomes a query's seed threshold: m = ceil(lambda + 6 sqrt(lambda)) + 4 with
// lambda = kp * frac, the expected number of the true top-kp rows in a sample of fraction `frac`.  More than m of them in the
// sample has probability ~1e-8, so the m-th smallest sampled key ranks behind the kp-th row.
inline double seed_lambda(uint32_t kp, double frac) { return (double) kp * frac; }
uint32_t seed_rank(uint32_t kp, double frac);

// Survivors a wave-tile (64 rows x 16 queries) of the K2w main launch can expect: what a query admits over the rows it scans
// (kp + 6 sqrt(kp / f) + 4 / f at the plan's sampling fraction f) x 1024 pairs per wave-tile / the pairs of an average query.
// Up to MASK_EPI_SURVIVORS the mask epilogue wins (vsr_mfmaw.h, EPI = 1); the planner keeps a thinner sample below it too.
constexpr double MASK_EPI_SURVIVORS = 4.0;
inline double survivors_per_wave_tile(const Plan& plan, int nq)
{
    const double kp = plan.keep;
    const double f = plan.kp_frac > 0 ? plan.kp_frac / kp : 1.0 / 16;
    const double admitted = kp + 6.0 * std::sqrt(kp / f) + 4.0 / f;
    const double rows_per_query = (double) plan.scan_pairs / std::max(1, nq);
    return rows_per_query > 0 ? 1024.0 * admitted / rows_per_query : 2.0 * MASK_EPI_SURVIVORS;
}

// the instantiation the main scan launch of a plan resolves to (bench.py reports it beside the roofline)
std::string scan_kernel_name(const Plan& plan, const vsr_corpus* c, int metric, bool k2i = false);

}  // namespace vsr
