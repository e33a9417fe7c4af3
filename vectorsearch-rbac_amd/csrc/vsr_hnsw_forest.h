// vsr_hnsw_forest.h -- the schedule of vsr_hnsw_build_partitions and vsr_hnsw_extend_partitions (vsr_hnsw_build_rt.hip): the batches of
// many HNSW builds, or of many extensions, packed into shared rounds.  Plain C++, no HIP call: tests/test_hnsw_forest_cpu.py compiles this file alone with the host compiler.
//
// All partitions live in one global element space: partition g owns elements base[g] .. base[g + 1] - 1.  Every partition keeps
// the build's own schedule (hnsw_build_batch, vsr_hnsw_sizing.h: max(1, min(done / 8, batch_max, left)) elements, done from 0) and the
// build's own entry-point rule (HnswUpdateGraphInMemory: after a batch, the first element above the entry's level takes over,
// the first element of all when there is no entry yet).  A ROUND walks the unfinished partitions in ascending index and takes
// each one's next batch while the round's elements stay within `cap`; a partition whose batch does not fit waits for the next
// round.  A round is never empty: the first unfinished partition's batch is taken even when it alone is larger than the cap
// (a cap below the build's batch size, VSR_HNSW_FOREST_BATCH), because splitting a batch would let its second half see the
// first and change the graph.  So a round holds either ONE batch (<= batch_max) or several that sum to at most cap <=
// batch_max: its elements number at most batch_max, which is what the source-index bits of the reverse edges' sort key hold.
//
// What a round carries: its elements in ascending global id (partitions ascend, a batch is a run of ids), per element the entry
// point of its graph and that entry's level WHEN THE ROUND BEGAN (-1 / -1: the graph has no element yet), and its record
// capacity, the sum over its elements of 2m + level * m (what an element of that level emits at most).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "vsr_hnsw_sizing.h"                 // the build's batch rule and record capacity

namespace vsr {

struct HnswForestRound {
    uint64_t first_slot = 0;                 // where the round's elements begin in the slot arrays
    uint32_t count = 0;                      // its elements
    uint32_t rec_cap = 0;                    // its record slots
    uint32_t batches = 0;                    // the batches (partitions) it holds
};

struct HnswForestPlan {
    std::vector<int32_t> elems;              // [total] slot -> global element; ascending within a round
    std::vector<int32_t> entry;              // [total] slot -> global entry point of the element's graph when the round began, -1
    std::vector<int32_t> entry_level;        // [total] its level, -1
    std::vector<HnswForestRound> rounds;
    std::vector<int32_t> final_entry;        // [n_parts] global entry point of every finished graph, -1 for an empty partition
};

// The plan of graphs that are partly there already (vsr_hnsw_extend_partitions): partition g's first start_done[g] elements are its
// prior graph, whose entry point is the GLOBAL element start_entry[g] of level start_entry_level[g] (-1 / -1: no element yet); its
// batches are the build's schedule from done = start_done[g], and only the elements behind the prior ones appear in the slots, so
// plan.elems holds base[n_parts] minus the sum of start_done entries.  level[] is read for those elements alone.  A nullptr start
// array stands for zeros (start_done) or -1 (the entry arrays).  The rest as hnsw_forest_plan, which is this plan from nothing.
inline bool hnsw_forest_plan_from(int n_parts, const int64_t* base, const int32_t* level, int m, uint32_t cap, const int64_t* start_done,
                                  const int32_t* start_entry, const int32_t* start_entry_level, HnswForestPlan& plan)
{
    size_t total = 0;
    for (int g = 0; g < n_parts; ++g) total += (size_t) std::max<int64_t>(base[g + 1] - base[g] - (start_done ? start_done[g] : 0), 0);
    plan = HnswForestPlan{};
    plan.elems.reserve(total);
    plan.entry.reserve(total);
    plan.entry_level.reserve(total);
    plan.final_entry.assign((size_t) std::max(n_parts, 0), -1);
    std::vector<int64_t> done((size_t) std::max(n_parts, 0), 0);
    std::vector<int32_t> ent_level((size_t) std::max(n_parts, 0), -1);
    std::vector<int> open;                                                    // unfinished partitions, ascending
    for (int g = 0; g < n_parts; ++g) {
        if (start_done) done[(size_t) g] = start_done[g];
        if (start_entry) plan.final_entry[(size_t) g] = start_entry[g];
        if (start_entry_level) ent_level[(size_t) g] = start_entry_level[g];
        if (base[g + 1] - base[g] > done[(size_t) g]) open.push_back(g);
    }
    std::vector<int> taken;
    while (!open.empty()) {
        HnswForestRound r;
        r.first_slot = plan.elems.size();
        uint64_t rec = 0;
        taken.clear();
        for (int g : open) {
            const int64_t n = base[g + 1] - base[g];
            const int64_t b = hnsw_build_batch(done[(size_t) g], n);
            if (r.count > 0 && (uint64_t) r.count + (uint64_t) b > cap) continue;   // waits for the next round
            for (int64_t e = base[g] + done[(size_t) g]; e < base[g] + done[(size_t) g] + b; ++e) {
                plan.elems.push_back((int32_t) e);
                plan.entry.push_back(plan.final_entry[(size_t) g]);
                plan.entry_level.push_back(ent_level[(size_t) g]);
                rec += hnsw_rec_cap(m, level[(size_t) e]);
            }
            r.count += (uint32_t) b;
            ++r.batches;
            taken.push_back(g);
            if (r.count >= cap) break;
        }
        if (rec > 0x7FFFFFFFull) return false;
        r.rec_cap = (uint32_t) rec;
        plan.rounds.push_back(r);
        // the entry points move when the round is over: its elements did not see each other
        for (int g : taken) {
            const int64_t n = base[g + 1] - base[g];
            const int64_t b = hnsw_build_batch(done[(size_t) g], n);
            for (int64_t e = base[g] + done[(size_t) g]; e < base[g] + done[(size_t) g] + b; ++e)
                if (plan.final_entry[(size_t) g] < 0 || level[(size_t) e] > ent_level[(size_t) g]) {
                    plan.final_entry[(size_t) g] = (int32_t) e;
                    ent_level[(size_t) g] = level[(size_t) e];
                }
            done[(size_t) g] += b;
        }
        open.erase(std::remove_if(open.begin(), open.end(), [&](int g) { return done[(size_t) g] >= base[g + 1] - base[g]; }), open.end());
    }
    return true;
}

// base[n_parts + 1]: ascending, base[0] = 0, base[n_parts] < 2^31; level[base[n_parts]]: the level of every global element;
// cap: 1 .. HB_BATCH_MAX.  Returns false when a round's record capacity would pass 2^31 - 1 (the plan is then unusable).
inline bool hnsw_forest_plan(int n_parts, const int64_t* base, const int32_t* level, int m, uint32_t cap, HnswForestPlan& plan)
{
    return hnsw_forest_plan_from(n_parts, base, level, m, cap, nullptr, nullptr, nullptr, plan);
}

}  // namespace vsr
