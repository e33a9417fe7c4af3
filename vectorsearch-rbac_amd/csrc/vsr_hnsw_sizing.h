// vsr_hnsw_sizing.h -- everything the batched HNSW build, extend, partition build and vacuum (vsr_hnsw_build_rt.hip) decide without a
// GPU: the level stream, the batch rule, the per-wave LDS of the build's and the repair's search kernel, the initial sizes and one
// step of the restart ladder.  Plain C++, no HIP call: tests/test_hnsw_sizing_cpu.py compiles this file alone with the host compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vsr {

constexpr int HB_NBR = 256;                // neighbour ids of one expansion / one list (2m <= 200)
constexpr uint32_t HB_BATCH_MAX = 4096;    // elements of one batch
constexpr uint32_t HB_ERR_VISITED = 16u;   // guard-word bit: a visited table filled up (the call restarts with a larger one)
constexpr uint32_t HB_ERR_RECORDS = 32u;   // guard-word bit: reverse edges past rec_cap were dropped
constexpr uint32_t HB_ERR_CANDIDATES = 64u;   // guard-word bit (sparse build, vacuum): the candidate array dropped an unexpanded candidate as
                                              // near as the furthest of W, which pgvector's unbounded heap would still expand (the call
                                              // restarts with a longer array)
constexpr uint32_t HB_ERR_BITS = HB_ERR_VISITED | HB_ERR_RECORDS | HB_ERR_CANDIDATES;
constexpr uint32_t HB_SLOTS_MAX = 32768;   // the largest visited table of a layer search
constexpr size_t HN_LDS_BUDGET = 156 * 1024;   // of the CU's 160 KB (dynamic LDS of one workgroup)

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
        if (u == 0.0) return cap;                                             // -ln(0) is +inf: no int holds it
        return std::min((int) (-std::log(u) * ml), cap);
    }
};

// the schedule: the batch that follows `done` inserted elements of n never exceeds 1/8 of the graph it is inserted into (its
// elements do not see each other)
inline int64_t hnsw_build_batch(int64_t done, int64_t n)
{
    return std::max<int64_t>(1, std::min<int64_t>({done / 8, (int64_t) HB_BATCH_MAX, n - done}));
}
// an element of level l emits at most 2m + l * m reverse edges, so a batch's record slots are known on the host
inline uint64_t hnsw_rec_cap(int m, int32_t level) { return (uint64_t) (2 * m + level * m); }

// per-wave LDS of the build's search kernel (hnsw_build_search_kernel's carve-up) with `slots` visited-table entries and, a sparse
// build, the wave's left-hand table of sp_slots (index, value) slots behind them
inline size_t hnsw_build_lds_per_wave(uint32_t caps, uint32_t slots, uint32_t sp_slots = 0)
{
    return (((size_t) caps * 8 + ((caps + 15) & ~15u) + (size_t) HB_NBR * 12 + (size_t) caps * 4 + (size_t) slots * 4 + 15) & ~(size_t) 15) +
           (size_t) sp_slots * 8;
}
// per-wave LDS of the repair's search kernel (hb_search_body, VAC): S and the flags, the three HB_NBR arrays, the visited table; the
// selection's scratch lies over the table, so an entry of S costs 9 bytes and a graph's whole working set can be thousands long
inline size_t hnsw_vacuum_lds_per_wave(uint32_t caps, uint32_t slots)
{
    return ((size_t) caps * 8 + ((caps + 15) & ~15u) + (size_t) HB_NBR * 12 + (size_t) slots * 4 + 15) & ~(size_t) 15;
}
// the longest candidate array of a repair that fits `budget` beside `slots` visited slots, a multiple of 16
inline uint32_t hnsw_vacuum_caps_fit(size_t budget, uint32_t slots)
{
    const size_t fixed = (size_t) HB_NBR * 12 + (size_t) slots * 4 + 64;
    return budget > fixed ? (uint32_t) ((budget - fixed) / 9) & ~15u : 0u;
}
// waves (elements) of one workgroup
inline uint32_t hnsw_build_wpb(size_t budget, size_t per_wave) { return (uint32_t) std::min<size_t>(4, budget / per_wave); }

// the visited table a layer search starts with when nothing sets it
inline uint32_t hnsw_default_visited_slots(int ef_construction, int m)
{
    uint32_t slots = 4096;
    while (slots < (uint32_t) ef_construction * 2u * (uint32_t) m * 2u && slots < HB_SLOTS_MAX) slots <<= 1;
    return slots;
}

// The restart ladder.  A call never returns a thinner graph than it was asked for: when an attempt's kernels set guard bits, the
// attempt is thrown away and run again with larger arrays, as long as they fit the LDS.  RECORDS is fatal; CANDIDATES doubles the
// candidate array (up to caps_ceiling); VISITED doubles the table (up to HB_SLOTS_MAX).  With both bits the array grows first and the
// table is then judged beside the longer array.
struct HnswLadder {
    bool     vacuum = false;                 // hnsw_vacuum_lds_per_wave; else hnsw_build_lds_per_wave with sp_slots
    uint32_t sp_slots = 0;
    size_t   budget = HN_LDS_BUDGET;
    uint32_t caps_ceiling = 0xFFFFFFFFu;     // vacuum: hnsw_vacuum_caps_fit(budget, slots)
    size_t lds(uint32_t caps, uint32_t slots) const { return vacuum ? hnsw_vacuum_lds_per_wave(caps, slots) : hnsw_build_lds_per_wave(caps, slots, sp_slots); }
};
enum HnswLadderEnd { HB_LADDER_ON = 0, HB_LADDER_RECORDS, HB_LADDER_CANDIDATES, HB_LADDER_VISITED };

// One step: HB_LADDER_ON with the next sizes in *caps / *slots, or the ladder that ended.  A size whose ladder ended stays as it was
// (the refusals name it); the candidate array that grew before the table's ladder ended stays grown (vacuum's mixed attempt runs at
// those sizes).
inline HnswLadderEnd hnsw_ladder_step(const HnswLadder& l, uint32_t guard, uint32_t* caps, uint32_t* slots)
{
    if (guard & HB_ERR_RECORDS) return HB_LADDER_RECORDS;
    if (guard & HB_ERR_CANDIDATES) {
        const uint32_t next = (uint32_t) std::min<uint64_t>((uint64_t) *caps * 2u, l.caps_ceiling);
        if (next <= *caps || l.lds(next, *slots) > l.budget) return HB_LADDER_CANDIDATES;
        *caps = next;
    }
    if (guard & HB_ERR_VISITED) {
        if (*slots >= HB_SLOTS_MAX || l.lds(*caps, *slots * 2u) > l.budget) return HB_LADDER_VISITED;
        *slots *= 2u;
    }
    return HB_LADDER_ON;
}

}  // namespace vsr
