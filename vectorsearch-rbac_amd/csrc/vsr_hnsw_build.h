// vsr_hnsw_build.h -- parameters of the batched HNSW build (vsr_hnsw_build.hip), shared with the host loops in vsr_hnsw_build_rt.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "vsr_hnsw_sizing.h"               // HB_NBR, HB_BATCH_MAX, the HB_ERR_* guard-word bits

namespace vsr {

constexpr int HB_TIDS = 10;                // heap TIDs of one element (HNSW_HEAPTIDS, hnsw.h:37)
constexpr int HB_SRC_BITS = 12;            // a reverse edge's sort key ends in its source's index in the batch (< HB_BATCH_MAX)
constexpr int HB_KEY_BITS = 8 + 32 + HB_SRC_BITS;   // layer (<= 255) | target | source index: the bits the sort looks at

struct HnswBuildParams {
    const float4*  rows = nullptr;           // corpus rows (internal order), zero padded to stride4 float4
    uint32_t       stride4 = 0;
    int            metric = 0;               // M_L2 / M_IP (cosine opclass: unit rows, negative inner product)
    int            bits = 0;                 // 1: a bit corpus -- rows are stride4 16-byte chunks of packed bits, metric M_HAMMING / M_JACCARD
    const float*   row_pop = nullptr;        // bits: popcount of every row (Jaccard)
    int            halves = 0;               // 1: a halfvec corpus -- rows are stride4 16-byte chunks of 8 binary16 values, metric M_L2 / M_IP
    int            sparse = 0;               // 1: a sparse corpus -- rows are interleaved (index, value) entries, row r owns entries sp_off[r] ..
                                             // sp_off[r + 1]; stride4 = 1, so that rows + r NAMES row r (never dereferenced); metric M_L2 / M_IP / M_L1
    const uint64_t* sp_off = nullptr;        // sparse: [rows + 1]
    uint32_t       sp_slots = 0;             // sparse: slots of a wave's left-hand table in LDS, a power of two >= 2 x the largest row
    uint32_t       sp_lanes = 0;             // sparse: lanes per row, 4 / 16 / 64 (the corpus's entry-count class)
    uint32_t       m = 0, efc = 0, max_level = 1;
    int32_t*       nbr0 = nullptr;           // [n][2m] neighbour ids, -1 padded
    float*         dist0 = nullptr;          // [n][2m] their distances to the owner
    const int32_t* up_slot = nullptr;        // element -> slot of its upper lists, -1 for level 0
    int32_t*       up_nbr = nullptr;         // [n_upper][max_level][m]
    float*         up_dist = nullptr;
    const int32_t* level = nullptr;          // element -> top level
    const int32_t* elem_row = nullptr;       // element -> the row that holds its vector; nullptr: element e is row e
    int32_t        entry = -1, entry_level = -1;   // the graph's entry point when the batch begins
    uint32_t       first = 0, count = 0;     // the batch: elements first .. first + count - 1
    uint64_t*      rec_key = nullptr;        // reverse edges: (layer << 44) | (target << 12) | the new element's index in the batch
    uint64_t*      rec_val = nullptr;        //                (new element << 32) | distance bits
    uint32_t*      rec_count = nullptr;
    uint32_t       rec_cap = 0;              // record slots of this batch: what its elements can emit at most (from their levels)
    uint32_t       caps = 0;                 // entries of the sorted candidate array (ef_construction + 2m)
    uint32_t       hash_slots = 0;           // visited set of a layer search: open-addressing table in LDS (power of two)
    uint32_t       lds_per_wave = 0;
    uint32_t       wpb = 1;                  // waves (elements) per workgroup
    uint32_t*      err = nullptr;            // the session's guard word: HB_ERR_VISITED / HB_ERR_RECORDS, read by hnsw_build after the last batch
};

// vsr_hnsw_vacuum: what the repair forms of the two build kernels take beside HnswBuildParams (a second kernel argument, so that the
// build's own launches keep theirs).  The batch is elems[0 .. p.count), not p.first ..; p.efc is ef_construction + 1
struct HnswVacuumParams {
    const int32_t* live = nullptr;           // [n_elem] 1: the element has a heap TID left
    const int32_t* elems = nullptr;          // [p.count] the elements this batch repairs, ascending
    int32_t*       stage_nbr = nullptr;      // [p.count][stage_stride] the new lists: layer 0 (2m), then layers 1 .. max_level (m each)
    float*         stage_dist = nullptr;     // their distances
    uint32_t       stage_stride = 0;         // 2m + max_level * m
    // the spill form (hnsw_vacuum_search_spill_kernel): repairs whose working set is in a workspace in global memory
    uint32_t*      spill_count = nullptr;    // mixed attempt: a repair of the LDS kernel that outgrows its arrays appends its batch index to
    int32_t*       spill_list = nullptr;     // spill_list[p.count] and sets no guard bit; nullptr: the guard bits, as ever
    unsigned char* spill_ws = nullptr;       // [spill_pool] workspaces of spill_ws_bytes each (hnsw_vacuum_spill_ws_bytes(spill_n))
    uint64_t       spill_ws_bytes = 0;
    uint32_t       spill_pool = 0;           // waves of the spill launch; wave w takes spilled repairs w, w + spill_pool, ..; 0: no launch
    uint32_t       spill_n = 0;              // n_elem: what every array of a workspace holds
    uint32_t       spill_all = 0;            // 1: every repair of the batch runs in the spill form and the LDS kernel is not launched
    uint32_t*      spill_total = nullptr;    // += the repairs the spill launches ran
};

// vsr_hnsw_build_partitions: what the forest form of the search kernel takes beside HnswBuildParams (a second kernel argument, so
// that the build's own launches keep theirs).  A round (vsr_hnsw_forest.h) is elems[0 .. p.count); the element of batch slot i
// searches from entry[i], not from p.entry.  Elements are GLOBAL ids: every build array holds all partitions' graphs
struct HnswForestParams {
    const int32_t* elems = nullptr;          // [p.count] the round's elements, ascending
    const int32_t* entry = nullptr;          // [p.count] the entry point of the element's graph when the round began; -1: none yet
    const int32_t* entry_level = nullptr;    // [p.count] its level
};

// one graph of the forest, as the split launch writes it out: the arrays of a vsr_hnsw of its own
struct HnswForestGraph {
    int32_t *level = nullptr, *elem_row = nullptr, *nbr0 = nullptr, *up_slot = nullptr, *up_nbr = nullptr, *tid_count = nullptr, *tids = nullptr;
    int32_t base = 0, n_elem = 0;            // global elements base .. base + n_elem - 1 (n_elem >= 1)
    int32_t slot_base = 0;                   // its first upper slot in the global numbering (slots follow element order)
    int32_t max_level = 1;                   // its own stride of the upper lists
};

// vsr_hnsw_extend_partitions: the prior graph of forest graph i (d_priors[i] beside d_graphs[i]), the device arrays of the index it
// lives in.  n_elem = 0: no prior graph, the pointers are not read
struct HnswForestPrior {
    const int32_t *level = nullptr, *elem_row = nullptr, *nbr0 = nullptr, *up_slot = nullptr, *up_nbr = nullptr, *tid_count = nullptr,
                  *tids = nullptr;
    int32_t n_elem = 0;                      // the graph's first n_elem elements are the prior's, in its numbering
    int32_t n_upper = 0, max_level = 1;      // its upper slots (the graph's first n_upper) and the stride of its upper lists
};
// what the join launches write beside p.nbr0 / p.up_nbr: the per-element arrays p reads, the slot -> owner table of the edge-distance
// launch, and two result words
struct HnswForestJoin {
    int32_t *level = nullptr, *elem_row = nullptr, *up_slot = nullptr;   // [n_total]; the new elements' entries are the host's
    int32_t* up_owner = nullptr;             // [all upper slots], -1 filled by the caller
    uint32_t n_rows = 0;                     // rows of the corpus: what an element's row and a heap TID are bounded by
    uint32_t* bad = nullptr;                 // min over the graphs with a prior array that held a value outside its range of the graph's
                                             // index (the element was joined as a level-0 element without edges; the caller throws the
                                             // attempt away); all ones: none
    unsigned long long* held = nullptr;      // min over the prior heap TIDs that name a new row of their graph of (graph index << 32) | row;
                                             // all ones: none
};

// one workspace of the spill form for a graph of n elements: C, W and T (8 bytes an element each), wd (4) and the visited bitmap
inline size_t hnsw_vacuum_spill_ws_bytes(uint32_t n)
{
    return ((size_t) n * 28 + (((size_t) n + 31) / 32) * 4 + 15) & ~(size_t) 15;
}

// what the merging pre-pass (vsr_hnsw_dedup.hip) leaves: device arrays of n_elem entries, the caller's to hipFree
struct HnswElemTable {
    int32_t  n_elem = 0;
    int32_t* elem_row = nullptr;             // the element's first member (internal row): its vector
    int32_t* tid_count = nullptr;            // members, 1 .. HB_TIDS
    int32_t* tids = nullptr;                 // [n_elem][HB_TIDS] internal rows in insertion order, -1 padded
    int32_t* level = nullptr;                // the level drawn for the first member
};
struct HnswDedupTimes {                      // device-event times of the pre-pass's phases, summed over its rounds
    float hash_ms = 0, sort_ms = 0, resolve_ms = 0, table_ms = 0;
    int   rounds = 0;
};

}  // namespace vsr

// byte-identical rows -> elements of up to HB_TIDS members (include/vsrbac.h, VSR_HNSW_BUILD_MERGE_DUPLICATES).  hash_bits:
// 1 .. 64 bits of the row hash that take part; d_row_level: the level drawn for every row.  Synchronises s.
hipError_t vsr_hnsw_dedup_elements(const float4* rows, uint32_t n, uint32_t stride4, int hash_bits, const int32_t* d_row_level,
                                   vsr::HnswElemTable* out, vsr::HnswDedupTimes* times, hipStream_t s);
// one batch: search + select + own lists, sort of the reverse edges, their application (all on stream s, no synchronisation)
hipError_t vsr_hnsw_build_batch(vsr::HnswBuildParams& p, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt, uint64_t* d_val_alt,
                                hipStream_t s);
size_t vsr_hnsw_build_sort_bytes(uint32_t rec_cap);
// vsr_hnsw_build_partitions.  One round (p.count <= HB_BATCH_MAX elements, f.elems): the forest searches, the sort and the link
// launch, all on s.  p.elem_row is set (IND = true); p.first, p.entry and p.entry_level are not read.
hipError_t vsr_hnsw_forest_round(vsr::HnswBuildParams& p, const vsr::HnswForestParams& f, void* d_sort_tmp, size_t sort_tmp_bytes,
                                 uint64_t* d_key_alt, uint64_t* d_val_alt, hipStream_t s);
// every graph's own arrays from the global ones (one launch on s): ids minus base, upper slots minus slot_base, upper lists at
// the graph's max_level, one heap TID per element.  d_graphs[n_graphs]: the non-empty graphs, ascending base, covering 0 .. n_total - 1
hipError_t vsr_hnsw_forest_split(const vsr::HnswBuildParams& p, const vsr::HnswForestGraph* d_graphs, uint32_t n_graphs, uint32_t n_total,
                                 hipStream_t s);
// vsr_hnsw_extend_partitions.  The inverse of the split, for the graphs that arrive (two launches on s): every prior graph's arrays
// into the global ones -- ids plus base, upper slots plus slot_base, upper lists at the global stride p.max_level, j.up_owner --
// and j.held.  The caller has filled p.nbr0 / p.up_nbr / j.up_owner with -1 and written the new elements' level, row (ascending within
// a graph) and upper slot.  d_graphs[i].n_elem counts prior and new elements; the output pointers of d_graphs are not read
hipError_t vsr_hnsw_forest_join(const vsr::HnswBuildParams& p, const vsr::HnswForestJoin& j, const vsr::HnswForestGraph* d_graphs,
                                const vsr::HnswForestPrior* d_priors, uint32_t n_graphs, uint32_t n_total, hipStream_t s);
// vsr_hnsw_forest_split for joined graphs: a prior element keeps the heap TIDs of d_priors, a new one holds its row alone
hipError_t vsr_hnsw_forest_split_carry(const vsr::HnswBuildParams& p, const vsr::HnswForestGraph* d_graphs, const vsr::HnswForestPrior* d_priors,
                                       uint32_t n_graphs, uint32_t n_total, hipStream_t s);
// vsr_hnsw_vacuum.  One repair batch (p.count <= HB_BATCH_MAX elements, v.elems): the searches into v.stage_*, the install launch,
// the sort and the link launch, all on s.  The selection's scratch lies over the visited table (hash_slots / 3 candidates).
// With v.spill_pool > 0 the spill launch runs between the searches and the install: over the repairs the LDS launch listed
// (v.spill_count / v.spill_list, the mixed attempt) or over all of them, the LDS launch left out (v.spill_all).
hipError_t vsr_hnsw_vacuum_batch(vsr::HnswBuildParams& p, const vsr::HnswVacuumParams& v, void* d_sort_tmp, size_t sort_tmp_bytes,
                                 uint64_t* d_key_alt, uint64_t* d_val_alt, hipStream_t s);
// scratch of the compaction and the scan below, for n_elem elements
size_t vsr_hnsw_vacuum_tmp_bytes(uint32_t n_elem);
// d_flag[e] = NeedsUpdated(e) for every live e != skip; d_list (may be nullptr): the flagged elements ascending, *d_num of them
hipError_t vsr_hnsw_vacuum_mark(const vsr::HnswBuildParams& p, const int32_t* d_live, uint32_t n_elem, int32_t skip, uint8_t* d_flag,
                                int32_t* d_list, int32_t* d_num, void* d_tmp, size_t tmp_bytes, hipStream_t s);
// d_map = exclusive scan of d_live; the live elements' lists, renumbered, into the compacted arrays (memset to -1 by the caller)
hipError_t vsr_hnsw_vacuum_renumber(const vsr::HnswBuildParams& p, const int32_t* d_live, int32_t* d_map, const int32_t* d_slot_map,
                                    uint32_t n_elem, int32_t* d_new_nbr0, int32_t* d_new_up_nbr, uint32_t new_max_level, void* d_tmp,
                                    size_t tmp_bytes, hipStream_t s);
// vsr_hnsw_extend: fills p.dist0 / p.up_dist for the lists of elements 0 .. n_prior - 1 from the ids p.nbr0 / p.up_nbr hold (one
// launch on s, no synchronisation).  d_up_owner[n_upper_prior]: upper slot -> its element, -1 for a slot no element names.  Every
// id in those lists is in [-1, n_prior), lists are packed, and a neighbour on layer lc has an upper slot: the caller checked.
hipError_t vsr_hnsw_edge_distances(const vsr::HnswBuildParams& p, uint32_t n_prior, const int32_t* d_up_owner, uint32_t n_upper_prior,
                                   hipStream_t s);
