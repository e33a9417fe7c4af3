// vsr_hnsw_build.hip — CREATE INDEX ... USING hnsw on the GPU: batched insertion (pgvector/src/hnswbuild.c:357-470,
// hnswutils.c:813-1346).
//
// pgvector inserts one element at a time: HnswFindElementNeighbors searches the graph as it stands (greedy descent, then
// HnswSearchLayer with ef_construction on every layer the element lives on), SelectNeighbors picks up to m (2m on layer 0)
// of the candidates with the "closer to the query than to any neighbour already selected" heuristic, and
// HnswUpdateConnection adds the reverse edge to every selected neighbour, pruning that neighbour's list with the same
// heuristic when it is full.  Its own parallel build runs several such insertions at once against a graph the others are
// changing under it, so the graph is not reproducible even in the reference; what it guarantees (and tests:
// test/t/012_hnsw_vector_build_recall.pl) is recall.
//
// The GPU build inserts BATCHES: every element of a batch searches the graph as it stood when the batch began (one wave per
// element, vsr_hnsw.h's search machinery), selects its neighbours and writes its own lists; the reverse edges of the whole
// batch are then sorted by (layer, target, source's index in the batch) and one wave per (layer, target) applies its run of
// HnswUpdateConnection calls one after another, in ascending source element.  Elements of one batch do not see each other, so
// a batch is never larger than 1/8 of the graph it is inserted into (the first elements go in one by one).
// Nothing in this depends on timing -- the record slots are claimed in wave arrival order, which is why the source index is part
// of the sort key -- so the same rows, seed, m, ef_construction and flags give the same graph, run to run, and on integer-valued
// rows (fp32 sums independent of their order) that graph is the one the serial restatement of THIS algorithm builds
// (the test suite's orc_hnsw_build_batched; tests/test_gpu_hnsw_build_model.py compares the exported arrays).
// Tie rules: where pgvector leaves an order open (equal distances in a heap) keys are (distance, element id), lower id first,
// in S, in hb_select's input and in the full-list sort of the link kernel; where it is definite the kernels follow it
// (CheckElementCloser's <=, keep-pruned-connections, which candidate counts as pruned, replace in place or append, and
// SelectNeighbors returning a short candidate list as it came: furthest first).
// A visited table that fills up ends the element's search early and sets HB_ERR_VISITED in the guard word; records past rec_cap
// set HB_ERR_RECORDS.  hnsw_build (vsr_hnsw_build_rt.hip) reads the word after the last batch: it never returns such a graph.
// Levels come from the same seeded xorshift64* stream as the test suite's serial CPU restatement
// (level = floor(-ln(u) / ln(m)), hnswutils.c:243), so both builds place the same elements on the same layers.
// Identical vectors: pgvector folds a row whose vector equals a selected layer-0 neighbour's into that element's heap TIDs
// (up to 10, hnswbuild.c:309-355).  ef_search bounds ELEMENTS, so this changes what a search returns: on a corpus of
// 8-fold duplicates a graph of one element per row emits at most ef_search rows where the merged graph emits 8 x as many.
// vsr_hnsw_build keeps one element per row; vsr_hnsw_build_ex with VSR_HNSW_BUILD_MERGE_DUPLICATES runs
// vsr_hnsw_dedup.hip's pre-pass first and the kernels below then insert ELEMENTS, reaching an element's vector through
// HnswBuildParams::elem_row (template parameter IND; without it element e is row e and the gather is the plain one).
//
// Bit corpora (vsr_hnsw_build_bit, bit_hamming_ops / bit_jaccard_ops): template parameter ROWS = ROWS_BIT gives hb_distances --
// the one place that reads row values -- K4b's lane mapping and integer arithmetic (bit_graph_distances, vsr_bitops.h);
// SelectNeighbors, the reverse-edge pass, the batching and the level stream do not know the row format.  The pre-pass of the
// merging build compares rows as 16-byte chunks and serves packed bits as it stands.  Parity: pgvector's
// test/t/020_hnsw_bit_build_recall.pl floors (tests/test_gpu_hnsw_bit.py).
//
// Halfvec corpora (vsr_hnsw_build_half, halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops): ROWS = ROWS_HALF gives hb_distances
// K4h's lane mapping and arithmetic (half_graph_distances, vsr_halfops.h: both rows widened to fp32, fmaf sums); the inserted
// element's row is the "query" and is binary16 already.  The pre-pass compares the binary16 bytes, so +0.0 and -0.0 differ
// (datumIsEqual on a halfvec).  Parity: pgvector's test/t/024_hnsw_halfvec_build_recall.pl floors (tests/test_gpu_hnsw_half.py).
//
// Sparse corpora (vsr_hnsw_build_sparse, sparsevec_l2_ops / sparsevec_ip_ops / sparsevec_cosine_ops / sparsevec_l1_ops): ROWS =
// ROWS_SPARSE gives hb_distances K4s's lane mapping and arithmetic (sparse_graph_distances, vsr_sparseops.h).  The left-hand vector
// -- the inserted element in the search, a candidate in hb_select, a target's neighbour in the link kernel -- is a hash table in the
// wave's LDS that the wave rebuilds from the left-hand row whenever that row changes (sparse_left_load: sized once per build from
// the corpus's largest row, at most 2048 slots = 16 KB).  Which slot an entry lands in may depend on lane timing; what a lookup
// returns and the order of every sum do not, so the build stays deterministic.  No merging build: the pre-pass compares
// fixed-stride rows.  Parity: pgvector's test/t/028_hnsw_sparsevec_build_recall.pl floors (tests/test_gpu_hnsw_sparse.py).
//
// Extension (vsr_hnsw_extend): the same batches inserted into a graph that arrived as arrays.  The one piece of state such a graph
// lacks, the distance of every edge (dist0 / up_dist, read when a full list is re-selected), is filled in by hnsw_edge_dist_kernel
// before the first batch; elements reach their rows through elem_row whenever element != internal row (a merged prior graph, new
// rows that sort between old ones).  fp32, halfvec and bit rows; tests/test_gpu_hnsw_extend.py.
//
// Partitions (vsr_hnsw_build_partitions): the graphs of many row subsets of one corpus, built in one global element space over one
// set of build arrays.  A round (vsr_hnsw_forest.h) holds the next batch of every partition that has one due; its searches are
// hnsw_forest_search_kernel -- the search body with the batch as a list and the entry point per batch slot -- and its sort and link
// launch are the build's, which act on each graph as its own would because targets of different graphs are disjoint.
// hnsw_forest_split_kernel then writes every graph's own arrays.  fp32, halfvec and bit rows; tests/test_gpu_hnsw_partitions.py.
//
// Partitions that exist (vsr_hnsw_extend_partitions): the extension of many graphs in that element space.  hnsw_forest_join_kernel is
// the split's inverse for the prior graphs, hnsw_forest_held_kernel looks every prior heap TID up among its graph's new rows,
// hnsw_edge_dist_kernel runs over all elements, the rounds are the partition build's from done = the prior n_elem, and
// hnsw_forest_split_kernel<true> carries the prior TID lists over.  tests/test_gpu_hnsw_extend_partitions.py.
//
// Parity definition (tests/test_gpu_index.py): recall@20 at ef_search = 40 against the exact scan >= pgvector's TAP
// thresholds on its own case (10 000 x 3-d: 0.99; inner product 0.97), and within 0.01 of that serial build's recall on
// the same rows; and (tests/test_gpu_hnsw_build_model.py) graph identity with the batched model, as above.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "vsr_device.h"
#include "vsr_topk.h"
#include "vsr_bitops.h"
#include "vsr_halfops.h"
#include "vsr_sparseops.h"
#include "vsr_hnsw_build.h"

namespace vsr {

// (hnsw_rank_value: vsr_halfops.h)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// global-memory stores of the wave visible to its later loads, and LDS as wave_sync (vsr_hnsw.h has the same for K4's discard array)
__device__ __forceinline__ void wave_sync_global()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int32_t* hb_list(const HnswBuildParams& p, uint32_t e, int lc, float** dist)
{
    if (lc == 0) {
        *dist = p.dist0 + (size_t) e * 2 * p.m;
        return p.nbr0 + (size_t) e * 2 * p.m;
    }
    const size_t at = ((size_t) p.up_slot[e] * p.max_level + (uint32_t) (lc - 1)) * p.m;
    *dist = p.up_dist + at;
    return p.up_nbr + at;
}

// distance (the opclass's index distance: squared L2 or negative inner product) of row `a` to `cnt` elements listed in ids[]
// -> out[]; two elements per wave instruction (32 lanes each), fp32 sums
// the vector of element e (I: the id's own integer type, so that the direct form is the address arithmetic it always was)
template <bool IND, class I>
__device__ __forceinline__ const float4* hb_row(const HnswBuildParams& p, I e)
{
    return p.rows + (size_t) (IND ? (I) p.elem_row[e] : e) * p.stride4;
}

// ROWS_BIT (a bit corpus, metric M_HAMMING / M_JACCARD): the lane mapping and arithmetic of K4b (bit_graph_distances, vsr_bitops.h)
// ROWS_HALF (a halfvec corpus, metric M_L2 / M_IP): those of K4h (half_graph_distances, vsr_halfops.h)
// ROWS_SPARSE (a sparse corpus, metric M_L2 / M_IP / M_L1): those of K4s (sparse_graph_distances, vsr_sparseops.h).  The left-hand
// operand is a table in the wave's LDS (left: which row it holds), rebuilt here whenever `a` names another row
template <bool IND, int ROWS>
__device__ __forceinline__ void hb_distances(const HnswBuildParams& p, const float4* a, const int32_t* ids, int cnt, float* out, int lane,
                                             SparseLeft* left = nullptr)
{
    if constexpr (ROWS == ROWS_SPARSE) {
        sparse_left_load(*left, p.rows, p.sp_off, (int64_t) (a - p.rows), lane);      // (stride4 = 1: a names the row)
        const uint32_t mask = p.sp_slots - 1u, shift = (uint32_t) __clz((int) p.sp_slots) + 1u;
        sparse_graph_distances_metric(p.metric, p.rows, p.sp_off, p.sp_lanes, IND ? p.elem_row : nullptr, (lds_u64) left->tab, mask, shift,
                                      left->q2, left->q1, ids, cnt, out, lane);
        wave_sync();
        return;
    } else if constexpr (ROWS == ROWS_BIT) {
        const uint32_t G = bit_graph_lanes(p.stride4), gl = (uint32_t) lane & (G - 1u);
        const uint4* rows = reinterpret_cast<const uint4*>(p.rows);
        const uint4* qs = reinterpret_cast<const uint4*>(a);
        uint4 qreg = make_uint4(0u, 0u, 0u, 0u);
        if (p.stride4 <= 64u && gl < p.stride4) qreg = qs[gl];
        const int32_t* er = IND ? p.elem_row : nullptr;
        if (p.metric == M_JACCARD)
            bit_graph_distances<true>(rows, p.stride4, G, er, p.row_pop, qs, qreg, p.row_pop[(size_t) (a - p.rows) / p.stride4], ids, cnt, out, lane);
        else
            bit_graph_distances<false>(rows, p.stride4, G, er, p.row_pop, qs, qreg, 0.0f, ids, cnt, out, lane);
        wave_sync();
        return;
    } else if constexpr (ROWS == ROWS_HALF) {
        // (rows are stride4 16-byte chunks of 8 binary16 values; `a` is such a row)
        const uint32_t G = bit_graph_lanes(p.stride4), gl = (uint32_t) lane & (G - 1u);
        const uint4* rows = reinterpret_cast<const uint4*>(p.rows);
        const uint4* qs = reinterpret_cast<const uint4*>(a);
        uint4 qreg = make_uint4(0u, 0u, 0u, 0u);
        if (p.stride4 <= 64u && gl < p.stride4) qreg = qs[gl];
        const int32_t* er = IND ? p.elem_row : nullptr;
        if (p.metric == M_L2) half_graph_distances<true>(rows, p.stride4, G, er, qs, qreg, ids, cnt, out, lane);
        else half_graph_distances<false>(rows, p.stride4, G, er, qs, qreg, ids, cnt, out, lane);
        wave_sync();
        return;
    } else {
    const int half = lane >> 5, hl = lane & 31;
    for (int c0 = 0; c0 < cnt; c0 += 8) {
        float s[4];
        const float4* b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 2 * u + half;
            s[u] = 0.0f;
            b[u] = hb_row<IND>(p, c < cnt ? ids[c] : ids[0]);
        }
        for (uint32_t ch = (uint32_t) hl; ch < p.stride4; ch += 32) {
            const float4 av = a[ch];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 bv = b[u][ch];
                if (p.metric == M_L2) {
                    const float d0 = av.x - bv.x, d1 = av.y - bv.y, d2 = av.z - bv.z, d3 = av.w - bv.w;
                    s[u] = fmaf(d0, d0, s[u]); s[u] = fmaf(d1, d1, s[u]); s[u] = fmaf(d2, d2, s[u]); s[u] = fmaf(d3, d3, s[u]);
                } else {
                    s[u] = fmaf(av.x, bv.x, s[u]); s[u] = fmaf(av.y, bv.y, s[u]); s[u] = fmaf(av.z, bv.z, s[u]); s[u] = fmaf(av.w, bv.w, s[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            for (int mm = 16; mm >= 1; mm >>= 1) s[u] += __shfl_xor(s[u], mm);
            const int c = c0 + 2 * u + half;
            if (hl == 0 && c < cnt) out[c] = hnsw_rank_value(p.metric, s[u]);
        }
    }
    wave_sync();
    }
}

// SelectNeighbors (hnswutils.c:1053-1154): cand[0 .. n) = (distance to the owner, element) nearest first; keeps up to lm of them
// in sel[] (indices into cand, selection order).  A candidate is taken when it is closer to the owner than to every
// neighbour already taken (CheckElementCloser); when fewer than lm pass, the passed-over ones fill up in order ("keep
// pruned connections").  *pruned = index of the candidate pgvector would call pruned (only meaningful for n > lm).
// scratch: ids[lm], nd[lm] in LDS.  Returns the number selected.
template <bool IND, int ROWS>
__device__ __forceinline__ int hb_select(const HnswBuildParams& p, const uint64_t* cand, int n, int lm, int32_t* sel, int32_t* wd,
                                         int32_t* ids, float* nd, int* pruned, int lane, SparseLeft* left = nullptr)
{
    if (n <= lm) {
        // "return c" (hnswutils.c:1071-1072): the candidates as HnswSearchLayer's w lists them, FURTHEST first
        for (int i = lane; i < n; i += 64) sel[i] = n - 1 - i;
        *pruned = -1;
        wave_sync();
        return n;
    }
    int nsel = 0, nwd = 0, i = 0;
    for (; i < n && nsel < lm; ++i) {
        const uint32_t e = (uint32_t) cand[i];
        const float de = mono_to_float((uint32_t) (cand[i] >> 32));
        bool closer = true;
        if (nsel > 0) {
            hb_distances<IND, ROWS>(p, hb_row<IND>(p, e), ids, nsel, nd, lane, left);
            bool bad = false;
            for (int j = lane; j < nsel; j += 64) bad |= nd[j] <= de;
            closer = __ballot(bad) == 0;
        }
        if (lane == 0) {
            if (closer) { sel[nsel] = i; ids[nsel] = (int32_t) e; }
            else wd[nwd] = i;
        }
        if (closer) ++nsel; else ++nwd;
        wave_sync();
    }
    int wdoff = 0;
    while (wdoff < nwd && nsel < lm) {
        if (lane == 0) sel[nsel] = wd[wdoff];
        ++nsel;
        ++wdoff;
    }
    wave_sync();
    // pruned: the next passed-over candidate, or (none left) the furthest candidate still in the working list
    *pruned = wdoff < nwd ? wd[wdoff] : n - 1;
    return nsel;
}

// ---- phase 1: one wave per new element: search the frozen graph, select, write the element's own lists, emit reverse edges ----
// VAC (vsr_hnsw_vacuum): the REPAIR of an element that is in the graph already -- HnswFindElementNeighbors with existing = true
// (hnswvacuum.c's RepairGraphElement).  The batch is v.elems[]; deleted elements (v.live[e] == 0) and the element itself are walked
// and stay in W, but only live elements count towards the beam (CountElement): a live push that takes the live count beyond ef
// takes the furthest entry, deleted or live, off W.  The count starts at the live entry points and is never taken back, so a layer
// entered with more than ef live entry points loses one entry per live push from the start.  Every push after the first loss is
// nearer than W's furthest, so W is the nearest pushed - popped entries of everything pushed: still a prefix of S.
// Before the selection the deleted elements
// and the element itself leave the candidates (RemoveElements); the new lists go to v.stage_* and not to the graph, which the
// other waves of the batch are reading.  S can outgrow any bound here (a graph with few live elements admits everything), so the
// loss check of the sparse build is on, and so is one for a W longer than S.
// MIXED (VAC only): the mixed attempt's form, see the end of the body
// FOREST (vsr_hnsw_build_partitions; not with VAC): a round of many graphs that share the build arrays.  The batch is f.elems[],
// and the entry point and its level are those of the element's own graph, f.entry[bi] / f.entry_level[bi], where the build reads
// p.entry / p.entry_level.  A wave whose graph has no entry yet emits nothing, as the build's first element.  Nothing else differs:
// the LDS carve-up is the build's
template <bool IND, int ROWS, bool VAC, bool MIXED = false, bool FOREST = false>
__device__ __forceinline__ void hb_search_body(const HnswBuildParams& p, const HnswVacuumParams& v, const HnswForestParams& f = HnswForestParams{})
{
    static_assert(!(VAC && FOREST), "the forest form is a build");
    extern __shared__ __align__(16) unsigned char smem_all[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint32_t bi = blockIdx.x * p.wpb + wave;
    if (wave >= p.wpb || bi >= p.count) return;                               // (waves are independent: no workgroup barrier)
    uint32_t me_;
    if constexpr (VAC) me_ = (uint32_t) v.elems[bi]; else if constexpr (FOREST) me_ = (uint32_t) f.elems[bi]; else me_ = p.first + bi;
    const uint32_t me = me_;
    int32_t entry_ = p.entry, entry_level_ = p.entry_level;
    if constexpr (FOREST) {
        entry_ = f.entry[bi];
        entry_level_ = f.entry_level[bi];
    }
    const int32_t entry = entry_, entry_level = entry_level_;                 // the entry point this search starts from, and its level
    unsigned char* smem = smem_all + (size_t) wave * p.lds_per_wave;
    uint64_t* S = reinterpret_cast<uint64_t*>(smem);                          // [caps] candidates, sorted, nearest first
    uint8_t*  X = reinterpret_cast<uint8_t*>(S + p.caps);                     // [caps] expanded flags
    int32_t*  nb = reinterpret_cast<int32_t*>(X + ((p.caps + 15) & ~15u));    // [HB_NBR] neighbour ids of an expansion / selected ids
    float*    nd = reinterpret_cast<float*>(nb + HB_NBR);                     // [HB_NBR] distances
    int32_t*  sel = reinterpret_cast<int32_t*>(nd + HB_NBR);                  // [HB_NBR] selected candidate indices
    int32_t*  wd = sel + HB_NBR;                                              // [caps] passed-over candidate indices
    uint32_t* lv = reinterpret_cast<uint32_t*>(wd + p.caps);                  // [hash_slots] visited set
    // VAC: S can be thousands of entries long, so the selection's scratch does not get arrays of caps entries of its own.  T[tcap],
    // the candidates without the deleted elements and `me`, and wd[tcap] lie over the visited table, which no one reads between the
    // end of a layer search and the clear_visited() of the next: 12 bytes a candidate, tcap = hash_slots / 3
    uint64_t* T = nullptr;
    uint32_t tcap = 0;
    if constexpr (VAC) {
        lv = reinterpret_cast<uint32_t*>(sel + HB_NBR);
        T = reinterpret_cast<uint64_t*>(lv);
        tcap = p.hash_slots / 3u;
        wd = reinterpret_cast<int32_t*>(T + tcap);
    }
    const float4* q = hb_row<IND>(p, me);
    const int my_level = p.level[me];
    SparseLeft left;                                                          // ROWS_SPARSE: the left-hand table, the last sp_slots * 8 bytes
    if constexpr (ROWS == ROWS_SPARSE) {
        left.tab = reinterpret_cast<uint64_t*>(smem + p.lds_per_wave - (size_t) p.sp_slots * 8);
        left.slots = p.sp_slots;
    }

    // VAC: the staged lists of `me`
    int32_t* st_n = nullptr;
    float* st_d = nullptr;
    if constexpr (VAC) {
        st_n = v.stage_nbr + (size_t) bi * v.stage_stride;
        st_d = v.stage_dist + (size_t) bi * v.stage_stride;
    }
    auto own_list = [&](int lc, float** dist) -> int32_t* {
        if constexpr (VAC) {
            const uint32_t at = lc == 0 ? 0u : (uint32_t) (lc + 1) * p.m;     // 2m + (lc - 1) m
            *dist = st_d + at;
            return st_n + at;
        } else {
            return hb_list(p, me, lc, dist);
        }
    };

    // the element's own lists start empty
    for (int lc = 0; lc <= my_level; ++lc) {
        float* dl;
        int32_t* nl = own_list(lc, &dl);
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        for (uint32_t j = (uint32_t) lane; j < lm; j += 64) { nl[j] = -1; dl[j] = 0.0f; }
    }
    if (entry < 0) return;                                                    // the very first element (VAC: nobody else is left)

    constexpr bool defer = VAC && MIXED;                                      // mixed attempt: records wait until every layer is done
    bool overflow = false;
    uint32_t used = 0;
    auto clear_visited = [&]() {
        for (uint32_t i = (uint32_t) lane; i < p.hash_slots; i += 64) lv[i] = 0u;
        used = 0;
        wave_sync();
    };
    auto visit = [&](uint32_t e) -> bool {
        const uint32_t mask = p.hash_slots - 1u;
        uint32_t h = (e * 2654435761u) >> 7;
        for (uint32_t probe = 0; probe <= mask; ++probe, ++h) {
            const uint32_t old = atomicCAS(&lv[h & mask], 0u, e + 1u);
            if (old == 0u) return true;
            if (old == e + 1u) return false;
        }
        return false;
    };
    uint32_t count = 0, pushed = 0, first_open = 0;
    // ROWS_SPARSE: S is bounded where pgvector's candidate heap is not.  A key that does not enter S, or falls off its end
    // unexpanded, is lost for good only when it is as near as the furthest of W -- then the heap would still expand it (c.dist >
    // f.dist is what ends the search).  Sparse rows make that common: every pair without a common index has inner product 0.
    // Such a loss is reported (HB_ERR_CANDIDATES) and hnsw_build runs the build again with a longer S.  cur_ef: the beam of the
    // layer search in progress
    uint32_t cur_ef = 1;
    bool lost = false;
    uint32_t live_pushed = 0, popped = 0;                                     // VAC: the live elements among `pushed`; entries W lost
    // entries of W: min(pushed, ef); VAC: every live push beyond ef took the furthest entry, deleted or live, off W
    auto w_len = [&](uint32_t ef_) -> uint32_t {
        if constexpr (VAC) return pushed - popped;
        else return pushed < ef_ ? pushed : ef_;
    };
    auto as_near_as_w = [&](uint64_t key) -> bool {
        const uint32_t wl = w_len(cur_ef);
        return mono_to_float((uint32_t) (key >> 32)) <= mono_to_float((uint32_t) (S[(wl < count ? wl : count) - 1] >> 32));
    };
    auto insert = [&](uint64_t key) {
        uint32_t lo = 0, hi = count;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S[mid] < key) lo = mid + 1; else hi = mid;
        }
        const uint32_t pos = lo;
        if constexpr (ROWS == ROWS_SPARSE || VAC) {
            if (pos >= p.caps) lost |= as_near_as_w(key);
            else if (count == p.caps && X[p.caps - 1] == 0) lost |= as_near_as_w(S[p.caps - 1]);
        }
        if (pos >= p.caps) return;
        const uint32_t last = count < p.caps ? count : p.caps - 1;
        for (int64_t base = (int64_t) ((last - 1) & ~63u); last > pos && base >= (int64_t) (pos & ~63u); base -= 64) {
            const uint32_t i = (uint32_t) base + (uint32_t) lane;
            const bool mv = i >= pos && i < last;
            const uint64_t kk = mv ? S[i] : 0;
            const uint8_t xx = mv ? X[i] : 0;
            wave_sync();
            if (mv) { S[i + 1] = kk; X[i + 1] = xx; }
            wave_sync();
        }
        if (lane == 0) { S[pos] = key; X[pos] = 0; }
        if (count < p.caps) ++count;
        if (pos < first_open) first_open = pos;
        wave_sync();
    };
    // HnswSearchLayer (hnswutils.c:813-976) on layer lc with beam ef_: S holds the entry points on entry, W on exit
    auto search_layer = [&](int lc, uint32_t ef_) {
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        cur_ef = ef_;
        clear_visited();
        for (uint32_t i = (uint32_t) lane; i < count; i += 64) (void) visit((uint32_t) S[i]);
        used = count;
        pushed = count;
        first_open = 0;
        if constexpr (VAC) {                                                  // the entry points' live count
            live_pushed = 0;
            popped = 0;
            for (uint32_t base = 0; base < count; base += 64) {
                const uint32_t i = base + (uint32_t) lane;
                live_pushed += (uint32_t) __popcll(__ballot(i < count && v.live[(uint32_t) S[i]] != 0));
            }
        }
        wave_sync();
        for (;;) {
            uint32_t cpos = 0xFFFFFFFFu;
            for (uint32_t base = first_open & ~63u; base < count && cpos == 0xFFFFFFFFu; base += 64) {
                const uint32_t i = base + (uint32_t) lane;
                const uint64_t mk = __ballot(i < count && i >= first_open && X[i] == 0);
                if (mk) cpos = base + (uint32_t) __ffsll((unsigned long long) mk) - 1;
            }
            if (cpos == 0xFFFFFFFFu) break;
            first_open = cpos + 1;
            const uint64_t ckey = S[cpos];
            const uint32_t wl = w_len(ef_);
            const uint64_t fkey = S[(wl < count ? wl : count) - 1];
            if (mono_to_float((uint32_t) (ckey >> 32)) > mono_to_float((uint32_t) (fkey >> 32))) break;
            if (lane == 0) X[cpos] = 1;
            const uint32_t ce = (uint32_t) ckey;
            float* dl;
            const int32_t* nl = hb_list(p, ce, lc, &dl);
            int cnt = 0;
            for (uint32_t j0 = 0; j0 < lm; j0 += 64) {
                const uint32_t j = j0 + (uint32_t) lane;
                const int32_t my = j < lm ? nl[j] : -1;
                const bool fresh = my >= 0 && visit((uint32_t) my);
                const uint64_t fm = __ballot(fresh);
                if (fresh) nb[cnt + __popcll(fm & ((1ull << lane) - 1ull))] = my;
                cnt += __popcll(fm);
                wave_sync();
            }
            used += (uint32_t) cnt;
            if (used * 4u > p.hash_slots * 3u) { overflow = true; break; }
            if (cnt == 0) continue;
            hb_distances<IND, ROWS>(p, q, nb, cnt, nd, lane, &left);
            for (int i = 0; i < cnt; ++i) {
                const uint32_t e = (uint32_t) nb[i];
                const float ed = nd[i];
                bool always_;
                if constexpr (VAC) always_ = live_pushed < ef_; else always_ = pushed < ef_;
                const bool always = always_;
                const uint32_t wl2 = w_len(ef_);
                const float fd = mono_to_float((uint32_t) (S[(wl2 < count ? wl2 : count) - 1] >> 32));
                if (!(ed < fd || always)) continue;
                insert(make_key(ed, e));
                ++pushed;
                if constexpr (VAC) {
                    if (v.live[e] != 0 && ++live_pushed > ef_) ++popped;
                    lost |= w_len(ef_) > p.caps;                              // W no longer fits S
                }
            }
        }
        const uint32_t wl = w_len(ef_);
        count = wl < count ? wl : count;
    };

    // HnswFindElementNeighbors (hnswutils.c:1270-1346)
    if (lane == 0) nb[0] = entry;
    wave_sync();
    hb_distances<IND, ROWS>(p, q, nb, 1, nd, lane, &left);
    insert(make_key(nd[0], (uint32_t) entry));
    for (int lc = entry_level; lc >= my_level + 1; --lc) {
        search_layer(lc, 1);
        if (lane == 0)
            for (uint32_t i = 0; i < count; ++i) X[i] = 0;
        wave_sync();
    }
    for (int lc = my_level < entry_level ? my_level : entry_level; lc >= 0; --lc) {
        search_layer(lc, p.efc);
        const int lm = (int) (lc == 0 ? 2 * p.m : p.m);
        int pruned;
        const uint64_t* C = S;                                                // the candidates of the selection, nearest first
        int nc = (int) count;
        if constexpr (VAC) {                                                  // RemoveElements: without the deleted ones and `me`, order kept
            nc = 0;
            for (uint32_t base = 0; base < count; base += 64) {
                const uint32_t i = base + (uint32_t) lane;
                const uint64_t kk = i < count ? S[i] : 0;
                const bool keep = i < count && (uint32_t) kk != me && v.live[(uint32_t) kk] != 0;
                const uint64_t km = __ballot(keep);
                const uint32_t at = (uint32_t) nc + (uint32_t) __popcll(km & ((1ull << lane) - 1ull));
                if (keep && at < tcap) T[at] = kk;
                nc += __popcll(km);
            }
            if ((uint32_t) nc > tcap) {                                       // more live candidates than the table's bytes hold: a larger table
                overflow = true;
                nc = (int) tcap;
            }
            wave_sync();
            C = T;
        }
        const int ns = hb_select<IND, ROWS>(p, C, nc, lm, sel, wd, nb, nd, &pruned, lane, &left);
        // AddConnections + the reverse edges HnswUpdateNeighborsInMemory will apply
        float* dl;
        int32_t* nl = own_list(lc, &dl);
        uint32_t base = 0;
        if (lane == 0 && ns > 0 && !defer) base = atomicAdd(p.rec_count, (uint32_t) ns);
        base = (uint32_t) __shfl((int) base, 0);
        for (int j = lane; j < ns; j += 64) {
            const uint64_t key = C[sel[j]];
            nl[j] = (int32_t) (uint32_t) key;
            dl[j] = mono_to_float((uint32_t) (key >> 32));
            if (!defer && base + (uint32_t) j < p.rec_cap) {
                // slots are claimed in wave arrival order; the sort key carries the index in the batch (< 4096 = 2^HB_SRC_BITS),
                // so that a (layer, target) run comes out in ascending source element whatever the arrival order was
                p.rec_key[base + j] = ((uint64_t) (uint32_t) lc << (32 + HB_SRC_BITS)) | ((uint64_t) (uint32_t) key << HB_SRC_BITS) | bi;
                p.rec_val[base + j] = ((uint64_t) me << 32) | __float_as_uint(mono_to_float((uint32_t) (key >> 32)));
            }
        }
        if (!defer && lane == 0 && ns > 0 && base + (uint32_t) ns > p.rec_cap) atomicOr(p.err, HB_ERR_RECORDS);   // (cannot happen: the host sizes rec_cap from the levels)
        if (lane == 0)
            for (uint32_t i = 0; i < count; ++i) X[i] = 0;                    // W is the next layer's entry set
        wave_sync();
    }
    if constexpr (defer) {
        {
            // mixed attempt: a repair that outgrew its arrays leaves no record and no guard bit, only its batch index -- the spill
            // launch redoes it from scratch, staged lists included; one that fit emits the records of its staged lists now (each
            // lane reads back what it stored itself; the lists are packed, so their lengths are the counts of the selections)
            if (overflow || lost) {
                if (lane == 0) v.spill_list[atomicAdd(v.spill_count, 1u)] = (int32_t) bi;
                return;
            }
            for (int lc = my_level; lc >= 0; --lc) {
                float* dl;
                const int32_t* nl = own_list(lc, &dl);
                const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
                uint32_t ns = 0;
                for (uint32_t j0 = 0; j0 < lm; j0 += 64) ns += (uint32_t) __popcll(__ballot(j0 + (uint32_t) lane < lm && nl[j0 + (uint32_t) lane] >= 0));
                if (ns == 0) continue;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(p.rec_count, ns);
                base = (uint32_t) __shfl((int) base, 0);
                for (uint32_t j = (uint32_t) lane; j < ns; j += 64) {
                    if (base + j < p.rec_cap) {
                        p.rec_key[base + j] = ((uint64_t) (uint32_t) lc << (32 + HB_SRC_BITS)) | ((uint64_t) (uint32_t) nl[j] << HB_SRC_BITS) | bi;
                        p.rec_val[base + j] = ((uint64_t) me << 32) | __float_as_uint(dl[j]);
                    }
                }
                if (lane == 0 && base + ns > p.rec_cap) atomicOr(p.err, HB_ERR_RECORDS);
            }
            return;
        }
    }
    if (overflow && lane == 0) atomicOr(p.err, HB_ERR_VISITED);
    if constexpr (ROWS == ROWS_SPARSE || VAC)
        if (lost && lane == 0) atomicOr(p.err, HB_ERR_CANDIDATES);
}

template <bool IND, int ROWS>
__global__ __launch_bounds__(256) void hnsw_build_search_kernel(const HnswBuildParams p)
{
    hb_search_body<IND, ROWS, false>(p, HnswVacuumParams{});
}

// the forest form (vsr_hnsw_build_partitions): an instantiation of its own, so that the build's compiles as it did
template <int ROWS>
__global__ __launch_bounds__(256) void hnsw_forest_search_kernel(const HnswBuildParams p, const HnswForestParams f)
{
    hb_search_body<true, ROWS, false, false, true>(p, HnswVacuumParams{}, f);
}

template <bool IND, int ROWS, bool MIXED>
__global__ __launch_bounds__(256) void hnsw_vacuum_search_kernel(const HnswBuildParams p, const HnswVacuumParams v)
{
    hb_search_body<IND, ROWS, true, MIXED>(p, v);
}

// ---- the spill form of the repair (vsr_hnsw_vacuum): the algorithm of hb_search_body<.., VAC = true> with everything that grows
// with the working set in a per-wave workspace in GLOBAL memory (HnswVacuumParams::spill_ws), for repairs whose working set no
// LDS holds.  An element is visited once and pushed once in a layer search, so arrays of n_elem entries cannot overflow: this
// form has no ladder and sets neither HB_ERR_VISITED nor HB_ERR_CANDIDATES.
// The sorted array S of the LDS form is pgvector's two heaps here (hnswutils.c:813-976): C, a binary min-heap of everything pushed
// and not yet expanded, and W, a binary max-heap of the nearest pushed - popped entries, both on (distance, id) keys, which are
// distinct, so what a pop returns does not depend on the heaps' inner order.  "first open entry of S" is C's top, "S[wl - 1]" is
// W's top, a live push beyond ef pops W.  A shifting insert into a sorted array of thousands of entries would cost count / 64
// dependent round trips to memory per push; a heap operation costs at most log2(count), and only lane 0 touches the heaps, so they
// need no ordering between lanes.  Between layers W is copied to C and C is sorted by the whole wave (bitonic, in place): a sorted
// array is a min-heap, and it is W nearest first, which RemoveElements filters into T for hb_select.
// Visited set: an exact bitmap of n_elem bits, set with atomicOr, cleared before every layer search -- so nothing of the previous
// layer or of the previous repair in this workspace is left.  Stores of one lane that other lanes load (the copy, the sort, T)
// are ordered with wave_sync_global(): wave_sync()'s wavefront scope orders LDS only.
template <bool MAX>
__device__ __forceinline__ void hs_heap_push(uint64_t* H, uint32_t& n, const uint64_t key)
{
    uint32_t i = n++;
    while (i > 0) {
        const uint32_t up = (i - 1) >> 1;
        const uint64_t uk = H[up];
        if (MAX ? uk >= key : uk <= key) break;
        H[i] = uk;
        i = up;
    }
    H[i] = key;
}

// removes the top (n >= 1)
template <bool MAX>
__device__ __forceinline__ void hs_heap_pop(uint64_t* H, uint32_t& n)
{
    const uint64_t key = H[--n];
    uint32_t i = 0;
    for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= n) break;
        uint64_t ck = H[c];
        if (c + 1 < n) {
            const uint64_t c2 = H[c + 1];
            if (MAX ? c2 > ck : c2 < ck) { ck = c2; ++c; }
        }
        if (MAX ? key >= ck : key <= ck) break;
        H[i] = ck;
        i = c;
    }
    H[i] = key;                                                               // (n == 0: H[0] again, harmless)
}

// one repair: batch element bi in workspace ws; nb, nd, sel: the wave's HB_NBR arrays in LDS
template <bool IND, int ROWS>
__device__ __forceinline__ void hb_spill_repair(const HnswBuildParams& p, const HnswVacuumParams& v, const uint32_t bi, unsigned char* ws,
                                                int32_t* nb, float* nd, int32_t* sel, const int lane)
{
    const uint32_t n = v.spill_n, words = (n + 31u) / 32u;
    uint64_t* Cq = reinterpret_cast<uint64_t*>(ws);                           // [n] min-heap: pushed, not expanded
    uint64_t* Wq = Cq + n;                                                    // [n] max-heap: W
    uint64_t* T = Wq + n;                                                     // [n] the selection's candidates
    int32_t*  wd = reinterpret_cast<int32_t*>(T + n);                         // [n] its passed-over candidates
    uint32_t* bm = reinterpret_cast<uint32_t*>(wd + n);                       // [words] visited
    const uint32_t me = (uint32_t) v.elems[bi];
    const float4* q = hb_row<IND>(p, me);
    const int my_level = p.level[me];
    int32_t* st_n = v.stage_nbr + (size_t) bi * v.stage_stride;
    float* st_d = v.stage_dist + (size_t) bi * v.stage_stride;
    for (int lc = 0; lc <= my_level; ++lc) {                                  // the element's staged lists start empty
        const uint32_t at = lc == 0 ? 0u : (uint32_t) (lc + 1) * p.m, lm = lc == 0 ? 2 * p.m : p.m;
        for (uint32_t j = (uint32_t) lane; j < lm; j += 64) { st_n[at + j] = -1; st_d[at + j] = 0.0f; }
    }
    if (p.entry < 0) return;                                                  // nobody else is left

    uint32_t cn = 0, wn = 0;                                                  // entries of C and W (uniform: lane 0 changes them, then shares)
    // HnswSearchLayer: on entry W holds the entry points and C the same keys, sorted; on exit W is the layer's result
    auto search_layer = [&](int lc, uint32_t ef_) {
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        for (uint32_t i = (uint32_t) lane; i < words; i += 64) bm[i] = 0u;
        wave_sync_global();
        uint32_t live_pushed = 0;
        for (uint32_t base = 0; base < cn; base += 64) {
            const uint32_t i = base + (uint32_t) lane;
            const uint32_t e = i < cn ? (uint32_t) Cq[i] : 0u;
            if (i < cn) (void) atomicOr(&bm[e >> 5], 1u << (e & 31u));
            live_pushed += (uint32_t) __popcll(__ballot(i < cn && v.live[e] != 0));
        }
        wave_sync_global();
        for (;;) {
            uint32_t ce = 0xFFFFFFFFu;
            if (lane == 0 && cn > 0) {
                const uint64_t ckey = Cq[0], fkey = Wq[0];
                if (!(mono_to_float((uint32_t) (ckey >> 32)) > mono_to_float((uint32_t) (fkey >> 32)))) {
                    ce = (uint32_t) ckey;
                    hs_heap_pop<false>(Cq, cn);
                }
            }
            ce = (uint32_t) __shfl((int) ce, 0);
            if (ce == 0xFFFFFFFFu) break;                                     // (an element id is below 2^31)
            cn = (uint32_t) __shfl((int) cn, 0);
            float* dl;
            const int32_t* nl = hb_list(p, ce, lc, &dl);
            int cnt = 0;
            for (uint32_t j0 = 0; j0 < lm; j0 += 64) {
                const uint32_t j = j0 + (uint32_t) lane;
                const int32_t my = j < lm ? nl[j] : -1;
                bool fresh = false;
                if (my >= 0) {
                    const uint32_t bit = 1u << ((uint32_t) my & 31u);
                    fresh = (atomicOr(&bm[(uint32_t) my >> 5], bit) & bit) == 0u;
                }
                const uint64_t fm = __ballot(fresh);
                if (fresh) nb[cnt + __popcll(fm & ((1ull << lane) - 1ull))] = my;
                cnt += __popcll(fm);
                wave_sync();
            }
            if (cnt == 0) continue;
            hb_distances<IND, ROWS>(p, q, nb, cnt, nd, lane);
            if (lane == 0) {
                for (int i = 0; i < cnt; ++i) {
                    const uint32_t e = (uint32_t) nb[i];
                    const float ed = nd[i];
                    const bool always = live_pushed < ef_;
                    const float fd = mono_to_float((uint32_t) (Wq[0] >> 32));
                    if (!(ed < fd || always)) continue;
                    const uint64_t key = make_key(ed, e);
                    hs_heap_push<false>(Cq, cn, key);
                    hs_heap_push<true>(Wq, wn, key);
                    if (v.live[e] != 0 && ++live_pushed > ef_) hs_heap_pop<true>(Wq, wn);
                }
            }
            cn = (uint32_t) __shfl((int) cn, 0);
            wn = (uint32_t) __shfl((int) wn, 0);
            live_pushed = (uint32_t) __shfl((int) live_pushed, 0);
        }
        // W becomes the next layer's entry set: C = W, sorted nearest first
        wave_sync_global();
        for (uint32_t i = (uint32_t) lane; i < wn; i += 64) Cq[i] = Wq[i];
        cn = wn;
        wave_sync_global();
        uint32_t n2 = 1, lg = 0;
        while (n2 < cn) { n2 <<= 1; ++lg; }
        for (uint32_t ls = 1; ls <= lg; ++ls) {                               // bitonic: positions >= cn act as +inf and are never touched
            const uint32_t size = 1u << ls, half = size >> 1;
            for (uint32_t tt = (uint32_t) lane; tt < n2 / 2; tt += 64) {
                const uint32_t i = ((tt >> (ls - 1)) << ls) + (tt & (half - 1)), j = i ^ (size - 1);
                if (j < cn) {
                    const uint64_t a = Cq[i], b = Cq[j];
                    if (a > b) { Cq[i] = b; Cq[j] = a; }
                }
            }
            wave_sync_global();
            for (uint32_t ld = ls - 1; ld >= 1; --ld) {
                const uint32_t stride = 1u << (ld - 1);
                for (uint32_t tt = (uint32_t) lane; tt < n2 / 2; tt += 64) {
                    const uint32_t i = ((tt >> (ld - 1)) << ld) + (tt & (stride - 1)), j = i + stride;
                    if (j < cn) {
                        const uint64_t a = Cq[i], b = Cq[j];
                        if (a > b) { Cq[i] = b; Cq[j] = a; }
                    }
                }
                wave_sync_global();
            }
        }
    };

    // HnswFindElementNeighbors, existing = true
    if (lane == 0) nb[0] = p.entry;
    wave_sync();
    hb_distances<IND, ROWS>(p, q, nb, 1, nd, lane);
    if (lane == 0) Cq[0] = Wq[0] = make_key(nd[0], (uint32_t) p.entry);
    cn = wn = 1;
    wave_sync_global();
    for (int lc = p.entry_level; lc >= my_level + 1; --lc) search_layer(lc, 1);
    for (int lc = my_level < p.entry_level ? my_level : p.entry_level; lc >= 0; --lc) {
        search_layer(lc, p.efc);
        const int lm = (int) (lc == 0 ? 2 * p.m : p.m);
        int nc = 0;                                                           // RemoveElements: without the deleted ones and `me`, order kept
        for (uint32_t base = 0; base < cn; base += 64) {
            const uint32_t i = base + (uint32_t) lane;
            const uint64_t kk = i < cn ? Cq[i] : 0;
            const bool keep = i < cn && (uint32_t) kk != me && v.live[(uint32_t) kk] != 0;
            const uint64_t km = __ballot(keep);
            if (keep) T[(uint32_t) nc + (uint32_t) __popcll(km & ((1ull << lane) - 1ull))] = kk;
            nc += __popcll(km);
        }
        wave_sync_global();
        int pruned;
        const int ns = hb_select<IND, ROWS>(p, T, nc, lm, sel, wd, nb, nd, &pruned, lane);
        const uint32_t at = lc == 0 ? 0u : (uint32_t) (lc + 1) * p.m;
        uint32_t base = 0;
        if (lane == 0 && ns > 0) base = atomicAdd(p.rec_count, (uint32_t) ns);
        base = (uint32_t) __shfl((int) base, 0);
        for (int j = lane; j < ns; j += 64) {
            const uint64_t key = T[sel[j]];
            st_n[at + j] = (int32_t) (uint32_t) key;
            st_d[at + j] = mono_to_float((uint32_t) (key >> 32));
            if (base + (uint32_t) j < p.rec_cap) {
                p.rec_key[base + j] = ((uint64_t) (uint32_t) lc << (32 + HB_SRC_BITS)) | ((uint64_t) (uint32_t) key << HB_SRC_BITS) | bi;
                p.rec_val[base + j] = ((uint64_t) me << 32) | __float_as_uint(mono_to_float((uint32_t) (key >> 32)));
            }
        }
        if (lane == 0 && ns > 0 && base + (uint32_t) ns > p.rec_cap) atomicOr(p.err, HB_ERR_RECORDS);
        wave_sync();
    }
}

// one wave per workspace: wave w redoes spilled repairs w, w + spill_pool, .. of the batch (a static stride: which workspace a repair
// gets depends on the order the LDS launch listed them in, its result does not)
template <bool IND, int ROWS>
__global__ __launch_bounds__(256) void hnsw_vacuum_search_spill_kernel(const HnswBuildParams p, const HnswVacuumParams v)
{
    __shared__ __align__(16) int32_t nb_all[4][HB_NBR];
    __shared__ __align__(16) float nd_all[4][HB_NBR];
    __shared__ __align__(16) int32_t sel_all[4][HB_NBR];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint32_t w = blockIdx.x * 4 + wave;
    if (w >= v.spill_pool) return;                                            // (waves are independent: no workgroup barrier)
    uint32_t todo = p.count;
    if (!v.spill_all) {
        todo = *v.spill_count;
        if (todo > p.count) todo = p.count;
    }
    if (w == 0 && lane == 0 && todo > 0) atomicAdd(v.spill_total, todo);
    unsigned char* ws = v.spill_ws + (size_t) w * v.spill_ws_bytes;
    for (uint32_t t = w; t < todo; t += v.spill_pool) {
        const uint32_t bi = v.spill_all ? t : (uint32_t) v.spill_list[t];
        hb_spill_repair<IND, ROWS>(p, v, bi, ws, nb_all[wave], nd_all[wave], sel_all[wave], lane);
        wave_sync_global();
    }
}

// ---- phase 2: reverse edges, sorted by (layer, target, source): the wave of a run's first record applies the whole
// (layer, target) run, sources in ascending element id ----
// VAC (vsr_hnsw_vacuum): UpdateNeighborOnDisk's cases come first (hnswinsert.c:470-560): a source the list names already is
// skipped, a list that is not full takes it at its end, a full list that names a deleted element (live[] == 0) gives the first such
// slot away (LoadElementsForInsert); only then HnswUpdateConnection's re-selection
template <bool IND, int ROWS, bool VAC>
__device__ __forceinline__ void hb_link_body(const HnswBuildParams& p, const int32_t* __restrict__ live)
{
    extern __shared__ __align__(16) unsigned char smem_all[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint32_t ri = blockIdx.x * 4 + wave;
    const uint32_t n_rec = *p.rec_count < p.rec_cap ? *p.rec_count : p.rec_cap;
    if (ri >= n_rec) return;
    const uint64_t key = p.rec_key[ri] >> HB_SRC_BITS;                        // (layer, target)
    if (ri > 0 && (p.rec_key[ri - 1] >> HB_SRC_BITS) == key) return;          // not the first of its run
    const int lc = (int) (key >> 32);
    const uint32_t owner = (uint32_t) key;
    const int lm = (int) (lc == 0 ? 2 * p.m : p.m);
    unsigned char* smem = smem_all + (size_t) wave * (HB_NBR * 32);
    SparseLeft left;                                                          // ROWS_SPARSE: the waves' left-hand tables lie behind the four lists
    if constexpr (ROWS == ROWS_SPARSE) {
        left.tab = reinterpret_cast<uint64_t*>(smem_all + (size_t) 4 * (HB_NBR * 32) + (size_t) wave * p.sp_slots * 8);
        left.slots = p.sp_slots;
    }
    uint64_t* cand = reinterpret_cast<uint64_t*>(smem);                       // [lm + 1] (distance, element), sorted
    int32_t*  sel = reinterpret_cast<int32_t*>(cand + HB_NBR);
    int32_t*  wd = sel + HB_NBR;
    int32_t*  ids = wd + HB_NBR;
    float*    nd = reinterpret_cast<float*>(ids + HB_NBR);
    float* dl;
    int32_t* nl = hb_list(p, owner, lc, &dl);
    for (uint32_t r = ri; r < n_rec && (p.rec_key[r] >> HB_SRC_BITS) == key; ++r) {   // HnswUpdateConnection, one after another
        const uint32_t e = (uint32_t) (p.rec_val[r] >> 32);
        const float de = __uint_as_float((uint32_t) p.rec_val[r]);
        int dead_at = 0x7FFFFFFF;                                             // VAC: the first slot that names a deleted element
        if constexpr (VAC) {
            bool has = false;
            for (int j = lane; j < lm; j += 64) {
                const int32_t id = nl[j];
                has |= id == (int32_t) e;
                if (id >= 0 && live[id] == 0 && j < dead_at) dead_at = j;
            }
            if (__ballot(has) != 0) continue;
            for (int mm = 32; mm >= 1; mm >>= 1) {
                const int o = __shfl_xor(dead_at, mm);
                dead_at = o < dead_at ? o : dead_at;
            }
        }
        // current length of the list (-1 padded)
        int len = 0;
        for (int j0 = 0; j0 < lm; j0 += 64) {
            const int j = j0 + lane;
            len += __popcll(__ballot(j < lm && nl[j] >= 0));
        }
        if (len < lm) {
            if (lane == 0) { nl[len] = (int32_t) e; dl[len] = de; }
            wave_sync();
            continue;
        }
        if constexpr (VAC) {
            if (dead_at < lm) {
                if (lane == 0) { nl[dead_at] = (int32_t) e; dl[dead_at] = de; }
                wave_sync();
                continue;
            }
        }
        // full: the list and the new element, nearest first (ties: the lower element id first, the order list_sort leaves
        // with CompareCandidateDistances read from the tail)
        for (int j = lane; j < lm; j += 64) cand[j] = make_key(dl[j], (uint32_t) nl[j]);
        if (lane == 0) cand[lm] = make_key(de, e);
        wave_sync();
        const int n = lm + 1;
        for (int j = lane; j < n; j += 64) {                                  // rank sort: n <= 201
            const uint64_t kk = cand[j];
            int rank = 0;
            for (int t = 0; t < n; ++t) rank += cand[t] < kk || (cand[t] == kk && t < j);
            sel[j] = rank;
        }
        wave_sync();
        uint64_t mine[4];
        int nm = 0;
        for (int j = lane; j < n; j += 64) mine[nm++] = cand[j];
        wave_sync();
        nm = 0;
        for (int j = lane; j < n; j += 64) cand[sel[j]] = mine[nm++];
        wave_sync();
        int pruned;
        (void) hb_select<IND, ROWS>(p, cand, n, lm, sel, wd, ids, nd, &pruned, lane, &left);
        const uint32_t pe = (uint32_t) cand[pruned];
        if (pe != e) {                                                        // the new element replaces the pruned one
            for (int j = lane; j < lm; j += 64)
                if ((uint32_t) nl[j] == pe) { nl[j] = (int32_t) e; dl[j] = de; }
        }
        wave_sync();
    }
}

template <bool IND, int ROWS>
__global__ __launch_bounds__(256) void hnsw_build_link_kernel(const HnswBuildParams p)
{
    hb_link_body<IND, ROWS, false>(p, nullptr);
}

template <bool IND, int ROWS>
__global__ __launch_bounds__(256) void hnsw_vacuum_link_kernel(const HnswBuildParams p, const int32_t* __restrict__ live)
{
    hb_link_body<IND, ROWS, true>(p, live);
}

// ---- vacuum (vsr_hnsw_vacuum): the small kernels around the two repair forms above ----
// the staged lists of a batch become the elements' lists: after every search of the batch has ended, before the link kernel.
// One wave per batch element
__global__ __launch_bounds__(256) void hnsw_vacuum_install_kernel(const HnswBuildParams p, const HnswVacuumParams v)
{
    const int lane = threadIdx.x & 63;
    const uint32_t bi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bi >= p.count) return;
    const uint32_t me = (uint32_t) v.elems[bi];
    const int my_level = p.level[me];
    for (int lc = 0; lc <= my_level; ++lc) {
        float* dl;
        int32_t* nl = hb_list(p, me, lc, &dl);
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        const size_t at = (size_t) bi * v.stage_stride + (lc == 0 ? 0u : (uint32_t) (lc + 1) * p.m);
        for (uint32_t j = (uint32_t) lane; j < lm; j += 64) { nl[j] = v.stage_nbr[at + j]; dl[j] = v.stage_dist[at + j]; }
    }
}

// NeedsUpdated (hnswvacuum.c:190-235): flag[e] = 1 when live element e (other than `skip`, the entry point; -1: none) has a list that
// names a deleted element, or a layer-0 list that is not full.  Lists are packed: the first -1 ends one.  One thread per element
__global__ __launch_bounds__(256) void hnsw_vacuum_mark_kernel(const HnswBuildParams p, const int32_t* __restrict__ live, const uint32_t n_elem,
                                                               const int32_t skip, uint8_t* __restrict__ flag)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n_elem) return;
    uint8_t f = 0;
    if (live[e] != 0 && (int32_t) e != skip) {
        const int my_level = p.level[e];
        for (int lc = 0; lc <= my_level; ++lc) {
            float* dl;
            const int32_t* nl = hb_list(p, e, lc, &dl);
            const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
            uint32_t j = 0;
            for (; j < lm; ++j) {
                const int32_t id = nl[j];
                if (id < 0) break;
                if (live[id] == 0) f = 1;
            }
            if (lc == 0 && j < lm) f = 1;
        }
    }
    flag[e] = f;
}

// pass 3: the lists of the live elements into the compacted arrays, ids through map[] (the exclusive scan of live[]), upper slots
// through slot_map[], the upper arrays at the new graph's max_level.  A list of a live element that still names a deleted one would
// be a fault of the repair: HB_ERR_RECORDS, never a thinner list in silence.  One wave per element
__global__ __launch_bounds__(256) void hnsw_vacuum_renumber_kernel(const HnswBuildParams p, const int32_t* __restrict__ live,
                                                                   const int32_t* __restrict__ map, const int32_t* __restrict__ slot_map,
                                                                   const uint32_t n_elem, int32_t* __restrict__ new_nbr0,
                                                                   int32_t* __restrict__ new_up_nbr, const uint32_t new_max_level)
{
    const int lane = threadIdx.x & 63;
    const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_elem || live[e] == 0) return;
    const uint32_t ne = (uint32_t) map[e];
    const int my_level = p.level[e];                                          // (<= new_max_level: the new entry is on the top live level)
    bool bad = false;
    for (int lc = 0; lc <= my_level && lc <= (int) new_max_level; ++lc) {
        float* dl;
        const int32_t* nl = hb_list(p, e, lc, &dl);
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        int32_t* out = lc == 0 ? new_nbr0 + (size_t) ne * 2 * p.m
                               : new_up_nbr + ((size_t) slot_map[p.up_slot[e]] * new_max_level + (uint32_t) (lc - 1)) * p.m;
        for (uint32_t j = (uint32_t) lane; j < lm; j += 64) {
            const int32_t id = nl[j];
            bad |= id >= 0 && live[id] == 0;
            out[j] = id >= 0 && live[id] != 0 ? map[id] : -1;
        }
    }
    if (bad) atomicOr(p.err, HB_ERR_RECORDS);
}

// ---- extension (vsr_hnsw_extend): the per-edge distances of a graph that arrived without them.  One wave per (element, layer)
// list of the prior graph: lists 0 .. n_prior - 1 are the layer-0 lists, the rest (slot, layer) pairs of the upper arrays, whose
// owner comes from up_owner[slot] (-1: a slot no element names).  The ids go to the wave's LDS, hb_distances takes the owner's row
// as the left operand, and the rank values land where phase 1 and the link kernel would have left them.  Every id the gather goes
// through has been bounded before this launch: by the host for arrays that came from a caller (hnsw_extend_prepare,
// vsr_hnsw_build_rt.hip), by hnsw_forest_join_kernel for the prior indexes of vsr_hnsw_extend_partitions, which stay on the device
// (ids into [base, base + n_elem) of their graph, rows into the corpus, slots into the graph's own).  Waves are independent: no
// workgroup barrier ----
template <bool IND, int ROWS>
__global__ __launch_bounds__(256) void hnsw_edge_dist_kernel(const HnswBuildParams p, const uint32_t n_prior, const int32_t* __restrict__ up_owner,
                                                             const uint32_t n_upper_prior)
{
    __shared__ __align__(16) int32_t ids_all[4][HB_NBR];
    __shared__ __align__(16) float nd_all[4][HB_NBR];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint64_t li = (uint64_t) blockIdx.x * 4 + wave;
    uint32_t e;
    int lc = 0;
    if (li < n_prior) {
        e = (uint32_t) li;
    } else {
        const uint64_t u = li - n_prior, slot = u / p.max_level;
        if (slot >= n_upper_prior) return;
        const int32_t owner = up_owner[slot];
        lc = (int) (u % p.max_level) + 1;
        if (owner < 0 || lc > p.level[owner]) return;
        e = (uint32_t) owner;
    }
    int32_t* ids = ids_all[wave];
    float* nd = nd_all[wave];
    const uint32_t lm = lc == 0 ? 2 * p.m : p.m;                              // (<= 200 < HB_NBR)
    float* dl;
    const int32_t* nl = hb_list(p, e, lc, &dl);
    int cnt = 0;
    bool open = true;                                                         // the valid prefix: lists are packed
    for (uint32_t j0 = 0; j0 < lm; j0 += 64) {
        const uint32_t j = j0 + (uint32_t) lane;
        const int32_t my = j < lm ? nl[j] : -1;
        ids[j] = my;
        const uint64_t gap = __ballot(my < 0);
        if (open) {
            if (gap == 0) cnt += 64;
            else { cnt += __ffsll((unsigned long long) gap) - 1; open = false; }
        }
    }
    wave_sync();
    if (cnt == 0) return;
    hb_distances<IND, ROWS>(p, hb_row<IND>(p, e), ids, cnt, nd, lane);
    for (int j = lane; j < cnt; j += 64) dl[j] = mono_to_float(mono_bits(nd[j]));   // as a key carries it (-0 -> +0)
}

// ---- partitions (vsr_hnsw_build_partitions): every graph's own arrays out of the global ones.  One wave per global element e; its
// graph is the last one whose base is <= e (graphs[] holds the non-empty graphs in ascending base).  Ids lose the graph's base,
// upper slots its slot_base (slots were numbered in global element order, so a graph's are a run), the upper lists go from the
// global stride p.max_level to the graph's own max_level (layers above an element's level hold -1 in both), and the element's
// one heap TID is its row.  CARRY (vsr_hnsw_extend_partitions): the graph's first priors[].n_elem elements keep the heap TIDs of the
// prior index, count and list; priors is not read without it.  Waves are independent: no workgroup barrier ----
template <bool CARRY>
__global__ __launch_bounds__(256) void hnsw_forest_split_kernel(const HnswBuildParams p, const HnswForestGraph* __restrict__ graphs,
                                                                const uint32_t n_graphs, const uint32_t n_total,
                                                                const HnswForestPrior* __restrict__ priors)
{
    const int lane = threadIdx.x & 63;
    const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_total) return;
    uint32_t lo = 0, hi = n_graphs;                                           // graphs[lo].base <= e < graphs[hi].base
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t) graphs[mid].base <= e) lo = mid; else hi = mid;
    }
    const HnswForestGraph g = graphs[lo];
    const uint32_t le = e - (uint32_t) g.base;
    if (le >= (uint32_t) g.n_elem) return;                                    // (cannot happen: the graphs cover 0 .. n_total - 1)
    const int32_t row = p.elem_row[e], slot = p.up_slot[e];
    int32_t tid_count = 1, tid = lane == 0 ? row : -1;
    if (CARRY) {
        const HnswForestPrior pr = priors[lo];
        if (le < (uint32_t) pr.n_elem) {
            tid_count = min(max(pr.tid_count[le], 1), HB_TIDS);
            tid = lane < tid_count ? pr.tids[(size_t) le * HB_TIDS + lane] : -1;
        }
    }
    if (lane == 0) {
        g.level[le] = p.level[e];
        g.elem_row[le] = row;
        g.up_slot[le] = slot >= 0 ? slot - g.slot_base : -1;
        g.tid_count[le] = tid_count;
    }
    if (lane < HB_TIDS) g.tids[(size_t) le * HB_TIDS + lane] = tid;
    for (uint32_t j = (uint32_t) lane; j < 2 * p.m; j += 64) {
        const int32_t id = p.nbr0[(size_t) e * 2 * p.m + j];
        g.nbr0[(size_t) le * 2 * p.m + j] = id >= 0 ? id - g.base : -1;
    }
    if (slot < 0) return;
    const size_t from = (size_t) slot * p.max_level * p.m, to = (size_t) (slot - g.slot_base) * (uint32_t) g.max_level * p.m;
    for (uint32_t j = (uint32_t) lane; j < (uint32_t) g.max_level * p.m; j += 64) {   // (g.max_level <= p.max_level)
        const int32_t id = p.up_nbr[from + j];
        g.up_nbr[to + j] = id >= 0 ? id - g.base : -1;
    }
}

// the graph of global element e: the last one whose base is <= e (graphs[] ascends in base and covers 0 .. n_total - 1)
__device__ __forceinline__ uint32_t hb_forest_graph_of(const HnswForestGraph* __restrict__ graphs, uint32_t n_graphs, uint32_t e)
{
    uint32_t lo = 0, hi = n_graphs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t) graphs[mid].base <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- partitions that exist already (vsr_hnsw_extend_partitions): the split's inverse.  One wave per global element e; only the
// first priors[].n_elem elements of a graph have anything to bring, the rest are the rows to insert and were written by the host.
// Ids gain the graph's base, upper slots its slot_base, the upper lists go from the prior's own stride to the global one (the
// layers above it were filled with -1), and the slot's owner is noted for the edge-distance launch.  Every value read from a prior
// array is bounded before it becomes an address, here or in a later launch: an element with a value out of range is joined as a
// level-0 element of row 0 without edges and j.bad takes its graph's index.  Waves are independent: no workgroup barrier ----
__global__ __launch_bounds__(256) void hnsw_forest_join_kernel(const HnswBuildParams p, const HnswForestJoin j,
                                                               const HnswForestGraph* __restrict__ graphs,
                                                               const HnswForestPrior* __restrict__ priors, const uint32_t n_graphs,
                                                               const uint32_t n_total)
{
    const int lane = threadIdx.x & 63;
    const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_total) return;
    const uint32_t gi = hb_forest_graph_of(graphs, n_graphs, e);
    const HnswForestGraph g = graphs[gi];
    const HnswForestPrior pr = priors[gi];
    const uint32_t le = e - (uint32_t) g.base;
    if (le >= (uint32_t) pr.n_elem || le >= (uint32_t) g.n_elem) return;
    int32_t lev = pr.level[le], slot = pr.up_slot[le], row = pr.elem_row[le];
    const bool ok = lev >= 0 && lev <= pr.max_level && (uint32_t) pr.max_level <= p.max_level && row >= 0 && (uint32_t) row < j.n_rows &&
                    (lev >= 1 ? slot >= 0 && slot < pr.n_upper : slot == -1);
    bool bad = !ok;
    if (!ok) { lev = 0; slot = -1; row = 0; }
    if (lane == 0) {
        j.level[e] = lev;
        j.elem_row[e] = row;
        j.up_slot[e] = slot >= 0 ? slot + g.slot_base : -1;
        if (slot >= 0) j.up_owner[slot + g.slot_base] = (int32_t) e;
    }
    if (ok) {
        for (uint32_t i = (uint32_t) lane; i < 2 * p.m; i += 64) {
            const int32_t id = pr.nbr0[(size_t) le * 2 * p.m + i];
            bad |= id < -1 || id >= pr.n_elem;
            p.nbr0[(size_t) e * 2 * p.m + i] = id >= 0 && id < pr.n_elem ? id + g.base : -1;
        }
        if (slot >= 0) {
            const size_t from = (size_t) slot * (uint32_t) pr.max_level * p.m, to = (size_t) (slot + g.slot_base) * p.max_level * p.m;
            for (uint32_t i = (uint32_t) lane; i < (uint32_t) pr.max_level * p.m; i += 64) {   // (pr.max_level <= p.max_level: checked above)
                const int32_t id = pr.up_nbr[from + i];
                bad |= id < -1 || id >= pr.n_elem;
                p.up_nbr[to + i] = id >= 0 && id < pr.n_elem ? id + g.base : -1;
            }
        }
    }
    if (bad) atomicMin(j.bad, gi);
}

// "already held": one thread per prior element; each of its heap TIDs is looked up among the graph's new rows, which lie ascending in
// p.elem_row behind the prior elements.  The least (graph, row) found stays in j.held
__global__ __launch_bounds__(256) void hnsw_forest_held_kernel(const HnswBuildParams p, const HnswForestJoin j,
                                                               const HnswForestGraph* __restrict__ graphs,
                                                               const HnswForestPrior* __restrict__ priors, const uint32_t n_graphs,
                                                               const uint32_t n_total)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_total) return;
    const uint32_t gi = hb_forest_graph_of(graphs, n_graphs, e);
    const HnswForestGraph g = graphs[gi];
    const HnswForestPrior pr = priors[gi];
    const uint32_t le = e - (uint32_t) g.base;
    if (le >= (uint32_t) pr.n_elem || le >= (uint32_t) g.n_elem) return;
    const int32_t* fresh = p.elem_row + (size_t) g.base + (uint32_t) pr.n_elem;
    const uint32_t n_fresh = (uint32_t) (g.n_elem - pr.n_elem);
    const int cnt = min(max(pr.tid_count[le], 0), HB_TIDS);
    for (int t = 0; t < cnt; ++t) {
        const int32_t row = pr.tids[(size_t) le * HB_TIDS + t];
        uint32_t lo = 0, hi = n_fresh;                                        // the first new row >= row
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (fresh[mid] < row) lo = mid + 1; else hi = mid;
        }
        if (lo < n_fresh && fresh[lo] == row && row >= 0) atomicMin(j.held, ((unsigned long long) gi << 32) | (uint32_t) row);
    }
}

}  // namespace vsr

using namespace vsr;

template <bool IND, int ROWS>
static hipError_t edge_distances(const HnswBuildParams& p, uint32_t n_prior, const int32_t* d_up_owner, uint32_t n_upper_prior, hipStream_t s)
{
    const uint64_t lists = (uint64_t) n_prior + (uint64_t) n_upper_prior * p.max_level;
    if (lists == 0) return hipSuccess;
    if ((lists + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_edge_dist_kernel<IND, ROWS>), dim3((uint32_t) ((lists + 3) / 4)), dim3(256), 0, s, p, n_prior, d_up_owner,
                       n_upper_prior);
    return hipGetLastError();
}

hipError_t vsr_hnsw_edge_distances(const HnswBuildParams& p, uint32_t n_prior, const int32_t* d_up_owner, uint32_t n_upper_prior, hipStream_t s)
{
    if (p.sparse || 2 * p.m > (uint32_t) HB_NBR) return hipErrorInvalidValue;   // (no element -> row instantiation over sparse rows)
    if (p.bits)
        return p.elem_row ? edge_distances<true, ROWS_BIT>(p, n_prior, d_up_owner, n_upper_prior, s)
                          : edge_distances<false, ROWS_BIT>(p, n_prior, d_up_owner, n_upper_prior, s);
    if (p.halves)
        return p.elem_row ? edge_distances<true, ROWS_HALF>(p, n_prior, d_up_owner, n_upper_prior, s)
                          : edge_distances<false, ROWS_HALF>(p, n_prior, d_up_owner, n_upper_prior, s);
    return p.elem_row ? edge_distances<true, ROWS_F32>(p, n_prior, d_up_owner, n_upper_prior, s)
                      : edge_distances<false, ROWS_F32>(p, n_prior, d_up_owner, n_upper_prior, s);
}

// host side: see vsr_hnsw_build_rt.hip (vsr_hnsw_build) for the batch loop; these are the two launches and the sort of a batch
template <bool IND, int ROWS>
static hipError_t build_batch(HnswBuildParams& p, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt, uint64_t* d_val_alt, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(p.rec_count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    // unused record slots sort to the end
    e = hipMemsetAsync(p.rec_key, 0xFF, (size_t) p.rec_cap * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const size_t lds1 = (size_t) p.lds_per_wave * p.wpb;
    if (lds1 > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_build_search_kernel<IND, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds1);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_build_search_kernel<IND, ROWS>), dim3((p.count + p.wpb - 1) / p.wpb), dim3(64 * p.wpb), lds1, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.entry < 0) return hipSuccess;                                       // the first element has nobody to link to
    hipcub::DoubleBuffer<uint64_t> keys(p.rec_key, d_key_alt), vals(p.rec_val, d_val_alt);
    e = hipcub::DeviceRadixSort::SortPairs(d_sort_tmp, sort_tmp_bytes, keys, vals, (int) p.rec_cap, 0, HB_KEY_BITS, s);
    if (e != hipSuccess) return e;
    HnswBuildParams q = p;
    q.rec_key = keys.Current();
    q.rec_val = vals.Current();
    const size_t lds2 = (size_t) 4 * HB_NBR * 32 + (ROWS == ROWS_SPARSE ? (size_t) 4 * p.sp_slots * 8 : 0);
    if (lds2 > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_build_link_kernel<IND, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds2);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_build_link_kernel<IND, ROWS>), dim3((p.rec_cap + 3) / 4), dim3(256), lds2, s, q);
    return hipGetLastError();
}

hipError_t vsr_hnsw_build_batch(HnswBuildParams& p, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt, uint64_t* d_val_alt,
                                hipStream_t s)
{
    if (p.sparse) {                                                           // (no merging build over sparse rows: element e is row e)
        if (p.elem_row || p.stride4 != 1 || p.sp_slots < 2 || (p.sp_slots & (p.sp_slots - 1)) != 0 ||
            (p.sp_lanes != 4 && p.sp_lanes != 16 && p.sp_lanes != 64))
            return hipErrorInvalidValue;
        return build_batch<false, ROWS_SPARSE>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    }
    if (p.bits)
        return p.elem_row ? build_batch<true, ROWS_BIT>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                          : build_batch<false, ROWS_BIT>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    if (p.halves)
        return p.elem_row ? build_batch<true, ROWS_HALF>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                          : build_batch<false, ROWS_HALF>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    return p.elem_row ? build_batch<true, ROWS_F32>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                      : build_batch<false, ROWS_F32>(p, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
}

// one round of vsr_hnsw_build_partitions: build_batch with the forest searches.  No round is skipped for want of an entry point:
// the graphs of a round are at different stages, and a wave without one emits no record
template <int ROWS>
static hipError_t forest_round(HnswBuildParams& p, const HnswForestParams& f, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt,
                               uint64_t* d_val_alt, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(p.rec_count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p.rec_key, 0xFF, (size_t) p.rec_cap * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const size_t lds1 = (size_t) p.lds_per_wave * p.wpb;
    if (lds1 > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_forest_search_kernel<ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds1);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_forest_search_kernel<ROWS>), dim3((p.count + p.wpb - 1) / p.wpb), dim3(64 * p.wpb), lds1, s, p, f);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipcub::DoubleBuffer<uint64_t> keys(p.rec_key, d_key_alt), vals(p.rec_val, d_val_alt);
    e = hipcub::DeviceRadixSort::SortPairs(d_sort_tmp, sort_tmp_bytes, keys, vals, (int) p.rec_cap, 0, HB_KEY_BITS, s);
    if (e != hipSuccess) return e;
    HnswBuildParams q = p;
    q.rec_key = keys.Current();
    q.rec_val = vals.Current();
    const size_t lds2 = (size_t) 4 * HB_NBR * 32;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_build_link_kernel<true, ROWS>), dim3((p.rec_cap + 3) / 4), dim3(256), lds2, s, q);
    return hipGetLastError();
}

hipError_t vsr_hnsw_forest_round(HnswBuildParams& p, const HnswForestParams& f, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt,
                                 uint64_t* d_val_alt, hipStream_t s)
{
    if (p.sparse || !p.elem_row || !f.elems || !f.entry || !f.entry_level || 2 * p.m > (uint32_t) HB_NBR || p.count == 0 ||
        p.count > HB_BATCH_MAX || p.rec_cap == 0)
        return hipErrorInvalidValue;
    if (p.bits) return forest_round<ROWS_BIT>(p, f, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    if (p.halves) return forest_round<ROWS_HALF>(p, f, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    return forest_round<ROWS_F32>(p, f, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
}

hipError_t vsr_hnsw_forest_split(const HnswBuildParams& p, const HnswForestGraph* d_graphs, uint32_t n_graphs, uint32_t n_total, hipStream_t s)
{
    if (n_total == 0) return hipSuccess;
    if (!d_graphs || n_graphs == 0 || !p.elem_row) return hipErrorInvalidValue;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_forest_split_kernel<false>), dim3((n_total + 3) / 4), dim3(256), 0, s, p, d_graphs, n_graphs, n_total,
                       (const HnswForestPrior*) nullptr);
    return hipGetLastError();
}

hipError_t vsr_hnsw_forest_split_carry(const HnswBuildParams& p, const HnswForestGraph* d_graphs, const HnswForestPrior* d_priors, uint32_t n_graphs,
                                       uint32_t n_total, hipStream_t s)
{
    if (n_total == 0) return hipSuccess;
    if (!d_graphs || !d_priors || n_graphs == 0 || !p.elem_row) return hipErrorInvalidValue;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_forest_split_kernel<true>), dim3((n_total + 3) / 4), dim3(256), 0, s, p, d_graphs, n_graphs, n_total,
                       d_priors);
    return hipGetLastError();
}

hipError_t vsr_hnsw_forest_join(const HnswBuildParams& p, const HnswForestJoin& j, const HnswForestGraph* d_graphs, const HnswForestPrior* d_priors,
                                uint32_t n_graphs, uint32_t n_total, hipStream_t s)
{
    if (n_total == 0) return hipSuccess;
    if (!d_graphs || !d_priors || n_graphs == 0 || !p.elem_row || !p.nbr0 || !p.up_nbr || !j.level || !j.elem_row || !j.up_slot || !j.up_owner ||
        !j.bad || !j.held)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hnsw_forest_join_kernel, dim3((n_total + 3) / 4), dim3(256), 0, s, p, j, d_graphs, d_priors, n_graphs, n_total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hnsw_forest_held_kernel, dim3((n_total + 255) / 256), dim3(256), 0, s, p, j, d_graphs, d_priors, n_graphs, n_total);
    return hipGetLastError();
}

// one repair batch of vsr_hnsw_vacuum: searches into the staging buffer, install, sort of the reverse edges, their application
template <bool IND, int ROWS>
static hipError_t vacuum_batch(HnswBuildParams& p, const HnswVacuumParams& v, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt,
                               uint64_t* d_val_alt, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(p.rec_count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p.rec_key, 0xFF, (size_t) p.rec_cap * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const size_t lds1 = (size_t) p.lds_per_wave * p.wpb;
    // the mixed attempt's searches are an instantiation of their own, so that the one every other attempt runs compiles as it did
    const void* search = v.spill_count ? reinterpret_cast<const void*>(hnsw_vacuum_search_kernel<IND, ROWS, true>)
                                       : reinterpret_cast<const void*>(hnsw_vacuum_search_kernel<IND, ROWS, false>);
    if (lds1 > 64 * 1024) {
        e = hipFuncSetAttribute(search, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds1);
        if (e != hipSuccess) return e;
    }
    if (v.spill_count && (e = hipMemsetAsync(v.spill_count, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if (!v.spill_all) {
        const dim3 grid((p.count + p.wpb - 1) / p.wpb), block(64 * p.wpb);
        if (v.spill_count) hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_vacuum_search_kernel<IND, ROWS, true>), grid, block, lds1, s, p, v);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_vacuum_search_kernel<IND, ROWS, false>), grid, block, lds1, s, p, v);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (v.spill_pool > 0) {                                                   // the repairs the launch above listed, or all of them: before the install
        const uint32_t waves = std::min(v.spill_pool, p.count);               // (wave w >= count has nothing to do)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_vacuum_search_spill_kernel<IND, ROWS>), dim3((waves + 3) / 4), dim3(256), 0, s, p, v);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hnsw_vacuum_install_kernel, dim3((p.count + 3) / 4), dim3(256), 0, s, p, v);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.entry < 0) return hipSuccess;                                       // nobody else is left: the lists stay empty
    hipcub::DoubleBuffer<uint64_t> keys(p.rec_key, d_key_alt), vals(p.rec_val, d_val_alt);
    e = hipcub::DeviceRadixSort::SortPairs(d_sort_tmp, sort_tmp_bytes, keys, vals, (int) p.rec_cap, 0, HB_KEY_BITS, s);
    if (e != hipSuccess) return e;
    HnswBuildParams q = p;
    q.rec_key = keys.Current();
    q.rec_val = vals.Current();
    const size_t lds2 = (size_t) 4 * HB_NBR * 32;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hnsw_vacuum_link_kernel<IND, ROWS>), dim3((p.rec_cap + 3) / 4), dim3(256), lds2, s, q, v.live);
    return hipGetLastError();
}

hipError_t vsr_hnsw_vacuum_batch(HnswBuildParams& p, const HnswVacuumParams& v, void* d_sort_tmp, size_t sort_tmp_bytes, uint64_t* d_key_alt,
                                 uint64_t* d_val_alt, hipStream_t s)
{
    if (p.sparse || 2 * p.m > (uint32_t) HB_NBR || p.count == 0 || p.count > HB_BATCH_MAX) return hipErrorInvalidValue;
    // the spill form: a pool with workspaces for this graph; the mixed attempt's list goes with a pool, `all` needs one
    if (v.spill_pool > 0 && (!v.spill_ws || !v.spill_total || v.spill_n == 0 || v.spill_ws_bytes < vsr::hnsw_vacuum_spill_ws_bytes(v.spill_n)))
        return hipErrorInvalidValue;
    if ((v.spill_all != 0 && v.spill_pool == 0) || ((v.spill_count != nullptr) != (v.spill_pool > 0 && v.spill_all == 0)) ||
        (v.spill_count && !v.spill_list))
        return hipErrorInvalidValue;
    if (p.bits)
        return p.elem_row ? vacuum_batch<true, ROWS_BIT>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                          : vacuum_batch<false, ROWS_BIT>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    if (p.halves)
        return p.elem_row ? vacuum_batch<true, ROWS_HALF>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                          : vacuum_batch<false, ROWS_HALF>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
    return p.elem_row ? vacuum_batch<true, ROWS_F32>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s)
                      : vacuum_batch<false, ROWS_F32>(p, v, d_sort_tmp, sort_tmp_bytes, d_key_alt, d_val_alt, s);
}

size_t vsr_hnsw_vacuum_tmp_bytes(uint32_t n_elem)
{
    size_t a = 0, b = 0;
    (void) hipcub::DeviceSelect::Flagged(nullptr, a, hipcub::CountingInputIterator<int32_t>(0), (const uint8_t*) nullptr, (int32_t*) nullptr,
                                         (int32_t*) nullptr, (int) n_elem, (hipStream_t) 0);
    (void) hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*) nullptr, (int32_t*) nullptr, (int) n_elem, (hipStream_t) 0);
    return std::max(a, b);
}

hipError_t vsr_hnsw_vacuum_mark(const HnswBuildParams& p, const int32_t* d_live, uint32_t n_elem, int32_t skip, uint8_t* d_flag, int32_t* d_list,
                                int32_t* d_num, void* d_tmp, size_t tmp_bytes, hipStream_t s)
{
    hipLaunchKernelGGL(hnsw_vacuum_mark_kernel, dim3((n_elem + 255) / 256), dim3(256), 0, s, p, d_live, n_elem, skip, d_flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_list) return e;
    return hipcub::DeviceSelect::Flagged(d_tmp, tmp_bytes, hipcub::CountingInputIterator<int32_t>(0), d_flag, d_list, d_num, (int) n_elem, s);
}

hipError_t vsr_hnsw_vacuum_renumber(const HnswBuildParams& p, const int32_t* d_live, int32_t* d_map, const int32_t* d_slot_map, uint32_t n_elem,
                                    int32_t* d_new_nbr0, int32_t* d_new_up_nbr, uint32_t new_max_level, void* d_tmp, size_t tmp_bytes, hipStream_t s)
{
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_live, d_map, (int) n_elem, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hnsw_vacuum_renumber_kernel, dim3((n_elem + 3) / 4), dim3(256), 0, s, p, d_live, d_map, d_slot_map, n_elem, d_new_nbr0,
                       d_new_up_nbr, new_max_level);
    return hipGetLastError();
}

size_t vsr_hnsw_build_sort_bytes(uint32_t rec_cap)
{
    size_t bytes = 0;
    hipcub::DoubleBuffer<uint64_t> keys(nullptr, nullptr), vals(nullptr, nullptr);
    (void) hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, vals, (int) rec_cap, 0, HB_KEY_BITS, (hipStream_t) 0);
    return bytes;
}
