// vsr_hnsw.h — K4: HNSW layer search on the GPU, one wave per query, up to four queries per workgroup.
//
// Replaces HnswSearchLayer (pgvector/src/hnswutils.c:813-976) as hnswgettuple's first call drives it (GetScanItems,
// hnswscan.c:15-45): greedy descent with ef = 1 through the upper layers, then the ef_search beam on layer 0, then the
// heap TIDs of the result elements nearest first (newest TID of an element first, hnswscan.c:278-311), the permission bit
// of every row (the executor's RLS filter above the index scan) and the first k.
//
// Candidates are totally ordered by key = (monotone fp32 index distance << 32) | element id: a fixed choice where
// pgvector's pairing heaps leave candidates of equal distance to insertion history (the tests' CPU checker makes the
// same choice).  Both of Algorithm 2's sets live in ONE sorted array S in LDS: every element ever pushed, with an
// "expanded" flag.  W (the ef best found) is S's first min(pushed, ef) entries, C (still to expand) its unexpanded
// entries.  An expansion reads the neighbour list (2m ids on layer 0, up to 200: HNSW_MAX_M = 100, hnsw.h:40), marks them
// in the query's visited set, computes the distances of the unvisited ones with 8 row gathers in flight per wave (half a
// wave per row) and then applies the admission rule  d < furthest(W) || |W| < ef  to them one by one in list order,
// exactly like the sequential loop (the order matters for ties).
//
// Visited set of layer 0 (the reference: a hash table of TIDs, hnswutils.c:662-699), by size of the graph:
//   VIS_LDS_BITMAP  n_elem / 8 bytes of LDS per query: exact, no global traffic at all (graphs up to ~1M elements)
//   VIS_LDS_HASH    open-addressing table in LDS sized by ef (not by the graph): a query that fills it beyond 3/4 reports
//                   status 1 and is re-run by the host entry point with the global bitmap
//   VIS_GLOBAL      one bitmap per query in global memory (round 2's only form; n_elem / 8 bytes per query, cleared per call)
// Upper layers (ef = 1) keep a short visited list in LDS.
//
// predicate_aware (vsr_hnsw_set_predicate_aware; off by default = pgvector's behaviour, where the executor filters what the
// index returns): the layer-0 walk itself applies the query's permission bitmap, in the manner of ACORN-1 (Patel et al., the
// library acorn_benchmark/src/acorn_search.cpp:144-181 calls; its source is not in the reference tree, so this variant is
// pinned by the tests' CPU restatement of THIS walk and by recall against the exact filtered scan, not by ACORN's code):
// W and C hold permitted elements only; expanding c takes c's unvisited neighbours that are permitted, and for every
// unvisited neighbour that is NOT permitted its permitted unvisited neighbours (two hops), in list order, up to HN_NBR
// candidates per expansion.  The descent through the upper layers and the entry point are unfiltered.
//
// Iterative index scans (hnsw_iterative_kernel: hnsw.iterative_scan = relaxed_order / strict_order, hnsw.max_scan_tuples;
// hnswscan.c:47-76,227-312, hnswutils.c:813-976 with a `discarded` heap).  Per query a visited set V that lasts the whole
// scan, a discarded set D (keys as above), a counter T (so->tuples) and P = -inf (so->previousDistance):
//   round 0   the search above.  T = the layer-0 entry point + the unvisited neighbours of every expansion (= out_visited).
//             D receives every neighbour that fails admission and every element pushed out of W: S's entries at positions
//             >= ef at the end of the round and every key insert() pushes off the end of S.
//   emission  W nearest first, each element's TIDs newest first; strict_order drops a TID whose element is nearer than P,
//             else P = its distance; a TID the query's filter admits is a result; the scan stops at k results.
//   W empty   T >= max_scan_tuples: D's smallest key is the next W alone (the drain; taken here 64 keys at a time, in
//             order: the same stream), stop when D is empty.  Otherwise stop when D is empty, else the min(ef, |D|)
//             smallest keys leave D and are the entry points of another layer-0 search with ef (ResumeScanItems: entry
//             points are neither marked nor counted again, T grows by the unvisited neighbours of expansions, both kinds
//             of discard go to D again); its W is the next batch.
// Not modelled: the memory stop (work_mem x hnsw.scan_mem_multiplier, hnswscan.c:244): only max_scan_tuples ends the
// search phase.  Rows come back in stream order, not re-sorted (relaxed_order may be out of order, as in pgvector); the
// stream depends on neither k nor the filter, so the answer for k1 is a prefix of the answer for k2 > k1.
// D is one append buffer of keys per query in global memory (cap_d keys; a query that would overflow it reports status 1
// and is re-run by the host entry point with cap_d = n_elem, which cannot overflow: an element is in at most one of D, W
// and "already emitted").  Taking keys out of D: an MSB-first radix select of the threshold key over D (histogram in the
// wave's LDS), a pass that moves the selected keys into S and compacts D in place, a bitonic sort of S.  The visited set
// is the LDS bitmap when it fits and the global bitmap otherwise (the LDS hash is sized by ef, not by the scan).
#pragma once
#include "vsr_device.h"
#include "vsr_topk.h"
#include "vsr_bitops.h"
#include "vsr_halfops.h"
#include "vsr_sparseops.h"
#include "vsr_hnsw_sizing.h"     // HN_LDS_BUDGET

namespace vsr {

enum HnswVisited : int { VIS_LDS_BITMAP = 0, VIS_LDS_HASH = 1, VIS_GLOBAL = 2 };
// (HnswRows, the row format the search body is instantiated for: vsr_bitops.h; ROWS_BIT is K4b, see above hnsw_search_body)

struct HnswParams {
    const float4*   rows = nullptr;          // base corpus rows (internal order)
    uint32_t        stride4 = 0;
    int             metric = 0;              // M_L2 / M_IP / M_COSINE (unit rows: ranked by negative inner product); ROWS_BIT: M_HAMMING / M_JACCARD
    const float*    queries = nullptr;       // [nq][q_stride] floats (q_stride >= dim; elements past dim are not read)
    uint32_t        q_stride = 0, dim = 0, nq = 0;
    uint32_t        n_elem = 0;
    int32_t         entry = -1, entry_level = -1;
    uint32_t        m = 0, max_level = 0;
    const int32_t*  elem_row = nullptr;      // element -> internal row holding its vector
    const int32_t*  nbr0 = nullptr;          // [n_elem][2m], -1 padded
    const int32_t*  up_slot = nullptr;       // element -> slot in up_nbr or -1
    const int32_t*  up_nbr = nullptr;        // [n_upper][max_level][m], -1 padded
    const int32_t*  level = nullptr;         // element -> top level
    const int32_t*  tid_count = nullptr;     // element -> heap TIDs (<= 10)
    const int32_t*  tids = nullptr;          // [n_elem][10] internal rows
    const uint64_t* const* bitmaps = nullptr;  // per query: permission bitmap over internal rows, or nullptr
    int             predicate_aware = 0;     // 1: the layer-0 walk applies the bitmap (see above); 0: only the results are filtered
    uint32_t        ef = 0, k = 0, caps = 0;   // caps: capacity of S (>= ef + 2m)
    int             vis_mode = VIS_GLOBAL;
    uint32_t        vis_words = 0;           // LDS bitmap / global bitmap: 32-bit words per query; LDS hash: slots (power of two)
    uint32_t*       visited = nullptr;       // VIS_GLOBAL: [nq][vis_words], zero on entry
    uint32_t        qpb = 1;                 // queries (waves) per workgroup
    uint32_t        lds_per_query = 0;       // bytes
    const int64_t*  block_ids = nullptr; const int32_t* doc_ids = nullptr; const int64_t* orig_rows = nullptr;
    int64_t* out_block = nullptr; int32_t* out_doc = nullptr; int64_t* out_row = nullptr; float* out_dist = nullptr; int32_t* out_count = nullptr;
    int64_t*        out_visited = nullptr;   // optional [nq]: elements entered into the visited set on layer 0
    int32_t*        out_status = nullptr;    // optional [nq]: 0 = ok, 1 = the LDS hash overflowed (result not valid: re-run with VIS_GLOBAL)
    uint32_t*       err = nullptr;
    // ROWS_BIT only.  rows: stride4 16-byte chunks of packed bits per row (pad bits zero); queries: the STAGED queries, q_stride / 4
    // = stride4 chunks each, pad bits cleared (stage_bit_kernel)
    const float*    row_pop = nullptr;       // popcount of every row (the corpus's d_norm2), Jaccard
    const float*    q_pop = nullptr;         // [nq] popcount of every staged query
    uint64_t*       out_keys = nullptr;      // optional [nq][k]: make_key(distance, internal row + key_row_offset) of every result,
                                             // KEY_EMPTY past the count: the stage-1 keys of the two-stage search (ShortlistParams::s1_keys)
    uint32_t        key_row_offset = 0;
    // ROWS_HALF only.  rows: stride4 16-byte chunks of 8 binary16 values per row (elements past dim zero); queries: fp32, as for ROWS_F32
    uint32_t        q_chunks = 0;            // 16-byte chunks of the wave's LDS that hold the rounded query: stride4 when stride4 > 64
                                             // (set before hnsw_plan*, which count it), else 0 -- the query lives in registers
    // ROWS_SPARSE only.  rows: the corpus's interleaved (index, value) entries, row r owns entries sp_off[r] .. sp_off[r + 1]; queries is
    // not read: query qi is the table sp_tab + qi * sp_slots that stage_sparse_kernel made, with its double totals sp_qtot[2 qi] (Q2)
    // and sp_qtot[2 qi + 1] (Q1).  q_chunks = sp_slots / 2 when the wave keeps a copy of the table in its LDS, 0 when it reads it where
    // staging wrote it; metric may be M_L1
    const uint64_t* sp_off = nullptr;        // [rows + 1]
    const uint2*    sp_tab = nullptr;        // [nq][sp_slots]
    const double*   sp_qtot = nullptr;       // [nq][2]
    uint32_t        sp_slots = 0;            // a power of two >= 2
    uint32_t        sp_lanes = 0;            // lanes per row: 4, 16 or 64 (the corpus's entry-count class)
    // hnsw_iterative_kernel only (out_visited then reports T when the scan stopped; status 1 = D overflowed)
    int             iter_mode = 0;           // VSR_HNSW_ITERATIVE_RELAXED = 1 / STRICT = 2
    int64_t         max_scan = 0;            // hnsw.max_scan_tuples
    uint64_t*       disc = nullptr;          // D: [nq][cap_d] keys
    uint32_t        cap_d = 0;
};

// The forest kernels (vsr_hnsw_forest_search.h: hnsw_forest_search_kernel and its half / bit forms) take this beside HnswParams, as a
// second kernel argument, so that the parameter block of the eight kernels below stays what it was.  One descriptor per graph of the
// forest: the per-index fields of HnswParams.
struct HnswGraphDesc {
    uint32_t       n_elem = 0;
    int32_t        entry = -1, entry_level = -1;
    uint32_t       max_level = 0;
    const int32_t* elem_row = nullptr;
    const int32_t* nbr0 = nullptr;
    const int32_t* up_slot = nullptr;
    const int32_t* up_nbr = nullptr;
    const int32_t* level = nullptr;
    const int32_t* tid_count = nullptr;
    const int32_t* tids = nullptr;
};
// A task is a (query, graph) pair; HnswParams::nq counts the launch's tasks.  The task's results are keys only: out_keys
// [slot][k] = make_key(rank value, internal row), KEY_EMPTY past the count; out_count / out_status / out_visited [slot].
struct HnswForestTasks {
    const HnswGraphDesc* graphs = nullptr;   // [n_indexes]
    const int32_t*       task_query = nullptr;   // [tasks] the query: its row, its popcount, its bitmap
    const int32_t*       task_graph = nullptr;   // [tasks]
    const int32_t*       task_slot = nullptr;    // [tasks] where the task's outputs go; nullptr: slot = task (a re-run names the slots
                                                 // of the tasks it repeats; the global visited words are the launch's own, by task)
};

constexpr int HN_UPPER_VISITED = 1024;     // visited list of an upper-layer (ef = 1) search, in LDS
constexpr int HN_NBR = 256;                // neighbour ids of one expansion (2m <= 200)

// (hnsw_rank_value: vsr_halfops.h)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// What a search reports for a result whose rank value (the index distance) is d: written once for emit() below and for the merge
// kernel of a forest search (vsr_hnsw_forest_search.h), the rule of vsr_exact.h -- arithmetic two kernels share has one definition.
__device__ __forceinline__ float hnsw_reported_distance(int rows, int metric, float d)
{
    if (rows == ROWS_BIT) return d;                                          // <~> / <%>: the index distance is the operator's value
    if (rows == ROWS_SPARSE && metric == M_L1) return d;                     // <+>: the index distance is the operator's value
    if (metric == M_L2) return (float) sqrt((double) d);                     // l2_distance, vector.c:577
    if (metric == M_IP) return d;                                            // <#> = negative inner product
    double sim = -(double) d;                                                // unit rows: cosine distance = 1 - dot
    if (sim > 1.0) sim = 1.0; else if (sim < -1.0) sim = -1.0;
    return (float) (1.0 - sim);
}

constexpr int HN_HIST = 256;               // radix-select histogram of the iterative kernel (8-bit digits), in LDS

// global-memory stores of the wave (D) visible to its later loads, and LDS as wave_sync
__device__ __forceinline__ void wave_sync_global()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// K4b, ROWS = ROWS_BIT: the graph of a bit corpus (bit_hamming_ops / bit_jaccard_ops, hnswutils.c:1398-1410).  K4 gives half a
// wave to each gathered row; a 128-bit row is ONE 16-byte chunk, which would leave 31 of 32 lanes idle.  The bit distance stage
// (bit_graph_distances, vsr_bitops.h) gives a row G lanes, G the smallest power of two >= its chunks (at most 64): 64 neighbours
// per wave step at 128 bits, 8 at 1024 bits, and beyond 8192 bits the 64 lanes loop over the chunks.  The lane keeps its chunk
// of the staged query in a register across expansions (re-read from the staged copy when a row has more than 64 chunks);
// partials are integer popcounts, reduced by shuffles inside the lane group, converted once with K1b's own expression
// (rank_value_bits: Hamming the count, Jaccard in double then rounded).  The reported distance is that fp32 value (no sqrt).
//
// K4h, ROWS = ROWS_HALF: the graph of a halfvec corpus (halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops, hnswutils.c:1385-1396).
// A row is C = ceil(dim / 8) 16-byte chunks of 8 binary16 values, half the bytes K4 gathers.  The half distance stage
// (half_graph_distances, vsr_halfops.h) gives a row G lanes as K4b does: 4 neighbours per wave step at 128 dimensions, 32 at 10,
// and beyond 512 dimensions the 64 lanes loop over the chunks.  The query arrives as fp32 and is rounded to binary16 once, when
// the wave loads it (`$1::halfvec`): the lane keeps its chunk in a register when C <= 64, otherwise the wave keeps the rounded
// query in its LDS (q_chunks chunks in front of the visited set); both last across expansions and there is no staging launch.
// Arithmetic: both operands widened to fp32, fmaf sums (halfutils.c), ranked and reported exactly as K4 does.
//
// K4s, ROWS = ROWS_SPARSE: the graph of a sparse corpus (sparsevec_l2_ops / sparsevec_ip_ops / sparsevec_cosine_ops /
// sparsevec_l1_ops, hnswutils.c:1352-1361, 1411-1422).  A row is a CSR run of (index, value) entries of any length up to 1000; the
// query is K1s's open-addressing table (stage_sparse_kernel: one launch in front of the search, on the same stream).  The wave
// copies its query's table once into its LDS, into the q_chunks area in front of the visited set (sp_slots / 2 chunks: 16 KB at 1000
// non-zeros); a table that does not fit beside S at one query per workgroup is read where staging wrote it.  The sparse distance
// stage (sparse_graph_distances, vsr_sparseops.h) gives a row 4, 16 or 64 lanes by the corpus's entry-count class.  Arithmetic:
// K1s's (fp32 sum over the row's entries, double sum over the hits, the rest term of L2 and L1); ranked by squared L2, the L1 sum or
// the negated inner product; reported as K4 reports, L1 as the sum itself.
//
// FOREST (vsr_hnsw_forest_search.h): the wave serves one TASK, a (query, graph) pair of a forest of graphs over one corpus.  qi is
// the task; the query's row, popcount and bitmap are taken by the query index qq, the graph fields of the wave's copy of the
// parameters come from the graph's descriptor, the global visited words are the task's, and emission writes keys only (out_keys
// [slot][k], make_key(rank value, internal row)): identities and reported distances are the merge kernel's.
template <bool ITER, int ROWS = ROWS_F32, bool FOREST = false>
__device__ __forceinline__ void hnsw_search_body(const HnswParams pk, const HnswForestTasks ft = HnswForestTasks{})
{
    static_assert(!FOREST || (!ITER && ROWS != ROWS_SPARSE), "forest search: the plain search over fp32, halfvec and bit rows");
    extern __shared__ __align__(16) unsigned char smem_all[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const uint32_t qi = blockIdx.x * pk.qpb + wave;
    if (wave >= pk.qpb || qi >= pk.nq) return;                               // (waves are independent: no workgroup barrier below)
    HnswParams p = pk;
    uint32_t qq = qi;                        // the query whose row, popcount and bitmap the wave reads
    uint32_t so = qi;                        // where its outputs go
    if constexpr (FOREST) {
        qq = (uint32_t) __builtin_amdgcn_readfirstlane(ft.task_query[qi]);
        const uint32_t g = (uint32_t) __builtin_amdgcn_readfirstlane(ft.task_graph[qi]);
        if (ft.task_slot) so = (uint32_t) __builtin_amdgcn_readfirstlane(ft.task_slot[qi]);
        const HnswGraphDesc gd = ft.graphs[g];
        p.n_elem = gd.n_elem; p.entry = gd.entry; p.entry_level = gd.entry_level; p.max_level = gd.max_level;
        p.elem_row = gd.elem_row; p.nbr0 = gd.nbr0; p.up_slot = gd.up_slot; p.up_nbr = gd.up_nbr; p.level = gd.level;
        p.tid_count = gd.tid_count; p.tids = gd.tids;
    }
    unsigned char* smem = smem_all + (size_t) wave * p.lds_per_query;
    uint64_t* S = reinterpret_cast<uint64_t*>(smem);                         // [caps] sorted keys
    uint8_t*  X = reinterpret_cast<uint8_t*>(S + p.caps);                    // [caps] expanded flags
    int32_t*  nb = reinterpret_cast<int32_t*>(X + ((p.caps + 15) & ~15u));   // [HN_NBR] neighbour ids of the expansion
    float*    nd = reinterpret_cast<float*>(nb + HN_NBR);                    // [HN_NBR] their distances
    int32_t*  uv = reinterpret_cast<int32_t*>(nd + HN_NBR);                  // [HN_UPPER_VISITED] upper-layer visited list
    uint32_t* lv = reinterpret_cast<uint32_t*>(uv + HN_UPPER_VISITED);       // layer-0 visited set: bitmap words or hash slots
    uint4*    qh = nullptr;                                                  // ROWS_HALF: [q_chunks] the rounded query
    if constexpr (ROWS == ROWS_HALF) {
        qh = reinterpret_cast<uint4*>(lv);
        lv += 4u * p.q_chunks;
    }
    uint64_t* qt = nullptr;                                                  // ROWS_SPARSE: [sp_slots] the query's table (q_chunks != 0)
    if constexpr (ROWS == ROWS_SPARSE) {
        qt = reinterpret_cast<uint64_t*>(lv);
        lv += 4u * p.q_chunks;
    }
    uint32_t* hist = nullptr;                                               // ITER: [HN_HIST] radix-select histogram
    if constexpr (ITER) {
        hist = lv;
        lv += HN_HIST;
    }
    const float* q = p.queries + (size_t) qq * p.q_stride;
    uint32_t* gvis = p.vis_mode == VIS_GLOBAL ? p.visited + (size_t) qi * p.vis_words : nullptr;
    const int half = lane >> 5, hl = lane & 31;
    const uint32_t d4 = (p.dim + 3) / 4;
    bool overflow = false;
    uint32_t hash_used = 0;

    if (p.vis_mode != VIS_GLOBAL) {
        for (uint32_t i = (uint32_t) lane; i < p.vis_words; i += 64) lv[i] = 0u;
        wave_sync();
    }
    // mark element e visited; true when it was not yet (lanes of the wave call this concurrently)
    auto visit = [&](uint32_t e) -> bool {
        if (p.vis_mode == VIS_GLOBAL) {
            const uint32_t old = atomicOr(&gvis[e >> 5], 1u << (e & 31));
            return !((old >> (e & 31)) & 1u);
        }
        if (p.vis_mode == VIS_LDS_BITMAP) {
            const uint32_t old = atomicOr(&lv[e >> 5], 1u << (e & 31));
            return !((old >> (e & 31)) & 1u);
        }
        const uint32_t mask = p.vis_words - 1u;
        uint32_t h = (e * 2654435761u) >> 7;
        for (uint32_t probe = 0; probe <= mask; ++probe, ++h) {
            const uint32_t old = atomicCAS(&lv[h & mask], 0u, e + 1u);
            if (old == 0u) return true;
            if (old == e + 1u) return false;
        }
        return false;                                                        // table full: reported through `overflow` below
    };

    // ROWS_BIT: lanes per row, this lane's chunk of the staged query, the query's popcount
    uint32_t bit_g = 1;
    uint4 qreg = make_uint4(0u, 0u, 0u, 0u);
    float q_pop = 0.0f;
    if constexpr (ROWS == ROWS_BIT) {
        bit_g = bit_graph_lanes(p.stride4);
        const uint32_t gl = (uint32_t) lane & (bit_g - 1u);
        if (p.stride4 <= 64u && gl < p.stride4) qreg = reinterpret_cast<const uint4*>(q)[gl];
        q_pop = p.q_pop[qq];
    }
    // ROWS_HALF: the same lane groups; the query rounded to binary16 once, this lane's chunk of it or the copy in LDS
    if constexpr (ROWS == ROWS_HALF) {
        bit_g = bit_graph_lanes(p.stride4);
        const uint32_t gl = (uint32_t) lane & (bit_g - 1u);
        if (p.stride4 <= 64u) {
            if (gl < p.stride4) qreg = half_query_chunk(q, p.dim, gl);
        } else {
            for (uint32_t ch = (uint32_t) lane; ch < p.q_chunks; ch += 64) qh[ch] = half_query_chunk(q, p.dim, ch);
            wave_sync();
        }
    }
    // ROWS_SPARSE: the staged table of the query, copied into the wave's LDS when the plan gave it room; its double totals
    const uint64_t* sp_gtab = nullptr;
    uint32_t sp_mask = 0, sp_shift = 0;
    double sp_q2 = 0.0, sp_q1 = 0.0;
    if constexpr (ROWS == ROWS_SPARSE) {
        sp_gtab = reinterpret_cast<const uint64_t*>(p.sp_tab) + (size_t) qi * p.sp_slots;
        sp_mask = p.sp_slots - 1u;
        sp_shift = (uint32_t) __clz((int) p.sp_slots) + 1u;                   // 32 - log2 slots
        sp_q2 = p.sp_qtot[2 * (size_t) qi];
        sp_q1 = p.sp_qtot[2 * (size_t) qi + 1];
        if (p.q_chunks) {
            for (uint32_t i = (uint32_t) lane; i < p.sp_slots; i += 64) qt[i] = sp_gtab[i];
            wave_sync();
        }
    }
    // distance of the query to `cnt` elements listed in nb[] -> nd[] (fp32 sum; exact on integer-valued data in any order)
    auto distances = [&](int cnt) {
        if constexpr (ROWS == ROWS_BIT) {
            const uint4* brows = reinterpret_cast<const uint4*>(p.rows);
            const uint4* qs = reinterpret_cast<const uint4*>(q);
            if (p.metric == M_JACCARD)
                bit_graph_distances<true>(brows, p.stride4, bit_g, p.elem_row, p.row_pop, qs, qreg, q_pop, nb, cnt, nd, lane);
            else
                bit_graph_distances<false>(brows, p.stride4, bit_g, p.elem_row, p.row_pop, qs, qreg, q_pop, nb, cnt, nd, lane);
            wave_sync();
            return;
        } else if constexpr (ROWS == ROWS_HALF) {
            const uint4* hrows = reinterpret_cast<const uint4*>(p.rows);
            if (p.metric == M_L2) half_graph_distances<true>(hrows, p.stride4, bit_g, p.elem_row, qh, qreg, nb, cnt, nd, lane);
            else half_graph_distances<false>(hrows, p.stride4, bit_g, p.elem_row, qh, qreg, nb, cnt, nd, lane);
            wave_sync();
            return;
        } else if constexpr (ROWS == ROWS_SPARSE) {
            if (p.q_chunks)
                sparse_graph_distances_metric(p.metric, p.rows, p.sp_off, p.sp_lanes, p.elem_row, (lds_u64) qt, sp_mask, sp_shift, sp_q2, sp_q1,
                                              nb, cnt, nd, lane);
            else
                sparse_graph_distances_metric(p.metric, p.rows, p.sp_off, p.sp_lanes, p.elem_row, as_global(sp_gtab), sp_mask, sp_shift, sp_q2,
                                              sp_q1, nb, cnt, nd, lane);
            wave_sync();
            return;
        } else {
        constexpr int U = 4;
        for (int c0 = 0; c0 < cnt; c0 += 2 * U) {
            float s[U];
            int32_t row[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + 2 * u + half;
                s[u] = 0.0f;
                row[u] = c < cnt ? p.elem_row[nb[c]] : 0;
            }
            for (uint32_t ch = hl; ch < d4; ch += 32) {
                float4 b;
                if (4 * ch + 3 < p.dim && (p.q_stride & 3u) == 0) b = *reinterpret_cast<const float4*>(q + 4 * ch);
                else {
                    b.x = 4 * ch < p.dim ? q[4 * ch] : 0.0f;
                    b.y = 4 * ch + 1 < p.dim ? q[4 * ch + 1] : 0.0f;
                    b.z = 4 * ch + 2 < p.dim ? q[4 * ch + 2] : 0.0f;
                    b.w = 4 * ch + 3 < p.dim ? q[4 * ch + 3] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(p.rows + (size_t) row[u] * p.stride4 + ch);
                    if (p.metric == M_L2) {
                        const float d0 = av[0] - b.x, d1 = av[1] - b.y, d2 = av[2] - b.z, d3 = av[3] - b.w;
                        s[u] = fmaf(d0, d0, s[u]); s[u] = fmaf(d1, d1, s[u]); s[u] = fmaf(d2, d2, s[u]); s[u] = fmaf(d3, d3, s[u]);
                    } else {
                        s[u] = fmaf(av[0], b.x, s[u]); s[u] = fmaf(av[1], b.y, s[u]); s[u] = fmaf(av[2], b.z, s[u]); s[u] = fmaf(av[3], b.w, s[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                for (int mm = 16; mm >= 1; mm >>= 1) s[u] += __shfl_xor(s[u], mm);
                const int c = c0 + 2 * u + half;
                if (hl == 0 && c < cnt) nd[c] = hnsw_rank_value(p.metric, s[u]);
            }
        }
        wave_sync();
        }
    };

    const uint64_t* bm = p.bitmaps ? p.bitmaps[qq] : nullptr;
    const bool pa = p.predicate_aware && bm != nullptr;
    // element e is permitted when one of its heap rows is
    auto permitted = [&](uint32_t e) -> bool {
        const uint32_t nt = (uint32_t) p.tid_count[e];
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t row = (uint32_t) p.tids[(size_t) e * 10 + t];
            if ((bm[row >> 6] >> (row & 63)) & 1ull) return true;
        }
        return false;
    };
    uint32_t count = 0;                      // entries of S
    uint32_t pushed = 0;                     // wlen of the reference: pushes so far (never decremented)
    uint32_t first_open = 0;                 // every entry before this position is expanded
    // insert (key, unexpanded) into S keeping it sorted; beyond caps the largest entry falls off (ITER: returned, else
    // KEY_EMPTY)
    auto insert = [&](uint64_t key) -> uint64_t {
        uint64_t dropped = KEY_EMPTY;
        // position = number of keys < key.  A binary search is a chain of log2(count) dependent LDS reads (eleven at ef_search
        // in the thousands: over a microsecond per insert); the wave does a 64-ary search instead: lane l compares the LAST key of
        // segment l (count / 64 keys, rounded up), the segments entirely below the key are a prefix, and the one segment that is
        // left is compared key by key -- two or three LDS round trips whatever the count.
        uint32_t pos = 0;
        if (count) {
            const uint32_t seg_len = (count + 63u) / 64u;
            const uint32_t s0 = (uint32_t) lane * seg_len;
            const uint32_t s1 = s0 + seg_len < count ? s0 + seg_len : count;
            const bool has = s0 < count;
            const uint64_t pivot = has ? S[s1 - 1] : KEY_EMPTY;
            const uint32_t seg = (uint32_t) __popcll(__ballot(has && pivot < key));      // segments whose every key is < key
            const uint32_t b0 = seg * seg_len;
            const uint32_t b1 = b0 + seg_len < count ? b0 + seg_len : count;
            pos = b0 < count ? b0 : count;
            for (uint32_t o = b0; o < b1; o += 64) {
                const uint32_t i = o + (uint32_t) lane;
                pos += (uint32_t) __popcll(__ballot(i < b1 && S[i] < key));
            }
        }
        if (pos >= p.caps) {
            if constexpr (ITER) dropped = key;
            return dropped;
        }
        if constexpr (ITER)
            if (count == p.caps) dropped = S[p.caps - 1];
        const uint32_t last = count < p.caps ? count : p.caps - 1;      // index the shifted tail ends at
        // the tail [pos, last) moves up by one, 256 entries per step from the end (four per lane: a step is two wave barriers
        // whatever it moves, and at ef_search in the thousands the tail is a thousand entries long)
        for (int64_t base = (int64_t) ((last - 1) & ~255u); last > pos && base >= (int64_t) (pos & ~255u); base -= 256) {
            const uint32_t i0 = (uint32_t) base + 4u * (uint32_t) lane;
            uint64_t kk[4];
            uint8_t xx[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + (uint32_t) u;
                const bool mv = i >= pos && i < last;
                kk[u] = mv ? S[i] : 0;
                xx[u] = mv ? X[i] : 0;
            }
            wave_sync();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + (uint32_t) u;
                if (i >= pos && i < last) { S[i + 1] = kk[u]; X[i + 1] = xx[u]; }
            }
            wave_sync();
        }
        if (lane == 0) { S[pos] = key; X[pos] = 0; }
        if (count < p.caps) ++count;
        if (pos < first_open) first_open = pos;
        wave_sync();
        return dropped;
    };

    // ITER: D, the discarded keys of this query (global memory), n_disc of them
    uint64_t* Dq = nullptr;
    uint32_t n_disc = 0;
    if constexpr (ITER) Dq = p.disc + (size_t) qi * p.cap_d;
    // append the keys of the lanes with `pass` (one ballot-compacted write); beyond cap_d: overflow, nothing written
    auto disc_append = [&](bool pass, uint64_t key) {
        const uint64_t m = __ballot(pass);
        const uint32_t add = (uint32_t) __popcll(m);
        if (n_disc + add > p.cap_d) { overflow = true; return; }
        if (pass) Dq[n_disc + (uint32_t) __popcll(m & ((1ull << lane) - 1ull))] = key;
        n_disc += add;
    };

    int64_t visited_l0 = 0;
    // Algorithm 2 on layer lc with beam ef_; S holds the entry points (unexpanded) on entry and W (sorted) on exit.
    // mark_entries = false (ITER resume rounds): the entry points come from D, already visited and counted
    auto search_layer = [&](int lc, uint32_t ef_, bool mark_entries) {
        const uint32_t lm = lc == 0 ? 2 * p.m : p.m;
        uint32_t n_uv = 0;
        // entry points count as visited
        if (lc == 0) {
            if (!ITER || mark_entries) {
                for (uint32_t i = (uint32_t) lane; i < count; i += 64) (void) visit((uint32_t) S[i]);
                visited_l0 += count;
                hash_used += count;
            }
        } else {                             // (one entry point per upper layer)
            if (lane == 0) uv[0] = (int32_t) (uint32_t) S[0];
            n_uv = 1;
        }
        pushed = count;
        first_open = 0;
        wave_sync();
        for (;;) {
            // c = nearest unexpanded entry
            uint32_t cpos = 0xFFFFFFFFu;
            for (uint32_t base = first_open & ~63u; base < count && cpos == 0xFFFFFFFFu; base += 64) {
                const uint32_t i = base + (uint32_t) lane;
                const uint64_t mk = __ballot(i < count && i >= first_open && X[i] == 0);
                if (mk) cpos = base + (uint32_t) __ffsll((unsigned long long) mk) - 1;
            }
            if (cpos == 0xFFFFFFFFu) break;                                  // C is empty
            first_open = cpos + 1;
            const uint64_t ckey = S[cpos];
            const uint32_t wl = pushed < ef_ ? pushed : ef_;                   // |W|
            const uint64_t fkey = S[(wl < count ? wl : count) - 1];
            if (mono_to_float((uint32_t) (ckey >> 32)) > mono_to_float((uint32_t) (fkey >> 32))) break;
            if (lane == 0) X[cpos] = 1;
            const uint32_t ce = (uint32_t) ckey;
            // neighbour list of c on this layer, 64 ids at a time, unvisited ones kept in list order
            int cnt = 0;
            const int32_t* nl;
            if (lc == 0) nl = p.nbr0 + (size_t) ce * 2 * p.m;
            else {
                const int32_t slot = p.up_slot[ce];
                nl = slot >= 0 ? p.up_nbr + ((size_t) slot * p.max_level + (uint32_t) (lc - 1)) * p.m : nullptr;
            }
            if (pa && lc == 0) {
                // ---- predicate-aware expansion: permitted neighbours, then the permitted neighbours of the others ----
                int32_t* hop = reinterpret_cast<int32_t*>(nd);               // (nd is free until distances(): <= 2m <= 200 ids)
                int n_hop = 0;
                uint32_t marked = 0;
                for (uint32_t j0 = 0; j0 < lm; j0 += 64) {
                    const uint32_t j = j0 + (uint32_t) lane;
                    const int32_t my = j < lm ? nl[j] : -1;
                    const bool fresh = my >= 0 && visit((uint32_t) my);
                    const bool okp = fresh && permitted((uint32_t) my);
                    const uint64_t fm = __ballot(okp), hm = __ballot(fresh && !okp);
                    if (okp) nb[cnt + __popcll(fm & ((1ull << lane) - 1ull))] = my;
                    if (fresh && !okp) hop[n_hop + __popcll(hm & ((1ull << lane) - 1ull))] = my;
                    cnt += __popcll(fm);
                    n_hop += __popcll(hm);
                    marked += (uint32_t) __popcll(fm | hm);
                    wave_sync();
                }
                for (int h = 0; h < n_hop && cnt < HN_NBR; ++h) {
                    const int32_t* nl2 = p.nbr0 + (size_t) (uint32_t) hop[h] * 2 * p.m;
                    for (uint32_t j0 = 0; j0 < lm && cnt < HN_NBR; j0 += 64) {
                        const uint32_t j = j0 + (uint32_t) lane;
                        const int32_t my = j < lm ? nl2[j] : -1;
                        const bool ok2 = my >= 0 && permitted((uint32_t) my) && visit((uint32_t) my);
                        const uint64_t fm = __ballot(ok2);
                        const int at = cnt + __popcll(fm & ((1ull << lane) - 1ull));
                        if (ok2 && at < HN_NBR) nb[at] = my;                 // (beyond the cap: marked visited, dropped)
                        marked += (uint32_t) __popcll(fm);
                        cnt += __popcll(fm);
                        if (cnt > HN_NBR) cnt = HN_NBR;
                        wave_sync();
                    }
                }
                visited_l0 += marked;
                hash_used += marked;
                if (p.vis_mode == VIS_LDS_HASH && hash_used * 4u > p.vis_words * 3u) { overflow = true; break; }
            } else {
            for (uint32_t j0 = 0; j0 < lm && nl; j0 += 64) {
                const uint32_t j = j0 + (uint32_t) lane;
                const int32_t my = j < lm ? nl[j] : -1;
                bool fresh = false;
                if (my >= 0) {
                    if (lc == 0) fresh = visit((uint32_t) my);
                    else {
                        fresh = true;
                        for (uint32_t u = 0; u < n_uv; ++u) fresh &= uv[u] != my;
                    }
                }
                const uint64_t fm = __ballot(fresh);
                const int add = __popcll(fm);
                if (fresh) {
                    const int at = cnt + __popcll(fm & ((1ull << lane) - 1ull));
                    nb[at] = my;
                    if (lc != 0) {
                        const uint32_t ua = n_uv + (uint32_t) (at - cnt);
                        if (ua < (uint32_t) HN_UPPER_VISITED) uv[ua] = my;
                        else atomicOr(p.err, 8u);                           // cannot happen at ef = 1
                    }
                }
                if (lc != 0) n_uv += (uint32_t) add;
                cnt += add;
                wave_sync();
            }
            if (lc == 0) {
                visited_l0 += cnt;
                hash_used += (uint32_t) cnt;
                if (p.vis_mode == VIS_LDS_HASH && hash_used * 4u > p.vis_words * 3u) { overflow = true; break; }
            }
            }
            if (cnt == 0) continue;
            distances(cnt);
            uint32_t admitted = 0;                   // ITER: bit i >> 6 of lane i & 63 = neighbour i entered W
            for (int i = 0; i < cnt; ++i) {                                  // the sequential admission of Algorithm 2
                const uint32_t e = (uint32_t) nb[i];
                const float ed = nd[i];
                const bool always = pushed < ef_;
                const uint32_t wl2 = pushed < ef_ ? pushed : ef_;
                const float fd = mono_to_float((uint32_t) (S[(wl2 < count ? wl2 : count) - 1] >> 32));
                if (!(ed < fd || always)) continue;
                if (lc != 0 && p.level[e] < lc) continue;                    // (every element lives on layer 0)
                const uint64_t fell = insert(make_key(ed, e));
                ++pushed;
                if constexpr (ITER) {
                    if (lane == (i & 63)) admitted |= 1u << (i >> 6);
                    if (lc == 0 && fell != KEY_EMPTY) disc_append(lane == 0, fell);     // pushed out of W (and S)
                }
            }
            if constexpr (ITER) {
                if (lc == 0) {                                               // the neighbours admission rejected
                    for (int c0 = 0; c0 < cnt; c0 += 64) {
                        const int i = c0 + lane;
                        const bool rej = i < cnt && !((admitted >> (c0 >> 6)) & 1u);
                        disc_append(rej, rej ? make_key(nd[i], (uint32_t) nb[i]) : 0ull);
                    }
                    if (overflow) break;
                }
            }
        }
        const uint32_t wl = pushed < ef_ ? pushed : ef_;
        if constexpr (ITER) {
            if (lc == 0 && !overflow)                                        // pushed out of W, still in S
                for (uint32_t b = wl; b < count; b += 64) {
                    const uint32_t i = b + (uint32_t) lane;
                    disc_append(i < count, i < count ? S[i] : 0ull);
                }
        }
        count = wl < count ? wl : count;                                     // S = W, nearest first
    };

    auto write_empty = [&](uint32_t from) {
        for (uint32_t i = from + (uint32_t) lane; i < p.k; i += 64) {
            const size_t o = (size_t) so * p.k + i;
            if constexpr (FOREST) {
                p.out_keys[o] = KEY_EMPTY;
                continue;
            }
            p.out_block[o] = -1; p.out_doc[o] = -1;
            if (p.out_row) p.out_row[o] = -1;
            p.out_dist[o] = __builtin_inff();
            if constexpr (ROWS == ROWS_BIT)
                if (p.out_keys) p.out_keys[o] = KEY_EMPTY;
        }
    };
    if (p.out_status && lane == 0) p.out_status[so] = 0;
    if (p.entry < 0) {
        if (lane == 0) p.out_count[so] = 0;
        if constexpr (ITER || FOREST)
            if (p.out_visited && lane == 0) p.out_visited[so] = 0;
        write_empty(0);
        return;
    }
    // HnswEntryCandidate
    if (lane == 0) nb[0] = p.entry;
    wave_sync();
    distances(1);
    insert(make_key(nd[0], (uint32_t) p.entry));
    for (int lc = p.entry_level; lc >= 1; --lc) {
        search_layer(lc, 1, true);
        if (lane == 0)
            for (uint32_t i = 0; i < count; ++i) X[i] = 0;                    // W becomes the next layer's entry points
        wave_sync();
    }
    search_layer(0, p.ef, true);
    if constexpr (!ITER)
        if (p.out_visited && lane == 0) p.out_visited[so] = visited_l0;
    auto fail_query = [&]() {                                                // status 1: no result
        if (lane == 0) {
            p.out_count[so] = -1;
            if (p.out_status) p.out_status[so] = 1;
        }
        write_empty(0);
    };
    if (overflow) {                                                          // the visited table filled up (ITER: D did)
        if constexpr (ITER)
            if (p.out_visited && lane == 0) p.out_visited[so] = visited_l0;
        fail_query();
        return;
    }

    // hnswgettuple: elements nearest first, their heap TIDs newest first, the permission bit, the first k
    uint32_t out = 0;
    float prev_d = -__builtin_inff();        // ITER strict_order: so->previousDistance (index distance)
    // emit S[0, n) after what is out already
    auto emit = [&](uint32_t n) {
    for (uint32_t base = 0; base < n && out < p.k; base += 64) {
        const uint32_t i = base + (uint32_t) lane;
        uint32_t e = 0, nt = 0, okmask = 0;
        float d = 0.0f;
        if (i < n) {
            e = (uint32_t) S[i];
            d = mono_to_float((uint32_t) (S[i] >> 32));
            nt = (uint32_t) p.tid_count[e];
            if constexpr (ITER)
                if (p.iter_mode == 2 && d < prev_d) nt = 0;                  // strict_order: nearer than the last one out
            for (uint32_t t = 0; t < nt; ++t) {                              // bit t: TID nt-1-t (newest first) is permitted
                const uint32_t row = (uint32_t) p.tids[(size_t) e * 10 + (nt - 1 - t)];
                if (!bm || ((bm[row >> 6] >> (row & 63)) & 1ull)) okmask |= 1u << t;
            }
        }
        if constexpr (ITER) {
            if (p.iter_mode == 2) {              // S is sorted: what passes is a suffix of the chunk, the last one sets P
                float mx = nt > 0 ? d : -__builtin_inff();
                for (int dd = 32; dd >= 1; dd >>= 1) mx = fmaxf(mx, __shfl_xor(mx, dd));
                prev_d = fmaxf(prev_d, mx);
            }
        }
        uint32_t mine = (uint32_t) __popc(okmask), incl = mine;
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t o = (uint32_t) __shfl_up((int) incl, dd);
            if (lane >= dd) incl += o;
        }
        uint32_t at = out + incl - mine;
        for (uint32_t t = 0; t < nt; ++t)
            if ((okmask >> t) & 1u) {
                if (at < p.k) {
                    const uint32_t row = (uint32_t) p.tids[(size_t) e * 10 + (nt - 1 - t)];
                    const size_t o = (size_t) so * p.k + at;
                    if constexpr (FOREST) p.out_keys[o] = make_key(d, row);      // the merge kernel's input: nothing else
                    else {
                    p.out_block[o] = p.block_ids[row];
                    p.out_doc[o] = p.doc_ids[row];
                    if (p.out_row) p.out_row[o] = p.orig_rows[row];
                    if constexpr (ROWS == ROWS_BIT)
                        if (p.out_keys) p.out_keys[o] = make_key(d, row + p.key_row_offset);
                    p.out_dist[o] = hnsw_reported_distance(ROWS, p.metric, d);
                    }
                }
                ++at;
            }
        out += (uint32_t) __shfl((int) incl, 63);
    }
    };
    emit(count);

    if constexpr (ITER) {
        // radix select: the key t such that exactly `want` (< n_disc) keys of D are <= t (keys are distinct)
        auto threshold = [&](uint32_t want) -> uint64_t {
            uint64_t prefix = 0, pmask = 0;
            uint32_t need = want;
            for (int shift = 56; shift >= 0; shift -= 8) {
                for (uint32_t b = (uint32_t) lane; b < (uint32_t) HN_HIST; b += 64) hist[b] = 0u;
                wave_sync();
                for (uint32_t i = (uint32_t) lane; i < n_disc; i += 64) {
                    const uint64_t key = Dq[i];
                    if ((key & pmask) == prefix) atomicAdd(&hist[(uint32_t) (key >> shift) & 255u], 1u);
                }
                wave_sync();
                uint32_t h[4], sum = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) { h[u] = hist[4 * lane + u]; sum += h[u]; }
                uint32_t incl = sum;
                for (int dd = 1; dd < 64; dd <<= 1) {
                    const uint32_t o = (uint32_t) __shfl_up((int) incl, dd);
                    if (lane >= dd) incl += o;
                }
                const uint32_t excl = incl - sum;
                const int owner = __ffsll((unsigned long long) __ballot(excl < need && incl >= need)) - 1;
                uint32_t below = excl, bin = 0, in_bin = 0;
                bool found = false;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!found && below + h[u] >= need) { found = true; bin = 4u * (uint32_t) lane + (uint32_t) u; in_bin = h[u]; }
                    else if (!found) below += h[u];
                }
                bin = (uint32_t) __shfl((int) bin, owner);
                in_bin = (uint32_t) __shfl((int) in_bin, owner);
                below = (uint32_t) __shfl((int) below, owner);
                prefix |= (uint64_t) bin << shift;
                pmask |= 255ull << shift;
                need -= below;
                wave_sync();                                                 // (hist is cleared again below)
                if (in_bin == need) break;                                   // the whole bin is taken
            }
            return prefix | ~pmask;
        };
        // the `want` smallest keys of D leave it and become S, sorted, unexpanded
        auto take = [&](uint32_t want) {
            wave_sync_global();
            const uint64_t t = want < n_disc ? threshold(want) : KEY_EMPTY;
            uint32_t kept = 0, sel = 0;
            for (uint32_t base = 0; base < n_disc; base += 64) {             // (writes never pass the reads: in place)
                const uint32_t i = base + (uint32_t) lane;
                const uint64_t key = i < n_disc ? Dq[i] : KEY_EMPTY;
                const bool s = i < n_disc && key <= t, kp = i < n_disc && key > t;
                const uint64_t sm = __ballot(s), km = __ballot(kp);
                const uint64_t below_me = (1ull << lane) - 1ull;
                if (s) S[sel + (uint32_t) __popcll(sm & below_me)] = key;
                if (kp) Dq[kept + (uint32_t) __popcll(km & below_me)] = key;
                sel += (uint32_t) __popcll(sm);
                kept += (uint32_t) __popcll(km);
            }
            n_disc = kept;
            count = sel;
            wave_sync_global();
            // bitonic sort of S[0, count): positions >= count act as +inf and are never touched
            uint32_t n2 = 1, lg = 0;
            while (n2 < count) { n2 <<= 1; ++lg; }
            for (uint32_t ls = 1; ls <= lg; ++ls) {
                const uint32_t size = 1u << ls, half = size >> 1;
                for (uint32_t tt = (uint32_t) lane; tt < n2 / 2; tt += 64) {  // flip: i against its mirror in the block
                    const uint32_t i = ((tt >> (ls - 1)) << ls) + (tt & (half - 1)), j = i ^ (size - 1);
                    if (j < count) {
                        const uint64_t a = S[i], b = S[j];
                        if (a > b) { S[i] = b; S[j] = a; }
                    }
                }
                wave_sync();
                for (uint32_t ld = ls - 1; ld >= 1; --ld) {
                    const uint32_t stride = 1u << (ld - 1);
                    for (uint32_t tt = (uint32_t) lane; tt < n2 / 2; tt += 64) {
                        const uint32_t i = ((tt >> (ld - 1)) << ld) + (tt & (stride - 1)), j = i + stride;
                        if (j < count) {
                            const uint64_t a = S[i], b = S[j];
                            if (a > b) { S[i] = b; S[j] = a; }
                        }
                    }
                    wave_sync();
                }
            }
            for (uint32_t i = (uint32_t) lane; i < count; i += 64) X[i] = 0;
            wave_sync();
        };
        while (out < p.k && n_disc > 0) {
            if (visited_l0 >= p.max_scan) {                                  // the drain: D in order, 64 keys at a time
                take(n_disc < 64u ? n_disc : 64u);
            } else {                                                         // ResumeScanItems
                take(n_disc < p.ef ? n_disc : p.ef);
                search_layer(0, p.ef, false);
                if (overflow) break;
            }
            emit(count);
        }
        if (p.out_visited && lane == 0) p.out_visited[so] = visited_l0;
        if (overflow) {
            fail_query();
            return;
        }
    }
    if (out > p.k) out = p.k;
    write_empty(out);
    if (lane == 0) p.out_count[so] = (int32_t) out;
}

__global__ __launch_bounds__(256) void hnsw_search_kernel(const HnswParams p) { hnsw_search_body<false>(p); }
__global__ __launch_bounds__(256) void hnsw_bit_search_kernel(const HnswParams p) { hnsw_search_body<false, ROWS_BIT>(p); }
__global__ __launch_bounds__(256) void hnsw_half_search_kernel(const HnswParams p) { hnsw_search_body<false, ROWS_HALF>(p); }

// pgvector's iterative index scan (see the header comment): every round of a query inside the one launch
__global__ __launch_bounds__(256) void hnsw_iterative_kernel(const HnswParams p) { hnsw_search_body<true>(p); }
__global__ __launch_bounds__(256) void hnsw_bit_iterative_kernel(const HnswParams p) { hnsw_search_body<true, ROWS_BIT>(p); }
__global__ __launch_bounds__(256) void hnsw_half_iterative_kernel(const HnswParams p) { hnsw_search_body<true, ROWS_HALF>(p); }

// K4s: the search and the iterative scan over a sparse corpus
__global__ __launch_bounds__(256) void hnsw_sparse_search_kernel(const HnswParams p) { hnsw_search_body<false, ROWS_SPARSE>(p); }
__global__ __launch_bounds__(256) void hnsw_sparse_iterative_kernel(const HnswParams p) { hnsw_search_body<true, ROWS_SPARSE>(p); }

// (q_chunks: HnswParams::q_chunks, the rounded query of a K4h wave; 0 for every other kernel)
inline size_t hnsw_lds_fixed(uint32_t caps, uint32_t q_chunks = 0)
{
    return ((((size_t) caps * 8 + ((caps + 15) & ~15u) + (size_t) HN_NBR * 8 + (size_t) HN_UPPER_VISITED * 4) + 15) & ~(size_t) 15) +
           (size_t) q_chunks * 16;
}

// visited form, table size, queries per workgroup for a graph of n_elem elements searched with ef (see the header comment);
// force_global: the re-run of queries whose LDS hash overflowed.  false: ef too large for the LDS
inline bool hnsw_plan(HnswParams& p, bool force_global)
{
    const size_t fixed = hnsw_lds_fixed(p.caps, p.q_chunks);
    if (fixed > HN_LDS_BUDGET) return false;
    const size_t bitmap_bytes = (((size_t) p.n_elem + 31) / 32) * 4;
    const size_t room = HN_LDS_BUDGET - fixed;
    size_t vis_bytes = 0;
    if (force_global) {
        p.vis_mode = VIS_GLOBAL;
        p.vis_words = (uint32_t) (bitmap_bytes / 4);
    } else if (bitmap_bytes <= room && bitmap_bytes <= 128 * 1024) {
        p.vis_mode = VIS_LDS_BITMAP;
        p.vis_words = (uint32_t) (bitmap_bytes / 4);
        vis_bytes = bitmap_bytes;
    } else {
        size_t want = 2048;                                                  // slots: ~4/3 x (48 visits per unit of ef + slack), power of two
        while (want < (size_t) p.ef * 64 + 4096) want <<= 1;
        while (want * 4 > room && want > 1024) want >>= 1;
        if (want * 4 > room) {
            p.vis_mode = VIS_GLOBAL;
            p.vis_words = (uint32_t) (bitmap_bytes / 4);
        } else {
            p.vis_mode = VIS_LDS_HASH;
            p.vis_words = (uint32_t) want;
            vis_bytes = want * 4;
        }
    }
    p.lds_per_query = (uint32_t) ((fixed + vis_bytes + 15) & ~(size_t) 15);
    const size_t fit = HN_LDS_BUDGET / p.lds_per_query;
    // several waves per workgroup only while that does not cost residency: ~40 KB per workgroup keeps 4 workgroups per CU
    p.qpb = (uint32_t) (fit >= 4 && (size_t) p.lds_per_query * 4 <= 40 * 1024 ? 4 : fit >= 2 && (size_t) p.lds_per_query * 2 <= 40 * 1024 ? 2 : 1);
    return true;
}

// the iterative kernel: S and the rest as above plus the radix-select histogram; the layer-0 visited set is the LDS bitmap
// when it fits and the global bitmap otherwise (force_global: always).  false: ef too large for the LDS
inline bool hnsw_plan_iterative(HnswParams& p, bool force_global)
{
    const size_t fixed = hnsw_lds_fixed(p.caps, p.q_chunks) + (size_t) HN_HIST * 4;
    if (fixed > HN_LDS_BUDGET) return false;
    const size_t bitmap_bytes = (((size_t) p.n_elem + 31) / 32) * 4;
    const size_t room = HN_LDS_BUDGET - fixed;
    size_t vis_bytes = 0;
    p.vis_words = (uint32_t) (bitmap_bytes / 4);
    if (!force_global && bitmap_bytes <= room && bitmap_bytes <= 128 * 1024) {
        p.vis_mode = VIS_LDS_BITMAP;
        vis_bytes = bitmap_bytes;
    } else
        p.vis_mode = VIS_GLOBAL;
    p.lds_per_query = (uint32_t) ((fixed + vis_bytes + 15) & ~(size_t) 15);
    const size_t fit = HN_LDS_BUDGET / p.lds_per_query;
    p.qpb = (uint32_t) (fit >= 4 && (size_t) p.lds_per_query * 4 <= 40 * 1024 ? 4 : fit >= 2 && (size_t) p.lds_per_query * 2 <= 40 * 1024 ? 2 : 1);
    return true;
}

template <bool ITER, int ROWS>
inline hipError_t launch_hnsw_rows(const HnswParams& p, hipStream_t s)
{
    if (p.nq == 0) return hipSuccess;
    const size_t lds = (size_t) p.lds_per_query * p.qpb;
    if (lds > HN_LDS_BUDGET || p.qpb < 1 || p.qpb > 4) return hipErrorInvalidValue;
    const auto kernel = ROWS == ROWS_BIT    ? (ITER ? hnsw_bit_iterative_kernel : hnsw_bit_search_kernel)
                        : ROWS == ROWS_HALF ? (ITER ? hnsw_half_iterative_kernel : hnsw_half_search_kernel)
                        : ROWS == ROWS_SPARSE ? (ITER ? hnsw_sparse_iterative_kernel : hnsw_sparse_search_kernel)
                                            : (ITER ? hnsw_iterative_kernel : hnsw_search_kernel);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((p.nq + p.qpb - 1) / p.qpb), dim3(64 * p.qpb), lds, s, p);
    return hipGetLastError();
}

// K4 (F32), K4h (HALF) or K4b (BIT); iterative: the iterative-scan kernel of that row format
inline hipError_t launch_hnsw(RowFormat f, bool iterative, const HnswParams& p, hipStream_t s)
{
    switch (f) {
    case RowFormat::F32:  return iterative ? launch_hnsw_rows<true, ROWS_F32>(p, s) : launch_hnsw_rows<false, ROWS_F32>(p, s);
    case RowFormat::HALF: return iterative ? launch_hnsw_rows<true, ROWS_HALF>(p, s) : launch_hnsw_rows<false, ROWS_HALF>(p, s);
    case RowFormat::BIT:  return iterative ? launch_hnsw_rows<true, ROWS_BIT>(p, s) : launch_hnsw_rows<false, ROWS_BIT>(p, s);
    case RowFormat::SPARSE:
        if (p.sp_slots < 2 || (p.sp_slots & (p.sp_slots - 1)) != 0 || (p.q_chunks != 0 && p.q_chunks != p.sp_slots / 2) ||
            (p.sp_lanes != 4 && p.sp_lanes != 16 && p.sp_lanes != 64))
            return hipErrorInvalidValue;
        return iterative ? launch_hnsw_rows<true, ROWS_SPARSE>(p, s) : launch_hnsw_rows<false, ROWS_SPARSE>(p, s);
    default:              return hipErrorInvalidValue;
    }
}

}  // namespace vsr
