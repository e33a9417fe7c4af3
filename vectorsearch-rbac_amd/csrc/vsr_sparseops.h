// vsr_sparseops.h — the distance stage of the graph kernels over a sparse corpus, shared by K4s (vsr_hnsw.h, ROWS_SPARSE) and the
// sparse build (vsr_hnsw_build.hip): one definition of the lane mapping and of the arithmetic, so that a build distance and a
// search distance of the same pair are the same fp32 bit pattern (the sparsevec_l2_ops / sparsevec_ip_ops / sparsevec_cosine_ops /
// sparsevec_l1_ops opclasses, pgvector/src/hnswutils.c:1352-1361, 1411-1422).
//
// Left-hand operand: K1s's open-addressing table of (index, value) slots (vsr_scans.h: a power of two >= 2 x nnz slots, empty
// slots hold index SPARSE_EMPTY, sparse_lookup's hash and linear probing) with the two double totals Q2 = sum v^2 and Q1 = sum |v|.
// The search wave copies the table stage_sparse_kernel made for its query into its own LDS (or reads it where staging wrote it when
// it does not fit); the build wave makes the table of the left-hand ROW itself (sparse_left_load) whenever that row changes.
// Right-hand operand: an element's CSR row, entries sp_off[row] .. sp_off[row + 1] of interleaved (index, value) pairs, an even
// count of them (pad entries: index SPARSE_EMPTY, value 0), read as 16-byte pairs.
// Arithmetic: K1s's accum_sparse -- fp32 s over the row's entries, double m over the hits, L2 / L1 add the rest term
// (float) (Q - m) clamped at 0 (the left-hand entries no row entry met), a butterfly inside the lane group, fp32 and double.
#pragma once
#include "vsr_device.h"
#include "vsr_scans.h"
#include "vsr_halfops.h"

namespace vsr {

constexpr int HNSW_SPARSE_MAX_NNZ = 1000;    // HNSW_MAX_NNZ (hnsw.h): non-zeros of an indexed sparsevec

// Distances of one sparse vector (the table `tab` of mask + 1 slots, shift = 32 - log2 slots; q_tot: Q2 for L2, Q1 for L1) to `cnt`
// elements, for the graph kernels: ids[c] names an element, elem_row (may be nullptr: element e is row e) the row holding its
// entries.  G lanes share a row (4, 16 or 64: the corpus's entry-count class, sparse_lpr_for_mean_nnz) and stride over its entry
// pairs, so 64 / G rows are in flight per wave step.  A lane reads entry pairs of its own row only, between that row's two
// offsets; an id past cnt is never dereferenced (its lanes run an empty loop and only take part in the shuffles).  out[c] is the
// index distance -- L2: squared, L1: the sum, inner product and cosine: the negated sum -- written by the group's first lane; the
// caller synchronises the wave.  Nothing here depends on where in the table an entry lies: the sums run in entry order.
template <int METRIC, class TAB>
__device__ __forceinline__ void sparse_graph_distances(const float4* rows, const uint64_t* sp_off, uint32_t G, const int32_t* elem_row,
                                                       TAB tab, uint32_t mask, uint32_t shift, double q_tot, const int32_t* ids, int cnt,
                                                       float* out, int lane)
{
    constexpr bool REST = METRIC == M_L2 || METRIC == M_L1;
    const uint32_t per = 64u / G, gl = (uint32_t) lane & (G - 1u), grp = (uint32_t) lane / G;
    const auto g_rows = as_global(reinterpret_cast<const u32x4*>(rows));      // two entries per 16 bytes
    const auto g_off = as_global(sp_off);
    for (int c0 = 0; c0 < cnt; c0 += (int) per) {
        const int c = c0 + (int) grp;
        uint64_t pb = 0, pe = 0;                                               // entry pairs [pb, pe) of the lane's row
        if (c < cnt) {
            const int64_t row = elem_row ? (int64_t) elem_row[ids[c]] : (int64_t) ids[c];
            pb = g_off[row] >> 1;
            pe = g_off[row + 1] >> 1;
        }
        float s = 0.0f;
        double m = 0.0;
        for (uint64_t e = pb + gl; e < pe; e += G) {
            const u32x4 x = g_rows[e];
            bool h0, h1;
            const float b0 = sparse_lookup(tab, mask, shift, x.x, h0);
            const float b1 = sparse_lookup(tab, mask, shift, x.z, h1);
            accum_sparse<METRIC>(s, m, __uint_as_float(x.y), b0, h0);
            accum_sparse<METRIC>(s, m, __uint_as_float(x.w), b1, h1);
        }
        for (uint32_t d = G >> 1; d >= 1u; d >>= 1) {
            s += __shfl_xor(s, (int) d);
            if constexpr (REST) m += __shfl_xor(m, (int) d);
        }
        if (gl == 0u && c < cnt) {
            float v = s;
            if constexpr (REST) {
                const float rest = (float) (q_tot - m);
                if (rest > 0.0f) v += rest;
            }
            out[c] = hnsw_rank_value(METRIC, v);
        }
    }
}

// metric dispatch of the above (cosine: unit rows, ranked by the negated inner product); q2 / q1: the table's double totals
template <class TAB>
__device__ __forceinline__ void sparse_graph_distances_metric(int metric, const float4* rows, const uint64_t* sp_off, uint32_t G,
                                                              const int32_t* elem_row, TAB tab, uint32_t mask, uint32_t shift, double q2,
                                                              double q1, const int32_t* ids, int cnt, float* out, int lane)
{
    if (metric == M_L2) sparse_graph_distances<M_L2>(rows, sp_off, G, elem_row, tab, mask, shift, q2, ids, cnt, out, lane);
    else if (metric == M_L1) sparse_graph_distances<M_L1>(rows, sp_off, G, elem_row, tab, mask, shift, q1, ids, cnt, out, lane);
    else sparse_graph_distances<M_IP>(rows, sp_off, G, elem_row, tab, mask, shift, 0.0, ids, cnt, out, lane);
}

// The left-hand operand of a BUILD wave: the table of corpus row `row` in the wave's LDS, its totals, and which row it holds.
struct SparseLeft {
    uint64_t* tab = nullptr;                 // [slots] in the wave's LDS: index low, value bits high
    uint32_t  slots = 0;                     // a power of two >= 2 x the corpus's largest row
    int64_t   row = -1;                      // the row the table holds (-1: none yet)
    double    q2 = 0.0, q1 = 0.0;
};

// Rebuilds the wave's table from `row` when it holds another: clears the slots, inserts the row's entries by LDS compare-and-swap
// on the index word (stage_sparse_kernel's insertion; which slot of a probe chain an entry wins depends on lane timing, what a
// lookup returns does not) and sums Q2 and Q1 in double in the same pass -- lane l takes entries l, l + 64, .. and the partials
// meet in stage_sparse_kernel's butterfly, so the totals are the bits staging would give the same vector as a query.
__device__ __forceinline__ void sparse_left_load(SparseLeft& L, const float4* rows, const uint64_t* sp_off, int64_t row, int lane)
{
    if (L.row == row) return;                                                 // (wave-uniform)
    L.row = row;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();                                          // the lookups of the previous table are done
    uint32_t* words = reinterpret_cast<uint32_t*>(L.tab);
    for (uint32_t i = (uint32_t) lane; i < L.slots; i += 64) L.tab[i] = (uint64_t) SPARSE_EMPTY;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t beg = sp_off[row], end = sp_off[row + 1];
    const uint2* ent = reinterpret_cast<const uint2*>(rows);
    const uint32_t mask = L.slots - 1u, shift = (uint32_t) __clz((int) L.slots) + 1u;
    double q2 = 0.0, q1 = 0.0;
    for (uint64_t e = beg + (uint32_t) lane; e < end; e += 64) {
        const uint2 x = ent[e];
        if (x.x == SPARSE_EMPTY) continue;                                    // the pad entry of an odd row
        uint32_t h = (x.x * SPARSE_HASH_MUL) >> shift;
        for (;;) {
            const uint32_t prev = atomicCAS(&words[2u * h], SPARSE_EMPTY, x.x);
            if (prev == SPARSE_EMPTY || prev == x.x) break;
            h = (h + 1u) & mask;
        }
        words[2u * h + 1u] = x.y;
        const double v = (double) __uint_as_float(x.y);
        q2 += v * v;
        q1 += fabs(v);
    }
    for (int mm = 32; mm >= 1; mm >>= 1) {
        q2 += __shfl_xor(q2, mm);
        q1 += __shfl_xor(q1, mm);
    }
    L.q2 = q2;
    L.q1 = q1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace vsr
