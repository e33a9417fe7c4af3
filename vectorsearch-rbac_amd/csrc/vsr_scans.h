// vsr_scans.h — K1s: K1 (vsr_scan.h) over a sparse corpus: sparsevec distance + RBAC permission test + running top-k.
//
// Replaces, for a whole ORDER BY col <-> $1 / <#> / <=> / <+> LIMIT k scan over a sparsevec column, the per-row calls of
//   pgvector/src/sparsevec.c:803-846 SparsevecL2SquaredDistance, :882-913 SparsevecInnerProduct,
//   :948-988 sparsevec_cosine_distance, :993-1037 sparsevec_l1_distance.
//
// K1's skeleton, restated as vsr_scanb.h restates it: ScanParams / ScanGroup passes found by block_begin, tile descriptors and
// the 64-bit bitmap window, the LDS candidate list with topk_append / topk_compact and the overflow vote, partial lists of kp
// keys for K5.  What differs is the row: entries p.sp_off[r] .. p.sp_off[r + 1] of interleaved (index, value) pairs, an even
// count of them (pad entries: index SPARSE_EMPTY, value 0), so a lane loads two entries as 16 bytes.
// Shape: a tile is 64 consecutive internal rows -- one bitmap window; LPR lanes (4, 16 or 64, chosen per corpus at load from
// the mean entry count) share a row and stride over its entries; a wave walks its tile in LPR steps of 64 / LPR rows.  Only
// permitted rows are read.  Rows are not kept in registers (their length varies): every sub-batch of QI queries streams the
// tile's entries again, from L2 after the first.
// Arithmetic: the query is an open-addressing table (stage_sparse_kernel, vsr_sparse.hip).  Per row entry (i, a) and query the
// lane looks up b = q[i] (0 when absent): inner product / cosine s += a b; L2 s += (a - b)^2 and m += b^2 for a hit; L1
// s += |a - b| and m += |b| for a hit.  s is fp32, m is DOUBLE: the query entries no row entry met contribute
// (float) (Q - m), clamped at 0, Q the staged double total -- pgvector's set of terms in another order, with the cancellation
// kept out of fp32 (a near-duplicate row comes out ~0, never NaN).  A pad entry meets an empty slot: b = 0, m += 0, no special
// case.  The LPR lanes are reduced by a butterfly, fp32 and double; cosine's epilogue is K1's, with |row|^2 from the load.
// GLOBAL_TAB = false: the tables of the pass's queries are copied once per workgroup into LDS.  true: a table that does not fit
// SCAN_LDS_BUDGET beside the candidate lists (16000 non-zeros need 256 KiB) is read where staging wrote it; qmax = QI then.
// Not carried over from scan_kernel (a second kernel body, as K1b is: a fix to K1's top-k or overflow protocol belongs in all
// three): p.tau_init, p.sample_stride, p.rank and p.fused.
#pragma once
#include "vsr_scan.h"

namespace vsr {

using lds_u64 = const __attribute__((address_space(3))) uint64_t*;   // a table slot as one 8-byte word: index low, value bits high

// b = q[index] and whether the slot that ended the probe holds `index` (a pad entry "hits" an empty slot: value 0)
template <class TAB>
__device__ __forceinline__ float sparse_lookup(TAB tab, uint32_t mask, uint32_t shift, uint32_t index, bool& hit)
{
    uint32_t h = (index * SPARSE_HASH_MUL) >> shift;
    uint64_t t = tab[h];
    while ((uint32_t) t != index && (uint32_t) t != SPARSE_EMPTY) {            // load factor <= 1/2: an empty slot ends every chain
        h = (h + 1u) & mask;
        t = tab[h];
    }
    hit = (uint32_t) t == index;
    return hit ? __uint_as_float((uint32_t) (t >> 32)) : 0.0f;
}

template <int METRIC>
__device__ __forceinline__ void accum_sparse(float& s, double& m, float a, float b, bool hit)
{
    if constexpr (METRIC == M_L2) {
        const float d = a - b;
        s = fmaf(d, d, s);
        if (hit) m += (double) b * (double) b;
    } else if constexpr (METRIC == M_L1) {
        s += fabsf(a - b);
        if (hit) m += fabs((double) b);
    } else {
        s = fmaf(a, b, s);
    }
}

template <int METRIC, int LPR, int QI, bool GLOBAL_TAB>
__global__ __launch_bounds__(SCAN_THREADS, VSR_MINWAVES) void scans_kernel(const ScanParams p)
{
    constexpr int G = 64 / LPR;                              // rows per step
    constexpr int RW = 64;
    constexpr bool REST = METRIC == M_L2 || METRIC == M_L1;  // the metric has terms for unmatched query entries
    constexpr int SLACK = scan_slack(RW);
    static_assert(SCAN_WAVES * RW <= SLACK, "append slack: one vote per iteration");

    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = lane % LPR;
    const int g = lane / LPR;

    // ---- which (filter, query chunk) does this workgroup serve ----
    uint32_t lo = 0, hi = p.n_groups;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.groups[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
    }
    const ScanGroup grp = p.groups[lo];
    const auto g_tiles = as_global(grp.tiles);
    const auto g_bitmap = as_global(grp.bitmap);
    const uint32_t local_block = blockIdx.x - grp.block_begin;
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);

    const uint32_t cap = p.cap, k = p.k, qmax = p.qmax, slots = p.sp_slots;
    const uint32_t lds_slots = GLOBAL_TAB ? 0u : slots;
    const uint32_t tmask = slots - 1u, tshift = (uint32_t) __clz((int) slots) + 1u;   // 32 - log2 slots
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                        // [qmax][cap]
    TopKCtrl* ctrl = reinterpret_cast<TopKCtrl*>(keys + (size_t) qmax * cap);  // [qmax]
    uint2*    tlds = reinterpret_cast<uint2*>(ctrl + qmax);                    // [qmax][lds_slots]
    double*   qtl = reinterpret_cast<double*>(tlds + (size_t) qmax * lds_slots);   // [qmax] Q: sum q^2 (L2) / sum |q| (L1)
    float*    qnl = reinterpret_cast<float*>(qtl + qmax);                      // [qmax] |q|^2 in fp32 (cosine)
    uint32_t* flags = reinterpret_cast<uint32_t*>(qnl + qmax);                 // [4] overflow votes

    const uint32_t q_count = grp.q_count;
    const uint32_t n_sub = (q_count + QI - 1) / QI;                            // wave-uniform; n_sub * QI <= qmax (planner)
    for (uint32_t qi = tid; qi < qmax; qi += SCAN_THREADS) {
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
        ctrl[qi].tau = KEY_EMPTY;
        ctrl[qi].count = 0;
        qtl[qi] = REST ? p.sp_qtot[2 * (size_t) slot + (METRIC == M_L1 ? 1 : 0)] : 0.0;
        qnl[qi] = METRIC == M_COSINE ? p.q_norm2[slot] : 0.0f;
    }
    if (tid < 4) flags[tid] = 0;
    if constexpr (!GLOBAL_TAB) {
        for (uint32_t qi = 0; qi < n_sub * QI; ++qi) {                         // pad slots repeat query 0
            const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
            const uint2* src = p.sp_tab + (size_t) slot * slots;
            for (uint32_t i = tid; i < slots; i += SCAN_THREADS) tlds[(size_t) qi * slots + i] = src[i];
        }
    }
    __syncthreads();

    const uint32_t trigger = cap - SLACK;
    const uint32_t iters = ((t1 - t0) + SCAN_WAVES - 1) / SCAN_WAVES;
    const auto g_off = as_global(p.sp_off);
    const auto g_rows = as_global(reinterpret_cast<const u32x4*>(p.rows));     // two entries per 16 bytes

    uint32_t round = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t t = t0 + it * SCAN_WAVES + wave;
        uint32_t start = 0;
        uint64_t mask = 0;
        if (t < t1) {
            uint32_t nrows;
            if (g_tiles) {
                const uint2 tl = load_tile(g_tiles, t);
                start = tl.x;
                nrows = tl.y;
            } else {
                start = t * RW;
                nrows = p.n_rows - start < (uint32_t) RW ? p.n_rows - start : (uint32_t) RW;
            }
            mask = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
            if (g_bitmap) mask &= bitmap_window(g_bitmap, start);
        }

        if (mask) {                                                            // wave-uniform
            for (int step = 0; step < LPR; ++step) {
                const int row = step * G + g;
                if (((mask >> (step * G)) & (G == 64 ? ~0ull : (1ull << G) - 1ull)) == 0) continue;   // no permitted row in this step (wave-uniform)
                const bool ok = (mask >> row) & 1ull;
                // entry pairs [pb, pe) of the lane's row; a row that is not permitted is not read
                uint64_t pb = 0, pe = 0;
                float rn = 0.0f;
                if (ok) {
                    pb = g_off[start + row] >> 1;
                    pe = g_off[start + row + 1] >> 1;
                    if constexpr (METRIC == M_COSINE) rn = p.norm2[start + row];
                }
                for (uint32_t sb = 0; sb < n_sub; ++sb) {
                    float s[QI];
                    double m[QI];
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi) { s[qi] = 0.0f; m[qi] = 0.0; }
                    for (uint64_t e = pb + (uint32_t) l; e < pe; e += LPR) {
                        const u32x4 x = g_rows[e];
                        const float a0 = __uint_as_float(x.y), a1 = __uint_as_float(x.w);
#pragma unroll
                        for (int qi = 0; qi < QI; ++qi) {
                            const uint32_t qs = sb * QI + qi;
                            bool h0, h1;
                            float b0, b1;
                            if constexpr (GLOBAL_TAB) {
                                const auto tab = as_global(reinterpret_cast<const uint64_t*>(p.sp_tab) + (size_t) p.q_slots[grp.q_begin + (qs < q_count ? qs : 0)] * slots);
                                b0 = sparse_lookup(tab, tmask, tshift, x.x, h0);
                                b1 = sparse_lookup(tab, tmask, tshift, x.z, h1);
                            } else {
                                const auto tab = (lds_u64) reinterpret_cast<const uint64_t*>(tlds + (size_t) qs * slots);
                                b0 = sparse_lookup(tab, tmask, tshift, x.x, h0);
                                b1 = sparse_lookup(tab, tmask, tshift, x.z, h1);
                            }
                            accum_sparse<METRIC>(s[qi], m[qi], a0, b0, h0);
                            accum_sparse<METRIC>(s[qi], m[qi], a1, b1, h1);
                        }
                    }
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi) {
                        const uint32_t qs = sb * QI + qi;
#pragma unroll
                        for (int d = LPR / 2; d >= 1; d >>= 1) {
                            s[qi] += __shfl_xor(s[qi], d);
                            if constexpr (REST) m[qi] += __shfl_xor(m[qi], d);
                        }
                        const bool live = l == 0 && ok && qs < q_count;
                        float v = 0.0f;
                        if (live) {
                            if constexpr (REST) {
                                const float rest = (float) (qtl[qs] - m[qi]);
                                v = s[qi] + (rest > 0.0f ? rest : 0.0f);
                            } else {
                                v = rank_value<METRIC>(s[qi], rn, qnl[qs]);    // the division: permitted pairs only
                            }
                        }
                        const uint64_t key = make_key(v, start + row);
                        const uint64_t tau = lds_peek(&ctrl[qs].tau);
                        topk_append(keys + (size_t) qs * cap, &ctrl[qs], live && key < tau, key);
                    }
                }
            }
        }

        if (it + 1 < iters) {                                                  // workgroup-uniform
            // overflow vote: one barrier; flag slot `round % 3`, recycled two rounds later
            bool need = false;
            for (uint32_t qs = 0; qs < q_count; ++qs)
                need |= lds_peek(&ctrl[qs].count) > trigger;
            const uint32_t slot = round % 3;
            if (need && lane == 0) atomicOr(&flags[slot], 1u);
            __syncthreads();
            const bool any = lds_peek(&flags[slot]) != 0;
            if (tid == 0) flags[(round + 2) % 3] = 0;
            ++round;
            if (any) {
                for (uint32_t qs = 0; qs < q_count; ++qs)
                    if (ctrl[qs].count > trigger)                              // same value in every thread
                        topk_compact<SCAN_THREADS>(keys + (size_t) qs * cap, &ctrl[qs], k, tid, false);
            }
        }
    }

    // ---- publish this workgroup's k best per query ----
    __syncthreads();
    for (uint32_t qs = 0; qs < q_count; ++qs) {
        topk_compact<SCAN_THREADS>(keys + (size_t) qs * cap, &ctrl[qs], k, tid, false);
        const uint32_t n = ctrl[qs].count < k ? ctrl[qs].count : k;
        uint64_t* dst = p.partial + (size_t) (grp.partial_begin + qs * grp.n_blocks + local_block) * p.kp;
        for (uint32_t i = tid; i < p.kp; i += SCAN_THREADS) dst[i] = i < n ? keys[(size_t) qs * cap + i] : KEY_EMPTY;
    }
}

template <int METRIC, int LPR, int QI, bool GLOBAL_TAB>
hipError_t launch_scans_inst(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    const size_t lds = scans_lds_bytes(p.qmax, p.cap, GLOBAL_TAB ? 0u : p.sp_slots);
    auto kern = scans_kernel<METRIC, LPR, QI, GLOBAL_TAB>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(SCAN_THREADS), lds, s, p);
    return hipGetLastError();
}

// shape dispatch for one metric; instantiated once per metric in its own translation unit
template <int METRIC>
hipError_t launch_scans_metric(const ScanParams& p, int lpr, int qi, bool global_tab, uint32_t n_blocks, hipStream_t s)
{
    if (p.sp_slots < 2 || (p.sp_slots & (p.sp_slots - 1)) != 0 || p.qmax < (uint32_t) qi || p.qmax % (uint32_t) qi != 0 ||
        (global_tab && p.qmax != (uint32_t) qi))
        return hipErrorInvalidValue;
#define VSR_CASE(LPR_)                                                                                      \
    if (lpr == LPR_) {                                                                                      \
        if (qi == 1) return global_tab ? launch_scans_inst<METRIC, LPR_, 1, true>(p, n_blocks, s)           \
                                       : launch_scans_inst<METRIC, LPR_, 1, false>(p, n_blocks, s);         \
        if (qi == 4) return global_tab ? launch_scans_inst<METRIC, LPR_, 4, true>(p, n_blocks, s)           \
                                       : launch_scans_inst<METRIC, LPR_, 4, false>(p, n_blocks, s);         \
        return hipErrorInvalidValue;                                                                        \
    }
    VSR_CASE(4)
    VSR_CASE(16)
    VSR_CASE(64)
#undef VSR_CASE
    return hipErrorInvalidValue;
}

}  // namespace vsr
