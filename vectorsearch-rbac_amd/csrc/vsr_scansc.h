// vsr_scansc.h — K1sc: K1sm's shared passes over a sparse corpus with a COMPACT query block, for queries of up to 128 non-zeros.
//
// K1sm (vsr_scansm.h) keeps the pass's queries as the dense Qd[column][query]: 2 QW^2 sp_slots bytes, which at k = 100 leaves
// QW = 32 to queries of <= 8 non-zeros, QW = 16 up to 32, and nothing beyond.  Nearly all of Qd is zeros: a column has a value
// only for the queries that hold its index.  Here the block keeps the values alone, and one record per column to find them:
//   union table   K1sm's, as it stands: scansm_union_slots slots of (index, column), K1s's hash, linear probing, filled by
//                 compare-and-swap, columns numbered by the prefix count in slot order
//   rec           [columns] (mask, base), 8 bytes: bit q of mask = query q of the pass holds the index; base = the exclusive
//                 prefix sum of popcount(mask) over the columns in column order
//   vals          fp32, one per (query, non-zero): vals[base + popcount(mask & ((1 << q) - 1))] = query q's value at the index
// 12 bytes per column at the most instead of 4 QW: scansc_lds_bytes (vsr_scansm_sizing.h) grows as QW x sp_slots, so QW = 32 fits
// up to 64 non-zeros and QW = 16 up to 128 at k = 100.  Masks and bases depend on the keys alone (the columns do, see K1sm), so
// the layout is deterministic whichever thread wins a slot.
// Prologue (per workgroup, from what stage_sparse_kernel wrote: p.sp_tab, p.sp_qtot, p.q_norm2; no launch, no buffer of its own):
// 1. the indices are inserted; 2. the occupied slots are numbered (per-thread count, __shfl_up scan, four wave totals) and
// rec[0, columns) is cleared; 3. every (query, entry) ORs its bit into its column's mask (LDS atomic; pad queries, q >= q_count,
// have no entries and set no bit); 4. the same scan over popcount(mask) in column order gives the bases; 5. the values are
// written to their places.  A staged table holds an index once, so no two entries write one place.
// Scan: K1sm's loop, restated (as K1sm restates K2b's and K1m's skeleton: a fix to the vote / publish protocol belongs in all
// of them): lane (r, q) = (lane / QW, lane % QW), R = 64 / QW rows per step, offsets loaded by the lanes of permitted rows only,
// steps without a permitted row skipped, the next step's first entries requested early, rounds of 2 QW entries per row, ONE
// probe per entry, the miss term summed lane-locally and reduced by a butterfly at the end.  Only the hit path differs: the hit's
// (a, column) is broadcast as in K1sm; every lane of the row reads the column's record -- one address, a broadcast read --
// and lane q takes b = vals[base + rank of q in mask] if bit q is set, else 0; the set lanes read consecutive words (no bank
// conflict).  accum_sparse's terms then run as in K1sm with that b, so for a given QW the sums are K1sm's, in K1sm's order.
// Not here: QW = 64 (a 64-bit mask), queries of more than 128 non-zeros (the union table alone is 64 KB at sp_slots = 512),
// tau_init / sample passes, the rank map (launch_scansc_metric refuses p.rank: a view stays on K1s).
#pragma once
#include "vsr_scansm.h"                                      // union_lookup, and through it K1s's helpers; nothing of it is edited

namespace vsr {

struct ScColumn { uint32_t mask, base; };                    // which queries of the pass hold the index; where their values start

template <int METRIC, int QW>
__global__ __launch_bounds__(SM_THREADS, 2) void scansc_kernel(const ScanParams p)
{
    static_assert(QW == 16 || QW == 32, "lane = (row, query): QW divides 64, and a column's query mask and a row's hit mask fit 32 bits");
    static_assert(SM_WAVES * 64 * K2_VOTE_EVERY <= K2_SLACK, "append slack: one vote every K2_VOTE_EVERY tiles per wave");
    static_assert(sizeof(ScColumn) == 8, "scansc_lds_bytes counts 8 bytes per column record");
    constexpr int R = 64 / QW;                               // rows per step
    constexpr bool REST = METRIC == M_L2 || METRIC == M_L1;  // the metric has terms for unmatched entries
    constexpr uint32_t GM = QW == 32 ? 0xFFFFFFFFu : 0xFFFFu;

    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane % QW;
    const int r = lane / QW;
    const uint32_t qbit = 1u << q, below = qbit - 1u;        // the lane's query in a column mask; the queries before it

    // workgroup -> (pass, block of the pass), as in scansm_kernel
    uint32_t lo = 0, mapped_block = 0;
    if (p.block_map) {
        const uint2 m = p.block_map[blockIdx.x];
        if (m.x == 0xFFFFFFFFu) return;                                        // padding workgroup of a short XCD lane
        lo = m.x;
        mapped_block = m.y;
    } else {
        uint32_t hi = p.n_groups;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (p.groups[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
        }
    }
    const ScanGroup grp = p.groups[lo];
    const uint32_t local_block = p.block_map ? mapped_block : blockIdx.x - grp.block_begin;
    const auto g_tiles = as_global(grp.tiles);
    const auto g_bitmap = as_global(grp.bitmap);

    const uint32_t cap = p.cap, keep = p.k, slots = p.sp_slots, q_count = grp.q_count;
    const uint32_t uslots = scansm_union_slots(QW, slots), umask = uslots - 1u, ushift = (uint32_t) __clz((int) uslots) + 1u;
    const uint32_t max_cols = scansm_max_columns(QW, slots);                   // of columns, and of values

    // LDS (scansc_lds_bytes)
    uint64_t* sortbuf = reinterpret_cast<uint64_t*>(smem);                     // [cap]
    uint64_t* utab = sortbuf + cap;                                            // [uslots] index low, column high
    ScColumn* rec = reinterpret_cast<ScColumn*>(utab + uslots);                // [max_cols]
    float*    vals = reinterpret_cast<float*>(rec + max_cols);                 // [max_cols]
    uint32_t* wsum = reinterpret_cast<uint32_t*>(vals + max_cols);             // [SM_WAVES][4]: [0] columns, [1] values of a wave
    TopKCtrl* ctrl = reinterpret_cast<TopKCtrl*>(wsum + SM_WAVES * 4);         // [QW]
    double*   qtl = reinterpret_cast<double*>(ctrl + QW);                      // [QW] Q: sum q^2 (L2) / sum |q| (L1)
    float*    qnl = reinterpret_cast<float*>(qtl + QW);                        // [QW] |q|^2 in fp32 (cosine)
    uint32_t* flags = reinterpret_cast<uint32_t*>(qnl + QW);                   // [4] overflow votes
    uint32_t* uw = reinterpret_cast<uint32_t*>(utab);

    // ---- prologue: the pass's query block ----
    for (uint32_t qi = tid; qi < (uint32_t) QW; qi += SM_THREADS) {
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
        ctrl[qi].tau = KEY_EMPTY;
        ctrl[qi].count = 0;
        qtl[qi] = REST ? p.sp_qtot[2 * (size_t) slot + (METRIC == M_L1 ? 1 : 0)] : 0.0;
        qnl[qi] = METRIC == M_COSINE ? p.q_norm2[slot] : 0.0f;
    }
    if (tid < 4) flags[tid] = 0;
    for (uint32_t i = tid; i < uslots; i += SM_THREADS) utab[i] = (uint64_t) SPARSE_EMPTY;
    __syncthreads();
    const uint32_t n_src = q_count * slots, slog = 31u - (uint32_t) __clz((int) slots);
    const auto g_tab = as_global(reinterpret_cast<const uint64_t*>(p.sp_tab));    // a staged slot as 8 bytes: index low, value bits high
    for (uint32_t e = tid; e < n_src; e += SM_THREADS) {                       // 1. the distinct indices
        const uint32_t slot = p.q_slots[grp.q_begin + (e >> slog)];
        const uint32_t idx = (uint32_t) g_tab[(size_t) slot * slots + (e & (slots - 1u))];
        if (idx == SPARSE_EMPTY) continue;
        uint32_t h = (idx * SPARSE_HASH_MUL) >> ushift;
        for (;;) {
            const uint32_t prev = atomicCAS(&uw[2u * h], SPARSE_EMPTY, idx);
            if (prev == SPARSE_EMPTY || prev == idx) break;
            h = (h + 1u) & umask;
        }
    }
    __syncthreads();
    // the exclusive prefix of a per-thread count over the workgroup's threads in thread order, and the total (in wsum[.][which])
    auto scan = [&](uint32_t cnt, int which, uint32_t& total) -> uint32_t {
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t) __shfl_up((int) incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave * 4 + which] = incl;
        __syncthreads();
        uint32_t excl = incl - cnt;
        total = 0;
        for (int w = 0; w < SM_WAVES; ++w) {
            const uint32_t ws = wsum[w * 4 + which];
            if (w < wave) excl += ws;
            total += ws;
        }
        return excl;
    };
    // 2. columns in slot order: thread t numbers slots [t per, (t + 1) per)
    const uint32_t per = uslots > (uint32_t) SM_THREADS ? uslots / SM_THREADS : 1u;
    const uint32_t s0 = (uint32_t) tid * per;
    uint32_t cnt = 0, ncols, nvals;
    for (uint32_t j = 0; j < per; ++j)
        if (s0 + j < uslots && uw[2u * (s0 + j)] != SPARSE_EMPTY) ++cnt;
    uint32_t col = scan(cnt, 0, ncols);
    for (uint32_t j = 0; j < per; ++j)
        if (s0 + j < uslots && uw[2u * (s0 + j)] != SPARSE_EMPTY) uw[2u * (s0 + j) + 1u] = col++;
    // (cannot happen: more distinct indices than the staged tables can hold.  Nothing is scanned then, the lists come out empty)
    bool broken = ncols > max_cols;
    if (broken) ncols = 0;
    for (uint32_t i = tid; i < ncols; i += SM_THREADS) rec[i] = ScColumn{0u, 0u};
    __syncthreads();
    const auto ltab = (lds_u64) utab;
    for (uint32_t e = tid; e < n_src && !broken; e += SM_THREADS) {            // 3. who holds which column
        const uint32_t qi = e >> slog;
        const uint32_t slot = p.q_slots[grp.q_begin + qi];
        const uint32_t idx = (uint32_t) g_tab[(size_t) slot * slots + (e & (slots - 1u))];
        uint32_t c;
        if (union_lookup(ltab, umask, ushift, idx, c)) atomicOr(&rec[c].mask, 1u << qi);
    }
    __syncthreads();
    // 4. bases in column order: thread t sums columns [t cper, (t + 1) cper)
    const uint32_t cper = max_cols > (uint32_t) SM_THREADS ? max_cols / SM_THREADS : 1u;
    const uint32_t c0 = (uint32_t) tid * cper;
    cnt = 0;
    for (uint32_t j = 0; j < cper; ++j)
        if (c0 + j < ncols) cnt += (uint32_t) __popc(rec[c0 + j].mask);
    uint32_t base = scan(cnt, 1, nvals);
    for (uint32_t j = 0; j < cper; ++j)
        if (c0 + j < ncols) {
            rec[c0 + j].base = base;
            base += (uint32_t) __popc(rec[c0 + j].mask);
        }
    broken = broken || nvals > max_cols;                                       // (cannot happen either: a staged table is at most half full)
    if (broken && tid == 0) atomicOr(p.err, 2u);
    __syncthreads();
    for (uint32_t e = tid; e < n_src && !broken; e += SM_THREADS) {            // 5. the values, only now
        const uint32_t qi = e >> slog;
        const uint32_t slot = p.q_slots[grp.q_begin + qi];
        const uint64_t ent = g_tab[(size_t) slot * slots + (e & (slots - 1u))];
        uint32_t c;
        if (union_lookup(ltab, umask, ushift, (uint32_t) ent, c)) {
            const ScColumn cr = rec[c];
            vals[cr.base + (uint32_t) __popc(cr.mask & ((1u << qi) - 1u))] = __uint_as_float((uint32_t) (ent >> 32));
        }
    }
    __syncthreads();

    // ---- the scan ----
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t iters = broken ? 0u : ((t1 - t0) + SM_WAVES - 1) / SM_WAVES;
    const uint32_t trigger = cap - K2_SLACK;
    uint64_t* cand = p.cand + (size_t) (grp.partial_begin + local_block) * cand_pitch(cap);
    const size_t cand_qstride = (size_t) grp.n_blocks * cand_pitch(cap);
    const auto g_off = as_global(p.sp_off);
    const auto g_rows = as_global(reinterpret_cast<const u32x4*>(p.rows));     // two entries per 16 bytes
    const auto g_norm = as_global(p.norm2);
    const bool qlive = (uint32_t) q < q_count;
    const double my_qt = qtl[q];
    const float my_qn = qnl[q];
    uint64_t* my_cand = cand + (size_t) q * cand_qstride;                      // (written by live query columns only)
    const u32x4 pad = {SPARSE_EMPTY, 0u, SPARSE_EMPTY, 0u};

    uint32_t round = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t t = t0 + it * SM_WAVES + wave;
        uint32_t start = 0;
        uint64_t mask = 0;
        if (t < t1) {
            uint32_t nrows;
            if (g_tiles) {
                const uint2 tl = load_tile(g_tiles, t);
                start = tl.x;
                nrows = tl.y;
            } else {
                start = t * 64u;
                nrows = p.n_rows - start < 64u ? p.n_rows - start : 64u;
            }
            if (nrows > 0 && (start >= p.n_rows || nrows > p.n_rows - start || nrows > 64u)) {               // cannot happen; never read past the corpus
                if (lane == 0) atomicOr(p.err, 1u);
                nrows = 0;
            }
            mask = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
            if (g_bitmap) mask &= bitmap_window(g_bitmap, start);
        }

        if (mask) {                                                            // wave-uniform
            // the tile's offsets, one row per lane, permitted rows only; the steps take them by shuffle
            uint64_t ob = 0;
            uint32_t olen = 0;
            float orn = 0.0f;
            if ((mask >> lane) & 1ull) {
                ob = g_off[start + lane] >> 1;
                olen = (uint32_t) ((g_off[start + lane + 1] >> 1) - ob);
                if constexpr (METRIC == M_COSINE) orn = g_norm[start + lane];
            }
            // entry pairs [pb, pb + len) of the lane's row at a step (len = 0: not permitted) and the lane's pair of round 0
            auto fetch = [&](int step_, uint64_t& pb_, uint32_t& len_, float& rn_) -> u32x4 {
                const int row_ = step_ * R + r;
                pb_ = __shfl(ob, row_);
                len_ = __shfl(olen, row_);
                rn_ = METRIC == M_COSINE ? __shfl(orn, row_) : 0.0f;
                u32x4 x_ = pad;
                if ((uint32_t) q < len_) x_ = g_rows[pb_ + (uint32_t) q];
                return x_;
            };
            uint64_t pb, pbn = 0;
            uint32_t len, lenn = 0;
            float rn, rnn = 0.0f;
            u32x4 x = fetch(0, pb, len, rn);
            for (int step = 0; step < QW; ++step) {
                u32x4 xn = pad;
                if (step + 1 < QW) xn = fetch(step + 1, pbn, lenn, rnn);       // in flight under this step
                if ((mask >> (step * R)) & ((1ull << R) - 1ull)) {             // a permitted row in this step (wave-uniform)
                    const int row = step * R + r;
                    const bool ok = (mask >> row) & 1ull;
                    float s = 0.0f, miss = 0.0f;
                    double m = 0.0;
                    // the hits among one entry of every lane: (a, column) to the row's lanes; lane q finds its b through the record
                    auto hits = [&](bool h, float a, uint32_t c) {
                        uint64_t hm = __ballot(h);
                        uint32_t gm = (uint32_t) (hm >> (r * QW)) & GM;
                        while (hm) {                                           // wave-uniform
                            const bool has = gm != 0;
                            const int src = r * QW + (has ? __ffs((int) gm) - 1 : 0);
                            const float av = __shfl(a, src);
                            const uint32_t cv = (uint32_t) __shfl((int) c, src);
                            if (has) {
                                const ScColumn cr = rec[cv];                   // one address per row: a broadcast read
                                float b = 0.0f;
                                if (cr.mask & qbit) b = vals[cr.base + (uint32_t) __popc(cr.mask & below)];
                                if constexpr (METRIC == M_L2) {
                                    const float d = av - b;
                                    s = fmaf(d, d, s);
                                    m += (double) b * (double) b;
                                } else if constexpr (METRIC == M_L1) {
                                    s += fabsf(av - b);
                                    m += fabs((double) b);
                                } else {
                                    s = fmaf(av, b, s);
                                }
                                gm &= gm - 1u;
                            }
                            hm = __ballot(gm != 0);
                        }
                    };
                    for (uint32_t e0 = 0;; e0 += QW) {                         // rounds of 2 QW entries per row
                        const float a0 = __uint_as_float(x.y), a1 = __uint_as_float(x.w);
                        uint32_t k0, k1;
                        const bool h0 = union_lookup(ltab, umask, ushift, x.x, k0);
                        const bool h1 = union_lookup(ltab, umask, ushift, x.z, k1);
                        if constexpr (METRIC == M_L2) {
                            if (!h0) miss = fmaf(a0, a0, miss);
                            if (!h1) miss = fmaf(a1, a1, miss);
                        } else if constexpr (METRIC == M_L1) {
                            if (!h0) miss += fabsf(a0);
                            if (!h1) miss += fabsf(a1);
                        }
                        hits(h0, a0, k0);
                        hits(h1, a1, k1);
                        if (__ballot(e0 + QW < len) == 0) break;               // wave-uniform
                        x = pad;
                        if (e0 + QW + (uint32_t) q < len) x = g_rows[pb + e0 + QW + (uint32_t) q];
                    }
                    if constexpr (REST) {
#pragma unroll
                        for (int d = QW / 2; d >= 1; d >>= 1) miss += __shfl_xor(miss, d);
                        s += miss;
                    }
                    const bool live = ok && qlive;
                    float v = 0.0f;
                    if (live) {
                        if constexpr (REST) {
                            const float rest = (float) (my_qt - m);
                            v = s + (rest > 0.0f ? rest : 0.0f);
                        } else {
                            v = rank_value<METRIC>(s, rn, my_qn);              // the division: permitted pairs only
                        }
                    }
                    const uint64_t key = make_key(v, start + (uint32_t) row);
                    const uint64_t tau = lds_peek(&ctrl[q].tau);
                    if (live && key < tau) {
                        const uint32_t at = atomicAdd(&ctrl[q].count, 1u);
                        if (at < cap) my_cand[at] = key;
                        else atomicOr(p.err, 2u);                              // cannot happen (append slack protocol)
                    }
                }
                x = xn;
                pb = pbn;
                len = lenn;
                rn = rnn;
            }
        }

        if (it + 1 < iters && (it + 1) % K2_VOTE_EVERY == 0) {                 // workgroup-uniform
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
                for (uint32_t qs = 0; qs < q_count; ++qs) {
                    const uint32_t n = ctrl[qs].count < cap ? ctrl[qs].count : cap;
                    if (n > trigger) {                                         // only the buffers that are filling up
                        uint64_t* cq = cand + (size_t) qs * cand_qstride;
                        for (uint32_t i = tid; i < n; i += SM_THREADS) sortbuf[i] = cq[i];
                        __syncthreads();
                        if (tid == 0) ctrl[qs].count = n;
                        __syncthreads();
                        topk_compact<SM_THREADS>(sortbuf, &ctrl[qs], keep, tid, false);
                        for (uint32_t i = tid; i < keep; i += SM_THREADS) cq[i] = sortbuf[i];
                        __syncthreads();
                    }
                }
            }
        }
    }

    // ---- publish this workgroup's k best per query ----
    __syncthreads();
    for (uint32_t qs = 0; qs < q_count; ++qs) {
        const uint32_t n = ctrl[qs].count < cap ? ctrl[qs].count : cap;
        const uint64_t* cq = cand + (size_t) qs * cand_qstride;
        for (uint32_t i = tid; i < n; i += SM_THREADS) sortbuf[i] = cq[i];
        __syncthreads();
        if (tid == 0) ctrl[qs].count = n;
        __syncthreads();
        topk_compact<SM_THREADS>(sortbuf, &ctrl[qs], keep, tid, false);
        const uint32_t m = ctrl[qs].count < keep ? ctrl[qs].count : keep;
        uint64_t* dst = p.partial + (size_t) (grp.partial_begin + qs * grp.n_blocks + local_block) * p.kp;
        for (uint32_t i = tid; i < p.kp; i += SM_THREADS) dst[i] = i < m ? sortbuf[i] : KEY_EMPTY;
        __syncthreads();
    }
}

template <int METRIC>
hipError_t launch_scansc_metric(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    if (!p.cand || !p.sp_off || !p.sp_tab || !p.sp_qtot || !p.q_norm2 || p.rank || (METRIC == M_COSINE && !p.norm2) || p.sp_slots < 2 ||
        (p.sp_slots & (p.sp_slots - 1)) != 0 || (p.qmax != 16 && p.qmax != 32) || p.cap < 2 * K2_SLACK)
        return hipErrorInvalidValue;
    const size_t lds = scansc_lds_bytes((int) p.qmax, p.sp_slots, p.cap);
    if (lds > SCANSM_LDS_BUDGET) return hipErrorInvalidValue;                  // (the planner plans such a call without K1sc)
    auto launch = [&](auto kern) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(SM_THREADS), lds, s, p);
        return hipGetLastError();
    };
    return p.qmax == 32 ? launch(scansc_kernel<METRIC, 32>) : launch(scansc_kernel<METRIC, 16>);
}

}  // namespace vsr
