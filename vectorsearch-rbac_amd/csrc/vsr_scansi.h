// vsr_scansi.h — K1si: the passes of a sparse corpus over its INVERTED image.  Exact; reads only what a query's own indices meet.
//
// K1s, K1sm and K1sc stream every stored entry of every permitted row and look it up in the pass's queries; nearly every probe
// misses, and what a missed entry adds to a distance is a constant of its row.  Here the corpus also lies inverted
// (vsr_sparse_inverted.hip): rows cut into row blocks of SI_RB rows, and per block the distinct indices of its rows (bterm,
// ascending), the start of each index's posting segment (boff, one end sentinel per block) and the postings (row in block,
// value), ordered by (block, index, row); per row A2 = sum a^2 and A1 = sum |a| in double.  A (row, query) pair then needs one
// double: t = sum over the entries both hold of a b (<#>, <=>, <->) or of |a| + |b| - |a - b| (<+>), and
//   <->  max(0, A2 + Q2 - 2 t)      <+>  max(0, A1 + Q1 - t)      <#>, <=>  t
// rounded to fp32 where K1s holds fp32 and ranked by K1s's functions (rank_value, make_key; output_distance downstream).
// Work split: the planner's passes, tile lists and workgroup ranges as they are (K1sm's skeleton, restated: a fix to the vote /
// publish protocol belongs in all of them).  A workgroup walks its tile run in CHUNKS: the tiles, or parts of tiles, whose rows
// lie in one row block.  A pass of up to SI_QMAX queries runs in rounds of SI_WAVES; in a round wave w serves query w alone:
//   prologue    (once per round) the wave collects the non-empty slots of its query's staged table (p.sp_tab: staging's
//               validation stays what it is) and sorts them ascending by index in its LDS (bitonic_sort_wave): which slot of
//               a probe chain an entry won in staging decides nothing here
//   accumulate  (per chunk) the wave clears acc[rows of the chunk], doubles in its own LDS; 64 terms at a time, every lane
//               finds its term in the block's bterm by binary search and, where the chunk covers part of the block only,
//               narrows the segment to the chunk's rows (postings ascend by row inside a segment); then the terms are walked
//               one after the other, in index order, the lanes striding over a term's postings: a segment holds a row once,
//               so acc[row] += .. is a plain read-modify-write -- no barrier, no atomic, one summation order whatever the
//               launch.  The next term's first postings are requested before the current term's are added
//   sweep       (per tile of the chunk) lane = row: bitmap window, A2 / A1 or |row|^2 of the permitted rows, the value, the
//               key, admission by key < tau on the full key, append to the query's global candidate buffer (p.cand)
// and every SI_VOTE_CHUNKS chunks the workgroup votes on compaction (through the LDS sort buffer, as K1sm); kp keys per query
// are published for K5.  Every offset read from the image is bounded by the image's sizes before use (p.err otherwise).
// Not here: the rank map (launch_scansi_metric refuses p.rank: a view stays on K1s), tau_init / sample passes.
#pragma once
#include "vsr_scans.h"
#include "vsr_scansi_sizing.h"

namespace vsr {

constexpr uint32_t SI_VOTE_CHUNKS = K2_SLACK / SI_RB;        // a chunk appends at most SI_RB keys per query

template <int METRIC>
__device__ __forceinline__ double scansi_term(float a, float b)
{
    if constexpr (METRIC == M_L1) return fabs((double) a) + fabs((double) b) - fabs((double) a - (double) b);
    else return (double) a * (double) b;
}

__device__ __forceinline__ void scansi_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int METRIC>
__global__ __launch_bounds__(SI_THREADS, 2) void scansi_kernel(const ScanParams p)
{
    static_assert(SI_VOTE_CHUNKS >= 1 && SI_VOTE_CHUNKS * SI_RB <= K2_SLACK, "append slack: one vote every SI_VOTE_CHUNKS chunks");
    static_assert(SI_QMAX % SI_WAVES == 0, "whole rounds");

    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // workgroup -> (pass, block of the pass), as in scansm_kernel
    uint32_t lo_g = 0, mapped_block = 0;
    if (p.block_map) {
        const uint2 m = p.block_map[blockIdx.x];
        if (m.x == 0xFFFFFFFFu) return;                                        // padding workgroup of a short XCD lane
        lo_g = m.x;
        mapped_block = m.y;
    } else {
        uint32_t hi_g = p.n_groups;
        while (hi_g - lo_g > 1) {
            const uint32_t mid = (lo_g + hi_g) >> 1;
            if (p.groups[mid].block_begin <= blockIdx.x) lo_g = mid; else hi_g = mid;
        }
    }
    const ScanGroup grp = p.groups[lo_g];
    const uint32_t local_block = p.block_map ? mapped_block : blockIdx.x - grp.block_begin;
    const auto g_tiles = as_global(grp.tiles);
    const auto g_bitmap = as_global(grp.bitmap);

    const uint32_t cap = p.cap, keep = p.k, slots = p.sp_slots;
    const uint32_t q_count = grp.q_count < (uint32_t) SI_QMAX ? grp.q_count : (uint32_t) SI_QMAX;

    // LDS (scansi_lds_bytes)
    uint64_t* sortbuf = reinterpret_cast<uint64_t*>(smem);                     // [cap]
    double*   acc_all = reinterpret_cast<double*>(sortbuf + cap);              // [SI_WAVES][SI_RB]
    uint64_t* terms_all = reinterpret_cast<uint64_t*>(acc_all + (size_t) SI_WAVES * SI_RB);   // [SI_WAVES][SI_MAX_TERMS] index high, value bits low
    TopKCtrl* ctrl = reinterpret_cast<TopKCtrl*>(terms_all + (size_t) SI_WAVES * SI_MAX_TERMS);   // [SI_QMAX]
    uint32_t* flags = reinterpret_cast<uint32_t*>(ctrl + SI_QMAX);             // [4] overflow votes
    double*   acc = acc_all + (size_t) wave * SI_RB;                           // the wave's own
    uint64_t* terms = terms_all + (size_t) wave * SI_MAX_TERMS;

    if (tid < SI_QMAX) {
        ctrl[tid].tau = KEY_EMPTY;
        ctrl[tid].count = 0;
    }
    if (tid < 4) flags[tid] = 0;
    __syncthreads();

    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t trigger = cap - K2_SLACK;
    uint64_t* cand = p.cand + (size_t) (grp.partial_begin + local_block) * cand_pitch(cap);
    const size_t cand_qstride = (size_t) grp.n_blocks * cand_pitch(cap);
    const auto g_tab = as_global(reinterpret_cast<const uint64_t*>(p.sp_tab));    // a staged slot as 8 bytes: index low, value bits high
    const auto g_post = as_global(reinterpret_cast<const uint64_t*>(p.si_post));  // a posting as 8 bytes: row in block low, value bits high
    const auto g_bterm = as_global(p.si_bterm);
    const auto g_boff = as_global(p.si_boff);
    const auto g_bbeg = as_global(p.si_bbeg);
    const auto g_a = as_global(p.si_a + (METRIC == M_L1 ? (size_t) p.n_rows : 0));
    const auto g_norm = as_global(p.norm2);
    const uint64_t n_post = p.si_n_post;
    const uint32_t n_blocks_img = (p.n_rows + SI_RB - 1) >> SI_RB_LOG2;

    // tile t of the pass: (first row, rows), never past the corpus
    auto tile_at = [&](uint32_t t) -> uint2 {
        uint2 tl;
        if (g_tiles) {
            tl = load_tile(g_tiles, t);
        } else {
            tl.x = t * 64u;
            tl.y = p.n_rows - tl.x < 64u ? p.n_rows - tl.x : 64u;
        }
        if (tl.y > 0 && (tl.x >= p.n_rows || tl.y > p.n_rows - tl.x || tl.y > 64u)) {                    // cannot happen
            if (lane == 0) atomicOr(p.err, 1u);
            tl.y = 0;
        }
        return tl;
    };

    uint32_t round = 0;
    for (uint32_t r0 = 0; r0 < q_count; r0 += SI_WAVES) {                      // workgroup-uniform
        const uint32_t qi = r0 + (uint32_t) wave;
        const bool serving = qi < q_count;                                     // wave-uniform
        // ---- prologue: the wave's query, its terms ascending by index ----
        uint32_t n_terms = 0;
        double qt = 0.0;
        float qn = 0.0f;
        if (serving) {
            const uint32_t slot = p.q_slots[grp.q_begin + qi];
            if constexpr (METRIC == M_L2 || METRIC == M_L1) qt = p.sp_qtot[2 * (size_t) slot + (METRIC == M_L1 ? 1 : 0)];
            if constexpr (METRIC == M_COSINE) qn = p.q_norm2[slot];
            scansi_wave_sync();                                                // the previous round's reads of `terms` are done
            for (uint32_t i0 = 0; i0 < slots; i0 += 64) {
                const uint64_t ent = i0 + (uint32_t) lane < slots ? g_tab[(size_t) slot * slots + i0 + (uint32_t) lane] : (uint64_t) SPARSE_EMPTY;
                const bool has = (uint32_t) ent != SPARSE_EMPTY;
                const uint64_t m = __ballot(has);
                const uint32_t at = n_terms + (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
                if (has && at < SI_MAX_TERMS) terms[at] = (ent << 32) | (ent >> 32);
                n_terms += (uint32_t) __popcll(m);
            }
            if (n_terms > SI_MAX_TERMS) {                                      // cannot happen (scansi_fits): nothing is accumulated
                if (lane == 0) atomicOr(p.err, 2u);
                n_terms = 0;
            }
            const uint32_t np = next_pow2(n_terms);
            for (uint32_t i = n_terms + (uint32_t) lane; i < np; i += 64) terms[i] = ~0ull;
            scansi_wave_sync();
            bitonic_sort_wave(terms, np, lane);
        }
        uint64_t* my_cand = cand + (size_t) (serving ? qi : 0) * cand_qstride; // (written by serving waves only)

        // ---- the chunks of the tile run ----
        uint32_t ta = t0, row_from = 0, chunk = 0;
        while (ta < t1) {                                                      // workgroup-uniform: every thread reads the same tiles
            const uint2 tf = tile_at(ta);
            const uint32_t rlo = tf.x > row_from ? tf.x : row_from;
            if (tf.y == 0 || rlo >= tf.x + tf.y) {                             // an empty tile, or one the last chunk finished
                ++ta;
                continue;
            }
            const uint32_t blk = rlo >> SI_RB_LOG2, lo = blk << SI_RB_LOG2;
            const uint32_t hi = p.n_rows - lo < SI_RB ? p.n_rows : lo + SI_RB;
            uint32_t tb = ta + 1, th = t1;                                     // the first tile that starts behind the block (starts ascend)
            while (tb < th) {
                const uint32_t mid = tb + ((th - tb) >> 1);
                const uint32_t ms = g_tiles ? load_tile(g_tiles, mid).x : mid * 64u;
                if (ms < hi) tb = mid + 1; else th = mid;
            }
            const uint2 tl = tile_at(tb - 1);
            uint32_t rhi = tl.x + tl.y < hi ? tl.x + tl.y : hi;
            if (rhi <= rlo || blk >= n_blocks_img) {                           // cannot happen: a tile list that does not ascend
                if (lane == 0) atomicOr(p.err, 4u);
                rhi = rlo;
            }

            if (serving && rhi > rlo) {
                // -- accumulate --
                const uint32_t z0 = rlo - lo, z1 = rhi - lo;
                scansi_wave_sync();                                            // the last chunk's sweep has read its sums
                for (uint32_t i = z0 + (uint32_t) lane; i < z1; i += 64) acc[i] = 0.0;
                scansi_wave_sync();
                uint32_t bb = g_bbeg[blk], be = g_bbeg[blk + 1];
                if (bb > be || be > p.si_n_terms) {                            // cannot happen
                    if (lane == 0) atomicOr(p.err, 1u);
                    be = bb = 0;
                }
                const bool partial = rlo > lo || rhi < hi;
                for (uint32_t b0 = 0; b0 < n_terms; b0 += 64) {
                    uint64_t o0 = 0, o1 = 0;
                    float bv = 0.0f;
                    if (b0 + (uint32_t) lane < n_terms) {
                        const uint64_t tk = terms[b0 + (uint32_t) lane];
                        const uint32_t idx = (uint32_t) (tk >> 32);
                        bv = __uint_as_float((uint32_t) tk);
                        uint32_t l = bb, h = be;
                        while (l < h) {
                            const uint32_t mid = l + ((h - l) >> 1);
                            if (g_bterm[mid] < idx) l = mid + 1; else h = mid;
                        }
                        if (l < be && g_bterm[l] == idx) {
                            o0 = g_boff[(size_t) l + blk];
                            o1 = g_boff[(size_t) l + blk + 1];
                            if (o0 > o1 || o1 > n_post) {                      // cannot happen
                                atomicOr(p.err, 1u);
                                o1 = o0 = 0;
                            }
                            if (partial) {                                     // the postings of rows [z0, z1) only
                                uint64_t a = o0, b = o1;
                                while (a < b) {
                                    const uint64_t mid = a + ((b - a) >> 1);
                                    if ((uint32_t) g_post[mid] < z0) a = mid + 1; else b = mid;
                                }
                                o0 = a;
                                b = o1;
                                while (a < b) {
                                    const uint64_t mid = a + ((b - a) >> 1);
                                    if ((uint32_t) g_post[mid] < z1) a = mid + 1; else b = mid;
                                }
                                o1 = a;
                            }
                        }
                    }
                    // the terms one after the other, in index order
                    auto add = [&](uint64_t x, float b) {
                        const uint32_t rib = (uint32_t) x;
                        if (rib < SI_RB) acc[rib] += scansi_term<METRIC>(__uint_as_float((uint32_t) (x >> 32)), b);
                        else atomicOr(p.err, 1u);                              // cannot happen
                    };
                    auto fetch = [&](uint64_t lv, uint64_t& s0, uint64_t& s1, float& b, uint64_t& x) {
                        const int j = __ffsll((unsigned long long) lv) - 1;
                        s0 = __shfl(o0, j);
                        s1 = __shfl(o1, j);
                        b = __shfl(bv, j);
                        x = ~0ull;
                        if (s0 + (uint32_t) lane < s1) x = g_post[s0 + (uint32_t) lane];
                    };
                    uint64_t live = __ballot(o1 > o0);
                    uint64_t s0 = 0, s1 = 0, x = 0;
                    float b = 0.0f;
                    if (live) fetch(live, s0, s1, b, x);
                    while (live) {                                             // wave-uniform
                        live &= live - 1ull;
                        uint64_t n0 = 0, n1 = 0, nx = 0;
                        float nb = 0.0f;
                        if (live) fetch(live, n0, n1, nb, nx);                 // in flight under this term
                        if (s0 + (uint32_t) lane < s1) add(x, b);
                        for (uint64_t e = s0 + 64u + (uint32_t) lane; e < s1; e += 64) add(g_post[e], b);
                        scansi_wave_sync();                                    // a row's sum is read by whichever lane meets it next
                        s0 = n0; s1 = n1; b = nb; x = nx;
                    }
                }

                // -- sweep: lane = row --
                for (uint32_t t = ta; t < tb; ++t) {
                    const uint2 tt = tile_at(t);
                    const uint32_t row = tt.x + (uint32_t) lane;
                    uint64_t mask = __ballot((uint32_t) lane < tt.y && row >= rlo && row < rhi);
                    if (mask && g_bitmap) mask &= bitmap_window(g_bitmap, tt.x);
                    if (!mask) continue;                                       // wave-uniform
                    const bool ok = (mask >> lane) & 1ull;
                    float v = 0.0f;
                    if (ok) {
                        const double t_ = acc[row - lo];
                        if constexpr (METRIC == M_L2) {
                            const double d = g_a[row] + qt - 2.0 * t_;
                            v = (float) (d > 0.0 ? d : 0.0);
                        } else if constexpr (METRIC == M_L1) {
                            const double d = g_a[row] + qt - t_;
                            v = (float) (d > 0.0 ? d : 0.0);
                        } else {
                            v = rank_value<METRIC>((float) t_, METRIC == M_COSINE ? g_norm[row] : 0.0f, qn);   // the division: permitted pairs only
                        }
                    }
                    const uint64_t key = make_key(v, row);
                    const uint64_t tau = lds_peek(&ctrl[qi].tau);
                    const bool pass = ok && key < tau;
                    const uint64_t pm = __ballot(pass);
                    if (pm) {
                        const int leader = __ffsll((unsigned long long) pm) - 1;
                        uint32_t base = 0;
                        if (lane == leader) base = atomicAdd(&ctrl[qi].count, (uint32_t) __popcll(pm));
                        base = __shfl(base, leader) + (uint32_t) __popcll(pm & ((1ull << lane) - 1ull));
                        if (pass) {
                            if (base < cap) my_cand[base] = key;
                            else atomicOr(p.err, 2u);                          // cannot happen (append slack protocol)
                        }
                    }
                }
            }

            // -- the next chunk: the last tile again if it reaches into the next block --
            if (tl.y > 0 && tl.x + tl.y > hi) {
                ta = tb - 1;
                row_from = hi;
            } else {
                ta = tb;
                row_from = 0;
            }

            if (++chunk % SI_VOTE_CHUNKS == 0) {                               // workgroup-uniform
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
                        if (n > trigger) {                                     // only the buffers that are filling up
                            uint64_t* cq = cand + (size_t) qs * cand_qstride;
                            for (uint32_t i = tid; i < n; i += SI_THREADS) sortbuf[i] = cq[i];
                            __syncthreads();
                            if (tid == 0) ctrl[qs].count = n;
                            __syncthreads();
                            topk_compact<SI_THREADS>(sortbuf, &ctrl[qs], keep, tid, false);
                            for (uint32_t i = tid; i < keep; i += SI_THREADS) cq[i] = sortbuf[i];
                            __syncthreads();
                        }
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
        for (uint32_t i = tid; i < n; i += SI_THREADS) sortbuf[i] = cq[i];
        __syncthreads();
        if (tid == 0) ctrl[qs].count = n;
        __syncthreads();
        topk_compact<SI_THREADS>(sortbuf, &ctrl[qs], keep, tid, false);
        const uint32_t m = ctrl[qs].count < keep ? ctrl[qs].count : keep;
        uint64_t* dst = p.partial + (size_t) (grp.partial_begin + qs * grp.n_blocks + local_block) * p.kp;
        for (uint32_t i = tid; i < p.kp; i += SI_THREADS) dst[i] = i < m ? sortbuf[i] : KEY_EMPTY;
        __syncthreads();
    }
}

template <int METRIC>
hipError_t launch_scansi_metric(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    if (!p.cand || !p.sp_tab || !p.sp_qtot || !p.q_norm2 || p.rank || (METRIC == M_COSINE && !p.norm2) || !p.si_post || !p.si_bterm ||
        !p.si_boff || !p.si_bbeg || !p.si_a || (p.sp_slots & (p.sp_slots - 1)) != 0 || !scansi_fits(p.sp_slots, p.cap) ||
        p.qmax != (uint32_t) SI_QMAX || p.cap < 2 * K2_SLACK)
        return hipErrorInvalidValue;                                           // (the planner keeps such a call off K1si)
    const size_t lds = scansi_lds_bytes(p.cap);
    auto kern = scansi_kernel<METRIC>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(SI_THREADS), lds, s, p);
    return hipGetLastError();
}

}  // namespace vsr
