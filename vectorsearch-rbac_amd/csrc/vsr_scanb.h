// vsr_scanb.h — K1b: K1 (vsr_scan.h) over a bit corpus: Hamming / Jaccard distance + RBAC permission test + running top-k.
//
// Replaces, for a whole ORDER BY col <~> $1 / col <%> $1 LIMIT k scan, the per-row calls of
//   pgvector/src/bitvec.c:46-77 hamming_distance / jaccard_distance over
//   pgvector/src/bitutils.c:34-61 BitHammingDistanceDefault, :96-129 BitJaccardDistanceDefault.
//
// K1's skeleton, restated: ScanParams / ScanGroup passes, the bitmap window per tile, LPR lanes sharing a row (ScanShape),
// up to qmax queries of a pass in LDS applied in sub-batches of QI to the register-resident tile, the LDS candidate list with a
// running threshold (vsr_topk.h) and partial lists of kp keys for K5.  A row is ceil(dim / 128) 16-byte chunks of packed
// bits, zero padded (bits past dim are cleared at load and at query staging), so the shape classes count those chunks
// (scan_shape, BIT): at dim <= 128 LPR = 1 and one load instruction reads 64 rows as 1 KiB.  p.stride4 is the chunks
// per row AND per query slot.
// The arithmetic is integer: per (row chunk, query) four xor (Hamming) or and (Jaccard) and four popcount-accumulates into a
// uint32 partial; the butterfly over the LPR lanes is reduce_slots in uint32.  Jaccard takes |row| from p.norm2 (the popcounts
// written at load, exact in fp32) and |query| from p.q_norm2 (staging), and evaluates bitutils.c:125-128 in double for the
// lane that owns the finished row.  The ranking value is (float) of the operator's float8: a Hamming count <= 64000 is exact
// in fp32, rounding a Jaccard value is monotone.  Nothing is screened: every result is exact by construction.
// No matrix cores: CDNA4 has no 1-bit MFMA.
// Not carried over from scan_kernel (this is a second kernel body: a fix to K1's top-k or overflow protocol belongs in both):
// p.tau_init (no seeded thresholds), p.sample_stride (no sample pass) and p.fused (the one-query in-kernel merge, FusedTail, is
// not instantiated here).  p.rank IS carried, by the VIEW instantiations (K3b, the list-ordered view of an IVFFlat index over a bit
// corpus): a finished row's key holds p.rank[view row], the base row, on both the compile-time-chunk and the runtime-chunk path --
// read for permitted rows only, so never past the view -- and the view's p.norm2 holds the popcounts gathered with the rows.
// VIEW is a template argument, not a test of p.rank in the kernel: the runtime test cost the 1000-query RBAC leg of
// tools/bit_probe.py 3.5 - 4 % (profiles/ivf_bit.json), outside the parent kernel's own spread, so a corpus scanned directly
// (p.rank == nullptr) runs the kernel it ran before.  Only Hamming has VIEW instantiations: ivfflat has no Jaccard opclass.
#pragma once
#include "vsr_scan.h"
#include "vsr_bitops.h"

namespace vsr {

// MetricBit, accum_bits and rank_value_bits: vsr_bitops.h (shared with the graph kernels)

// reduce_slots (vsr_scan.h) over uint32 partials: N live registers over lanes differing in bit M (and below)
template <int M, int N>
__device__ __forceinline__ void reduce_slots_u32(uint32_t* p, int lane)
{
    if constexpr (M >= 1) {
        if constexpr (N > 1) {
            const bool hi = (lane & M) != 0;
#pragma unroll
            for (int i = 0; i < N / 2; ++i) {
                const uint32_t keep = hi ? p[i + N / 2] : p[i];
                const uint32_t send = hi ? p[i] : p[i + N / 2];
                p[i] = keep + (uint32_t) __shfl_xor((int) send, M);
            }
            reduce_slots_u32<M / 2, N / 2>(p, lane);
        } else {
            p[0] += (uint32_t) __shfl_xor((int) p[0], M);
            reduce_slots_u32<M / 2, 1>(p, lane);
        }
    }
}

// C > 0: compile-time chunk count.  C == 0: runtime chunk loop (rows of more than 128 chunks; LPR = 64, qmax <= QI).
template <bool JACCARD, int LPR, int C, int R, int QI, bool VIEW = false>
__global__ __launch_bounds__(SCAN_THREADS, VSR_MINWAVES) void scanb_kernel(const ScanParams p)
{
    using S = ScanShape<LPR, R>;
    constexpr int G = S::G, RW = S::RW, D = S::D, XCHK = S::XCHK;
    constexpr int CC = C > 0 ? C : 1;

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
    const auto g_rank = as_global(p.rank);                                     // VIEW: keys carry the base row
    const uint32_t local_block = blockIdx.x - grp.block_begin;
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);

    const uint32_t cap = p.cap, k = p.k, qmax = p.qmax, rstride = p.stride4;   // 16-byte chunks per row and per query slot
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                       // [qmax][cap]
    TopKCtrl* ctrl = reinterpret_cast<TopKCtrl*>(keys + (size_t) qmax * cap); // [qmax]
    uint4*    qlds = reinterpret_cast<uint4*>(ctrl + qmax);                   // [qmax][rstride]
    float*    qnl = reinterpret_cast<float*>(qlds + (size_t) qmax * rstride); // [qmax] |q|
    uint32_t* flags = reinterpret_cast<uint32_t*>(qnl + qmax);                // [4] overflow votes

    const uint32_t q_count = grp.q_count;
    const uint32_t n_sub = (q_count + QI - 1) / QI;                           // wave-uniform; n_sub * QI <= qmax (planner)
    for (uint32_t qi = tid; qi < qmax; qi += SCAN_THREADS) {
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
        ctrl[qi].tau = KEY_EMPTY;
        ctrl[qi].count = 0;
        qnl[qi] = JACCARD ? p.q_norm2[slot] : 0.0f;
    }
    if (tid < 4) flags[tid] = 0;
    for (uint32_t qi = 0; qi < n_sub * QI; ++qi) {                            // pad slots repeat query 0
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
        const uint4* qsrc = reinterpret_cast<const uint4*>(p.queries) + (size_t) slot * rstride;
        for (uint32_t i = tid; i < rstride; i += SCAN_THREADS) qlds[(size_t) qi * rstride + i] = qsrc[i];
    }
    __syncthreads();

    // the row this lane finishes after the butterfly
    const bool own = (l % D) == 0;
    const int row_own = (l / D) * G + g;
    const uint32_t trigger = cap - S::SLACK;
    const uint32_t iters = ((t1 - t0) + SCAN_WAVES - 1) / SCAN_WAVES;
    const uint4* rows = reinterpret_cast<const uint4*>(p.rows);

    // issue the loads of tile t (no waits): descriptor, permission bits, row chunks
    auto fetch = [&](uint32_t t, TileRegs<R, CC, uint4>& tr) {
        tr.mask = 0;
        tr.start = 0;
        tr.rn = 0.0f;
        if (t >= t1) return;
        uint32_t start, nrows;
        if (g_tiles) {
            const uint2 tl = load_tile(g_tiles, t);
            start = tl.x;
            nrows = tl.y;
        } else {
            start = t * RW;
            nrows = p.n_rows - start < (uint32_t) RW ? p.n_rows - start : (uint32_t) RW;
        }
        uint64_t mask = nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
        if (g_bitmap) mask &= bitmap_window(g_bitmap, start);
        tr.start = start;
        tr.mask = mask;
        if (!mask) return;
        if constexpr (JACCARD) {
            if (own && ((mask >> row_own) & 1ull)) tr.rn = p.norm2[start + row_own];
        }
        if constexpr (C > 0) {
            const uint4* base = rows + (size_t) start * rstride;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = r * G + g;
                const bool ok = (mask >> row) & 1ull;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t chunk = c * LPR + l;
                    tr.x[r][c] = (ok && chunk < rstride) ? base[(size_t) row * rstride + chunk] : make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
    };

    TileRegs<R, CC, uint4> cur;
    uint32_t round = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        fetch(t0 + it * SCAN_WAVES + wave, cur);

        if (cur.mask) {                                                        // wave-uniform
            const uint32_t start = cur.start;
            const bool ok_own = (cur.mask >> row_own) & 1ull;
            if constexpr (C > 0) {
                for (uint32_t sb = 0; sb < n_sub; ++sb) {
                    uint32_t acc[QI][R];
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
                        for (int r = 0; r < R; ++r) acc[qi][r] = 0u;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const uint32_t chunk = c * LPR + l;
#pragma unroll
                        for (int qi = 0; qi < QI; ++qi) {
                            // (every lane of a row group reads the same address per l: an LDS broadcast at LPR = 1)
                            const uint4 qv = chunk < rstride ? qlds[(size_t) (sb * QI + qi) * rstride + chunk] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                            for (int r = 0; r < R; ++r) accum_bits<JACCARD>(acc[qi][r], cur.x[r][c], qv);
                        }
                    }
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi) {
                        const uint32_t qs = sb * QI + qi;
                        reduce_slots_u32<LPR / 2, R>(acc[qi], lane);
                        const bool live = own && ok_own && qs < q_count;
                        const float v = live ? rank_value_bits<JACCARD>(acc[qi][0], cur.rn, qnl[qs]) : 0.0f;   // the division: permitted pairs only
                        uint32_t key_row = start + row_own;
                        if constexpr (VIEW) key_row = live ? g_rank[key_row] : key_row;
                        const uint64_t key = make_key(v, key_row);
                        const uint64_t tau = lds_peek(&ctrl[qs].tau);
                        topk_append(keys + (size_t) qs * cap, &ctrl[qs], live && key < tau, key);
                    }
                }
            } else {
                // long rows: stream the rows chunk by chunk, all (<= QI) queries at once
                const uint4* base = rows + (size_t) start * rstride;
                uint32_t acc[QI][R];
#pragma unroll
                for (int qi = 0; qi < QI; ++qi)
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[qi][r] = 0u;
#pragma unroll 4
                for (uint32_t chunk = l; chunk < rstride; chunk += 64) {
                    uint4 x[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const bool ok = (cur.mask >> r) & 1ull;
                        x[r] = ok ? base[(size_t) r * rstride + chunk] : make_uint4(0u, 0u, 0u, 0u);
                    }
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi) {
                        const uint4 qv = qlds[(size_t) qi * rstride + chunk];
#pragma unroll
                        for (int r = 0; r < R; ++r) accum_bits<JACCARD>(acc[qi][r], x[r], qv);
                    }
                }
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) {
                    reduce_slots_u32<LPR / 2, R>(acc[qi], lane);
                    const bool live = own && ok_own && (uint32_t) qi < q_count;
                    const float v = live ? rank_value_bits<JACCARD>(acc[qi][0], cur.rn, qnl[qi]) : 0.0f;
                    uint32_t key_row = start + row_own;
                    if constexpr (VIEW) key_row = live ? g_rank[key_row] : key_row;
                    const uint64_t key = make_key(v, key_row);
                    const uint64_t tau = lds_peek(&ctrl[qi].tau);
                    topk_append(keys + (size_t) qi * cap, &ctrl[qi], live && key < tau, key);
                }
            }
        }

        if ((it % XCHK) == XCHK - 1 && it + 1 < iters) {                       // workgroup-uniform
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

template <bool JACCARD, int LPR, int C, int R, int QI, bool VIEW = false>
hipError_t launch_scanb_inst(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    const size_t lds = scan_lds_bytes(p.qmax, p.cap, p.stride4);
    auto kern = scanb_kernel<JACCARD, LPR, C, R, QI, VIEW>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(SCAN_THREADS), lds, s, p);
    return hipGetLastError();
}

// shape dispatch for one metric; instantiated once per metric in its own translation unit
template <bool JACCARD>
hipError_t launch_scanb_metric(const ScanParams& p, int dim, int qi, uint32_t n_blocks, hipStream_t s)
{
    const KernelShape sh = scan_shape(RowFormat::BIT, dim);
    const bool view = p.rank != nullptr;                   // a list-ordered view (K3b): the VIEW instantiations, Hamming only
    if (view && JACCARD) return hipErrorInvalidValue;
#define VSR_CASE(LPR_, C_, R_)                                                             \
    if (sh.lpr == LPR_ && sh.c == C_) {                                                    \
        if constexpr (!JACCARD) {                                                          \
            if (view && qi == 1) return launch_scanb_inst<false, LPR_, C_, R_, 1, true>(p, n_blocks, s);   \
            if (view && qi == 4) return launch_scanb_inst<false, LPR_, C_, R_, 4, true>(p, n_blocks, s);   \
        }                                                                                  \
        if (qi == 1) return launch_scanb_inst<JACCARD, LPR_, C_, R_, 1>(p, n_blocks, s);   \
        if (qi == 4) return launch_scanb_inst<JACCARD, LPR_, C_, R_, 4>(p, n_blocks, s);   \
        return hipErrorInvalidValue;                                                       \
    }
    VSR_CASE(1, 1, 1)
    VSR_CASE(4, 1, 4)
    VSR_CASE(16, 1, 8)
    VSR_CASE(32, 1, 8)
    VSR_CASE(64, 1, 8)
    VSR_CASE(64, 2, 4)
    VSR_CASE(64, 0, 2)
#undef VSR_CASE
    return hipErrorInvalidValue;
}

}  // namespace vsr
