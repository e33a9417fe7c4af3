// vsr_mfmahw.h — K2hw: workgroup-shared f16 MFMA passes over a halfvec corpus (opt-in: vsr_set_half_wide).
//
// K2h (vsr_mfmah.h) gives every WAVE its own 64-row tile and 16 (32) queries, so a part seen by 1000 queries is streamed
// ~31 times.  K2hw is K2w's work split (vsr_mfmaw.h) over the resident binary16 rows, which are their own screening plane:
// a 64-row tile is staged ONCE per WORKGROUP into an XOR-swizzled LDS image and multiplied against up to 64 queries,
//
//   >= 3 query groups (16 queries each): wave w owns group w and reads the whole shared tile
//   2 groups: two waves per group, two 16-row sub-tiles each; 1 group: four waves, one sub-tile each (row split).
//
// Arithmetic: v_mfma_f32_16x16x32_f16 with fp32 accumulation and K2h's lane roles -- lane (i = lane & 15, kq = lane >> 4)
// feeds chunk 4t + kq of row i (A, from the image) and chunk 4t + kq of query i's binary16 image (B, StageParams::q_h16) to
// K-step t, the same chunk on both sides, so the sum is over matching k whatever order the hardware walks a fragment in.
// Products of two halves are exact in fp32; the only error is the accumulation (half_err_g).  The keys are K2h's
// (screen_value on the fp32 accumulator with the fp32 |x|^2, |q|^2) and only screen: select_rerank_kernel re-ranks the
// kept 2k exactly on the half rows, a flagged query re-runs on K1h.  No fp16 arithmetic outside the MFMA.
//
// Pipeline: a stage is 16 chunks (128 elements) of all 64 rows, 16 KB; a thread owns 4 chunks of it.  Register staging,
// one stage ahead: as soon as a stage's registers are in LDS the loads of the next stage -- at a tile's last stage, of the
// next TILE's first -- are issued and fly under the MFMAs.  Two stage buffers, one LDS-only barrier per stage.
// B operands: rows of <= 256 elements (NSTR = 1, 2 stages) keep a wave's fragments in registers for the whole pass; longer
// rows (NSTR = 0, up to 16 000 elements) stage the pass's 64 query columns like a second tile, beside the row tile: the
// stage's query chunks are loaded once per workgroup, not once per wave.
// Row mapping, candidates, sample pass: K2w's.  The descriptor of tile it + 3 is fetched, row / permission word / |row|^2
// of tile it + 2 are started and those of tile it + 1 are written to an LDS ring by wave 0 during tile `it`; survivors are
// parked in a wave-private LDS ring and flushed to the queries' global buffers (ScanParams::qcand / qcnt) in two phases
// that ride on the row pipeline; SAMPLE keeps minima only.  A list-ordered view's keys go through p.rank at emit.
// An unfiltered pass over a halfvec corpus has no tile list (grp.tiles == nullptr): tile t is rows [t rw, t rw + rw).
#pragma once
#include "vsr_mfma.h"

namespace vsr {

constexpr int HW_THREADS = 256;
constexpr int HW_WAVES = 4;
constexpr int HW_S = 16;                   // 16-byte chunks per row and stage
constexpr int HW_ROWS = 64;                // rows per workgroup tile
constexpr int HW_NQ = MF_NQ * HW_WAVES;    // query slots of a pass

// workgroup barrier that orders LDS traffic only (K2w's lds_barrier): the prefetched row loads stay in flight across it
__device__ __forceinline__ void hw_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// NSTR > 0: stages per row, B fragments in registers; NSTR == 0: runtime stage count, the queries' chunks through LDS
template <int METRIC, int NSTR, bool SAMPLE>
__global__ __launch_bounds__(HW_THREADS, 2) void mfmahw_scan_kernel(const ScanParams p)
{
    constexpr bool QLDS = NSTR == 0;
    constexpr int NB = QLDS ? 1 : NSTR;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

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
    const auto g_tiles = as_global(grp.tiles);                                 // global_load, not flat (vsr_device.h)
    const auto g_bitmap = as_global(grp.bitmap);
    const auto g_norm2 = as_global(p.norm2);
    const auto g_ones = as_global(p.ones);
    const auto g_rank = as_global(p.rank);

    const uint32_t nchunk = p.stride4 / 2;                                     // 16-byte chunks of 8 halves per row
    const uint32_t nstage = QLDS ? (nchunk + HW_S - 1) / HW_S : (uint32_t) NSTR;
    const uint32_t q_count = grp.q_count;
    const bool sample_fine = SAMPLE && (grp.partial_begin & 1u);               // sample pass: one entry per lane, not per column
    const u32x4* rows16 = reinterpret_cast<const u32x4*>(p.rows);
    const u32x4* q16 = reinterpret_cast<const u32x4*>(p.q_scr);               // [n_slots][nchunk] binary16 query images

    // LDS: [row stage buffers | (QLDS) query stage buffers | row index ring | |row|^2 ring | parked survivors per wave]
    u32x4*    stage = reinterpret_cast<u32x4*>(smem);                           // [2][64 * HW_S]
    u32x4*    qstage = stage + 2 * HW_ROWS * HW_S;                              // [2][64 * HW_S] (QLDS)
    unsigned char* after = smem + (QLDS ? 4 : 2) * HW_ROWS * HW_S * 16;
    int32_t*  rowidx = reinterpret_cast<int32_t*>(after);                       // [HW_RING][64]
    float*    rownorm = reinterpret_cast<float*>(after + HW_RING * 64 * 4);     // [HW_RING][64]
    unsigned char* pend = after + HW_RING * 64 * 8;
    uint32_t* pend_v = reinterpret_cast<uint32_t*>(pend) + (size_t) wave * MW_PEND;                       // key high word
    uint32_t* pend_r = reinterpret_cast<uint32_t*>(pend + 4 * MW_PEND * 4) + (size_t) wave * MW_PEND;     // row
    uint32_t* pend_c = reinterpret_cast<uint32_t*>(pend + 8 * MW_PEND * 4) + (size_t) wave * MW_PEND;     // query column 0..15

    // ---- wave roles ----
    const uint32_t ngt = (q_count + MF_NQ - 1) / MF_NQ;                         // 16-query groups of this pass (1..4)
    const uint32_t rsplit = ngt == 1 ? 4u : ngt == 2 ? 2u : 1u;                 // waves sharing one group's rows
    const uint32_t g0 = (uint32_t) wave / rsplit;                               // this wave's query group
    const uint32_t sub0 = ((uint32_t) wave % rsplit) * (4u / rsplit);           // its first 16-row sub-tile
    const bool gact = g0 < ngt;                                                 // wave-uniform

    // MFMA lane roles (16x16x32): A lane = (row li, k-octet kq); B / result lane = (k-octet kq | row quad kq, query jq)
    const int li = lane & 15;
    const int kq = lane >> 4;
    const int jq = li;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};                                      // eight +0.0 halves
    const uint32_t my_qi = g0 * MF_NQ + (uint32_t) jq < (uint32_t) HW_NQ ? g0 * MF_NQ + (uint32_t) jq : 0u;
    const bool qok = my_qi < q_count;
    const uint32_t my_slot = p.q_slots[grp.q_begin + (qok ? my_qi : 0u)];      // pad columns repeat query 0
    const uint64_t my_tau = p.tau_init ? p.tau_init[my_slot] : KEY_EMPTY;      // this lane's query: threshold (KEY_EMPTY = open)
    const float my_qn = p.q_norm2[my_slot];
    // screening limit: a value passes unless it is greater (NaN values pass; an open threshold admits everything)
    const float tau_lim = my_tau == KEY_EMPTY ? __builtin_inff() : mono_to_float((uint32_t) (my_tau >> 32));
    u32x4 bq[NB][4];                                                           // !QLDS: this lane's B fragments of every stage
    if constexpr (!QLDS) {
        const u32x4* qsrc = q16 + (size_t) my_slot * nchunk;
#pragma unroll
        for (int s = 0; s < NSTR; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t idx = (uint32_t) (s * HW_S + 4 * t + kq);
                bq[s][t] = idx < nchunk ? qsrc[idx] : zero4;                   // chunks past the row end: zeros
            }
    }

    // ---- this workgroup's tiles ----
    const uint32_t rw = p.rw, tps = HW_ROWS / rw;                               // list tiles per 64-row workgroup tile
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t n_super = (t1 - t0 + tps - 1) / tps;
    const uint32_t ss = p.sample_stride;                                        // sample pass: every ss-th tile
    const uint32_t n_it = (n_super + ss - 1) / ss;

    // ---- row mapping pipeline (lane = row slot), branch-free around its loads as in K2w: addresses are clamped and results
    // selected, so that the compiler can count the outstanding loads instead of draining the prefetched rows.  Groups with
    // n_tiles == 0 are never launched.  No tile list: the ones word is loaded in the descriptor's place and ignored.
    const uint32_t tile_last = grp.n_tiles - 1u;
    auto fetch_desc = [&](uint32_t it_) -> uint2 {                 // (start, nrows) of this lane's list tile, or (0, 0)
        const uint32_t t = t0 + it_ * ss * tps + (uint32_t) lane / rw;
        const bool ok = it_ < n_it && t < t1;
        const uint32_t tc = t < tile_last ? t : tile_last;
        const uint2 d = load_tile(g_tiles ? g_tiles : (gptr<uint2>) g_ones, g_tiles ? tc : 0u);
        const uint32_t start = g_tiles ? d.x : tc * rw;
        const uint32_t left = p.n_rows > start ? p.n_rows - start : 0u;
        const uint32_t nrows = g_tiles ? d.y : left < rw ? left : rw;
        return make_uint2(ok ? start : 0u, ok ? nrows : 0u);
    };
    bool bad_row = false;                                          // cannot happen; reported once at the end
    auto start_rows = [&](uint2 d, int32_t& row, uint64_t& bw, float& nrm) {
        const uint32_t r = (uint32_t) lane % rw;
        const uint32_t rr = d.x + r;
        const bool ok = r < d.y && rr < p.n_rows;
        bad_row |= r < d.y && rr >= p.n_rows;
        const uint32_t rc = ok ? rr : 0u;
        row = ok ? (int32_t) rr : -1;
        bw = *(g_bitmap ? g_bitmap + (rc >> 6) : g_ones);          // no bitmap: one all-ones word
        nrm = g_norm2[rc];
    };
    // every wave runs the (identical) mapping loads and wave 0 writes the ring (K2w: no wave-0-only branch around loads)
    auto finish_rows = [&](uint32_t it_, int32_t row, uint64_t bw, float nrm) {
        if (row >= 0 && !((bw >> ((uint32_t) row & 63u)) & 1ull)) row = -1;
        if (wave == 0) {
            rowidx[(it_ % HW_RING) * 64 + lane] = row;
            rownorm[(it_ % HW_RING) * 64 + lane] = nrm;
        }
    };
    int32_t  pend_row;                                             // tile it + 2: row (before the permission bit)
    uint64_t pend_bw;                                              //              its bitmap word (in flight)
    float    pend_nrm;                                             //              its |row|^2 (in flight)
    uint2    dsc_a;                                                // tile it + 3: descriptor (in flight)
    {
        const uint2 d0 = fetch_desc(0), d1 = fetch_desc(1);
        dsc_a = fetch_desc(2);
        int32_t r0;
        uint64_t b0;
        float n0;
        start_rows(d0, r0, b0, n0);
        finish_rows(0, r0, b0, n0);
        start_rows(d1, pend_row, pend_bw, pend_nrm);
    }
    __syncthreads();

    // ---- staging: thread -> (row slot u * 16 + lrow, chunk lchunk) of every stage; QLDS: the same of the query columns ----
    const int lrow = tid >> 4, lchunk = tid & 15;
    const uint32_t last_row = p.n_rows - 1u;
    u32x4 X[4], XQ[4];
    const u32x4* qsrc_u[4];                                        // QLDS: the query whose chunks this thread stages, per u
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t qc = (uint32_t) (u * 16 + lrow);
        qsrc_u[u] = q16 + (size_t) p.q_slots[grp.q_begin + (qc < q_count ? qc : 0u)] * nchunk;
    }
    auto issue = [&](uint32_t it_, uint32_t s_) {                  // loads of (tile it_, stage s_) into X / XQ (no waits)
        // An invalid slot (masked row, ragged tile) loads row 0 and its products are discarded by the epilogue's row test.
        // The padding chunks of a ragged last stage load chunk 0 and meet zero B chunks (finite x 0: the runtime keeps
        // corpora with NaN / Inf elements off the screening kernels); nothing touches the registers while they are in flight.
        const uint32_t chunk = s_ * (uint32_t) HW_S + (uint32_t) lchunk;
        const uint32_t cc = chunk < nchunk ? chunk : 0u;
        const int32_t* ridx = rowidx + (it_ % HW_RING) * 64;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t r = ridx[u * 16 + lrow];
            const uint32_t rc = (uint32_t) (r < 0 ? 0 : r);
            X[u] = rows16[(size_t) (rc < last_row ? rc : last_row) * nchunk + cc];
            if constexpr (QLDS) XQ[u] = qsrc_u[u][cc];
        }
    };
    issue(0, 0);

    // ---- parked survivors -> their queries' buffers: K2w's parking ring and two-phase flush (vsr_mfmaw.h), one query group
    // per wave.  Entries [p_head, p_tail) are parked, each {key high word, row, query column of the wave's group}.
    //   A (right BEFORE a tile's row loads are issued): lane c < 16 reserves room for ALL entries of column c with ONE
    //     returning atomic on its query's counter;
    //   B (after the next tile's rows have been waited for, so the atomics' results are there too): the keys are stored.
    uint32_t p_head = 0, p_tail = 0, f_n = 0;
    constexpr int FL_R = 2;                                        // flush rounds: up to 64 * FL_R entries at a time
    uint32_t f_rank[FL_R];                                         // per lane and round: rank of its entry within the column
    uint32_t f_base = 0;                                           // lanes 0..15: first position of column `lane`
#pragma unroll
    for (int r = 0; r < FL_R; ++r) f_rank[r] = 0;
    auto flush_issue = [&]() __attribute__((always_inline)) {      // phase A
        const uint32_t have = p_tail - p_head;
        f_n = have < 64u * FL_R ? have : 64u * FL_R;
        uint32_t col[FL_R];
#pragma unroll
        for (int r = 0; r < FL_R; ++r) {
            const uint32_t e = (uint32_t) (r * 64 + lane);
            col[r] = e < f_n ? pend_c[(p_head + e) % MW_PEND] : 0xFFu;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int c = 0; c < MF_NQ; ++c) {
            uint32_t before = 0;
#pragma unroll
            for (int r = 0; r < FL_R; ++r) {
                const uint64_t m = __ballot(col[r] == (uint32_t) c);
                if (col[r] == (uint32_t) c)
                    f_rank[r] = before + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
                before += (uint32_t) __popcll(m);
            }
            if (lane == c) mine = before;
        }
        if (lane < MF_NQ && mine) f_base = atomicAdd(p.qcnt + my_slot, mine);  // lane c (kq 0, jq c) owns column c
    };
    auto flush_store = [&]() __attribute__((always_inline)) {      // phase B
#pragma unroll
        for (int r = 0; r < FL_R; ++r) {
            const uint32_t e = (uint32_t) (r * 64 + lane);
            const uint32_t idx = (p_head + e) % MW_PEND;
            const uint32_t c = e < f_n ? pend_c[idx] : 0u;
            const uint32_t base = (uint32_t) __shfl((int) f_base, (int) c);
            const uint32_t slot = (uint32_t) __shfl((int) my_slot, (int) c);
            if (e < f_n) {
                const uint32_t row = pend_r[idx];
                const uint32_t at = base + f_rank[r];
                if (at < p.capq)
                    p.qcand[(size_t) slot * p.capq + at] = ((uint64_t) pend_v[idx] << 32) | (g_rank ? g_rank[row] : row);
            }
        }
        p_head += f_n;
        f_n = 0;
    };
    // one entry per lane with `has` (wave-uniform call): the position is the wave's running count + the lane's rank
    auto park = [&](bool has, uint32_t key_hi, uint32_t row) __attribute__((always_inline)) {
        const uint64_t act = __ballot(has);
        const uint32_t room = MW_PEND - (p_tail - p_head);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) act, 0u));
        if (has) {
            if (rank < room) {
                const uint32_t at = (p_tail + rank) % MW_PEND;
                pend_v[at] = key_hi;
                pend_r[at] = row;
                pend_c[at] = (uint32_t) jq;
            } else {                                               // the ring is full (a burst): reserve directly
                const uint32_t ga = atomicAdd(p.qcnt + my_slot, 1u);
                if (ga < p.capq) p.qcand[(size_t) my_slot * p.capq + ga] = ((uint64_t) key_hi << 32) | (g_rank ? g_rank[row] : row);
            }
        }
        const uint32_t n_act = (uint32_t) __popcll(act);
        p_tail += n_act < room ? n_act : room;
    };

    auto run = [&](auto nsc) {
        constexpr int NS = decltype(nsc)::value;                   // 16-row sub-tiles of this wave (1, 2 or 4)
        int buf = 0;
        for (uint32_t it = 0; it < n_it; ++it) {
            f32x4 acc[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

            for (uint32_t s = 0; s < nstage; ++s) {
                u32x4* img = stage + (size_t) buf * (HW_ROWS * HW_S);
                u32x4* qimg = qstage + (size_t) buf * (HW_ROWS * HW_S);
                const bool in_row = s * (uint32_t) HW_S + (uint32_t) lchunk < nchunk;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int slot = u * 16 + lrow;
                    img[slot * HW_S + (lchunk ^ (slot & 15))] = X[u];          // XOR-swizzled image
                    if constexpr (QLDS) qimg[slot * HW_S + (lchunk ^ (slot & 15))] = in_row ? XQ[u] : zero4;
                }
                if (s == 0) {                                      // row mapping, one step per tile (see above)
                    if (f_n) flush_store();                        // the image write above waited for this tile's rows, which
                                                                   // were issued after the atomics: their results are here
                    finish_rows(it + 1, pend_row, pend_bw, pend_nrm);
                    start_rows(dsc_a, pend_row, pend_bw, pend_nrm);
                    dsc_a = fetch_desc(it + 3);
                }
                hw_lds_barrier();
                if (s == 0 && !f_n && p_tail - p_head >= 64u * FL_R) flush_issue();
                // the next stage -- of the next tile after a tile's last -- in flight under this stage's MFMAs (past the last
                // tile: all slots invalid, row 0 from the cache)
                const bool last = s + 1 == nstage;
                issue(last ? it + 1 : it, last ? 0u : s + 1);
                if (gact) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        u32x4 braw;
                        if constexpr (QLDS) {
                            braw = qimg[((int) g0 * MF_NQ + jq) * HW_S + ((4 * t + kq) ^ jq)];
                        } else {
                            braw = bq[0][t];
#pragma unroll
                            for (int s2 = 1; s2 < NSTR; ++s2)
                                if (s == (uint32_t) s2) braw = bq[s2][t];
                        }
                        const f16x8 b = __builtin_bit_cast(f16x8, braw);
                        f16x8 a[NS];
#pragma unroll
                        for (int i = 0; i < NS; ++i)
                            a[i] = __builtin_bit_cast(f16x8, img[(((int) sub0 + i) * 16 + li) * HW_S + ((4 * t + kq) ^ li)]);
#pragma unroll
                        for (int i = 0; i < NS; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b, acc[i], 0, 0, 0);
                    }
                }
                buf ^= 1;
            }

            // results: acc[i][r] = dot(row slot (sub0 + i) * 16 + kq * 4 + r, query column jq of the wave's group).  Screening
            // test in float: a value is a candidate unless it is greater than the threshold's distance (NaN values and an
            // open / NaN threshold pass): a superset of `key <= tau`.
            if (gact) {
                const int32_t* ridx = rowidx + (it % HW_RING) * 64;
                const float* rnrm = rownorm + (it % HW_RING) * 64;
                uint32_t pmask = 0;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int base = ((int) sub0 + i) * 16 + kq * 4;
                    const int4 ri = *reinterpret_cast<const int4*>(&ridx[base]);
                    const float4 rn = *reinterpret_cast<const float4*>(&rnrm[base]);
                    const int32_t rows4[4] = {ri.x, ri.y, ri.z, ri.w};
                    const float nx4[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = screen_value<METRIC>(acc[i][r], nx4[r], my_qn);
                        const uint32_t ok = (uint32_t) !(v > tau_lim) & (uint32_t) (rows4[r] >= 0) & (uint32_t) qok;   // no branches
                        pmask |= ok << (i * 4 + r);
                    }
                }
                if (__ballot(pmask != 0) != 0) {                   // wave-uniform
                    if constexpr (SAMPLE) {
                        // The seed only needs the SMALLEST sampled values of a query, so a lane contributes the minimum of
                        // its valid pairs (`fine` passes) or the four row-quad lanes of a query column reduce theirs to one.
                        // The m-th smallest of any subset of the sample is >= the m-th smallest of the whole sample: the
                        // threshold only gets looser.
                        uint64_t best = KEY_EMPTY;
#pragma unroll
                        for (int j = 0; j < NS * 4; ++j) {
                            const int slot = ((int) sub0 + (j >> 2)) * 16 + kq * 4 + (j & 3);
                            const float v = screen_value<METRIC>(acc[j >> 2][j & 3], rnrm[slot], my_qn);
                            const uint64_t key = make_key(v, (uint32_t) ridx[slot]);
                            best = ((pmask >> j) & 1u) && key < best ? key : best;
                        }
                        if (!sample_fine) {
                            uint64_t o = __shfl_xor(best, 16);
                            best = o < best ? o : best;
                            o = __shfl_xor(best, 32);
                            best = o < best ? o : best;
                            if (kq != 0) best = KEY_EMPTY;
                        }
                        park(best != KEY_EMPTY, (uint32_t) (best >> 32), (uint32_t) best);
                    } else {
                        // one round per survivor of the busiest lane (1 - 2 at the usual ~1 % admission)
                        while (__ballot(pmask != 0)) {
                            const bool has = pmask != 0;
                            const int j = has ? __builtin_ctz(pmask) : 0;
                            pmask &= pmask - 1u;                   // (0 stays 0)
                            const int slot = ((int) sub0 + (j >> 2)) * 16 + kq * 4 + (j & 3);
                            float a = acc[0][0];                   // acc[j >> 2][j & 3]
#pragma unroll
                            for (int jj = 1; jj < NS * 4; ++jj) a = j == jj ? acc[jj >> 2][jj & 3] : a;
                            const float v = screen_value<METRIC>(a, rnrm[slot], my_qn);
                            park(has, mono_bits(v), (uint32_t) ridx[slot]);
                        }
                    }
                }
            }
        }
    };
    if (rsplit == 4) run(std::integral_constant<int, 1>{});
    else if (rsplit == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 4>{});
    if (f_n) flush_store();                                                    // drain the parking ring
    while (p_tail != p_head) {
        flush_issue();
        flush_store();
    }

    if (bad_row) atomicOr(p.err, 1u);                                          // a tile reached past the corpus: results invalid
}

template <int METRIC>
hipError_t launch_mfmahw_metric(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    // the queries' binary16 image in whole chunks; K2w's candidate buffers; at most one 16-query group per wave
    if (!p.q_scr || p.stride4 == 0 || p.stride4 % 2 != 0 || !p.qcand || !p.qcnt || p.qmax > (uint32_t) HW_NQ || p.n_rows == 0)
        return hipErrorInvalidValue;
    const uint32_t nstage = (p.stride4 / 2 + HW_S - 1) / HW_S;
    const size_t lds = mfmahw_lds_bytes(nstage > 2);
    auto launch = [&](auto kern) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(HW_THREADS), lds, s, p);
        return hipGetLastError();
    };
    const bool sample = p.sample_stride > 1;
    if (nstage == 1) return sample ? launch(mfmahw_scan_kernel<METRIC, 1, true>) : launch(mfmahw_scan_kernel<METRIC, 1, false>);
    if (nstage == 2) return sample ? launch(mfmahw_scan_kernel<METRIC, 2, true>) : launch(mfmahw_scan_kernel<METRIC, 2, false>);
    return sample ? launch(mfmahw_scan_kernel<METRIC, 0, true>) : launch(mfmahw_scan_kernel<METRIC, 0, false>);
}

}  // namespace vsr
