// vsr_gemmh.h — K2gh: 256-query f16 GEMM passes over the LONG rows of a halfvec corpus (opt-in: vsr_set_half_gemm).
//
// K2hw (vsr_mfmahw.h) stages a 64-row tile per workgroup for 64 queries: a part seen by 1000 queries is walked 16 times and,
// for rows of more than 256 elements, every tile re-stages its 64 query columns.  K2gh is K2g's shape (vsr_gemm.h) over the
// resident binary16 rows, which are their own operand -- no planes, no second image of the corpus in any layout:
//
//   * tile = 256 rows x 256 queries per workgroup of 8 waves (2 x 4; a wave owns 128 rows x 64 query columns = 8 x 4 blocks
//     of v_mfma_f32_16x16x32_f16, 128 fp32 accumulator registers per lane).  A product of two halves is exact in fp32, so
//     the only error is the accumulation (half_err_g); no fp16 arithmetic outside the MFMA;
//   * A operand: the row-major rows themselves (p.rows, nchunk = format_row_chunks 16-byte chunks per row), gathered per row
//     slot by LDS-DMA (global_load_lds, 16 bytes per lane); B operand: the queries' binary16 image that staging writes
//     (StageParams::q_h16), here with rows of gemmh_q_chunks(nchunk) chunks, zero-padded to whole K-steps, loaded the same
//     way into the same stage slot.  The XOR swizzle of the 64-byte LDS rows is applied on the SOURCE chunk index;
//   * K-step = 32 elements = 4 chunks = HALF a 128-byte line of a row; ring of 4 stage slots of 32 KB, three K-steps in
//     flight under the MFMAs of one, counted s_waitcnt vmcnt(8) + a bare s_barrier per K-step.  Consecutive K-steps take the
//     two halves of a line: the four lanes of a row slot fetch chunks 4 ks .. 4 ks + 3, and the same lanes fetch the line's
//     other half one stage (~1/3 of the in-flight window) later, when the line is still in L2.  A whole-line K-step
//     (64 elements) would need 64 KB per slot: two slots, nothing in flight across a barrier;
//   * ROW TAIL: rows are not padded to a K-step.  A source chunk index past the row's last chunk is CLAMPED to the row's
//     last chunk (min(4 ks + c, nchunk - 1)): the load never leaves the row, so never the allocation either, and the
//     repeated chunk meets the zero pad of the query image -- rows are finite under k2_safe, so x * 0 = 0 exactly;
//   * row mapping as in K2g: resolved by threads 0..255 one tile ahead in three steps over K-steps 0 / 2 / 4, riding the
//     same vector-memory queue as 4-byte LDS-DMA loads; masked or absent slots load row 0 and carry a NaN threshold.  An
//     unfiltered pass over a halfvec corpus has no tile list (grp.tiles == nullptr): tile t = rows [t rw, t rw + rw) by
//     arithmetic, permission word = the context's ones word.  So rows need nks = ceil(nchunk / 4) >= 8 K-steps: nchunk >= 29,
//     d >= 225 (gemmh_supported).  Views (p.rank) are not served;
//   * epilogue as in K2g: thresholds folded into the accumulators' start values, one compare per pair, candidates parked
//     per wave, one aggregated reservation per tile consumed a tile later; the generic epilogue (SAMPLE, open thresholds)
//     keeps one minimum per column and 128-row wave-tile, or per lane (`fine`).  Keys are K2hw's: screen_value<METRIC> on
//     the fp32 dot product with the fp32 |x|^2 and |q|^2; they only screen -- select_rerank_kernel<HALF> re-ranks the kept
//     2k exactly on the half rows, a flagged query re-runs on K1h.
#pragma once
#include "vsr_device.h"
#include "vsr_topk.h"
#include "vsr_mfma.h"

namespace vsr {

constexpr int GH_THREADS = 512;
constexpr int GH_BM = 256;                 // rows per workgroup tile
constexpr int GH_BN = 256;                 // query slots per pass
constexpr int GH_KC = 4;                   // 16-byte chunks (8 halves) per row and K-step: 32 elements, half a 128-byte line
constexpr int GH_SLOTS = 4;                // stage ring: one slot being multiplied, three in flight
constexpr size_t GH_STAGE_U4 = (size_t) (GH_BM + GH_BN) * GH_KC;                  // uint4 per stage slot (32 KB)
constexpr int GH_PARK = 64;                // candidates a wave parks per tile before they go to their queries' buffers
// [stage ring | row ring: index, compare value, |row|^2 | column constants, thresholds | mapping scratch: descriptor,
//  permission word, norm | flag | per wave: parked candidates, column counts]
inline size_t gemmh_lds_bytes() { return GH_SLOTS * GH_STAGE_U4 * 16 + 2 * GH_BM * 12 + GH_BN * 20 + GH_BM * 20 + 16 + 8 * (GH_PARK * 16 + 64 * 4); }
static_assert(GH_SLOTS * GH_STAGE_U4 * 16 + 2 * GH_BM * 12 + GH_BN * 20 + GH_BM * 20 + 16 + 8 * (GH_PARK * 16 + 64 * 4) <= 159744,
              "K2gh: everything lives in the one dynamic LDS array");

using gh_lds_u4 = __attribute__((address_space(3))) uint4;
using gh_lds_u32 = __attribute__((address_space(3))) uint32_t;

__device__ __forceinline__ void gh_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Every vector-memory operation of the tile loop is an LDS-DMA load; a wave issues four operand pieces per K-step (after at
// most three mapping loads), so "at most 8 outstanding" means that stage g -- and any mapping load issued before stage
// g + 1 -- has landed.  The barrier then makes that true of every wave's share.
__device__ __forceinline__ void gh_wait_barrier()
{
    asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int METRIC, bool SAMPLE>
__global__ __launch_bounds__(GH_THREADS, 2) void gemmh_screen_kernel(const ScanParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2;                                                  // 128-row half of the tile
    const int wn = wave & 3;                                                   // 64-query quarter of the pass

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
    const bool has_tiles = grp.tiles != nullptr;                               // (no list: an unfiltered pass, tiles by arithmetic)
    const auto g_bitmap = as_global(grp.bitmap ? grp.bitmap : p.ones);          // no bitmap: one all-ones word
    const bool has_bitmap = grp.bitmap != nullptr;
    const auto g_norm2 = as_global(p.norm2);

    uint4*   stage = reinterpret_cast<uint4*>(smem);
    int32_t* rowidx = reinterpret_cast<int32_t*>(smem + GH_SLOTS * GH_STAGE_U4 * 16);  // [2][256]
    float*   rowval = reinterpret_cast<float*>(rowidx + 2 * GH_BM);            // [2][256] what a candidate's acc must reach (NaN: no row)
    float*   rownrm = rowval + 2 * GH_BM;                                       // [2][256] |row|^2
    float4*  colc = reinterpret_cast<float4*>(rownrm + 2 * GH_BM);             // [256] {acc start, compare scale, |q|^2, slot bits}
    float*   collim = reinterpret_cast<float*>(colc + GH_BN);                   // [256] the threshold itself (generic epilogue)
    uint32_t* mapd = reinterpret_cast<uint32_t*>(collim + GH_BN);               // [2][256] tile descriptor words (x | y) of every row slot
    uint32_t* mapb = mapd + 2 * GH_BM;                                          // [2][256] permission word (lo | hi)
    float*    mapn = reinterpret_cast<float*>(mapb + 2 * GH_BM);                // [256] |row|^2
    uint32_t* s_open = reinterpret_cast<uint32_t*>(mapn + GH_BM);               // any query column without a threshold
    // per wave: parked candidates {value bits, row, wave-local column, rank within the column} and the columns' counts
    uint32_t* pk_v = s_open + 4 + (size_t) wave * (GH_PARK * 4 + 64);
    uint32_t* pk_r = pk_v + GH_PARK;
    uint32_t* pk_c = pk_r + GH_PARK;
    uint32_t* pk_k = pk_c + GH_PARK;
    uint32_t* pk_n = pk_k + GH_PARK;                                            // [64] candidates per column of this wave

    const bool sample_fine = SAMPLE && (grp.partial_begin & 1u);               // sample pass: one entry per lane, not per column
    const uint32_t nchunk = p.stride4 / 2;                                     // 16-byte chunks of 8 halves per row
    const uint32_t chunk_last = nchunk - 1u;
    const uint32_t nks = (nchunk + GH_KC - 1) / GH_KC;                         // K-steps per tile (>= 8)
    const uint32_t qchunk = nks * GH_KC;                                       // chunks per query image row (gemmh_q_chunks)
    const uint32_t q_count = grp.q_count;
    const uint4* rows16 = reinterpret_cast<const uint4*>(p.rows);

    // ---- query columns: thresholds folded into what the accumulators start from ----
    if (tid == 0) *s_open = 0u;
    __syncthreads();
    if (tid < GH_BN) {
        const bool qok = (uint32_t) tid < q_count;
        const uint32_t slot = p.q_slots[grp.q_begin + (qok ? (uint32_t) tid : 0u)];
        const uint64_t tau = (!SAMPLE && p.tau_init) ? p.tau_init[slot] : KEY_EMPTY;
        const bool open = tau == KEY_EMPTY;
        const float lim = mono_to_float((uint32_t) (tau >> 32));
        const float qn = p.q_norm2[slot];
        float start = 0.0f, scale = 0.0f;
        if (!SAMPLE && !open) {
            if constexpr (METRIC == M_L2) start = 0.5f * (lim - qn);
            else if constexpr (METRIC == M_IP) start = lim;
            else scale = (1.0f - lim) * sqrtf(qn);
        }
        if (!qok) {                                                            // pad column: nothing is ever a candidate
            if constexpr (METRIC == M_COSINE) scale = __builtin_inff();
            else start = -__builtin_inff();
        }
        if (qok && open) *s_open = 1u;
        colc[tid] = make_float4(start, scale, qn, __uint_as_float(qok ? slot : 0xFFFFFFFFu));
        collim[tid] = !qok ? -__builtin_inff() : open ? __builtin_inff() : lim;
    }
    // open thresholds (a query whose sample was too thin; the sample pass itself): the generic epilogue
    __syncthreads();
    const bool generic = SAMPLE || lds_peek(s_open) != 0u;

    // ---- this workgroup's tiles ----
    const uint32_t rw = p.rw, tps = GH_BM / rw;                                // list tiles per 256-row tile
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t n_super = (t1 - t0 + tps - 1) / tps;
    const uint32_t ss = p.sample_stride;
    const uint32_t n_it = (n_super + ss - 1) / ss;
    if (n_it == 0) return;
    const uint32_t tile_last = grp.n_tiles - 1u;
    const uint32_t last_row = p.n_rows - 1u;
    const uint32_t mslot = (uint32_t) tid & (GH_BM - 1);                        // row slot this thread maps (threads 0..255)

    // what row slot `mslot` of tile it_ is, from its list-tile descriptor d: (row or -1, clamped row)
    auto list_tile_of = [&](uint32_t it_) -> uint32_t { return t0 + it_ * ss * tps + mslot / rw; };
    auto arith_tile = [&](uint32_t it_) -> uint2 {                              // no tile list: (start, rows) of the clamped tile
        const uint32_t t = list_tile_of(it_);
        const uint32_t start = (t < tile_last ? t : tile_last) * rw;            // (< n_rows: n_tiles = ceil(n_rows / rw))
        const uint32_t left = p.n_rows - start;
        return make_uint2(start, left < rw ? left : rw);
    };
    auto slot_row = [&](uint32_t it_, uint2 d, uint32_t& rc) -> int32_t {
        const uint32_t t = list_tile_of(it_);
        const bool tile_ok = it_ < n_it && t < t1;
        const uint32_t r = mslot % rw;
        const uint32_t rr = d.x + r;
        const bool ok = tile_ok && r < d.y && rr <= last_row;
        rc = ok ? rr : 0u;
        return ok ? (int32_t) rr : -1;
    };
    auto commit = [&](uint32_t it_, int32_t row, uint64_t bw, float nrm) {
        if (row >= 0 && !((bw >> ((uint32_t) row & 63u)) & 1ull)) row = -1;
        float v;
        if constexpr (METRIC == M_L2) v = 0.5f * nrm;
        else if constexpr (METRIC == M_IP) v = 0.0f;
        else v = sqrtf(nrm);
        rowidx[(it_ & 1u) * GH_BM + mslot] = row;
        rowval[(it_ & 1u) * GH_BM + mslot] = row >= 0 ? v : __builtin_nanf("");
        rownrm[(it_ & 1u) * GH_BM + mslot] = nrm;
    };
    // tile 0 is mapped with plain loads (nothing is in flight yet); later tiles through the LDS-DMA chain in the loop
    if (tid < GH_BM) {
        const uint32_t t = list_tile_of(0);
        const uint2 d = has_tiles ? load_tile(g_tiles, t < tile_last ? t : tile_last) : arith_tile(0);
        uint32_t rc;
        const int32_t row = slot_row(0, d, rc);
        const uint64_t bw = g_bitmap[has_bitmap ? rc >> 6 : 0u];
        commit(0, row, bw, g_norm2[rc]);
    }
    __syncthreads();

    // ---- operand staging: wave w issues the 1-KB pieces 2w, 2w+1 of the row half and of the query half of a stage ----
    // piece = 16 slots x 64 bytes; lane -> (slot = 16 piece + (lane >> 2), LDS chunk = lane & 3) fetches chunk
    // (lane & 3) ^ sw(slot) of the K-step, sw(slot) = (-(slot >> 2)) & 3: with it the 16-byte fragment reads of a 16-lane group
    // (4 banks each) cover all 64 banks exactly once.  The four lanes of a slot read one contiguous 64-byte half line.
    const uint32_t l_slot = (uint32_t) lane >> 2;
    const uint32_t l_src = ((uint32_t) lane & 3u) ^ ((0u - (l_slot >> 2)) & 3u);   // (slot >> 2) & 3 == (l_slot >> 2) & 3: pieces start at multiples of 16
    const uint4* a_cur[2];
    const uint4* a_nxt[2];
    const uint4* b_src[2];
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
        const uint32_t qs = (uint32_t) (wave * 2 + pc) * 16u + l_slot;
        const uint32_t slot = p.q_slots[grp.q_begin + (qs < q_count ? qs : 0u)];   // pad columns repeat the pass's first query
        b_src[pc] = reinterpret_cast<const uint4*>(p.q_scr) + (size_t) slot * qchunk + l_src;
    }
    auto rows_of = [&](uint32_t it_, const uint4* (&dst)[2]) {
        const int32_t* ridx = rowidx + (it_ & 1u) * GH_BM;
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
            const int32_t r = ridx[(wave * 2 + pc) * 16 + (int) l_slot];
            dst[pc] = rows16 + (size_t) (uint32_t) (r < 0 ? 0 : r) * nchunk;    // (r <= last_row: slot_row)
        }
    };
    // this lane's source chunk of K-step ks in its row: the tail rule (header) -- never past the row's last chunk
    auto a_chunk = [&](uint32_t ks) -> uint32_t {
        const uint32_t c = ks * GH_KC + l_src;
        return c < chunk_last ? c : chunk_last;
    };
    auto issue = [&](const uint4* (&a)[2], uint32_t ks, uint32_t slot_) {
        gh_lds_u4* dst = (gh_lds_u4*) (stage + (size_t) slot_ * GH_STAGE_U4);
        const uint32_t ac = a_chunk(ks);
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
            __builtin_amdgcn_global_load_lds(as_global(a[pc] + ac), dst + (wave * 2 + pc) * 64, 16, 0, 0);
            __builtin_amdgcn_global_load_lds(as_global(b_src[pc] + (size_t) ks * GH_KC), dst + GH_BM * GH_KC + (wave * 2 + pc) * 64, 16, 0, 0);
        }
    };

    // MFMA lane roles (16x16x32): A lane = (row li, k-octet kq); B / result lane = (k-octet kq | row quad kq, query li)
    const int li = lane & 15;
    const int kq = lane >> 4;
    const uint32_t frag_off = (uint32_t) li * GH_KC + ((uint32_t) kq ^ ((0u - ((uint32_t) li >> 2)) & 3u));   // + 64 per 16-slot block
    f32x4 acc[8][4];

    // parked candidates of the previous tile -> their queries' buffers (see the epilogue)
    uint32_t n_park = 0, n_flush = 0;                                           // wave-uniform
    uint32_t fl_base = 0;                                                       // lane c: first position of column c's candidates
    const uint32_t my_col_slot = __float_as_uint(colc[wn * 64 + lane].w);      // lane c: query slot of the wave's column c
    auto flush_reserve = [&]() {
        n_flush = n_park;
        if (n_flush == 0) return;
        pk_n[lane] = 0u;
        gh_wave_fence();
        if ((uint32_t) lane < n_flush) pk_k[lane] = atomicAdd(&pk_n[pk_c[lane]], 1u);      // LDS: rank within its column
        gh_wave_fence();
        const uint32_t mine = pk_n[lane];
        if (mine) fl_base = atomicAdd(p.qcnt + my_col_slot, mine);             // one wave instruction; consumed a tile later
    };
    auto flush_store = [&]() {
        if (n_flush == 0) return;
        const uint32_t c = (uint32_t) lane < n_flush ? pk_c[lane] : 0u;
        const uint32_t base = (uint32_t) __shfl((int) fl_base, (int) c);
        const uint32_t slot = (uint32_t) __shfl((int) my_col_slot, (int) c);
        if ((uint32_t) lane < n_flush) {
            const uint32_t at = base + pk_k[lane];
            if (at < p.capq) p.qcand[(size_t) slot * p.capq + at] = ((uint64_t) pk_v[lane] << 32) | pk_r[lane];
        }
        n_flush = 0;
        gh_wave_fence();
    };

    rows_of(0, a_cur);
    a_nxt[0] = a_cur[0];
    a_nxt[1] = a_cur[1];
    // stages are numbered through all tiles: g = it * nks + ks lives in ring slot g & 3; three are in flight
    issue(a_cur, 0, 0);
    issue(a_cur, 1, 1);
    issue(a_cur, 2, 2);
    uint32_t g = 0;
    for (uint32_t it = 0; it < n_it; ++it) {
        // accumulators start from the folded thresholds of their query columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = generic ? 0.0f : colc[wn * 64 + j * 16 + li].x;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i][j] = f32x4{s, s, s, s};
        }
        for (uint32_t ks = 0; ks < nks; ++ks, ++g) {
            gh_wait_barrier();                               // stage g has landed in every wave's share; slot (g + 3) & 3 is free
            // ---- row mapping of tile it + 1 (threads 0..255), spread over K-steps 0 / 2 / 4 ----
            if (tid < GH_BM) {
                if (ks == 0) {
                    if (has_tiles) {
                        const uint32_t t = list_tile_of(it + 1);
                        const gptr<uint32_t> src = (gptr<uint32_t>) (g_tiles + (t < tile_last ? t : tile_last));
                        __builtin_amdgcn_global_load_lds(src, (gh_lds_u32*) mapd + wave * 64, 4, 0, 0);
                        __builtin_amdgcn_global_load_lds(src + 1, (gh_lds_u32*) mapd + GH_BM + wave * 64, 4, 0, 0);
                    }
                } else if (ks == 2) {
                    uint32_t rc;
                    (void) slot_row(it + 1, has_tiles ? make_uint2(mapd[mslot], mapd[GH_BM + mslot]) : arith_tile(it + 1), rc);
                    const gptr<uint32_t> bsrc = (gptr<uint32_t>) (g_bitmap + (has_bitmap ? rc >> 6 : 0u));
                    __builtin_amdgcn_global_load_lds(bsrc, (gh_lds_u32*) mapb + wave * 64, 4, 0, 0);
                    __builtin_amdgcn_global_load_lds(bsrc + 1, (gh_lds_u32*) mapb + GH_BM + wave * 64, 4, 0, 0);
                    __builtin_amdgcn_global_load_lds((gptr<uint32_t>) (g_norm2 + rc), (gh_lds_u32*) mapn + wave * 64, 4, 0, 0);
                } else if (ks == 4) {
                    uint32_t rc;
                    const int32_t row = slot_row(it + 1, has_tiles ? make_uint2(mapd[mslot], mapd[GH_BM + mslot]) : arith_tile(it + 1), rc);
                    commit(it + 1, row, ((uint64_t) mapb[GH_BM + mslot] << 32) | mapb[mslot], mapn[mslot]);
                }
            }
            // ---- three stages ahead: stage g + 3 (of the next tile from K-step nks - 3 on) ----
            const uint32_t ks3 = ks + 3 < nks ? ks + 3 : ks + 3 - nks;
            if (ks + 3 == nks) rows_of(it + 1, a_nxt);       // (committed at K-step 4 <= nks - 4, a barrier ago at least)
            const bool nxt = ks + 3 >= nks;                   // past the last tile: row 0, never used
            const uint32_t ac3 = a_chunk(ks3);
            const uint4* sa = stage + (size_t) (g & 3u) * GH_STAGE_U4 + (size_t) (wm * 128) * GH_KC + frag_off;
            const uint4* sb = stage + (size_t) (g & 3u) * GH_STAGE_U4 + (size_t) (GH_BM + wn * 64) * GH_KC + frag_off;
            // All twelve fragment reads first (an LDS-DMA write may not overtake an LDS read); the four LDS-DMA pieces of stage
            // g + 3 then go out one by one BETWEEN the MFMA groups, so that no two waves of a SIMD pay their issue cost at the
            // same time with the matrix pipe idle (K2g's schedule, vsr_gemm.h).
            f16x8 bfr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = __builtin_bit_cast(f16x8, sb[j * 64]);
            f16x8 afr[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) afr[i] = __builtin_bit_cast(f16x8, sa[i * 64]);
            gh_lds_u4* dst = (gh_lds_u4*) (stage + (size_t) ((g + 3) & 3u) * GH_STAGE_U4);
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
#pragma unroll
                for (int i = 2 * qd; i < 2 * qd + 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[i], bfr[j], acc[i][j], 0, 0, 0);
                const int pc = qd >> 1;
                if ((qd & 1) == 0)
                    __builtin_amdgcn_global_load_lds(as_global((nxt ? a_nxt[pc] : a_cur[pc]) + ac3), dst + (wave * 2 + pc) * 64, 16, 0, 0);
                else
                    __builtin_amdgcn_global_load_lds(as_global(b_src[pc] + (size_t) ks3 * GH_KC),
                                                     dst + GH_BM * GH_KC + (wave * 2 + pc) * 64, 16, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        a_cur[0] = a_nxt[0];
        a_cur[1] = a_nxt[1];

        // ---- epilogue: acc[i][j][r] belongs to row slot wm * 128 + i * 16 + kq * 4 + r and query column wn * 64 + j * 16 + li ----
        const int32_t* ridx = rowidx + (it & 1u) * GH_BM + wm * 128;
        const float* rval = rowval + (it & 1u) * GH_BM + wm * 128;
        const float* rnrm = rownrm + (it & 1u) * GH_BM + wm * 128;
        auto append = [&](uint32_t slot, float v, int32_t row) {
            const uint32_t at = atomicAdd(p.qcnt + slot, 1u);
            if (at < p.capq) p.qcand[(size_t) slot * p.capq + at] = make_key(v, (uint32_t) row);
        };
        if (!generic) {
            // Candidates are PARKED in LDS while the tile's results are looked through (no returning global atomic in there).
            // Afterwards ONE wave instruction reserves room for all of them (lane c: the candidates of column c), and the keys
            // are stored at the start of the NEXT tile's epilogue, when that atomic has long returned.
            flush_store();
            n_park = 0;
            float tr[8][4];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 t4 = *reinterpret_cast<const float4*>(&rval[i * 16 + kq * 4]);
                tr[i][0] = t4.x; tr[i][1] = t4.y; tr[i][2] = t4.z; tr[i][3] = t4.w;
            }
            float cs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cs[j] = METRIC == M_COSINE ? colc[wn * 64 + j * 16 + li].y : 0.0f;
            // one pass over the 32 result blocks: the block's largest acc - (what it must reach) (a NaN row threshold drops out
            // of fmaxf), one ballot, and only a block that holds a candidate looks at its four values again
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float sl[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (METRIC == M_COSINE) sl[r] = fmaf(-cs[j], tr[i][r], acc[i][j][r]);
                        else sl[r] = acc[i][j][r] - tr[i][r];
                    }
                    const float best = fmaxf(fmaxf(sl[0], sl[1]), fmaxf(sl[2], sl[3]));
                    if (__ballot(best >= 0.0f)) {
                        const float4 cc = colc[wn * 64 + j * 16 + li];
                        const uint32_t slot = __float_as_uint(cc.w);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool c = sl[r] >= 0.0f;
                            const uint64_t cm = __ballot(c);
                            if (!cm) continue;
                            const int32_t row = ridx[i * 16 + kq * 4 + r];
                            // K2hw's key: the dot product without the folded start (cosine folds nothing: cc.x = 0)
                            const float v = screen_value<METRIC>(acc[i][j][r] - cc.x, rnrm[i * 16 + kq * 4 + r], cc.z);
                            const uint32_t at = n_park + __builtin_amdgcn_mbcnt_hi((uint32_t) (cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) cm, 0u));
                            if (c) {
                                if (at < (uint32_t) GH_PARK) {
                                    pk_v[at] = mono_bits(v);
                                    pk_r[at] = (uint32_t) row;
                                    pk_c[at] = (uint32_t) (j * 16 + li);
                                } else
                                    append(slot, v, row);                      // a burst beyond the parking area: directly
                            }
                            n_park += (uint32_t) __popcll(cm);
                        }
                    }
                }
            if (n_park > (uint32_t) GH_PARK) n_park = GH_PARK;
            flush_reserve();
        } else {
            // generic: the screening value of every valid pair.  SAMPLE keeps one minimum per query column and wave-tile
            // (128 rows), or per lane (`fine`); an open threshold admits every valid pair (only planned for filters that fit the buffer)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 cc = colc[wn * 64 + j * 16 + li];
                const uint32_t slot = __float_as_uint(cc.w);
                const float lim = collim[wn * 64 + j * 16 + li];                // (generic main pass: columns with a threshold keep it)
                uint64_t best = KEY_EMPTY;
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int32_t row = ridx[i * 16 + kq * 4 + r];
                        const float v = screen_value<METRIC>(acc[i][j][r], rnrm[i * 16 + kq * 4 + r], cc.z);
                        if (row < 0 || slot == 0xFFFFFFFFu) continue;
                        if constexpr (SAMPLE) {
                            const uint64_t key = make_key(v, (uint32_t) row);
                            best = key < best ? key : best;
                        } else {
                            if (!(v > lim)) append(slot, v, row);
                        }
                    }
                if constexpr (SAMPLE) {
                    if (!sample_fine) {                                        // one minimum per column and wave-tile (128 rows)
                        uint64_t o = __shfl_xor(best, 16);
                        best = o < best ? o : best;
                        o = __shfl_xor(best, 32);
                        best = o < best ? o : best;
                        if (kq != 0) best = KEY_EMPTY;
                    }
                    if (best != KEY_EMPTY) {
                        const uint32_t at = atomicAdd(p.qcnt + slot, 1u);
                        if (at < p.capq) p.qcand[(size_t) slot * p.capq + at] = best;
                    }
                }
            }
        }
    }
    if (!generic) flush_store();
    // the three stages still in flight write LDS: they must have landed before the workgroup gives its LDS back
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int METRIC>
hipError_t launch_gemmh_metric(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    const size_t lds = gemmh_lds_bytes();
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(GH_THREADS), lds, s, p);
        return hipGetLastError();
    };
    // whole chunks, rows long enough for the pipeline, the padded binary16 query image, K2w's candidate buffers, no view
    if (p.stride4 % 2 != 0 || !gemmh_supported(p.stride4 / 2) || !p.rows || !p.q_scr || !p.qcand || !p.qcnt || !p.ones || p.rank ||
        p.rw == 0 || GH_BM % p.rw != 0 || p.qmax > (uint32_t) GH_BN || p.n_rows == 0)
        return hipErrorInvalidValue;
    return p.sample_stride > 1 ? launch(gemmh_screen_kernel<METRIC, true>) : launch(gemmh_screen_kernel<METRIC, false>);
}

}  // namespace vsr
