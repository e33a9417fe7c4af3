// vsr_mfmab.h — K2b: shared passes over a bit corpus on the int8 matrix cores.  Hamming and Jaccard, exact.
//
// CDNA4 has no 1-bit MFMA and needs none: popcount(a & b) of two packed bit strings is the dot product of the strings
// unpacked to bytes of 0 / 1, and v_mfma_i32_16x16x64_i8 computes that dot product exactly in int32 -- 16 rows x 16 queries
// x 64 bits per instruction, where K1b (vsr_scanb.h) spends 4 x (and | xor) + 4 x popcount per (row, query) and 128 bits.
// With ab from the matrix cores, aa = |row| (p.norm2, written at load) and bb = |query| (p.q_norm2, written by staging):
//     Hamming = aa + bb - 2 ab          Jaccard = bitutils.c:125-128 on (ab, aa, bb), rank_value_bits (vsr_bitops.h)
// Everything is an integer, so the keys are K1b's keys: make_key(rank_value_bits(...), internal row), admitted by
// `key < tau`.  No screening tier, no error bound, no flags, no re-rank, no tau_init, no sample pass, no rank map (a
// list-ordered view stays on K1b: launch_mfmab_metric refuses p.rank).
//
// Skeleton: K2's (vsr_mfma.h, restated as K2h restates it; a fix to the vote / publish protocol belongs in all three):
// ScanParams / ScanGroup passes, block_map or the search on block_begin, MF_WAVES waves that each own 64-row tiles, NG
// groups of 16 query columns (pad columns repeat query 0 and never append), per-query TopKCtrl in LDS, candidates appended
// to the workgroup's global buffers (p.cand), overflow vote every K2_VOTE_EVERY tiles, publish of kp keys per query.
//
// Operands.  A row (and a staged query) is stride4 16-byte chunks of packed bits, pad bits zero.  One chunk feeds two
// K-steps of 64 bits.  Lane (i = lane & 15, kq = lane >> 4) owns, at K-step t, the 16 bits of half (t & 1) of dword kq of
// chunk t >> 1 -- of row i for the A operand, of query i for B -- and unpacks them to 16 bytes of 0 / 1 (one i32x4
// fragment): four bits become four bytes by (nibble * 0x00204081) & 0x01010101 (the products' bit positions i + 7 j are
// distinct: no carries).  A and B take the same 16 bits for the same (t, kq), so the sum runs over matching bit positions
// whatever order the hardware walks a fragment in (the argument of vsr_mfmah.h); the C / D layout is K2's.  This slicing
// (a lane's two K-steps of a chunk in ONE dword) instead of bits [64 t + 16 kq, + 16) makes the lane's share of a chunk a
// single global_load_dword: the four lanes of a row read the chunk's 16 bytes once, nothing is loaded twice or discarded.
//
// Data movement.  No LDS image of the rows: a 64-row tile at 768 bits is 6 KB and a lane wants 4 bytes of a chunk, so
// the lanes load their dwords straight from global memory (as_global, as K2r's register-fed operands), a stage of MB_SC
// chunks (8 K-steps) at a time, the next stage in flight under the unpacking and MFMAs of the current one.  The next
// tile is resolved under the current one: its descriptor arrives one tile ahead, its permission word and popcount are
// requested at the top of the current tile, and its first stage is issued before the current tile's last stage is
// consumed.  The unpacked A fragments of a K-step are reused by the NG groups; the B fragments are unpacked once per pass
// and stay in registers for rows of up to NSTR stages (NSTR > 0), else (NSTR == 0) the packed query dwords are streamed
// from the staged copy one stage ahead and unpacked at each K-step.
#pragma once
#include "vsr_mfma.h"
#include "vsr_bitops.h"

namespace vsr {

constexpr int MB_SC = 4;                  // 16-byte chunks per stage
constexpr int MB_KS = 2 * MB_SC;          // K-steps (64 bits) per stage

// the low 16 bits of w >> sh as 16 bytes of 0 / 1
__device__ __forceinline__ i32x4 unpack_bits16(uint32_t w, int sh)
{
    i32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (int) (__umul24((w >> (sh + 4 * j)) & 0xFu, 0x00204081u) & 0x01010101u);
    return r;
}

template <bool JACCARD, int NSTR, int NG>
__global__ __launch_bounds__(MF_THREADS, 2) void mfmab_scan_kernel(const ScanParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // workgroup -> (pass, block of the pass), as in mfma_scan_kernel
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
    const auto g_rows = as_global(reinterpret_cast<const uint32_t*>(p.rows));
    const auto g_norm = as_global(p.norm2);

    const uint32_t nchunk = p.stride4, cap = p.cap, keep = p.k;
    const uint32_t nstage = (nchunk + MB_SC - 1) / MB_SC;
    const uint32_t q_count = grp.q_count;

    // LDS (mfmab_lds_bytes): the sort buffer of a compaction (cap keys; its head doubles as the publish's histograms),
    // per wave the tile's row indices and popcounts for the epilogue, the per-query control words
    constexpr int NQ = MF_NQ * NG;
    uint64_t* sortbuf = reinterpret_cast<uint64_t*>(smem);
    unsigned char* after = smem + (size_t) cap * 8;
    int32_t*  ridx = reinterpret_cast<int32_t*>(after) + wave * 64;
    float*    rnrm = reinterpret_cast<float*>(after + MF_WAVES * 64 * 4) + wave * 64;
    TopKCtrl* ctrl = reinterpret_cast<TopKCtrl*>(after + MF_WAVES * 64 * 8);
    float*    qnl = reinterpret_cast<float*>(ctrl + NQ);
    uint32_t* flags = reinterpret_cast<uint32_t*>(qnl + NQ);

    for (uint32_t qi = tid; qi < (uint32_t) NQ; qi += MF_THREADS) {
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];
        ctrl[qi].tau = KEY_EMPTY;
        ctrl[qi].count = 0;
        qnl[qi] = p.q_norm2[slot];
    }
    if (tid < 4) flags[tid] = 0;
    __syncthreads();

    // MFMA lane roles: A operand lane = (row i, dword kq of a chunk); B operand / result lane = (dword kq, query jq)
    const int li = lane & 15;
    const int kq = lane >> 4;
    const int jq = li;
    constexpr int NB = NSTR > 0 ? NSTR : 1;
    i32x4 bq[NB][NG][MB_KS];                                                   // NSTR > 0: the pass's B fragments
    float my_qn[NG];
    gptr<uint32_t> qsrc_g[NG];                                                 // this lane's query column per group
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t qi = (uint32_t) (g * MF_NQ + jq);
        my_qn[g] = qnl[qi];
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0)];   // pad columns repeat query 0
        qsrc_g[g] = as_global(reinterpret_cast<const uint32_t*>(p.queries)) + (size_t) slot * nchunk * 4 + kq;
        if constexpr (NSTR > 0) {
#pragma unroll
            for (int s = 0; s < NSTR; ++s)
#pragma unroll
                for (int c = 0; c < MB_SC; ++c) {
                    const uint32_t idx = (uint32_t) (s * MB_SC + c);
                    const uint32_t w = idx < nchunk ? qsrc_g[g][idx * 4] : 0u;   // chunks past the row end multiply as zero
                    bq[s][g][2 * c] = unpack_bits16(w, 0);
                    bq[s][g][2 * c + 1] = unpack_bits16(w, 16);
                }
        }
    }
    // NSTR == 0: the packed query dwords of the stage in use (qcur) and of the next one (qnxt, raw loads: zeroed for chunks
    // past the row end only when they become qcur, so that nothing touches them while they are in flight)
    uint32_t qcur[NG][MB_SC], qnxt[NG][MB_SC];
    auto issue_b = [&](uint32_t s_) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int c = 0; c < MB_SC; ++c) {
                const uint32_t idx = s_ * MB_SC + (uint32_t) c;
                qnxt[g][c] = qsrc_g[g][(idx < nchunk ? idx : 0u) * 4];
            }
    };
    auto take_b = [&](uint32_t s_) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int c = 0; c < MB_SC; ++c) qcur[g][c] = s_ * MB_SC + (uint32_t) c < nchunk ? qnxt[g][c] : 0u;
    };

    const uint32_t rw = p.rw, tps = 64 / rw;
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t n_super = (t1 - t0 + tps - 1) / tps;
    const uint32_t iters = (n_super + MF_WAVES - 1) / MF_WAVES;
    const uint32_t trigger = cap - MF_SLACK;
    const uint32_t last_row = p.n_rows - 1u;
    uint64_t* cand = p.cand + (size_t) (grp.partial_begin + local_block) * cand_pitch(cap);
    const size_t cand_qstride = (size_t) grp.n_blocks * cand_pitch(cap);

    auto fetch_desc = [&](uint32_t it_) -> uint2 {               // (start, nrows) of this lane's list tile, or (0, 0)
        const uint32_t sup = it_ * MF_WAVES + wave;
        if (it_ >= iters || sup >= n_super) return make_uint2(0u, 0u);
        const uint32_t t = t0 + sup * tps + (uint32_t) lane / rw;
        if (t >= t1) return make_uint2(0u, 0u);
        if (t >= grp.n_tiles) {                                  // cannot happen; never read past the tile list
            atomicOr(p.err, 4u);
            return make_uint2(0u, 0u);
        }
        if (g_tiles) return load_tile(g_tiles, t);
        const uint32_t start = t * rw;
        return make_uint2(start, p.n_rows - start < rw ? p.n_rows - start : rw);
    };
    // A tile is resolved in two halves so that nothing waits for a load where it is issued: `ask` requests the permission
    // word and the popcount of this lane's row of the tile (an in-range row whatever the descriptor says), `settle` turns
    // them into the lane's row or -1.
    struct Asked { uint32_t row; bool in; uint64_t word; float pop; };
    auto ask = [&](uint2 d) -> Asked {
        Asked a;
        const uint32_t r = (uint32_t) lane % rw;
        a.in = r < d.y;
        a.row = d.x + r;
        if (a.in && a.row >= p.n_rows) {                         // cannot happen; never read past the corpus
            atomicOr(p.err, 1u);
            a.in = false;
        }
        const uint32_t rc = a.in ? a.row : 0u;
        a.word = g_bitmap ? g_bitmap[rc >> 6] : ~0ull;
        a.pop = g_norm[rc];
        return a;
    };
    auto settle = [&](const Asked& a) -> int32_t {
        return a.in && ((a.word >> (a.row & 63u)) & 1ull) ? (int32_t) a.row : -1;
    };
    // this lane's A rows: row (sub * 16 + li) of the tile whose rows the lanes hold in `row`, as a dword offset (64-bit: a corpus may exceed 16 GiB); an invalid
    // slot (masked row, ragged tile) reads row 0 and its products are discarded by the `rows4[r] >= 0` test of the epilogue
    auto a_rows = [&](int32_t row, uint64_t (&off)[4]) {
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int32_t r = __shfl(row, sub * 16 + li);
            const uint32_t rc = r < 0 ? 0u : (uint32_t) r;
            off[sub] = (uint64_t) (rc < last_row ? rc : last_row) * (nchunk * 4u) + (uint32_t) kq;
        }
    };
    // global loads of stage s (no waits, nothing may consume the registers here); the padding chunks of a ragged last
    // stage load chunk 0 and meet zero B fragments
    auto issue = [&](uint32_t s, const uint64_t (&off)[4], uint32_t (&x)[4][MB_SC]) {
#pragma unroll
        for (int c = 0; c < MB_SC; ++c) {
            const uint32_t chunk = s * MB_SC + (uint32_t) c;
            const uint32_t cc = (chunk < nchunk ? chunk : 0u) * 4u;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) x[sub][c] = g_rows[off[sub] + cc];
        }
    };

    // pipeline state: `nxt` holds the loads in flight -- the next stage of this tile, or stage 0 of the next tile
    uint32_t nxt[4][MB_SC];
    uint64_t aoff[4], aoff_n[4];
    Asked asked = ask(fetch_desc(0));
    int32_t myrow = settle(asked);
    float myrn = asked.pop;
    a_rows(myrow, aoff);
    issue(0, aoff, nxt);
    uint2 desc_n = fetch_desc(1);
    uint32_t round = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const bool have = __ballot(myrow >= 0) != 0;                           // wave-uniform
        asked = ask(desc_n);                                                   // the next tile's word and popcount: requested now,
        desc_n = fetch_desc(it + 2);                                           // used in next_tile; the descriptor after it
        int32_t nrow = -1;
        auto next_tile = [&]() {                                               // resolve the next tile and issue its first stage
            nrow = settle(asked);
            a_rows(nrow, aoff_n);
            issue(0, aoff_n, nxt);
        };
        if (have) {
            ridx[lane] = myrow;
            rnrm[lane] = myrn;

            i32x4 acc[NG][4];
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) acc[g][sub] = i32x4{0, 0, 0, 0};

            if constexpr (NSTR == 0) {
                issue_b(0);
                take_b(0);
            }
            auto do_stage = [&](uint32_t s, const i32x4 (&bs)[NG][MB_KS]) {
                uint32_t cur[4][MB_SC];
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int c = 0; c < MB_SC; ++c) cur[sub][c] = nxt[sub][c];
                if (s + 1 < nstage) issue(s + 1, aoff, nxt);                   // in flight during the MFMAs
                else next_tile();
                if constexpr (NSTR == 0)
                    if (s + 1 < nstage) issue_b(s + 1);
#pragma unroll
                for (int t = 0; t < MB_KS; ++t) {
                    if (s * MB_KS + (uint32_t) t >= 2u * nchunk) break;        // wave-uniform: K-steps past the row end
                    i32x4 b[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        if constexpr (NSTR > 0) b[g] = bs[g][t];
                        else b[g] = unpack_bits16(qcur[g][t >> 1], 16 * (t & 1));
                    }
                    // the A fragments of the four 16-row sub-tiles are unpacked once and multiplied against every group
                    i32x4 a[4];
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub) a[sub] = unpack_bits16(cur[sub][t >> 1], 16 * (t & 1));
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int g = 0; g < NG; ++g)
                            acc[g][sub] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[sub], b[g], acc[g][sub], 0, 0, 0);
                }
                if constexpr (NSTR == 0)
                    if (s + 1 < nstage) take_b(s + 1);                         // landed under this stage's MFMAs
            };
            if constexpr (NSTR > 0) {
#pragma unroll
                for (int s = 0; s < NSTR; ++s)
                    if ((uint32_t) s < nstage) do_stage((uint32_t) s, bq[s]);
            } else {
                for (uint32_t s = 0; s < nstage; ++s) do_stage(s, bq[0]);
            }

            // results: acc[g][sub][r] = popcount(row sub*16 + kq*4 + r AND query g*16 + jq)
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const uint32_t qi = (uint32_t) (g * MF_NQ + jq);
                const uint64_t tau = lds_peek(&ctrl[qi].tau);
                const bool qok = qi < q_count;
                uint64_t keys[16];
                uint32_t pmask = 0;
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const int4 ri = *reinterpret_cast<const int4*>(&ridx[sub * 16 + kq * 4]);
                    const float4 rn = *reinterpret_cast<const float4*>(&rnrm[sub * 16 + kq * 4]);
                    const int32_t rows4[4] = {ri.x, ri.y, ri.z, ri.w};
                    const float nx4[4] = {rn.x, rn.y, rn.z, rn.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool live = qok && rows4[r] >= 0;
                        const uint32_t ab = (uint32_t) acc[g][sub][r];
                        // Hamming: popcount(a ^ b) = aa + bb - 2 ab (popcounts up to 64000: exact in fp32 and uint32)
                        const uint32_t pv = JACCARD ? ab : (uint32_t) nx4[r] + (uint32_t) my_qn[g] - 2u * ab;
                        const float v = live ? rank_value_bits<JACCARD>(pv, nx4[r], my_qn[g]) : 0.0f;   // the division: live pairs only
                        const uint64_t key = make_key(v, (uint32_t) rows4[r]);
                        keys[sub * 4 + r] = key;
                        if (live && key < tau) pmask |= 1u << (sub * 4 + r);
                    }
                }
                if (__ballot(pmask != 0) != 0) {                               // wave-uniform
                    uint32_t base = 0;
                    if (pmask) base = atomicAdd(&ctrl[qi].count, (uint32_t) __popc(pmask));
                    if (pmask && base + (uint32_t) __popc(pmask) > cap) {      // cannot happen (append slack protocol)
                        atomicOr(p.err, 2u);
                        pmask = 0;
                    }
                    uint64_t* dst = cand + (size_t) qi * cand_qstride + base;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (pmask & (1u << i)) dst[__popc(pmask & ((1u << i) - 1u))] = keys[i];
                }
            }
        } else {
            next_tile();
        }
        myrow = nrow;
        myrn = asked.pop;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) aoff[sub] = aoff_n[sub];

        if (it + 1 < iters && (it + 1) % K2_VOTE_EVERY == 0) {
            bool need = false;
            for (uint32_t q = 0; q < q_count; ++q)
                need |= lds_peek(&ctrl[q].count) > trigger;
            const uint32_t slot = round % 3;
            if (need && lane == 0) atomicOr(&flags[slot], 1u);
            __syncthreads();
            const bool any = lds_peek(&flags[slot]) != 0;
            if (tid == 0) flags[(round + 2) % 3] = 0;
            ++round;
            if (any) {
                for (uint32_t q = 0; q < q_count; ++q) {
                    const uint32_t n = ctrl[q].count < cap ? ctrl[q].count : cap;
                    if (n > trigger) {                                         // only the buffers that are filling up
                        uint64_t* cq = cand + (size_t) q * cand_qstride;
                        for (uint32_t i = tid; i < n; i += MF_THREADS) sortbuf[i] = cq[i];
                        __syncthreads();
                        topk_compact<MF_THREADS>(sortbuf, &ctrl[q], keep, tid, false);
                        for (uint32_t i = tid; i < keep; i += MF_THREADS) cq[i] = sortbuf[i];
                        __syncthreads();
                    }
                }
            }
        }
    }

    __syncthreads();
    constexpr int PR = 32;                                                     // candidate keys per lane at publish
    if (cap <= (uint32_t) (64 * PR)) {
        // publish, one wave per query: radix select of the `keep` smallest candidates (vsr_topk.h), as mfma_scan_kernel
        uint32_t* hist = reinterpret_cast<uint32_t*>(smem) + wave * 256;       // wave-private; the sort buffer is dead by now
        for (uint32_t q = (uint32_t) wave; q < q_count; q += MF_WAVES) {
            const uint32_t n = ctrl[q].count < cap ? ctrl[q].count : cap;
            const uint64_t* cq = cand + (size_t) q * cand_qstride;
            uint64_t* dst = p.partial + (size_t) (grp.partial_begin + q * grp.n_blocks + local_block) * p.kp;
            if (n <= keep) {                                                   // nothing to drop
                for (uint32_t i = (uint32_t) lane; i < p.kp; i += 64) dst[i] = i < n ? cq[i] : KEY_EMPTY;
                continue;
            }
            auto pick = [&](auto rc) {                                         // RR keys per lane cover the n candidates
                constexpr int RR = decltype(rc)::value;
                uint64_t reg[RR];
#pragma unroll
                for (int r = 0; r < RR; ++r) {
                    const uint32_t i = (uint32_t) (r * 64 + lane);
                    reg[r] = cq[i < n ? i : 0u];
                }
#pragma unroll
                for (int r = 0; r < RR; ++r)
                    if ((uint32_t) (r * 64 + lane) >= n) reg[r] = KEY_EMPTY;
                uint64_t tsel, kth;
                wave_radix_select<RR>(reg, n, keep, hist, lane, tsel, kth);
                const uint32_t want = wave_emit_selected<RR>(reg, n, keep, tsel, kth, dst, lane);
                for (uint32_t i = want + (uint32_t) lane; i < p.kp; i += 64) dst[i] = KEY_EMPTY;
            };
            if (n <= 256) pick(std::integral_constant<int, 4>{});
            else if (n <= 512) pick(std::integral_constant<int, 8>{});
            else pick(std::integral_constant<int, PR>{});
        }
        return;
    }
    for (uint32_t q = 0; q < q_count; ++q) {
        const uint32_t n = ctrl[q].count < cap ? ctrl[q].count : cap;
        const uint64_t* cq = cand + (size_t) q * cand_qstride;
        for (uint32_t i = tid; i < n; i += MF_THREADS) sortbuf[i] = cq[i];
        __syncthreads();
        topk_compact<MF_THREADS>(sortbuf, &ctrl[q], keep, tid, false);
        const uint32_t m = ctrl[q].count < keep ? ctrl[q].count : keep;
        uint64_t* dst = p.partial + (size_t) (grp.partial_begin + q * grp.n_blocks + local_block) * p.kp;
        for (uint32_t i = tid; i < p.kp; i += MF_THREADS) dst[i] = i < m ? sortbuf[i] : KEY_EMPTY;
        __syncthreads();
    }
}

template <bool JACCARD>
hipError_t launch_mfmab_metric(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    if (!p.cand || !p.norm2 || !p.q_norm2 || p.rank || p.stride4 == 0) return hipErrorInvalidValue;   // (a view stays on K1b)
    const uint32_t nstage = (p.stride4 + MB_SC - 1) / MB_SC;
    const int ng = p.qmax > (uint32_t) MF_NQ ? 2 : 1;
    const size_t lds = mfmab_lds_bytes(p.cap, ng * MF_NQ);
    auto launch = [&](auto kern) -> hipError_t {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(MF_THREADS), lds, s, p);
        return hipGetLastError();
    };
    auto pick = [&](auto nstr) -> hipError_t {
        constexpr int N = decltype(nstr)::value;
        return ng == 2 ? launch(mfmab_scan_kernel<JACCARD, N, 2>) : launch(mfmab_scan_kernel<JACCARD, N, 1>);
    };
    // B fragments in registers for one stage, for two with one query group (mfmab_nstr), streamed beyond
    switch (mfmab_nstr(nstage, ng)) {
    case 1:  return pick(std::integral_constant<int, 1>{});
    case 2:  return launch(mfmab_scan_kernel<JACCARD, 2, 1>);
    default: return pick(std::integral_constant<int, 0>{});
    }
}

}  // namespace vsr
