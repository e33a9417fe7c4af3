// vsr_i8r.h — K2r: the int8 sample pass of a class-view plan, fed from registers.
//
// K2i's sample pass (vsr_i8s.h, SAMPLE) was picked on the time it takes ALONE.  In the headline three batches are in flight
// and the pass runs beside the other batches' main launches, which keep four workgroups per CU resident (~104 VGPRs per
// wave, ~34 KB of LDS each: 136 of a CU's 160 KB).  K2i's workgroup needs 132 VGPRs and ~68 KB of LDS, so it enters a CU
// only after TWO main workgroups have retired and then holds their place for a kernel that is all prologue and memory
// latency.  K2r computes the same sample inside what four resident main workgroups leave over: at most 96 VGPRs (one more
// wave per SIMD) and ~9 KB of LDS.
//
//   * dense class view only (Plan::class_view): a pass's tile list is a slice of the view's identity list over ONE
//     contiguous run of rows (vsr_mfmaw.h, DENSE), so two descriptor loads in the prologue give the workgroup's rows
//     [row_lo, row_hi) and every address after that is affine in the stage index: no descriptor, bitmap or row-index load
//     in the loop;
//   * no LDS image of the rows: lane (li, kq) loads its A fragments of v_mfma_i32_16x16x64_i8 straight from global memory
//     (the 16 bytes of row li at byte blk * 64 + kq * 16: four lanes cover 64 contiguous bytes, the two K-blocks the 128-byte
//     row) and |row|^2 of its four result rows as one dwordx4.  The unit of the pipeline is a 16-row block (half a stage):
//     a ring of four units in registers (12 VGPRs each), three in flight under the arithmetic of the fourth.  All loads
//     return into registers, so the compiler counts the waits itself (s_waitcnt vmcnt(9) in the steady state); every load is
//     unconditional and its address clamped, never branched around (the rules in the header of vsr_mfmaw.h);
//   * the B fragments of the pass's <= 64 query columns are parked ONCE in LDS (8 KB per workgroup, fragment-major: a
//     ds_read_b128 per K-block and 16-column group, no bank conflict) and one group's accumulators live at a time;
//   * the sample is K2i's, bit for bit: the same 32-row stages, every ss-th stage of the same workgroup ranges, stage s of the
//     workgroup on wave s % 4, every lane's smallest (value, row) per query column over the wave's stream, 4 entries per
//     column and wave appended with one returning atomic per column and workgroup.  try_k2i_sample's thickness estimate,
//     seed_rank and seed_select_kernel do not know which of the two kernels ran.
//
// The only workgroup barriers are outside the loop: one after the B fragments are parked, two around the hand-over of the
// waves' minima (the B area is reused for them, so the last barrier replaces K2i's arrival counter).
#pragma once
#include <type_traits>
#include "vsr_device.h"
#include "vsr_topk.h"
#include "vsr_mfma.h"

namespace vsr {

constexpr int KR_THREADS = 256;
constexpr int KR_WAVES = 4;
constexpr int KR_RING = 4;                 // 16-row units in registers per wave: one being multiplied, three in flight
constexpr int KR_OCC = 5;                  // waves per SIMD the register allocation aims at: 512 / 5 -> 96 VGPRs

template <int NQG>
__global__ __launch_bounds__(KR_THREADS, KR_OCC) void i8_sample_reg_kernel(const ScanParams p)
{
    constexpr int NC = NQG * 16;                                                // query columns of a sample group, at most
    static_assert(NC == 64, "one lane of the appending wave per query column");
    __shared__ __align__(16) uint4 s_b[NQG * 2 * 64];                           // B fragments [group][K-block][lane]; at the end the
                                                                                // waves' minima [wave][column][row quad] (8 KB)
    __shared__ uint2 s_col[NC];                                                 // {|q|^2 bits, slot (pad column: ~0u)}
    static_assert(sizeof(uint4) * NQG * 2 * 64 >= sizeof(uint64_t) * KR_WAVES * NC * 4, "minima do not fit the B area");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    uint32_t lo = 0, hi = p.n_groups;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.groups[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
    }
    const ScanGroup grp = p.groups[lo];
    const uint32_t local_block = blockIdx.x - grp.block_begin;
    const auto g_tiles = as_global(grp.tiles);
    const auto g_norm2 = as_global(p.norm2);
    const auto g_rank = as_global(p.rank);
    const uint32_t q_count = grp.q_count;

    // ---- query columns and their B fragments: lane L of fragment (j, ks) is query j * 16 + (L & 15), chunk ks * 4 + (L >> 4) ----
    uint4 bq[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t idx = (uint32_t) tid + 256u * e;
        const uint32_t qi = (idx >> 7) * 16u + (idx & 15u);
        const uint32_t slot = p.q_slots[grp.q_begin + (qi < q_count ? qi : 0u)];                 // pad columns repeat query 0
        bq[e] = p.q_scr[(size_t) slot * p.pstride4 + ((idx >> 6) & 1u) * 4u + ((idx & 63u) >> 4)];
    }
    if (tid < NC) {
        const bool qok = (uint32_t) tid < q_count;
        const uint32_t slot = p.q_slots[grp.q_begin + (qok ? (uint32_t) tid : 0u)];
        s_col[tid] = make_uint2(__float_as_uint(p.q_norm2[slot]), qok ? slot : 0xFFFFFFFFu);
    }

    // ---- this wave's stages (K2i's geometry): stage i of the wave = list tiles t0 + 2 ss (wave + 4 i) + {0, 1} ----
    const uint32_t t0 = (uint32_t) (((uint64_t) grp.n_tiles * local_block) / grp.n_blocks);
    const uint32_t t1 = (uint32_t) (((uint64_t) grp.n_tiles * (local_block + 1)) / grp.n_blocks);
    const uint32_t ss = p.sample_stride;
    const uint32_t n_st = (((t1 - t0 + 1u) >> 1) + ss - 1u) / ss;
    const uint32_t n_w = n_st > (uint32_t) wave ? (n_st - (uint32_t) wave + 3u) >> 2 : 0u;
    const uint32_t n_units = 2u * n_w;                                          // 16-row units: two per stage
    const uint32_t unit_last = n_units ? n_units - 1u : 0u;

    // the workgroup's rows: two descriptors, then arithmetic (every tile of an identity list but a class's last is full)
    const uint32_t tile_last = grp.n_tiles - 1u;
    uint32_t row_lo, row_hi;
    bool bad_row;
    {
        const uint2 da = load_tile(g_tiles, t0 < tile_last ? t0 : tile_last);
        const uint2 db = load_tile(g_tiles, t1 > t0 && t1 - 1u < tile_last ? t1 - 1u : tile_last);
        row_lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) da.x);
        row_hi = t1 > t0 ? (uint32_t) __builtin_amdgcn_readfirstlane((int) (db.x + db.y)) : row_lo;
        bad_row = row_hi > p.n_rows || row_hi < row_lo;                         // cannot happen: reported once at the end
        row_hi = bad_row ? row_lo : row_hi;
    }
    // Whole units are loaded wherever they start (rows from row_hi on are masked by their threshold): the first row is
    // clamped to the last 16-row boundary inside the planes, and the planes and norms are padded past it by more than
    // the 15 rows such a read can reach (ClassView, vsr_runtime.h).
    const uint32_t row_clamp = (p.n_rows - 1u) & ~15u;

    // MFMA lane roles (16x16x64 int8): A lane = (row li, 16-byte k-chunk kq); B / result lane = (k-chunk kq | row quad kq, query li)
    const int li = lane & 15;
    const int kq = lane >> 4;
    const uint32_t ngt = (q_count + 15u) >> 4;                                  // 16-query groups in use (wave-uniform)
    const uint32_t voff = (uint32_t) li * 128u + (uint32_t) kq * 16u;
    const char* scr = reinterpret_cast<const char*>(p.scr);

    // first row of unit u of this wave (wave-uniform); units past the wave's last repeat it: same lines, nothing new from HBM
    auto unit_row = [&](uint32_t u) -> uint32_t {
        const uint32_t uc = u < unit_last ? u : unit_last;
        return row_lo + 32u * ss * ((uint32_t) wave + 4u * (uc >> 1)) + 16u * (uc & 1u);
    };
    i32x4 a8[KR_RING][2];                                                       // A fragments of the ring's units, two K-blocks
    f32x4 nrm[KR_RING];                                                         // |row|^2 of the lane's four result rows
    auto issue = [&](auto K, uint32_t u) {
        constexpr int k = decltype(K)::value;
        const uint32_t r0 = unit_row(u);
        const uint32_t rc = r0 < row_clamp ? r0 : row_clamp;
        const gptr<uint4> src = as_global(reinterpret_cast<const uint4*>(scr + (size_t) rc * 128u + voff));
        a8[k][0] = __builtin_bit_cast(i32x4, src[0]);
        a8[k][1] = __builtin_bit_cast(i32x4, src[4]);
        nrm[k] = *reinterpret_cast<gptr<f32x4>>(g_norm2 + rc + (uint32_t) kq * 4u);
    };
    issue(std::integral_constant<int, 0>{}, 0u);
    issue(std::integral_constant<int, 1>{}, 1u);
    issue(std::integral_constant<int, 2>{}, 2u);

    s_b[tid] = bq[0];
    s_b[tid + 256] = bq[1];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");             // (LDS only: the units in flight are not waited for)

    int64_t smin[NQG];                                                          // per column of this lane, (value, row)
#pragma unroll
    for (int j = 0; j < NQG; ++j) smin[j] = ((int64_t) 0x3FFFFFFF << 32);
    // acc[r] = row kq * 4 + r of the unit, query column j * 16 + li; values are compared as integers (|x'|^2 - 2 x'.q')
    auto compute = [&](auto K, uint32_t u) {
        constexpr int k = decltype(K)::value;
        const uint32_t row = unit_row(u) + (uint32_t) kq * 4u;
        int32_t nx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) nx[r] = row + (uint32_t) r < row_hi ? (int32_t) nrm[k][r] : 0x3FFFFFFF;   // no row: never the minimum
#pragma unroll
        for (int j = 0; j < NQG; ++j) {
            if ((uint32_t) j < ngt) {
                const i32x4 b0 = __builtin_bit_cast(i32x4, s_b[(j * 2 + 0) * 64 + lane]);
                const i32x4 b1 = __builtin_bit_cast(i32x4, s_b[(j * 2 + 1) * 64 + lane]);
                i32x4 acc = i32x4{0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a8[k][0], b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a8[k][1], b1, acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int32_t w = nx[r] - 2 * acc[r];
                    const int64_t cand = ((int64_t) w << 32) | (int64_t) (row + (uint32_t) r);
                    smin[j] = cand < smin[j] ? cand : smin[j];
                }
            }
        }
    };
    // Four units per trip, so that every ring slot is a compile-time index.  A trip may run up to two units past the wave's
    // last: they repeat the last unit, and taking a minimum twice changes nothing.
    for (uint32_t u = 0; u < n_units; u += 4u) {
        issue(std::integral_constant<int, 3>{}, u + 3u);
        compute(std::integral_constant<int, 0>{}, u);
        issue(std::integral_constant<int, 0>{}, u + 4u);
        compute(std::integral_constant<int, 1>{}, u + 1u);
        issue(std::integral_constant<int, 1>{}, u + 5u);
        compute(std::integral_constant<int, 2>{}, u + 2u);
        issue(std::integral_constant<int, 2>{}, u + 6u);
        compute(std::integral_constant<int, 3>{}, u + 3u);
    }

    // ---- every wave's minima go to the (now idle) B area; wave 0 appends all of them: one returning atomic per query
    // column and workgroup (vsr_i8s.h).  A wave without a stage hands over empty keys. ----
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");             // nobody reads B fragments any more
    uint64_t* keys = reinterpret_cast<uint64_t*>(s_b);                          // [wave][NC][4]: column, row quad
#pragma unroll
    for (int j = 0; j < NQG; ++j) {
        const int32_t w = (int32_t) (smin[j] >> 32);
        uint64_t key = KEY_EMPTY;
        if ((uint32_t) j < ngt && w < 0x20000000) {
            const uint2 cc = s_col[j * 16 + li];
            const uint32_t row = (uint32_t) smin[j];
            if (cc.y != 0xFFFFFFFFu) key = make_key((float) w + __uint_as_float(cc.x), g_rank ? g_rank[row] : row);   // integers below 2^24: the fp32 distance
        }
        keys[(wave * NC + j * 16 + li) * 4 + kq] = key;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == 0) {
        const int c = lane;
        const uint32_t slot = s_col[c].y;
        uint64_t keys16[4 * KR_WAVES];
        uint32_t n = 0;
#pragma unroll
        for (int w2 = 0; w2 < KR_WAVES; ++w2)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const uint64_t kk = keys[(w2 * NC + c) * 4 + q4];
                keys16[w2 * 4 + q4] = kk;
                n += kk != KEY_EMPTY;
            }
        if (n && slot != 0xFFFFFFFFu) {
            uint32_t at = atomicAdd(p.qcnt + slot, n);
#pragma unroll
            for (int t = 0; t < 4 * KR_WAVES; ++t)
                if (keys16[t] != KEY_EMPTY) {
                    if (at < p.capq) p.qcand[(size_t) slot * p.capq + at] = keys16[t];
                    ++at;
                }
        }
        if (bad_row && lane == 0) atomicOr(p.err, 1u);                          // a range reached past the planes: results invalid
    }
}

// Drop-in for launch_i8_stream's SAMPLE launch when every group's tile list is a slice of a class view's identity list.
inline hipError_t launch_i8_sample_reg(const ScanParams& p, uint32_t n_blocks, hipStream_t s)
{
    if (p.plane_ho != 2 || p.pstride4 != 8 || p.rw != 16 || p.sample_stride < 2 || p.block_map || p.n_rows < 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(i8_sample_reg_kernel<4>, dim3(n_blocks), dim3(KR_THREADS), 0, s, p);   // (sample groups never exceed 64 columns)
    return hipGetLastError();
}

}  // namespace vsr
