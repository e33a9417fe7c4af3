// vsr_scansi_sizing.h — what the planner, the image build and the launcher of K1si (vsr_scansi.h) decide without a GPU: the row
// block of the inverted image, the longest query the kernel sorts, and the LDS of a workgroup.  Plain C++ (no HIP header), so
// that a host compiler can build it alone; everything is constexpr, which makes it callable from device code too.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vsr {

constexpr int      SI_THREADS = 512;                     // 8 waves per workgroup: a round serves 8 queries of a pass
constexpr int      SI_WAVES = SI_THREADS / 64;
constexpr int      SI_QMAX = 16;                         // queries per pass (two rounds)
constexpr uint32_t SI_MAX_TERMS = 256;                   // non-zeros of the longest query a wave sorts in its LDS
constexpr size_t   SI_LDS_BUDGET = 80 * 1024;            // per workgroup at k = 100: two fit a CU's 160 KiB (K1sm's budget)
constexpr size_t   SI_LDS_MAX = 160 * 1024;              // per workgroup at any k: one fits

// LDS of one workgroup with row blocks of rb rows: the sort buffer of a compaction (cap keys), per wave the accumulators of a
// row block (rb doubles) and the query's sorted terms (SI_MAX_TERMS x (index, value)), the control words of a pass's queries
// (TopKCtrl: 16 bytes each) and the vote flags
constexpr size_t scansi_lds_bytes_rb(uint32_t cap, uint32_t rb)
{
    return (size_t) cap * 8 + (size_t) SI_WAVES * ((size_t) rb * 8 + (size_t) SI_MAX_TERMS * 8) + (size_t) SI_QMAX * 16 + 16;
}

// SI_RB, rows per row block of the image: the largest power of two (a multiple of 64: whole bitmap windows) at which the
// workgroup fits SI_LDS_BUDGET beside the sort buffer of k = 100 (cap = 2048 keys, mfma_cap_for_k).  A larger block halves the
// (block, index) segments a query term has to find and doubles their length, but the accumulators are what bounds the waves a
// CU keeps in flight, and the accumulate phase is a chain of dependent loads: 1024 rows would leave one workgroup per CU
// (96 KiB), 512 rows leave two (64 KiB)
constexpr uint32_t scansi_rows_per_block()
{
    uint32_t rb = 64;
    while (scansi_lds_bytes_rb(2048, rb * 2) <= SI_LDS_BUDGET) rb *= 2;
    return rb;
}
constexpr uint32_t SI_RB = scansi_rows_per_block();
constexpr uint32_t SI_RB_LOG2 = SI_RB == 64 ? 6 : SI_RB == 128 ? 7 : SI_RB == 256 ? 8 : SI_RB == 512 ? 9 : 10;
static_assert(SI_RB == (1u << SI_RB_LOG2) && SI_RB % 64 == 0, "a row block is a power of two of whole 64-row windows");

constexpr size_t scansi_lds_bytes(uint32_t cap) { return scansi_lds_bytes_rb(cap, SI_RB); }

// a call is planned on K1si when its per-query table (sp_slots: a power of two >= 2 x the call's longest query) holds at most
// SI_MAX_TERMS non-zeros and the workgroup fits a CU at the call's cap
constexpr bool scansi_fits(uint32_t sp_slots, uint32_t cap)
{
    return sp_slots >= 2 && sp_slots <= 2 * SI_MAX_TERMS && scansi_lds_bytes(cap) <= SI_LDS_MAX;
}

// ---- the inverted image (vsr_sparse_inverted.hip) ----
// 8 bytes per stored entry (postings: row in block, value), 12 per (row block, distinct index) and per row block (bterm: 4,
// boff: 8, one end sentinel of boff and one begin of the block's run), 16 per row (A2, A1 in double); 4 more close the begins
constexpr size_t sparse_inverted_bytes(uint64_t entries, uint64_t block_terms, uint64_t rows)
{
    const uint64_t blocks = (rows + SI_RB - 1) / SI_RB;
    return (size_t) (entries * 8 + block_terms * 12 + blocks * 12 + 4 + rows * 16);
}
// the build's sort key: (row block, index, row in block); an index is below 2^30 (SPARSE_MAX_DIM = 10^9)
constexpr int SI_KEY_INDEX_BITS = 30;

}  // namespace vsr
