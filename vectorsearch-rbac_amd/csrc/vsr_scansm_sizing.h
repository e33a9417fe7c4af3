// vsr_scansm_sizing.h — what the planner and the launcher of K1sm (vsr_scansm.h) decide without a GPU: the sizes of the pass's
// query block and the LDS they need.  Plain C++ (no HIP header), so that a host compiler can build it alone; the two sizes the
// kernel carves its LDS by are constexpr, which makes them callable from device code too.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vsr {

constexpr int    SM_THREADS = 256;                       // 4 waves per workgroup
constexpr int    SM_WAVES = SM_THREADS / 64;
constexpr size_t SCANSM_LDS_BUDGET = 80 * 1024;          // per workgroup: two fit a CU's 160 KiB (K2b's budget)

// slots of the union table over the distinct indices of a pass's qw queries: the power of two >= 2 x qw x (sp_slots / 2), so
// its load factor stays <= 1/2 whatever the queries share (sp_slots: the call's per-query table, a power of two >= 2 x nnz)
constexpr uint32_t scansm_union_slots(int qw, uint32_t sp_slots)
{
    uint32_t u = 2;
    while (u < (uint32_t) qw * sp_slots) u <<= 1;
    return u;
}
// most columns of the dense block: every query with sp_slots / 2 indices of its own
constexpr uint32_t scansm_max_columns(int qw, uint32_t sp_slots) { return (uint32_t) qw * (sp_slots / 2); }

// LDS of one workgroup: the sort buffer of a compaction (cap keys), the union table (8 bytes a slot), Qd[columns][qw] fp32
// (2 x qw^2 x sp_slots bytes), 16 bytes of scratch per wave (the prologue's prefix count), and per query the control words
// (TopKCtrl), the double total and |q|^2; the vote flags
inline size_t scansm_lds_bytes(int qw, uint32_t sp_slots, uint32_t cap)
{
    return (size_t) cap * 8 + (size_t) scansm_union_slots(qw, sp_slots) * 8 + (size_t) scansm_max_columns(qw, sp_slots) * qw * 4 +
           (size_t) SM_WAVES * 16 + (size_t) qw * (16 + 8 + 4) + 32;
}

// queries per pass (QW): 32 if the block fits the budget, else 16, else 0 (the call stays on K1s); max_qw: the caller's ceiling
inline int scansm_qw(uint32_t sp_slots, uint32_t cap, int max_qw)
{
    if (max_qw >= 32 && scansm_lds_bytes(32, sp_slots, cap) <= SCANSM_LDS_BUDGET) return 32;
    if (max_qw >= 16 && scansm_lds_bytes(16, sp_slots, cap) <= SCANSM_LDS_BUDGET) return 16;
    return 0;
}

// K1sc (vsr_scansc.h): the same pass over a compact block.  LDS of one workgroup: the sort buffer, the union table, one record
// (mask, base: 8 bytes) per column, one fp32 per (query, non-zero) -- at most scansm_max_columns of either --, and the small
// terms of scansm_lds_bytes.  Grows as qw x sp_slots where the dense block grows as qw^2 x sp_slots
inline size_t scansc_lds_bytes(int qw, uint32_t sp_slots, uint32_t cap)
{
    return (size_t) cap * 8 + (size_t) scansm_union_slots(qw, sp_slots) * 8 + (size_t) scansm_max_columns(qw, sp_slots) * (8 + 4) +
           (size_t) SM_WAVES * 16 + (size_t) qw * (16 + 8 + 4) + 32;
}

// queries per pass of K1sc: 32 if the compact block fits the budget, else 16, else 0 (the call is planned without K1sc)
inline int scansc_qw(uint32_t sp_slots, uint32_t cap, int max_qw)
{
    if (max_qw >= 32 && scansc_lds_bytes(32, sp_slots, cap) <= SCANSM_LDS_BUDGET) return 32;
    if (max_qw >= 16 && scansc_lds_bytes(16, sp_slots, cap) <= SCANSM_LDS_BUDGET) return 16;
    return 0;
}

}  // namespace vsr
