// vsr_sparse.hip — the small kernels of sparse corpora (pgvector's type sparsevec, sparsevec.c): query staging, the pair
// functions, and the capacity rules the planner takes for K1s.  The scan itself is K1s (vsr_scans.h).
#include "vsr_device.h"

namespace vsr {

// Per-batch staging of a sparse search, see SparseStageParams.  Workgroups [0, ceil(nq / 4)): one WAVE per query; the rest copy
// the descriptor block.  A query's wave clears its table, then inserts its entries: slot = hash(index), linear probing, the index
// word claimed by atomic compare-and-swap (a repeated index -- device queries are not validated -- lands in the slot it already
// owns), the value stored behind it.  The table is read by later launches only.
__global__ __launch_bounds__(256) void stage_sparse_kernel(const SparseStageParams p)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const uint32_t q_blocks = (p.nq + 3) / 4;
    if (blockIdx.x >= q_blocks) {
        const uint32_t nb = gridDim.x - q_blocks;
        for (uint32_t i = (blockIdx.x - q_blocks) * 256 + (uint32_t) tid; i < p.n16; i += nb * 256) p.dst16[i] = p.src16[i];
        return;
    }
    const uint32_t s = blockIdx.x * 4 + (uint32_t) (tid >> 6);
    if (s >= p.nq) return;                                   // wave-uniform
    uint2* tab = p.tab + (size_t) s * p.slots;
    for (uint32_t i = (uint32_t) lane; i < p.slots; i += 64) tab[i] = make_uint2(SPARSE_EMPTY, 0u);
    __threadfence();                                         // the cleared slots are in memory before any compare-and-swap on them
    __builtin_amdgcn_wave_barrier();

    const int64_t beg = p.indptr[s], end = p.indptr[s + 1];
    const bool bad = beg < 0 || end < beg || end - beg > (int64_t) p.max_nnz;           // not staged: an empty query, and the guard word says so
    const uint32_t nnz = bad ? 0u : (uint32_t) (end - beg);
    bool dropped = false;
    double q2 = 0.0, q1 = 0.0;
    float q2f = 0.0f;
    const uint32_t mask = p.slots - 1u;
    for (uint32_t e = (uint32_t) lane; e < nnz; e += 64) {
        const uint32_t idx = (uint32_t) p.indices[beg + e];
        const float v = p.values[beg + e];
        if (idx >= p.dim) { dropped = true; continue; }      // (also keeps SPARSE_EMPTY out of the table)
        uint32_t h = (idx * SPARSE_HASH_MUL) >> p.shift;
        for (;;) {
            const uint32_t prev = atomicCAS(&tab[h].x, SPARSE_EMPTY, idx);
            if (prev == SPARSE_EMPTY || prev == idx) break;
            h = (h + 1u) & mask;
        }
        tab[h].y = __float_as_uint(v);
        q2 += (double) v * (double) v;
        q1 += fabs((double) v);
        q2f = fmaf(v, v, q2f);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        q2 += __shfl_xor(q2, m);
        q1 += __shfl_xor(q1, m);
        q2f += __shfl_xor(q2f, m);
    }
    if (__ballot(bad || dropped) && lane == 0) atomicOr(p.err, SPARSE_ERR_QUERY);
    if (lane == 0) {
        p.qtot[2 * (size_t) s] = q2;
        p.qtot[2 * (size_t) s + 1] = q1;
        p.q_norm2[s] = q2f;
        p.flags[s] = 0;
        p.tau[s] = KEY_EMPTY;
    }
}

hipError_t launch_stage_sparse(const SparseStageParams& p, hipStream_t s)
{
    const uint32_t copy_blocks = p.n16 ? (p.n16 + 1023) / 1024 < 64 ? (p.n16 + 1023) / 1024 : 64 : 0;
    const uint32_t q_blocks = (p.nq + 3) / 4;
    if (q_blocks + copy_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_sparse_kernel, dim3(q_blocks + copy_blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// One thread per pair: sparsevec.c's loops as they stand -- SparsevecL2SquaredDistance (:803-846), SparsevecInnerProduct
// (:882-913), sparsevec_cosine_distance (:948-988), sparsevec_l1_distance (:993-1037) -- every product and sum rounded to fp32
// on its own (fp contraction is off in this kernel: pgvector's build has no fused multiply-add), then the operator's float8.
__global__ __launch_bounds__(256) void sparse_pair_distance_kernel(const int64_t* a_ptr, const int32_t* a_idx, const float* a_val,
                                                                   const int64_t* b_ptr, const int32_t* b_idx, const float* b_val,
                                                                   int64_t n_pairs, int metric, double* out)
{
#pragma clang fp contract(off)                               // every product and sum below is rounded on its own
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (int64_t) gridDim.x * 256) {
        const int32_t* ai_ = a_idx + a_ptr[i];
        const float* ax = a_val + a_ptr[i];
        const int annz = (int) (a_ptr[i + 1] - a_ptr[i]);
        const int32_t* bi_ = b_idx + b_ptr[i];
        const float* bx = b_val + b_ptr[i];
        const int bnnz = (int) (b_ptr[i + 1] - b_ptr[i]);
        float distance = 0.0f;
        int bpos = 0;
        if (metric == M_L2 || metric == M_L1) {
            const bool l1 = metric == M_L1;
            for (int x = 0; x < annz; ++x) {
                const int ai = ai_[x];
                int bi = -1;
                for (int j = bpos; j < bnnz; ++j) {
                    bi = bi_[j];
                    if (ai == bi) {
                        const float diff = ax[x] - bx[j];
                        distance = distance + (l1 ? fabsf(diff) : (diff * diff));
                    } else if (ai > bi)
                        distance = distance + (l1 ? fabsf(bx[j]) : (bx[j] * bx[j]));
                    if (ai >= bi) bpos = j + 1;
                    if (bi >= ai) break;
                }
                if (ai != bi) distance = distance + (l1 ? fabsf(ax[x]) : (ax[x] * ax[x]));
            }
            for (int j = bpos; j < bnnz; ++j) distance = distance + (l1 ? fabsf(bx[j]) : (bx[j] * bx[j]));
            out[i] = l1 ? (double) distance : sqrt((double) distance);
            continue;
        }
        for (int x = 0; x < annz; ++x) {
            const int ai = ai_[x];
            for (int j = bpos; j < bnnz; ++j) {
                const int bi = bi_[j];
                if (ai == bi) distance = distance + ax[x] * bx[j];
                if (ai >= bi) bpos = j + 1;
                if (bi >= ai) break;
            }
        }
        if (metric == M_IP) {
            out[i] = (double) -distance;
            continue;
        }
        float norma = 0.0f, normb = 0.0f;
        for (int x = 0; x < annz; ++x) norma = norma + ax[x] * ax[x];
        for (int j = 0; j < bnnz; ++j) normb = normb + bx[j] * bx[j];
        double similarity = (double) distance / sqrt((double) norma * (double) normb);
        if (similarity > 1.0) similarity = 1.0;
        else if (similarity < -1.0) similarity = -1.0;
        out[i] = 1.0 - similarity;
    }
}

hipError_t launch_sparse_pair_distances(const int64_t* a_ptr, const int32_t* a_idx, const float* a_val, const int64_t* b_ptr,
                                        const int32_t* b_idx, const float* b_val, int64_t n_pairs, int metric, double* out,
                                        hipStream_t s)
{
    if (n_pairs == 0) return hipSuccess;
    int64_t blocks = (n_pairs + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sparse_pair_distance_kernel, dim3((uint32_t) blocks), dim3(256), 0, s, a_ptr, a_idx, a_val, b_ptr, b_idx, b_val,
                       n_pairs, metric, out);
    return hipGetLastError();
}

// Support functions of the cosine opclass, batched, one thread per vector with sparsevec.c's loops as they stand: sparsevec_l2_norm
// (:1044-1055: a double sum of double products in entry order, then sqrt) and sparsevec_l2_normalize (:1060-1120: (float) (v / norm)
// with the norm in double; a zero norm leaves the values as they are; an infinite result is reported; entries that became 0 are
// counted -- the caller drops them).  out_values == nullptr: norms only.
__global__ __launch_bounds__(256) void sparse_norm_kernel(const int64_t* ptr, const float* val, int64_t n, double* out_norm, float* out_values,
                                                          int* overflow, unsigned long long* zeros)
{
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t beg = ptr[i], end = ptr[i + 1];
        double norm = 0.0;
        for (int64_t e = beg; e < end; ++e) norm += (double) val[e] * (double) val[e];
        norm = sqrt(norm);
        if (out_norm) out_norm[i] = norm;
        if (!out_values) continue;
        unsigned long long z = 0;
        bool inf = false;
        for (int64_t e = beg; e < end; ++e) {
            float r = val[e];
            if (norm > 0) {
                r = (float) ((double) val[e] / norm);
                inf |= isinf(r);
                z += r == 0.0f ? 1ull : 0ull;
            }
            out_values[e] = r;
        }
        if (inf) atomicOr(overflow, 1);
        if (z) atomicAdd(zeros, z);
    }
}

hipError_t launch_sparse_norms(const int64_t* ptr, const float* val, int64_t n, double* out_norm, float* out_values, int* overflow,
                               unsigned long long* zeros, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sparse_norm_kernel, dim3((uint32_t) blocks), dim3(256), 0, s, ptr, val, n, out_norm, out_values, overflow, zeros);
    return hipGetLastError();
}

// ---- K1s capacity rules (host) ----
// A lane group of LPR lanes takes 2 LPR entries of a row per step (16-byte loads): 4 lanes up to a dozen stored entries per row
// on average, 16 up to about a hundred, a whole wave beyond.
int sparse_lpr_for_mean_nnz(double mean_nnz) { return mean_nnz <= 12.0 ? 4 : mean_nnz <= 96.0 ? 16 : 64; }

bool scan_sparse_table_in_lds(uint32_t slots, int k)
{
    return scans_lds_bytes(1, scan_cap_for_rw(k, 64), slots) <= SCAN_LDS_BUDGET;
}

int scan_qmax_sparse(uint32_t slots, int k)
{
    const bool lds = scan_sparse_table_in_lds(slots, k);
    const size_t per_query = scans_lds_bytes(1, scan_cap_for_rw(k, 64), lds ? slots : 0u) - 16;
    const int q = (int) ((SCAN_LDS_BUDGET - 16) / per_query);
    if (q < 4) return 1;
    if (!lds) return 4;                                      // global tables: one sub-batch (qmax = QI)
    return (q < SCAN_QMAX ? q : SCAN_QMAX) / 4 * 4;
}

}  // namespace vsr
