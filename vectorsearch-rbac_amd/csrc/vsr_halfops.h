// vsr_halfops.h — the distance stage of the graph kernels over a halfvec corpus, shared by K4h (vsr_hnsw.h, ROWS_HALF) and the
// half build (vsr_hnsw_build.hip): one definition of the lane mapping and of the arithmetic, so that a build distance and a
// search distance of the same pair are the same fp32 bit pattern.
//   pgvector/src/halfutils.c:27-40 HalfvecL2SquaredDistanceDefault, :79-90 HalfvecInnerProductDefault: both operands widened
//   to fp32, fp32 sums (here fmaf; on integer-valued data every order of summation gives the same value).
#pragma once
#include "vsr_device.h"
#include "vsr_scan.h"
#include "vsr_bitops.h"

namespace vsr {

// the index distance the graph ranks by: squared L2, the L1 sum (sparsevec_l1_ops), or the negative inner product (cosine opclass:
// unit rows)
__device__ __forceinline__ float hnsw_rank_value(int metric, float s) { return metric == M_L2 || metric == M_L1 ? s : -s; }

// 8 floats (elements past `dim` zero) starting at element 8 * ch of a query -> one chunk of binary16 values: Float4ToHalf,
// round to nearest even, which is what `$1::halfvec` holds
__device__ __forceinline__ uint4 half_query_chunk(const float* q, uint32_t dim, uint32_t ch)
{
    f16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t e = 8u * ch + (uint32_t) i;
        v[i] = (_Float16) (e < dim ? q[e] : 0.0f);
    }
    return __builtin_bit_cast(uint4, v);
}

// Distances of one halfvec to `cnt` others, for the graph kernels: ids[c] names an element, elem_row (may be nullptr: element e
// is row e) the row holding its values, a row is C 16-byte chunks of 8 binary16 values (elements past dim zero).  G lanes share
// a row (G: the smallest power of two >= C, at most 64: bit_graph_lanes), so 64 / G rows are gathered per wave step and U steps
// are in flight; every lane loads whole chunks of its own row only, a lane whose chunk index is >= C loads nothing, an id
// past cnt is never dereferenced.  The query side is binary16 too: `qreg` is the lane's chunk (lane % G) when C <= 64 (zero for
// a lane past the row's end), else the G = 64 lanes loop over the chunks and re-read `qs` (the wave's LDS in the search, the
// row itself in the build).  fp32 partials, a shuffle butterfly inside the lane group (none at G = 1), hnsw_rank_value at the
// end.  out[c] is written by the group's first lane; the caller synchronises the wave.
template <bool L2>
__device__ __forceinline__ void half_graph_distances(const uint4* rows, uint32_t C, uint32_t G, const int32_t* elem_row,
                                                     const uint4* qs, const uint4& qreg, const int32_t* ids, int cnt, float* out,
                                                     int lane)
{
    constexpr int U = 4;
    constexpr int METRIC = L2 ? M_L2 : M_IP;
    const uint32_t per = 64u / G, gl = (uint32_t) lane & (G - 1u), grp = (uint32_t) lane / G;
    for (int c0 = 0; c0 < cnt; c0 += U * (int) per) {
        float acc[U];
        int64_t row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * (int) per + (int) grp;
            acc[u] = 0.0f;
            row[u] = -1;
            if (c < cnt) row[u] = elem_row ? (int64_t) elem_row[ids[c]] : (int64_t) ids[c];
        }
        if (C <= 64u) {
            uint4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = make_uint4(0u, 0u, 0u, 0u);
                if (row[u] >= 0 && gl < C) x[u] = rows[(size_t) row[u] * C + gl];
            }
            float4 qa, qb;
            widen8(qreg, qa, qb);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float4 xa, xb;
                widen8(x[u], xa, xb);
                accum4<METRIC>(acc[u], xa, qa);
                accum4<METRIC>(acc[u], xb, qb);
            }
        } else {
            for (uint32_t ch = gl; ch < C; ch += 64u) {
                float4 qa, qb;
                widen8(qs[ch], qa, qb);
                uint4 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    x[u] = make_uint4(0u, 0u, 0u, 0u);
                    if (row[u] >= 0) x[u] = rows[(size_t) row[u] * C + ch];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float4 xa, xb;
                    widen8(x[u], xa, xb);
                    accum4<METRIC>(acc[u], xa, qa);
                    accum4<METRIC>(acc[u], xb, qb);
                }
            }
        }
        for (uint32_t mm = G >> 1; mm >= 1u; mm >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] += __shfl_xor(acc[u], (int) mm);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * (int) per + (int) grp;
            if (gl == 0u && c < cnt) out[c] = hnsw_rank_value(METRIC, acc[u]);
        }
    }
}

}  // namespace vsr
