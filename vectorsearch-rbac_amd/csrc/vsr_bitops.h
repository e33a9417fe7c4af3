// vsr_bitops.h — the arithmetic of pgvector's bit distances, shared by K1b (vsr_scanb.h), K4b (vsr_hnsw.h) and the bit build
// (vsr_hnsw_build.hip): one definition of the popcount accumulation and of the operator's value, so that an index distance
// and a scan distance of the same pair are the same fp32 bit pattern.
//   pgvector/src/bitutils.c:34-61 BitHammingDistanceDefault, :96-129 BitJaccardDistanceDefault.
#pragma once
#include "vsr_device.h"

namespace vsr {

enum MetricBit : int { M_HAMMING = 4, M_JACCARD = 5 };
// row format of the corpus under an HNSW graph: a template parameter of the search body (vsr_hnsw.h) and of the build kernels
// (vsr_hnsw_build.hip).  Everything but the distance stage and the reported distance is shared between the two
// (ROWS_HALF: a halfvec corpus, vsr_halfops.h)
enum HnswRows : int { ROWS_F32 = 0, ROWS_BIT = 1, ROWS_HALF = 2, ROWS_SPARSE = 3 };

template <bool JACCARD>
__device__ __forceinline__ void accum_bits(uint32_t& p, const uint4& x, const uint4& q)
{
    if constexpr (JACCARD) {
        p += (uint32_t) __popc(x.x & q.x); p += (uint32_t) __popc(x.y & q.y);
        p += (uint32_t) __popc(x.z & q.z); p += (uint32_t) __popc(x.w & q.w);
    } else {
        p += (uint32_t) __popc(x.x ^ q.x); p += (uint32_t) __popc(x.y ^ q.y);
        p += (uint32_t) __popc(x.z ^ q.z); p += (uint32_t) __popc(x.w ^ q.w);
    }
}

// (float) of the operator's float8.  Hamming: the count.  Jaccard (bitutils.c:125-128): ab == 0 ? 1 : 1 - ab / (double) (aa + bb - ab)
template <bool JACCARD>
__device__ __forceinline__ float rank_value_bits(uint32_t p, float row_pop, float q_pop)
{
    if constexpr (JACCARD) {
        if (p == 0) return 1.0f;
        const double uni = (double) row_pop + (double) q_pop - (double) p;      // integers < 2^17: exact
        return (float) (1.0 - (double) p / uni);
    } else {
        return (float) p;
    }
}

// Distances of one bit string to `cnt` others, for the graph kernels: ids[c] names an element, elem_row (may be nullptr:
// element e is row e) the row holding its bits, a row is stride4 16-byte chunks.  G lanes share a row (G: the smallest power
// of two >= stride4, at most 64), so 64 / G rows are gathered per wave step and U steps are in flight; every lane loads whole
// uint4 chunks of its own row only.  The query side: `qreg` is the lane's chunk (lane % G) when stride4 <= 64 (zero for a lane
// past the row's end), else the G = 64 lanes loop over the chunks and re-read `qs`.  Integer partials, a shuffle butterfly
// inside the lane group (none at G = 1), one conversion at the end (rank_value_bits).  out[c] is written by the group's first
// lane; the caller synchronises the wave.
template <bool JACCARD>
__device__ __forceinline__ void bit_graph_distances(const uint4* rows, uint32_t stride4, uint32_t G, const int32_t* elem_row,
                                                    const float* row_pop, const uint4* qs, const uint4& qreg, float q_pop,
                                                    const int32_t* ids, int cnt, float* out, int lane)
{
    constexpr int U = 4;
    const uint32_t per = 64u / G, gl = (uint32_t) lane & (G - 1u), grp = (uint32_t) lane / G;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int c0 = 0; c0 < cnt; c0 += U * (int) per) {
        uint32_t acc[U];
        int64_t row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * (int) per + (int) grp;
            acc[u] = 0u;
            row[u] = -1;
            if (c < cnt) row[u] = elem_row ? (int64_t) elem_row[ids[c]] : (int64_t) ids[c];
        }
        if (stride4 <= 64u) {
            uint4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = (row[u] >= 0 && gl < stride4) ? rows[(size_t) row[u] * stride4 + gl] : zero;
#pragma unroll
            for (int u = 0; u < U; ++u) accum_bits<JACCARD>(acc[u], x[u], qreg);
        } else {
            for (uint32_t ch = gl; ch < stride4; ch += 64u) {
                const uint4 qv = qs[ch];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint4 x = row[u] >= 0 ? rows[(size_t) row[u] * stride4 + ch] : zero;
                    accum_bits<JACCARD>(acc[u], x, qv);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            for (uint32_t mm = G >> 1; mm >= 1u; mm >>= 1) acc[u] += (uint32_t) __shfl_xor((int) acc[u], (int) mm);
            const int c = c0 + u * (int) per + (int) grp;
            if (gl == 0u && c < cnt) out[c] = rank_value_bits<JACCARD>(acc[u], JACCARD ? row_pop[row[u]] : 0.0f, q_pop);
        }
    }
}

// lanes per row of bit_graph_distances
inline __host__ __device__ uint32_t bit_graph_lanes(uint32_t stride4)
{
    uint32_t g = 1;
    while (g < stride4 && g < 64u) g <<= 1;
    return g;
}

}  // namespace vsr
