// vsr_exact.h — arithmetic that more than one kernel must perform identically, each piece written once:
//   * the operator arithmetic of vector.c on fp32 rows as the exact re-rank runs it (half a wave per row, several rows in
//     flight): K5r's rerank_body (vsr_kernels.hip) and K3's iterative batch scan (vsr_ivf_iter.h);
//   * GetScanLists' centre distance (ivfscan.c:36-107): ivf_probe_kernel and ivf_iterative_kernel, so that the list order of
//     an iterative scan can never drift away from the lists vsr_ivf_probe reports.
#pragma once
#include "vsr_topk.h"

#include <type_traits>

namespace vsr {

__device__ __forceinline__ float output_distance(int metric, float v)
{
    // L2 ranks by the fp32 sum; the operator value is sqrt((double) sum), vector.c:577
    return metric == M_L2 ? (float) sqrt((double) v) : v;
}

// |q|^2 of a zero-padded query of stride4 float4, by one whole wave (every lane gets the sum)
__device__ __forceinline__ float wave_query_norm2(const float4* q, uint32_t stride4, int lane)
{
    float qn_part = 0.0f;
    for (uint32_t c = lane; c < stride4; c += 64) {
        const float4 v = q[c];
        qn_part = fmaf(v.x, v.x, qn_part); qn_part = fmaf(v.y, v.y, qn_part);
        qn_part = fmaf(v.z, v.z, qn_part); qn_part = fmaf(v.w, v.w, qn_part);
    }
    for (int m = 32; m >= 1; m >>= 1) qn_part += __shfl_xor(qn_part, m);
    return qn_part;
}

// Half a wave per row (32 lanes x float4 = 128 floats per step), U rows per half-wave in flight: lane hl of the half adds
// the terms of chunks hl, hl + 32, ... of rows row[0 .. U) against the query, then the half-wave is summed, so every lane of
// the half ends with s[u] = sum (a - b)^2 (L2) or sum a b (IP, cosine) and nx[u] = sum a^2 (cosine only).  Callers pass a
// valid row (0) for an empty slot and drop its sums: there is no branch around the gather, the U loads of a half-wave are
// all in flight before the first FMA waits.
// HALF: `rows` is a halfvec corpus -- stride4 / 2 16-byte chunks of 8 halves per row -- and a lane's step is one such chunk,
// widened in registers and added element by element against the query's two float4 with the fmaf sequence K1h runs
// (vsr_scan.h): on data whose sums do not depend on the order, the re-rank and K1h give the same bits.
template <int U, bool HALF = false>
__device__ __forceinline__ void halfwave_row_sums(const float4* rows, uint32_t stride4, const float4* q, int metric,
                                                  const uint32_t (&row)[U], int hl, float (&s)[U], float (&nx)[U])
{
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = nx[u] = 0.f;
    if constexpr (HALF) {
        const uint32_t nchunk = stride4 / 2;
        const u32x4* rows16 = reinterpret_cast<const u32x4*>(rows);
        auto add4 = [&](float& su, float& nu, float a0, float a1, float a2, float a3, const float4& b) {
            if (metric == M_L2) {
                const float d0 = a0 - b.x, d1 = a1 - b.y, d2 = a2 - b.z, d3 = a3 - b.w;
                su = fmaf(d0, d0, su); su = fmaf(d1, d1, su); su = fmaf(d2, d2, su); su = fmaf(d3, d3, su);
            } else {
                su = fmaf(a0, b.x, su); su = fmaf(a1, b.y, su); su = fmaf(a2, b.z, su); su = fmaf(a3, b.w, su);
                if (metric == M_COSINE) {
                    nu = fmaf(a0, a0, nu); nu = fmaf(a1, a1, nu); nu = fmaf(a2, a2, nu); nu = fmaf(a3, a3, nu);
                }
            }
        };
        for (uint32_t ch = hl; ch < nchunk; ch += 32) {
            const float4 b0 = q[2 * ch], b1 = q[2 * ch + 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const f16x8 a = __builtin_bit_cast(f16x8, rows16[(size_t) row[u] * nchunk + ch]);
                add4(s[u], nx[u], (float) a[0], (float) a[1], (float) a[2], (float) a[3], b0);
                add4(s[u], nx[u], (float) a[4], (float) a[5], (float) a[6], (float) a[7], b1);
            }
        }
    } else {
        for (uint32_t ch = hl; ch < stride4; ch += 32) {
            const float4 b = q[ch];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(rows + (size_t) row[u] * stride4 + ch);
                const float4 a = make_float4(av[0], av[1], av[2], av[3]);
                if (metric == M_L2) {
                    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
                    s[u] = fmaf(d0, d0, s[u]); s[u] = fmaf(d1, d1, s[u]); s[u] = fmaf(d2, d2, s[u]); s[u] = fmaf(d3, d3, s[u]);
                } else {
                    s[u] = fmaf(a.x, b.x, s[u]); s[u] = fmaf(a.y, b.y, s[u]); s[u] = fmaf(a.z, b.z, s[u]); s[u] = fmaf(a.w, b.w, s[u]);
                    if (metric == M_COSINE) {
                        nx[u] = fmaf(a.x, a.x, nx[u]); nx[u] = fmaf(a.y, a.y, nx[u]);
                        nx[u] = fmaf(a.z, a.z, nx[u]); nx[u] = fmaf(a.w, a.w, nx[u]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        for (int m = 16; m >= 1; m >>= 1) {                                // within the half-wave
            s[u] += __shfl_xor(s[u], m);
            nx[u] += __shfl_xor(nx[u], m);
        }
}

// the ranking value of a row from its sums: the fp32 sum (L2), the negative inner product, or the cosine distance with
// float8 post-processing (vector.c:646-668)
__device__ __forceinline__ float exact_rank_value(int metric, float s, float nx, float qn)
{
    if (metric == M_L2) return s;
    if (metric == M_IP) return -s;
    double sim = (double) s / sqrt((double) nx * (double) qn);
    if (sim > 1.0) sim = 1.0; else if (sim < -1.0) sim = -1.0;
    return (float) (1.0 - sim);
}

// 32-bit monotone image of the opclass distance between a query and centre c (L2 squared, or negative inner product).
// centers_t[j][c]: the centres TRANSPOSED (element j of all lists contiguous), so that the 64 lanes of a wave -- one centre
// each -- read 256 contiguous bytes per element instead of 64 lines 4 * dim bytes apart; every lane adds its own centre's
// terms in element order, in the order and rounding of vector.c's loops compiled without contraction.
//
// FORM says what the two sides hold (K3h: the halfvec opclasses, halfutils.c:27-40, 79-90 on the widened values):
//   IVF_F32      fp32 centres, fp32 query: the vector opclasses;
//   IVF_HALF_Q32 binary16 centres (a wave's element step is 128 contiguous bytes), an fp32 query whose every element is rounded
//                to binary16 (Float4ToHalf, nearest even) as it is loaded and widened again: `$1::halfvec` (probe, iterative scan);
//   IVF_HALF_ROW binary16 centres, the query is a binary16 row read in place (the build's assignment over a halfvec corpus).
// The two half forms run the same fp32 sequence on the same widened values: a (query, centre) pair has one key.
//   IVF_BIT      K3b, bit_hamming_ops (ivfutils.c:364-377: FUNCTION 1 is hamming_distance): the centres are packed bit strings,
//                transposed by 32-bit word -- centers_t[w][c], `dim` counts WORDS here -- so a wave's word step is again 256
//                contiguous bytes; the query side is packed words with the pad bits clear (a staged query, the query in LDS of
//                the iterative scan, or a corpus row in place: rows are zero padded to whole 16-byte chunks >= the words).  The
//                key is the popcount sum itself: monotone already, at most 64000, never the `taken` mark.  `metric` is not read.
enum { IVF_F32 = 0, IVF_HALF_Q32 = 1, IVF_HALF_ROW = 2, IVF_BIT = 3 };

template <int FORM>
__device__ __forceinline__ float ivf_query_element(const void* q, int j)
{
    if constexpr (FORM == IVF_F32) return static_cast<const float*>(q)[j];
    else if constexpr (FORM == IVF_HALF_Q32) return (float) (_Float16) static_cast<const float*>(q)[j];
    else return (float) static_cast<const _Float16*>(q)[j];
}

template <int FORM = IVF_F32>
__device__ __forceinline__ uint32_t ivf_center_key(const void* centers_t, int lists, int dim, int c, const void* q, int metric)
{
    if constexpr (FORM == IVF_BIT) {
        const uint32_t* x = static_cast<const uint32_t*>(centers_t) + c;
        const uint32_t* qw = static_cast<const uint32_t*>(q);
        uint32_t count = 0;
        for (int w = 0; w < dim; ++w) count += (uint32_t) __popc(x[(size_t) w * lists] ^ qw[w]);
        return count;
    }
    using CT = typename std::conditional<FORM == IVF_F32, float, _Float16>::type;
    const CT* x = static_cast<const CT*>(centers_t) + c;
    float sum = 0.0f;
    if (metric == M_L2) {
        for (int j = 0; j < dim; ++j) {
            const float d = __fsub_rn((float) x[(size_t) j * lists], ivf_query_element<FORM>(q, j));
            sum = __fadd_rn(sum, __fmul_rn(d, d));
        }
    } else {
        for (int j = 0; j < dim; ++j) sum = __fadd_rn(sum, __fmul_rn((float) x[(size_t) j * lists], ivf_query_element<FORM>(q, j)));
        sum = -sum;
    }
    return mono_bits(sum);
}

// The nearest centre not yet taken among keys[0 .. lists) (0xFFFFFFFF = taken: above the canonical NaN's image), equal
// distances to the lower list id, by a 256-thread workgroup; the winner is marked taken.  Returns (key << 32 | list) in
// every thread, KEY_EMPTY when none is left.  s_best: 4 LDS words of scratch.  Two workgroup barriers.
__device__ __forceinline__ uint64_t ivf_extract_nearest(uint32_t* keys, int lists, uint64_t* s_best, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint64_t best = KEY_EMPTY;
    for (int c = tid; c < lists; c += 256) {
        const uint32_t kc = keys[c];
        const uint64_t cand = kc == 0xFFFFFFFFu ? KEY_EMPTY : (((uint64_t) kc << 32) | (uint32_t) c);
        best = cand < best ? cand : best;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) best, m), hi = (uint32_t) __shfl_xor((int) (uint32_t) (best >> 32), m);
        const uint64_t o = ((uint64_t) hi << 32) | lo;
        best = o < best ? o : best;
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    uint64_t b = s_best[0];
    for (int w = 1; w < 4; ++w) b = s_best[w] < b ? s_best[w] : b;
    if (tid == 0 && b != KEY_EMPTY) keys[(uint32_t) b] = 0xFFFFFFFFu;
    __syncthreads();
    return b;
}

}  // namespace vsr
