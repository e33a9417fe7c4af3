// vsr_bit.hip — the small kernels of bit corpora (pgvector's type bit, bitvec.c / bitutils.c): query staging, row popcounts,
// binary_quantize and the pair functions.  The scan itself is K1b (vsr_scanb.h).
// Layout everywhere: PostgreSQL's varbit order, element i = bit 7 - i % 8 of byte i / 8.  Popcount, xor and and are
// indifferent to the order, so only binary_quantize has to know it; bits past `dim` never count: they are cleared on the way
// in (staging, corpus load) or masked (pair functions).
#include "vsr_device.h"

namespace vsr {

// the valid bits of byte j of a dim-bit string
__device__ __forceinline__ uint32_t bit_byte_mask(uint32_t j, uint32_t dim)
{
    const uint32_t first = j * 8u;
    if (first >= dim) return 0u;
    const uint32_t live = dim - first;
    return live >= 8u ? 0xFFu : (0xFF00u >> live) & 0xFFu;
}

// Per-batch staging of a bit search, see StageParams (q_bits).  Workgroups [0, nq): one query each, byte by byte (device
// queries need no alignment); the rest copy the descriptor block.
__global__ __launch_bounds__(256) void stage_bit_kernel(const StageParams p)
{
    __shared__ uint32_t s_pop[4];
    const int tid = threadIdx.x;
    if (blockIdx.x >= p.nq) {
        const uint32_t nb = gridDim.x - p.nq;
        for (uint32_t i = (blockIdx.x - p.nq) * 256 + (uint32_t) tid; i < p.n16; i += nb * 256) p.dst16[i] = p.src16[i];
        return;
    }
    const uint32_t s = blockIdx.x;
    const uint32_t slot_bytes = p.qfloats * 4u;              // a whole number of 16-byte chunks
    const uint32_t src_bytes = (p.dim + 7u) / 8u;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(p.q_src) + (size_t) s * p.q_stride;
    uint8_t* dst = reinterpret_cast<uint8_t*>(p.q_dst) + (size_t) s * slot_bytes;
    uint32_t pop = 0;
    for (uint32_t j = (uint32_t) tid; j < slot_bytes; j += 256) {
        const uint32_t v = j < src_bytes ? (uint32_t) src[j] & bit_byte_mask(j, p.dim) : 0u;
        dst[j] = (uint8_t) v;
        pop += (uint32_t) __popc(v);
    }
    for (int m = 32; m >= 1; m >>= 1) pop += (uint32_t) __shfl_xor((int) pop, m);
    if ((tid & 63) == 0) s_pop[tid >> 6] = pop;
    __syncthreads();
    if (tid == 0) {
        p.q_norm2[s] = (float) (s_pop[0] + s_pop[1] + s_pop[2] + s_pop[3]);
        p.flags[s] = 0;
        p.tau[s] = KEY_EMPTY;
    }
}

hipError_t launch_stage_bit(const StageParams& p, hipStream_t s)
{
    const uint32_t copy_blocks = p.n16 ? (p.n16 + 1023) / 1024 < 64 ? (p.n16 + 1023) / 1024 : 64 : 0;
    if (p.nq + copy_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_bit_kernel, dim3(p.nq + copy_blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// one thread per output byte
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t* src, uint32_t src_stride, uint32_t n, uint32_t dim, uint8_t* dst,
                                                        uint32_t dst_bytes)
{
    const uint32_t src_bytes = (dim + 7u) / 8u;
    const uint64_t total = (uint64_t) n * dst_bytes;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t) gridDim.x * 256) {
        const uint32_t s = (uint32_t) (i / dst_bytes), j = (uint32_t) (i % dst_bytes);
        dst[i] = j < src_bytes ? (uint8_t) ((uint32_t) src[(size_t) s * src_stride + j] & bit_byte_mask(j, dim)) : (uint8_t) 0;
    }
}

hipError_t launch_pack_bits(const uint8_t* src, uint32_t src_stride, uint32_t n, uint32_t dim, uint8_t* dst, uint32_t dst_bytes,
                            hipStream_t s)
{
    const uint64_t total = (uint64_t) n * dst_bytes;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_bits_kernel, dim3((uint32_t) std::min<uint64_t>((total + 255) / 256, 16384)), dim3(256), 0, s, src, src_stride, n,
                       dim, dst, dst_bytes);
    return hipGetLastError();
}

// one wave per row
__global__ __launch_bounds__(256) void row_popcounts_kernel(const uint4* rows, uint32_t n_rows, uint32_t chunks, float* pop)
{
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;                               // wave-uniform
    const uint4* r = rows + (size_t) row * chunks;
    uint32_t acc = 0;
    for (uint32_t c = (uint32_t) lane; c < chunks; c += 64) {
        const uint4 x = r[c];
        acc += (uint32_t) (__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w));
    }
    for (int m = 32; m >= 1; m >>= 1) acc += (uint32_t) __shfl_xor((int) acc, m);
    if (lane == 0) pop[row] = (float) acc;
}

hipError_t launch_row_popcounts(const uint4* rows, uint32_t n_rows, uint32_t chunks, float* pop, hipStream_t s)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(row_popcounts_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, s, rows, n_rows, chunks, pop);
    return hipGetLastError();
}

// one thread per output byte: 8 elements -> 1 byte.  NaN, -0.0 and 0 give 0 (vector.c:953-964: `ax[i] > 0`); a widened half
// is positive exactly when the half is (halfvec.c binary_quantize: HalfToFloat4(ax[i]) > 0)
template <class T>
__global__ __launch_bounds__(256) void binary_quantize_kernel(const T* src, uint64_t n_rows, uint32_t dim, uint32_t src_stride,
                                                              uint8_t* dst, uint32_t dst_bytes)
{
    const uint64_t total = n_rows * dst_bytes;
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t) gridDim.x * 256) {
        const uint64_t row = i / dst_bytes;
        const uint32_t j = (uint32_t) (i - row * dst_bytes);
        const T* x = src + row * src_stride;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const uint32_t e = j * 8u + b;
            if (e < dim && (float) x[e] > 0.0f) v |= 0x80u >> b;
        }
        dst[i] = (uint8_t) v;
    }
}

hipError_t launch_binary_quantize(const void* src, int src_half, uint64_t n_rows, uint32_t dim, uint32_t src_stride, uint8_t* dst,
                                  uint32_t dst_bytes, hipStream_t s)
{
    const uint64_t total = n_rows * dst_bytes;
    if (total == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t) ((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (src_half)
        hipLaunchKernelGGL(binary_quantize_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, static_cast<const _Float16*>(src), n_rows,
                           dim, src_stride, dst, dst_bytes);
    else
        hipLaunchKernelGGL(binary_quantize_kernel<float>, dim3(blocks), dim3(256), 0, s, static_cast<const float*>(src), n_rows, dim,
                           src_stride, dst, dst_bytes);
    return hipGetLastError();
}

// One wave per pair, byte by byte; the operator's float8 (bitvec.c:46-77, bitutils.c:34-61, 96-129).  metric: 4 Hamming, 5 Jaccard
__global__ __launch_bounds__(256) void bit_pair_distance_kernel(const uint8_t* a, const uint8_t* b, int64_t n_pairs, int dim,
                                                                int b_broadcast, int metric, double* out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t) blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t) gridDim.x * 256) >> 6;
    const uint32_t bytes = ((uint32_t) dim + 7u) / 8u;
    for (int64_t i = wave; i < n_pairs; i += n_waves) {
        const uint8_t* x = a + i * bytes;
        const uint8_t* y = b_broadcast ? b : b + i * bytes;
        uint32_t dx = 0, ab = 0, aa = 0, bb = 0;
        for (uint32_t j = (uint32_t) lane; j < bytes; j += 64) {
            const uint32_t m = bit_byte_mask(j, (uint32_t) dim);
            const uint32_t u = x[j] & m, v = y[j] & m;
            dx += (uint32_t) __popc(u ^ v);
            ab += (uint32_t) __popc(u & v);
            aa += (uint32_t) __popc(u);
            bb += (uint32_t) __popc(v);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            dx += (uint32_t) __shfl_xor((int) dx, m);
            ab += (uint32_t) __shfl_xor((int) ab, m);
            aa += (uint32_t) __shfl_xor((int) aa, m);
            bb += (uint32_t) __shfl_xor((int) bb, m);
        }
        if (lane == 0) out[i] = metric == 4 ? (double) dx : ab == 0 ? 1.0 : 1.0 - (double) ab / (double) (aa + bb - ab);
    }
}

hipError_t launch_bit_pair_distances(const uint8_t* a, const uint8_t* b, int64_t n_pairs, int dim, int b_broadcast, int metric,
                                     double* out, hipStream_t s)
{
    if (n_pairs == 0) return hipSuccess;
    int64_t blocks = (n_pairs + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(bit_pair_distance_kernel, dim3((uint32_t) blocks), dim3(256), 0, s, a, b, n_pairs, dim, b_broadcast, metric, out);
    return hipGetLastError();
}

}  // namespace vsr
