// vsr_bounds.h — relative error bounds of the screening tiers: |dot_s - dot| <= g(d) |x| |q|.
//
// Plain C++ (no HIP): the re-rank's flag test (vsr_kernels.hip, rerank_body) relies on these constants, and the CPU
// suite compiles this header on its own to check them (tests/test_screening_bounds_cpu.py).
//
// bf16 keeps 8 significand bits, so round-to-nearest moves a value by at most half a bf16 ulp: for x in the binade
// [2^E, 2^(E+1)), |x - bf16(x)| <= 2^(E-8) <= u |x| with u = 2^-8.  A product of two bf16 values is exact in fp32; the
// MFMA chains add the products in fp32, (m + c) 2^-24 relative to the sum of |products| for m products (c: slack for
// the padding and the K-step order), and that sum is at most (1 + 2^-5) |x||q| for every split below (Cauchy-Schwarz).
//
// The constant terms hold while the bf16 parts are normal numbers or exact: |x| >= 2^-126 (coarse), |x| >= 2^-117 (planes,
// whose mid part must round with an error below 2^-17 |x|).  Smaller elements have absolute, not relative, errors.
#pragma once

// K2g, coarse planes: dot_s = sum xh qh, xh = x (1 + a), qh = q (1 + b), |a|, |b| <= u:
//   |xh qh - x q| = |x q| |a + b + a b| <= (2u + u^2) |x q| = 2^-7 (1 + 2^-9) |x q|
// (worst case: x = q just below 1 + 2^-8, both rounded down to 1: 1.99 2^-8 relative).
inline float coarse_err_g(int dim)
{
    return 7.8277588e-3f + (float) (dim + 64) * 5.9604645e-8f * 1.03125f;              // 2^-7 (1 + 2^-9) + (d + 64) 2^-24 (1 + 2^-5)
}

// K2w, hi + mid planes: x = xh + xm + ex with xh = bf16(x), xm = bf16(x - xh) (x - xh is exact in fp32), so
//   |xm| <= 2^-8 |x|,  |ex| <= half a bf16 ulp of x - xh <= 2^-17 |x|.
// The screen drops xm qm and the residues:  x q - (xh qh + xh qm + xm qh) = xm qm + (xh + xm) eq + ex (qh + qm) + ex eq,
//   <= (2^-16 + 2 * 2^-17 (1 + 2^-17) + 2^-34) |x q| <= 2^-15 (1 + 2^-17) |x q|
// (worst case measured over a whole binade: 7.95 2^-18).  3 d products per dot product.
inline float plane_err_g(int dim)
{
    return 3.0517811e-5f + (float) (3 * dim + 8) * 5.9604645e-8f * 1.03125f;           // 2^-15 (1 + 2^-17) + (3d + 8) 2^-24 (1 + 2^-5)
}

// K2, fp32 MFMA on the fp32 rows: every product rounded once (2^-24 relative), d of them accumulated in fp32
inline float k2_err_g(int dim) { return (float) (dim + 8) * 5.9604645e-8f; }          // (d + 8) 2^-24

// K2h, f16 MFMA on the binary16 rows of a halfvec corpus and the binary16-rounded query: nothing is rounded on the way in,
// and a product of two halves (11 x 11 significand bits, exponents within +-32) is exact in fp32.  What remains is the
// fp32 accumulation of the d products, in an order the hardware chooses.  Any order of n - 1 rounded additions is within
// gamma = (n - 1) u / (1 - (n - 1) u) of the sum of |products|, u = 2^-24, and that sum is at most |x||q| (Cauchy-Schwarz).
// The slack: up to VECTOR_MAX_DIM = 16000 the second-order part of gamma is (n - 1)^2 u^2 <= 15.3 u, and the zero padding
// adds exactly.  ASSUMPTION, as for the bf16 MFMA chains above: the f16 MFMA adds its products with no more than one
// fp32 rounding (to nearest) per product; the instruction's internal order and rounding are not documented, and
// tests/test_gpu_halfvec_mfma.py checks the bound on the device.  Subnormal halves count like any other value: their
// products are exact too (the same test checks that the hardware keeps them).
inline float half_err_g(int dim) { return (float) (dim + 16) * 5.9604645e-8f; }       // (d + 16) 2^-24
