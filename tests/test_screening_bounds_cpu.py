"""The screening error bounds of csrc/vsr_bounds.h against a CPU model of the bf16 splits (tests/screening_model.py).

(a) per element: over every fp32 significand of a binade, the worst relative error of each tier's product stays within
    the constant term of its g(d) -- in [1, 2), in the lowest binade the header claims (mid parts subnormal) and at a
    large exponent;
(b) per dot product: for every tier x metric x d in the tier's range, the flag test's err covers the worst screening
    value error (constant term + fp32 accumulation + forming the value).
The header is compiled on its own with the host C++ compiler, so these are the constants the kernels use."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import screening_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "vsr_bounds.h"
int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        const int d = atoi(argv[i]);
        printf("%d %.9g %.9g %.9g\n", d, (double) coarse_err_g(d), (double) plane_err_g(d), (double) k2_err_g(d));
    }
    return 0;
}
"""

DIMS = {"coarse": [193, 256, 384, 512, 768, 1000, 1024],        # K2g: coarse planes exist for d > 192 (<= 1024)
        "planes": [61, 64, 100, 128, 192, 256, 512, 768, 1024],  # K2w: d = 61 .. 1024
        "k2": [61, 128, 768, 1536, 4100]}                       # K2: d >= 61


@pytest.fixture(scope="module")
def g_of(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("bounds")
    src, exe = d / "g.cpp", d / "g"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)])
    dims = sorted({x for v in DIMS.values() for x in v} | {1})
    out = subprocess.check_output([str(exe)] + [str(x) for x in dims], text=True)
    table = {}
    for line in out.split("\n"):
        if line.strip():
            f = line.split()
            table[int(f[0])] = {"coarse": float(f[1]), "planes": float(f[2]), "k2": float(f[3])}
    return lambda tier, dim: table[dim][tier]


def _binade(e):
    """Every fp32 of [2^e, 2^(e+1))."""
    bits = (np.uint32(e + 127) << np.uint32(23)) | np.arange(1 << 23, dtype=np.uint32)
    return bits.view(np.float32)


def _worst(tier, e):
    """Worst relative error of one element's screened product over every pair (x, q) of the binade, from per-element
    extremes (so it bounds all 2^46 pairs), and the worst on the diagonal x = q (a pair that reaches it)."""
    x = _binade(e)
    x64 = x.astype(np.float64)
    hi, mid = sm.split(x)
    if tier == "coarse":
        a = (hi.astype(np.float64) - x64) / x64                          # xh = x (1 + a)
        amax = np.abs(a).max()
        bound = 2 * amax + amax * amax
        diag = np.abs((1 + a) ** 2 - 1).max()
    else:
        r = mid.astype(np.float64) / x64                                 # xm / x
        b = (x64 - hi.astype(np.float64) - mid.astype(np.float64)) / x64  # ex / x
        rmax, bmax = np.abs(r).max(), np.abs(b).max()
        bound = rmax * rmax + 2 * bmax * (1 + bmax) + bmax * bmax
        diag = np.abs(r * r + 2 * b * (1 - b) + b * b).max()
    return bound, diag


CONST = {"coarse": lambda g, d: g - (d + 64) * 2.0 ** -24 * 1.03125,
         "planes": lambda g, d: g - (3 * d + 8) * 2.0 ** -24 * 1.03125}


@pytest.mark.parametrize("tier", ["coarse", "planes"])
@pytest.mark.parametrize("e", [0, -117, 100])
def test_constant_term_covers_every_element_of_a_binade(g_of, tier, e):
    bound, diag = _worst(tier, e)
    assert diag <= bound
    d = 64
    const = CONST[tier](g_of(tier, d), d)
    assert bound <= const, (tier, e, bound / 2.0 ** -18, const / 2.0 ** -18)
    if e == 0:
        # the worst case is reached: x = q just below 1 + 2^-8 (coarse, 1.99 2^-8), x = q = 1.0039136 (planes, 7.83 2^-18)
        assert diag > (1.98 * 2.0 ** -8 if tier == "coarse" else 7.8 * 2.0 ** -18)


def test_bf16_rounding_matches_round_to_nearest_even():
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, 259.0, 1.0039061, 1.0039064, -257.0, 2.0 ** -130],
                 np.float32)
    want = np.array([1.0, 1.0 + 2 * 2.0 ** -7, 256.0, 260.0, 1.0, 1.0 + 2.0 ** -7, -256.0, 2.0 ** -130], np.float32)
    np.testing.assert_array_equal(sm.bf16(v), want)
    hi, mid = sm.split(np.array([257.0, 1.0039136], np.float32))
    assert hi[0] == 256 and mid[0] == 1 and hi[1] == 1.0078125 and mid[1] < 0


def _value_error(tier, metric, d, nxm, qn, elem):
    """Worst |screening value - exact value| over rows with |x|^2 <= nxm: elem (per-element constant) + fp32
    accumulation of the products (m of them, |products| summing to at most (1 + 2^-5) |x||q|) + a few ulp of forming
    the value (fma / rsqrt on fp32 operands)."""
    m = {"coarse": d, "planes": 3 * d, "k2": d}[tier]
    per_elem = elem + (2.0 ** -24 if tier == "k2" else 0.0)              # K2 rounds every fp32 product once
    g_true = per_elem + m * 2.0 ** -24 * 1.03125
    xq = np.sqrt(nxm * qn)
    if metric == "l2":
        return 2 * g_true * xq + 4 * 2.0 ** -24 * (nxm + qn + 2 * xq)
    if metric == "ip":
        return g_true * xq + 2 * 2.0 ** -24 * xq
    return g_true + 4 * 2.0 ** -24


@pytest.mark.parametrize("tier", sm.TIERS)
@pytest.mark.parametrize("metric", sm.METRICS)
def test_flag_err_covers_the_screening_error(g_of, tier, metric):
    elem = {"coarse": _worst("coarse", 0)[0], "planes": _worst("planes", 0)[0], "k2": 0.0}[tier]
    for d in DIMS[tier]:
        g = g_of(tier, d)
        for nxm, qn in ((1.0, 1.0), (100.0, 1.0), (1.0, 100.0), (3e4, 2e4)):
            need = _value_error(tier, metric, d, nxm, qn, elem)
            err = sm.flag_err(tier, metric, g, nxm, qn, a_last=0.0)
            assert err >= need, (tier, metric, d, nxm, qn, err, need)


def test_old_coarse_constant_is_defeated():
    """The derivation with 2^-9 per operand (the constant before this test) misses the coarse worst case by ~2x."""
    d = 768
    need = _value_error("coarse", "l2", d, 1.0, 1.0, _worst("coarse", 0)[0])
    assert sm.flag_err("coarse", "l2", sm.old_g("coarse", d), 1.0, 1.0) < need
