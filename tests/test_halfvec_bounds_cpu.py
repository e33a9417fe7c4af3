"""half_err_g (csrc/vsr_bounds.h), the bound of K2h's screening dot product, against a numpy model.

K2h multiplies binary16 rows with binary16-rounded queries on the f16 matrix cores: the products are exact in fp32 and
only their fp32 accumulation rounds, in an order the hardware chooses.  The model forms the exact products of random
binary16 values (float64 holds them exactly) and adds them in fp32 in several orders -- one chain, a pairwise tree, blocks
of 32 (a K-step of the 16x16x32 MFMA) that are then chained -- and the worst |dot_s - dot| / (|x||q|) must stay below g.
The bound must also stay within twice K2's, so that it cannot be made vacuous.  The header is compiled on its own with the
host C++ compiler, so these are the constants the kernels use."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

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
        printf("%d %.9g %.9g\n", d, (double) half_err_g(d), (double) k2_err_g(d));
    }
    return 0;
}
"""

DIMS = [64, 128, 768, 4096]


@pytest.fixture(scope="module")
def g_of(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("half_bounds")
    src, exe = d / "g.cpp", d / "g"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)] + [str(x) for x in DIMS + [1, 8, 61, 16000]], text=True)
    table = {}
    for line in out.split("\n"):
        if line.strip():
            f = line.split()
            table[int(f[0])] = (float(f[1]), float(f[2]))
    return table


def _sequential(p):
    """p: [cases, d] float32 products; one fp32 chain per case."""
    s = np.zeros(p.shape[0], np.float32)
    for j in range(p.shape[1]):
        s = (s + p[:, j]).astype(np.float32)
    return s


def _pairwise(p):
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
        p = (p[:, 0::2] + p[:, 1::2]).astype(np.float32)
    return p[:, 0]


def _blocks_of_32(p):
    """Each block of 32 products summed by a tree, the block sums chained onto the accumulator."""
    s = np.zeros(p.shape[0], np.float32)
    for b in range(0, p.shape[1], 32):
        s = (s + _pairwise(p[:, b:b + 32])).astype(np.float32)
    return s


def _operands(rng, kind, cases, d):
    if kind == "normal":
        x, q = rng.normal(size=(cases, d)), rng.normal(size=(cases, d))
    elif kind == "positive":                                 # no cancellation in the exact sum: the rounding errors add up
        x, q = rng.random((cases, d)) + 0.5, rng.random((cases, d)) + 0.5
    else:                                                    # magnitudes over the whole binary16 range, subnormals included
        x = rng.normal(size=(cases, d)) * np.exp2(rng.integers(-24, 13, (cases, d)))
        q = rng.normal(size=(cases, d)) * np.exp2(rng.integers(-24, 13, (cases, d)))
    return x.astype(np.float16), q.astype(np.float16)


@pytest.mark.parametrize("d", DIMS)
def test_half_err_g_covers_fp32_accumulation_in_any_order(g_of, d):
    g = g_of[d][0]
    rng = np.random.default_rng(d)
    cases = 48 if d <= 768 else 12
    worst = 0.0
    for kind in ("normal", "positive", "wide"):
        x, q = _operands(rng, kind, cases, d)
        x64, q64 = x.astype(np.float64), q.astype(np.float64)
        prod = x64 * q64                                     # exact: 11 x 11 significand bits
        p32 = prod.astype(np.float32)
        assert (p32.astype(np.float64) == prod).all(), "a product of two halves must be exact in fp32"
        dot = np.array([math.fsum(prod[i]) for i in range(cases)])   # correctly rounded
        scale = np.sqrt((x64 ** 2).sum(1) * (q64 ** 2).sum(1))
        for order in (_sequential, _pairwise, _blocks_of_32):
            err = np.abs(order(p32).astype(np.float64) - dot) / scale
            worst = max(worst, float(err.max()))
    print(f"d = {d}: worst |dot_s - dot| / (|x||q|) = {worst:.3e}, g = {g:.3e}")
    assert 0.0 < worst < g, (d, worst, g)


@pytest.mark.parametrize("d", DIMS + [1, 8, 61, 16000])
def test_half_err_g_is_not_vacuous(g_of, d):
    g, k2 = g_of[d]
    assert g > 0 and g <= 2 * k2, (d, g, k2)
    assert g >= d * 2.0 ** -24                               # one rounding per product, at least
