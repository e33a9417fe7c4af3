"""csrc/vsr_scansi_sizing.h compiled alone with the host C++ compiler: K1si's row block, LDS and routing rule, and the image's
byte count.  Expected from the header's description: 8 cap (sort buffer), per wave 8 SI_RB (accumulators) + 8 x 256 (sorted
terms), 16 x 16 control words, 16 for the flags; SI_RB the largest power of two that fits 80 KB at cap = 2048."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vectorsearch-rbac_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include "vsr_scansi_sizing.h"
int main()
{
    unsigned slots, cap;
    unsigned long long e, t, n;
    printf("%u %d %d %u\n", vsr::SI_RB, vsr::SI_WAVES, vsr::SI_QMAX, vsr::SI_MAX_TERMS);
    while (scanf("%u %u %llu %llu %llu", &slots, &cap, &e, &t, &n) == 5)
        printf("%zu %d %zu\n", vsr::scansi_lds_bytes(cap), (int) vsr::scansi_fits(slots, cap), vsr::sparse_inverted_bytes(e, t, n));
    return 0;
}
"""
lds = lambda cap, rb: 8 * cap + 8 * (8 * rb + 8 * 256) + 16 * 16 + 16


@pytest.mark.parametrize("slots,cap,fits", [(2, 2048, 1), (512, 2048, 1), (1024, 2048, 0), (512, 8192, 1), (1, 2048, 0)])
def test_sizes(tmp_path, slots, cap, fits):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    (tmp_path / "s.cpp").write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(tmp_path / "s.cpp"), "-o", str(tmp_path / "s")])
    out = subprocess.run([str(tmp_path / "s")], input=f"{slots} {cap} 1000 300 1061\n", capture_output=True, text=True, check=True).stdout.split()
    rb, waves, qmax, terms = (int(v) for v in out[:4])
    assert (rb, waves, qmax, terms) == (512, 8, 16, 256)
    assert lds(2048, rb) <= 80 * 1024 < lds(2048, 2 * rb)        # the derivation of SI_RB
    assert [int(v) for v in out[4:]] == [lds(cap, rb), fits, 8 * 1000 + 12 * 300 + 12 * 3 + 4 + 16 * 1061]
