"""csrc/vsr_scansm_sizing.h compiled alone with the host C++ compiler: the LDS of a K1sm pass's query block and the QW it allows.
Expected from the formula's description: 8 cap (sort buffer), 8 bytes x QW x sp_slots (union table), 2 QW^2 sp_slots (Qd), 16 per
wave, 28 per query, 32 for the flags; budget 80 KB."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vectorsearch-rbac_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include "vsr_scansm_sizing.h"
int main()
{
    unsigned qw, slots, cap;
    int max_qw;
    while (scanf("%u %u %u %d", &qw, &slots, &cap, &max_qw) == 4)
        printf("%zu %d\n", vsr::scansm_lds_bytes((int) qw, slots, cap), vsr::scansm_qw(slots, cap, max_qw));
    return 0;
}
"""
lds = lambda qw, slots, cap: 8 * cap + 8 * qw * slots + 2 * qw * qw * slots + 4 * 16 + 28 * qw + 32


@pytest.fixture(scope="module")
def sizing(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("scansm")
    (d / "s.cpp").write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "s.cpp"), "-o", str(d / "s")])
    run = lambda *a: subprocess.run([str(d / "s")], input=" ".join(map(str, a)) + "\n", capture_output=True, text=True, check=True).stdout
    return lambda *a: tuple(int(v) for v in run(*a).split())


# cap = 2048 at k = 100 (mfma_cap_for_k); slots = the power of two >= 2 x the longest query
@pytest.mark.parametrize("slots,cap,max_qw,want", [
    (16, 2048, 32, 32),      # <= 8 non-zeros: 32 queries per pass (54 240 bytes)
    (32, 2048, 32, 16),      # 9 .. 16: Qd alone would be 64 KB at QW = 32
    (64, 2048, 32, 16),      # <= 32 non-zeros, the README's shape: 57 888 bytes at QW = 16, 164 832 at 32
    (128, 2048, 32, 0),      # 33 and more: K1s
    (16, 2048, 16, 16),      # VSR_MAX_QB caps QW
    (16, 2048, 8, 0),
    (16, 8192, 32, 16),      # k = 2048: a 64 KB sort buffer leaves room for QW = 16 only
])
def test_qw_thresholds(sizing, slots, cap, max_qw, want):
    for qw in (16, 32):
        assert sizing(qw, slots, cap, max_qw)[0] == lds(qw, slots, cap)
    assert sizing(16, slots, cap, max_qw)[1] == want
    assert (lds(16, 64, 2048), lds(32, 16, 2048), lds(32, 64, 2048)) == (57888, 54240, 164832)
