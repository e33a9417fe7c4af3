"""csrc/vsr_scansm_sizing.h compiled alone with the host C++ compiler: the LDS of a K1sc pass's compact query block and the QW it
allows.  Expected from the formula's description: 8 cap (sort buffer), 8 bytes x QW x sp_slots (union table), 8 + 4 bytes x QW x
sp_slots / 2 (column records, packed values), 16 per wave, 28 per query, 32 for the flags; budget 80 KB.  K1sm's own functions
must answer what they answered before the header grew; DESIGN's three byte counts are at cap = 2048 (k = 100)."""
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
        printf("%zu %d %zu %d\n", vsr::scansc_lds_bytes((int) qw, slots, cap), vsr::scansc_qw(slots, cap, max_qw),
               vsr::scansm_lds_bytes((int) qw, slots, cap), vsr::scansm_qw(slots, cap, max_qw));
    return 0;
}
"""
small = lambda qw, cap: 8 * cap + 4 * 16 + 28 * qw + 32
compact = lambda qw, slots, cap: small(qw, cap) + 8 * qw * slots + 12 * qw * slots // 2
dense = lambda qw, slots, cap: small(qw, cap) + 8 * qw * slots + 2 * qw * qw * slots


@pytest.fixture(scope="module")
def sizing(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("scansc")
    (d / "s.cpp").write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "s.cpp"), "-o", str(d / "s")])
    run = lambda *a: subprocess.run([str(d / "s")], input=" ".join(map(str, a)) + "\n", capture_output=True, text=True, check=True).stdout
    return lambda *a: tuple(int(v) for v in run(*a).split())


# slots = the power of two >= 2 x the longest query; (K1sc's QW, K1sm's QW as before this header grew)
@pytest.mark.parametrize("slots,cap,max_qw,want,want_dense", [
    (16, 2048, 32, 32, 32),
    (32, 2048, 32, 32, 16),
    (64, 2048, 32, 32, 16),
    (128, 2048, 32, 32, 0),    # <= 64 non-zeros
    (256, 2048, 32, 16, 0),    # <= 128
    (512, 2048, 32, 0, 0),     # the union table alone is 64 KB
    (128, 2048, 16, 16, 0),    # VSR_MAX_QB caps QW
    (128, 2048, 8, 0, 0),
    (128, 8192, 32, 0, 0),     # k = 2048: a 64 KB sort buffer
    (16, 8192, 32, 32, 16),
])
def test_qw_thresholds(sizing, slots, cap, max_qw, want, want_dense):
    for qw in (16, 32):
        got = sizing(qw, slots, cap, max_qw)
        assert got[0] == compact(qw, slots, cap) and got[2] == dense(qw, slots, cap)
        assert got[2] > 80 * 1024 or got[0] <= got[2]            # never larger than the dense block where that one fits
    assert sizing(16, slots, cap, max_qw)[1::2] == (want, want_dense)
    assert (compact(32, 128, 2048), compact(16, 256, 2048), compact(32, 64, 2048), dense(32, 64, 2048)) == (74720, 74272, 46048, 164832)
