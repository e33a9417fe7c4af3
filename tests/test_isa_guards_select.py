"""Build-time guards on the one-wave-per-query selections of int8 (exact_screen) plans, seed_select_wave_kernel and
select_emit_wave_kernel (vsr_kernels.hip).  No GPU needed: hipcc cross-compiles to assembly and only the kernels' metadata
is read.

Both kernels exist to be resident beside four workgroups of the int8 main launch, which leave a SIMD 96 VGPRs and one wave
slot and a CU 32 KB of LDS: 64-thread workgroups, at most 96 VGPRs + AGPRs, nothing spilled, and the static LDS plus the
largest dynamic LDS their launchers can ask for within 9 KB (seed: m < SEED_MAX_M kept keys and the histogram) and 5.5 KB
(final selection: np2(GQ_MAX_KP) keys and the histogram).  None of this shows in any test of results."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = "seed_select_wave_kernel"
EMIT = "select_emit_wave_kernel"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("selw") / "vsr_kernels.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", os.path.join(CSRC, "vsr_kernels.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    return out.read_text().splitlines()


def _meta(lines, kernel, key):
    """The entry of the kernel whose mangled name holds `kernel` in the code object's metadata (entries start at `  - .`)."""
    at = [i for i, l in enumerate(lines) if l.split()[:1] == [".name:"] and l.split()[1].startswith("_ZN3vsr") and kernel in l]
    assert len(at) == 1, (kernel, at)
    starts = [i for i, l in enumerate(lines) if l.startswith("  - .")]
    lo = max(i for i in starts if i < at[0])
    hi = min([i for i in starts if i > at[0]] + [len(lines)])
    vals = [l.split(":")[1].strip() for l in lines[lo:hi] if l[4:].startswith(key + ":")]
    assert len(vals) == 1, (kernel, key, vals)
    return int(vals[0])


def _constant(name):
    """`constexpr uint32_t NAME = value;` of vsr_device.h: what the launchers size their dynamic LDS from."""
    with open(os.path.join(CSRC, "vsr_device.h")) as f:
        m = re.search(r"constexpr uint32_t " + name + r" = (\d+);", f.read())
    assert m, name
    return int(m.group(1))


def _np2(v):
    n = 2
    while n < v:
        n <<= 1
    return n


# the launcher's largest dynamic LDS: seed_wave_lds_bytes(SEED_MAX_M - 1), select_emit_wave_lds_bytes(GQ_MAX_KP)
LARGEST_DYNAMIC = {SEED: lambda: 8 * (_constant("SEED_MAX_M") - 1), EMIT: lambda: 8 * _np2(_constant("GQ_MAX_KP"))}
LDS_BUDGET = {SEED: 9 * 1024, EMIT: 5 * 1024 + 512}


@pytest.mark.parametrize("kernel", [SEED, EMIT])
def test_wave_selection_fits_beside_four_main_workgroups(asm, kernel):
    assert _meta(asm, kernel, ".vgpr_count") + _meta(asm, kernel, ".agpr_count") <= 96
    assert _meta(asm, kernel, ".vgpr_spill_count") == 0 and _meta(asm, kernel, ".sgpr_spill_count") == 0
    assert _meta(asm, kernel, ".private_segment_fixed_size") == 0
    assert _meta(asm, kernel, ".max_flat_workgroup_size") == 64
    assert _meta(asm, kernel, ".group_segment_fixed_size") + LARGEST_DYNAMIC[kernel]() <= LDS_BUDGET[kernel]

