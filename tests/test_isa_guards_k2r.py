"""Build-time guards on K2r (vsr_i8r.h), the register-fed int8 sample pass (no GPU needed: hipcc cross-compiles to assembly).

The kernel exists to fit beside four resident workgroups of the int8 main launch: at most 96 VGPRs (a fifth wave per SIMD),
no scratch, at most 16 KB of LDS.  Its unit loop keeps three 16-row units of loads in flight per wave; the compiler counts the
waits for them itself, and one `s_waitcnt vmcnt(0)` inside the loop would drain the queue at every unit without changing a
result.  Neither a register count nor a wait shows in any test of results, so both are pinned here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MANGLED = "_ZN3vsr20i8_sample_reg_kernelILi4EEEvNS_10ScanParamsE"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("k2r")
    src = d / "tu.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "vsr_i8r.h"\n'
                   "namespace vsr { template __global__ void i8_sample_reg_kernel<4>(const ScanParams); }\n")
    out = d / "tu.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", str(src), "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text().splitlines()


def _meta(lines, key):
    """The kernel's entry of that name in the code object's metadata (entries start at `  - .agpr_count`)."""
    at = next(i for i, l in enumerate(lines) if l.split() == [".name:", MANGLED])
    starts = [i for i, l in enumerate(lines) if l.startswith("  - .")]
    lo = max(i for i in starts if i < at)
    hi = min([i for i in starts if i > at] + [len(lines)])
    vals = [l.split(":")[1].strip() for l in lines[lo:hi] if l[4:].startswith(key + ":")]
    assert len(vals) == 1, (key, vals)
    return int(vals[0])


def test_k2r_fits_beside_four_main_workgroups(asm):
    assert _meta(asm, ".vgpr_count") + _meta(asm, ".agpr_count") <= 96
    assert _meta(asm, ".vgpr_spill_count") == 0 and _meta(asm, ".sgpr_spill_count") == 0
    assert _meta(asm, ".private_segment_fixed_size") == 0
    assert _meta(asm, ".group_segment_fixed_size") <= 16 * 1024


def test_k2r_unit_loop_has_only_counted_waits(asm):
    start = next(i for i, l in enumerate(asm) if l.startswith(MANGLED + ":"))
    end = next(i for i in range(start, len(asm)) if "s_endpgm" in asm[i])
    k = asm[start:end + 1]
    mfma = [i for i, l in enumerate(k) if "v_mfma_i32_16x16x64_i8" in l]
    assert len(mfma) == 32, len(mfma)                                      # 4 units x 4 groups x 2 K-blocks per trip
    head = max(i for i, l in enumerate(k) if "Loop Header" in l and "Depth=1" in l and i < mfma[0])
    label = k[head].split(":")[0]
    tail = max(i for i, l in enumerate(k) if "Header=" + label.lstrip(".L") in l)          # the last block of the loop
    body = k[head:tail]
    loads = [l for l in body if "global_load_dwordx4" in l]
    assert len(loads) == 12, len(loads)                                  # 4 units x (2 A fragments + |row|^2)
    assert not any(re.search(r"\b(ds_write|ds_store|s_barrier|buffer_|flat_|scratch_)", l) for l in body)
    waits = [l.strip() for l in body if "s_waitcnt" in l and "vmcnt" in l]
    assert waits, "the counted waits are gone"
    # a unit is used with the three units behind it in flight: 9 loads, or 8 where the wait sits before the third of a unit
    assert all(re.fullmatch(r"s_waitcnt vmcnt\((8|9)\)", w) for w in waits), waits
