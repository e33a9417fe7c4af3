"""The ABI and Python surface of vsr_hnsw_vacuum_spill_info, what a vacuum reports about the repairs it ran in the global-memory
form (tests/test_gpu_hnsw_vacuum_spill.py has the behaviour).  Nothing here needs a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_ffi_agree_on_spill_info():
    from vsrbac import _ffi
    text = open(os.path.join(ROOT, "include", "vsrbac.h")).read()
    decl = re.search(r"\bint vsr_hnsw_vacuum_spill_info\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, args = _ffi.SYMBOLS["vsr_hnsw_vacuum_spill_info"]
    assert len(params) == len(args) == 3 and restype is ctypes.c_int
    assert [p.split()[-1].lstrip("*") for p in params] == ["index", "spilled_repairs", "workspace_bytes"]
    assert params[1].startswith("int32_t*") and params[2].startswith("int64_t*")
    assert args[0] is ctypes.c_void_p and args[1] is ctypes.POINTER(ctypes.c_int32) and args[2] is ctypes.POINTER(ctypes.c_int64)
    assert "#define VSR_ABI_VERSION 2" in text


def test_stats_struct_is_unchanged():
    from vsrbac import _ffi
    assert ctypes.sizeof(_ffi.HnswVacuumStats) == 32
    assert [f for f, _ in _ffi.HnswVacuumStats._fields_] == ["tuples_removed", "tuples_kept", "elements_removed", "elements_repaired",
                                                            "batches", "attempts"]


def test_python_surface():
    import inspect
    from vsrbac.engine import HnswIndex
    assert list(inspect.signature(HnswIndex.vacuum_spill_info).parameters) == ["self"]
    doc = " ".join(HnswIndex.vacuum_spill_info.__doc__.split())
    for word in ("spilled_repairs", "workspace_bytes", "vsr_hnsw_vacuum_spill_info", "(0, 0)"):
        assert word in doc, word
