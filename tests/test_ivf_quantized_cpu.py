"""The two-stage search through the bit IVFFlat index (vsr_ivf_search_quantized*, K3q) without a GPU: the symbols, the Python
surface, the model's two identities and K3q's LDS formula (csrc/vsr_ivf_lds.h, compiled alone with the host C++ compiler)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bit_model
from ivf_quantized_model import IvfQuantizedModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")

NAMES = {"vsr_ivf_search_quantized": 18, "vsr_ivf_search_quantized_device": 19}


def test_symbols_declared_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    text = open(os.path.join(ROOT, "include", "vsrbac.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(vsrbac.library_path())                 # the built library; never touches the GPU
    for name, n_args in NAMES.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/vsrbac.h"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(lib, name), name
        assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == n_args
    assert vsrbac.abi_version() == 2


def test_corpus_methods_exist():
    import inspect
    from vsrbac.engine import Corpus
    sig = inspect.signature(Corpus.search_quantized_ivf)
    assert list(sig.parameters)[1:] == ["bit_index", "queries", "k", "shortlist", "probes", "metric", "filters", "mode", "max_probes"]
    assert sig.parameters["probes"].default == 1 and sig.parameters["mode"].default == "off"
    assert sig.parameters["max_probes"].default == 32768 and sig.parameters["metric"].default == "l2"
    assert hasattr(Corpus, "search_quantized_ivf_device")


@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(11)
    n, dim, lists = 600, 40, 6
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    blk = rng.permutation(n).astype(np.int64) + 1
    doc = rng.integers(1, 31, n).astype(np.int32)
    centers = bit_model.pack(rng.random((lists, dim)) < 0.5)
    row_list = rng.integers(0, lists - 1, n).astype(np.int32)          # the last list stays empty
    q = rng.integers(-8, 9, (7, dim)).astype(np.float32)
    return IvfQuantizedModel(oracle, x, centers, row_list, doc, blk), q


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_model_with_every_list_probed_is_the_scanned_two_stage_search(small, metric):
    model, q = small
    for k, shortlist in ((10, 10), (5, 100), (50, 600)):
        want = model.qm.search(metric, q, k, shortlist)
        for mode, probes in (("off", model.lists), ("off", 50), ("relaxed_order", model.lists)):
            for i in range(len(q)):
                idx, dist, S, scanned = model.search(metric, q[i], k, shortlist, probes, mode, 1)
                np.testing.assert_array_equal(S, want[i][2])
                np.testing.assert_array_equal(idx, want[i][0])
                np.testing.assert_array_equal(dist, want[i][1])
                assert scanned == model.lists


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_model_with_a_mask_that_fits_the_shortlist_is_the_exact_search(small, metric):
    model, q = small
    rng = np.random.default_rng(12)
    mask = np.zeros(len(model.doc), dtype=np.uint8)
    mask[rng.choice(mask.size, 90, replace=False)] = 1
    for k in (10, 90, 120):
        for shortlist in (max(k, 90), 200):
            for i in range(len(q)):
                idx, dist, S, scanned = model.search(metric, q[i], k, shortlist, 1, "relaxed_order", model.lists, mask)
                assert scanned == model.lists and set(S.tolist()) == set(np.flatnonzero(mask).tolist())
                want_idx, want_dist = model.qm.exact(metric, q[i], k, mask)
                np.testing.assert_array_equal(idx, want_idx)
                np.testing.assert_array_equal(dist.astype(np.float32), np.asarray(want_dist).astype(np.float32))
    # one list, iterative scan off: only what that list holds
    idx, _, S, scanned = model.search(metric, q[0], 10, 200, 1, "off", model.lists, mask)
    first = model.ivf.probe(bit_model.binary_quantize(q[0])[0], 1)[0]
    assert scanned == 1 and (model.ivf.assign[S] == first).all() and len(S) == int((mask.astype(bool) & (model.ivf.assign == first)).sum())


# ---- the LDS formula -------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "vsr_ivf_lds.h"
int main(int argc, char** argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const unsigned lists = (unsigned) atoi(argv[i]), bits = (unsigned) atoi(argv[i + 1]), shortlist = (unsigned) atoi(argv[i + 2]);
        const unsigned chunks = (bits + 127u) / 128u;
        printf("%u %u %u %zu %zu\n", lists, bits, shortlist, vsr::ivf_shortlist_lds_bytes(lists, chunks, shortlist),
               vsr::ivf_iter_lds_bytes(lists, chunks, shortlist, true));
    }
    return 0;
}
"""

SHAPES = [(lists, bits, shortlist) for lists in (1, 1000, 32768) for bits in (52, 768, 64000) for shortlist in (1, 512, 513, 2048)]


def _restated(lists, bits, shortlist):
    kept = 512
    while kept < shortlist:
        kept *= 2
    centre_keys = (lists * 4 + 15) // 16 * 16
    query = (bits + 127) // 128 * 16                         # whole 16-byte chunks of packed bits
    row_slots = counts = 4 * 64 * 4                          # 4 waves x 64 x 4 bytes
    return centre_keys + query + row_slots + counts + kept * 8 + 512 * 8 + 64


def test_lds_formula_agrees_with_a_restatement(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)] + [str(v) for s in SHAPES for v in s], text=True)
    lines = [ln.split() for ln in out.split("\n") if ln.strip()]
    assert len(lines) == len(SHAPES)
    for f, (lists, bits, shortlist) in zip(lines, SHAPES):
        assert (int(f[0]), int(f[1]), int(f[2])) == (lists, bits, shortlist)
        want = _restated(lists, bits, shortlist)
        assert int(f[3]) == want, (lists, bits, shortlist, f[3], want)
        assert int(f[4]) == want                             # the carve is K3i's bit form at k = shortlist
        assert want <= 160 * 1024                            # every shape the entry point admits fits a compute unit
    assert _restated(1000, 768, 400) == 14400
