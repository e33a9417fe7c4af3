"""CPU checks of HNSW over halfvec corpora (vsr_hnsw_load_half / vsr_hnsw_build_half / vsr_hnsw_device_bytes): the library
exports and binds the new entry points; the known-answer fixture is what numpy computes in the type's arithmetic; the inputs
of the GPU query-rounding test really are not binary16 values and really change the oracle's answer; pgvector's recall floor
holds for the oracle's serial build on the cases the GPU build test uses."""
import ctypes
import os

import numpy as np
import pytest

from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_half_model import (ROUNDING_NQ, TAP_EF, TAP_LIMIT, exact_order, known_answer_rows, known_answers, recall, round_query,
                             rounding_case, tap_case, to_half, widen)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"vsr_hnsw_load_half": "int", "vsr_hnsw_build_half": "int", "vsr_hnsw_device_bytes": "int64_t"}


def test_new_symbols_are_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    header = open(os.path.join(ROOT, "include", "vsrbac.h")).read()
    lib = ctypes.CDLL(vsrbac.library_path())                 # the built library; never touches the GPU
    for name, ret in NEW_SYMBOLS.items():
        assert f"{ret} {name}(" in header, name
        assert hasattr(lib, name), f"{name} is not exported by libvsrbac.so"
        assert name in _ffi.SYMBOLS, name
    bound = vsrbac.load_library()
    assert bound.vsr_hnsw_load_half.argtypes == _ffi.SYMBOLS["vsr_hnsw_load"][1]
    assert bound.vsr_hnsw_build_half.argtypes == _ffi.SYMBOLS["vsr_hnsw_build_ex"][1]
    assert bound.vsr_hnsw_device_bytes.restype == ctypes.c_int64
    assert bound.vsr_hnsw_device_bytes(None) == 0
    from vsrbac.engine import Corpus, HnswIndex
    for cls, names in ((Corpus, ("load_hnsw_half", "build_hnsw_half")), (HnswIndex, ("device_bytes",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_known_answers_are_the_types_arithmetic(golden_dir):
    """test/expected/hnsw_halfvec.out: the orders numpy computes on the widened rows with the rounded query."""
    cases = known_answers(golden_dir)
    assert [c["opclass"] for c in cases] == ["halfvec_l2_ops", "halfvec_ip_ops", "halfvec_cosine_ops"]
    for c in cases:
        held, orig = known_answer_rows(c)
        rows_half = to_half(held)
        q = np.array(c["query"], dtype=np.float32)
        order, d = exact_order(c["metric"], rows_half, q)
        assert orig[order].astype(int).tolist() == c["expected"], (c["opclass"], order, d)
        assert (np.diff(d[order]) > 0).all()                 # no ties: the order is the only one
        if c["metric"] == "cosine":                          # the opclass ranks the unit rows by negative inner product: same order
            ip_order, _ = exact_order("ip", rows_half, q / np.linalg.norm(q))
            assert ip_order.tolist() == order.tolist()


@pytest.fixture(scope="module")
def rounding(oracle):
    x, raw, rounded = rounding_case()
    return x, raw, rounded, OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=5)


def test_rounding_inputs_are_not_binary16_values(rounding):
    x, raw, rounded, _ = rounding
    assert (widen(to_half(x)) == x).all()                    # the rows are exact in binary16
    touched = raw != 0
    assert touched.sum() > raw.size // 2
    assert (rounded[touched] != raw[touched]).all()          # no non-zero element survives the rounding unchanged
    assert (rounded == np.rint(rounded)).all()               # ... every one becomes an integer, exact in binary16
    assert (raw[:ROUNDING_NQ // 2, 3] == 2049).all() and (rounded[:ROUNDING_NQ // 2, 3] == 2048).all()
    assert np.abs(rounded).max() <= 2048 and (round_query(rounded) == rounded).all()


def test_rounding_changes_the_oracles_answer(rounding):
    """The walk of the raw fp32 query differs from the walk of its rounded copy: a kernel that skipped the rounding would be
    caught by the GPU test."""
    x, raw, rounded, oh = rounding
    differ = 0
    for i in range(len(raw)):
        rows_raw, dist_raw, _, _ = oh.search(raw[i], 40)
        rows_rnd, dist_rnd, _, _ = oh.search(rounded[i], 40)
        differ += int(rows_raw.size != rows_rnd.size or (rows_raw != rows_rnd).any() or (dist_raw != dist_rnd).any())
    print(f"{differ} of {len(raw)} queries answer differently when the rounding is skipped")
    assert differ >= 1


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_reference_recall_floor(oracle, metric):
    """024_hnsw_halfvec_build_recall.pl's floor (0.98, all opclasses) on the GPU build test's own rows and seeds, by the reference
    alone: the oracle's serial build on the widened rows, asked with the rounded queries."""
    rows_half, q = tap_case(metric)
    oh = OracleHnsw(oracle, metric, widen(rows_half), m=16, ef_construction=64, seed=1)
    rq = round_query(q)
    expected = [exact_order(metric, rows_half, q[i])[0][:TAP_LIMIT] for i in range(len(q))]
    found = [oh.search(rq[i], TAP_EF)[0][:TAP_LIMIT] for i in range(len(q))]
    r = recall(found, expected)
    print(f"reference recall@{TAP_LIMIT} ef={TAP_EF} {metric}: {r:.4f} (floor 0.98)")
    assert r >= 0.98
