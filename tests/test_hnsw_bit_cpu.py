"""CPU checks of HNSW over bit corpora (vsr_hnsw_*_bit, vsr_hnsw_search_quantized*): the library binds the new entry points;
the numpy model of the bit walk (tests/hnsw_bit_model.py) is pinned to the index oracle -- squared L2 on rows unpacked to
0 / 1 floats IS the Hamming distance -- and to pgvector's known answers; pgvector's own recall floors hold on the case the GPU
build test uses."""
import json
import os

import numpy as np
import pytest

import bit_model
from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_bit_model import BitGraph, BitScan, search, tap_case, tap_recall, tie_aware_expected

NEW_SYMBOLS = ("vsr_hnsw_load_bit", "vsr_hnsw_build_bit", "vsr_hnsw_search_bit", "vsr_hnsw_search_bit_device",
               "vsr_hnsw_search_bit_iterative", "vsr_hnsw_search_bit_iterative_device", "vsr_hnsw_search_quantized",
               "vsr_hnsw_search_quantized_device")


def test_new_symbols_are_bound():
    from vsrbac import _ffi
    import vsrbac
    for name in NEW_SYMBOLS:
        assert name in _ffi.SYMBOLS, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsrbac.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    lib = vsrbac.load_library()                              # binds every symbol; never touches the GPU
    assert lib.vsr_abi_version() == 2
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == _ffi.SYMBOLS[name][1]
    from vsrbac.engine import Corpus, HnswIndex
    for cls, names in ((Corpus, ("load_hnsw_bit", "build_hnsw_bit", "search_quantized_hnsw", "search_quantized_hnsw_device")),
                       (HnswIndex, ("search_bit", "search_bit_device", "search_bit_iterative", "search_bit_iterative_device"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


@pytest.fixture(scope="module")
def graph3k(oracle):
    rng = np.random.default_rng(52)
    n, dim = 3000, 52
    packed = bit_model.pack(rng.integers(0, 2, (n, dim)).astype(bool))
    packed[2000:2012] = packed[5]                            # 13 copies: elements with 10 and more heap TIDs
    unpacked = bit_model.unpack(packed, dim).astype(np.float32)
    h = OracleHnsw(oracle, "l2", unpacked, m=16, ef_construction=64, seed=3)
    q = bit_model.pack(rng.integers(0, 2, (16, dim)).astype(bool))
    q[0] = packed[5]
    return packed, unpacked, dim, h, BitGraph(h.export(), packed, dim), q


@pytest.mark.parametrize("ef", [10, 40, 200])
def test_hamming_walk_is_the_oracle_l2_walk(graph3k, ef):
    """Rows, distances and visited counts; Hamming distances tie constantly, so this is the (distance, element id) order."""
    packed, unpacked, dim, h, g, q = graph3k
    ties = 0
    for i in range(len(q)):
        rows_o, dist_o, _, nv = h.search(bit_model.unpack(q[i:i + 1], dim)[0].astype(np.float32), ef)
        rows, dist, t = search(g, q[i], ef, "hamming")
        np.testing.assert_array_equal(rows, rows_o)
        np.testing.assert_array_equal(dist, dist_o)
        assert t == nv
        ties += int((np.diff(dist) == 0).sum())
    assert ties > len(q)                                     # the tie rule really was exercised


def test_pgvector_known_answers(golden_dir, oracle):
    """test/expected/hnsw_bit.out, both opclasses, through the model with a full-width beam."""
    cases = json.load(open(os.path.join(golden_dir, "pgvector_hnsw_bit_known_answers.json")))["cases"]
    assert {c["opclass"] for c in cases} == {"bit_hamming_ops", "bit_jaccard_ops"}
    for c in cases:
        dim = c["dim"]
        bits = np.array([[ch == "1" for ch in r] for r in c["rows"]], dtype=bool)
        packed = bit_model.pack(bits)
        h = OracleHnsw(oracle, "l2", bits.astype(np.float32), m=16, ef_construction=64, seed=1)
        g = BitGraph(h.export(), packed, dim)
        q = bit_model.pack(np.array([[ch == "1" for ch in c["query"]]], dtype=bool))[0]
        rows, dist, _ = search(g, q, len(c["rows"]), c["metric"])
        assert [c["rows"][r] for r in rows] == c["expected"], (c["opclass"], rows, dist)
        assert (np.diff(dist) >= 0).all()


@pytest.fixture(scope="module")
def tap(oracle):
    rows, queries, dim, limit, ef = tap_case()
    h = OracleHnsw(oracle, "l2", bit_model.unpack(rows, dim).astype(np.float32), m=16, ef_construction=64, seed=1)
    return rows, queries, dim, limit, ef, BitGraph(h.export(), rows, dim)


@pytest.mark.parametrize("metric,floor", [("hamming", 0.98), ("jaccard", 0.95)])
def test_reference_recall_floor(tap, metric, floor):
    """020_hnsw_bit_build_recall.pl's floors on its own case, by the reference alone: the oracle's serial build, walked with
    Hamming distances (= the oracle's own search, see above) and, for bit_jaccard_ops, with Jaccard distances."""
    rows, queries, dim, limit, ef, g = tap
    exact = bit_model.BitModel(rows, dim).distances(metric, queries).astype(np.float32)
    found = [search(g, queries[i], ef, metric)[0] for i in range(len(queries))]
    expected = [tie_aware_expected(exact[i], limit) for i in range(len(queries))]
    r = tap_recall(found, expected, limit)
    print(f"reference recall@{limit} ef={ef} {metric}: {r:.4f} (floor {floor})")
    assert r >= floor
