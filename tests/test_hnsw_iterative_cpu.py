"""CPU checks of pgvector's HNSW iterative index scan (vsr_hnsw_search_iterative): the numpy restatement of the stream
(tests/hnsw_iterative_model.py) is pinned to the index oracle's search for round 0, and its invariants are checked; the
library exports the new entry points without changing the ABI version."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_iterative_model import Graph, IterativeScan, Stream


@pytest.fixture(scope="module")
def graph5k(oracle):
    rng = np.random.default_rng(31)
    n, dim = 5_000, 32
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    x[1000:1012] = x[7]                                # 13 copies of one vector: elements with 10 and more heap TIDs
    h = OracleHnsw(oracle, "l2", x, m=8, ef_construction=32, seed=2)
    q = x[rng.integers(0, n, 20)] + rng.integers(-2, 3, (20, dim)).astype(np.float32)
    q[0] = x[7]
    return x, h, Graph(h.export(), x), q


@pytest.mark.parametrize("ef", [10, 40, 200])
def test_round0_is_the_oracle_search(graph5k, ef):
    """Mode off (round 0 only): the oracle's rows, index distances and visited count."""
    x, h, g, q = graph5k
    for i in range(len(q)):
        rows_o, dist_o, _, nv = h.search(q[i], ef)
        scan = IterativeScan(g, q[i], ef, "l2", "off")
        got = list(scan)
        np.testing.assert_array_equal([r for r, _, _ in got], rows_o)
        np.testing.assert_array_equal([d for _, d, _ in got], dist_o)
        assert scan.tuples == nv
        assert all(t == nv for _, _, t in got)
        # relaxed_order emits round 0 first, unchanged
        rel = Stream(IterativeScan(g, q[i], ef, "l2", "relaxed_order"))
        r, d, _ = rel.answer(rows_o.size)
        np.testing.assert_array_equal(r, rows_o)


@pytest.mark.parametrize("ef", [10, 40])
def test_strict_order_is_non_decreasing(graph5k, ef):
    x, h, g, q = graph5k
    for i in range(0, len(q), 4):
        d = [dd for _, dd, _ in IterativeScan(g, q[i], ef, "l2", "strict_order", max_scan_tuples=2000)]
        assert len(d) > ef
        assert (np.diff(d) >= 0).all()


@pytest.mark.parametrize("max_scan", [300, 10**9])
def test_full_relaxed_stream_emits_each_row_once(graph5k, max_scan):
    """The whole stream: no row twice; its length is the summed TID counts of the elements it emitted, and with
    max_scan_tuples >= n the final T is the number of elements visited (the graph may leave a few unreachable)."""
    x, h, g, q = graph5k
    for i in (0, 5):
        scan = IterativeScan(g, q[i], 40, "l2", "relaxed_order", max_scan_tuples=max_scan)
        elems = [e for e, _ in scan.elements()]
        assert len(set(elems)) == len(elems)
        scan2 = IterativeScan(g, q[i], 40, "l2", "relaxed_order", max_scan_tuples=max_scan)
        rows = [r for r, _, _ in scan2]
        assert len(set(rows)) == len(rows)
        assert len(rows) == sum(g.tid_count[e] for e in elems)
        assert scan2.tuples == len(elems)                  # every visited element was emitted in the end
        if max_scan == 300:                                # the drain: T stops growing a round after it reaches 300
            assert scan2.tuples < 0.5 * g.n_elem
        else:
            assert len(elems) >= 0.95 * g.n_elem


def test_prefix_property_of_the_model(graph5k):
    x, h, g, q = graph5k
    mask = (np.arange(len(x)) % 7 == 0)
    s = Stream(IterativeScan(g, q[3], 40, "l2", "relaxed_order", max_scan_tuples=3000))
    r200, _, _ = s.answer(200, mask)
    r40, _, _ = s.answer(40, mask)
    np.testing.assert_array_equal(r40, r200[:40])
    assert mask[r200].all()


def test_iterative_symbols_exported_and_abi_unchanged():
    import vsrbac
    from vsrbac import _ffi
    lib = ctypes.CDLL(vsrbac.library_path())
    for name in ("vsr_hnsw_search_iterative", "vsr_hnsw_search_iterative_device"):
        assert hasattr(lib, name), name
        assert name in _ffi.SYMBOLS
    assert vsrbac.abi_version() == 2
    from vsrbac.engine import HnswIndex, ITERATIVE_MODES
    assert ITERATIVE_MODES == {"off": 0, "relaxed_order": 1, "strict_order": 2}
    assert hasattr(HnswIndex, "search_iterative") and hasattr(HnswIndex, "search_iterative_device")
