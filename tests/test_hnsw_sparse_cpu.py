"""The numpy model of the sparse HNSW scan (tests/hnsw_sparse_model.py) against the index oracle, on the CPU.

1. On integer-valued CSR rows the model's walk -- tests/hnsw_iterative_model.py's with tests/sparse_model.py's sums -- is
   oracle.HnswIndex(...).search on the densified rows, for the four sparsevec opclasses: rows, index distances, visited counts.
   Its iterative streams equal hnsw_iterative_model.IterativeScan's over the dense rows.
2. pgvector's recall TAP case for the type (test/t/028_hnsw_sparsevec_build_recall.pl) as numpy: the oracle's serial build and
   the batched build the GPU restates both clear pgvector's floors for every opclass.
3. l2_norms / l2_normalize, the restatements of sparsevec_l2_norm / sparsevec_l2_normalize, on pgvector's own expectations."""
import numpy as np
import pytest

from hnsw_iterative_model import Graph, IterativeScan
from hnsw_sparse_model import (METRICS, SparseGraph, SparseScan, densify, l2_norms, l2_normalize, reported, search, sparsify,
                               tap_case, tap_recall, tie_aware_expected, unit_rows)
from oracle.oracle import HnswIndex as OracleHnsw

F = np.float32


def _int_csr(rng, n, dim, max_nnz):
    """Rows of 0 .. max_nnz non-zero integers in -4 .. 4 (row 3 empty, row 5 full), as dense float32."""
    x = np.zeros((n, dim), dtype=F)
    for r in range(n):
        nnz = int(rng.integers(0, max_nnz + 1))
        if r == 3:
            nnz = 0
        if r == 5:
            nnz = max_nnz
        cols = rng.choice(dim, nnz, replace=False)
        x[r, cols] = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], nnz)
    return x


@pytest.fixture(scope="module")
def case(oracle):
    rng = np.random.default_rng(2801)
    n, dim = 800, 24
    x = _int_csr(rng, n, dim, 10)
    q = _int_csr(rng, 10, dim, 12)
    q[0] = 0                                                  # the empty query
    q[1] = x[5]
    graphs = {}
    for metric in METRICS:
        oh = OracleHnsw(oracle, metric, x, m=8, ef_construction=32, seed=3)
        graphs[metric] = (oh, SparseGraph(oh.export(), *sparsify(x)))
    return x, q, graphs


@pytest.mark.parametrize("metric", METRICS)
def test_model_walk_is_the_oracle_walk(case, metric):
    x, q, graphs = case
    oh, g = graphs[metric]
    for ef in (1, 10, 40, 200):
        for i in range(len(q)):
            _, qi, qx, _ = sparsify(q[i])
            rows, dist, t = search(g, qi, qx, ef, metric)
            rows_o, dist_o, _, nv = oh.search(q[i], ef)
            np.testing.assert_array_equal(rows, rows_o, err_msg=str((metric, ef, i)))
            np.testing.assert_array_equal(dist, dist_o, err_msg=str((metric, ef, i)))
            assert t == nv, (metric, ef, i, t, nv)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("mode", ["relaxed_order", "strict_order"])
def test_model_streams_are_the_dense_streams(case, metric, mode):
    x, q, graphs = case
    oh, g = graphs[metric]
    dense = Graph(oh.export(), x)
    for max_scan in (1, 150, 20000):
        for i in range(len(q)):
            _, qi, qx, _ = sparsify(q[i])
            a = list(SparseScan(g, qi, qx, 20, metric, mode, max_scan))
            b = list(IterativeScan(dense, q[i], 20, metric, mode, max_scan))
            assert a == b, (metric, mode, max_scan, i)


def test_reported_distances():
    d = np.array([0.0, 9.0, 2.0], dtype=np.float64)
    np.testing.assert_array_equal(reported("l2", d), np.sqrt(d).astype(F))
    np.testing.assert_array_equal(reported("l1", d), d.astype(F))
    np.testing.assert_array_equal(reported("ip", -d), (-d).astype(F))
    np.testing.assert_array_equal(reported("cosine", np.array([-0.25, -2.0, 2.0])), np.array([0.75, 0.0, 2.0], dtype=F))


def _exact(metric, rows, q):
    x, qq = rows.astype(np.float64), q.astype(np.float64)
    if metric == "l2":
        return ((x - qq) ** 2).sum(axis=1)
    if metric == "l1":
        return np.abs(x - qq).sum(axis=1)
    if metric == "ip":
        return -(x @ qq)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - (x @ qq) / np.sqrt((x * x).sum(axis=1) * (qq * qq).sum())


@pytest.mark.parametrize("metric", METRICS)
def test_tap_case_floors_on_the_cpu(oracle, metric):
    """028_hnsw_sparsevec_build_recall.pl: recall@20 at ef_search 40 >= 0.99 (0.97 for <#>) for the serial build; the batched
    build the GPU restates clears the same floor.  Cosine runs on unit rows and unit queries (K4's convention)."""
    rows, queries, limit, ef = tap_case()
    floor = 0.97 if metric == "ip" else 0.99
    expected = [tie_aware_expected(_exact(metric, rows, q), limit) for q in queries]
    xs, qs = (unit_rows(rows), unit_rows(queries)) if metric == "cosine" else (rows, queries)
    for name, build in (("serial", lambda: OracleHnsw(oracle, metric, xs, m=16, ef_construction=64, seed=28)),
                        ("batched", lambda: OracleHnsw.batched(oracle, metric, xs, 16, 64, 28))):
        oh = build()
        r = tap_recall([oh.search(q, ef)[0] for q in qs], expected, limit)
        print(f"sparsevec TAP case, {metric}, {name} build: recall@{limit} ef={ef} = {r:.4f} (floor {floor})")
        assert r >= floor, (metric, name, r)


def test_l2_norm_and_normalize_restatements():
    """pgvector's regress expectations (test/expected/sparsevec.out: l2_norm, l2_normalize) and the edges the GPU tests use."""
    ip, ix, vx, dim = sparsify(np.array([[3, 4, 0], [0, 1, 0], [0, 0, 0], [3e37, 4e37, 0], [0, 0.1, 0]], dtype=F))
    n = l2_norms(ip, vx)
    assert n[0] == 5.0 and n[1] == 1.0 and n[2] == 0.0
    assert float(F(n[3])) == float(F(5e37))
    op, oi, ov, od, dropped = l2_normalize(ip, ix, vx, dim)
    np.testing.assert_array_equal(densify(op, oi, ov, od),
                                  np.array([[0.6, 0.8, 0], [0, 1, 0], [0, 0, 0], [0.6, 0.8, 0], [0, 1, 0]], dtype=F))
    assert dropped == 0
    # an entry that underflows to 0 is dropped: 1e-30 / 1e30 in float4
    ip, ix, vx, dim = sparsify(np.array([[1e-30, 0, 1e30]], dtype=F))
    op, oi, ov, od, dropped = l2_normalize(ip, ix, vx, dim)
    assert dropped == 1 and op.tolist() == [0, 1] and oi.tolist() == [2] and ov.tolist() == [1.0]
    # sequential double sums: the value depends on the order, and the restatement keeps the entry order
    rng = np.random.default_rng(7)
    v = rng.normal(size=300).astype(F)
    want = 0.0
    for t in v.tolist():
        want += t * t
    assert l2_norms([0, 300], v)[0] == np.sqrt(want)
