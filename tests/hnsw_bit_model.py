"""pgvector's HNSW scan over a bit column restated in numpy (the contract of vsr_hnsw_search_bit* and of
vsr_hnsw_search_quantized, include/vsrbac.h).

The walk is tests/hnsw_iterative_model.py's, unchanged: descent, layer-0 beam, discarded set, iterative rounds, the
(distance, element id) tie rule.  Only the per-element distance differs -- bit_hamming_ops / bit_jaccard_ops
(hnswutils.c:1398-1410) over packed rows:

  hamming   popcount(a ^ b), an integer
  jaccard   the double of bitutils.c:96-129 rounded to fp32, the value vsr_search_bit reports (tests/bit_model.py)

both held as the fp32 value the GPU keys carry, so that ties are the GPU's ties.  Mode "off" is the plain search.

On rows unpacked to 0 / 1 floats squared L2 IS the Hamming distance, so oracle.HnswIndex("l2", unpacked) is the serial
pgvector build and GetScanItems walk of bit_hamming_ops; tests/test_hnsw_bit_cpu.py pins this model to it.

indexed_two_stage restates vsr_hnsw_search_quantized: the shortlist is this model's Hamming answer for k = shortlist, the
re-rank is tests/quantized_model.py's."""
import numpy as np

import bit_model
from hnsw_iterative_model import Graph, IterativeScan, Stream


class BitGraph(Graph):
    """The export() arrays of a graph over packed rows [n, (dim + 7) // 8] of `dim` bits (caller row order)."""

    def __init__(self, g, packed, dim):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        super().__init__(g, bit_model.unpack(packed, dim).astype(np.float32))
        self.dim = int(dim)
        self.packed = packed
        self.elem_model = bit_model.BitModel(packed[self.elem_row], dim)      # one row per element: its first TID's


def element_distances(g, metric, q_packed):
    """fp32 index distances of every element to the packed query, as Python floats (exact images of the fp32 values)."""
    d = g.elem_model.distances(metric, np.atleast_2d(np.asarray(q_packed, dtype=np.uint8)))[0]
    return d.astype(np.float32).astype(np.float64).tolist()


class BitScan(IterativeScan):
    """IterativeScan over a BitGraph: (row, fp32 index distance, T at emission) of one query's stream."""

    def __init__(self, g, q_packed, ef, metric="hamming", mode="off", max_scan_tuples=20000):
        assert metric in ("hamming", "jaccard") and mode in ("off", "relaxed_order", "strict_order")
        self.g, self.ef, self.mode, self.max_scan = g, int(ef), mode, int(max_scan_tuples)
        self.dist = element_distances(g, metric, q_packed)
        self.tuples = 0


def search(g, q_packed, ef, metric="hamming"):
    """The plain search of one query: (rows in emission order, fp32 distances as float64, visited count)."""
    scan = BitScan(g, q_packed, ef, metric, "off")
    got = list(scan)
    return (np.array([r for r, _, _ in got], dtype=np.int64), np.array([d for _, d, _ in got], dtype=np.float64), scan.tuples)


def indexed_two_stage(qm, g, queries, k, shortlist, ef, metric, masks=None):
    """vsr_hnsw_search_quantized: per query (rows, float64 distances, S).  qm: quantized_model.QuantizedModel of the source;
    g: the BitGraph over binary_quantize(source); masks[i]: permitted rows of query i or None."""
    queries = np.atleast_2d(np.asarray(queries, dtype=np.float32))
    qb = bit_model.binary_quantize(queries)
    out = []
    for i, q in enumerate(queries):
        mask = None if masks is None else masks[i]
        S, _, _ = Stream(BitScan(g, qb[i], ef, "hamming", "off")).answer(shortlist, mask)
        if S.size == 0:
            out.append((np.zeros(0, dtype=np.int64), np.zeros(0), S))
            continue
        idx, dist = qm.rerank(metric, q, k, S)
        out.append((idx, dist, S))
    return out


def tie_aware_expected(dist_row, limit):
    """The expected set of pgvector's recall TAP tests (020_hnsw_bit_build_recall.pl:84-92): every row no farther than the
    limit-th nearest."""
    d = np.asarray(dist_row)
    kth = np.sort(d, kind="stable")[min(limit, d.size) - 1]
    return np.flatnonzero(d <= kth)


def tap_recall(found_rows_per_query, expected_per_query, limit):
    """020_hnsw_bit_build_recall.pl:39-50: returned ids found in the expected set, over queries x limit."""
    correct = sum(int(np.isin(f[:limit], e).sum()) for f, e in zip(found_rows_per_query, expected_per_query))
    return correct / (len(found_rows_per_query) * limit)


def tap_case(seed=20):
    """The case of 020_hnsw_bit_build_recall.pl: 10 000 random 52-bit rows, 20 random queries, LIMIT 20, ef_search 100.
    (packed rows, packed queries, dim, limit, ef).  One fixed seed: the CPU floor test and the GPU build test share the rows."""
    rng = np.random.default_rng(seed)
    dim = 52
    rows = bit_model.pack(rng.integers(0, 2, (10_000, dim)).astype(bool))
    queries = bit_model.pack(rng.integers(0, 2, (20, dim)).astype(bool))
    return rows, queries, dim, 20, 100
