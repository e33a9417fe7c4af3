"""The contract of vsr_hnsw_forest_search* in numpy: the result of a query is what HnswIndex.search / search_bit returns for it on
each of its graphs, put together, ordered by (distance, document_id, block_id), the first occurrence of each row kept, the first k
taken.

The library orders by the index's RANK value (squared L2, the negated inner product, the Hamming count); this model orders by the
REPORTED distance, which is all the per-graph call hands out.  On the tests' rows the two orders are the same.  Inner product and
Hamming report the rank value itself.  L2 reports sqrt of it, and the rows are integers in -8..8 at 16 dimensions: a squared distance
is an integer of at most 16 * 16^2 = 4096, its root is at most 64, the roots of neighbouring integers there differ by at least
sqrt(4096) - sqrt(4095) > 1/128, and fp32 values below 64 are spaced 2^-18 apart at most -- so sqrt, correctly rounded from double to
fp32, merges no two values and keeps their order.  On real-valued rows (one test) two rank values an ulp apart could share a
root; the model then orders by the per-graph call's own distance all the same, as the issue sets it."""
import numpy as np


def merge_model(per_graph, tasks, k):
    """per_graph[g]: the SearchResult of graph g over ALL queries of the call (None for a graph no task names); tasks: per query the
    graph ids.  Returns (block_ids, doc_ids, rows, dist, counts) as the forest call lays them out: -1 / +Inf past the count."""
    nq = len(tasks)
    blk = np.full((nq, k), -1, dtype=np.int64)
    doc = np.full((nq, k), -1, dtype=np.int32)
    row = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.int32)
    for i, graphs in enumerate(tasks):
        parts = []
        for g in graphs:
            r = per_graph[g]
            n = int(r.counts[i])
            assert n >= 0, "a per-graph result that is not valid"
            parts.append((r.block_ids[i, :n], r.doc_ids[i, :n], r.rows[i, :n], r.dist[i, :n]))
        if not parts:
            continue
        b, d, rw, ds = (np.concatenate([p[j] for p in parts]) for j in range(4))
        order = np.lexsort((b, d, ds))                      # distance, then document_id, then block_id
        b, d, rw, ds = b[order], d[order], rw[order], ds[order]
        _, first = np.unique(rw, return_index=True)         # the first occurrence of every row, in order
        keep = np.sort(first)[:k]
        n = keep.size
        blk[i, :n], doc[i, :n], row[i, :n], dist[i, :n], cnt[i] = b[keep], d[keep], rw[keep], ds[keep], n
    return blk, doc, row, dist, cnt


def assert_same_groups(got, want, candidates):
    """got / want: lists of (block_id, document_id, content, distance) cut at the same k by two merges that agree on the order of
    distances but may break ties differently (harness.merge_results keeps the order its input came in, the library orders a tie by
    (document_id, block_id)).  Every distance group in front of the last one must hold the same rows; the last group, which the cut
    may have split, must have the same size and hold rows that `candidates` (all rows that went into the merge) has at that distance."""
    assert len(got) == len(want)
    if not got:
        return
    dg, dw = sorted({r[3] for r in got}), sorted({r[3] for r in want})
    assert dg == dw, (dg, dw)
    group = lambda rows, d: {(r[1], r[0]) for r in rows if r[3] == d}
    for d in dg[:-1]:
        assert group(got, d) == group(want, d), d
    last = dg[-1]
    assert len(group(got, last)) == len(group(want, last))
    assert group(got, last) <= group(candidates, last) and group(want, last) <= group(candidates, last)
