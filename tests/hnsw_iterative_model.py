"""pgvector's HNSW iterative index scan restated in numpy (the contract of vsr_hnsw_search_iterative, include/vsrbac.h).

hnswgettuple with hnsw.iterative_scan != off (pgvector/src/hnswscan.c:47-76,227-312) over HnswSearchLayer with a discarded
heap (hnswutils.c:813-976), on the arrays of oracle.oracle.HnswIndex.export() and the rows.  Candidates are ordered by
(index distance, element id), the tie rule of K4 and of the index oracle.  Per query:

  V  visited set, kept for the whole scan        D  discarded candidates (admission rejects, elements pushed out of W)
  T  so->tuples                                  P  so->previousDistance (strict_order)

Round 0 is the greedy descent and the layer-0 search with ef; when W runs dry, T >= max_scan_tuples drains D one element at
a time, otherwise the min(ef, |D|) nearest of D are the entry points of another layer-0 search (not marked or counted
again).  The stream of emitted rows depends on neither k nor the filter: the answer for a filter and k is the first k
permitted rows of the stream, and T is its value when the k-th came out (or the final T when there are fewer).

Distances are computed in float64 from float32 rows: on integer-valued rows they equal the GPU's fp32 sums exactly.
"""
import heapq

import numpy as np


def rank_values(metric, rows, q):
    """Index distances of every row to q: squared L2, or the negative inner product (inner product and cosine opclasses)."""
    x = rows.astype(np.float64)
    qq = np.asarray(q, dtype=np.float32).astype(np.float64)
    if metric == "l2":
        d = x - qq
        return np.einsum("ij,ij->i", d, d)
    return -(x @ qq)


class Graph:
    """The export() arrays in the form the walk wants (Python lists: the walk is scalar code)."""

    def __init__(self, g, rows):
        self.m = int(g["m"])
        self.entry = int(g["entry"])
        self.level = np.asarray(g["level"]).tolist()
        self.nbr0 = np.asarray(g["nbr0"]).tolist()
        self.tid_count = np.asarray(g["tid_count"]).tolist()
        self.tids = np.asarray(g["tids"]).tolist()
        self.up_slot = np.asarray(g["up_slot"]).tolist()
        self.up_nbr = np.asarray(g["up_nbr"])
        self.n_elem = len(self.level)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.elem_row = np.asarray(g["tids"])[:, 0]

    def neighbours(self, e, lc):
        if lc == 0:
            return self.nbr0[e]
        slot = self.up_slot[e]
        return self.up_nbr[slot, lc - 1].tolist() if slot >= 0 else []


def _search_layer(g, dist, ep, ef, lc, visited, discarded, count_entries):
    """HnswSearchLayer: ep = [(d, e)] entry points; returns (W nearest first, tuples added).  visited: set (shared across
    rounds on layer 0); discarded: None or a heap of (d, e)."""
    tuples = 0
    C = []
    W = []                                      # max-heap by (d, e): entries (-d, -e)
    for d, e in ep:
        if count_entries:
            visited.add(e)
            tuples += 1
        heapq.heappush(C, (d, e))
        heapq.heappush(W, (-d, -e))
    wlen = len(ep)
    while C:
        cd, ce = heapq.heappop(C)
        if cd > -W[0][0]:
            break
        unvisited = []
        for e in g.neighbours(ce, lc):
            if e < 0 or e in visited:
                continue
            visited.add(e)
            unvisited.append(e)
        tuples += len(unvisited)
        for e in unvisited:
            ed = dist[e]
            if not (ed < -W[0][0] or wlen < ef):
                if discarded is not None:
                    heapq.heappush(discarded, (ed, e))
                continue
            if g.level[e] < lc:
                continue
            heapq.heappush(C, (ed, e))
            heapq.heappush(W, (-ed, -e))
            wlen += 1
            if wlen > ef:
                nd, ne = heapq.heappop(W)
                if discarded is not None:
                    heapq.heappush(discarded, (-nd, -ne))
    w = sorted((-d, -e) for d, e in W)
    return w, tuples


class IterativeScan:
    """Iterate over (row, index_distance, T at emission) of one query's unfiltered stream (strict_order drops applied).
    After the iteration ends, .tuples is the final T."""

    def __init__(self, g, q, ef, metric="l2", mode="relaxed_order", max_scan_tuples=20000):
        assert mode in ("off", "relaxed_order", "strict_order")
        self.g, self.ef, self.mode, self.max_scan = g, int(ef), mode, int(max_scan_tuples)
        self.dist = rank_values(metric, g.rows[g.elem_row], q).tolist()   # per element
        self.tuples = 0

    def elements(self):
        """(element, distance) in emission order (before the strict filter), updating self.tuples."""
        g, dist = self.g, self.dist
        if g.entry < 0:
            return
        ep = [(dist[g.entry], g.entry)]
        for lc in range(g.level[g.entry], 0, -1):
            ep, _ = _search_layer(g, dist, ep, 1, lc, set(), None, True)
        visited = set()
        discarded = [] if self.mode != "off" else None
        w, t = _search_layer(g, dist, ep, self.ef, 0, visited, discarded, True)
        self.tuples = t
        while True:
            for d, e in w:
                yield e, d
            if self.mode == "off" or not discarded:
                return
            if self.tuples >= self.max_scan:          # the drain
                w = [heapq.heappop(discarded)]
                continue
            ep = [heapq.heappop(discarded) for _ in range(min(self.ef, len(discarded)))]
            w, t = _search_layer(g, dist, ep, self.ef, 0, visited, discarded, False)
            self.tuples += t

    def __iter__(self):
        prev = -np.inf
        for e, d in self.elements():
            nt = self.g.tid_count[e]
            if nt == 0:
                continue
            if self.mode == "strict_order":
                if d < prev:
                    continue
                prev = d
            for t in range(nt - 1, -1, -1):            # newest heap TID first
                yield self.g.tids[e][t], d, self.tuples


class Stream:
    """One walk serving every filter and k: the rows of a scan materialised as far as some caller needed them."""

    def __init__(self, scan):
        self.scan, self._it, self.rows, self.dist, self.t, self.done = scan, iter(scan), [], [], [], False

    def _more(self):
        try:
            row, d, t = next(self._it)
        except StopIteration:
            self.done = True
            return False
        self.rows.append(row)
        self.dist.append(d)
        self.t.append(t)
        return True

    def answer(self, k, mask=None):
        """(rows, index distances, T) for LIMIT k under mask (None = every row)."""
        rows, dists, i = [], [], 0
        while len(rows) < k:
            if i == len(self.rows) and not self._more():
                return np.array(rows, dtype=np.int64), np.array(dists), self.scan.tuples
            r = self.rows[i]
            if mask is None or mask[r]:
                rows.append(r)
                dists.append(self.dist[i])
                t = self.t[i]
            i += 1
        return np.array(rows, dtype=np.int64), np.array(dists), t
