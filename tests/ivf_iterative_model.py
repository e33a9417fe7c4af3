"""pgvector's IVFFlat iterative index scan (ivfflat.iterative_scan = relaxed_order, ivfflat.max_probes; ivfscan.c:112-176,
249-272, 375-381) restated in numpy on top of the index oracle -- the model vsr_ivf_search_iterative is pinned to -- and the
fixtures the CPU and the GPU tests of it share.

The stream of one query: the M = min(max(max_probes, probes), lists) nearest lists in the oracle's probe order, cut into
batches of P = min(probes, lists) lists (the last one may be short); each batch's rows sorted by the exact filtered top-k
(distance, then (document_id, block_id)); batches are concatenated, never re-sorted.  A batch is begun only while fewer than
k permitted rows are out and lists remain."""
import numpy as np


def batch_bounds(probes, max_probes, lists):
    """[(first, end)) positions in the list order of every batch the scan could run."""
    p = min(int(probes), int(lists))
    m = min(max(int(max_probes), int(probes)), int(lists))
    return [(b, min(b + p, m)) for b in range(0, m, p)]


def iterative_search(oivf, q, k, probes, max_probes, doc=None, blk=None, mask=None):
    """rows (int64), distances (float64, the operator's value as the oracle reports it), lists scanned (so->listIndex)."""
    orc, n = oivf.orc, len(oivf.rows)
    m = min(max(int(max_probes), int(probes)), oivf.lists)
    order = oivf.probe(q, m)                                  # GetScanLists with so->maxProbes
    allowed = np.ones(n, dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)
    rows, dist, scanned = [], [], 0
    for lo, hi in batch_bounds(probes, max_probes, oivf.lists):
        have = sum(len(r) for r in rows)
        if have >= k:
            break
        sel = np.isin(oivf.assign, order[lo:hi]).astype(np.uint8) & allowed
        r, d = orc.filtered_topk(oivf.metric, oivf.rows, q, k - have, doc, blk, sel)
        rows.append(r)
        dist.append(d)
        scanned = hi
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64),
            np.concatenate(dist) if dist else np.zeros(0, np.float64), scanned)


class ParityFixture:
    """6000 x 16 integer rows in 0..31 (every fp32 sum is exact; many equal distances across the lists of a batch), 64
    centres of which 4 own no row, three users seeing 2 %, 25 % and none of the rows, 16 queries."""

    def __init__(self, oracle, n=6000, dim=16, seed=141):
        from oracle.oracle import IvfIndex as OracleIvf
        rng = np.random.default_rng(seed)
        self.n, self.dim = n, dim
        x = rng.integers(0, 32, (n, dim)).astype(np.float32)
        x[n // 2:n // 2 + 12] = x[17]
        self.x = x
        self.doc = (np.arange(n) // 10 + 1).astype(np.int32)
        self.blk = (np.arange(n) + 1).astype(np.int64)
        ndocs = int(self.doc.max())
        docs = np.arange(1, ndocs + 1)
        self.perms = [(1, int(d)) for d in rng.choice(docs, ndocs // 50, replace=False)] + \
                     [(2, int(d)) for d in rng.choice(docs, ndocs // 4, replace=False)]
        centers = np.concatenate([x[np.sort(rng.choice(n, 60, replace=False))] + 0.25,
                                  1000.0 + rng.integers(0, 32, (4, dim)).astype(np.float32)]).astype(np.float32)
        self.centers = centers
        self.oivf = OracleIvf.from_centers(oracle, "l2", x, centers)
        self.user_roles = [(1, 1), (2, 2), (3, 3)]           # role 3 has no permission
        self.masks = {u: oracle.user_row_mask(u, self.user_roles, self.perms, self.doc) for u in (1, 2, 3)}
        self.masks[None] = None
        q = x[rng.integers(0, n, 16)] + rng.integers(-1, 2, (16, dim)).astype(np.float32)
        q[0] = x[17]
        self.q = q.astype(np.float32)
        self._cache = {}

    def model(self, user, i, k, probes, max_probes):
        """The model's answer for query i under user's filter (None: no filter), computed once."""
        key = (user, i, k, probes, max_probes)
        if key not in self._cache:
            self._cache[key] = iterative_search(self.oivf, self.q[i], k, probes, max_probes, self.doc, self.blk, self.masks[user])
        return self._cache[key]


def tap_corpus(oracle):
    """The corpus of pgvector's test/t/041 and 042 mirrors: 100 000 x 3 uniform floats, 100 lists."""
    from oracle.oracle import IvfIndex as OracleIvf
    rng = np.random.default_rng(42)
    x = rng.random((100_000, 3)).astype(np.float32)
    return x, OracleIvf(oracle, "l2", x, lists=100, seed=7)


def tap_queries():
    """20 random queries of the 042 mirror."""
    return np.random.default_rng(43).random((20, 3)).astype(np.float32)


def recall_at(got_rows, want_rows):
    return len(set(got_rows.tolist()) & set(want_rows.tolist())) / max(len(want_rows), 1)
