"""numpy restatement of pgvector's sparsevec distances and of the library's filtered top-k over them (the expected answer of
tests/test_gpu_sparsevec.py; pinned against pgvector's own known answers by tests/test_sparse_model_cpu.py).

  pair_distance      sparsevec.c:803-1037 as the C loops run: one sequential merge, every product and sum rounded to fp32,
                     then the operator's float8 -- <-> sqrt((double) sum), <#> (double) -sum, <=> 1 - clamp(sum /
                     sqrt((double) na * (double) nb)), <+> (double) sum
  SparseModel        the same four values for one query against a whole CSR corpus, vectorised and summed in float64.  On data
                     whose fp32 sums are exact in any order (small integers) that is pair_distance bit for bit -- which
                     test_sparse_model_cpu.py checks -- and on real data it is the more accurate of the two
  topk               (float32 distance, NaN last, document_id, block_id)

A sparse value is (indices int32 zero-based ascending, values float32); a corpus is CSR: indptr, indices, values, dim."""
import numpy as np

METRICS = ["l2", "ip", "cosine", "l1"]
F = np.float32


def pair_distance(metric, ai, ax, bi, bx):
    """The operator's float8 for one pair, in pgvector's order of operations."""
    ai, bi = np.asarray(ai, dtype=np.int64), np.asarray(bi, dtype=np.int64)
    ax, bx = np.asarray(ax, dtype=F), np.asarray(bx, dtype=F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        distance = F(0.0)
        bpos = 0
        if metric in ("l2", "l1"):
            term = (lambda v: v * v) if metric == "l2" else (lambda v: F(abs(v)))
            for i in range(ai.size):
                a_i, b_i = ai[i], -1
                for j in range(bpos, bi.size):
                    b_i = bi[j]
                    if a_i == b_i:
                        distance = F(distance + term(F(ax[i] - bx[j])))
                    elif a_i > b_i:
                        distance = F(distance + term(bx[j]))
                    if a_i >= b_i:
                        bpos = j + 1
                    if b_i >= a_i:
                        break
                if a_i != b_i:
                    distance = F(distance + term(ax[i]))
            for j in range(bpos, bi.size):
                distance = F(distance + term(bx[j]))
            return float(np.sqrt(np.float64(distance))) if metric == "l2" else float(distance)
        for i in range(ai.size):
            a_i = ai[i]
            for j in range(bpos, bi.size):
                b_i = bi[j]
                if a_i == b_i:
                    distance = F(distance + F(ax[i] * bx[j]))
                if a_i >= b_i:
                    bpos = j + 1
                if b_i >= a_i:
                    break
        if metric == "ip":
            return float(-distance)
        norma = normb = F(0.0)
        for v in ax:
            norma = F(norma + F(v * v))
        for v in bx:
            normb = F(normb + F(v * v))
        sim = np.float64(distance) / np.sqrt(np.float64(norma) * np.float64(normb))
        if sim > 1:
            sim = np.float64(1.0)
        elif sim < -1:
            sim = np.float64(-1.0)
        return float(1.0 - sim)


class SparseModel:
    """A CSR corpus with its identity: the distances of one query to every row, and the library's order."""

    def __init__(self, indptr, indices, values, dim, doc=None, blk=None):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.values = np.asarray(values, dtype=F).astype(np.float64)
        self.dim = int(dim)
        n = self.n = self.indptr.size - 1
        self.doc = np.zeros(n, dtype=np.int32) if doc is None else np.asarray(doc)
        self.blk = np.arange(n, dtype=np.int64) if blk is None else np.asarray(blk)
        self.row_of = np.repeat(np.arange(n), np.diff(self.indptr))           # the row of every entry
        self.by_id = np.lexsort((self.blk, self.doc))                         # the tie order, computed once
        with np.errstate(over="ignore"):
            self.norm2 = self._per_row(self.values * self.values).astype(F)   # pgvector's fp32 norma

    def _per_row(self, w):
        return np.bincount(self.row_of, weights=w, minlength=self.n) if self.row_of.size else np.zeros(self.n)

    def row(self, r):
        lo, hi = self.indptr[r], self.indptr[r + 1]
        return self.indices[lo:hi].astype(np.int32), self.values[lo:hi].astype(F)

    def distances(self, metric, qi, qx):
        """float32 operator values [n] (as the library reports them) of the query against every row."""
        qi = np.asarray(qi, dtype=np.int64)
        qx = np.asarray(qx, dtype=F).astype(np.float64)
        if qi.size:
            pos = np.minimum(np.searchsorted(qi, self.indices), qi.size - 1)
            hit = qi[pos] == self.indices                                     # the row entry meets a query entry
            b = np.where(hit, qx[pos], 0.0)
        else:
            hit = np.zeros(self.indices.size, dtype=bool)
            b = np.zeros(self.indices.size)
        a = self.values
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if metric == "l2":
                rest = (qx * qx).sum() - self._per_row(np.where(hit, b * b, 0.0))     # the query entries no row entry met
                s = self._per_row((a - b) ** 2) + np.maximum(rest, 0.0)             # (two orders of one sum: never below 0)
                return np.sqrt(s.astype(F).astype(np.float64)).astype(F)
            if metric == "l1":
                rest = np.abs(qx).sum() - self._per_row(np.where(hit, np.abs(b), 0.0))
                s = self._per_row(np.abs(a - b)) + np.maximum(rest, 0.0)
                return s.astype(F)
            ip = self._per_row(a * b).astype(F)
            if metric == "ip":
                return -ip
            qn = F((qx * qx).sum())
            sim = ip.astype(np.float64) / np.sqrt(self.norm2.astype(np.float64) * np.float64(qn))
            sim = np.where(sim > 1, 1.0, np.where(sim < -1, -1.0, sim))       # (NaN stays NaN)
            return (1.0 - sim).astype(F)

    def topk(self, dist, k, mask=None):
        """(caller row indices, float32 distances) of the k nearest permitted rows by (distance, NaN last, document_id,
        block_id): a stable sort by distance of the rows in id order (numpy sorts NaN last)."""
        dist32 = np.asarray(dist, dtype=F)
        ids = self.by_id if mask is None else self.by_id[np.asarray(mask, dtype=bool)[self.by_id]]
        order = ids[np.argsort(dist32[ids], kind="stable")][:k]
        return order, dist32[order]


def csr(rows):
    """[(indices, values), ...] -> (indptr int64, indices int32, values float32)."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, (ix, _) in enumerate(rows):
        indptr[i + 1] = indptr[i] + len(ix)
    ix = np.concatenate([np.asarray(r[0], dtype=np.int32) for r in rows]) if rows else np.zeros(0, np.int32)
    vx = np.concatenate([np.asarray(r[1], dtype=F) for r in rows]) if rows else np.zeros(0, F)
    return indptr, ix.astype(np.int32), vx.astype(F)


def user_row_mask(user, user_roles, permissions, doc):
    """rows visible to `user`: some role of the user is permitted the row's document."""
    roles = {r for u, r in user_roles if u == user}
    docs = np.asarray(sorted({d for r, d in permissions if r in roles}), dtype=np.int64)
    return np.isin(np.asarray(doc), docs)
