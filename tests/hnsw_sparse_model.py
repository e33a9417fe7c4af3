"""pgvector's HNSW scan over a sparsevec column restated in numpy (the contract of vsr_hnsw_search_sparse*, include/vsrbac.h),
and numpy restatements of sparsevec_l2_norm / sparsevec_l2_normalize (vsr_sparse_norms / vsr_sparse_l2_normalize).

The walk is tests/hnsw_iterative_model.py's, unchanged: descent, layer-0 beam, discarded set, iterative rounds, the
(distance, element id) tie rule.  Only the per-element distance differs -- the sparsevec opclasses (hnswutils.c:1352-1361,
1411-1422) over CSR rows, with tests/sparse_model.py's sums:

  l2       squared L2                      reported sqrt((double) d)
  l1       the L1 sum                      reported as it is
  ip       the negated inner product       reported as it is
  cosine   the negated inner product       reported 1 - clamp(dot): the caller loads unit rows and passes unit queries

held as the fp32 value the GPU keys carry, so that ties are the GPU's ties.  The sums run in float64 and are rounded once: on
integer-valued data (every partial sum exact in fp32) that is the GPU's value bit for bit, and the index oracle on the
densified rows gives the same walk (tests/test_hnsw_sparse_cpu.py pins this model to it).  Mode "off" is the plain search."""
import numpy as np

from hnsw_iterative_model import Graph, IterativeScan
from sparse_model import SparseModel

F = np.float32
METRICS = ["l2", "ip", "cosine", "l1"]
HNSW_MAX_NNZ = 1000


def densify(indptr, indices, values, dim):
    """CSR rows as a dense float32 [n, dim] array (affordable at the shapes of the tests)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    x = np.zeros((n, int(dim)), dtype=F)
    x[np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices, dtype=np.int64)] = np.asarray(values, dtype=F)
    return x


def sparsify(x):
    """Dense rows -> (indptr int64, indices int32, values float32, dim): the entries that are not zero."""
    x = np.atleast_2d(np.asarray(x, dtype=F))
    nz = x != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(nz)
    return indptr, cols.astype(np.int32), x[rows, cols].astype(F), x.shape[1]


def take_rows(csr, rows):
    """The CSR triple of the listed rows, in that order."""
    indptr, indices, values, dim = csr
    rows = np.asarray(rows, dtype=np.int64)
    lens = indptr[rows + 1] - indptr[rows]
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sel = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows]) if rows.size else np.zeros(0, dtype=np.int64)
    sel = sel.astype(np.int64)
    return out_ptr, np.asarray(indices)[sel].astype(np.int32), np.asarray(values)[sel].astype(F), dim


def index_distances(model, metric, qi, qx):
    """fp32 index distances of every row of a SparseModel to the query (indices, values), as float64 images of the fp32 values."""
    qi = np.asarray(qi, dtype=np.int64)
    qx = np.asarray(qx, dtype=F).astype(np.float64)
    if qi.size:
        pos = np.minimum(np.searchsorted(qi, model.indices), qi.size - 1)
        hit = qi[pos] == model.indices
        b = np.where(hit, qx[pos], 0.0)
    else:
        hit = np.zeros(model.indices.size, dtype=bool)
        b = np.zeros(model.indices.size)
    a = model.values
    if metric == "l2":
        rest = (qx * qx).sum() - model._per_row(np.where(hit, b * b, 0.0))
        s = model._per_row((a - b) ** 2).astype(F) + np.maximum(rest, 0.0).astype(F)
    elif metric == "l1":
        rest = np.abs(qx).sum() - model._per_row(np.where(hit, np.abs(b), 0.0))
        s = model._per_row(np.abs(a - b)).astype(F) + np.maximum(rest, 0.0).astype(F)
    else:
        s = -model._per_row(a * b).astype(F)
    return s.astype(F).astype(np.float64)


def reported(metric, d):
    """The float32 distances a search reports for fp32 index distances d (K4's rule, and L1 as it is)."""
    d = np.asarray(d, dtype=np.float64)
    if metric == "l2":
        return np.sqrt(d).astype(F)
    if metric == "cosine":
        return (1.0 - np.clip(-d, -1.0, 1.0)).astype(F)
    return d.astype(F)


class SparseGraph(Graph):
    """The export() arrays of a graph over CSR rows (caller row order)."""

    def __init__(self, g, indptr, indices, values, dim):
        super().__init__(g, np.zeros((0, 1), dtype=F))                        # (the walk never reads dense rows)
        self.dim = int(dim)
        self.csr = (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), np.asarray(values, dtype=F), self.dim)
        ep, ei, ev, _ = take_rows(self.csr, self.elem_row)                    # one row per element: its first TID's
        self.elem_model = SparseModel(ep, ei, ev, dim)


class SparseScan(IterativeScan):
    """IterativeScan over a SparseGraph: (row, fp32 index distance, T at emission) of one query's stream."""

    def __init__(self, g, qi, qx, ef, metric="l2", mode="off", max_scan_tuples=20000):
        assert metric in METRICS and mode in ("off", "relaxed_order", "strict_order")
        self.g, self.ef, self.mode, self.max_scan = g, int(ef), mode, int(max_scan_tuples)
        self.dist = index_distances(g.elem_model, metric, qi, qx).tolist()
        self.tuples = 0


def search(g, qi, qx, ef, metric="l2"):
    """The plain search of one query: (rows in emission order, fp32 index distances as float64, visited count)."""
    scan = SparseScan(g, qi, qx, ef, metric, "off")
    got = list(scan)
    return (np.array([r for r, _, _ in got], dtype=np.int64), np.array([d for _, d, _ in got], dtype=np.float64), scan.tuples)


# ---- sparsevec_l2_norm / sparsevec_l2_normalize ------------------------------------------------------------------------------
def l2_norms(indptr, values):
    """sparsevec.c:1044-1055 per row: a double sum of double products in entry order, then sqrt."""
    indptr = np.asarray(indptr, dtype=np.int64)
    values = np.asarray(values, dtype=F)
    out = np.zeros(indptr.size - 1, dtype=np.float64)
    for r in range(out.size):
        norm = 0.0
        for v in values[indptr[r]:indptr[r + 1]].tolist():                    # (Python floats: IEEE doubles, one rounding per step)
            norm += v * v
        out[r] = np.sqrt(norm)
    return out


def l2_normalize(indptr, indices, values, dim):
    """sparsevec.c:1060-1120 per row: (float) (v / norm) with the norm in double; a zero norm leaves the row as it is; entries
    that became 0 are dropped; OverflowError for an infinite result.  Returns (indptr, indices, values, dim, dropped)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    values = np.asarray(values, dtype=F)
    norms = l2_norms(indptr, values)
    out_ptr, out_idx, out_val, dropped = [0], [], [], 0
    for r in range(norms.size):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        v = values[lo:hi]
        if norms[r] > 0:
            with np.errstate(over="ignore", invalid="ignore"):
                v = (v.astype(np.float64) / norms[r]).astype(F)
            if np.isinf(v).any():
                raise OverflowError("value out of range: overflow")
            keep = v != 0
            dropped += int((~keep).sum())
        else:
            keep = np.ones(hi - lo, dtype=bool)
        out_idx.append(indices[lo:hi][keep])
        out_val.append(v[keep])
        out_ptr.append(out_ptr[-1] + int(keep.sum()))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return np.asarray(out_ptr, dtype=np.int64), cat(out_idx, np.int32), cat(out_val, F), int(dim), dropped


# ---- pgvector's recall TAP case ---------------------------------------------------------------------------------------------
def tie_aware_expected(dist_row, limit):
    """Every row no farther than the limit-th nearest."""
    d = np.asarray(dist_row)
    kth = np.sort(d, kind="stable")[min(limit, d.size) - 1]
    return np.flatnonzero(d <= kth)


def tap_recall(found_rows_per_query, expected_per_query, limit):
    """028_hnsw_sparsevec_build_recall.pl:13-47: returned ids found in the expected set, over queries x limit."""
    correct = sum(int(np.isin(f[:limit], e).sum()) for f, e in zip(found_rows_per_query, expected_per_query))
    return correct / (len(found_rows_per_query) * limit)


def tap_case(seed=28):
    """The set-up of 028_hnsw_sparsevec_build_recall.pl: 10 000 rows of 3 dimensions, random() * random() each, 20 queries of
    three random() values; LIMIT 20, ef_search 40 (the default), m = 16, ef_construction = 64.  (dense rows, dense queries, limit,
    ef).  One fixed seed: the CPU floor test and the GPU build test share the rows."""
    rng = np.random.default_rng(seed)
    rows = (rng.random((10_000, 3)) * rng.random((10_000, 3))).astype(F)
    queries = rng.random((20, 3)).astype(F)
    return rows, queries, 20, 40


def unit_rows(x):
    """Dense rows scaled to unit length the way sparsevec_l2_normalize scales them (zero rows stay zero)."""
    x = np.asarray(x, dtype=F)
    ip, ix, vx, dim = sparsify(x)
    return densify(*l2_normalize(ip, ix, vx, dim)[:4])
