"""The cases of the fp32 HNSW search (K4, the ROWS_F32 branch of hnsw_search_body, csrc/vsr_hnsw.h) at its row, graph and launch
edges, generated deterministically for tests/test_hnsw_search_edges_cpu.py and tests/test_gpu_hnsw_search_edges.py.

A case is (rows, metric, m, ef_construction, seed, queries, (k, ef) pairs): the index oracle builds the graph of `rows`, the GPU
loads its export, and every query is searched with every (k, ef) pair.

Every fp32 sum of a case is exact in any order, so rows, distances and visited counts are compared without a tolerance:
  l2 / ip   rows and queries are small integers with dim * max_term < 2^24 (max_term: the largest square of a difference, or the
            largest product): every partial sum is an integer below 2^24.
  cosine    unit rows that fp32 holds exactly: 4^j non-zero entries of +-2^-j, j = 0 .. 3.  Entries are multiples of 2^-3, so a dot
            product is a multiple of 2^-6 in [-1, 1], again far below 24 bits.  Queries 0 and 1 are a row and the negative of a row
            (distances 0 and 2).  Queries 2 and 3 are twice a row and minus twice a row: not unit vectors, dot products of +-2, the
            one way exact rows reach the clamp of the reported distance (hnsw_reported_distance: 1 - clamp(dot)).
assert_exact() states these bounds and the generator calls it for every case."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "rows metric m ef_construction seed queries pairs")

NQ = 9
ROW_LENGTH_DIMS = (1, 2, 3, 4, 5, 127, 128, 129, 256, 260, 1000, 2000)      # chunks of four: 1, 1, 1, 1, 2, 32, 32, 33, 64, 65, 250, 500
ROW_LENGTH_IP_DIMS = (3, 129, 260, 2000)
COSINE_DIMS = (64, 260)
COSINE_SEEDS = (5264, 5468)                 # seeds whose graphs reach all 600 rows from the entry point (the CPU test asserts it)
ITERATIVE_DIMS = (3, 129, 260)
DUP_GROUPS = (2, 10, 11, 25)                # sizes of the groups of identical vectors in the "duplicates" corpus
LAUNCH_EFS = (40, 200, 1000)                # 4, 2 and 1 waves per workgroup (queries_per_workgroup below)
LAUNCH_NQS = (1, 5, 9)


def _amplitude(dim):
    """Rows are integers in [-a, a]: a wide range at the shortest rows, where 17 values per coordinate would make most rows equal."""
    return 500 if dim <= 5 else 8


def _integer_case(n, dim, metric, m, efc, seed, pairs, rows=None):
    rng = np.random.default_rng(seed)
    a = _amplitude(dim)
    if rows is None:
        rows = rng.integers(-a, a + 1, (n, dim)).astype(np.float32)
    queries = rows[rng.integers(0, len(rows), NQ)] + rng.integers(-2, 3, (NQ, dim)).astype(np.float32)
    return Case(rows, metric, m, efc, seed, queries, tuple(pairs))


def _unit_rows(rng, n, dim):
    x = np.zeros((n, dim), dtype=np.float32)
    for r in range(n):
        j = int(rng.integers(0, 4))
        at = rng.choice(dim, 4 ** j, replace=False)
        x[r, at] = rng.choice([-1.0, 1.0], 4 ** j) * 2.0 ** -j
    return x


def _cosine_case(dim, seed):
    rng = np.random.default_rng(seed)
    rows = _unit_rows(rng, 600, dim)
    queries = _unit_rows(rng, NQ, dim)
    queries[0], queries[1] = rows[17], -rows[230]                 # distances 0 and 2
    queries[2], queries[3] = 2.0 * rows[391], -2.0 * rows[54]     # dot products of +-2: the clamp
    return Case(rows, "cosine", 8, 32, seed, queries, ((10, 40), (600, 600)))     # (600, 600): every row, the antipode last


def duplicate_rows():
    """400 rows at 5 dimensions; group g of DUP_GROUPS is DUP_GROUPS[g] identical vectors, spread over the row order (rows of a
    group are 3 apart, and none is among the first 40: the reference returns a candidate list of at most m elements unsorted, so
    the first few insertions do not find their duplicates): duplicate_group_rows()."""
    rng = np.random.default_rng(5105)
    rows = rng.integers(-500, 501, (400, 5)).astype(np.float32)
    for rr in duplicate_group_rows():
        rows[rr] = rows[rr[0]]
    return rows


def duplicate_group_rows():
    return [np.arange(size) * 3 + 91 * g + 40 for g, size in enumerate(DUP_GROUPS)]


def duplicate_filter_mask():
    """The byte mask of the filtered case: every second row of each group (a strict, non-empty subset of it), and about half of the
    other rows."""
    mask = (np.random.default_rng(5106).random(400) < 0.5).astype(np.uint8)
    for rr in duplicate_group_rows():
        mask[rr] = 0
        mask[rr[::2]] = 1
    return mask


def _duplicates_case():
    rows = duplicate_rows()
    c = _integer_case(400, 5, "l2", 8, 32, 5105, ((10, 40), (40, 40)), rows=rows)
    for g, rr in enumerate(duplicate_group_rows()):               # one query at every group's vector
        c.queries[g] = rows[rr[0]]
    return c


def _cases():
    cases = {}
    for dim in ROW_LENGTH_DIMS:
        for metric in ("l2", "ip") if dim in ROW_LENGTH_IP_DIMS else ("l2",):
            n = 300 if dim >= 1000 else 600
            cases[f"rows-{metric}-{dim}"] = _integer_case(n, dim, metric, 8, 32, 5000 + dim, ((10, 40),))
    for dim, seed in zip(COSINE_DIMS, COSINE_SEEDS):
        cases[f"cosine-{dim}"] = _cosine_case(dim, seed)
    for n in (1, 2, 3):
        cases[f"graph-n{n}"] = _integer_case(n, 5, "l2", 8, 32, 5300 + n, ((10, 40), (1, 1)))
    cases["graph-n17"] = _integer_case(17, 5, "l2", 8, 32, 5317, ((40, 40), (10, 100)))
    cases["graph-m2"] = _integer_case(1500, 5, "l2", 2, 32, 5402, ((10, 40),))
    # ef_construction = 120: late insertions get lists shorter than 2 m = 200, back-links fill those of the early ones.  (pgvector
    # refuses ef_construction < 2 m; at 300 rows every list of such a build is full.  The oracle builds it all the same.)
    cases["graph-m100"] = _integer_case(300, 5, "l2", 100, 120, 5500, ((10, 40), (100, 200)))
    cases["graph-duplicates"] = _duplicates_case()
    cases["graph-k-ef"] = _integer_case(600, 5, "l2", 8, 32, 5600, ((1, 1), (1, 40), (40, 40)))
    cases["launch"] = _integer_case(1500, 16, "l2", 8, 32, 5700, ((10, 40), (100, 200), (100, 1000)))
    for name, c in cases.items():
        assert_exact(c, name)
    return cases


def exactness_bound(case):
    """dim * max_term in units of the grid the terms live on; every fp32 sum of the case is exact while this is below 2^24."""
    rows, q = case.rows.astype(np.float64), case.queries.astype(np.float64)
    dim = rows.shape[1]
    if case.metric == "cosine":                                   # entries on the 2^-3 grid, products on the 2^-6 grid
        rows, q = rows * 8.0, q * 8.0
    assert (rows == np.rint(rows)).all() and (q == np.rint(q)).all(), "entries off the grid"
    ra, qa = np.abs(rows).max(initial=0.0), np.abs(q).max(initial=0.0)
    max_term = (ra + qa) ** 2 if case.metric == "l2" else ra * qa
    return dim * max_term


def assert_exact(case, name=""):
    bound = exactness_bound(case)
    assert bound < 2 ** 24, (name, bound)
    if case.metric == "cosine":
        n2 = (case.rows.astype(np.float64) ** 2).sum(axis=1)
        assert (n2 == 1.0).all(), (name, "rows are not unit vectors")


CASES = _cases()

ROW_LENGTH_CASES = [n for n in CASES if n.startswith("rows-")]
SHORT_CASES = {"graph-n1": 1, "graph-n2": 2, "graph-n3": 3, "graph-n17": 17}     # n < k for a pair of the case: fewer than k rows


def reported_distance(metric, index_distance):
    """What the operator reports for the oracle's index distance (float8): l2_distance = sqrt, <#> = the value itself, cosine
    distance = 1 - clamp(dot), in double, then rounded to fp32."""
    d = np.asarray(index_distance, dtype=np.float64)
    if metric == "l2":
        return np.sqrt(d).astype(np.float32)
    if metric == "ip":
        return d.astype(np.float32)
    return (1.0 - np.clip(-d, -1.0, 1.0)).astype(np.float32)


# The plan of a launch, restated from csrc/vsr_hnsw.h so that the launch case keeps covering 4, 2 and 1 waves per workgroup if the
# constants move: caps (vsr_hnsw_rt.hip, hnsw_params: `p.caps = 2 * ef + 2 * h->m + 64`), hnsw_lds_fixed (`caps * 8 +
# ((caps + 15) & ~15) + HN_NBR * 8 + HN_UPPER_VISITED * 4`, rounded up to 16; HN_NBR = 256, HN_UPPER_VISITED = 1024), the LDS bitmap
# of hnsw_plan (`((n_elem + 31) / 32) * 4`) and its last line, the 40 KB rule (`lds_per_query * 4 <= 40 * 1024 ? 4 : ... * 2 ... ? 2
# : 1`; HN_LDS_BUDGET = 156 KB, vsr_hnsw_sizing.h, never binds here).
def queries_per_workgroup(n_elem, m, ef):
    caps = 2 * ef + 2 * m + 64
    fixed = (caps * 8 + ((caps + 15) & ~15) + 256 * 8 + 1024 * 4 + 15) & ~15
    lds = (fixed + (n_elem + 31) // 32 * 4 + 15) & ~15
    return 4 if lds * 4 <= 40 * 1024 else 2 if lds * 2 <= 40 * 1024 else 1


_ORACLE_INDEXES = {}


def oracle_index(oracle, name):
    """The index oracle's graph of a case, built once per process."""
    if name not in _ORACLE_INDEXES:
        from oracle.oracle import HnswIndex
        c = CASES[name]
        _ORACLE_INDEXES[name] = HnswIndex(oracle, c.metric, c.rows, m=c.m, ef_construction=c.ef_construction, seed=c.seed)
    return _ORACLE_INDEXES[name]
