"""The GPU HNSW build with identical vectors merged (vsr_hnsw_build_ex, VSR_HNSW_BUILD_MERGE_DUPLICATES) and the graph
export (vsr_hnsw_export_shape / vsr_hnsw_export).

The merge is exhaustive where pgvector's is opportunistic (include/vsrbac.h), so the TID lists are checked against the
canonical grouping -- a dict on the rows' bytes, chunked by 10 in row order -- not against the index oracle's; what is
compared with the oracle is the element count (never more than the oracle's) and recall.  m = 16, ef_construction = 64
throughout."""
import ctypes as C

import numpy as np
import pytest

from helpers import check_graph as _check_graph, same_graph as _same_graph
from oracle.oracle import HnswIndex as OracleHnsw

pytestmark = pytest.mark.gpu

M, EFC = 16, 64


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _sift_like(rng, n, dim):
    return np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)


def _plant(x, sizes, rng, ends_group=None):
    """Copies of one row at scattered places, a group per entry of `sizes`; group `ends_group` holds row 0 and the last."""
    n = len(x)
    free = rng.permutation(np.arange(1, n - 1))
    at = 0
    for gi, g in enumerate(sizes):
        rows = free[at:at + g]
        at += g
        if gi == ends_group:
            rows = np.concatenate(([0, n - 1], rows[2:]))
        x[rows] = x[rows[0]]
    return free[at:]                                   # rows no group took


_PLANTED = {}


def _planted(dim):
    """3000 SIFT-like rows with planted groups, and a pair that differs only in the sign of a zero."""
    if dim not in _PLANTED:
        rng = np.random.default_rng(4100 + dim)
        x = _sift_like(rng, 3000, dim)
        rest = _plant(x, [2, 3, 5, 10, 11, 20, 21, 25, 40], rng, ends_group=2)          # the group of 5
        a, b = int(rest[0]), int(rest[1])
        x[b] = x[a]
        x[a, dim // 2] = 0.0
        x[b, dim // 2] = -0.0
        _PLANTED[dim] = (x, a, b)
    return _PLANTED[dim]


def _canonical(x):
    """Sorted TID tuples of the exhaustive grouping: identical bytes, 10 per element, in row order."""
    groups = {}
    for r in range(len(x)):
        groups.setdefault(x[r].tobytes(), []).append(r)
    return sorted(tuple(rows[i:i + 10]) for rows in groups.values() for i in range(0, len(rows), 10))


def _tid_tuples(g):
    return [tuple(int(t) for t in g["tids"][e, :g["tid_count"][e]]) for e in range(len(g["level"]))]


_EXPORTS = {}


def _merged_export(ctx, dim):
    """(merged export, unmerged export) of _planted(dim), seed 11; built once per module."""
    if dim not in _EXPORTS:
        x, _, _ = _planted(dim)
        corpus = ctx.load_corpus(x)
        merged = corpus.build_hnsw(M, EFC, "l2", seed=11, merge_duplicates=True)
        plain = corpus.build_hnsw(M, EFC, "l2", seed=11)
        _EXPORTS[dim] = (merged.export(), plain.export())
        merged.free()
        plain.free()
        corpus.free()
    return _EXPORTS[dim]


# ---- 1. canonical grouping ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 128, 260])
def test_merged_build_groups_identical_rows_canonically(ctx, dim):
    x, a, b = _planted(dim)
    n = len(x)
    g, plain = _merged_export(ctx, dim)
    tids, tc = g["tids"], g["tid_count"]
    got = _tid_tuples(g)
    want = _canonical(x)
    print(f"dim {dim}: {n} rows -> {len(got)} elements (canonical {len(want)}), max_level {g['max_level']}")
    assert sorted(got) == want
    assert (tids[np.arange(10)[None, :] >= tc[:, None]] == -1).all()
    assert (np.diff(tids[:, 0]) > 0).all(), "elements are numbered by their first member"
    elem_of = {t: e for e, ts in enumerate(got) for t in ts}
    assert elem_of[0] == elem_of[n - 1]
    assert elem_of[a] != elem_of[b], "+0.0 and -0.0 are different bytes"
    assert len(plain["level"]) == n and (plain["tid_count"] == 1).all() and (plain["tids"][:, 0] == np.arange(n)).all()
    assert (g["level"] == plain["level"][tids[:, 0]]).all()
    _check_graph(g)
    _check_graph(plain)


@pytest.fixture(scope="module")
def dup4000(oracle):
    rng = np.random.default_rng(4216)
    x = _sift_like(rng, 4000, 16)
    _plant(x, [2] * 50 + [10] * 10 + [4] * 20, rng)
    return x, OracleHnsw(oracle, "l2", x, m=M, ef_construction=EFC, seed=9)


def test_merged_build_has_no_more_elements_than_the_serial_build(ctx, dup4000):
    x, ref = dup4000
    corpus = ctx.load_corpus(x)
    gpu = corpus.build_hnsw(M, EFC, "l2", seed=9, merge_duplicates=True)
    g = gpu.export()
    want = _canonical(x)
    print(f"4000 x 16: GPU {len(g['level'])} elements, canonical {len(want)}, oracle {ref.n_elem}")
    assert sorted(_tid_tuples(g)) == want
    assert gpu.info()[0] == len(g["level"]) <= ref.n_elem
    _check_graph(g)
    gpu.free()
    corpus.free()


# ---- 2. why it matters: ef_search bounds elements, not rows --------------------------------------------------------------
def _recall_by_distance(x, q, rows, k):
    """Share of the returned rows that are no further than the exact k-th distance (integer-valued rows: exact in float64)."""
    hit = 0
    for i in range(len(q)):
        d_all = ((x.astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(axis=1)
        kth = np.partition(d_all, k - 1)[k - 1]
        hit += int((d_all[rows[i]] <= kth).sum())
    return hit / (len(q) * k)


def test_merged_build_returns_k_rows_where_the_unmerged_one_cannot(ctx, oracle):
    rng = np.random.default_rng(77)
    base = _sift_like(rng, 1500, 16)
    x = np.repeat(base, 8, axis=0)[rng.permutation(12_000)]
    n, dim, k, ef = len(x), 16, 100, 40
    q = x[rng.integers(0, n, 30)] + rng.integers(-3, 4, (30, dim)).astype(np.float32)
    corpus = ctx.load_corpus(x)
    merged = corpus.build_hnsw(M, EFC, "l2", seed=9, merge_duplicates=True)
    got, _ = merged.search(q, k, ef, "l2")
    ref = OracleHnsw(oracle, "l2", x, m=M, ef_construction=EFC, seed=9)
    ref_rows = [ref.search(q[i], ef)[0][:k] for i in range(len(q))]
    r_ref = _recall_by_distance(x, q, ref_rows, k)
    print(f"merged: {merged.info()[0]} elements (oracle {ref.n_elem}), counts {got.counts.min()} .. {got.counts.max()}")
    assert (got.counts == k).all()
    r_gpu = _recall_by_distance(x, q, [got.rows[i][:k] for i in range(len(q))], k)
    print(f"recall@{k} by distance at ef_search = {ef}: GPU merged {r_gpu:.4f}, serial port {r_ref:.4f}")
    assert r_gpu >= r_ref - 0.02, (r_gpu, r_ref)
    assert merged.info()[0] <= ref.n_elem
    plain = corpus.build_hnsw(M, EFC, "l2", seed=9)
    res, _ = plain.search(q, k, ef, "l2")
    print(f"unmerged: {plain.info()[0]} elements, counts {res.counts.min()} .. {res.counts.max()}")
    assert plain.info()[0] == n
    assert (res.counts <= ef).all()
    for h in (merged, plain):
        h.free()
    corpus.free()


# ---- 3. export and load round trip ---------------------------------------------------------------------------------
def test_export_of_a_loaded_graph_is_the_graph(ctx, dup4000):
    x, ref = dup4000
    want = ref.export()
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_hnsw(want)
    _same_graph(gpu.export(), want)
    gpu.free()
    corpus.free()


def test_a_built_graph_survives_export_and_load(ctx, dup4000):
    x, _ = dup4000
    rng = np.random.default_rng(4301)
    n = len(x)
    q = x[rng.integers(0, n, 24)] + rng.integers(-3, 4, (24, x.shape[1])).astype(np.float32)
    corpus = ctx.load_corpus(x)
    built = corpus.build_hnsw(M, EFC, "l2", seed=9, merge_duplicates=True)
    g = built.export()
    loaded = corpus.load_hnsw(g)
    _same_graph(loaded.export(), g)
    assert loaded.info() == built.info()
    flt = corpus.filter_from_bytemask((rng.random(n) < 0.3).astype(np.uint8))
    for filters in (None, [flt] * len(q)):
        for ef in (10, 40):
            a, va = built.search(q, 20, ef, "l2", filters)
            b, vb = loaded.search(q, 20, ef, "l2", filters)
            for name in ("rows", "dist", "counts", "block_ids", "doc_ids"):
                np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=f"{name} ef={ef}")
            np.testing.assert_array_equal(va, vb)
            assert (a.counts > 0).all()
    a, ta = built.search_iterative(q, 20, 40, "l2", [flt] * len(q), "relaxed_order", 20000)
    b, tb = loaded.search_iterative(q, 20, 40, "l2", [flt] * len(q), "relaxed_order", 20000)
    for name in ("rows", "dist", "counts"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    np.testing.assert_array_equal(ta, tb)
    assert (a.counts == 20).all()
    for h in (built, loaded):
        h.free()
    corpus.free()


def test_exported_tids_are_caller_rows_under_a_permuted_corpus(ctx, dup4000):
    x, _ = dup4000
    n = len(x)
    rng = np.random.default_rng(4302)
    doc = rng.integers(1, 40, n).astype(np.int32)                         # internal order: (document, block), not the caller's
    blk = rng.permutation(n).astype(np.int64) + 1
    corpus = ctx.load_corpus(x, blk, doc)
    gpu = corpus.build_hnsw(M, EFC, "l2", seed=9, merge_duplicates=True)
    g = gpu.export()
    tids, tc = g["tids"], g["tid_count"]
    assert len(g["level"]) == len(_canonical(x))
    seen = np.zeros(n, dtype=np.int64)
    for e in range(len(tc)):
        rows = tids[e, :tc[e]]
        assert (tids[e, tc[e]:] == -1).all()
        assert all(x[r].tobytes() == x[rows[0]].tobytes() for r in rows), e
        seen[rows] += 1
    assert (seen == 1).all(), "every caller row is in exactly one element"
    loaded = corpus.load_hnsw(g)
    _same_graph(loaded.export(), g)
    for h in (gpu, loaded):
        h.free()
    corpus.free()


# ---- 4. degenerate shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,sizes", [(37, [10, 10, 10, 7]), (11, [10, 1]), (1, [1])])
def test_identical_rows_only(ctx, n, sizes):
    x = np.tile(np.array([[3.0, 1.0, 4.0]], dtype=np.float32), (n, 1))
    corpus = ctx.load_corpus(x)
    gpu = corpus.build_hnsw(M, EFC, "l2", seed=2, merge_duplicates=True)
    g = gpu.export()
    assert g["tid_count"].tolist() == sizes
    assert [t for ts in _tid_tuples(g) for t in ts] == list(range(n))
    _check_graph(g)
    res, _ = gpu.search(x[:1], n, 10, "l2")
    assert res.counts[0] == n
    assert sorted(res.rows[0].tolist()) == list(range(n))
    assert (res.dist[0] == 0.0).all()
    gpu.free()
    corpus.free()


# ---- 5. the collision path -----------------------------------------------------------------------------------------
def test_hash_collisions_change_nothing(ctx, monkeypatch):
    x, _, _ = _planted(128)
    g, _ = _merged_export(ctx, 128)
    monkeypatch.setenv("VSR_HNSW_DEDUP_HASH_BITS", "8")                   # 3000 rows in 256 hash values: every run collides
    corpus = ctx.load_corpus(x)
    gpu = corpus.build_hnsw(M, EFC, "l2", seed=11, merge_duplicates=True)
    g8 = gpu.export()
    monkeypatch.delenv("VSR_HNSW_DEDUP_HASH_BITS")
    assert _tid_tuples(g8) == _tid_tuples(g)
    assert sorted(_tid_tuples(g8)) == _canonical(x)
    np.testing.assert_array_equal(g8["level"], g["level"])
    gpu.free()
    corpus.free()


# ---- 6. arguments --------------------------------------------------------------------------------------------------
def test_arguments(ctx, dup4000):
    import vsrbac
    from vsrbac import _ffi
    lib = vsrbac.load_library()
    x, ref = dup4000
    corpus = ctx.load_corpus(x[:200])
    h = C.c_void_p()
    for flags in (2, 1 | 4, 0x80000000):
        assert lib.vsr_hnsw_build_ex(corpus._h, M, EFC, vsrbac.L2, 1, flags, C.byref(h)) == _ffi.ERR_INVALID
        assert not h.value
    assert lib.vsr_hnsw_build_ex(None, M, EFC, vsrbac.L2, 1, 1, C.byref(h)) == _ffi.ERR_INVALID
    assert lib.vsr_hnsw_build_ex(corpus._h, M, EFC, vsrbac.L2, 1, 1, None) == _ffi.ERR_INVALID
    v = [C.c_int32() for _ in range(5)]
    assert lib.vsr_hnsw_export_shape(None, *[C.byref(a) for a in v]) == _ffi.ERR_INVALID
    gpu = corpus.build_hnsw(M, EFC, "l2", seed=1, merge_duplicates=True)
    good = gpu.export()
    arrays = [good[name] for name in ("level", "nbr0", "tid_count", "tids", "up_slot", "up_nbr")]
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    assert (good["up_slot"] >= 0).any()                                   # (so that up_nbr is not optional here)
    assert lib.vsr_hnsw_export(None, *ptrs) == _ffi.ERR_INVALID
    for hole in range(len(ptrs)):
        args = [None if i == hole else p for i, p in enumerate(ptrs)]
        assert lib.vsr_hnsw_export(gpu._h, *args) == _ffi.ERR_INVALID, hole
    assert lib.vsr_hnsw_export_shape(gpu._h, None, None, None, None, None) == _ffi.OK
    gpu.free()
    corpus.free()
    # a loaded graph reports the shape it was loaded with
    want = ref.export()
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_hnsw(want)
    assert lib.vsr_hnsw_export_shape(gpu._h, *[C.byref(a) for a in v]) == _ffi.OK
    assert [a.value for a in v] == [M, ref.n_elem, ref.entry, ref.n_upper, want["max_level"]]
    assert ref.n_upper == int((want["up_slot"] >= 0).sum()) > 0
    gpu.free()
    corpus.free()
