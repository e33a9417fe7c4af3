"""vsr_hnsw_build_partitions (Corpus.build_hnsw_partitions): the HNSW graphs of many row subsets of one corpus in one call.

The contract is equality with the standalone build: partition g's export is, array for array, the export of build_hnsw* with the
same m, ef_construction, metric and seed over a corpus that holds only g's rows with their (document_id, block_id), the heap TIDs
mapped through the partition's row list.  Both sides run the same kernels' arithmetic, so the comparison is exact on any rows;
the rows are small integers all the same (every distance exact, as in tests/test_gpu_hnsw_build_model.py), which keeps a failure
readable.  The standalone exports are built once per (kind, metric, m, ef_construction) and shared.  The schedule that packs the
partitions' batches into rounds is pinned without a GPU by tests/test_hnsw_forest_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from helpers import check_built_graph, same_graph
from hnsw_half_model import to_half

pytestmark = pytest.mark.gpu

N, SEED = 3000, 41
SIZES = [0, 1, 2, 17, 129, 700, 1500]                                           # the issue's partitions
KINDS = [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming")]


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class World:
    """3000 rows with shuffled document and block ids, and the seven row lists: unsorted, overlapping."""

    def __init__(self):
        rng = np.random.default_rng(9100)
        self.rows = {"f32": rng.integers(-8, 9, (N, 16)).astype(np.float32),   # 4 * 16 * 64 < 2^24: sums are exact
                     "bit": rng.integers(0, 2, (N, 64)).astype(np.float32)}    # 64-bit rows
        self.rows["half"] = self.rows["f32"]                                    # small integers are binary16 values
        self.real = rng.normal(size=(N, 16)).astype(np.float32)
        self.doc = rng.permutation(np.arange(N) // 4 + 1).astype(np.int32)     # 750 documents of 4 blocks, shuffled
        self.blk = (rng.permutation(N) + 1).astype(np.int64)
        self.parts = [rng.choice(N, n, replace=False).astype(np.int64) for n in SIZES]
        assert np.intersect1d(self.parts[5], self.parts[6]).size > 0 and (np.diff(self.parts[6]) < 0).any()
        # the caller row of every element: a partition's rows in internal (document_id, block_id) order
        self.order = [p[np.lexsort((self.blk[p], self.doc[p]))] for p in self.parts]
        self.perms = np.array([(r, d) for r in (1, 2, 3) for d in range(1, N // 4 + 2) if d % (r + 1) == 0], dtype=np.int32)
        self.user_roles = np.array([(1, 1), (2, 2), (2, 3)], dtype=np.int32)


@pytest.fixture(scope="module")
def world():
    return World()


def _load(ctx, kind, x, blk, doc):
    if kind == "f32":
        return ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32), blk, doc)
    if kind == "half":
        return ctx.load_corpus_half(to_half(x), blk, doc)
    return ctx.load_corpus_bit(np.asarray(x) != 0, None, blk, doc)


def _build_one(corpus, kind, m, efc, metric, seed=SEED):
    fn = {"f32": corpus.build_hnsw, "half": corpus.build_hnsw_half, "bit": corpus.build_hnsw_bit}[kind]
    return fn(m, efc, metric, seed=seed)


_STANDALONE = {}


def _standalone(ctx, world, kind, metric, m, efc, x=None):
    """Per partition: the export of the standalone build over a sub-corpus of its rows, TIDs mapped to rows of the whole corpus."""
    key = (kind, metric, m, efc, x is None)
    if key not in _STANDALONE:
        rows = world.rows[kind] if x is None else x
        out = []
        for p in world.parts:
            sub = _load(ctx, kind, rows[p], world.blk[p], world.doc[p])
            index = _build_one(sub, kind, m, efc, metric)
            g = index.export()
            g["tids"] = np.where(g["tids"] >= 0, p[np.maximum(g["tids"], 0)], -1)
            out.append(g)
            index.free()
            sub.free()
        ctx.screening_check(0)
        _STANDALONE[key] = out
    return _STANDALONE[key]


def _forest(ctx, world, kind, metric, m, efc, x=None, parts=None):
    corpus = _load(ctx, kind, world.rows[kind] if x is None else x, world.blk, world.doc)
    indexes = corpus.build_hnsw_partitions(world.parts if parts is None else parts, m, efc, metric, SEED)
    ctx.screening_check(0)                                                      # fails on a guard word that is not as it was found
    out = [h.export() for h in indexes]
    infos = [(h.info(), h.device_bytes()) for h in indexes]
    for h in indexes:
        h.free()
    corpus.free()
    return out, infos


def _same_forest(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        try:
            same_graph(a, b)
        except AssertionError as e:
            raise AssertionError(f"partition {g} ({len(b['level'])} elements): {e}") from None


# ---- 1: equality with the standalone builds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", KINDS)
def test_every_partition_is_the_standalone_build(ctx, world, kind, metric):
    m, efc = 8, 32
    want = _standalone(ctx, world, kind, metric, m, efc)
    got, infos = _forest(ctx, world, kind, metric, m, efc)
    _same_forest(got, want)
    for g, (p, order, a) in enumerate(zip(world.parts, world.order, got)):
        assert len(a["level"]) == len(p) and infos[g][0][0] == len(p)
        np.testing.assert_array_equal(a["tids"][:, 0], order)                  # element e: the e-th row in (document_id, block_id) order
        assert (a["tid_count"] == 1).all() and (a["tids"][:, 1:] == -1).all()
        if len(p) > 1:
            check_built_graph(a, m)
    assert got[0]["entry"] == -1 and got[0]["max_level"] == 1 and infos[0][0] == (0, -1, -1, 1) and infos[0][1] == 0
    assert got[1]["entry"] == 0 and (got[1]["nbr0"] == -1).all()


# ---- 2: the packing into rounds does not change a graph ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ["1", "5"])
def test_round_cap_does_not_change_any_graph(ctx, world, monkeypatch, cap):
    want, _ = _forest(ctx, world, "f32", "l2", 8, 32)
    monkeypatch.setenv("VSR_HNSW_FOREST_BATCH", cap)
    got, _ = _forest(ctx, world, "f32", "l2", 8, 32)
    monkeypatch.delenv("VSR_HNSW_FOREST_BATCH")
    _same_forest(got, want)
    for a, b in zip(got, want):
        for key in ("level", "nbr0", "tids", "up_slot", "up_nbr"):
            assert a[key].tobytes() == b[key].tobytes(), key


# ---- 3: a visited-table overflow restarts the whole call ---------------------------------------------------------------------------
def test_visited_table_overflow_restarts_the_call(ctx, world, monkeypatch):
    """256 slots overflow once a layer search has visited more than 192 elements.  At ef_construction = 64 the search of an element
    of the 1500-row partition keeps 64 in W alone and expands each of them over lists of up to 16: the first attempts stop early,
    and only a restart that begins every graph again can give the standalone builds' graphs."""
    m, efc = 8, 64
    want = _standalone(ctx, world, "f32", "l2", m, efc)
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "256")
    got, _ = _forest(ctx, world, "f32", "l2", m, efc)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    _same_forest(got, want)


# ---- 4: graphs of different heights -------------------------------------------------------------------------------------------------
def test_partitions_of_different_heights_keep_their_own_stride(ctx, world):
    m, efc = 4, 16
    want = _standalone(ctx, world, "f32", "l2", m, efc)
    heights = [g["max_level"] for g in want]
    assert len(set(heights)) > 1, heights                                       # else the re-striding of the upper lists is not exercised
    got, infos = _forest(ctx, world, "f32", "l2", m, efc)
    _same_forest(got, want)
    assert [i[0][3] for i in infos] == heights
    assert [a["up_nbr"].shape[1] for a in got] == heights


# ---- 5: a partition index answers like the standalone index ------------------------------------------------------------------------
def _mapped(res, rows):
    """A SearchResult of the standalone index with its rows as rows of the whole corpus."""
    return np.where(res.rows >= 0, rows[np.maximum(res.rows, 0)], -1)


@pytest.mark.parametrize("g", [4, 5])
def test_partition_index_searches_like_the_standalone_index(ctx, world, g):
    m, efc, k = 8, 32, 10
    x, p = world.rows["f32"], world.parts[g]
    rng = np.random.default_rng(9200 + g)
    q = x[rng.integers(0, N, 9)] + rng.integers(-2, 3, (9, 16)).astype(np.float32)
    corpus = _load(ctx, "f32", x, world.blk, world.doc)
    corpus.load_rbac(world.user_roles, world.perms)
    index = corpus.build_hnsw_partitions(world.parts, m, efc, "l2", SEED)[g]
    sub = _load(ctx, "f32", x[p], world.blk[p], world.doc[p])
    sub.load_rbac(world.user_roles, world.perms)
    alone = _build_one(sub, "f32", m, efc, "l2")
    assert index.device_bytes() == alone.device_bytes() and index.info() == alone.info()
    role, role_alone = corpus.filter_for_roles([1]), sub.filter_for_roles([1])
    assert 0 < role_alone.allowed_rows < len(p)
    for ef in (40, 1000):                                                       # 1000 >= the partition's size: the whole graph is the beam
        for f, fa in ((None, None), ([role] * 9, [role_alone] * 9)):
            (res, vis), (want, want_vis) = index.search(q, k, ef, "l2", f), alone.search(q, k, ef, "l2", fa)
            assert np.isin(res.rows[res.rows >= 0], p).all(), "a row outside the partition"
            np.testing.assert_array_equal(res.rows, _mapped(want, p))
            np.testing.assert_array_equal(res.dist, want.dist)
            np.testing.assert_array_equal(res.counts, want.counts)
            np.testing.assert_array_equal(res.block_ids, want.block_ids)
            np.testing.assert_array_equal(res.doc_ids, want.doc_ids)
            np.testing.assert_array_equal(vis, want_vis)
            if ef == 1000 and f is None:
                assert (res.counts == min(k, len(p))).all()
    for h in (index, alone):
        h.set_predicate_aware(True)
    (res, vis), (want, want_vis) = index.search(q, k, 40, "l2", [role] * 9), alone.search(q, k, 40, "l2", [role_alone] * 9)
    np.testing.assert_array_equal(res.rows, _mapped(want, p))
    np.testing.assert_array_equal(vis, want_vis)
    for h in (index, alone):
        h.set_predicate_aware(False)
    (res, tup), (want, want_tup) = (index.search_iterative(q, k, 20, "l2", [role] * 9, "relaxed_order"),
                                    alone.search_iterative(q, k, 20, "l2", [role_alone] * 9, "relaxed_order"))
    np.testing.assert_array_equal(res.rows, _mapped(want, p))
    np.testing.assert_array_equal(res.dist, want.dist)
    np.testing.assert_array_equal(res.counts, want.counts)
    np.testing.assert_array_equal(tup, want_tup)
    ctx.screening_check(0)
    again = corpus.load_hnsw(index.export())                                    # an ordinary index: its export loads
    np.testing.assert_array_equal(again.search(q, k, 40, "l2")[0].rows, index.search(q, k, 40, "l2")[0].rows)
    for h in (again, index, alone):
        h.free()
    sub.free()
    corpus.free()


# ---- 6: determinism on real-valued rows -----------------------------------------------------------------------------------------------
def test_two_calls_on_real_valued_rows_agree(ctx, world):
    a, _ = _forest(ctx, world, "f32", "l2", 8, 32, x=world.real)
    b, _ = _forest(ctx, world, "f32", "l2", 8, 32, x=world.real)
    _same_forest(a, b)
    _same_forest(a, _standalone(ctx, world, "f32", "l2", 8, 32, x=world.real))   # same kernels, same sums: equal here too


# ---- 7: the deployment's spelling -----------------------------------------------------------------------------------------------------
def test_deployment_builds_one_index_per_partition(ctx, world):
    from vsrbac.harness import Deployment
    x = world.rows["f32"]
    dep = Deployment(ctx, x, world.blk, world.doc, world.user_roles, world.perms)
    partition_docs = {7: [3, 1, 2, 500], 2: [], 9: list(range(100, 160)) + [1]}
    dep.load_partitions(partition_docs, {(1,): [7, 9]})
    graphs = dep.build_partition_hnsw(m=8, ef_construction=32, seed=SEED)
    assert sorted(graphs) == [2, 7, 9]
    pids = sorted(partition_docs)
    parts = [np.flatnonzero(np.isin(world.doc, partition_docs[p])) for p in pids]
    assert [len(p) for p in parts] == [0, 16, 244]
    want, _ = _forest(ctx, world, "f32", "l2", 8, 32, parts=parts)
    _same_forest([graphs[p].export() for p in pids], want)
    for h in graphs.values():
        h.free()
    dep.close()


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------------
def _raises(status, fragment, fn, *args, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError, match=fragment) as info:
        fn(*args, **kw)
    assert info.value.status == status, (info.value.status, status)


def _raw(corpus, off, rows, m=8, efc=32, metric=0, flags=0, n_parts=None, out=True, sentinel=0xDEAD0):
    """The C call itself; returns the out array, every slot preset to a sentinel so that a refusal must have cleared it."""
    from vsrbac._ffi import load_library
    from vsrbac.engine import _ptr, check
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    n = (len(off) - 1 if off is not None else 0) if n_parts is None else n_parts
    handles = (C.c_void_p * max(n, 1))(*([sentinel] * max(n, 1)))
    try:
        check(load_library().vsr_hnsw_build_partitions(corpus._h if corpus is not None else None, n, _ptr(off), _ptr(rows), m, efc, metric,
                                                       SEED, flags, handles if out else None))
    except Exception:
        if out:
            assert all(handles[g] is None for g in range(n)), "a refusal left an out[g] that is not NULL"
        raise
    return handles


def test_refusals_leave_every_out_null(ctx, world, monkeypatch):
    from vsrbac import _ffi
    x = world.rows["f32"][:400]
    corpus = _load(ctx, "f32", x, None, None)
    off, rows = [0, 3, 3, 8], [5, 6, 7, 1, 2, 3, 4, 5]                          # row 5 in two partitions: allowed
    handles = _raw(corpus, off, rows)
    for g in range(3):
        corpus._lib.vsr_hnsw_free(C.c_void_p(handles[g]))
    _raw(corpus, None, None, n_parts=0, out=False)                             # no partitions: succeeds and writes nothing
    assert _raw(corpus, [0], None)[0] == 0xDEAD0
    INV, UNS = _ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED
    _raises(UNS, "VSR_HNSW_BUILD_MERGE_DUPLICATES", _raw, corpus, off, rows, flags=1)
    _raises(INV, "unknown flag bits", _raw, corpus, off, rows, flags=2)
    _raises(INV, "partition 2, position 3: row 1 is named twice", _raw, corpus, off, [5, 6, 7, 1, 2, 3, 1, 5])
    _raises(INV, "partition 0, position 1: row 400 is outside", _raw, corpus, off, [5, 400, 7, 1, 2, 3, 4, 5])
    _raises(INV, "partition 2, position 4: row -1 is outside", _raw, corpus, off, [5, 6, 7, 1, 2, 3, 4, -1])
    _raises(INV, "part_off does not ascend at partition 1", _raw, corpus, [0, 3, 2, 8], rows)
    _raises(INV, "part_off\\[0\\] is 1", _raw, corpus, [1, 3, 3, 8], rows)
    _raises(INV, "NULL argument", _raw, corpus, off, None)
    _raises(INV, "NULL argument", _raw, corpus, None, rows, n_parts=3)
    _raises(INV, "NULL argument", _raw, corpus, off, rows, out=False)
    _raises(INV, "NULL argument", _raw, None, off, rows)
    _raises(UNS, "m must be between 2 and 100", _raw, corpus, off, rows, m=101, efc=400)
    _raises(UNS, "ef_construction must be between 4 and 1000 and at least 2 \\* m", _raw, corpus, off, rows, efc=7)
    _raises(UNS, "L2, inner product and cosine operator classes only", _raw, corpus, off, rows, metric=4)
    for bad in ("0", "4097", "-1", "8x", ""):
        monkeypatch.setenv("VSR_HNSW_FOREST_BATCH", bad)
        _raises(INV, "VSR_HNSW_FOREST_BATCH must be a number from 1 to 4096", _raw, corpus, off, rows)
    monkeypatch.delenv("VSR_HNSW_FOREST_BATCH")
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "300")
    _raises(INV, "VSR_HNSW_BUILD_VISITED_SLOTS", _raw, corpus, off, rows)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    with pytest.raises(Exception, match="named twice"):
        corpus.build_hnsw_partitions([[1, 2], [3, 3]], 8, 32)
    corpus.free()
    rng = np.random.default_rng(9300)
    dense = np.where(rng.random((50, 40)) < 0.2, rng.integers(1, 5, (50, 40)), 0).astype(np.float32)
    dense[:, 0] = 1
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    sparse = ctx.load_corpus_sparse(indptr, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32), 40)
    _raises(UNS, "sparsevec", _raw, sparse, off, rows)
    _raises(UNS, "sparsevec", sparse.build_hnsw_partitions, [[1, 2]], 8, 32)
    sparse.free()
    bits = _load(ctx, "bit", world.rows["bit"][:100], None, None)
    _raises(INV, "not an operator class of bit", bits.build_hnsw_partitions, [[1, 2]], 8, 32, "l2")
    for h in bits.build_hnsw_partitions([[1, 2, 3]], 8, 32):                    # the default metric of a bit corpus is its Hamming opclass
        h.free()
    bits.free()
    ctx.screening_check(0)
