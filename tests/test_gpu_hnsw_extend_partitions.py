"""vsr_hnsw_extend_partitions (Corpus.extend_hnsw_partitions, Deployment.extend_partition_hnsw): new rows for many partition graphs
over one resident corpus in one call.

The contract is equality with vsr_hnsw_extend run on every graph alone: out[g]'s export is, array for array, the export of
Corpus.extend_hnsw(export(prior[g])) with the same ef_construction, metric and seed over a corpus that holds only graph g's rows, old
and new, with their (document_id, block_id), TIDs mapped there and back.  Both sides run the same kernels' arithmetic, so the
comparison is exact; the rows are small integers all the same (every distance exact), which keeps a failure readable.  The seven
graphs are the issue's table.  The results of the one call and of the per-graph route are computed once per (kind, metric) and
shared.  The schedule that packs the extensions' batches into rounds is pinned without a GPU by tests/test_hnsw_forest_extend_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from helpers import check_built_graph, same_graph
from hnsw_forest_search_model import assert_same_groups, merge_model
from hnsw_half_model import to_half

pytestmark = pytest.mark.gpu

N, SEED, M, EFC = 3000, 41, 8, 32
PRIOR = [0, 0, 1, 2, 129, 700, 1500]                                            # elements of the prior graph (0: NULL) ...
ADDED = [0, 17, 1, 127, 0, 800, 3]                                              # ... and the rows it takes
KINDS = [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming")]


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class World:
    """3000 rows with shuffled document and block ids; per graph the rows it holds and the rows it takes, unsorted, disjoint."""

    def __init__(self):
        rng = np.random.default_rng(9400)
        self.rows = {"f32": rng.integers(-8, 9, (N, 16)).astype(np.float32),   # 4 * 16 * 64 < 2^24: sums are exact
                     "bit": rng.integers(0, 2, (N, 64)).astype(np.float32)}    # 64-bit rows
        self.rows["half"] = self.rows["f32"]                                    # small integers are binary16 values
        self.real = rng.normal(size=(N, 16)).astype(np.float32)
        self.doc = rng.permutation(np.arange(N) // 4 + 1).astype(np.int32)     # 750 documents of 4 blocks, shuffled
        self.blk = (rng.permutation(N) + 1).astype(np.int64)
        both = [rng.choice(N, p + a, replace=False).astype(np.int64) for p, a in zip(PRIOR, ADDED)]
        self.old = [b[:p] for b, p in zip(both, PRIOR)]
        self.new = [b[p:] for b, p in zip(both, PRIOR)]
        assert np.intersect1d(both[5], both[6]).size > 0                        # graphs 5 and 6 share rows
        assert np.intersect1d(self.new[5], self.old[6]).size > 0                # a row new to one graph is old in another
        self.queries = self.rows["f32"][rng.integers(0, N, 8)] + rng.integers(-2, 3, (8, 16)).astype(np.float32)
        self.perms = np.array([(r, d) for r in (1, 2, 3) for d in range(1, N // 4 + 2) if d % (r + 1) == 0], dtype=np.int32)
        self.user_roles = np.array([(1, 1), (2, 2), (2, 3)], dtype=np.int32)

    def order(self, rows):
        """rows in internal (document_id, block_id) order: the order a build or an extension inserts them in."""
        return rows[np.lexsort((self.blk[rows], self.doc[rows]))]


@pytest.fixture(scope="module")
def world():
    return World()


def _load(ctx, kind, x, blk, doc):
    if kind == "f32":
        return ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32), blk, doc)
    if kind == "half":
        return ctx.load_corpus_half(to_half(x), blk, doc)
    return ctx.load_corpus_bit(np.asarray(x) != 0, None, blk, doc)


def _load_graph(corpus, kind, graph, metric):
    if kind == "half":
        return corpus.load_hnsw_half(graph)
    return corpus.load_hnsw_bit(graph, metric) if kind == "bit" else corpus.load_hnsw(graph)


def _alone(ctx, world, kind, metric, prior, rows, x, seed=SEED, efc=EFC):
    """The per-graph route: extend_hnsw(prior, an export over the whole corpus) over a sub-corpus of `rows` (caller rows of the
    whole corpus: the prior's and the new ones).  Returns the export with its TIDs as rows of the whole corpus again."""
    back = np.full(N, -1, dtype=np.int64)
    back[rows] = np.arange(len(rows))
    g = dict(prior)
    g["tids"] = np.where(prior["tids"] >= 0, back[np.maximum(prior["tids"], 0)], -1)
    assert (g["tids"][prior["tids"] >= 0] >= 0).all()
    sub = _load(ctx, kind, x[rows], world.blk[rows], world.doc[rows])
    index = sub.extend_hnsw(g, efc, metric, seed)
    out = index.export()
    out["tids"] = np.where(out["tids"] >= 0, rows[np.maximum(out["tids"], 0)], -1)
    index.free()
    sub.free()
    return out


class Case:
    """One corpus with the priors of the table (build_hnsw_partitions of the old rows; graphs 0 and 1 have none), the one call's
    results, and per graph what vsr_hnsw_extend makes of it alone."""

    def __init__(self, ctx, world, kind, metric, x=None, alone=True):
        self.kind, self.metric = kind, metric
        x = world.rows[kind] if x is None else x
        self.corpus = _load(ctx, kind, x, world.blk, world.doc)
        built = self.corpus.build_hnsw_partitions(world.old, M, EFC, metric, SEED)
        self.empties = built[:2]                                                # indexes of n_elem = 0
        self.priors = [None, None] + built[2:]
        self.prior_exports = [h.export() for h in built]                        # (graphs 0 and 1: the export of no elements)
        self.out = self.corpus.extend_hnsw_partitions(self.priors, world.new, EFC, metric, SEED)
        ctx.screening_check(0)                                                  # fails on a guard word that is not as it was found
        self.got = [h.export() for h in self.out]
        self.want = None
        if alone:
            self.want = []
            for g in range(len(PRIOR)):
                if ADDED[g] == 0:
                    self.want.append(self.prior_exports[g])
                else:
                    rows = np.concatenate([world.old[g], world.new[g]])
                    self.want.append(_alone(ctx, world, kind, metric, self.prior_exports[g], rows, x))
            ctx.screening_check(0)

    def free(self):
        for h in self.out + self.empties + [p for p in self.priors if p is not None]:
            h.free()
        self.corpus.free()


_CASES = {}


@pytest.fixture(scope="module")
def case(ctx, world):
    def get(kind, metric):
        if (kind, metric) not in _CASES:
            _CASES[(kind, metric)] = Case(ctx, world, kind, metric)
        return _CASES[(kind, metric)]
    yield get
    for c in _CASES.values():
        c.free()
    _CASES.clear()


def _same_all(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        try:
            same_graph(a, b)
        except AssertionError as e:
            raise AssertionError(f"graph {g} ({len(b['level'])} elements): {e}") from None


def _extended(ctx, world, case, priors=None, new=None, seed=SEED):
    out = case.corpus.extend_hnsw_partitions(case.priors if priors is None else priors, world.new if new is None else new, EFC,
                                             case.metric, seed)
    ctx.screening_check(0)
    got = [h.export() for h in out]
    for h in out:
        h.free()
    return got


# ---- a: equality with vsr_hnsw_extend on every graph alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", KINDS)
def test_every_graph_is_what_extend_makes_of_it_alone(ctx, world, case, kind, metric):
    c = case(kind, metric)
    _same_all(c.got, c.want)
    for g, a in enumerate(c.got):
        n = PRIOR[g] + ADDED[g]
        assert len(a["level"]) == n and c.out[g].info()[0] == n
        # prior elements keep their TIDs; the new rows follow in (document_id, block_id) order, one TID each
        np.testing.assert_array_equal(a["tids"][:PRIOR[g], 0], world.order(world.old[g]))
        np.testing.assert_array_equal(a["tids"][PRIOR[g]:, 0], world.order(world.new[g]))
        assert (a["tid_count"] == 1).all() and (a["tids"][:, 1:] == -1).all()
        if n > 1:
            check_built_graph(a, M)
    assert c.got[0]["entry"] == -1 and c.got[0]["max_level"] == 1 and c.out[0].info() == (0, -1, -1, 1) and c.out[0].device_bytes() == 0
    same_graph(c.got[4], c.prior_exports[4])                                    # nothing added: the prior's export
    assert c.out[4]._h.value != c.priors[4]._h.value                            # ... in an index of its own
    # graph 3: the entry point moves to a new element and the top level rises, so the upper arrays are re-strided
    before, after = c.prior_exports[3], c.got[3]
    assert after["entry"] >= PRIOR[3] > before["entry"] >= 0, (before["entry"], after["entry"])
    assert after["max_level"] > before["max_level"], (before["max_level"], after["max_level"])
    assert after["up_nbr"].shape[1] == after["max_level"]
    # the priors are as they were
    for g in range(2, len(PRIOR)):
        same_graph(c.priors[g].export(), c.prior_exports[g])


# ---- b: prefixes cut at batch boundaries, extended, are the partition build of the full partitions ---------------------------------------
def _boundary(n):
    """A `done` at which a batch of the build's schedule 0 -> n ends, from the batch rule; about the middle one.  0 for n < 2."""
    ends, done = [], 0
    while done < n:
        done += max(1, min(done // 8, 4096, n - done))
        ends.append(done)
    inner = [b for b in ends if b < n]
    return inner[len(inner) // 2] if inner else 0


@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("bit", "hamming")])
def test_boundary_prefixes_extended_are_the_full_partition_build(ctx, world, kind, metric):
    sizes = [0, 1, 2, 17, 129, 700, 1500]
    rng = np.random.default_rng(9401)
    full = [world.order(rng.choice(N, n, replace=False).astype(np.int64)) for n in sizes]
    cuts = [_boundary(n) for n in sizes]
    assert cuts[:3] == [0, 0, 1] and all(0 < c < n for c, n in zip(cuts[3:], sizes[3:])), cuts
    corpus = _load(ctx, kind, world.rows[kind], world.blk, world.doc)
    whole = corpus.build_hnsw_partitions(full, M, EFC, metric, SEED)
    priors = corpus.build_hnsw_partitions([f[:c] for f, c in zip(full, cuts)], M, EFC, metric, SEED)   # cut 0: an index of n_elem = 0
    rest = [rng.permutation(f[c:]) for f, c in zip(full, cuts)]                 # the order the caller names them in does not matter
    out = corpus.extend_hnsw_partitions(priors, rest, EFC, metric, SEED)
    ctx.screening_check(0)
    _same_all([h.export() for h in out], [h.export() for h in whole])
    assert [h.info() for h in out] == [h.info() for h in whole]
    assert [h.device_bytes() for h in out] == [h.device_bytes() for h in whole]
    for h in out + priors + whole:
        h.free()
    corpus.free()


# ---- c: the environment knobs change no graph -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value", [("VSR_HNSW_FOREST_BATCH", "1"), ("VSR_HNSW_FOREST_BATCH", "5"), ("VSR_HNSW_BUILD_VISITED_SLOTS", "256")])
def test_environment_knobs_change_no_graph(ctx, world, case, monkeypatch, name, value):
    c = case("f32", "l2")
    monkeypatch.setenv(name, value)
    got = _extended(ctx, world, c)
    monkeypatch.delenv(name)
    _same_all(got, c.got)
    for a, b in zip(got, c.got):
        for key in ("level", "nbr0", "tids", "up_slot", "up_nbr"):
            assert a[key].tobytes() == b[key].tobytes(), key


# ---- d: a prior that was loaded, not made here ----------------------------------------------------------------------------------------------
def test_loaded_priors_give_the_same_graphs_and_keep_their_tid_lists(ctx, world, case):
    c = case("f32", "l2")
    loaded = [None if p is None else _load_graph(c.corpus, "f32", e, "l2") for p, e in zip(c.priors, c.prior_exports)]
    _same_all(_extended(ctx, world, c, priors=loaded), c.got)
    # graph 6 with a second heap TID under element 0: a row neither the graph nor its new rows name
    g = 6
    extra = int(np.setdiff1d(np.arange(N), np.concatenate([world.old[g], world.new[g]]))[0])
    multi = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.prior_exports[g].items()}
    multi["tid_count"][0], multi["tids"][0, 1] = 2, extra
    two = _load_graph(c.corpus, "f32", multi, "l2")
    got = _extended(ctx, world, c, priors=loaded[:g] + [two])[g]
    assert got["tid_count"][0] == 2 and got["tids"][0, 1] == extra and (got["tid_count"][1:] == 1).all()
    np.testing.assert_array_equal(got["tids"][:PRIOR[g]], multi["tids"])
    rows = np.concatenate([world.old[g], [extra], world.new[g]])
    same_graph(got, _alone(ctx, world, "f32", "l2", multi, rows, world.rows["f32"]))
    for h in loaded + [two]:
        if h is not None:
            h.free()
    ctx.screening_check(0)


# ---- e: the results are ordinary indexes ------------------------------------------------------------------------------------------------------
def test_results_search_alone_and_as_a_forest(ctx, world, case):
    c = case("f32", "l2")
    q, k, ef = world.queries, 10, 40
    per = [h.search(q, k, ef, "l2")[0] for h in c.out]
    for g, res in enumerate(per):
        holds = np.concatenate([world.old[g], world.new[g]])
        assert np.isin(res.rows[res.rows >= 0], holds).all(), "a row outside the graph"
        assert (res.counts <= min(k, len(holds))).all() and (len(holds) == 0 or (res.counts > 0).all())
    again = c.corpus.load_hnsw(c.got[5])                                        # an export of a result loads and answers alike
    np.testing.assert_array_equal(again.search(q, k, ef, "l2")[0].rows, per[5].rows)
    again.free()
    tasks = [[5, 6], [1, 2, 3], [0], [6, 5, 3, 1], [4], [2, 4, 6], [5], [0, 1, 2, 3, 4, 5, 6]]
    forest = c.corpus.hnsw_forest(c.out)
    res, _ = forest.search(q, tasks, k, ef, "l2")
    forest.free()
    blk, doc, row, dist, cnt = merge_model(per, tasks, k)
    np.testing.assert_array_equal(res.counts, cnt)
    np.testing.assert_array_equal(res.rows, row)
    np.testing.assert_array_equal(res.block_ids, blk)
    np.testing.assert_array_equal(res.doc_ids, doc)
    np.testing.assert_array_equal(res.dist, dist)
    ctx.screening_check(0)


# ---- f: determinism on real-valued rows -----------------------------------------------------------------------------------------------------
def test_two_calls_on_real_valued_rows_agree(ctx, world):
    c = Case(ctx, world, "f32", "l2", x=world.real, alone=False)
    again = _extended(ctx, world, c)
    c.free()
    _same_all(again, c.got)
    for a, b in zip(again, c.got):
        for key in ("level", "nbr0", "tids", "up_slot", "up_nbr"):
            assert a[key].tobytes() == b[key].tobytes(), key


# ---- g: refusals ------------------------------------------------------------------------------------------------------------------------------
def _raises(status, fragment, fn, *args, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError, match=fragment) as info:
        fn(*args, **kw)
    assert info.value.status == status, (info.value.status, status, str(info.value))


def _raw(corpus, priors, off, rows, efc=EFC, metric=0, flags=0, n_parts=None, out=True, no_priors=False, sentinel=0xDEAD0):
    """The C call itself; returns the out array, every slot preset to a sentinel so that a refusal must have cleared it."""
    from vsrbac._ffi import load_library
    from vsrbac.engine import _ptr, check
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    n = len(priors) if n_parts is None else n_parts
    handles = (C.c_void_p * max(n, 1))(*([sentinel] * max(n, 1)))
    arr = (C.c_void_p * max(len(priors), 1))(*[None if h is None else h._h for h in priors])
    try:
        check(load_library().vsr_hnsw_extend_partitions(corpus._h if corpus is not None else None, n, None if no_priors else arr, _ptr(off),
                                                        _ptr(rows), efc, metric, SEED, flags, handles if out else None))
    except Exception:
        if out:
            assert all(handles[g] is None for g in range(n)), "a refusal left an out[g] that is not NULL"
        raise
    return handles


def test_refusals_leave_every_out_null_and_the_priors_searchable(ctx, world, monkeypatch):
    from vsrbac import _ffi
    INV, UNS = _ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED
    x = world.rows["f32"][:400]
    corpus = _load(ctx, "f32", x, None, None)
    old = [np.arange(0, 200), np.arange(150, 160), np.zeros(0, dtype=np.int64)]
    priors = corpus.build_hnsw_partitions(old, M, EFC, "l2", SEED)
    exports = [h.export() for h in priors]
    assert exports[0]["up_nbr"].shape[0] > 1 and (exports[0]["up_nbr"] >= 0).any()   # the bad neighbour below needs an upper list
    q = x[:5] + 1
    before = [h.search(q, 5, 40, "l2")[0].rows.copy() for h in priors[:2]]
    off, rows = [0, 3, 3, 8], [205, 206, 207, 201, 202, 203, 204, 205]          # row 205 new in two partitions: allowed
    handles = _raw(corpus, priors, off, rows)
    assert [corpus._lib.vsr_hnsw_free(C.c_void_p(handles[g])) for g in range(3)] == [0, 0, 0]
    _raw(corpus, [], None, None, n_parts=0, out=False, no_priors=True)         # no partitions: succeeds and writes nothing
    assert _raw(corpus, [], [0], None, n_parts=0)[0] == 0xDEAD0
    _raises(UNS, "VSR_HNSW_BUILD_MERGE_DUPLICATES", _raw, corpus, priors, off, rows, flags=1)
    _raises(INV, "unknown flag bits", _raw, corpus, priors, off, rows, flags=2)
    _raises(INV, "partition 2, position 3: row 201 is named twice", _raw, corpus, priors, off, [205, 206, 207, 201, 202, 203, 201, 205])
    _raises(INV, "partition 0, position 1: row 400 is outside", _raw, corpus, priors, off, [205, 400, 207, 201, 202, 203, 204, 205])
    _raises(INV, "partition 2, position 4: row -1 is outside", _raw, corpus, priors, off, [205, 206, 207, 201, 202, 203, 204, -1])
    _raises(INV, "new_off does not ascend at partition 1", _raw, corpus, priors, [0, 3, 2, 8], rows)
    _raises(INV, "new_off\\[0\\] is 1", _raw, corpus, priors, [1, 3, 3, 8], rows)
    _raises(INV, "NULL argument", _raw, corpus, priors, off, None)
    _raises(INV, "NULL argument", _raw, corpus, priors, None, rows)
    _raises(INV, "NULL argument", _raw, corpus, priors, off, rows, out=False)
    _raises(INV, "NULL argument", _raw, corpus, priors, off, rows, no_priors=True)
    _raises(INV, "NULL argument", _raw, None, priors, off, rows)
    _raises(INV, "every prior index is NULL", _raw, corpus, [None, None, None], off, rows)
    _raises(UNS, "ef_construction must be between 4 and 1000 and at least 2 \\* m", _raw, corpus, priors, off, rows, efc=7)
    _raises(UNS, "L2, inner product and cosine operator classes only", _raw, corpus, priors, off, rows, metric=4)
    # a new row the graph holds already: graph 0 holds rows 0 .. 199, graph 1 rows 150 .. 159
    _raises(INV, "partition 0: new row 17 is under a heap TID", _raw, corpus, priors, off, [205, 17, 207, 201, 202, 203, 204, 205])
    _raises(INV, "partition 1: new row 155 is under a heap TID", _raw, corpus, priors, [0, 1, 2, 3], [205, 155, 206])
    handles = _raw(corpus, priors, [0, 1, 2, 3], [206, 5, 150])                 # held by ANOTHER partition's graph only: allowed
    assert [corpus._lib.vsr_hnsw_free(C.c_void_p(handles[g])) for g in range(3)] == [0, 0, 0]
    # priors that do not belong: another m, another corpus, another row format / opclass
    other_m = corpus.build_hnsw_partitions([np.arange(20)], 4, EFC, "l2", SEED)[0]
    _raises(INV, "partition 1: the prior index has m = 4", _raw, corpus, [priors[0], other_m, None], off, rows)
    twin = _load(ctx, "f32", x, None, None)
    stranger = twin.build_hnsw_partitions([np.arange(20)], M, EFC, "l2", SEED)[0]
    _raises(INV, "partition 2: the prior index is over another corpus", _raw, corpus, [priors[0], None, stranger], off, rows)
    stranger.free()
    twin.free()
    other_m.free()
    # a loaded prior is checked on the host before anything is launched: a neighbour id of n_elem in an upper list, which
    # load_hnsw's own checks do not look at
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in exports[0].items()}
    slot, lc, j = np.argwhere(bad["up_nbr"] >= 0)[0]
    bad["up_nbr"][slot, lc, j] = len(bad["level"])
    loaded = corpus.load_hnsw(bad)
    _raises(INV, "partition 1: the prior index: element .* lists neighbour 200 on layer", _raw, corpus, [priors[0], loaded, None], [0, 1, 4, 8],
            [205, 206, 207, 201, 202, 203, 204, 205])
    handles = _raw(corpus, [priors[0], loaded, None], [0, 3, 3, 8], rows)      # ... and is only copied when it takes no rows
    assert [corpus._lib.vsr_hnsw_free(C.c_void_p(handles[g])) for g in range(3)] == [0, 0, 0]
    loaded.free()
    for bad_env in ("0", "4097", "8x"):
        monkeypatch.setenv("VSR_HNSW_FOREST_BATCH", bad_env)
        _raises(INV, "VSR_HNSW_FOREST_BATCH must be a number from 1 to 4096", _raw, corpus, priors, off, rows)
    monkeypatch.delenv("VSR_HNSW_FOREST_BATCH")
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "300")
    _raises(INV, "VSR_HNSW_BUILD_VISITED_SLOTS", _raw, corpus, priors, off, rows)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    with pytest.raises(ValueError, match="3 indexes but 2 row lists"):
        corpus.extend_hnsw_partitions(priors, [[201], [202]])
    # after all that: the priors are as they were and answer as before
    for h, e, rows_before in zip(priors[:2], exports[:2], before):
        same_graph(h.export(), e)
        np.testing.assert_array_equal(h.search(q, 5, 40, "l2")[0].rows, rows_before)
    for h in priors:
        h.free()
    corpus.free()
    rng = np.random.default_rng(9402)
    dense = np.where(rng.random((50, 40)) < 0.2, rng.integers(1, 5, (50, 40)), 0).astype(np.float32)
    dense[:, 0] = 1
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    sparse = ctx.load_corpus_sparse(indptr, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32), 40)
    _raises(UNS, "sparsevec", _raw, sparse, [None], [0, 2], [1, 2])
    _raises(UNS, "sparsevec", sparse.extend_hnsw_partitions, [None], [[1, 2]])
    sparse.free()
    bits = _load(ctx, "bit", world.rows["bit"][:100], None, None)
    ham = bits.build_hnsw_partitions([[1, 2, 3]], M, EFC)[0]                    # the default metric of a bit corpus is its Hamming opclass
    _raises(INV, "partition 0: the prior index's opclass", bits.extend_hnsw_partitions, [ham], [[4, 5]], EFC, "jaccard")
    _raises(INV, "partition 0: the prior index's opclass", bits.extend_hnsw_partitions, [ham], [[4, 5]], EFC, "l2")
    more = bits.extend_hnsw_partitions([ham], [[4, 5]], EFC)[0]
    assert more.info()[0] == 5
    halves = _load(ctx, "half", world.rows["half"][:100], None, None)
    _raises(INV, "partition 0: the prior index is over another corpus", _raw, halves, [ham], [0, 1], [7])
    halves.free()
    more.free()
    ham.free()
    bits.free()
    ctx.screening_check(0)


def test_a_copy_of_a_loaded_prior_is_still_checked_when_a_later_call_gives_it_rows(ctx, world):
    """A partition without new rows comes back as a plain copy that nobody read.  The copy of a loaded graph must not pass for a graph
    this library made: given rows in a SECOND call it goes through the host checks like the loaded index, before anything is launched.
    The copy of a graph the library made is written through as it is, and gives what extending the original gives."""
    from vsrbac import _ffi
    from vsrbac.engine import HnswIndex
    x = world.rows["f32"][:400]
    corpus = _load(ctx, "f32", x, None, None)
    made = corpus.build_hnsw_partitions([np.arange(0, 200)], M, EFC, "l2", SEED)[0]
    bad = made.export()
    slot, lc, j = np.argwhere(bad["up_nbr"] >= 0)[0]
    bad["up_nbr"][slot, lc, j] = len(bad["level"])                             # a neighbour id of n_elem, where load_hnsw does not look
    loaded = corpus.load_hnsw(bad)
    copies = corpus.extend_hnsw_partitions([made, loaded], [[], []], EFC, "l2", SEED)
    same_graph(copies[1].export(), bad)
    rows = [201, 205, 210]
    _raises(_ffi.ERR_INVALID, "partition 1: the prior index: element .* lists neighbour 200 on layer", _raw, corpus, [made, copies[1]],
            [0, 0, 3], rows)
    again = corpus.extend_hnsw_partitions([None, copies[1]], [[], []], EFC, "l2", SEED)   # a copy of the copy is no better
    _raises(_ffi.ERR_INVALID, "partition 0: the prior index: element .* lists neighbour 200 on layer", _raw, corpus, [again[1], None],
            [0, 3, 3], rows)
    want = corpus.extend_hnsw_partitions([made], [rows], EFC, "l2", SEED)[0]
    got = corpus.extend_hnsw_partitions([copies[0]], [rows], EFC, "l2", SEED)[0]
    same_graph(got.export(), want.export())
    freed = corpus.extend_hnsw_partitions([made], [[]], EFC, "l2", SEED)[0]
    freed.free()
    with pytest.raises(ValueError, match="indexes\\[1\\] has been freed"):
        corpus.extend_hnsw_partitions([made, freed], [rows, rows], EFC, "l2", SEED)
    assert isinstance(got, HnswIndex)
    for h in [got, want, made, loaded] + copies + again:
        h.free()
    corpus.free()
    ctx.screening_check(0)


# ---- h: the deployment's spelling ---------------------------------------------------------------------------------------------------------------
def test_deployment_extends_its_partition_graphs(ctx, world):
    import vsrbac
    from vsrbac.harness import Deployment, merge_results
    x = world.rows["f32"]
    dep = Deployment(ctx, x, world.blk, world.doc, world.user_roles, world.perms)
    first = {11: list(range(2, 200, 2)), 12: list(range(1, 120)), 13: list(range(90, 260, 3)), 14: []}
    added = {12: list(range(120, 150)), 11: [200, 202, 204], 14: [300, 301]}
    combs = {(1,): [11, 12], (2, 3): [12, 13, 14]}                              # user 1 has role 1, user 2 roles 2 and 3
    dep.load_partitions(first, combs)
    graphs = dep.build_partition_hnsw(m=M, ef_construction=EFC, seed=SEED)
    new = dep.extend_partition_hnsw(graphs, added, ef_construction=EFC, seed=SEED)
    assert sorted(new) == [11, 12, 14] and all(new[p]._h.value != graphs[p]._h.value for p in new)
    # the same graphs as the corpus call on the rows of those documents
    pids = sorted(added)
    parts = [np.flatnonzero(np.isin(world.doc, added[p])) for p in pids]
    assert [len(p) for p in parts] == [12, 120, 8]
    direct = dep.corpus.extend_hnsw_partitions([graphs[p] for p in pids], parts, EFC, "l2", SEED)
    _same_all([new[p].export() for p in pids], [h.export() for h in direct])
    for p, rows in zip(pids, parts):
        assert new[p].info()[0] == graphs[p].info()[0] + len(rows)
        assert np.isin(rows, new[p].export()["tids"][:, 0]).all()
    for h in direct:
        h.free()
    with pytest.raises(ValueError, match="no graph to extend"):
        dep.extend_partition_hnsw(graphs, {99: [1]})
    # the caller's part: free what was replaced, tell the deployment the documents and the graphs
    for p in new:
        graphs[p].free()
    graphs.update(new)
    dep.load_partitions({p: first[p] + added.get(p, []) for p in first}, combs)
    dep.use_partition_hnsw(graphs)
    topk, ef = 7, 40
    users = [1, 2, 1, 2]
    queries = [world.queries[i] for i in range(3)] + [x[parts[1][5]]]           # the last one is a row that partition 12 took
    for u, qv in zip(users, queries):
        rows, _ = dep.dynamic_partition_search_hnsw(u, qv, topk, "sql", ef)
        f = dep.corpus.filter_for_user(u, vsrbac.BITMAP)
        every = []
        for pid in sorted(set(combs[tuple(sorted(dep.user_roles[u]))])):
            res, _ = graphs[pid].search(qv, topk, ef, "l2", [f])
            every.extend(dep._rows(res))
        assert_same_groups(rows, merge_results(every, topk), every)
        assert rows and all(any(r[1] % (role + 1) == 0 for role in dep.user_roles[u]) for r in rows)
    dep.close_partition_hnsw()
    for h in graphs.values():
        h.free()
    dep.close()
    ctx.screening_check(0)
