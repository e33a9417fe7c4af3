"""vsr_hnsw_forest_search* (HnswForest, Deployment.dynamic_partition_search_hnsw): the partition graphs of a query searched in one
launch and merged on the GPU.

The contract is "what the existing entry points return, merged": every expected value here comes from HnswIndex.search /
search_bit / search_device on each graph plus the numpy model (hnsw_forest_search_model.py), never from the forest call.  Both sides
run the same search body, so block ids, document ids, rows, counts, the distances' bits and the per-task visited counts are compared
exactly.  The world is that of tests/test_gpu_hnsw_partitions.py (3000 rows of small integers, shuffled ids, seven overlapping row
lists from 0 to 1500 rows), built once per kind."""
import ctypes as C

import numpy as np
import pytest

from hnsw_forest_search_model import assert_same_groups, merge_model
from hnsw_half_model import to_half

pytestmark = pytest.mark.gpu

N, SEED, M, EFC = 3000, 41, 8, 32
SIZES = [0, 1, 2, 17, 129, 700, 1500]
KINDS = [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming")]
NQ = 40


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class World:
    def __init__(self):
        rng = np.random.default_rng(9100)
        self.rows = {"f32": rng.integers(-8, 9, (N, 16)).astype(np.float32),
                     "bit": rng.integers(0, 2, (N, 64)).astype(np.float32)}
        self.rows["half"] = self.rows["f32"]
        self.real = rng.normal(size=(N, 16)).astype(np.float32)
        self.doc = rng.permutation(np.arange(N) // 4 + 1).astype(np.int32)
        self.blk = (rng.permutation(N) + 1).astype(np.int64)
        self.parts = [rng.choice(N, n, replace=False).astype(np.int64) for n in SIZES]
        self.perms = np.array([(r, d) for r in (1, 2, 3) for d in range(1, N // 4 + 2) if d % (r + 1) == 0], dtype=np.int32)
        self.user_roles = np.array([(1, 1), (2, 2), (2, 3), (3, 3)], dtype=np.int32)         # three users
        q = np.random.default_rng(9400)
        self.queries = {"f32": self.rows["f32"][q.integers(0, N, NQ)] + q.integers(-2, 3, (NQ, 16)).astype(np.float32),
                        "bit": q.integers(0, 2, (NQ, 64)).astype(bool),
                        "real": q.normal(size=(NQ, 16)).astype(np.float32)}
        self.queries["half"] = self.queries["f32"]
        # task lists of 0..7 graphs; then the four the issue names
        self.tasks = [list(q.choice(7, q.integers(0, 8), replace=False)) for _ in range(NQ)]
        self.tasks[0], self.tasks[1], self.tasks[2], self.tasks[3] = [], [0], [6, 6], [0, 1, 2, 3, 4, 5, 6]
        self.users = [int(u) for u in q.integers(1, 4, NQ)]


@pytest.fixture(scope="module")
def world():
    return World()


def _load(ctx, kind, x, blk, doc):
    if kind == "f32":
        return ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32), blk, doc)
    if kind == "half":
        return ctx.load_corpus_half(to_half(x), blk, doc)
    return ctx.load_corpus_bit(np.asarray(x) != 0, None, blk, doc)


class Built:
    """One corpus with its RBAC tables, the seven partition graphs and the forest over them."""

    def __init__(self, ctx, world, kind, metric, x=None):
        self.kind, self.metric = kind, metric
        self.corpus = _load(ctx, kind, world.rows[kind] if x is None else x, world.blk, world.doc)
        self.corpus.load_rbac(world.user_roles, world.perms)
        self.indexes = self.corpus.build_hnsw_partitions(world.parts, M, EFC, metric, SEED)
        self.forest = self.corpus.hnsw_forest(self.indexes)

    def per_graph(self, q, k, ef, filters=None, graphs=range(7)):
        """HnswIndex.search / search_bit of every graph over all the queries: ({g: SearchResult}, {g: visited})."""
        res, vis = {}, {}
        for g in graphs:
            fn = self.indexes[g].search_bit if self.kind == "bit" else self.indexes[g].search
            res[g], vis[g] = fn(q, k, ef, self.metric, filters)
        return res, vis

    def search(self, q, tasks, k, ef, filters=None):
        fn = self.forest.search_bit if self.kind == "bit" else self.forest.search
        return fn(q, tasks, k, ef, self.metric, filters)

    def free(self):
        self.forest.free()
        for h in self.indexes:
            h.free()
        self.corpus.free()


_BUILT = {}


@pytest.fixture(scope="module")
def built(ctx, world):
    def get(kind, metric, real=False):
        key = (kind, metric, real)
        if key not in _BUILT:
            _BUILT[key] = Built(ctx, world, kind, metric, world.real if real else None)
        return _BUILT[key]
    yield get
    for b in _BUILT.values():
        b.free()
    _BUILT.clear()


def _same(res, want, what=""):
    blk, doc, row, dist, cnt = want
    np.testing.assert_array_equal(res.counts, cnt, err_msg=what)
    np.testing.assert_array_equal(res.rows, row, err_msg=what)
    np.testing.assert_array_equal(res.block_ids, blk, err_msg=what)
    np.testing.assert_array_equal(res.doc_ids, doc, err_msg=what)
    assert res.dist.view(np.uint32).tobytes() == dist.view(np.uint32).tobytes(), f"{what}: the distances' bits differ"


def _task_visited(tasks, vis):
    """Per task, the visited count of the per-graph call.  Graph 0 is empty: vsr_hnsw_search writes no count for a graph without an
    entry point (the word keeps what the scratch block held), the forest call reports the 0 elements it visited."""
    return np.array([vis[g][i] if g != 0 else 0 for i, graphs in enumerate(tasks) for g in graphs], dtype=np.int64)


# ---- 1: equality with the per-graph searches, merged ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", KINDS)
def test_forest_search_equals_the_per_graph_searches_merged(ctx, world, built, kind, metric):
    b = built(kind, metric)
    q, k, ef = world.queries[kind], 10, 40
    per, vis = b.per_graph(q, k, ef)
    res, tvis = b.search(q, world.tasks, k, ef)
    want = merge_model(per, world.tasks, k)
    _same(res, want, kind)
    np.testing.assert_array_equal(tvis, _task_visited(world.tasks, vis))
    assert res.counts[0] == 0 and res.counts[1] == 0                           # no task; only the empty graph
    np.testing.assert_array_equal(res.rows[2], per[6].rows[2])                 # the same graph twice: its own answer, every row once
    assert res.counts[3] == k and len(set(res.rows[3])) == k
    assert (want[4] > 0).sum() > 20 and any(len(set(t)) > 3 for t in world.tasks)
    ctx.screening_check(0)


def test_forest_search_on_real_valued_rows(ctx, world, built):
    """Both sides run the same arithmetic, so the bits are compared here too; the model orders by the per-graph call's distance."""
    b = built("f32", "l2", real=True)
    q, k, ef = world.queries["real"], 10, 40
    per, vis = b.per_graph(q, k, ef)
    res, tvis = b.search(q, world.tasks, k, ef)
    _same(res, merge_model(per, world.tasks, k), "real")
    np.testing.assert_array_equal(tvis, _task_visited(world.tasks, vis))


# ---- 2: filters, the forest predicate-aware off and on --------------------------------------------------------------------------------
@pytest.mark.parametrize("aware", [False, True])
def test_filters_and_the_predicate_aware_walk(ctx, world, built, aware):
    import vsrbac
    b = built("f32", "l2")
    q, k, ef = world.queries["f32"], 10, 40
    by_user = {u: b.corpus.filter_for_user(u, vsrbac.BITMAP) for u in (1, 2, 3)}
    assert all(0 < f.allowed_rows < N for f in by_user.values())
    filters = [by_user[u] for u in world.users]
    for h in b.indexes:
        h.set_predicate_aware(aware)
    b.forest.set_predicate_aware(aware)
    try:
        per, vis = b.per_graph(q, k, ef, filters)
        res, tvis = b.search(q, world.tasks, k, ef, filters)
        for h in b.indexes:                                                    # the indexes' own flags are not read
            h.set_predicate_aware(not aware)
        res2, tvis2 = b.search(q, world.tasks, k, ef, filters)
    finally:
        for h in b.indexes:
            h.set_predicate_aware(False)
        b.forest.set_predicate_aware(False)
    want = merge_model(per, world.tasks, k)
    _same(res, want, f"aware={aware}")
    _same(res2, want, f"aware={aware}, index flags flipped")
    np.testing.assert_array_equal(tvis, _task_visited(world.tasks, vis))
    np.testing.assert_array_equal(tvis2, tvis)
    unfiltered, _ = b.search(q, world.tasks, k, ef)
    assert (unfiltered.rows != res.rows).any()                                 # the filters did something
    ctx.screening_check(0)


# ---- 3: results shorter than k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("bit", "hamming")])
def test_short_results_and_exact_padding(world, built, kind, metric):
    b = built(kind, metric)
    q, k = world.queries[kind][:6], 10
    tasks = [[1], [2], [1, 2], [2, 1], [1, 1, 2], [2, 2]]
    per, vis = b.per_graph(q, k, 40, graphs=(1, 2))
    res, tvis = b.search(q, tasks, k, 40)
    want = merge_model(per, tasks, k)
    _same(res, want, kind)
    both = len(set(world.parts[1]) | set(world.parts[2]))
    np.testing.assert_array_equal(res.counts, [1, 2, both, both, both, 2])
    assert res.counts.min() >= 1 and res.counts.max() <= 3
    for i, n in enumerate(res.counts):
        assert (res.block_ids[i, n:] == -1).all() and (res.doc_ids[i, n:] == -1).all() and (res.rows[i, n:] == -1).all()
        assert (res.dist[i, n:].view(np.uint32) == 0x7F800000).all()
    np.testing.assert_array_equal(tvis, _task_visited(tasks, vis))


# ---- 4: the number of merge passes does not change the result -----------------------------------------------------------------------------
def test_merge_capacity_does_not_change_the_result(world, built, monkeypatch):
    b = built("f32", "l2")
    q, k, ef = world.queries["f32"][:12], 100, 100
    tasks = [[0, 1, 2, 3, 4, 5, 6]] * 11 + [[6, 5, 4, 3, 2, 1, 0, 6, 5]]
    per, _ = b.per_graph(q, k, ef)
    want = merge_model(per, tasks, k)
    got = {}
    for cap in ("256", "1024", None):                                          # 256: the smallest power of two >= 2 k, six passes
        if cap is None:
            monkeypatch.delenv("VSR_HNSW_FOREST_MERGE_KEYS", raising=False)
        else:
            monkeypatch.setenv("VSR_HNSW_FOREST_MERGE_KEYS", cap)
        got[cap], _ = b.search(q, tasks, k, ef)
        _same(got[cap], want, f"capacity {cap}")
    for cap in ("256", "1024"):
        for a, c in zip(got[cap], got[None]):
            assert a.tobytes() == c.tobytes()
    assert (got[None].counts == k).all()


# ---- 5: the forms of the visited set ---------------------------------------------------------------------------------------------------
def _device(b, q, tasks, k, ef, filters=None):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    nq, nt = len(q), sum(len(t) for t in tasks)
    host_q = np.packbits(q, axis=1) if b.kind == "bit" else np.ascontiguousarray(q, dtype=np.float32)
    d_q = torch.from_numpy(host_q).to(dev)
    o = {"blk": torch.full((nq, k), 7, dtype=torch.int64, device=dev), "doc": torch.full((nq, k), 7, dtype=torch.int32, device=dev),
         "row": torch.full((nq, k), 7, dtype=torch.int64, device=dev), "dist": torch.full((nq, k), 7.0, dtype=torch.float32, device=dev),
         "cnt": torch.full((nq,), 7, dtype=torch.int32, device=dev), "vis": torch.full((max(nt, 1),), 7, dtype=torch.int64, device=dev)}
    torch.cuda.synchronize()
    fn = b.forest.search_bit_device if b.kind == "bit" else b.forest.search_device
    keep = fn(p(d_q), nq, tasks, k, ef, b.metric, filters, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    b.corpus.ctx.synchronize()
    del keep
    out = {key: v.cpu().numpy() for key, v in o.items()}
    out["vis"] = out["vis"][:nt]
    return out


def _graph_device_counts(b, g, q, k, ef):
    """The counts of HnswIndex.search_device on graph g: -1 marks the queries whose visited table overflowed."""
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    o = [torch.empty((nq, k), dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int64, torch.float32)]
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    b.indexes[g].search_device(p(d_q), nq, k, ef, b.metric, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(cnt))
    b.corpus.ctx.synchronize()
    return cnt.cpu().numpy()


def test_visited_forms(world, built, monkeypatch):
    b = built("f32", "l2")
    q, k, ef, tasks = world.queries["f32"], 10, 40, world.tasks
    monkeypatch.delenv("VSR_HNSW_VISITED", raising=False)
    base, base_vis = b.search(q, tasks, k, ef)
    monkeypatch.setenv("VSR_HNSW_VISITED", "global")
    res, vis = b.search(q, tasks, k, ef)
    for a, c in zip(res, base):
        assert a.tobytes() == c.tobytes()
    np.testing.assert_array_equal(vis, base_vis)
    # 64 slots overflow beyond 48 visited elements: the larger graphs do, the small ones cannot
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:64")
    res, vis = b.search(q, tasks, k, ef)                                       # the host form: those tasks again, merged again
    for a, c in zip(res, base):
        assert a.tobytes() == c.tobytes()
    np.testing.assert_array_equal(vis, base_vis)
    failed = {g: _graph_device_counts(b, g, q, k, ef) < 0 for g in range(7)}   # per graph and query, by the existing entry point
    assert failed[6].any() and not failed[3].any()
    lost = np.array([any(failed[g][i] for g in graphs) for i, graphs in enumerate(tasks)])
    assert lost.any() and not lost.all()
    dev = _device(b, q, tasks, k, ef)
    monkeypatch.delenv("VSR_HNSW_VISITED")
    np.testing.assert_array_equal(dev["cnt"] == -1, lost)
    assert (dev["blk"][lost] == -1).all() and np.isinf(dev["dist"][lost]).all()  # never a partial result
    keepers = ~lost
    np.testing.assert_array_equal(dev["cnt"][keepers], base.counts[keepers])
    np.testing.assert_array_equal(dev["row"][keepers], base.rows[keepers])
    assert dev["dist"][keepers].tobytes() == base.dist[keepers].tobytes()


# ---- 6: the device form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("half", "l2"), ("bit", "hamming")])
def test_device_form_equals_the_host_form(ctx, world, built, kind, metric):
    import vsrbac
    b = built(kind, metric)
    q, k, ef = world.queries[kind], 10, 40
    flt = [b.corpus.filter_for_user(u, vsrbac.BITMAP) for u in world.users] if kind == "f32" else None
    res, vis = b.search(q, world.tasks, k, ef, flt)
    dev = _device(b, q, world.tasks, k, ef, flt)
    np.testing.assert_array_equal(dev["cnt"], res.counts)
    np.testing.assert_array_equal(dev["row"], res.rows)
    np.testing.assert_array_equal(dev["blk"], res.block_ids)
    np.testing.assert_array_equal(dev["doc"], res.doc_ids)
    assert dev["dist"].tobytes() == res.dist.tobytes()
    np.testing.assert_array_equal(dev["vis"], vis)
    ctx.screening_check(0)


# ---- 7: the deployment's spelling -----------------------------------------------------------------------------------------------------------
def test_deployment_searches_through_the_partition_graphs(ctx, world):
    import vsrbac
    from vsrbac.harness import Deployment, merge_results
    x = world.rows["f32"]
    dep = Deployment(ctx, x, world.blk, world.doc, world.user_roles, world.perms)
    # documents of role r: multiples of r + 1.  Partition 11 holds only documents all of role 1 may see (pure for user 1), 12 mixes in
    # documents that roles 2 and 3 cannot see (impure for them), 13 overlaps both
    partition_docs = {11: list(range(2, 200, 2)), 12: list(range(1, 120)), 13: list(range(90, 260, 3)), 14: []}
    combs = {(1,): [11, 12], (2, 3): [12, 13, 14], (3,): [13, 12]}
    dep.load_partitions(partition_docs, combs)
    graphs = dep.build_partition_hnsw(m=M, ef_construction=EFC, seed=SEED)
    dep.use_partition_hnsw(graphs)
    topk, ef = 7, 40
    users = [1, 2, 3, 1, 2, 3, 2]
    queries = [world.queries["f32"][i] for i in range(len(users))]
    singles = []
    for u, qv in zip(users, queries):
        rows, secs = dep.dynamic_partition_search_hnsw(u, qv, topk, "sql", ef)
        assert secs > 0
        singles.append(rows)
        f = dep.corpus.filter_for_user(u, vsrbac.BITMAP)
        comb = tuple(sorted(dep.user_roles[u]))
        every = []
        for pid in sorted(set(combs[comb])):
            res, _ = graphs[pid].search(qv, topk, ef, "l2", [f])
            every.extend(dep._rows(res))
        want = merge_results(every, topk)
        assert_same_groups(rows, want, every)
        assert rows and all(any(r[1] % (role + 1) == 0 for role in dep.user_roles[u]) for r in rows)   # only documents the user may see
    assert dep.dynamic_partition_search_hnsw_batch(users, queries, topk, ef) == singles
    exact, _ = dep.dynamic_partition_search(1, queries[0], topk, "system")     # the exact route is still there, untouched
    assert len(exact) == topk
    dep.close_partition_hnsw()
    for h in graphs.values():
        h.free()
    dep.close()
    ctx.screening_check(0)


# ---- 8: refusals --------------------------------------------------------------------------------------------------------------------------
def _raises(status, fragment, fn, *args, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError, match=fragment) as info:
        fn(*args, **kw)
    assert info.value.status == status, (info.value.status, status, str(info.value))
    return str(info.value)


def test_refusals(ctx, world, built, monkeypatch):
    from vsrbac import _ffi
    from vsrbac.engine import HnswForest
    INV, UNS = _ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED
    b, bits, half = built("f32", "l2"), built("bit", "hamming"), built("half", "l2")
    q, qb = world.queries["f32"][:4], world.queries["bit"][:4]
    # what a forest may hold
    other = _load(ctx, "f32", world.rows["f32"][:300], None, None)
    far = other.build_hnsw(M, EFC, "l2", seed=SEED)
    wide = b.corpus.build_hnsw_partitions([world.parts[3]], 4, 16, "l2", SEED)[0]
    _raises(INV, "index 2 is over another corpus than index 0", HnswForest, [b.indexes[3], b.indexes[4], far])
    _raises(INV, "index 1 has m = 4, index 0 has m = 8", HnswForest, [b.indexes[3], wide])
    _raises(INV, "index 1 is over halfvec rows, index 0 over vector rows", HnswForest, [b.indexes[3], half.indexes[3]])
    rng = np.random.default_rng(9300)
    dense = np.where(rng.random((50, 40)) < 0.2, rng.integers(1, 5, (50, 40)), 0).astype(np.float32)
    dense[:, 0] = 1
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    sparse = ctx.load_corpus_sparse(indptr, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32), 40)
    sp = sparse.build_hnsw_sparse(M, EFC, "l2", seed=SEED)
    _raises(UNS, "sparsevec", HnswForest, [sp])
    for h in (far, wide, sp):
        h.free()
    other.free()
    sparse.free()
    # the queries of the wrong kind: the status and the text of the single-index entry points
    tasks = [[3], [4], [], [5, 6]]
    import vsrbac
    for single_call, forest_call in ((lambda: bits.indexes[3].search(q, 10, 40), lambda: bits.forest.search(q, tasks, 10, 40)),
                                     (lambda: b.indexes[3].search_bit(qb, 10, 40, dim=64), lambda: b.forest.search_bit(qb, tasks, 10, 40, dim=64))):
        with pytest.raises(vsrbac.VsrError) as single:
            single_call()
        with pytest.raises(vsrbac.VsrError) as forest:
            forest_call()
        assert forest.value.status == single.value.status and forest.value.status in (INV, UNS)
        assert str(forest.value).split(": ", 1)[1] == str(single.value).split(": ", 1)[1]          # all but the entry point's name
    # malformed task tables
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    _raises(INV, "q_off decreases at query 1", b.forest.search, q, (i64([0, 2, 1, 3, 3]), i32([3, 4, 5])), 10)
    _raises(INV, "q_off\\[0\\] is 1", b.forest.search, q, (i64([1, 2, 2, 3, 3]), i32([3, 4, 5])), 10)
    _raises(INV, "task 1 names graph -1 of a forest of 7", b.forest.search, q, (i64([0, 2, 2, 3, 3]), i32([3, -1, 5])), 10)
    _raises(INV, "task 2 names graph 7 of a forest of 7", b.forest.search, q, (i64([0, 2, 2, 3, 3]), i32([3, 4, 7])), 10)
    _raises(INV, "ef_search must be between 1 and 5000", b.forest.search, q, tasks, 10, 0)
    for bad in ("8", "16", "24", "32768", "x", "", "-64"):                      # k = 10: 32 .. 16384
        monkeypatch.setenv("VSR_HNSW_FOREST_MERGE_KEYS", bad)
        _raises(INV, "VSR_HNSW_FOREST_MERGE_KEYS must be a power of two from 32", b.forest.search, q, tasks, 10)
    monkeypatch.setenv("VSR_HNSW_FOREST_MERGE_KEYS", "32")
    lo, _ = b.search(q, tasks, 10, 40)
    monkeypatch.delenv("VSR_HNSW_FOREST_MERGE_KEYS")
    ok, _ = b.search(q, tasks, 10, 40)
    np.testing.assert_array_equal(lo.rows, ok.rows)
    # an empty forest: queries without tasks only
    empty = HnswForest([])
    res, vis = empty.search(q, [[], [], [], []], 10)
    assert (res.counts == 0).all() and (res.rows == -1).all() and np.isinf(res.dist).all() and vis.size == 0
    _raises(INV, "names graph 0 of a forest of 0", empty.search, q, [[0], [], [], []], 10)
    empty.free()
    ctx.screening_check(0)
