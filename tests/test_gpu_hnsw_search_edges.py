"""The fp32 HNSW search (K4: hnsw_search_kernel, the ROWS_F32 branch of hnsw_search_body in csrc/vsr_hnsw.h) at its row, graph and
launch edges, against the index oracle on the oracle's own graph (load_hnsw of HnswIndex.export(): the GPU build is not involved).

The cases come from tests/hnsw_search_edge_cases.py; tests/test_hnsw_search_edges_cpu.py holds the conditions that keep these tests
from passing vacuously.  Every fp32 sum of a case is exact in any order, so nothing here has a tolerance: counts, rows in order, the
BITS of the reported distances (the oracle's index distance through the operator's rule in double, rounded to fp32) and the visited
count of every query."""
import ctypes as C

import numpy as np
import pytest

import hnsw_search_edge_cases as ec
from hnsw_forest_search_model import merge_model
from hnsw_half_model import to_half
from hnsw_iterative_model import Graph, IterativeScan, Stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx, oracle):
    """name -> (case, oracle index, corpus, GPU index over the oracle's export), loaded once."""
    made = {}

    def get(name):
        if name not in made:
            c, oh = ec.CASES[name], ec.oracle_index(oracle, name)
            corpus = ctx.load_corpus(c.rows)
            made[name] = (c, oh, corpus, corpus.load_hnsw(oh.export()))
        return made[name]
    yield get
    for _, _, corpus, gpu in made.values():
        gpu.free()
        corpus.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_matches_the_oracle(res, vis, oh, metric, q, k, ef, what):
    for i in range(len(q)):
        rows_o, dist_o, _, nv = oh.search(q[i], ef)
        m = min(k, rows_o.size)
        at = (what, k, ef, i)
        assert res.counts[i] == m, (at, res.counts[i], m)
        np.testing.assert_array_equal(res.rows[i, :m], rows_o[:m], err_msg=str(at))
        want = ec.reported_distance(metric, dist_o[:m])
        np.testing.assert_array_equal(_bits(res.dist[i, :m]), _bits(want), err_msg=f"{at}: {res.dist[i, :m]} != {want}")
        assert (res.rows[i, m:] == -1).all() and (res.block_ids[i, m:] == -1).all(), at
        assert vis[i] == nv, (at, vis[i], nv)


# ---- 1: every case, every (k, ef) pair ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.CASES))
def test_search_matches_the_oracle(ctx, loaded, name):
    c, oh, corpus, gpu = loaded(name)
    for k, ef in c.pairs:
        res, vis = gpu.search(c.queries, k, ef, c.metric)
        _assert_matches_the_oracle(res, vis, oh, c.metric, c.queries, k, ef, name)
    ctx.screening_check(0)


# ---- 2: the device form: the query tensor's stride is dim, so 1, 3, 5, 127 and 129 load the query element by element ----------------------
def _device_search(gpu, q, k, ef, metric):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    assert d_q.stride(0) == q.shape[1]
    o = {"blk": torch.full((nq, k), 7, dtype=torch.int64, device=dev), "doc": torch.full((nq, k), 7, dtype=torch.int32, device=dev),
         "row": torch.full((nq, k), 7, dtype=torch.int64, device=dev), "dist": torch.full((nq, k), 7.0, dtype=torch.float32, device=dev),
         "cnt": torch.full((nq,), 7, dtype=torch.int32, device=dev), "vis": torch.full((nq,), 7, dtype=torch.int64, device=dev)}
    torch.cuda.synchronize()
    gpu.search_device(p(d_q), nq, k, ef, metric, None, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    gpu.corpus.ctx.synchronize()
    return {key: v.cpu().numpy() for key, v in o.items()}


@pytest.mark.parametrize("name", ec.ROW_LENGTH_CASES)
def test_device_form_equals_the_host_form(ctx, loaded, name):
    c, oh, corpus, gpu = loaded(name)
    for k, ef in c.pairs:
        res, vis = gpu.search(c.queries, k, ef, c.metric)
        dev = _device_search(gpu, c.queries, k, ef, c.metric)
        np.testing.assert_array_equal(dev["cnt"], res.counts)
        np.testing.assert_array_equal(dev["row"], res.rows)
        np.testing.assert_array_equal(dev["blk"], res.block_ids)
        np.testing.assert_array_equal(dev["doc"], res.doc_ids)
        np.testing.assert_array_equal(_bits(dev["dist"]), _bits(res.dist))
        np.testing.assert_array_equal(dev["vis"], vis)
        _assert_matches_the_oracle(res, vis, oh, c.metric, c.queries, k, ef, name)      # ... and both are the oracle's answer
    ctx.screening_check(0)


# ---- 3: 4, 2 and 1 waves per workgroup; one query, and launches whose last workgroup is short ------------------------------------------
@pytest.mark.parametrize("nq", ec.LAUNCH_NQS)
def test_launch_shapes(ctx, loaded, nq):
    c, oh, corpus, gpu = loaded("launch")
    q = c.queries[:nq]
    for k, ef in c.pairs:
        res, vis = gpu.search(q, k, ef, c.metric)
        assert res.rows.shape == (nq, k)
        _assert_matches_the_oracle(res, vis, oh, c.metric, q, k, ef, f"launch nq={nq}")
    ctx.screening_check(0)


# ---- 4: filters over elements with 1 to 10 heap TIDs of which some are permitted ---------------------------------------------------------
@pytest.mark.parametrize("aware", [False, True])
def test_filters_on_the_duplicate_corpus(ctx, loaded, aware):
    import vsrbac
    c, oh, corpus, gpu = loaded("graph-duplicates")
    mask = ec.duplicate_filter_mask()
    nq = len(c.queries)
    gpu.set_predicate_aware(aware)
    try:
        for mode in (vsrbac.BITMAP, vsrbac.RANGES):
            flt = corpus.filter_from_bytemask(mask, mode)
            for k, ef in c.pairs:
                res, vis = gpu.search(c.queries, k, ef, "l2", [flt] * nq)
                for i in range(nq):
                    rows_o, dist_o, _, nv = oh.search_predicate_aware(c.queries[i], ef, mask) if aware else oh.search(c.queries[i], ef)
                    keep = mask[rows_o] != 0
                    want, wd = rows_o[keep][:k], dist_o[keep][:k]
                    at = (aware, mode, k, ef, i)
                    assert res.counts[i] == want.size, (at, res.counts[i], want.size)
                    np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str(at))
                    np.testing.assert_array_equal(_bits(res.dist[i, :want.size]), _bits(ec.reported_distance("l2", wd)), err_msg=str(at))
                    assert (res.block_ids[i, want.size:] == -1).all(), at
                    assert vis[i] == nv, (at, vis[i], nv)
            flt.free()
    finally:
        gpu.set_predicate_aware(False)
    ctx.screening_check(0)


# ---- 5: the iterative form over the same distance loop, against the numpy model of the stream ----------------------------------------------
@pytest.mark.parametrize("mode", ["relaxed_order", "strict_order"])
@pytest.mark.parametrize("dim", ec.ITERATIVE_DIMS)
def test_iterative_matches_the_model(ctx, loaded, dim, mode):
    import vsrbac
    c, oh, corpus, gpu = loaded(f"rows-l2-{dim}")
    q, nq, ef = c.queries, len(c.queries), 40
    g = Graph(oh.export(), c.rows)
    mask = (np.arange(len(c.rows)) % 3 == 0)
    flt = corpus.filter_from_bytemask(mask.astype(np.uint8), vsrbac.BITMAP)
    for max_scan in (50, 20000):                                               # 50: below the first round's count, the drain
        streams = [Stream(IterativeScan(g, q[i], ef, "l2", mode, max_scan)) for i in range(nq)]
        for k in (10, 100):
            for filters, mk in ((None, None), ([flt] * nq, mask)):
                res, tup = gpu.search_iterative(q, k, ef, "l2", filters, mode, max_scan)
                for i in range(nq):
                    rows, d, t = streams[i].answer(k, mk)
                    at = (dim, mode, max_scan, k, mk is not None, i)
                    assert res.counts[i] == rows.size, (at, res.counts[i], rows.size)
                    np.testing.assert_array_equal(res.rows[i, :rows.size], rows, err_msg=str(at))
                    np.testing.assert_array_equal(_bits(res.dist[i, :rows.size]), _bits(ec.reported_distance("l2", d)), err_msg=str(at))
                    assert tup[i] == t, (at, tup[i], t)
                    assert (res.rows[i, rows.size:] == -1).all(), at
    flt.free()
    ctx.screening_check(0)


# ---- 6: the forest form of the body at rows longer than a wave step -----------------------------------------------------------------------
# fp32 at 260 dimensions (65 chunks: a lane group loops), halfvec at 520 (65 chunks of 8: the rounded query lives in the wave's LDS, in
# front of the visited set), bit rows of 8320 bits (65 chunks: the 64 lanes loop).  600 rows, partitions of 1, 129 and 400 rows, 7 queries;
# the expectation is the per-graph searches merged by the numpy model, as in tests/test_gpu_hnsw_forest_search.py.
FOREST_KINDS = [("f32", "l2", 260), ("half", "l2", 520), ("bit", "hamming", 8320)]
FOREST_TASKS = [[0], [1], [2], [0, 1], [2, 1], [0, 1, 2], [2, 2, 0]]


@pytest.mark.parametrize("kind,metric,dim", FOREST_KINDS)
def test_forest_search_of_long_rows(ctx, kind, metric, dim):
    rng = np.random.default_rng(5800 + dim)
    n, nq, k, ef = 600, len(FOREST_TASKS), 10, 40
    blk = (rng.permutation(n) + 1).astype(np.int64)
    doc = rng.permutation(np.arange(n) // 4 + 1).astype(np.int32)
    parts = [rng.choice(n, size, replace=False).astype(np.int64) for size in (1, 129, 400)]
    pick = rng.integers(0, n, nq)
    if kind == "bit":
        x = rng.integers(0, 2, (n, dim)).astype(bool)
        q = x[pick] ^ (rng.random((nq, dim)) < 0.01)
        corpus = ctx.load_corpus_bit(x, None, blk, doc)
    else:
        # integers in -8 .. 8 (binary16 values): a squared distance is an integer of at most dim * 18^2 < 2^20, where sqrt rounded to
        # fp32 keeps distinct values distinct -- the model orders by the reported distance, the library by the squared one
        x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
        q = x[pick] + rng.integers(-2, 3, (nq, dim)).astype(np.float32)
        assert dim * 18 ** 2 < 2 ** 20
        corpus = ctx.load_corpus_half(to_half(x), blk, doc) if kind == "half" else ctx.load_corpus(x, blk, doc)
    indexes = corpus.build_hnsw_partitions(parts, 8, 32, metric, 41)
    forest = corpus.hnsw_forest(indexes)
    try:
        per, vis = {}, {}
        for gi, h in enumerate(indexes):
            per[gi], vis[gi] = (h.search_bit if kind == "bit" else h.search)(q, k, ef, metric)
        res, tvis = (forest.search_bit if kind == "bit" else forest.search)(q, FOREST_TASKS, k, ef, metric)
        w_blk, w_doc, w_row, w_dist, w_cnt = merge_model(per, FOREST_TASKS, k)
        np.testing.assert_array_equal(res.counts, w_cnt)
        np.testing.assert_array_equal(res.rows, w_row)
        np.testing.assert_array_equal(res.block_ids, w_blk)
        np.testing.assert_array_equal(res.doc_ids, w_doc)
        np.testing.assert_array_equal(_bits(res.dist), _bits(w_dist))
        np.testing.assert_array_equal(tvis, [vis[gi][i] for i, graphs in enumerate(FOREST_TASKS) for gi in graphs])
        assert res.counts.tolist() == [1, 10, 10, 10, 10, 10, 10]
        assert set(res.rows[0, :1]) == set(parts[0]) and set(res.rows[1]) <= set(parts[1]) and set(res.rows[2]) <= set(parts[2])
        # the distances are right, not merely equal on both sides: every reported one is the exact distance of its row
        for i in range(nq):
            got = res.rows[i, :res.counts[i]]
            if kind == "bit":
                exact = (x[got] ^ q[i]).sum(axis=1).astype(np.float64)
            else:
                exact = np.sqrt(((x[got].astype(np.float64) - q[i]) ** 2).sum(axis=1))
            np.testing.assert_array_equal(res.dist[i, :res.counts[i]], exact.astype(np.float32), err_msg=f"{kind} query {i}")
    finally:
        forest.free()
        for h in indexes:
            h.free()
        corpus.free()
    ctx.screening_check(0)
