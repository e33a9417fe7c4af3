"""HNSW over halfvec corpora on the GPU (K4h: vsr_hnsw_load_half / vsr_hnsw_build_half, searched by vsr_hnsw_search*).

pgvector computes halfvec distances on the widened operands, so the index oracle's serial build and walk on the widened fp32
rows IS pgvector's halfvec build and walk.  On integer-valued rows (-8 .. 8: exact in binary16, every sum below 2^24) every
order of summation gives the same fp32 value: rows, distances and visited counts must be identical, not close."""
import ctypes
import os

import numpy as np
import pytest

from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_iterative_model import Graph, IterativeScan, Stream
from hnsw_half_model import (TAP_EF, TAP_LIMIT, exact_order, int_queries, int_rows, known_answer_rows, known_answers, recall,
                             round_query, rounding_case, tap_case, to_half, want_dist, widen)

pytestmark = pytest.mark.gpu

NQ = 24
FIELDS = ("block_ids", "doc_ids", "rows", "dist", "counts")


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


_CASES = {}


def _case(ctx, oracle, n, dim, m=16, efc=64, metrics=("l2", "ip")):
    """Integer rows with 40 planted copies of row 100, the oracle's L2 and inner-product graphs on them, the half corpus with
    5 % / 25 % users and both graphs loaded, 24 integer queries (0: the planted row).  Built once per module."""
    key = (n, dim, m)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(2000 + dim + m)
    x = int_rows(rng, n, dim)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), max(1, ndocs // 20), replace=False)]
    perms += [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 4, replace=False)]
    ur = [(1, 1), (2, 2)]
    corpus = ctx.load_corpus_half(to_half(x), blk, doc)
    corpus.load_rbac(ur, perms)
    c = {"n": n, "dim": dim, "x": x, "corpus": corpus, "q": int_queries(rng, x, NQ), "blk": blk, "doc": doc,
         "masks": {u: oracle.user_row_mask(u, ur, perms, doc).astype(bool) for u in (1, 2)}, "oh": {}, "export": {}, "gpu": {}}
    for metric in metrics:
        oh = OracleHnsw(oracle, metric, x, m=m, ef_construction=efc, seed=5)
        g = oh.export()
        # (under L2 a copy's nearest neighbour is its twin: the serial build folds the copies into elements of 10 TIDs)
        assert metric != "l2" or m != 16 or g["tid_count"].max() == 10
        c["oh"][metric], c["export"][metric], c["gpu"][metric] = oh, g, corpus.load_hnsw_half(g)
    _CASES[key] = c
    return c


def _check_walk(c, metric, ef, k=600, q=None, ask=None):
    """The GPU's answer to `ask` (default: q) equals the oracle's walk of q."""
    q = c["q"] if q is None else q
    gpu, oh = c["gpu"][metric], c["oh"][metric]
    res, vis = gpu.search(q if ask is None else ask, k, ef, metric)
    for i in range(len(q)):
        rows_o, dist_o, _, nv = oh.search(q[i], ef)
        want = rows_o[:k]
        where = (metric, ef, i)
        assert res.counts[i] == want.size, (where, res.counts[i], want.size)
        np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str(where))
        np.testing.assert_array_equal(res.dist[i, :want.size], want_dist(metric, dist_o[:k]), err_msg=str(where))
        assert vis[i] == nv, (where, vis[i], nv)
        assert (res.rows[i, want.size:] == -1).all()
    return res


# (n, dim): one partial chunk; C = 2 with a partial second chunk (the TAP shape); full chunks; C = 13, G = 16: idle lanes and a
# partial chunk; C = G = 16; C = 17, G = 32; C = 65: the chunk loop with a one-chunk tail; C = 96: the chunk loop
SHAPES = [(3000, 3), (3000, 10), (3000, 16), (3000, 100), (3000, 128), (2000, 129), (1200, 520), (1200, 768)]


# ---- 1. walk parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", SHAPES)
def test_walk_is_the_oracle_walk(ctx, oracle, n, dim):
    c = _case(ctx, oracle, n, dim)
    for metric in ("l2", "ip"):
        for ef in (10, 40, 500):
            res = _check_walk(c, metric, ef)
        if metric == "l2":
            # the planted row: its copies come out at distance 0, an element's TIDs newest first
            cnt = res.counts[0]
            zero = res.rows[0, :cnt][res.dist[0, :cnt] == 0]
            assert set(range(n // 2, n // 2 + 40)) | {100} <= set(zero.tolist())
            g = c["export"]["l2"]
            full = np.flatnonzero(g["tid_count"] == 10)[0]
            at = int(np.flatnonzero(res.rows[0, :cnt] == g["tids"][full, 9])[0])
            np.testing.assert_array_equal(res.rows[0, at:at + 10], g["tids"][full, ::-1])


@pytest.mark.parametrize("n,dim,m,efc,metrics", [(1500, 64, 100, 200, ("l2",)), (1500, 64, 4, 32, ("l2", "ip"))])
def test_walk_wide_and_narrow_lists(ctx, oracle, n, dim, m, efc, metrics):
    """m = 100: 2m = 200 neighbours per expansion (the oracle's serial build at m = 100 takes ~20 s per graph, and the width of a
    list does not meet the metric anywhere in the kernel: one metric there); m = 4: lists of 8, both metrics."""
    c = _case(ctx, oracle, n, dim, m, efc, metrics)
    for metric in metrics:
        for ef in (10, 40, 500):
            _check_walk(c, metric, ef)


# ---- 2. the same answer as K4 over the widened rows ------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(3000, 10), (3000, 128), (1200, 520)])
def test_same_answer_as_fp32_index_on_the_same_graph(ctx, oracle, n, dim):
    import vsrbac
    c = _case(ctx, oracle, n, dim)
    twin = ctx.load_corpus(widen(to_half(c["x"])), c["blk"], c["doc"])
    twin.load_rbac([(2, 2)], [(2, int(d)) for d in np.unique(c["doc"][c["masks"][2]])])
    for metric in ("l2", "ip"):
        half, full = c["gpu"][metric], twin.load_hnsw(c["export"][metric])
        assert half.device_bytes() == full.device_bytes() > 0
        for flt_h, flt_f in ((None, None), ([c["corpus"].filter_for_user(2, vsrbac.BITMAP)] * NQ, [twin.filter_for_user(2, vsrbac.BITMAP)] * NQ)):
            for ef in (10, 40, 500):
                a, va = half.search(c["q"], 100, ef, metric, flt_h)
                b, vb = full.search(c["q"], 100, ef, metric, flt_f)
                for f in FIELDS:
                    assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (metric, ef, f)
                assert va.tobytes() == vb.tobytes()
        full.free()
    twin.free()


# ---- the device entry points -------------------------------------------------------------------------------------------------
def _device(gpu, q, k, ef, metric, flt=None, iterative=None):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.empty((nq,), dtype=torch.int64, device=dev)}
    if iterative:
        keep = gpu.search_iterative_device(p(d_q), nq, k, ef, metric, flt, iterative[0], iterative[1], p(o["blk"]), p(o["doc"]),
                                           p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    else:
        keep = gpu.search_device(p(d_q), nq, k, ef, metric, flt, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]),
                                 p(o["vis"]))
    gpu.corpus.ctx.synchronize()
    del keep
    return {key: v.cpu().numpy() for key, v in o.items()}


def _same(d, host, vis):
    np.testing.assert_array_equal(d["row"], host.rows)
    np.testing.assert_array_equal(d["blk"], host.block_ids)
    np.testing.assert_array_equal(d["doc"], host.doc_ids)
    np.testing.assert_array_equal(d["dist"], host.dist)
    np.testing.assert_array_equal(d["cnt"], host.counts)
    np.testing.assert_array_equal(d["vis"], vis)


# ---- 3. query rounding ---------------------------------------------------------------------------------------------------
def test_queries_are_rounded_to_binary16(ctx, oracle):
    """Raw queries (x + 2**-12, 2049) answer exactly as their rounded copies and as the oracle's walk of the rounded copies;
    the oracle's walk of the RAW fp32 queries is another answer, so the rounding is applied and not skipped."""
    x, raw, rounded = rounding_case()
    corpus = ctx.load_corpus_half(to_half(x))
    oh = OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=5)
    gpu = corpus.load_hnsw_half(oh.export())
    c = {"gpu": {"l2": gpu, "ip": gpu}, "oh": {"l2": oh}}
    differ = 0
    for ef in (40, 200):
        res = _check_walk(c, "l2", ef, k=300, q=rounded, ask=raw)
        pre, vis = gpu.search(rounded, 300, ef, "l2")
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(res, f), getattr(pre, f))
        _same(_device(gpu, raw, 300, ef, "l2"), pre, vis)
        for i in range(len(raw)):
            rows_raw, dist_raw, _, _ = oh.search(raw[i], ef)
            n = min(rows_raw.size, 300)
            differ += int(res.counts[i] != n or (res.rows[i, :n] != rows_raw[:n]).any() or
                          (res.dist[i, :n] != want_dist("l2", dist_raw[:n])).any())
        for f in FIELDS:                                     # inner product on the same graph: raw == rounded as well
            np.testing.assert_array_equal(getattr(gpu.search(raw, 300, ef, "ip")[0], f), getattr(gpu.search(rounded, 300, ef, "ip")[0], f))
    assert differ >= 1
    gpu.free()
    corpus.free()


# ---- 4. filters ------------------------------------------------------------------------------------------------------------
def test_filters_plain_and_predicate_aware(ctx, oracle):
    import vsrbac
    c = _case(ctx, oracle, 3000, 128)
    corpus, k = c["corpus"], 20
    for metric in ("l2", "ip"):
        gpu, oh = c["gpu"][metric], c["oh"][metric]
        for user in (1, 2):
            mask = c["masks"][user]
            for mode in (vsrbac.BITMAP, vsrbac.RANGES):
                flt = [corpus.filter_for_user(user, mode)] * NQ
                for ef in (20, 100):
                    for aware in (False, True):
                        gpu.set_predicate_aware(aware)
                        res, vis = gpu.search(c["q"], k, ef, metric, flt)
                        for i in range(NQ):
                            rows_o, dist_o, _, nv = (oh.search_predicate_aware(c["q"][i], ef, mask.astype(np.uint8)) if aware
                                                     else oh.search(c["q"][i], ef))
                            keep = mask[rows_o]
                            want, wd = rows_o[keep][:k], dist_o[keep][:k]
                            where = (metric, user, mode, ef, aware, i)
                            assert res.counts[i] == want.size, where
                            np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str(where))
                            np.testing.assert_array_equal(res.dist[i, :want.size], want_dist(metric, wd), err_msg=str(where))
                            assert vis[i] == nv, where
                    gpu.set_predicate_aware(False)


# ---- 5. iterative scans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_iterative_matches_the_model(ctx, oracle, metric, monkeypatch):
    import vsrbac
    c = _case(ctx, oracle, 3000, 128)
    corpus, gpu, q = c["corpus"], c["gpu"][metric], c["q"][:12]
    g = Graph(c["export"][metric], c["x"])
    nq, ef = len(q), 40
    filters = {"none": (None, None), "5%": ([corpus.filter_for_user(1, vsrbac.BITMAP)] * nq, c["masks"][1])}

    def check(modes, scans, ks):
        for mode in modes:
            for max_scan in scans:
                streams = [Stream(IterativeScan(g, q[i], ef, metric, mode, max_scan)) for i in range(nq)]
                for k in ks:
                    for fname, (flt, mask) in filters.items():
                        res, tup = gpu.search_iterative(q, k, ef, metric, flt, mode, max_scan)
                        for i in range(nq):
                            rows, d, t = streams[i].answer(k, mask)
                            where = (metric, mode, max_scan, k, fname, i)
                            assert res.counts[i] == rows.size, (where, res.counts[i], rows.size)
                            np.testing.assert_array_equal(res.rows[i, :rows.size], rows, err_msg=str(where))
                            np.testing.assert_array_equal(res.dist[i, :rows.size], want_dist(metric, d), err_msg=str(where))
                            assert tup[i] == t, (where, tup[i], t)

    check(("relaxed_order", "strict_order"), (1, 200, 20000), (5, 60))
    monkeypatch.setenv("VSR_HNSW_DISCARD_CAP", "64")         # D overflows: the host entry point re-runs with room for every element
    check(("relaxed_order",), (20000,), (60,))
    monkeypatch.delenv("VSR_HNSW_DISCARD_CAP")
    flt5 = filters["5%"][0]
    for mode in ("relaxed_order", "strict_order"):           # the prefix property
        a, _ = gpu.search_iterative(q, 20, ef, metric, flt5, mode, 20000)
        b, _ = gpu.search_iterative(q, 80, ef, metric, flt5, mode, 20000)
        for i in range(nq):
            assert a.counts[i] == min(20, b.counts[i])
            np.testing.assert_array_equal(a.rows[i, :a.counts[i]], b.rows[i, :a.counts[i]])
            np.testing.assert_array_equal(a.dist[i, :a.counts[i]], b.dist[i, :a.counts[i]])
    for flt, _ in filters.values():                          # mode off is search, bit for bit
        a, vis = gpu.search(q, 60, ef, metric, flt)
        b, tup = gpu.search_iterative(q, 60, ef, metric, flt, mode="off")
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        np.testing.assert_array_equal(vis, tup)


# ---- 6. visited forms and the device API -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(2000, 129), (1200, 520)])   # the query in registers / in the wave's LDS
def test_visited_forms_and_device_entry_points(ctx, oracle, monkeypatch, n, dim):
    import vsrbac
    c = _case(ctx, oracle, n, dim)
    corpus, q, k, ef = c["corpus"], c["q"], 50, 40
    flt = [corpus.filter_for_user(2, vsrbac.BITMAP)] * NQ
    for metric in ("l2", "ip"):
        gpu = c["gpu"][metric]
        for f in (None, flt):
            host, vis = gpu.search(q, k, ef, metric, f)
            _same(_device(gpu, q, k, ef, metric, f), host, vis)
            hi, tup = gpu.search_iterative(q, k, ef, metric, f, "relaxed_order", 500)
            _same(_device(gpu, q, k, ef, metric, f, ("relaxed_order", 500)), hi, tup)
    lds = _check_walk(c, "l2", 40)
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:64")        # the LDS hash overflows: the host entry point re-runs, the device one reports
    re_run = _check_walk(c, "l2", 40)
    d = _device(c["gpu"]["l2"], q, k, ef, "l2")
    assert (d["cnt"] == -1).all() and (d["row"] == -1).all()
    monkeypatch.setenv("VSR_HNSW_VISITED", "global")
    glob = _check_walk(c, "l2", 40)
    monkeypatch.delenv("VSR_HNSW_VISITED")
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(lds, f), getattr(glob, f))
        np.testing.assert_array_equal(getattr(lds, f), getattr(re_run, f))


# ---- 7. build ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_build_reaches_the_tap_floor(ctx, oracle, metric):
    """024_hnsw_halfvec_build_recall.pl's case and floor (0.98 for every opclass; the rows and seeds of
    tests/test_hnsw_half_cpu.py), and recall within 0.01 of the oracle's serial build on the same rows."""
    rows_half, q = tap_case(metric)
    corpus = ctx.load_corpus_half(rows_half)
    exact = corpus.search(q, TAP_LIMIT, metric)              # truth as the operator ranks it, on the half corpus
    expected = [exact.rows[i, :exact.counts[i]] for i in range(len(q))]
    assert all(len(e) == TAP_LIMIT for e in expected)
    gpu = corpus.build_hnsw_half(16, 64, metric, seed=1)
    n_elem, entry, entry_level, max_level = gpu.info()
    assert n_elem == len(rows_half) and 0 <= entry < n_elem and 1 <= entry_level <= max_level
    res, _ = gpu.search(q, TAP_LIMIT, TAP_EF, metric)
    r = recall([res.rows[i, :res.counts[i]] for i in range(len(q))], expected)
    oh = OracleHnsw(oracle, metric, widen(rows_half), m=16, ef_construction=64, seed=1)
    rq = round_query(q)
    ro = recall([oh.search(rq[i], TAP_EF)[0][:TAP_LIMIT] for i in range(len(q))], expected)
    print(f"build_hnsw_half {metric}: recall@{TAP_LIMIT} ef={TAP_EF} = {r:.4f} (floor 0.98), oracle serial build {ro:.4f}")
    assert r >= 0.98, (r, ro)
    assert r >= ro - 0.01, (r, ro)
    gpu.free()
    corpus.free()


def test_build_on_clustered_real_rows_reports_the_types_distances(ctx):
    """4000 x 128 clustered real-valued rows: every reported distance within 1e-4 relative of the distance recomputed in
    float64 from the widened rows and the rounded query (128 fp32 fmaf steps: ~128 * 2^-24 = 8e-6 relative at the worst)."""
    rng = np.random.default_rng(4128)
    n, dim, k = 4000, 128, 20
    centres = rng.normal(0, 1, (40, dim))
    rows_half = to_half(centres[rng.integers(0, 40, n)] + rng.normal(0, 0.3, (n, dim)))
    q = (centres[rng.integers(0, 40, 32)] + rng.normal(0, 0.3, (32, dim))).astype(np.float32)
    corpus = ctx.load_corpus_half(rows_half)
    gpu = corpus.build_hnsw_half(16, 64, "l2", seed=2)
    res, _ = gpu.search(q, k, 100, "l2")
    x64, q64 = widen(rows_half).astype(np.float64), round_query(q).astype(np.float64)
    assert (res.counts == k).all()
    for i in range(len(q)):
        want = np.sqrt(((x64[res.rows[i]] - q64[i]) ** 2).sum(axis=1))
        np.testing.assert_allclose(res.dist[i].astype(np.float64), want, rtol=1e-4, atol=0)
        assert (np.diff(res.dist[i]) >= 0).all()
    exact = corpus.search(q, k, "l2")
    r = recall([res.rows[i] for i in range(len(q))], [exact.rows[i] for i in range(len(q))])
    print(f"4000 x 128 clustered halfvec rows: recall@{k} ef=100 = {r:.4f}")
    assert r >= 0.9
    gpu.free()
    corpus.free()


# ---- 8. merging build --------------------------------------------------------------------------------------------------------
def test_merging_build(ctx, monkeypatch):
    """3000 x 5 rows over {-1, 0, 1} (243 possible values: full of duplicates), a planted group of 25 holding a value of their
    own, and a pair that differs only in the sign of a zero."""
    rng = np.random.default_rng(55)
    n, dim = 3000, 5
    x = rng.integers(-1, 2, (n, dim)).astype(np.float16)
    planted = np.array([1, -1, 1, -1, 1], dtype=np.float16)
    x[(x == planted).all(axis=1), 0] = 0                     # nobody else holds the planted value
    spots = np.sort(rng.choice(n, 27, replace=False))
    where, a, b = spots[:25], int(spots[25]), int(spots[26])
    x[where] = planted
    x[a] = np.array([1, 0.0, 1, 1, -1], dtype=np.float16)
    x[b] = np.array([1, -0.0, 1, 1, -1], dtype=np.float16)
    assert x[a].tobytes() != x[b].tobytes() and (x[a] == x[b]).all()
    corpus = ctx.load_corpus_half(x)
    merged = corpus.build_hnsw_half(8, 32, "l2", seed=11, merge_duplicates=True)
    plain = corpus.build_hnsw_half(8, 32, "l2", seed=11)
    g, gp = merged.export(), plain.export()
    groups = {}
    for r in range(n):
        groups.setdefault(x[r].tobytes(), []).append(r)
    want = sorted(tuple(rows[i:i + 10]) for rows in groups.values() for i in range(0, len(rows), 10))
    tuples = lambda gg: [tuple(int(t) for t in gg["tids"][e, :gg["tid_count"][e]]) for e in range(len(gg["level"]))]
    assert merged.info()[0] == len(g["level"]) == sum(-(-len(rows) // 10) for rows in groups.values())
    assert sorted(tuples(g)) == want                         # ceil(g / 10) elements per group, members in insertion order
    assert (b,) in tuples(g) and not any(a in t and b in t for t in tuples(g))       # +0.0 / -0.0: not merged
    assert (np.diff(g["tids"][:, 0]) > 0).all(), "elements are numbered by their first member"
    assert len(gp["level"]) == n and (gp["tid_count"] == 1).all() and (gp["tids"][:, 0] == np.arange(n)).all()
    assert (g["level"] == gp["level"][g["tids"][:, 0]]).all()            # the same seed: the same levels
    res, _ = merged.search(planted[None, :].astype(np.float32), 100, 400, "l2")
    zero = res.rows[0, :res.counts[0]][res.dist[0, :res.counts[0]] == 0]
    assert sorted(zero.tolist()) == where.tolist()
    monkeypatch.setenv("VSR_HNSW_DEDUP_HASH_BITS", "3")      # eight hash values: the collision path
    collide = corpus.build_hnsw_half(8, 32, "l2", seed=11, merge_duplicates=True)
    monkeypatch.delenv("VSR_HNSW_DEDUP_HASH_BITS")
    assert sorted(tuples(collide.export())) == want
    again = corpus.load_hnsw_half(g)                          # the export, loaded, answers like the exported index
    qs = x[rng.integers(0, n, 16)].astype(np.float32) + rng.integers(-1, 2, (16, dim)).astype(np.float32)
    for metric in ("l2", "ip"):
        for ef in (10, 100):
            p, vp = merged.search(qs, 50, ef, metric)
            r, vr = again.search(qs, 50, ef, metric)
            for f in FIELDS:
                assert getattr(p, f).tobytes() == getattr(r, f).tobytes()
            np.testing.assert_array_equal(vp, vr)
    for h in (again, collide, merged, plain):
        h.free()
    corpus.free()


# ---- 9. known answers ----------------------------------------------------------------------------------------------------------
def test_pgvector_known_answers(ctx, golden_dir):
    """test/sql/hnsw_halfvec.sql: build_hnsw_half reproduces each expected order."""
    for case in known_answers(golden_dir):
        held, orig = known_answer_rows(case)
        corpus = ctx.load_corpus_half(to_half(held))
        gpu = corpus.build_hnsw_half(16, 64, case["metric"], seed=1)
        q = np.array([case["query"]], dtype=np.float32)
        if case["metric"] == "cosine":
            q /= np.linalg.norm(q)
        res, _ = gpu.search(q, len(held), 40, case["metric"])
        assert res.counts[0] == len(held)
        assert orig[res.rows[0]].astype(int).tolist() == case["expected"], (case["opclass"], res.rows[0], res.dist[0])
        gpu.free()
        corpus.free()


# ---- 10. errors and memory -----------------------------------------------------------------------------------------------------
def test_errors_and_memory(ctx, oracle):
    from vsrbac import VsrError
    c = _case(ctx, oracle, 3000, 10)
    corpus, gpu, g, q, dim = c["corpus"], c["gpu"]["l2"], c["export"]["l2"], c["q"], c["dim"]

    def refused(status, word, fn, *a, **kw):
        with pytest.raises(VsrError) as e:
            fn(*a, **kw)
        assert e.value.status == status and word in str(e.value), (status, word, e.value.status, str(e.value))

    # the old entry points keep refusing a halfvec corpus and name the new ones
    for fn, args, kw in ((corpus.load_hnsw, (g,), {}), (corpus.build_hnsw, (16, 64, "l2"), {}),
                         (corpus.build_hnsw, (16, 64, "l2"), {"merge_duplicates": True})):
        refused(6, "halfvec", fn, *args, **kw)
        refused(6, "vsr_hnsw_load_half", fn, *args, **kw)
        refused(6, "vsr_hnsw_build_half", fn, *args, **kw)
    # the new ones refuse any other corpus
    full = ctx.load_corpus(c["x"][:200])
    refused(1, "not a halfvec corpus", full.load_hnsw_half, g)
    refused(1, "not a halfvec corpus", full.build_hnsw_half, 16, 64, "l2")
    full.free()
    bits = ctx.load_corpus_bit(np.zeros((8, 2), np.uint8), 16)
    refused(1, "not a halfvec corpus", bits.build_hnsw_half, 16, 64, "l2")
    bits.free()
    wide = ctx.load_corpus_half(np.zeros((4, 4001), np.float16))
    refused(6, "column cannot have more than 4000 dimensions for hnsw index", wide.build_hnsw_half, 16, 64, "l2")
    refused(6, "column cannot have more than 4000 dimensions for hnsw index", wide.load_hnsw_half, g)
    wide.free()
    # m, ef_construction, flags' companions and metrics as vsr_hnsw_build_ex checks them
    refused(6, "m must be", corpus.build_hnsw_half, 101, 400, "l2")
    refused(6, "m must be", corpus.build_hnsw_half, 1, 64, "l2")
    refused(6, "ef_construction", corpus.build_hnsw_half, 16, 31, "l2")
    refused(6, "ef_construction", corpus.build_hnsw_half, 16, 1001, "l2")
    refused(6, "operator classes only", corpus.build_hnsw_half, 16, 64, "l1")
    refused(6, "m must be", corpus.load_hnsw_half, dict(g, m=101))
    h = ctypes.c_void_p()
    lib = corpus._lib
    assert lib.vsr_hnsw_build_half(corpus._h, 16, 64, 0, 1, 2, ctypes.byref(h)) == 1      # an unknown flag bit
    # searches
    refused(6, "L1", gpu.search, q, 10, 40, "l1")
    refused(6, "L1", gpu.search_iterative, q, 10, 40, "l1")
    refused(2, f"different halfvec dimensions {dim} and {dim + 1}", gpu.search, np.zeros((1, dim + 1), np.float32), 10, 40, "l2")
    refused(1, "ef_search", gpu.search, q, 10, 0, "l2")
    refused(1, "max_scan_tuples", gpu.search_iterative, q, 10, 40, "l2", max_scan_tuples=0)
    bad = q.copy()
    bad[3, 2] = 65520.0
    refused(1, '"65520" is out of range for type halfvec', gpu.search, bad, 10, 40, "l2")
    refused(1, '"65520" is out of range for type halfvec', gpu.search_iterative, bad, 10, 40, "l2")
    bad[3, 2] = -70000.0
    refused(1, '"-70000" is out of range for type halfvec', gpu.search, bad, 10, 40, "l2")
    bad[3, 2] = 65519.0                                      # rounds to 65504: accepted
    res, _ = gpu.search(bad, 10, 40, "l2")
    assert (res.counts == 10).all()
    d = _device(gpu, np.where(np.abs(bad) > 60000, np.float32(70000.0), bad), 10, 40, "l2")     # the device entry point does not look
    assert (d["cnt"] >= 0).all()
    refused(1, "not over a bit corpus", gpu.search_bit, np.zeros((1, 2), np.uint8), 10, 40, "hamming", dim=dim)
    gpu.set_predicate_aware(True)
    refused(6, "predicate-aware", gpu.search_iterative, q, 10, 40, "l2")
    gpu.set_predicate_aware(False)
    # memory: the graph arrays only, the same as an fp32 index of the same graph; no fp32 image of the rows
    twin = ctx.load_corpus(c["x"])
    tw = twin.load_hnsw(g)
    ne, m, n_upper = len(g["level"]), g["m"], int((g["up_slot"] >= 0).sum())
    assert gpu.device_bytes() == tw.device_bytes() == 4 * (ne * 4 + ne * 2 * m + ne * 10 + n_upper * g["max_level"] * m)
    assert corpus.device_bytes() < twin.device_bytes()
    tw.free()
    twin.free()
    # every handle works afterwards
    _check_walk(c, "l2", 40)
