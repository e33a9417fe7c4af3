"""K1sm (vsr_scansm.h, Context.set_sparse_shared) against tests/sparse_model.py.  Integer-valued cases (values in -8..8: every
fp32 sum is exact in any order, as tests/test_gpu_sparsevec.py argues) are compared for EQUALITY of rows, ids, fp32 distances and
counts; real-valued cases within the README's 1e-4.  Every search names its kernel: K1sm with its QW (32 when the call's longest
query has <= 8 non-zeros, 16 up to 32, at k <= 100), or K1s where a call stays there."""
import numpy as np
import pytest

import sparse_model
from sparse_model import SparseModel

pytestmark = pytest.mark.gpu

METRICS = sparse_model.METRICS
HASH_MUL = 2654435761                                         # SPARSE_HASH_MUL, vsr_device.h
NNZ = {32: 8, 16: 32}                                         # QW -> the longest query that still gets it
EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.float32))


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    c.set_sparse_shared(True)
    yield c
    c.close()


_ints = lambda rng, m: (rng.integers(1, 9, m) * rng.choice([-1, 1], m)).astype(np.float32)
_ids = lambda n: ((np.arange(n) + 1).astype(np.int64), (np.arange(n) // 7 + 1).astype(np.int32))   # internal order = caller order


def _vec(rng, pool, nnz, values=_ints):
    ix = np.sort(rng.choice(pool, size=min(nnz, pool.size), replace=False)).astype(np.int32)
    return ix, values(rng, ix.size)


def _load(ctx, rows, dim, blk=None, doc=None):
    indptr, indices, values = sparse_model.csr(rows)
    return ctx.load_corpus_sparse(indptr, indices, values, dim, blk, doc), SparseModel(indptr, indices, values, dim, doc, blk)


def _check(ctx, corpus, model, queries, k, metric, filters=None, masks=None, kernel="K1sm", close=False):
    indptr, indices, values = sparse_model.csr(queries)
    res = corpus.search_sparse(indptr, k, metric, filters, indices=indices, values=values)
    name = ctx.last_scan_kernel()
    assert "scans_kernel" in name if kernel == "K1s" else "scansm_kernel" in name and "K1sm" in name and kernel in name, name
    for i, (qi, qx) in enumerate(queries):
        want = model.distances(metric, qi, qx)
        idx, d = model.topk(want, k, None if masks is None else masks[i])
        m = res.counts[i]
        assert m == idx.size, (i, m, idx.size)
        assert (res.rows[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
        if close:
            assert len(set(res.rows[i, :m].tolist())) == m
            np.testing.assert_allclose(res.dist[i, :m], want[res.rows[i, :m]], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(res.dist[i, :m], d, rtol=1e-4, atol=1e-4)
            continue
        np.testing.assert_array_equal(res.rows[i, :m], idx)
        assert (res.block_ids[i, :m] == model.blk[idx]).all() and (res.doc_ids[i, :m] == model.doc[idx]).all()
        np.testing.assert_array_equal(res.dist[i, :m], d)     # (NaN == NaN here)
    return res


@pytest.fixture(scope="module")
def small(ctx):
    # 300 rows of 0..40 entries at dim = 1000, two of them empty, under a small RBAC
    rng = np.random.default_rng(1)
    n, dim = 300, 1000
    pool = rng.choice(dim, size=120, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(n)]
    rows[5] = rows[77] = EMPTY
    blk, doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 31, n).astype(np.int32)
    corpus, model = _load(ctx, rows, dim, blk, doc)
    perms = sorted({(r, int(d)) for r in (1, 2, 3) for d in rng.choice(np.arange(1, 31), size=12, replace=False)})
    ur = [(1, 1), (1, 2), (2, 2), (2, 3)]
    corpus.load_rbac(ur, perms)
    masks = {u: sparse_model.user_row_mask(u, ur, perms, doc) for u in (1, 2)}
    yield corpus, model, pool, masks
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qw,dq", [(qw, dq) for qw in (16, 32) for dq in (2 - qw, -1, 0, 1)])
def test_queries_per_pass(ctx, small, qw, dq, metric):
    """2, QW - 1, QW, QW + 1 queries, the first empty (cosine: NaN, id order); unfiltered and under two users' RANGES / BITMAP filters."""
    import vsrbac
    corpus, model, pool, masks = small
    rng = np.random.default_rng(qw + dq)
    nq = qw + dq
    queries = [EMPTY, _vec(rng, pool, NNZ[qw])] + [_vec(rng, pool, int(rng.integers(1, NNZ[qw] + 1))) for _ in range(nq - 2)]
    _check(ctx, corpus, model, queries, 10, metric, kernel=f"QW={qw}")
    users = [1 + (i // 2) % 2 for i in range(nq)]
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        fs = {u: corpus.filter_for_user(u, mode) for u in (1, 2)}
        _check(ctx, corpus, model, queries, 10, metric, [fs[u] for u in users], [masks[u] for u in users], kernel=f"QW={qw}")


@pytest.mark.parametrize("qw", [16, 32])
def test_row_lengths_around_a_load_round(ctx, qw):
    """Row lengths around a round of 2 QW entries (odd: the pad entry must miss); a step / all but one row of a tile denied."""
    rng = np.random.default_rng(qw)
    n, dim, R = 150, 1000, 64 // qw
    pool = rng.choice(dim, size=400, replace=False)
    lengths = [0, 1, 2, 2 * qw - 1, 2 * qw, 2 * qw + 1, 300]
    rows = [_vec(rng, pool, lengths[i % 7]) for i in range(n)]
    corpus, model = _load(ctx, rows, dim, *_ids(n))
    queries = [_vec(rng, pool, NNZ[qw]) for _ in range(3)]
    at = np.arange(n)
    no_step, one_row = at >= R, (at < 64) | (at >= 128) | (at == 64 + 37)
    for metric in METRICS:
        _check(ctx, corpus, model, queries, 20, metric, kernel=f"QW={qw}")
        for mask in (no_step, one_row):
            f = corpus.filter_from_bytemask(mask)
            _check(ctx, corpus, model, queries, 20, metric, [f] * 3, [mask] * 3, kernel=f"QW={qw}")
            f.free()
    corpus.free()


@pytest.mark.parametrize("qw", [16, 32])
@pytest.mark.parametrize("kind", ["same", "disjoint", "collide"])
def test_union_table_at_its_bounds(ctx, kind, qw):
    """One index set for all; disjoint sets (the most columns); one home slot, the last (the chain wraps).  dim = 10^9."""
    rng = np.random.default_rng(qw + len(kind))
    dim, nnz = 1_000_000_000, NNZ[qw]
    uslots, want = qw * 2 * nnz, qw * nnz // 4                # scansm_union_slots: QW x the call's per-query table
    if kind == "collide":
        cand = np.arange(0, 1_500_000, dtype=np.uint64)
        home = ((cand * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - int(np.log2(uslots)))
        own = cand[home == np.uint64(uslots - 1)][:want].astype(np.int64)
        assert own.size == want
    else:
        m = (nnz if kind == "same" else qw * nnz) - 1
        own = np.append(rng.permutation(np.unique(rng.integers(0, dim - 1, 2 * m)))[:m], dim - 1)
    if kind == "disjoint":
        sets = np.split(rng.permutation(own), qw)
        queries = [(np.sort(s).astype(np.int32), _ints(rng, nnz)) for s in sets]
    else:
        queries = [_vec(rng, own, nnz) for _ in range(qw)]
    pool = np.concatenate([own, np.setdiff1d(rng.integers(0, dim, 200), own)])
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(200)]
    rows[0] = _vec(rng, own, 40)
    corpus, model = _load(ctx, rows, dim, *_ids(200))
    for metric in METRICS:
        _check(ctx, corpus, model, queries, 10, metric, kernel=f"QW={qw}")
    corpus.free()


@pytest.mark.parametrize("case", ["overflow", "ties", 9, 10, 11])
def test_candidate_protocol(ctx, case):
    """overflow: 6000 rows, each nearer than the last, one workgroup (cap = 2048), then the default launch: compactions run.  ties: nine rows
    in ten share no index with the queries, so <#> ties at 0 and ids decide.  9, 10, 11: that many permitted rows at k = 10."""
    rng = np.random.default_rng(4)
    one = lambda v: (np.array([2], np.int32), np.array([v], np.float32))
    if case == "overflow":
        n = 6000
        corpus, model = _load(ctx, [one(float(r + 1)) for r in range(n)], 8)
        for metric, queries in (("ip", [one(1.0), one(2.0)]), ("l1", [one(30000.0), one(40000.0)])):
            assert (np.diff(model.distances(metric, *queries[0])) < 0).all()
            for budget in (1, 0):
                ctx.tune(block_budget=budget)
                _check(ctx, corpus, model, queries, 10, metric, kernel="QW=32")
        ctx.tune(block_budget=0)
    elif case == "ties":
        n, dim = 3000, 1000
        rows = [_vec(rng, np.arange(10), 3) if i % 10 == 0 else _vec(rng, np.arange(500, 1000), 5) for i in range(n)]
        corpus, model = _load(ctx, rows, dim, rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 41, n).astype(np.int32))
        queries = [(np.arange(10, dtype=np.int32), np.abs(_ints(rng, 10))) for _ in range(3)]
        res = _check(ctx, corpus, model, queries, 400, "ip", kernel="QW=16")
        assert (res.dist[:, -1] == 0).all()
    else:
        n = 200
        rows = [_vec(rng, np.arange(50), 6) for _ in range(n)]
        corpus, model = _load(ctx, rows, 50, *_ids(n))
        mask = np.zeros(n, dtype=bool)
        mask[rng.choice(n, size=case, replace=False)] = True
        f = corpus.filter_from_bytemask(mask)
        queries = [_vec(rng, np.arange(50), 8) for _ in range(4)]
        for metric in METRICS:
            res = _check(ctx, corpus, model, queries, 10, metric, [f] * 4, [mask] * 4, kernel="QW=32")
            assert (res.counts == min(case, 10)).all()
        f.free()
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
def test_real_values(ctx, metric):
    """Within 1e-4 of the model; a corpus row as the query (L2, L1) comes out within 1e-6 |q| of 0, never NaN."""
    rng = np.random.default_rng(5)
    n, dim = 700, 30522
    pool = rng.choice(dim, size=300, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(8, 33)), lambda r, m: ((r.normal(size=m) + 3) * 100).astype(np.float32)) for _ in range(n)]
    corpus, model = _load(ctx, rows, dim)
    pick = rng.integers(0, n, 20)
    res = _check(ctx, corpus, model, [rows[i] for i in pick], 5, metric, kernel="QW=16", close=True)
    assert not np.isnan(res.dist).any()
    if metric in ("l2", "l1"):
        for j, i in enumerate(pick):
            qn = float(np.sqrt((rows[i][1].astype(np.float64) ** 2).sum()))
            assert res.rows[j, 0] == i and 0 <= res.dist[j, 0] <= 1e-6 * qn, (metric, i, res.dist[j, 0], qn)
    corpus.free()


def test_routing(monkeypatch):
    """Default off; on by call or environment.  On: one query, or a 33-entry query (no block at QW = 16), stay on K1s."""
    import vsrbac
    rng = np.random.default_rng(6)
    n, dim = 500, 1000
    pool = rng.choice(dim, size=150, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(n)]
    queries = [_vec(rng, pool, 8) for _ in range(5)]
    for env, call, shared in ((None, False, "K1s"), (None, True, "QW=32"), ("1", False, "QW=32")):
        if env:
            monkeypatch.setenv("VSR_SPARSE_SHARED", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_SPARSE_SHARED", raising=False)
        if call:
            c.set_sparse_shared(True)
        corpus, model = _load(c, rows, dim, *_ids(n))
        for metric in METRICS:
            _check(c, corpus, model, queries, 10, metric, kernel=shared)
            _check(c, corpus, model, queries[:1], 10, metric, kernel="K1s")
            _check(c, corpus, model, queries + [_vec(rng, pool, 33)], 10, metric, kernel="K1s")
        if call:
            c.set_sparse_shared(False)
            _check(c, corpus, model, queries, 10, "l2", kernel="K1s")
        corpus.free()
        c.close()
