"""K1sc (vsr_scansc.h, Context.set_sparse_compact) against tests/sparse_model.py.  Integer-valued cases (values in -8..8: every
fp32 sum is exact in any order) are compared for EQUALITY of rows, ids, fp32 distances and counts; real-valued cases within the
README's 1e-4.  Every search names its kernel: K1sc with QW = 32 while the call's longest query has <= 64 non-zeros, 16 up to
128 (k <= 100), or the kernel a call falls back to."""
import numpy as np
import pytest

import sparse_model
from test_gpu_sparse_shared import EMPTY, HASH_MUL, _ids, _ints, _load, _vec   # the K1sm tests' data helpers

pytestmark = pytest.mark.gpu

METRICS = sparse_model.METRICS
NNZ = {32: 64, 16: 128}                                       # QW -> the longest query that still gets it
_reals = lambda rng, m: ((rng.normal(size=m) + 3) * 100).astype(np.float32)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    c.set_sparse_compact(True)
    yield c
    c.close()


def _check(ctx, corpus, model, queries, k, metric, filters=None, masks=None, kernel="K1sc", qw=None, close=False):
    indptr, indices, values = sparse_model.csr(queries)
    res = corpus.search_sparse(indptr, k, metric, filters, indices=indices, values=values)
    name = ctx.last_scan_kernel()
    assert f"({kernel}, sparse rows)" in name and (qw is None or f"QW={qw}>" in name), name
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
    rng = np.random.default_rng(1)                            # 300 rows of 0..40 entries, two of them empty, under a small RBAC
    n, dim = 300, 1000
    pool = rng.choice(dim, size=200, replace=False)
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
@pytest.mark.parametrize("qw,longest,dq", [(qw, ln, dq) for qw, ln in ((32, 64), (16, 65), (16, 128)) for dq in (2 - qw, -1, 0, 1)])
def test_queries_per_pass(ctx, small, qw, longest, dq, metric):
    """2, QW - 1, QW, QW + 1 queries, the first empty (cosine: NaN, id order), one at the longest length that keeps this QW;
    unfiltered and under two users' RANGES / BITMAP filters."""
    import vsrbac
    corpus, model, pool, masks = small
    rng = np.random.default_rng(qw + longest + dq)
    nq = qw + dq
    queries = [EMPTY, _vec(rng, pool, longest)] + [_vec(rng, pool, int(rng.integers(1, longest + 1))) for _ in range(nq - 2)]
    _check(ctx, corpus, model, queries, 10, metric, qw=qw)
    users = [1 + (i // 2) % 2 for i in range(nq)]
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        fs = {u: corpus.filter_for_user(u, mode) for u in (1, 2)}
        _check(ctx, corpus, model, queries, 10, metric, [fs[u] for u in users], [masks[u] for u in users], qw=qw)


@pytest.mark.parametrize("qw", [16, 32])
@pytest.mark.parametrize("kind", ["same", "disjoint", "collide", "staircase"])
def test_column_records_at_their_bounds(ctx, kind, qw):
    """same: every mask full.  disjoint: the most columns, one bit each, vals full.  collide: one home slot, the last (the chain
    wraps).  staircase: the j-th index is held by the queries q >= j mod QW -- masks of every popcount, every rank read.  dim = 10^9."""
    rng = np.random.default_rng(qw + len(kind))
    dim, nnz = 1_000_000_000, NNZ[qw]
    uslots, want = qw * 2 * nnz, qw * nnz // 4                # scansm_union_slots: QW x the call's per-query table
    if kind == "collide":
        cand = np.arange(0, 3_000_000, dtype=np.uint64)
        home = ((cand * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - int(np.log2(uslots)))
        own = cand[home == np.uint64(uslots - 1)][:want].astype(np.int64)
        assert own.size == want
    else:
        m = (qw * nnz if kind == "disjoint" else nnz) - 1
        own = np.append(rng.permutation(np.unique(rng.integers(0, dim - 1, 2 * m)))[:m], dim - 1)
    if kind == "disjoint":
        queries = [(np.sort(s).astype(np.int32), _ints(rng, nnz)) for s in np.split(rng.permutation(own), qw)]
    elif kind == "staircase":
        queries = [(ix, _ints(rng, ix.size)) for ix in (np.sort(own[np.arange(nnz) % qw <= q]).astype(np.int32) for q in range(qw))]
    else:
        queries = [_vec(rng, own, nnz) for _ in range(qw)]
    pool = np.concatenate([own, np.setdiff1d(rng.integers(0, dim, 200), own)])
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(200)]
    rows[0] = _vec(rng, own, 40)
    corpus, model = _load(ctx, rows, dim, *_ids(200))
    for metric in METRICS:
        _check(ctx, corpus, model, queries, 10, metric, qw=qw)
    corpus.free()


@pytest.mark.parametrize("qw", [16, 32])
def test_row_lengths_around_a_load_round(ctx, qw):
    """Row lengths around a round of 2 QW entries (odd: the pad entry must miss) against a query of the longest length; a step /
    all but one row of a tile denied."""
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
        _check(ctx, corpus, model, queries, 20, metric, qw=qw)
        for mask in (no_step, one_row):
            f = corpus.filter_from_bytemask(mask)
            _check(ctx, corpus, model, queries, 20, metric, [f] * 3, [mask] * 3, qw=qw)
            f.free()
    corpus.free()


@pytest.mark.parametrize("budget", [1, 0])
def test_candidate_buffers_overflow(ctx, budget):
    """6000 rows, each nearer than the last, in one workgroup (cap = 2048) and in the default launch: compactions run.  The third
    query's 40 non-zeros put the call out of K1sm's reach."""
    one = lambda v: (np.array([2], np.int32), np.array([v], np.float32))
    corpus, model = _load(ctx, [one(float(r + 1)) for r in range(6000)], 64)
    long = _vec(np.random.default_rng(4), np.arange(8, 64), 40)
    ctx.tune(block_budget=budget)
    for metric, queries in (("ip", [one(1.0), one(2.0), long]), ("l1", [one(30000.0), one(40000.0), long])):
        assert (np.diff(model.distances(metric, *queries[0])) < 0).all()
        _check(ctx, corpus, model, queries, 10, metric, qw=32)
    ctx.tune(block_budget=0)
    corpus.free()


@pytest.fixture(scope="module")
def real(ctx):
    rng = np.random.default_rng(5)
    pool = rng.choice(30522, size=300, replace=False)
    rows = [_vec(rng, pool, 128 if i == 0 else int(rng.integers(33, 129)), _reals) for i in range(700)]
    corpus, model = _load(ctx, rows, 30522)
    yield corpus, model, rows, pool
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
def test_real_values(ctx, real, metric):
    """Corpus rows of 33 .. 128 non-zeros as queries: within 1e-4 of the model, L2 and L1 self-distance within 1e-6 |q| of 0, no
    NaN.  Queries of <= 8 non-zeros, where K1sm runs QW = 32 too: the same rows and distance bits from both kernels."""
    corpus, model, rows, pool = real
    rng = np.random.default_rng(6)
    pick = np.append(0, rng.integers(1, len(rows), 19))
    res = _check(ctx, corpus, model, [rows[i] for i in pick], 5, metric, qw=16, close=True)
    assert not np.isnan(res.dist).any()
    if metric in ("l2", "l1"):
        for j, i in enumerate(pick):
            qn = float(np.sqrt((rows[i][1].astype(np.float64) ** 2).sum()))
            assert res.rows[j, 0] == i and 0 <= res.dist[j, 0] <= 1e-6 * qn, (metric, i, res.dist[j, 0], qn)
    short = [_vec(rng, pool, int(rng.integers(1, 9)), _reals) for _ in range(40)]
    a = _check(ctx, corpus, model, short, 5, metric, qw=32, close=True)
    ctx.set_sparse_compact(False), ctx.set_sparse_shared(True)
    try:
        b = _check(ctx, corpus, model, short, 5, metric, kernel="K1sm", qw=32, close=True)
    finally:
        ctx.set_sparse_shared(False), ctx.set_sparse_compact(True)
    np.testing.assert_array_equal(a.rows, b.rows)
    np.testing.assert_array_equal(a.dist.view(np.uint32), b.dist.view(np.uint32))


def test_routing(monkeypatch):
    """Default off; on by call or environment.  On: one query, or a 129-entry query in the call (no block even at QW = 16), run
    as with the switch off -- K1s, also with K1sm's switch on, whose block is never the smaller one.  Off again: K1sm's switch rules."""
    import vsrbac
    rng = np.random.default_rng(7)
    n, dim = 500, 1000
    pool = rng.choice(dim, size=150, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(n)]
    queries = [_vec(rng, pool, 8) for _ in range(4)] + [_vec(rng, pool, 70)]
    for env, call, kernel, qw in ((None, False, "K1s", None), (None, True, "K1sc", 16), ("1", False, "K1sc", 16)):
        if env:
            monkeypatch.setenv("VSR_SPARSE_COMPACT", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_SPARSE_COMPACT", raising=False)
        if call:
            c.set_sparse_compact(True)
        corpus, model = _load(c, rows, dim, *_ids(n))
        for metric in METRICS:
            _check(c, corpus, model, queries, 10, metric, kernel=kernel, qw=qw)
            _check(c, corpus, model, queries[:1], 10, metric, kernel="K1s")
            _check(c, corpus, model, queries + [_vec(rng, pool, 129)], 10, metric, kernel="K1s")
        if call:                                              # with K1sm's switch: K1sc first; off again, what that switch alone gives
            c.set_sparse_shared(True)
            for qs, on, off in ((queries + [_vec(rng, pool, 129)], "K1s", "K1s"), (queries[:4], "K1sc", "K1sm"), (queries, "K1sc", "K1s")):
                c.set_sparse_compact(True)
                _check(c, corpus, model, qs, 10, "l2", kernel=on)
                c.set_sparse_compact(False)
                _check(c, corpus, model, qs, 10, "l2", kernel=off, qw=32 if off == "K1sm" else None)
            c.set_sparse_shared(False)
            _check(c, corpus, model, queries[:4], 10, "l2", kernel="K1s")
        corpus.free()
        c.close()
