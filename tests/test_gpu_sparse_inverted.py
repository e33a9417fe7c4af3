"""K1si (vsr_scansi.h, Corpus.build_sparse_inverted + Context.set_sparse_inverted) against tests/sparse_model.py.  Integer-valued
cases (values in -8..8: every sum is exact in any order and any precision) are compared for EQUALITY of rows, ids, fp32 distances
and counts; real-valued cases within the README's 1e-4.  Every search names its kernel."""
import numpy as np
import pytest

import sparse_model
from test_gpu_sparse_shared import EMPTY, _ids, _ints, _load, _vec   # the K1sm tests' data helpers

pytestmark = pytest.mark.gpu

METRICS = sparse_model.METRICS
SI_RB, SI_WAVES, SI_MAX_TERMS = 512, 8, 256                   # vsr_scansi_sizing.h
_reals = lambda rng, m: ((rng.normal(size=m) + 3) * 100).astype(np.float32)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    c.set_sparse_inverted(True)
    yield c
    c.close()


def _load_inv(ctx, rows, dim, blk=None, doc=None):
    corpus, model = _load(ctx, rows, dim, blk, doc)
    corpus.build_sparse_inverted()
    return corpus, model


def _check(ctx, corpus, model, queries, k, metric, filters=None, masks=None, kernel="K1si", close=False):
    indptr, indices, values = sparse_model.csr(queries)
    res = corpus.search_sparse(indptr, k, metric, filters, indices=indices, values=values)
    name = ctx.last_scan_kernel()
    assert f"({kernel}, sparse rows)" in name, name
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
    rng = np.random.default_rng(1)                            # two row blocks and a partial third, two empty rows, a small RBAC
    n, dim = 2 * SI_RB + 37, 1000
    pool = rng.choice(dim, size=200, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(n)]
    rows[5] = rows[SI_RB + 77] = EMPTY
    blk, doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 31, n).astype(np.int32)
    corpus, model = _load_inv(ctx, rows, dim, blk, doc)
    perms = sorted({(r, int(d)) for r in (1, 2, 3) for d in rng.choice(np.arange(1, 31), size=12, replace=False)})
    ur = [(1, 1), (1, 2), (2, 2), (2, 3)]
    corpus.load_rbac(ur, perms)
    masks = {u: sparse_model.user_row_mask(u, ur, perms, doc) for u in (1, 2)}
    yield corpus, model, pool, masks
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [1, SI_WAVES - 1, SI_WAVES, SI_WAVES + 1, 17])
def test_rows_per_block_and_queries_per_round(ctx, small, nq, metric):
    """1 .. 17 queries (rounds of SI_WAVES, passes of 16), the first empty (cosine: NaN, id order); unfiltered and under two
    users' RANGES / BITMAP filters, whose tiles start anywhere in a row block."""
    import vsrbac
    corpus, model, pool, masks = small
    rng = np.random.default_rng(nq)
    queries = [EMPTY] + [_vec(rng, pool, int(rng.integers(1, 41))) for _ in range(nq - 1)]
    _check(ctx, corpus, model, queries, 10, metric)
    users = [1 + (i // 2) % 2 for i in range(nq)]
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        fs = {u: corpus.filter_for_user(u, mode) for u in (1, 2)}
        _check(ctx, corpus, model, queries, 10, metric, [fs[u] for u in users], [masks[u] for u in users])


def test_segment_edges(ctx):
    """dim = 10^9.  Index 7 is held by every row of block 1 and by no other row, index 11 by the last row of the partial last
    block only, index dim - 1 by a few rows; a query index no row holds; a query of SI_MAX_TERMS non-zeros, and one of one more,
    which runs on K1s."""
    rng = np.random.default_rng(2)
    dim, n = 1_000_000_000, 2 * SI_RB + 37
    own = np.unique(rng.integers(100, dim - 1, 700))
    rows = [_vec(rng, own, int(rng.integers(0, 41))) for _ in range(n)]
    with_ix = lambda r, ix: (np.sort(np.append(r[0], ix)).astype(np.int32), _ints(rng, r[0].size + 1))
    for r in range(SI_RB, 2 * SI_RB):
        rows[r] = with_ix(rows[r], 7)
    rows[n - 1] = with_ix(rows[n - 1], 11)
    for r in (0, SI_RB - 1, n - 2):
        rows[r] = with_ix(rows[r], dim - 1)
    corpus, model = _load_inv(ctx, rows, dim, *_ids(n))
    edge = (np.array([7, 11, 13, dim - 1], np.int32), _ints(rng, 4))   # 13: no row holds it
    longest = _vec(rng, np.concatenate([[7, 11, dim - 1], own[:SI_MAX_TERMS + 40]]), SI_MAX_TERMS)
    past = _vec(rng, own, SI_MAX_TERMS + 1)
    for metric in METRICS:
        _check(ctx, corpus, model, [edge, longest], 10, metric)
        _check(ctx, corpus, model, [edge, past], 10, metric, kernel="K1s")
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
def test_split_blocks(ctx, small, metric):
    """Eight workgroups over the 17 tiles of a one-query pass: several share a row block and narrow their segments.  Bytemasks
    that admit one row of a block, deny a whole block, admit only the first and the last row of the corpus."""
    corpus, model, pool, masks = small
    rng = np.random.default_rng(3)
    n = model.n
    internal = np.empty(n, np.int64)
    internal[model.by_id] = np.arange(n)                      # caller row -> internal row (masks are in caller order)
    one_row = (internal < SI_RB) | (internal >= 2 * SI_RB) | (internal == SI_RB + 300)
    no_block = (internal < SI_RB) | (internal >= 2 * SI_RB)
    ends = (internal == 0) | (internal == n - 1)
    query = [_vec(rng, pool, 30)]
    ctx.tune(block_budget=8, min_rows_per_block=64)
    try:
        _check(ctx, corpus, model, query, 20, metric)
        for mask in (one_row, no_block, ends):
            f = corpus.filter_from_bytemask(mask)
            _check(ctx, corpus, model, query, 20, metric, [f], [mask])
            f.free()
    finally:
        ctx.tune(block_budget=0, min_rows_per_block=256)


@pytest.mark.parametrize("budget", [1, 0])
def test_candidate_buffers_overflow(ctx, budget):
    """6000 one-entry rows, each nearer than the last, in one workgroup (cap = 2048) and in the default launch: compactions run."""
    one = lambda v: (np.array([2], np.int32), np.array([v], np.float32))
    corpus, model = _load_inv(ctx, [one(float(r + 1)) for r in range(6000)], 64)
    ctx.tune(block_budget=budget)
    try:
        for metric, queries in (("ip", [one(1.0), one(2.0)]), ("l1", [one(30000.0), one(40000.0)])):
            assert (np.diff(model.distances(metric, *queries[0])) < 0).all()
            _check(ctx, corpus, model, queries, 10, metric)
    finally:
        ctx.tune(block_budget=0)
    corpus.free()


@pytest.mark.parametrize("metric", METRICS)
def test_real_values(ctx, metric):
    """Corpus rows of 33 .. 128 non-zeros as queries: within 1e-4 of the model, L2 and L1 self-distance within 1e-6 |q| of 0, no
    NaN, and the same distance bits from two consecutive calls."""
    rng = np.random.default_rng(5)
    pool = rng.choice(30522, size=300, replace=False)
    rows = [_vec(rng, pool, 128 if i == 0 else int(rng.integers(33, 129)), _reals) for i in range(700)]
    corpus, model = _load_inv(ctx, rows, 30522)
    pick = np.append(0, rng.integers(1, len(rows), 19))
    res = _check(ctx, corpus, model, [rows[i] for i in pick], 5, metric, close=True)
    again = _check(ctx, corpus, model, [rows[i] for i in pick], 5, metric, close=True)
    assert not np.isnan(res.dist).any()
    np.testing.assert_array_equal(res.rows, again.rows)
    np.testing.assert_array_equal(res.dist.view(np.uint32), again.dist.view(np.uint32))
    if metric in ("l2", "l1"):
        for j, i in enumerate(pick):
            qn = float(np.sqrt((rows[i][1].astype(np.float64) ** 2).sum()))
            assert res.rows[j, 0] == i and 0 <= res.dist[j, 0] <= 1e-6 * qn, (metric, i, res.dist[j, 0], qn)
    corpus.free()


def test_routing_and_build(monkeypatch):
    """Default off; the switch without the image: K1s; the image and the switch, by call or by environment: K1si, ahead of K1sc
    and K1sm.  A second build is OK and builds nothing; device_bytes grows by 8 per stored entry, 12 per (row block, distinct index)
    and per row block, 4, 16 per row; a dense corpus is refused."""
    import vsrbac
    rng = np.random.default_rng(7)
    n, dim = SI_RB + 100, 1000
    pool = rng.choice(dim, size=150, replace=False)
    rows = [_vec(rng, pool, int(rng.integers(0, 41))) for _ in range(n)]
    queries = [_vec(rng, pool, 8) for _ in range(4)]
    stored = sum((r[0].size + 1) // 2 * 2 for r in rows)      # every row an even number of entries
    block_terms = sum(np.unique(np.concatenate([r[0] for r in rows[b:b + SI_RB]])).size for b in range(0, n, SI_RB))
    for env, call in ((None, False), (None, True), ("1", False)):
        if env:
            monkeypatch.setenv("VSR_SPARSE_INVERTED", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_SPARSE_INVERTED", raising=False)
        if call:
            c.set_sparse_inverted(True)
        on = "K1si" if env or call else "K1s"
        corpus, model = _load(c, rows, dim, *_ids(n))
        _check(c, corpus, model, queries, 10, "l2", kernel="K1s")             # no image yet
        before = corpus.device_bytes()
        corpus.build_sparse_inverted()
        grown = corpus.device_bytes()
        assert grown - before == 8 * stored + 12 * block_terms + 12 * 2 + 4 + 16 * n
        corpus.build_sparse_inverted()
        assert corpus.device_bytes() == grown
        for metric in METRICS:
            _check(c, corpus, model, queries, 10, metric, kernel=on)
            _check(c, corpus, model, queries[:1], 10, metric, kernel=on)
        if call:
            c.set_sparse_shared(True), c.set_sparse_compact(True)
            _check(c, corpus, model, queries, 10, "l2")
            c.set_sparse_inverted(False)
            _check(c, corpus, model, queries, 10, "l2", kernel="K1sc")
        corpus.free()
        c.close()
    c = vsrbac.Context(0)
    dense = c.load_corpus(rng.normal(size=(10, 8)).astype(np.float32))
    with pytest.raises(vsrbac.VsrError, match="not a sparse corpus") as e:
        dense.build_sparse_inverted()
    assert e.value.status == 6                                # VSR_ERR_UNSUPPORTED
    dense.free()
    c.close()
