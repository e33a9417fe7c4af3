"""K2h: matrix-core screening over a halfvec corpus (csrc/vsr_mfmah.h), with the exact re-rank over half rows behind it.

The expected answer is always the existing oracle on `rows.astype(np.float32)` and the binary16-rounded query, as in
test_gpu_halfvec.py.  Unless a test says otherwise "exact" means row ids and fp32 distances bit for bit on integer data
0..31 (exact in binary16, sums exact in fp32 in any order).  Reported rows and distances never come from the screen: they
are K5r's (halfwave_row_sums, half form) or, for a flagged query, K1h's."""
import ctypes

import numpy as np
import pytest

import screening_model as sm
from helpers import assert_valid_topk

pytestmark = pytest.mark.gpu

TOL = 1e-4                                                    # test_gpu_halfvec.py's


def half_g(dim):
    """half_err_g of csrc/vsr_bounds.h (tests/test_halfvec_bounds_cpu.py checks the header itself)."""
    return (dim + 16) * 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _ids(n, rows_per_doc=7):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _rq(q):
    """The query `$1::halfvec` holds, widened."""
    with np.errstate(over="ignore"):
        return np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float32)


def _small_ints(rng, shape):
    return np.clip(np.rint(np.abs(rng.normal(0, 6, shape))), 0, 31).astype(np.float32)


def _ran(ctx, what):
    name = ctx.last_scan_kernel()
    assert what in name and "half" in name, name


def _expect_exact(oracle, res, qi, metric, x, q, k, doc=None, blk=None, mask=None):
    idx, dist = oracle.filtered_topk(metric, x, _rq(q), k, doc, blk, mask)
    m = res.counts[qi]
    assert m == idx.size, (qi, m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.dist[qi, :m].view(np.uint32), dist.astype(np.float32).view(np.uint32))


def _ref_all(metric, x, q):
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    if metric == "l2":
        return np.sqrt(((x64 - q64) ** 2).sum(1))
    if metric == "ip":
        return -(x64 @ q64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = (x64 @ q64) / np.sqrt((x64 ** 2).sum(1) * (q64 ** 2).sum())
    return 1.0 - np.clip(sim, -1, 1)


class _Dev:
    """Device buffers of one search_device call."""

    def __init__(self, q, k):
        import torch
        dev = torch.device("cuda", 0)
        nq = len(q)
        self.q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        self.blk = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.doc = torch.empty((nq, k), dtype=torch.int32, device=dev)
        self.row = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        self.cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()                              # the library runs on its own stream

    def qp(self):
        return ctypes.c_void_p(self.q.data_ptr())

    def args(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return p(self.blk), p(self.doc), p(self.row), p(self.dist), p(self.cnt)

    def result(self):
        from types import SimpleNamespace
        return SimpleNamespace(rows=self.row.cpu().numpy(), dist=self.dist.cpu().numpy(), counts=self.cnt.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 1. the kernel runs where K2 would, and only there
# ---------------------------------------------------------------------------------------------
def test_k2h_runs_for_shared_passes_only(ctx, oracle):
    rng = np.random.default_rng(1)
    n, dim, k = 5000, 128, 10
    x = _small_ints(rng, (n, dim))
    q = _small_ints(rng, (16, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    res = corpus.search(q, k, "l2")
    _ran(ctx, "K2h")
    for i in range(0, 16, 5):
        _expect_exact(oracle, res, i, "l2", x, q[i], k)
    corpus.search(q[:1], k, "l2")                             # one query per call
    _ran(ctx, "K1h")
    corpus.search(q, k, "l1")                                 # no L1 on the matrix cores
    _ran(ctx, "K1h")
    corpus.free()
    short = ctx.load_corpus_half(x[:, :32].astype(np.float16))
    short.search(q[:, :32], k, "l2")                          # rows shorter than one MFMA stage can use (dim < 61)
    _ran(ctx, "K1h")
    short.free()


# ---------------------------------------------------------------------------------------------
# 2. the f16 MFMA's A / B lane maps and the C / D layout, on asymmetric integer data
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [16, 32])
@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_lane_map_on_asymmetric_integers(ctx, oracle, metric, dim, nq):
    """Row r holds 1 + r % 29 at coordinate r % d and 3 at (7 r + 3) % d; query j is 1 + (i % 31) rotated by 5 j + 1.  A row's
    product with a query picks two of the query's coordinates: any permutation of k inside a fragment, or a row / column
    swap of the result tile, changes the top k."""
    n, k = 4096, 10
    r = np.arange(n)
    x = np.zeros((n, dim), np.float32)
    x[r, (7 * r + 3) % dim] = 3
    x[r, r % dim] = 1 + r % 29
    base = (1 + np.arange(dim) % 31).astype(np.float32)
    q = np.stack([np.roll(base, 5 * j + 1) for j in range(nq)])
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    res = corpus.search(q, k, metric)
    _ran(ctx, "K2h")
    for i in range(nq):
        _expect_exact(oracle, res, i, metric, x, q[i], k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 3. randomized shapes, exact
# ---------------------------------------------------------------------------------------------
DIMS = [64, 72, 100, 128, 136, 200, 256, 264, 512, 520, 768, 1032]     # d % 8 != 0, ragged last stages, NSTR 1 | 2 | 4 | 0


@pytest.mark.parametrize("seed", range(12))
def test_randomized_shapes_exact(ctx, oracle, seed):
    """Every d of the list four times over the seeds; n, nq, k, metric and filter kind at random.  A launch is K2h as soon as
    one pass carries two queries.  Whether one does is the library's own account (vsr_stats: scan_rows[1] counts the rows
    of shared-pass launches): two users with the same roles get the same partition, so distinct users may share a pass
    too.  Queries that carry the same filter object, or none, must share one."""
    import vsrbac
    rng = np.random.default_rng(7000 + seed)
    for j in range(4):
        dim = DIMS[(4 * seed + j) % len(DIMS)]
        n = int(rng.choice([60, 700, 5000, 30000]))
        nq = int(rng.choice([2, 7, 16, 17, 32, 33, 100]))
        k = int(rng.choice([1, 10, 100, 200]))
        metric = str(rng.choice(["l2", "ip"]))
        kind = str(rng.choice(["none", "ranges", "bitmap", "classes"]))
        if kind == "classes":
            nq = max(nq, 32)                                  # the planner decomposes role filters from 32 queries on
        x = _small_ints(rng, (n, dim))
        blk, doc = _ids(n, int(rng.choice([1, 7, 50])))
        corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
        q = _small_ints(rng, (nq, dim))
        masks, filters, shared = [None] * nq, None, nq >= 2
        if kind == "bitmap":
            base = [(rng.random(n) < p).astype(np.uint8) for p in (0.03, 0.5)]
            fs = [corpus.filter_from_bytemask(m) for m in base]
            pick = rng.integers(0, 2, nq)
            filters, masks = [fs[p] for p in pick], [base[p] for p in pick]
            shared = max(np.bincount(pick, minlength=2)) >= 2
        elif kind in ("ranges", "classes"):
            ndocs, nroles, nusers = int(doc.max()), 5, 9
            perms = sorted({(int(r), int(d)) for r in range(1, nroles + 1)
                            for d in rng.choice(np.arange(1, ndocs + 1), size=max(1, ndocs // 3), replace=False)})
            ur = sorted({(u, int(r)) for u in range(1, nusers + 1)
                         for r in rng.choice(np.arange(1, nroles + 1), size=int(rng.integers(1, 3)), replace=False)})
            corpus.load_rbac(ur, perms)
            users = rng.integers(1, nusers + 1, nq)
            mode = vsrbac.RANGES if kind == "ranges" or rng.random() < 0.5 else vsrbac.BITMAP
            per_user = {int(u): corpus.filter_for_user(int(u), mode) for u in set(users.tolist())}
            filters = [per_user[int(u)] for u in users]
            masks = [oracle.user_row_mask(int(u), ur, perms, doc) for u in users]
            shared = max(np.bincount(users)) >= 2
        ctx.stats_reset()
        res = corpus.search(q, k, metric, filters)
        if any(m is None or m.any() for m in masks):          # (every filter empty: nothing is launched)
            st = ctx.stats()
            lib_shared = st["scan_rows"][1] > 0
            assert lib_shared or not shared, (kind, nq, st["scan_rows"])
            _ran(ctx, "K2h" if lib_shared else "K1h")
        for i in range(0, nq, max(1, nq // 5)):
            _expect_exact(oracle, res, i, metric, x, q[i], k, doc, blk, masks[i])
        corpus.free()


# ---------------------------------------------------------------------------------------------
# 4. real-valued data: the screen proves nearly every query
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("dim", [128, 768])
def test_real_valued_under_a_mask(ctx, oracle, metric, dim):
    """Gaussian rows: the CPU model of the screen under the K2-tier bound flags 0 of 33 such queries, so at most a tenth may
    be re-run -- a kernel that flags everything would pass the value checks by falling back to K1h."""
    rng = np.random.default_rng(dim)
    n, k, nq = 1500, 20, 33
    h = rng.normal(size=(n, dim)).astype(np.float16)
    x = h.astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    q = (x[rng.integers(10, n, nq)] + 0.01 * rng.normal(size=(nq, dim))).astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    f = corpus.filter_from_bytemask(mask)
    b = _Dev(q, k)
    corpus.search_device(b.qp(), nq, k, metric, [f] * nq, *b.args())
    ctx.synchronize()
    _ran(ctx, "K2h")
    flagged = int((b.cnt.cpu().numpy() < 0).sum())
    print(f"{metric} d = {dim}: {flagged} of {nq} queries flagged")
    assert flagged / nq <= 0.1, flagged
    res = corpus.search(q, k, metric, f)
    for i in range(nq):
        qi = _rq(q[i])
        assert res.counts[i] == k
        assert_valid_topk(res.rows[i, :k], res.dist[i, :k], _ref_all(metric, x, qi), k, TOL, candidates=np.flatnonzero(mask))
        _, odist = oracle.filtered_topk(metric, x, qi, k, mask=mask)
        np.testing.assert_allclose(res.dist[i, :k], odist, rtol=TOL, atol=TOL)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 5. binary16 subnormals are values like any other
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rows", "queries"])
def test_subnormal_operands(ctx, oracle, which):
    """Elements m 2^-24, m = 0..1023 (every binary16 subnormal, and zero) against integers 0..31: every inner product is
    below 2^24 units of 2^-24, so it is exact in fp32 in any order.  A matrix core that flushed subnormal inputs would
    rank by zeros."""
    rng = np.random.default_rng(5)
    n, dim, nq, k = 5000, 128, 16, 10
    sub = (rng.integers(0, 1024, (n + nq, dim)) * 2.0 ** -24).astype(np.float32)
    ints = rng.integers(0, 32, (n + nq, dim)).astype(np.float32)
    x, q = (sub[:n], ints[n:]) if which == "rows" else (ints[:n], sub[n:])
    h = x.astype(np.float16)
    assert (h.astype(np.float32) == x).all() and (_rq(q) == q).all()
    corpus = ctx.load_corpus_half(h)
    res = corpus.search(q, k, "ip")
    _ran(ctx, "K2h")
    for i in range(nq):
        _expect_exact(oracle, res, i, "ip", x, q[i], k)
    b = _Dev(q, k)
    corpus.search_device(b.qp(), nq, k, "ip", None, *b.args())
    ctx.synchronize()
    got = b.result()
    proven = np.flatnonzero(got.counts >= 0)                  # what the screen published without a re-run is exact too
    print(f"subnormal {which}: {nq - proven.size} of {nq} queries flagged")
    for i in proven:
        _expect_exact(oracle, got, i, "ip", x, q[i], k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 6. at the bound: the screen cannot prove these, and says so
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(128, 20000), (768, 8000)])
def test_offset_rows_are_flagged_and_exact(ctx, oracle, dim, n):
    """Rows 1024 + r (r = 0..15), queries a row +- 1: |x|^2 ~ 2^20 d cancels in the screen's expansion of L2, so the gap
    between the kept set and the rest is far inside the bound."""
    rng = np.random.default_rng(dim)
    nq, k = 40, 10
    x = sm.offset_rows(rng, n, dim, 1024)
    q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    h = x.astype(np.float16)
    assert (h.astype(np.float32) == x).all() and (_rq(q) == q).all()          # 1023 .. 1040 are binary16 values
    model = [sm.screen("k2", "l2", x, q[i], k, half_g(dim))[1] for i in range(nq)]
    assert all(model), f"the model flags only {sum(model)} of {nq}"
    blk, doc = _ids(n, 10)
    corpus = ctx.load_corpus_half(h, blk, doc)
    b = _Dev(q, k)
    corpus.search_device(b.qp(), nq, k, "l2", None, *b.args())
    ctx.synchronize()
    _ran(ctx, "K2h")
    _, flags = ctx.screening_check(nq)
    cnt = b.cnt.cpu().numpy()
    assert (cnt < 0).all() and np.count_nonzero(flags) == nq, int((cnt >= 0).sum())
    res = corpus.search(q, k, "l2")
    n_rerun = corpus.search_device_exact(b.qp(), nq, k, "l2", None, *b.args())
    assert n_rerun == nq
    _ran(ctx, "K1h")                                          # the last rung for a half corpus
    got = b.result()
    for i in range(nq):
        _expect_exact(oracle, res, i, "l2", x, q[i], k, doc, blk)
        _expect_exact(oracle, got, i, "l2", x, q[i], k, doc, blk)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 7. extremes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_largest_halves_among_small_integers(ctx, oracle, metric):
    """+-65504 in a few coordinates: products up to 2^32 and |x|^2 ~ 2^34 are fine in fp32; the screen flags what the huge
    norms leave it unable to prove and the answer stays exact.  (One huge coordinate in each of 40 rows and integer data: 65504 q <= 2^21 is a
    multiple of 32, so the inner products that reach the top k are exact sums, and no such row reaches the top k of L2.)"""
    rng = np.random.default_rng(65504)
    n, dim, nq, k = 5000, 128, 16, 10
    x = _small_ints(rng, (n, dim))
    big = rng.choice(n, 40, replace=False)
    x[big, rng.integers(0, dim, 40)] = rng.choice([65504.0, -65504.0], 40)
    q = _small_ints(rng, (nq, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    res = corpus.search(q, k, metric)
    _ran(ctx, "K")                                            # K2h, or K1h when every query was re-run
    for i in range(nq):
        _expect_exact(oracle, res, i, metric, x, q[i], k)
    corpus.free()


def test_nonfinite_rows_stay_on_k1h(ctx, oracle):
    """test_gpu_halfvec.py::test_nonfinite_rows_sort_last's expectations at d = 64, several queries per pass."""
    rng = np.random.default_rng(9)
    n, dim = 700, 64
    x = _small_ints(rng, (n, dim))
    h = x.astype(np.float16)
    h[5, 0] = np.inf
    h[6, 1] = np.nan
    x = h.astype(np.float32)
    q = _small_ints(rng, (16, dim))
    corpus = ctx.load_corpus_half(h)
    res = corpus.search(q, n, "l2")
    _ran(ctx, "K1h")
    for i in range(0, 16, 5):
        idx, dist = oracle.filtered_topk("l2", x, q[i], n)
        np.testing.assert_array_equal(res.rows[i], idx)
        np.testing.assert_array_equal(res.dist[i], dist.astype(np.float32))                 # ..., +Inf, NaN
        assert res.rows[i, n - 2] == 5 and np.isposinf(res.dist[i, n - 2]) and res.rows[i, n - 1] == 6 and np.isnan(res.dist[i, n - 1])
    corpus.free()


def test_infinite_device_query_is_flagged(ctx, oracle):
    rng = np.random.default_rng(10)
    n, dim, nq, k = 5000, 128, 16, 10
    x = _small_ints(rng, (n, dim))
    q = _small_ints(rng, (nq, dim))
    q[3, 17] = np.inf
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    b = _Dev(q, k)
    corpus.search_device(b.qp(), nq, k, "l2", None, *b.args())
    ctx.synchronize()
    _ran(ctx, "K2h")
    cnt = b.cnt.cpu().numpy()
    assert cnt[3] < 0, cnt
    n_rerun = corpus.search_device_exact(b.qp(), nq, k, "l2", None, *b.args())
    assert n_rerun >= 1
    got = b.result()
    want = corpus.search(q[3:4], k, "l2")                     # one query per call: K1h
    _ran(ctx, "K1h")
    assert got.counts[3] == want.counts[0] == k and np.isposinf(got.dist[3]).all()         # every distance is +Inf
    np.testing.assert_array_equal(got.rows[3], want.rows[0])
    for i in (0, 4, 15):
        _expect_exact(oracle, got, i, "l2", x, q[i], k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 8. the switches keep a half corpus on K1h, with the same answers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["VSR_NO_HALF_MFMA", "VSR_NO_SCREENING", "set_screening"])
def test_switches_fall_back_to_k1h(ctx, monkeypatch, switch):
    import vsrbac
    rng = np.random.default_rng(8)
    n, dim, nq, k = 5000, 128, 33, 10
    x = _small_ints(rng, (n, dim))
    q = _small_ints(rng, (nq, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    want = corpus.search(q, k, "l2")
    _ran(ctx, "K2h")
    corpus.free()
    if switch == "set_screening":
        other = vsrbac.Context(0)
        other.set_screening(False)
    else:
        monkeypatch.setenv(switch, "1")
        other = vsrbac.Context(0)
        monkeypatch.delenv(switch)
    try:
        c2 = other.load_corpus_half(x.astype(np.float16))
        got = c2.search(q, k, "l2")
        _ran(other, "K1h")
        for name in ("rows", "block_ids", "doc_ids", "counts"):
            np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
        np.testing.assert_array_equal(got.dist.view(np.uint32), want.dist.view(np.uint32))
        c2.free()
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------
# 9. a seeded run
# ---------------------------------------------------------------------------------------------
def test_seeded_run_is_exact(ctx, oracle):
    """512 unfiltered queries over 66000 x 128: 32 passes x 66000 rows cross the seeding threshold (seed_min_rows = 2,000,000
    pass-rows) and kp = 200 >= SEED_LIST, so the sample launch and the seeded thresholds run.  No statistic of vsr_stats
    counts the sample launch (its time goes to a debug-only counter), so the test asserts what makes it run -- the
    pass-rows of shared passes -- and that results stay exact under seeded thresholds."""
    rng = np.random.default_rng(9)
    n, dim, nq, k = 66000, 128, 512, 100
    x = _small_ints(rng, (n, dim))
    q = _small_ints(rng, (nq, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    ctx.stats_reset()
    res = corpus.search(q, k, "l2")
    _ran(ctx, "K2h")
    st = ctx.stats()
    assert st["scan_rows"][1] >= 2_000_000, st["scan_rows"]
    for i in range(0, nq, 37):
        _expect_exact(oracle, res, i, "l2", x, q[i], k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 10. two sessions in flight over one half corpus
# ---------------------------------------------------------------------------------------------
def test_two_sessions_in_flight(ctx, oracle):
    import vsrbac
    rng = np.random.default_rng(10)
    n, dim, nq, k = 30000, 128, 48, 10
    x = _small_ints(rng, (n, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    other = vsrbac.Context(0)
    try:
        batches = []
        for r in range(4):
            q = _small_ints(rng, (nq, dim))
            batches.append((q, _Dev(q, k)))
        for r, (q, b) in enumerate(batches):
            corpus.search_device(b.qp(), nq, k, "ip" if r >= 2 else "l2", None, *b.args(), None, session=other if r % 2 else None)
        ctx.synchronize()
        other.synchronize()
        _ran(ctx, "K2h")
        _ran(other, "K2h")
        for r, (q, b) in enumerate(batches):
            got = b.result()
            proven = np.flatnonzero(got.counts >= 0)          # (a tie between the k-th and the kp-th distance flags its query)
            assert proven.size >= 0.9 * nq, got.counts
            for i in proven[::7]:
                _expect_exact(oracle, got, i, "ip" if r >= 2 else "l2", x, q[i], k)
    finally:
        corpus.free()
        other.close()
