"""pgvector's IVFFlat iterative index scan on the GPU (vsr_ivf_search_iterative) against the numpy model of the stream
(tests/ivf_iterative_model.py, on top of the index oracle).  The parity fixture holds integer rows, so ids, distances, counts
and the lists scanned are compared bit for bit, every query of every call."""
import numpy as np
import pytest

from ivf_iterative_model import ParityFixture, iterative_search, recall_at, tap_corpus, tap_queries
from oracle.oracle import IvfIndex as OracleIvf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class Loaded:
    def __init__(self, ctx, fx):
        import vsrbac
        self.fx = fx
        self.corpus = ctx.load_corpus(fx.x, fx.blk, fx.doc)
        self.corpus.load_rbac(fx.user_roles, fx.perms)
        self.gpu = self.corpus.load_ivf(fx.centers, fx.oivf.assign)
        self.filters = {(None, None): None}
        for u in (1, 2, 3):
            for mode in (vsrbac.BITMAP, vsrbac.RANGES):
                self.filters[(u, mode)] = [self.corpus.filter_for_user(u, mode)] * len(fx.q)

    def free(self):
        self.gpu.free()
        self.corpus.free()


@pytest.fixture(scope="module")
def main(ctx, oracle):
    ld = Loaded(ctx, ParityFixture(oracle))
    yield ld
    ld.free()


def check_against_model(res, scanned, want, k):
    """want[i] = (rows, float64 distances, lists scanned) of the model; every query is compared."""
    assert len(want) == len(res.counts)
    for i, (rows, dist, lists) in enumerate(want):
        m = int(res.counts[i])
        assert m == len(rows), (i, m, len(rows))
        np.testing.assert_array_equal(res.rows[i, :m], rows, err_msg=f"query {i}")
        np.testing.assert_array_equal(res.dist[i, :m], dist.astype(np.float32), err_msg=f"query {i}")
        assert int(scanned[i]) == lists, (i, int(scanned[i]), lists)
        assert (res.rows[i, m:] == -1).all() and (res.block_ids[i, m:] == -1).all() and (res.doc_ids[i, m:] == -1).all()
        assert np.isposinf(res.dist[i, m:]).all()
    assert res.rows.shape[1] == max(k, 1)


@pytest.mark.parametrize("probes", [1, 3, 5])
@pytest.mark.parametrize("user", [None, 1, 2, 3])
def test_stream_matches_the_model(main, user, probes):
    import vsrbac
    fx = main.fx
    nq = len(fx.q)
    for max_probes in (1, 7, 20, 64, 32768):
        for k in (1, 10, 100, 2048):
            want = [fx.model(user, i, k, probes, max_probes) for i in range(nq)]
            if user == 1 and probes == 1 and k == 10 and max_probes == 32768:       # not vacuous: see the CPU test
                assert all(w[2] > 1 and (np.diff(w[1]) < 0).any() for w in want)
            if user == 1 and probes == 1 and k == 100 and max_probes == 64:
                assert all(42 <= w[2] <= 51 for w in want)
            if user == 1 and k == 100 and max_probes == 20:
                assert all(w[2] == 20 and len(w[0]) < 100 for w in want)
            if user == 3:
                assert all(len(w[0]) == 0 and w[2] == min(max(max_probes, probes), 64) for w in want)
            if user is None and probes >= 3 and k <= 100:
                assert all(w[2] == probes for w in want)                            # the kernel's early exit
            for mode in ((None,) if user is None else (vsrbac.BITMAP, vsrbac.RANGES)):
                res, scanned = main.gpu.search_iterative(fx.q, k, probes, "l2", main.filters[(user, mode)], "relaxed_order", max_probes)
                check_against_model(res, scanned, want, k)
                m = res.counts
                for i in range(nq):
                    np.testing.assert_array_equal(res.block_ids[i, :m[i]], fx.blk[want[i][0]])
                    np.testing.assert_array_equal(res.doc_ids[i, :m[i]], fx.doc[want[i][0]])


def test_short_last_batch(main):
    """probes = 5, max_probes = 64: twelve batches of 5 lists and one of 4; user 3 sees nothing and walks them all."""
    fx = main.fx
    import vsrbac
    res, scanned = main.gpu.search_iterative(fx.q, 10, 5, "l2", main.filters[(3, vsrbac.BITMAP)], "relaxed_order", 64)
    assert (scanned == 64).all() and (res.counts == 0).all()


@pytest.mark.parametrize("dim", [10, 128])
def test_other_dimensions(ctx, oracle, dim):
    """dim = 10 is no multiple of 4 (row padding); dim = 128 takes one full step of the half-wave loop."""
    import vsrbac
    fx = ParityFixture(oracle, n=3000, dim=dim, seed=142 + dim)
    ld = Loaded(ctx, fx)
    try:
        for user, probes, max_probes, k in ((1, 1, 64, 10), (1, 3, 20, 100), (2, 1, 7, 100), (None, 1, 64, 2048)):
            want = [fx.model(user, i, k, probes, max_probes) for i in range(len(fx.q))]
            assert any(w[2] > probes for w in want)
            res, scanned = ld.gpu.search_iterative(fx.q, k, probes, "l2", ld.filters[(user, None if user is None else vsrbac.BITMAP)],
                                                   "relaxed_order", max_probes)
            check_against_model(res, scanned, want, k)
    finally:
        ld.free()


def test_inner_product_opclass(main, oracle):
    """vector_ip_ops over the main fixture's rows: centres and rows by negative inner product (integers: exact).  Without
    the four far centres, which would own every row under this operator."""
    import vsrbac
    fx = main.fx
    centers = np.ascontiguousarray(fx.centers[:60])
    oivf = OracleIvf.from_centers(oracle, "ip", fx.x, centers)
    gpu = main.corpus.load_ivf(centers, oivf.assign)
    try:
        for user, probes, max_probes, k in ((1, 1, 60, 10), (1, 3, 20, 100)):
            want = [iterative_search(oivf, fx.q[i], k, probes, max_probes, fx.doc, fx.blk, fx.masks[user]) for i in range(len(fx.q))]
            assert any(w[2] > probes for w in want)
            res, scanned = gpu.search_iterative(fx.q, k, probes, "ip", main.filters[(user, vsrbac.RANGES)], "relaxed_order", max_probes)
            check_against_model(res, scanned, want, k)
    finally:
        gpu.free()


def test_cosine_opclass_on_unit_rows(ctx, oracle):
    """vector_cosine_ops (the recipe of test_ivf_cosine_opclass_on_unit_rows, smaller): a centre-distance near-tie may order
    two lists the other way, so queries are compared where the lists scanned agree, and nearly all must."""
    rng = np.random.default_rng(171)
    n, dim = 6000, 96
    x = rng.normal(size=(n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    oivf = OracleIvf(oracle, "cosine", x, lists=30, seed=2)
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_ivf(oivf.centers, oivf.assign)
    mask = (np.arange(n) % 50 == 0).astype(np.uint8)
    filt = [corpus.filter_from_bytemask(mask)] * 12
    q = x[rng.integers(0, n, 12)] + 0.05 * rng.normal(size=(12, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = q.astype(np.float32)
    res, scanned = gpu.search_iterative(q, 20, 2, "cosine", filt, "relaxed_order", 30)
    lists_gpu = gpu.probe(q, 30, "cosine")
    agree = 0
    for i in range(12):
        rows, dist, lists = iterative_search(oivf, q[i], 20, 2, 30, mask=mask)
        assert lists > 2
        if lists_gpu[i, :lists].tolist() != oivf.probe(q[i], 30)[:lists].tolist():
            continue
        agree += 1
        assert res.counts[i] == len(rows) and scanned[i] == lists
        assert len(set(res.rows[i, :len(rows)].tolist()) & set(rows.tolist())) >= len(rows) - 1
        np.testing.assert_allclose(res.dist[i, :len(rows)], dist, rtol=1e-4, atol=1e-4)
    assert agree >= 11
    gpu.free()
    corpus.free()


def test_mode_off_and_no_further_lists_are_the_plain_search(main):
    import vsrbac
    fx = main.fx
    filt = main.filters[(1, vsrbac.BITMAP)]
    for probes, mode, max_probes in ((3, "off", 64), (3, "off", 1), (5, "relaxed_order", 5), (5, "relaxed_order", 2), (64, "relaxed_order", 32768)):
        plain = main.gpu.search(fx.q, 100, probes, "l2", filt)
        res, scanned = main.gpu.search_iterative(fx.q, 100, probes, "l2", filt, mode, max_probes)
        for a, b in zip(plain, res):
            np.testing.assert_array_equal(a, b)
        assert (scanned == probes).all()


def test_prefix_property(main):
    import vsrbac
    fx = main.fx
    filt = main.filters[(1, vsrbac.RANGES)]
    big, s_big = main.gpu.search_iterative(fx.q, 100, 3, "l2", filt, "relaxed_order", 64)
    for k in (1, 10, 37):
        res, s = main.gpu.search_iterative(fx.q, k, 3, "l2", filt, "relaxed_order", 64)
        np.testing.assert_array_equal(res.rows, big.rows[:, :k])
        np.testing.assert_array_equal(res.dist, big.dist[:, :k])
        assert (res.counts == np.minimum(big.counts, k)).all() and (s <= s_big).all()


def test_device_form_equals_host_form(main):
    import torch
    import vsrbac
    fx = main.fx
    nq, k, probes, max_probes = len(fx.q), 10, 1, 64
    filt = main.filters[(1, vsrbac.BITMAP)]
    host, h_scanned = main.gpu.search_iterative(fx.q, k, probes, "l2", filt, "relaxed_order", max_probes)
    dq = torch.from_numpy(fx.q).cuda()
    d_blk = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_doc = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    d_dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    d_pr = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    main.gpu.search_iterative_device(dq.data_ptr(), nq, k, probes, "l2", filt, "relaxed_order", max_probes, d_blk.data_ptr(),
                                     d_doc.data_ptr(), d_row.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), d_pr.data_ptr())
    np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)
    np.testing.assert_array_equal(d_row.cpu().numpy(), host.rows)
    np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
    np.testing.assert_array_equal(d_doc.cpu().numpy(), host.doc_ids)
    np.testing.assert_array_equal(d_dist.cpu().numpy(), host.dist)
    np.testing.assert_array_equal(d_pr.cpu().numpy(), h_scanned)
    assert (h_scanned > 1).all()
    # doc / row / probes outputs are optional
    main.gpu.search_iterative_device(dq.data_ptr(), nq, k, probes, "l2", filt, "relaxed_order", max_probes, d_blk.data_ptr(),
                                     None, None, d_dist.data_ptr(), d_cnt.data_ptr(), None)
    np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
    np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)


def test_arguments_and_errors(main):
    import vsrbac
    from vsrbac import _ffi
    fx = main.fx
    res, scanned = main.gpu.search_iterative(np.zeros((0, fx.dim), np.float32), 10, 3)
    assert res.counts.size == 0 and scanned.size == 0

    def status(**kw):
        a = dict(queries=fx.q, k=10, probes=3, metric="l2", filters=None, mode=1, max_probes=64)
        a.update(kw)
        with pytest.raises(vsrbac.VsrError) as e:
            main.gpu.search_iterative(**a)
        return e.value.status, str(e.value)

    assert status(mode=2)[0] == _ffi.ERR_INVALID                       # IVFFlat has no strict order
    assert status(mode=-1)[0] == _ffi.ERR_INVALID
    assert status(max_probes=0)[0] == _ffi.ERR_INVALID
    assert status(max_probes=32769)[0] == _ffi.ERR_INVALID
    assert status(mode=0, max_probes=0)[0] == _ffi.ERR_INVALID
    assert status(probes=0)[0] == _ffi.ERR_INVALID
    assert status(k=0)[0] == _ffi.ERR_INVALID
    assert status(k=2049)[0] == _ffi.ERR_UNSUPPORTED
    assert status(metric="l1")[0] == _ffi.ERR_UNSUPPORTED
    st, msg = status(queries=np.zeros((2, fx.dim + 1), np.float32))
    assert st == _ffi.ERR_DIM_MISMATCH and msg == f"different vector dimensions {fx.dim} and {fx.dim + 1}"
    with pytest.raises(ValueError, match='invalid value for parameter "ivfflat.iterative_scan": "strict_order"'):
        main.gpu.search_iterative(fx.q, 10, 3, mode="strict_order")


def test_9000_lists(ctx, oracle):
    """9000 lists on the recipe of test_ivf_device_search_and_more_than_8192_lists; k = 2048 makes every query walk all 200."""
    import vsrbac
    rng = np.random.default_rng(77)
    n, dim, lists = 20_000, 16, 9000
    x = rng.integers(0, 64, (n, dim)).astype(np.float32)
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    centers = x[np.sort(rng.choice(n, lists, replace=False))] + 0.5
    oivf = OracleIvf.from_centers(oracle, "l2", x, centers)
    corpus = ctx.load_corpus(x, blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 2, replace=False)]
    ur = [(1, 1)]
    corpus.load_rbac(ur, perms)
    gpu = corpus.load_ivf(centers, oivf.assign)
    nq, probes, max_probes = 12, 40, 200
    q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    mask = oracle.user_row_mask(1, ur, perms, doc)
    filt = [corpus.filter_for_user(1, vsrbac.RANGES)] * nq
    for k in (10, 2048):
        want = [iterative_search(oivf, q[i], k, probes, max_probes, doc, blk, mask) for i in range(nq)]
        if k == 2048:
            assert all(w[2] == 200 for w in want)
        res, scanned = gpu.search_iterative(q, k, probes, "l2", filt, "relaxed_order", max_probes)
        check_against_model(res, scanned, want, k)
    gpu.free()
    corpus.free()


def test_launch_above_64_kib_of_lds(ctx, oracle):
    """12000 lists (48 KB of centre keys) and k = 2048 (20 KB of result keys): the launch asks for more than the 64 KiB a
    kernel gets by default.  Most lists are empty, and an empty batch must not stop the scan."""
    rng = np.random.default_rng(78)
    n, dim, lists = 4000, 4, 12000
    x = rng.integers(0, 64, (n, dim)).astype(np.float32)
    centers = rng.integers(0, 64, (lists, dim)).astype(np.float32) + 0.5
    oivf = OracleIvf.from_centers(oracle, "l2", x, centers)
    assert len(set(oivf.assign.tolist())) < lists // 2
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_ivf(centers, oivf.assign)
    mask = (np.arange(n) % 2 == 0).astype(np.uint8)
    nq = 6
    filt = [corpus.filter_from_bytemask(mask)] * nq
    q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    for k, probes, max_probes in ((2048, 50, 3000), (300, 7, 32768)):
        want = [iterative_search(oivf, q[i], k, probes, max_probes, mask=mask) for i in range(nq)]
        assert all(w[2] > 5 * probes for w in want)
        res, scanned = gpu.search_iterative(q, k, probes, "l2", filt, "relaxed_order", max_probes)
        check_against_model(res, scanned, want, k)
    gpu.free()
    corpus.free()


@pytest.fixture(scope="module")
def tap(ctx, oracle):
    x, oivf = tap_corpus(oracle)
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_ivf(oivf.centers, oivf.assign)
    yield x, oivf, corpus, gpu
    gpu.free()
    corpus.free()


def test_tap_041_counts(tap):
    """pgvector test/t/041_ivfflat_iterative_scan: 10 of 100 000 rows pass the filter, LIMIT 11, probes = 10."""
    x, oivf, corpus, gpu = tap
    mask = (np.arange(len(x)) % 10000 == 0).astype(np.uint8)
    filt = [corpus.filter_from_bytemask(mask)] * 20
    res, _ = gpu.search_iterative(x[:20], 11, 10, "l2", filt, "relaxed_order", 32768)
    assert (res.counts == 10).all()
    for max_probes in (30, 50, 70):
        res, scanned = gpu.search_iterative(x[:20], 11, 10, "l2", filt, "relaxed_order", max_probes)
        mean = res.counts.mean()
        print("max_probes", max_probes, "mean count", mean)
        assert (scanned == max_probes).all()
        assert max_probes / 10 - 2 < mean < max_probes / 10 + 2


@pytest.mark.parametrize("c,probes,threshold", [(100, 1, 0.57), (100, 10, 0.98), (1000, 1, 0.80)])
def test_tap_042_recall(oracle, tap, c, probes, threshold):
    """pgvector test/t/042_ivfflat_iterative_scan_recall: recall of the first 20 of the stream against the exact answer."""
    x, oivf, corpus, gpu = tap
    mask = (np.arange(len(x)) % c == 0).astype(np.uint8)
    q = tap_queries()
    filt = [corpus.filter_from_bytemask(mask)] * len(q)
    res, _ = gpu.search_iterative(q, 20, probes, "l2", filt, "relaxed_order", 32768)
    exact = corpus.search(q, 20, "l2", filt)
    assert (res.counts == 20).all()
    rec = np.mean([recall_at(res.rows[i], exact.rows[i]) for i in range(len(q))])
    print("c", c, "probes", probes, "recall", rec)
    assert rec >= threshold
