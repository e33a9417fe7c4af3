"""pgvector's IVFFlat iterative index scan over a bit index (K3i's bit instantiation: vsr_ivf_search_bit_iterative(_device))
against the stream of tests/ivf_bit_model.py: rows, fp32 Hamming counts, counts and out_probes, exactly.  The fixture is the
parity fixture of the float scans as bits: 6000 x 136, 64 lists of which 4 own no row, users none / 1 (~2 % of the rows) / 2 (a
quarter) / 3 (nothing).  Queries go in with their pad bits set."""
import numpy as np
import pytest

from ivf_bit_model import BitFixture

pytestmark = pytest.mark.gpu

CASES = ((1, 1), (1, 3), (3, 64), (5, 32768))                 # (probes, max_probes)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class LoadedParity:
    def __init__(self, ctx, fx):
        import vsrbac
        self.fx = fx
        self.corpus = ctx.load_corpus_bit(fx.rows, fx.dim, fx.blk, fx.doc)
        self.corpus.load_rbac(fx.user_roles, fx.perms)
        self.gpu = self.corpus.load_ivf_bit(fx.centers, fx.m.assign)
        self.filters = {(None, None): None}
        for u in (1, 2, 3):
            for mode in (vsrbac.BITMAP, vsrbac.RANGES):
                self.filters[(u, mode)] = [self.corpus.filter_for_user(u, mode)] * len(fx.q)

    def free(self):
        self.gpu.free()
        self.corpus.free()


@pytest.fixture(scope="module")
def parity(ctx):
    fx = BitFixture(6000, 136, 64, 16, seed=141, twin=False)
    assert len(set(fx.m.assign.tolist())) == 60               # 4 lists own no row
    ld = LoadedParity(ctx, fx)
    yield ld
    ld.free()


def _check_stream(ld, user, mode, k, probes, max_probes):
    fx = ld.fx
    want = [fx.m.iterative(fx.q[i], k, probes, max_probes, fx.masks[user]) for i in range(len(fx.q))]
    res, scanned = ld.gpu.search_bit_iterative(fx.q, k, probes, "hamming", ld.filters[(user, mode)], "relaxed_order", max_probes)
    for i, (rows, dist, lists) in enumerate(want):
        m = int(res.counts[i])
        assert m == len(rows), (i, m, len(rows))
        np.testing.assert_array_equal(res.rows[i, :m], rows, err_msg=f"query {i}")
        np.testing.assert_array_equal(res.dist[i, :m], dist, err_msg=f"query {i}")
        np.testing.assert_array_equal(res.block_ids[i, :m], fx.blk[rows])
        np.testing.assert_array_equal(res.doc_ids[i, :m], fx.doc[rows])
        assert int(scanned[i]) == lists, (i, int(scanned[i]), lists)
        assert (res.rows[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
    return any(w[2] > min(probes, fx.lists) for w in want)


@pytest.mark.parametrize("user", [None, 1, 2, 3])
def test_iterative_stream_matches_the_model(parity, user):
    import vsrbac
    went_on = False
    for probes, max_probes in CASES:
        for k in (10, 100):
            for mode in ((None,) if user is None else (vsrbac.BITMAP, vsrbac.RANGES)):
                went_on |= _check_stream(parity, user, mode, k, probes, max_probes)
    assert went_on                                            # the iterative kernel scanned lists past batch 0


def test_a_user_without_permission_ends_at_max_probes(parity):
    import vsrbac
    fx = parity.fx
    for probes, max_probes, end in ((1, 3, 3), (3, 64, 64), (5, 32768, 64), (7, 20, 20)):
        res, scanned = parity.gpu.search_bit_iterative(fx.q, 10, probes, "hamming", parity.filters[(3, vsrbac.BITMAP)], "relaxed_order",
                                                       max_probes)
        assert (res.counts == 0).all() and (scanned == end).all()
        assert (res.rows == -1).all() and np.isposinf(res.dist).all()


def test_off_is_search_bit_and_the_device_form_is_the_host_form(parity):
    import torch
    import vsrbac
    fx = parity.fx
    nq = len(fx.q)
    filt = parity.filters[(1, vsrbac.BITMAP)]
    for probes, mode, max_probes in ((3, "off", 64), (5, "relaxed_order", 5), (64, "relaxed_order", 32768)):
        plain = parity.gpu.search_bit(fx.q, 100, probes, "hamming", filt)
        res, scanned = parity.gpu.search_bit_iterative(fx.q, 100, probes, "hamming", filt, mode, max_probes)
        for a, b in zip(plain, res):
            np.testing.assert_array_equal(a, b)
        assert (scanned == probes).all()
    # the prefix property
    filt_r = parity.filters[(1, vsrbac.RANGES)]
    big, s_big = parity.gpu.search_bit_iterative(fx.q, 100, 3, "hamming", filt_r, "relaxed_order", 64)
    res, s = parity.gpu.search_bit_iterative(fx.q, 10, 3, "hamming", filt_r, "relaxed_order", 64)
    np.testing.assert_array_equal(res.rows, big.rows[:, :10])
    np.testing.assert_array_equal(res.dist, big.dist[:, :10])
    assert (res.counts == np.minimum(big.counts, 10)).all() and (s <= s_big).all()
    # device form
    k, probes, max_probes = 100, 1, 64
    host, h_scanned = parity.gpu.search_bit_iterative(fx.q, k, probes, "hamming", filt, "relaxed_order", max_probes)
    assert (h_scanned > 1).all()
    dq = torch.from_numpy(fx.q).cuda()
    d_blk = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_doc = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    d_dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    d_pr = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    parity.gpu.search_bit_iterative_device(dq.data_ptr(), nq, k, probes, "hamming", filt, "relaxed_order", max_probes, d_blk.data_ptr(),
                                           d_doc.data_ptr(), d_row.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), d_pr.data_ptr())
    np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)
    np.testing.assert_array_equal(d_row.cpu().numpy(), host.rows)
    np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
    np.testing.assert_array_equal(d_doc.cpu().numpy(), host.doc_ids)
    np.testing.assert_array_equal(d_dist.cpu().numpy(), host.dist)
    np.testing.assert_array_equal(d_pr.cpu().numpy(), h_scanned)


def test_long_rows_16392_bits(ctx):
    """129 chunks per row: the lane groups are whole waves that loop over the chunks and re-read the query from LDS."""
    import vsrbac
    fx = BitFixture(600, 16392, 64, 6, seed=142, twin=False)
    ld = LoadedParity(ctx, fx)
    try:
        went_on = False
        for user, mode in ((None, None), (1, vsrbac.BITMAP), (2, vsrbac.RANGES)):
            for k, probes, max_probes in ((10, 1, 3), (100, 3, 64)):
                went_on |= _check_stream(ld, user, mode, k, probes, max_probes)
        assert went_on
    finally:
        ld.free()


def test_more_than_64_kib_of_keys(ctx):
    """16 500 lists are 66 000 bytes of centre keys: the bit instantiation of the iterative kernel must raise its own
    dynamic-LDS limit.  k = 300 rows under the filter need more than the first 40 lists."""
    import vsrbac
    import bit_model
    from ivf_bit_model import IvfBit
    rng = np.random.default_rng(731)
    n, dim, lists = 2000, 136, 16_500
    bits = rng.random((n, dim)) < 0.2
    rows = bit_model.set_pad_bits(bit_model.pack(bits), dim)
    centers = bit_model.set_pad_bits(bit_model.pack(bits[rng.integers(0, n, lists)] ^ (rng.random((lists, dim)) < 0.03)), dim)
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    m = IvfBit(rows, dim, centers, doc, blk)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 2, replace=False)]
    ur = [(1, 1)]
    mask = bit_model.user_row_mask(1, ur, perms, doc)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    corpus.load_rbac(ur, perms)
    try:
        gpu = corpus.load_ivf_bit(centers, m.assign)
        q = bit_model.set_pad_bits(bit_model.pack(bits[rng.integers(0, n, 4)] ^ (rng.random((4, dim)) < 0.02)), dim)
        filt = [corpus.filter_for_user(1, vsrbac.RANGES)] * 4
        res, scanned = gpu.search_bit_iterative(q, 300, 40, "hamming", filt, "relaxed_order", 4000)
        for i in range(4):
            rows_w, dist_w, lists_scanned = m.iterative(q[i], 300, 40, 4000, mask)
            assert lists_scanned > 40
            assert res.counts[i] == len(rows_w) and scanned[i] == lists_scanned
            np.testing.assert_array_equal(res.rows[i, :len(rows_w)], rows_w)
            np.testing.assert_array_equal(res.dist[i, :len(rows_w)], dist_w)
        gpu.free()
    finally:
        corpus.free()
