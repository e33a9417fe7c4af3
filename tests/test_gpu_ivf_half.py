"""IVFFlat over halfvec corpora (K3h: vsr_ivf_kmeans_half / vsr_ivf_assign_half / vsr_ivf_load_half, searched by the float
vsr_ivf_* entry points) against the index oracle.  A halfvec index IS the oracle's index over the widened rows with the binary16
centres widened, asked with the query rounded to binary16:
    OracleIvf.from_centers(oracle, metric, x16.astype(np.float32), c16.astype(np.float32))   and   q.astype(f16).astype(f32)

Bit-for-bit comparisons use data whose fp32 row sums are exact in any order (the row kernels use fmaf): rows of small integers,
centres that are binary16 values, and queries integer + 0.5 + 2^-13 -- fp32 values that round to integer + 0.5 in binary16, so a
kernel that forgets to round the query returns other distance bits (and, for the centres, possibly other lists).  Centre
distances are sequential on both sides, so probe and assign compare bit for bit on any data."""
import ctypes

import numpy as np
import pytest

import ivf_half_model as kmodel
from ivf_iterative_model import ParityFixture, iterative_search
from oracle.oracle import IvfIndex as OracleIvf

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32
Q_OFFSET = F32(0.5 + 2.0 ** -13)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _small_ints(rng, shape):
    return rng.integers(0, 32, shape).astype(F32)


def _rounded(q):
    return np.asarray(q, dtype=F32).astype(F16).astype(F32)


def _queries(rng, x, nq):
    """integer + 0.5 + 2^-13 in every element; what `$1::halfvec` holds is integer + 0.5"""
    q = (x[rng.integers(0, len(x), nq)] + rng.integers(-1, 2, (nq, x.shape[1])).astype(F32) + Q_OFFSET).astype(F32)
    assert (_rounded(q) != q).all() and (_rounded(q) * 2 == np.floor(_rounded(q) * 2)).all()
    return q


def _is_f16(a):
    return (np.asarray(a, dtype=F32).astype(F16).astype(F32) == a).all()


class Fixture:
    """n x dim rows of 0..31, `lists` centres of which some own no row (the far ones), a small RBAC: user 1 sees ~2 % of the
    documents, user 2 a quarter, user 3 none."""

    def __init__(self, oracle, n, dim, lists, nq, seed):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.lists = n, dim, lists
        self.x = _small_ints(rng, (n, dim))
        self.doc = (np.arange(n) // 10 + 1).astype(np.int32)
        self.blk = (np.arange(n) + 1).astype(np.int64)
        ndocs = int(self.doc.max())
        docs = np.arange(1, ndocs + 1)
        self.perms = [(1, int(d)) for d in rng.choice(docs, max(ndocs // 50, 2), replace=False)] + \
                     [(2, int(d)) for d in rng.choice(docs, ndocs // 4, replace=False)]
        self.user_roles = [(1, 1), (2, 2), (3, 3)]
        far = max(lists // 16, 1)
        self.centers = np.concatenate([self.x[np.sort(rng.choice(n, lists - far, replace=False))] + 0.25,
                                       1000.0 + _small_ints(rng, (far, dim))]).astype(F32)
        assert _is_f16(self.centers) and _is_f16(self.x)
        self.oivf = OracleIvf.from_centers(oracle, "l2", self.x, self.centers)
        assert len(set(self.oivf.assign.tolist())) < lists                     # some lists own no row
        self.masks = {u: oracle.user_row_mask(u, self.user_roles, self.perms, self.doc) for u in (1, 2, 3)}
        self.q = _queries(rng, self.x, nq)
        self.qr = _rounded(self.q)
        self.users = rng.integers(1, 3, nq)


class Loaded:
    def __init__(self, ctx, fx):
        self.fx = fx
        self.corpus = ctx.load_corpus_half(fx.x.astype(F16), fx.blk, fx.doc)
        self.corpus.load_rbac(fx.user_roles, fx.perms)
        self.gpu = self.corpus.load_ivf_half(fx.centers.astype(F16), fx.oivf.assign)

    def free(self):
        self.gpu.free()
        self.corpus.free()


@pytest.fixture(scope="module")
def fx16(oracle):
    return Fixture(oracle, 6000, 16, 64, 12, seed=301)


@pytest.fixture(scope="module")
def fx64(oracle):
    return Fixture(oracle, 6000, 64, 64, 40, seed=302)


def _check_probe_and_search(ctx, ld, k=100, probes_set=(1, 5, None)):
    import vsrbac
    fx = ld.fx
    nq = len(fx.q)
    kernels = set()
    for probes in probes_set:
        probes = fx.lists if probes is None else probes
        got_lists = ld.gpu.probe(fx.q, probes)
        for i in range(nq):
            assert got_lists[i].tolist() == fx.oivf.probe(fx.qr[i], probes).tolist(), (probes, i)
        for kind in ("none", "ranges", "bitmap"):
            if kind == "none":
                filters, ms = None, [None] * nq
            else:
                mode = vsrbac.RANGES if kind == "ranges" else vsrbac.BITMAP
                filters = [ld.corpus.filter_for_user(int(u), mode) for u in fx.users]
                ms = [fx.masks[int(u)] for u in fx.users]
            res = ld.gpu.search(fx.q, k, probes, "l2", filters)
            kernels.add(ctx.last_scan_kernel())
            for i in range(nq):
                idx, dist = fx.oivf.search(fx.qr[i], k, probes, fx.doc, fx.blk, ms[i])
                m = int(res.counts[i])
                assert m == idx.size, (probes, kind, i, m, idx.size)
                np.testing.assert_array_equal(res.rows[i, :m], idx, err_msg=f"{probes} {kind} {i}")
                np.testing.assert_array_equal(res.dist[i, :m], dist.astype(F32), err_msg=f"{probes} {kind} {i}")
                np.testing.assert_array_equal(res.block_ids[i, :m], fx.blk[idx])
                np.testing.assert_array_equal(res.doc_ids[i, :m], fx.doc[idx])
                assert (res.rows[i, m:] == -1).all() and (res.block_ids[i, m:] == -1).all() and (res.doc_ids[i, m:] == -1).all()
                assert np.isposinf(res.dist[i, m:]).all()
    return kernels


@pytest.mark.parametrize("which", ["fx16", "fx64"])
def test_probe_search_filters(ctx, request, which):
    """6000 x 16 takes K1h (dim < 61); 6000 x 64 with 40 queries shares passes between the queries of a list.  Either way the
    kernel that scans the view must be a half instantiation."""
    fx = request.getfixturevalue(which)
    ld = Loaded(ctx, fx)
    try:
        kernels = _check_probe_and_search(ctx, ld)
        print(which, "scan kernels:", sorted(kernels))
        assert kernels and all("half rows" in name for name in kernels), kernels
        # probes = lists is the exact scan of the half corpus
        full = ld.corpus.search(fx.q, 100, "l2")
        res = ld.gpu.search(fx.q, 100, fx.lists, "l2")
        np.testing.assert_array_equal(res.rows, full.rows)
        np.testing.assert_array_equal(res.dist, full.dist)
        np.testing.assert_array_equal(res.counts, full.counts)
    finally:
        ld.free()


@pytest.mark.parametrize("dim", [20, 264])
def test_other_dimensions(ctx, oracle, dim):
    """dim 20: padding inside a 16-byte chunk of 8 halves; dim 264: 33 chunks, a half-wave's second step."""
    fx = Fixture(oracle, 400, dim, 8, 5, seed=310 + dim)
    ld = Loaded(ctx, fx)
    try:
        kernels = _check_probe_and_search(ctx, ld, k=20, probes_set=(1, 3, None))
        assert all("half rows" in name for name in kernels), kernels
    finally:
        ld.free()


def test_same_answers_as_the_fp32_index(ctx, fx16):
    """An fp32 corpus of the widened rows, loaded with the widened centres and asked with the rounded queries, returns the half
    index's rows, distances and counts.  device_bytes of both count the list-ordered image of the rows (2 against 4 bytes per
    element; the fp32 one with its screening planes when the corpus has them), the per-row norms and rank map, the centres (2
    against 4 bytes per element) and the list offsets -- not the filters' cached bitmaps."""
    import vsrbac
    fx = fx16
    ld = Loaded(ctx, fx)
    c32 = ctx.load_corpus(fx.x, fx.blk, fx.doc)
    c32.load_rbac(fx.user_roles, fx.perms)
    g32 = c32.load_ivf(fx.centers, fx.oivf.assign)
    try:
        for probes in (1, 5, 64):
            for mode in (None, vsrbac.RANGES, vsrbac.BITMAP):
                fh = None if mode is None else [ld.corpus.filter_for_user(int(u), mode) for u in fx.users]
                f32 = None if mode is None else [c32.filter_for_user(int(u), mode) for u in fx.users]
                a = ld.gpu.search(fx.q, 100, probes, "l2", fh)
                b = g32.search(fx.qr, 100, probes, "l2", f32)
                np.testing.assert_array_equal(a.rows, b.rows)
                np.testing.assert_array_equal(a.dist, b.dist)
                np.testing.assert_array_equal(a.counts, b.counts)
        hb, fb = ld.gpu.device_bytes(), g32.device_bytes()
        print("device_bytes half", hb, "fp32", fb)
        rows_h, rows_f = fx.n * fx.dim * 2, fx.n * fx.dim * 4
        assert rows_h <= hb < fb and fb >= rows_f
        assert hb <= rows_h + fx.n * 8 + fx.lists * fx.dim * 2 + (fx.lists + 1) * 4 + 4096
    finally:
        g32.free()
        c32.free()
        ld.free()


def test_assign_in_caller_order_with_tied_centres(ctx, oracle, fx16):
    fx = fx16
    rng = np.random.default_rng(320)
    centers = fx.centers.copy()
    centers[9] = centers[3]                                   # duplicated centres: every tie goes to the lower list
    centers[40] = centers[3]
    centers[21] = centers[20]
    perm = rng.permutation(fx.n)                              # caller order != (document, block) order
    corpus = ctx.load_corpus_half(fx.x[perm].astype(F16), fx.blk[perm], fx.doc[perm])
    try:
        for metric in ("l2", "ip", "cosine"):
            cs = centers if metric == "l2" else centers[:60]  # (the far centres would own every row by inner product)
            oivf = OracleIvf.from_centers(oracle, metric, fx.x, cs)
            got = corpus.ivf_assign_half(cs.astype(F16), metric)
            np.testing.assert_array_equal(got, oivf.assign[perm], err_msg=metric)
            if metric == "l2":
                assert not np.isin(got, (9, 40, 21)).any() and np.isin(got, (3, 20)).any()
                gpu = corpus.load_ivf_half(cs.astype(F16), got)
                res = gpu.search(fx.q, 20, 3, "l2")
                for i in range(len(fx.q)):
                    idx, dist = oivf.search(fx.qr[i], 20, 3, fx.doc, fx.blk)
                    m = idx.size
                    assert res.counts[i] == m
                    np.testing.assert_array_equal(res.block_ids[i, :m], fx.blk[idx])
                    np.testing.assert_array_equal(res.rows[i, :m], perm.argsort()[idx])     # the caller's row numbers
                    np.testing.assert_array_equal(res.dist[i, :m], dist.astype(F32))
                gpu.free()
    finally:
        corpus.free()


def test_more_than_64_kib_of_keys(ctx, oracle):
    """17 000 lists are 68 000 bytes of centre keys: the probe (fp32 queries), the assignment (binary16 rows) and the iterative
    scan are three kernel instantiations that each must raise their own dynamic-LDS limit."""
    import torch
    import vsrbac
    rng = np.random.default_rng(330)
    n, dim, lists = 20_000, 8, 17_000
    x = _small_ints(rng, (n, dim))
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    centers = (x[np.sort(rng.choice(n, lists, replace=False))] + 0.5).astype(F32)
    oivf = OracleIvf.from_centers(oracle, "l2", x, centers)
    corpus = ctx.load_corpus_half(x.astype(F16), blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 2, replace=False)]
    ur = [(1, 1)]
    corpus.load_rbac(ur, perms)
    try:
        np.testing.assert_array_equal(corpus.ivf_assign_half(centers.astype(F16), "l2"), oivf.assign)
        gpu = corpus.load_ivf_half(centers.astype(F16), oivf.assign)
        nq, k, probes = 12, 10, 40
        q = _queries(rng, x, nq)
        qr = _rounded(q)
        got_lists = gpu.probe(q, probes)
        for i in range(nq):
            assert got_lists[i].tolist() == oivf.probe(qr[i], probes).tolist(), i
        mask = oracle.user_row_mask(1, ur, perms, doc)
        filt = [corpus.filter_for_user(1, vsrbac.RANGES)] * nq
        host = gpu.search(q, k, probes, "l2", filt)
        dq = torch.from_numpy(q).cuda()
        d_blk = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        d_row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        d_doc = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu.search_device(dq.data_ptr(), nq, k, probes, "l2", filt, d_blk.data_ptr(), d_doc.data_ptr(), d_row.data_ptr(),
                          d_dist.data_ptr(), d_cnt.data_ptr())
        np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)
        np.testing.assert_array_equal(d_row.cpu().numpy(), host.rows)
        np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
        np.testing.assert_array_equal(d_doc.cpu().numpy(), host.doc_ids)
        np.testing.assert_array_equal(d_dist.cpu().numpy(), host.dist)
        for i in range(nq):
            idx, dist = oivf.search(qr[i], k, probes, doc, blk, mask)
            m = host.counts[i]
            assert m == idx.size
            np.testing.assert_array_equal(host.rows[i, :m], idx)
            np.testing.assert_array_equal(host.dist[i, :m], dist.astype(F32))
        # the iterative scan's instantiation: k = 300 rows under the filter need more than the first 40 lists
        res, scanned = gpu.search_iterative(q[:4], 300, probes, "l2", filt[:4], "relaxed_order", 400)
        for i in range(4):
            rows, dist, lists_scanned = iterative_search(oivf, qr[i], 300, probes, 400, doc, blk, mask)
            assert lists_scanned > probes
            assert res.counts[i] == len(rows) and scanned[i] == lists_scanned
            np.testing.assert_array_equal(res.rows[i, :len(rows)], rows)
            np.testing.assert_array_equal(res.dist[i, :len(rows)], dist.astype(F32))
        gpu.free()
    finally:
        corpus.free()


# ---- iterative scans: ParityFixture as a halfvec corpus and index ---------------------------------------------------------
class LoadedParity:
    def __init__(self, ctx, fx):
        import vsrbac
        self.fx = fx
        self.corpus = ctx.load_corpus_half(fx.x.astype(F16), fx.blk, fx.doc)
        self.corpus.load_rbac(fx.user_roles, fx.perms)
        self.gpu = self.corpus.load_ivf_half(fx.centers.astype(F16), fx.oivf.assign)
        self.filters = {(None, None): None}
        for u in (1, 2, 3):
            for mode in (vsrbac.BITMAP, vsrbac.RANGES):
                self.filters[(u, mode)] = [self.corpus.filter_for_user(u, mode)] * len(fx.q)

    def free(self):
        self.gpu.free()
        self.corpus.free()


@pytest.fixture(scope="module")
def parity(ctx, oracle):
    fx = ParityFixture(oracle)
    assert _is_f16(fx.x) and _is_f16(fx.centers)
    fx.q_gpu = (fx.q + Q_OFFSET).astype(F32)                  # what the GPU is asked
    fx.q = _rounded(fx.q_gpu)                                 # what the model is asked: `$1::halfvec`
    assert (fx.q != fx.q_gpu).all()
    ld = LoadedParity(ctx, fx)
    yield ld
    ld.free()


@pytest.mark.parametrize("user", [None, 1, 2, 3])
def test_iterative_stream_matches_the_model(parity, user):
    import vsrbac
    fx = parity.fx
    nq = len(fx.q)
    went_on = False
    for probes, max_probes in ((1, 64), (3, 7), (5, 5)):
        for k in (1, 10, 100):
            want = [fx.model(user, i, k, probes, max_probes) for i in range(nq)]
            went_on |= any(w[2] > probes for w in want)
            for mode in ((None,) if user is None else (vsrbac.BITMAP, vsrbac.RANGES)):
                res, scanned = parity.gpu.search_iterative(fx.q_gpu, k, probes, "l2", parity.filters[(user, mode)], "relaxed_order",
                                                           max_probes)
                for i, (rows, dist, lists) in enumerate(want):
                    m = int(res.counts[i])
                    assert m == len(rows), (i, m, len(rows))
                    np.testing.assert_array_equal(res.rows[i, :m], rows, err_msg=f"query {i}")
                    np.testing.assert_array_equal(res.dist[i, :m], dist.astype(F32), err_msg=f"query {i}")
                    np.testing.assert_array_equal(res.block_ids[i, :m], fx.blk[rows])
                    assert int(scanned[i]) == lists, (i, int(scanned[i]), lists)
                    assert (res.rows[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
    assert went_on or user is None                            # the iterative kernel scanned lists past batch 0


def test_iterative_off_prefix_and_device_form(parity):
    import torch
    import vsrbac
    fx = parity.fx
    nq = len(fx.q)
    filt = parity.filters[(1, vsrbac.BITMAP)]
    for probes, mode, max_probes in ((3, "off", 64), (5, "relaxed_order", 5), (64, "relaxed_order", 32768)):
        plain = parity.gpu.search(fx.q_gpu, 100, probes, "l2", filt)
        res, scanned = parity.gpu.search_iterative(fx.q_gpu, 100, probes, "l2", filt, mode, max_probes)
        for a, b in zip(plain, res):
            np.testing.assert_array_equal(a, b)
        assert (scanned == probes).all()
    filt_r = parity.filters[(1, vsrbac.RANGES)]
    big, s_big = parity.gpu.search_iterative(fx.q_gpu, 100, 3, "l2", filt_r, "relaxed_order", 64)
    res, s = parity.gpu.search_iterative(fx.q_gpu, 10, 3, "l2", filt_r, "relaxed_order", 64)
    np.testing.assert_array_equal(res.rows, big.rows[:, :10])
    np.testing.assert_array_equal(res.dist, big.dist[:, :10])
    assert (res.counts == np.minimum(big.counts, 10)).all() and (s <= s_big).all()
    k, probes, max_probes = 10, 1, 64
    host, h_scanned = parity.gpu.search_iterative(fx.q_gpu, k, probes, "l2", filt, "relaxed_order", max_probes)
    assert (h_scanned > 1).all()
    dq = torch.from_numpy(fx.q_gpu).cuda()
    d_blk = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d_doc = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    d_dist = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    d_pr = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    parity.gpu.search_iterative_device(dq.data_ptr(), nq, k, probes, "l2", filt, "relaxed_order", max_probes, d_blk.data_ptr(),
                                       d_doc.data_ptr(), d_row.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), d_pr.data_ptr())
    np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)
    np.testing.assert_array_equal(d_row.cpu().numpy(), host.rows)
    np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
    np.testing.assert_array_equal(d_doc.cpu().numpy(), host.doc_ids)
    np.testing.assert_array_equal(d_dist.cpu().numpy(), host.dist)
    np.testing.assert_array_equal(d_pr.cpu().numpy(), h_scanned)


def test_cosine_opclass_on_real_valued_unit_rows(ctx, oracle):
    """halfvec_cosine_ops on the pattern of test_ivf_cosine_opclass_on_unit_rows, with its tolerances: unit rows rounded to
    binary16, the oracle's spherical centres rounded to binary16.  A centre-distance near-tie may order two lists the other way
    (the rows' sums use fmaf), so rows are compared where the lists agree, and nearly all must."""
    rng = np.random.default_rng(71)
    n, dim = 30_000, 96
    x = rng.normal(size=(n, dim)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x16 = x.astype(F16)
    xw = x16.astype(F32)
    c16 = OracleIvf(oracle, "cosine", xw, lists=30, seed=2).centers.astype(F16)
    oivf = OracleIvf.from_centers(oracle, "cosine", xw, c16.astype(F32))
    corpus = ctx.load_corpus_half(x16)
    got = corpus.ivf_assign_half(c16, "cosine")
    np.testing.assert_array_equal(got, oivf.assign)           # sequential sums on both sides: any data
    gpu = corpus.load_ivf_half(c16, got)
    q = x[rng.integers(0, n, 20)] + 0.05 * rng.normal(size=(20, dim)).astype(F32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = q.astype(F32)
    qr = _rounded(q)
    got_lists = gpu.probe(q, 4, "cosine")
    res = gpu.search(q, 50, 4, "cosine")
    agree = 0
    for i in range(20):
        want_lists = oivf.probe(qr[i], 4)
        agree += got_lists[i].tolist() == want_lists.tolist()
        if got_lists[i].tolist() != want_lists.tolist():
            continue
        idx, dist = oivf.search(qr[i], 50, 4)
        assert len(set(res.rows[i].tolist()) & set(idx.tolist())) >= 49
        np.testing.assert_allclose(res.dist[i], dist, rtol=1e-4, atol=1e-4)
    assert agree >= 19
    gpu.free()
    corpus.free()


def test_refusals(ctx, fx16):
    import vsrbac
    from vsrbac import _ffi
    fx = fx16
    c16 = fx.centers.astype(F16)

    def refused(fn, *a, **kw):
        with pytest.raises(vsrbac.VsrError) as e:
            fn(*a, **kw)
        return e.value.status, str(e.value)

    # the _half entry points on an fp32 corpus
    c32 = ctx.load_corpus(fx.x, fx.blk, fx.doc)
    st, msg = refused(c32.load_ivf_half, c16, fx.oivf.assign)
    assert st == _ffi.ERR_INVALID and "the corpus is not a halfvec corpus" in msg
    st, msg = refused(c32.ivf_assign_half, c16)
    assert st == _ffi.ERR_INVALID and "the corpus is not a halfvec corpus" in msg
    c32.free()
    ld = Loaded(ctx, fx)
    try:
        corpus, gpu = ld.corpus, ld.gpu
        # the float entry points on the half corpus, still
        st, msg = refused(corpus.load_ivf, fx.centers, fx.oivf.assign)
        assert st == 6 and "halfvec" in msg and "vsr_ivf_load_half" in msg
        st, msg = refused(corpus.ivf_assign, fx.centers)
        assert st == 6 and "halfvec" in msg and "vsr_ivf_assign_half" in msg
        # L1
        assert refused(gpu.search, fx.q, 10, 3, "l1")[0] == _ffi.ERR_UNSUPPORTED
        assert refused(gpu.search_iterative, fx.q, 10, 3, "l1")[0] == _ffi.ERR_UNSUPPORTED
        assert refused(corpus.ivf_assign_half, c16, "l1")[0] == _ffi.ERR_UNSUPPORTED
        assert refused(ctx.ivf_kmeans_half, fx.x[:100].astype(F16), 4, "l1")[0] == _ffi.ERR_UNSUPPORTED
        # wrong dimension
        bad = np.zeros((2, fx.dim + 1), F32)
        want = f"different halfvec dimensions {fx.dim} and {fx.dim + 1}"
        for fn, args in ((gpu.search, (bad, 10, 3)), (gpu.search_iterative, (bad, 10, 3)), (gpu.probe, (bad, 3))):
            st, msg = refused(fn, *args)
            assert st == _ffi.ERR_DIM_MISMATCH and msg == want, (fn, msg)
        # a host query element that overflows binary16
        big = fx.q.copy()
        big[1, 3] = 70000.0
        for fn, args in ((gpu.search, (big, 10, 3)), (gpu.search_iterative, (big, 10, 3)), (gpu.probe, (big, 3)),
                         (gpu.search_iterative, (big, 10, 3, "l2", None, "off"))):
            st, msg = refused(fn, *args)
            assert st == _ffi.ERR_INVALID and msg == '"70000" is out of range for type halfvec', (fn, msg)
        big[1, 3] = np.inf                                    # not finite: no error, as `$1::halfvec` takes it
        gpu.search(big, 10, 3)
        # lists out of the reloption's range
        zero = np.zeros(fx.n, np.int32)
        h = ctypes.c_void_p()
        as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert ctx._lib.vsr_ivf_load_half(corpus._h, as_ptr(c16), 0, as_ptr(zero), ctypes.byref(h)) == _ffi.ERR_UNSUPPORTED
        assert "lists must be between 1 and 32768 (got 0)" in ctx._lib.vsr_last_error().decode() and not h.value
        assert ctx._lib.vsr_ivf_assign_half(corpus._h, as_ptr(c16), 0, 0, as_ptr(zero)) == _ffi.ERR_UNSUPPORTED
        assert refused(corpus.load_ivf_half, np.zeros((32769, fx.dim), F16), zero)[0] == _ffi.ERR_UNSUPPORTED
        assert refused(corpus.ivf_assign_half, np.zeros((32769, fx.dim), F16))[0] == _ffi.ERR_UNSUPPORTED
        assert refused(ctx.ivf_kmeans_half, fx.x[:100].astype(F16), 0)[0] == _ffi.ERR_INVALID          # as vsr_ivf_kmeans
        assert refused(ctx.ivf_kmeans_half, fx.x[:100].astype(F16), 32769)[0] == _ffi.ERR_INVALID
        # a row_list entry out of range
        rl = fx.oivf.assign.copy()
        rl[77] = fx.lists
        st, msg = refused(corpus.load_ivf_half, c16, rl)
        assert st == _ffi.ERR_INVALID and "row 77 has list 64" in msg
        rl[77] = -1
        assert refused(corpus.load_ivf_half, c16, rl)[0] == _ffi.ERR_INVALID
        # halfvec values only
        with pytest.raises(ValueError, match="np.float16"):
            corpus.load_ivf_half(fx.centers, fx.oivf.assign)
    finally:
        ld.free()
    # n = 0
    empty = ctx.load_corpus_half(np.zeros((0, 8), dtype=F16))
    assert empty.ivf_assign_half(np.zeros((3, 8), F16)).size == 0
    g0 = empty.load_ivf_half(np.zeros((3, 8), F16), np.zeros(0, np.int32))
    res = g0.search(np.ones((2, 8), F32), 5, 2)
    assert (res.counts == 0).all() and (res.rows == -1).all()
    res, scanned = g0.search_iterative(np.ones((2, 8), F32), 5, 1, "l2", None, "relaxed_order", 3)
    assert (res.counts == 0).all() and (scanned == 3).all()
    g0.free()
    empty.free()


# ---- k-means ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["integer", "repeated"])
def test_kmeans_half_equals_the_model(ctx, case):
    """Switch on: vsr_ivf_kmeans_half against tests/ivf_half_model.py (pinned to the oracle, switch off, by test_ivf_half_cpu.py):
    the same binary16 centres and the same number of Elkan iterations."""
    x, lists = kmodel.integer_case() if case == "integer" else kmodel.repeated_case()
    assert _is_f16(x)
    for seed in (1, 7):
        want, want_it = kmodel.kmeans(x, lists, seed, "l2", round_half=True)
        got, got_it = ctx.ivf_kmeans_half(x.astype(F16), lists, "l2", seed)
        assert got.dtype == F16 and got.shape == want.shape
        np.testing.assert_array_equal(got.view(np.uint16), want.astype(F16).view(np.uint16))
        assert got_it == want_it
        assert _is_f16(want)
    want0, _ = kmodel.kmeans(np.zeros((0, 8), F32), 5, 3, "l2", round_half=True)
    got0, it0 = ctx.ivf_kmeans_half(np.zeros((0, 8), F16), 5, "l2", 3)
    np.testing.assert_array_equal(got0.view(np.uint16), want0.astype(F16).view(np.uint16))
    assert it0 == 0


def test_kmeans_half_spherical_centres_are_unit_halfvecs(ctx):
    """The spherical variant goes through acos, whose last bit differs between libms, and one such bit can flip a binary16
    rounding: it is not compared to the model.  Each centre is the binary16 rounding of a unit vector, so its norm misses 1 by the
    rounding errors of its elements only; between the model and the GPU only the sign pattern of those errors can differ, the
    bound per element is the same.  Measured on this data (1500 x 8 unit rows rounded to binary16, 6 lists, seed 7): the model's
    largest |norm - 1| is 2.768e-4; the GPU's must be within twice the model's."""
    x, lists = kmodel.integer_case()
    u16 = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F16)
    want, _ = kmodel.kmeans(u16.astype(F32), lists, 7, "cosine", round_half=True)
    dev_model = np.abs(np.sqrt((want.astype(np.float64) ** 2).sum(axis=1)) - 1).max()
    for metric in ("cosine", "ip"):
        got, it = ctx.ivf_kmeans_half(u16, lists, metric, 7)
        dev = np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1).max()
        print(metric, "iterations", it, "largest |norm - 1|: model", dev_model, "gpu", dev)
        assert it >= 1 and 0 < dev_model < 1e-3
        assert dev <= 2 * dev_model


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_build_recall(ctx, metric):
    """pgvector test/t/032_ivfflat_halfvec_build_recall.pl: 100 000 x 10 uniform rows, 20 queries, lists = 100, LIMIT 20.  The
    expected set is tie-aware: every row whose exact distance is <= the 20th.  Floors: probes 1 >= 0.33 and probes 10 >= 0.93
    (not checked for <#>, as in the reference), probes 100 = 1.00 (cosine >= 0.98).  Cosine: unit rows and queries, as the
    opclass is defined here."""
    rng = np.random.default_rng(3200)
    n, dim, k = 100_000, 10, 20
    x = rng.random((n, dim)).astype(F32)
    q = rng.random((20, dim)).astype(F32)
    if metric == "cosine":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    x16 = x.astype(F16)
    corpus = ctx.load_corpus_half(x16)
    c32 = ctx.load_corpus(x16.astype(F32))
    try:
        gpu, centers, row_list = corpus.build_ivf_half(x16, lists=100, metric=metric, seed=1)
        g32, _, _ = c32.build_ivf(x16.astype(F32), lists=100, metric=metric, seed=1)
        assert centers.dtype == F16 and centers.shape == (100, dim) and row_list.shape == (n,)
        exact = corpus.search(q, 64, metric)
        expected = []
        for i in range(len(q)):
            assert exact.dist[i, 63] > exact.dist[i, k - 1]   # the tie class of the 20th ends inside the 64
            expected.append(set(exact.rows[i, exact.dist[i] <= exact.dist[i, k - 1]].tolist()))

        def recall(index, probes):
            res = index.search(_rounded(q) if index is g32 else q, k, probes, metric)
            hit = sum(len(set(res.rows[i, :res.counts[i]].tolist()) & expected[i]) for i in range(len(q)))
            return hit / (k * len(q))

        floors = {1: 0.33, 10: 0.93, 100: 0.98 if metric == "cosine" else 1.00}
        for probes, floor in floors.items():
            r, r32 = recall(gpu, probes), recall(g32, probes)
            print(metric, "probes", probes, "recall half", r, "fp32 build over the widened rows", r32)
            if metric == "ip" and probes < 100:
                continue
            assert r >= floor, (metric, probes, r)
        gpu.free()
        g32.free()
    finally:
        c32.free()
        corpus.free()
