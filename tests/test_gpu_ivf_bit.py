"""IVFFlat over bit corpora (K3b, pgvector's ivfflat bit_hamming_ops: vsr_ivf_kmeans_bit / vsr_ivf_assign_bit / vsr_ivf_load_bit /
vsr_ivf_probe_bit / vsr_ivf_search_bit(_device)) against tests/ivf_bit_model.py, which tests/test_ivf_bit_cpu.py licenses.
Everything is an integer count, so every comparison is exact: lists, rows, fp32 distances, counts, the -1 / +Inf fill, and the
k-means byte for byte with its iteration count.  Queries, rows and centres go in with their pad bits SET: they must not count.
The iterative scans: tests/test_gpu_ivf_bit_iterative.py."""
import ctypes

import numpy as np
import pytest

import bit_model
import ivf_bit_model as model
import ivf_half_model as kmodel
from ivf_bit_model import BitFixture as Fixture

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


class Loaded:
    def __init__(self, ctx, fx):
        self.fx = fx
        self.corpus = ctx.load_corpus_bit(fx.rows, fx.dim, fx.blk, fx.doc)
        self.corpus.load_rbac(fx.user_roles, fx.perms)
        self.gpu = self.corpus.load_ivf_bit(fx.centers, fx.m.assign)

    def free(self):
        self.gpu.free()
        self.corpus.free()


def _check(res, i, j, want_rows, want_dist, fx, tag):
    m = int(res.counts[j])
    assert m == len(want_rows), (tag, i, m, len(want_rows))
    np.testing.assert_array_equal(res.rows[j, :m], want_rows, err_msg=f"{tag} {i}")
    np.testing.assert_array_equal(res.dist[j, :m], want_dist, err_msg=f"{tag} {i}")
    np.testing.assert_array_equal(res.block_ids[j, :m], fx.blk[want_rows])
    np.testing.assert_array_equal(res.doc_ids[j, :m], fx.doc[want_rows])
    assert (res.rows[j, m:] == -1).all() and (res.block_ids[j, m:] == -1).all() and (res.doc_ids[j, m:] == -1).all()
    assert np.isposinf(res.dist[j, m:]).all()


def _check_probe_and_search(ctx, ld, k=100, probes_set=(1, 5, None), single=6):
    import vsrbac
    fx = ld.fx
    nq = len(fx.q)
    kernels = set()
    for probes in probes_set:
        probes = fx.lists if probes is None else probes
        got_lists = ld.gpu.probe_bit(fx.q, probes)
        for i in range(nq):
            assert got_lists[i].tolist() == fx.m.probe(fx.q[i], probes).tolist(), (probes, i)
        for kind in ("none", "ranges", "bitmap"):
            if kind == "none":
                filters, ms = None, [None] * nq
            else:
                mode = vsrbac.RANGES if kind == "ranges" else vsrbac.BITMAP
                filters = [ld.corpus.filter_for_user(int(u), mode) for u in fx.users]
                ms = [fx.masks[int(u)] for u in fx.users]
            want = [fx.m.search(fx.q[i], k, probes, ms[i]) for i in range(nq)]
            res = ld.gpu.search_bit(fx.q, k, probes, "hamming", filters)             # all queries in one call: shared passes
            kernels.add(ctx.last_scan_kernel())
            for i in range(nq):
                _check(res, i, i, want[i][0], want[i][1], fx, f"{probes} {kind} batch")
            for i in range(min(single, nq)):                                          # one query per call
                one = ld.gpu.search_bit(fx.q[i:i + 1], k, probes, "hamming", None if filters is None else filters[i:i + 1])
                kernels.add(ctx.last_scan_kernel())
                _check(one, i, 0, want[i][0], want[i][1], fx, f"{probes} {kind} single")
    return kernels


# one chunk; one full chunk; two chunks with pad bits; 8 chunks; 129 chunks (K1b's runtime-chunk path, 600 rows)
@pytest.mark.parametrize("dim", [52, 128, 136, 1000, 16392])
def test_probe_search_filters(ctx, dim):
    n = 600 if dim == 16392 else 6000
    fx = Fixture(n, dim, 64, 40, seed=700 + dim)
    ld = Loaded(ctx, fx)
    try:
        kernels = _check_probe_and_search(ctx, ld, single=3 if dim == 16392 else 6)
        print(dim, "scan kernels:", sorted(kernels))
        assert kernels and all("K1b" in name for name in kernels), kernels
        assert any("QI=4" in name for name in kernels) and any("QI=1" in name for name in kernels)
        if dim == 16392:
            assert all("C=0" in name for name in kernels), kernels
        # probes = lists is the exact scan of the bit corpus
        full = ld.corpus.search_bit(fx.q, 100, "hamming")
        res = ld.gpu.search_bit(fx.q, 100, fx.lists)
        for a, b in zip(full, res):
            np.testing.assert_array_equal(a, b)
    finally:
        ld.free()


def test_ties_rows_by_document_and_block_centres_by_list_id(ctx):
    fx = Fixture(6000, 136, 64, 4, seed=711)
    ld = Loaded(ctx, fx)
    try:
        # two centres at the same count: probe and assign take the lower list id
        lists = ld.gpu.probe_bit(fx.q[:1], 12)[0].tolist()
        assert lists[0] == 0 and lists[1] == 11
        got = ld.corpus.ivf_assign_bit(fx.centers)
        np.testing.assert_array_equal(got, fx.m.assign)
        assert (got[:10] == 0).all() and not (got == 11).any()
        # ten copies at distance 0 come back in (document_id, block_id) order
        res = ld.gpu.search_bit(fx.q[:1], 10, 1)
        order = np.lexsort((fx.blk[:10], fx.doc[:10]))
        assert res.counts[0] == 10 and (res.dist[0] == 0).all()
        np.testing.assert_array_equal(res.rows[0], order)
        np.testing.assert_array_equal(res.doc_ids[0], fx.doc[order])
        assert len(set(fx.doc[:10].tolist())) >= 5
    finally:
        ld.free()


def test_caller_order_row_offset_and_small_corners(ctx):
    """Rows handed over in shuffled order: assignment and results speak the caller's row numbers.  row_offset, lists > n, k
    larger than the rows probed, n = 0."""
    fx = Fixture(6000, 136, 64, 8, seed=712)
    rng = np.random.default_rng(713)
    perm = rng.permutation(fx.n)
    inv = perm.argsort()
    corpus = ctx.load_corpus_bit(fx.rows[perm], fx.dim, fx.blk[perm], fx.doc[perm], row_offset=1000)
    try:
        got = corpus.ivf_assign_bit(fx.centers)
        np.testing.assert_array_equal(got, fx.m.assign[perm])
        gpu = corpus.load_ivf_bit(fx.centers, got)
        res = gpu.search_bit(fx.q, 2000, 3)                                   # k above the rows of three lists
        for i in range(len(fx.q)):
            rows, dist = fx.m.search(fx.q[i], 2000, 3)
            m = len(rows)
            assert 0 < m < 2000 and res.counts[i] == m
            np.testing.assert_array_equal(res.rows[i, :m], inv[rows])          # the caller's row numbers
            np.testing.assert_array_equal(res.block_ids[i, :m], fx.blk[rows])
            np.testing.assert_array_equal(res.dist[i, :m], dist)
            assert (res.rows[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
        gpu.free()
    finally:
        corpus.free()
    # lists > n
    small = Fixture(40, 52, 10, 3, seed=714)
    centers = np.concatenate([small.centers, small.rows])                      # 50 centres over 40 rows
    m = model.IvfBit(small.rows, 52, centers, small.doc, small.blk)
    corpus = ctx.load_corpus_bit(small.rows, 52, small.blk, small.doc)
    try:
        np.testing.assert_array_equal(corpus.ivf_assign_bit(centers), m.assign)
        gpu = corpus.load_ivf_bit(centers, m.assign)
        for probes in (1, 7, 50, 60):
            np.testing.assert_array_equal(gpu.probe_bit(small.q, probes), np.stack([m.probe(q, probes) for q in small.q]))
            res = gpu.search_bit(small.q, 100, probes)
            for i in range(len(small.q)):
                rows, dist = m.search(small.q[i], 100, probes)
                assert res.counts[i] == len(rows)
                np.testing.assert_array_equal(res.rows[i, :len(rows)], rows)
                np.testing.assert_array_equal(res.dist[i, :len(rows)], dist)
        gpu.free()
    finally:
        corpus.free()
    # n = 0
    empty = ctx.load_corpus_bit(np.zeros((0, 7), dtype=np.uint8), 52)
    assert empty.ivf_assign_bit(small.centers).size == 0
    g0 = empty.load_ivf_bit(small.centers, np.zeros(0, np.int32))
    res = g0.search_bit(small.q, 5, 2)
    assert (res.counts == 0).all() and (res.rows == -1).all() and np.isposinf(res.dist).all()
    assert g0.probe_bit(small.q, 3).shape == (3, 3)
    g0.free()
    empty.free()


def test_more_than_64_kib_of_keys(ctx):
    """16 500 lists are 66 000 bytes of centre keys: the probe (staged queries) and the assignment (rows in place) run the bit
    instantiation of the probe kernel, which must raise its own dynamic-LDS limit.  Device form = host form."""
    import torch
    import vsrbac
    rng = np.random.default_rng(730)
    n, dim, lists = 2000, 136, 16_500
    bits = rng.random((n, dim)) < 0.2
    rows = bit_model.set_pad_bits(bit_model.pack(bits), dim)
    cbits = bits[rng.integers(0, n, lists)] ^ (rng.random((lists, dim)) < 0.03)
    centers = bit_model.set_pad_bits(bit_model.pack(cbits), dim)
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    m = model.IvfBit(rows, dim, centers, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 2, replace=False)]
    ur = [(1, 1)]
    corpus.load_rbac(ur, perms)
    try:
        np.testing.assert_array_equal(corpus.ivf_assign_bit(centers), m.assign)
        gpu = corpus.load_ivf_bit(centers, m.assign)
        nq, k, probes = 12, 10, 400
        q = bit_model.set_pad_bits(bit_model.pack(bits[rng.integers(0, n, nq)] ^ (rng.random((nq, dim)) < 0.02)), dim)
        got_lists = gpu.probe_bit(q, probes)
        for i in range(nq):
            assert got_lists[i].tolist() == m.probe(q[i], probes).tolist(), i
        mask = bit_model.user_row_mask(1, ur, perms, doc)
        filt = [corpus.filter_for_user(1, vsrbac.RANGES)] * nq
        host = gpu.search_bit(q, k, probes, "hamming", filt)
        for i in range(nq):
            rows_w, dist_w = m.search(q[i], k, probes, mask)
            assert host.counts[i] == len(rows_w)
            np.testing.assert_array_equal(host.rows[i, :len(rows_w)], rows_w)
            np.testing.assert_array_equal(host.dist[i, :len(rows_w)], dist_w)
        dq = torch.from_numpy(q).cuda()
        d_blk = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        d_row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        d_doc = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu.search_bit_device(dq.data_ptr(), nq, k, probes, "hamming", filt, d_blk.data_ptr(), d_doc.data_ptr(), d_row.data_ptr(),
                              d_dist.data_ptr(), d_cnt.data_ptr())
        np.testing.assert_array_equal(d_cnt.cpu().numpy(), host.counts)
        np.testing.assert_array_equal(d_row.cpu().numpy(), host.rows)
        np.testing.assert_array_equal(d_blk.cpu().numpy(), host.block_ids)
        np.testing.assert_array_equal(d_doc.cpu().numpy(), host.doc_ids)
        np.testing.assert_array_equal(d_dist.cpu().numpy(), host.dist)
        gpu.free()
    finally:
        corpus.free()


def test_centers_of_three_bit_strings(ctx):
    """pgvector test/t/036_ivfflat_bit_centers.pl: 100 rows of bit(3) with all 8 values present, lists = 100 -- far more lists than
    values, so most centres are random draws.  For every value, probes = 1 and LIMIT 100 return exactly that value's rows."""
    rng = np.random.default_rng(36)
    vals = np.concatenate([np.arange(8), rng.integers(0, 8, 92)])
    bits = ((vals[:, None] >> np.array([2, 1, 0])[None, :]) & 1).astype(bool)
    rows = bit_model.pack(bits)
    corpus = ctx.load_corpus_bit(rows, 3)
    try:
        for seed in (1, 2, 3):
            gpu, centers, row_list = corpus.build_ivf_bit(rows, lists=100, seed=seed)
            assert centers.shape == (100, 1) and not (centers & 0x1F).any() and row_list.shape == (100,)
            for v in range(8):
                q = bit_model.pack(((v >> np.array([2, 1, 0])) & 1).astype(bool)[None, :])
                res = gpu.search_bit(q, 100, 1)
                m = int(res.counts[0])
                assert sorted(res.rows[0, :m].tolist()) == np.nonzero(vals == v)[0].tolist(), (seed, v)
                assert (res.dist[0, :m] == 0).all()
            gpu.free()
    finally:
        corpus.free()


def test_build_recall(ctx):
    """pgvector test/t/035_ivfflat_bit_build_recall.pl: 100 000 rows of 52 random bits, lists = 100 (so 10 000 sampled rows), 20
    queries, LIMIT 20, against the tie-aware exact set: every row whose Hamming count is <= the 20th.  pgvector's floors: probes
    1 >= 0.08, probes 10 >= 0.50, probes 100 = 1.00.  (A numpy restatement of this build on three seeds gave 0.17-0.22,
    0.74-0.83 and 1.00.)"""
    rng = np.random.default_rng(3500)
    n, dim, k = 100_000, 52, 20
    rows = bit_model.pack(rng.random((n, dim)) < 0.5)
    q = bit_model.pack(rng.random((20, dim)) < 0.5)
    corpus = ctx.load_corpus_bit(rows, dim)
    try:
        gpu, centers, row_list = corpus.build_ivf_bit(rows, lists=100, seed=1)
        assert centers.shape == (100, 7) and row_list.shape == (n,)
        exact = corpus.search_bit(q, 2048, "hamming")
        expected = []
        for i in range(len(q)):
            assert exact.dist[i, 2047] > exact.dist[i, k - 1]                 # the tie class of the 20th ends inside the 2048
            expected.append(set(exact.rows[i, exact.dist[i] <= exact.dist[i, k - 1]].tolist()))
        for probes, floor in ((1, 0.08), (10, 0.50), (100, 1.00)):
            res = gpu.search_bit(q, k, probes)
            hit = sum(len(set(res.rows[i, :res.counts[i]].tolist()) & expected[i]) for i in range(len(q)))
            r = hit / (k * len(q))
            print("probes", probes, "recall", r)
            assert r >= floor, (probes, r)
        gpu.free()
    finally:
        corpus.free()


# ---- k-means ------------------------------------------------------------------------------------------------------------------
def _kmeans_case(name):
    rng = np.random.default_rng({"blobs": 41, "repeated": 42, "wide": 43, "max": 44}[name])
    if name == "blobs":                                       # 1500 x 52 around 6 blobs, 6 lists
        dim, lists = 52, 6
        blobs = rng.random((6, dim)) < 0.5
        bits = blobs[rng.integers(0, 6, 1500)] ^ (rng.random((1500, dim)) < 0.1)
    elif name == "repeated":                                  # 200 x 136: 40 distinct values, 48 lists -> empty centres draw bits
        dim, lists = 136, 48
        base = rng.random((40, dim)) < 0.5
        bits = np.tile(base, (5, 1))[rng.permutation(200)]
    elif name == "wide":                                      # 300 x 1000, 8 lists
        dim, lists = 1000, 8
        blobs = rng.random((8, dim)) < 0.5
        bits = blobs[rng.integers(0, 8, 300)] ^ (rng.random((300, dim)) < 0.2)
    else:                                                     # the type's longest string: 64 x 64000, 4 lists
        dim, lists = 64000, 4
        blobs = rng.random((4, dim)) < 0.5
        bits = blobs[rng.integers(0, 4, 64)] ^ (rng.random((64, dim)) < 0.3)
    return bit_model.set_pad_bits(bit_model.pack(bits), dim), dim, lists


@pytest.mark.parametrize("case", ["blobs", "repeated", "wide", "max"])
def test_kmeans_bit_equals_the_model(ctx, case):
    """vsr_ivf_kmeans_bit against tests/ivf_bit_model.py byte for byte, out_iterations included: every quantity of this k-means is
    an integer or half-integer exact in fp32 and double, so there is no tolerance to grant."""
    samples, dim, lists = _kmeans_case(case)
    for seed in ((1, 7) if case != "max" else (1,)):
        want, want_it = model.kmeans(samples, dim, lists, seed)
        got, got_it = ctx.ivf_kmeans_bit(samples, lists, dim, seed)
        assert got.dtype == np.uint8 and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        assert got_it == want_it and got_it >= 2
        if case == "repeated":                                # not vacuous: at least 8 centres are drawn, not sample means
            distinct = {r.tobytes() for r in bit_model.pack(bit_model.unpack(samples, dim))}
            assert sum(r.tobytes() not in distinct for r in got) >= 8


def test_kmeans_bit_without_samples_is_the_random_fill(ctx):
    for dim, lists, seed in ((52, 5, 3), (136, 3, 8)):
        want, _ = model.kmeans(np.zeros((0, (dim + 7) // 8), np.uint8), dim, lists, seed)
        got, it = ctx.ivf_kmeans_bit(np.zeros((0, (dim + 7) // 8), np.uint8), lists, dim, seed)
        np.testing.assert_array_equal(got, want)
        assert it == 0 and got.any()


def test_float_and_half_kmeans_are_unchanged(ctx):
    """The kernels vsr_ivf_kmeans and vsr_ivf_kmeans_half share with the bit form still return the model's centres."""
    x, lists = kmodel.integer_case()
    for seed in (1, 7):
        want, want_it = kmodel.kmeans(x, lists, seed, "l2", round_half=False)
        got, got_it = ctx.ivf_kmeans(x, lists, "l2", seed)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got_it == want_it
        want, want_it = kmodel.kmeans(x, lists, seed, "l2", round_half=True)
        got, got_it = ctx.ivf_kmeans_half(x.astype(np.float16), lists, "l2", seed)
        np.testing.assert_array_equal(got.view(np.uint16), want.astype(np.float16).view(np.uint16))
        assert got_it == want_it


def test_device_bytes_hold_no_fp32_image(ctx):
    """6000 x 1000 bits, 64 lists: packed rows (chunks x 16 bytes), popcount and rank per row, packed centres (4 bytes per 32-bit
    word) and the offsets.  An fp32 image of the rows alone would be 24 MB."""
    fx = Fixture(6000, 1000, 64, 2, seed=740)
    ld = Loaded(ctx, fx)
    try:
        chunks, words = (fx.dim + 127) // 128, (fx.dim + 31) // 32
        b = ld.gpu.device_bytes()
        print("device_bytes", b)
        assert fx.n * chunks * 16 <= b <= fx.n * (chunks * 16 + 8) + fx.lists * (4 * words + 4) + 4096
    finally:
        ld.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import vsrbac
    from vsrbac import _ffi
    from vsrbac.engine import MAX_K
    INVALID, DIM, UNSUPPORTED = _ffi.ERR_INVALID, _ffi.ERR_DIM_MISMATCH, _ffi.ERR_UNSUPPORTED
    fx = Fixture(600, 136, 16, 4, seed=750)
    lib = ctx._lib
    as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def refused(fn, *a, **kw):
        with pytest.raises(vsrbac.VsrError) as e:
            fn(*a, **kw)
        return e.value.status, str(e.value)

    def last():
        return lib.vsr_last_error().decode()

    out = [np.zeros((4, 10), np.int64), np.zeros((4, 10), np.int32), np.zeros((4, 10), np.int64), np.zeros((4, 10), F32),
           np.zeros(4, np.int32)]
    outs = [as_ptr(a) for a in out]
    pr = np.zeros(4, np.int32)
    lists_out = np.zeros((4, 3), np.int32)
    qf = np.zeros((4, fx.dim), F32)

    # ---- a corpus that is not a bit corpus
    x32 = bit_model.unpack(fx.rows, fx.dim).astype(F32)
    c32 = ctx.load_corpus(x32, fx.blk, fx.doc)
    g32 = c32.load_ivf(bit_model.unpack(fx.centers, fx.dim).astype(F32), fx.m.assign)
    h = ctypes.c_void_p()
    zero = np.zeros(fx.n, np.int32)
    assert lib.vsr_ivf_load_bit(c32._h, as_ptr(fx.centers), fx.lists, as_ptr(zero), ctypes.byref(h)) == INVALID
    assert last() == "vsr_ivf_load_bit: the corpus is not a bit corpus" and not h.value
    assert lib.vsr_ivf_assign_bit(c32._h, as_ptr(fx.centers), fx.lists, as_ptr(zero)) == INVALID
    assert last() == "vsr_ivf_assign_bit: the corpus is not a bit corpus"
    # ---- the bit entry points on an index that is not over a bit corpus; the format refusal wins over a wrong dimension too
    for dim in (fx.dim, fx.dim + 1):
        q = np.zeros((4, (dim + 7) // 8), np.uint8)
        calls = {
            "vsr_ivf_probe_bit": lambda: lib.vsr_ivf_probe_bit(g32._h, as_ptr(q), 4, dim, 3, as_ptr(lists_out)),
            "vsr_ivf_search_bit": lambda: lib.vsr_ivf_search_bit(g32._h, as_ptr(q), 4, dim, 10, 3, 4, None, *outs),
            "vsr_ivf_search_bit_device": lambda: lib.vsr_ivf_search_bit_device(g32._h, as_ptr(q), 4, dim, 10, 3, 4, None, *outs),
            "vsr_ivf_search_bit_iterative": lambda: lib.vsr_ivf_search_bit_iterative(g32._h, as_ptr(q), 4, dim, 10, 3, 4, None, 1, 9,
                                                                                     *outs, as_ptr(pr)),
            "vsr_ivf_search_bit_iterative_device": lambda: lib.vsr_ivf_search_bit_iterative_device(g32._h, as_ptr(q), 4, dim, 10, 3, 4,
                                                                                                   None, 1, 9, *outs, as_ptr(pr)),
        }
        for who, call in calls.items():
            assert call() == INVALID, who
            assert last() == f"{who}: the index is not over a bit corpus (it is searched with vsr_ivf_search*)"
    g32.free()
    c32.free()

    ld = Loaded(ctx, fx)
    try:
        corpus, gpu = ld.corpus, ld.gpu
        # ---- the float entry points on a bit index, with the right and with a wrong dimension
        for dim in (fx.dim, fx.dim + 1):
            q = np.zeros((4, dim), F32)
            calls = {
                "vsr_ivf_probe": lambda: lib.vsr_ivf_probe(gpu._h, as_ptr(q), 4, dim, 3, 0, as_ptr(lists_out)),
                "vsr_ivf_search": lambda: lib.vsr_ivf_search(gpu._h, as_ptr(q), 4, dim, 10, 3, 0, None, *outs),
                "vsr_ivf_search_device": lambda: lib.vsr_ivf_search_device(gpu._h, as_ptr(q), 4, dim, 10, 3, 0, None, *outs),
                "vsr_ivf_search_iterative": lambda: lib.vsr_ivf_search_iterative(gpu._h, as_ptr(q), 4, dim, 10, 3, 0, None, 1, 9, *outs,
                                                                                 as_ptr(pr)),
                "vsr_ivf_search_iterative_device": lambda: lib.vsr_ivf_search_iterative_device(gpu._h, as_ptr(q), 4, dim, 10, 3, 0, None,
                                                                                               1, 9, *outs, as_ptr(pr)),
            }
            for who, call in calls.items():
                assert call() == UNSUPPORTED, who
                assert last() == f"{who}: the index is over a bit corpus: it is searched with vsr_ivf_search_bit* (<~>)"
        # ---- vsr_ivf_load / vsr_ivf_assign over the bit corpus keep their status and text
        st, msg = refused(corpus.load_ivf, qf[:3], fx.m.assign)
        assert st == UNSUPPORTED and msg == ("vsr_ivf_load: a bit corpus has no index path yet (the bit_hamming_ops / bit_jaccard_ops "
                                             "opclasses)")
        st, msg = refused(corpus.ivf_assign, qf[:3])
        assert st == UNSUPPORTED and msg == ("vsr_ivf_assign: a bit corpus has no index path yet (the bit_hamming_ops / "
                                             "bit_jaccard_ops opclasses)")
        # ---- metrics
        for fn, who in ((gpu.search_bit, "vsr_ivf_search_bit"), (gpu.search_bit_iterative, "vsr_ivf_search_bit_iterative")):
            st, msg = refused(fn, fx.q, 10, 3, "jaccard")
            assert st == UNSUPPORTED and msg == f"{who}: ivfflat has no bit_jaccard_ops operator class"
            st, msg = refused(fn, fx.q, 10, 3, "l2")
            assert st == INVALID and msg == f"{who}: metric 0"
            st, msg = refused(fn, fx.q, 10, 3, 6)
            assert st == INVALID and msg == f"{who}: metric 6"
        # ---- a dimension mismatch: CheckDims' words, the column's length first
        bad = np.zeros((2, (fx.dim + 1 + 7) // 8), np.uint8)
        want = f"different bit lengths {fx.dim} and {fx.dim + 1}"
        for fn, args in ((gpu.search_bit, (bad, 10, 3)), (gpu.search_bit_iterative, (bad, 10, 3)), (gpu.probe_bit, (bad, 3))):
            st, msg = refused(fn, *args, dim=fx.dim + 1)
            assert st == DIM and msg == want, (fn, msg)
        # ---- probes, max_probes, mode, k, NULL: the float entry points' checks
        st, msg = refused(gpu.search_bit, fx.q, 10, 0)
        assert st == INVALID and msg == "vsr_ivf_search_bit: probes must be >= 1 (got 0)"
        st, msg = refused(gpu.probe_bit, fx.q, 0)
        assert st == INVALID and msg == "vsr_ivf_probe_bit: probes must be >= 1 (got 0)"
        st, msg = refused(gpu.search_bit_iterative, fx.q, 10, 3, "hamming", None, "relaxed_order", 0)
        assert st == INVALID and msg == "vsr_ivf_search_bit_iterative: max_probes must be between 1 and 32768 (got 0)"
        st, msg = refused(gpu.search_bit_iterative, fx.q, 10, 3, "hamming", None, "relaxed_order", 32769)
        assert st == INVALID and "max_probes must be between 1 and 32768 (got 32769)" in msg
        st, msg = refused(gpu.search_bit_iterative, fx.q, 10, 3, "hamming", None, 2)
        assert st == INVALID and msg == "vsr_ivf_search_bit_iterative: iterative scan mode 2 (ivfflat has off and relaxed_order)"
        st, msg = refused(gpu.search_bit, fx.q, 0, 3)
        assert st == INVALID and msg == "vsr_ivf_search_bit: k must be >= 1 (got 0)"
        st, msg = refused(gpu.search_bit, fx.q, MAX_K + 1, 3)
        assert st == UNSUPPORTED and msg == f"vsr_ivf_search_bit: k = {MAX_K + 1} exceeds VSR_MAX_K = {MAX_K}"
        assert lib.vsr_ivf_search_bit(None, as_ptr(fx.q), 4, fx.dim, 10, 3, 4, None, *outs) == INVALID
        assert last() == "vsr_ivf_search_bit: index is NULL"
        assert lib.vsr_ivf_search_bit(gpu._h, None, 4, fx.dim, 10, 3, 4, None, *outs) == INVALID
        assert last() == "vsr_ivf_search_bit: queries is NULL"
        assert lib.vsr_ivf_search_bit(gpu._h, as_ptr(fx.q), 4, fx.dim, 10, 3, 4, None, None, *outs[1:]) == INVALID
        assert last() == "vsr_ivf_search_bit: output is NULL"
        assert lib.vsr_ivf_probe_bit(gpu._h, as_ptr(fx.q), 4, fx.dim, 3, None) == INVALID
        assert last() == "vsr_ivf_probe_bit: NULL argument"
        assert lib.vsr_ivf_load_bit(corpus._h, None, fx.lists, as_ptr(zero), ctypes.byref(h)) == INVALID
        assert last() == "vsr_ivf_load_bit: NULL argument"
        assert lib.vsr_ivf_assign_bit(corpus._h, as_ptr(fx.centers), fx.lists, None) == INVALID
        assert last() == "vsr_ivf_assign_bit: NULL argument"
        # ---- lists and list ids
        assert lib.vsr_ivf_load_bit(corpus._h, as_ptr(fx.centers), 0, as_ptr(zero), ctypes.byref(h)) == UNSUPPORTED
        assert last() == "vsr_ivf_load_bit: lists must be between 1 and 32768 (got 0)" and not h.value
        assert lib.vsr_ivf_assign_bit(corpus._h, as_ptr(fx.centers), 32769, as_ptr(zero)) == UNSUPPORTED
        assert last() == "vsr_ivf_assign_bit: lists must be between 1 and 32768 (got 32769)"
        rl = fx.m.assign.copy()
        rl[77] = fx.lists
        st, msg = refused(corpus.load_ivf_bit, fx.centers, rl)
        assert st == INVALID and msg == f"vsr_ivf_load_bit: row 77 has list {fx.lists}"
        rl[77] = -1
        assert refused(corpus.load_ivf_bit, fx.centers, rl)[0] == INVALID
        # ---- k-means: bit lengths 1 .. 64000, lists 1 .. 32768
        assert refused(ctx.ivf_kmeans_bit, np.zeros((4, 8001), np.uint8), 2, 64001)[0] == INVALID
        assert refused(ctx.ivf_kmeans_bit, fx.rows[:50], 0, fx.dim)[0] == INVALID
        assert refused(ctx.ivf_kmeans_bit, fx.rows[:50], 32769, fx.dim)[0] == INVALID
        assert refused(ctx.ivf_kmeans, np.zeros((4, 16001), F32), 2)[0] == INVALID       # the float limit stays at 16000
        # bit strings only
        with pytest.raises(ValueError, match="bit strings"):
            corpus.load_ivf_bit(qf[:3], fx.m.assign)
    finally:
        ld.free()
