"""The screening tiers at their error bounds: corpora built by tests/screening_model.py so that the screen drops a true
top-k row (A) and only the flag test (rerank_body, g from csrc/vsr_bounds.h) can notice.

For every case the model first checks that the input really defeats the screen (A is not among the kp kept rows) and,
for K2g, that the bound before the bf16 constants were re-derived would NOT have flagged it: these are not easy cases.
On the GPU the asynchronous API (vsr_search_device) must then FLAG the queries (negative counts), and vsr_search /
vsr_search_device_exact must return the oracle's rows and fp32 distances bit for bit (every top-k distance here is
exact in fp32, whatever the summation order)."""
import ctypes

import numpy as np
import pytest

import screening_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _ids(n, rows_per_doc=10):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


class _Dev:
    """Device buffers of one search_device call."""

    def __init__(self, q, k):
        import torch
        dev = torch.device("cuda", 0)
        nq = len(q)
        self.q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        self.blk = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.doc = torch.empty((nq, k), dtype=torch.int32, device=dev)
        self.row = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        self.cnt = torch.empty((nq,), dtype=torch.int32, device=dev)

    def args(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return p(self.blk), p(self.doc), p(self.row), p(self.dist), p(self.cnt)


def _search_flagged(ctx, corpus, q, k, metric, filters=None):
    """vsr_search_device (no re-run tier behind it): (counts, flags, kernel name, buffers)."""
    nq = len(q)
    b = _Dev(q, k)
    corpus.search_device(ctypes.c_void_p(b.q.data_ptr()), nq, k, metric, filters, *b.args())
    ctx.synchronize()
    name = ctx.last_scan_kernel()
    _, flags = ctx.screening_check(nq)
    return b.cnt.cpu().numpy(), flags, name, b


def _expect_exact(oracle, rows, dist, cnt, qi, metric, x, q, k, doc, blk, mask=None):
    idx, ref = oracle.filtered_topk(metric, x, q, k, doc, blk, mask)
    assert cnt == idx.size, (qi, cnt, idx.size)
    np.testing.assert_array_equal(rows[:cnt], idx)
    np.testing.assert_array_equal(dist[:cnt], ref.astype(np.float32))


def _corpus_of(build, dim, nq, n_min, seed):
    """nq copies of one adversarial construction, each on its own permutation of the coordinates (query i's rows are far
    from query j's), at random positions among filler rows (1 on the last coordinate when the construction leaves it 0:
    far for every metric; without one, a single copy serves every query).  Returns the corpus, the queries, k, A's row
    per query and query 0's construction."""
    rng = np.random.default_rng(seed)
    X0, q0, k, hidden = build(dim)
    fill = np.zeros(dim, np.float32)
    spare = not (X0[:, dim - 1] != 0).any() and q0[dim - 1] == 0
    if spare:
        fill[dim - 1] = 1
    copies = nq if spare else 1                            # (no free coordinate to permute: every query is q0)
    n = max(n_min, copies * len(X0))
    x = np.repeat(fill[None, :], n, axis=0)
    pos = rng.permutation(n)[: copies * len(X0)].reshape(copies, len(X0))
    q = np.empty((nq, dim), np.float32)
    for i in range(copies):
        perm = np.arange(dim)
        if i:                                              # query 0 keeps the construction as built
            perm[: dim - 1] = rng.permutation(dim - 1)
        x[pos[i]] = X0[:, perm]
        q[i] = q0[perm]
    q[copies:] = q0
    pos = pos[np.minimum(np.arange(nq), copies - 1)]
    return x, q, k, pos[:, hidden], (X0, q0, hidden)


def _self_check(tier, metric, construction, k, defeat_old):
    x, q0, a_row = construction
    kept, flagged_old, _ = sm.screen(tier, metric, x, q0, k, sm.old_g(tier, x.shape[1]))
    assert a_row not in kept, "the construction no longer hides its true neighbour from the screen"
    if defeat_old:
        assert not flagged_old, "the old bound would flag this input: it no longer tests the constant"


@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_k2g_flags_at_the_coarse_bound(ctx, oracle, metric, dim):
    """K2g, 256 queries in one pass: both operands of A . q round down to bf16 (the coarse screen's worst case, 1.99 2^-8
    relative), and at least kp = 128 rows that are exactly worse than A screen better.  The query must be flagged."""
    build = {"l2": sm.coarse_l2, "ip": sm.coarse_ip, "cosine": sm.coarse_cosine}[metric]
    nq = 256
    x, q, k, a_rows, built = _corpus_of(build, dim, nq, 60_000, seed=dim + len(metric))
    _self_check("coarse", metric, built, k, defeat_old=True)
    blk, doc = _ids(len(x))
    corpus = ctx.load_corpus(x, blk, doc)
    cnt, flags, name, b = _search_flagged(ctx, corpus, q, k, metric)
    assert "(K2g" in name, name
    assert (cnt < 0).all(), f"{int((cnt >= 0).sum())} of {nq} queries published past the coarse bound"
    assert np.count_nonzero(flags) == nq
    n_rerun = corpus.search_device_exact(ctypes.c_void_p(b.q.data_ptr()), nq, k, metric, None, *b.args())
    assert n_rerun == nq
    rows, dist, dcnt = b.row.cpu().numpy(), b.dist.cpu().numpy(), b.cnt.cpu().numpy()
    res = corpus.search(q, k, metric)
    for i in range(0, nq, 16):
        assert a_rows[i] in res.rows[i, :k]
        _expect_exact(oracle, rows[i], dist[i], dcnt[i], i, metric, x, q[i], k, doc, blk)
        _expect_exact(oracle, res.rows[i], res.dist[i], res.counts[i], i, metric, x, q[i], k, doc, blk)
    corpus.free()


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_k2w_flags_at_the_plane_bound(ctx, oracle, metric, dim):
    """K2w on hi + mid planes, 64 queries: L2 on the planes' worst-case operands (x = q = 1.0039136: xm qm and both split
    residues add up), IP on 257 = 256 + 1 (the dropped xm qm).  A is screened out; the result must still be exact."""
    build = {"l2": sm.planes_l2, "ip": sm.planes_ip}[metric]
    nq = 64
    x, q, k, a_rows, built = _corpus_of(build, dim, nq, 20_000, seed=dim * 3 + len(metric))
    _self_check("planes", metric, built, k, defeat_old=False)
    blk, doc = _ids(len(x))
    corpus = ctx.load_corpus(x, blk, doc)
    cnt, flags, name, _ = _search_flagged(ctx, corpus, q, k, metric)
    assert "(K2w" in name and "hi+mid" in name, name
    assert (cnt < 0).all() and np.count_nonzero(flags) == nq, int((cnt >= 0).sum())
    res = corpus.search(q, k, metric)
    for i in range(0, nq, 8):
        assert a_rows[i] in res.rows[i, :k]
        _expect_exact(oracle, res.rows[i], res.dist[i], res.counts[i], i, "l2" if metric == "l2" else "ip", x, q[i], k,
                      doc, blk)
    corpus.free()


def _offset_case(ctx, oracle, x, q, k, want, filters=None, masks=None):
    blk, doc = _ids(len(x))
    corpus = ctx.load_corpus(x, blk, doc)
    if filters is not None:
        filters = filters(corpus, doc)
    flt = filters[0] if filters else None
    cnt, flags, name, _ = _search_flagged(ctx, corpus, q, k, "l2", flt)
    assert want in name, name
    assert np.count_nonzero(flags) > 0 and (flags != 0).sum() == (cnt < 0).sum()
    res = corpus.search(q, k, "l2", flt)
    for i in range(len(q)):
        _expect_exact(oracle, res.rows[i], res.dist[i], res.counts[i], i, "l2", x, q[i], k, doc, blk,
                      None if masks is None else masks[i])
    corpus.free()


def test_offset_rows_on_k2w_with_rbac(ctx, oracle):
    """Rows 4096 + r (r = 0..15): exact differences, |x|^2 ~ 2^31 cancels in the screen, values neither bf16-exact nor
    u8.  K2w with role pre-filters; every answer bit-exact, and the screen flags what it cannot prove."""
    import vsrbac
    from vsrbac.datasets import tree_rbac
    rng = np.random.default_rng(7)
    n, dim, nq, k = 20_000, 128, 48, 10
    x = sm.offset_rows(rng, n, dim, 4096)
    q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    rbac = tree_rbac(num_users=50, num_roles=20, num_docs=n // 10, seed=3)
    users = rng.integers(1, 51, nq)
    masks = [None] * nq

    def filters(corpus, doc):
        corpus.load_rbac(rbac.user_roles, rbac.permissions)
        for i, u in enumerate(users):
            masks[i] = oracle.user_row_mask(int(u), rbac.user_roles, rbac.permissions, doc)
        return [[corpus.filter_for_user(int(u), vsrbac.RANGES) for u in users]]

    _offset_case(ctx, oracle, x, q, k, "(K2w", filters, masks)


@pytest.mark.parametrize("dim,base,no_wide", [(128, 4096, True), (1536, 2 ** 17, False)])
def test_offset_rows_on_k2(oracle, monkeypatch, dim, base, no_wide):
    """K2 (fp32 MFMA) on rows base + r: 128-d with the wide kernels switched off, and 1536-d rows (longer than K2w takes)
    at 2^17 + r, where |x|^2 ~ 2^44 leaves the screen no usable digit of the differences."""
    import vsrbac
    if no_wide:
        monkeypatch.setenv("VSR_NO_WIDE", "1")
    c = vsrbac.Context(0)
    if no_wide:
        monkeypatch.delenv("VSR_NO_WIDE")
    try:
        rng = np.random.default_rng(dim)
        n, nq, k = (20_000 if dim <= 256 else 8_000), 40, 10
        x = sm.offset_rows(rng, n, dim, base)
        q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
        _, flagged, _ = sm.screen("k2", "l2", x, q[0], k, sm.old_g("k2", dim))
        assert flagged, "K2's bound must flag rows this far inside the screen's rounding"
        _offset_case(c, oracle, x, q, k, "(K2)")
    finally:
        c.close()
