"""K2gh (csrc/vsr_gemmh.h): 256-query f16 GEMM passes over the long rows of a halfvec corpus, switched on by
Context.set_half_gemm.

The expected answer is the CPU oracle's exact filtered top-k over the widened rows and the binary16-rounded query.  Integer
data (-5 .. 11, asymmetric, exact in binary16, every sum exact in fp32): row ids, fp32 distances and counts bit for bit.
Reported rows and distances never come from the screen: they are the re-rank's or, for a flagged query, K1h's."""
import numpy as np
import pytest

from helpers import assert_valid_topk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    c.set_half_gemm(True)
    yield c
    c.close()


def _ints(rng, shape):
    return rng.integers(-5, 12, shape).astype(np.float32)


def _exact(oracle, res, i, metric, x, q, k, doc=None, blk=None, mask=None):
    idx, dist = oracle.filtered_topk(metric, x, q, k, doc, blk, mask)
    m = res.counts[i]
    assert m == idx.size, (i, m, idx.size)
    np.testing.assert_array_equal(res.rows[i, :m], idx)
    np.testing.assert_array_equal(res.dist[i, :m].view(np.uint32), dist.astype(np.float32).view(np.uint32))


# dim: 225 = 29 chunks is the smallest admitted (8 K-steps of 4 chunks), 224 stays off K2gh; 256 / 512 are whole K-steps; 264 /
# 776 a K-step plus one chunk and 257 / 769 plus one element (three of the last K-step's four chunks are the clamped tail; mode
# none: the part is the corpus, so its last row is the allocation's); 232 a whole chunk count inside a K-step.  part: the
# 256-row tile's edge, several tiles with a ragged last one.  nq: just over the gate of 128 (127 pad columns), a full pass,
# two passes.  k = 100: keep = 200 exceeds the 150-row part.
CASES = [(225, 256, 129, "l2", "none", 10), (224, 300, 129, "l2", "none", 10), (256, 255, 256, "ip", "ranges", 10),
         (512, 257, 257, "cosine", "bitmap", 1), (264, 700, 300, "l2", "none", 10), (776, 257, 129, "ip", "none", 1),
         (257, 255, 130, "cosine", "none", 10), (769, 256, 129, "l2", "bitmap", 10), (264, 150, 129, "cosine", "ranges", 100),
         (776, 700, 257, "l2", "none", 100), (232, 257, 300, "ip", "bitmap", 10)]


@pytest.mark.parametrize("dim,part,nq,metric,mode,k", CASES)
def test_shapes_exact(ctx, oracle, dim, part, nq, metric, mode, k):
    """`nq` queries share one filter part of `part` rows; under a filter one more query, alone on a second part of 200 rows, is
    a one-query pass of the same launch.  ranges: a role pre-filter (tile lists whose first tile starts inside a tile);
    bitmap: the same role as an RLS bitmap over scattered rows."""
    import vsrbac
    rng = np.random.default_rng(dim + part + nq)
    n = part if mode == "none" else 700
    x = _ints(rng, (n, dim))
    blk, doc = (np.arange(n) + 1).astype(np.int64), (np.arange(n) + 1).astype(np.int32)       # one row per document
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    filters, masks = None, [None] * nq
    if mode != "none":
        mine = np.arange(5, 5 + part) if mode == "ranges" else np.sort(rng.permutation(390)[:part])
        ur, perms = [(1, 1), (2, 2)], [(1, int(d) + 1) for d in mine] + [(2, d + 1) for d in range(400, 600)]
        corpus.load_rbac(ur, perms)
        fm = vsrbac.RANGES if mode == "ranges" else vsrbac.BITMAP
        nq += 1
        filters = [corpus.filter_for_user(1, fm)] * (nq - 1) + [corpus.filter_for_user(2, fm)]
        masks = [oracle.user_row_mask(u, ur, perms, doc) for u in [1] * (nq - 1) + [2]]
        assert masks[0].sum() == part
    q = _ints(rng, (nq, dim))
    res = corpus.search(q, k, metric, filters)
    name = ctx.last_scan_kernel()
    assert ("(K2gh, f16 rows)" in name) == (dim >= 225), name
    for i in range(nq):
        _exact(oracle, res, i, metric, x, q[i], k, doc, blk, masks[i])
    corpus.free()


def test_switch_and_kernel_names(oracle, monkeypatch):
    """Off by default (K2h); on by the call and by VSR_HALF_GEMM=1 at open (K2gh).  With the switch on, L1 stays on K1h and a
    20-query call (below the gate) and the list scans of a half IVFFlat index (a view) on K2h."""
    import vsrbac
    rng = np.random.default_rng(2)
    n, dim, nq = 2000, 256, 150
    x, q = _ints(rng, (n, dim)), _ints(rng, (nq, dim))
    for env, call, want in ((None, False, "K2h,"), (None, True, "K2gh"), ("1", False, "K2gh")):
        if env:
            monkeypatch.setenv("VSR_HALF_GEMM", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_HALF_GEMM", raising=False)
        if call:
            c.set_half_gemm(True)
        corpus = c.load_corpus_half(x.astype(np.float16))
        for metric, queries, kernel in (("l2", q, want), ("l1", q, "K1h"), ("l2", q[:20], "K2h,")):
            res = corpus.search(queries, 10, metric)
            assert kernel in c.last_scan_kernel(), c.last_scan_kernel()
            for i in range(0, len(queries), 19):
                _exact(oracle, res, i, metric, x, queries[i], 10)
        if want == "K2gh":
            index = corpus.load_ivf_half(x[:4].astype(np.float16), (np.arange(n) % 4).astype(np.int32))
            res = index.search(q, 10, 4, "l2")
            assert "K2h," in c.last_scan_kernel(), c.last_scan_kernel()
            assert (res.counts == 10).all()
        corpus.free()
        c.close()


def test_duplicate_rows_across_the_keep_boundary(ctx, oracle):
    """3000 rows, 40 distinct vectors: every distance occurs ~75 times, so keep = 32 cuts through a run of equal screening keys
    and (document_id, block_id) decide, against a shuffled caller order."""
    rng = np.random.default_rng(3)
    n, dim, nq, k = 3000, 264, 150, 10
    x = _ints(rng, (40, dim))[rng.integers(0, 40, n)]
    q = _ints(rng, (nq, dim))
    blk, doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 41, n).astype(np.int32)
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    for metric in ("l2", "ip"):
        res = corpus.search(q, k, metric)                         # (a query the ties flag is re-run on K1h: the last kernel named)
        for i in range(nq):
            _exact(oracle, res, i, metric, x, q[i], k, doc, blk)
    corpus.free()


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_seeded_main_pass_exact(ctx, oracle, metric):
    """A corpus large enough for the sample pass to seed every query: the main pass runs with thresholds folded into the
    accumulators (the small cases above run with open thresholds).  Two passes of 136 columns, a clamped tail chunk."""
    rng = np.random.default_rng(6)
    n, dim, nq, k = 40000, 264, 260, 10
    x, q = _ints(rng, (n, dim)), _ints(rng, (nq, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    res = corpus.search(q, k, metric)
    assert "(K2gh, f16 rows)" in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    for i in range(0, nq, 7):
        _exact(oracle, res, i, metric, x, q[i], k)
    corpus.free()


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_real_valued(ctx, oracle, metric):
    """Gaussian rows at a non-K-step width under a 50 % mask, queries near rows: within the project's 1e-4 of the float64
    distances, nothing better left out (near ties may swap), and the oracle's distances."""
    rng = np.random.default_rng(5)
    n, dim, nq, k, tol = 1500, 264, 150, 20, 1e-4
    h = rng.normal(size=(n, dim)).astype(np.float16)
    x = h.astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    q = (x[rng.integers(10, n, nq)] + 0.01 * rng.normal(size=(nq, dim))).astype(np.float16).astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    res = corpus.search(q, k, metric, corpus.filter_from_bytemask(mask))
    assert "(K2gh, f16 rows)" in ctx.last_scan_kernel() or "K1h" in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    x64 = x.astype(np.float64)
    for i in range(nq):
        q64 = q[i].astype(np.float64)
        ref = {"l2": np.sqrt(((x64 - q64) ** 2).sum(1)), "ip": -(x64 @ q64),
               "cosine": 1.0 - (x64 @ q64) / np.sqrt((x64 ** 2).sum(1) * (q64 ** 2).sum())}[metric]
        assert res.counts[i] == k
        assert_valid_topk(res.rows[i, :k], res.dist[i, :k], ref, k, tol, candidates=np.flatnonzero(mask))
        _, odist = oracle.filtered_topk(metric, x, q[i], k, mask=mask)
        np.testing.assert_allclose(res.dist[i, :k], odist, rtol=tol, atol=tol)
    corpus.free()
