"""K2hw (csrc/vsr_mfmahw.h): workgroup-shared f16 MFMA passes over a halfvec corpus, switched on by Context.set_half_wide.

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
    c.set_half_wide(True)
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


# dim: one chunk (below K2h's own gate of 61 elements: K1h), a short stage, exactly one stage, a stage plus a chunk, the register
# limit, the first LDS-query width, long rows.  rows of the part: the tile edge and several tiles.  nq queries share the part:
# one / two / three / four 16-query groups with their row splits, and a second pass.  k = 100: keep = 200 exceeds the part.
CASES = [(8, 300, 17, "l2", "none", 10), (120, 63, 16, "l2", "ranges", 10), (128, 64, 17, "ip", "bitmap", 1),
         (136, 65, 33, "cosine", "none", 10), (256, 300, 48, "l2", "bitmap", 10), (264, 300, 64, "ip", "ranges", 10),
         (776, 300, 65, "cosine", "bitmap", 1), (128, 300, 65, "l2", "none", 10), (264, 65, 16, "l2", "none", 1),
         (776, 63, 33, "ip", "ranges", 10), (256, 64, 64, "cosine", "ranges", 100), (136, 300, 48, "ip", "none", 100)]


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
    assert ("(K2hw, f16 rows)" in name and f"NSTR={1 if dim <= 128 else 2 if dim <= 256 else 0}" in name) if dim >= 61 else "K1h" in name, name
    for i in range(nq):
        _exact(oracle, res, i, metric, x, q[i], k, doc, blk, masks[i])
    corpus.free()


def test_switch_and_kernel_names(oracle, monkeypatch):
    """Off by default (K2h); on by the call and by VSR_HALF_WIDE=1 at open (K2hw); L1 with the switch on stays on K1h."""
    import vsrbac
    rng = np.random.default_rng(2)
    x, q = _ints(rng, (2000, 128)), _ints(rng, (20, 128))
    for env, call, want in ((None, False, "K2h,"), (None, True, "K2hw"), ("1", False, "K2hw")):
        if env:
            monkeypatch.setenv("VSR_HALF_WIDE", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_HALF_WIDE", raising=False)
        if call:
            c.set_half_wide(True)
        corpus = c.load_corpus_half(x.astype(np.float16))
        for metric, kernel in (("l2", want), ("l1", "K1h")):
            res = corpus.search(q, 10, metric)
            assert kernel in c.last_scan_kernel(), c.last_scan_kernel()
            for i in range(0, 20, 7):
                _exact(oracle, res, i, metric, x, q[i], 10)
        corpus.free()
        c.close()


def test_duplicate_rows_across_the_keep_boundary(ctx, oracle):
    """3000 rows, 40 distinct vectors: every distance occurs ~75 times, so keep = 32 cuts through a run of equal screening keys
    and (document_id, block_id) decide, against a shuffled caller order."""
    rng = np.random.default_rng(3)
    n, dim, nq, k = 3000, 128, 33, 10
    x = _ints(rng, (40, dim))[rng.integers(0, 40, n)]
    q = _ints(rng, (nq, dim))
    blk, doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 41, n).astype(np.int32)
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    for metric in ("l2", "ip"):
        res = corpus.search(q, k, metric)                         # (a query the ties flag is re-run on K1h: the last kernel named)
        for i in range(nq):
            _exact(oracle, res, i, metric, x, q[i], k, doc, blk)
    corpus.free()


@pytest.mark.parametrize("probes", [3, 12])
def test_half_ivfflat_lists_equal_the_narrow_kernel(ctx, probes):
    """The list scans of a half IVFFlat index (a list-ordered view: keys go through the rank map) with the switch on return
    what they return with it off, a few probes and every list."""
    rng = np.random.default_rng(4)
    n, dim, lists, nq, k = 6000, 128, 12, 40, 10
    x = _ints(rng, (n, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    index = corpus.load_ivf_half(x[:lists].astype(np.float16), (np.arange(n) % lists).astype(np.int32))
    q = _ints(rng, (nq, dim))
    got = {}
    for on in (False, True):
        ctx.set_half_wide(on)
        res = index.search(q, k, probes, "l2")
        assert ("K2hw" if on else "K2h,") in ctx.last_scan_kernel(), ctx.last_scan_kernel()
        got[on] = (res.rows.copy(), res.dist.copy(), res.counts.copy())
    for a, b in zip(got[True], got[False]):
        np.testing.assert_array_equal(a, b)
    assert (got[True][2] == k).all()
    corpus.free()


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_real_valued(ctx, oracle, metric):
    """Gaussian rows under a 50 % mask, queries near rows: within the project's 1e-4 of the float64 distances, nothing better
    left out (near ties may swap), and the oracle's distances."""
    rng = np.random.default_rng(5)
    n, dim, nq, k, tol = 1500, 264, 33, 20, 1e-4
    h = rng.normal(size=(n, dim)).astype(np.float16)
    x = h.astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    q = (x[rng.integers(10, n, nq)] + 0.01 * rng.normal(size=(nq, dim))).astype(np.float16).astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    res = corpus.search(q, k, metric, corpus.filter_from_bytemask(mask))
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
