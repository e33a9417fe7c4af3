"""GPU index paths against the index oracle (oracle/vsr_index_oracle.c = pgvector's IVFFlat / HNSW restated).

K3 (IVFFlat list probe): given the oracle's centres and list assignment, the GPU must probe exactly the oracle's lists
(GetScanLists, ivfscan.c:36-107) and return exactly the oracle's rows for probes in {1, 5, lists}, unfiltered and under
RBAC filters (the executor's filter above the index scan).  Integer-valued rows: fp32 sums are exact, so ids and
distances are compared bit for bit."""
import numpy as np
import pytest

from helpers import check_built_graph
from oracle.oracle import HnswIndex as OracleHnsw
from oracle.oracle import IvfIndex as OracleIvf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sift60k(oracle):
    rng = np.random.default_rng(61)
    n, dim = 60_000, 128
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    ivf = OracleIvf(oracle, "l2", x, lists=50, seed=9)
    return x, blk, doc, ivf


@pytest.mark.parametrize("nq", [3, 40])
def test_ivf_probe_and_search_match_the_oracle(ctx, oracle, sift60k, nq):
    import vsrbac
    x, blk, doc, oivf = sift60k
    n = len(x)
    rng = np.random.default_rng(62 + nq)
    corpus = ctx.load_corpus(x, blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 3, replace=False)] + \
            [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 10, replace=False)]
    ur = [(u, 1 + u % 2) for u in range(1, 7)] + [(6, 1)]
    corpus.load_rbac(ur, perms)
    gpu = corpus.load_ivf(oivf.centers, oivf.assign)
    q = x[rng.integers(0, n, nq)] + rng.integers(-2, 3, (nq, x.shape[1])).astype(np.float32)
    users = rng.integers(1, 7, nq)
    masks = [oracle.user_row_mask(int(u), ur, perms, doc) for u in users]
    for probes in (1, 5, 50):
        got_lists = gpu.probe(q, probes)
        for i in range(nq):
            assert got_lists[i].tolist() == oivf.probe(q[i], probes).tolist(), (probes, i)
        for kind in ("none", "ranges", "bitmap"):
            if kind == "none":
                filters, ms = None, [None] * nq
            else:
                mode = vsrbac.RANGES if kind == "ranges" else vsrbac.BITMAP
                filters, ms = [corpus.filter_for_user(int(u), mode) for u in users], masks
            res = gpu.search(q, 100, probes, "l2", filters)
            for i in range(0, nq, max(1, nq // 8)):
                idx, dist = oivf.search(q[i], 100, probes, doc, blk, ms[i])
                m = res.counts[i]
                assert m == idx.size, (probes, kind, i, m, idx.size)
                np.testing.assert_array_equal(res.rows[i, :m], idx)
                np.testing.assert_array_equal(res.dist[i, :m], dist.astype(np.float32))
                assert (res.block_ids[i, m:] == -1).all()
    # probes = lists is the exact scan of the corpus
    full = corpus.search(q, 100, "l2")
    np.testing.assert_array_equal(gpu.search(q, 100, 50, "l2").rows, full.rows)
    gpu.free()
    corpus.free()


def test_ivf_build_assignment_on_the_gpu(ctx, oracle, sift60k):
    """Index build, the pass over every row (ivfbuild.c:404-445): the GPU assigns all rows to their nearest centre
    exactly as the index oracle does (same arithmetic, ties to the lower list), in the caller's row order even when the
    corpus is stored in another order; an index loaded from that assignment answers like one loaded from the oracle's."""
    x, blk, doc, oivf = sift60k
    rng = np.random.default_rng(91)
    perm = rng.permutation(len(x))                       # caller order != (document, block) order
    corpus = ctx.load_corpus(x[perm], blk[perm], doc[perm])
    got = corpus.ivf_assign(oivf.centers, "l2")
    np.testing.assert_array_equal(got, oivf.assign[perm])
    gpu = corpus.load_ivf(oivf.centers, got)
    q = x[rng.integers(0, len(x), 8)]
    res = gpu.search(q, 20, 3, "l2")
    for i in range(8):
        idx, dist = oivf.search(q[i], 20, 3)
        np.testing.assert_array_equal(res.block_ids[i], blk[idx])
        np.testing.assert_array_equal(res.dist[i], dist.astype(np.float32))
    gpu.free()
    corpus.free()


def test_ivf_device_search_and_more_than_8192_lists(ctx, oracle):
    """vsr_ivf_search_device (queries and results resident; only the probed list ids cross PCIe) returns what the host
    form returns, and the probe kernel takes the reloption's upper range (lists up to 32768, ivfflat.h:42-44: 9000 lists
    here, beyond the 8192 the 64-bit LDS keys of round 2 allowed)."""
    import torch
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
    np.testing.assert_array_equal(corpus.ivf_assign(centers, "l2"), oivf.assign)
    gpu = corpus.load_ivf(centers, oivf.assign)
    nq, k, probes = 12, 10, 40
    q = x[rng.integers(0, n, nq)] + rng.integers(-1, 2, (nq, dim)).astype(np.float32)
    got_lists = gpu.probe(q, probes)
    for i in range(nq):
        assert got_lists[i].tolist() == oivf.probe(q[i], probes).tolist(), i
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
        idx, dist = oivf.search(q[i], k, probes, doc, blk, mask)
        m = host.counts[i]
        assert m == idx.size
        np.testing.assert_array_equal(host.rows[i, :m], idx)
        np.testing.assert_array_equal(host.dist[i, :m], dist.astype(np.float32))
    gpu.free()
    corpus.free()


def test_ivf_cosine_opclass_on_unit_rows(ctx, oracle):
    """vector_cosine_ops: spherical k-means centres, probe by negative inner product, rows are unit vectors."""
    rng = np.random.default_rng(71)
    n, dim = 30_000, 96
    x = rng.normal(size=(n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    oivf = OracleIvf(oracle, "cosine", x, lists=30, seed=2)
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_ivf(oivf.centers, oivf.assign)
    q = x[rng.integers(0, n, 20)] + 0.05 * rng.normal(size=(20, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    got_lists = gpu.probe(q, 4, "cosine")
    res = gpu.search(q, 50, 4, "cosine")
    agree = 0
    for i in range(20):
        want_lists = oivf.probe(q[i], 4)
        agree += got_lists[i].tolist() == want_lists.tolist()
        if got_lists[i].tolist() != want_lists.tolist():
            continue                                  # a centre-distance near-tie resolved the other way: different lists
        idx, dist = oivf.search(q[i], 50, 4)
        assert len(set(res.rows[i].tolist()) & set(idx.tolist())) >= 49
        np.testing.assert_allclose(res.dist[i], dist, rtol=1e-4, atol=1e-4)
    assert agree >= 19
    gpu.free()
    corpus.free()


# ---------------------------------------------------------------------------------------------
# K4: HNSW layer search.  Same graph (exported from the oracle's pgvector-faithful build) => the GPU search returns the
# rows the oracle's GetScanItems returns, in the same order, and visits the same number of elements, for
# ef_search in {10, 40, 500}; recall@k against the exact scan is reported by the same test.
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hnsw20k(oracle):
    rng = np.random.default_rng(81)
    n, dim = 20_000, 128
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    x[5000:5040] = x[100]                              # 41 copies of one vector: elements with 10 heap TIDs each
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    h = OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=4)
    return x, blk, doc, h


@pytest.mark.parametrize("ef", [10, 40, 500])
def test_hnsw_search_matches_the_oracle(ctx, oracle, hnsw20k, ef):
    import vsrbac
    x, blk, doc, oh = hnsw20k
    n = len(x)
    rng = np.random.default_rng(82 + ef)
    corpus = ctx.load_corpus(x, blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 4, replace=False)]
    ur = [(1, 1)]
    corpus.load_rbac(ur, perms)
    gpu = corpus.load_hnsw(oh.export())
    nq, k = 24, min(ef, 100)
    qrows = rng.integers(0, n, nq)
    qrows[0] = 100                                     # the duplicated vector
    q = x[qrows] + rng.integers(-2, 3, (nq, x.shape[1])).astype(np.float32)
    q[0] = x[100]
    res, vis = gpu.search(q, k, ef, "l2")
    hits = total = 0
    for i in range(nq):
        rows_o, dist_o, _, nv = oh.search(q[i], ef)
        m = min(k, rows_o.size)
        assert res.counts[i] == m, (i, res.counts[i], m)
        np.testing.assert_array_equal(res.rows[i, :m], rows_o[:m])
        np.testing.assert_array_equal(res.dist[i, :m], np.sqrt(dist_o[:m]).astype(np.float32))
        assert vis[i] == nv, (i, vis[i], nv)
        exact, _ = oracle.filtered_topk("l2", x, q[i], k, doc, blk)
        hits += len(set(res.rows[i, :m].tolist()) & set(exact.tolist()))
        total += k
    print(f"hnsw ef_search={ef}: recall@{k} vs the exact scan = {hits / total:.3f}")
    if ef >= 40:
        assert hits / total >= 0.5                     # i.i.d. synthetic rows have no cluster structure; real SIFT is far higher
    if ef == 500:                                      # the beam is wide enough to reach the planted duplicates: the 10 heap
        assert (res.dist[0, :10] == 0).all()           # TIDs of one element come out together, newest first
        assert (np.diff(res.rows[0, :10]) < 0).all()
    # RLS semantics: the permission test is applied to the index's candidates, so fewer than k rows may come back
    f = corpus.filter_for_user(1, vsrbac.BITMAP)
    fr = corpus.filter_for_user(1, vsrbac.RANGES)
    mask = oracle.user_row_mask(1, ur, perms, doc)
    for flt in (f, fr):
        resf, _ = gpu.search(q, k, ef, "l2", [flt] * nq)
        for i in range(nq):
            rows_o, dist_o, _, _ = oh.search(q[i], ef)
            keep = rows_o[mask[rows_o] != 0][:k]
            assert resf.counts[i] == keep.size
            np.testing.assert_array_equal(resf.rows[i, :keep.size], keep)
            assert (resf.block_ids[i, keep.size:] == -1).all()
    gpu.free()
    corpus.free()


@pytest.mark.parametrize("share", [0.05, 0.25])
def test_hnsw_predicate_aware_walk(ctx, oracle, hnsw20k, share):
    """vsr_hnsw_set_predicate_aware: the layer-0 walk applies the permission bitmap itself (ACORN-1 style two-hop expansion;
    BASELINE config 5's "predicate-aware HNSW + RBAC").  ACORN's source is not part of the reference tree (PARITY UNPINNED
    against it): the walk is pinned against the index oracle's restatement (same rows, distances and marked-element counts
    on the same graph) and, by recall, against the exact filtered scan -- where it beats the plain graph + result filter at
    the same ef_search by a wide margin when few rows are permitted.  Unfiltered queries are searched as before."""
    import vsrbac
    x, blk, doc, oh = hnsw20k
    n = len(x)
    rng = np.random.default_rng(int(share * 1000))
    corpus = ctx.load_corpus(x, blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), max(1, int(ndocs * share)), replace=False)]
    ur = [(1, 1)]
    corpus.load_rbac(ur, perms)
    mask = oracle.user_row_mask(1, ur, perms, doc)
    gpu = corpus.load_hnsw(oh.export())
    nq, k = 16, 20
    q = x[rng.integers(0, n, nq)] + rng.integers(-2, 3, (nq, x.shape[1])).astype(np.float32)
    for ef in (20, 100):
        recalls = {}
        for aware in (False, True):
            gpu.set_predicate_aware(aware)
            for flt in (corpus.filter_for_user(1, vsrbac.BITMAP), corpus.filter_for_user(1, vsrbac.RANGES)):
                res, vis = gpu.search(q, k, ef, "l2", [flt] * nq)
                hits = 0
                for i in range(nq):
                    rows_o, dist_o, _, nv = oh.search_predicate_aware(q[i], ef, mask) if aware else oh.search(q[i], ef)
                    keep = mask[rows_o] != 0
                    want, wd = rows_o[keep][:k], dist_o[keep][:k]
                    assert res.counts[i] == want.size, (aware, ef, i, res.counts[i], want.size)
                    np.testing.assert_array_equal(res.rows[i, :want.size], want)
                    np.testing.assert_array_equal(res.dist[i, :want.size], np.sqrt(wd).astype(np.float32))
                    assert vis[i] == nv, (aware, ef, i, vis[i], nv)
                    exact, _ = oracle.filtered_topk("l2", x, q[i], k, doc, blk, mask)
                    hits += len(set(res.rows[i, :want.size].tolist()) & set(exact.tolist()))
                recalls[aware] = hits / (nq * k)
            res0, vis0 = gpu.search(q, k, ef, "l2")                       # no filter: the same walk either way
            for i in range(nq):
                rows_o, _, _, nv = oh.search(q[i], ef)
                np.testing.assert_array_equal(res0.rows[i, :min(k, rows_o.size)], rows_o[:k])
                assert vis0[i] == nv
        print(f"hnsw share={share} ef={ef}: recall@{k} plain+filter {recalls[False]:.3f}, predicate-aware {recalls[True]:.3f}")
        assert recalls[True] >= recalls[False]
        if ef == 100:
            assert recalls[True] >= 0.6, recalls
    gpu.set_predicate_aware(False)
    gpu.free()
    corpus.free()


def test_index_caches_forget_freed_filters(ctx, oracle, hnsw20k):
    """The index-side caches (IVFFlat view-order bitmaps and probe parts, HNSW row bitmaps) are keyed by the filter's
    never-reused id and purged when the filter dies: a filter created after another one was freed -- typically at the
    SAME address -- or after a second vsr_rbac_load must never inherit the dead filter's permissions."""
    import vsrbac
    x, blk, doc, oh = hnsw20k
    n = len(x)
    rng = np.random.default_rng(97)
    corpus = ctx.load_corpus(x, blk, doc)
    oivf = OracleIvf(oracle, "l2", x, lists=20, seed=5)
    ivf = corpus.load_ivf(oivf.centers, oivf.assign)
    hnsw = corpus.load_hnsw(oh.export())
    ndocs = int(doc.max())
    q = x[rng.integers(0, n, 12)]
    docs_a = np.arange(1, ndocs // 2 + 1, dtype=np.int32)
    docs_b = np.arange(ndocs // 2 + 1, ndocs + 1, dtype=np.int32)

    def check(flt, allowed_docs):
        allowed = set(int(d) for d in allowed_docs)
        r1 = ivf.search(q, 50, 20, "l2", [flt] * len(q))                  # probes = lists: the exact filtered scan
        r2, _ = hnsw.search(q, 50, 200, "l2", [flt] * len(q))
        mask = np.isin(doc, np.asarray(sorted(allowed), dtype=np.int32)).astype(np.uint8)
        for i in range(len(q)):
            for r in (r1, r2):
                got = r.doc_ids[i, :r.counts[i]]
                assert set(got.tolist()) <= allowed, (i, sorted(set(got.tolist()) - allowed)[:5])
            idx, dist = oracle.filtered_topk("l2", x, q[i], 50, doc, blk, mask)
            np.testing.assert_array_equal(r1.rows[i, :r1.counts[i]], idx)
            rows_o, _, _, _ = oh.search(q[i], 200)
            keep = rows_o[mask[rows_o] != 0][:50]
            np.testing.assert_array_equal(r2.rows[i, :r2.counts[i]], keep)

    for _ in range(3):                                                     # free, re-create: the allocator hands the address back
        fa = corpus.filter_from_documents(docs_a)
        check(fa, docs_a)
        fa.free()
        fb = corpus.filter_from_documents(docs_b)
        check(fb, docs_b)
        fb.free()
    ma = np.isin(doc, docs_a).astype(np.uint8)
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        fa = corpus.filter_from_bytemask(ma, mode)
        check(fa, docs_a)
        fa.free()
        fb = corpus.filter_from_bytemask(1 - ma, mode)
        check(fb, docs_b)
        fb.free()
    # role filters are cached by the corpus and deleted by the next vsr_rbac_load
    for docs_now in (docs_a, docs_b, docs_a):
        corpus.load_rbac([(1, 1)], [(1, int(d)) for d in docs_now])
        for mode in (vsrbac.RANGES, vsrbac.BITMAP):
            check(corpus.filter_for_user(1, mode), docs_now)
    hnsw.free()
    ivf.free()
    corpus.free()


def test_hnsw_limits_device_api_and_visited_forms(ctx, oracle, monkeypatch):
    """pgvector's parameter ranges (m up to 100: neighbour lists longer than a wave; ef_search up to 5000), the device API
    (one launch, no synchronisation, same answers), and the three forms of the visited set: the LDS bitmap (default on a
    small graph), the LDS hash table (forced), its overflow -> global-bitmap re-run (forced with a tiny table)."""
    import ctypes
    import torch
    rng = np.random.default_rng(123)
    n, dim = 6000, 64
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    oh = OracleHnsw(oracle, "l2", x, m=40, ef_construction=64, seed=11)     # 2m = 80 neighbours on layer 0
    corpus = ctx.load_corpus(x, blk, doc)
    gpu = corpus.load_hnsw(oh.export())
    nq = 16
    q = x[rng.integers(0, n, nq)] + rng.integers(-2, 3, (nq, dim)).astype(np.float32)

    def check(ef, k):
        res, vis = gpu.search(q, k, ef, "l2")
        for i in range(nq):
            rows_o, dist_o, _, nv = oh.search(q[i], ef)
            m = min(k, rows_o.size)
            assert res.counts[i] == m, (ef, i, res.counts[i], m)
            np.testing.assert_array_equal(res.rows[i, :m], rows_o[:m])
            np.testing.assert_array_equal(res.dist[i, :m], np.sqrt(dist_o[:m]).astype(np.float32))
            assert vis[i] == nv, (ef, i, vis[i], nv)
        return res

    base = check(40, 40)
    check(2000, 100)
    check(5000, 100)                                                    # HNSW_MAX_EF_SEARCH: the whole graph is the beam
    with pytest.raises(Exception):
        gpu.search(q, 10, 5001, "l2")
    # device API
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    d_q = torch.from_numpy(q).to(dev)
    o = {"blk": torch.empty((nq, 40), dtype=torch.int64, device=dev), "doc": torch.empty((nq, 40), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, 40), dtype=torch.int64, device=dev), "dist": torch.empty((nq, 40), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.empty((nq,), dtype=torch.int64, device=dev)}
    gpu.search_device(p(d_q), nq, 40, 40, "l2", None, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    ctx.synchronize()
    np.testing.assert_array_equal(o["row"].cpu().numpy(), base.rows)
    np.testing.assert_array_equal(o["dist"].cpu().numpy(), base.dist)
    np.testing.assert_array_equal(o["cnt"].cpu().numpy(), base.counts)
    # visited forms
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:8192")
    check(40, 40)
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:256")                 # overflows for every query: global-bitmap re-run
    check(40, 40)
    gpu.search_device(p(d_q), nq, 40, 40, "l2", None, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    ctx.synchronize()
    assert (o["cnt"].cpu().numpy() == -1).all()                         # the device API reports, it cannot re-run
    monkeypatch.setenv("VSR_HNSW_VISITED", "global")
    check(40, 40)
    monkeypatch.delenv("VSR_HNSW_VISITED")
    # the predicate-aware walk on this graph: neighbour lists of 80 (two 64-lane steps per list), few rows permitted (the
    # two-hop expansion runs into its 256-candidate cap), under every form of the visited set
    import vsrbac
    allowed = (rng.random(n) < 0.08).astype(np.uint8)
    flt = corpus.filter_from_bytemask(allowed, vsrbac.BITMAP)
    gpu.set_predicate_aware(True)

    def check_pa(ef, k):
        res, vis = gpu.search(q, k, ef, "l2", [flt] * nq)
        for i in range(nq):
            rows_o, dist_o, _, nv = oh.search_predicate_aware(q[i], ef, allowed)
            keep = allowed[rows_o] != 0
            want, wd = rows_o[keep][:k], dist_o[keep][:k]
            assert res.counts[i] == want.size, (ef, i, res.counts[i], want.size)
            np.testing.assert_array_equal(res.rows[i, :want.size], want)
            np.testing.assert_array_equal(res.dist[i, :want.size], np.sqrt(wd).astype(np.float32))
            assert vis[i] == nv, (ef, i, vis[i], nv)

    check_pa(40, 40)
    check_pa(600, 100)
    for form in ("hash:8192", "hash:256", "global"):
        monkeypatch.setenv("VSR_HNSW_VISITED", form)
        check_pa(40, 40)
    monkeypatch.delenv("VSR_HNSW_VISITED")
    gpu.set_predicate_aware(False)
    gpu.free()
    corpus.free()


@pytest.mark.parametrize("lists,n", [(50, 60_000), (7, 3_000)])
def test_ivf_kmeans_on_the_gpu_equals_the_oracle(ctx, oracle, sift60k, lists, n):
    """vsr_ivf_kmeans (k-means++ + Elkan, ivfkmeans.c) against orc_ivf_kmeans: the same seed and samples give the same
    centres BIT FOR BIT (L2 opclass, integer-valued rows: every float sum is exact and the random stream, the bound tests
    and the centre order are the reference's); the whole build (kmeans -> assign -> load) then answers like an index
    loaded from the oracle's arrays."""
    x, blk, doc, oivf50 = sift60k
    x = x[:n]
    want = max(lists * 50, 10000)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(n, size=min(n, want), replace=False))
    samples = np.ascontiguousarray(x[pick])
    ref = np.zeros((lists, x.shape[1]), dtype=np.float32)
    from oracle.oracle import METRICS
    assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], x.shape[1], samples, len(samples), lists, 9, ref) == 0
    got, iters = ctx.ivf_kmeans(samples, lists, "l2", seed=9)
    assert iters >= 2
    np.testing.assert_array_equal(got, ref)
    if lists == 50:
        np.testing.assert_array_equal(got, oivf50.centers)             # (the fixture's index: same seed, same sampling rule)
        corpus = ctx.load_corpus(x, blk[:n], doc[:n])
        gpu, centers, row_list = corpus.build_ivf(x, lists, "l2", seed=9)
        np.testing.assert_array_equal(centers, oivf50.centers)
        np.testing.assert_array_equal(row_list, oivf50.assign)
        q = x[rng.integers(0, n, 6)]
        res = gpu.search(q, 20, 3, "l2")
        for i in range(6):
            idx, dist = oivf50.search(q[i], 20, 3)
            np.testing.assert_array_equal(res.rows[i], idx)
        gpu.free()
        corpus.free()
    # no samples at all: RandomCenters (ivfkmeans.c:124-147)
    ref0 = np.zeros((lists, 8), dtype=np.float32)
    assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], 8, np.zeros((0, 8), dtype=np.float32), 0, lists, 5, ref0) == 0
    got0, _ = ctx.ivf_kmeans(np.zeros((0, 8), dtype=np.float32), lists, "l2", seed=5)
    np.testing.assert_array_equal(got0, ref0)


def test_ivf_kmeans_spherical_variant(ctx, oracle):
    """Inner-product / cosine opclasses: spherical k-means (unit centres, angular distance through acos): centres within
    1e-6 of the oracle's and the same assignment of every row."""
    from oracle.oracle import METRICS
    rng = np.random.default_rng(17)
    n, dim, lists = 20_000, 48, 20
    x = rng.normal(size=(n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    samples = np.ascontiguousarray(x[:10_000])
    ref = np.zeros((lists, dim), dtype=np.float32)
    assert oracle.lib.orc_ivf_kmeans(METRICS["cosine"], dim, samples, len(samples), lists, 3, ref) == 0
    got, _ = ctx.ivf_kmeans(samples, lists, "cosine", seed=3)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# f2: HNSW build on the GPU (vsr_hnsw_build: batched insertion).  Graph identity is not reproducible even in the reference
# (its parallel build races), so parity WITH PGVECTOR = recall (graph identity with the serial model of the batched build:
# tests/test_gpu_hnsw_build_model.py): pgvector's own TAP case and thresholds
# (pgvector/test/t/012_hnsw_vector_build_recall.pl: 10 000 rows of 3-d random() * random(), 20 queries, LIMIT 20, default m,
# ef_construction, ef_search; >= 0.99, inner product >= 0.97), and recall within 0.01 of the index oracle's serial build.
# ---------------------------------------------------------------------------------------------
def _recall(found_rows, exact_rows):
    hit = sum(len(set(f.tolist()) & set(e.tolist())) for f, e in zip(found_rows, exact_rows))
    return hit / sum(len(e) for e in exact_rows)


@pytest.mark.parametrize("metric,floor", [("l2", 0.99), ("ip", 0.97), ("cosine", 0.99)])
def test_hnsw_build_on_the_gpu_recall_parity_tap_case(ctx, oracle, metric, floor):
    rng = np.random.default_rng(1201)
    n, k = 10_000, 20
    x = (rng.random((n, 3)) * rng.random((n, 3))).astype(np.float32)
    q = rng.random((20, 3)).astype(np.float32)
    if metric == "cosine":                                                 # the opclass ranks unit vectors by inner product
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    corpus = ctx.load_corpus(x)
    exact = corpus.search(q, k, metric).rows
    gpu = corpus.build_hnsw(16, 64, metric, seed=3)
    n_elem, entry, entry_level, max_level = gpu.info()
    assert n_elem == n and 0 <= entry < n and 1 <= entry_level <= max_level
    got, _ = gpu.search(q, k, 40, metric)
    r_gpu = _recall([got.rows[i][:got.counts[i]] for i in range(len(q))], exact)
    ref = OracleHnsw(oracle, metric, x, m=16, ef_construction=64, seed=3)
    r_ref = _recall([ref.search(q[i], 40)[0][:k] for i in range(len(q))], exact)
    print(f"hnsw build {metric}: recall@20 GPU batched {r_gpu:.4f}, serial port {r_ref:.4f}")
    assert r_gpu >= floor, (r_gpu, r_ref)
    assert r_gpu >= r_ref - 0.01, (r_gpu, r_ref)
    check_built_graph(gpu.export(), 16)
    gpu.free()
    corpus.free()


def test_hnsw_build_on_the_gpu_128d(ctx, oracle):
    """SIFT-like 128-d rows: the batched build's graph answers like the serial port's at the same ef_search (recall within
    0.02), and the exported graph is well formed: lists of 2m / m at most, neighbours that live on their layer, no element but
    the first without a layer-0 neighbour, the first element of the highest level as entry point (helpers.check_built_graph)."""
    rng = np.random.default_rng(1202)
    n, dim, k = 20_000, 128, 10
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    q = x[rng.integers(0, n, 50)] + rng.integers(-3, 4, (50, dim)).astype(np.float32)
    corpus = ctx.load_corpus(x)
    exact = corpus.search(q, k, "l2").rows
    gpu = corpus.build_hnsw(16, 64, "l2", seed=5)
    ref = OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=5)
    for ef in (40, 200):
        got, _ = gpu.search(q, k, ef, "l2")
        r_gpu = _recall([got.rows[i][:got.counts[i]] for i in range(len(q))], exact)
        r_ref = _recall([ref.search(q[i], ef)[0][:k] for i in range(len(q))], exact)
        print(f"hnsw build 128-d ef={ef}: recall@10 GPU batched {r_gpu:.4f}, serial port {r_ref:.4f}")
        assert r_gpu >= r_ref - 0.02, (ef, r_gpu, r_ref)
    check_built_graph(gpu.export(), 16)
    gpu.free()
    corpus.free()
