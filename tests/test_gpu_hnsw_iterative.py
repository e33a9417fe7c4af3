"""pgvector's HNSW iterative index scans on the GPU (vsr_hnsw_search_iterative, K4's hnsw_iterative_kernel).

Exact parity with the numpy restatement of the stream (tests/hnsw_iterative_model.py, itself pinned to the index oracle):
rows, distances, counts and tuple counters, on an integer-valued graph where fp32 and float64 distances agree.  Then the
properties the shim relies on (mode off = vsr_hnsw_search, the prefix property, the device variant, the re-run paths),
mirrors of pgvector's TAP tests 043 and 044, and the errors."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_iterative_model import Graph, IterativeScan, Stream

pytestmark = pytest.mark.gpu

MODES = ("relaxed_order", "strict_order")


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g20k(oracle, ctx):
    """test_gpu_index.py's hnsw20k recipe: 20k x 128 integer rows, 41 copies of one vector (an element with 10 TIDs);
    user 1 may read 5 % of the documents, user 2 25 %."""
    rng = np.random.default_rng(81)
    n, dim = 20_000, 128
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, dim)))), 0, 255).astype(np.float32)
    x[5000:5040] = x[100]
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    h = OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=4)
    g = h.export()
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 20, replace=False)]
    perms += [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 4, replace=False)]
    ur = [(1, 1), (2, 2)]
    corpus = ctx.load_corpus(x, blk, doc)
    corpus.load_rbac(ur, perms)
    gpu = corpus.load_hnsw(g)
    masks = {u: oracle.user_row_mask(u, ur, perms, doc).astype(bool) for u in (1, 2)}
    nq = 24
    q = x[rng.integers(0, n, nq)] + rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    q[0] = x[100]
    yield {"x": x, "g": Graph(g, x), "corpus": corpus, "gpu": gpu, "masks": masks, "q": q}
    gpu.free()
    corpus.free()


def _want_dist(metric, d):
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt(d).astype(np.float32) if metric == "l2" else d.astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("ef", [10, 40, 200])
def test_iterative_matches_the_model(g20k, metric, ef):
    import vsrbac
    corpus, gpu, q, g, masks = g20k["corpus"], g20k["gpu"], g20k["q"], g20k["g"], g20k["masks"]
    nq = len(q)
    filters = {"none": (None, None)}
    for u, share in ((1, 5), (2, 25)):
        for mode_f, name in ((vsrbac.BITMAP, "bitmap"), (vsrbac.RANGES, "ranges")):
            filters[f"{share}%-{name}"] = ([corpus.filter_for_user(u, mode_f)] * nq, masks[u])
    checked = 0
    for mode in MODES:
        for max_scan in (300, 3000, 20000):
            streams = [Stream(IterativeScan(g, q[i], ef, metric, mode, max_scan)) for i in range(nq)]
            for k in (10, 100):
                for fname, (flt, mask) in filters.items():
                    res, tup = gpu.search_iterative(q, k, ef, metric, flt, mode, max_scan)
                    for i in range(nq):
                        rows, d, t = streams[i].answer(k, mask)
                        ctx_ = (metric, ef, mode, max_scan, k, fname, i)
                        assert res.counts[i] == rows.size, (ctx_, res.counts[i], rows.size)
                        np.testing.assert_array_equal(res.rows[i, :rows.size], rows, err_msg=str(ctx_))
                        np.testing.assert_array_equal(res.dist[i, :rows.size], _want_dist(metric, d), err_msg=str(ctx_))
                        assert tup[i] == t, (ctx_, tup[i], t)
                        assert (res.rows[i, rows.size:] == -1).all()
                        checked += 1
    print(f"iterative {metric} ef={ef}: {checked} (query, setting) pairs identical to the model")


def test_mode_off_is_the_plain_search(g20k):
    gpu, q, corpus = g20k["gpu"], g20k["q"], g20k["corpus"]
    import vsrbac
    for flt in (None, [corpus.filter_for_user(1, vsrbac.BITMAP)] * len(q)):
        for ef in (10, 100):
            a, vis = gpu.search(q, 50, ef, "l2", flt)
            b, tup = gpu.search_iterative(q, 50, ef, "l2", flt, mode="off")
            for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
                np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
            np.testing.assert_array_equal(vis, tup)


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(g20k, mode):
    import vsrbac
    gpu, q, corpus = g20k["gpu"], g20k["q"], g20k["corpus"]
    flt = [corpus.filter_for_user(1, vsrbac.RANGES)] * len(q)
    a, _ = gpu.search_iterative(q, 40, 40, "l2", flt, mode, 20000)
    b, _ = gpu.search_iterative(q, 200, 40, "l2", flt, mode, 20000)
    for i in range(len(q)):
        assert a.counts[i] == min(40, b.counts[i])
        np.testing.assert_array_equal(a.rows[i, :a.counts[i]], b.rows[i, :a.counts[i]])
        np.testing.assert_array_equal(a.dist[i, :a.counts[i]], b.dist[i, :a.counts[i]])


def _device_run(gpu, q, k, ef, flt, mode, max_scan):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "tup": torch.empty((nq,), dtype=torch.int64, device=dev)}
    keep = gpu.search_iterative_device(p(d_q), nq, k, ef, "l2", flt, mode, max_scan, p(o["blk"]), p(o["doc"]), p(o["row"]),
                                       p(o["dist"]), p(o["cnt"]), p(o["tup"]))
    gpu.corpus.ctx.synchronize()
    del keep
    return {key: v.cpu().numpy() for key, v in o.items()}


@pytest.mark.parametrize("mode", MODES)
def test_device_variant_equals_host(g20k, mode):
    import vsrbac
    gpu, q, corpus = g20k["gpu"], g20k["q"], g20k["corpus"]
    flt = [corpus.filter_for_user(1, vsrbac.BITMAP)] * len(q)
    for max_scan in (300, 20000):
        res, tup = gpu.search_iterative(q, 100, 40, "l2", flt, mode, max_scan)
        o = _device_run(gpu, q, 100, 40, flt, mode, max_scan)
        np.testing.assert_array_equal(o["cnt"], res.counts)
        np.testing.assert_array_equal(o["row"], res.rows)
        np.testing.assert_array_equal(o["dist"], res.dist)
        np.testing.assert_array_equal(o["tup"], tup)


def test_rerun_paths(g20k, monkeypatch):
    """VSR_HNSW_DISCARD_CAP=64: D overflows for most queries; the host entry point re-runs them with room for every element,
    the device variant reports them with count -1.  VSR_HNSW_VISITED=global: the global visited bitmap, same answers."""
    import vsrbac
    gpu, q, corpus = g20k["gpu"], g20k["q"], g20k["corpus"]
    flt = [corpus.filter_for_user(1, vsrbac.BITMAP)] * len(q)
    for mode in MODES:
        ref, rtup = gpu.search_iterative(q, 100, 40, "l2", flt, mode, 20000)
        for var, val in (("VSR_HNSW_DISCARD_CAP", "64"), ("VSR_HNSW_VISITED", "global")):
            monkeypatch.setenv(var, val)
            res, tup = gpu.search_iterative(q, 100, 40, "l2", flt, mode, 20000)
            np.testing.assert_array_equal(res.counts, ref.counts)
            np.testing.assert_array_equal(res.rows, ref.rows)
            np.testing.assert_array_equal(res.dist, ref.dist)
            np.testing.assert_array_equal(tup, rtup)
            if var == "VSR_HNSW_DISCARD_CAP":
                o = _device_run(gpu, q, 100, 40, flt, mode, 20000)
                over = o["cnt"] == -1
                assert over.sum() >= len(q) // 2, o["cnt"]
                ok = ~over
                np.testing.assert_array_equal(o["cnt"][ok], ref.counts[ok])
                np.testing.assert_array_equal(o["row"][ok], ref.rows[ok])
                assert (o["row"][over] == -1).all()
            monkeypatch.delenv(var)


@pytest.fixture(scope="module")
def tap043(oracle, ctx):
    rng = np.random.default_rng(43)
    n = 100_000
    x = rng.random((n, 3)).astype(np.float32)
    h = OracleHnsw(oracle, "l2", x, m=16, ef_construction=64, seed=43)
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_hnsw(h.export())
    allowed = ((np.arange(n) + 1) % 10000 == 0).astype(np.uint8)       # WHERE i % 10000 = 0 (i = 1 .. n)
    flt = corpus.filter_from_bytemask(allowed)
    yield x, gpu, flt
    gpu.free()
    corpus.free()


def test_tap043_max_scan_tuples(tap043):
    """pgvector test/t/043_hnsw_iterative_scan.pl on the serial build's graph: LIMIT 11 over 10 permitted rows returns all
    10 with max_scan_tuples = 100000; with 30000 / 50000 / 70000 the mean count over the queries i = 1 .. 20 lies within 2 of
    max_scan_tuples / 10000."""
    x, gpu, flt = tap043
    res, _ = gpu.search_iterative(x[:1], 11, 40, "l2", [flt], "relaxed_order", 100000)
    assert res.counts[0] == 10
    for max_scan in (30000, 50000, 70000):
        res, tup = gpu.search_iterative(x[:20], 11, 40, "l2", [flt] * 20, "relaxed_order", max_scan)
        avg = res.counts.mean()
        print(f"tap043 max_scan_tuples={max_scan}: mean count {avg:.2f} (expected {max_scan / 10000:.0f} +- 2), "
              f"mean tuples {tup.mean():.0f}")
        assert max_scan / 10000 - 2 < avg < max_scan / 10000 + 2


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_tap044_recall(oracle, ctx, metric):
    """pgvector test/t/044_hnsw_iterative_scan_recall.pl on the serial build's graph: WHERE i % c = 0 (c = 50, 500),
    ef_search 40, LIMIT 20; the expected set is every row within the 20th exact permitted distance."""
    rng = np.random.default_rng(44)
    n, k = 50_000, 20
    x = rng.random((n, 3)).astype(np.float32)
    q = rng.random((20, 3)).astype(np.float32)
    if metric == "cosine":                                                 # the opclass ranks unit vectors by inner product
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    h = OracleHnsw(oracle, metric, x, m=16, ef_construction=64, seed=44)
    corpus = ctx.load_corpus(x)
    gpu = corpus.load_hnsw(h.export())
    x64 = x.astype(np.float64)
    for c in (50, 500):
        allowed = ((np.arange(n) + 1) % c == 0)
        flt = corpus.filter_from_bytemask(allowed.astype(np.uint8))
        for mode in MODES:
            res, _ = gpu.search_iterative(q, k, 40, metric, [flt] * len(q), mode, 20000)
            correct = 0
            for i in range(len(q)):
                qq = q[i].astype(np.float64)
                dist = ((x64 - qq) ** 2).sum(1) if metric == "l2" else 1.0 - x64 @ qq
                top = np.sort(dist[allowed])[k - 1]
                expected = set(np.nonzero(dist <= top)[0].tolist())
                correct += len(set(res.rows[i, :res.counts[i]].tolist()) & expected)
            recall = correct / (k * len(q))
            print(f"tap044 {metric} {mode} c={c}: recall {recall:.3f}")
            assert recall >= 0.99, (metric, mode, c, recall)
    gpu.free()
    corpus.free()


def test_errors(g20k):
    import vsrbac
    from vsrbac._ffi import ERR_INVALID, ERR_UNSUPPORTED
    gpu, q = g20k["gpu"], g20k["q"]
    with pytest.raises(vsrbac.VsrError) as e:
        gpu.search_iterative(q, 10, 40, "l2", None, 3)
    assert e.value.status == ERR_INVALID
    for bad in (0, -1, 2**31):
        with pytest.raises(vsrbac.VsrError) as e:
            gpu.search_iterative(q, 10, 40, "l2", None, "relaxed_order", bad)
        assert e.value.status == ERR_INVALID
    res, _ = gpu.search_iterative(q, 10, 40, "l2", None, "relaxed_order", 2**31 - 1)
    assert (res.counts == 10).all()
    with pytest.raises(vsrbac.VsrError) as e:
        gpu.search_iterative(q, 10, 40, "l1", None, "relaxed_order")
    assert e.value.status == ERR_UNSUPPORTED
    with pytest.raises(vsrbac.VsrError) as e:
        gpu.search_iterative(q, 4096, 40, "l2", None, "relaxed_order")
    assert e.value.status == ERR_UNSUPPORTED
    gpu.set_predicate_aware(True)
    try:
        with pytest.raises(vsrbac.VsrError) as e:
            gpu.search_iterative(q, 10, 40, "l2", None, "strict_order")
        assert e.value.status == ERR_UNSUPPORTED
        gpu.search_iterative(q, 10, 40, "l2", None, "off")                  # off: the plain (predicate-aware) search
    finally:
        gpu.set_predicate_aware(False)


def test_short_answers_get_filled(g20k, oracle):
    """5 % of the documents permitted, ef 40, k 100: wherever the plain walk + filter comes back short, relaxed_order fills
    the answer."""
    import vsrbac
    gpu, q, corpus, masks, x = g20k["gpu"], g20k["q"], g20k["corpus"], g20k["masks"], g20k["x"]
    flt = [corpus.filter_for_user(1, vsrbac.BITMAP)] * len(q)
    plain, _ = gpu.search(q, 100, 40, "l2", flt)
    it, _ = gpu.search_iterative(q, 100, 40, "l2", flt, "relaxed_order", 20000)
    short = plain.counts < 100
    assert short.any()
    assert (it.counts[short] == 100).all(), it.counts
    n = len(x)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    hits = {"plain": 0, "relaxed": 0}
    for i in range(len(q)):
        exact, _ = oracle.filtered_topk("l2", x, q[i], 100, doc, blk, masks[1].astype(np.uint8))
        ex = set(exact.tolist())
        hits["plain"] += len(set(plain.rows[i, :plain.counts[i]].tolist()) & ex)
        hits["relaxed"] += len(set(it.rows[i, :it.counts[i]].tolist()) & ex)
    r = {key: v / (100 * len(q)) for key, v in hits.items()}
    print(f"5% permitted, ef 40, k 100: recall plain walk + filter {r['plain']:.3f}, relaxed_order {r['relaxed']:.3f}")
    assert r["relaxed"] > r["plain"]
