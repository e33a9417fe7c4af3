"""HNSW over bit corpora on the GPU (K4b: vsr_hnsw_load_bit / build_bit / search_bit*, vsr_hnsw_search_quantized*).

Hamming: squared L2 on rows unpacked to 0 / 1 floats IS the Hamming distance, an exact integer in fp32, so the index oracle
built on the unpacked rows is pgvector's serial build and GetScanItems walk for bit_hamming_ops, tie rule included; rows,
distances and visited counts must be identical.  Jaccard has no float twin: it is pinned by the numpy walk of
tests/hnsw_bit_model.py (itself pinned to the oracle by tests/test_hnsw_bit_cpu.py) on the same graphs."""
import ctypes

import numpy as np
import pytest

import bit_model
from oracle.oracle import HnswIndex as OracleHnsw
from hnsw_iterative_model import Stream
from hnsw_bit_model import BitGraph, BitScan, indexed_two_stage, search, tap_case, tap_recall, tie_aware_expected
from quantized_model import QuantizedModel

pytestmark = pytest.mark.gpu

NQ = 24
ZERO_ROW = 7                                                 # an all-zero row in every case (Jaccard: distance 1 to everything)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _clustered(rng, n, dim, centres=200):
    """Rows around a few hundred random centres with 5-10 % of the bits flipped: a graph with structure."""
    c = rng.integers(0, 2, (centres, dim)).astype(bool)
    flip = rng.random((n, dim)) < rng.uniform(0.05, 0.10, (n, 1))
    return c[rng.integers(0, centres, n)] ^ flip


_CASES = {}


def _case(ctx, oracle, n, dim, m=16, efc=64):
    """Rows (40 exact copies of row 100 planted, row ZERO_ROW all zeros), the oracle's graph on the unpacked rows, the corpus
    with 5 % / 25 % users, both opclasses loaded, 24 queries (0: the planted row, 1: all zeros).  Built once per module."""
    key = (n, dim, m)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 + dim + m)
    bits = _clustered(rng, n, dim)
    bits[ZERO_ROW] = False
    bits[n // 2:n // 2 + 40] = bits[100]
    packed = bit_model.pack(bits)
    unpacked = bits.astype(np.float32)
    oh = OracleHnsw(oracle, "l2", unpacked, m=m, ef_construction=efc, seed=5)
    g = oh.export()
    assert m != 16 or g["tid_count"].max() == 10             # (the serial build folds the copies into elements of 10 TIDs)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), max(1, ndocs // 20), replace=False)]
    perms += [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 4, replace=False)]
    ur = [(1, 1), (2, 2)]
    corpus = ctx.load_corpus_bit(packed, dim, blk, doc)
    corpus.load_rbac(ur, perms)
    qbits = bits[rng.integers(0, n, NQ)] ^ (rng.random((NQ, dim)) < 0.03)
    qbits[0] = bits[100]
    qbits[1] = False
    c = {"n": n, "dim": dim, "packed": packed, "unpacked": unpacked, "oh": oh, "g": BitGraph(g, packed, dim), "export": g,
         "corpus": corpus, "q": bit_model.pack(qbits), "qf": qbits.astype(np.float32),
         "masks": {u: oracle.user_row_mask(u, ur, perms, doc).astype(bool) for u in (1, 2)},
         "hamming": corpus.load_hnsw_bit(g, "hamming"), "jaccard": corpus.load_hnsw_bit(g, "jaccard")}
    _CASES[key] = c
    return c


SHAPES = [(4000, 52), (4000, 128), (3000, 129), (2000, 1001), (600, 8200)]    # G = 1, G = 1, two chunks + pad bits, eight
                                                                              # chunks + a partial byte, stride4 = 65: the chunk loop


def _check_hamming(c, ef, k=600):
    gpu, oh = c["hamming"], c["oh"]
    res, vis = gpu.search_bit(c["q"], k, ef, "hamming", dim=c["dim"])
    pad, vis_pad = gpu.search_bit(bit_model.set_pad_bits(c["q"], c["dim"]), k, ef, "hamming", dim=c["dim"])   # garbage pad bits
    for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
        np.testing.assert_array_equal(getattr(res, f), getattr(pad, f))
    np.testing.assert_array_equal(vis, vis_pad)
    for i in range(NQ):
        rows_o, dist_o, _, nv = oh.search(c["qf"][i], ef)
        want = rows_o[:k]
        assert res.counts[i] == want.size, (ef, i, res.counts[i], want.size)
        np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str((ef, i)))
        np.testing.assert_array_equal(res.dist[i, :want.size], dist_o[:k].astype(np.float32), err_msg=str((ef, i)))
        assert vis[i] == nv, (ef, i, vis[i], nv)
        assert (res.rows[i, want.size:] == -1).all()
    return res


# ---- 1. walk parity, Hamming -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", SHAPES)
def test_hamming_walk_is_the_oracle_walk(ctx, oracle, n, dim):
    c = _case(ctx, oracle, n, dim)
    for ef in (10, 40, 500):
        res = _check_hamming(c, ef)
    # the planted row: its copies come out at distance 0, an element's TIDs newest first
    cnt = res.counts[0]
    zero = res.rows[0, :cnt][res.dist[0, :cnt] == 0]
    assert set(range(n // 2, n // 2 + 40)) | {100} <= set(zero.tolist())
    tids = c["export"]["tids"]
    full = np.flatnonzero(c["export"]["tid_count"] == 10)[0]
    at = int(np.flatnonzero(res.rows[0, :cnt] == tids[full, 9])[0])
    np.testing.assert_array_equal(res.rows[0, at:at + 10], tids[full, ::-1])


@pytest.mark.parametrize("n,dim,m,efc", [(1500, 64, 100, 200), (2000, 64, 4, 32)])
def test_hamming_walk_wide_and_narrow_lists(ctx, oracle, n, dim, m, efc):
    """m = 100: 2m = 200 neighbours per expansion (four 64-neighbour wave steps at G = 1); m = 4: lists of 8."""
    c = _case(ctx, oracle, n, dim, m, efc)
    for ef in (10, 40, 500):
        _check_hamming(c, ef)


# ---- 2. walk parity, Jaccard -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [s for s in SHAPES if s[1] <= 2048])
def test_jaccard_walk_is_the_model_walk(ctx, oracle, n, dim):
    """dim <= 2048: no two distinct Jaccard values round to the same fp32, so fp32 ties are true ties."""
    c = _case(ctx, oracle, n, dim)
    gpu, g, k = c["jaccard"], c["g"], 600
    for ef in (10, 40, 500):
        res, vis = gpu.search_bit(c["q"], k, ef, "jaccard", dim=dim)
        for i in range(NQ):
            rows, dist, t = search(g, c["q"][i], ef, "jaccard")
            want = rows[:k]
            assert res.counts[i] == want.size, (ef, i)
            np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str((ef, i)))
            np.testing.assert_array_equal(res.dist[i, :want.size], dist[:k].astype(np.float32), err_msg=str((ef, i)))
            assert vis[i] == t, (ef, i, vis[i], t)
        cnt = res.counts[1]
        assert (res.dist[1, :cnt] == 1.0).all()              # the all-zero query: no common bit with anything
        zr = np.flatnonzero(res.rows[:, :] == ZERO_ROW)
        assert (res.dist.ravel()[zr] == 1.0).all()           # the all-zero row, wherever it came out


# ---- 3. filters --------------------------------------------------------------------------------------------------------
def test_filters_plain_and_predicate_aware(ctx, oracle):
    """Plain walk: the oracle's stream filtered.  Predicate-aware walk: Hamming equals oracle.search_predicate_aware on the
    unpacked rows at filter shares 0.05 and 0.25.  Jaccard has no restatement of the predicate-aware walk: it is checked by
    recall against search_bit under the same filter, compared with the plain walk (the second of the two options)."""
    import vsrbac
    c = _case(ctx, oracle, 4000, 128)
    corpus, oh, k = c["corpus"], c["oh"], 20
    ham, jac = c["hamming"], c["jaccard"]
    for user in (1, 2):
        mask = c["masks"][user]
        for mode in (vsrbac.BITMAP, vsrbac.RANGES):
            flt = [corpus.filter_for_user(user, mode)] * NQ
            for ef in (20, 100):
                for aware in (False, True):
                    ham.set_predicate_aware(aware)
                    res, vis = ham.search_bit(c["q"], k, ef, "hamming", flt)
                    for i in range(NQ):
                        rows_o, dist_o, _, nv = (oh.search_predicate_aware(c["qf"][i], ef, mask.astype(np.uint8)) if aware
                                                 else oh.search(c["qf"][i], ef))
                        keep = mask[rows_o]
                        want, wd = rows_o[keep][:k], dist_o[keep][:k]
                        assert res.counts[i] == want.size, (user, mode, ef, aware, i)
                        np.testing.assert_array_equal(res.rows[i, :want.size], want)
                        np.testing.assert_array_equal(res.dist[i, :want.size], wd.astype(np.float32))
                        assert vis[i] == nv
                ham.set_predicate_aware(False)
        # Jaccard, by recall
        flt = [corpus.filter_for_user(user, vsrbac.BITMAP)] * NQ
        exact = corpus.search_bit(c["q"], k, "jaccard", flt)
        recalls = {}
        for aware in (False, True):
            jac.set_predicate_aware(aware)
            res, _ = jac.search_bit(c["q"], k, 100, "jaccard", flt)
            hits = sum(len(set(res.rows[i, :res.counts[i]].tolist()) & set(exact.rows[i, :exact.counts[i]].tolist()))
                       for i in range(NQ))
            recalls[aware] = hits / max(1, int(exact.counts.sum()))
            if not aware:                                    # the plain walk: the model's stream filtered
                for i in range(NQ):
                    rows, dist, _ = search(c["g"], c["q"][i], 100, "jaccard")
                    want = rows[mask[rows]][:k]
                    np.testing.assert_array_equal(res.rows[i, :want.size], want)
                    assert res.counts[i] == want.size
        jac.set_predicate_aware(False)
        print(f"jaccard user {user}: recall@{k} ef=100 plain+filter {recalls[False]:.3f}, predicate-aware {recalls[True]:.3f}")
        assert recalls[True] >= recalls[False]


# ---- 4. iterative scans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["hamming", "jaccard"])
def test_iterative_matches_the_model(ctx, oracle, metric, monkeypatch):
    import vsrbac
    c = _case(ctx, oracle, 4000, 128)
    corpus, gpu, g, q = c["corpus"], c[metric], c["g"], c["q"][:12]
    nq, ef = len(q), 40
    filters = {"none": (None, None), "5%": ([corpus.filter_for_user(1, vsrbac.BITMAP)] * nq, c["masks"][1])}

    def check(modes, scans, ks):
        for mode in modes:
            for max_scan in scans:
                streams = [Stream(BitScan(g, q[i], ef, metric, mode, max_scan)) for i in range(nq)]
                for k in ks:
                    for fname, (flt, mask) in filters.items():
                        res, tup = gpu.search_bit_iterative(q, k, ef, metric, flt, mode, max_scan)
                        for i in range(nq):
                            rows, d, t = streams[i].answer(k, mask)
                            where = (metric, mode, max_scan, k, fname, i)
                            assert res.counts[i] == rows.size, (where, res.counts[i], rows.size)
                            np.testing.assert_array_equal(res.rows[i, :rows.size], rows, err_msg=str(where))
                            np.testing.assert_array_equal(res.dist[i, :rows.size], np.asarray(d).astype(np.float32), err_msg=str(where))
                            assert tup[i] == t, (where, tup[i], t)

    check(("relaxed_order", "strict_order"), (1, 200, 20000), (5, 60))
    monkeypatch.setenv("VSR_HNSW_DISCARD_CAP", "64")         # D overflows: the host entry point re-runs with room for every element
    check(("relaxed_order",), (20000,), (60,))
    monkeypatch.delenv("VSR_HNSW_DISCARD_CAP")
    for flt, _ in filters.values():                          # mode off is search_bit, bit for bit
        a, vis = gpu.search_bit(q, 60, ef, metric, flt)
        b, tup = gpu.search_bit_iterative(q, 60, ef, metric, flt, mode="off")
        for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        np.testing.assert_array_equal(vis, tup)


# ---- 5. visited forms and the device API ---------------------------------------------------------------------------------
def _device(gpu, q, k, ef, metric, flt=None, iterative=None):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq = len(q)
    raw = torch.zeros(q.size + 1, dtype=torch.uint8, device=dev)
    raw[1:] = torch.from_numpy(np.ascontiguousarray(q).ravel()).to(dev)       # an odd address: device queries need no alignment
    d_q = ctypes.c_void_p(raw.data_ptr() + 1)
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.empty((nq,), dtype=torch.int64, device=dev)}
    if iterative:
        keep = gpu.search_bit_iterative_device(d_q, nq, k, ef, metric, flt, iterative[0], iterative[1], p(o["blk"]), p(o["doc"]),
                                               p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    else:
        keep = gpu.search_bit_device(d_q, nq, k, ef, metric, flt, p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]),
                                     p(o["vis"]))
    gpu.corpus.ctx.synchronize()
    del keep
    return {key: v.cpu().numpy() for key, v in o.items()}


def test_visited_forms_and_device_entry_points(ctx, oracle, monkeypatch):
    import vsrbac
    c = _case(ctx, oracle, 3000, 129)
    corpus, q, k, ef = c["corpus"], c["q"], 50, 40
    flt = [corpus.filter_for_user(2, vsrbac.BITMAP)] * NQ
    for metric in ("hamming", "jaccard"):
        gpu = c[metric]
        for f in (None, flt):
            host, vis = gpu.search_bit(q, k, ef, metric, f)
            d = _device(gpu, q, k, ef, metric, f)
            np.testing.assert_array_equal(d["row"], host.rows)
            np.testing.assert_array_equal(d["blk"], host.block_ids)
            np.testing.assert_array_equal(d["doc"], host.doc_ids)
            np.testing.assert_array_equal(d["dist"], host.dist)
            np.testing.assert_array_equal(d["cnt"], host.counts)
            np.testing.assert_array_equal(d["vis"], vis)
            hi, tup = gpu.search_bit_iterative(q, k, ef, metric, f, "relaxed_order", 500)
            di = _device(gpu, q, k, ef, metric, f, ("relaxed_order", 500))
            np.testing.assert_array_equal(di["row"], hi.rows)
            np.testing.assert_array_equal(di["dist"], hi.dist)
            np.testing.assert_array_equal(di["cnt"], hi.counts)
            np.testing.assert_array_equal(di["vis"], tup)
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:64")        # the LDS hash overflows: the host entry point re-runs, the device one reports
    _check_hamming(c, 40)
    d = _device(c["hamming"], q, k, ef, "hamming")
    assert (d["cnt"] == -1).all() and (d["row"] == -1).all()
    monkeypatch.setenv("VSR_HNSW_VISITED", "global")
    _check_hamming(c, 40)
    monkeypatch.delenv("VSR_HNSW_VISITED")


# ---- 6. build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,floor", [("hamming", 0.98), ("jaccard", 0.95)])
def test_build_reaches_the_tap_floor(ctx, oracle, metric, floor):
    """020_hnsw_bit_build_recall.pl's case and floors (the rows and seeds of tests/test_hnsw_bit_cpu.py); Hamming within 0.01
    of the oracle's serial build on the same rows, the margin tests/test_gpu_index.py uses for the float build."""
    rows, queries, dim, limit, ef = tap_case()
    corpus = ctx.load_corpus_bit(rows, dim)
    exact = corpus.search_bit(queries, 2048, metric)
    model = bit_model.BitModel(rows, dim).distances(metric, queries).astype(np.float32)
    expected = []
    for i in range(len(queries)):                            # tie-aware, as the TAP test builds it: every row no farther than the 20th
        kth = exact.dist[i, limit - 1]
        assert exact.dist[i, exact.counts[i] - 1] > kth      # (the 2048 rows asked for hold the whole tie group)
        expected.append(np.sort(exact.rows[i, :exact.counts[i]][exact.dist[i, :exact.counts[i]] <= kth]))
        np.testing.assert_array_equal(expected[-1], tie_aware_expected(model[i], limit))
    gpu = corpus.build_hnsw_bit(16, 64, metric, seed=1)
    res, _ = gpu.search_bit(queries, limit, ef, metric)
    r = tap_recall([res.rows[i, :res.counts[i]] for i in range(len(queries))], expected, limit)
    print(f"build_hnsw_bit {metric}: recall@{limit} ef={ef} = {r:.4f} (floor {floor})")
    assert r >= floor
    if metric == "hamming":
        oh = OracleHnsw(oracle, "l2", bit_model.unpack(rows, dim).astype(np.float32), m=16, ef_construction=64, seed=1)
        qf = bit_model.unpack(queries, dim).astype(np.float32)
        ro = tap_recall([oh.search(qf[i], ef)[0] for i in range(len(queries))], expected, limit)
        print(f"  oracle serial build: {ro:.4f}")
        assert r >= ro - 0.01
    gpu.free()
    corpus.free()


def test_build_on_clustered_128_bit_rows(ctx, oracle):
    rng = np.random.default_rng(128)
    n, dim, k, ef = 20_000, 128, 20, 40
    bits = _clustered(rng, n, dim, centres=400)
    packed = bit_model.pack(bits)
    q = bit_model.pack(bits[rng.integers(0, n, 40)] ^ (rng.random((40, dim)) < 0.03))
    corpus = ctx.load_corpus_bit(packed, dim)
    gpu = corpus.build_hnsw_bit(16, 64, "hamming", seed=2)
    res, _ = gpu.search_bit(q, k, ef, "hamming")
    exact = bit_model.BitModel(packed, dim).distances("hamming", q)
    expected = [tie_aware_expected(exact[i], k) for i in range(len(q))]
    r = tap_recall([res.rows[i, :res.counts[i]] for i in range(len(q))], expected, k)
    oh = OracleHnsw(oracle, "l2", bits.astype(np.float32), m=16, ef_construction=64, seed=2)
    qf = bit_model.unpack(q, dim).astype(np.float32)
    ro = tap_recall([oh.search(qf[i], ef)[0] for i in range(len(q))], expected, k)
    print(f"20000 x 128 clustered: recall@{k} ef={ef} GPU build {r:.4f}, oracle build {ro:.4f}")
    assert r >= ro - 0.01
    gpu.free()
    corpus.free()


def test_merging_build(ctx):
    """3000 x 10-bit rows (1024 possible values: full of duplicates) with a planted group of 25."""
    rng = np.random.default_rng(10)
    n, dim = 3000, 10
    bits = rng.integers(0, 2, (n, dim)).astype(bool)
    planted = np.array([1, 1, 0, 1, 0, 0, 1, 1, 0, 1], dtype=bool)
    bits[(bits == planted).all(axis=1)] ^= np.array([1] + [0] * 9, dtype=bool)       # nobody else holds the planted value
    where = np.sort(rng.choice(n, 25, replace=False))
    bits[where] = planted
    packed = bit_model.pack(bits)
    corpus = ctx.load_corpus_bit(packed, dim)
    merged = corpus.build_hnsw_bit(8, 32, "hamming", seed=11, merge_duplicates=True)
    plain = corpus.build_hnsw_bit(8, 32, "hamming", seed=11)
    g, gp = merged.export(), plain.export()
    groups = {}
    for r in range(n):
        groups.setdefault(packed[r].tobytes(), []).append(r)
    want = sorted(tuple(rows[i:i + 10]) for rows in groups.values() for i in range(0, len(rows), 10))
    assert merged.info()[0] == len(g["level"]) == sum(-(-len(rows) // 10) for rows in groups.values())
    got = [tuple(int(t) for t in g["tids"][e, :g["tid_count"][e]]) for e in range(len(g["level"]))]
    assert sorted(got) == want
    assert (np.diff(g["tids"][:, 0]) > 0).all(), "elements are numbered by their first member"
    assert len(gp["level"]) == n and (gp["tid_count"] == 1).all() and (gp["tids"][:, 0] == np.arange(n)).all()
    assert (g["level"] == gp["level"][g["tids"][:, 0]]).all()
    q = bit_model.pack(planted[None, :])
    res, _ = merged.search_bit(q, 100, 400, "hamming")
    zero = res.rows[0, :res.counts[0]][res.dist[0, :res.counts[0]] == 0]
    assert sorted(zero.tolist()) == where.tolist()
    again = corpus.load_hnsw_bit(g, "hamming")
    qs = packed[rng.integers(0, n, 16)]
    for ef in (10, 100):
        a, va = merged.search_bit(qs, 50, ef, "hamming")
        b, vb = again.search_bit(qs, 50, ef, "hamming")
        for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        np.testing.assert_array_equal(va, vb)
    for h in (again, merged, plain):
        h.free()
    corpus.free()


# ---- 7. indexed two-stage ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_stage(ctx, oracle):
    import vsrbac
    rng = np.random.default_rng(64)
    n, dim = 5000, 64
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 10 + 1).astype(np.int32)
    q = x[rng.integers(0, n, 12)] + rng.integers(-2, 3, (12, dim)).astype(np.float32)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 4, replace=False)]
    perms += [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), 12, replace=False)]       # 120 rows
    ur = [(1, 1), (2, 2)]
    out = {"x": x, "q": q, "doc": doc, "blk": blk, "masks": {u: oracle.user_row_mask(u, ur, perms, doc).astype(bool) for u in (1, 2)}}
    for name, src in (("fp32", ctx.load_corpus(x, blk, doc)), ("half", ctx.load_corpus_half(x, blk, doc))):
        bits = src.binary_quantize()
        bits.load_rbac(ur, perms)
        index = bits.build_hnsw_bit(16, 64, "hamming", seed=3, merge_duplicates=True)
        out[name] = {"src": src, "bits": bits, "index": index, "qm": QuantizedModel(oracle, x, doc, blk, half=name == "half"),
                     "g": BitGraph(index.export(), bit_model.binary_quantize(x), dim)}
    yield out
    for name in ("fp32", "half"):
        out[name]["index"].free()
        out[name]["bits"].free()
        out[name]["src"].free()


def _want_dist(metric, d):
    return np.asarray(d, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("kind", ["fp32", "half"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_indexed_two_stage_is_the_model(ctx, two_stage, kind, metric):
    import torch
    import vsrbac
    t, q, k = two_stage[kind], two_stage["q"], 10
    src, bits, index, nq = t["src"], t["bits"], t["index"], len(two_stage["q"])
    dev = torch.device("cuda", 0)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    for shortlist in (20, 200):
        for ef in (40, 400):
            for flt, mask in ((None, None), ([bits.filter_for_user(1, vsrbac.BITMAP)] * nq, two_stage["masks"][1])):
                want = indexed_two_stage(t["qm"], t["g"], q, k, shortlist, ef, metric, None if mask is None else [mask] * nq)
                res = src.search_quantized_hnsw(index, q, k, shortlist, ef, metric, flt)
                d_q = torch.from_numpy(q).to(dev)
                o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
                     "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
                     "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "keys": torch.empty((nq, k), dtype=torch.int64, device=dev)}
                keep = src.search_quantized_hnsw_device(index, p(d_q), nq, k, shortlist, ef, metric, flt, p(o["blk"]), p(o["doc"]),
                                                        p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["keys"]))
                bits.ctx.synchronize()
                del keep
                for i in range(nq):
                    idx, dist, S = want[i]
                    where = (kind, metric, shortlist, ef, flt is not None, i)
                    assert res.counts[i] == idx.size, (where, res.counts[i], idx.size)
                    np.testing.assert_array_equal(res.rows[i, :idx.size], idx, err_msg=str(where))
                    if metric != "cosine":                   # (cosine: the oracle's float8 against the GPU's fp32 form, as test_gpu_quantized.py)
                        np.testing.assert_array_equal(res.dist[i, :idx.size], _want_dist(metric, dist), err_msg=str(where))
                np.testing.assert_array_equal(o["row"].cpu().numpy(), res.rows)
                np.testing.assert_array_equal(o["dist"].cpu().numpy(), res.dist)
                np.testing.assert_array_equal(o["cnt"].cpu().numpy(), res.counts)
                keys = o["keys"].cpu().numpy().view(np.uint64)
                for i in range(nq):
                    c = res.counts[i]
                    assert (keys[i, c:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
                    assert ((keys[i, :c] >> np.uint64(32)) != np.uint64(0xFFFFFFFF)).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_indexed_two_stage_small_filter_is_the_exact_search(ctx, two_stage, metric):
    """A filter admitting fewer rows than the shortlist, all of which a wide beam reaches: the answer of vsr_search."""
    import vsrbac
    t, q = two_stage["fp32"], two_stage["q"][:6]
    nq, mask, ef = len(q), two_stage["masks"][2], 5000
    assert 10 < mask.sum() < 200
    for i in range(nq):                                      # the precondition: the beam holds every permitted row
        S, _, _ = Stream(BitScan(t["g"], bit_model.binary_quantize(q[i:i + 1])[0], ef, "hamming", "off")).answer(200, mask)
        assert S.size == mask.sum()
    res = t["src"].search_quantized_hnsw(t["index"], q, 10, 200, ef, metric, [t["bits"].filter_for_user(2, vsrbac.BITMAP)] * nq)
    own = t["src"].filter_from_bytemask(mask.astype(np.uint8), vsrbac.BITMAP)
    exact = t["src"].search(q, 10, metric, [own] * nq)
    np.testing.assert_array_equal(res.rows, exact.rows)
    np.testing.assert_array_equal(res.dist, exact.dist)
    np.testing.assert_array_equal(res.counts, exact.counts)


# ---- 8. errors --------------------------------------------------------------------------------------------------------
def test_errors(ctx, oracle, two_stage):
    from vsrbac import VsrError
    from vsrbac.engine import MAX_K
    c = _case(ctx, oracle, 4000, 52)
    corpus, ham, jac, g, q, dim = c["corpus"], c["hamming"], c["jaccard"], c["export"], c["q"], c["dim"]

    def refused(status, word, fn, *a, **kw):
        with pytest.raises(VsrError) as e:
            fn(*a, **kw)
        assert e.value.status == status and word in str(e.value), (status, word, e.value.status, str(e.value))

    # the old entry points keep refusing a bit corpus, the float searches a bit index
    refused(6, "bit", corpus.load_hnsw, g)
    refused(6, "bit", corpus.build_hnsw, 16, 64, "l2")
    refused(6, "bit", corpus.build_hnsw, 16, 64, "l2", merge_duplicates=True)
    refused(6, "bit", ham.search, c["qf"], 10, 40, "l2")
    refused(6, "bit", ham.search_iterative, c["qf"], 10, 40, "l2")
    # dimension, metric, wrong entry point
    refused(2, f"different bit lengths {dim} and {dim + 1}", ham.search_bit, np.zeros((1, (dim + 8) // 8), np.uint8), 10, 40, "hamming", dim=dim + 1)
    refused(1, "Jaccard", ham.search_bit, q, 10, 40, "jaccard")
    refused(1, "Hamming", jac.search_bit, q, 10, 40, "hamming")
    refused(1, "Hamming", jac.search_bit_iterative, q, 10, 40, "hamming")
    refused(1, "metric", ham.search_bit, q, 10, 40, "l2")
    refused(1, "ef_search", ham.search_bit, q, 10, 0, "hamming")
    refused(1, "max_scan_tuples", ham.search_bit_iterative, q, 10, 40, "hamming", max_scan_tuples=0)
    refused(1, "metric", corpus.load_hnsw_bit, g, "l2")
    refused(1, "metric", corpus.build_hnsw_bit, 16, 64, "cosine")
    refused(6, "m must be", corpus.build_hnsw_bit, 101, 400, "hamming")
    ham.set_predicate_aware(True)
    refused(6, "predicate-aware", ham.search_bit_iterative, q, 10, 40, "hamming")
    ham.set_predicate_aware(False)
    fp = two_stage["fp32"]
    fsrc = fp["src"]
    refused(1, "not a bit corpus", fsrc.load_hnsw_bit, g)
    refused(1, "not a bit corpus", fsrc.build_hnsw_bit, 16, 64, "hamming")
    fidx = fsrc.build_hnsw(8, 32, "l2", seed=1)
    refused(1, "bit", fidx.search_bit, np.zeros((1, 8), np.uint8), 10, 40, "hamming", dim=64)
    # the indexed two-stage search
    x, qf = two_stage["x"], two_stage["q"]
    refused(1, "was not made from", fsrc.search_quantized_hnsw, ham, qf, 10, 20)
    refused(1, "not a bit corpus", fsrc.search_quantized_hnsw, fidx, qf, 10, 20)
    jq = fp["bits"].build_hnsw_bit(8, 32, "jaccard", seed=1)
    refused(1, "Hamming", fsrc.search_quantized_hnsw, jq, qf, 10, 20)
    refused(1, "shorter than k", fsrc.search_quantized_hnsw, fp["index"], qf, 10, 5)
    refused(1, "VSR_MAX_K", fsrc.search_quantized_hnsw, fp["index"], qf, 10, MAX_K + 1)
    refused(6, "L1", fsrc.search_quantized_hnsw, fp["index"], qf, 10, 20, 40, "l1")
    refused(2, "different vector dimensions", fsrc.search_quantized_hnsw, fp["index"], qf[:, :32], 10, 20)
    jq.free()
    fidx.free()
    # every handle works afterwards
    _check_hamming(c, 40)
    res = fsrc.search_quantized_hnsw(fp["index"], qf, 10, 20, 40, "l2")
    assert (res.counts == 10).all()
