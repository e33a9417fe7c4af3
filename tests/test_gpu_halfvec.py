"""halfvec corpora on the GPU (vsr_corpus_load_half, K1h: vsr_scan.h with HALF = true).

pgvector computes every halfvec distance by widening both operands to fp32 and doing vector.c's arithmetic (halfutils.c;
pinned on the CPU by tests/test_halfvec_formats.py), so the expected answer everywhere is the existing oracle on
`rows.astype(np.float32)` and `q.astype(np.float16).astype(np.float32)`.  Integer-valued inputs 0..31 are exact in binary16
and their fp32 sums are exact in any order (31^2 * 4100 < 2^24): ids and distances bit for bit.  Real-valued inputs: 1e-4.
Every search asserts that the half instantiation ran (`half` in vsr_last_scan_kernel)."""
import ctypes
import json
import math
import os

from types import SimpleNamespace

import numpy as np
import pytest

from helpers import assert_valid_topk, sift_like

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_halfvec_known_answers.json")) as f:
        return json.load(f)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ids(n, rows_per_doc):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _rq(q):
    """The query `$1::halfvec` holds, widened."""
    with np.errstate(over="ignore"):
        return np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float32)


def _small_ints(rng, shape):
    return np.clip(np.rint(np.abs(rng.normal(0, 6, shape))), 0, 31).astype(np.float32)


def _half_ran(ctx, fused=None):
    name = ctx.last_scan_kernel()
    assert "half" in name.lower(), name
    if fused is not None:
        assert ("in-kernel merge" in name) == fused, name


def _expect_exact(oracle, res, qi, metric, x, q, k, doc, blk, mask=None):
    """x: the half rows widened to fp32; q: the caller's fp32 query (rounded here)."""
    idx, dist = oracle.filtered_topk(metric, x, _rq(q), k, doc, blk, mask)
    m = res.counts[qi]
    assert m == idx.size, (m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.block_ids[qi, :m], blk[idx])
    np.testing.assert_array_equal(res.doc_ids[qi, :m], doc[idx])
    np.testing.assert_array_equal(res.dist[qi, :m], dist.astype(np.float32))
    assert (res.block_ids[qi, m:] == -1).all() and (res.doc_ids[qi, m:] == -1).all() and np.isposinf(res.dist[qi, m:]).all()


def _ref_all(metric, x, q):
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    if metric == "l2":
        return np.sqrt(((x64 - q64) ** 2).sum(1))
    if metric == "ip":
        return -(x64 @ q64)
    if metric == "l1":
        return np.abs(x64 - q64).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = (x64 @ q64) / np.sqrt((x64 ** 2).sum(1) * (q64 ** 2).sum())
    return 1.0 - np.clip(sim, -1, 1)


def _device_outputs(torch, dev, nq, k, keys=False):
    o = SimpleNamespace(blk=torch.empty((nq, k), dtype=torch.int64, device=dev), doc=torch.empty((nq, k), dtype=torch.int32, device=dev),
                        row=torch.empty((nq, k), dtype=torch.int64, device=dev), dist=torch.empty((nq, k), dtype=torch.float32, device=dev),
                        cnt=torch.empty((nq,), dtype=torch.int32, device=dev),
                        keys=torch.empty((nq, k), dtype=torch.int64, device=dev) if keys else None)
    torch.cuda.synchronize()                                  # the library runs on its own stream
    return o


def _as_result(o):
    return SimpleNamespace(block_ids=o.blk.cpu().numpy(), doc_ids=o.doc.cpu().numpy(), rows=o.row.cpu().numpy(),
                           dist=o.dist.cpu().numpy(), counts=o.cnt.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 2. pgvector's halfvec known answers through the search path
# ---------------------------------------------------------------------------------------------
def test_known_answers(ctx, known):
    """A corpus of the b operand, the a operand as the query, k = 1: the distance is halfvec.out's, exactly.  (The dimension
    case the other way round: the column is the operator's left operand, so its dimension comes first in the message.)"""
    import vsrbac
    metric = {"l2_distance": "l2", "inner_product": "ip", "negative_inner_product": "ip", "cosine_distance": "cosine",
              "l1_distance": "l1"}
    ran = 0
    for fn, a, b, want in known["distances"]:
        if isinstance(want, str) and want.startswith("ERROR:"):
            corpus = ctx.load_corpus_half(np.asarray([a], dtype=np.float32))
            with pytest.raises(vsrbac.VsrError) as e:
                corpus.search([b], 1, metric[fn])
            assert e.value.status == 2 and str(e.value) == known["dim_error"] and "ERROR:  " + str(e.value) == want
            corpus.free()
            continue
        corpus = ctx.load_corpus_half(np.asarray([b], dtype=np.float32))
        assert corpus.is_half
        res = corpus.search([a], 1, metric[fn])
        _half_ran(ctx)
        assert res.counts[0] == 1 and res.rows[0, 0] == 0
        got = float(res.dist[0, 0])
        if want == "NaN":
            assert math.isnan(got)
        else:
            assert got == (-want if fn == "inner_product" else want), (fn, a, b, got, want)    # the search ranks by <#> = -inner_product
        ran += 1
        corpus.free()
    assert ran >= 20


# ---------------------------------------------------------------------------------------------
# 3. randomized differential test, bit-exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_randomized_shapes_exact(ctx, oracle, seed):
    """The structure of test_gpu_parity.py::test_randomized_shapes_exact over half corpora: every row-layout class, one query
    per pass and shared passes, ranges, bitmaps and class decomposition, one or two selection levels."""
    import vsrbac
    rng = np.random.default_rng(5000 + seed)
    for _ in range(4):
        n = int(rng.choice([60, 700, 5000, 30000]))
        dim = int(rng.choice([1, 3, 7, 8, 9, 16, 100, 128, 129, 200, 320, 768]))
        k = int(rng.choice([1, 5, 10, 64, 100, 200]))
        nq = int(rng.choice([1, 2, 7, 16, 33, 100]))
        metric = str(rng.choice(["l2", "ip", "l1"]))
        x = _small_ints(rng, (n, dim))
        rows_per_doc = int(rng.choice([1, 7, 50]))
        blk, doc = _ids(n, rows_per_doc)
        corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
        q = _small_ints(rng, (nq, dim))
        kind = str(rng.choice(["none", "mask", "rbac"]))
        masks = [None] * nq
        filters = None
        if kind == "mask":
            base = [(rng.random(n) < p).astype(np.uint8) for p in (0.03, 0.5)]
            fs = [corpus.filter_from_bytemask(m) for m in base]
            pick = rng.integers(0, 2, nq)
            filters = [fs[j] for j in pick]
            masks = [base[j] for j in pick]
        elif kind == "rbac":
            ndocs = int(doc.max())
            nroles, nusers = 5, 9
            perms = sorted({(int(r), int(d)) for r in range(1, nroles + 1)
                            for d in rng.choice(np.arange(1, ndocs + 1), size=max(1, ndocs // 3), replace=False)})
            ur = sorted({(u, int(r)) for u in range(1, nusers + 1)
                         for r in rng.choice(np.arange(1, nroles + 1), size=int(rng.integers(1, 3)), replace=False)})
            corpus.load_rbac(ur, perms)
            users = rng.integers(1, nusers + 1, nq)
            mode = vsrbac.RANGES if rng.random() < 0.5 else vsrbac.BITMAP
            filters = [corpus.filter_for_user(int(u), mode) for u in users]
            masks = [oracle.user_row_mask(int(u), ur, perms, doc) for u in users]
        res = corpus.search(q, k, metric, filters)
        if any(m is None or m.any() for m in masks):           # (every filter empty: nothing is launched)
            _half_ran(ctx)
        for i in range(0, nq, max(1, nq // 6)):
            _expect_exact(oracle, res, i, metric, x, q[i], k, doc, blk, masks[i])
        corpus.free()


# ---------------------------------------------------------------------------------------------
# 4. every row-layout class on real-valued rows
# ---------------------------------------------------------------------------------------------
# (8 | 9, 32 | 33, 128 | 129, 256 | 257, 512 | 513, 1024 | 1025: the boundaries of scan_shape(RowFormat::HALF, dim))
LAYOUT_DIMS = [1, 3, 7, 8, 9, 15, 17, 32, 33, 64, 100, 128, 129, 255, 256, 257, 512, 513, 768, 1024, 1025, 1536, 2000, 4100]


@pytest.mark.parametrize("dim", LAYOUT_DIMS)
def test_row_layout_classes_real_valued(ctx, dim):
    rng = np.random.default_rng(40000 + dim)
    n, k = 1500, 20
    h = rng.normal(size=(n, dim)).astype(np.float16)
    x = h.astype(np.float32)
    q = rng.normal(size=(3, dim)).astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    res = corpus.search(q, k, "l2")
    _half_ran(ctx)
    for i in range(3):
        assert res.counts[i] == k
        assert_valid_topk(res.rows[i, :k], res.dist[i, :k], _ref_all("l2", x, _rq(q[i])), k, TOL)
    one = corpus.search(q[:1], k, "l2")                       # one query per pass (fused when the row needs no padding)
    _half_ran(ctx)
    assert_valid_topk(one.rows[0, :k], one.dist[0, :k], _ref_all("l2", x, _rq(q[0])), k, TOL)
    corpus.free()


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine", "l1"])
@pytest.mark.parametrize("dim", [128, 768])
def test_metrics_real_valued_under_a_mask(ctx, oracle, metric, dim):
    rng = np.random.default_rng(41)
    n, k = 1500, 20
    h = rng.normal(size=(n, dim)).astype(np.float16)
    if metric == "cosine":
        h[5] = 0                                              # one zero vector -> NaN distance, sorted last
    x = h.astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[5] = 1
    q = (x[rng.integers(10, n, 3)] + 0.01 * rng.normal(size=(3, dim))).astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    f = corpus.filter_from_bytemask(mask)
    kk = int(mask.sum()) if metric == "cosine" else k         # cosine: every permitted row, so the NaN row is part of the answer
    res = corpus.search(q, kk, metric, f)
    _half_ran(ctx)
    for i in range(3):
        qi = _rq(q[i])
        m = res.counts[i]
        assert m == kk
        assert_valid_topk(res.rows[i, :m], res.dist[i, :m], _ref_all(metric, x, qi), kk, TOL, candidates=np.flatnonzero(mask))
        oidx, odist = oracle.filtered_topk(metric, x, qi, kk, mask=mask)
        np.testing.assert_allclose(res.dist[i, :m], odist, rtol=TOL, atol=TOL)
        if metric == "cosine":
            assert res.rows[i, m - 1] == 5 and math.isnan(res.dist[i, m - 1]) and not np.isnan(res.dist[i, :m - 1]).any()
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 5. queries are rounded to binary16, ties to even
# ---------------------------------------------------------------------------------------------
ROUNDING = [([1.0, 1.0009765625], 1.0004, 0),                # without rounding: row 0 at 0.0004
            ([1.0, 1.0009765625], 1.00048828125, 0),          # the tie: to even
            ([1.0009765625, 1.001953125], 1.00146484375, 1)]  # the tie above it: to even is up


def test_query_rounding(ctx, oracle):
    import torch
    import vsrbac
    dev = torch.device("cuda", 0)
    for rows, q, want_row in ROUNDING:
        corpus = ctx.load_corpus_half(np.asarray(rows, dtype=np.float16)[:, None])
        res = corpus.search([[q]], 1, "l2")
        _half_ran(ctx)
        assert res.counts[0] == 1 and res.rows[0, 0] == want_row and res.dist[0, 0] == 0.0, (rows, q, res.rows[0], res.dist[0])
        o = _device_outputs(torch, dev, 1, 1)
        d_q = torch.tensor([[q]], dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        corpus.search_device(_p(d_q), 1, 1, "l2", None, _p(o.blk), _p(o.doc), _p(o.row), _p(o.dist), _p(o.cnt))
        ctx.synchronize()
        _half_ran(ctx)
        got = _as_result(o)
        assert got.counts[0] == 1 and got.rows[0, 0] == want_row and got.dist[0, 0] == 0.0
        corpus.free()
    # two queries per call take the staging kernel's rounding instead of the scan's own
    corpus = ctx.load_corpus_half(np.asarray([1.0, 1.0009765625], dtype=np.float16)[:, None])
    res = corpus.search([[1.0004], [1.0006]], 1, "l2")
    _half_ran(ctx)
    assert res.rows[:, 0].tolist() == [0, 1] and (res.dist[:, 0] == 0.0).all()
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.search([[65520.0]], 1, "l2")
    assert e.value.status == 1 and str(e.value).endswith("is out of range for type halfvec"), str(e.value)
    res = corpus.search([[65519.0]], 1, "l2")                 # just below: rounds to the largest finite half, 65504
    idx, dist = oracle.filtered_topk("l2", np.asarray([[1.0], [1.0009765625]], dtype=np.float32), [65504.0], 1)
    assert res.rows[0, 0] == idx[0] and res.dist[0, 0] == np.float32(dist[0]) == np.float32(65503.0)
    # the one-launch path reads the caller's query itself (no staging kernel): the scan kernel rounds it
    wide = ctx.load_corpus_half(np.repeat(np.asarray([1.0, 1.0009765625], dtype=np.float16)[:, None], 8, axis=1))
    res = wide.search([[1.0004] * 8], 1, "l2")
    _half_ran(ctx, fused=True)
    assert res.rows[0, 0] == 0 and res.dist[0, 0] == 0.0
    res = wide.search([[1.0006] * 8], 1, "l2")
    assert res.rows[0, 0] == 1 and res.dist[0, 0] == 0.0
    wide.free()
    with pytest.raises(vsrbac.VsrError) as e:
        ctx.load_corpus_half(np.asarray([[1.0, -70000.0]], dtype=np.float32))
    assert e.value.status == 1 and str(e.value).endswith("is out of range for type halfvec")
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 6. the rows stay fp16 on the device
# ---------------------------------------------------------------------------------------------
def test_residency(ctx):
    rng = np.random.default_rng(6)
    n, dim = 20000, 100
    x = _small_ints(rng, (n, dim))
    half = ctx.load_corpus_half(x.astype(np.float16))
    full = ctx.load_corpus(x)
    bound = n * (2 * 104 + 16)                                # 104 = dim padded to whole 8-element chunks; 16: |row|^2 and slack
    assert half.is_half and not full.is_half
    assert 0 < half.device_bytes() <= bound, (half.device_bytes(), bound)
    assert full.device_bytes() >= 2 * bound, (full.device_bytes(), bound)
    ctx.stats_reset()
    half.search(x[:1], 10, "l2")
    _half_ran(ctx)
    st = ctx.stats()
    assert n * dim * 2 <= st["scan_bytes"][0] < n * dim * 2 + 4096, st["scan_bytes"]       # rows*dim*2 (+ k*12)
    half.free()
    full.free()


# ---------------------------------------------------------------------------------------------
# 7. one query per call: one launch, in-kernel merge
# ---------------------------------------------------------------------------------------------
def test_one_query_per_call_is_one_launch_and_exact(ctx, oracle):
    import torch
    import vsrbac
    rng = np.random.default_rng(77)
    n, dim = 600_000, 128
    base = sift_like(rng, 3000)                               # integers 0..255: exact in binary16, sums exact in fp32 (255^2 * 128 < 2^24)
    x = base[rng.integers(0, len(base), n)]                   # every vector ~200 times: ties break by row id
    blk, doc = _ids(n, 100)
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in range(1, ndocs + 1, 3)] + [(2, 7)] + [(3, int(d)) for d in range(1, ndocs + 1)]
    ur = [(1, 1), (2, 2), (3, 3), (4, 4)]                     # user 2 sees one document (100 rows), user 4 nothing
    corpus.load_rbac(ur, perms)
    q = base[5] + rng.integers(0, 3, dim).astype(np.float32)
    for user, mode in ((1, vsrbac.RANGES), (1, vsrbac.BITMAP), (2, vsrbac.BITMAP), (4, vsrbac.RANGES)):
        f = corpus.filter_for_user(user, mode)
        mask = oracle.user_row_mask(user, ur, perms, doc)
        for k in (1, 100, 256):
            res = corpus.search(q[None, :], k, "l2", [f])
            if mask.any():
                _half_ran(ctx, fused=True)
            _expect_exact(oracle, res, 0, "l2", x, q, k, doc, blk, mask)
    res = corpus.search(q[None, :], 100, "ip")
    _half_ran(ctx, fused=True)
    _expect_exact(oracle, res, 0, "ip", x, q, 100, doc, blk)
    res = corpus.search(q[None, :], 600, "l2")                # k > 512: staging + K1h + K5
    _half_ran(ctx, fused=False)
    _expect_exact(oracle, res, 0, "l2", x, q, 600, doc, blk)
    res = corpus.search(q[None, :], 50, "cosine")
    _half_ran(ctx, fused=False)
    oidx, odist = oracle.filtered_topk("cosine", x, q, 50, doc, blk)
    np.testing.assert_allclose(res.dist[0, :50], odist, rtol=TOL, atol=TOL)
    # device-resident query, asynchronous call, twice in a row (the arrival counters must be back at zero)
    dev = torch.device("cuda", 0)
    k = 100
    o = _device_outputs(torch, dev, 1, k)
    d_q = torch.from_numpy(q[None, :].copy()).to(dev)
    torch.cuda.synchronize()
    f = corpus.filter_for_user(1, vsrbac.RANGES)
    mask = oracle.user_row_mask(1, ur, perms, doc)
    for _ in range(2):
        corpus.search_device(_p(d_q), 1, k, "l2", [f], _p(o.blk), _p(o.doc), _p(o.row), _p(o.dist), _p(o.cnt))
        ctx.synchronize()
        _half_ran(ctx, fused=True)
        _expect_exact(oracle, _as_result(o), 0, "l2", x, q, k, doc, blk, mask)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 8. the device API and shards
# ---------------------------------------------------------------------------------------------
def test_device_exact_and_shard_merge(ctx, oracle):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(88)
    n, dim, k, nq = 5000, 128, 100, 33
    x = _small_ints(rng, (n, dim))
    h = x.astype(np.float16)
    blk, doc = _ids(n, 7)
    q = _small_ints(rng, (nq, dim))
    q = np.where(q >= 8, q + np.float32(0.001), q)            # off the binary16 grid (steps of 2^-7 from 8 on): rounded back
    d_q = torch.from_numpy(q).to(dev)
    rec = ctx.packed_result_bytes(nq, k)
    nk = nq * k
    pack = torch.empty((2 * rec,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.set_screening(True)                                   # no effect on a half corpus
    shards = []
    for r, (lo, hi) in enumerate(((0, 2100), (2100, n))):
        c = ctx.load_corpus_half(h[lo:hi], blk[lo:hi], doc[lo:hi], row_offset=lo)
        view = lambda a, b, dt: pack[r * rec + a:r * rec + b].view(dt)
        keys, pblk = view(0, nk * 8, torch.int64), view(nk * 8, nk * 16, torch.int64)
        pdoc, pdist = view(nk * 16, nk * 20, torch.int32), view(nk * 20, nk * 24, torch.float32)
        cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        n_rerun = c.search_device_exact(_p(d_q), nq, k, "l2", None, _p(pblk), _p(pdoc), None, _p(pdist), _p(cnt), _p(keys))
        assert n_rerun == 0
        _half_ran(ctx)
        ctx.synchronize()
        low = keys.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)
        assert low.min() >= lo and low.max() < hi             # raw keys carry row_offset + the internal row
        shards.append(c)
    o = _device_outputs(torch, dev, nq, k)
    ctx.merge_topk_packed_device(_p(pack), 2, nq, k, _p(o.blk), _p(o.doc), _p(o.dist), None, _p(o.cnt))
    ctx.synchronize()
    whole = ctx.load_corpus_half(h, blk, doc)
    res = whole.search(q, k, "l2")
    _half_ran(ctx)
    np.testing.assert_array_equal(o.cnt.cpu().numpy(), res.counts)
    np.testing.assert_array_equal(o.blk.cpu().numpy(), res.block_ids)
    np.testing.assert_array_equal(o.doc.cpu().numpy(), res.doc_ids)
    np.testing.assert_array_equal(o.dist.cpu().numpy().view(np.uint32), res.dist.view(np.uint32))
    for i in range(0, nq, 6):
        _expect_exact(oracle, res, i, "l2", x, q[i], k, doc, blk)
    whole.free()
    for c in shards:
        c.free()


# ---------------------------------------------------------------------------------------------
# 9. edges
# ---------------------------------------------------------------------------------------------
def test_nonfinite_rows_sort_last(ctx, oracle):
    h = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [np.inf, 0, 0, 0], [np.nan, 1, 0, 0]],
                   dtype=np.float16)
    x = h.astype(np.float32)
    corpus = ctx.load_corpus_half(h)
    res = corpus.search([[1, 0, 0, 0]], 7, "cosine")
    _half_ran(ctx)
    idx, dist = oracle.filtered_topk("cosine", x, [1, 0, 0, 0], 7)
    np.testing.assert_array_equal(res.rows[0], idx)
    assert np.isnan(res.dist[0, 3:]).all() and np.isnan(dist[3:]).all()       # zero rows, Inf / Inf and NaN: all NaN, last
    np.testing.assert_allclose(res.dist[0, :3], dist[:3], atol=1e-6)
    res = corpus.search([[1, 0, 0, 0]], 7, "l2")
    idx, dist = oracle.filtered_topk("l2", x, [1, 0, 0, 0], 7)
    np.testing.assert_array_equal(res.rows[0], idx)
    np.testing.assert_array_equal(res.dist[0], dist.astype(np.float32))       # ..., +Inf, NaN
    assert np.isposinf(res.dist[0, 5]) and np.isnan(res.dist[0, 6])
    corpus.free()


def test_unsorted_identities_are_reordered(ctx, oracle):
    rng = np.random.default_rng(8)
    n = 3000
    x = _small_ints(rng, (n, 36))                             # 36: the permuting loader also pads the rows to 40 halves
    doc = rng.integers(1, 40, n).astype(np.int32)
    blk = rng.permutation(n).astype(np.int64)
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    res = corpus.search(x[:4], 64, "l2")
    _half_ran(ctx)
    for i in range(4):
        _expect_exact(oracle, res, i, "l2", x, x[i], 64, doc, blk)
    corpus.free()


def test_sizes_at_the_edges(ctx, oracle):
    import vsrbac
    rng = np.random.default_rng(9)
    empty = ctx.load_corpus_half(np.zeros((0, 8), dtype=np.float16))
    assert empty.is_half
    res = empty.search(np.zeros((1, 8), np.float32), 5, "l2")
    assert res.counts[0] == 0 and (res.block_ids[0] == -1).all() and np.isposinf(res.dist[0]).all()
    empty.free()
    n, dim = 3000, 24
    x = _small_ints(rng, (n, dim))
    blk, doc = _ids(n, 10)
    corpus = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    few = ctx.load_corpus_half(x[:37].astype(np.float16), blk[:37], doc[:37])
    for nq in (1, 3):
        res = few.search(x[:nq], 100, "l2")                   # k > n
        _half_ran(ctx)
        for i in range(nq):
            _expect_exact(oracle, res, i, "l2", x[:37], x[i], 100, doc[:37], blk[:37])
        res = corpus.search(x[:nq], 2048, "l1")               # k = VSR_MAX_K
        _half_ran(ctx)
        for i in range(nq):
            _expect_exact(oracle, res, i, "l1", x, x[i], 2048, doc, blk)
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.search(x[:1], 2049, "l2")
    assert e.value.status == 6
    few.free()
    corpus.free()


def test_indexes_are_unsupported(ctx):
    import vsrbac
    rng = np.random.default_rng(10)
    n, dim = 500, 16
    x = _small_ints(rng, (n, dim))
    corpus = ctx.load_corpus_half(x.astype(np.float16))
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.load_ivf(x[:4], np.zeros(n, dtype=np.int32))
    assert e.value.status == 6 and "halfvec" in str(e.value)
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.ivf_assign(x[:4])
    assert e.value.status == 6 and "halfvec" in str(e.value)
    for merge in (False, True):
        with pytest.raises(vsrbac.VsrError) as e:
            corpus.build_hnsw(m=8, ef_construction=32, merge_duplicates=merge)
        assert e.value.status == 6 and "halfvec" in str(e.value)
    graph = {"m": 4, "entry": 0, "max_level": 1, "level": np.zeros(n, np.int32), "nbr0": np.full((n, 8), -1, np.int32),
             "tid_count": np.ones(n, np.int32), "tids": np.zeros((n, 10), np.int64), "up_slot": np.full(n, -1, np.int32),
             "up_nbr": np.zeros((1, 1, 4), np.int32)}
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.load_hnsw(graph)
    assert e.value.status == 6 and "halfvec" in str(e.value)
    corpus.free()
