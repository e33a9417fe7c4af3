"""Bit corpora on the GPU (vsr_corpus_load_bit, K1b: vsr_scanb.h): pgvector's type bit under <~> (Hamming) and <%> (Jaccard).

Distances are small integers (Hamming) or one double division of small integers rounded to fp32 (Jaccard), so the expected
answer everywhere is the numpy model of tests/bit_model.py -- pinned against pgvector's own regression output by
tests/test_bit_formats.py -- and row ids, block ids, document ids and fp32 distances are compared bit for bit: nothing here
needs a tolerance.  Every search asserts that the bit instantiation ran (`bit` in vsr_last_scan_kernel)."""
import ctypes
import json
import os

from types import SimpleNamespace

import numpy as np
import pytest

import bit_model
from bit_model import BitModel

pytestmark = pytest.mark.gpu

METRICS = ["hamming", "jaccard"]


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_bit_known_answers.json")) as f:
        return json.load(f)


def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _ids(n, rows_per_doc):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _shuffled_ids(rng, n, n_docs):
    """Caller order unrelated to (document, block) order."""
    return rng.permutation(n).astype(np.int64) + 1, rng.integers(1, n_docs + 1, n).astype(np.int32)


def _bits(rng, shape, density):
    return bit_model.pack(rng.random(shape) < density)


def _bit_ran(ctx):
    name = ctx.last_scan_kernel()
    assert "bit" in name and "K1b" in name, name


def _expect(model, res, qi, dist_row, k, mask=None):
    idx, dist = model.topk(dist_row, k, mask)
    m = res.counts[qi]
    assert m == idx.size, (m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.block_ids[qi, :m], model.blk[idx])
    np.testing.assert_array_equal(res.doc_ids[qi, :m], model.doc[idx])
    np.testing.assert_array_equal(res.dist[qi, :m], dist)
    assert (res.block_ids[qi, m:] == -1).all() and (res.doc_ids[qi, m:] == -1).all() and (res.rows[qi, m:] == -1).all()
    assert np.isposinf(res.dist[qi, m:]).all()


def _device_outputs(torch, dev, nq, k):
    o = SimpleNamespace(blk=torch.empty((nq, k), dtype=torch.int64, device=dev), doc=torch.empty((nq, k), dtype=torch.int32, device=dev),
                        row=torch.empty((nq, k), dtype=torch.int64, device=dev), dist=torch.empty((nq, k), dtype=torch.float32, device=dev),
                        cnt=torch.empty((nq,), dtype=torch.int32, device=dev), keys=torch.empty((nq, k), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()                                  # the library runs on its own stream
    return o


def _as_result(o):
    return SimpleNamespace(block_ids=o.blk.cpu().numpy(), doc_ids=o.doc.cpu().numpy(), rows=o.row.cpu().numpy(),
                           dist=o.dist.cpu().numpy(), counts=o.cnt.cpu().numpy())


def _rbac(rng, doc, n_roles, n_users):
    """Random tables, as tests/test_gpu_halfvec.py builds them."""
    ndocs = int(doc.max())
    perms = sorted({(int(r), int(d)) for r in range(1, n_roles + 1)
                    for d in rng.choice(np.arange(1, ndocs + 1), size=max(1, ndocs // 3), replace=False)})
    ur = sorted({(u, int(r)) for u in range(1, n_users + 1)
                 for r in rng.choice(np.arange(1, n_roles + 1), size=int(rng.integers(1, 3)), replace=False)})
    return ur, perms


# ---------------------------------------------------------------------------------------------
# 1. pgvector's known answers
# ---------------------------------------------------------------------------------------------
def test_known_answers(ctx, known):
    """Every statement of bit.out through the pair function, exact float8; every pair with at least one bit also as a one-row
    corpus (the b operand) searched with the a operand, k = 1.  A length mismatch keeps pgvector's text; for a search the
    column is the operator's left operand, so its length comes first."""
    import vsrbac
    from vsrbac import formats
    for c in known["distances"]:
        a, b = formats.bit_from_text(c["a"]), formats.bit_from_text(c["b"])
        metric = "hamming" if c["fn"] == "hamming_distance" else "jaccard"
        if "error" in c:
            with pytest.raises(vsrbac.VsrError) as e:
                ctx.bit_pair_distances(metric, a[None, :], b[None, :])
            assert e.value.status == 2 and str(e.value) == c["error"]
            corpus = ctx.load_corpus_bit(a[None, :])
            with pytest.raises(vsrbac.VsrError) as e:
                corpus.search_bit(bit_model.pack(b), 1, metric, dim=b.size)
            assert e.value.status == 2 and str(e.value) == c["error"]     # (a is the column here: the same order as the statement)
            corpus.free()
            continue
        got = ctx.bit_pair_distances(metric, a[None, :], b[None, :])
        assert got.dtype == np.float64 and got.shape == (1,) and got[0] == c["expected"], (c["fn"], a.size, got)
        got = ctx.bit_pair_distances(metric, np.stack([a, a]), b)         # broadcast form
        assert (got == c["expected"]).all()
        if a.size == 0:
            continue
        corpus = ctx.load_corpus_bit(b[None, :])
        assert corpus.is_bit and corpus.dim == a.size
        res = corpus.search_bit(a[None, :], 1, metric)
        _bit_ran(ctx)
        assert res.counts[0] == 1 and res.rows[0, 0] == 0 and res.dist[0, 0] == np.float32(c["expected"]), (c["fn"], a.size, res.dist)
        corpus.free()


# ---------------------------------------------------------------------------------------------
# 2. every row shape
# ---------------------------------------------------------------------------------------------
# (at and around every byte and 128-bit chunk boundary; 1024 | 4099: LPR 16 | 32 of scan_shape(RowFormat::BIT, dim); 64000: the
# widest column, 500 chunks, the streaming instantiation)
SHAPE_DIMS = [1, 7, 8, 9, 64, 127, 128, 129, 255, 1000, 1024, 4099, 64000]


@pytest.mark.parametrize("dim", SHAPE_DIMS)
def test_row_shapes(ctx, dim):
    rng = np.random.default_rng(1000 + dim)
    n, k = (300 if dim == 64000 else 3000), 10
    blk, doc = _ids(n, 7)
    for density in (0.5, 0.02):                               # 0.02: many empty intersections, Jaccard's ab == 0 branch
        rows = _bits(rng, (n, dim), density)
        q = _bits(rng, (5, dim), density)
        model = BitModel(rows, dim, doc, blk)
        corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
        dirty = ctx.load_corpus_bit(bit_model.set_pad_bits(rows, dim), dim, blk, doc)      # every pad bit set: ignored
        for metric in METRICS:
            want = model.distances(metric, q)
            if metric == "jaccard" and density < 0.1 and 7 <= dim <= 255:
                assert (want == 1.0).any()
            for nq in (1, 5):
                res = corpus.search_bit(q[:nq], k, metric)
                _bit_ran(ctx)
                again = dirty.search_bit(bit_model.set_pad_bits(q[:nq], dim), k, metric)
                _bit_ran(ctx)
                for i in range(nq):
                    _expect(model, res, i, want[i], k)
                    _expect(model, again, i, want[i], k)
        corpus.free()
        dirty.free()


# ---------------------------------------------------------------------------------------------
# 3. ties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 100, 2048])
def test_ties_are_broken_by_ids(ctx, k):
    """16 bits: 17 possible Hamming values over 50 000 rows, so the order is decided almost entirely by (document, block) --
    across tiles, workgroups and the selection's merges -- with the caller's order shuffled against it."""
    rng = np.random.default_rng(3)
    n, dim = 50_000, 16
    rows = _bits(rng, (n, dim), 0.5)
    blk, doc = _shuffled_ids(rng, n, 400)
    q = _bits(rng, (5, dim), 0.5)
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    for metric in METRICS:
        want = model.distances(metric, q)
        for nq in (1, 5):
            res = corpus.search_bit(q[:nq], k, metric)
            _bit_ran(ctx)
            for i in range(nq):
                _expect(model, res, i, want[i], k)
    corpus.free()


def test_all_equal_distances_and_k_beyond_n(ctx):
    rng = np.random.default_rng(33)
    n, dim = 50_000, 16
    blk, doc = _shuffled_ids(rng, n, 400)
    zeros = np.zeros((n, 2), dtype=np.uint8)
    model = BitModel(zeros, dim, doc, blk)
    corpus = ctx.load_corpus_bit(zeros, dim, blk, doc)
    for k in (1, 100, 2048):                                  # jaccard('0..0', '0..0') = 1 for every row: the first k by (doc, block)
        res = corpus.search_bit(zeros[:1], k, "jaccard")
        _bit_ran(ctx)
        assert (res.dist[0] == 1.0).all()
        _expect(model, res, 0, np.ones(n), k)
    corpus.free()
    few_rows = _bits(rng, (37, dim), 0.5)
    few = ctx.load_corpus_bit(few_rows, dim, blk[:37], doc[:37])
    fm = BitModel(few_rows, dim, doc[:37], blk[:37])
    q = _bits(rng, (3, dim), 0.5)
    for metric in METRICS:
        want = fm.distances(metric, q)
        for nq in (1, 3):
            res = few.search_bit(q[:nq], 100, metric)         # k > n: count n, the rest -1 / +Inf
            _bit_ran(ctx)
            for i in range(nq):
                assert res.counts[i] == 37
                _expect(fm, res, i, want[i], 100)
    few.free()


# ---------------------------------------------------------------------------------------------
# 4. filters
# ---------------------------------------------------------------------------------------------
def test_filters(ctx):
    import vsrbac
    rng = np.random.default_rng(4)
    n, dim, k = 40_000, 128, 100
    rows = _bits(rng, (n, dim), 0.5)
    blk, doc = _ids(n, 50)
    ur, perms = _rbac(rng, doc, 5, 9)
    ur = ur + [(10, 6), (11, 7)]
    perms = perms + [(6, 3)]                                  # user 10: one document, 50 rows < k; user 11: a role without permissions
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    corpus.load_rbac(ur, perms)
    q = _bits(rng, (8, dim), 0.5)
    bytemask = rng.random(n) < 0.3
    docs = np.arange(5, 400, 3, dtype=np.int32)
    user_mask = {u: bit_model.user_row_mask(u, ur, perms, doc) for u in range(1, 12)}
    assert user_mask[10].sum() == 50 and not user_mask[11].any()
    role_mask = np.isin(doc, [d for r, d in perms if r in (2, 4)])
    cases = [
        ([corpus.filter_for_user(u, vsrbac.RANGES) for u in (1, 2, 3, 4, 5, 6, 7, 8)], [user_mask[u] for u in (1, 2, 3, 4, 5, 6, 7, 8)]),
        ([corpus.filter_for_user(u, vsrbac.BITMAP) for u in (1, 2, 3, 4, 5, 6, 7, 8)], [user_mask[u] for u in (1, 2, 3, 4, 5, 6, 7, 8)]),
        ([corpus.filter_for_roles([2, 4], m) for m in (vsrbac.RANGES, vsrbac.BITMAP)] * 4, [role_mask] * 8),
        ([corpus.filter_from_bytemask(bytemask)] * 8, [bytemask] * 8),
        ([corpus.filter_from_documents(docs)] * 4 + [corpus.filter_from_documents(docs, user_id=3)] * 4,
         [np.isin(doc, docs)] * 4 + [np.isin(doc, docs) & user_mask[3]] * 4),
        # fewer than k rows, none at all, and no filter, mixed into one call
        ([corpus.filter_for_user(10, vsrbac.RANGES), corpus.filter_for_user(11, vsrbac.RANGES), None, corpus.filter_for_user(1, vsrbac.BITMAP),
          corpus.filter_for_user(10, vsrbac.BITMAP), corpus.filter_for_user(11, vsrbac.BITMAP), None, corpus.filter_from_bytemask(bytemask)],
         [user_mask[10], user_mask[11], None, user_mask[1], user_mask[10], user_mask[11], None, bytemask]),
    ]
    for metric in METRICS:
        want = model.distances(metric, q)
        for filters, masks in cases:
            res = corpus.search_bit(q, k, metric, filters)
            _bit_ran(ctx)
            assert (res.counts >= 0).all()
            for i in range(8):
                _expect(model, res, i, want[i], k, masks[i])
            one = corpus.search_bit(q[1:2], k, metric, filters[1:2])          # one query per call
            if masks[1] is None or masks[1].any():                              # (an empty filter: nothing is launched)
                _bit_ran(ctx)
            _expect(model, one, 0, want[1], k, masks[1])
        # a filter that admits fewer than k rows: a partially filled result, -1 / +Inf behind it (checked by _expect), in the
        # mixed call above and alone, in both modes
        assert 0 < res.counts[0] == 50 < k and 0 < res.counts[4] == 50 < k and res.counts[1] == 0 and res.counts[5] == 0
        for i in (0, 4):
            one = corpus.search_bit(q[i:i + 1], k, metric, cases[-1][0][i:i + 1])
            _bit_ran(ctx)
            assert 0 < one.counts[0] == 50 < k
            _expect(model, one, 0, want[i], k, user_mask[10])
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 5. shared passes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [128, 1000])
def test_shared_passes(ctx, dim, metric):
    """300 queries of 30 users over 6 roles: several users per permission class, so the class passes are shared."""
    import vsrbac
    rng = np.random.default_rng(5)
    n, k, nq = 60_000, 100, 300
    rows = _bits(rng, (n, dim), 0.5)
    blk, doc = _ids(n, 100)
    ur, perms = _rbac(rng, doc, 6, 30)
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    corpus.load_rbac(ur, perms)
    q = _bits(rng, (nq, dim), 0.5)
    users = rng.integers(1, 31, nq)
    masks = {u: bit_model.user_row_mask(u, ur, perms, doc) for u in range(1, 31)}
    want = model.distances(metric, q)
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        filters = [corpus.filter_for_user(int(u), mode) for u in users]
        ctx.stats_reset()
        ctx.profiling(True)
        res = corpus.search_bit(q, k, metric, filters)
        st = ctx.stats()
        ctx.profiling(False)
        _bit_ran(ctx)
        assert st["scan_launches"][1] > 0 and st["scan_launches"][0] == 0, st["scan_launches"]
        assert (res.counts >= 0).all()
        for i in range(nq):
            _expect(model, res, i, want[i], k, masks[int(users[i])])
    corpus.free()


def test_scan_bytes_count_packed_rows(ctx):
    rng = np.random.default_rng(55)
    n, dim = 20_000, 100
    rows = _bits(rng, (n, dim), 0.5)
    corpus = ctx.load_corpus_bit(rows, dim)
    assert 0 < corpus.device_bytes() <= n * (16 + 4) + 2048   # one 16-byte chunk and one popcount per row
    ctx.stats_reset()
    corpus.search_bit(rows[:1], 10, "hamming")
    _bit_ran(ctx)
    st = ctx.stats()
    assert n * 13 <= st["scan_bytes"][0] < n * 13 + 4096, st["scan_bytes"]
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 6. the device API, sessions and shards
# ---------------------------------------------------------------------------------------------
def test_device_api_unaligned_queries_and_sessions(ctx):
    import torch
    import vsrbac
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    n, dim, k, nq = 5000, 100, 40, 9
    rows = _bits(rng, (n, dim), 0.5)
    blk, doc = _shuffled_ids(rng, n, 60)
    q = _bits(rng, (nq, dim), 0.5)
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    buf = torch.zeros((1 + q.size,), dtype=torch.uint8, device=dev)
    buf[1:] = torch.from_numpy(q.ravel().copy()).to(dev)      # the queries start one byte into the allocation
    torch.cuda.synchronize()
    session = vsrbac.Context(0)
    for metric in METRICS:
        want = model.distances(metric, q)
        for sess in (None, session):
            o = _device_outputs(torch, dev, nq, k)
            corpus.search_bit_device(_p(buf, 1), nq, k, metric, None, _p(o.blk), _p(o.doc), _p(o.row), _p(o.dist), _p(o.cnt), _p(o.keys),
                                     session=sess)
            (sess or ctx).synchronize()
            assert "bit" in (sess or ctx).last_scan_kernel()
            got = _as_result(o)
            for i in range(nq):
                _expect(model, got, i, want[i], k)
            keys = o.keys.cpu().numpy().view(np.uint64)
            assert (keys[:, 1:] > keys[:, :-1]).all()         # raw keys: strictly ascending
    session.close()
    corpus.free()


def test_shard_merge_equals_the_single_corpus(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(66)
    n, dim, k, nq = 6000, 24, 100, 33                         # 24 bits: heavy ties across the two shards
    rows = _bits(rng, (n, dim), 0.5)
    blk, doc = _ids(n, 7)
    q = _bits(rng, (nq, dim), 0.5)
    d_q = torch.from_numpy(q.copy()).to(dev)
    rec = ctx.packed_result_bytes(nq, k)
    nk = nq * k
    model = BitModel(rows, dim, doc, blk)
    for metric in METRICS:
        pack = torch.empty((2 * rec,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        shards = []
        for r, (lo, hi) in enumerate(((0, 2500), (2500, n))):
            c = ctx.load_corpus_bit(rows[lo:hi], dim, blk[lo:hi], doc[lo:hi], row_offset=lo)
            view = lambda a, b, dt: pack[r * rec + a:r * rec + b].view(dt)
            keys, pblk = view(0, nk * 8, torch.int64), view(nk * 8, nk * 16, torch.int64)
            pdoc, pdist = view(nk * 16, nk * 20, torch.int32), view(nk * 20, nk * 24, torch.float32)
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            c.search_bit_device(_p(d_q), nq, k, metric, None, _p(pblk), _p(pdoc), None, _p(pdist), _p(cnt), _p(keys))
            ctx.synchronize()
            _bit_ran(ctx)
            low = keys.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)
            assert low.min() >= lo and low.max() < hi         # raw keys carry row_offset + the internal row
            shards.append(c)
        o = _device_outputs(torch, dev, nq, k)
        ctx.merge_topk_packed_device(_p(pack), 2, nq, k, _p(o.blk), _p(o.doc), _p(o.dist), None, _p(o.cnt))
        ctx.synchronize()
        whole = ctx.load_corpus_bit(rows, dim, blk, doc)
        res = whole.search_bit(q, k, metric)
        _bit_ran(ctx)
        np.testing.assert_array_equal(o.cnt.cpu().numpy(), res.counts)
        np.testing.assert_array_equal(o.blk.cpu().numpy(), res.block_ids)
        np.testing.assert_array_equal(o.doc.cpu().numpy(), res.doc_ids)
        np.testing.assert_array_equal(o.dist.cpu().numpy(), res.dist)
        want = model.distances(metric, q)
        for i in range(nq):
            _expect(model, res, i, want[i], k)
        whole.free()
        for c in shards:
            c.free()


# ---------------------------------------------------------------------------------------------
# 7. binary_quantize
# ---------------------------------------------------------------------------------------------
def _quantize_input(rng, n, dim):
    x = rng.normal(size=(n, dim)).astype(np.float32)
    special = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40], dtype=np.float32)
    pick = rng.random((n, dim)) < 0.3
    x[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    return x


@pytest.mark.parametrize("dim", [3, 8, 11, 128, 770])
def test_binary_quantize(ctx, dim):
    rng = np.random.default_rng(7000 + dim)
    x = _quantize_input(rng, 1000, dim)
    got = ctx.binary_quantize(x)
    with np.errstate(invalid="ignore"):
        want = np.packbits(x > 0, axis=1)
    assert got.dtype == np.uint8 and got.shape == (1000, (dim + 7) // 8)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("half", [False, True])
def test_quantized_corpus_searches_like_the_loaded_one(ctx, half):
    import vsrbac
    rng = np.random.default_rng(77)
    n, dim, k = 20_000, 100, 50
    x = _quantize_input(rng, n, dim)
    if half:
        x[np.isnan(x)] = 0.0                                  # (a halfvec column holds no NaN; the fp32 source keeps every special, NaN too)
        with np.errstate(over="ignore"):
            x = x.astype(np.float16).astype(np.float32)       # subnormal floats flush to +-0 halves: positive exactly when the half is
    blk, doc = _shuffled_ids(rng, n, 200)
    src = ctx.load_corpus_half(x.astype(np.float16), blk, doc) if half else ctx.load_corpus(x, blk, doc)
    packed = bit_model.binary_quantize(x)
    quant = src.binary_quantize()
    loaded = ctx.load_corpus_bit(packed, dim, blk, doc)
    assert quant.is_bit and not src.is_bit and quant.dim == dim and quant.n == n
    q = ctx.binary_quantize(_quantize_input(rng, 7, dim))
    model = BitModel(packed, dim, doc, blk)
    want = model.distances("hamming", q)
    a = quant.search_bit(q, k, "hamming")
    _bit_ran(ctx)
    b = loaded.search_bit(q, k, "hamming")
    _bit_ran(ctx)
    for i in range(7):
        _expect(model, a, i, want[i], k)
        _expect(model, b, i, want[i], k)
    with pytest.raises(vsrbac.VsrError) as e:                 # RBAC tables are not inherited
        quant.filter_for_user(1)
    assert e.value.status == 7
    ur, perms = _rbac(rng, doc, 4, 6)
    for c in (quant, loaded):
        c.load_rbac(ur, perms)
    users = [1, 2, 3, 4, 5, 6, 1]
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        a = quant.search_bit(q, k, "hamming", [quant.filter_for_user(u, mode) for u in users])
        _bit_ran(ctx)
        b = loaded.search_bit(q, k, "hamming", [loaded.filter_for_user(u, mode) for u in users])
        _bit_ran(ctx)
        for i, u in enumerate(users):
            mask = bit_model.user_row_mask(u, ur, perms, doc)
            _expect(model, a, i, want[i], k, mask)
            _expect(model, b, i, want[i], k, mask)
    with pytest.raises(vsrbac.VsrError) as e:
        quant.binary_quantize()
    assert e.value.status == 1
    src.free()                                                # the quantized corpus is independent of its source
    a = quant.search_bit(q[:1], k, "hamming")
    _bit_ran(ctx)
    _expect(model, a, 0, want[0], k)
    quant.free()
    loaded.free()


# ---------------------------------------------------------------------------------------------
# 8. arguments
# ---------------------------------------------------------------------------------------------
def test_arguments(ctx):
    import vsrbac
    lib = vsrbac.load_library()
    rng = np.random.default_rng(8)
    n, dim = 500, 16
    rows = _bits(rng, (n, dim), 0.5)
    h = ctypes.c_void_p()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for bad_dim in (0, 64001, -5):
        assert lib.vsr_corpus_load_bit(ctx._h, ptr(rows), n, bad_dim, None, None, 0, ctypes.byref(h)) == 1
        assert "bit" in lib.vsr_last_error().decode() and not h.value
    assert lib.vsr_corpus_load_bit(ctx._h, None, n, dim, None, None, 0, ctypes.byref(h)) == 1
    assert lib.vsr_corpus_load_bit(ctx._h, ptr(rows), n, dim, None, None, 0, None) == 1
    corpus = ctx.load_corpus_bit(rows, dim)
    blk, dist, cnt = np.zeros(4, np.int64), np.zeros(4, np.float32), np.zeros(1, np.int32)
    args = lambda q, b, d, c, k=4, metric=4: (corpus._h, q, 1, dim, k, metric, None, b, None, None, d, c)
    assert lib.vsr_search_bit(*args(None, ptr(blk), ptr(dist), ptr(cnt))) == 1
    assert lib.vsr_search_bit(*args(ptr(rows), None, ptr(dist), ptr(cnt))) == 1
    assert lib.vsr_search_bit(*args(ptr(rows), ptr(blk), None, ptr(cnt))) == 1
    assert lib.vsr_search_bit(*args(ptr(rows), ptr(blk), ptr(dist), None)) == 1
    assert lib.vsr_search_bit(*args(ptr(rows), ptr(blk), ptr(dist), ptr(cnt))) == 0 and cnt[0] == 4
    _bit_ran(ctx)
    assert lib.vsr_search_bit(corpus._h, None, 0, dim, 4, 4, None, None, None, None, None, None) == 0      # nq = 0
    assert lib.vsr_search_bit(None, ptr(rows), 1, dim, 4, 4, None, ptr(blk), None, None, ptr(dist), ptr(cnt)) == 1
    res = corpus.search_bit(rows[:0], 3, "hamming")
    assert res.counts.size == 0
    for k, status in ((0, 1), (-1, 1), (2049, 6)):
        with pytest.raises(vsrbac.VsrError) as e:
            corpus.search_bit(rows[:1], k, "hamming")
        assert e.value.status == status
    res = corpus.search_bit(rows[:1], 2048, "hamming")        # k = VSR_MAX_K > n
    _bit_ran(ctx)
    assert res.counts[0] == n
    for metric in (0, 1, 2, 3, 6, -1):
        with pytest.raises(vsrbac.VsrError) as e:
            corpus.search_bit(rows[:1], 5, metric)
        assert e.value.status == 1
    with pytest.raises(vsrbac.VsrError) as e:
        ctx.bit_pair_distances(2, rows[:1], rows[:1], dim)
    assert e.value.status == 1
    x = rng.normal(size=(n, dim)).astype(np.float32)
    full = ctx.load_corpus(x)
    for metric in (4, 5):                                     # the float entry points keep rejecting the bit metrics
        with pytest.raises(vsrbac.VsrError) as e:
            full.search(x[:1], 5, metric)
        assert e.value.status == 1
        with pytest.raises(vsrbac.VsrError) as e:
            ctx.pair_distances(metric, x[:1], x[:1])
        assert e.value.status == 1
    with pytest.raises(vsrbac.VsrError) as e:
        full.search_bit(rows[:1], 5, "hamming")
    assert e.value.status == 1
    assert not full.is_bit and corpus.is_bit and not corpus.is_half
    full.free()
    # a bit corpus has no float search and no index path
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.search(x[:1], 5, "l2")
    assert e.value.status == 6 and "bit" in str(e.value)
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.load_ivf(x[:4], np.zeros(n, dtype=np.int32))
    assert e.value.status == 6 and "bit" in str(e.value)
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.ivf_assign(x[:4])
    assert e.value.status == 6 and "bit" in str(e.value)
    for merge in (False, True):
        with pytest.raises(vsrbac.VsrError) as e:
            corpus.build_hnsw(m=8, ef_construction=32, merge_duplicates=merge)
        assert e.value.status == 6 and "bit" in str(e.value)
    graph = {"m": 4, "entry": 0, "max_level": 1, "level": np.zeros(n, np.int32), "nbr0": np.full((n, 8), -1, np.int32),
             "tid_count": np.ones(n, np.int32), "tids": np.zeros((n, 10), np.int64), "up_slot": np.full(n, -1, np.int32),
             "up_nbr": np.zeros((1, 1, 4), np.int32)}
    with pytest.raises(vsrbac.VsrError) as e:
        corpus.load_hnsw(graph)
    assert e.value.status == 6 and "bit" in str(e.value)
    empty = ctx.load_corpus_bit(rows[:0], dim)
    res = empty.search_bit(rows[:1], 5, "jaccard")            # (no rows: nothing is launched, so no kernel to name)
    assert res.counts[0] == 0 and (res.block_ids[0] == -1).all() and np.isposinf(res.dist[0]).all()
    empty.free()
    corpus.free()
