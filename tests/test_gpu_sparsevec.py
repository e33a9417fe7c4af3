"""Sparse corpora on the GPU (vsr_corpus_load_sparse, K1s: vsr_scans.h): pgvector's type sparsevec under <->, <#>, <=>, <+>.

The expected answer everywhere is the numpy model of tests/sparse_model.py, pinned against pgvector's own regression output by
tests/test_sparse_model_cpu.py.  Integer-valued cases use values in -8..8: with at most 32 000 union entries every fp32 sum stays
below 2^24, so any summation order is exact and row ids and fp32 distances are compared for EQUALITY.  Real-valued cases use the
README's 1e-4.  Every search asserts that the sparse instantiation ran (`K1s` in vsr_last_scan_kernel)."""
import ctypes
import json
import math
import os

from types import SimpleNamespace

import numpy as np
import pytest

import sparse_model
from sparse_model import SparseModel

pytestmark = pytest.mark.gpu

METRICS = sparse_model.METRICS
FN = {"l2_distance": "l2", "<->": "l2", "inner_product": "ip", "<#>": "ip", "cosine_distance": "cosine", "<=>": "cosine",
      "l1_distance": "l1", "<+>": "l1"}
HASH_MUL = 2654435761                                         # SPARSE_HASH_MUL, vsr_device.h
LDS_BUDGET = 72 * 1024                                        # SCAN_LDS_BUDGET


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_sparsevec_known_answers.json")) as f:
        return json.load(f)


def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _ids(n, rows_per_doc):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _shuffled_ids(rng, n, n_docs):
    """Caller order unrelated to (document, block) order."""
    return rng.permutation(n).astype(np.int64) + 1, rng.integers(1, n_docs + 1, n).astype(np.int32)


def _int_values(rng, m):
    return (rng.integers(1, 9, m) * rng.choice([-1, 1], m)).astype(np.float32)


def _real_values(rng, m):
    v = rng.normal(size=m).astype(np.float32)
    v[v == 0] = 1
    return v


def _indices(rng, dim, nnz, pool=None):
    """At most nnz distinct ascending indices below dim (from `pool` when given); now and then the top of the range."""
    nnz = min(nnz, dim if pool is None else pool.size)
    if nnz == 0:
        return np.zeros(0, np.int32)
    if pool is not None:
        ix = rng.choice(pool, size=nnz, replace=False)
    elif dim <= 4 * nnz:
        ix = rng.choice(dim, size=nnz, replace=False)
    else:
        ix = rng.integers(0, dim, nnz)
    if pool is None and rng.random() < 0.2:
        ix[0] = dim - 1
    return np.unique(ix).astype(np.int32)


def _rows(rng, n, dim, nnz_lo, nnz_hi, values=_int_values, pool=None):
    rows = []
    for _ in range(n):
        ix = _indices(rng, dim, int(rng.integers(nnz_lo, nnz_hi + 1)), pool)
        rows.append((ix, values(rng, ix.size)))
    return rows


def _sparse_ran(ctx, *parts):
    name = ctx.last_scan_kernel()
    assert "scans_kernel" in name and "K1s" in name, name
    for p in parts:
        assert p in name, (p, name)
    return name


def _expect(model, res, qi, dist, k, mask=None):
    idx, d = model.topk(dist, k, mask)
    m = res.counts[qi]
    assert m == idx.size, (m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.block_ids[qi, :m], model.blk[idx])
    np.testing.assert_array_equal(res.doc_ids[qi, :m], model.doc[idx])
    np.testing.assert_array_equal(res.dist[qi, :m], d)        # (NaN == NaN here)
    assert (res.block_ids[qi, m:] == -1).all() and (res.doc_ids[qi, m:] == -1).all() and (res.rows[qi, m:] == -1).all()
    assert np.isposinf(res.dist[qi, m:]).all()


def _expect_close(model, res, qi, dist, k):
    """Real-valued data: the distances of the returned rows and the returned distance list, within the README's 1e-4."""
    idx, d = model.topk(dist, k)
    m = res.counts[qi]
    assert m == idx.size
    assert len(set(res.rows[qi, :m].tolist())) == m
    np.testing.assert_allclose(res.dist[qi, :m], dist[res.rows[qi, :m]], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(res.dist[qi, :m], d, rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(res.block_ids[qi, :m], model.blk[res.rows[qi, :m]])


def _load(ctx, rows, dim, blk=None, doc=None, **kw):
    indptr, indices, values = sparse_model.csr(rows)
    corpus = ctx.load_corpus_sparse(indptr, indices, values, dim, blk, doc, **kw)
    assert corpus.is_sparse and not corpus.is_bit and not corpus.is_half
    return corpus, SparseModel(indptr, indices, values, dim, doc, blk)


def _search(corpus, queries, k, metric, filters=None):
    indptr, indices, values = sparse_model.csr(queries)
    return corpus.search_sparse(indptr, k, metric, filters, indices=indices, values=values)


def _rbac(rng, doc, n_roles, n_users):
    ndocs = int(doc.max())
    perms = sorted({(int(r), int(d)) for r in range(1, n_roles + 1)
                    for d in rng.choice(np.arange(1, ndocs + 1), size=max(1, ndocs // 3), replace=False)})
    ur = sorted({(u, int(r)) for u in range(1, n_users + 1)
                 for r in rng.choice(np.arange(1, n_roles + 1), size=int(rng.integers(1, 3)), replace=False)})
    return ur, perms


def _device_outputs(torch, dev, nq, k):
    o = SimpleNamespace(blk=torch.empty((nq, k), dtype=torch.int64, device=dev), doc=torch.empty((nq, k), dtype=torch.int32, device=dev),
                        row=torch.empty((nq, k), dtype=torch.int64, device=dev), dist=torch.empty((nq, k), dtype=torch.float32, device=dev),
                        cnt=torch.empty((nq,), dtype=torch.int32, device=dev), keys=torch.empty((nq, k), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()                                  # the library runs on its own stream
    return o


def _as_result(o):
    return SimpleNamespace(block_ids=o.blk.cpu().numpy(), doc_ids=o.doc.cpu().numpy(), rows=o.row.cpu().numpy(),
                           dist=o.dist.cpu().numpy(), counts=o.cnt.cpu().numpy())


def _device_csr(torch, dev, queries):
    indptr, indices, values = sparse_model.csr(queries)
    pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)      # (an empty tensor has no address)
    d = SimpleNamespace(ptr=torch.from_numpy(indptr.copy()).to(dev), idx=torch.from_numpy(pad(indices).copy()).to(dev),
                        val=torch.from_numpy(pad(values).copy()).to(dev), max_nnz=int(np.diff(indptr).max()) if len(queries) else 0)
    torch.cuda.synchronize()
    return d


def _table_in_lds(nnz, k):
    """vsr_device.h restated: scan_cap_for_rw(k, 64), sparse_slots_for_nnz, scans_lds_bytes(1, cap, slots) <= SCAN_LDS_BUDGET."""
    cap = 512
    while cap < 2 * k + 512:
        cap *= 2
    slots = 2
    while slots < 2 * nnz:
        slots *= 2
    return cap * 8 + 16 + slots * 8 + 12 + 16 <= LDS_BUDGET


# ---------------------------------------------------------------------------------------------
# 1. pgvector's known answers
# ---------------------------------------------------------------------------------------------
def _want(c):
    v = float(c["expected"].replace("Infinity", "inf"))
    return -v if c["fn"] == "inner_product" else v


def test_known_answers_pairs(ctx, known):
    import vsrbac
    from vsrbac import formats
    for c in known["distances"]:
        ai, ax, da = formats.sparsevec_from_text(c["a"])
        bi, bx, db = formats.sparsevec_from_text(c["b"])
        a = (np.array([0, ai.size]), ai, ax, da)
        b = (np.array([0, bi.size]), bi, bx, db)
        if "error" in c:
            with pytest.raises(vsrbac.VsrError) as e:
                ctx.sparse_pair_distances(FN[c["fn"]], a, b)
            assert e.value.status == 2 and str(e.value) == c["error"], c
            continue
        got = float(ctx.sparse_pair_distances(FN[c["fn"]], a, b)[0])
        want = _want(c)
        assert (math.isnan(got) and math.isnan(want)) or got == want, (c, got)


def test_pair_distances_are_pgvectors_bits_on_real_data(ctx):
    rng = np.random.default_rng(11)
    dim, n = 5000, 200
    a = _rows(rng, n, dim, 0, 120, _real_values)
    b = _rows(rng, n, dim, 0, 120, _real_values, pool=np.unique(np.concatenate([r[0] for r in a])))
    pa, pb = sparse_model.csr(a), sparse_model.csr(b)
    for metric in METRICS:
        got = ctx.sparse_pair_distances(metric, pa + (dim,), pb + (dim,))
        want = np.array([sparse_model.pair_distance(metric, a[i][0], a[i][1], b[i][0], b[i][1]) for i in range(n)])
        np.testing.assert_array_equal(got, want)              # float8, bit for bit (NaN == NaN)


def test_known_answers_one_row_corpus(ctx, known):
    from vsrbac import formats
    for c in known["distances"]:
        if "error" in c:
            continue
        ai, ax, dim = formats.sparsevec_from_text(c["a"])
        bi, bx, _ = formats.sparsevec_from_text(c["b"])
        corpus, _ = _load(ctx, [(ai, ax)], dim)
        res = _search(corpus, [(bi, bx)], 1, FN[c["fn"]])
        _sparse_ran(ctx)
        want = np.float32(_want(c))
        assert res.counts[0] == 1 and res.rows[0, 0] == 0
        assert (np.isnan(res.dist[0, 0]) and np.isnan(want)) or res.dist[0, 0] == want, (c, res.dist[0, 0])
        corpus.free()


# ---------------------------------------------------------------------------------------------
# 2. randomised shapes
# ---------------------------------------------------------------------------------------------
DIMS = [1, 2, 7, 300, 30522, 1_000_000_000]


@pytest.mark.parametrize("seed", range(16))
def test_random_shapes(ctx, seed):
    import vsrbac
    rng = np.random.default_rng(1000 + seed)
    dim = DIMS[seed % len(DIMS)]
    n = [1, 63, 64, 65, 700, 5000][(seed // 2) % 6] if seed < 12 else int(rng.integers(1, 5001))
    k = [1, 10, 100, 2048][seed % 4]
    rows = _rows(rng, n, dim, 0, min(dim, 300))
    rows[int(rng.integers(0, n))] = (np.zeros(0, np.int32), np.zeros(0, np.float32))       # an empty row
    if dim >= 16000 and seed % 2:
        ix = np.sort(rng.choice(min(dim, 1 << 20), size=16000, replace=False)).astype(np.int32)
        if dim > 1 << 20:
            ix[-1] = dim - 1
        rows[int(rng.integers(0, n))] = (ix, _int_values(rng, 16000))                      # one row of 16 000
    blk, doc = _shuffled_ids(rng, n, max(1, n // 9))
    corpus, model = _load(ctx, rows, dim, blk, doc)
    ur, perms = _rbac(rng, doc, 4, 6)
    corpus.load_rbac(ur, perms)
    used = np.unique(np.concatenate([r[0] for r in rows]))   # query entries mostly meet row entries

    def some(m):
        ix = _indices(rng, dim, m, used if used.size and rng.random() < 0.7 else None)
        return ix, _int_values(rng, ix.size)

    queries = [(np.zeros(0, np.int32), np.zeros(0, np.float32)), some(1), some(min(dim, 200)), rows[int(rng.integers(0, n))],
               some(min(dim, 40))]
    users = rng.integers(1, 7, len(queries))
    masks = {u: sparse_model.user_row_mask(u, ur, perms, doc) for u in range(1, 7)}
    for metric in METRICS:
        want = [model.distances(metric, qi, qx) for qi, qx in queries]
        res = _search(corpus, queries, k, metric)
        _sparse_ran(ctx)
        for i in range(len(queries)):
            _expect(model, res, i, want[i], k)
        if metric == "cosine":                                # the zero query: every distance NaN, NaN sorts last = id order
            assert np.isnan(res.dist[0, :res.counts[0]]).all()
        for mode in (vsrbac.RANGES, vsrbac.BITMAP):
            res = _search(corpus, queries, k, metric, [corpus.filter_for_user(int(u), mode) for u in users])
            _sparse_ran(ctx)
            for i in range(len(queries)):
                _expect(model, res, i, want[i], k, masks[int(users[i])])
    total, _ = ctx.screening_check()
    assert total == 0
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 3. the LPR classes, real-valued data
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_nnz,lpr", [(4, 4), (40, 16), (200, 64)])
def test_lpr_classes_real_values(ctx, mean_nnz, lpr):
    rng = np.random.default_rng(30 + lpr)
    n, dim, k = 3000, 30522, 50
    pool = rng.choice(dim, size=40 * mean_nnz, replace=False)
    rows = _rows(rng, n, dim, mean_nnz // 2, mean_nnz * 3 // 2, _real_values, pool)
    corpus, model = _load(ctx, rows, dim)
    queries = _rows(rng, 6, dim, 8, 64, _real_values, pool)
    entries = sum((r[0].size + 1) // 2 * 2 for r in rows)
    assert entries * 8 <= corpus.device_bytes() <= entries * 8 + 1024 + (n + 1) * 8 + n * 4
    for metric in METRICS:
        ctx.stats_reset()
        res = _search(corpus, queries[:1], k, metric)
        _sparse_ran(ctx, f"LPR={lpr}", "QI=1", "TAB=lds")
        st = ctx.stats()
        assert entries * 8 <= st["scan_bytes"][0] < entries * 8 + 4096, st["scan_bytes"]     # 8 bytes per stored entry
        _expect_close(model, res, 0, model.distances(metric, *queries[0]), k)
        res = _search(corpus, queries, k, metric)
        _sparse_ran(ctx, f"LPR={lpr}", "QI=4")
        for i, (qi, qx) in enumerate(queries):
            _expect_close(model, res, i, model.distances(metric, qi, qx), k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 4. the query table
# ---------------------------------------------------------------------------------------------
def test_query_indices_in_one_slot_chain(ctx):
    rng = np.random.default_rng(4)
    dim, m = 1_000_000_000, 32
    slots = 2 * m                                             # the table of a 32-entry query
    shift = 32 - int(math.log2(slots))
    cand = np.arange(0, 400_000, dtype=np.uint64)
    home = ((cand * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)
    chain = cand[home == np.uint64(slots - 1)][:m].astype(np.int32)          # all hash to the last slot: the chain wraps
    assert chain.size == m
    others = np.setdiff1d(rng.integers(0, dim, 300).astype(np.int32), chain)
    pool = np.concatenate([chain, others])
    rows = _rows(rng, 500, dim, 0, 60, pool=pool)
    corpus, model = _load(ctx, rows, dim)
    q = (np.sort(chain), _int_values(rng, m))
    for metric in METRICS:
        res = _search(corpus, [q], 20, metric)
        _sparse_ran(ctx, "TAB=lds")
        _expect(model, res, 0, model.distances(metric, *q), 20)
    corpus.free()


def test_table_in_lds_and_in_global_memory(ctx):
    rng = np.random.default_rng(41)
    dim, n, k = 1_000_000, 400, 10
    largest = 2048
    assert _table_in_lds(largest, k) and not _table_in_lds(largest + 1, k)
    pool = rng.choice(dim, size=20000, replace=False)
    rows = _rows(rng, n, dim, 0, 300, pool=pool)
    rows[7] = (np.sort(pool[:16000]).astype(np.int32), _int_values(rng, 16000))
    corpus, model = _load(ctx, rows, dim)
    mk = lambda m: (lambda ix: (ix, _int_values(rng, m)))(np.sort(rng.choice(pool, size=m, replace=False)).astype(np.int32))
    for nnz, where in ((largest, "TAB=lds"), (largest + 1, "TAB=global"), (16000, "TAB=global")):
        q = mk(nnz)
        for metric in METRICS:
            res = _search(corpus, [q], k, metric)
            _sparse_ran(ctx, where, "QI=1")                   # the kernel name shows where the table was read
            _expect(model, res, 0, model.distances(metric, *q), k)
    # several queries per pass from global tables: qmax = QI = 4
    qs = [mk(largest + 1 + i) for i in range(5)]
    for metric in ("l2", "cosine"):
        res = _search(corpus, qs, k, metric)
        _sparse_ran(ctx, "TAB=global", "QI=4")
        for i, q in enumerate(qs):
            _expect(model, res, i, model.distances(metric, *q), k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 5. shared passes
# ---------------------------------------------------------------------------------------------
def test_shared_passes_under_the_tree_rbac(ctx, golden_dir):
    import vsrbac
    with open(os.path.join(golden_dir, "rbac_tree_small.json")) as f:
        fx = json.load(f)
    rng = np.random.default_rng(5)
    rows_per_doc, k, nq = 12, 30, 40
    n = fx["params"]["num_docs"] * rows_per_doc
    dim = 30522
    pool = rng.choice(dim, size=600, replace=False)
    rows = _rows(rng, n, dim, 0, 50, pool=pool)
    blk, doc = _ids(n, rows_per_doc)
    corpus, model = _load(ctx, rows, dim, blk, doc)
    corpus.load_rbac(fx["user_roles"], fx["permissions"])
    queries = [(lambda ix: (ix, _int_values(rng, ix.size)))(_indices(rng, dim, 1 + 3 * i, pool)) for i in range(nq)]   # 1 .. 118 entries
    users = rng.integers(1, fx["num_users"] + 1, nq)
    masks = {int(u): sparse_model.user_row_mask(int(u), fx["user_roles"], fx["permissions"], doc) for u in set(users.tolist())}
    for metric in METRICS:
        want = [model.distances(metric, qi, qx) for qi, qx in queries]
        for mode in (vsrbac.RANGES, vsrbac.BITMAP):
            filters = [corpus.filter_for_user(int(u), mode) for u in users]
            ctx.stats_reset()
            ctx.profiling(True)
            res = _search(corpus, queries, k, metric, filters)
            st = ctx.stats()
            ctx.profiling(False)
            _sparse_ran(ctx, "QI=4")                          # qmax > 1: passes shared by several queries
            assert st["scan_launches"][1] > 0 and st["scan_launches"][0] == 0, st["scan_launches"]
            for i in range(nq):
                _expect(model, res, i, want[i], k, masks[int(users[i])])
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 6. ties, 7. overflow, 8. near-duplicates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 100, 2048])
def test_ties_are_broken_by_ids(ctx, k):
    rng = np.random.default_rng(6)
    n, dim = 3000, 1000
    row = (np.array([3, 500, 999], np.int32), np.array([1, -2, 3], np.float32))
    blk, doc = _shuffled_ids(rng, n, 40)
    corpus, model = _load(ctx, [row] * n, dim, blk, doc)
    q = (np.array([3, 4], np.int32), np.array([2, 5], np.float32))
    for metric in METRICS:
        res = _search(corpus, [q], k, metric)
        _sparse_ran(ctx)
        _expect(model, res, 0, model.distances(metric, *q), k)
        assert len(set(res.dist[0, :res.counts[0]].tolist())) == 1
    corpus.free()


@pytest.mark.parametrize("k", [10, 2048])
def test_overflow_every_row_nearer_than_the_last(ctx, k):
    """20 000 rows in scan order, each nearer than the one before: every row passes the running threshold, so every workgroup
    fills its candidate list, votes and compacts."""
    n, dim = 20_000, 8
    rows = [(np.array([2], np.int32), np.array([float(r + 1)], np.float32)) for r in range(n)]
    corpus, model = _load(ctx, rows, dim)
    for metric, q in (("ip", (np.array([2], np.int32), np.array([1.0], np.float32))),
                      ("l1", (np.array([2], np.int32), np.array([30000.0], np.float32)))):
        d = model.distances(metric, *q)
        assert (np.diff(d) < 0).all()
        for budget in (1, 0):                                 # one workgroup walks every tile; then the default launch
            ctx.tune(block_budget=budget)
            res = _search(corpus, [q], k, metric)
            _sparse_ran(ctx)
            _expect(model, res, 0, d, k)
    ctx.tune(block_budget=0)
    corpus.free()


def test_near_duplicates_have_no_cancellation(ctx):
    rng = np.random.default_rng(8)
    n, dim, k = 1500, 30522, 5
    rows = _rows(rng, n, dim, 60, 200, lambda r, m: (_real_values(r, m) * np.float32(100)).astype(np.float32))
    corpus, model = _load(ctx, rows, dim)
    pick = rng.integers(0, n, 24)
    for metric in ("l2", "l1"):
        res = _search(corpus, [rows[i] for i in pick], k, metric)
        _sparse_ran(ctx)
        assert not np.isnan(res.dist).any()
        for j, i in enumerate(pick):
            qn = float(np.sqrt((rows[i][1].astype(np.float64) ** 2).sum()))
            assert res.rows[j, 0] == i and 0 <= res.dist[j, 0] <= 1e-6 * qn, (metric, i, res.dist[j, 0], qn)
            _expect_close(model, res, j, model.distances(metric, *rows[i]), k)
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 9. the device API, sessions and shards
# ---------------------------------------------------------------------------------------------
def test_device_api_two_sessions_in_flight(ctx):
    import torch
    import vsrbac
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    n, dim, k, nq = 4000, 30522, 40, 9
    pool = rng.choice(dim, size=800, replace=False)
    rows = _rows(rng, n, dim, 0, 80, pool=pool)
    blk, doc = _shuffled_ids(rng, n, 60)
    corpus, model = _load(ctx, rows, dim, blk, doc)
    queries = _rows(rng, nq, dim, 0, 50, pool=pool)
    dq = _device_csr(torch, dev, queries)
    s1, s2 = vsrbac.Context(0), vsrbac.Context(0)
    for metric in METRICS:
        want = [model.distances(metric, qi, qx) for qi, qx in queries]
        outs = []
        for sess in (s1, s2, None):                           # enqueued back to back: two sessions in flight, then the corpus's own
            o = _device_outputs(torch, dev, nq, k)
            corpus.search_sparse_device(_p(dq.ptr), _p(dq.idx), _p(dq.val), nq, dq.max_nnz, k, metric, None, _p(o.blk), _p(o.doc),
                                        _p(o.row), _p(o.dist), _p(o.cnt), _p(o.keys), session=sess)
            outs.append((sess or ctx, o))
        for sess, o in outs:
            sess.synchronize()
            assert "K1s" in sess.last_scan_kernel()
            got = _as_result(o)
            for i in range(nq):
                _expect(model, got, i, want[i], k)
            keys = o.keys.cpu().numpy().view(np.uint64)
            assert (keys[:, 1:] > keys[:, :-1]).all()         # raw keys: strictly ascending
            assert sess.screening_check()[0] == 0
    # a device query longer than max_query_nnz is not staged, and the session's guard word says so
    o = _device_outputs(torch, dev, nq, k)
    corpus.search_sparse_device(_p(dq.ptr), _p(dq.idx), _p(dq.val), nq, dq.max_nnz - 1, k, "l2", None, _p(o.blk), _p(o.doc), _p(o.row),
                                _p(o.dist), _p(o.cnt), None, session=s2)
    with pytest.raises(vsrbac.VsrError) as e:
        s2.screening_check()
    assert e.value.status == vsrbac._ffi.ERR_HIP and "guard" in str(e.value)
    assert s1.screening_check()[0] == 0                       # (per session)
    s1.close()
    s2.close()
    corpus.free()


def test_shard_merge_equals_the_single_corpus(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(99)
    n, dim, k, nq = 5000, 64, 100, 17                         # 64 dimensions, small integers: heavy ties across the two shards
    rows = _rows(rng, n, dim, 0, 6)
    blk, doc = _ids(n, 7)
    queries = _rows(rng, nq, dim, 0, 6)
    dq = _device_csr(torch, dev, queries)
    rec = ctx.packed_result_bytes(nq, k)
    nk = nq * k
    whole, model = _load(ctx, rows, dim, blk, doc)
    for metric in METRICS:
        pack = torch.empty((2 * rec,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        shards = []
        for r, (lo, hi) in enumerate(((0, 2100), (2100, n))):
            c, _ = _load(ctx, rows[lo:hi], dim, blk[lo:hi], doc[lo:hi], row_offset=lo)
            view = lambda a, b, dt: pack[r * rec + a:r * rec + b].view(dt)
            keys, pblk = view(0, nk * 8, torch.int64), view(nk * 8, nk * 16, torch.int64)
            pdoc, pdist = view(nk * 16, nk * 20, torch.int32), view(nk * 20, nk * 24, torch.float32)
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            c.search_sparse_device(_p(dq.ptr), _p(dq.idx), _p(dq.val), nq, dq.max_nnz, k, metric, None, _p(pblk), _p(pdoc), None,
                                   _p(pdist), _p(cnt), _p(keys))
            ctx.synchronize()
            _sparse_ran(ctx)
            low = keys.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)
            assert low.min() >= lo and low.max() < hi         # raw keys carry row_offset + the internal row
            shards.append(c)
        o = _device_outputs(torch, dev, nq, k)
        ctx.merge_topk_packed_device(_p(pack), 2, nq, k, _p(o.blk), _p(o.doc), _p(o.dist), None, _p(o.cnt))
        ctx.synchronize()
        res = _search(whole, queries, k, metric)
        np.testing.assert_array_equal(o.cnt.cpu().numpy(), res.counts)
        np.testing.assert_array_equal(o.blk.cpu().numpy(), res.block_ids)
        np.testing.assert_array_equal(o.doc.cpu().numpy(), res.doc_ids)
        np.testing.assert_array_equal(o.dist.cpu().numpy(), res.dist)
        for i, (qi, qx) in enumerate(queries):
            _expect(model, res, i, model.distances(metric, qi, qx), k)
        for c in shards:
            c.free()
    whole.free()


# ---------------------------------------------------------------------------------------------
# 10. load order
# ---------------------------------------------------------------------------------------------
def test_unsorted_identities_are_reordered(ctx):
    rng = np.random.default_rng(10)
    n, dim = 300, 50
    rows = _rows(rng, n, dim, 0, 20)
    blk = np.arange(n, 0, -1).astype(np.int64)                # descending block ids, documents interleaved
    doc = (np.arange(n) % 7 + 1).astype(np.int32)
    corpus, model = _load(ctx, rows, dim, blk, doc)
    class CsrLike:                                            # any object with .indptr / .indices / .data / .shape
        pass
    m = CsrLike()
    m.indptr, m.indices, m.data = sparse_model.csr(rows)
    m.shape = (n, dim)
    again = ctx.load_corpus_sparse(m, block_ids=blk, doc_ids=doc)
    qs = CsrLike()
    qs.indptr, qs.indices, qs.data = sparse_model.csr(rows[:3])
    qs.shape = (3, dim)
    for metric in METRICS:
        for c, res in ((corpus, _search(corpus, rows[:3], n, metric)), (again, again.search_sparse(qs, n, metric))):
            for i in range(3):
                _expect(model, res, i, model.distances(metric, *rows[i]), n)       # every row, in (distance, document, block) order
    again.free()
    corpus.free()


# ---------------------------------------------------------------------------------------------
# 11. arguments
# ---------------------------------------------------------------------------------------------
def _raises(status, text, fn, *a, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError) as e:
        fn(*a, **kw)
    assert e.value.status == status and text in str(e.value), (status, text, e.value.status, str(e.value))


def test_arguments(ctx):
    import vsrbac
    from vsrbac import _ffi
    INV, DIMM, UNS = _ffi.ERR_INVALID, _ffi.ERR_DIM_MISMATCH, _ffi.ERR_UNSUPPORTED
    i32, f32 = (lambda *a: np.array(a, np.int32)), (lambda *a: np.array(a, np.float32))
    load = lambda ip, ix, vx, dim: ctx.load_corpus_sparse(np.array(ip, np.int64), ix, vx, dim)
    # ---- validation, in pgvector's words (sparsevec.c:53-133, 493-539)
    _raises(INV, "sparsevec must have at least 1 dimension", load, [0, 0], i32(), f32(), 0)
    _raises(INV, "sparsevec cannot have more than 1000000000 dimensions", load, [0, 0], i32(), f32(), 1_000_000_001)
    _raises(INV, "sparsevec cannot have negative number of elements", load, [1, 0], i32(0), f32(1), 5)
    _raises(INV, "sparsevec cannot have more than 16000 non-zero elements", load, [0, 16001], np.arange(16001, dtype=np.int32),
            np.ones(16001, np.float32), 20000)
    _raises(INV, "sparsevec cannot have more elements than dimensions", load, [0, 2], i32(0, 1), f32(1, 1), 1)
    _raises(INV, "sparsevec index out of bounds", load, [0, 1], i32(5), f32(1), 5)
    _raises(INV, "sparsevec index out of bounds", load, [0, 1], i32(-1), f32(1), 5)
    _raises(INV, "sparsevec indices must be in ascending order", load, [0, 2], i32(2, 1), f32(1, 1), 5)
    _raises(INV, "sparsevec indices must not contain duplicates", load, [0, 2], i32(1, 1), f32(1, 1), 5)
    _raises(INV, "NaN not allowed in sparsevec", load, [0, 1], i32(0), f32(np.nan), 5)
    _raises(INV, "infinite value not allowed in sparsevec", load, [0, 1], i32(0), f32(-np.inf), 5)
    _raises(INV, "binary representation of sparsevec cannot contain zero values", load, [0, 1], i32(0), f32(0), 5)
    top = load([0, 0, 2], i32(0, 999_999_999), f32(1, 2), 1_000_000_000)       # {}/d and the widest dimension are legal
    assert top.is_sparse and top.n == 2
    top.free()

    rng = np.random.default_rng(12)
    dim, n = 40, 200
    rows = _rows(rng, n, dim, 0, 10)
    sparse, model = _load(ctx, rows, dim)
    dense_rows = rng.integers(0, 9, (n, dim)).astype(np.float32)
    dense = ctx.load_corpus(dense_rows)
    half = ctx.load_corpus_half(dense_rows.astype(np.float16))
    bits = ctx.load_corpus_bit(dense_rows > 4)
    q = (i32(1, 7), f32(2, -3))
    qp = np.array([0, 2], np.int64)
    # ---- queries are validated as rows are; the dimension message is CheckDims'
    _raises(INV, "sparsevec indices must be in ascending order", sparse.search_sparse, qp, 5, "l2", None, i32(7, 1), f32(1, 1))
    _raises(INV, "binary representation of sparsevec cannot contain zero values", sparse.search_sparse, qp, 5, "l2", None, i32(1, 7), f32(1, 0))
    _raises(INV, "sparsevec index out of bounds", sparse.search_sparse, qp, 5, "l2", None, i32(1, 40), f32(1, 1))
    _raises(DIMM, "different sparsevec dimensions 40 and 41", sparse.search_sparse, qp, 5, "l2", None, q[0], q[1], 41)
    _raises(DIMM, "different sparsevec dimensions 40 and 41", ctx.sparse_pair_distances, "l1", (qp, q[0], q[1], 40), (qp, q[0], q[1], 41))
    _raises(INV, "metric", sparse.search_sparse, qp, 5, 4, None, q[0], q[1])
    _raises(INV, "metric", ctx.sparse_pair_distances, 5, (qp, q[0], q[1], 40), (qp, q[0], q[1], 40))
    _raises(INV, "k must be >= 1", sparse.search_sparse, qp, 0, "l2", None, q[0], q[1])
    _raises(UNS, "VSR_MAX_K", sparse.search_sparse, qp, 2049, "l2", None, q[0], q[1])
    _raises(INV, "max_query_nnz", sparse.search_sparse_device, 8, 8, 8, 1, 16001, 5, "l2", None, 8, 8, 8, 8, 8)
    for other in (dense, half, bits):
        _raises(INV, "not a sparse corpus", other.search_sparse, qp, 5, "l2", None, q[0], q[1], dim)
        _raises(INV, "not a sparse corpus", other.search_sparse_device, 8, 8, 8, 1, 2, 5, "l2", None, 8, 8, 8, 8, 8)
    foreign = dense.filter_from_bytemask(np.ones(n, np.uint8))
    _raises(INV, "belongs to another corpus", sparse.search_sparse, qp, 5, "l2", [foreign], q[0], q[1])
    foreign.free()
    # ---- every other entry point refuses a sparse corpus and names sparsevec
    dq = dense_rows[:1]
    _raises(UNS, "sparsevec", sparse.search, dq, 5, "l2")
    _raises(UNS, "sparsevec", sparse.search_device, 8, 1, 5, "l2", None, 8, 8, 8, 8, 8)
    _raises(UNS, "sparsevec", sparse.search_device_exact, 8, 1, 5, "l2", None, 8, 8, 8, 8, 8)
    _raises(UNS, "sparsevec", sparse.search_bit, dq > 4, 5, "hamming")
    _raises(UNS, "sparsevec", sparse.search_bit_device, 8, 1, 5, "hamming", None, 8, 8, 8, 8, 8)
    _raises(UNS, "sparsevec", sparse.binary_quantize)
    _raises(UNS, "sparsevec", sparse.search_quantized, bits, dq, 5, 10, "l2")
    _raises(UNS, "sparsevec", dense.search_quantized, sparse, dq, 5, 10, "l2")
    _raises(UNS, "sparsevec", sparse.search_quantized_device, bits, 8, 1, 5, 10, "l2", None, 8, 8, 8, 8, 8)
    _raises(UNS, "sparsevec", sparse.load_ivf, np.zeros((2, dim), np.float32), np.zeros(n, np.int32))
    _raises(UNS, "sparsevec", sparse.ivf_assign, np.zeros((2, dim), np.float32))
    _raises(UNS, "sparsevec", sparse.build_hnsw)
    _raises(UNS, "sparsevec", sparse.build_hnsw, merge_duplicates=True)
    graph = dict(m=4, entry=0, level=np.zeros(n, np.int32), nbr0=np.full((n, 8), -1, np.int32), tid_count=np.ones(n, np.int32),
                 tids=np.arange(n, dtype=np.int64), up_slot=np.full(n, -1, np.int32), up_nbr=np.zeros((0, 4), np.int32), max_level=1)
    _raises(UNS, "sparsevec", sparse.load_hnsw, graph)
    # ---- the sparse corpus and the other handles answer as before afterwards
    res = sparse.search_sparse(qp, 5, "l2", None, q[0], q[1])
    _sparse_ran(ctx)
    _expect(model, res, 0, model.distances("l2", *q), 5)
    r = dense.search(dq, 1, "l2")
    assert r.rows[0, 0] == 0 and r.dist[0, 0] == 0 and "K1" in ctx.last_scan_kernel()
    r = half.search(dq, 1, "l2")
    assert r.rows[0, 0] == 0 and r.dist[0, 0] == 0 and "half" in ctx.last_scan_kernel()
    r = bits.search_bit(dense_rows[:1] > 4, 1, "hamming")
    assert r.dist[0, 0] == 0 and "K1b" in ctx.last_scan_kernel()
    assert ctx.screening_check()[0] == 0
    for c in (sparse, dense, half, bits):
        c.free()
