"""HNSW over sparse corpora on the GPU (K4s: vsr_hnsw_load_sparse / build_sparse / search_sparse*, vsr_sparse_norms /
vsr_sparse_l2_normalize).

Exactness: unless said otherwise the data is integer valued -- values in -4 .. 4, non-zero, at most 1000 entries per row and 3000
per query -- so every fp32 sum is exact in any order (<= 3000 x 64 < 2^24) and parity means EQUALITY of rows, fp32 distances and
visited counts.  The reference is the index oracle (oracle.HnswIndex) on the densified rows: its index distance has L2, L1 and the
negated inner product, which is also what the cosine opclass ranks by (unit rows are the caller's business, K4's convention).
Iterative scans are pinned by the numpy walk of tests/hnsw_sparse_model.py (itself pinned to the oracle by
tests/test_hnsw_sparse_cpu.py)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import check_built_graph, same_graph
from hnsw_iterative_model import Stream
from hnsw_sparse_model import (METRICS, SparseGraph, SparseScan, densify, l2_norms, l2_normalize, reported, sparsify, take_rows,
                               tap_case, tap_recall, tie_aware_expected, unit_rows)
from oracle.oracle import HnswIndex as OracleHnsw

pytestmark = pytest.mark.gpu

F = np.float32
M, EFC = 8, 32
VALUES = np.array([-4, -3, -2, -1, 1, 2, 3, 4], dtype=F)
LDS_BUDGET = 156 * 1024                                      # HN_LDS_BUDGET, vsr_hnsw.h


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _int_rows(rng, lens, dim):
    """CSR rows of the given lengths: random ascending indices, values in -4 .. 4 without 0."""
    lens = np.asarray(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(dim, int(l), replace=False)) for l in lens]).astype(np.int32) if lens.sum() else np.zeros(0, np.int32)
    val = rng.choice(VALUES, int(lens.sum())).astype(F)
    return indptr, idx, val, int(dim)


def _lanes(csr):
    """sparse_lpr_for_mean_nnz over the stored entries (rows padded to an even count)."""
    lens = np.diff(csr[0])
    mean = ((lens + 1) // 2 * 2).mean()
    return 4 if mean <= 12 else 16 if mean <= 96 else 64


_CASES = {}


def _case(ctx, oracle, name):
    """Rows, queries, the oracle's serial graph per opclass (cosine shares the inner-product graph: both rank by the negated inner
    product), the corpus with a 10 % byte mask, one loaded index per graph.  Built once per module."""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng({"a": 41, "b": 42, "c": 43}[name])
    if name == "a":                                          # tables of 2 .. 16 slots, empty and full rows; 4 lanes per row
        n, dim = 600, 8
        lens = rng.integers(0, 9, n)
        lens[:9] = np.arange(9)
        qlens = np.concatenate([np.arange(9), rng.integers(0, 9, 7)])
    elif name == "b":                                        # 16 lanes per row
        n, dim = 1500, 512
        lens = rng.integers(1, 41, n)
        qlens = np.array([1, 32, 200] * 4)
    else:                                                    # odd counts with a pad entry, lane-group boundaries, the limit; 64 lanes
        n, dim = 400, 4096
        lens = rng.integers(100, 501, n)
        edges = [0, 1, 2, 63, 64, 65, 127, 128, 129, 999, 1000]
        lens[:len(edges)] = edges
        lens[200:200 + len(edges)] = edges
        qlens = np.array([0, 1, 1000, 3000, 129, 64])
    csr = _int_rows(rng, lens, dim)
    assert _lanes(csr) == {"a": 4, "b": 16, "c": 64}[name]
    q = _int_rows(rng, qlens, dim)
    dense, qdense = densify(*csr), densify(*q)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 20 + 1).astype(np.int32)
    corpus = ctx.load_corpus_sparse(*csr, block_ids=blk, doc_ids=doc)
    mask = rng.random(n) < 0.10
    oh, gpu = {}, {}
    for metric in ("l2", "ip", "l1"):
        oh[metric] = OracleHnsw(oracle, metric, dense, m=M, ef_construction=EFC, seed=5)
        gpu[metric] = corpus.load_hnsw_sparse(oh[metric].export())
    oh["cosine"], gpu["cosine"] = oh["ip"], gpu["ip"]
    c = SimpleNamespace(n=n, dim=dim, csr=csr, q=q, dense=dense, qdense=qdense, nq=len(qlens), corpus=corpus, oh=oh, gpu=gpu,
                        mask=mask, blk=blk, doc=doc)
    _CASES[name] = c
    return c


def _query_subset(q, rows):
    return take_rows(q, rows)[:3]


def _check_walk(c, metric, ef, k=600, queries=None, gpu=None):
    """search_sparse against the oracle's walk on the densified rows: rows, reported distances, visited counts."""
    qs = np.arange(c.nq) if queries is None else np.asarray(queries)
    ip, ix, vx = _query_subset(c.q, qs)
    res, vis = (gpu or c.gpu[metric]).search_sparse(ip, k, ef, metric, None, ix, vx)
    for j, i in enumerate(qs):
        rows_o, dist_o, _, nv = c.oh[metric].search(c.qdense[i], ef)
        want = rows_o[:k]
        where = (metric, ef, int(i))
        assert res.counts[j] == want.size, (where, res.counts[j], want.size)
        np.testing.assert_array_equal(res.rows[j, :want.size], want, err_msg=str(where))
        np.testing.assert_array_equal(res.dist[j, :want.size], reported(metric, dist_o[:k]), err_msg=str(where))
        np.testing.assert_array_equal(res.block_ids[j, :want.size], c.blk[want])
        np.testing.assert_array_equal(res.doc_ids[j, :want.size], c.doc[want])
        assert vis[j] == nv, (where, vis[j], nv)
        assert (res.rows[j, want.size:] == -1).all()
    return res, vis


# ---- 1. walk parity on oracle-built graphs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_walk_is_the_oracle_walk(ctx, oracle, name, metric):
    c = _case(ctx, oracle, name)
    for ef in (10, 40, 200):
        _check_walk(c, metric, ef)
    if name == "a":                                          # one call per query length 0 .. 8: tables of 2, 2, 4, 8, 8, 16 .. slots
        for i in range(9):
            _check_walk(c, metric, 40, queries=[i])
    assert ctx.screening_check()[0] == 0


def _lds_fixed(caps, q_chunks):
    """hnsw_lds_fixed, vsr_hnsw.h: S, its flags, the neighbour ids and distances, the upper-layer visited list, the table."""
    return ((caps * 8 + ((caps + 15) & ~15) + 256 * 8 + 1024 * 4 + 15) & ~15) + q_chunks * 16


def _table_in_lds(max_nnz, ef, m=M):
    slots = 2
    while slots < 2 * max_nnz:
        slots *= 2
    return _lds_fixed(2 * ef + 2 * m + 64, slots // 2) <= LDS_BUDGET


@pytest.mark.parametrize("metric", METRICS)
def test_walk_long_rows_and_where_the_table_lives(ctx, oracle, metric):
    """Case (c): rows of 0 .. 1000 entries, one call per query length so that each call sizes its own tables.  The 3000-entry
    query (8192 slots, 64 KB) lives in the wave's LDS at ef_search = 40 and leaves it at ef_search = 5000, where S itself takes
    95 KB; the 1000-entry query (2048 slots) stays in LDS at both.  Both paths give the oracle's walk."""
    c = _case(ctx, oracle, "c")
    lens = np.diff(c.q[0])
    for i in range(c.nq):
        for ef in (10, 40):
            assert _table_in_lds(int(lens[i]), ef)
            _check_walk(c, metric, ef, queries=[i])
    assert _table_in_lds(1000, 5000) and not _table_in_lds(3000, 5000)
    for i in (2, 3):                                         # 1000 entries: LDS; 3000: read where staging wrote it
        _check_walk(c, metric, 5000, queries=[i])
    _check_walk(c, metric, 40)                               # one call for all: every table sized by the longest query
    assert ctx.screening_check()[0] == 0


# ---- 2. index range ----------------------------------------------------------------------------------------------------------
def test_index_range_other_hash_chains_same_answers(ctx, oracle):
    """Case (b) with every index multiplied by 1 953 125 in 1 000 000 000 dimensions: other hash chains, the same answers byte
    for byte."""
    c = _case(ctx, oracle, "b")
    scale, dim = 1_953_125, 1_000_000_000
    wide = lambda t: (t[0], (t[1].astype(np.int64) * scale).astype(np.int32), t[2], dim)
    rows, q = wide(c.csr), wide(c.q)
    assert int(rows[1].max()) < dim and int(rows[1].max()) > 2 ** 29
    corpus = ctx.load_corpus_sparse(*rows, block_ids=c.blk, doc_ids=c.doc)
    for metric in METRICS:
        gpu = corpus.load_hnsw_sparse(c.oh[metric].export())
        for ef in (10, 40, 200):
            a, va = c.gpu[metric].search_sparse(c.q[0], 600, ef, metric, None, c.q[1], c.q[2])
            b, vb = gpu.search_sparse(q[0], 600, ef, metric, None, q[1], q[2])
            for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (metric, ef, f)
            assert va.tobytes() == vb.tobytes()
        gpu.free()
    corpus.free()


# ---- 3. inherited behaviour --------------------------------------------------------------------------------------------------
def test_predicate_aware_walk_under_a_ten_percent_mask(ctx, oracle):
    import vsrbac
    c = _case(ctx, oracle, "b")
    flt = c.corpus.filter_from_bytemask(c.mask.astype(np.uint8), vsrbac.BITMAP)
    for metric in ("l2", "l1"):
        gpu, oh = c.gpu[metric], c.oh[metric]
        for aware in (False, True):
            gpu.set_predicate_aware(aware)
            for ef in (20, 100):
                res, vis = gpu.search_sparse(c.q[0], 20, ef, metric, [flt] * c.nq, c.q[1], c.q[2])
                for i in range(c.nq):
                    rows_o, dist_o, _, nv = (oh.search_predicate_aware(c.qdense[i], ef, c.mask.astype(np.uint8)) if aware
                                             else oh.search(c.qdense[i], ef))
                    keep = c.mask[rows_o]
                    want, wd = rows_o[keep][:20], dist_o[keep][:20]
                    assert res.counts[i] == want.size, (metric, aware, ef, i)
                    np.testing.assert_array_equal(res.rows[i, :want.size], want)
                    np.testing.assert_array_equal(res.dist[i, :want.size], reported(metric, wd))
                    assert vis[i] == nv
        gpu.set_predicate_aware(False)
    flt.free()


@pytest.mark.parametrize("metric", ["l2", "l1", "ip"])
def test_iterative_scans_match_the_model(ctx, oracle, metric, monkeypatch):
    """relaxed_order and strict_order with small and large max_scan_tuples, with and without the filter; the discard-overflow
    re-run; mode off is search_sparse bit for bit."""
    import vsrbac
    c = _case(ctx, oracle, "b")
    gpu, ef = c.gpu[metric], 40
    g = SparseGraph(c.oh[metric].export(), *c.csr)
    nq = 6
    ip, ix, vx = _query_subset(c.q, np.arange(nq))
    flt = c.corpus.filter_from_bytemask(c.mask.astype(np.uint8), vsrbac.BITMAP)
    filters = {"none": (None, None), "10%": ([flt] * nq, c.mask)}

    def check(modes, scans, ks):
        for mode in modes:
            for max_scan in scans:
                streams = [Stream(SparseScan(g, ix[ip[i]:ip[i + 1]], vx[ip[i]:ip[i + 1]], ef, metric, mode, max_scan)) for i in range(nq)]
                for k in ks:
                    for fname, (fl, mask) in filters.items():
                        res, tup = gpu.search_sparse_iterative(ip, k, ef, metric, fl, mode, max_scan, ix, vx)
                        for i in range(nq):
                            rows, d, t = streams[i].answer(k, mask)
                            where = (metric, mode, max_scan, k, fname, i)
                            assert res.counts[i] == rows.size, (where, res.counts[i], rows.size)
                            np.testing.assert_array_equal(res.rows[i, :rows.size], rows, err_msg=str(where))
                            np.testing.assert_array_equal(res.dist[i, :rows.size], reported(metric, d), err_msg=str(where))
                            assert tup[i] == t, (where, tup[i], t)

    check(("relaxed_order", "strict_order"), (1, 200, 20000), (5, 60))
    monkeypatch.setenv("VSR_HNSW_DISCARD_CAP", "64")         # D overflows: the host entry point re-runs with room for every element
    check(("relaxed_order",), (20000,), (60,))
    monkeypatch.delenv("VSR_HNSW_DISCARD_CAP")
    for fl, _ in filters.values():
        a, vis = gpu.search_sparse(ip, 60, ef, metric, fl, ix, vx)
        b, tup = gpu.search_sparse_iterative(ip, 60, ef, metric, fl, "off", 20000, ix, vx)
        for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        np.testing.assert_array_equal(vis, tup)
    flt.free()


def _device(gpu, q, k, ef, metric, flt=None, iterative=None, max_nnz=None):
    """The device entry points: CSR arrays in device memory, results from device arrays."""
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ip, ix, vx = q[:3]
    nq = ip.size - 1
    pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)              # (an empty tensor has no address)
    d_ip, d_ix, d_vx = (torch.from_numpy(pad(np.ascontiguousarray(a)).copy()).to(dev) for a in (ip, ix, vx))
    mx = int(np.diff(ip).max(initial=0)) if max_nnz is None else max_nnz
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.empty((nq,), dtype=torch.int64, device=dev)}
    if iterative:
        keep = gpu.search_sparse_iterative_device(p(d_ip), p(d_ix), p(d_vx), nq, mx, k, ef, metric, flt, iterative[0], iterative[1],
                                                  p(o["blk"]), p(o["doc"]), p(o["row"]), p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    else:
        keep = gpu.search_sparse_device(p(d_ip), p(d_ix), p(d_vx), nq, mx, k, ef, metric, flt, p(o["blk"]), p(o["doc"]), p(o["row"]),
                                        p(o["dist"]), p(o["cnt"]), p(o["vis"]))
    gpu.corpus.ctx.synchronize()
    del keep
    return {key: v.cpu().numpy() for key, v in o.items()}


def test_visited_forms_and_device_entry_points(ctx, oracle, monkeypatch):
    """Host entry = device entry, plain and iterative, with and without the filter; the LDS hash overflows into the re-run (the
    device entry reports count -1); the global bitmap; all three forms give the oracle's walk."""
    import vsrbac
    c = _case(ctx, oracle, "b")
    k, ef = 50, 40
    flt = [c.corpus.filter_from_bytemask(c.mask.astype(np.uint8), vsrbac.BITMAP)] * c.nq
    for metric in METRICS:
        gpu = c.gpu[metric]
        for f in (None, flt):
            host, vis = gpu.search_sparse(c.q[0], k, ef, metric, f, c.q[1], c.q[2])
            d = _device(gpu, c.q, k, ef, metric, f)
            np.testing.assert_array_equal(d["row"], host.rows)
            np.testing.assert_array_equal(d["blk"], host.block_ids)
            np.testing.assert_array_equal(d["doc"], host.doc_ids)
            np.testing.assert_array_equal(d["dist"], host.dist)
            np.testing.assert_array_equal(d["cnt"], host.counts)
            np.testing.assert_array_equal(d["vis"], vis)
            hi, tup = gpu.search_sparse_iterative(c.q[0], k, ef, metric, f, "relaxed_order", 500, c.q[1], c.q[2])
            di = _device(gpu, c.q, k, ef, metric, f, ("relaxed_order", 500))
            np.testing.assert_array_equal(di["row"], hi.rows)
            np.testing.assert_array_equal(di["dist"], hi.dist)
            np.testing.assert_array_equal(di["cnt"], hi.counts)
            np.testing.assert_array_equal(di["vis"], tup)
    assert ctx.screening_check()[0] == 0
    monkeypatch.setenv("VSR_HNSW_VISITED", "hash:64")        # the LDS hash overflows: the host entry point re-runs, the device one reports
    _check_walk(c, "l2", 40)
    _check_walk(c, "l1", 40)
    d = _device(c.gpu["l2"], c.q, k, ef, "l2")
    assert (d["cnt"] == -1).all() and (d["row"] == -1).all()
    monkeypatch.setenv("VSR_HNSW_VISITED", "global")
    _check_walk(c, "l2", 40)
    _check_walk(c, "l1", 40)
    monkeypatch.delenv("VSR_HNSW_VISITED")
    _check_walk(c, "l2", 40)
    flt[0].free()


def test_device_query_longer_than_max_query_nnz_sets_the_guard_bit(ctx, oracle):
    """A device query longer than max_query_nnz becomes an empty table -- it is answered as the empty query -- and the session's
    guard word says so, as in vsr_search_sparse_device."""
    import vsrbac
    c = _case(ctx, oracle, "b")
    longest = int(np.diff(c.q[0]).max())
    sess = vsrbac.Context(0)                                 # (the guard word is the session's and stays set: a session of its own)
    corpus = sess.load_corpus_sparse(*c.csr, block_ids=c.blk, doc_ids=c.doc)
    gpu = corpus.load_hnsw_sparse(c.oh["l2"].export())
    d = _device(gpu, c.q, 20, 40, "l2")
    assert sess.screening_check()[0] == 0
    d = _device(gpu, c.q, 20, 40, "l2", max_nnz=longest - 1)
    with pytest.raises(vsrbac.VsrError) as e:
        sess.screening_check()
    assert e.value.status == vsrbac._ffi.ERR_HIP and "guard" in str(e.value)
    gpu.free()
    corpus.free()
    sess.close()
    lens = np.diff(c.q[0])
    empty = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, F))
    want, _ = c.gpu["l2"].search_sparse(empty[0], 20, 40, "l2", None, empty[1], empty[2])
    full, _ = c.gpu["l2"].search_sparse(c.q[0], 20, 40, "l2", None, c.q[1], c.q[2])
    for i in range(c.nq):
        if lens[i] == longest:                               # squared norm 0 + |row|^2: the empty query's answer
            np.testing.assert_array_equal(d["row"][i], want.rows[0])
            np.testing.assert_array_equal(d["dist"][i], want.dist[0])
        else:
            np.testing.assert_array_equal(d["row"][i], full.rows[i])
    assert ctx.screening_check()[0] == 0                     # (per session)


def test_ten_tid_elements_and_export_load_round_trip(ctx, oracle):
    """A hand-merged graph: 25 copies of row 50 folded into elements of 10, 10 and 6 heap TIDs (oracle.HnswIndex.batched with
    explicit elements), loaded with load_hnsw_sparse: an element's TIDs come out newest first, at the element's distance.
    export -> load_hnsw_sparse answers bit for bit."""
    rng = np.random.default_rng(77)
    n, dim = 500, 64
    csr = _int_rows(rng, rng.integers(1, 13, n), dim)
    dense = densify(*csr)
    copies = list(range(300, 325))
    dense[copies] = dense[50]
    csr = sparsify(dense)
    groups = [(50,) + tuple(copies[:9]), tuple(copies[9:19]), tuple(copies[19:])]
    elements = [(r,) for r in range(n) if r != 50 and r not in copies] + groups
    order = np.argsort([t[0] for t in elements], kind="stable")
    elements = [elements[i] for i in order]
    q = _int_rows(rng, rng.integers(1, 20, 8), dim)
    q = (np.concatenate([q[0], [q[0][-1] + int(np.diff(csr[0])[50])]]), np.concatenate([q[1], csr[1][csr[0][50]:csr[0][51]]]),
         np.concatenate([q[2], csr[2][csr[0][50]:csr[0][51]]]), dim)                      # the last query: row 50 itself
    qdense = densify(*q)
    corpus = ctx.load_corpus_sparse(*csr)
    for metric in ("l2", "l1", "ip"):
        oh = OracleHnsw.batched(oracle, metric, dense, M, EFC, 9, elements=elements)
        g = oh.export()
        assert sorted(g["tid_count"].tolist())[-3:] == [6, 10, 10]
        gpu = corpus.load_hnsw_sparse(g)
        again = corpus.load_hnsw_sparse(gpu.export())
        same_graph(gpu.export(), again.export())
        for ef in (10, 40, 200):                             # (at 200 the L1 walk, too, reaches the copies: the oracle finds 26 rows at 0)
            res, vis = gpu.search_sparse(q[0], 600, ef, metric, None, q[1], q[2])
            res2, vis2 = again.search_sparse(q[0], 600, ef, metric, None, q[1], q[2])
            for f in ("block_ids", "doc_ids", "rows", "dist", "counts"):
                assert getattr(res, f).tobytes() == getattr(res2, f).tobytes()
            assert vis.tobytes() == vis2.tobytes()
            for i in range(len(qdense)):
                rows_o, dist_o, _, nv = oh.search(qdense[i], ef)
                assert res.counts[i] == rows_o.size and vis[i] == nv
                np.testing.assert_array_equal(res.rows[i, :rows_o.size], rows_o)
                np.testing.assert_array_equal(res.dist[i, :rows_o.size], reported(metric, dist_o))
        if metric != "ip":                                   # the copies of the query row: distance 0, each element newest TID first
            cnt = res.counts[-1]
            zero = res.rows[-1, :cnt][res.dist[-1, :cnt] == 0]
            assert set(copies) | {50} <= set(zero.tolist())
            full = int(np.flatnonzero(g["tid_count"] == 10)[0])
            at = int(np.flatnonzero(res.rows[-1, :cnt] == g["tids"][full, 9])[0])
            np.testing.assert_array_equal(res.rows[-1, at:at + 10], g["tids"][full, ::-1])
        gpu.free()
        again.free()
    corpus.free()


# ---- 4. build ----------------------------------------------------------------------------------------------------------------
def _built(ctx, csr, metric, seed, m=M, efc=EFC):
    corpus = ctx.load_corpus_sparse(*csr)
    gpu = corpus.build_hnsw_sparse(m, efc, metric, seed=seed)
    ctx.screening_check(0)                                   # raises when a kernel left a guard bit behind
    g = gpu.export()
    gpu.free()
    corpus.free()
    return g


@pytest.mark.parametrize("metric", METRICS)
def test_build_is_the_batched_model(ctx, oracle, metric, monkeypatch):
    """1500 x 512, 1 .. 40 entries per row, m = 8, ef_construction = 32: the exported arrays equal oracle.HnswIndex.batched on
    the densified rows; a second run with the same seed gives identical arrays; so does the restart from a visited table of 256
    slots.

    Inner product and cosine are the hard ones: rows without a common index all have inner product 0, so a layer search holds far
    more candidates of one distance than a candidate array of ef_construction + 2 m entries keeps, and pgvector's unbounded heap
    expands every one that is as near as the furthest of W.  A build that silently dropped them differed from the model in 43 of
    the 24 000 entries of nbr0 here; the sparse build reports the loss and starts again with an array twice as long (one restart
    on these rows)."""
    c = _case(ctx, oracle, "b")
    want = OracleHnsw.batched(oracle, metric, c.dense, M, EFC, 21).export()
    got = _built(ctx, c.csr, metric, 21)
    np.testing.assert_array_equal(got["level"], want["level"])
    same_graph(got, want)
    check_built_graph(got, M)
    same_graph(_built(ctx, c.csr, metric, 21), got)
    if metric in ("l2", "l1"):
        monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "256")
        same_graph(_built(ctx, c.csr, metric, 21), got)
        monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")


@pytest.mark.parametrize("metric", ["l2"])
def test_build_is_the_fp32_build_of_the_densified_rows(ctx, oracle, metric):
    """The graph machinery does not know the row format: on integer-valued rows, where both distance stages are exact, the sparse
    build and vsr_hnsw_build over the densified rows export the same arrays.  L2 only: L1 has no fp32 build, and on these rows the
    fp32 inner-product build loses candidates of equal distance from its bounded array, which the sparse build does not (see
    test_build_is_the_batched_model)."""
    c = _case(ctx, oracle, "b")
    dense = ctx.load_corpus(c.dense)
    gpu = dense.build_hnsw(M, EFC, metric, seed=21)
    want = gpu.export()
    gpu.free()
    dense.free()
    same_graph(_built(ctx, c.csr, metric, 21), want)


def test_build_over_long_rows_is_the_batched_model(ctx, oracle):
    """Case (c): 64 lanes per row, rows of 0 .. 1000 entries (tables of 2048 slots)."""
    c = _case(ctx, oracle, "c")
    for metric in ("l2", "l1"):
        want = OracleHnsw.batched(oracle, metric, c.dense, M, EFC, 22).export()
        got = _built(ctx, c.csr, metric, 22)
        same_graph(got, want)


def _exact_dense(metric, rows, q):
    x, qq = rows.astype(np.float64), q.astype(np.float64)
    if metric == "l2":
        return ((x - qq) ** 2).sum(axis=1)
    if metric == "l1":
        return np.abs(x - qq).sum(axis=1)
    if metric == "ip":
        return -(x @ qq)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - (x @ qq) / np.sqrt((x * x).sum(axis=1) * (qq * qq).sum())


@pytest.mark.parametrize("metric", METRICS)
def test_build_reaches_the_tap_floor(ctx, oracle, metric):
    """028_hnsw_sparsevec_build_recall.pl's case per opclass: recall@20 at ef_search 40 >= 0.99 (0.97 for <#>) against
    vsr_search_sparse, and >= the oracle's serial build on the same rows - 0.01.  Cosine runs on rows from sparse_l2_normalize."""
    rows, queries, limit, ef = tap_case()
    floor = 0.97 if metric == "ip" else 0.99
    csr, q = sparsify(rows), sparsify(queries)
    if metric == "cosine":
        csr, q = ctx.sparse_l2_normalize(*csr), ctx.sparse_l2_normalize(*q)
        np.testing.assert_array_equal(densify(*csr), unit_rows(rows))
    corpus = ctx.load_corpus_sparse(*csr)
    exact = corpus.search_sparse(q[0], 2048, metric, None, q[1], q[2])
    expected = []
    for i in range(len(queries)):                            # tie-aware: every row no farther than the 20th
        kth = exact.dist[i, limit - 1]
        assert exact.dist[i, exact.counts[i] - 1] > kth
        expected.append(np.sort(exact.rows[i, :exact.counts[i]][exact.dist[i, :exact.counts[i]] <= kth]))
    gpu = corpus.build_hnsw_sparse(16, 64, metric, seed=28)
    res, _ = gpu.search_sparse(q[0], limit, ef, metric, None, q[1], q[2])
    r = tap_recall([res.rows[i, :res.counts[i]] for i in range(len(queries))], expected, limit)
    oh = OracleHnsw(oracle, metric, densify(*csr), m=16, ef_construction=64, seed=28)
    qd = densify(*q)
    ro = tap_recall([oh.search(qd[i], ef)[0] for i in range(len(queries))], expected, limit)
    print(f"build_hnsw_sparse {metric}: recall@{limit} ef={ef} = {r:.4f} (floor {floor}; oracle serial build {ro:.4f})")
    assert r >= floor
    assert r >= ro - 0.01
    gpu.free()
    corpus.free()


# ---- 5. real-valued data -----------------------------------------------------------------------------------------------------
def _clustered(rng, n, dim, nnz, centres=60):
    """Rows whose supports are mostly drawn from one of a few dozen centre supports, values from a normal law."""
    sup = [rng.choice(dim, 3 * nnz, replace=False) for _ in range(centres)]
    x = np.zeros((n, dim), dtype=F)
    for r in range(n):
        k = int(rng.integers(nnz - 8, nnz + 9))
        cols = np.unique(np.concatenate([rng.choice(sup[int(rng.integers(centres))], k - 4, replace=False), rng.choice(dim, 4)]))
        x[r, cols] = rng.normal(0, 1, cols.size).astype(F)
    return x


@pytest.fixture(scope="module")
def real_world(ctx, oracle):
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(48)
    x = _clustered(rng, 4000, 2048, 48)
    pick = rng.integers(0, 4000, 24)
    q = (x[pick] + (rng.random((24, 2048)) < 0.004) * rng.normal(0, 1, (24, 2048))).astype(F)
    q[:8] = x[pick[:8]]                                      # eight rows queried with themselves
    corpus = ctx.load_corpus_sparse(*sparsify(x))
    # the floors: the oracle's serial builds on the densified rows, the slow part of this case (2048 dense dimensions per distance).
    # Both run beside the GPU work, in threads of their own (the C oracle holds no interpreter lock)
    pool = ThreadPoolExecutor(2)
    serial = {m: pool.submit(OracleHnsw, oracle, m, x, 16, 64, 3) for m in ("l2", "l1")}
    yield SimpleNamespace(x=x, q=q, pick=pick, corpus=corpus, serial=serial)
    pool.shutdown()
    corpus.free()


@pytest.mark.parametrize("metric", ["l2", "l1"])
def test_real_valued_build_and_search(ctx, oracle, real_world, metric):
    """4000 x 2048, ~48 non-zeros, clustered supports.  Every reported distance within 1e-4 relative of a float64 recomputation;
    recall@20 at ef_search 100 at least the oracle's serial build on the densified rows - 0.02 (measured here); a row queried with
    itself under <-> comes back first at distance <= 1e-6 |q|, not NaN."""
    w = real_world
    k, ef = 20, 100
    gpu = w.corpus.build_hnsw_sparse(16, 64, metric, seed=3)
    assert ctx.screening_check()[0] == 0
    qc = sparsify(w.q)
    res, _ = gpu.search_sparse(qc[0], k, ef, metric, None, qc[1], qc[2])
    assert not np.isnan(res.dist).any()
    exact = [_exact_dense(metric, w.x, w.q[i]) for i in range(len(w.q))]
    for i in range(len(w.q)):
        rows = res.rows[i, :res.counts[i]]
        want = np.sqrt(exact[i][rows]) if metric == "l2" else exact[i][rows]
        # 1e-4 relative; next to 0 a relative bound means nothing (the double totals of the query and of the hits differ in
        # their last bits), and the floor is the one a row queried with itself is held to: 1e-6 |q|
        tol = np.maximum(1e-4 * want, 1e-6 * np.linalg.norm(w.q[i].astype(np.float64)))
        assert (np.abs(res.dist[i, :rows.size].astype(np.float64) - want) <= tol).all(), (metric, i)
    expected = [tie_aware_expected(e, k) for e in exact]
    r = tap_recall([res.rows[i, :res.counts[i]] for i in range(len(w.q))], expected, k)
    oh = w.serial[metric].result()
    ro = tap_recall([oh.search(w.q[i], ef)[0] for i in range(len(w.q))], expected, k)
    print(f"real-valued 4000 x 2048 {metric}: recall@{k} ef={ef} GPU build {r:.4f}, oracle serial build {ro:.4f}")
    assert r >= ro - 0.02
    if metric == "l2":
        # rows queried with themselves.  A walk need not reach every row of a graph over clustered supports (at ef_search 1000
        # one of the eight rows above is still not found, and that is the graph's doing), so the rows asked are ones every walk
        # evaluates: the entry point and its first layer-0 neighbours
        g = gpu.export()
        nbrs = g["nbr0"][g["entry"]]
        own_rows = np.concatenate([[g["entry"]], nbrs[nbrs >= 0][:7]])
        own = sparsify(w.x[own_rows])
        res, _ = gpu.search_sparse(own[0], k, ef, metric, None, own[1], own[2])
        assert not np.isnan(res.dist).any()
        for i, r in enumerate(own_rows):
            assert res.rows[i, 0] == r, (i, r, res.rows[i, :3], res.dist[i, :3])
            assert res.dist[i, 0] <= 1e-6 * np.linalg.norm(w.x[r].astype(np.float64)), (i, res.dist[i, 0])
    gpu.free()


# ---- 6. sparse_norms / sparse_l2_normalize -----------------------------------------------------------------------------------
def test_sparse_norms_and_normalize(ctx):
    rng = np.random.default_rng(6)
    x = _clustered(rng, 300, 512, 40, centres=10)
    x[7] = 0                                                 # a zero row: norm 0, left as it is
    x[9, :3] = [1e-30, 0, 1e30]                              # 1e-30 / 1e30 underflows to 0 in float4: counted, dropped by the binding
    x[9, 3:] = 0
    x[11, :2] = [3e38, 3e38]                                 # |row|^2 overflows float4, not the double sum
    x[11, 2:] = 0
    csr = sparsify(x)
    got = ctx.sparse_norms(*csr)
    np.testing.assert_array_equal(got, l2_norms(csr[0], csr[2]))
    assert got[7] == 0.0 and np.isfinite(got[11])
    ip, ix, vx, dim = ctx.sparse_l2_normalize(*csr)
    wp, wi, wv, _, dropped = l2_normalize(*csr)
    assert dropped == 1 and dim == 512
    np.testing.assert_array_equal(ip, wp)
    np.testing.assert_array_equal(ix, wi)
    assert vx.tobytes() == wv.tobytes()                      # values bit for bit
    assert ip[8] == ip[7] and ip[10] - ip[9] == 1 and vx[ip[9]] == 1.0
    np.testing.assert_allclose(vx[ip[11]:ip[12]], np.full(2, 1 / np.sqrt(2.0)), rtol=1e-7)
    ctx.load_corpus_sparse(ip, ix, vx, dim).free()           # the result is a legal sparsevec
    # the scipy-like form and three arrays are the same call; an empty batch is legal
    assert ctx.sparse_norms(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, F), 5).size == 0
    # sparsevec_l2_normalize's overflow refusal (float_overflow_error) cannot be reached from finite values: |v| <= norm, so the
    # quotient never exceeds 1.  Values that are not finite are not sparsevec values; the quotient is then NaN or 0, never Inf:
    # the call succeeds, as pgvector's would.
    bad = (np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.array([np.inf, 1.0], F), 4)
    _, _, v, _ = ctx.sparse_l2_normalize(*bad)
    assert v.size == 1 and np.isnan(v[0])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def _raises(status, text, fn, *args, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError) as e:
        fn(*args, **kw)
    assert e.value.status == status and text in str(e.value), (status, text, e.value.status, str(e.value))


def test_refusals(ctx, oracle):
    from vsrbac import _ffi
    INV, DIMM, UNS = _ffi.ERR_INVALID, _ffi.ERR_DIM_MISMATCH, _ffi.ERR_UNSUPPORTED
    c = _case(ctx, oracle, "a")
    n, dim = c.n, c.dim
    rng = np.random.default_rng(70)
    dense_rows = rng.integers(0, 9, (n, dim)).astype(F)
    dense = ctx.load_corpus(dense_rows)
    half = ctx.load_corpus_half(dense_rows.astype(np.float16))
    bits = ctx.load_corpus_bit(dense_rows > 4)
    g = c.oh["l2"].export()
    sp = c.gpu["l2"]
    qp, qi, qv = np.array([0, 2], np.int64), np.array([1, 7], np.int32), np.array([2, -3], F)
    # ---- every new entry point against the four formats
    for other in (dense, half, bits):
        _raises(INV, "vsr_hnsw_load_sparse: the corpus is not a sparse corpus", other.load_hnsw_sparse, g)
        _raises(INV, "vsr_hnsw_build_sparse: the corpus is not a sparse corpus", other.build_hnsw_sparse, M, EFC, "l2")
    fidx = dense.load_hnsw(g)
    hidx = half.load_hnsw_half(g)
    bidx = bits.load_hnsw_bit(g, "hamming")
    for idx in (fidx, hidx, bidx):
        _raises(INV, "not over a sparse corpus", idx.search_sparse, qp, 5, 40, "l2", None, qi, qv, dim)
        _raises(INV, "not over a sparse corpus", idx.search_sparse_iterative, qp, 5, 40, "l2", None, "relaxed_order", 100, qi, qv, dim)
        _raises(INV, "not over a sparse corpus", idx.search_sparse_device, 8, 8, 8, 1, 2, 5, 40, "l2", None, 8, 8, 8, 8, 8)
        _raises(INV, "not over a sparse corpus", idx.search_sparse_iterative_device, 8, 8, 8, 1, 2, 5, 40, "l2", None, "relaxed_order", 100,
                8, 8, 8, 8, 8)
    # ---- a sparse index given to the float and bit entry points: the message names the _sparse entry points
    for fn, args in ((sp.search, (dense_rows[:1], 5, 40, "l2")), (sp.search_iterative, (dense_rows[:1], 5, 40, "l2")),
                     (sp.search_device, (8, 1, 5, 40, "l2", None, 8, 8, 8, 8, 8)),
                     (sp.search_iterative_device, (8, 1, 5, 40, "l2", None, "relaxed_order", 100, 8, 8, 8, 8, 8)),
                     (sp.search_bit, (dense_rows[:1] > 4, 5, 40, "hamming")),
                     (sp.search_bit_device, (8, 1, 5, 40, "hamming", None, 8, 8, 8, 8, 8))):
        _raises(UNS, "vsr_hnsw_search_sparse", fn, *args)
    # ---- vsr_hnsw_load / vsr_hnsw_build over a sparse corpus: still today's text
    old = "a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)"
    _raises(UNS, "vsr_hnsw_load: " + old, c.corpus.load_hnsw, g)
    _raises(UNS, "vsr_hnsw_build: " + old, c.corpus.build_hnsw)
    _raises(UNS, "vsr_hnsw_build_ex: " + old, c.corpus.build_hnsw, merge_duplicates=True)
    _raises(INV, "not a halfvec corpus", c.corpus.load_hnsw_half, g)
    _raises(INV, "not a bit corpus", c.corpus.load_hnsw_bit, g)
    # ---- the 1001-non-zero row at load and at build; the merge flag; metrics
    long_rows = _int_rows(rng, [1001, 1000, 3], 2000)
    big = ctx.load_corpus_sparse(*long_rows)
    tiny = dict(m=4, entry=0, level=np.zeros(3, np.int32), nbr0=np.full((3, 8), -1, np.int32), tid_count=np.ones(3, np.int32),
                tids=np.concatenate([np.arange(3, dtype=np.int64)[:, None], np.full((3, 9), -1, np.int64)], axis=1),
                up_slot=np.full(3, -1, np.int32), up_nbr=np.zeros((0, 4), np.int32), max_level=1)
    words = "sparsevec cannot have more than 1000 non-zero elements for hnsw index"
    _raises(UNS, words, big.load_hnsw_sparse, tiny)
    _raises(UNS, words, big.build_hnsw_sparse, 4, 16, "l2")
    big.free()
    ok = ctx.load_corpus_sparse(*take_rows(long_rows, [1, 2]))
    ok.build_hnsw_sparse(4, 16, "l1").free()                 # 1000 is legal
    ok.free()
    _raises(UNS, "VSR_HNSW_BUILD_MERGE_DUPLICATES is not supported over a sparse corpus", c.corpus.build_hnsw_sparse, M, EFC, "l2",
            merge_duplicates=True)
    _raises(INV, "not an operator class of sparsevec", c.corpus.build_hnsw_sparse, M, EFC, "hamming")
    _raises(UNS, "m must be between 2 and 100", c.corpus.build_hnsw_sparse, 1, EFC, "l2")
    # ---- queries: validated as vsr_search_sparse validates them; the device form's max_query_nnz
    _raises(INV, "sparsevec indices must be in ascending order", sp.search_sparse, qp, 5, 40, "l2", None, qi[::-1].copy(), qv)
    _raises(INV, "sparsevec index out of bounds", sp.search_sparse, qp, 5, 40, "l2", None, np.array([1, dim], np.int32), qv)
    _raises(INV, "binary representation of sparsevec cannot contain zero values", sp.search_sparse_iterative, qp, 5, 40, "l2", None,
            "relaxed_order", 100, qi, np.array([1, 0], F))
    _raises(DIMM, f"different sparsevec dimensions {dim} and {dim + 1}", sp.search_sparse, qp, 5, 40, "l2", None, qi, qv, dim + 1)
    _raises(INV, "metric", sp.search_sparse, qp, 5, 40, "hamming", None, qi, qv)
    _raises(INV, "ef_search must be between 1 and 5000", sp.search_sparse, qp, 5, 5001, "l2", None, qi, qv)
    _raises(INV, "k must be >= 1", sp.search_sparse, qp, 0, 40, "l2", None, qi, qv)
    _raises(INV, "max_query_nnz must be between 0 and 16000", sp.search_sparse_device, 8, 8, 8, 1, 16001, 5, 40, "l2", None, 8, 8, 8, 8, 8)
    _raises(INV, "max_query_nnz must be between 0 and 16000", sp.search_sparse_iterative_device, 8, 8, 8, 1, -1, 5, 40, "l2", None,
            "relaxed_order", 100, 8, 8, 8, 8, 8)
    _raises(INV, "iterative scan mode", sp.search_sparse_iterative, qp, 5, 40, "l2", None, 7, 100, qi, qv)
    # ---- everything answers as before afterwards
    _check_walk(c, "l2", 40)
    _check_walk(c, "l1", 40)
    r, _ = fidx.search(dense_rows[:1], 1, 40, "l2")
    assert r.dist[0, 0] == 0
    assert sp.info()[0] == len(g["level"]) and sp.device_bytes() == fidx.device_bytes()
    assert ctx.screening_check()[0] == 0
    for h in (fidx, hidx, bidx):
        h.free()
    for co in (dense, half, bits):
        co.free()
