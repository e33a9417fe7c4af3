"""K2b (vsr_mfmab.h): the shared passes of a bit corpus on the int8 matrix cores, switched on by Context.set_bit_mfma.

The kernel is exact, so everything is compared bit for bit against tests/bit_model.py -- row ids, block and document ids, fp32
distances, counts -- and every shared pass must name K2b: there is no permitted fallback."""
import ctypes

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
    c.set_bit_mfma(True)
    yield c
    c.close()


def _ids(n, rows_per_doc=7):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _bits(rng, shape, density=0.5):
    return bit_model.pack(rng.random(shape) < density)


def _check(ctx, corpus, model, q, k, metric, filters=None, masks=None, kernel="K2b"):
    res = corpus.search_bit(q, k, metric, filters)
    assert kernel in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    want = model.distances(metric, q)
    for i in range(q.shape[0]):
        idx, dist = model.topk(want[i], k, None if masks is None else masks[i])
        m = res.counts[i]
        assert m == idx.size, (i, m, idx.size)
        np.testing.assert_array_equal(res.rows[i, :m], idx)
        np.testing.assert_array_equal(res.block_ids[i, :m], model.blk[idx])
        np.testing.assert_array_equal(res.doc_ids[i, :m], model.doc[idx])
        np.testing.assert_array_equal(res.dist[i, :m].view(np.uint32), dist.view(np.uint32))
        assert (res.rows[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
    return res


def test_switch(monkeypatch):
    """Off by default; on by the call and by VSR_BIT_MFMA=1 at open; a one-query call stays on K1b either way."""
    import vsrbac
    rng = np.random.default_rng(1)
    rows, q = _bits(rng, (500, 100)), _bits(rng, (16, 100))
    blk, doc = _ids(500)
    model = BitModel(rows, 100, doc, blk)
    for env, call, shared in ((None, False, "K1b"), (None, True, "K2b"), ("1", False, "K2b")):
        if env:
            monkeypatch.setenv("VSR_BIT_MFMA", env)
        c = vsrbac.Context(0)
        monkeypatch.delenv("VSR_BIT_MFMA", raising=False)
        if call:
            c.set_bit_mfma(True)
        corpus = c.load_corpus_bit(rows, 100, blk, doc)
        _check(c, corpus, model, q, 10, "hamming", kernel=shared)
        _check(c, corpus, model, q[:1], 10, "hamming", kernel="K1b")
        if call:
            c.set_bit_mfma(False)                              # from the next search
            _check(c, corpus, model, q, 10, "hamming", kernel="K1b")
        corpus.free()
        c.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [16, 32])
@pytest.mark.parametrize("dim", [128, 192])
def test_lane_maps(ctx, dim, nq, metric):
    """One set bit per row and per query, at positions that depend on the row, the query, the K-step, the dword and the nibble
    without any symmetry between them: a transposed fragment or a swapped K-slice moves the zero distances to other pairs.
    200 rows: three full tiles and one of 8."""
    n = 200
    rpos = (np.arange(n) * 37 + 11) % dim
    qpos = rpos[(np.arange(nq) * 7 + 3) % n]                   # every query meets the bit of at least one row
    rows = np.zeros((n, dim), dtype=bool)
    rows[np.arange(n), rpos] = True
    q = np.zeros((nq, dim), dtype=bool)
    q[np.arange(nq), qpos] = True
    blk, doc = _ids(n)
    corpus = ctx.load_corpus_bit(bit_model.pack(rows), dim, blk, doc)
    res = _check(ctx, corpus, BitModel(bit_model.pack(rows), dim, doc, blk), bit_model.pack(q), 10, metric)
    assert (res.dist[:, 0] == 0).all() and (res.dist[:, -1] > 0).all()
    corpus.free()


# 52, 200: pad bits inside a K-step and inside a chunk; 513 / 1025: the first widths whose query fragments are streamed instead
# of register-resident with two / one query groups (mfmab_nstr); 8200: 17 streamed stages
@pytest.mark.parametrize("nq", [5, 17])
@pytest.mark.parametrize("dim", [52, 200, 513, 1025, 8200])
def test_row_edges(ctx, dim, nq):
    rng = np.random.default_rng(dim + nq)
    n = 700
    rows, q = _bits(rng, (n, dim)), _bits(rng, (nq, dim))
    blk, doc = _ids(n)
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(bit_model.set_pad_bits(rows, dim), dim, blk, doc)           # every pad bit set: ignored
    for metric in METRICS:
        _check(ctx, corpus, model, bit_model.set_pad_bits(q, dim), 10, metric)
        name = ctx.last_scan_kernel()
        ng = 2 if nq > 16 else 1
        nstr = 1 if dim <= 512 else 2 if dim <= 1024 and ng == 1 else 0
        assert f"NSTR={nstr}, NG={ng}" in name, name
    corpus.free()


def test_ties_and_degenerate_values(ctx):
    """16 bits over 3000 rows: 17 Hamming values, so (document_id, block_id) decide, with the caller's order shuffled against
    them; all-zero rows and an all-zero query: Jaccard's ab == 0 gives 1."""
    rng = np.random.default_rng(3)
    n, dim = 3000, 16
    rows, q = _bits(rng, (n, dim)), _bits(rng, (16, dim))
    rows[::5] = 0
    q[3] = 0
    blk, doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, 41, n).astype(np.int32)
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    for metric in METRICS:
        for k in (1, 100):
            res = _check(ctx, corpus, model, q, k, metric)
    assert (res.dist[3] == 1.0).all()
    corpus.free()


@pytest.mark.parametrize("k", [1, 100])
def test_filters(ctx, k):
    """A ~50 % byte mask, ranges whose last range ends inside a tile, a filter admitting fewer rows than k, and queries of one
    call under different filters (one of them unfiltered)."""
    import vsrbac
    rng = np.random.default_rng(4)
    n, dim, nq = 1500, 100, 18
    rows, q = _bits(rng, (n, dim)), _bits(rng, (nq, dim))
    blk, doc = _ids(n)                                         # internal row order = caller order
    model = BitModel(rows, dim, doc, blk)
    corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
    half = rng.random(n) < 0.5
    ranges = np.zeros(n, dtype=bool)
    ranges[10:75] = ranges[130:171] = ranges[900:1003] = True
    few = np.zeros(n, dtype=bool)
    few[[3, 64, 65, 700, 1499]] = True
    masks = {"half": half, "ranges": ranges, "few": few}
    fs = {"half": corpus.filter_from_bytemask(half), "ranges": corpus.filter_from_bytemask(ranges, vsrbac.RANGES),
          "few": corpus.filter_from_bytemask(few)}
    for metric in METRICS:
        for name in fs:
            res = _check(ctx, corpus, model, q, k, metric, [fs[name]] * nq, [masks[name]] * nq)
        assert (res.counts == min(k, 5)).all()
        mix = ["half", "ranges", None, "few", "ranges", "half"] * 3
        _check(ctx, corpus, model, q, k, metric, [fs[m] if m else None for m in mix], [masks[m] if m else None for m in mix])
    corpus.free()


def test_two_stage(ctx):
    """vsr_search_quantized_device with the switch on returns the bytes it returns with it off; stage 1 names K2b."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    n, dim, nq, k, shortlist = 4000, 128, 16, 10, 64
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    blk, doc = _ids(n)
    source = ctx.load_corpus(x, blk, doc)
    bits = source.binary_quantize()
    d_q = torch.from_numpy(rng.integers(-8, 9, (nq, dim)).astype(np.float32)).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    got = {}
    for on in (False, True):
        ctx.set_bit_mfma(on)
        o = SimpleNamespace(blk=torch.zeros((nq, k), dtype=torch.int64, device=dev), doc=torch.zeros((nq, k), dtype=torch.int32, device=dev),
                            row=torch.zeros((nq, k), dtype=torch.int64, device=dev), dist=torch.zeros((nq, k), dtype=torch.float32, device=dev),
                            cnt=torch.zeros((nq,), dtype=torch.int32, device=dev), keys=torch.zeros((nq, k), dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        source.search_quantized_device(bits, p(d_q), nq, k, shortlist, "l2", None, p(o.blk), p(o.doc), p(o.row), p(o.dist), p(o.cnt), p(o.keys))
        ctx.synchronize()
        assert ("K2b" if on else "K1b") in ctx.last_scan_kernel(), ctx.last_scan_kernel()
        got[on] = [t.cpu().numpy().tobytes() for t in (o.blk, o.doc, o.row, o.dist, o.cnt, o.keys)]
    assert got[True] == got[False] and np.frombuffer(got[True][4], dtype=np.int32).min() == k
    bits.free()
    source.free()
