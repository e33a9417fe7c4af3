"""The two-stage search on the GPU (vsr_search_quantized*: K1b shortlist on the quantized rows, shortlist_rerank_kernel on the
source rows) against tests/quantized_model.py.

Integer-valued rows and queries (-8 .. 8, zeros included) have exact sums in fp32 and in binary16 whatever the order, so row
ids AND fp32 distances must equal the model's bit for bit; the real-valued case compares within 1e-4, like the exact search's
tests.  The shortlist is deterministic -- (Hamming, document_id, block_id) -- so nothing here is "by recall"."""
import ctypes

from types import SimpleNamespace

import numpy as np
import pytest

import bit_model
from quantized_model import QuantizedModel, recall, round_half

pytestmark = pytest.mark.gpu

SWEEP = [(10, 10), (10, 37), (1, 300), (100, 2048)]          # (k, shortlist)
USERS = (1, 2, 3, 4, 5, 6, 7, 8)


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _ints(rng, shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


def _ids(n, rows_per_doc):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _shuffled_ids(rng, n, n_docs):
    """Caller order unrelated to (document, block) order."""
    return rng.permutation(n).astype(np.int64) + 1, rng.integers(1, n_docs + 1, n).astype(np.int32)


def _rbac(rng, doc, n_roles, n_users):
    ndocs = int(doc.max())
    perms = sorted({(int(r), int(d)) for r in range(1, n_roles + 1)
                    for d in rng.choice(np.arange(1, ndocs + 1), size=max(1, ndocs // 3), replace=False)})
    ur = sorted({(u, int(r)) for u in range(1, n_users + 1)
                 for r in rng.choice(np.arange(1, n_roles + 1), size=int(rng.integers(1, 3)), replace=False)})
    return ur, perms


def _expect(model, res, qi, want, k):
    idx, dist = want[0], want[1]
    m = res.counts[qi]
    assert m == idx.size, (m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.block_ids[qi, :m], model.blk[idx])
    np.testing.assert_array_equal(res.doc_ids[qi, :m], model.doc[idx])
    np.testing.assert_array_equal(res.dist[qi, :m], dist.astype(np.float32))
    assert (res.block_ids[qi, m:] == -1).all() and (res.doc_ids[qi, m:] == -1).all() and (res.rows[qi, m:] == -1).all()
    assert np.isposinf(res.dist[qi, m:]).all()


def _ran(session):
    name = session.last_scan_kernel()
    assert "K1b" in name and name.endswith("shortlist re-rank"), name


def _never_flags(session, res, nq):
    total, flags = session.screening_check(nq)               # (raises if a kernel's bounds guard tripped)
    assert total >= 0 and not flags.any() and (np.asarray(res.counts) >= 0).all()


class Case:
    """A source corpus, its quantized corpus with RBAC tables of its own, the model and 33 queries."""

    def __init__(self, ctx, oracle, seed, n, dim, half=False, n_docs=60):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.half = n, dim, half
        self.x = _ints(rng, (n, dim))
        self.blk, self.doc = _shuffled_ids(rng, n, n_docs)
        self.q = _ints(rng, (33, dim))
        if half:
            self.q[0, 0] = 2.5004883                         # binary16 holds 2.5: the distances are those of 2.5
            self.q[0, 3] = 1e-9                              # zero in binary16, but its bit comes from the fp32 value
            self.q[5, 1] = 1e-9
            assert round_half(self.q)[0, 0] == 2.5 and round_half(self.q)[0, 3] == 0.0
        self.source = ctx.load_corpus_half(self.x, self.blk, self.doc) if half else ctx.load_corpus(self.x, self.blk, self.doc)
        self.bits = self.source.binary_quantize()
        self.ur, self.perms = _rbac(rng, self.doc, 6, len(USERS))
        self.bits.load_rbac(self.ur, self.perms)             # (not inherited: the quantized corpus owns its filters)
        self.model = QuantizedModel(oracle, self.x, self.doc, self.blk, half=half)
        self.ham = self.model.hamming(self.q)
        self.user_mask = {u: bit_model.user_row_mask(u, self.ur, self.perms, self.doc) for u in USERS}
        self._lists = {}

    def filters(self, mode, nq):
        """(filters of the bits corpus, masks) for queries 0 .. nq: mode None, vsrbac.RANGES or vsrbac.BITMAP."""
        if mode is None:
            return None, [None] * nq
        users = [USERS[i % len(USERS)] for i in range(nq)]
        return [self.bits.filter_for_user(u, mode) for u in users], [self.user_mask[u] for u in users]

    def want(self, metric, qi, k, shortlist, mask, tag):
        key = (qi, shortlist, tag)
        if key not in self._lists:
            self._lists[key] = self.model.shortlist(self.ham[qi], shortlist, mask)
        return self.model.rerank(metric, self.q[qi], k, self._lists[key])

    def check_sweep(self, ctx, metric, mode, sweep=SWEEP):
        for k, shortlist in sweep:
            for nq in (1, 33):
                filters, masks = self.filters(mode, nq)
                res = self.source.search_quantized(self.bits, self.q[:nq], k, shortlist, metric, filters)
                _ran(ctx)
                for i in range(nq):
                    _expect(self.model, res, i, self.want(metric, i, k, shortlist, masks[i], mode), k)
                _never_flags(ctx, res, nq)

    def free(self):
        self.bits.free()
        self.source.free()


@pytest.fixture(scope="module")
def case1(ctx, oracle):
    c = Case(ctx, oracle, 1, 5000, 40)                       # 40 bits: pad bits in the last byte, a padded last chunk
    yield c
    c.free()


# ---------------------------------------------------------------------------------------------
# 1. parity, fp32 source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "ranges", "bitmap"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_parity_fp32_source(ctx, case1, metric, mode):
    import vsrbac
    case1.check_sweep(ctx, metric, {None: None, "ranges": vsrbac.RANGES, "bitmap": vsrbac.BITMAP}[mode])


# ---------------------------------------------------------------------------------------------
# 2. parity, halfvec source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("dim", [24, 130])
def test_parity_halfvec_source(ctx, oracle, dim, metric):
    import vsrbac
    case = Case(ctx, oracle, 20 + dim, 3000, dim, half=True)
    assert case.source.is_half and case.bits.is_bit
    for mode in (None, vsrbac.RANGES, vsrbac.BITMAP):
        case.check_sweep(ctx, metric, mode)
    # the tiny element's bit is set although the re-rank sees a zero there
    assert ctx.binary_quantize(case.q[:1])[0, 0] & (0x80 >> 3)
    case.free()


# ---------------------------------------------------------------------------------------------
# 3. the shortlist's cut falls inside a Hamming tie
# ---------------------------------------------------------------------------------------------
def test_shortlist_boundary_ties(ctx, oracle):
    case = Case(ctx, oracle, 3, 3000, 16, n_docs=45)         # 17 Hamming values over 3000 rows; ids shuffled
    rng = np.random.default_rng(33)
    bytemask = (rng.random(case.n) < 0.4).astype(np.uint8)
    f = case.bits.filter_from_bytemask(bytemask)
    nq = 5
    for filters, mask, tag in ((None, None, "all"), ([f] * nq, bytemask, "mask")):
        for k, shortlist in ((50, 50), (10, 200), (300, 300)):
            S = [case.model.shortlist(case.ham[i], shortlist, mask) for i in range(nq)]
            pool = np.ones(case.n, bool) if mask is None else mask.astype(bool)
            cut = [case.ham[i][S[i]].max() for i in range(nq)]
            inside = [(case.ham[i][pool] == cut[i]).sum() > (case.ham[i][S[i]] == cut[i]).sum() for i in range(nq)]
            assert sum(inside) >= 3, inside                  # the cut really falls inside a tie (a property of the data)
            res = case.source.search_quantized(case.bits, case.q[:nq], k, shortlist, "l2", filters)
            for i in range(nq):
                _expect(case.model, res, i, case.model.rerank("l2", case.q[i], k, S[i]), k)
                if k == shortlist:                           # everything of S comes back: the prefix itself is pinned
                    assert set(res.rows[i].tolist()) == set(S[i].tolist())
    f.free()
    case.free()


# ---------------------------------------------------------------------------------------------
# 4. a shortlist that holds every permitted row: the exact search
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_equals_the_exact_search_when_the_filter_fits(ctx, case1, metric):
    rng = np.random.default_rng(4)
    mask = np.zeros(case1.n, dtype=np.uint8)
    mask[rng.choice(case1.n, 900, replace=False)] = 1
    fb, fs = case1.bits.filter_from_bytemask(mask), case1.source.filter_from_bytemask(mask)
    nq = 33
    for k in (10, 100):
        got = case1.source.search_quantized(case1.bits, case1.q, k, 1024, metric, [fb] * nq)
        want = case1.source.search(case1.q, k, metric, [fs] * nq)
        for name in ("block_ids", "doc_ids", "rows", "dist", "counts"):
            np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)
        assert (got.counts == k).all()
    fb.free()
    fs.free()


def test_fewer_permitted_rows_than_k(ctx, case1):
    mask = np.zeros(case1.n, dtype=np.uint8)
    mask[[3, 77, 1500, 1501, 2999, 4000, 4999]] = 1
    fb = case1.bits.filter_from_bytemask(mask)
    for shortlist in (10, 2048):
        res = case1.source.search_quantized(case1.bits, case1.q[:4], 10, shortlist, "cosine", [fb] * 4)
        assert (res.counts == 7).all()
        for i in range(4):
            _expect(case1.model, res, i, case1.model.rerank("cosine", case1.q[i], 10, np.flatnonzero(mask)), 10)
        assert (res.block_ids[:, 7:] == -1).all() and (res.rows[:, 7:] == -1).all() and np.isposinf(res.dist[:, 7:]).all()
        _never_flags(ctx, res, 4)
    fb.free()


# ---------------------------------------------------------------------------------------------
# 5. the longest shortlist, all of it returned
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_k_equals_shortlist_equals_max_k(ctx, oracle, half):
    import vsrbac
    assert vsrbac.MAX_K == 2048
    case = Case(ctx, oracle, 5, 2500, 24, half=half, n_docs=30)
    for metric in ("l2", "cosine"):
        res = case.source.search_quantized(case.bits, case.q[:3], 2048, 2048, metric)
        assert (res.counts == 2048).all()
        for i in range(3):
            S = case.model.shortlist(case.ham[i], 2048)
            _expect(case.model, res, i, case.model.rerank(metric, case.q[i], 2048, S), 2048)
    case.free()


# ---------------------------------------------------------------------------------------------
# 6. the device API: raw keys, row_offset, sessions
# ---------------------------------------------------------------------------------------------
def _device_outputs(torch, dev, nq, k):
    o = SimpleNamespace(blk=torch.empty((nq, k), dtype=torch.int64, device=dev), doc=torch.empty((nq, k), dtype=torch.int32, device=dev),
                        row=torch.empty((nq, k), dtype=torch.int64, device=dev), dist=torch.empty((nq, k), dtype=torch.float32, device=dev),
                        cnt=torch.empty((nq,), dtype=torch.int32, device=dev), keys=torch.empty((nq, k), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()                                  # the library runs on its own stream
    return o


def _as_result(o):
    return SimpleNamespace(block_ids=o.blk.cpu().numpy(), doc_ids=o.doc.cpu().numpy(), rows=o.row.cpu().numpy(),
                           dist=o.dist.cpu().numpy(), counts=o.cnt.cpu().numpy())


def test_device_api_keys_and_sessions(ctx, oracle):
    import torch
    import vsrbac
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    n, dim, k, shortlist, nq, off = 5000, 40, 10, 37, 9, 1000
    x, q = _ints(rng, (n, dim)), _ints(rng, (nq, dim))
    blk, doc = _ids(n, 50)                                    # load order = internal order: key rows are caller rows
    model = QuantizedModel(oracle, x, doc, blk)
    want = model.search("cosine", q, k, shortlist)
    source = ctx.load_corpus(x, blk, doc, row_offset=off)
    bits = source.binary_quantize()
    buf = torch.zeros((1 + q.size,), dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(q.ravel().copy()).to(dev)      # 4-byte aligned, not 16
    torch.cuda.synchronize()
    session = vsrbac.Context(0)

    def run(sess, o):
        source.search_quantized_device(bits, _p(buf, 4), nq, k, shortlist, "cosine", None, _p(o.blk), _p(o.doc), _p(o.row), _p(o.dist),
                                       _p(o.cnt), _p(o.keys), session=sess)

    def check(o):
        got = _as_result(o)
        for i in range(nq):
            _expect(model, got, i, want[i], k)
        keys = o.keys.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.int64), got.rows + off)
        assert (keys[:, 1:] > keys[:, :-1]).all()             # the keys sort as the output is ordered

    for sess in (None, session):
        o = _device_outputs(torch, dev, nq, k)
        run(sess, o)
        (sess or ctx).synchronize()
        _ran(sess or ctx)
        check(o)
    a, b = _device_outputs(torch, dev, nq, k), _device_outputs(torch, dev, nq, k)
    run(None, a)                                              # two calls in flight, one per session
    run(session, b)
    ctx.synchronize()
    session.synchronize()
    check(a)
    check(b)
    # screening switches and query hints belong to other paths
    ctx.set_screening(False)
    ctx.set_query_hint(True)
    o = _device_outputs(torch, dev, nq, k)
    run(None, o)
    ctx.synchronize()
    check(o)
    ctx.set_screening(True)
    ctx.set_query_hint(False)
    session.close()
    bits.free()
    source.free()


# ---------------------------------------------------------------------------------------------
# 7. real-valued rows
# ---------------------------------------------------------------------------------------------
def test_real_valued_rows(ctx, oracle):
    rng = np.random.default_rng(7)
    n, dim, k, nq = 4000, 768, 10, 8
    centres = rng.normal(0, 1, (40, dim))
    x = (centres[rng.integers(0, 40, n)] + 0.6 * rng.normal(0, 1, (n, dim))).astype(np.float32)
    q = (x[rng.choice(n, nq, replace=False)] + 0.3 * rng.normal(0, 1, (nq, dim))).astype(np.float32)
    model = QuantizedModel(oracle, x)
    source = ctx.load_corpus(x)
    bits = source.binary_quantize()
    x64 = x.astype(np.float64)
    last = np.full(nq, -1.0)
    for shortlist in (10, 100, 1000):
        res = source.search_quantized(bits, q, k, shortlist, "cosine")
        want = model.search("cosine", q, k, shortlist)
        for i in range(nq):
            idx, _, S = want[i]
            rows = res.rows[i]
            assert res.counts[i] == k and len(set(rows.tolist())) == k and np.isin(rows, S).all()
            q64 = q[i].astype(np.float64)
            ref = 1.0 - (x64[rows] @ q64) / np.sqrt((x64[rows] ** 2).sum(1) * (q64 ** 2).sum())
            assert np.abs(res.dist[i] - ref).max() <= 1e-4
            assert (res.dist[i][1:] >= res.dist[i][:-1]).all()
            exact_rows, _ = model.exact("cosine", q[i], k)
            r_gpu, r_model = recall(rows, exact_rows), recall(idx, exact_rows)
            assert abs(r_gpu - r_model) <= 1.0 / k + 1e-12, (shortlist, i, r_gpu, r_model)    # one position of slack: near-ties inside 1e-4
            assert r_gpu >= last[i], (shortlist, i, r_gpu, last[i])
            last[i] = r_gpu
        _never_flags(ctx, res, nq)
    bits.free()
    source.free()


# ---------------------------------------------------------------------------------------------
# 8. arguments
# ---------------------------------------------------------------------------------------------
def test_arguments(ctx, oracle, case1):
    import vsrbac
    src, bits, q = case1.source, case1.bits, case1.q[:2]

    def refused(status, word, fn):
        with pytest.raises(vsrbac.VsrError) as e:
            fn()
        assert e.value.status == status and word in str(e.value), (e.value.status, str(e.value))

    loaded = ctx.load_corpus_bit(bit_model.binary_quantize(case1.x), case1.dim, case1.blk, case1.doc)
    refused(1, "vsr_corpus_load_bit", lambda: src.search_quantized(loaded, q, 5, 10))
    other = ctx.load_corpus(case1.x, case1.blk, case1.doc)
    other_bits = other.binary_quantize()
    refused(1, "was not made from source corpus", lambda: src.search_quantized(other_bits, q, 5, 10))
    other.free()                                              # either may go first
    again = ctx.load_corpus(case1.x, case1.blk, case1.doc)   # the same rows loaded again are another corpus
    refused(1, "was not made from source corpus", lambda: again.search_quantized(other_bits, q, 5, 10))
    refused(1, "shorter than k", lambda: src.search_quantized(bits, q, 11, 10))
    refused(1, "k must be >= 1", lambda: src.search_quantized(bits, q, 0, 10))
    refused(1, "VSR_MAX_K", lambda: src.search_quantized(bits, q, 5, vsrbac.MAX_K + 1))
    refused(6, "L1", lambda: src.search_quantized(bits, q, 5, 10, "l1"))
    refused(1, "metric 4", lambda: src.search_quantized(bits, q, 5, 10, "hamming"))
    f_src = src.filter_from_bytemask(np.ones(case1.n, dtype=np.uint8))
    refused(1, "belongs to another corpus", lambda: src.search_quantized(bits, q, 5, 10, "l2", [f_src, None]))
    f_src.free()
    wide = np.zeros((2, case1.dim + 1), dtype=np.float32)
    refused(2, f"different vector dimensions {case1.dim} and {case1.dim + 1}", lambda: src.search_quantized(bits, wide, 5, 10))
    refused(1, "source corpus is a bit corpus", lambda: bits.search_quantized(bits, q, 5, 10))
    refused(1, "not a bit corpus", lambda: src.search_quantized(src, q, 5, 10))
    half = ctx.load_corpus_half(case1.x[:100], case1.blk[:100], case1.doc[:100])
    half_bits = half.binary_quantize()
    refused(2, f"different halfvec dimensions {case1.dim} and {case1.dim + 1}", lambda: half.search_quantized(half_bits, wide, 5, 10))
    big = q.copy()
    big[1, 2] = 70000.0
    refused(1, "out of range for type halfvec", lambda: half.search_quantized(half_bits, big, 5, 10))
    for c in (half_bits, half, other_bits, again, loaded):
        c.free()
    # the handles are as good as before
    case1.check_sweep(ctx, "l2", vsrbac.RANGES, sweep=[(10, 37)])
    case1.check_sweep(ctx, "cosine", None, sweep=[(10, 37)])
