"""The two-stage search through the bit IVFFlat index on the GPU (vsr_ivf_search_quantized*: K3q shortlist from the lists of a
vsr_ivf_load_bit index, shortlist_rerank_kernel on the source rows) against tests/ivf_quantized_model.py.

Indexes are loaded from hand-written centres and row -> list assignments, so list shapes are the test's: sizes 0, 1, 63, 64, 65,
700 and the rest put list starts on, before and after the 64-row words of a step, and two centres are equal (the list id
decides).  Integer-valued rows and queries (-8 .. 8) have exact sums in fp32 and binary16, so ids, fp32 distances, counts and
the lists scanned must equal the model's bit for bit; real-valued rows compare within 1e-4, like the exact search's tests."""
import ctypes

from types import SimpleNamespace

import numpy as np
import pytest

import bit_model
from ivf_quantized_model import IvfQuantizedModel

pytestmark = pytest.mark.gpu

METRICS = ("l2", "ip", "cosine")
LISTS = 7
NAME = "ivf_bit_shortlist_kernel + shortlist re-rank"


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


def _list_sizes(n):
    """By list id; starts at 0, 63, 64, 128, 128, 193 and 193 + min(700, ...): before, on and after 64-row words."""
    big = 700 if n >= 2000 else 50
    return [63, 1, 64, 0, 65, big, n - 193 - big]


def _row_list(rng, n):
    sizes = _list_sizes(n)
    assert min(sizes) >= 0 and sum(sizes) == n
    return rng.permutation(np.repeat(np.arange(LISTS), sizes)).astype(np.int32)


def _centers(rng, dim):
    c = rng.random((LISTS, dim)) < 0.5
    c[3] = c[2]                                              # equal Hamming counts for every query: the lower list id first
    return bit_model.set_pad_bits(bit_model.pack(c), dim)   # pad bits of the centres are ignored


def _expect(model, res, qi, idx, dist):
    m = res.counts[qi]
    assert m == idx.size, (qi, m, idx.size)
    np.testing.assert_array_equal(res.rows[qi, :m], idx)
    np.testing.assert_array_equal(res.block_ids[qi, :m], model.blk[idx])
    np.testing.assert_array_equal(res.doc_ids[qi, :m], model.doc[idx])
    np.testing.assert_array_equal(res.dist[qi, :m], dist.astype(np.float32))
    assert (res.block_ids[qi, m:] == -1).all() and (res.doc_ids[qi, m:] == -1).all() and (res.rows[qi, m:] == -1).all()
    assert np.isposinf(res.dist[qi, m:]).all()


class Case:
    """A source corpus, its quantized corpus, the hand-made index over it, the model and a few queries."""

    def __init__(self, ctx, oracle, seed, n, dim, half=False, n_docs=60, nq=3, row_offset=0, ordered_ids=False):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.half = n, dim, half
        self.x = _ints(rng, (n, dim))
        if ordered_ids:                                      # load order = internal order: key rows are caller rows
            self.blk, self.doc = (np.arange(n) + 1).astype(np.int64), (np.arange(n) // 50 + 1).astype(np.int32)
        else:
            self.blk, self.doc = rng.permutation(n).astype(np.int64) + 1, rng.integers(1, n_docs + 1, n).astype(np.int32)
        self.q = _ints(rng, (nq, dim))
        load = ctx.load_corpus_half if half else ctx.load_corpus
        self.source = load(self.x, self.blk, self.doc, row_offset=row_offset)
        self.bits = self.source.binary_quantize()
        self.centers, self.row_list = _centers(rng, dim), _row_list(rng, n)
        self.index = self.bits.load_ivf_bit(self.centers, self.row_list)
        self.model = IvfQuantizedModel(oracle, self.x, self.centers, self.row_list, self.doc, self.blk, half=half)

    def check(self, ctx, metric, k, shortlist, probes, mode, max_probes, filters=None, masks=None, q=None):
        q = self.q if q is None else q
        res, scanned = self.source.search_quantized_ivf(self.index, q, k, shortlist, probes, metric, filters, mode, max_probes)
        assert ctx.last_scan_kernel() == NAME
        for i in range(len(q)):
            idx, dist, _, want_scanned = self.model.search(metric, q[i], k, shortlist, probes, mode, max_probes,
                                                           None if masks is None else masks[i])
            tag = (metric, k, shortlist, probes, mode, max_probes, i)
            assert scanned[i] == want_scanned, (tag, scanned[i], want_scanned)
            _expect(self.model, res, i, idx, dist)
        return res, scanned

    def free(self):
        self.index.free()
        self.bits.free()
        self.source.free()


# ---------------------------------------------------------------------------------------------
# 1. against the model, integer-valued data: bit for bit
# ---------------------------------------------------------------------------------------------
MODES = (("off", 1), ("relaxed_order", 1), ("relaxed_order", 2), ("relaxed_order", LISTS))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "halfvec"])
@pytest.mark.parametrize("dim,n", [(16, 3000), (52, 3000), (128, 3000), (768, 3000), (1032, 3000), (8200, 300)])
def test_against_the_model(ctx, oracle, dim, n, half):
    case = Case(ctx, oracle, 100 + dim, n, dim, half=half, n_docs=45)
    combo = 0
    for pi, probes in enumerate((1, 3, 7, 50)):
        for si, shortlist in enumerate((10, 100, 512, 513, 2048)):
            for mi, (mode, max_probes) in enumerate(MODES):
                metric = METRICS[(pi + si + mi) % 3]
                k = shortlist if si == 0 or (si == 4 and mi == pi) else 10      # shortlist = k at both ends
                case.check(ctx, metric, k, shortlist, probes, mode, max_probes)
                combo += 1
    assert combo == 80
    ctx.screening_check(len(case.q))                         # (raises if the re-rank's bounds guard tripped)
    case.free()


def test_hamming_ties_at_the_cut(ctx, oracle):
    case = Case(ctx, oracle, 3, 3000, 16, n_docs=45, nq=5)   # 17 Hamming values over 3000 rows
    ham = case.model.qm.hamming(case.q)
    for shortlist in (50, 300):
        inside = 0
        for i in range(5):
            S, _ = case.model.shortlist(case.q[i], shortlist, LISTS)
            cut = ham[i][S].max()
            inside += int((ham[i] == cut).sum() > (ham[i][S] == cut).sum())
        assert inside >= 3                                   # the cut really falls inside a tie (a property of the data)
        res, _ = case.check(ctx, "l2", shortlist, shortlist, LISTS, "off", 1)
        case.check(ctx, "l2", 10, shortlist, 2, "relaxed_order", LISTS)
    case.free()


# ---------------------------------------------------------------------------------------------
# 2. against the existing GPU paths, real-valued data
# ---------------------------------------------------------------------------------------------
def test_real_valued_rows_against_the_existing_paths(ctx, oracle):
    rng = np.random.default_rng(7)
    n, dim, k, nq, lists = 4000, 768, 10, 8, 40
    centres = rng.normal(0, 1, (lists, dim))
    x = (centres[rng.integers(0, lists, n)] + 0.6 * rng.normal(0, 1, (n, dim))).astype(np.float32)
    q = (x[rng.choice(n, nq, replace=False)] + 0.3 * rng.normal(0, 1, (nq, dim))).astype(np.float32)
    packed = bit_model.binary_quantize(centres)
    model = IvfQuantizedModel(oracle, x, packed)             # (rows go to their nearest centre)
    source = ctx.load_corpus(x)
    bits = source.binary_quantize()
    index = bits.load_ivf_bit(packed, model.ivf.assign)
    x64 = x.astype(np.float64)
    for metric in METRICS:
        for shortlist in (10, 100, 1000):
            # every list probed, iterative scan off: the scanned two-stage search, byte for byte
            got, scanned = source.search_quantized_ivf(index, q, k, shortlist, lists, metric)
            want = source.search_quantized(bits, q, k, shortlist, metric)
            for name in ("block_ids", "doc_ids", "rows", "dist", "counts"):
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (metric, shortlist, name)
            assert (scanned == lists).all()
    qb = bit_model.binary_quantize(q)
    for mode, probes, max_probes in (("off", 3, 1), ("relaxed_order", 1, 5), ("relaxed_order", 2, lists)):
        for shortlist in (10, 400):
            # k = shortlist: the whole shortlist comes back; it is the index scan's answer on the bits
            got, scanned = source.search_quantized_ivf(index, q, shortlist, shortlist, probes, "cosine", None, mode, max_probes)
            s1, s1_scanned = index.search_bit_iterative(qb, shortlist, probes, "hamming", None, mode, max_probes)
            np.testing.assert_array_equal(scanned, s1_scanned)
            np.testing.assert_array_equal(got.counts, s1.counts)
            for i in range(nq):
                m = got.counts[i]
                assert set(got.rows[i, :m].tolist()) == set(s1.rows[i, :m].tolist())
                S, want_scanned = model.shortlist(q[i], shortlist, probes, mode, max_probes)
                assert set(S.tolist()) == set(got.rows[i, :m].tolist()) and want_scanned == scanned[i]
                rows = got.rows[i, :m]
                q64 = q[i].astype(np.float64)
                ref = 1.0 - (x64[rows] @ q64) / np.sqrt((x64[rows] ** 2).sum(1) * (q64 ** 2).sum())
                assert np.abs(got.dist[i, :m] - ref).max() <= 1e-4
                assert (got.dist[i, 1:m] >= got.dist[i, :m - 1]).all()
    index.free()
    bits.free()
    source.free()


# ---------------------------------------------------------------------------------------------
# 3. filters
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case3(ctx, oracle):
    c = Case(ctx, oracle, 31, 3000, 52, n_docs=300, nq=6)
    yield c
    c.free()


def test_filters_of_the_bit_corpus(ctx, case3):
    import vsrbac
    from vsrbac.datasets import tree_rbac
    rbac = tree_rbac(num_users=12, num_roles=9, num_docs=300, seed=5)
    case3.bits.load_rbac(rbac.user_roles, rbac.permissions)
    users = [1 + i % 12 for i in range(6)]
    user_masks = [bit_model.user_row_mask(u, rbac.user_roles, rbac.permissions, case3.doc) for u in users]
    assert any(m.any() for m in user_masks)
    rng = np.random.default_rng(32)
    bytemask = (rng.random(case3.n) < 0.3).astype(np.uint8)
    f_mask, f_none = case3.bits.filter_from_bytemask(bytemask), case3.bits.filter_from_bytemask(np.zeros(case3.n, np.uint8))
    settings = [(None, None)]
    for fmode in (vsrbac.RANGES, vsrbac.BITMAP):
        settings.append(([case3.bits.filter_for_user(u, fmode) for u in users], user_masks))
    settings.append(([f_mask] * 6, [bytemask] * 6))
    settings.append(([f_mask, None, f_none, f_mask, None, f_none], [bytemask, None, np.zeros(case3.n, np.uint8)] * 2))
    for si, (filters, masks) in enumerate(settings):
        for ci, (probes, shortlist, mode, max_probes) in enumerate(((1, 100, "off", 1), (2, 100, "relaxed_order", 5), (1, 513, "relaxed_order", LISTS),
                                                                    (50, 2048, "off", 1), (3, 10, "relaxed_order", 4))):
            case3.check(ctx, METRICS[(si + ci) % 3], 10, shortlist, probes, mode, max_probes, filters, masks)
    # a mask admitting no row: count 0, full fill, every list the scan may take taken
    res, scanned = case3.check(ctx, "l2", 10, 100, 2, "relaxed_order", LISTS, [f_none] * 6, [np.zeros(case3.n, np.uint8)] * 6)
    assert (res.counts == 0).all() and (res.rows == -1).all() and np.isposinf(res.dist).all() and (scanned == LISTS).all()
    f_mask.free()
    f_none.free()


@pytest.mark.parametrize("metric", METRICS)
def test_a_mask_that_fits_the_shortlist_is_the_exact_search(ctx, case3, metric):
    rng = np.random.default_rng(33)
    mask = np.zeros(case3.n, dtype=np.uint8)
    mask[rng.choice(case3.n, 90, replace=False)] = 1
    fb, fs = case3.bits.filter_from_bytemask(mask), case3.source.filter_from_bytemask(mask)
    nq = len(case3.q)
    for k in (10, 90):
        got, scanned = case3.source.search_quantized_ivf(case3.index, case3.q, k, 100, 1, metric, [fb] * nq, "relaxed_order", LISTS)
        want = case3.source.search(case3.q, k, metric, [fs] * nq)
        for name in ("block_ids", "doc_ids", "rows", "dist", "counts"):
            np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)
        assert (got.counts == k).all() and (scanned == LISTS).all()
    # one list, iterative scan off: the same mask returns only what that list holds
    got, scanned = case3.source.search_quantized_ivf(case3.index, case3.q, 10, 100, 1, metric, [fb] * nq, "off", LISTS)
    assert (scanned == 1).all()
    for i in range(nq):
        first = case3.model.ivf.probe(bit_model.binary_quantize(case3.q[i])[0], 1)[0]
        held = np.flatnonzero(mask.astype(bool) & (case3.row_list == first))
        m = got.counts[i]
        assert m == min(10, held.size) and np.isin(got.rows[i, :m], held).all() and (got.rows[i, m:] == -1).all()
    case3.check(ctx, metric, 10, 100, 1, "off", LISTS, [fb] * nq, [mask] * nq)
    fb.free()
    fs.free()


# ---------------------------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------------------------
def test_query_counts(ctx, oracle, case3):
    rng = np.random.default_rng(41)
    res, scanned = case3.source.search_quantized_ivf(case3.index, np.zeros((0, case3.dim), np.float32), 10, 100, 2)
    assert res.rows.shape == (0, 10) and scanned.shape == (0,)
    q = _ints(rng, (65, case3.dim))
    case3.check(ctx, "l2", 10, 100, 2, "relaxed_order", 4, q=q[:1])
    case3.check(ctx, "cosine", 10, 513, 1, "relaxed_order", LISTS, q=q)


def test_zero_negative_zero_and_nan_quantize_to_zero(ctx, case3):
    q = case3.q[:3].copy()
    q[0, ::3], q[0, 1::3] = 0.0, -0.0
    q[1, :] = np.where(np.arange(case3.dim) % 2 == 0, -0.0, 0.0)          # the all-zero string
    q[2, 5], q[2, 17] = np.nan, np.nan
    qb = bit_model.binary_quantize(q)
    assert not qb[1].any() and np.array_equal(ctx.binary_quantize(q), qb)
    case3.check(ctx, "l2", 10, 100, 2, "relaxed_order", LISTS, q=q[:2])
    # the NaN elements give bit 0; every distance to that query is NaN, so only the shortlist itself is compared
    got, scanned = case3.source.search_quantized_ivf(case3.index, q[2:], 100, 100, 2, "l2", None, "relaxed_order", LISTS)
    S, want_scanned = case3.model.shortlist(q[2], 100, 2, "relaxed_order", LISTS)
    assert got.counts[0] == 100 and set(got.rows[0].tolist()) == set(S.tolist()) and scanned[0] == want_scanned


def _device_outputs(torch, dev, nq, k):
    o = SimpleNamespace(blk=torch.empty((nq, k), dtype=torch.int64, device=dev), doc=torch.empty((nq, k), dtype=torch.int32, device=dev),
                        row=torch.empty((nq, k), dtype=torch.int64, device=dev), dist=torch.empty((nq, k), dtype=torch.float32, device=dev),
                        cnt=torch.empty((nq,), dtype=torch.int32, device=dev), keys=torch.empty((nq, k), dtype=torch.int64, device=dev),
                        probes=torch.empty((nq,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()                                  # the library runs on its own stream
    return o


def _as_result(o):
    return SimpleNamespace(block_ids=o.blk.cpu().numpy(), doc_ids=o.doc.cpu().numpy(), rows=o.row.cpu().numpy(),
                           dist=o.dist.cpu().numpy(), counts=o.cnt.cpu().numpy())


def test_device_api_row_offset_alignment_and_calls_in_flight(ctx, oracle):
    import torch
    dev = torch.device("cuda", 0)
    n, dim, k, shortlist, nq, off = 3000, 52, 10, 100, 9, 1000
    case = Case(ctx, oracle, 6, n, dim, nq=nq, row_offset=off, ordered_ids=True)
    buf = torch.zeros((1 + case.q.size,), dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(case.q.ravel().copy()).to(dev)             # 4-byte aligned, not 16
    torch.cuda.synchronize()
    rng = np.random.default_rng(61)
    masks = [(rng.random(n) < p).astype(np.uint8) for p in (0.5, 0.02)]
    f = [case.bits.filter_from_bytemask(m) for m in masks]

    def run(o, filters, probes=2, mode="relaxed_order", max_probes=LISTS):
        return case.source.search_quantized_ivf_device(case.index, _p(buf, 4), nq, k, shortlist, probes, "cosine", filters, mode, max_probes,
                                                       _p(o.blk), _p(o.doc), _p(o.row), _p(o.dist), _p(o.cnt), _p(o.probes), _p(o.keys))

    def check(o, mask, probes=2, mode="relaxed_order", max_probes=LISTS):
        got = _as_result(o)
        scanned = o.probes.cpu().numpy()
        for i in range(nq):
            idx, dist, _, want_scanned = case.model.search("cosine", case.q[i], k, shortlist, probes, mode, max_probes, mask)
            assert scanned[i] == want_scanned
            _expect(case.model, got, i, idx, dist)
        keys = o.keys.cpu().numpy().view(np.uint64)
        live = got.rows >= 0
        np.testing.assert_array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.int64)[live], (got.rows + off)[live])   # the source's offset
        assert (keys[~live] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        assert (keys[:, 1:] >= keys[:, :-1]).all()

    o = _device_outputs(torch, dev, nq, k)
    keep = run(o, None, probes=1, mode="off")
    ctx.synchronize()
    assert ctx.last_scan_kernel() == NAME
    check(o, None, probes=1, mode="off")
    for j in range(2):                                        # each filter's view-order bitmap exists from here on
        keep = run(o, [f[j]] * nq)
        ctx.synchronize()
        check(o, masks[j])
    # two calls with different filters behind each other, one wait: each sees its own table of bitmap addresses
    a, b = _device_outputs(torch, dev, nq, k), _device_outputs(torch, dev, nq, k)
    keep_a = run(a, [f[0]] * nq)
    keep_b = run(b, [f[1]] * nq)
    ctx.synchronize()
    check(a, masks[0])
    check(b, masks[1])
    del keep, keep_a, keep_b
    # out_probes and out_keys may be NULL
    o = _device_outputs(torch, dev, nq, k)
    case.source.search_quantized_ivf_device(case.index, _p(buf, 4), nq, k, shortlist, 2, "cosine", None, "relaxed_order", LISTS, _p(o.blk), _p(o.doc),
                                            _p(o.row), _p(o.dist), _p(o.cnt))
    ctx.synchronize()
    got = _as_result(o)
    for i in range(nq):
        idx, dist, _, _ = case.model.search("cosine", case.q[i], k, shortlist, 2, "relaxed_order", LISTS)
        _expect(case.model, got, i, idx, dist)
    for x in f:
        x.free()
    case.free()


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(ctx, oracle, case3):
    import vsrbac
    src, index, q = case3.source, case3.index, case3.q[:2]

    def refused(status, word, fn):
        with pytest.raises(vsrbac.VsrError) as e:
            fn()
        assert e.value.status == status and word in str(e.value), (e.value.status, str(e.value))

    refused(6, "L1", lambda: src.search_quantized_ivf(index, q, 5, 10, 1, "l1"))
    refused(1, "shorter than k", lambda: src.search_quantized_ivf(index, q, 11, 10))
    refused(1, "VSR_MAX_K", lambda: src.search_quantized_ivf(index, q, 5, vsrbac.MAX_K + 1))
    centers32 = np.zeros((3, case3.dim), dtype=np.float32)
    centers32[1], centers32[2] = 1.0, -1.0
    index32 = src.load_ivf(centers32, src.ivf_assign(centers32))
    refused(1, "the index is not over a bit corpus", lambda: src.search_quantized_ivf(index32, q, 5, 10))
    index32.free()
    other = ctx.load_corpus(case3.x, case3.blk, case3.doc)   # the same rows loaded again are another corpus
    refused(1, "was not made from source corpus", lambda: other.search_quantized_ivf(index, q, 5, 10))
    other.free()
    f_src = src.filter_from_bytemask(np.ones(case3.n, dtype=np.uint8))
    refused(1, "belongs to another corpus", lambda: src.search_quantized_ivf(index, q, 5, 10, 1, "l2", [f_src, None]))
    f_src.free()
    refused(1, "probes must be >= 1", lambda: src.search_quantized_ivf(index, q, 5, 10, 0))
    refused(1, "iterative scan mode 3", lambda: src.search_quantized_ivf(index, q, 5, 10, 1, "l2", None, 3))
    refused(1, "max_probes must be between 1 and 32768", lambda: src.search_quantized_ivf(index, q, 5, 10, 1, "l2", None, "relaxed_order", 0))
    wide = np.zeros((2, case3.dim + 1), dtype=np.float32)
    refused(2, f"different vector dimensions {case3.dim} and {case3.dim + 1}", lambda: src.search_quantized_ivf(index, wide, 5, 10))
    # the handles are as good as before
    case3.check(ctx, "l2", 10, 100, 2, "relaxed_order", LISTS)
