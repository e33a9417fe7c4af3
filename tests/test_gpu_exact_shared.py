"""K1m (csrc/vsr_mq.h, mq_scan_kernel), the exact shared-pass scan every other tier falls back on, at its own edges.  The
inputs are test_exact_shared_cpu.py's, pinned there without a GPU.

Everything is compared with the CPU oracle bit for bit (integer values: every fp32 partial sum is exact) -- rows, order,
distances, ids, counts, padding.  Cosine is the exception: 1 - x.q / sqrt(|x|^2 |q|^2) is rounded differently by the kernel
(one division in double) and by the oracle, so it is held to the float64 reference through helpers.assert_valid_topk at
test_gpu_parity.py's TOL, and to the oracle's distances with allclose at the same TOL; its NaN tail (all-zero rows) must be
the oracle's rows in the oracle's order.

  1. the list-length edges of the candidate buffers (cap = the first power of two >= 2k + 256, trigger = cap - 256), all four
     metrics, q_count 1 .. 16, ragged last stage (d = 100), RANGES and BITMAP parts, one and several workgroups per pass,
     block map and binary search: test_k1m_list_length_edges, test_cosine_zero_rows_come_last
  2. the row lengths: test_row_length_edges, test_one_row_and_rw_minus_one_row_tiles
  3. the seeded run (SAMPLE = true, tau_init, K5's flag): test_seeded_run_*
  4. a rank map (an IVFFlat view): test_k1m_over_a_rank_map

Kernel names observed on an MI355X are asserted in every call named above (last_scan_kernel)."""
import contextlib
import math

import numpy as np
import pytest

import test_exact_shared_cpu as cpu
from helpers import assert_valid_topk
from oracle.oracle import IvfIndex as OracleIvf
from test_gpu_parity import TOL, _expect_exact, _ref_all
from test_screen_edges import FINE, _Dev, _check_one

pytestmark = pytest.mark.gpu

KS = cpu.KS
NAMES = {"l2": "L2", "ip": "IP", "cosine": "COSINE", "l1": "L1"}


def _k1m(metric):
    return f"vsr::mq_scan_kernel<{NAMES[metric]}, SAMPLE=false> (K1m)"


@contextlib.contextmanager
def _context(monkeypatch, env=None, screening=None):
    """A fresh context opened under `env`; screening: set_screening's argument, None = leave the default."""
    import vsrbac
    for name, v in (env or {}).items():
        monkeypatch.setenv(name, v)
    ctx = vsrbac.Context(0)
    for name in env or {}:
        monkeypatch.delenv(name)
    try:
        if screening is not None:
            ctx.set_screening(screening)
        yield ctx
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def ctx_default():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    import vsrbac
    c = vsrbac.Context(0)
    c.set_screening(False)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the list-length edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    return cpu.exact_world()


@pytest.fixture(scope="module")
def zero_world():
    return cpu.zero_rows_world()


_COS = {}


def _check_cosine(oracle, w, res, j, i, k, metric="cosine"):
    """Query i of the world as row j of `res`: a valid top k of the float64 reference within TOL, the oracle's distances
    within TOL, NaN distances last and on the oracle's rows, padding behind the count."""
    rows = w.allowed_rows(oracle, int(w.quser[i]))
    if (id(w), int(i)) not in _COS:
        ref = np.full(w.n, np.nan)
        ref[rows] = _ref_all("cosine", w.x[rows], w.q[i])
        _COS[(id(w), int(i))] = ref
    ref = _COS[(id(w), int(i))]
    oidx, odist = w.ref(oracle, i, "cosine")
    oidx, odist = oidx[:k], odist[:k]
    m = int(res.counts[j])
    assert m == min(k, rows.size) == oidx.size, (k, int(i), m, rows.size)
    assert_valid_topk(res.rows[j, :m], res.dist[j, :m], ref, k, TOL, candidates=rows)
    np.testing.assert_allclose(res.dist[j, :m], odist, rtol=TOL, atol=TOL, equal_nan=True)
    nan = np.isnan(odist)
    np.testing.assert_array_equal(np.isnan(res.dist[j, :m]), nan)
    if nan.any():
        assert nan[np.argmax(nan):].all()
        np.testing.assert_array_equal(res.rows[j, :m][nan], oidx[nan])
    np.testing.assert_array_equal(res.block_ids[j, :m], w.blk[res.rows[j, :m]])
    np.testing.assert_array_equal(res.doc_ids[j, :m], w.doc[res.rows[j, :m]])
    assert (res.rows[j, m:] == -1).all() and (res.block_ids[j, m:] == -1).all() and (res.doc_ids[j, m:] == -1).all()
    assert np.isposinf(res.dist[j, m:]).all()


def _run_edges(oracle, ctx, w, metric, short_calls=True):
    """Every k of KS in RANGES and BITMAP mode: calls of 3 and of all queries through vsr_search, of all queries through
    vsr_search_device; K1m in every call of all queries, every query against the oracle, nothing flagged."""
    import vsrbac
    check = _check_cosine if metric == "cosine" else _check_one
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(*w.rbac())
    everybody = np.arange(w.nq)
    flagged_before = ctx.screening_check(0)[0]
    for mode in (vsrbac.RANGES, vsrbac.BITMAP):
        per_user = {int(u): corpus.filter_for_user(int(u), mode) for u in np.unique(w.quser)}
        filters = [per_user[int(u)] for u in w.quser]
        for ki, k in enumerate(KS):
            s = (37 * ki + 5) % (w.nq - 3)
            for sel in ([np.arange(s, s + 3)] if short_calls else []) + [everybody]:
                res = corpus.search(w.q[sel], k, metric, [filters[i] for i in sel])
                if sel.size == w.nq:
                    assert ctx.last_scan_kernel() == _k1m(metric), (mode, k)
                assert (res.counts >= 0).all()
                for j, i in enumerate(sel):
                    check(oracle, w, res, j, i, k, metric)
            b = _Dev(w.q, k)
            keep = corpus.search_device(b.qp(), w.nq, k, metric, filters, *b.args())
            ctx.synchronize()
            del keep
            assert ctx.last_scan_kernel() == _k1m(metric), (mode, k)
            _, flags = ctx.screening_check(w.nq)
            assert not flags.any(), (mode, k, np.flatnonzero(flags))
            got = b.result()
            assert (got.counts >= 0).all(), (mode, k, np.flatnonzero(got.counts < 0))
            for i in everybody:
                check(oracle, w, got, i, i, k, metric)
    assert ctx.screening_check(0)[0] == flagged_before
    corpus.free()


NO_SCREENING = {"VSR_NO_SCREENING": "1"}
CONFIGS = {
    # name: (environment at open, set_screening argument)
    "set_screening": ({}, False),
    "no_screening_env": (NO_SCREENING, None),
    "default": ({}, None),
    "no_xcd_map": ({"VSR_NO_XCD_MAP": "1"}, None),
    "fine": (FINE, None),
    "fine_no_screening": ({**FINE, **NO_SCREENING}, None),
}


@pytest.mark.parametrize("config,metric", [
    ("set_screening", "l2"), ("set_screening", "ip"), ("set_screening", "cosine"),
    ("no_screening_env", "l2"), ("no_screening_env", "ip"), ("no_screening_env", "cosine"),
    ("default", "l1"),
    ("no_xcd_map", "l1"),
    ("fine", "l1"), ("fine_no_screening", "l2"), ("fine_no_screening", "cosine")])
def test_k1m_list_length_edges(oracle, monkeypatch, world, config, metric):
    """L2, IP and cosine reach K1m with screening off (both switches), L1 in a default context.  no_xcd_map: workgroups find
    their pass by binary search over block_begin instead of the block map.  fine: test_screen_edges.py's switches, several
    workgroups per small pass, so K5 merges more than one list per query."""
    env, screening = CONFIGS[config]
    with _context(monkeypatch, env, screening) as ctx:
        _run_edges(oracle, ctx, world, metric)


def test_cosine_zero_rows_come_last(oracle, monkeypatch, zero_world):
    """Three all-zero rows, in the classes of 129 and 2049 allowed rows: NaN distances, last, in row order; the count stays
    min(k, allowed); at k = 2048 one of the two NaN rows of the class of 2049 is the last result."""
    w, zero = zero_world
    seen = 0
    for i in range(w.nq):
        idx, dist = w.ref(oracle, i, "cosine")
        nan = np.isnan(dist)
        assert np.isin(idx[nan], zero).all() and (np.diff(idx[nan]) > 0).all()
        seen += int(nan.any())
    assert seen == 5 + 33
    with _context(monkeypatch, {}, False) as ctx:
        _run_edges(oracle, ctx, w, "cosine", short_calls=False)


# ---------------------------------------------------------------------------------------------------------------------
# 2. row lengths
# ---------------------------------------------------------------------------------------------------------------------
def _ids(n, rows_per_doc=7):
    return (np.arange(n) + 1).astype(np.int64), (np.arange(n) // rows_per_doc + 1).astype(np.int32)


def _expect_kernel(name, metric, d):
    width, mq = cpu.expected_pass_width(d, cpu.ROW_K)
    if mq:
        assert name == _k1m(metric), (d, name)
    else:
        qi = 4 if width >= 4 else 1
        assert name.startswith(f"vsr::scan_kernel<{NAMES[metric]}, ") and name.endswith(f"QI={qi}> (K1)"), (d, name)
        assert ("C=0," in name) == ((d + 3) // 4 > 256), (d, name)             # rows of more than 256 chunks: the runtime-chunk kernel
    return width


@pytest.mark.parametrize("d", cpu.ROW_DIMS)
def test_row_length_edges(oracle, ctx_default, ctx_off, d):
    """L1 in a default context and L2 with screening off, 5 and 16 queries, unfiltered and under a 50 % mask (BITMAP and RANGES:
    tiles of one or two rows at every rw); n is no multiple of rw, so the last implicit tile is short.  K1m from d = 61 to
    5760; scan_kernel (K1) at d = 60 (QI = 4) and at d = 5761 (the runtime-chunk kernel; four of its padded queries and
    candidate lists pass K1's 72 KiB, so its passes carry one query: QI = 1).  Unfiltered calls also hold the restated
    queries per pass to the planner: pass rows = ceil(nq / width) x n."""
    import vsrbac
    x, q, mask = cpu.row_case(d)
    n, k = x.shape[0], cpu.ROW_K
    blk, doc = _ids(n)
    for ctx, metric in ((ctx_default, "l1"), (ctx_off, "l2")):
        corpus = ctx.load_corpus(x, blk, doc)
        filters = [(None, None), (corpus.filter_from_bytemask(mask, vsrbac.BITMAP), mask), (corpus.filter_from_bytemask(mask, vsrbac.RANGES), mask)]
        for f, m in filters:
            for nq in (5, 16):
                ctx.stats_reset()
                res = corpus.search(q[:nq], k, metric, f)
                width = _expect_kernel(ctx.last_scan_kernel(), metric, d)
                if f is None:
                    st = ctx.stats()
                    assert sum(st["scan_rows"]) == math.ceil(nq / width) * n, (d, nq, width, st["scan_rows"])
                for i in range(nq):
                    _expect_exact(oracle, res, i, metric, x, q[i], k, doc, blk, m)
        for f, _ in filters[1:]:
            f.free()
        corpus.free()


@pytest.mark.parametrize("d", cpu.SHORT_TILE_DIMS)
def test_one_row_and_rw_minus_one_row_tiles(oracle, ctx_default, ctx_off, d):
    """An RBAC of one-row documents in RANGES mode: the tile list is runs of 1 and of rw - 1 rows, starting at every offset,
    for rw = 32, 16, 8, 4 and 2."""
    import vsrbac
    x, q, doc, blk, ur, perms, allowed = cpu.short_tile_case(d)
    k = cpu.ROW_K
    for ctx, metric in ((ctx_default, "l1"), (ctx_off, "l2")):
        corpus = ctx.load_corpus(x, blk, doc)
        corpus.load_rbac(ur, perms)
        f = corpus.filter_for_user(1, vsrbac.RANGES)
        assert f.allowed_rows == f.scanned_rows == int(allowed.sum())
        for nq in (5, 16):
            res = corpus.search(q[:nq], k, metric, f)
            assert ctx.last_scan_kernel() == _k1m(metric), d
            for i in range(nq):
                _expect_exact(oracle, res, i, metric, x, q[i], k, doc, blk, allowed)
        corpus.free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the seeded run of an exact kernel
# ---------------------------------------------------------------------------------------------------------------------
_SEEDED = {}


def _seeded(adversarial):
    if adversarial not in _SEEDED:
        x, q = cpu.seeded_case(adversarial)
        blk, doc = _ids(x.shape[0], 50)
        _SEEDED[adversarial] = (x, q, blk, doc, {})
    return _SEEDED[adversarial]


def _seeded_exact(oracle, case, res, i, k):
    """Query i against the oracle's top max(SEEDED_KS), computed once per query (a smaller k is its head)."""
    x, q, blk, doc, refs = case
    if i not in refs:
        refs[i] = oracle.filtered_topk("l1", x, q[i], max(cpu.SEEDED_KS), doc, blk)
    idx, dist = refs[i][0][:k], refs[i][1][:k]
    assert res.counts[i] == k
    np.testing.assert_array_equal(res.rows[i], idx)
    np.testing.assert_array_equal(res.block_ids[i], blk[idx])
    np.testing.assert_array_equal(res.doc_ids[i], doc[idx])
    np.testing.assert_array_equal(res.dist[i], dist.astype(np.float32))


def _sampled_queries():
    return sorted(set(range(0, cpu.SEEDED_NQ, 37)) | set(cpu.ADVERSARIES))


@pytest.mark.parametrize("k", cpu.SEEDED_KS)
def test_seeded_run_is_exact(oracle, ctx_default, k):
    """512 unfiltered queries over 66 000 x 64, L1: 32 passes x 66 000 rows cross seed_min_rows and kp = k >= SEED_LIST, so
    search_general runs mq_scan_kernel<L1, SAMPLE=true>, seeds tau_init and scans under it.  No statistic counts the sample
    launch; as for K2h (test_gpu_halfvec_mfma.py) the pass rows that make it run are asserted -- the adversarial test below
    shows that it did.  On an ordinary corpus nothing is flagged and the results are exact."""
    ctx = ctx_default
    case = _seeded(False)
    x, q, blk, doc, _ = case
    corpus = ctx.load_corpus(x, blk, doc)
    ctx.stats_reset()
    res = corpus.search(q, k, "l1")
    assert ctx.last_scan_kernel() == _k1m("l1")
    st = ctx.stats()
    assert st["scan_rows"][1] >= 2_000_000, st["scan_rows"]
    for i in _sampled_queries():
        _seeded_exact(oracle, case, res, i, k)
    b = _Dev(q, k)
    corpus.search_device(b.qp(), cpu.SEEDED_NQ, k, "l1", None, *b.args())
    _, flags = ctx.screening_check(cpu.SEEDED_NQ)
    got = b.result()
    assert not flags.any() and (got.counts == k).all(), (np.flatnonzero(flags), np.flatnonzero(got.counts != k))
    for i in _sampled_queries():
        _seeded_exact(oracle, case, got, i, k)
    corpus.free()


@pytest.mark.parametrize("k", cpu.SEEDED_KS)
def test_seeded_run_flags_a_seed_that_is_too_tight(oracle, ctx_default, k):
    """The adversarial corpus: for five queries the 64 rows every sample visits are nearer than all others, so the seed --
    the m-th best sampled candidate, m <= SEED_LIST = 64 -- is the m-th nearest row and fewer than k rows pass it.  K5 must
    flag exactly those five (count -1 - m', m' < k; k = 100: select_radix_kernel, k = 600: select_kernel), publish the other
    507 exact, vsr_search_device_exact re-runs five and vsr_search returns the exact answer.  The flag is also the only
    outside evidence that the sample launch and tau_init ran.  (Observed on an MI355X: m' = 18 at k = 100, 49 at k = 600 --
    seed_rank at 32 workgroups per pass; nothing below depends on it.)"""
    ctx = ctx_default
    case = _seeded(True)
    x, q, blk, doc, _ = case
    nq = cpu.SEEDED_NQ
    adv = np.asarray(cpu.ADVERSARIES)
    corpus = ctx.load_corpus(x, blk, doc)
    b = _Dev(q, k)
    ctx.stats_reset()
    corpus.search_device(b.qp(), nq, k, "l1", None, *b.args())
    _, flags = ctx.screening_check(nq)
    assert ctx.last_scan_kernel() == _k1m("l1")
    assert ctx.stats()["scan_rows"][1] >= 2_000_000
    got = b.result()
    print(f"k = {k}: flagged {np.flatnonzero(flags).tolist()}, their counts {got.counts[flags != 0].tolist()}")
    np.testing.assert_array_equal(np.flatnonzero(flags), adv)
    np.testing.assert_array_equal(np.flatnonzero(got.counts < 0), adv)
    kept = -1 - got.counts[adv]
    assert ((kept >= 1) & (kept < k) & (kept <= cpu.NEAR_ROWS)).all(), kept
    others = np.delete(np.arange(nq), adv)
    for i in others:
        _seeded_exact(oracle, case, got, i, k)
    n_rerun = corpus.search_device_exact(b.qp(), nq, k, "l1", None, *b.args())
    assert n_rerun == adv.size
    got = b.result()
    for i in range(nq):
        _seeded_exact(oracle, case, got, i, k)
    res = corpus.search(q, k, "l1")
    assert (res.counts == k).all()
    for i in _sampled_queries():
        _seeded_exact(oracle, case, res, i, k)
    corpus.free()


# ---------------------------------------------------------------------------------------------------------------------
# 4. K1m over a rank map
# ---------------------------------------------------------------------------------------------------------------------
def test_k1m_over_a_rank_map(oracle, ctx_off):
    """An IVFFlat index (8 lists over 4 003 x 64) is searched through a list-ordered view of the corpus: keys carry
    g_rank[view row], the corpus's own row order, so ties and identities are the corpus's.  16 queries of two users, probes = 2:
    queries that probe the same list under the same filter share a pass, so the scan is K1m (last_scan_kernel reports index
    searches too: they run search_general on the view).  Equal to the oracle's IVF model bit for bit, as in test_gpu_index.py."""
    import vsrbac
    ctx = ctx_off
    rng = np.random.default_rng(88)
    n, dim, lists, nq, probes = 4003, 64, 8, 16, 2
    base = rng.integers(0, 256, (n // 2 + 1, dim)).astype(np.float32)
    x = base[rng.integers(0, base.shape[0], n)]                              # most vectors twice or more: ties in every list
    blk, doc = _ids(n, 20)
    oivf = OracleIvf(oracle, "l2", x, lists=lists, seed=3)
    ndocs = int(doc.max())
    perms = [(1, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 2, replace=False)] + \
            [(2, int(d)) for d in rng.choice(np.arange(1, ndocs + 1), ndocs // 3, replace=False)]
    ur = [(1, 1), (2, 2)]
    corpus = ctx.load_corpus(x, blk, doc)
    corpus.load_rbac(ur, perms)
    gpu = corpus.load_ivf(oivf.centers, oivf.assign)
    q = x[rng.integers(0, n, nq)] + rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    users = 1 + np.arange(nq) % 2
    masks = {u: oracle.user_row_mask(u, ur, perms, doc) for u in (1, 2)}
    got_lists = gpu.probe(q, probes)
    for i in range(nq):
        assert got_lists[i].tolist() == oivf.probe(q[i], probes).tolist(), i
    shared = {}
    for i in range(nq):
        for l in got_lists[i]:
            shared[(int(users[i]), int(l))] = shared.get((int(users[i]), int(l)), 0) + 1
    assert max(shared.values()) >= 2                                          # some (filter, list) pass carries several queries
    for kind in ("none", "ranges", "bitmap"):
        if kind == "none":
            filters, ms = None, [None] * nq
        else:
            mode = vsrbac.RANGES if kind == "ranges" else vsrbac.BITMAP
            per_user = {u: corpus.filter_for_user(u, mode) for u in (1, 2)}
            filters, ms = [per_user[int(u)] for u in users], [masks[int(u)] for u in users]
        for k in (10, 100):
            res = gpu.search(q, k, probes, "l2", filters)
            assert ctx.last_scan_kernel() == _k1m("l2"), (kind, k)
            for i in range(nq):
                idx, dist = oivf.search(q[i], k, probes, doc, blk, ms[i])
                m = res.counts[i]
                assert m == idx.size, (kind, k, i, m, idx.size)
                np.testing.assert_array_equal(res.rows[i, :m], idx)
                np.testing.assert_array_equal(res.block_ids[i, :m], blk[idx])
                np.testing.assert_array_equal(res.doc_ids[i, :m], doc[idx])
                np.testing.assert_array_equal(res.dist[i, :m], dist.astype(np.float32))
                assert (res.block_ids[i, m:] == -1).all() and np.isposinf(res.dist[i, m:]).all()
    gpu.free()
    corpus.free()
