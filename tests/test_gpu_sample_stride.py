"""The planner's sample stride of int8 class-view plans (vsr_plan.hip, VIEW_SAMPLE_STRIDE): every 32nd stage instead of every
16th when the sample launch is K2r, every query's sample stays thick enough for its seed and the main launch keeps the mask
epilogue under the looser seeds; otherwise the call is planned at the context's stride as before, and an explicit
VSR_SAMPLE_STRIDE always wins.  A seed only decides which rows become candidates -- a looser one admits more of them -- so the
results must be the same bytes at every stride: rows, distances, counts, block ids, document ids are compared with a context
opened under VSR_SAMPLE_STRIDE=16 and with the oracle, and no query may be flagged.  `last_scan_kernel()` names the stride
the sample launch ran at ("K2r, stride N").

Two worlds of integer rows in 0..255, d = 128, documents of 100 rows, every document owned by one role (a permission class =
a role's documents):
  * large: 200 000 rows.  The public class has ~175 000 of them and is seen by 60 queries (k = 10, kp = 32: a query admits
    32 + 6 sqrt(32 * 32) + 4 * 32 = 352 rows at 1/32, and 1024 * 352 / ~170 000 rows per query = 2.1 survivors per wave-tile,
    below the mask epilogue's 4).  One user sees 300 rows only: all of them fit the candidate buffer, the query runs with an
    open threshold and does not hold the stride back.  One user sees a class of 24 000 rows only (more than the buffer holds).
  * small: 20 000 rows, 16 000 public: 1024 * 352 / ~16 000 = 22 survivors per wave-tile, so the plan keeps stride 16."""
import numpy as np
import pytest

from helpers import sift_like

pytestmark = pytest.mark.gpu

K = 10
PUBLIC, SMALL, MID = 1, 2, 3                   # roles; users 2 and 3 hold only SMALL / MID, users 100.. only PUBLIC


def _ctx(monkeypatch, **env):
    import vsrbac
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = vsrbac.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return c


class World:
    def __init__(self, n_docs, small_docs, mid_docs, n_public_queries, seed):
        rng = np.random.default_rng(seed)
        owner = np.full(n_docs, PUBLIC)
        special = rng.choice(n_docs, small_docs + mid_docs, replace=False)      # scattered: class order differs from base order
        owner[special[:small_docs]] = SMALL
        owner[special[small_docs:]] = MID
        self.doc = np.repeat(np.arange(1, n_docs + 1), 100).astype(np.int32)
        self.n = int(self.doc.size)
        self.blk = (np.arange(self.n) + 1).astype(np.int64)
        self.x = sift_like(rng, self.n)
        self.permissions = np.asarray([(int(owner[d]), d + 1) for d in range(n_docs)], dtype=np.int32)
        users = [(2, SMALL), (3, MID)] + [(100 + j, PUBLIC) for j in range(n_public_queries)]
        self.user_roles = np.asarray(users, dtype=np.int32)
        self.quser = np.asarray([u for u, _ in users])
        row_role = np.repeat(owner, 100)
        q = []
        for u, r in users:
            rows = np.flatnonzero(row_role == r)
            v = self.x[rows[int(rng.integers(0, rows.size))]].copy()           # a row the user sees (distance 0 comes first) ...
            if u % 3:
                v[:5] = rng.integers(0, 256, 5)                                # ... or nearly one
            q.append(v)
        self.q = np.asarray(q, dtype=np.float32)
        self._ref = {}

    def ref(self, oracle, i):
        if i not in self._ref:
            mask = oracle.user_row_mask(int(self.quser[i]), self.user_roles, self.permissions, self.doc)
            self._ref[i] = oracle.filtered_topk("l2", self.x, self.q[i], K, self.doc, self.blk, mask)
        return self._ref[i]


@pytest.fixture(scope="module")
def large():
    return World(2000, 3, 240, 60, 20261021)


@pytest.fixture(scope="module")
def small():
    return World(200, 3, 37, 60, 20261022)


def _check(oracle, w, res, sel, queries):
    for j in queries:
        idx, dist = w.ref(oracle, int(sel[j]))
        m = int(res.counts[j])
        assert m == idx.size, (j, m, idx.size)
        np.testing.assert_array_equal(res.rows[j, :m], idx)
        np.testing.assert_array_equal(res.dist[j, :m], dist.astype(np.float32))
        np.testing.assert_array_equal(res.block_ids[j, :m], w.blk[idx])
        np.testing.assert_array_equal(res.doc_ids[j, :m], w.doc[idx])


def _same(a, b):
    for f in ("counts", "rows", "dist", "block_ids", "doc_ids"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def _run(monkeypatch, w, sel, **env):
    """The queries `sel` of the world on a context opened under `env`: (result, kernel name, flagged queries)."""
    import vsrbac
    ctx = _ctx(monkeypatch, **env)
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(w.user_roles, w.permissions)
    res = corpus.search(w.q[sel], K, "l2", [corpus.filter_for_user(int(u), vsrbac.RANGES) for u in w.quser[sel]])
    name = ctx.last_scan_kernel()
    flagged = ctx.screening_check(0)[0]                                   # (raises if a kernel's bounds guard tripped)
    corpus.free()
    ctx.close()
    return res, name, flagged


def test_large_call_samples_every_32nd_stage_and_gives_the_same_bytes(oracle, monkeypatch, large):
    w = large
    sel = np.flatnonzero(w.quser != 3)                                    # the public queries and the 300-row user
    res, name, flagged = _run(monkeypatch, w, sel)
    assert "class view" in name and "K2r, stride 32" in name, name
    ref, ref_name, ref_flagged = _run(monkeypatch, w, sel, VSR_SAMPLE_STRIDE="16")
    assert "class view" in ref_name and "K2r, stride 16" in ref_name, ref_name
    assert flagged == 0 and ref_flagged == 0
    assert res.counts[0] == K                                             # (the 300-row user)
    _same(res, ref)
    _check(oracle, w, res, sel, range(0, sel.size, 3))


def test_mid_size_class_gets_the_same_bytes_at_the_planners_stride(oracle, monkeypatch, large):
    """With the user whose 24 000 rows do not fit the candidate buffer (a seed it must have, from ~750 stages of its class):
    whichever stride the thickness check lets the plan keep, the bytes are those of stride 16 and of the oracle."""
    w = large
    sel = np.arange(w.quser.size)
    res, name, flagged = _run(monkeypatch, w, sel)
    assert "class view" in name and "K2r, stride " in name, name
    ref, _, ref_flagged = _run(monkeypatch, w, sel, VSR_SAMPLE_STRIDE="16")
    assert flagged == 0 and ref_flagged == 0
    _same(res, ref)
    _check(oracle, w, res, sel, [0, 1, 2, 3])


def test_explicit_stride_wins(monkeypatch, large):
    w = large
    sel = np.flatnonzero(w.quser != 3)
    res, name, flagged = _run(monkeypatch, w, sel, VSR_SAMPLE_STRIDE="64")
    assert "K2r, stride 64" in name and flagged == 0, name
    ref, _, _ = _run(monkeypatch, w, sel, VSR_SAMPLE_STRIDE="16")
    _same(res, ref)


def test_small_call_keeps_stride_16(oracle, monkeypatch, small):
    """Too few rows per query for the mask epilogue under the looser seeds: the call is planned as before."""
    w = small
    sel = np.arange(w.quser.size)
    res, name, flagged = _run(monkeypatch, w, sel)
    assert "class view" in name and "K2r, stride 16" in name and flagged == 0, name
    forced, forced_name, forced_flagged = _run(monkeypatch, w, sel, VSR_SAMPLE_STRIDE="32")
    assert "K2r, stride 32" in forced_name and forced_flagged == 0, forced_name
    _same(res, forced)
    _check(oracle, w, res, sel, range(0, sel.size, 2))
