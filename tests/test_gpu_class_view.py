"""The class view (ClassView, vsr_runtime.h): role pre-filters scanned over a permission-class-ordered copy of the int8 planes.

Integer-valued rows (0..255): every fp32 sum of vector.c is exact, so ids, order and distances are compared bit for bit
with the oracle, and every search is repeated by a context opened under VSR_NO_CLASS_VIEW=1 (base-order planes): counts,
rows, distances and block ids must be the same bytes.
The main launch of a class-view plan is K2w's DENSE instantiation (rows by arithmetic, vsr_mfmaw.h), in both epilogue
forms; the sample launch keeps the general row mapping over the view's tile list.

One corpus for the whole file: ~60 000 rows x 128 in documents of 1, 15, 16, 17, 37, 63, 64, 65 and 100 rows in rotation,
and a dozen roles whose permission classes (documents with the same role set) include a single 1-row document, exactly 64
rows, 65 rows, 32 rows (fewer than k) and four large classes scattered over the whole corpus.  Role 1 is held by most
users (its class is seen by > 150 queries: several passes), the other classes by 40, 22 and 3 queries; one user's role
has no permission at all.  Byte-identical rows sit in documents of three classes whose class order differs from their
(document, block) order."""
import numpy as np
import pytest

from helpers import sift_like

pytestmark = pytest.mark.gpu

K = 50
DOC_ROWS = (1, 15, 16, 17, 37, 63, 64, 65, 100)
# role -> what its class is made of.  1: the public class; 6, 7, 8: large classes; 2: one 1-row document; 3: one 64-row
# document; 4: one 65-row document; 5: a 15-row and a 17-row document (32 rows < k); 9: a role without permissions
BIG = (1, 6, 7, 8)


def _ctx(monkeypatch, **env):
    import vsrbac
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = vsrbac.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return c


class World:
    def __init__(self):
        rng = np.random.default_rng(20260417)
        sizes = []
        while sum(sizes) < 60_000:
            sizes.append(DOC_ROWS[len(sizes) % len(DOC_ROWS)])
        sizes = np.asarray(sizes)
        ndocs = sizes.size
        self.doc = np.repeat(np.arange(1, ndocs + 1), sizes).astype(np.int32)
        self.n = int(self.doc.size)
        self.blk = (np.arange(self.n) + 1).astype(np.int64)
        self.x = sift_like(rng, self.n)
        # documents -> owning role: the special documents first found of their size, the rest dealt over the big classes
        # (the FIRST document belongs to role 7, so class order -- first document seen -- differs from role order)
        owner = np.asarray([BIG[(3 * d + d // 7 + 2) % 4] for d in range(ndocs)])
        first = {s: [d for d in range(20, ndocs) if sizes[d] == s] for s in DOC_ROWS}
        owner[first[1][0]] = 2
        owner[first[64][0]] = 3
        owner[first[65][0]] = 4
        owner[first[15][0]] = 5
        owner[first[17][0]] = 5
        self.owner, self.sizes = owner, sizes
        self.permissions = np.asarray([(int(owner[d]), d + 1) for d in range(ndocs)], dtype=np.int32)
        # a second table that makes different classes: role 6 also sees a third of role 7's documents, role 8 loses half
        # of its own (documents without any role form a class nobody sees)
        p2 = [(int(owner[d]), d + 1) for d in range(ndocs) if not (owner[d] == 8 and d % 2)]
        p2 += [(6, d + 1) for d in range(ndocs) if owner[d] == 7 and d % 3 == 0]
        self.permissions2 = np.asarray(p2, dtype=np.int32)
        # users: (roles, queries).  Users 100.. hold role 1 only.
        users = {6: ((1, 6), 40), 7: ((1, 7), 22), 8: ((1, 8), 3), 2: ((2,), 3), 3: ((1, 3), 3), 4: ((1, 4), 3), 5: ((5,), 3),
                 9: ((9,), 2), 20: ((1, 6, 7), 4)}
        for u in range(100, 190):
            users[u] = ((1,), 1)
        self.user_roles = np.asarray([(u, r) for u, (roles, _) in users.items() for r in roles], dtype=np.int32)
        quser = np.concatenate([np.full(c, u) for u, (_, c) in users.items()])
        rng.shuffle(quser)
        self.quser = quser
        self.nq = int(quser.size)
        # byte-identical rows: one in a role-7 document (low id), one public, one of role 6, one more public, later ones
        self.dup_rows = []
        want = [7, 1, 6, 1, 7, 6]
        d = 30
        for role in want:
            while owner[d] != role or sizes[d] < 15:
                d += 1
            self.dup_rows.append(int(np.flatnonzero(self.doc == d + 1)[sizes[d] // 2]))
            d += 11
        self.x[self.dup_rows] = self.x[self.dup_rows[0]]
        q = self.x[rng.integers(0, self.n, self.nq)].copy()
        q[:, :5] = rng.integers(0, 256, (self.nq, 5)).astype(np.float32)
        q[quser == 20] = self.x[self.dup_rows[0]]            # user 20 sees all the classes that hold the identical rows
        self.q = q
        self._masks = {}
        self._ref = {}

    def mask(self, oracle, user, perms=None):
        key = (int(user), perms is not None)
        if key not in self._masks:
            self._masks[key] = oracle.user_row_mask(int(user), self.user_roles, self.permissions if perms is None else perms, self.doc)
        return self._masks[key]

    def ref(self, oracle, i, perms=None):
        key = (int(i), perms is not None)
        if key not in self._ref:
            self._ref[key] = oracle.filtered_topk("l2", self.x, self.q[i], K, self.doc, self.blk, self.mask(oracle, self.quser[i], perms))
        return self._ref[key]

    def checked_queries(self):
        small = [int(i) for i in np.flatnonzero(~np.isin(self.quser, (6, 7)) & (self.quser < 100))]
        return sorted(set(small + list(range(0, self.nq, 9))))


@pytest.fixture(scope="module")
def world():
    return World()


def _check(oracle, w, res, qs, perms=None):
    for i in qs:
        idx, dist = w.ref(oracle, i, perms)
        m = int(res.counts[i])
        assert m == idx.size, (i, int(w.quser[i]), m, idx.size)
        np.testing.assert_array_equal(res.rows[i, :m], idx)
        np.testing.assert_array_equal(res.dist[i, :m], dist.astype(np.float32))
        assert (res.block_ids[i, m:] == -1).all()


def _same(a, b):
    np.testing.assert_array_equal(a.counts, b.counts)
    np.testing.assert_array_equal(a.rows, b.rows)
    np.testing.assert_array_equal(a.dist, b.dist)
    np.testing.assert_array_equal(a.block_ids, b.block_ids)


def _role_filters(corpus, w, mode=None):
    import vsrbac
    return [corpus.filter_for_user(int(u), vsrbac.RANGES if mode is None else mode) for u in w.quser]


def _search_both(monkeypatch, w, env, run):
    """run(ctx, corpus) on a context with the class view and on one opened under VSR_NO_CLASS_VIEW=1."""
    out = []
    for extra in ({}, {"VSR_NO_CLASS_VIEW": "1"}):
        ctx = _ctx(monkeypatch, **env, **extra)
        corpus = ctx.load_corpus(w.x, w.blk, w.doc)
        out.append(run(ctx, corpus))
        corpus.free()
        ctx.close()
    return out


@pytest.mark.parametrize("epi", ["1", "0"])
def test_class_view_matches_oracle_and_base_planes(oracle, monkeypatch, world, epi):
    """The shapes that can go wrong: classes of 1, 32, 64 and 65 rows, a role that sees nothing, counts < k, passes of one,
    two and three query groups and a class cut into several passes, both epilogues of the main launch, several workgroups
    per class."""
    w = world

    def run(ctx, corpus):
        corpus.load_rbac(w.user_roles, w.permissions)
        res = corpus.search(w.q, K, "l2", _role_filters(corpus, w))
        return res, ctx.last_scan_kernel()

    (res, name), (base, base_name) = _search_both(monkeypatch, w, {"VSR_FORCE_EPI": epi, "VSR_MIN_ROWS_PER_BLOCK": "16"}, run)
    assert "class view" in name and "K2w" in name and "int8" in name, name
    assert not any(s in name for s in ("K2g", "K2i", "HO=true")), name
    assert "class view" not in base_name and "int8" in base_name, base_name
    assert (res.counts[w.quser == 9] == 0).all()
    assert (res.counts[w.quser == 2] == 1).all() and (res.counts[w.quser == 5] == 32).all()
    _check(oracle, w, res, w.checked_queries())
    _same(res, base)


def test_ties_keep_base_order(oracle, monkeypatch, world):
    """Byte-identical rows in documents of different classes: at equal distance the order is the base (document, block)
    order, not the view's class order."""
    w = world

    def run(ctx, corpus):
        corpus.load_rbac(w.user_roles, w.permissions)
        return corpus.search(w.q, K, "l2", _role_filters(corpus, w)), ctx.last_scan_kernel()

    (res, name), (base, _) = _search_both(monkeypatch, w, {"VSR_FORCE_EPI": "1"}, run)
    assert "class view" in name, name
    tied = [int(i) for i in np.flatnonzero(w.quser == 20)]
    assert tied
    for i in tied:
        m = len(w.dup_rows)
        assert (res.dist[i, :m] == 0).all()
        np.testing.assert_array_equal(res.rows[i, :m], np.sort(w.dup_rows))
    _check(oracle, w, res, tied)
    _same(res, base)


def test_rbac_reload_rebuilds_the_view(oracle, monkeypatch, world):
    w = world

    def run(ctx, corpus):
        out = []
        for perms in (w.permissions, w.permissions2):
            corpus.load_rbac(w.user_roles, perms)
            out.append((corpus.search(w.q, K, "l2", _role_filters(corpus, w)), ctx.last_scan_kernel()))
        return out

    view, base = _search_both(monkeypatch, w, {"VSR_FORCE_EPI": "1"}, run)
    for j, perms in enumerate((None, w.permissions2)):
        res, name = view[j]
        assert "class view" in name, (j, name)
        _check(oracle, w, res, w.checked_queries(), perms)
        _same(res, base[j][0])
    assert not np.array_equal(view[0][0].rows, view[1][0].rows)


def test_only_whole_class_batches_take_the_view(oracle, monkeypatch, world):
    """All role filters: class view.  One unfiltered query among them, or BITMAP filters: planned as before."""
    import vsrbac
    w = world
    ctx = _ctx(monkeypatch, VSR_FORCE_EPI="1")
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(w.user_roles, w.permissions)
    ranges = _role_filters(corpus, w)
    res = corpus.search(w.q, K, "l2", ranges)
    assert "class view" in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    _check(oracle, w, res, w.checked_queries()[::3])

    free = int(np.flatnonzero(w.quser >= 100)[0])
    mixed = list(ranges)
    mixed[free] = None
    res_m = corpus.search(w.q, K, "l2", mixed)
    assert "class view" not in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    idx, dist = oracle.filtered_topk("l2", w.x, w.q[free], K, w.doc, w.blk, None)
    np.testing.assert_array_equal(res_m.rows[free], idx)
    np.testing.assert_array_equal(res_m.dist[free], dist.astype(np.float32))
    others = np.arange(w.nq) != free
    np.testing.assert_array_equal(res_m.rows[others], res.rows[others])
    np.testing.assert_array_equal(res_m.dist[others], res.dist[others])

    res_b = corpus.search(w.q, K, "l2", _role_filters(corpus, w, vsrbac.BITMAP))
    assert "class view" not in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    _same(res_b, res)
    corpus.free()
    ctx.close()


def test_three_sessions_in_flight(oracle, monkeypatch, world):
    """The benchmark's call shape: device-resident queries under the u8 hint, three sessions on their own streams over one
    corpus, calls interleaved, one synchronisation at the end."""
    import torch
    import vsrbac
    w = world
    ctx = _ctx(monkeypatch, VSR_FORCE_EPI="1")
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(w.user_roles, w.permissions)
    filters = corpus.pack_filters(_role_filters(corpus, w))
    host = corpus.search(w.q, K, "l2", filters)
    sessions = [_ctx(monkeypatch, VSR_FORCE_EPI="1") for _ in range(3)]
    dq = torch.from_numpy(w.q).cuda()
    outs = []
    for s in sessions:
        s.set_query_hint(True)
        outs.append((torch.empty((w.nq, K), dtype=torch.int64, device="cuda"), torch.empty((w.nq, K), dtype=torch.int32, device="cuda"),
                     torch.empty((w.nq, K), dtype=torch.int64, device="cuda"), torch.empty((w.nq, K), dtype=torch.float32, device="cuda"),
                     torch.empty((w.nq,), dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for _ in range(2):
        for s, o in zip(sessions, outs):
            corpus.search_device(dq.data_ptr(), w.nq, K, "l2", filters, *(t.data_ptr() for t in o), session=s)
    for s in sessions:
        s.synchronize()
    for s, o in zip(sessions, outs):
        assert "class view" in s.last_scan_kernel(), s.last_scan_kernel()
        cnt = o[4].cpu().numpy()
        assert (cnt >= 0).all()
        np.testing.assert_array_equal(cnt, host.counts)
        rows, dist, blk = o[2].cpu().numpy(), o[3].cpu().numpy(), o[0].cpu().numpy()
        for i in range(w.nq):
            m = cnt[i]
            np.testing.assert_array_equal(rows[i, :m], host.rows[i, :m])
            np.testing.assert_array_equal(dist[i, :m], host.dist[i, :m])
            np.testing.assert_array_equal(blk[i, :m], host.block_ids[i, :m])
    _check(oracle, w, host, w.checked_queries()[::3])
    for s in sessions:
        s.close()
    corpus.free()
    ctx.close()
