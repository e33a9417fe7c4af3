"""K2r (vsr_i8r.h): the register-fed int8 sample pass of class-view plans, against the oracle and against K2i's sample pass.

K2r must take the SAME sample as i8_stream_kernel<4, true>: the seeds, the candidate sets and therefore the results of a
search are the same bytes under VSR_SAMPLE_REG=1 (the default) and VSR_SAMPLE_REG=0, and both equal the oracle's exact
filtered top-k (integer-valued rows 0..255: every fp32 sum of vector.c is exact, so ids, order and distances are compared
bit for bit).  The library's statistics carry no per-call candidate counts, so "same thresholds" is pinned through the
results and the screening check only.

One corpus for the whole file: ~44 000 rows x 128 in documents of at most 100 rows, dealt in random order over seven
permission classes of 1, 31, 32, 33, 2047, 2049 and 40 000 rows.  The RBAC is a tree as vsrbac.datasets.tree_rbac makes it
(a role is permitted its own documents and its ancestors'; a user holds one role): the root role owns one class, its six
children one each, and the children's users ask 1, 15, 16, 17, 64 and 65 queries -- the widths of the passes over their
classes (65: two passes, i.e. two sample groups), while the root's class is seen by all 178 (64 + 64 + 50).  `rot` rotates
which class the root owns, so every class size meets every pass width.  Queries that do not see the 40 000-row class fit
their candidate buffer: their thresholds stay open.

Geometries (where the sample kernel takes another path):
  default   2048 rows per workgroup of a shared pass: streams of one and two stages per wave, the 2049-row class's fifth
            sampled stage holds ONE row (its second list tile lies past the range), trips of four and of two units;
  fine      64 rows per workgroup: ranges that sample exactly one stage, three idle waves, hundreds of workgroups per class;
  stride3   every third stage: the ragged last stage of the 2047-row class (31 rows) is sampled, longer streams per wave."""
import numpy as np
import pytest

from helpers import sift_like

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 2047, 2049, 40_000)
WIDTHS = (1, 15, 16, 17, 64, 65)
GEOMETRY = {"default": {}, "fine": {"VSR_MIN_ROWS_PER_BLOCK": "16", "VSR_MIN_SHARED_ROWS": "64"}, "stride3": {"VSR_SAMPLE_STRIDE": "3"}}
OLD_SAMPLE = "i8_stream_kernel<NQG=4, SAMPLE=true>"


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
        rng = np.random.default_rng(20261018)
        doc_rows, doc_class = [], []
        for cls, size in enumerate(SIZES):
            parts = [100] * (size // 100) + ([size % 100] if size % 100 else [])
            if size in (31, 32, 33):                                   # two documents each: 15 + 16, 15 + 17, 16 + 17
                parts = {31: [15, 16], 32: [15, 17], 33: [16, 17]}[size]
            doc_rows += parts
            doc_class += [cls] * len(parts)
        order = rng.permutation(len(doc_rows))                         # every class scattered over the whole corpus
        self.doc_rows = np.asarray(doc_rows)[order]
        self.doc_class = np.asarray(doc_class)[order]
        self.doc = np.repeat(np.arange(1, len(order) + 1), self.doc_rows).astype(np.int32)
        self.n = int(self.doc.size)
        assert self.n == sum(SIZES)
        self.blk = (np.arange(self.n) + 1).astype(np.int64)
        self.x = sift_like(rng, self.n)
        # query i is asked by the user of child role 1 + quser[i]; the same vectors whatever the rotation
        self.quser = np.concatenate([np.full(w, j + 1) for j, w in enumerate(WIDTHS)])
        rng.shuffle(self.quser)
        self.nq = int(self.quser.size)
        q = self.x[rng.integers(0, self.n, self.nq)].copy()
        q[:, :5] = rng.integers(0, 256, (self.nq, 5)).astype(np.float32)
        self.q = q
        self._ref = {}
        self._mask = {}

    def rbac(self, rot):
        """Role 1 = the root, owning class rot; role 1 + j (user j) = its j-th child, owning class (rot + j) % 7."""
        owner_of_class = {(rot + j) % len(SIZES): 1 + j for j in range(len(SIZES))}
        perms = []
        for d, cls in enumerate(self.doc_class):
            role = owner_of_class[int(cls)]
            perms += [(role, d + 1)] if role != 1 else [(r, d + 1) for r in range(1, len(SIZES) + 1)]
        user_roles = [(j, 1 + j) for j in range(1, len(SIZES))]
        return np.asarray(user_roles, dtype=np.int32), np.asarray(perms, dtype=np.int32)

    def ref(self, oracle, rot, i, k):
        key = (rot, int(i))
        if key not in self._ref:
            user = int(self.quser[i])
            if (rot, user) not in self._mask:
                ur, perms = self.rbac(rot)
                self._mask[(rot, user)] = oracle.user_row_mask(user, ur, perms, self.doc)
            self._ref[key] = oracle.filtered_topk("l2", self.x, self.q[i], 100, self.doc, self.blk, self._mask[(rot, user)])
        idx, dist = self._ref[key]                                     # (the top 10 are the head of the top 100: same order)
        return idx[:k], dist[:k]


@pytest.fixture(scope="module")
def world():
    return World()


def _check(oracle, w, rot, res, k):
    for i in range(w.nq):
        idx, dist = w.ref(oracle, rot, i, k)
        m = int(res.counts[i])
        assert m == idx.size, (rot, i, int(w.quser[i]), m, idx.size)
        np.testing.assert_array_equal(res.rows[i, :m], idx)
        np.testing.assert_array_equal(res.dist[i, :m], dist.astype(np.float32))
        assert (res.block_ids[i, m:] == -1).all()


def _same(a, b):
    np.testing.assert_array_equal(a.counts, b.counts)
    np.testing.assert_array_equal(a.rows, b.rows)
    np.testing.assert_array_equal(a.dist, b.dist)
    np.testing.assert_array_equal(a.block_ids, b.block_ids)


def _search(monkeypatch, w, rot, env, mode=None):
    """{k: (result, kernel name)} for k = 100 and 10 on a fresh context opened under `env`; no query may be flagged."""
    import vsrbac
    ctx = _ctx(monkeypatch, VSR_FORCE_EPI="1", **env)
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(*w.rbac(rot))
    filters = [corpus.filter_for_user(int(u), vsrbac.RANGES if mode is None else mode) for u in w.quser]
    out = {}
    for k in (100, 10):
        res = corpus.search(w.q, k, "l2", filters)
        out[k] = (res, ctx.last_scan_kernel())
    assert ctx.screening_check(0)[0] == 0
    corpus.free()
    ctx.close()
    return out


@pytest.mark.parametrize("geometry", list(GEOMETRY))
@pytest.mark.parametrize("rot", range(len(SIZES)))
def test_register_fed_sample_matches_oracle_and_stream_sample(oracle, monkeypatch, world, rot, geometry):
    w = world
    reg = _search(monkeypatch, w, rot, {"VSR_SAMPLE_REG": "1", **GEOMETRY[geometry]})
    old = _search(monkeypatch, w, rot, {"VSR_SAMPLE_REG": "0", **GEOMETRY[geometry]})
    for k in (100, 10):
        (res, name), (res0, name0) = reg[k], old[k]
        assert "class view" in name and "K2r" in name and OLD_SAMPLE not in name, name
        assert "class view" in name0 and "K2r" not in name0 and OLD_SAMPLE in name0, name0
        _check(oracle, w, rot, res, k)
        _check(oracle, w, rot, res0, k)
        _same(res, res0)


def test_default_is_the_register_fed_sample(monkeypatch, world):
    out = _search(monkeypatch, world, 0, {})
    assert "K2r" in out[100][1], out[100][1]


def test_bitmap_filters_keep_their_sample_kernel(oracle, monkeypatch, world):
    """A plan that does not take the class view (BITMAP filters) samples on the kernel it always did -- K2i's streams or, where
    the planner finds that sample too thin, K2w's own SAMPLE instantiation -- whatever VSR_SAMPLE_REG says."""
    import vsrbac
    w = world
    reg = _search(monkeypatch, w, 2, {"VSR_SAMPLE_REG": "1"}, vsrbac.BITMAP)
    old = _search(monkeypatch, w, 2, {"VSR_SAMPLE_REG": "0"}, vsrbac.BITMAP)
    for k in (100, 10):
        (res, name), (res0, name0) = reg[k], old[k]
        assert "class view" not in name and "K2r" not in name, name
        assert OLD_SAMPLE in name or "mfma_wide_kernel<L2, NCH=1, SAMPLE=true, PL=int8>" in name, name
        assert name == name0
        _check(oracle, w, 2, res, k)
        _same(res, res0)
