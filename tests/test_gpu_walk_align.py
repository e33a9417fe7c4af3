"""Walk alignment (WalkHint, vsr_device.h): the DENSE int8 main launch of a class-view plan takes its block_map rotated by a
per-session word that the seed selection in front of it derives from the class view's position word.

A rotation only changes which workgroup of the launch scans which rows, so every output -- counts, rows, distances, block
ids -- must be the same bytes as under VSR_WALK_ALIGN=0 (no rotation, no position word, passes in first-seen order), and
the same as the oracle's (integer-valued rows: every sum is exact).

One corpus for the whole file, modelled on test_gpu_class_view.py: ~60 000 rows x 128 in documents of 1 ... 100 rows; one role
per document, so a permission class is a role's documents and the view holds the classes in the order of their first
document: two large classes, a class of ~5 000 rows that no query sees (in the middle of the view), two more large classes,
classes of 1, 64, 65 and 32 rows.  The sessions search it with device-resident queries under the u8 hint, as the benchmark
does; VSR_BLOCK_BUDGET / VSR_MIN_SHARED_ROWS / VSR_MIN_ROWS_PER_BLOCK cut the launch into well over 64 workgroups."""
import os
import re

import numpy as np
import pytest

from helpers import sift_like

pytestmark = pytest.mark.gpu

K = 50
DOC_ROWS = (1, 15, 16, 17, 37, 63, 64, 65, 100)
BIG = (1, 6, 7, 8)
UNSEEN = 10
COMMON = {"VSR_BLOCK_BUDGET": "160", "VSR_MIN_ROWS_PER_BLOCK": "64", "VSR_MIN_SHARED_ROWS": "256"}
N_BATCHES = 12


def _open(**env):
    """A context opened under COMMON and `env` (the knobs are read at creation)."""
    import vsrbac
    env = {**COMMON, **env}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return vsrbac.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class World:
    def __init__(self):
        rng = np.random.default_rng(20261020)
        sizes = []
        while sum(sizes) < 60_000:
            sizes.append(DOC_ROWS[len(sizes) % len(DOC_ROWS)])
        sizes = np.asarray(sizes)
        ndocs = sizes.size
        self.doc = np.repeat(np.arange(1, ndocs + 1), sizes).astype(np.int32)
        self.n = int(self.doc.size)
        self.blk = (np.arange(self.n) + 1).astype(np.int64)
        self.x = sift_like(rng, self.n)
        owner = np.asarray([BIG[(3 * d + d // 7 + 2) % 4] for d in range(ndocs)])
        owner[2::11] = UNSEEN                                   # its first document is the third: the class lies inside the view
        first = {s: [d for d in range(20, ndocs) if sizes[d] == s] for s in DOC_ROWS}
        owner[first[1][0]] = 2
        owner[first[64][0]] = 3
        owner[first[65][0]] = 4
        owner[first[15][0]] = 5
        owner[first[17][0]] = 5
        self.permissions = np.asarray([(int(owner[d]), d + 1) for d in range(ndocs)], dtype=np.int32)
        # the view's layout (build_class_view): classes in the order of their first document, each padded to 64 rows
        order = list(dict.fromkeys(int(r) for r in owner))
        rows = {r: int(sizes[owner == r].sum()) for r in order}
        self.view_start, at = {}, 0
        for r in order:
            self.view_start[r] = at
            at += (rows[r] + 63) // 64 * 64
        self.view_rows, self.n_view = rows, at
        assert rows[2] == 1 and rows[5] == 32 and rows[3] == 64 and rows[4] == 65 and rows[UNSEEN] > 1024
        assert 0 < order.index(UNSEEN) < len(order) - 1
        users = {6: ((1, 6), 40), 7: ((1, 7), 22), 8: ((1, 8), 3), 2: ((2,), 3), 3: ((1, 3), 3), 4: ((1, 4), 3), 5: ((5,), 3),
                 9: ((9,), 2), 20: ((1, 6, 7), 4)}
        for u in range(100, 190):
            users[u] = ((1,), 1)
        self.user_roles = np.asarray([(u, r) for u, (roles, _) in users.items() for r in roles], dtype=np.int32)
        quser = np.concatenate([np.full(c, u) for u, (_, c) in users.items()])
        rng.shuffle(quser)
        self.nq = int(quser.size)
        q = self.x[rng.integers(0, self.n, self.nq)].copy()
        q[:, :5] = rng.integers(0, 256, (self.nq, 5)).astype(np.float32)
        # batch j: the same queries and users rolled by 7 j places -- another query names each class first, so the planner
        # meets the classes in another order
        self.perm = [np.roll(np.arange(self.nq), 7 * j) for j in range(N_BATCHES)]
        self.q, self.quser = q, quser

    def checked_queries(self):
        small = [int(i) for i in np.flatnonzero(~np.isin(self.quser, (6, 7)) & (self.quser < 100))]
        return sorted(set(small + list(range(0, self.nq, 9))))


class Rig:
    """The corpus on its own context, the batches' queries on the device, the filters; run() = one call on a session."""

    def __init__(self, w):
        import torch
        import vsrbac
        self.w, self.torch = w, torch
        self.ctx = _open()
        self.corpus = self.ctx.load_corpus(w.x, w.blk, w.doc)
        self.corpus.load_rbac(w.user_roles, w.permissions)
        role = {int(u): self.corpus.filter_for_user(int(u), vsrbac.RANGES) for u in np.unique(w.quser)}
        bitmap = {int(u): self.corpus.filter_for_user(int(u), vsrbac.BITMAP) for u in np.unique(w.quser)}
        self.filters = [self.corpus.pack_filters([role[int(u)] for u in w.quser[p]]) for p in w.perm]
        self.bitmap_filters = self.corpus.pack_filters([bitmap[int(u)] for u in w.quser])
        mixed = [role[int(u)] for u in w.quser]
        self.free_query = int(np.flatnonzero(w.quser >= 100)[0])
        mixed[self.free_query] = None
        self.mixed_filters = self.corpus.pack_filters(mixed)
        self.dq = [torch.from_numpy(np.ascontiguousarray(w.q[p])).cuda() for p in w.perm]
        self._base, self._n_launch = {}, {}

    def buffers(self):
        t, nq = self.torch, self.w.nq
        return (t.full((nq, K), -7, dtype=t.int64, device="cuda"), t.full((nq, K), -7, dtype=t.int32, device="cuda"),
                t.full((nq, K), -7, dtype=t.int64, device="cuda"), t.full((nq, K), -7.0, dtype=t.float32, device="cuda"),
                t.full((nq,), -7, dtype=t.int32, device="cuda"))

    def enqueue(self, session, batch, out, filters=None):
        self.corpus.search_device(self.dq[batch].data_ptr(), self.w.nq, K, "l2", self.filters[batch] if filters is None else filters,
                                  *(t.data_ptr() for t in out), session=session)

    @staticmethod
    def host(out):
        return {"block_ids": out[0].cpu().numpy(), "rows": out[2].cpu().numpy(), "dist": out[3].cpu().numpy(), "counts": out[4].cpu().numpy()}

    def run(self, batch=0, filters=None, **env):
        s = _open(**env)
        s.set_query_hint(True)
        out = self.buffers()
        self.enqueue(s, batch, out, filters)
        s.synchronize()
        name = s.last_scan_kernel()
        s.close()
        return self.host(out), name

    def base(self, batch=0, epi="1"):
        """The same call alone under VSR_WALK_ALIGN=0 (computed once)."""
        if (batch, epi) not in self._base:
            res, name = self.run(batch, VSR_WALK_ALIGN="0", VSR_FORCE_EPI=epi)
            assert "class view" in name and "walk-aligned" not in name, name
            self._base[(batch, epi)] = res
        return self._base[(batch, epi)]

    def n_launch(self, epi):
        """Dispatch slots of batch 0's main launch (computed once)."""
        if epi not in self._n_launch:
            self._n_launch[epi] = _n_launch(self.run(VSR_FORCE_EPI=epi)[1])
        return self._n_launch[epi]

    def close(self):
        self.corpus.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig(World())
    yield r
    r.close()


def _same(a, b):
    for key in ("counts", "rows", "dist", "block_ids"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _check_oracle(oracle, w, res, qs):
    for i in qs:
        mask = oracle.user_row_mask(int(w.quser[i]), w.user_roles, w.permissions, w.doc)
        idx, dist = oracle.filtered_topk("l2", w.x, w.q[i], K, w.doc, w.blk, mask)
        m = int(res["counts"][i])
        assert m == idx.size, (i, int(w.quser[i]), m, idx.size)
        np.testing.assert_array_equal(res["rows"][i, :m], idx)
        np.testing.assert_array_equal(res["dist"][i, :m], dist.astype(np.float32))
        assert (res["block_ids"][i, m:] == -1).all()


def _n_launch(name):
    m = re.search(r", class view, walk-aligned over (\d+) slots\)", name)
    assert m, name
    return int(m.group(1))


def test_default_arm_matches_oracle_and_unaligned(oracle, rig):
    """The shipped path: the rotation comes from the position word (zero at creation, then whatever the launch before left)."""
    w = rig.w
    for epi in ("1", "0"):
        res, name = rig.run(VSR_FORCE_EPI=epi)
        assert "K2w" in name and "int8" in name and _n_launch(name) >= 64 and _n_launch(name) % 8 == 0, name
        _same(res, rig.base(0, epi))
        assert (res["counts"][w.quser == 9] == 0).all()
        assert (res["counts"][w.quser == 2] == 1).all() and (res["counts"][w.quser == 5] == 32).all()
    _check_oracle(oracle, w, res, w.checked_queries())


@pytest.mark.parametrize("epi", ["1", "0"])
@pytest.mark.parametrize("which", ["0", "1", "n/16", "n/8-1", "n/8", "huge"])
def test_every_rotation_gives_the_same_bytes(rig, which, epi):
    """VSR_WALK_ROT=<n>: rot = (8 n) mod n_launch -- no rotation, one row of slots, the middle of the map, its last row, a wrap
    to 0 and a value far beyond it."""
    n = rig.n_launch(epi)
    rot = {"0": 0, "1": 1, "n/16": n // 16, "n/8-1": n // 8 - 1, "n/8": n // 8, "huge": (1 << 40) + 3}[which]
    res, name = rig.run(VSR_FORCE_EPI=epi, VSR_WALK_ROT=str(rot))
    assert _n_launch(name) == n, name
    _same(res, rig.base(0, epi))


@pytest.mark.parametrize("which", ["row 0", "unseen class", "last view row", "n_rows >> 6", "0xFFFFFFFF"])
def test_every_branch_of_the_translation(rig, which):
    """VSR_WALK_POS=<n>: the seed selection translates n instead of the word -- the view's first rows, a row inside the class no
    query sees (-> the next class the batch scans), the view's last row, and two positions past the view (-> slot 0)."""
    w = rig.w
    pos = {"row 0": 0, "unseen class": (w.view_start[UNSEEN] + w.view_rows[UNSEEN] // 2) >> 6, "last view row": (w.n_view - 1) >> 6,
           "n_rows >> 6": w.n_view >> 6, "0xFFFFFFFF": 0xFFFFFFFF}[which]
    for kernel in ("1", "0"):                                # seed_select_wave_kernel, seed_select_kernel
        res, name = rig.run(VSR_FORCE_EPI="1", VSR_WALK_POS=str(pos), VSR_SELECT_WAVE=kernel)
        assert "walk-aligned" in name, name
        _same(res, rig.base(0, "1"))


def test_three_sessions_in_flight(rig):
    """Three sessions over one corpus, 12 calls round-robin with no synchronisation in between, a different batch per call:
    every launch rotates by whatever position the launches in flight last published.  Every output equals the same call made
    alone under VSR_WALK_ALIGN=0."""
    sessions = [_open(VSR_FORCE_EPI="1") for _ in range(3)]
    for s in sessions:
        s.set_query_hint(True)
    outs = [rig.buffers() for _ in range(N_BATCHES)]
    rig.torch.cuda.synchronize()
    for j in range(N_BATCHES):
        rig.enqueue(sessions[j % 3], j, outs[j])
    for s in sessions:
        s.synchronize()
    for s in sessions:
        assert "walk-aligned" in s.last_scan_kernel(), s.last_scan_kernel()
        s.close()
    for j in range(N_BATCHES):
        _same(rig.host(outs[j]), rig.base(j, "1"))


def test_plans_that_leave_the_view_are_not_rotated(oracle, rig):
    """One unfiltered query, or BITMAP filters: no class view, no rotation, results as under VSR_WALK_ALIGN=0."""
    w = rig.w
    for filters in (rig.mixed_filters, rig.bitmap_filters):
        res, name = rig.run(filters=filters, VSR_FORCE_EPI="1")
        assert "class view" not in name and "walk-aligned" not in name, name
        base, base_name = rig.run(filters=filters, VSR_FORCE_EPI="1", VSR_WALK_ALIGN="0")
        assert base_name == name
        _same(res, base)
    _same(base, rig.base(0, "1"))                            # (BITMAP filters admit the same rows as the role filters)
    res, _ = rig.run(filters=rig.mixed_filters, VSR_FORCE_EPI="1")
    i = rig.free_query
    idx, dist = oracle.filtered_topk("l2", w.x, w.q[i], K, w.doc, w.blk, None)
    np.testing.assert_array_equal(res["rows"][i], idx)
    np.testing.assert_array_equal(res["dist"][i], dist.astype(np.float32))
