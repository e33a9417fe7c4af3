"""vsr_hnsw_vacuum_partitions (Corpus.vacuum_hnsw_partitions): rows leave many partition graphs over one resident corpus in one call.

The contract is equality with vsr_hnsw_vacuum run on every graph alone: out[g]'s export, element map and stats (bar attempts) are
those of Corpus.vacuum_hnsw(export(prior[g]), dead[g]).  Two of the graphs are also held against the serial model
(tests/hnsw_vacuum_model.py), so that the new path stands on a plain reference.  Rows are small integers: every distance is exact in
any order.  Eight partitions of one scenario: 0 shares a dead row with 1, where it lives; 1 loses its entry point; 2 loses its whole
top level; 3 loses every row; 4 loses nothing; 5 has no prior; 6 and 7 name ONE loaded prior with multi-TID elements, some of which
lose one TID and some all, with different dead rows.  The schedule is pinned without a GPU by tests/test_hnsw_forest_vacuum_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import hnsw_vacuum_model as vm
from helpers import same_graph
from hnsw_forest_search_model import merge_model
from hnsw_half_model import to_half

pytestmark = pytest.mark.gpu

N, SEED, EFC = 4000, 43, 32
KINDS = [("f32", "l2", 8), ("f32", "ip", 4), ("half", "l2", 4), ("bit", "hamming", 8)]   # (rows, metric, m)
DIM = {"f32": 16, "half": 24, "bit": 52}
SIZES = [1500, 700, 300, 200, 250, 400]                                         # the built graphs; the last becomes the loaded prior
STAT_KEYS = ("tuples_removed", "tuples_kept", "elements_removed", "elements_repaired", "batches")


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _load(ctx, kind, x):
    if kind == "f32":
        return ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32), None, None)
    if kind == "half":
        return ctx.load_corpus_half(to_half(x), None, None)
    return ctx.load_corpus_bit(np.asarray(x) != 0, None, None, None)


class Scene:
    """The corpus, the priors, every partition's dead rows, and per VSR_HNSW_VACUUM_BATCH what vacuum_hnsw makes of each graph alone."""

    def __init__(self, ctx, kind, metric, m):
        rng = np.random.default_rng(9500)
        self.kind, self.metric, self.m = kind, metric, m
        self.x = (rng.integers(0, 2, (N, DIM[kind])) if kind == "bit" else rng.integers(-8, 9, (N, DIM[kind]))).astype(np.float32)
        self.corpus = _load(ctx, kind, self.x)
        parts = [rng.choice(N, n, replace=False).astype(np.int64) for n in SIZES]
        parts[1] = np.concatenate([parts[0][:300], np.setdiff1d(np.arange(N), parts[0])[:400]])   # 0 and 1 overlap
        self.built = self.corpus.build_hnsw_partitions(parts, m, EFC, metric, SEED)
        ex = [h.export() for h in self.built]
        g = ex[5]                                                               # the loaded prior: elements 0 .. 9 get a second TID, 10 .. 19
        spare = np.setdiff1d(np.arange(N), parts[5])[:30]                       # a second and a third, rows the graph does not hold
        outside = np.setdiff1d(np.arange(N), parts[5])[30:31]                   # a dead row no TID of graph 6 names
        g["tids"][:10, 1], g["tids"][10:20, 1], g["tids"][10:20, 2] = spare[:10], spare[10:20], spare[20:30]
        g["tid_count"][:10], g["tid_count"][10:20] = 2, 3
        self.loaded = (self.corpus.load_hnsw_half(g) if kind == "half" else self.corpus.load_hnsw_bit(g, metric) if kind == "bit"
                       else self.corpus.load_hnsw(g))
        self.priors = self.built[:5] + [None, self.loaded, self.loaded]
        self.exports = ex[:5] + [None, g, g]
        top = np.flatnonzero(ex[2]["level"] == ex[2]["level"].max())
        assert ex[2]["max_level"] >= 2, "graph 2 has no top level to lose"
        shared = parts[0][:300]
        self.dead = [np.concatenate([shared[:20], parts[0][300:430]]),          # rows 0 .. 19 of the overlap die in graph 0 and live in 1
                     np.concatenate([ex[1]["tids"][ex[1]["entry"], :1], shared[20:60]]),
                     np.concatenate([ex[2]["tids"][top, 0], parts[2][:10]]),
                     parts[3], np.zeros(0, dtype=np.int64), np.array([1, 2]),
                     np.concatenate([g["tids"][:5, 0], g["tids"][10:13, :3].ravel(), g["tids"][40:70, 0], g["tids"][40:42, 0], outside]),
                     np.concatenate([g["tids"][5:8, 1], g["tids"][13:15, :3].ravel(), g["tids"][100:120, 0]])]
        self.dead = [np.asarray(d, dtype=np.int64) for d in self.dead]
        assert np.isin(self.dead[0][:20], ex[1]["tids"][:, 0]).all() and not np.isin(self.dead[0][:20], self.dead[1]).any()
        self.alone = {}

    def reference(self, ctx, monkeypatch, vbatch):
        """[(export, stats)] per partition from vacuum_hnsw alone, under VSR_HNSW_VACUUM_BATCH = vbatch (None: the default)."""
        if vbatch not in self.alone:
            if vbatch:
                monkeypatch.setenv("VSR_HNSW_VACUUM_BATCH", str(vbatch))
            out = []
            for g, d in zip(self.exports, self.dead):
                if g is None:
                    out.append(None)
                    continue
                idx, st = self.corpus.vacuum_hnsw(g, d, EFC, self.metric)
                out.append((idx.export(), st))
                idx.free()
            monkeypatch.delenv("VSR_HNSW_VACUUM_BATCH", raising=False)
            ctx.screening_check(0)
            self.alone[vbatch] = out
        return self.alone[vbatch]

    def free(self):
        for h in self.built + [self.loaded]:
            h.free()
        self.corpus.free()


_SCENES = {}


@pytest.fixture(scope="module")
def scene(ctx):
    def get(kind, metric, m):
        if (kind, metric) not in _SCENES:
            _SCENES[(kind, metric)] = Scene(ctx, kind, metric, m)
        return _SCENES[(kind, metric)]
    yield get
    for s in _SCENES.values():
        s.free()
    _SCENES.clear()


def _check(ctx, s, want, env=None, monkeypatch=None, attempts_above=0):
    """One call under `env`; every partition against want[g] = (export, stats).  Returns the indexes."""
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, str(value))
    out, maps, stats = s.corpus.vacuum_hnsw_partitions(s.priors, s.dead, EFC, s.metric)
    for name in env or {}:
        monkeypatch.delenv(name)
    ctx.screening_check(0)                                                      # fails on a guard word that is not as it was found
    for g, w in enumerate(want):
        got = out[g].export()
        if w is None:
            assert len(got["level"]) == 0 and got["entry"] == -1 and maps[g].size == 0
            continue
        try:
            same_graph(got, w[0])
        except AssertionError as e:
            raise AssertionError(f"graph {g}: {e}") from None
        np.testing.assert_array_equal(maps[g], w[1]["elem_map"], err_msg=f"graph {g}: element map")
        assert {k: stats[g][k] for k in STAT_KEYS} == {k: w[1][k] for k in STAT_KEYS}, g
        assert stats[g]["attempts"] > attempts_above
    return out


# ---- 1: equality with vsr_hnsw_vacuum on every graph alone, however the batches wait for rounds ------------------------------------
@pytest.mark.parametrize("vbatch", [64, None])
@pytest.mark.parametrize("fbatch", [1, 5, None])
@pytest.mark.parametrize("kind,metric,m", KINDS)
def test_every_graph_is_what_vacuum_makes_of_it_alone(ctx, scene, monkeypatch, kind, metric, m, fbatch, vbatch):
    s = scene(kind, metric, m)
    want = s.reference(ctx, monkeypatch, vbatch)
    env = {k: v for k, v in (("VSR_HNSW_FOREST_BATCH", fbatch), ("VSR_HNSW_VACUUM_BATCH", vbatch)) if v}
    out = _check(ctx, s, want, env, monkeypatch)
    if fbatch is None and vbatch is None:
        # the scenario is what it claims to be
        assert want[1][1]["elem_map"][s.exports[1]["entry"]] == -1, "graph 1 kept its entry point"
        assert want[2][0]["max_level"] < s.exports[2]["max_level"], "graph 2 kept its top level"
        assert len(want[3][0]["level"]) == 0 and want[3][1]["elements_removed"] == SIZES[3]
        same_graph(want[4][0], s.exports[4])
        assert (want[6][0]["tid_count"][:5] == 1).all() and (want[6][1]["elem_map"][10:13] == -1).all()
        assert not np.array_equal(want[6][1]["elem_map"], want[7][1]["elem_map"])
        same_graph(s.loaded.export(), s.exports[6])                             # the priors are as they were
    for h in out:
        h.free()


# ---- 2: against the serial model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric,m", [KINDS[0], KINDS[3]])
def test_against_the_serial_model(ctx, scene, kind, metric, m):
    s = scene(kind, metric, m)
    out, maps, stats = s.corpus.vacuum_hnsw_partitions(s.priors, s.dead, EFC, s.metric)
    for g in (2, 6, 7):
        want, wst = vm.vacuum(s.exports[g], s.x, "l2", s.dead[g], EFC)          # (a bit graph: 0 / 1 rows under l2 are its Hamming distances)
        same_graph(out[g].export(), want)
        np.testing.assert_array_equal(maps[g], wst["elem_map"])
        assert {k: stats[g][k] for k in STAT_KEYS} == {k: wst[k] for k in STAT_KEYS}
        vm.check_invariants(want, s.dead[g])
    for h in out:
        h.free()


# ---- 3: the restart, and the refusal where the ladders end -------------------------------------------------------------------------
def test_both_ladders_are_climbed_and_the_graphs_stay(ctx, scene, monkeypatch):
    s = scene(*KINDS[0])
    want = s.reference(ctx, monkeypatch, None)
    out = _check(ctx, s, want, {"VSR_HNSW_BUILD_VISITED_SLOTS": 256, "VSR_HNSW_VACUUM_CAPS": EFC + 1}, monkeypatch, attempts_above=1)
    for h in out:
        h.free()


def test_where_the_ladders_end_the_partition_is_named(ctx, scene, monkeypatch):
    from vsrbac import _ffi
    from vsrbac._ffi import load_library
    from vsrbac.engine import _ptr
    s = scene(*KINDS[0])
    rows = s.exports[0]["tids"][:, 0]
    dead = [np.zeros(0, dtype=np.int64), rows[40:]]                             # partition 1: graph 0 with 40 of 1500 elements left
    monkeypatch.setenv("VSR_HNSW_VACUUM_LDS", "4416")                          # the least the knob takes at ef_construction = 32
    idx, st = s.corpus.vacuum_hnsw(s.exports[0], dead[1], EFC, s.metric)       # alone it succeeds, through the spill form
    assert idx.vacuum_spill_info()[0] > 0 and idx.info()[0] == 40
    idx.free()
    off = np.array([0, dead[0].size, dead[0].size + dead[1].size], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate(dead))
    handles = (C.c_void_p * 2)(0xDEAD0, 0xDEAD0)
    prior = (C.c_void_p * 2)(s.built[4]._h, s.built[0]._h)
    rc = load_library().vsr_hnsw_vacuum_partitions(s.corpus._h, 2, prior, _ptr(off), _ptr(flat), EFC, 0, 0, None, None, handles)
    monkeypatch.delenv("VSR_HNSW_VACUUM_LDS")
    assert rc == _ffi.ERR_UNSUPPORTED and handles[0] is None and handles[1] is None
    message = load_library().vsr_last_error().decode()
    assert "partition 1:" in message and "alone with vsr_hnsw_vacuum" in message, message
    ctx.screening_check(0)


# ---- 4: the results are ordinary indexes ----------------------------------------------------------------------------------------------
def test_the_vacuumed_graphs_open_as_a_forest(ctx, scene):
    s = scene(*KINDS[0])
    out, _, _ = s.corpus.vacuum_hnsw_partitions(s.priors, s.dead, EFC, s.metric)
    rng = np.random.default_rng(9501)
    q = s.x[rng.integers(0, N, 6)] + rng.integers(-2, 3, (6, DIM["f32"])).astype(np.float32)
    k, ef = 10, 40
    per = [h.search(q, k, ef, "l2")[0] for h in out]
    for g, res in enumerate(per):
        assert not np.isin(res.rows[res.rows >= 0], s.dead[g]).any(), f"graph {g} returned a row that is dead in it"
    tasks = [[0, 1], [2, 3, 4], [5], [6, 7], [0, 1, 2, 3, 4, 5, 6, 7], [1, 6]]
    forest = s.corpus.hnsw_forest(out)
    res, _ = forest.search(q, tasks, k, ef, "l2")
    forest.free()
    blk, doc, row, dist, cnt = merge_model(per, tasks, k)
    np.testing.assert_array_equal(res.counts, cnt)
    np.testing.assert_array_equal(res.rows, row)
    np.testing.assert_array_equal(res.dist, dist)
    for h in out:
        h.free()
    ctx.screening_check(0)


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------
def _bad_loaded(s):
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.exports[0].items()}
    slot, lc, j = np.argwhere(bad["up_nbr"] >= 0)[0]
    bad["up_nbr"][slot, lc, j] = len(bad["level"])                             # a neighbour id of n_elem, where load_hnsw does not look
    return s.corpus.load_hnsw(bad)


REFUSALS = {
    "merge flag": ("UNSUPPORTED", "VSR_HNSW_BUILD_MERGE_DUPLICATES", lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4]], [[1]], EFC, "l2", 1)),
    "unknown flag": ("INVALID", "unknown flag bits", lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4]], [[1]], EFC, "l2", 2)),
    "foreign corpus": ("INVALID", "partition 1: the prior index is over another corpus",
                       lambda s, c: c.twin.vacuum_hnsw_partitions([None, s.built[4]], [[], [1]], EFC)),
    "mixed m": ("INVALID", "partition 1: the prior index has m = 4", lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4], c.other_m], [[1], [1]], EFC)),
    "all NULL": ("INVALID", "every prior index is NULL", lambda s, c: s.corpus.vacuum_hnsw_partitions([None, None], [[1], []], EFC)),
    "row out of range": ("INVALID", "partition 1, position 2: dead row 4000 is outside",
                         lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4], s.built[3]], [[1], [5, 6, N]], EFC)),
    "corrupted loaded prior": ("INVALID", "partition 1: the prior index: element .* lists neighbour 1500 on layer",
                               lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4], c.bad], [[1], [1]], EFC)),
    "ef_construction": ("UNSUPPORTED", "at least 2 \\* m", lambda s, c: s.corpus.vacuum_hnsw_partitions([s.built[4]], [[1]], 7)),
}


class _Extras:
    def __init__(self, ctx, s):
        self.twin = _load(ctx, "f32", s.x[:100])
        self.other_m = s.corpus.build_hnsw_partitions([np.arange(20)], 4, EFC, "l2", SEED)[0]
        self.bad = _bad_loaded(s)


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["sparse", "duplicate rows are vacuum's: harmless"])
def test_refusals(ctx, scene, what):
    import vsrbac
    from vsrbac import _ffi
    s = scene(*KINDS[0])
    if what == "sparse":
        sparse = ctx.load_corpus_sparse(np.arange(9, dtype=np.int64), np.arange(8, dtype=np.int32), np.ones(8, dtype=np.float32), 8)
        with pytest.raises(vsrbac.VsrError, match="sparsevec") as info:
            sparse.vacuum_hnsw_partitions([None], [[1]], EFC)
        assert info.value.status == _ffi.ERR_UNSUPPORTED
        sparse.free()
        return
    if what.startswith("duplicate"):
        d = s.dead[0]
        a, ma, _ = s.corpus.vacuum_hnsw_partitions([s.built[0]], [d], EFC)
        b, mb, _ = s.corpus.vacuum_hnsw_partitions([s.built[0]], [np.concatenate([d, d[:7], d[:1]])], EFC)
        same_graph(a[0].export(), b[0].export())
        np.testing.assert_array_equal(ma[0], mb[0])
        a[0].free()
        b[0].free()
        return
    status, fragment, call = REFUSALS[what]
    extras = _Extras(ctx, s)
    with pytest.raises(vsrbac.VsrError, match=fragment) as info:
        call(s, extras)
    assert info.value.status == getattr(_ffi, "ERR_" + status)
    extras.other_m.free()
    extras.bad.free()
    extras.twin.free()
    same_graph(s.built[4].export(), s.exports[4])                               # nothing was written through
    ctx.screening_check(0)
