"""vsr_hnsw_vacuum (Corpus.vacuum_hnsw): rows deleted from an HNSW graph, the graph repaired on the GPU and compacted.

The contract is tests/hnsw_vacuum_model.py, pgvector's hnswvacuum.c under the GPU's batched schedule with pgvector's two heaps
taken literally; tests/test_hnsw_vacuum_cpu.py pins its pieces to the serial model of the build.  Rows are small integers, so
every distance is exact and the comparison is array for array: elem_map, entry, every exported array, the stats.  Inputs are
exports of vsr_hnsw_build*.  Recall parity: the floors of pgvector's test/t/014 (vector), 026 (halfvec), 022 (bit) and 011."""
import numpy as np
import pytest

import hnsw_vacuum_model as vm
from helpers import same_graph
from hnsw_bit_model import tap_recall, tie_aware_expected
from hnsw_half_model import to_half
from test_gpu_hnsw_extend import _corpus, _build_on, _damaged, _raises, _same_result

pytestmark = pytest.mark.gpu

STAT_KEYS = ("tuples_removed", "tuples_kept", "elements_removed", "elements_repaired", "batches")


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _model_rows(kind, x):
    """The rows the model measures on: a bit corpus as 0 / 1 floats, where squared L2 is the Hamming distance."""
    return (np.asarray(x) != 0).astype(np.float32) if kind == "bit" else np.asarray(x, dtype=np.float32)


def _model_metric(metric):
    return "l2" if metric == "hamming" else metric


def _vacuum(ctx, kind, x, g, dead, efc, metric, doc=None):
    """(export, stats) of the vacuumed index; the guard word must be clean afterwards."""
    corpus = _corpus(ctx, kind, x, doc)
    idx, st = corpus.vacuum_hnsw(g, dead, efc, metric)
    ctx.screening_check(0)
    out = idx.export()
    idx.free()
    corpus.free()
    return out, st


def _same_as_model(got, st, want, wst):
    for key in ("level", "nbr0", "tid_count", "tids", "up_slot"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["entry"], got["max_level"], got["m"]) == (want["entry"], want["max_level"], want["m"])
    n_upper = int((want["up_slot"] >= 0).sum())
    assert got["up_nbr"].shape == want["up_nbr"].shape
    np.testing.assert_array_equal(got["up_nbr"][:n_upper], want["up_nbr"][:n_upper], err_msg="up_nbr")
    np.testing.assert_array_equal(st["elem_map"], wst["elem_map"])
    assert {k: st[k] for k in STAT_KEYS} == {k: wst[k] for k in STAT_KEYS}
    assert st["attempts"] >= 1


# ---- 1: equality with the model ---------------------------------------------------------------------------------------------------------
CASE1 = {}                                                                      # (kind, metric) -> the case, built once
M1, EFC1 = 8, 32


def _case1(ctx, kind, metric):
    """1500 x 8 rows of integers 0 .. 15 (bit: 1500 x 64 bits), m = 8, ef_construction = 32; 450 scattered rows and the entry's
    row are deleted.  Holds the build's export, the dead rows, the default vacuum and the model's (batch 4096)."""
    key = (kind, metric)
    if key not in CASE1:
        rng = np.random.default_rng(8100)
        x = rng.integers(0, 2, (1500, 64)).astype(np.float32) if kind == "bit" else rng.integers(0, 16, (1500, 8)).astype(np.float32)
        corpus = _corpus(ctx, kind, x)
        idx = _build_on(corpus, kind, M1, EFC1, metric, 41)
        g = idx.export()
        idx.free()
        corpus.free()
        entry_row = int(g["tids"][g["entry"], 0])
        dead = np.union1d(rng.choice(1500, 450, replace=False), [entry_row])
        got, st = _vacuum(ctx, kind, x, g, dead, EFC1, metric)
        want, wst = vm.vacuum(g, _model_rows(kind, x), _model_metric(metric), dead, EFC1)
        CASE1[key] = {"x": x, "g": g, "dead": dead, "got": got, "st": st, "want": want, "wst": wst}
    return CASE1[key]


@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming")])
def test_vacuum_is_the_model(ctx, kind, metric):
    c = _case1(ctx, kind, metric)
    print(f"vacuum {kind} {metric}: stats {({k: c['st'][k] for k in STAT_KEYS + ('attempts',)})}, model {({k: c['wst'][k] for k in STAT_KEYS})}")
    _same_as_model(c["got"], c["st"], c["want"], c["wst"])
    vm.check_invariants(c["got"], c["dead"])
    assert c["st"]["elements_removed"] == len(c["dead"]) and c["st"]["elements_repaired"] > 450


# ---- 2: the entry phase -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """600 rows, m = 4 (several layers), ef_construction = 16."""
    x = np.random.default_rng(8200).integers(0, 16, (600, 8)).astype(np.float32)
    corpus = _corpus(ctx, "f32", x)
    idx = _build_on(corpus, "f32", 4, 16, "l2", 42)
    g = idx.export()
    idx.free()
    corpus.free()
    assert g["max_level"] >= 2 and (g["tids"][:, 0] == np.arange(600)).all()
    return x, g


@pytest.mark.parametrize("case", ["entry_dead", "entry_neighbour_dead", "only_entry", "only_one_other"])
def test_entry_phase_against_the_model(ctx, small, case):
    x, g = small
    entry = int(g["entry"])
    keep = 17 if entry != 17 else 18
    dead = {"entry_dead": [entry], "entry_neighbour_dead": [int(g["nbr0"][entry, 0])], "only_entry": np.delete(np.arange(600), entry),
            "only_one_other": np.delete(np.arange(600), keep)}[case]           # the last one walks the whole dead graph
    got, st = _vacuum(ctx, "f32", x, g, dead, 16, "l2")
    want, wst = vm.vacuum(g, x, "l2", dead, 16)
    _same_as_model(got, st, want, wst)
    vm.check_invariants(got, dead)
    if case == "entry_dead":
        assert st["elem_map"][entry] == -1 and got["tids"][got["entry"], 0] != entry
    if case == "entry_neighbour_dead":
        assert got["tids"][got["entry"], 0] == entry
    if case in ("only_entry", "only_one_other"):
        assert len(got["level"]) == 1 and (got["nbr0"] == -1).all() and got["entry"] == 0 and st["elements_repaired"] == 1
        assert got["tids"][0, 0] == (entry if case == "only_entry" else keep)


def test_everything_dead_leaves_an_empty_index(ctx, small):
    x, g = small
    corpus = _corpus(ctx, "f32", x)
    idx, st = corpus.vacuum_hnsw(g, np.arange(600), 16, "l2")
    assert idx.info()[:2] == (0, -1) and (st["elem_map"] == -1).all()
    assert (st["tuples_removed"], st["tuples_kept"], st["elements_removed"], st["elements_repaired"]) == (600, 0, 600, 0)
    out = idx.export()
    assert len(out["level"]) == 0 and out["entry"] == -1
    res, _ = idx.search(x[:3], 5, 40, "l2")
    assert (res.counts == 0).all()
    idx.free()
    corpus.free()


# ---- 3: several batches ---------------------------------------------------------------------------------------------------------------------
def test_batch_knob_reaches_the_schedule(ctx, monkeypatch):
    c = _case1(ctx, "f32", "l2")
    monkeypatch.setenv("VSR_HNSW_VACUUM_BATCH", "64")
    got, st = _vacuum(ctx, "f32", c["x"], c["g"], c["dead"], EFC1, "l2")
    monkeypatch.delenv("VSR_HNSW_VACUUM_BATCH")
    want, wst = vm.vacuum(c["g"], c["x"], "l2", c["dead"], EFC1, batch=64)
    _same_as_model(got, st, want, wst)
    assert st["batches"] > c["st"]["batches"]
    assert any((got[k] != c["got"][k]).any() for k in ("nbr0", "up_nbr")), "batches of 64 and of 4096 gave one graph"


# ---- 4: both ladders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,value", [("VSR_HNSW_BUILD_VISITED_SLOTS", "256"), ("VSR_HNSW_VACUUM_CAPS", str(EFC1 + 1))])
def test_restarts_give_the_default_runs_arrays(ctx, monkeypatch, knob, value):
    c = _case1(ctx, "f32", "l2")
    monkeypatch.setenv(knob, value)
    got, st = _vacuum(ctx, "f32", c["x"], c["g"], c["dead"], EFC1, "l2")
    monkeypatch.delenv(knob)
    print(f"{knob}={value}: attempts {st['attempts']} (default run {c['st']['attempts']})")
    same_graph(got, c["got"])
    np.testing.assert_array_equal(st["elem_map"], c["st"]["elem_map"])
    assert st["attempts"] > 1 and {k: st[k] for k in STAT_KEYS} == {k: c["st"][k] for k in STAT_KEYS}


# ---- 5: a merged prior graph ----------------------------------------------------------------------------------------------------------------
def test_merged_elements_lose_tids_before_they_go(ctx):
    """800 rows: 70 distinct vectors ten times over plus 100 singles, built with merge_duplicates.  3 of an element's 10 TIDs deleted:
    it stays, the other 7 in order, its vector still its first survivor's row; all 10 deleted: it goes."""
    rng = np.random.default_rng(8500)
    base = rng.integers(0, 16, (170, 8)).astype(np.float32)
    assert len(np.unique(base, axis=0)) == 170
    x = np.concatenate([np.repeat(base[:70], 10, axis=0), base[70:]])[rng.permutation(800)]
    corpus = _corpus(ctx, "f32", x)
    idx = _build_on(corpus, "f32", 8, 32, "l2", 45, merge=True)
    g = idx.export()
    idx.free()
    full = np.flatnonzero(g["tid_count"] == 10)
    assert len(g["level"]) == 170 and len(full) == 70
    thin, gone = int(full[3]), int(full[9])
    dead = np.concatenate([g["tids"][thin, [0, 4, 9]], g["tids"][gone, :10]])
    new, st = corpus.vacuum_hnsw(g, dead, 32, "l2")
    out = new.export()
    want, wst = vm.vacuum(g, x, "l2", dead, 32)
    _same_as_model(out, st, want, wst)
    vm.check_invariants(out, dead)
    k = st["elem_map"][thin]
    assert st["elem_map"][gone] == -1 and k >= 0 and out["tid_count"][k] == 7
    np.testing.assert_array_equal(out["tids"][k, :7], g["tids"][thin, [1, 2, 3, 5, 6, 7, 8]])
    assert (st["tuples_removed"], st["tuples_kept"], st["elements_removed"]) == (13, 787, 1)
    res, _ = new.search(x[g["tids"][thin, 1]][None, :], 7, 40, "l2")
    assert sorted(res.rows[0, :7].tolist()) == sorted(g["tids"][thin, [1, 2, 3, 5, 6, 7, 8]].tolist()) and (res.dist[0, :7] == 0).all()
    new.free()
    corpus.free()


# ---- 6: interleaved document order -----------------------------------------------------------------------------------------------------------
def test_interleaved_document_order_takes_the_element_to_row_map(ctx):
    """The same rows under document ids that shuffle the internal order: elements reach their rows through the map, and the
    result is the direct form's."""
    c = _case1(ctx, "f32", "l2")
    doc = (np.random.default_rng(8600).permutation(1500) + 1).astype(np.int32)
    got, st = _vacuum(ctx, "f32", c["x"], c["g"], c["dead"], EFC1, "l2", doc=doc)
    same_graph(got, c["got"])
    np.testing.assert_array_equal(st["elem_map"], c["st"]["elem_map"])


# ---- 7: round trip, validity, composition ----------------------------------------------------------------------------------------------------
def test_round_trip_validity_and_composition(ctx):
    from vsrbac.formats import remap_hnsw_rows
    c = _case1(ctx, "f32", "l2")
    x, dead = c["x"], c["dead"]
    rng = np.random.default_rng(8700)
    q = x[rng.integers(0, 1500, 12)] + rng.integers(-2, 3, (12, 8)).astype(np.float32)
    corpus = _corpus(ctx, "f32", x)
    old = corpus.load_hnsw(c["g"])
    vac, st = old.vacuumed(dead, EFC1)
    again = corpus.load_hnsw(vac.export())
    for ef in (10, 40, 200):
        a = vac.search(q, 10, ef, "l2")
        _same_result(a, again.search(q, 10, ef, "l2"))
        assert not np.isin(a[0].rows[a[0].rows >= 0], dead).any()
    # the recipe: onto a corpus without the dead rows
    live = np.setdiff1d(np.arange(1500), dead)
    new_of = np.full(1500, -1)
    new_of[live] = np.arange(len(live))
    packed = _corpus(ctx, "f32", x[live])
    remapped = remap_hnsw_rows(vac.export(), new_of)
    moved = packed.load_hnsw(remapped)
    same = packed.extend_hnsw(remapped, EFC1, "l2", 41)                         # no new rows there: the full host validation
    same_graph(same.export(), remapped)
    same.free()
    a, b = vac.search(q, 10, 40, "l2")[0], moved.search(q, 10, 40, "l2")[0]
    np.testing.assert_array_equal(new_of[a.rows], b.rows)
    np.testing.assert_array_equal(a.dist, b.dist)
    for h in (moved, again, vac, old):
        h.free()
    packed.free()
    corpus.free()


def test_update_is_vacuum_then_extend(ctx):
    """UPDATE of 30 % of the rows: the old versions vacuumed, the graph moved onto a corpus of the live rows plus the new versions
    (the extension inserts every row no TID names, so the dead rows must be gone), the new versions inserted.  The insert floor
    of pgvector's 013: 0.99 at ef_search 40, LIMIT 20, m = 16, ef_construction = 64."""
    from vsrbac.formats import remap_hnsw_rows
    rng = np.random.default_rng(8701)
    n, k = 4000, 20
    x = (rng.random((n, 3)) * rng.random((n, 3))).astype(np.float32)
    fresh = (rng.random((1200, 3)) * rng.random((1200, 3))).astype(np.float32)
    q = rng.random((20, 3)).astype(np.float32)
    dead = rng.choice(n, 1200, replace=False)
    live = np.setdiff1d(np.arange(n), dead)
    new_of = np.full(n, -1)
    new_of[live] = np.arange(len(live))
    corpus = _corpus(ctx, "f32", x)
    built = _build_on(corpus, "f32", 16, 64, "l2", 3)
    vac, _ = built.vacuumed(dead, 64)
    g = remap_hnsw_rows(vac.export(), new_of)
    y = np.concatenate([x[live], fresh])
    both = _corpus(ctx, "f32", y)
    idx = both.extend_hnsw(g, 64, "l2", 3)
    assert idx.info()[0] == n
    got, _ = idx.search(q, k, 40, "l2")
    hit = 0
    for i in range(20):
        d = ((y.astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(axis=1)
        hit += int((d[got.rows[i, :got.counts[i]]] <= np.sort(d)[k - 1]).sum())
    print(f"vacuum then extend: recall@20 {hit / (20 * k):.4f}")
    assert hit / (20 * k) >= 0.99
    for h in (idx, vac, built):
        h.free()
    both.free()
    corpus.free()


# ---- 8: pgvector's floors ---------------------------------------------------------------------------------------------------------------------
def _tap_case(ctx, kind, seed, n=10_000, keep=2500):
    """test/t/014_hnsw_vector_vacuum_recall.pl: n rows of 3 random() values (022: 52 random bits), m = 4, ef_construction = 8, the
    rows >= keep deleted, 20 random queries, LIMIT 20.  Returns recall before the vacuum (dead rows filtered from the answers, as
    the executor does) and after, per ef_search, tie-aware."""
    rng = np.random.default_rng(seed)
    if kind == "bit":
        x = rng.integers(0, 2, (n, 52)).astype(np.float32)
        q = rng.integers(0, 2, (20, 52)).astype(np.float32)
        metric = "hamming"
    else:
        x = rng.random((n, 3)).astype(np.float32)
        q = rng.random((20, 3)).astype(np.float32)
        metric = "l2"
        if kind == "half":
            x, q = to_half(x).astype(np.float32), to_half(q).astype(np.float32)
    d = ((x[None, :keep].astype(np.float64) - q[:, None].astype(np.float64)) ** 2).sum(axis=2)
    expected = [tie_aware_expected(d[i], 20) for i in range(20)]
    corpus = _corpus(ctx, kind, x)
    idx = _build_on(corpus, kind, 4, 8, metric, seed)
    vac, st = idx.vacuumed(np.arange(keep, n), 8, metric)

    def recall(index, ef):
        if kind == "bit":
            res, _ = index.search_bit(q != 0, ef, ef, metric)
        else:
            res, _ = index.search(q, ef, ef, metric)
        found = [res.rows[i, :res.counts[i]] for i in range(20)]
        return tap_recall([f[f < keep] for f in found], expected, 20)

    out = {"before": {ef: recall(idx, ef) for ef in (20, 100)}, "after": {ef: recall(vac, ef) for ef in (20, 100)}, "stats": st,
           "graph": vac.export()}
    for h in (vac, idx):
        h.free()
    corpus.free()
    return out


@pytest.mark.parametrize("kind", ["f32", "half"])
def test_vacuum_recall_floors_of_pgvector_014_026(ctx, kind):
    r = _tap_case(ctx, kind, 14)
    print(f"vacuum recall {kind}: before {r['before']}, after {r['after']}, stats {({k: r['stats'][k] for k in STAT_KEYS + ('attempts',)})}")
    vm.check_invariants(r["graph"], np.arange(2500, 10_000))
    assert r["before"][20] >= 0.18 and r["before"][100] >= 0.93
    assert r["after"][20] >= 0.95


def test_vacuum_recall_floors_of_pgvector_022_bit(ctx):
    r = _tap_case(ctx, "bit", 22)
    print(f"vacuum recall bit: before {r['before']}, after {r['after']}, stats {({k: r['stats'][k] for k in STAT_KEYS + ('attempts',)})}")
    vm.check_invariants(r["graph"], np.arange(2500, 10_000))
    assert r["before"][100] >= 0.35
    assert r["after"][100] >= 0.80


def test_delete_all_but_one_of_pgvector_011(ctx):
    """test/t/011_hnsw_vacuum.pl: 10 000 x 3 rows i % v (v = 1 + three draws below 1000, seed 11), default m and ef_construction,
    every row but 123 deleted: a search from [0, 0, 0] returns 123 alone.
    The one repair (row 123, searched from the deleted entry point) admits every element it meets, so its working set is all
    10 000 elements: the candidate array and the visited table that hold them (9 bytes and 4 bytes an entry) fill the LDS of one
    workgroup, the largest single repair the call can run."""
    v = np.random.default_rng(11).integers(0, 1000, 3) + 1
    x = (np.arange(10_000)[:, None] % v[None, :]).astype(np.float32)
    corpus = _corpus(ctx, "f32", x)
    idx = corpus.build_hnsw(16, 64, "l2", seed=11)
    vac, st = idx.vacuumed(np.delete(np.arange(10_000), 123), 64)
    print(f"vacuum 011: stats {({k: st[k] for k in STAT_KEYS + ('attempts',)})}")
    res, _ = vac.search(np.zeros((1, 3), np.float32), 10, 40, "l2")
    assert res.counts[0] == 1 and res.rows[0, 0] == 123
    for h in (vac, idx):
        h.free()
    corpus.free()


# ---- 9: determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_on_real_valued_rows_agree(ctx):
    rng = np.random.default_rng(8900)
    x = rng.standard_normal((3000, 24)).astype(np.float32)
    dead = rng.choice(3000, 1000, replace=False)
    corpus = _corpus(ctx, "f32", x)
    idx = _build_on(corpus, "f32", 8, 32, "l2", 49)
    a, sa = idx.vacuumed(dead, 32)
    b, sb = idx.vacuumed(dead, 32)
    ga = a.export()
    same_graph(ga, b.export())
    vm.check_invariants(ga, dead)
    assert {k: sa[k] for k in STAT_KEYS} == {k: sb[k] for k in STAT_KEYS}
    for h in (a, b, idx):
        h.free()
    corpus.free()


# ---- 10: more than 4096 repairs ----------------------------------------------------------------------------------------------------------------
def test_more_repairs_than_one_batch_holds(ctx):
    r = _tap_case(ctx, "f32", 15, n=12_000, keep=6000)
    print(f"vacuum 12 000: before {r['before']}, after {r['after']}, stats {({k: r['stats'][k] for k in STAT_KEYS + ('attempts',)})}")
    vm.check_invariants(r["graph"], np.arange(6000, 12_000))
    assert r["stats"]["elements_repaired"] > 4096 and r["stats"]["batches"] >= 2
    assert r["after"][20] >= 0.95


# ---- 11: refusals -------------------------------------------------------------------------------------------------------------------------------
def _raw_vacuum(corpus, g, dead, efc=16, metric=0, flags=0, m=None):
    import ctypes as C
    from vsrbac.engine import _ptr, check
    a = lambda name, dt: np.ascontiguousarray(g[name], dtype=dt)
    arrays = [a("level", np.int32), a("nbr0", np.int32), a("tid_count", np.int32), a("tids", np.int64), a("up_slot", np.int32),
              a("up_nbr", np.int32)]
    dead = np.ascontiguousarray(dead, dtype=np.int64)
    h = C.c_void_p()
    check(corpus._lib.vsr_hnsw_vacuum(corpus._h, int(g["m"] if m is None else m), arrays[0].size, int(g["entry"]), *[_ptr(v) for v in arrays],
                                      int((arrays[4] >= 0).sum()), int(g["max_level"]), efc, metric, _ptr(dead), dead.size, flags, None, None,
                                      C.byref(h)))
    corpus._lib.vsr_hnsw_free(h)


def test_refused_corpora_flags_and_parameters(ctx, small):
    from vsrbac import _ffi
    from hnsw_extend_model import empty_graph
    x, g = small
    rng = np.random.default_rng(8901)
    dense = np.where(rng.random((50, 40)) < 0.2, rng.integers(1, 5, (50, 40)), 0).astype(np.float32)
    dense[:, 0] = 1
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    sparse = ctx.load_corpus_sparse(indptr, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32), 40)
    _raises(_ffi.ERR_UNSUPPORTED, "sparsevec", sparse.vacuum_hnsw, empty_graph(4), [1], 16, "l2")
    sparse.free()
    corpus = _corpus(ctx, "f32", x)
    _raises(_ffi.ERR_INVALID, "flags must be 0", _raw_vacuum, corpus, g, [1], flags=1)
    _raises(_ffi.ERR_INVALID, "dead row 600 is outside", corpus.vacuum_hnsw, g, [3, 600], 16)
    _raises(_ffi.ERR_INVALID, "dead row -1 is outside", corpus.vacuum_hnsw, g, [-1], 16)
    _raises(_ffi.ERR_UNSUPPORTED, "m must be between 2 and 100", _raw_vacuum, corpus, g, [1], m=101, efc=400)
    _raises(_ffi.ERR_UNSUPPORTED, "ef_construction must be between 4 and 1000 and at least 2 \\* m", corpus.vacuum_hnsw, g, [1], 7)
    _raises(_ffi.ERR_UNSUPPORTED, "ef_construction must be between", corpus.vacuum_hnsw, g, [1], 1001)
    _raises(_ffi.ERR_UNSUPPORTED, "L2, inner product and cosine operator classes only", corpus.vacuum_hnsw, g, [1], 16, "hamming")
    _raises(_ffi.ERR_INVALID, "VSR_HNSW_VACUUM_BATCH must be between 1 and 4096", _with_env, "VSR_HNSW_VACUUM_BATCH", "4097", corpus.vacuum_hnsw, g, [1], 16)
    _raises(_ffi.ERR_INVALID, "VSR_HNSW_VACUUM_CAPS must be between 17 and", _with_env, "VSR_HNSW_VACUUM_CAPS", "16", corpus.vacuum_hnsw, g, [1], 16)
    idx, st = corpus.vacuum_hnsw(g, [], 16)                                     # no dead rows: the graph as it is
    same_graph(idx.export(), g)
    assert st["attempts"] == 0 and st["tuples_kept"] == 600 and (st["elem_map"] == np.arange(600)).all()
    idx.free()
    idx, st = corpus.vacuum_hnsw(g, [5, 5, 5], 16)                              # duplicates are one deletion
    assert (st["tuples_removed"], st["elements_removed"], idx.info()[0]) == (1, 1, 599)
    idx.free()
    corpus.free()


def _with_env(name, value, fn, *args):
    import os
    os.environ[name] = value
    try:
        return fn(*args)
    finally:
        del os.environ[name]


@pytest.mark.parametrize("rule", ["tid_count", "level", "tid_row", "id_high", "id_low", "upper_id", "packed", "neighbour_level",
                                  "slot_range", "slot_missing", "slot_shared", "slot_on_level_0", "entry", "row_twice"])
def test_damaged_prior_graphs_are_refused_naming_the_element(ctx, small, rule):
    from vsrbac import _ffi
    x, g = small
    assert (g["level"] >= 1).sum() >= 2 and g["tids"][3, 0] == 3
    bad, fragment = _damaged(g, rule)
    fragment = fragment.replace("row 400", "row 600") if rule == "tid_row" else fragment
    if rule == "tid_row":
        bad["tids"][7, 0] = 600
    corpus = _corpus(ctx, "f32", x)
    _raises(_ffi.ERR_INVALID, fragment, corpus.vacuum_hnsw, bad, [1], 16, "l2")
    corpus.free()
