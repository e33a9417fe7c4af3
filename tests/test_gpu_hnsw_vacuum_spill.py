"""vsr_hnsw_vacuum where a repair's working set outgrows the LDS: the spill form (hnsw_vacuum_search_spill_kernel), which keeps the
candidates, the selection's scratch and the visited set of a repair in a workspace in global memory, the mixed attempt that runs
where the ladders end, and the three knobs that reach them (VSR_HNSW_VACUUM_SPILL, VSR_HNSW_VACUUM_LDS,
VSR_HNSW_VACUUM_SPILL_WAVES).

The contract is the one of tests/test_gpu_hnsw_vacuum.py: tests/hnsw_vacuum_model.py on integer-valued rows, array for array;
which form a repair ran in must not show in the result."""
import time

import numpy as np
import pytest

import hnsw_vacuum_model as vm
from helpers import same_graph
from test_gpu_hnsw_extend import _corpus, _build_on, _raises
from test_gpu_hnsw_vacuum import EFC1, STAT_KEYS, _case1, _model_metric, _model_rows, _same_as_model

pytestmark = pytest.mark.gpu

# The LDS budget of the mixed test, found on the GPU for the seeded data of _case1("f32", "l2"): a sweep over 4416 (the least the
# knob takes at ef_construction = 32), 5000, 6000, 8000, 12 000, 16 000 and 24 000 bytes, printing vacuum_spill_info() for each.
# At 6000 bytes the sizing gives 80 candidates beside a visited table of 512 entries; the table fills at 384 visited elements and
# the next one (1024 entries, 7888 bytes) does not fit, so the visited ladder ends at once and the repairs that visit more than
# 384 elements spill while the others stay on the LDS kernel.  The assertion 0 < spilled < repaired is what guards the value.
MIXED_LDS = "6000"


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _vacuum(ctx, monkeypatch, env, kind, x, g, dead, efc, metric, doc=None):
    """(export, stats, (spilled_repairs, workspace_bytes)) of a vacuum under the knobs in `env`; the guard word must be clean."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    try:
        corpus = _corpus(ctx, kind, x, doc)
        idx, st = corpus.vacuum_hnsw(g, dead, efc, metric)
    finally:
        for name in env:
            monkeypatch.delenv(name)
    ctx.screening_check(0)
    out, info = idx.export(), idx.vacuum_spill_info()
    idx.free()
    corpus.free()
    return out, st, info


ALL = {"VSR_HNSW_VACUUM_SPILL": "all"}


# ---- 1: the spill form is the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming")])
def test_spill_form_is_the_model(ctx, monkeypatch, kind, metric):
    c = _case1(ctx, kind, metric)
    got, st, (spilled, ws_bytes) = _vacuum(ctx, monkeypatch, ALL, kind, c["x"], c["g"], c["dead"], EFC1, metric)
    print(f"spill all {kind} {metric}: spilled {spilled}, workspace {ws_bytes} bytes, attempts {st['attempts']}")
    _same_as_model(got, st, c["want"], c["wst"])
    same_graph(got, c["got"])
    vm.check_invariants(got, c["dead"])
    assert spilled == st["elements_repaired"] and st["attempts"] == 1 and ws_bytes > 0


def test_spill_form_through_the_element_to_row_map(ctx, monkeypatch):
    c = _case1(ctx, "f32", "l2")
    doc = (np.random.default_rng(8600).permutation(1500) + 1).astype(np.int32)
    got, st, (spilled, _) = _vacuum(ctx, monkeypatch, ALL, "f32", c["x"], c["g"], c["dead"], EFC1, "l2", doc=doc)
    _same_as_model(got, st, c["want"], c["wst"])
    assert spilled == st["elements_repaired"]


def test_default_run_of_a_graph_that_fits_spills_nothing(ctx):
    c = _case1(ctx, "f32", "l2")
    corpus = _corpus(ctx, "f32", c["x"])
    idx, st = corpus.vacuum_hnsw(c["g"], c["dead"], EFC1, "l2")
    assert idx.vacuum_spill_info() == (0, 0) and st["attempts"] == c["st"]["attempts"]
    idx.free()
    corpus.free()


# ---- 2: the entry phase in spill form ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """600 rows, m = 4 (several layers), ef_construction = 16."""
    x = np.random.default_rng(8200).integers(0, 16, (600, 8)).astype(np.float32)
    corpus = _corpus(ctx, "f32", x)
    idx = _build_on(corpus, "f32", 4, 16, "l2", 42)
    g = idx.export()
    info = idx.vacuum_spill_info()
    idx.free()
    corpus.free()
    assert g["max_level"] >= 2 and (g["tids"][:, 0] == np.arange(600)).all()
    return x, g, info


@pytest.mark.parametrize("case", ["entry_dead", "entry_neighbour_dead", "only_entry", "only_one_other"])
def test_entry_phase_in_spill_form(ctx, monkeypatch, small, case):
    x, g, _ = small
    entry = int(g["entry"])
    keep = 17 if entry != 17 else 18
    dead = {"entry_dead": [entry], "entry_neighbour_dead": [int(g["nbr0"][entry, 0])], "only_entry": np.delete(np.arange(600), entry),
            "only_one_other": np.delete(np.arange(600), keep)}[case]           # only_entry: a batch of one searched from -1
    got, st, (spilled, _) = _vacuum(ctx, monkeypatch, ALL, "f32", x, g, dead, 16, "l2")
    want, wst = vm.vacuum(g, x, "l2", dead, 16)
    _same_as_model(got, st, want, wst)
    vm.check_invariants(got, dead)
    assert spilled == st["elements_repaired"] >= 1
    if case in ("only_entry", "only_one_other"):
        assert len(got["level"]) == 1 and (got["nbr0"] == -1).all() and st["elements_repaired"] == 1


# ---- 3: the mixed attempt ---------------------------------------------------------------------------------------------------------------
def test_mixed_attempt_where_the_ladder_ends(ctx, monkeypatch):
    from vsrbac import _ffi
    c = _case1(ctx, "f32", "l2")
    got, st, (spilled, ws_bytes) = _vacuum(ctx, monkeypatch, {"VSR_HNSW_VACUUM_LDS": MIXED_LDS}, "f32", c["x"], c["g"], c["dead"], EFC1, "l2")
    print(f"mixed at {MIXED_LDS} bytes: spilled {spilled} of {st['elements_repaired']} repairs, attempts {st['attempts']}, workspace {ws_bytes}")
    assert 0 < spilled < st["elements_repaired"] and st["attempts"] >= 2
    _same_as_model(got, st, c["want"], c["wst"])
    same_graph(got, c["got"])
    vm.check_invariants(got, c["dead"])
    monkeypatch.setenv("VSR_HNSW_VACUUM_LDS", MIXED_LDS)
    monkeypatch.setenv("VSR_HNSW_VACUUM_SPILL", "0")
    corpus = _corpus(ctx, "f32", c["x"])
    _raises(_ffi.ERR_UNSUPPORTED, "fits the LDS", corpus.vacuum_hnsw, c["g"], c["dead"], EFC1, "l2")
    monkeypatch.delenv("VSR_HNSW_VACUUM_LDS")
    monkeypatch.delenv("VSR_HNSW_VACUUM_SPILL")
    ctx.screening_check(0)
    corpus.free()


# ---- 4: workspaces are reused -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", ["1", "3"])
def test_a_small_pool_reuses_its_workspaces(ctx, monkeypatch, waves):
    c = _case1(ctx, "f32", "l2")
    env = dict(ALL, VSR_HNSW_VACUUM_SPILL_WAVES=waves)
    got, st, (spilled, ws_bytes) = _vacuum(ctx, monkeypatch, env, "f32", c["x"], c["g"], c["dead"], EFC1, "l2")
    same_graph(got, c["got"])
    np.testing.assert_array_equal(st["elem_map"], c["st"]["elem_map"])
    assert {k: st[k] for k in STAT_KEYS} == {k: c["st"][k] for k in STAT_KEYS} and spilled == st["elements_repaired"]
    # one workspace: 28 bytes and a bit per element of the graph, rounded up to 16 bytes
    assert ws_bytes == int(waves) * ((1500 * 28 + ((1500 + 31) // 32) * 4 + 15) // 16 * 16)


def test_spill_form_in_batches_of_64(ctx, monkeypatch):
    c = _case1(ctx, "f32", "l2")
    env = dict(ALL, VSR_HNSW_VACUUM_BATCH="64", VSR_HNSW_VACUUM_SPILL_WAVES="3")
    got, st, (spilled, _) = _vacuum(ctx, monkeypatch, env, "f32", c["x"], c["g"], c["dead"], EFC1, "l2")
    want, wst = vm.vacuum(c["g"], c["x"], "l2", c["dead"], EFC1, batch=64)
    _same_as_model(got, st, want, wst)
    assert spilled == st["elements_repaired"] and st["batches"] > c["st"]["batches"]


# ---- 5: a call that used to be refused --------------------------------------------------------------------------------------------------
LIVE_011 = sorted([123] + list(range(200, 16_000, 250))[:63])


def test_16000_rows_all_but_a_few_deleted(ctx, monkeypatch):
    """The data of test_delete_all_but_one_of_pgvector_011 at 16 000 rows: i % v, seed 11, m = 16, ef_construction = 64, every row but
    LIVE_011 deleted.  A repair stops admitting everything once it has pushed ef_construction + 1 = 65 live elements, itself among
    them; with 64 live rows it never does, so each repair's working set is the whole graph: 16 000 visited elements need a table of
    32 768 entries (it fills at 3/4), and beside that table the LDS holds (159 744 - 3 072 - 131 072 - 64) / 9 = 2 832 candidates,
    far below 16 000: without the spill form the call is refused.  64 live rows are the most for which that reasoning holds, and
    fewer than the CPU model could repair in 10 s: it repairs the 64 in 1.9 s, the vacuum takes 0.2 s (times printed)."""
    from vsrbac import _ffi
    n = 16_000
    v = np.random.default_rng(11).integers(0, 1000, 3) + 1
    x = (np.arange(n)[:, None] % v[None, :]).astype(np.float32)
    dead = np.setdiff1d(np.arange(n), LIVE_011)
    corpus = _corpus(ctx, "f32", x)
    idx = corpus.build_hnsw(16, 64, "l2", seed=11)
    g = idx.export()
    t0 = time.perf_counter()
    vac, st = corpus.vacuum_hnsw(g, dead, 64, "l2")
    t1 = time.perf_counter()
    spilled, ws_bytes = vac.vacuum_spill_info()
    ctx.screening_check(0)
    want, wst = vm.vacuum(g, x, "l2", dead, 64)
    t2 = time.perf_counter()
    print(f"16 000 rows, {len(LIVE_011)} live: spilled {spilled} of {st['elements_repaired']} repairs, attempts {st['attempts']}, "
          f"workspace {ws_bytes} bytes, vacuum {t1 - t0:.2f} s, model {t2 - t1:.2f} s")
    assert spilled >= 1
    _same_as_model(vac.export(), st, want, wst)
    res, _ = vac.search(np.zeros((1, 3), np.float32), 100, 100, "l2")
    assert res.counts[0] == len(LIVE_011) and sorted(res.rows[0, :len(LIVE_011)].tolist()) == LIVE_011
    monkeypatch.setenv("VSR_HNSW_VACUUM_SPILL", "0")
    _raises(_ffi.ERR_UNSUPPORTED, "fits the LDS", corpus.vacuum_hnsw, g, dead, 64, "l2")
    monkeypatch.delenv("VSR_HNSW_VACUUM_SPILL")
    ctx.screening_check(0)
    for h in (vac, idx):
        h.free()
    corpus.free()


# ---- 6: half of a graph deleted at m = 16 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "half", "bit"])
def test_half_of_a_graph_deleted(ctx, monkeypatch, kind):
    rng = np.random.default_rng(8960)
    x = rng.integers(0, 2, (6000, 128)).astype(np.float32) if kind == "bit" else rng.standard_normal((6000, 16)).astype(np.float32)
    metric = "hamming" if kind == "bit" else "l2"
    dead = rng.choice(6000, 3000, replace=False)
    corpus = _corpus(ctx, kind, x)
    idx = _build_on(corpus, kind, 16, 64, metric, 96)
    g = idx.export()
    idx.free()
    corpus.free()
    a, sa, (spilled, _) = _vacuum(ctx, monkeypatch, {}, kind, x, g, dead, 64, metric)
    b, sb, _ = _vacuum(ctx, monkeypatch, {}, kind, x, g, dead, 64, metric)
    s, ss, (all_spilled, ws_bytes) = _vacuum(ctx, monkeypatch, ALL, kind, x, g, dead, 64, metric)
    print(f"half deleted {kind}: default run spilled {spilled} of {sa['elements_repaired']} repairs in {sa['attempts']} attempts; "
          f"all: {all_spilled} repairs in a pool of {ws_bytes} bytes")
    same_graph(a, b)
    same_graph(a, s)
    np.testing.assert_array_equal(sa["elem_map"], ss["elem_map"])
    assert {k: sa[k] for k in STAT_KEYS} == {k: sb[k] for k in STAT_KEYS} == {k: ss[k] for k in STAT_KEYS}
    vm.check_invariants(a, dead)
    assert all_spilled == ss["elements_repaired"]


# ---- 7: the knobs ---------------------------------------------------------------------------------------------------------------------------
def test_knob_validation_and_info_of_a_built_index(ctx, monkeypatch, small):
    from vsrbac import _ffi
    x, g, info = small
    assert info == (0, 0)
    corpus = _corpus(ctx, "f32", x)
    for name, value, fragment in (("VSR_HNSW_VACUUM_SPILL", "2", "VSR_HNSW_VACUUM_SPILL must be 0, 1 or all"),
                                  ("VSR_HNSW_VACUUM_LDS", "100", "VSR_HNSW_VACUUM_LDS must be between [0-9]+ and [0-9]+"),
                                  ("VSR_HNSW_VACUUM_SPILL_WAVES", "0", "VSR_HNSW_VACUUM_SPILL_WAVES must be between 1 and [0-9]+")):
        monkeypatch.setenv(name, value)
        _raises(_ffi.ERR_INVALID, fragment, corpus.vacuum_hnsw, g, [1], 16)
        monkeypatch.delenv(name)
    loaded = corpus.load_hnsw(g)
    assert loaded.vacuum_spill_info() == (0, 0)
    loaded.free()
    corpus.free()
