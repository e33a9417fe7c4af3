"""The restatement tests/test_gpu_hnsw_vacuum.py rests on (tests/hnsw_vacuum_model.py): its pieces pinned to the serial model of
the build, its invariants, the entry-phase cases; and the ABI and Python surface of vsr_hnsw_vacuum.  Nothing here needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import hnsw_vacuum_model as vm
from helpers import same_graph
from oracle.oracle import HnswIndex as OracleHnsw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, dim=6, top=30, seed=7300):
    x = np.random.default_rng(seed).integers(0, top, (n, dim)).astype(np.float32)
    assert len(np.unique(x, axis=0)) == n
    return x


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_models_pieces_are_the_serial_builds(oracle, metric):
    """Run as an insertion -- no skip element, nothing dead, ef_construction as it is -- search_layer, select, the installation
    and link extend the serial build of 299 rows by row 299 to the serial build of all 300, array for array."""
    x = _rows(300)
    m, efc, seed = 4, 16, 5
    g299 = OracleHnsw.batched(oracle, metric, x[:299], m, efc, seed, batch_limit=1).export()
    g300 = OracleHnsw.batched(oracle, metric, x, m, efc, seed, batch_limit=1).export()
    lv = int(g300["level"][299])
    g = vm.Graph(g299, x, metric, extra_levels=[lv])
    if lv >= 1:
        g.up_slot[299] = int((g299["level"] >= 1).sum())
    vm.repair_batch(g, [299], g.entry, efc, [True] * 300, skip=False)
    if lv > g.level[g.entry]:
        g.entry = 299
    same_graph(vm.export(g), g300)


@pytest.fixture(scope="module")
def built(oracle):
    x = _rows(600, seed=7301)
    return x, OracleHnsw.batched(oracle, "l2", x, 4, 16, 9).export()


def _highest(g, dead_elems):
    cand = [e for e in range(len(g["level"])) if e != g["entry"] and e not in dead_elems]
    return max(cand, key=lambda e: (g["level"][e], -e)) if cand else -1


def test_model_invariants_after_a_scattered_vacuum(built):
    x, g = built
    dead = np.random.default_rng(3).choice(600, 200, replace=False)
    for batch in (vm.BATCH_MAX, 32):
        out, st = vm.vacuum(g, x, "l2", dead, 16, batch=batch)
        vm.check_invariants(out, dead)
        assert st["tuples_removed"] == 200 and st["tuples_kept"] == 400 and st["elements_removed"] == 200
        assert len(out["level"]) == 400 and (st["elem_map"] >= 0).sum() == 400
        assert st["elements_repaired"] >= 200 // 8 and st["batches"] >= 1
        live = np.setdiff1d(np.arange(600), dead)
        np.testing.assert_array_equal(out["tids"][:, 0], live)               # ascending old id, one TID each
        np.testing.assert_array_equal(st["elem_map"][live], np.arange(400))


def test_entry_dead_highest_live(built):
    x, g = built
    out, st = vm.vacuum(g, x, "l2", [g["entry"]], 16)
    vm.check_invariants(out, [g["entry"]])
    hp = _highest(g, {g["entry"]})
    assert out["entry"] == st["elem_map"][hp] and st["elem_map"][g["entry"]] == -1
    assert out["max_level"] == max(1, g["level"][hp])


def test_entry_live_with_a_dead_neighbour(built):
    x, g = built
    victim = int(g["nbr0"][g["entry"], 0])
    out, st = vm.vacuum(g, x, "l2", [victim], 16)
    vm.check_invariants(out, [victim])
    assert out["entry"] == st["elem_map"][g["entry"]] and st["elements_repaired"] >= 1


def test_only_the_entry_lives(built):
    x, g = built
    out, st = vm.vacuum(g, x, "l2", np.delete(np.arange(600), g["entry"]), 16)
    assert len(out["level"]) == 1 and out["entry"] == 0 and (out["nbr0"] == -1).all()
    assert out["tids"][0, 0] == g["entry"] and st["elements_repaired"] == 1
    assert (out["up_nbr"] <= 0).all()


def test_only_one_other_element_lives(built):
    x, g = built
    keep = 17 if g["entry"] != 17 else 18
    out, st = vm.vacuum(g, x, "l2", np.delete(np.arange(600), keep), 16)
    assert len(out["level"]) == 1 and out["entry"] == 0 and (out["nbr0"] == -1).all()      # it walked the whole dead graph
    assert out["tids"][0, 0] == keep and st["elements_repaired"] == 1 and st["elem_map"][keep] == 0
    assert out["max_level"] == max(1, g["level"][keep])


def test_everything_dead(built):
    x, g = built
    out, st = vm.vacuum(g, x, "l2", np.arange(600), 16)
    assert len(out["level"]) == 0 and out["entry"] == -1 and st["elements_repaired"] == 0 and (st["elem_map"] == -1).all()


def test_header_and_ffi_agree():
    from vsrbac import _ffi
    text = open(os.path.join(ROOT, "include", "vsrbac.h")).read()
    decl = re.search(r"\bint vsr_hnsw_vacuum\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, args = _ffi.SYMBOLS["vsr_hnsw_vacuum"]
    assert len(params) == len(args) == 20
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["corpus", "m", "n_elem", "entry", "level", "nbr0", "tid_count", "tids", "up_slot", "up_nbr", "n_upper", "max_level",
                     "ef_construction", "metric", "dead_rows", "n_dead", "flags", "out_elem_map", "out_stats", "out"]
    assert [f for f, _ in _ffi.HnswVacuumStats._fields_] == ["tuples_removed", "tuples_kept", "elements_removed", "elements_repaired",
                                                            "batches", "attempts"]
    import ctypes
    assert ctypes.sizeof(_ffi.HnswVacuumStats) == 32 and args[15] is ctypes.c_int64 and args[16] is ctypes.c_uint32
    assert "#define VSR_ABI_VERSION 2" in text


def test_python_surface():
    from vsrbac.engine import Corpus, HnswIndex
    from vsrbac import formats
    p = inspect.signature(Corpus.vacuum_hnsw).parameters
    assert list(p) == ["self", "graph", "dead_rows", "ef_construction", "metric"]
    assert (p["ef_construction"].default, p["metric"].default) == (64, None)
    p = inspect.signature(HnswIndex.vacuumed).parameters
    assert list(p) == ["self", "dead_rows", "ef_construction", "metric"]
    assert (p["ef_construction"].default, p["metric"].default) == (64, None)
    assert list(inspect.signature(formats.remap_hnsw_rows).parameters) == ["graph", "new_index_of_old_row"]
    for fn in (Corpus.vacuum_hnsw, HnswIndex.vacuumed, formats.remap_hnsw_rows):
        doc = " ".join(fn.__doc__.split())
        for word in ("vacuum", "export", "remap_hnsw_rows", "reload the corpus", "load_hnsw", "free the old pair"):
            assert word in doc, (fn.__name__, word)
    for fn in (Corpus.vacuum_hnsw, HnswIndex.vacuumed):
        assert "UPDATE is vacuum" in " ".join(fn.__doc__.split()) and "extend_hnsw" in fn.__doc__


def test_remap_hnsw_rows_on_a_hand_made_graph():
    from vsrbac.formats import remap_hnsw_rows
    g = {"m": 2, "entry": 1, "max_level": 1, "level": np.array([0, 1, 0], np.int32),
         "nbr0": np.array([[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]], np.int32), "tid_count": np.array([1, 2, 1], np.int32),
         "tids": np.array([[0] + [-1] * 9, [2, 5] + [-1] * 8, [6] + [-1] * 9], np.int64), "up_slot": np.array([-1, 0, -1], np.int32),
         "up_nbr": np.full((1, 1, 2), -1, np.int32)}
    new_of = np.array([0, -1, 1, -1, -1, 2, 3])                                  # rows 1, 3 and 4 are gone
    out = remap_hnsw_rows(g, new_of)
    np.testing.assert_array_equal(out["tids"][:, :2], [[0, -1], [1, 2], [3, -1]])
    assert (out["tids"][:, 2:] == -1).all() and out["tids"].dtype == np.int64
    assert g["tids"][1, 0] == 2 and out["nbr0"] is g["nbr0"]                    # a new dict, the input untouched
    g["tids"][0, 3] = 1                                                          # past tid_count: padding, ignored
    np.testing.assert_array_equal(remap_hnsw_rows(g, new_of)["tids"], out["tids"])
    with pytest.raises(ValueError, match="row 5"):
        remap_hnsw_rows(g, np.array([0, -1, 1, -1, -1, -1, 3]))
    with pytest.raises(ValueError, match="outside"):
        remap_hnsw_rows(g, new_of[:6])
