"""CPU checks of pgvector's IVFFlat iterative index scan (vsr_ivf_search_iterative): the numpy restatement of the stream
(tests/ivf_iterative_model.py) is pinned to the index oracle's search, its invariants and the fixture's own conditions are
checked, it meets the thresholds of pgvector's TAP tests, and the library exports the new entry points without changing
the ABI version."""
import ctypes
import os
import re

import numpy as np
import pytest

from ivf_iterative_model import ParityFixture, batch_bounds, iterative_search, recall_at, tap_corpus, tap_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(oracle):
    return ParityFixture(oracle)


@pytest.fixture(scope="module")
def tap(oracle):
    return tap_corpus(oracle)


@pytest.mark.parametrize("probes,max_probes", [(1, 1), (3, 1), (5, 5), (64, 7), (100, 32768)])
def test_without_further_lists_the_model_is_the_oracle_search(fx, probes, max_probes):
    for user in (None, 1, 2):
        for i in range(0, 16, 3):
            rows, dist, scanned = iterative_search(fx.oivf, fx.q[i], 10, probes, max_probes, fx.doc, fx.blk, fx.masks[user])
            idx, d = fx.oivf.search(fx.q[i], 10, probes, fx.doc, fx.blk, fx.masks[user])
            np.testing.assert_array_equal(rows, idx)
            np.testing.assert_array_equal(dist, d)
            assert scanned == min(probes, 64)


@pytest.mark.parametrize("probes", [1, 3, 5])
def test_prefix_property_of_the_model(fx, probes):
    for user in (None, 1, 2):
        for i in range(16):
            r100, d100, s100 = fx.model(user, i, 100, probes, 64)
            for k in (1, 10):
                r, d, s = fx.model(user, i, k, probes, 64)
                np.testing.assert_array_equal(r, r100[:k])
                np.testing.assert_array_equal(d, d100[:k])
                assert s <= s100 and s % probes in (0, 64 % probes)


def test_batch_arithmetic_when_probes_do_not_divide_max_probes():
    assert batch_bounds(5, 64, 64) == [(b, min(b + 5, 64)) for b in range(0, 64, 5)]
    assert batch_bounds(5, 64, 64)[-1] == (60, 64)                      # the short last batch: 4 lists
    assert batch_bounds(3, 7, 64) == [(0, 3), (3, 6), (6, 7)]
    assert batch_bounds(5, 1, 64) == [(0, 5)]                           # max_probes below probes: batch 0 only
    assert batch_bounds(100, 32768, 64) == [(0, 64)]
    assert batch_bounds(1, 32768, 3) == [(0, 1), (1, 2), (2, 3)]


def test_the_parity_fixture_exercises_what_it_is_for(fx):
    """The conditions the GPU parity test relies on, about the model itself."""
    assert sorted(set(range(64)) - set(fx.oivf.assign.tolist())) == [60, 61, 62, 63]     # four empty lists
    assert [int(fx.masks[u].sum()) for u in (1, 2, 3)] == [120, 1500, 0]
    for i in range(16):
        # 2 % permitted, probes = 1: batch 0 is short of k = 10, and the relaxed stream is out of global order
        assert len(fx.model(1, i, 10, 1, 1)[0]) < 10
        rows, dist, scanned = fx.model(1, i, 10, 1, 32768)
        assert len(rows) == 10 and scanned > 1 and (np.diff(dist) < 0).any()
        assert 42 <= fx.model(1, i, 100, 1, 64)[2] <= 51
        rows, _, scanned = fx.model(1, i, 100, 1, 20)
        assert scanned == 20 and len(rows) < 100                        # exhausted
        assert fx.model(3, i, 10, 3, 7)[2] == 7 and len(fx.model(3, i, 10, 3, 7)[0]) == 0
        for probes in (3, 5):
            for k in (1, 10, 100):
                assert fx.model(None, i, k, probes, 64)[2] == probes    # unfiltered: nothing continues
    assert any(fx.model(1, i, 100, 5, 64)[2] == 50 for i in range(16))


def test_tap_041_counts(tap):
    """pgvector test/t/041_ivfflat_iterative_scan: 10 of 100 000 rows pass the filter, LIMIT 11, probes = 10."""
    x, oivf = tap
    mask = (np.arange(len(x)) % 10000 == 0).astype(np.uint8)
    for i in range(0, 20, 5):
        assert len(iterative_search(oivf, x[i], 11, 10, 32768, mask=mask)[0]) == 10
    for max_probes in (30, 50, 70):
        mean = np.mean([len(iterative_search(oivf, x[i], 11, 10, max_probes, mask=mask)[0]) for i in range(20)])
        print("max_probes", max_probes, "mean count", mean)
        assert max_probes / 10 - 2 < mean < max_probes / 10 + 2


@pytest.mark.parametrize("c,probes,threshold", [(100, 1, 0.57), (100, 10, 0.98), (1000, 1, 0.80)])
def test_tap_042_recall(oracle, tap, c, probes, threshold):
    """pgvector test/t/042_ivfflat_iterative_scan_recall: recall of the relaxed stream's first 20 against the exact answer."""
    x, oivf = tap
    mask = (np.arange(len(x)) % c == 0).astype(np.uint8)
    rec = []
    for q in tap_queries():
        want, _ = oracle.filtered_topk("l2", x, q, 20, None, None, mask)
        got, _, _ = iterative_search(oivf, q, 20, probes, 32768, mask=mask)
        rec.append(recall_at(got, want))
    print("c", c, "probes", probes, "recall", np.mean(rec))
    assert np.mean(rec) >= threshold


def test_iterative_symbols_declared_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    text = open(os.path.join(ROOT, "include", "vsrbac.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(vsrbac.library_path())
    for name in ("vsr_ivf_search_iterative", "vsr_ivf_search_iterative_device"):
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/vsrbac.h"
        assert len(m.group(1).split(",")) == 16
        assert hasattr(lib, name), name
        assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == 16
    assert re.search(r"VSR_IVF_ITERATIVE_OFF\s*=\s*0\s*,\s*VSR_IVF_ITERATIVE_RELAXED\s*=\s*1", text)
    assert vsrbac.abi_version() == 2
    from vsrbac.engine import IVF_ITERATIVE_MODES, IvfIndex, _ivf_iterative_mode
    assert IVF_ITERATIVE_MODES == {"off": 0, "relaxed_order": 1}
    assert hasattr(IvfIndex, "search_iterative") and hasattr(IvfIndex, "search_iterative_device")
    with pytest.raises(ValueError, match='invalid value for parameter "ivfflat.iterative_scan": "strict_order"'):
        _ivf_iterative_mode("strict_order")
