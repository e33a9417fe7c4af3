"""The serial model of the GPU's batched HNSW build (oracle.HnswIndex.batched, vsr_index_oracle.c: orc_hnsw_build_batched)
pinned to the pgvector-faithful serial build (orc_hnsw_build) before anything is compared with a GPU.

With every batch forced to one element the batched schedule IS the serial one: an element searches the graph as it stands,
its reverse edges are applied at once, the entry point moves after it.  What is left to differ is the duplicate fold, which
the model does not have, so the rows here hold no duplicates; distance ties are left in (small integers), because both builds
order equal distances by (distance, element id)."""
import numpy as np
import pytest

from helpers import check_graph, same_graph, sift_like
from oracle.oracle import HnswIndex as OracleHnsw


def _distinct(x):
    """x without repeated rows, first occurrences in order."""
    _, first = np.unique(x, axis=0, return_index=True)
    return np.ascontiguousarray(x[np.sort(first)])


def _cases():
    rng = np.random.default_rng(5100)
    return {
        "l2-3d-ties": ("l2", _distinct(rng.integers(0, 12, (900, 3)).astype(np.float32)), 16, 64, 3),
        "l2-16d-m4": ("l2", _distinct(sift_like(rng, 800, 16)), 4, 16, 5),
        "ip-10d": ("ip", _distinct(rng.integers(-8, 9, (700, 10)).astype(np.float32)), 8, 32, 7),
        "l2-128d": ("l2", _distinct(sift_like(rng, 400, 128)), 16, 64, 9),
        "jaccard-52": ("jaccard", _distinct(rng.integers(0, 2, (600, 52)).astype(np.float32)), 8, 32, 11),
    }


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_batches_of_one_are_the_serial_build(oracle, name):
    metric, x, m, efc, seed = CASES[name]
    if metric == "jaccard":
        # the serial entry point has no Jaccard of its own: the model is its own serial build there, and what is checked is
        # that a batch limit of 1 and the explicit identity grouping agree, on a well-formed graph
        a = OracleHnsw.batched(oracle, metric, x, m, efc, seed, batch_limit=1)
        b = OracleHnsw.batched(oracle, metric, x, m, efc, seed, elements=[(r,) for r in range(len(x))], batch_limit=1)
        same_graph(a.export(), b.export())
        check_graph(a.export())
        return
    serial = OracleHnsw(oracle, metric, x, m=m, ef_construction=efc, seed=seed)
    assert serial.n_elem == len(x), "the rows hold a duplicate the serial build folded"
    model = OracleHnsw.batched(oracle, metric, x, m, efc, seed, batch_limit=1)
    assert (model.n_elem, model.entry, model.entry_level, model.n_upper) == (serial.n_elem, serial.entry, serial.entry_level, serial.n_upper)
    g = model.export()
    same_graph(g, serial.export())
    check_graph(g)
    rng = np.random.default_rng(1)
    for q in x[rng.integers(0, len(x), 5)] + 1.0:
        for ef in (10, 40):
            a, b = model.search(q, ef), serial.search(q, ef)
            for u, v in zip(a, b):
                np.testing.assert_array_equal(u, v)


def test_the_batched_schedule_differs_from_the_serial_one_and_is_well_formed(oracle):
    """The real schedule (batches of done / 8) on the same rows: same levels and entry, a well-formed graph, and -- so that the
    test above cannot pass because batching does nothing -- different lists."""
    metric, x, m, efc, seed = CASES["l2-16d-m4"]
    serial = OracleHnsw.batched(oracle, metric, x, m, efc, seed, batch_limit=1).export()
    g = OracleHnsw.batched(oracle, metric, x, m, efc, seed).export()
    check_graph(g)
    np.testing.assert_array_equal(g["level"], serial["level"])
    assert g["entry"] == serial["entry"]
    assert (g["nbr0"] != serial["nbr0"]).any()


def test_elements_of_several_rows_keep_their_tids_and_their_first_rows_level(oracle):
    rng = np.random.default_rng(5101)
    x = sift_like(rng, 300, 8)
    x[[40, 90, 200]] = x[10]
    groups = {}
    for r in range(len(x)):
        groups.setdefault(x[r].tobytes(), []).append(r)
    elements = sorted(tuple(rows) for rows in groups.values())
    plain = OracleHnsw.batched(oracle, "l2", x, 8, 32, 3).export()
    g = OracleHnsw.batched(oracle, "l2", x, 8, 32, 3, elements=elements).export()
    check_graph(g)
    assert len(g["level"]) == len(elements) == len(x) - 3
    for e, rows in enumerate(elements):
        assert g["tids"][e, :g["tid_count"][e]].tolist() == list(rows)
        assert g["level"][e] == plain["level"][rows[0]]
