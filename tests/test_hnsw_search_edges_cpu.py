"""The cases of tests/hnsw_search_edge_cases.py under the index oracle alone: the conditions that keep
tests/test_gpu_hnsw_search_edges.py from passing vacuously.  Each of them is a condition on the CASE: when one fails, the case is
changed, never the limit."""
import numpy as np
import pytest

import hnsw_search_edge_cases as ec
from hnsw_iterative_model import Graph, IterativeScan, Stream


def _searches(oracle, name):
    """(k, ef, [rows of every query]) of every pair of the case."""
    c, oh = ec.CASES[name], ec.oracle_index(oracle, name)
    return [(k, ef, [oh.search(q, ef)[0] for q in c.queries]) for k, ef in c.pairs]


@pytest.mark.parametrize("name", list(ec.CASES))
def test_every_sum_of_the_case_is_exact(name):
    c = ec.CASES[name]
    ec.assert_exact(c, name)
    assert c.rows.dtype == np.float32 and c.queries.dtype == np.float32 and len(c.queries) == ec.NQ
    # the fp32 sums in two opposite orders equal the double sum: the bound does what it says
    x, q = c.rows.astype(np.float64), c.queries[0].astype(np.float64)
    terms = (x - q) ** 2 if c.metric == "l2" else x * q
    for order in (slice(None), slice(None, None, -1)):
        acc = np.zeros(len(x), dtype=np.float32)
        for t in terms.T[order]:
            acc = (acc + t.astype(np.float32)).astype(np.float32)
        np.testing.assert_array_equal(acc.astype(np.float64), terms.sum(axis=1))


def test_the_row_lengths_cover_the_chunk_counts():
    chunks = sorted({(c.rows.shape[1] + 3) // 4 for n, c in ec.CASES.items() if n in ec.ROW_LENGTH_CASES})
    assert chunks == [1, 2, 32, 33, 64, 65, 250, 500]             # a lane group of 32 gets 0 or 1, exactly 1, 1 or 2, 2, 2 or 3 chunks
    assert {d % 4 for d in ec.ROW_LENGTH_DIMS} == {0, 1, 2, 3}    # every length of the zero fill
    for dim in ec.ROW_LENGTH_IP_DIMS:
        assert f"rows-ip-{dim}" in ec.CASES
    for dim in ec.ROW_LENGTH_DIMS:
        assert ec.CASES[f"rows-l2-{dim}"].rows.shape == (300 if dim >= 1000 else 600, dim)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_result_counts(oracle, name):
    """n < k: fewer than k rows.  Every other case: k rows for at least 8 of its 9 queries."""
    for k, ef, found in _searches(oracle, name):
        if name in ec.SHORT_CASES and k > ec.SHORT_CASES[name]:
            assert all(0 < len(r) < k for r in found), (name, k, ef, [len(r) for r in found])
            if ef >= ec.SHORT_CASES[name]:                        # the beam holds the whole graph
                assert all(len(r) == ec.SHORT_CASES[name] for r in found)
        else:
            full = sum(len(r) >= k for r in found)
            assert full >= 8, (name, k, ef, [len(r) for r in found])


def test_cosine_queries_reach_both_ends_and_the_clamp(oracle):
    for dim in ec.COSINE_DIMS:
        name = f"cosine-{dim}"
        c, oh = ec.CASES[name], ec.oracle_index(oracle, name)
        first = [oh.search(q, 40)[1][0] for q in c.queries[:4]]   # index distance = -dot of the nearest element
        assert first[0] == -1.0 and first[2] == -2.0, first      # the row itself; twice the row: past the clamp
        last = [oh.search(q, 600)[1][-1] for q in c.queries[:4]]  # ef = n: the farthest element of the graph
        assert last[1] == 1.0 and last[3] == 2.0, last           # the antipode; minus twice the row
        assert ec.reported_distance("cosine", [-1.0, 1.0, -2.0, 2.0]).tolist() == [0.0, 2.0, 0.0, 2.0]


def test_the_m2_graph_is_tall(oracle):
    oh = ec.oracle_index(oracle, "graph-m2")
    assert oh.entry_level >= 4, oh.entry_level
    assert int(oh.export()["level"].max()) == oh.entry_level


def test_the_m100_export_has_full_and_padded_lists(oracle):
    g = ec.oracle_index(oracle, "graph-m100").export()
    assert g["nbr0"].shape[1] == 200
    used = (g["nbr0"] >= 0).sum(axis=1)
    assert (used == 200).any() and (used < 200).any(), (used.min(), used.max())
    for e in np.nonzero(used < 200)[0]:                           # padded with -1 behind the neighbours, never in between
        assert (g["nbr0"][e, used[e]:] == -1).all()


def _group_elements(g, rows_of_group):
    """{element: its TIDs that belong to the group}."""
    out = {}
    for e in range(len(g["level"])):
        t = set(g["tids"][e, :g["tid_count"][e]].tolist()) & set(rows_of_group.tolist())
        if t:
            out[e] = t
    return out


def test_the_duplicate_corpus(oracle):
    c, oh = ec.CASES["graph-duplicates"], ec.oracle_index(oracle, "graph-duplicates")
    g = oh.export()
    groups = ec.duplicate_group_rows()
    assert [len(r) for r in groups] == list(ec.DUP_GROUPS) and len(np.unique(np.concatenate(groups))) == sum(ec.DUP_GROUPS)
    for rr in groups:
        assert (c.rows[rr] == c.rows[rr[0]]).all()
    sizes = [sorted(len(t) for t in _group_elements(g, rr).values()) for rr in groups]
    assert sizes == [[2], [10], [1, 10], [5, 10, 10]], sizes      # an element with exactly 10 TIDs; the 11th copy in another one
    eleven = _group_elements(g, groups[2])
    both = 0
    for k, ef, found in _searches(oracle, "graph-duplicates"):
        for r in found:
            both += all(set(r[:k].tolist()) & t for t in eleven.values())
    assert both >= 1
    # the filtered case: elements with some TIDs permitted and some refused
    mask = ec.duplicate_filter_mask()
    mixed = 0
    for e in range(len(g["level"])):
        allowed = mask[g["tids"][e, :g["tid_count"][e]]]
        mixed += 0 < allowed.sum() < allowed.size
    assert mixed >= len(groups), mixed
    for rr in groups:
        assert 0 < mask[rr].sum() < len(rr)


def test_the_launch_case_covers_every_workgroup_shape():
    c = ec.CASES["launch"]
    assert [ef for _, ef in c.pairs] == list(ec.LAUNCH_EFS)
    assert [ec.queries_per_workgroup(len(c.rows), c.m, ef) for ef in ec.LAUNCH_EFS] == [4, 2, 1]
    # a short last workgroup at 4 and at 2 waves, and a launch of one query
    assert 1 in ec.LAUNCH_NQS and any(n % 4 for n in ec.LAUNCH_NQS) and any(n % 2 and n > 1 for n in ec.LAUNCH_NQS)
    assert max(ec.LAUNCH_NQS) <= ec.NQ


@pytest.mark.parametrize("dim", ec.ITERATIVE_DIMS)
def test_the_iterative_model_agrees_with_the_oracle_on_the_first_round(oracle, dim):
    """mode off of the model is GetScanItems of the oracle: the two references of the GPU test are pinned together on its cases."""
    name = f"rows-l2-{dim}"
    c, oh = ec.CASES[name], ec.oracle_index(oracle, name)
    g = Graph(oh.export(), c.rows)
    for q in c.queries:
        rows_o, dist_o, _, nv = oh.search(q, 40)
        scan = IterativeScan(g, q, 40, "l2", "off")
        rows_m, dist_m, t = Stream(scan).answer(10 ** 6)
        np.testing.assert_array_equal(rows_m, rows_o)
        np.testing.assert_array_equal(dist_m, dist_o)
        assert t == nv
