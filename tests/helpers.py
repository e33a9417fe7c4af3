"""Shared checkers for the parity tests."""
import numpy as np


def sift_like(rng, n, d=128):
    """SIFT-like rows: integer-valued fp32 in [0,255] — fp32 sums are exact."""
    return np.clip(np.rint(np.abs(rng.normal(0, 45, (n, d)))), 0, 255).astype(np.float32)


def assert_valid_topk(ids, dist, ref_all, k, tol, candidates=None):
    """`ids`/`dist` is a valid top-k of the reference distance vector `ref_all` within `tol`:
    values right for the returned ids, sorted, and nothing better left out.
    Used for real-valued data where the reference itself is summation-order ambiguous
    (pgvector builds with -fassociative-math); integer-valued data is
    compared bit-exact instead."""
    ids = np.asarray(ids)
    dist = np.asarray(dist, dtype=np.float64)
    ref_all = np.asarray(ref_all, dtype=np.float64)
    cand = np.arange(ref_all.size) if candidates is None else np.asarray(candidates)
    want = min(k, cand.size)
    assert ids.size == want, (ids.size, want)
    if want == 0:
        return
    assert len(set(ids.tolist())) == ids.size, "duplicate ids"
    assert np.isin(ids, cand).all(), "returned a filtered-out row"
    r = ref_all[ids]
    scale = np.maximum(1.0, np.abs(r))
    ok = (np.abs(dist - r) <= tol * scale) | (np.isnan(dist) & np.isnan(r))
    assert ok.all(), (dist[~ok], r[~ok])
    rr = np.where(np.isnan(r), np.inf, r)
    fin = np.where(np.isnan(scale), 1.0, scale)         # (NaN rows rank as +inf; several may follow one another: inf - inf)
    assert (rr[1:] >= rr[:-1] - tol * fin[1:]).all(), "not sorted"
    rest = np.setdiff1d(cand, ids)
    if rest.size:
        rest_d = np.where(np.isnan(ref_all[rest]), np.inf, ref_all[rest])
        worst = rr.max()
        if np.isfinite(worst):
            assert rest_d.min() >= worst - tol * max(1.0, abs(worst)), (rest_d.min(), worst)


# ---- exported HNSW graphs (HnswIndex.export of the GPU package and of the index oracle) ----
def check_lists(lists, owner, n_elem):
    """lists [rows][width] of neighbour ids owned by owner[rows]: in range, -1 only as trailing padding, no self-loop, no
    repeated id."""
    assert lists.min(initial=-1) >= -1 and lists.max(initial=-1) < n_elem
    valid = lists >= 0
    assert (valid[:, 1:] <= valid[:, :-1]).all(), "-1 before a neighbour"
    assert not (lists == owner[:, None]).any(), "self-loop"
    s = np.sort(lists, axis=1)
    assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any(), "an id twice in one list"


def check_graph(g):
    """An exported HNSW graph (HnswIndex.export) is well formed: every list passes check_lists, upper slots are a permutation,
    no list above its owner's level, the entry is an element of the highest level."""
    level, up_slot, up_nbr = g["level"], g["up_slot"], g["up_nbr"]
    ne = len(level)
    check_lists(g["nbr0"], np.arange(ne), ne)
    assert ((up_slot >= 0) == (level >= 1)).all()
    upper = np.flatnonzero(up_slot >= 0)
    assert sorted(up_slot[upper].tolist()) == list(range(len(upper)))
    for lc in range(1, g["max_level"] + 1):
        lists = up_nbr[up_slot[upper], lc - 1]
        assert (lists[level[upper] < lc] == -1).all(), "an upper list above the element's level"
        check_lists(lists, upper, ne)
    assert level.max() <= g["max_level"]
    assert level[g["entry"]] == level.max()


def check_built_graph(g, m):
    """What holds exactly for every graph an insertion build leaves, whatever its rows: check_graph; lists of 2m / m entries at
    most; a neighbour on layer lc lives on layer lc; every element but the first found somebody on layer 0 (an element's own
    list never shrinks); the entry point is the first element of the highest level (a later element of the same level does
    not replace it)."""
    check_graph(g)
    level, nbr0, up_slot, up_nbr = g["level"], g["nbr0"], g["up_slot"], g["up_nbr"]
    assert g["m"] == m and nbr0.shape == (len(level), 2 * m) and up_nbr.shape[1:] == (g["max_level"], m)
    assert ((nbr0 >= 0).sum(axis=1) <= 2 * m).all() and ((up_nbr >= 0).sum(axis=2) <= m).all()
    upper = np.flatnonzero(up_slot >= 0)
    for lc in range(1, g["max_level"] + 1):
        lists = up_nbr[up_slot[upper], lc - 1]
        assert (level[lists[lists >= 0]] >= lc).all(), f"a neighbour on layer {lc} that does not live there"
    assert (nbr0[1:, 0] >= 0).all(), "an element without a layer-0 neighbour"
    assert g["entry"] == int(np.argmax(level)), "the entry point is not the first element of the highest level"


def same_graph(a, b):
    """Two exported HNSW graphs are equal key for key, array for array (dtype, shape, values)."""
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        else:
            assert a[key] == b[key], key
