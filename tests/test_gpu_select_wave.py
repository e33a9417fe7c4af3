"""seed_select_wave_kernel and select_emit_wave_kernel (vsr_kernels.hip): the one-wave-per-query seed and final selection of
int8 (exact_screen) plans, against the oracle and against seed_select_kernel / select_rerank_kernel (VSR_SELECT_WAVE=0).

The selections are exact on unique keys, so a search returns the same bytes whichever pair of kernels ran, and both equal the
oracle's exact filtered top-k (integer-valued rows 0..255: every fp32 sum of vector.c is exact, so ids, order, distances,
counts and padding are compared bit for bit).  No query may be flagged.

One corpus for the whole file, laid out like test_gpu_sample_reg.py's: ~62 000 rows x 128 in documents of at most 100 rows,
dealt in random order over twenty-three permission classes.  The RBAC is a tree as vsrbac.datasets.tree_rbac makes it (a role is
permitted its own documents and its ancestors'; a user holds one role): the root role owns ONE row and child c one row
less than CLASSES[c] says, so the queries of child c's user have exactly that many allowed rows.  A query with at most GQ_CAP
allowed rows runs with an open threshold -- every allowed row is a candidate -- so these are the candidate counts the final
selection sees:
  1 (the root's own user), k - 1, k and k + 1 for every k below, 1023 / 1024 / 1025 (the 64 x 16 chunk of the stream
  select: one chunk short of full, exactly full, one key into a second chunk) and 16 384 = GQ_CAP (a full buffer that did
  not overflow); the last class (40 000 rows) is past GQ_CAP: its queries are seeded from the sample.
The users ask 1, 15, 16, 17, 64 and 65 queries (the widths of the passes over their classes; 65: two passes).

Ties: inside a class every vector occurs one to three times, at scattered rows, so equal distances straddle the k-th place
of most queries (test_ties_straddle_every_k pins that they do for every k); they must come out in row order.

k = 1, 10, 100, 128, 129 and 512: below, at and above a power of two (the sorted list is np2(k) keys long) and GQ_MAX_KP.
The planner takes the wide path while the 2k survivors a bf16 screen would keep fit GQ_MAX_KP, so k = 512 runs on K2 and its
own selection -- the results are checked all the same -- and k = 256 is added as the longest list the wave kernel sorts.
Calls of 1, 3 and all queries.  Geometries as in test_gpu_sample_reg.py: they move the number of sampled entries per seeded
query from below m (no seed) past m to more than 1024 (two chunks of the seed's stream select)."""
import numpy as np
import pytest

from edge_world import World

pytestmark = pytest.mark.gpu

KS = (1, 10, 100, 128, 129, 256, 512)
K_REF = 513                                                            # one more than the largest k: the tie test looks past it
# (allowed rows of the class's queries, queries its user asks); the root comes last and owns the one row everybody sees
CLASSES = ((2, 1), (9, 15), (10, 16), (11, 17), (99, 64), (100, 65), (101, 1), (127, 15), (128, 16), (129, 17), (130, 1),
           (255, 1), (256, 15), (257, 1), (511, 15), (512, 16), (513, 17), (1023, 15), (1024, 16), (1025, 17), (16384, 64), (40001, 65), (1, 1))
GQ_CAP = 16384
GQ_MAX_KP = 512
GEOMETRY = {"default": {}, "fine": {"VSR_MIN_ROWS_PER_BLOCK": "16", "VSR_MIN_SHARED_ROWS": "64"}, "stride3": {"VSR_SAMPLE_STRIDE": "3"}}
WAVE, OLD = "select_emit_wave_kernel", "select_rerank_kernel"


def _ctx(monkeypatch, **env):
    import vsrbac
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = vsrbac.Context(0)
    for k in env:
        monkeypatch.delenv(k)
    return c


@pytest.fixture(scope="module")
def world():
    return World(CLASSES, k_ref=K_REF)


def _calls(w, ki):
    """The query subsets of the three calls at the ki-th k: one query, three, all (the short calls move with k)."""
    s = (37 * ki + 5) % (w.nq - 3)
    return [np.arange(s, s + 1), np.arange(s + 1, s + 4), np.arange(w.nq)]


def _check(oracle, w, res, sel, k):
    for j, i in enumerate(sel):
        idx, dist = w.ref(oracle, i)
        idx, dist = idx[:k], dist[:k]
        m = int(res.counts[j])
        assert m == idx.size, (k, int(i), int(w.quser[i]), m, idx.size)
        np.testing.assert_array_equal(res.rows[j, :m], idx)
        np.testing.assert_array_equal(res.dist[j, :m], dist.astype(np.float32))
        np.testing.assert_array_equal(res.block_ids[j, :m], w.blk[idx])
        np.testing.assert_array_equal(res.doc_ids[j, :m], w.doc[idx])
        assert (res.rows[j, m:] == -1).all() and (res.block_ids[j, m:] == -1).all() and (res.doc_ids[j, m:] == -1).all()
        assert np.isposinf(res.dist[j, m:]).all()


def _same(a, b):
    for f in ("counts", "rows", "dist", "block_ids", "doc_ids"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def _search(monkeypatch, w, env, ks=KS):
    """{(k, call): (result, kernel name)} on a fresh context opened under `env`; no query may be flagged."""
    import vsrbac
    ctx = _ctx(monkeypatch, VSR_FORCE_EPI="1", **env)
    corpus = ctx.load_corpus(w.x, w.blk, w.doc)
    corpus.load_rbac(*w.rbac())
    filters = [corpus.filter_for_user(int(u), vsrbac.RANGES) for u in w.quser]
    out = {}
    for ki, k in enumerate(ks):
        for c, sel in enumerate(_calls(w, ki)):
            res = corpus.search(w.q[sel], k, "l2", [filters[i] for i in sel])
            assert (res.counts >= 0).all()
            out[(k, c)] = (res, ctx.last_scan_kernel())
    assert ctx.screening_check(0)[0] == 0
    corpus.free()
    ctx.close()
    return out


def test_candidate_counts_sit_on_the_edges(oracle, world):
    w = world
    for c, (allowed, _) in enumerate(CLASSES):
        assert w.allowed_rows(oracle, w.role_of_class[c]).size == allowed
    edges = {a for a, _ in CLASSES}
    assert {1, 1023, 1024, 1025, GQ_CAP} <= edges and max(edges) > GQ_CAP
    assert all({k - 1, k, k + 1} - {0} <= edges for k in KS)


def test_ties_straddle_every_k(oracle, world):
    """For every k some query's k-th and (k + 1)-th distances are equal, and their rows ascend: the oracle's tie rule."""
    w = world
    for k in KS:
        hit = 0
        for i in range(w.nq):
            idx, dist = w.ref(oracle, i)
            if idx.size > k and dist[k - 1] == dist[k]:
                assert idx[k - 1] < idx[k]
                hit += 1
        assert hit >= 3, (k, hit)


@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_wave_selection_matches_oracle_and_old_kernels(oracle, monkeypatch, world, geometry):
    w = world
    new = _search(monkeypatch, w, {"VSR_SELECT_WAVE": "1", **GEOMETRY[geometry]})
    old = _search(monkeypatch, w, {"VSR_SELECT_WAVE": "0", **GEOMETRY[geometry]})
    for ki, k in enumerate(KS):
        for c, sel in enumerate(_calls(w, ki)):
            (res, name), (res0, name0) = new[(k, c)], old[(k, c)]
            print(f"{geometry} k={k} call of {sel.size}: {name}")
            if sel.size == w.nq and 2 * k <= GQ_MAX_KP:                # the whole batch takes the wide int8 path
                assert "int8" in name and WAVE in name and OLD not in name, name
                assert "int8" in name0 and OLD in name0 and WAVE not in name0, name0
            _check(oracle, w, res, sel, k)
            _check(oracle, w, res0, sel, k)
            _same(res, res0)


def test_default_is_the_wave_selection(monkeypatch, world):
    out = _search(monkeypatch, world, {}, ks=(10,))
    assert WAVE in out[(10, 2)][1], out[(10, 2)][1]


def test_bf16_planes_keep_select_rerank(oracle, monkeypatch):
    """A d = 96 corpus without int8 planes (one element is -1: not 0..255, still an exact bf16 value): the plan screens on the
    bf16 planes and re-ranks, on select_rerank_kernel's four waves, whatever VSR_SELECT_WAVE says."""
    w = World(((2048, 64), (4001, 65), (1, 1)), d=96, seed=7)
    w.x[0, 0] = -1.0
    new = _search(monkeypatch, w, {"VSR_SELECT_WAVE": "1"}, ks=(10,))
    old = _search(monkeypatch, w, {"VSR_SELECT_WAVE": "0"}, ks=(10,))
    for c, sel in enumerate(_calls(w, 0)):
        (res, name), (res0, name0) = new[(10, c)], old[(10, c)]
        if sel.size == w.nq:
            assert "int8" not in name and OLD in name and WAVE not in name, name
        assert name == name0
        _check(oracle, w, res, sel, 10)
        _same(res, res0)
