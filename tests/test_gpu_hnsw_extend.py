"""vsr_hnsw_extend (Corpus.extend_hnsw): rows inserted into an HNSW graph that exists, by the batched build's own loop.

The build's schedule max(1, min(done / 8, 4096, left)) depends on `done` alone, so a prefix build that ends at one of the full
build's batch boundaries, extended over all rows with the build's seed, must BE the full build's graph, and the model's
(oracle.HnswIndex.batched), array for array: what the extension adds -- starting the loop from uploaded arrays, the skipped level
draws, the recomputed per-edge distances, re-strided upper arrays, the element -> row map -- either reproduces the build's state
or moves an edge.  Rows are small integers as in tests/test_gpu_hnsw_build_model.py, so every distance is exact.  The schedule
and the level stream are restated in tests/hnsw_extend_model.py and pinned by tests/test_hnsw_extend_cpu.py.

A view corpus (the build's refusal, taken before the graph is looked at) is not covered: no public call hands one out."""
import numpy as np
import pytest

from helpers import check_built_graph, same_graph, sift_like
from hnsw_extend_model import boundaries, boundary_near, empty_graph, level_stream, schedule
from hnsw_half_model import to_half
from test_gpu_hnsw_build_model import _exact, _model, _small_ints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _corpus(ctx, kind, x, doc=None):
    if kind == "f32":
        return ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32), None, doc)
    if kind == "half":
        return ctx.load_corpus_half(to_half(x), None, doc)
    return ctx.load_corpus_bit(np.asarray(x) != 0, None, None, doc)


def _build_on(corpus, kind, m, efc, metric, seed, merge=False):
    fn = {"f32": corpus.build_hnsw, "half": corpus.build_hnsw_half, "bit": corpus.build_hnsw_bit}[kind]
    return fn(m, efc, metric, seed=seed, merge_duplicates=merge)


def _built(ctx, kind, x, m, efc, metric, seed, merge=False):
    corpus = _corpus(ctx, kind, x)
    gpu = _build_on(corpus, kind, m, efc, metric, seed, merge)
    ctx.screening_check(0)
    g = gpu.export()
    gpu.free()
    corpus.free()
    return g


def _extended(ctx, kind, x, graph, efc, metric, seed, doc=None):
    corpus = _corpus(ctx, kind, x, doc)
    gpu = corpus.extend_hnsw(graph, efc, metric, seed)
    total, _ = ctx.screening_check(0)
    g = gpu.export()
    gpu.free()
    corpus.free()
    return g


def _rows(kind, n, seed, bits=52):
    """f32: 16-d, -8 .. 8 (exact for L2 and inner product); half: 24-d; bit: 52 bits unless given."""
    if kind == "f32":
        return _exact(_small_ints(seed, n, 16, -8, 8))
    if kind == "half":
        return _exact(_small_ints(seed, n, 24, -8, 8))
    return _small_ints(seed, n, bits, 0, 1)


def _invariants(g, m, n_rows, n0_rows, n0_elem, seed):
    """What holds for every extended graph whatever the schedule: the structure the kernels rely on, and the identity of the new
    elements (levels from draws n0_rows ..., one TID each, every caller row under exactly one TID)."""
    level, nbr0, up_slot, up_nbr = g["level"], g["nbr0"], g["up_slot"], g["up_nbr"]
    ne = len(level)
    assert nbr0.shape == (ne, 2 * m) and up_nbr.shape[1:] == (g["max_level"], m)          # degree <= 2m / m by shape
    for lists in (nbr0, up_nbr.reshape(-1, m)):
        assert ((lists >= -1) & (lists < ne)).all()
        assert ((lists[:, 1:] < 0) | (lists[:, :-1] >= 0)).all(), "a list is not packed"
    assert ((up_slot >= 0) == (level >= 1)).all()
    slots = up_slot[up_slot >= 0]
    assert len(np.unique(slots)) == len(slots) and (slots < up_nbr.shape[0]).all()
    for e in np.flatnonzero(level >= 1):
        for lc in range(1, g["max_level"] + 1):
            ids = up_nbr[up_slot[e], lc - 1]
            ids = ids[ids >= 0]
            assert (level[ids] >= lc).all() and (lc <= level[e] or ids.size == 0)
    assert level[g["entry"]] == level.max() and g["max_level"] == max(level.max(), 1)
    new = np.arange(n0_elem, ne)
    np.testing.assert_array_equal(level[new], np.array(level_stream(seed, m, n_rows)[n0_rows:], dtype=np.int32))
    assert (g["tid_count"][new] == 1).all()
    named = np.concatenate([g["tids"][e, :g["tid_count"][e]] for e in range(ne)])
    np.testing.assert_array_equal(np.sort(named), np.arange(n_rows))
    assert (g["tids"][np.arange(10)[None, :] >= g["tid_count"][:, None]] == -1).all()


# ---- 1: extension from nothing is the build -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "ip"), ("half", "l2"), ("bit", "hamming"), ("bit", "jaccard")])
def test_extension_from_nothing_is_the_build(ctx, oracle, kind, metric):
    x = _rows(kind, 600, 7200)
    m, efc, seed = 8, 32, 31
    got = _extended(ctx, kind, x, empty_graph(m), efc, metric, seed)
    same_graph(got, _built(ctx, kind, x, m, efc, metric, seed))
    same_graph(got, _model(oracle, kind, x, m, efc, metric, seed).export())


# ---- 2: extension at a batch boundary is the build -----------------------------------------------------------------------------------
N2 = 3000


def _schedule_restated(start, n):
    out, done = [], start
    while done < n:
        out.append(done)
        done += max(1, min(done // 8, 4096, n - done))
    return out + [n]


def _boundary_case(ctx, oracle, kind, x, m, efc, metric, seed):
    """build(rows[:n0]) extended over all rows, for n0 near n / 3 and near 0.9 n, and the chain over both: each is the one-shot
    build and the model.  Returns (prefix, extended) for the first boundary."""
    n = len(x)
    assert _schedule_restated(0, n) == boundaries(0, n)
    n0, n1 = boundary_near(n, n // 3), boundary_near(n, 9 * n // 10)
    assert 0 < n0 < n1 < n and n0 in _schedule_restated(0, n) and n1 in _schedule_restated(0, n)
    full = _built(ctx, kind, x, m, efc, metric, seed)
    same_graph(full, _model(oracle, kind, x, m, efc, metric, seed).export())
    first = _built(ctx, kind, x[:n0], m, efc, metric, seed)
    ext = _extended(ctx, kind, x, first, efc, metric, seed)
    same_graph(ext, full)
    same_graph(_extended(ctx, kind, x, _built(ctx, kind, x[:n1], m, efc, metric, seed), efc, metric, seed), full)
    mid = _extended(ctx, kind, x[:n1], first, efc, metric, seed)
    same_graph(mid, _built(ctx, kind, x[:n1], m, efc, metric, seed))
    same_graph(_extended(ctx, kind, x, mid, efc, metric, seed), full)
    return first, ext, n0


@pytest.mark.parametrize("kind,metric,m,efc", [("f32", "l2", 8, 32), ("half", "l2", 8, 32), ("bit", "hamming", 16, 64)])
def test_extension_at_a_batch_boundary_is_the_build(ctx, oracle, kind, metric, m, efc):
    """bit: 136 bits (one full 16-byte chunk and a partial one) at the m and ef_construction at which
    tests/test_gpu_hnsw_build_model.py pins the bit build to the model.  On 3000 52-bit rows with m = 8, ef_construction = 32 the
    one-shot BUILD already leaves the model (30 of 48 000 layer-0 entries, before any extension): Hamming distances over 52 bits
    take few values, the case DESIGN.md 7 (9) lists -- the bounded candidate array of the fp32, bit and half builds drops
    candidates of equal distance where the model's heap keeps them."""
    _boundary_case(ctx, oracle, kind, _rows(kind, N2, 7300, bits=136), m, efc, metric, seed=32)


def _seed_with_a_new_top(m, n, n0):
    """The first seed whose stream puts a row past n0 above every row before it (a restated stream: the test asserts the
    consequences from the exported arrays)."""
    for seed in range(1, 500):
        lv = level_stream(seed, m, n)
        if max(lv[n0:]) > max(lv[:n0]):
            return seed
    raise AssertionError("no such seed")


def test_extension_raises_max_level_and_moves_the_entry_point(ctx, oracle):
    """m = 4, ef_construction = 16: a new element above the prior top, so the upper arrays are re-strided and the entry moves."""
    x = _exact(sift_like(np.random.default_rng(7301), N2, 16))
    n0 = boundary_near(N2, N2 // 3)
    seed = _seed_with_a_new_top(4, N2, n0)
    first, ext, n0 = _boundary_case(ctx, oracle, "f32", x, 4, 16, "l2", seed)
    assert ext["max_level"] > first["max_level"], "max_level did not grow: the upper arrays were not re-strided"
    assert ext["up_nbr"].shape[1] > first["up_nbr"].shape[1]
    assert ext["entry"] != first["entry"] and ext["entry"] >= n0, "the entry point did not move to a new element"
    assert ext["level"][n0:].max() > ext["level"][:n0].max()


# ---- 3: batches of HB_BATCH_MAX -------------------------------------------------------------------------------------------------------
def test_extension_by_batches_of_batch_max(ctx):
    """41 500 distinct 4-d rows (chosen as test_batches_of_batch_max chooses its own), m = 4, ef_construction = 16; the prefix ends
    at the schedule's boundary 35 655, the first from which a batch of 4096 starts: that batch and a short one.  (36 864 =
    32 768 + 4096 is no boundary of the schedule, which passes 32 768 inside the batch 31 694 .. 35 655; an extension from there
    is another schedule and need not be the one-shot build.)"""
    rng = np.random.default_rng(6600)
    cells = rng.permutation(24 ** 4)[:41_500]
    x = _exact(np.stack([(cells // 24 ** i) % 24 for i in range(4)], axis=1).astype(np.float32))
    assert len(np.unique(x, axis=0)) == 41_500
    assert schedule(35_655, 41_500) == [(35_655, 4096), (39_751, 1749)] and 35_655 in boundaries(0, 41_500)
    full = _built(ctx, "f32", x, 4, 16, "l2", 28)
    ext = _extended(ctx, "f32", x, _built(ctx, "f32", x[:35_655], 4, 16, "l2", 28), 16, "l2", 28)
    same_graph(ext, full)


# ---- 4: off a boundary ------------------------------------------------------------------------------------------------------------------
def test_extension_off_a_boundary_is_deterministic_composes_and_is_well_formed(ctx):
    n0, n, m, efc, seed = 1000, 2500, 8, 32, 33
    assert n0 not in boundaries(0, n)
    x = _rows("f32", n, 7400)
    mid = boundary_near(n, 1777, start=n0)
    assert mid in boundaries(n0, n) and n0 < mid < n
    first = _built(ctx, "f32", x[:n0], m, efc, "l2", seed)
    a = _extended(ctx, "f32", x, first, efc, "l2", seed)
    same_graph(_extended(ctx, "f32", x, first, efc, "l2", seed), a)
    step = _extended(ctx, "f32", x[:mid], first, efc, "l2", seed)
    same_graph(_extended(ctx, "f32", x, step, efc, "l2", seed), a)
    for key in ("level", "tid_count", "tids", "up_slot"):
        np.testing.assert_array_equal(a[key][:n0], first[key], err_msg=key)
    _invariants(a, m, n, n0, n0, seed)
    check_built_graph(a, m)


# ---- 5: new rows that sort between old ones ---------------------------------------------------------------------------------------------
def test_interleaved_rows_take_the_element_to_row_map(ctx):
    n0, n, m, efc, seed = 900, 1500, 8, 32, 34
    x = _rows("f32", n, 7500)
    assert len(np.unique(x, axis=0)) == n
    doc = np.zeros(n, dtype=np.int32)
    doc[:n0] = 10 * (np.arange(n0) + 1)
    between = np.arange(n0, n)[::3]                                             # a third of the new rows go between old ones
    doc[between] = 10 * (np.random.default_rng(7501).permutation(n0 - 1)[:len(between)] + 1) + 5
    rest = np.setdiff1d(np.arange(n0, n), between)
    doc[rest] = 10 * (n0 + 1) + np.arange(len(rest))
    assert len(np.unique(doc)) == n
    perm = np.argsort(doc, kind="stable")                                       # internal row r of A holds caller row perm[r]
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    first = _built(ctx, "f32", x[:n0], m, efc, "l2", seed)
    first_b = dict(first, tids=np.where(first["tids"] >= 0, inv[np.maximum(first["tids"], 0)], -1))
    corpus_a = _corpus(ctx, "f32", x, doc)
    index_a = corpus_a.extend_hnsw(first, efc, "l2", seed)
    a = index_a.export()
    b = _extended(ctx, "f32", x[perm], first_b, efc, "l2", seed)
    same_graph(dict(a, tids=np.where(a["tids"] >= 0, inv[np.maximum(a["tids"], 0)], -1)), b)
    new_rows = a["tids"][n0:, 0]
    np.testing.assert_array_equal(new_rows, np.arange(n0, n)[np.argsort(doc[n0:], kind="stable")])
    _invariants(a, m, n, n0, n0, seed)
    pick = np.concatenate([between[:20], rest[:15], np.arange(0, n0, 60)[:15]])
    res, _ = index_a.search(x[pick], 1, 40, "l2")
    np.testing.assert_array_equal(res.rows[:, 0], pick)
    assert (res.dist[:, 0] == 0).all() and (res.counts == 1).all()
    index_a.free()
    corpus_a.free()


# ---- 6: a merged prior graph ------------------------------------------------------------------------------------------------------------
def test_merged_prior_graph_is_extended(ctx):
    m, efc, seed = 8, 32, 35
    x = _rows("f32", 1200, 7600)
    assert len(np.unique(x, axis=0)) == 1200
    groups = [np.array([5, 300]), np.arange(20, 30), np.arange(400, 411)]      # 2, 10 and 11 identical rows
    for g in groups:
        x[g] = x[g[0]]
    first = _built(ctx, "f32", x[:800], m, efc, "l2", seed, merge=True)
    ne0 = len(first["level"])
    assert ne0 == 800 - 1 - 9 - 9 and sorted(first["tid_count"][first["tid_count"] > 1].tolist()) == [2, 10, 10]
    corpus = _corpus(ctx, "f32", x)
    gpu = corpus.extend_hnsw(first, efc, "l2", seed)
    ctx.screening_check(0)
    g = gpu.export()
    assert len(g["level"]) == ne0 + 400 and gpu.info()[0] == ne0 + 400
    for key in ("level", "tid_count", "tids", "up_slot"):
        np.testing.assert_array_equal(g[key][:ne0], first[key], err_msg=key)
    _invariants(g, m, 1200, 800, ne0, seed)
    res, _ = gpu.search(x[groups[1][:1]], 10, 40, "l2")
    assert res.counts[0] == 10 and sorted(res.rows[0].tolist()) == groups[1].tolist() and (res.dist[0] == 0).all()
    gpu.free()
    corpus.free()


# ---- 7: round trip and search surface -----------------------------------------------------------------------------------------------------
def _same_result(a, b):
    for u, v in zip(a[0], b[0]):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(a[1], b[1])


def test_extended_index_and_its_reloaded_export_answer_alike(ctx):
    n0, n, m, efc, seed = 1000, 2000, 8, 32, 36
    x = _rows("f32", n, 7700)
    rng = np.random.default_rng(7701)
    q = x[rng.integers(0, n, 12)] + rng.integers(-2, 3, (12, 16)).astype(np.float32)
    corpus = _corpus(ctx, "f32", x)
    ext = corpus.extend_hnsw(_built(ctx, "f32", x[:n0], m, efc, "l2", seed), efc, "l2", seed)
    again = corpus.load_hnsw(ext.export())
    assert ext.device_bytes() == again.device_bytes() and ext.info() == again.info()
    flt = corpus.filter_from_bytemask((rng.random(n) < 0.3).astype(np.uint8))
    for ef in (10, 40, 200):
        for filters in (None, [flt] * 12):
            _same_result(ext.search(q, 10, ef, "l2", filters), again.search(q, 10, ef, "l2", filters))
            for mode in ("relaxed_order", "strict_order"):
                _same_result(ext.search_iterative(q, 10, ef, "l2", filters, mode), again.search_iterative(q, 10, ef, "l2", filters, mode))
        for h in (ext, again):
            h.set_predicate_aware(True)
        _same_result(ext.search(q, 10, ef, "l2", [flt] * 12), again.search(q, 10, ef, "l2", [flt] * 12))
        for h in (ext, again):
            h.set_predicate_aware(False)
    ctx.screening_check(0)
    for h in (again, ext):
        h.free()
    corpus.free()


def test_extended_bit_index_and_its_reloaded_export_answer_alike(ctx):
    n0, n, m, efc, seed = 1000, 2000, 8, 32, 37
    x = _rows("bit", n, 7800)
    q = x[np.random.default_rng(7801).integers(0, n, 12)] != 0
    q[:, :3] ^= True
    corpus = _corpus(ctx, "bit", x)
    ext = corpus.extend_hnsw(_built(ctx, "bit", x[:n0], m, efc, "jaccard", seed), efc, "jaccard", seed)
    again = corpus.load_hnsw_bit(ext.export(), "jaccard")
    for ef in (10, 40, 200):
        _same_result(ext.search_bit(q, 10, ef, "jaccard"), again.search_bit(q, 10, ef, "jaccard"))
    with pytest.raises(Exception):
        ext.search_bit(q, 10, 40, "hamming")                                   # the extension's metric is the index's opclass
    for h in (again, ext):
        h.free()
    corpus.free()


# ---- 8: pgvector's insert floors (test/t/013_hnsw_vector_insert_recall.pl; 025 for halfvec) ----------------------------------------------
def _tie_aware_recall(metric, x, q, found, exact_rows, k):
    """A found row counts when it is as near as the exact scan's k-th row (float64 distances of the fp32 values)."""
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    hit = total = 0
    for i in range(len(q)):
        if metric == "l2":
            d = ((x64 - q64[i]) ** 2).sum(axis=1)
        elif metric == "ip":
            d = -(x64 @ q64[i])
        else:
            d = 1.0 - (x64 @ q64[i]) / (np.linalg.norm(x64, axis=1) * np.linalg.norm(q64[i]))
        kth = d[exact_rows[i][:k]].max()
        hit += int((d[found[i]] <= kth).sum())
        total += k
    return hit / total


@pytest.mark.parametrize("kind,metric,floor", [("f32", "l2", 0.99), ("f32", "ip", 0.97), ("f32", "cosine", 0.99), ("half", "l2", 0.99)])
def test_insert_recall_floors_of_pgvector(ctx, kind, metric, floor):
    """10 000 3-d rows of random() * random(), 20 uniform queries, LIMIT 20, ef_search 40, m = 16, ef_construction = 64; the
    graph grown 1000 -> 2500 -> 10 000.  Exact reference: the corpus's own exact scan.  The one-shot build on the same rows is
    held to the same floor, so the reference stands on its own."""
    rng = np.random.default_rng(1301)
    n, k, seed = 10_000, 20, 3
    x = (rng.random((n, 3)) * rng.random((n, 3))).astype(np.float32)
    q = rng.random((20, 3)).astype(np.float32)
    if metric == "cosine":
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    if kind == "half":
        x = to_half(x).astype(np.float32)
    g = _built(ctx, kind, x[:1000], 16, 64, metric, seed)
    g = _extended(ctx, kind, x[:2500], g, 64, metric, seed)
    corpus = _corpus(ctx, kind, x)
    exact = corpus.search(q, k, metric).rows
    recall = {}
    for name, index in (("extended", corpus.extend_hnsw(g, 64, metric, seed)), ("built", _build_on(corpus, kind, 16, 64, metric, seed))):
        assert index.info()[0] == n
        got, _ = index.search(q, k, 40, metric)
        recall[name] = _tie_aware_recall(metric, x, q, [got.rows[i][:got.counts[i]] for i in range(len(q))], exact, k)
        index.free()
    corpus.free()
    print(f"hnsw insert {kind} {metric}: recall@20 extended {recall['extended']:.4f}, one-shot build {recall['built']:.4f}")
    assert recall["built"] >= floor, recall
    assert recall["extended"] >= floor, recall


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    """A 300-row prefix graph (m = 4: several layers) and the 400 rows it is extended over."""
    x = _rows("f32", 400, 7900)
    return x, _built(ctx, "f32", x[:300], 4, 16, "l2", 38)


def _raises(status, fragment, fn, *args, **kw):
    import vsrbac
    with pytest.raises(vsrbac.VsrError, match=fragment) as info:
        fn(*args, **kw)
    assert info.value.status == status, (info.value.status, status)


def _raw_extend(corpus, g, efc=16, metric=0, seed=1, flags=0, m=None):
    import ctypes as C
    from vsrbac.engine import _ptr, check
    a = lambda name, dt: np.ascontiguousarray(g[name], dtype=dt)
    arrays = [a("level", np.int32), a("nbr0", np.int32), a("tid_count", np.int32), a("tids", np.int64), a("up_slot", np.int32),
              a("up_nbr", np.int32)]
    h = C.c_void_p()
    check(corpus._lib.vsr_hnsw_extend(corpus._h, int(g["m"] if m is None else m), arrays[0].size, int(g["entry"]), *[_ptr(v) for v in arrays],
                                      int((arrays[4] >= 0).sum()), int(g["max_level"]), efc, metric, seed, flags, C.byref(h)))
    return h


def test_refused_corpora_flags_and_parameters(ctx, small):
    from vsrbac import _ffi
    x, g = small
    rng = np.random.default_rng(7901)
    dense = np.where(rng.random((50, 40)) < 0.2, rng.integers(1, 5, (50, 40)), 0).astype(np.float32)
    dense[:, 0] = 1
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    sparse = ctx.load_corpus_sparse(indptr, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32), 40)
    _raises(_ffi.ERR_UNSUPPORTED, "sparsevec", sparse.extend_hnsw, empty_graph(4), 16, "l2")
    sparse.free()
    corpus = _corpus(ctx, "f32", x)
    _raises(_ffi.ERR_UNSUPPORTED, "VSR_HNSW_BUILD_MERGE_DUPLICATES", _raw_extend, corpus, g, flags=1)
    _raises(_ffi.ERR_INVALID, "unknown flag bits", _raw_extend, corpus, g, flags=2)
    _raises(_ffi.ERR_UNSUPPORTED, "m must be between 2 and 100", _raw_extend, corpus, g, m=101, efc=400)
    _raises(_ffi.ERR_UNSUPPORTED, "ef_construction must be between 4 and 1000 and at least 2 \\* m", corpus.extend_hnsw, g, 7)
    _raises(_ffi.ERR_UNSUPPORTED, "ef_construction must be between", corpus.extend_hnsw, g, 1001)
    _raises(_ffi.ERR_UNSUPPORTED, "L2, inner product and cosine operator classes only", corpus.extend_hnsw, g, 16, "hamming")
    corpus.free()
    bits = _corpus(ctx, "bit", _rows("bit", 100, 7902))
    _raises(_ffi.ERR_INVALID, "not an operator class of bit", bits.extend_hnsw, empty_graph(4), 16, "l2")
    bits.extend_hnsw(empty_graph(4), 16).free()                                # the default metric of a bit corpus is its Hamming opclass
    bits.free()


def _damaged(g, rule):
    """One hand-damaged copy of g per validation rule -> (graph, message fragment)."""
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    level, nbr0, up_slot, up_nbr = g["level"], g["nbr0"], g["up_slot"], g["up_nbr"]
    ne = len(level)
    low = int(np.flatnonzero(level == 0)[0])
    high = np.flatnonzero(level >= 1)
    if rule == "tid_count":
        g["tid_count"][7] = 11
        return g, "element 7 has 11 heap TIDs"
    if rule == "level":
        level[7] = g["max_level"] + 1
        return g, "element 7 has 1 heap TIDs / level"
    if rule == "tid_row":
        g["tids"][7, 0] = 400
        return g, "element 7 points at row 400"
    if rule == "id_high":
        nbr0[9, 0] = ne
        return g, f"element 9 lists neighbour {ne} on layer 0"
    if rule == "id_low":
        nbr0[9, 0] = -2
        return g, "element 9 lists neighbour -2 on layer 0"
    if rule == "upper_id":
        up_nbr[up_slot[high[0]], 0, 0] = ne + 5
        return g, f"element {high[0]} lists neighbour {ne + 5} on layer 1"
    if rule == "packed":
        assert nbr0[9, 1] >= 0
        nbr0[9, 0] = -1
        return g, "element 9: the layer 0 list is not packed"
    if rule == "neighbour_level":
        up_nbr[up_slot[high[0]], 0, 0] = low
        return g, f"element {high[0]} lists neighbour {low} on layer 1, above that element's level 0"
    if rule == "slot_range":
        up_slot[high[0]] = len(high)
        return g, f"element {high[0]} of level {level[high[0]]} has upper slot {len(high)}"
    if rule == "slot_missing":
        up_slot[high[1]] = -1                                                   # (n_upper is counted from up_slot: one fewer)
        return g, f"element {high[1]} of level {level[high[1]]} has upper slot -1"
    if rule == "slot_shared":
        up_slot[high[1]] = up_slot[high[0]]
        return g, f"element {high[1]} shares upper slot {up_slot[high[0]]} with element {high[0]}"
    if rule == "slot_on_level_0":
        up_slot[low] = 0
        return g, f"element {low} of level 0 has upper slot 0"
    if rule == "entry":
        g["entry"] = low
        return g, f"entry element {low} has level 0, below the highest level"
    if rule == "row_twice":
        g["tids"][8, 0] = g["tids"][3, 0]
        return g, "element 8 names row 3, which another heap TID names already"
    raise AssertionError(rule)


@pytest.mark.parametrize("rule", ["tid_count", "level", "tid_row", "id_high", "id_low", "upper_id", "packed", "neighbour_level",
                                  "slot_range", "slot_missing", "slot_shared", "slot_on_level_0", "entry", "row_twice"])
def test_damaged_prior_graphs_are_refused_naming_the_element(ctx, small, rule):
    from vsrbac import _ffi
    x, g = small
    assert (g["level"] >= 1).sum() >= 2 and g["tids"][3, 0] == 3
    bad, fragment = _damaged(g, rule)
    corpus = _corpus(ctx, "f32", x)
    _raises(_ffi.ERR_INVALID, fragment, corpus.extend_hnsw, bad, 16, "l2", 38)
    corpus.extend_hnsw(g, 16, "l2", 38).free()                                 # the undamaged graph is taken
    corpus.free()


def test_visited_table_overflow_restarts_the_extension_from_the_callers_arrays(ctx, monkeypatch):
    """256 slots: the first attempts fill the table, so only restarts that begin again from the prior arrays -- after an attempt
    has already written through its device copy -- can give the one-shot build's graph."""
    x = _rows("f32", N2, 7300)
    n0 = boundary_near(N2, N2 // 3)
    full = _built(ctx, "f32", x, 8, 32, "l2", 32)
    first = _built(ctx, "f32", x[:n0], 8, 32, "l2", 32)
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "256")
    got = _extended(ctx, "f32", x, first, 32, "l2", 32)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    same_graph(got, full)
