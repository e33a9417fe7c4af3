"""The batched HNSW build on the GPU (vsr_hnsw_build*, vsr_hnsw_build.hip) against its serial model, graph for graph.

The model is oracle.HnswIndex.batched (vsr_index_oracle.c: orc_hnsw_build_batched): pgvector's HnswFindElementNeighbors,
SelectNeighbors and HnswUpdateConnection under the GPU's schedule -- batches of max(1, min(done / 8, 4096)) elements that search
the graph as it stood when the batch began, reverse edges applied in ascending source element -- with candidates of equal
distance ordered by element id.  tests/test_hnsw_build_model_cpu.py pins it to the serial build.  Levels and TIDs are the
model's own: nothing here is read from the GPU before it is compared.

All rows are integer valued with every partial sum below 2^24 (_exact asserts it), so an fp32 distance does not depend on the
order of summation and the exported arrays must be EQUAL: a wrong prune, a lost reverse edge or a wrong tie shows as a
different list.  Jaccard distances are not integers, but one correctly rounded fp32 value of two integers.  After every build
the session's guard word must be clean."""
import numpy as np
import pytest

import bit_model
from helpers import check_built_graph, same_graph, sift_like
from hnsw_half_model import to_half, want_dist, widen
from oracle.oracle import HnswIndex as OracleHnsw
from test_gpu_hnsw_dedup import _canonical, _planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _exact(x):
    """World.exact_bound for plain rows: integer valued, and (|a| + |b|)^2 < 2^24 bounds every partial sum of a squared
    distance or an inner product of two rows."""
    x64 = np.asarray(x, dtype=np.float64)
    assert (x64 == np.rint(x64)).all()
    assert 4.0 * (x64 ** 2).sum(axis=1).max() < 2 ** 24
    return x


def _build(ctx, kind, x, m, efc, metric, seed, merge=False):
    """The GPU's export of a build over x (kind: "f32" rows, "half": x rounded to binary16, "bit": x as booleans)."""
    if kind == "f32":
        corpus = ctx.load_corpus(np.ascontiguousarray(x, dtype=np.float32))
        gpu = corpus.build_hnsw(m, efc, metric, seed=seed, merge_duplicates=merge)
    elif kind == "half":
        corpus = ctx.load_corpus_half(to_half(x))
        gpu = corpus.build_hnsw_half(m, efc, metric, seed=seed, merge_duplicates=merge)
    else:
        corpus = ctx.load_corpus_bit(np.asarray(x) != 0)
        gpu = corpus.build_hnsw_bit(m, efc, metric, seed=seed, merge_duplicates=merge)
    ctx.screening_check(0)                              # raises when a kernel left a guard bit behind
    g = gpu.export()
    gpu.free()
    corpus.free()
    return g


def _model(oracle, kind, x, m, efc, metric, seed, elements=None):
    """The model over the values the GPU holds: widened binary16 rows, 0 / 1 rows (Hamming is their squared L2)."""
    if kind == "half":
        x = widen(to_half(x))
    elif kind == "bit":
        x = (np.asarray(x) != 0).astype(np.float32)
        metric = {"hamming": "l2", "jaccard": "jaccard"}[metric]
    return OracleHnsw.batched(oracle, metric, x, m, efc, seed, elements=elements)


def _compare(ctx, oracle, kind, x, m, efc, metric, seed):
    want = _model(oracle, kind, x, m, efc, metric, seed).export()
    got = _build(ctx, kind, x, m, efc, metric, seed)
    np.testing.assert_array_equal(got["level"], want["level"])
    same_graph(got, want)
    check_built_graph(got, m)
    return got


def _small_ints(seed, n, dim, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi + 1, (n, dim)).astype(np.float32)


# ---- fp32 -------------------------------------------------------------------------------------------------------------------
_F32 = {}


def _f32_rows(n, dim):
    """SIFT-like at 128 and 260, small integers elsewhere; the 3-d rows (0 .. 11) repeat: distance-0 ties decided by element id."""
    if (n, dim) not in _F32:
        if dim >= 128:
            x = sift_like(np.random.default_rng(6000 + dim), n, dim)
        else:
            x = _small_ints(6000 + dim, n, dim, 0, 11 if dim == 3 else 40)
        _F32[(n, dim)] = _exact(x)
    return _F32[(n, dim)]


@pytest.mark.parametrize("n,dim", [(1500, 3), (1500, 10), (1200, 128), (600, 260)])
def test_fp32_l2_build_is_the_model(ctx, oracle, n, dim):
    """dims 3 and 10: the tail chunk; 260: the 32-lane loop takes a third step."""
    x = _f32_rows(n, dim)
    if dim == 3:
        assert len(np.unique(x, axis=0)) < n
    _compare(ctx, oracle, "f32", x, 16, 64, "l2", seed=21)


@pytest.mark.parametrize("n,dim", [(1500, 10), (1200, 128)])
def test_fp32_inner_product_build_is_the_model_and_cosine_is_ip(ctx, oracle, n, dim):
    x = _exact(_small_ints(6100 + dim, n, dim, -8, 8))
    got = _compare(ctx, oracle, "f32", x, 16, 64, "ip", seed=22)
    same_graph(_build(ctx, "f32", x, 16, 64, "cosine", seed=22), got)       # the build maps both opclasses to M_IP


def _wide_rows():
    return _exact(sift_like(np.random.default_rng(6200), 700, 16))


def test_narrow_lists_many_layers(ctx, oracle):
    """m = 4, ef_construction = 16: lists of 8 / 4, five or more layers, elements inserted above the entry level."""
    x = _exact(sift_like(np.random.default_rng(6201), 1500, 16))
    g = _compare(ctx, oracle, "f32", x, 4, 16, "l2", seed=23)
    level = g["level"]
    assert g["max_level"] >= 4
    top = np.maximum.accumulate(level)
    assert (level[1:] > top[:-1]).sum() >= 2, "no element was inserted above the entry level"


def test_wide_lists(ctx, oracle):
    """m = 48, ef_construction = 100: 2m = 96 > 64 lanes in every list loop, hb_select with more than 64 candidates, the rank
    sort over 97 keys."""
    g = _compare(ctx, oracle, "f32", _wide_rows(), 48, 100, "l2", seed=24)
    assert ((g["nbr0"] >= 0).sum(axis=1) == 96).any(), "no full layer-0 list: the link kernel never pruned"


# ---- halfvec and bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,dim", [(1500, 10), (1200, 128), (600, 520)])
def test_halfvec_build_is_the_model_on_the_widened_rows(ctx, oracle, n, dim, metric):
    x = _exact(_small_ints(6300 + dim, n, dim, -8, 8))
    _compare(ctx, oracle, "half", x, 16, 64, metric, seed=25)


@pytest.mark.parametrize("metric", ["hamming", "jaccard"])
@pytest.mark.parametrize("n,dim", [(1500, 52), (1200, 128), (300, 1032)])
def test_bit_build_is_the_model_on_the_unpacked_rows(ctx, oracle, n, dim, metric):
    """52 bits: one partial 16-byte chunk; 128: one full chunk; 1032: the chunk loop with a tail (the model walks 1032 floats per
    distance: 300 rows keep it to a second or two)."""
    x = _small_ints(6400 + dim, n, dim, 0, 1)
    _compare(ctx, oracle, "bit", x, 16, 64, metric, seed=26)


# ---- the merging build ----------------------------------------------------------------------------------------------------------
def _merged(ctx, oracle, kind, x, held, metric):
    """held: the rows as the corpus holds them (their bytes decide what is identical)."""
    elements = _canonical(held)
    assert len(elements) < len(x)
    want = _model(oracle, kind, x, 16, 64, metric, 11, elements=elements).export()
    got = _build(ctx, kind, x, 16, 64, metric, 11, merge=True)
    for key in ("level", "tid_count", "tids"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    same_graph(got, want)
    check_built_graph(got, 16)


@pytest.mark.parametrize("dim", [3, 128])
def test_merging_build_is_the_model_over_the_canonical_elements(ctx, oracle, dim):
    x = _exact(_planted(dim)[0])
    _merged(ctx, oracle, "f32", x, x, "l2")


def test_merging_halfvec_build_is_the_model(ctx, oracle):
    x = _exact(_planted(128)[0])
    _merged(ctx, oracle, "half", x, to_half(x), "l2")


def test_merging_bit_build_is_the_model(ctx, oracle):
    bits = (_planted(128)[0] > 30).astype(np.float32)
    _merged(ctx, oracle, "bit", bits, bit_model.pack(bits != 0), "hamming")


# ---- the batch schedule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 2, 8, 9, 16, 17, 25])
def test_first_batches(ctx, oracle, ne):
    """Batches of one element up to done = 16, the first batch of two there, a short last batch."""
    x = _exact(_small_ints(6500, 25, 6, 0, 20)[:ne])
    _compare(ctx, oracle, "f32", x, 16, 64, "l2", seed=27)


def test_batches_of_batch_max(ctx, oracle):
    """37 000 distinct 4-d rows, m = 4, ef_construction = 16: batches of 4096 begin at done = 32 768, the last one is short."""
    rng = np.random.default_rng(6600)
    cells = rng.permutation(24 ** 4)[:37_000]
    x = _exact(np.stack([(cells // 24 ** i) % 24 for i in range(4)], axis=1).astype(np.float32))
    assert len(np.unique(x, axis=0)) == 37_000
    _compare(ctx, oracle, "f32", x, 4, 16, "l2", seed=28)


# ---- run to run -------------------------------------------------------------------------------------------------------------------
def test_the_same_build_three_times(ctx, oracle):
    x = _f32_rows(1200, 128)
    first = _build(ctx, "f32", x, 16, 64, "l2", seed=21)
    for _ in range(2):
        same_graph(_build(ctx, "f32", x, 16, 64, "l2", seed=21), first)


def test_real_valued_rows_build_the_same_graph_twice(ctx):
    """No model here (a lane-order sum is not the serial sum on real values): the two exports only have to equal each other.
    What could differ is the order in which a target's reverse edges of one batch are applied."""
    x = np.random.default_rng(6700).normal(size=(2000, 24)).astype(np.float32)
    a = _build(ctx, "f32", x, 8, 32, "l2", seed=29)
    b = _build(ctx, "f32", x, 8, 32, "l2", seed=29)
    same_graph(a, b)
    check_built_graph(a, 8)


# ---- the walk over the built graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["128d", "m48"])
def test_walk_over_the_built_graph_is_the_models_walk(ctx, oracle, case):
    x, m, efc, seed = (_f32_rows(1200, 128), 16, 64, 21) if case == "128d" else (_wide_rows(), 48, 100, 24)
    rng = np.random.default_rng(6800)
    q = x[rng.integers(0, len(x), 12)] + rng.integers(-2, 3, (12, x.shape[1])).astype(np.float32)
    _exact(q)
    model = _model(oracle, "f32", x, m, efc, "l2", seed)
    corpus = ctx.load_corpus(x)
    gpu = corpus.build_hnsw(m, efc, "l2", seed=seed)
    k = 600
    for ef in (10, 40, 500):
        res, vis = gpu.search(q, k, ef, "l2")
        for i in range(len(q)):
            rows_o, dist_o, _, nv = model.search(q[i], ef)
            want = rows_o[:k]
            where = (case, ef, i)
            assert res.counts[i] == want.size, (where, res.counts[i], want.size)
            np.testing.assert_array_equal(res.rows[i, :want.size], want, err_msg=str(where))
            np.testing.assert_array_equal(res.dist[i, :want.size], want_dist("l2", dist_o[:k]), err_msg=str(where))
            assert vis[i] == nv, (where, vis[i], nv)
            assert (res.rows[i, want.size:] == -1).all()
    ctx.screening_check(0)
    gpu.free()
    corpus.free()


# ---- no silent degradation ---------------------------------------------------------------------------------------------------------
def test_visited_table_overflow_restarts_the_build(ctx, oracle, monkeypatch):
    """256 slots: a search of 64 entries plus its expansions passes 3/4 full, so only the restart with a larger table can
    produce the model's graph; the guard word is clean afterwards (_build checks it)."""
    x = _f32_rows(1500, 10)
    want = _model(oracle, "f32", x, 16, 64, "l2", 21).export()
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", "256")
    got = _build(ctx, "f32", x, 16, 64, "l2", seed=21)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    same_graph(got, want)


@pytest.mark.parametrize("value", ["128", "65536", "300", "4096x", "", "-256"])
def test_visited_slots_knob_rejects_what_is_no_table_size(ctx, monkeypatch, value):
    import vsrbac
    corpus = ctx.load_corpus(_f32_rows(1500, 10)[:50])
    monkeypatch.setenv("VSR_HNSW_BUILD_VISITED_SLOTS", value)
    with pytest.raises(vsrbac.VsrError, match="VSR_HNSW_BUILD_VISITED_SLOTS"):
        corpus.build_hnsw(16, 64, "l2", seed=1)
    monkeypatch.delenv("VSR_HNSW_BUILD_VISITED_SLOTS")
    corpus.build_hnsw(16, 64, "l2", seed=1).free()
    corpus.free()
