"""The restatements tests/test_gpu_hnsw_extend.py rests on (tests/hnsw_extend_model.py), pinned to the serial model of the batched
build, and the Python surface of vsr_hnsw_extend.  Nothing here needs a GPU."""
import inspect

import numpy as np

from helpers import same_graph
from hnsw_extend_model import BATCH_MAX, boundaries, boundary_near, level_stream, schedule
from oracle.oracle import HnswIndex as OracleHnsw


def _rows(n):
    x = np.random.default_rng(7100).integers(0, 30, (n, 6)).astype(np.float32)
    assert len(np.unique(x, axis=0)) == n
    return x


def test_schedule_restatement_agrees_with_the_models_batches(oracle):
    """The restatement says: batches of one element while done < 16 or one element is left (so 17 rows are inserted serially),
    the first batch of two at done = 16.  The model agrees where that can be seen in graphs: capped to batches of one it builds
    the same 17-row graph and a different 40-row graph."""
    assert [c for _, c in schedule(0, 17)] == [1] * 17
    assert schedule(0, 40)[16] == (16, 2) and max(c for _, c in schedule(0, 40)) == 4
    assert schedule(0, 40)[-1][0] + schedule(0, 40)[-1][1] == 40
    x = _rows(40)
    build = lambda rows, limit: OracleHnsw.batched(oracle, "l2", rows, 4, 16, 5, batch_limit=limit).export()
    same_graph(build(x[:17], 0), build(x[:17], 1))
    a, b = build(x, 0), build(x, 1)
    np.testing.assert_array_equal(a["level"], b["level"])
    assert (a["nbr0"] != b["nbr0"]).any() or (a["up_nbr"] != b["up_nbr"]).any()


def test_schedule_depends_on_done_alone():
    """A schedule started at one of its own boundaries is the rest of that schedule; batches reach BATCH_MAX once done passes
    8 x BATCH_MAX = 32 768.  The boundaries around it are 31 694, 35 655 and 39 751 -- 36 864 = 32 768 + 4096 is NOT one, the
    schedule never stands at 32 768 -- so the BATCH_MAX case of the GPU tests extends the prefix of 35 655."""
    full = schedule(0, 41_500)
    assert [b for b in boundaries(0, 41_500) if b > 30_000] == [31_694, 35_655, 39_751, 41_500]
    for start in (boundary_near(41_500, 14_000), 35_655):
        assert start in boundaries(0, 41_500)
        assert schedule(start, 41_500) == [bt for bt in full if bt[0] >= start]
    assert schedule(35_655, 41_500) == [(35_655, BATCH_MAX), (39_751, 1749)]
    assert schedule(36_864, 41_500) != [bt for bt in full if bt[0] >= 36_864]
    assert boundaries(1000, 2500)[0] == 1000 and boundaries(1000, 2500)[-1] == 2500


def test_level_stream_is_the_models(oracle):
    for m, seed, n in ((4, 5, 700), (16, 21, 900), (2, 3, 300)):
        x = np.random.default_rng(7101).integers(0, 50, (n, 5)).astype(np.float32)
        g = OracleHnsw.batched(oracle, "l2", x, m, 2 * m + 8, seed).export()
        np.testing.assert_array_equal(g["level"], np.array(level_stream(seed, m, n), dtype=np.int32))


def test_ffi_carries_the_symbol():
    from vsrbac import _ffi
    assert "vsr_hnsw_extend" in _ffi.SYMBOLS
    restype, args = _ffi.SYMBOLS["vsr_hnsw_extend"]
    assert len(args) == 17


def test_python_surface():
    """Corpus.extend_hnsw(graph, ef_construction=64, metric=None, seed=1) and HnswIndex.extended_over(corpus, ...): metric None
    resolves to "l2", or "hamming" on a bit corpus."""
    from vsrbac.engine import Corpus, HnswIndex
    p = inspect.signature(Corpus.extend_hnsw).parameters
    assert list(p) == ["self", "graph", "ef_construction", "metric", "seed"]
    assert (p["ef_construction"].default, p["metric"].default, p["seed"].default) == (64, None, 1)
    p = inspect.signature(HnswIndex.extended_over).parameters
    assert list(p) == ["self", "corpus", "ef_construction", "metric", "seed"]
    assert (p["ef_construction"].default, p["metric"].default, p["seed"].default) == (64, None, 1)
    for fn in (Corpus.extend_hnsw, HnswIndex.extended_over):
        assert "free the old" in " ".join(fn.__doc__.split())               # the recipe: reload, extend, free the old pair
