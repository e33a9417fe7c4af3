"""The exported HNSW graph off the GPU: the .npz form (formats.save_hnsw / load_hnsw) and the binding of the build / export
entry points.  No GPU: the graph is the index oracle's export."""
import numpy as np
import pytest

from oracle.oracle import HnswIndex as OracleHnsw


@pytest.fixture(scope="module")
def graph(oracle):
    rng = np.random.default_rng(4401)
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (600, 8)))), 0, 255).astype(np.float32)
    x[rng.permutation(600)[:45]] = x[7]                                  # elements of 10, 10, 10, ... heap TIDs
    return OracleHnsw(oracle, "l2", x, m=8, ef_construction=32, seed=3).export()


def test_save_and_load_round_trip_an_export_exactly(graph, tmp_path):
    from vsrbac import formats
    assert graph["tid_count"].max() > 1 and (graph["up_slot"] >= 0).any()
    path = tmp_path / "graph.hnsw"                                       # (no ".npz" appended to the name given)
    formats.save_hnsw(str(path), graph)
    assert path.exists()
    back = formats.load_hnsw(str(path))
    assert sorted(back) == sorted(graph)
    for key, want in graph.items():
        if isinstance(want, np.ndarray):
            assert back[key].dtype == want.dtype and back[key].shape == want.shape, key
            np.testing.assert_array_equal(back[key], want, err_msg=key)
        else:
            assert type(back[key]) is int and back[key] == want, key


def test_load_rejects_a_file_that_is_no_graph(tmp_path):
    from vsrbac import formats
    path = tmp_path / "other.npz"
    np.savez(str(path), level=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="not an HNSW graph file"):
        formats.load_hnsw(str(path))


def test_build_and_export_entry_points_are_bound():
    from vsrbac import _ffi
    import vsrbac
    for name in ("vsr_hnsw_build_ex", "vsr_hnsw_export_shape", "vsr_hnsw_export"):
        assert name in _ffi.SYMBOLS, name
    lib = vsrbac.load_library()
    assert lib.vsr_hnsw_build_ex.argtypes[5] is _ffi.C.c_uint32          # flags
    assert len(lib.vsr_hnsw_export.argtypes) == 7 and len(lib.vsr_hnsw_export_shape.argtypes) == 6
