"""tests/ivf_half_model.py against the index oracle's k-means (orc_ivf_kmeans), switch off: the numpy model must be the C code
bit for bit before it may serve, switch on, as the expectation of vsr_ivf_kmeans_half (tests/test_gpu_ivf_half.py).  No GPU."""
import numpy as np
import pytest

import ivf_half_model as model
from oracle.oracle import METRICS


def _oracle_kmeans(oracle, x, lists, seed):
    centers = np.zeros((lists, x.shape[1]), dtype=np.float32)
    assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], x.shape[1], np.ascontiguousarray(x), len(x), lists, seed, centers) == 0
    return centers


@pytest.mark.parametrize("case", ["integer", "repeated"])
def test_model_equals_the_oracle_bit_for_bit(oracle, case):
    x, lists = model.integer_case() if case == "integer" else model.repeated_case()
    for seed in (1, 7):
        want = _oracle_kmeans(oracle, x, lists, seed)
        got, iterations = model.kmeans(x, lists, seed, "l2", round_half=False)
        assert iterations >= 2
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        if case == "repeated":                               # not vacuous: some centre is a random fill, values in [0, 1)
            filled = (got < 1).all(axis=1) & (got != np.floor(got)).any(axis=1)
            assert filled.sum() >= lists - 40


def test_no_samples_is_the_random_fill(oracle):
    x = np.zeros((0, 5), dtype=np.float32)
    want = np.zeros((7, 5), dtype=np.float32)
    assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], 5, x, 0, 7, 3, want) == 0
    got, iterations = model.kmeans(x, 7, 3)
    assert iterations == 0
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_switch_on_rounds_every_centre_value():
    """Every centre of the half form is a binary16 value; on the integer case the means are not, so the switch changes them."""
    x, lists = model.integer_case()
    plain, _ = model.kmeans(x, lists, 1, "l2", round_half=False)
    half, _ = model.kmeans(x, lists, 1, "l2", round_half=True)
    np.testing.assert_array_equal(half, half.astype(np.float16).astype(np.float32))
    assert (plain != plain.astype(np.float16).astype(np.float32)).any()
    x, lists = model.repeated_case()
    half, _ = model.kmeans(x, lists, 1, "l2", round_half=True)
    np.testing.assert_array_equal(half, half.astype(np.float16).astype(np.float32))
    sph, _ = model.kmeans(x, lists, 1, "cosine", round_half=True)
    np.testing.assert_array_equal(sph, sph.astype(np.float16).astype(np.float32))
    norms = np.sqrt((sph.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norms - 1).max() < 8 * 2.0 ** -11          # dim 8 elements, each within half a binary16 ulp of its quotient
