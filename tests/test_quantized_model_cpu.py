"""The model of the two-stage search (tests/quantized_model.py) against the oracle it is built from: a shortlist that holds
every permitted row changes nothing, and the recall of a shorter one is the share of the exact answer it kept."""
import numpy as np
import pytest

from quantized_model import QuantizedModel, recall


def _corpus(seed, n, dim, n_docs):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    blk = rng.permutation(n).astype(np.int64) + 1
    doc = rng.integers(1, n_docs + 1, n).astype(np.int32)
    q = rng.integers(-8, 9, (6, dim)).astype(np.float32)
    return rng, x, blk, doc, q


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("half", [False, True])
def test_full_shortlist_is_the_exact_search(oracle, metric, half):
    rng, x, blk, doc, q = _corpus(1, 700, 24, 40)
    q[0, 0] = 2.5004883                                      # binary16 holds 2.5
    model = QuantizedModel(oracle, x, doc, blk, half=half)
    mask = (rng.random(700) < 0.3).astype(np.uint8)
    permitted = int(mask.sum())
    for k in (1, 10, permitted + 5):
        for shortlist in (permitted, permitted + 1, 700):
            got = model.search(metric, q, min(k, shortlist), shortlist, [mask] * len(q))
            for i, (idx, dist, S) in enumerate(got):
                want_idx, want_dist = model.exact(metric, q[i], min(k, shortlist), mask)
                assert S.size == permitted and mask[S].all()
                np.testing.assert_array_equal(idx, want_idx)
                np.testing.assert_array_equal(dist, want_dist)
    # no filter: the whole corpus
    for i, (idx, dist, S) in enumerate(model.search(metric, q, 10, 700)):
        want_idx, want_dist = model.exact(metric, q[i], 10)
        np.testing.assert_array_equal(idx, want_idx)
        np.testing.assert_array_equal(dist, want_dist)


def test_half_source_rounds_the_query_but_not_its_bits(oracle):
    _, x, blk, doc, q = _corpus(2, 300, 16, 20)
    q[0, 3] = 1e-9                                           # positive in fp32, zero in binary16
    fp32 = QuantizedModel(oracle, x, doc, blk, half=False)
    half = QuantizedModel(oracle, x, doc, blk, half=True)
    np.testing.assert_array_equal(fp32.hamming(q), half.hamming(q))
    zeroed = q.copy()
    zeroed[0, 3] = 0.0
    assert (half.hamming(q)[0] != half.hamming(zeroed)[0]).all()          # the bit is set: every distance moves by one
    a = half.search("l2", q[:1], 5, 300)[0]
    b = half.search("l2", zeroed[:1], 5, 300)[0]
    np.testing.assert_array_equal(a[1], b[1])                # ... and the distances are those of the rounded query


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_recall_is_the_share_of_the_exact_answer_in_the_shortlist(oracle, metric):
    _, x, blk, doc, q = _corpus(3, 1500, 32, 60)
    model = QuantizedModel(oracle, x, doc, blk)
    k = 20
    for i in range(len(q)):
        exact_rows, _ = model.exact(metric, q[i], k)
        last = -1.0
        for shortlist in (20, 60, 200, 1500):
            idx, _, S = model.search(metric, q[i:i + 1], k, shortlist)[0]
            r = recall(idx, exact_rows)
            assert r == np.intersect1d(S, exact_rows).size / k
            assert r >= last                                 # the shortlists are nested
            last = r
        assert last == 1.0
