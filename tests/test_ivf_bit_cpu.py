"""tests/ivf_bit_model.py licensed before it serves as the expectation of the bit IVFFlat entry points (tests/test_gpu_ivf_bit.py,
tests/test_gpu_ivf_bit_iterative.py).  No GPU.
  * The index.  On unpacked 0 / 1 rows with 0 / 1 centres squared L2 IS the Hamming count -- every term is 0 or 1 and fp32 adds
    them exactly -- so the index oracle over the unpacked rows must probe the same lists, assign the same rows and return the same
    rows per query as the model; the distances are bit_model's counts.
  * The k-means skeleton, with ivf_half_model's L2 distance and the identity update, is orc_ivf_kmeans bit for bit.
  * The two substitutions of the bit opclass on cases small enough to do by hand."""
import numpy as np
import pytest

import bit_model
import ivf_bit_model as model
import ivf_half_model as kmodel
from oracle.oracle import METRICS, IvfIndex as OracleIvf

F32 = np.float32


@pytest.mark.parametrize("dim", [52, 136])
def test_index_model_equals_the_oracle_on_unpacked_rows(oracle, dim):
    rng = np.random.default_rng(900 + dim)
    n, lists, nq = 1200, 24, 12
    bits = rng.random((n, dim)) < 0.3
    bits[:10] = bits[3]                                       # equal distances: the (document, block) order decides
    cbits = bits[rng.choice(n, lists, replace=False)] ^ (rng.random((lists, dim)) < 0.05)
    cbits[7] = cbits[2]                                       # equal centres: the lower list id wins
    cbits[-2:] = True                                         # far from every row: empty lists
    rows, centers = bit_model.pack(bits), bit_model.pack(cbits)
    doc = (rng.permutation(n) // 7 + 1).astype(np.int32)
    blk = (rng.permutation(n) + 1).astype(np.int64)
    mask = rng.random(n) < 0.3
    # pad bits set on every input of the model: they must not count
    m = model.IvfBit(bit_model.set_pad_bits(rows, dim), dim, bit_model.set_pad_bits(centers, dim), doc, blk)
    oivf = OracleIvf.from_centers(oracle, "l2", bits.astype(F32), cbits.astype(F32))
    np.testing.assert_array_equal(m.assign, oivf.assign)
    assert not np.isin(m.assign, (7, lists - 2, lists - 1)).any() and (m.assign == 2).any()
    qbits = bits[rng.integers(0, n, nq)] ^ (rng.random((nq, dim)) < 0.1)
    qbits[0] = bits[3]
    q = bit_model.set_pad_bits(bit_model.pack(qbits), dim)
    for i in range(nq):
        for probes in (1, 5, lists):
            np.testing.assert_array_equal(m.probe(q[i], probes), oivf.probe(qbits[i].astype(F32), probes))
            for msk in (None, mask):
                idx, _ = oivf.search(qbits[i].astype(F32), 50, probes, doc, blk, msk)
                rows_m, dist_m = m.search(q[i], 50, probes, msk)
                np.testing.assert_array_equal(rows_m, idx, err_msg=f"{i} {probes}")
                want = bit_model.distances("hamming", rows, bit_model.pack(qbits[i:i + 1]), dim)[rows_m]
                np.testing.assert_array_equal(dist_m, want.astype(F32))
        # the stream of an iterative scan is the batches of the same order, each a top-k of what is still wanted
        r, d, scanned = m.iterative(q[i], 40, 2, 9, mask)
        got, left, pos = [], 40, 0
        order = m.probe(q[i], 9)
        while left > 0 and pos < 9:
            rr, _ = m._topk(q[i], left, order[pos:pos + 2], mask)
            got.append(rr)
            left -= len(rr)
            pos = min(pos + 2, 9)
        np.testing.assert_array_equal(r, np.concatenate(got))
        assert scanned == pos and len(d) == len(r)


@pytest.mark.parametrize("case", ["integer", "repeated"])
def test_kmeans_skeleton_equals_the_oracle_bit_for_bit(oracle, case):
    x, lists = kmodel.integer_case() if case == "integer" else kmodel.repeated_case()
    l2 = lambda a, b: kmodel.distance("l2", a, b)
    for seed in (1, 7):
        want = np.zeros((lists, x.shape[1]), dtype=F32)
        assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], x.shape[1], np.ascontiguousarray(x), len(x), lists, seed, want) == 0
        got, iterations = model.kmeans_skeleton(x, lists, seed, l2, model.identity_update)
        assert iterations >= 2
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        ref, ref_it = kmodel.kmeans(x, lists, seed, "l2", round_half=False)
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
        assert iterations == ref_it
    x0 = np.zeros((0, 5), dtype=F32)
    want = np.zeros((7, 5), dtype=F32)
    assert oracle.lib.orc_ivf_kmeans(METRICS["l2"], 5, x0, 0, 7, 3, want) == 0
    got, iterations = model.kmeans_skeleton(x0, 7, 3, l2, model.identity_update)
    assert iterations == 0
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_bit_distance_and_update_by_hand():
    b = lambda s: np.array([[c == "1" for c in s]], dtype=F32)
    assert model.hamming_distance(b("000"), b("111")[0]).tolist() == [3.0]
    assert model.hamming_distance(np.concatenate([b("100"), b("111")]), b("110")[0]).tolist() == [1.0, 1.0]
    # B'000', B'100', B'111': sums 2 1 1 over 3 members -> 0.667 0.333 0.333 -> 100
    members = np.concatenate([b("000"), b("100"), b("111")])
    x = np.cumsum(members, axis=0, dtype=F32)[-1] / F32(3)
    assert model.bit_update(x).tolist() == [1.0, 0.0, 0.0]
    # a 2-of-4 tie is exactly 0.5, which is not > 0.5
    x = np.cumsum(np.concatenate([b("1"), b("1"), b("0"), b("0")]), axis=0, dtype=F32)[-1] / F32(4)
    assert x.tolist() == [0.5] and model.bit_update(x).tolist() == [0.0]
    x = np.cumsum(np.concatenate([b("1"), b("1"), b("1"), b("0")]), axis=0, dtype=F32)[-1] / F32(4)
    assert model.bit_update(x).tolist() == [1.0]


def test_majority_centre_and_empty_centre_draw():
    # one list over B'000', B'100', B'111' (any seed: the only centre owns all three)
    rows = bit_model.pack(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 1]], dtype=bool))
    for seed in (1, 2, 3):
        c, it = model.kmeans(bit_model.set_pad_bits(rows, 3), 3, 1, seed)
        assert c.tolist() == [[0b10000000]] and it >= 1
    # no sample: every centre is the draw, (centre, element) order from the seeded stream, (float) value > 0.5
    lists, dim, seed = 5, 11, 9
    rng = kmodel.Rng(seed)
    want = np.array([[F32(rng.double()) > F32(0.5) for _ in range(dim)] for _ in range(lists)])
    c, it = model.kmeans(np.zeros((0, 2), np.uint8), dim, lists, seed)
    assert it == 0
    np.testing.assert_array_equal(bit_model.unpack(c, dim), want)
    assert want.any() and not want.all()
    # 3 distinct values, 5 lists: at least two centres stay empty in every iteration and are drawn
    rng2 = np.random.default_rng(4)
    base = bit_model.pack(rng2.random((3, 20)) < 0.5)
    samples = base[rng2.integers(0, 3, 60)]
    c, it = model.kmeans(samples, 20, 5, 2)
    owned = {tuple(r) for r in base.tolist()}
    assert sum(tuple(r) in owned for r in c.tolist()) == 3 and it >= 2


@pytest.mark.parametrize("dim", [3, 52, 136])
def test_every_centre_is_a_legal_bit_string(dim):
    """Packed centres of (dim + 7) // 8 bytes whose pad bits are clear, whatever the samples' pad bits held."""
    rng = np.random.default_rng(dim)
    samples = bit_model.set_pad_bits(bit_model.pack(rng.random((150, dim)) < 0.4), dim)
    c, it = model.kmeans(samples, dim, 9, 5)
    assert c.dtype == np.uint8 and c.shape == (9, (dim + 7) // 8) and it >= 1
    np.testing.assert_array_equal(c, bit_model.pack(bit_model.unpack(c, dim)))
    plain, it2 = model.kmeans(bit_model.pack(bit_model.unpack(samples, dim)), dim, 9, 5)
    np.testing.assert_array_equal(c, plain)
    assert it == it2
