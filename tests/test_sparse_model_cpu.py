"""tests/sparse_model.py against pgvector: its sequential restatement of sparsevec.c's distances reproduces every distance /
operator statement of test/expected/sparsevec.out (tests/golden/pgvector_sparsevec_known_answers.json), and its vectorised
corpus form is that restatement bit for bit on the integer-valued data the GPU tests compare for equality.  CPU only."""
import json
import math
import os

import numpy as np
import pytest

import sparse_model
from sparse_model import SparseModel
from vsrbac import formats

FN = {"l2_distance": "l2", "<->": "l2", "inner_product": "ip", "<#>": "ip", "cosine_distance": "cosine", "<=>": "cosine",
      "l1_distance": "l1", "<+>": "l1"}


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_sparsevec_known_answers.json")) as f:
        return json.load(f)


def expected_value(c):
    """The float8 psql printed; inner_product prints the product, the model (like <#>) the negative one."""
    v = float(c["expected"].replace("Infinity", "inf"))
    return -v if c["fn"] == "inner_product" else v


def test_known_answers(known):
    cases = known["distances"]
    assert len(cases) == 36 and {FN[c["fn"]] for c in cases} == set(sparse_model.METRICS)
    for c in cases:
        ai, ax, da = formats.sparsevec_from_text(c["a"])
        bi, bx, db = formats.sparsevec_from_text(c["b"])
        if "error" in c:
            assert da != db and c["error"] == f"different sparsevec dimensions {da} and {db}"
            continue
        assert da == db
        got = sparse_model.pair_distance(FN[c["fn"]], ai, ax, bi, bx)
        want = expected_value(c)
        assert (math.isnan(got) and math.isnan(want)) or got == want, (c, got)


def test_vectorised_model_is_the_sequential_one_on_integers():
    rng = np.random.default_rng(2)
    dim, n = 97, 60
    rows = []
    for r in range(n):
        nnz = int(rng.integers(0, 40))
        ix = np.sort(rng.choice(dim, size=nnz, replace=False)).astype(np.int32)
        vx = rng.integers(1, 9, nnz).astype(np.float32) * rng.choice([-1, 1], nnz).astype(np.float32)
        rows.append((ix, vx))
    indptr, indices, values = sparse_model.csr(rows)
    m = SparseModel(indptr, indices, values, dim)
    for qr in (0, 5, 17, n - 1):
        qi, qx = rows[qr]
        for metric in sparse_model.METRICS:
            d = m.distances(metric, qi, qx)
            for r in range(n):
                want = np.float32(sparse_model.pair_distance(metric, rows[r][0], rows[r][1], qi, qx))
                assert (np.isnan(d[r]) and np.isnan(want)) or d[r] == want, (metric, qr, r, d[r], want)
    d = m.distances("cosine", [], [])
    assert np.isnan(d).all()
    order, dist = m.topk(m.distances("l2", rows[3][0], rows[3][1]), 5)
    assert order[0] == 3 and dist[0] == 0


def test_topk_order_nan_last_then_ids():
    indptr, indices, values = sparse_model.csr([([0], [1.0]), ([], []), ([0], [1.0]), ([0], [2.0])])
    m = SparseModel(indptr, indices, values, 4, doc=[2, 1, 1, 1], blk=[1, 2, 3, 4])
    order, dist = m.topk(m.distances("cosine", [0], [1.0]), 4)
    assert list(order) == [2, 3, 0, 1] and np.isnan(dist[3]) and (dist[:3] == 0).all()
