"""The inputs of test_gpu_exact_shared.py (K1m, the exact shared-pass scan of csrc/vsr_mq.h, at its own edges), pinned on the
CPU: the builders live here, the GPU file imports them.

  * EXACT: World(EXACT_CLASSES, d=100, k_ref=2050).  stride4 = 25: two stages of 16 chunks, the second with 9 (zero-filled
    query chunks, rows not loaded past stride4); rw = 16.  The classes put k - 1, k and k + 1 allowed rows next to every k of
    KS, the first and last k of each candidate-buffer size (scan_cap_for_rw: the first power of two >= 2k + 256, so it
    doubles after k = 128, 384, 896 and 1920) and VSR_MAX_K = 2048.  A class's queries share one filter part, so a call of
    all queries has passes of every q_count from 2 to 16, a class of 17 (16 + a one-query pass inside the QI = 4 launch) and
    one of 33 (16 + 16 + 1).  The classes of 898 and 1922 rows are there for k + 1 at k = 897 and 1921.
  * row_case(d): rows of every length at which K1m's code or the planner's choice changes (ROW_DIMS).
  * short_tile_case(d): one-row documents whose permitted runs are 1 and rw - 1 rows long, for every rw.
  * seeded_case(adversarial): 512 queries x 66 000 rows x 64, L1, for the seeded run of search_general.

mq_supported, mq_qmax, scan_qmax and the tile rows are restated from csrc/vsr_kernels.hip; the GPU tests hold the
restatement to the kernel names and to the pass rows the planner reports."""
import math

import numpy as np
import pytest

from edge_world import World

EXACT_CLASSES = ((127, 2), (128, 3), (129, 5), (130, 4),
                 (383, 6), (384, 7), (385, 8), (386, 9),
                 (895, 10), (896, 11), (897, 12), (898, 2),
                 (1919, 13), (1920, 14), (1921, 15), (1922, 3),
                 (2047, 16), (2048, 17), (2049, 33), (9000, 16),
                 (1, 1))
KS = (128, 129, 384, 385, 896, 897, 1920, 1921, 2048)
METRICS = ("l2", "ip", "cosine", "l1")
ZERO_CLASSES = ((2, 1), (18, 2))                                       # cosine: (class of EXACT_CLASSES, all-zero rows put into it)


def exact_world():
    return World(EXACT_CLASSES, d=100, k_ref=2050)


def zero_rows_world():
    """exact_world() with three all-zero rows: one in the class of 129 allowed rows, two in the class of 2049 (at k = 2048
    the lower of the two is the last result).  Returns (world, the zero rows)."""
    w = exact_world()
    row_class = np.repeat(w.doc_class, w.doc_rows)
    zero = []
    for cls, count in ZERO_CLASSES:
        rows = np.flatnonzero(row_class == cls)
        zero += [int(rows[(7 + 501 * j) % rows.size]) for j in range(count)]
    w.x[zero] = 0
    return w, np.sort(np.asarray(zero))


# ---------------------------------------------------------------------------------------------------------------------
# csrc/vsr_kernels.hip restated: mq_supported, mq_qmax, scan_shape_for_chunks (tile rows), scan_cap_for_rw, scan_qmax
# ---------------------------------------------------------------------------------------------------------------------
SCAN_QMAX = 16
SCAN_LDS_BUDGET = 72 * 1024


def mq_supported(dim):
    return (dim + 3) // 4 >= 16


def mq_qmax(dim):
    stride4 = (dim + 3) // 4
    per_query = (stride4 + 15) // 16 * 16 * 16 + 32
    fixed = 4 * 64 * 17 * 16 + 4 * 64 * 4 + 64

    def fit(budget):
        return (budget - fixed) // per_query if budget > fixed else 0
    q = fit(80 * 1024)
    if q < 8:
        q = fit(160 * 1024)
    q = min(q, SCAN_QMAX)
    return q // 4 * 4 if q >= 4 else 0


def tile_rows(dim):
    """rw of scan_shape_for_chunks: rows per list tile of an fp32 corpus."""
    d4 = (dim + 3) // 4
    return 64 if d4 <= 4 else 32 if d4 <= 16 else 16 if d4 <= 32 else 8 if d4 <= 64 else 4 if d4 <= 192 else 2


def scan_cap(k, rw=16):
    cap = 512
    while cap < 2 * k + max(8 * rw, 256):                                # scan_slack(rw), SCAN_WAVES = 8
        cap <<= 1
    return cap


def scan_qmax(dim, k):
    """K1's queries per pass (fp32 rows): the LDS budget over one query's candidate list and padded vector; the
    runtime-chunk kernel (rows of more than 256 chunks) takes one sub-batch of 4, or one query."""
    d4 = (dim + 3) // 4
    per_query = scan_cap(k, tile_rows(dim)) * 8 + 16 + d4 * 16 + 4
    q = SCAN_LDS_BUDGET // per_query
    if d4 > 256:
        q = min(q, 4)
    return min(q, SCAN_QMAX) // 4 * 4 if q >= 4 else 1


def expected_pass_width(dim, k):
    """(queries per shared pass, K1m?) of an exact plan over fp32 rows (vsr_plan.hip, choose_width)."""
    if mq_supported(dim) and mq_qmax(dim) >= 4:
        return mq_qmax(dim), True
    return scan_qmax(dim, k), False


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
ROW_DIMS = (60, 61, 64, 65, 128, 129, 256, 257, 320, 321, 1024, 1025, 5760, 5761)
ROW_K = 10


def row_case(d):
    """(x, q, mask): 700 rows (fewer where 700 x d x 4 bytes pass 8 MB, never fewer than 3 x 64; one fewer where 700 is a
    multiple of the tile rows, so that the last implicit tile is short), integers 0 .. v with 4 d v^2 < 2^24, twenty rows
    repeated so that equal distances occur, 16 queries near rows, a 50 % byte mask."""
    rng = np.random.default_rng(7000 + d)
    n = 700
    if n * d * 4 > 8_000_000:
        n = max(3 * 64, 8_000_000 // (4 * d))
    while n % tile_rows(d) == 0:
        n -= 1
    v = min(255, int(2000 / math.sqrt(d)))
    x = rng.integers(0, v + 1, (n, d)).astype(np.float32)
    x[n // 2:n // 2 + 20] = x[:20]
    q = x[rng.integers(0, n, 16)].copy()
    q[:, :3] = rng.integers(0, v + 1, (16, 3)).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    return x, q, mask


def value_bound(x, q):
    """World.exact_bound(l1=True) for plain arrays."""
    assert (x == np.rint(x)).all() and (q == np.rint(q)).all()
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    l2 = (np.sqrt((x64 ** 2).sum(1).max()) + np.sqrt((q64 ** 2).sum(1).max())) ** 2
    l1 = np.abs(x64).sum(1).max() + np.abs(q64).sum(1).max()
    return max(l2, l1)


SHORT_TILE_DIMS = (64, 100, 200, 300, 1100)                            # rw = 32, 16, 8, 4, 2


def short_tile_case(d):
    """(x, q, doc, blk, user_roles, perms, allowed): one-row documents; user 1 may read runs of 1 and of rw - 1 rows, one
    or two forbidden rows between two runs (period rw + 3, odd: the runs drift over every alignment), so a RANGES filter is
    a list of 1-row and (rw - 1)-row tiles."""
    rng = np.random.default_rng(7100 + d)
    rw = tile_rows(d)
    n = 40 * (rw + 3) + 3
    v = min(255, int(2000 / math.sqrt(d)))
    x = rng.integers(0, v + 1, (n, d)).astype(np.float32)
    x[n // 2:n // 2 + 20] = x[:20]
    pos = np.arange(n) % (rw + 3)
    allowed = (pos == 0) | ((pos >= 2) & (pos <= rw))
    doc = (np.arange(n) + 1).astype(np.int32)
    blk = (np.arange(n) + 1).astype(np.int64)
    perms = [(1, int(dd)) for dd in doc[allowed]]
    q = x[rng.integers(0, n, 16)].copy()
    q[:, :3] = rng.integers(0, v + 1, (16, 3)).astype(np.float32)
    return x, q, doc, blk, [(1, 1)], perms, allowed.astype(np.uint8)


SEEDED_N, SEEDED_D, SEEDED_NQ = 66_000, 64, 512
SEEDED_KS = (100, 600)                                                 # final selection: one wave per query / a workgroup (kp > 512)
ADVERSARIES = (3, 7, 100, 257, 511)                                    # two of them in one pass
NEAR_ROWS = 64


def seeded_case(adversarial):
    """(x, q): integers 0 .. 255.  adversarial: rows 0 .. 63 -- the first super-tile of workgroup 0 of every pass, which
    the sample launch always visits -- are one corner of the cube (every coordinate 0 or 255) with coordinate i moved
    inwards by i + 1, and the five ADVERSARIES ask for that corner with one coordinate moved inwards by 40 (a + 1): their L1
    distances to the 64 rows are distinct and below 300, every other row is thousands away.  To every other query the corner
    is about the farthest place there is, so the 64 rows cannot tighten its seed (a sample of 64 rows around a place NEAR
    other queries would: they are 3 % of every sample and 0.1 % of the corpus)."""
    rng = np.random.default_rng(66)
    x = rng.integers(0, 256, (SEEDED_N, SEEDED_D)).astype(np.float32)
    q = rng.integers(0, 256, (SEEDED_NQ, SEEDED_D)).astype(np.float32)
    if adversarial:
        corner = 255.0 * rng.integers(0, 2, SEEDED_D).astype(np.float32)
        inwards = np.where(corner == 0, 1.0, -1.0).astype(np.float32)
        each = np.arange(NEAR_ROWS)
        x[:NEAR_ROWS] = corner
        x[each, each] += inwards[each] * (each + 1)
        for a, i in enumerate(ADVERSARIES):
            q[i] = corner
            q[i, a] += inwards[a] * 40 * (a + 1)
    return x, q


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    return exact_world()


def test_partial_sums_are_exact_in_fp32(world):
    """Integer rows and queries; (|x| + |q|)^2 bounds every partial sum of L2, IP and the three cosine sums, |x|_1 + |q|_1
    those of L1; both below 2^24."""
    assert world.exact_bound(l1=True) < 2 ** 24
    assert world.x.shape[1] == 100 and tile_rows(100) == 16 and (100 + 3) // 4 == 25
    w0, zero = zero_rows_world()
    assert w0.exact_bound(l1=True) < 2 ** 24
    assert zero.size == 3 and not w0.x[zero].any() and (np.delete(w0.x, zero, 0) == np.delete(world.x, zero, 0)).all()
    assert (w0.q ** 2).sum(1).min() > 0                                    # no all-zero query


def test_allowed_counts_are_the_class_list(oracle, world):
    w = world
    ur, perms = w.rbac()
    for c, (allowed, queries) in enumerate(EXACT_CLASSES):
        user = w.role_of_class[c]
        assert int(oracle.user_row_mask(user, ur, perms, w.doc).sum()) == allowed == w.allowed_rows(oracle, user).size
        assert int((w.quser == user).sum()) == queries
    assert (w.allowed_of_query() == [w.allowed_rows(oracle, int(u)).size for u in w.quser]).all()
    w0, zero = zero_rows_world()
    row_class = np.repeat(w0.doc_class, w0.doc_rows)
    assert sorted(EXACT_CLASSES[c][0] for c in row_class[zero]) == [129, 2049, 2049]


def test_classes_sit_on_every_k_and_pass_width():
    edges = {a for a, _ in EXACT_CLASSES}
    for k in KS:
        assert {k - 1, k, k + 1} <= edges, k
    assert {2 * k + 256 <= scan_cap(k) < 2 * (2 * k + 256) for k in KS} == {True}
    assert [scan_cap(k) for k in (128, 129, 384, 385, 896, 897, 1920, 1921, 2048)] == [512, 1024, 1024, 2048, 2048, 4096, 4096, 8192, 8192]
    widths = {w for _, w in EXACT_CLASSES}
    assert set(range(2, 17)) <= widths and {17, 33, 1} <= widths         # q_count 2 .. 16, 16 + 1, 16 + 16 + 1


@pytest.mark.parametrize("metric", METRICS)
def test_equal_distances_straddle_every_k(oracle, world, metric):
    """For every k some query's k-th and (k + 1)-th oracle distances are equal, and their rows ascend (the tie rule)."""
    w = world
    allowed = w.allowed_of_query()
    for k in KS:
        hit = 0
        for i in np.flatnonzero(allowed > k):
            idx, dist = w.ref(oracle, i, metric)
            if dist[k - 1] == dist[k]:
                assert idx[k - 1] < idx[k]
                hit += 1
                break
        assert hit, (metric, k)


def test_restated_pass_widths():
    """mq_supported / mq_qmax of csrc/vsr_kernels.hip: K1m from d = 61 (16 chunks) to 5760.  16 queries per pass while 80 KiB
    hold them (d <= 128), 12 and 8 beyond, 16 again from d = 321 where fewer than 8 fit 80 KiB and the 160 KiB budget is
    taken, 4 at d = 5760, none at d = 5761 (K1 takes the rows; four of its padded queries and candidate lists pass the
    72 KiB of scan_qmax, so its passes have one query)."""
    assert not mq_supported(60) and all(mq_supported(d) for d in range(61, 66))
    assert {mq_qmax(d) for d in range(61, 129)} == {16}
    assert {mq_qmax(d) for d in range(129, 193)} == {12} and {mq_qmax(d) for d in range(193, 321)} == {8}
    assert mq_qmax(321) == 16 and (160 * 1024 - 70720) // ((96 * 16) + 32) >= 16 > (80 * 1024 - 70720) // ((96 * 16) + 32)
    assert [mq_qmax(d) for d in (1024, 1025, 5760, 5761)] == [16, 16, 4, 0]
    assert [expected_pass_width(d, ROW_K) for d in ROW_DIMS] == [
        (16, False), (16, True), (16, True), (16, True), (16, True), (12, True), (8, True), (8, True), (8, True), (16, True),
        (16, True), (16, True), (4, True), (1, False)]
    assert [tile_rows(d) for d in ROW_DIMS] == [32, 32, 32, 16, 16, 8, 8, 4, 4, 4, 2, 2, 2, 2]


@pytest.mark.parametrize("d", ROW_DIMS)
def test_row_cases_are_exact_and_end_in_a_short_tile(d):
    x, q, mask = row_case(d)
    n = x.shape[0]
    assert value_bound(x, q) < 2 ** 24
    assert 3 * 64 <= n <= 700 and n * d * 4 <= 8_000_000 and n % tile_rows(d) != 0
    assert 0.4 * n < mask.sum() < 0.6 * n
    if d == 5761:
        assert x.max() >= 15


@pytest.mark.parametrize("d", SHORT_TILE_DIMS)
def test_short_tile_cases(oracle, d):
    x, q, doc, blk, ur, perms, allowed = short_tile_case(d)
    rw = tile_rows(d)
    assert value_bound(x, q) < 2 ** 24
    assert (oracle.user_row_mask(1, ur, perms, doc) == allowed).all()
    edges = np.flatnonzero(np.diff(np.concatenate([[0], allowed, [0]])))
    runs = edges[1::2] - edges[::2]
    assert set(runs.tolist()) == {1, rw - 1} and runs.size >= 48
    assert len({int(s) % rw for s in edges[::2]}) == rw                    # a run starts at every offset of a tile


def test_seeded_shape_and_adversaries():
    """32 passes x 66 000 rows >= seed_min_rows = 2 000 000 and k >= SEED_LIST = 64 (vsr_search.hip); for the five adversaries
    rows 0 .. 63 have distinct L1 distances, all below every other row's: a seed of any rank m <= 64 is the m-th of them."""
    assert (SEEDED_NQ + 15) // 16 * SEEDED_N >= 2_000_000 and min(SEEDED_KS) >= 64
    x, q = seeded_case(True)
    x0, q0 = seeded_case(False)
    assert value_bound(x, q) < 2 ** 24 and value_bound(x0, q0) < 2 ** 24
    assert (x[NEAR_ROWS:] == x0[NEAR_ROWS:]).all() and (np.delete(q, ADVERSARIES, 0) == np.delete(q0, ADVERSARIES, 0)).all()
    for i in ADVERSARIES:
        dist = np.abs(x.astype(np.float64) - q[i].astype(np.float64)).sum(1)
        near = dist[:NEAR_ROWS]
        assert np.unique(near).size == NEAR_ROWS and near.max() < dist[NEAR_ROWS:].min(), (i, near.max(), dist[NEAR_ROWS:].min())
    # every other query: more than max(k) rows -- counted in 2048 of them -- are nearer than the nearest of the 64, so a seed
    # that is one of the 64 admits more than k rows
    others = np.delete(np.arange(SEEDED_NQ), ADVERSARIES)
    some = x[NEAR_ROWS:NEAR_ROWS + 2048].astype(np.float64)
    for i in others:
        nearest = np.abs(x[:NEAR_ROWS].astype(np.float64) - q[i].astype(np.float64)).sum(1).min()
        assert (np.abs(some - q[i].astype(np.float64)).sum(1) < nearest).sum() > max(SEEDED_KS), i
