"""Synthetic inputs for the multi-GPU merge (vsr_merge_topk_device / vsr_merge_topk_packed_device) and its reference:
a plain sort.  Per query the reference concatenates the real (non-KEY_EMPTY) keys of all parts as numpy.uint64, sorts them
and keeps the first k; the payload of a slot is the one that came with its key.  Keys within a query are unique (the
kernel's contract, csrc/vsr_topk.h), so the order is total and every comparison made with it is exact equality.

The generator asserts what it promises (empty parts, full parts, an all-empty query, queries with fewer than / exactly k
keys, distance ties across parts), so a change to it cannot quietly drop one of the cases the merge tests rely on."""
import numpy as np

KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max

# the (n_parts, k) cases of the merge tests and why each is there
SHAPES = [
    (1, 1), (1, 2048), (2, 1),            # degenerate ends; np2 has a minimum of 2
    (3, 5), (3, 43),                      # total = 15 / 129: padded to np2 = 16 / 256
    (2, 64), (8, 512),                    # total == np2; 4096 keys = 48 KB, the last size on the default LDS path
    (8, 513), (5, 1000),                  # first sizes above 64 KB of LDS (np2 = 8192, 96 KB)
    (4, 2048), (64, 128), (8192, 1),      # total = 8192, the API's limit, three aspect ratios
    (8, 100), (16, 500),                  # ordinary
]


def _bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


# one of every kind of value the monotone map treats differently (a NaN with a sign and a payload included: the key
# canonicalises it, the distance passes through bit for bit)
SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, _bits(0xFFC00001), FLT_MAX, -FLT_MAX, 1e-40, -1e-40],
                    dtype=np.float32)
# values handed out several times per query: their keys tie on distance and are ordered by the global row alone
# (-0.0 and +0.0 are ONE distance for the key, like the two NaNs)
REPEATED = [np.array([0.0, -0.0], np.float32), np.array([-2.25], np.float32), np.array([np.nan, _bits(0xFFC00001)], np.float32),
            np.array([1.5], np.float32)]


def _spread(rng, total, n_parts, k):
    """`total` entries over n_parts parts, none above k."""
    c = np.zeros(n_parts, dtype=np.int64)
    for _ in range(total):
        free = np.flatnonzero(c < k)
        c[rng.choice(free)] += 1
    return c


def _counts(rng, n_parts, k, nq):
    c = rng.integers(0, k + 1, (n_parts, nq))
    if nq >= 7 and n_parts >= 2:
        c[0, 0], c[1, 0] = 0, k                              # an empty part beside a full one
        c[:, 1] = 0                                          # a query with nothing at all
        c[:, 2] = _spread(rng, k - 1, n_parts, k)            # fewer than k real keys over all parts
        c[:, 3] = _spread(rng, k, n_parts, k)                # exactly k
        c[:, 4] = k                                          # every part full: n_parts * k keys, all but k dropped
    return c


def _values(rng, t):
    """t distances: about a third in tie groups (every repeated value at least twice), the rest specials and normals of
    both signs over the whole exponent range."""
    v = np.empty(t, dtype=np.float32)
    n_tie = 0 if t < 2 else max(2, -(-t // 3))
    groups = max(1, min(len(REPEATED), n_tie // 2))
    for i in range(n_tie):
        alt = REPEATED[i % groups]
        v[i] = alt[(i // groups) % alt.size]
    rest = t - n_tie
    pick = rng.random(rest)
    with np.errstate(over="ignore"):
        normals = (rng.standard_normal(rest) * 10.0 ** rng.uniform(-36, 38, rest)).astype(np.float32)
    v[n_tie:] = np.where(pick < 0.15, SPECIALS[rng.integers(0, SPECIALS.size, rest)], normals)
    return v


def _unique_rows(rng, t):
    """t distinct global rows from the whole 0 .. 2**32 - 1 range, the two ends included when there is room."""
    r = np.unique(rng.integers(1, 2**32 - 1, 2 * t + 16, dtype=np.uint64))
    r = rng.permutation(r)[:t]
    if t >= 2:
        r[0], r[1] = 0, 2**32 - 1
    return r


def make_case(n_parts, k, nq, seed):
    """Inputs in the [n_parts][nq][k] layout plus the reference outputs, all numpy."""
    from vsrbac.sharded import monotone_keys
    rng = np.random.default_rng(seed)
    c = _counts(rng, n_parts, k, nq)
    keys = np.full((n_parts, nq, k), KEY_EMPTY, dtype=np.uint64)
    block = np.full((n_parts, nq, k), -1, dtype=np.int64)
    doc = np.full((n_parts, nq, k), -1, dtype=np.int32)
    dist = np.full((n_parts, nq, k), np.inf, dtype=np.float32)
    ref = {"keys": np.full((nq, k), KEY_EMPTY, dtype=np.uint64), "block": np.full((nq, k), -1, dtype=np.int64),
           "doc": np.full((nq, k), -1, dtype=np.int32), "dist": np.full((nq, k), np.inf, dtype=np.float32),
           "counts": np.zeros(nq, dtype=np.int32)}
    cross_part_ties = 0
    for q in range(nq):
        t = int(c[:, q].sum())
        v = _values(rng, t)
        rows = _unique_rows(rng, t)
        key = monotone_keys(v, rows)
        assert np.unique(key).size == t and (key != KEY_EMPTY).all()
        blk = (rows.astype(np.int64) << 20) + 7                           # block ids beyond 32 bits
        dc = (rows * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)   # both signs
        order = rng.permutation(t)                                        # which entries land in which part
        key, v, blk, dc = key[order], v[order], blk[order], dc[order]
        part_of = np.repeat(np.arange(n_parts), c[:, q])
        hi = key >> np.uint64(32)
        uniq, inv, cnt = np.unique(hi, return_inverse=True, return_counts=True)
        if t >= 2:
            assert (cnt[inv] > 1).sum() * 4 >= t, "at least a quarter of a query's keys tie on distance"
        for g in np.flatnonzero(cnt > 1):
            cross_part_ties += np.unique(part_of[inv == g]).size > 1
        at = 0
        for p in range(n_parts):
            m = int(c[p, q])
            s = at + np.argsort(key[at:at + m])                           # every part's list is sorted by key
            keys[p, q, :m], block[p, q, :m], doc[p, q, :m], dist[p, q, :m] = key[s], blk[s], dc[s], v[s]
            at += m
        # the reference: concatenate the real keys, sort, keep k; the payload is looked up by key
        real = keys[:, q, :][keys[:, q, :] != KEY_EMPTY]
        assert real.size == t
        want = np.sort(real)[:k]
        where = {int(kk): i for i, kk in enumerate(key)}
        src = np.array([where[int(kk)] for kk in want], dtype=np.int64)
        m = want.size
        ref["keys"][q, :m], ref["counts"][q] = want, m
        ref["block"][q, :m], ref["doc"][q, :m], ref["dist"][q, :m] = blk[src], dc[src], v[src]
    if nq >= 7 and n_parts >= 2:
        tot = c.sum(0)
        assert ((c == 0) & (tot > 0)[None, :]).any(), "an empty part in a query that has keys"
        assert (c == k).any(), "a full part"
        assert (tot == 0).any(), "a query whose parts are all empty"
        assert (tot == k).any(), "a query with exactly k keys"
        assert k == 1 or ((tot > 0) & (tot < k)).any(), "a query with fewer than k keys"
        assert (tot > k).any(), "a query that has to drop keys"
        assert cross_part_ties > 0, "distance ties between parts"
    return {"n_parts": n_parts, "k": k, "nq": nq, "keys": keys, "block": block, "doc": doc, "dist": dist, "ref": ref}


def packed_records(case):
    """The same inputs as n_parts packed records {keys[nq][k], block[nq][k], doc[nq][k], dist[nq][k]}, as bytes."""
    out = []
    for p in range(case["n_parts"]):
        out += [case["keys"][p].tobytes(), case["block"][p].tobytes(), case["doc"][p].tobytes(), case["dist"][p].tobytes()]
    return np.frombuffer(b"".join(out), dtype=np.uint8)
