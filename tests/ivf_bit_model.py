"""IVFFlat over bit strings (pgvector's ivfflat bit_hamming_ops: ivfutils.c:248-252, 278-292, 316-323, 364-377 and ivfkmeans.c)
restated in numpy -- the expectation of vsr_ivf_kmeans_bit / vsr_ivf_assign_bit / vsr_ivf_load_bit / vsr_ivf_probe_bit /
vsr_ivf_search_bit* (tests/test_gpu_ivf_bit.py, tests/test_gpu_ivf_bit_iterative.py), licensed by tests/test_ivf_bit_cpu.py.

  * Centre order: (Hamming count, list id), the lower list id first among equals; the assignment is its first entry.
  * Rows inside the probed lists: bit_model's ((float) Hamming count, document_id, block_id).
  * Iterative stream: ivf_iterative_model.batch_bounds over the centre order, every batch a filtered top-k of what is still
    wanted, batches concatenated and never re-sorted.
  * k-means: the skeleton of ivf_half_model.kmeans -- the same stream, seeding, weighted draw, bound tests in centre order,
    500-iteration limit and stop -- with its two type-specific pieces as arguments: `distance(a, b)` (float64 per row of a) and
    `update(x)` (the fp32 vector the reference hands to updateCenter -> the centre's elements).  With ivf_half_model's L2 distance
    and the identity it is orc_ivf_kmeans bit for bit (pinned by test_ivf_bit_cpu.py); the bit opclass substitutes
        distance = the Hamming count as a double (hamming_distance),
        update   = x > 0.5 (BitUpdateCenter) on x = fp32 member-bit sums / fp32 member count (BitSumCenter, ComputeNewCenters),
    and an empty centre -- or every centre when there is no sample -- gets x[i] = (float) RandomDouble() in (centre, element)
    order and the same update.  Samples and centres are 0 / 1 float32 arrays inside; packed uint8 outside."""
import numpy as np

import bit_model
from ivf_half_model import FLT_MAX, F32, Rng
from ivf_iterative_model import batch_bounds


# ---- k-means ------------------------------------------------------------------------------------------------------------------
def kmeans_skeleton(samples, lists, seed, distance, update):
    """centres [lists][dim] float32, Elkan iterations run."""
    x = np.ascontiguousarray(samples, dtype=F32)
    ns, dim = x.shape if x.size else (0, x.shape[1])
    nc = int(lists)
    rng = Rng(seed)

    def random_center():
        return update(np.array([F32(rng.double()) for _ in range(dim)], dtype=F32))

    if ns == 0:                                                  # RandomCenters
        return np.stack([random_center() for _ in range(nc)]).astype(F32), 0
    centers = np.zeros((nc, dim), dtype=F32)
    lower = np.zeros((ns, nc), dtype=F32)
    # InitCenters (k-means++)
    centers[0] = x[rng.next() % ns]
    weight = np.full(ns, FLT_MAX, dtype=F32)
    for i in range(nc):
        d = distance(x, centers[i])
        lower[:, i] = d.astype(F32)
        d = d * d
        closer = d < weight.astype(np.float64)
        weight[closer] = d[closer].astype(F32)
        if i + 1 == nc:
            break
        total = np.cumsum(weight.astype(np.float64))[-1]
        choice = total * rng.double()
        walk = np.subtract.accumulate(np.concatenate([[choice], weight[:ns - 1].astype(np.float64)]))[1:]
        hit = np.nonzero(walk <= 0)[0]
        centers[i + 1] = x[int(hit[0]) if hit.size else ns - 1]
    closest = np.zeros(ns, dtype=np.int64)
    upper = np.full(ns, FLT_MAX, dtype=F32)
    for c in range(nc):                                          # the first strict minimum
        better = lower[:, c] < upper
        upper[better] = lower[better, c]
        closest[better] = c
    rows = np.arange(ns)
    iterations = 0
    for iteration in range(500):
        changes = 0
        half = np.zeros((nc, nc), dtype=F32)
        for j in range(nc - 1):
            d = (0.5 * distance(centers[j + 1:], centers[j])).astype(F32)
            half[j, j + 1:] = d
            half[j + 1:, j] = d
        off = np.where(np.eye(nc, dtype=bool), FLT_MAX, half)   # (a value >= FLT_MAX never lowers the minimum)
        s = np.full(nc, FLT_MAX, dtype=F32)
        for c in range(nc):
            better = off[:, c] < s
            s[better] = off[better, c]
        active = ~(upper <= s[closest])
        rj = np.full(ns, iteration != 0)
        for c in range(nc):
            m = active & (closest != c) & ~(upper <= lower[:, c]) & ~(upper <= half[closest, c])
            fresh = np.nonzero(m & rj)[0]
            if fresh.size:
                d = distance(x[fresh], centers[closest[fresh]]).astype(F32)
                lower[fresh, closest[fresh]] = d
                upper[fresh] = d
                rj[fresh] = False
            idx = np.nonzero(m)[0]
            if not idx.size:
                continue
            dxcx = upper[idx]
            need = (dxcx > lower[idx, c]) | (dxcx > half[closest[idx], c])
            idx, dxcx = idx[need], dxcx[need]
            if not idx.size:
                continue
            dxc = distance(x[idx], centers[c]).astype(F32)
            lower[idx, c] = dxc
            won = dxc < dxcx
            closest[idx[won]] = c
            upper[idx[won]] = dxc[won]
            changes += int(won.sum())
        # ComputeNewCenters
        newc = np.zeros((nc, dim), dtype=F32)
        counts = np.bincount(closest, minlength=nc)
        with np.errstate(over="ignore", invalid="ignore"):
            for c in range(nc):
                if counts[c] > 0:
                    v = np.cumsum(x[rows[closest == c]], axis=0, dtype=F32)[-1]
                    v = np.where(np.isinf(v), np.where(v > 0, FLT_MAX, -FLT_MAX), v).astype(F32)
                    newc[c] = update((v / F32(counts[c])).astype(F32))
                else:
                    newc[c] = random_center()
            newcdist = distance(centers, newc).astype(F32)
            d = lower - newcdist[None, :]
            lower = np.where(d < 0, F32(0), d).astype(F32)
            upper = (upper + newcdist[closest]).astype(F32)
        centers = newc
        iterations = iteration + 1
        if changes == 0 and iteration != 0:
            break
    return centers, iterations


def identity_update(x):
    return np.asarray(x, dtype=F32)


def hamming_distance(a, b):
    """hamming_distance of 0 / 1 rows a[i] against rows b[i] (or one row b): the count of differing positions, float64."""
    a = np.atleast_2d(np.asarray(a, dtype=F32))
    b = np.broadcast_to(np.asarray(b, dtype=F32), a.shape)
    return (a != b).sum(axis=1).astype(np.float64)


def bit_update(x):
    """BitUpdateCenter: bit i = x[i] > 0.5, on the fp32 vector."""
    return (np.asarray(x, dtype=F32) > F32(0.5)).astype(F32)


def kmeans(samples, dim, lists, seed):
    """vsr_ivf_kmeans_bit: packed samples [n, (dim + 7) // 8] (pad bits ignored) -> packed centres [lists, (dim + 7) // 8] with
    clear pad bits, Elkan iterations run."""
    x = bit_model.unpack(samples, dim).astype(F32) if len(samples) else np.zeros((0, dim), dtype=F32)
    centers, iterations = kmeans_skeleton(x, lists, seed, hamming_distance, bit_update)
    assert ((centers == 0) | (centers == 1)).all()
    return bit_model.pack(centers.astype(bool)), iterations


# ---- the index ----------------------------------------------------------------------------------------------------------------
def center_counts(centers, queries, dim):
    """Hamming counts [nq, lists] (int64) of packed queries against packed centres; pad bits never count."""
    c = bit_model.unpack(centers, dim).astype(F32)
    q = bit_model.unpack(queries, dim).astype(F32)
    ab = (q @ c.T).astype(np.int64)                              # integers < 2^24: exact in fp32
    return q.sum(axis=1, dtype=np.int64)[:, None] + c.sum(axis=1, dtype=np.int64)[None, :] - 2 * ab


def center_order(centers, queries, dim):
    """list ids [nq, lists] by (Hamming count, list id)."""
    return np.argsort(center_counts(centers, queries, dim), axis=1, kind="stable")


class IvfBit:
    """The index over given centres: rows packed [n, bytes] in caller order, identity arrays, the assignment."""

    def __init__(self, rows, dim, centers, doc=None, blk=None):
        self.dim, self.lists = dim, len(centers)
        self.rows, self.centers = np.asarray(rows, dtype=np.uint8), np.asarray(centers, dtype=np.uint8)
        self.bm = bit_model.BitModel(self.rows, dim, doc, blk)
        n = len(self.rows)
        self._dist = {}
        self.assign = np.zeros(n, dtype=np.int32)
        for lo in range(0, n, 4096):                             # (row, centre) pairs: the probe's key, first entry of the order
            self.assign[lo:lo + 4096] = center_order(self.centers, self.rows[lo:lo + 4096], dim)[:, 0]

    def probe(self, q, probes):
        return center_order(self.centers, np.atleast_2d(q), self.dim)[0, :min(int(probes), self.lists)].astype(np.int32)

    def _topk(self, q, k, lists, mask):
        sel = np.isin(self.assign, lists)
        if mask is not None:
            sel &= np.asarray(mask, dtype=bool)
        key = np.asarray(q, dtype=np.uint8).tobytes()            # a query's distances to every row, computed once
        if key not in self._dist:
            self._dist[key] = self.bm.distances("hamming", np.atleast_2d(q))[0]
        return self.bm.topk(self._dist[key], k, sel)

    def search(self, q, k, probes, mask=None):
        """(caller rows, float32 Hamming counts) of the k nearest permitted rows of the probed lists."""
        return self._topk(q, k, self.probe(q, probes), mask)

    def iterative(self, q, k, probes, max_probes, mask=None):
        """rows, float32 distances, lists scanned (so->listIndex): ivf_iterative_model.iterative_search over this index."""
        m = min(max(int(max_probes), int(probes)), self.lists)
        order = self.probe(q, m)
        rows, dist, scanned = [], [], 0
        for lo, hi in batch_bounds(probes, max_probes, self.lists):
            have = sum(len(r) for r in rows)
            if have >= k:
                break
            r, d = self._topk(q, k - have, order[lo:hi], mask)
            rows.append(r)
            dist.append(d)
            scanned = hi
        return (np.concatenate(rows) if rows else np.zeros(0, np.int64),
                np.concatenate(dist) if dist else np.zeros(0, np.float32), scanned)


class BitFixture:
    """The fixture the GPU tests of the bit index share: n x dim sparse bit rows (a fifth of the bits set), documents of 10 rows,
    user 1 sees ~2 % of the documents, user 2 a quarter, user 3 none.  `lists` centres: rows with a few bits flipped, two of them
    identical (twin: the second owns no row), and 4 all-ones centres far from every row, so some lists stay empty.  The first ten
    rows are copies of one row spread over several documents."""

    def __init__(self, n, dim, lists, nq, seed, twin=True):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.lists = n, dim, lists
        bits = rng.random((n, dim)) < 0.2
        bits[:10] = bits[3]
        self.doc = (np.arange(n) // 10 + 1).astype(np.int32)
        self.doc[:10] = np.array([5, 3, 3, 9, 1, 9, 2, 2, 7, 1], dtype=np.int32)      # copies in several documents, out of order
        self.blk = (np.arange(n) + 1).astype(np.int64)
        ndocs = int(self.doc.max())
        docs = np.arange(1, ndocs + 1)
        self.perms = [(1, int(d)) for d in rng.choice(docs, max(ndocs // 50, 2), replace=False)] + \
                     [(2, int(d)) for d in rng.choice(docs, ndocs // 4, replace=False)]
        self.user_roles = [(1, 1), (2, 2), (3, 3)]
        far = 4
        cbits = bits[np.sort(rng.choice(n, lists - far, replace=False))] ^ (rng.random((lists - far, dim)) < 3.0 / dim)
        cbits = np.concatenate([cbits, np.ones((far, dim), dtype=bool)])
        self.twin = 11 if lists > 16 else 2
        cbits[0] = bits[3]                                      # the copies' own centre ...
        if twin:
            cbits[self.twin] = cbits[0]                         # ... twice: list 0 takes them, its twin stays empty
        self.rows = bit_model.set_pad_bits(bit_model.pack(bits), dim)
        self.centers = bit_model.set_pad_bits(bit_model.pack(cbits), dim)
        self.m = IvfBit(self.rows, dim, self.centers, self.doc, self.blk)
        assert len(set(self.m.assign.tolist())) <= lists - far - (1 if twin else 0)
        assert not twin or not (self.m.assign == self.twin).any()
        self.masks = {u: bit_model.user_row_mask(u, self.user_roles, self.perms, self.doc) for u in (1, 2, 3)}
        self.masks[None] = None
        qbits = bits[rng.integers(0, n, nq)] ^ (rng.random((nq, dim)) < 0.02)
        qbits[0] = bits[3]                                      # ten rows at distance 0, and two centres at distance 0
        self.q = bit_model.set_pad_bits(bit_model.pack(qbits), dim)
        self.users = rng.integers(1, 3, nq)
