"""The project's IVFFlat k-means (vsr_kmeans.hip; oracle/vsr_index_oracle.c orc_ivf_kmeans; pgvector ivfkmeans.c:21-93 InitCenters,
:192-246 ComputeNewCenters, :259-498 ElkanKmeans) restated in numpy, with the one switch the halfvec build adds: `round_half`
rounds every value stored into a centre to binary16 and widens it again (HalfvecUpdateCenter, ivfutils.c:266-276;
halfvec_l2_normalize, halfvec.c:712-744).

What is kept so that the result is the C code's bit for bit:
  * the xorshift64* stream and its seeding (python ints, 64-bit wrap-around);
  * the k-means++ sweep (float32 running minimum of the squared double distance) and the weighted draw (one running double that
    walks the samples: np.subtract.accumulate is sequential);
  * Elkan's bound tests in centre order: a loop over the centres, vectorised over the samples with masks -- samples are
    independent of each other within an assignment step;
  * distances: float32 terms added in element order without contraction (a loop over the dimensions), sqrt / acos in double;
  * new centres: float32 sums in sample order (np.cumsum in float32 is a sequential accumulate, np.sum is pairwise);
  * the empty-centre fill in centre order, element order (the stream is serial).
With the switch off, tests/test_ivf_half_cpu.py pins this file to orc_ivf_kmeans; that licenses it as the expectation of
vsr_ivf_kmeans_half with the switch on."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
MASK = (1 << 64) - 1
F32 = np.float32


class Rng:
    def __init__(self, seed):
        self.s = (int(seed) * 0x9E3779B97F4A7C15 + 0x1234567) & MASK
        if not self.s:
            self.s = 1
        self.next()

    def next(self):
        x = self.s
        x ^= x >> 12
        x ^= (x << 25) & MASK
        x ^= x >> 27
        self.s = x
        return (x * 0x2545F4914F6CDD1D) & MASK

    def double(self):
        return float(self.next() >> 11) * (1.0 / 9007199254740992.0)


def round_to_half(v):
    """float32 -> binary16 (round to nearest even, overflow to +-Inf: Float4ToHalfUnchecked) -> float32"""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=F32).astype(np.float16).astype(F32)


def distance(metric, a, b):
    """The k-means distance of rows a[i] to rows b[i] (or to one row b), float64: l2_distance / vector_spherical_distance."""
    a = np.atleast_2d(np.asarray(a, dtype=F32))
    b = np.broadcast_to(np.asarray(b, dtype=F32), a.shape)
    s = np.zeros(a.shape[0], dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == "l2":
            for j in range(a.shape[1]):
                d = a[:, j] - b[:, j]
                s = s + d * d
            return np.sqrt(s.astype(np.float64))
        for j in range(a.shape[1]):
            s = s + a[:, j] * b[:, j]
        d = s.astype(np.float64)
        d = np.where(d > 1, 1.0, np.where(d < -1, -1.0, d))
        return np.arccos(d) / np.pi


def norm_center(c, round_half):
    """l2_normalize / halfvec_l2_normalize of one centre; a centre that would overflow stays as it is."""
    c = np.asarray(c, dtype=F32)
    norm = 0.0
    for v in c.astype(np.float64):
        norm += v * v
    norm = np.sqrt(norm)
    if not norm > 0:
        return np.zeros_like(c)
    with np.errstate(over="ignore"):
        r = (c.astype(np.float64) / norm).astype(F32)
    if round_half:
        r = round_to_half(r)
    return c if np.isinf(r).any() else r


def kmeans(samples, lists, seed, metric="l2", round_half=False):
    """centres [lists][dim] float32 (binary16 values when round_half), Elkan iterations run."""
    x = np.ascontiguousarray(samples, dtype=F32)
    ns, dim = x.shape if x.size else (0, x.shape[1])
    nc = int(lists)
    rng = Rng(seed)
    store = round_to_half if round_half else (lambda v: np.asarray(v, dtype=F32))
    if ns == 0:                                                  # RandomCenters
        c = store(np.array([F32(rng.double()) for _ in range(nc * dim)], dtype=F32)).reshape(nc, dim)
        if metric != "l2":
            c = np.stack([norm_center(c[j], round_half) for j in range(nc)])
        return c, 0
    centers = np.zeros((nc, dim), dtype=F32)
    lower = np.zeros((ns, nc), dtype=F32)
    # InitCenters (k-means++)
    centers[0] = x[rng.next() % ns]
    weight = np.full(ns, FLT_MAX, dtype=F32)
    for i in range(nc):
        d = distance(metric, x, centers[i])
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
            d = (0.5 * distance(metric, centers[j + 1:], centers[j])).astype(F32)
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
                d = distance(metric, x[fresh], centers[closest[fresh]]).astype(F32)
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
            dxc = distance(metric, x[idx], centers[c]).astype(F32)
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
                    newc[c] = store(v / F32(counts[c]))
                else:
                    newc[c] = store(np.array([F32(rng.double()) for _ in range(dim)], dtype=F32))
                if metric != "l2":
                    newc[c] = norm_center(newc[c], round_half)
            newcdist = distance(metric, centers, newc).astype(F32)
            d = lower - newcdist[None, :]
            lower = np.where(d < 0, F32(0), d).astype(F32)
            upper = (upper + newcdist[closest]).astype(F32)
        centers = newc
        iterations = iteration + 1
        if changes == 0 and iteration != 0:
            break
    return centers, iterations


def integer_case(seed=5, ns=1500, dim=8, lists=6):
    """1500 x 8 integer-valued samples (binary16 values), 6 lists."""
    rng = np.random.default_rng(seed)
    blobs = rng.integers(4, 28, (lists, dim))
    x = blobs[rng.integers(0, lists, ns)] + rng.integers(-3, 4, (ns, dim))
    return x.astype(F32), lists


def repeated_case(seed=6, distinct=40, copies=5, dim=8, lists=48):
    """40 distinct samples, each 5 times, and 48 lists: at least 8 centres own no sample in every iteration, so the
    empty-centre fill runs (and, after the 40th draw, the weighted draw over weights that are all zero)."""
    rng = np.random.default_rng(seed)
    base = np.unique(rng.integers(0, 32, (4 * distinct, dim)), axis=0)
    base = base[rng.permutation(len(base))[:distinct]]
    assert len(base) == distinct
    x = np.tile(base, (copies, 1))
    return x[rng.permutation(len(x))].astype(F32), lists
