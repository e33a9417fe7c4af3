"""CPU model of the three screening tiers and of the re-rank's flag test (vsr_kernels.hip, rerank_body).

Shared passes screen every (row, query) pair with a cheap dot product, keep the kp best screening values per query and
re-rank those exactly.  A query is published only if no dropped row can beat its k-th exact result, i.e. only if
    a_last - err > d_k
with a_last the worst kept screening value, d_k the k-th exact value among the kept rows and err a bound on the
screening's error, built from g(d) (csrc/vsr_bounds.h):  |dot_s - dot| <= g |x| |q|.

    tier      screened dot                       g             err (flag test)                    kp
    "coarse"  xh . qh                 (K2g)      coarse_err_g  tight: g (|x|^2max + |q|^2) ...    max(4k, 128)
    "planes"  xh . qh + xh . qm + xm . qh (K2w)  plane_err_g   loose: 2 g (|x|^2max + |q|^2) ...  max(2k, 32)
    "k2"      x . q in fp32           (K2)       k2_err_g      loose                              max(2k, 32)

with xh = bf16(x), xm = bf16(x - xh), rounded to nearest even like the kernels' (__bf16) conversion.  Screening values
are modelled in float64 from the fp32 operands (the GPU's fp32 sums differ by a few ulp, far inside the margins the
constructions below leave).  The model assumes the kept list is full (bound = worst kept key), which the corpora built
here guarantee: every one has at least kp rows that screen better than the row it hides.
"""
import numpy as np

TIERS = ("coarse", "planes", "k2")
METRICS = ("l2", "ip", "cosine")


def old_g(tier, dim):
    """g(d) before the bf16 constants were re-derived (2^-9 per operand instead of 2^-8): what the self-checks defeat."""
    if tier == "coarse":
        return 3.9138794e-3 + (dim + 64) * 5.9604645e-8
    if tier == "planes":
        return 3.0 * 3.8146973e-6 + (3 * dim + 8) * 5.9604645e-8
    return (dim + 8) * 5.9604645e-8


def bf16(x):
    """fp32 -> bf16 (round to nearest, ties to even), returned as fp32.  Finite inputs only."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split(x):
    """The screening planes of vsr_kernels.hip (split8): hi = bf16(x), mid = bf16(x - hi) (x - hi exact in fp32)."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16(x)
    mid = bf16((x - hi).astype(np.float32))
    return hi, mid


def kp_of(tier, k):
    return max(4 * k, 128) if tier == "coarse" else max(2 * k, 32)


def tight(tier):
    return tier == "coarse"


def screened_dots(tier, X, q):
    """Screened dot products of every row of X with q (float64)."""
    X = np.asarray(X, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    if tier == "k2":
        return X.astype(np.float64) @ q.astype(np.float64)
    xh, xm = split(X)
    qh, qm = split(q)
    xh, xm, qh, qm = (a.astype(np.float64) for a in (xh, xm, qh, qm))
    if tier == "coarse":
        return xh @ qh
    return xh @ qh + xh @ qm + xm @ qh


def _values(metric, dot, nx, qn):
    if metric == "l2":
        return nx + qn - 2.0 * dot
    if metric == "ip":
        return -dot
    return 1.0 - dot / np.sqrt(nx * qn)


def screen_values(tier, metric, X, q):
    """The screening value per row (squared L2 for "l2", as the kernels rank by it)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    return _values(metric, screened_dots(tier, X, q), (X64 ** 2).sum(1), (q64 ** 2).sum())


def exact_values(metric, X, q):
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    return _values(metric, X64 @ q64, (X64 ** 2).sum(1), (q64 ** 2).sum())


def flag_err(tier, metric, g, nxm, qn, a_last=0.0):
    """`err` of rerank_body's flag test, restated (float64)."""
    if tight(tier):
        if metric == "l2":
            return g * (nxm + qn) * 1.0001 + 4e-6 * (nxm + qn)
        if metric == "ip":
            return g * np.sqrt(nxm * qn) * 1.0001 + 4e-6 * np.sqrt(nxm * qn)
        return g * 1.0001 + 4e-6
    if metric == "l2":
        return 2.0 * g * (nxm + qn) + g * abs(a_last)
    if metric == "ip":
        return 2.0 * g * np.sqrt(nxm * qn)
    return 8.0 * g


def screen(tier, metric, X, q, k, g):
    """One query through screen + keep + re-rank + flag test.  Returns (kept row indices in screening order, flagged,
    exact top-k row indices of the kept set)."""
    X = np.asarray(X, dtype=np.float32)
    kp = kp_of(tier, k)
    s = screen_values(tier, metric, X, q)
    e = exact_values(metric, X, q)
    order = np.lexsort((np.arange(len(s)), s))
    assert len(s) > kp, "the model assumes a full survivor list"
    kept = order[:kp]
    a_last = s[kept[-1]]
    ek = np.lexsort((kept, e[kept]))
    d_k = e[kept][ek[k - 1]]
    nxm = float((X.astype(np.float64) ** 2).sum(1).max())
    qn = float((np.asarray(q, dtype=np.float64) ** 2).sum())
    err = flag_err(tier, metric, g, nxm, qn, a_last)
    flagged = not (a_last - err > d_k)
    return kept, flagged, kept[ek[:k]]


# ---------------------------------------------------------------------------------------------------------------------
# Adversarial corpora.  Each returns (rows, query, k, hidden): `hidden` is a true top-k row (A) that the screen drops.
# Coordinates not named stay 0.  Every value is an integer or a dyadic number whose fp32 sums are exact in any order, so
# the exact tiers and the oracle agree bit for bit on every distance that reaches the top k.

def coarse_l2(dim, m=128, side=16, t=48, n_b1=10, n_b2=200):
    """q = A: 257 on m "hot" coordinates (bf16 rounds 257 down to 256: both operands of A . q lose 2^-8, the coarse
    screen's worst case).  B1: 258 there (bf16-exact; exact distance^2 m).  B2: also t on `side` coordinates where q is 0
    (exact distance^2 m + side t^2, worse than A and B1, but screened better than A).  A: screened 1026 m, exact 0."""
    assert m + side <= dim and t * t * side < 509 * m
    q = np.zeros(dim, np.float32)
    q[:m] = 257
    b1 = q.copy()
    b1[:m] = 258
    b2 = b1.copy()
    b2[m:m + side] = t
    rows = [q.copy()] + [b1] * n_b1 + [b2] * n_b2
    return np.stack(rows), q, 10, 0


def coarse_ip(dim, m=128, side=64, s0=64, n_b1=9, n_c=125):
    """q = A: 257 on m hot coordinates, s0 on `side` more.  B1 (k - 1 rows): 259 on the hot ones (bf16 rounds 259 up to
    260 and 257 down to 256: their screening errors cancel; exact dot 514 m above A's).  C: like B1 with the side
    coordinates lowered by T in total, s0 T in (514 m, 1024 m): exactly worse than A, screened better.  A is the true
    k-th result; the kept list is B1 and the best C rows, whose screening values spread over more than the old bound."""
    assert m + side <= dim
    q = np.zeros(dim, np.float32)
    q[:m] = 257
    q[m:m + side] = s0
    b1 = q.copy()
    b1[:m] = 259
    rows = [q.copy()] + [b1] * n_b1
    lo, hi = 1040, 2032                     # T: s0 T from 520 m .. 1016 m at m = 128, s0 = 64
    for T in np.linspace(lo, hi, n_c).round().astype(int):
        c = b1.copy()
        per, extra = divmod(int(T), side)
        c[m:m + side] -= per
        c[m:m + extra] -= 1
        rows.append(c)
    return np.stack(rows), q, n_b1 + 1, 0


def coarse_cosine(dim, m=128, side=64, s0=64, n_c=130):
    """q = A (cosine distance 0, screened ~1.93 2^-8 because both hot operands round down).  k = 1.  C: 259 on the hot
    coordinates (errors cancel) and the side coordinates lowered by T in total: exact distances from ~1e-4 up to ~7e-3, screened
    within a few 1e-6 of that, so a_last (the kp-th of them) sits more than the old bound above the best C."""
    q = np.zeros(dim, np.float32)
    q[:m] = 257
    q[m:m + side] = s0
    rows = [q.copy()]
    for j in range(n_c):
        c = q.copy()
        c[:m] = 259
        T = int(round(2800 * np.sqrt((j + 1) / 128)))       # spread over the side coordinates
        per, extra = divmod(T, side)
        c[m:m + side] -= per
        c[m:m + extra] -= 1
        rows.append(c)
    return np.stack(rows), q, 1, 0


WORST_PLANES = np.float32(1.0039136)      # x = q = this: hi + mid + e with xm qm and both residues adding up (7.83 2^-18)


def planes_l2(dim, n_b=64):
    """K2w, hi + mid planes, worst-case operands: q = A = WORST_PLANES on every coordinate.  B: q + j 2^-20 on every
    coordinate, j picked so that B's own split residue cancels q's (screened better than A), exact distance^2
    dim j^2 2^-40 (exact in fp32).  k = 10; n_b rows hide A behind kp = 32."""
    q = np.full(dim, WORST_PLANES, np.float32)
    a = np.float32(WORST_PLANES)
    cand = []
    s_a = float(screen_values("planes", "l2", q[None, :1], q[:1])[0])
    for j in (s * i for i in range(1, 400) for s in (-1, 1)):
        b = np.float32(a + np.float32(j * 2.0 ** -20))
        s_b = float(screen_values("planes", "l2", np.array([[b]], np.float32), q[:1])[0])
        if s_b < 0.5 * s_a:
            cand.append(b)
        if len(cand) == n_b:
            break
    assert len(cand) == n_b
    rows = [q.copy()] + [np.full(dim, b, np.float32) for b in cand]
    return np.stack(rows), q, 10, 0


def planes_ip(dim, n_b1=9):
    """K2w IP: 257 = 256 + 1 splits exactly (hi 256, mid 1), so A . q is screened m (= xm qm summed) below its value.
    q = A: 257 on m hot coordinates, 1 on `side` more.  B1: one side coordinate 2 (exactly better than A).  C: half the
    hot coordinates 258, half 256 (bf16-exact, screened without error; dot equal to A's) and delta in 1 .. side of the
    side coordinates 0: exactly worse than A by delta, screened better.  Every sum is an integer below 2^24."""
    m, side = dim // 2, min(dim // 2 - 1, 63)
    q = np.zeros(dim, np.float32)
    q[:m] = 257
    q[m:m + side] = 1
    b1 = q.copy()
    b1[m] = 2
    rows = [q.copy()] + [b1] * n_b1
    for delta in range(1, side + 1):
        c = q.copy()
        c[:m // 2] = 258
        c[m // 2:m] = 256
        c[m:m + delta] = 0
        rows.append(c)
    return np.stack(rows), q, n_b1 + 1, 0


def offset_rows(rng, n, dim, base, r_max=15):
    """Rows base + r (r a small integer): differences and squared L2 distances exact, |x|^2 cancels heavily in the
    screen, and the values are neither bf16-exact (for base 4096) nor 0..255."""
    return (base + rng.integers(0, r_max + 1, (n, dim))).astype(np.float32)
