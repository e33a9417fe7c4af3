"""Cases shared by the CPU and GPU tests of HNSW over halfvec corpora (K4h: vsr_hnsw_load_half / vsr_hnsw_build_half).

pgvector computes every halfvec distance on the widened operands (halfutils.c), so the index oracle's serial build and walk on
the WIDENED fp32 rows, asked with the query ROUNDED to binary16, is pgvector's halfvec build and walk.  On integer-valued rows
(small integers: exactly representable, every sum below 2^24) the fp32 sums do not depend on the order of summation, so rows,
distances and visited counts of the GPU walk must be identical to the oracle's, not close."""
import json
import os

import numpy as np


def to_half(x):
    """Float4ToHalf: round to nearest even (numpy's float32 -> float16 conversion)."""
    return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16)


def widen(h):
    return np.asarray(h, dtype=np.float16).astype(np.float32)


def round_query(q):
    """What `$1::halfvec` holds, as fp32."""
    return widen(to_half(q))


def int_rows(rng, n, dim, planted=100, copies=40):
    """Integer-valued rows in -8 .. 8 with `copies` exact copies of row `planted` at n // 2 (elements of 10 TIDs in a serial build)."""
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    x[n // 2:n // 2 + copies] = x[planted]
    return x


def int_queries(rng, x, nq, planted=100):
    """Integer-valued queries near rows of x; query 0 is the planted row."""
    q = x[rng.integers(0, len(x), nq)] + rng.integers(-2, 3, (nq, x.shape[1])).astype(np.float32)
    q[0] = x[planted]
    return q


def want_dist(metric, d):
    """The distance vsr_hnsw_search reports for index distance d (float8 of the oracle)."""
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt(d).astype(np.float32) if metric == "l2" else d.astype(np.float32)


# ---- the query-rounding case ---------------------------------------------------------------------------------------------
ROUNDING_N, ROUNDING_DIM, ROUNDING_SEED, ROUNDING_NQ = 3000, 16, 316, 16


def rounding_case():
    """(rows, raw queries, their rounded copies): every non-zero element of a raw query is x + 2**-12 for a small integer x --
    not a binary16 value, it rounds to x -- and the first half of the queries carry 2049 in element 3, which rounds to 2048."""
    rng = np.random.default_rng(ROUNDING_SEED)
    x = int_rows(rng, ROUNDING_N, ROUNDING_DIM)
    base = int_queries(rng, x, ROUNDING_NQ)
    raw = base.copy()
    raw[base != 0] += np.float32(2.0 ** -12)
    raw[:ROUNDING_NQ // 2, 3] = 2049.0
    return x, raw, round_query(raw)


# ---- 024_hnsw_halfvec_build_recall.pl ------------------------------------------------------------------------------------
TAP_SEEDS = {"l2": 2401, "ip": 2402, "cosine": 2403}
TAP_LIMIT, TAP_EF = 20, 40


def tap_case(metric):
    """10 000 x 10 rows `2 * random() * random()` as halfvec, 20 queries `random()`; cosine: unit rows and queries (the rows
    rounded to binary16 after normalization, as a halfvec column of unit vectors holds them).  Returns (rows float16,
    queries float32)."""
    rng = np.random.default_rng(TAP_SEEDS[metric])
    x = (2.0 * rng.random((10_000, 10)) * rng.random((10_000, 10))).astype(np.float32)
    q = rng.random((20, 10)).astype(np.float32)
    if metric == "cosine":
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return to_half(x), q


def exact_order(metric, rows_half, q):
    """Row indices nearest first in the type's arithmetic (operands widened, the query rounded), evaluated in float64."""
    x = widen(rows_half).astype(np.float64)
    qq = round_query(q).astype(np.float64)
    if metric == "l2":
        d = ((x - qq) ** 2).sum(axis=1)
    elif metric == "ip":
        d = -(x @ qq)
    else:
        d = 1.0 - (x @ qq) / np.maximum(np.linalg.norm(x, axis=1) * np.linalg.norm(qq), 1e-300)
    return np.argsort(d, kind="stable"), d


def recall(found, expected):
    hit = sum(len(set(np.asarray(f).tolist()) & set(np.asarray(e).tolist())) for f, e in zip(found, expected))
    return hit / sum(len(e) for e in expected)


def known_answers(golden_dir):
    return json.load(open(os.path.join(golden_dir, "pgvector_hnsw_halfvec_known_answers.json")))["cases"]


def known_answer_rows(case):
    """(rows as the index holds them, their original values): cosine keeps the non-zero rows, normalized."""
    rows = np.array(case["rows"], dtype=np.float32)
    if case["metric"] == "cosine":
        keep = np.linalg.norm(rows, axis=1) > 0
        orig = rows[keep]
        return orig / np.linalg.norm(orig, axis=1, keepdims=True), orig
    return rows, rows
