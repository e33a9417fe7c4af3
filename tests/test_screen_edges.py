"""The inexact screening tiers -- bf16 planes (K2w), coarse bf16 planes (K2g), fp32 MFMA (K2) and f16 MFMA (K2h) -- at the
list-length edges of their final selection and of rerank_body's flag decision (vsr_kernels.hip), on the edge worlds of
tests/edge_world.py.  test_gpu_select_wave.py drives the same edges for the int8 planes, whose survivor list is max(k, 32)
long; here it is kp = max(2k, 32) (K2w / K2 / K2h) or max(4k, 128) (K2g), so the classes below add kp - 1, kp and kp + 1.

Worlds (all integer valued; World.exact_bound asserts that every partial sum stays below 2^24, so the oracle is order
independent and everything is compared bit for bit):
  W128    d = 128, sift_like rows, test_gpu_select_wave.py's classes plus 31 / 32 / 33, 199 / 200 / 201, 258 / 259: for every
          k of KS = 1, 10, 100, 128, 129, 256 the allowed counts k - 1, k, k + 1 and kp - 1, kp, kp + 1, next to 1, 1023 / 1024 /
          1025 (one round of wave_select_stream<16> short, full, one key over), 16 384 = GQ_CAP and 40 001 (seeded).
  Wdeep   d = 128, allowed counts 1791 .. 1793, 2047 .. 2049, 3583 .. 3585 and 9000, 16 or 17 queries each: k = 257, 512 and
          1792 run on K2 / K2h (kp = 3584 = the last mfma_cap_for_k(kp) <= 8192), k = 1793 and 2048 on K1m / K1h.
  Wcoarse d = 320, integers -15 .. 15 (exact in bf16: the coarse screen's products are exact), allowed counts 99 .. 101 and
          kp - 1, kp, kp + 1 of kp = max(4k, 128) for k = 1, 32, 100, 128, and one class past GQ_CAP; every class is asked by at
          least 130 queries (K2g's gate: parts seen by more than 128 queries).  The big class has 60 001 rows, not ~20 000: next
          to the one-tile classes its queries need a seed of rank m = kp + 6 sqrt(kp) + 4 = 652 at kp = 512, from a sample
          of at least 1.25 m + 8 entries (evaluate_stride); K2g's sample has 8 entries per 256-row tile, every second tile at
          the densest stride, so 20 001 rows (~750 entries if every tile were sampled) send k = 100 and 128 to K2w instead.
          One of the two classes of 513 rows is 512 copies of ONE vector: its k-th and kp-th values are equal, no screen can
          prove such a query, and the model flags its user's queries (7 % of all) on every tier -- the flagged half of the
          count encoding, screening_check and the re-run ladder run on them.

The CPU tests pin the inputs: the allowed counts sit on the edges, ties straddle every k, and the CPU model of the flag
test (screening_model.py, g from the compiled csrc/vsr_bounds.h, |x|^2 max over the whole corpus) flags no query of W128
and Wdeep on any tier and at most a tenth of Wcoarse's, with no margin close enough to zero for fp32 to flip it.

The GPU tests run every tier on a fresh context opened (and its corpus loaded) under the tier's switches, in calls of 1, 3
and all queries, through vsr_search (bit-exact: rows, order, fp32 distances, ids, counts, padding) and vsr_search_device
(a published query is bit-exact; a flagged one carries -1 - count and shows in screening_check; vsr_search_device_exact
then makes the batch exact and returns how many it re-ran; where the tier's kernel ran, the flagged queries with
allowed >= kp are exactly the model's).

Queries with allowed < kp have a survivor list that is not full, so rerank_body has a bound only if the query was seeded:
  * K2 / K2h (search_general) seed only from plan.scan_rows >= seed_min_rows = 2 000 000 pass-rows; these worlds stay far
    below, so tau_init is never set and such a query can never be flagged: asserted in every call.
  * K2w / K2g: the seed is the m-th smallest sample entry, m = seed_rank_of(kp_frac), kp_frac = kp x the densest pass's
    sampling fraction (vsr_plan.hip, evaluate_stride).  In a call of all queries the root class is a pass of its own whose
    single tile is sampled whole, so the fraction is 1 and m = kp + 6 sqrt(kp) + 4 > kp > allowed >= the query's sample
    entries: never seeded, never flagged -- asserted for the calls of all queries.  In the calls of 1 and 3 queries the
    passes are the users' own filters, the fraction can be below 1, and a seed -- then a sound flag -- is possible: only
    the two soundness rules are asserted there.

Zero inner products: keys canonicalise -0 to +0 (vsr_topk.h, mono_bits), so a zero <#> distance comes back as +0.0 where
vector.c's -(0.0f) and the oracle have -0.0 (Wcoarse's signed rows produce a few; every kernel reports distances out of its
keys, the exact ones too).  PostgreSQL compares the two equal.  The distances are compared bit for bit with the oracle's after
that one mapping: a zero must come back as +0.0, everything else as the oracle's bits.

Kernel names observed on an MI355X (last_scan_kernel, call of all queries):
  W128    hi-only, IP and L2 under VSR_NO_INT8, k <= 256: mfma_wide_kernel<.., NCH=1, SAMPLE=false, HO=true> (K2w, bf16 hi-only
          planes) + select vsr::select_rerank_kernel; under VSR_NO_HIONLY: ..<NCH=2, .., HO=false> (K2w, bf16 hi+mid planes);
          k = 257: mfma_scan_kernel<.., NSTR=4, SAMPLE=false, NG=1> (K2); under VSR_NO_WIDE every k on (K2); halfvec:
          mfmah_scan_kernel<.., NSTR=1, SAMPLE=false, NG=1> (K2h, half rows)
  Wdeep   k = 257, 512, 1792: (K2) / (K2h, half rows); k = 1793, 2048: mq_scan_kernel<.., SAMPLE=false> (K1m) /
          scan_kernel<.., LPR=16, C=1, R=8, QI=1, HALF=true> (K1h, half rows)
  Wcoarse k = 1, 32, 100, 128: gemm_screen_kernel<.., SAMPLE=false> (K2g, bf16 coarse planes) + select vsr::select_rerank_kernel;
          k = 129: mfma_wide_kernel<.., NCH=3, SAMPLE=false, HO=true> (K2w, bf16 hi-only planes)
The calls of 1 and 3 queries mostly run K1 / K1h (scan_kernel, one query per pass; a single query: + in-kernel merge).
"""
import contextlib
import ctypes
import hashlib
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import screening_model as sm
from edge_world import CLASSES, World, small_signed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")

GQ_CAP = 16384
GQ_MAX_KP = 512
KS = (1, 10, 100, 128, 129, 256)
W128_CLASSES = CLASSES[:-1] + ((31, 1), (32, 15), (33, 16), (199, 17), (200, 64), (201, 65), (258, 16), (259, 17)) + CLASSES[-1:]
DEEP_KS = (257, 512, 1792, 1793, 2048)
DEEP_K2_MAX = 1792                                                     # mfma_cap_for_k(2k) <= 8192
DEEP_CLASSES = ((1791, 16), (1792, 17), (1793, 16), (2047, 17), (2048, 16), (2049, 17), (3583, 16), (3584, 17), (3585, 16),
                (9000, 17), (1, 1))
COARSE_KS = (1, 32, 100, 128)
COARSE_CLASSES = ((99, 130), (100, 131), (101, 130), (127, 130), (128, 144), (129, 130), (399, 130), (400, 257), (401, 130),
                  (511, 130), (512, 145), (513, 130), (513, 130), (60001, 130), (1, 1))
COARSE_CLONES = 12                                                     # the second class of 513: all its rows are one vector
METRICS = ("l2", "ip")
FINE = {"VSR_MIN_ROWS_PER_BLOCK": "16", "VSR_MIN_SHARED_ROWS": "64"}

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "vsr_bounds.h"
int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        const int d = atoi(argv[i]);
        printf("%d %.9g %.9g %.9g %.9g\n", d, (double) coarse_err_g(d), (double) plane_err_g(d), (double) k2_err_g(d), (double) half_err_g(d));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def g_of(tmp_path_factory):
    """g(tier, d) of csrc/vsr_bounds.h, compiled on its own as in test_screening_bounds_cpu.py; "half": half_err_g."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("edge_bounds")
    src, exe = d / "g.cpp", d / "g"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)])
    table = {}
    for line in subprocess.check_output([str(exe), "128", "320"], text=True).split("\n"):
        if line.strip():
            f = line.split()
            table[int(f[0])] = dict(zip(("coarse", "planes", "k2", "half"), map(float, f[1:])))
    return lambda tier, dim: table[dim][tier]


@pytest.fixture(scope="module")
def w128():
    return World(W128_CLASSES)


@pytest.fixture(scope="module")
def wdeep():
    return World(DEEP_CLASSES, seed=20261020, k_ref=max(DEEP_KS) + 2)


@pytest.fixture(scope="module")
def wcoarse():
    w = World(COARSE_CLASSES, d=320, seed=20261021, rows=small_signed, q_range=(-15, 16), k_ref=131)
    rows = np.flatnonzero(np.repeat(w.doc_class, w.doc_rows) == COARSE_CLONES)
    w.x[rows] = w.x[rows[0]]                                               # k-th and kp-th value equal: no screen can prove these
    return w


# ---------------------------------------------------------------------------------------------------------------------
# the CPU model of the flag test, per world: screening_model.py's arithmetic, a class's queries at a time
# ---------------------------------------------------------------------------------------------------------------------
_VERDICTS = {}


def _screened(tier, X, Q):
    """Screened and exact dot products (float64), rows x queries."""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    exact = X64 @ Q64.T
    if tier == "k2":
        return exact, exact
    xh, xm = (a.astype(np.float64) for a in sm.split(X))
    qh, qm = (a.astype(np.float64) for a in sm.split(Q))
    if tier == "coarse":
        return xh @ qh.T, exact
    return xh @ qh.T + xh @ qm.T + xm @ qh.T, exact


def verdicts(oracle, w, tier, metric, g, ks):
    """{k: (flagged, margin, err)} over the world's queries: rerank_body's test on a full survivor list, restated.  margin =
    a_last - err - d_k; a query with fewer than kp allowed rows has no verdict (not flagged, margin and err NaN).  tier
    "k2" with another g serves K2h (half_err_g)."""
    key = (id(w), tier, metric, float(g), tuple(ks))
    if key in _VERDICTS:
        return _VERDICTS[key]
    out = {k: (np.zeros(w.nq, bool), np.full(w.nq, np.nan), np.full(w.nq, np.nan)) for k in ks}
    nxm = float((w.x.astype(np.float64) ** 2).sum(1).max())                  # norm2_max: over the whole corpus
    for user in np.unique(w.quser):
        rows = w.allowed_rows(oracle, int(user))
        qs = np.flatnonzero(w.quser == user)
        if all(rows.size < sm.kp_of(tier, k) for k in ks):
            continue
        X, Q = w.x[rows], np.stack([w.rq(w.q[i]) for i in qs])
        dot_s, dot = _screened(tier, X, Q)
        nx = (X.astype(np.float64) ** 2).sum(1)[:, None]
        qn = (Q.astype(np.float64) ** 2).sum(1)
        s, e = sm._values(metric, dot_s, nx, qn[None, :]), sm._values(metric, dot, nx, qn[None, :])
        kp_max = min(rows.size, max(sm.kp_of(tier, k) for k in ks))
        for j, i in enumerate(qs):
            col = s[:, j]                                                  # the kp_max best by (value, row), as the keys order them
            cand = np.flatnonzero(col <= np.partition(col, kp_max - 1)[kp_max - 1])
            order = cand[np.argsort(col[cand], kind="stable")]
            for k in ks:
                kp = sm.kp_of(tier, k)
                if rows.size < kp:
                    continue
                kept = order[:kp]
                a_last = s[kept[-1], j]
                d_k = np.partition(e[kept, j], k - 1)[k - 1]
                err = sm.flag_err(tier, metric, g, nxm, qn[j], a_last)
                flagged, margin, errs = out[k]
                margin[i], errs[i] = a_last - err - d_k, err
                flagged[i] = not (a_last - err > d_k)
    _VERDICTS[key] = out
    return out


def _tiers_of(g_of, dim):
    """(label, model tier, g) of the tiers that screen a d = 128 world."""
    return (("K2w", "planes", g_of("planes", dim)), ("K2", "k2", g_of("k2", dim)), ("K2h", "k2", g_of("half", dim)))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_moved_world_is_identical():
    """World(CLASSES) as test_gpu_select_wave.py builds it: x, q and quser hashed with the class as it stood in that file,
    before it moved to edge_world.py."""
    import test_gpu_select_wave as t
    assert t.CLASSES == CLASSES and t.World is World
    w = World(CLASSES)
    assert (w.n, w.nq, w.x.dtype, w.q.dtype) == (62586, 471, np.float32, np.float32)
    h = [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in (w.x, w.q, w.quser.astype(np.int64))]
    assert h == ["14b76127dfd397d14a84619efeaf08b9da0ea00055229428d11a1ce42352687c",
                 "0b8d19043adda23718623600087517e7d157b0387e3b55fa9a631c62954e2f48",
                 "1bcbdd782bf66e7374340eea3d96bb2cbf8ff67ff62ec0ac3facd73b41973b4c"]


def test_values_are_exact_in_fp32(w128, wdeep, wcoarse):
    for w in (w128, wdeep, wcoarse):
        w.exact_bound()
    for w in (w128, wdeep):                                                # halfvec: rows and queries are binary16 values
        assert (w.x.astype(np.float16).astype(np.float32) == w.x).all() and (_rq(w.q) == w.q).all() and w.q.max() < 2048
    assert (sm.bf16(wcoarse.x) == wcoarse.x).all() and (sm.bf16(wcoarse.q) == wcoarse.q).all()
    assert wcoarse.x.min() < 0 and (w128.x >= 0).all() and (w128.x <= 255).all()
    assert 20_000 <= wcoarse.n < 100_000 and wdeep.n < 100_000


def _edges_ok(oracle, w, classes):
    for c, (allowed, _) in enumerate(classes):
        assert w.allowed_rows(oracle, w.role_of_class[c]).size == allowed
    assert (w.allowed_of_query() == [w.allowed_rows(oracle, int(u)).size for u in w.quser]).all()
    return {a for a, _ in classes}


def test_candidate_counts_sit_on_the_edges(oracle, w128, wdeep, wcoarse):
    edges = _edges_ok(oracle, w128, W128_CLASSES)
    assert {1, 1023, 1024, 1025, GQ_CAP} <= edges and max(edges) > GQ_CAP
    for k in KS:
        kp = max(2 * k, 32)
        assert kp <= GQ_MAX_KP and {k - 1, k, k + 1} - {0} <= edges and {kp - 1, kp, kp + 1} <= edges, k
    assert {w for _, w in W128_CLASSES} >= {1, 15, 16, 17, 64, 65}
    edges = _edges_ok(oracle, wdeep, DEEP_CLASSES)
    assert {1791, 1792, 1793, 2047, 2048, 2049, 3583, 3584, 3585, 9000} <= edges
    assert {2 * DEEP_K2_MAX - 1, 2 * DEEP_K2_MAX, 2 * DEEP_K2_MAX + 1} <= edges
    assert all(w in (16, 17) for _, w in DEEP_CLASSES[:-1])
    edges = _edges_ok(oracle, wcoarse, COARSE_CLASSES)
    for k in COARSE_KS:
        kp = max(4 * k, 128)
        assert kp <= GQ_MAX_KP and {kp - 1, kp, kp + 1} <= edges, k
    assert {99, 100, 101} <= edges and max(edges) > GQ_CAP
    assert all(w >= 130 for _, w in COARSE_CLASSES[:-1])


@pytest.mark.parametrize("metric", METRICS)
def test_ties_straddle_every_k(oracle, w128, wdeep, wcoarse, metric):
    """For every k some query's k-th and (k + 1)-th distances are equal, and their rows ascend: the oracle's tie rule."""
    for w, ks in ((w128, KS + (257,)), (wdeep, DEEP_KS), (wcoarse, COARSE_KS + (129,))):
        allowed = w.allowed_of_query()
        for k in ks:
            hit = 0
            for i in np.flatnonzero(allowed > k):
                idx, dist = w.ref(oracle, i, metric)
                if dist[k - 1] == dist[k]:
                    assert idx[k - 1] < idx[k]
                    hit += 1
                if hit == 3:                                               # (enough: the references are made on demand)
                    break
            assert hit >= 3, (k, hit)


@pytest.mark.parametrize("metric", METRICS)
def test_model_flags_nothing_on_w128_and_wdeep(oracle, g_of, w128, wdeep, metric):
    """Conditions on the inputs: no tier's flag test fires for any query with allowed >= kp, and no margin is within
    1e-3 err of zero (an fp32-vs-float64 difference cannot flip a flag)."""
    for w, ks in ((w128, KS + (257,)), (wdeep, tuple(k for k in DEEP_KS if k <= DEEP_K2_MAX))):
        for label, tier, g in _tiers_of(g_of, 128):
            if label == "K2w" and w is wdeep:
                continue                                                   # kp > GQ_MAX_KP: never on the planes
            worst = np.inf
            for k, (flagged, margin, err) in verdicts(oracle, w, tier, metric, g, ks).items():
                have = ~np.isnan(margin)
                assert (have == (w.allowed_of_query() >= sm.kp_of(tier, k))).all()
                assert not flagged.any(), (label, metric, k, np.flatnonzero(flagged))
                assert (np.abs(margin[have]) >= 1e-3 * err[have]).all(), (label, metric, k)
                worst = min(worst, float((margin[have] / err[have]).min()))
            print(f"{label} {metric}: smallest margin {worst:.1f} x err")


@pytest.mark.parametrize("metric", METRICS)
def test_model_flags_at_most_a_tenth_of_wcoarse(oracle, g_of, wcoarse, metric):
    w = wcoarse
    for k, (flagged, margin, err) in verdicts(oracle, w, "coarse", metric, g_of("coarse", 320), COARSE_KS).items():
        have = ~np.isnan(margin)
        assert (have == (w.allowed_of_query() >= sm.kp_of("coarse", k))).all()
        print(f"K2g {metric} k = {k}: the model flags {int(flagged.sum())} of {int(have.sum())} queries")
        assert 1 <= flagged.sum() <= 0.1 * w.nq, (metric, k, int(flagged.sum()))
        assert (w.quser[flagged] == w.role_of_class[COARSE_CLONES]).all()
        assert (np.abs(margin[have]) >= 1e-3 * err[have]).all(), (metric, k)
    # k = 129 leaves the coarse tier (4k > GQ_MAX_KP) for the planes, whose bound is ~250 times tighter: only the clones are flagged
    flagged, margin, err = verdicts(oracle, w, "planes", metric, g_of("planes", 320), (129,))[129]
    have = ~np.isnan(margin)
    assert (w.quser[flagged] == w.role_of_class[COARSE_CLONES]).all() and (np.abs(margin[have]) >= 1e-3 * err[have]).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _rq(q):
    """The query `$1::halfvec` holds, widened."""
    return np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float32)


@contextlib.contextmanager
def _tier(monkeypatch, w, env, half=False):
    """A fresh context opened, and the world loaded, under `env` (VSR_NO_INT8 and VSR_NO_HIONLY are read when the planes
    are built); one filter per user."""
    import vsrbac
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = vsrbac.Context(0)
    try:
        corpus = ctx.load_corpus_half(w.x.astype(np.float16), w.blk, w.doc) if half else ctx.load_corpus(w.x, w.blk, w.doc)
        for name in env:
            monkeypatch.delenv(name)
        corpus.load_rbac(*w.rbac())
        per_user = {int(u): corpus.filter_for_user(int(u), vsrbac.RANGES) for u in np.unique(w.quser)}
        yield ctx, corpus, [per_user[int(u)] for u in w.quser]
        corpus.free()
    finally:
        ctx.close()


def _calls(w, ki):
    """The query subsets of the three calls at the ki-th k: one query, three, all (the short calls move with k)."""
    s = (37 * ki + 5) % (w.nq - 3)
    return [np.arange(s, s + 1), np.arange(s + 1, s + 4), np.arange(w.nq)]


def _check_one(oracle, w, res, j, i, k, metric):
    idx, dist = w.ref(oracle, i, metric)
    idx, dist = idx[:k], dist[:k]
    m = int(res.counts[j])
    assert m == idx.size, (metric, k, int(i), int(w.quser[i]), m, idx.size)
    np.testing.assert_array_equal(res.rows[j, :m], idx)
    want = dist.astype(np.float32) + np.float32(0)                         # -0.0 -> +0.0: see "Zero inner products" above
    np.testing.assert_array_equal(res.dist[j, :m].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(res.block_ids[j, :m], w.blk[idx])
    np.testing.assert_array_equal(res.doc_ids[j, :m], w.doc[idx])
    assert (res.rows[j, m:] == -1).all() and (res.block_ids[j, m:] == -1).all() and (res.doc_ids[j, m:] == -1).all()
    assert np.isposinf(res.dist[j, m:]).all()


def _check(oracle, w, res, sel, k, metric):
    for j, i in enumerate(sel):
        _check_one(oracle, w, res, j, i, k, metric)


def _same(a, b):
    for f in ("counts", "rows", "dist", "block_ids", "doc_ids"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


class _Dev:
    """Device buffers of one search_device call."""

    def __init__(self, q, k):
        import torch
        dev = torch.device("cuda", 0)
        nq = len(q)
        self.q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        self.blk = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.doc = torch.empty((nq, k), dtype=torch.int32, device=dev)
        self.row = torch.empty((nq, k), dtype=torch.int64, device=dev)
        self.dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        self.cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()                                           # the library runs on its own stream

    def qp(self):
        return ctypes.c_void_p(self.q.data_ptr())

    def args(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return p(self.blk), p(self.doc), p(self.row), p(self.dist), p(self.cnt)

    def result(self):
        return SimpleNamespace(rows=self.row.cpu().numpy(), dist=self.dist.cpu().numpy(), counts=self.cnt.cpu().numpy(),
                               block_ids=self.blk.cpu().numpy(), doc_ids=self.doc.cpu().numpy())


def _device_call(oracle, ctx, corpus, w, filters, sel, k, metric):
    """vsr_search_device, then vsr_search_device_exact, on the queries `sel`: the soundness rules of a published and of a
    flagged query, and the exact batch.  Returns (flagged queries as indices into the world, kernel name)."""
    nq = len(sel)
    fs = [filters[i] for i in sel]
    b = _Dev(w.q[sel], k)
    keep = corpus.search_device(b.qp(), nq, k, metric, fs, *b.args())
    ctx.synchronize()
    del keep
    name = ctx.last_scan_kernel()
    _, flags = ctx.screening_check(nq)
    got = b.result()
    for j, i in enumerate(sel):
        if got.counts[j] >= 0:
            assert flags[j] == 0, (metric, k, int(i))
            _check_one(oracle, w, got, j, i, k, metric)
        else:                                                              # flagged: -1 - count, and the flag is on record
            assert flags[j] != 0, (metric, k, int(i))
            assert -1 - int(got.counts[j]) == min(k, w.ref(oracle, i, metric)[0].size), (metric, k, int(i), int(got.counts[j]))
    flagged = sel[got.counts < 0]
    n_rerun = corpus.search_device_exact(b.qp(), nq, k, metric, fs, *b.args())
    assert n_rerun == flagged.size, (metric, k, n_rerun, flagged)
    _check(oracle, w, b.result(), sel, k, metric)
    return flagged, name


def _run_tier(oracle, monkeypatch, w, env, metric, ks, expect, model=None, half=False, never_seeded=False):
    """One tier: every k of `ks` in calls of 1, 3 and all queries through both entry points.  expect(k, name): asserts the
    kernel of the call of all queries and returns kp if the screening tier under test ran (None: an exact kernel).
    model: {k: (flagged, ...)} of verdicts().  never_seeded: no call of this tier can seed a threshold (else only the call
    of all queries cannot, see the module's docstring).  Returns {(k, call): result of vsr_search}."""
    out = {}
    allowed = w.allowed_of_query()
    with _tier(monkeypatch, w, env, half) as (ctx, corpus, filters):
        for ki, k in enumerate(ks):
            for c, sel in enumerate(_calls(w, ki)):
                res = corpus.search(w.q[sel], k, metric, [filters[i] for i in sel])
                host_name = ctx.last_scan_kernel()
                assert (res.counts >= 0).all()
                _check(oracle, w, res, sel, k, metric)
                out[(k, c)] = res
                flagged, name = _device_call(oracle, ctx, corpus, w, filters, sel, k, metric)
                print(f"{metric} k={k} call of {sel.size}: {name}; flagged {flagged.tolist()[:8]}{' ...' if flagged.size > 8 else ''}")
                full = sel.size == w.nq
                kp = expect(k, name) if full else None
                if full and not flagged.size:
                    assert host_name == name, (host_name, name)           # (a flagged query's re-run renames the host call)
                want = np.flatnonzero(model[k][0]) if model is not None and k in model else np.zeros(0, np.int64)
                if kp is None:
                    if full:
                        assert not flagged.size, (k, name, flagged)      # an exact kernel never flags
                    elif never_seeded:                                     # whichever kernel took the short call: no flag but the model's
                        assert np.isin(flagged, want).all(), (k, name, flagged)
                    continue
                assert (allowed[want] >= kp).all()
                # allowed >= kp: the model's flags and no other; allowed < kp: never seeded, so never flagged
                np.testing.assert_array_equal(np.sort(flagged), want, err_msg=f"{metric} k={k} {name}: flagged queries vs the model's; "
                                              f"allowed rows of the difference: {allowed[np.setxor1d(flagged, want)]}")
    return out


def _names(*parts, no=()):
    def check(name):
        assert all(p in name for p in parts) and not any(p in name for p in no), name
    return check


K2W_HO = _names("(K2w", "hi-only", "select_rerank_kernel", no=("int8", "hi+mid"))
K2W_MID = _names("(K2w", "hi+mid", "select_rerank_kernel", no=("int8", "hi-only"))
K2 = _names("(K2)")
K2H = _names("(K2h", "half")


def _expect_wide(wide):
    """K2w up to k = 256 (2k = GQ_MAX_KP), K2 from k = 257."""
    def expect(k, name):
        (wide if 2 * k <= GQ_MAX_KP else K2)(name)
        return max(2 * k, 32)
    return expect


@pytest.mark.gpu
@pytest.mark.parametrize("metric,geometry", [("ip", "default"), ("l2", "default"), ("ip", "fine")])
def test_k2w_planes_hi_only_and_hi_mid(oracle, g_of, monkeypatch, w128, metric, geometry):
    """W128 on the bf16 planes: hi-only (IP in a default context; L2 under VSR_NO_INT8, which keeps the corpus off its int8
    planes) and hi + mid (VSR_NO_HIONLY), which must return the same bytes; k = 257 hands over to K2 on the same corpus.  "fine"
    moves the workgroup geometry and with it which queries are seeded."""
    w = w128
    ks = KS + (257,)
    geo = FINE if geometry == "fine" else {}
    env = {"VSR_NO_INT8": "1"} if metric == "l2" else {}
    planes = verdicts(oracle, w, "planes", metric, g_of("planes", 128), ks)
    k2 = verdicts(oracle, w, "k2", metric, g_of("k2", 128), ks)
    model = {k: planes[k] if 2 * k <= GQ_MAX_KP else k2[k] for k in ks}
    ho = _run_tier(oracle, monkeypatch, w, {**env, **geo}, metric, ks, _expect_wide(K2W_HO), model)
    mid = _run_tier(oracle, monkeypatch, w, {"VSR_NO_HIONLY": "1", **env, **geo}, metric, ks, _expect_wide(K2W_MID), model)
    for key in ho:
        _same(ho[key], mid[key])


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_k2_fp32_mfma_on_w128(oracle, g_of, monkeypatch, w128, metric):
    """VSR_NO_WIDE: every shared pass of W128 on K2, K5 and rerank_kernel."""
    def expect(k, name):
        K2(name)
        return max(2 * k, 32)
    _run_tier(oracle, monkeypatch, w128, {"VSR_NO_WIDE": "1"}, metric, KS, expect,
              verdicts(oracle, w128, "k2", metric, g_of("k2", 128), KS), never_seeded=True)


def _expect_deep(screened, exact_no):
    def expect(k, name):
        if k <= DEEP_K2_MAX:
            screened(name)
            return 2 * k
        assert not any(p in name for p in exact_no) and "(K1" in name, name
        return None
    return expect


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_k2_hands_over_to_k1m_by_k(oracle, g_of, monkeypatch, wdeep, metric):
    """Wdeep in a default context: K2 while mfma_cap_for_k(2k) <= 8192 (k = 257, 512, 1792), K1m beyond (1793, 2048)."""
    ks = tuple(k for k in DEEP_KS if k <= DEEP_K2_MAX)
    _run_tier(oracle, monkeypatch, wdeep, {}, metric, DEEP_KS, _expect_deep(K2, ("(K2",)),
              verdicts(oracle, wdeep, "k2", metric, g_of("k2", 128), ks), never_seeded=True)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_k2h_on_w128(oracle, g_of, monkeypatch, w128, metric):
    """W128 as a halfvec corpus (u8 integers are binary16 values; rounding the queries is the identity): K2h for every k."""
    w = w128
    ks = KS + (257,)
    assert (w.x.astype(np.float16).astype(np.float32) == w.x).all() and (_rq(w.q) == w.q).all()

    def expect(k, name):
        K2H(name)
        return max(2 * k, 32)
    w.round_query = _rq                                                    # (the identity here: the fp32 references stay valid)
    try:
        _run_tier(oracle, monkeypatch, w, {}, metric, ks, expect, verdicts(oracle, w, "k2", metric, g_of("half", 128), ks),
                  half=True, never_seeded=True)
    finally:
        w.round_query = None


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_k2h_hands_over_to_k1h_by_k(oracle, g_of, monkeypatch, wdeep, metric):
    w = wdeep
    ks = (257, 512, 1792, 1793)
    assert (w.x.astype(np.float16).astype(np.float32) == w.x).all() and (_rq(w.q) == w.q).all()
    w.round_query = _rq
    try:
        _run_tier(oracle, monkeypatch, w, {}, metric, ks, _expect_deep(K2H, ("(K2",)),
                  verdicts(oracle, w, "k2", metric, g_of("half", 128), ks[:3]), half=True, never_seeded=True)
    finally:
        w.round_query = None


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_k2g_coarse_planes(oracle, g_of, monkeypatch, wcoarse, metric):
    """Wcoarse: K2g while 4k <= GQ_MAX_KP, with the model's flagged queries (at most a tenth) and nobody else's; K2w on the
    hi-only planes at k = 129."""
    w = wcoarse
    model = dict(verdicts(oracle, w, "coarse", metric, g_of("coarse", 320), COARSE_KS))
    model.update(verdicts(oracle, w, "planes", metric, g_of("planes", 320), (129,)))

    def expect(k, name):
        if 4 * k <= GQ_MAX_KP:
            _names("(K2g", "coarse", "select_rerank_kernel")(name)
            return max(4 * k, 128)
        K2W_HO(name)
        return 2 * k
    _run_tier(oracle, monkeypatch, w, {}, metric, COARSE_KS + (129,), expect, model)
