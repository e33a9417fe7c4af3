"""K2h (f16 matrix-core screening + exact re-rank) against K1h over the same halfvec corpus, in one process.

One half corpus, two sessions of the same GPU: `k2h` as the library runs it, `k1h` opened under VSR_NO_HALF_MFMA=1 -- the
kernel a half corpus ran before K2h existed, and the last rung of K2h's own re-run ladder.  Queries and results are
device-resident.  A call is vsr_search_device_exact: the search, a synchronise and the exact re-run of whatever the screen
flagged, so the K2h side pays for its flagged queries; it is timed by the host clock, the sides alternating inside every
repetition.  Per side: median / min / max over the repetitions, the kernel that ran, the queries re-run per call.

  (b) 10M x 128 integer-valued rows, 1000-query calls under the benchmark's tree RBAC (role pre-filter), k = 100
  (c) 1M x 768 real-valued rows (normal, rounded to binary16), 1000 unfiltered queries per call, k = 100
  (s) the rows of (b), unfiltered calls of 2, 4, 8, 16 and 64 queries: where shared passes start to pay on the matrix cores

`spread` of a leg is the larger of the two sides' (max - min) / median; K2h wins a leg when k1h's median over k2h's exceeds
1 + spread.

    python tools/halfvec_mfma_probe.py OUT_DIR [--rows 10000000] [--wide-rows 1000000] [--queries 1000] [--reps 11]

Writes OUT_DIR/halfvec_mfma.json and prints it."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, sift_like_corpus, sift_like_rows_at, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    k, nq, reps = args.k, args.queries, max(args.reps, 11)
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    ctx = vsrbac.Context(0)                                   # owns the corpora; the k2h side runs in it
    os.environ["VSR_NO_HALF_MFMA"] = "1"
    k1h = vsrbac.Context(0)
    del os.environ["VSR_NO_HALF_MFMA"]

    def outputs(n):
        o = {"blk": torch.empty((n, k), dtype=torch.int64, device=dev), "doc": torch.empty((n, k), dtype=torch.int32, device=dev),
             "row": torch.empty((n, k), dtype=torch.int64, device=dev), "dist": torch.empty((n, k), dtype=torch.float32, device=dev),
             "cnt": torch.empty((n,), dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        return o

    def leg(corpus, d_q, n_q, filters, exact_values, what, n_reps):
        sessions = {"k2h": ctx, "k1h": k1h}
        out = {name: outputs(n_q) for name in sessions}
        reruns = {name: [] for name in sessions}

        def call(name):
            o = out[name]
            n = corpus.search_device_exact(ptr(d_q), n_q, k, "l2", filters, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]),
                                           ptr(o["cnt"]), session=sessions[name])
            sessions[name].synchronize()
            return n

        kernels = {}
        for name, s in sessions.items():                      # warm-up: code objects, workspaces, cached filters
            o = out[name]
            corpus.search_device(ptr(d_q), n_q, k, "l2", filters, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]), ptr(o["cnt"]),
                                 session=s)
            s.synchronize()
            kernels[name] = s.last_scan_kernel()              # of the screening call itself, before any re-run
            for _ in range(2):
                call(name)
        secs = {name: [] for name in sessions}
        for _ in range(n_reps):
            for name in sessions:                             # sides alternating
                t = time.perf_counter()
                reruns[name].append(call(name))
                secs[name].append(time.perf_counter() - t)
        a, b = out["k2h"], out["k1h"]
        ra, rb = a["row"].cpu().numpy(), b["row"].cpu().numpy()
        da, db = a["dist"].cpu().numpy(), b["dist"].cpu().numpy()
        if exact_values:
            same = {"identical": bool((a["cnt"].cpu().numpy() == b["cnt"].cpu().numpy()).all() and (ra == rb).all() and
                                      (da.view(np.uint32) == db.view(np.uint32)).all())}
        else:
            common = np.mean([len(set(ra[i].tolist()) & set(rb[i].tolist())) / k for i in range(n_q)])
            same = {"rows_in_common": round(float(common), 5), "max_abs_distance_difference": float(np.abs(da - db).max())}
        res = {"what": what, "queries_per_call": n_q, "same_results": same}
        for name in sessions:
            ms = sorted(v * 1e3 for v in secs[name])
            res[name] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
                         "kernel": kernels[name], "queries_rerun_per_call": sorted(reruns[name])[len(reruns[name]) // 2]}
        spread = max((res[s]["max_ms"] - res[s]["min_ms"]) / res[s]["median_ms"] for s in sessions)
        res["spread"] = round(spread, 4)
        res["k1h_over_k2h_median"] = round(res["k1h"]["median_ms"] / res["k2h"]["median_ms"], 3)
        res["k2h_wins"] = bool(res["k1h_over_k2h_median"] > 1 + spread)
        print(json.dumps(res), flush=True)
        return res

    report = {"device": ctx.device_info()["name"], "k": k, "reps": reps,
              "timing": "host clock around vsr_search_device_exact (search, synchronise, exact re-run of flagged queries), device-resident "
                        "queries and results, sides alternating",
              "fp32_default_path_for_scale_ms": {"b": 0.52, "c": 2.2}}

    n, dim = args.rows, 128
    x, blk, doc = sift_like_corpus(n, dim, seed=args.seed)    # integers 0..255: exact in binary16, fp32 sums exact
    half = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    del x
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
    half.load_rbac(rbac.user_roles, rbac.permissions)
    qrow, quser = sample_queries(nq, n, 1000, seed=args.seed)
    d_q = torch.from_numpy(sift_like_rows_at(qrow, dim, seed=args.seed)).to(dev)
    fl = half.pack_filters([half.filter_for_user(int(u), vsrbac.RANGES) for u in quser])
    report["b"] = leg(half, d_q, nq, fl, True, f"{n} x {dim}, {nq} queries per call, tree RBAC role pre-filter", reps)
    report["s"] = [leg(half, d_q, m, None, True, f"{n} x {dim}, {m} unfiltered queries per call", 5) for m in (2, 4, 8, 16, 64)]
    del fl
    half.free()

    n, dim = args.wide_rows, 768
    rng = np.random.default_rng([args.seed, 23])
    h = rng.standard_normal((n, dim), dtype=np.float32).astype(np.float16)
    half = ctx.load_corpus_half(h)
    q = (h[rng.integers(0, n, nq)].astype(np.float32) + 0.05 * rng.standard_normal((nq, dim), dtype=np.float32))
    d_q = torch.from_numpy(q.astype(np.float16).astype(np.float32)).to(dev)
    del h
    report["c"] = leg(half, d_q, nq, None, False, f"{n} x {dim}, {nq} unfiltered queries per call, real-valued rows", reps)
    half.free()

    with open(os.path.join(args.out_dir, "halfvec_mfma.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    for s in (k1h, ctx):
        s.close()


if __name__ == "__main__":
    main()
