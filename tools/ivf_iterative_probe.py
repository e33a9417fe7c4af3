"""Filtered IVFFlat search: pgvector's iterative index scan (vsr_ivf_search_iterative_device) beside the emulation the
PostgreSQL shim used before it (vsr_ivf_search_device re-run with probes doubled until every query has k rows).

The reference's parameters: 300 000 SIFT-like 128-d rows, lists = 100 (k-means on the GPU, the index oracle's assignment),
1000 queries per call, k = 100, filters that admit 2 % and 10 % of the rows (every 50th / 10th block of 100 rows) and,
beyond the reference's own points, 0.5 %, where a scan needs many batches; probes 1 and 5, ivfflat.max_probes at its
default (32768: all lists).  Per point: the median, min and max of the repetitions' wall time per call (queries and results
resident, the call synchronised), the lists each method scanned per query, and a check of the new call's rows against
the numpy model (tests/ivf_iterative_model.py) on a sample of queries.

    python tools/ivf_iterative_probe.py OUT_DIR [--rows 300000] [--queries 1000] [--reps 11]

Writes OUT_DIR/ivf_iterative.json and prints it."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=300_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--lists", type=int, default=100)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--max-probes", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--sample", type=int, default=12, help="queries checked against the model per point")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()

    import torch
    import vsrbac
    from ivf_iterative_model import iterative_search
    from oracle.oracle import IvfIndex as OracleIvf
    from oracle.oracle import Oracle
    from vsrbac.datasets import sift_like_corpus

    os.makedirs(args.out_dir, exist_ok=True)
    n, k, nq, lists = args.rows, args.k, args.queries, args.lists
    x, _, _ = sift_like_corpus(n, 128, seed=args.seed)
    x = np.ascontiguousarray(x, dtype=np.float32)
    rng = np.random.default_rng(args.seed)
    q = np.ascontiguousarray(x[rng.integers(0, n, nq)] + np.rint(rng.normal(0, 2, (nq, 128))).astype(np.float32))

    ctx = vsrbac.Context(0)
    corpus = ctx.load_corpus(x)
    sample = x[np.sort(rng.choice(n, min(n, max(lists * 50, 10000)), replace=False))]
    centers = ctx.ivf_kmeans(sample, lists, "l2", seed=args.seed)
    centers = centers[0] if isinstance(centers, tuple) else centers
    oivf = OracleIvf.from_centers(Oracle("strict"), "l2", x, centers)
    gpu = corpus.load_ivf(centers, oivf.assign)

    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    d_q = torch.from_numpy(q).to(dev)
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "pr": torch.empty((nq,), dtype=torch.int32, device=dev)}
    outs = [ptr(o[key]) for key in ("blk", "doc", "row", "dist", "cnt")]

    def timed(call):
        call()                                             # warm-up: filters' view bitmaps and list parts are cached
        ctx.synchronize()
        secs = []
        for _ in range(args.reps):
            t = time.perf_counter()
            extra = call()
            ctx.synchronize()
            secs.append(time.perf_counter() - t)
        ms = sorted(s * 1e3 for s in secs)
        return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "reps": len(ms)}, extra

    points = []
    for frac_name, every in (("2%", 50), ("10%", 10), ("0.5%", 200)):
        allowed = (((np.arange(n) // 100) % every) == 3).astype(np.uint8)
        flt = corpus.filter_from_bytemask(allowed, vsrbac.BITMAP)
        fl = [flt] * nq
        for probes in args.probes:
            def iterative():
                gpu.search_iterative_device(ptr(d_q), nq, k, probes, "l2", fl, "relaxed_order", args.max_probes, *outs, ptr(o["pr"]))

            def emulation():
                # the shim's former refill: the whole search again with twice the probes for the queries still short of k
                # (their queries and filters packed; a query with k rows keeps them)
                p, todo, scanned = probes, np.arange(nq), np.zeros(nq, dtype=np.int64)
                final = np.zeros(nq, dtype=np.int64)
                while True:
                    m = len(todo)
                    dq = d_q if m == nq else d_q[torch.from_numpy(todo).to(dev)].contiguous()
                    gpu.search_device(ptr(dq), m, k, p, "l2", fl[:m], *outs)
                    cnt = o["cnt"][:m].cpu().numpy()
                    scanned[todo] += min(p, lists)
                    final[todo] = min(p, lists)
                    todo = todo[cnt < k]
                    if len(todo) == 0 or p >= min(args.max_probes, lists):
                        return scanned, final
                    p = min(2 * p, args.max_probes, lists)

            t_it, _ = timed(iterative)
            cnt_it, pr_it = o["cnt"].cpu().numpy().copy(), o["pr"].cpu().numpy().copy()
            rows_it, dist_it = o["row"].cpu().numpy().copy(), o["dist"].cpu().numpy().copy()
            t_em, (scanned_em, final_em) = timed(emulation)
            checked, agree = 0, 0
            for i in range(0, nq, max(1, nq // args.sample)):
                rows, dist, ls = iterative_search(oivf, q[i], k, probes, args.max_probes, mask=allowed)
                checked += 1
                agree += (cnt_it[i] == len(rows) and pr_it[i] == ls and (rows_it[i, :len(rows)] == rows).all()
                          and (dist_it[i, :len(rows)] == dist.astype(np.float32)).all())
            pt = {"permitted": frac_name, "probes": probes, "iterative": t_it, "emulation": t_em,
                  "iterative_over_emulation_median": round(t_it["median_ms"] / t_em["median_ms"], 3),
                  "iterative_lists_scanned_per_query": round(float(pr_it.mean()), 2),
                  "iterative_rows_per_query": round(float(cnt_it.mean()), 2),
                  "emulation_lists_scanned_per_query": round(float(scanned_em.mean()), 2),
                  "emulation_final_probes_per_query": round(float(final_em.mean()), 2),
                  "model_check": {"queries": checked, "identical": int(agree)}}
            points.append(pt)
            print(json.dumps(pt), flush=True)

    out = {"rows": n, "dim": 128, "lists": lists, "queries_per_call": nq, "k": k, "max_probes": args.max_probes,
           "device": ctx.device_info()["name"], "points": points}
    with open(os.path.join(args.out_dir, "ivf_iterative.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    gpu.free()
    corpus.free()
    ctx.close()


if __name__ == "__main__":
    main()
