"""Filtered HNSW search with and without pgvector's iterative index scans (vsr_hnsw_search_iterative), on bench.py's hnsw setup.

120 000 SIFT-like 128-d rows, a graph from vsr_hnsw_build(m = 16, ef_construction = 64), a filter that admits every 10th
block of 100 rows (10 %), 1000 queries per call, k = 100, ef_search 40 / 100 / 400.  For each of the plain walk + filter
(hnsw.iterative_scan = off), the predicate-aware walk, relaxed_order and strict_order (hnsw.max_scan_tuples = 20000):
queries/s of the device entry point (queries and results resident, one call per 1000 queries), recall@k against the
oracle's exact filtered top-k, rows returned and tuples counted per query.

    python tools/hnsw_iterative_probe.py OUT_DIR [--queries 1000] [--max-scan-tuples 20000]

Writes OUT_DIR/hnsw_iterative_probe.json and prints it."""
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
    ap.add_argument("--rows", type=int, default=120_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--ef", type=int, nargs="+", default=[40, 100, 400])
    ap.add_argument("--max-scan-tuples", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()

    import torch
    import vsrbac
    from oracle.oracle import Oracle
    from vsrbac.datasets import sift_like_corpus

    os.makedirs(args.out_dir, exist_ok=True)
    n, k, nq = args.rows, args.k, args.queries
    x, _, _ = sift_like_corpus(n, 128, seed=args.seed)
    x = np.ascontiguousarray(x, dtype=np.float32)
    rng = np.random.default_rng(args.seed)
    q = x[rng.integers(0, n, nq)] + rng.normal(0, 2, (nq, 128)).astype(np.float32)
    allowed = (((np.arange(n) // 100) % 10) == 3).astype(np.uint8)

    orc = Oracle("strict")
    t0 = time.perf_counter()
    exact = [set(orc.filtered_topk("l2", x, q[i], k, None, None, allowed)[0].tolist()) for i in range(nq)]
    oracle_s = time.perf_counter() - t0

    ctx = vsrbac.Context(0)
    corpus = ctx.load_corpus(x)
    t0 = time.perf_counter()
    gidx = corpus.build_hnsw(16, 64, "l2", seed=args.seed)
    build_s = time.perf_counter() - t0
    flt = corpus.filter_from_bytemask(allowed, vsrbac.BITMAP)
    fl = [flt] * nq
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
         "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "tup": torch.empty((nq,), dtype=torch.int64, device=dev)}
    outs = [ptr(o[key]) for key in ("blk", "doc", "row", "dist", "cnt", "tup")]

    def timed(call):
        keep = call()
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(args.reps):
            keep = call()
        ctx.synchronize()
        del keep
        return (time.perf_counter() - t) / args.reps

    def stats(secs, host_rerun):
        rows, cnt, tup = o["row"].cpu().numpy(), o["cnt"].cpu().numpy(), o["tup"].cpu().numpy()
        rerun = int((cnt < 0).sum())
        if rerun:                                          # (device variants report -1; the host entry point re-runs those)
            res, t2 = host_rerun()
            rows, cnt, tup = res.rows, res.counts, t2
        hit = sum(len(set(rows[i, :cnt[i]].tolist()) & exact[i]) for i in range(nq))
        return {"qps": round(nq / secs, 1), "ms_per_call": round(secs * 1e3, 3), "recall_at_k": round(hit / (k * nq), 4),
                "rows_returned_per_query": round(float(cnt.mean()), 2), "tuples_per_query": round(float(tup.mean()), 1),
                "queries_reported_for_rerun": rerun}

    sweep = []
    for ef in args.ef:
        pt = {"ef_search": ef}
        for name, aware in (("plain_walk_then_filter", False), ("predicate_aware", True)):
            gidx.set_predicate_aware(aware)
            secs = timed(lambda: gidx.search_device(ptr(d_q), nq, k, ef, "l2", fl, *outs))
            pt[name] = stats(secs, lambda: gidx.search(q, k, ef, "l2", fl))
        gidx.set_predicate_aware(False)
        for mode in ("relaxed_order", "strict_order"):
            secs = timed(lambda: gidx.search_iterative_device(ptr(d_q), nq, k, ef, "l2", fl, mode, args.max_scan_tuples, *outs))
            pt[mode] = stats(secs, lambda: gidx.search_iterative(q, k, ef, "l2", fl, mode, args.max_scan_tuples))
        # where round 0 already fills k: no filter, the iterative kernel beside the plain one at the same ef
        if ef >= k:
            secs_p = timed(lambda: gidx.search_device(ptr(d_q), nq, k, ef, "l2", None, *outs))
            secs_i = timed(lambda: gidx.search_iterative_device(ptr(d_q), nq, k, ef, "l2", None, "relaxed_order",
                                                                args.max_scan_tuples, *outs))
            pt["unfiltered"] = {"plain_ms_per_call": round(secs_p * 1e3, 3), "relaxed_ms_per_call": round(secs_i * 1e3, 3),
                                "relaxed_over_plain": round(secs_i / secs_p, 3)}
        sweep.append(pt)
        print(json.dumps(pt), flush=True)

    out = {"rows": n, "dim": 128, "queries_per_call": nq, "k": k, "m": 16, "ef_construction": 64,
           "graph": "vsr_hnsw_build", "graph_build_s": round(build_s, 2), "permitted_fraction": round(float(allowed.mean()), 4),
           "max_scan_tuples": args.max_scan_tuples, "oracle_exact_s": round(oracle_s, 1),
           "device": ctx.device_info()["name"], "sweep": sweep}
    with open(os.path.join(args.out_dir, "hnsw_iterative_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    gidx.free()
    corpus.free()
    ctx.close()


if __name__ == "__main__":
    main()
