"""The two-stage search (vsr_search_quantized_device: Hamming shortlist on the bits, exact re-rank on the source rows) beside the
default exact search (vsr_search_device) on one MI355X, in one process, the two sides alternating.

  1M x 768 real-valued clustered fp32 rows and their binary_quantize corpus; 1000 queries per call, cosine, k = 100;
  (a) unfiltered, (b) under the benchmark's tree RBAC (role pre-filter); shortlist in {100, 400, 1000, 2000}

Queries and results are device-resident; a call is timed by the host clock around the call and a synchronise.  Per setting:
median / min / max of the repetitions of either side, recall@k of the two-stage answer against the exact one (the exact side
through vsr_search_device_exact, so that no row of the baseline is unproven), and the device bytes of both corpora.  Numbers
are recorded, not gated.

    python tools/quantized_probe.py OUT_DIR [--rows 1000000] [--dim 768] [--queries 1000] [--reps 7]

Writes OUT_DIR/quantized.json and prints it."""
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


def clustered_rows(rng, n, dim, centres=1000, spread=0.7, chunk=50_000):
    c = rng.standard_normal((centres, dim), dtype=np.float32)
    x = np.empty((n, dim), dtype=np.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        x[lo:hi] = c[rng.integers(0, centres, hi - lo)] + spread * rng.standard_normal((hi - lo, dim), dtype=np.float32)
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--shortlists", type=int, nargs="+", default=[100, 400, 1000, 2000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    n, dim, nq, k, reps = args.rows, args.dim, args.queries, args.k, max(args.reps, 3)
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx = vsrbac.Context(0)
    rng = np.random.default_rng(args.seed)
    x = clustered_rows(rng, n, dim)
    blk = np.arange(n, dtype=np.int64)
    doc = (np.arange(n) // 100 + 1).astype(np.int32)
    q = x[rng.integers(0, n, nq)] + 0.35 * rng.standard_normal((nq, dim), dtype=np.float32)
    source = ctx.load_corpus(x, blk, doc)
    del x
    bits = source.binary_quantize()
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=max(n // 100, 1), seed=args.seed)
    source.load_rbac(rbac.user_roles, rbac.permissions)
    bits.load_rbac(rbac.user_roles, rbac.permissions)         # not inherited: the corpus that is scanned owns the filters
    _, quser = sample_queries(nq, n, 1000, seed=args.seed)
    d_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)

    def outputs():
        o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
             "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
             "cnt": torch.empty((nq,), dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        return o

    o2, o1 = outputs(), outputs()
    report = {"device": ctx.device_info()["name"], "rows": n, "dim": dim, "queries_per_call": nq, "k": k, "metric": "cosine", "reps": reps,
              "source_device_bytes": source.device_bytes(), "bits_device_bytes": bits.device_bytes(),
              "timing": "host clock around one call and a synchronise, device-resident queries and results; the two-stage call and "
                        "vsr_search_device alternate inside every repetition",
              "settings": []}

    def stats(secs):
        ms = sorted(v * 1e3 for v in secs)
        return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    for what, f_src, f_bits in (
            ("unfiltered", None, None),
            ("tree RBAC, role pre-filter", source.pack_filters([source.filter_for_user(int(u), vsrbac.RANGES) for u in quser]),
             bits.pack_filters([bits.filter_for_user(int(u), vsrbac.RANGES) for u in quser]))):
        exact = lambda: source.search_device(ptr(d_q), nq, k, "cosine", f_src, ptr(o1["blk"]), ptr(o1["doc"]), ptr(o1["row"]),
                                             ptr(o1["dist"]), ptr(o1["cnt"]))
        # the baseline answer, every row proven
        rerun = source.search_device_exact(ptr(d_q), nq, k, "cosine", f_src, ptr(o1["blk"]), ptr(o1["doc"]), ptr(o1["row"]),
                                           ptr(o1["dist"]), ptr(o1["cnt"]))
        exact_rows, exact_cnt = o1["row"].cpu().numpy(), o1["cnt"].cpu().numpy()
        exact()
        ctx.synchronize()
        exact_kernel = ctx.last_scan_kernel()
        for shortlist in args.shortlists:
            two = lambda s=shortlist: source.search_quantized_device(bits, ptr(d_q), nq, k, s, "cosine", f_bits, ptr(o2["blk"]),
                                                                     ptr(o2["doc"]), ptr(o2["row"]), ptr(o2["dist"]), ptr(o2["cnt"]))
            for _ in range(2):                                # warm-up: code objects, workspaces, cached filters
                two()
                exact()
            ctx.synchronize()
            t_two, t_exact = [], []
            for _ in range(reps):
                t = time.perf_counter()
                two()
                ctx.synchronize()
                t_two.append(time.perf_counter() - t)
                t = time.perf_counter()
                exact()
                ctx.synchronize()
                t_exact.append(time.perf_counter() - t)
            two()
            ctx.synchronize()
            kernel = ctx.last_scan_kernel()
            rows, cnt = o2["row"].cpu().numpy(), o2["cnt"].cpu().numpy()
            hits = sum(np.intersect1d(rows[i, :cnt[i]], exact_rows[i, :exact_cnt[i]]).size for i in range(nq))
            entry = {"filter": what, "shortlist": shortlist, "two_stage": stats(t_two), "exact": stats(t_exact),
                     "recall_at_k": round(hits / max(int(exact_cnt.sum()), 1), 4), "exact_queries_rerun_for_the_baseline": rerun,
                     "two_stage_kernel": kernel, "exact_kernel": exact_kernel}
            entry["speedup"] = round(entry["exact"]["median_ms"] / entry["two_stage"]["median_ms"], 2)
            report["settings"].append(entry)
            print(json.dumps(entry), flush=True)
        del f_src, f_bits

    with open(os.path.join(args.out_dir, "quantized.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))
    bits.free()
    source.free()
    ctx.close()


if __name__ == "__main__":
    main()
