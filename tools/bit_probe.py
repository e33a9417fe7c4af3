"""Bit corpora (vsr_corpus_load_bit, K1b) timed on one MI355X, in one process.

  (a) 10M x 128 random bits, unfiltered, one query per call, k = 100, Hamming and Jaccard
  (b) 10M x 1024 random bits, the same; the main scan launch's bytes per second stand beside K1's 5.65 TB/s over 10M x 128
      fp32 rows (README) as context only: K1b has no kernel at the parent commit to be compared with
  (c) the 128-bit rows, 1000-query calls under the benchmark's tree RBAC (role pre-filter, class passes), both metrics

Queries and results are device-resident; a call is timed by the host clock around the call(s) and a synchronise.  Per leg:
median / min / max of the repetitions' time per call, the main scan launch's own device time (vsr_profiling level 2, a second
set of repetitions), the algorithmic bytes of that launch (vsr_stats.scan_bytes: rows * ceil(dim / 8) + bitmap bytes + k * 12)
over that device time, and the kernel that ran.  A one-query call is three launches (staging, K1b, K5): the difference between
the call and the scan launch is what the other two and the launch overheads cost.  There is no threshold.

    python tools/bit_probe.py OUT_DIR [--rows 10000000] [--queries 1000] [--reps 11]

Writes OUT_DIR/bitvec.json and prints it."""
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

K1_FP32_TB_PER_S = 5.65                                      # README: the brute-force fp32 kernel, 10M x 128


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--singles", type=int, default=20, help="one-query calls per repetition of legs (a) and (b)")
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    k, nq, reps, n = args.k, args.queries, max(args.reps, 3), args.rows
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx = vsrbac.Context(0)
    rng = np.random.default_rng(args.seed)
    blk = np.arange(n, dtype=np.int64)
    doc = (np.arange(n) // 100 + 1).astype(np.int32)

    def outputs(m):
        o = {"blk": torch.empty((m, k), dtype=torch.int64, device=dev), "doc": torch.empty((m, k), dtype=torch.int32, device=dev),
             "row": torch.empty((m, k), dtype=torch.int64, device=dev), "dist": torch.empty((m, k), dtype=torch.float32, device=dev),
             "cnt": torch.empty((m,), dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        return o

    def measure(call, calls_per_rep):
        for i in range(min(calls_per_rep, 3)):                # warm-up: code objects, workspaces, cached filters
            call(i)
        ctx.synchronize()
        secs = []
        for _ in range(reps):
            t = time.perf_counter()
            for i in range(calls_per_rep):
                call(i)
            ctx.synchronize()
            secs.append((time.perf_counter() - t) / calls_per_rep)
        ms = sorted(v * 1e3 for v in secs)
        ctx.profiling(2)
        ctx.stats_reset()
        for _ in range(reps):
            for i in range(calls_per_rep):
                call(i)
        st = ctx.stats()
        ctx.profiling(False)
        cls = 0 if st["scan_launches"][0] else 1
        launches, kms, nbytes = st["scan_launches"][cls], st["scan_ms"][cls], st["scan_bytes"][cls]
        calls = reps * calls_per_rep
        return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
                "calls_per_rep": calls_per_rep, "kernel": ctx.last_scan_kernel(), "scan_kernel_ms_per_call": round(kms / calls, 4),
                "scan_launches_per_call": launches / calls, "scan_bytes_per_call": int(nbytes // calls),
                "scan_pairs_per_call": int(st["scan_pairs"][cls] // calls),
                "scan_TB_per_s": round(nbytes / (kms * 1e-3) / 1e12, 3) if kms > 0 else None}

    report = {"device": ctx.device_info()["name"], "rows": n, "k": k, "reps": reps, "k1_fp32_TB_per_s_for_context": K1_FP32_TB_PER_S,
              "timing": "host clock around the call(s) and a synchronise, device-resident queries and results; scan_kernel_ms: HIP "
                        "events around the main scan launch (vsr_profiling level 2) in a second set of repetitions"}

    for leg, dim in (("a", 128), ("b", 1024)):
        rows = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
        corpus = ctx.load_corpus_bit(rows, dim, blk, doc)
        q = rows[rng.integers(0, n, max(nq, args.singles))] ^ rng.integers(0, 256, (max(nq, args.singles), dim // 8), dtype=np.uint8) & np.uint8(0x11)
        del rows
        d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        o1 = outputs(1)
        out = {"what": f"unfiltered, one query per call, {dim} bits", "dim": dim, "device_bytes": corpus.device_bytes()}
        for metric in ("hamming", "jaccard"):
            call = lambda i, m=metric: corpus.search_bit_device(ptr(d_q[i:i + 1]), 1, k, m, None, ptr(o1["blk"]), ptr(o1["doc"]),
                                                                ptr(o1["row"]), ptr(o1["dist"]), ptr(o1["cnt"]))
            out[metric] = measure(call, args.singles)
        report[leg] = out
        print(json.dumps({leg: out}), flush=True)
        if dim == 128:                                        # (c): the same rows under the tree RBAC
            rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
            corpus.load_rbac(rbac.user_roles, rbac.permissions)
            _, quser = sample_queries(nq, n, 1000, seed=args.seed)
            fl = corpus.pack_filters([corpus.filter_for_user(int(u), vsrbac.RANGES) for u in quser])
            ob = outputs(nq)
            out = {"what": f"{nq} queries per call, tree RBAC role pre-filter, {dim} bits", "dim": dim}
            for metric in ("hamming", "jaccard"):
                call = lambda i, m=metric: corpus.search_bit_device(ptr(d_q), nq, k, m, fl, ptr(ob["blk"]), ptr(ob["doc"]), ptr(ob["row"]),
                                                                    ptr(ob["dist"]), ptr(ob["cnt"]))
                out[metric] = measure(call, 1)
                out[metric]["queries_per_s"] = round(nq / (out[metric]["median_ms"] * 1e-3))
            report["c"] = out
            print(json.dumps({"c": out}), flush=True)
            del fl
        corpus.free()

    with open(os.path.join(args.out_dir, "bitvec.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))
    ctx.close()


if __name__ == "__main__":
    main()
