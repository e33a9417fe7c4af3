"""Sparse corpora (vsr_corpus_load_sparse, K1s) timed on one MI355X, in one process.

  data   1M rows of 30 522 dimensions with ~128 non-zeros (a SPLADE-like shape: indices drawn with a Zipf-like skew, positive
         values), queries of ~32 non-zeros drawn from the same index distribution, k = 100
  (a)    unfiltered, one query per call, <#> and <->
  (b)    1000 queries per call under the benchmark's tree RBAC (role pre-filter, class passes), <#> and <->

Queries and results are device-resident; a call is timed by the host clock around the call(s) and a synchronise.  Per leg:
median / min / max of the repetitions' time per call, the main scan launch's own device time (vsr_profiling level 2, a second
set of repetitions), the algorithmic bytes of that launch (vsr_stats.scan_bytes: 8 per stored entry + bitmap bytes + k * 12)
over that device time -- beside the HBM figures of the architecture guide, 8.0 TB/s peak and 6.29 TB/s measured for a float4
copy, as context: each row entry also costs a divergent LDS gather per query, and which of the two bounds K1s is what this
probe is for -- and the kernel that ran.  K1s has no kernel at the parent commit to be compared with; there is no threshold.

    python tools/sparse_probe.py OUT_DIR [--rows 1000000] [--queries 1000] [--reps 11]

Writes OUT_DIR/sparsevec.json and prints it."""
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

HBM_PEAK_TB_PER_S, HBM_COPY_TB_PER_S = 8.0, 6.29


def sparse_rows(rng, n, dim, mean_nnz):
    """CSR rows: Poisson(mean_nnz) entries per row (1 .. 16000), indices skewed towards the low ones, values in (0, 3]."""
    nnz = np.clip(rng.poisson(mean_nnz, n), 1, min(dim, 16000)).astype(np.int64)
    indptr = np.zeros(n + 1, dtype=np.int64)
    draw = (dim * rng.random(int(nnz.sum()) * 2) ** 2.5).astype(np.int64)      # oversampled: duplicates inside a row are dropped
    row_of = np.repeat(np.arange(n), nnz * 2)
    keys = np.unique(row_of * dim + draw)
    rows, idx = keys // dim, keys % dim
    keep = np.ones(keys.size, dtype=bool)                                       # at most nnz[r] entries of row r (a random subset would do
    first = np.searchsorted(rows, np.arange(n))                                 # as well: the first ones in index order keep the skew)
    keep[np.arange(keys.size) - first[rows] >= nnz[rows]] = False
    rows, idx = rows[keep], idx[keep]
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    values = (3.0 * (1.0 - rng.random(idx.size))).astype(np.float32)
    return indptr, idx.astype(np.int32), values


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=30522)
    ap.add_argument("--row-nnz", type=int, default=128)
    ap.add_argument("--query-nnz", type=int, default=32)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--singles", type=int, default=20, help="one-query calls per repetition of leg (a)")
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    k, nq, reps, n, dim = args.k, args.queries, max(args.reps, 3), args.rows, args.dim
    dev = torch.device("cuda", 0)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
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
        tbs = nbytes / (kms * 1e-3) / 1e12 if kms > 0 else None
        return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
                "calls_per_rep": calls_per_rep, "kernel": ctx.last_scan_kernel(), "scan_kernel_ms_per_call": round(kms / calls, 4),
                "scan_launches_per_call": launches / calls, "scan_bytes_per_call": int(nbytes // calls),
                "scan_pairs_per_call": int(st["scan_pairs"][cls] // calls),
                "scan_TB_per_s": round(tbs, 3) if tbs else None,
                "fraction_of_hbm_copy": round(tbs / HBM_COPY_TB_PER_S, 3) if tbs else None}

    indptr, indices, values = sparse_rows(rng, n, dim, args.row_nnz)
    corpus = ctx.load_corpus_sparse(indptr, indices, values, dim, blk, doc)
    report = {"device": ctx.device_info()["name"], "rows": n, "dim": dim, "k": k, "reps": reps,
              "mean_row_nnz": round(float(np.diff(indptr).mean()), 2), "device_bytes": corpus.device_bytes(),
              "hbm_TB_per_s_for_context": {"peak": HBM_PEAK_TB_PER_S, "float4_copy": HBM_COPY_TB_PER_S},
              "timing": "host clock around the call(s) and a synchronise, device-resident queries and results; scan_kernel_ms: HIP "
                        "events around the main scan launch (vsr_profiling level 2) in a second set of repetitions"}
    del indices, values
    m = max(nq, args.singles)
    q_ptr, q_idx, q_val = sparse_rows(rng, m, dim, args.query_nnz)
    max_nnz = int(np.diff(q_ptr).max())
    report["mean_query_nnz"] = round(float(np.diff(q_ptr).mean()), 2)
    d_ptr, d_idx, d_val = (torch.from_numpy(a).to(dev) for a in (q_ptr, q_idx, q_val))
    d_one = torch.from_numpy(np.stack([np.zeros(m, np.int64), np.diff(q_ptr)], axis=1).copy()).to(dev)   # per query: its own [0, nnz]
    torch.cuda.synchronize()

    o1 = outputs(1)
    out = {"what": "unfiltered, one query per call"}
    for metric, op in (("ip", "<#>"), ("l2", "<->")):
        call = lambda i, mt=metric: corpus.search_sparse_device(ptr(d_one, 16 * i), ptr(d_idx, 4 * int(q_ptr[i])), ptr(d_val, 4 * int(q_ptr[i])),
                                                                1, max_nnz, k, mt, None, ptr(o1["blk"]), ptr(o1["doc"]), ptr(o1["row"]),
                                                                ptr(o1["dist"]), ptr(o1["cnt"]))
        out[op] = measure(call, args.singles)
    report["a"] = out
    print(json.dumps({"a": out}), flush=True)

    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
    corpus.load_rbac(rbac.user_roles, rbac.permissions)
    _, quser = sample_queries(nq, n, 1000, seed=args.seed)
    fl = corpus.pack_filters([corpus.filter_for_user(int(u), vsrbac.RANGES) for u in quser])
    ob = outputs(nq)
    d_ptr_nq = d_ptr[:nq + 1]
    out = {"what": f"{nq} queries per call, tree RBAC role pre-filter"}
    for metric, op in (("ip", "<#>"), ("l2", "<->")):
        call = lambda i, mt=metric: corpus.search_sparse_device(ptr(d_ptr_nq), ptr(d_idx), ptr(d_val), nq, max_nnz, k, mt, fl, ptr(ob["blk"]),
                                                                ptr(ob["doc"]), ptr(ob["row"]), ptr(ob["dist"]), ptr(ob["cnt"]))
        out[op] = measure(call, 1)
        out[op]["queries_per_s"] = round(nq / (out[op]["median_ms"] * 1e-3))
    report["b"] = out
    print(json.dumps({"b": out}), flush=True)
    total, _ = ctx.screening_check()                          # raises if a staged query was refused
    del fl
    corpus.free()

    with open(os.path.join(args.out_dir, "sparsevec.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))
    ctx.close()


if __name__ == "__main__":
    main()
