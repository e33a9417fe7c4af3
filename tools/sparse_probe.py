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

Writes OUT_DIR/sparsevec.json and prints it.

    python tools/sparse_probe.py OUT_DIR --shared-ab

runs instead the A/B leg of K1sm (vsr_scansm.h, Context.set_sparse_shared) against K1s: the same corpus, 1000 device-resident
queries of ~32 non-zeros cut at 32 (one longer query keeps the whole call on K1s), k = 100, <#> and <->, unfiltered and under the
tree RBAC; a K1s window and a K1sm window alternate in one process, median [min, max] of 9 windows per kernel, and the two
kernels' outputs of the last windows are compared query by query (real values: distances within 1e-4, and how many queries got
the same rows).  Writes OUT_DIR/sparse_shared.json.

    python tools/sparse_probe.py OUT_DIR --compact-ab

runs in the same way the two A/B comparisons of K1sc (vsr_scansc.h, Context.set_sparse_compact): queries of ~30 non-zeros cut at
32, K1sm (QW = 16 there) against K1sc (QW = 32); queries of ~100 cut at 128, which K1sm does not serve, K1s against K1sc
(QW = 16).  Writes OUT_DIR/sparse_compact.json.

    python tools/sparse_probe.py OUT_DIR --inverted-ab

builds the corpus's inverted image (Corpus.build_sparse_inverted: its bytes and build time are recorded) and runs, in the same
way, K1si (vsr_scansi.h, Context.set_sparse_inverted) against K1sc at queries of ~30 non-zeros cut at 32 and of ~100 cut at 128,
and against K1s with one query per call (the first of the ~30 non-zero queries).  Writes OUT_DIR/sparse_inverted.json."""
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


def kernel_ab(args, out_name, comparisons):
    """Two sparse scan kernels in one resident process, timed alternately window by window.  comparisons: (label, Poisson mean of the
    queries' non-zeros, cut, kernel A, kernel B), a kernel being K1s, K1sm (Context.set_sparse_shared) or K1sc (set_sparse_compact);
    K1si (build_sparse_inverted + set_sparse_inverted); an optional sixth element gives the queries per call (default: all of them);
    the report has one section per label, or none at all for a single unlabelled comparison."""
    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, tree_rbac

    n, dim, nq, k, windows, calls = args.rows, args.dim, args.queries, args.k, 9, args.ab_calls
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(args.seed)
    ctx = vsrbac.Context(0)
    indptr, indices, values = sparse_rows(rng, n, dim, args.row_nnz)
    corpus = ctx.load_corpus_sparse(indptr, indices, values, dim, np.arange(n, dtype=np.int64), (np.arange(n) // 100 + 1).astype(np.int32))
    mean_row_nnz = round(float(np.diff(indptr).mean()), 2)
    del indices, values
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
    corpus.load_rbac(rbac.user_roles, rbac.permissions)
    _, quser = sample_queries(nq, n, 1000, seed=args.seed)
    report = {"device": ctx.device_info()["name"], "rows": n, "dim": dim, "mean_row_nnz": mean_row_nnz, "queries": nq, "k": k,
              "windows": windows, "calls_per_window": calls,
              "timing": "host clock around calls_per_window calls and a synchronise, device-resident queries and results; a window of "
                        "each kernel alternates in one process; ms per call: median / min / max over the windows"}
    if any("K1si" in c[3:5] for c in comparisons):
        before = corpus.device_bytes()
        ctx.synchronize()
        t = time.perf_counter()
        corpus.build_sparse_inverted()
        ctx.synchronize()
        report["inverted_image"] = {"build_ms": round((time.perf_counter() - t) * 1e3, 2), "bytes": corpus.device_bytes() - before, "corpus_bytes": before}
    all_nq = nq
    for label, query_nnz, cut, kind_a, kind_b, *per_call in comparisons:
        kinds = (kind_a, kind_b)
        nq = per_call[0] if per_call else all_nq
        q_ptr, q_idx, q_val = sparse_rows(rng, all_nq, dim, query_nnz)
        keep = np.arange(q_idx.size) - np.repeat(q_ptr[:-1], np.diff(q_ptr)) < cut           # the first `cut` entries of every query
        q_idx, q_val = q_idx[keep], q_val[keep]
        q_ptr = np.concatenate([[0], np.cumsum(np.minimum(np.diff(q_ptr), cut))]).astype(np.int64)
        max_nnz = int(np.diff(q_ptr).max())
        d_ptr, d_idx, d_val = (torch.from_numpy(a).to(dev) for a in (q_ptr, q_idx, q_val))
        out = {kind: {"blk": torch.zeros((nq, k), dtype=torch.int64, device=dev), "doc": torch.zeros((nq, k), dtype=torch.int32, device=dev),
                      "row": torch.zeros((nq, k), dtype=torch.int64, device=dev), "dist": torch.zeros((nq, k), dtype=torch.float32, device=dev),
                      "cnt": torch.zeros((nq,), dtype=torch.int32, device=dev)} for kind in kinds}
        torch.cuda.synchronize()
        section = report.setdefault(label, {}) if label else report
        section.update({"mean_query_nnz": round(float(np.diff(q_ptr).mean()), 2), "max_query_nnz": max_nnz, "queries_per_call": nq})
        legs = (("unfiltered", None), ("tree_rbac", corpus.pack_filters([corpus.filter_for_user(int(u), vsrbac.RANGES) for u in quser[:nq]])))
        ab_legs(ctx, corpus, legs, kinds, (d_ptr, d_idx, d_val), nq, max_nnz, k, windows, calls, out, ptr, section, label)
    ctx.screening_check()                                      # raises if a staged query was refused
    with open(os.path.join(args.out_dir, out_name), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    ctx.close()


def ab_legs(ctx, corpus, legs, kinds, queries, nq, max_nnz, k, windows, calls, out, ptr, section, label):
    d_ptr, d_idx, d_val = queries
    for leg, fl in legs:
        for metric, op in (("ip", "<#>"), ("l2", "<->")):
            ms, names = {kind: [] for kind in kinds}, {}

            def window(kind):
                ctx.set_sparse_shared(kind == "K1sm")
                ctx.set_sparse_compact(kind == "K1sc")
                ctx.set_sparse_inverted(kind == "K1si")
                o = out[kind]
                ctx.synchronize()
                t = time.perf_counter()
                for _ in range(calls):
                    corpus.search_sparse_device(ptr(d_ptr), ptr(d_idx), ptr(d_val), nq, max_nnz, k, metric, fl, ptr(o["blk"]), ptr(o["doc"]),
                                                ptr(o["row"]), ptr(o["dist"]), ptr(o["cnt"]))
                ctx.synchronize()
                names[kind] = ctx.last_scan_kernel()
                return (time.perf_counter() - t) / calls * 1e3

            for kind in kinds:
                window(kind)                                   # warm-up: code objects, workspaces, cached filters
            for _ in range(windows):
                for kind in kinds:
                    ms[kind].append(window(kind))
            a, b = ({f: t.cpu().numpy() for f, t in out[kind].items()} for kind in kinds)
            entry = {"counts_equal": bool((a["cnt"] == b["cnt"]).all()),
                     "distances_within_1e-4": bool(np.allclose(a["dist"], b["dist"], rtol=1e-4, atol=1e-4)),
                     "queries_with_the_same_rows": int((a["row"] == b["row"]).all(axis=1).sum())}
            for kind in kinds:
                v = sorted(ms[kind])
                entry[kind] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "kernel": names[kind]}
            entry[f"{kinds[1]}_over_{kinds[0]}".lower()] = round(entry[kinds[1]]["median_ms"] / entry[kinds[0]]["median_ms"], 3)
            section.setdefault(leg, {})[op] = entry
            print(json.dumps({label or "ab": {leg: {op: entry}}}), flush=True)
    ctx.set_sparse_shared(False)
    ctx.set_sparse_compact(False)
    ctx.set_sparse_inverted(False)


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
    ap.add_argument("--shared-ab", action="store_true", help="only the K1s / K1sm A/B leg: writes OUT_DIR/sparse_shared.json")
    ap.add_argument("--compact-ab", action="store_true", help="only the K1sm / K1sc and K1s / K1sc A/B legs: writes OUT_DIR/sparse_compact.json")
    ap.add_argument("--inverted-ab", action="store_true", help="only the K1sc / K1si and K1s / K1si (one query per call) A/B legs: writes OUT_DIR/sparse_inverted.json")
    ap.add_argument("--ab-calls", type=int, default=3, help="calls per window of the A/B leg")
    args = ap.parse_args()
    if args.shared_ab or args.compact_ab or args.inverted_ab:
        os.makedirs(args.out_dir, exist_ok=True)
        if args.inverted_ab:
            return kernel_ab(args, "sparse_inverted.json", [("short_queries_cut_at_32", 32, 32, "K1sc", "K1si"),
                                                            ("long_queries_cut_at_128", 100, 128, "K1sc", "K1si"),
                                                            ("one_query_per_call", 32, 32, "K1s", "K1si", 1)])
        if args.shared_ab:
            return kernel_ab(args, "sparse_shared.json", [(None, args.query_nnz, 32, "K1s", "K1sm")])
        return kernel_ab(args, "sparse_compact.json", [("short_queries_cut_at_32", 32, 32, "K1sm", "K1sc"),
                                                       ("long_queries_cut_at_128", 100, 128, "K1s", "K1sc")])

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
