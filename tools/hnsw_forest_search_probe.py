"""One forest call for a query's partition graphs (vsr_hnsw_forest_search_device) against what a caller could do before it.

tools/hnsw_partitions_probe.py's corpus: 1M x 128 SIFT-like fp32 rows in 100 disjoint partitions of 10 000 rows (document g + 1 holds
partition g's rows), m = 16, ef_construction = 64, L2, the graphs from one build_hnsw_partitions call.  1000 device-resident
queries per call, each over T = 1 / 8 / 32 random partitions, k = 10, ef_search 40 / 100.  Three legs, every one ending with the
merged results in host memory:

  (a) forest     ONE HnswForest.search_device call, the copy back;
  (b) per graph  the queries grouped by graph (one device gather), one HnswIndex.search_device per graph that has a query, the
                 copy back, the merge on the host (numpy, vectorised over the queries: one lexsort per call);
  (c) exact      Corpus.search_device over the (query, partition filter) pairs (the filter array packed once, outside the windows), the
                 copy back, the same host merge: what Deployment.dynamic_partition_search does today.

The legs alternate; a window repeats one leg for ~0.25 s; the median of 9 windows, min and max, in ms per call.  recall@10 of (a)
against (c), and (a)'s rows against (b)'s for every query (they must be equal).

With --parent-lib: an A/B of vsr_hnsw_search_device itself, this library against the parent commit's, on a 120 000-row graph
(tools/hnsw_build_probe.py's rows), one resident process per library and a second process of this library as a control, 5 runs
each, alternating.

    python tools/hnsw_forest_search_probe.py [--parent-lib PATH] [--out profiles/hnsw_forest_search.json]

Prints one JSON record and writes it to --out; progress goes to stderr."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

M, EFC, DIM, K = 16, 64, 128, 10
NEW_SYMBOLS = ("vsr_hnsw_forest_open", "vsr_hnsw_forest_free", "vsr_hnsw_forest_set_predicate_aware", "vsr_hnsw_forest_search",
               "vsr_hnsw_forest_search_device", "vsr_hnsw_forest_search_bit", "vsr_hnsw_forest_search_bit_device")


def corpus_rows(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.abs(rng.normal(0, 45, (n, DIM)))), 0, 255).astype(np.float32)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def host_merge(blk, doc, row, dist, nq, t):
    """[nq * t, K] per-task results, task (i, j) at row i * t + j, -> the K best distinct rows per query by (dist, doc, blk)."""
    blk, doc, row, dist = (a.reshape(nq, t * K) for a in (blk, doc, row, dist))
    order = np.lexsort((blk, doc, dist), axis=-1)                             # (empty slots: +Inf, last)
    r = np.take_along_axis(row, order, -1)
    valid = r >= 0
    valid[:, 1:] &= r[:, 1:] != r[:, :-1]                                     # a repeated row has equal keys: its copies are neighbours
    rank = np.cumsum(valid, -1) - 1
    ii, jj = np.nonzero(valid & (rank < K))
    out = np.full((nq, K), -1, dtype=np.int64)
    out[ii, rank[ii, jj]] = r[ii, jj]
    return out


def legs(args):
    import torch
    import vsrbac
    dev = torch.device("cuda", 0)
    n_parts, size = args.partitions, args.rows // args.partitions
    ctx = vsrbac.Context(0)
    x = corpus_rows(args.rows, args.seed)
    perm = np.random.default_rng([args.seed, n_parts]).permutation(args.rows)
    parts = [np.sort(perm[g * size:(g + 1) * size]).astype(np.int64) for g in range(n_parts)]
    doc = np.zeros(args.rows, dtype=np.int32)
    for g, p in enumerate(parts):
        doc[p] = g + 1
    corpus = ctx.load_corpus(x, np.arange(1, args.rows + 1, dtype=np.int64), doc)
    t0 = time.perf_counter()
    indexes = corpus.build_hnsw_partitions(parts, M, EFC, "l2", args.seed)
    print(f"built {n_parts} graphs in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    forest = corpus.hnsw_forest(indexes)
    part_filter = [corpus.filter_from_documents([g + 1], -1) for g in range(n_parts)]
    rng = np.random.default_rng(args.seed + 1)
    nq = args.queries
    q = x[rng.integers(0, args.rows, nq)] + rng.integers(-3, 4, (nq, DIM)).astype(np.float32)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    out = []
    for t in args.tasks:
        graphs = np.stack([rng.choice(n_parts, t, replace=False) for _ in range(nq)]).astype(np.int32)       # [nq, t]
        q_off = np.arange(nq + 1, dtype=np.int64) * t
        nt = nq * t
        big = {"blk": torch.empty((nt, K), dtype=torch.int64, device=dev), "doc": torch.empty((nt, K), dtype=torch.int32, device=dev),
               "row": torch.empty((nt, K), dtype=torch.int64, device=dev), "dist": torch.empty((nt, K), dtype=torch.float32, device=dev),
               "cnt": torch.empty((nt,), dtype=torch.int32, device=dev)}
        small = {key: torch.empty((nq,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for key, v in big.items()}
        packed = corpus.pack_filters([part_filter[g] for g in graphs.reshape(-1)])   # (built once per shape, outside the windows)
        torch.cuda.synchronize()
        for ef in args.ef:
            def leg_a():
                keep = forest.search_device(ptr(d_q), nq, (q_off, graphs.reshape(-1)), K, ef, "l2", None, ptr(small["blk"]), ptr(small["doc"]),
                                            ptr(small["row"]), ptr(small["dist"]), ptr(small["cnt"]))
                ctx.synchronize()
                del keep
                assert int(small["cnt"].min()) >= 0, "a visited table overflowed: the device form has no result for that query"
                return small["row"].cpu().numpy()

            def leg_b():
                order = np.argsort(graphs.reshape(-1), kind="stable")                                        # tasks grouped by graph
                bounds = np.searchsorted(graphs.reshape(-1)[order], np.arange(n_parts + 1))
                d_sel = d_q[torch.from_numpy(order // t).to(dev)]
                torch.cuda.synchronize()
                for g in range(n_parts):
                    a, b = int(bounds[g]), int(bounds[g + 1])
                    if b > a:
                        indexes[g].search_device(ptr(d_sel[a:]), b - a, K, ef, "l2", None, ptr(big["blk"][a:]), ptr(big["doc"][a:]),
                                                 ptr(big["row"][a:]), ptr(big["dist"][a:]), ptr(big["cnt"][a:]))
                ctx.synchronize()
                inv = np.argsort(order)
                return host_merge(*(big[key].cpu().numpy()[inv] for key in ("blk", "doc", "row", "dist")), nq, t)

            def leg_c():
                d_rep = d_q.repeat_interleave(t, dim=0)
                torch.cuda.synchronize()
                keep = corpus.search_device(ptr(d_rep), nt, K, "l2", packed, ptr(big["blk"]), ptr(big["doc"]), ptr(big["row"]),
                                            ptr(big["dist"]), ptr(big["cnt"]))
                ctx.synchronize()
                del keep
                return host_merge(*(big[key].cpu().numpy() for key in ("blk", "doc", "row", "dist")), nq, t)

            fns = {"forest": leg_a, "per_graph": leg_b, "exact": leg_c}
            rows = {name: fn() for name, fn in fns.items()}                                                  # warm-up, and the answers
            equal = bool((rows["forest"] == rows["per_graph"]).all())
            recall = float(np.mean([len(set(rows["forest"][i]) & set(rows["exact"][i])) / K for i in range(nq)]))
            ms = {name: [] for name in fns}
            for _ in range(args.windows):                                                                    # the legs alternate
                for name, fn in fns.items():
                    n, t0 = 0, time.perf_counter()
                    while True:
                        fn()
                        n += 1
                        dt = time.perf_counter() - t0
                        if dt >= args.window_s:
                            break
                    ms[name].append(dt / n * 1e3)
            rec = {"tasks_per_query": t, "ef_search": ef, "forest_equals_per_graph": equal, "recall_at_10_vs_exact": recall,
                   "ms_per_call": {name: summary(v) for name, v in ms.items()}}
            rec["forest_speedup_over_per_graph"] = rec["ms_per_call"]["per_graph"]["median"] / rec["ms_per_call"]["forest"]["median"]
            rec["forest_speedup_over_exact"] = rec["ms_per_call"]["exact"]["median"] / rec["ms_per_call"]["forest"]["median"]
            print(json.dumps(rec), file=sys.stderr, flush=True)
            out.append(rec)
    forest.free()
    for h in indexes:
        h.free()
    corpus.free()
    ctx.close()
    return out


def ab_worker(args):
    """A resident process over the 120 000-row graph: `run` on stdin -> ms per vsr_hnsw_search_device call, one JSON line."""
    import torch
    from vsrbac import _ffi
    lib = C.CDLL(_ffi.library_path())
    for name in NEW_SYMBOLS:
        if not hasattr(lib, name):
            _ffi.SYMBOLS.pop(name, None)
    import vsrbac
    dev = torch.device("cuda", 0)
    ctx = vsrbac.Context(0)
    x = corpus_rows(args.ab_rows, args.seed)
    corpus = ctx.load_corpus(x)
    index = corpus.build_hnsw(M, EFC, "l2", seed=args.seed)
    rng = np.random.default_rng(args.seed + 2)
    nq = args.queries
    d_q = torch.from_numpy(np.ascontiguousarray(x[rng.integers(0, args.ab_rows, nq)] + 1.0)).to(dev)
    o = [torch.empty((nq, K), dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int64, torch.float32)]
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"ready": True, "lib": _ffi.library_path()}), flush=True)
    for line in sys.stdin:
        if line.split()[:1] != ["run"]:
            break
        res = {}
        for ef in args.ef:
            for _ in range(3):
                index.search_device(ptr(d_q), nq, K, ef, "l2", None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(cnt))
            ctx.synchronize()
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < args.window_s:
                index.search_device(ptr(d_q), nq, K, ef, "l2", None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(cnt))
                ctx.synchronize()
                n += 1
            res[str(ef)] = (time.perf_counter() - t0) / n * 1e3
        res["rows_checksum"] = int(o[2].sum().item())
        print(json.dumps(res), flush=True)
    index.free()
    corpus.free()
    ctx.close()


class Worker:
    def __init__(self, args, lib):
        env = dict(os.environ)
        if lib:
            env["VSRBAC_LIB"] = lib
        else:
            env.pop("VSRBAC_LIB", None)
        self.err = tempfile.TemporaryFile(mode="w+")
        cmd = [sys.executable, os.path.abspath(__file__), "--ab-worker", "--ab-rows", str(args.ab_rows), "--seed", str(args.seed),
               "--queries", str(args.queries), "--window-s", str(args.window_s), "--ef"] + [str(e) for e in args.ef]
        self.p = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=self.err, text=True)
        self.ready = self._reply()

    def _reply(self):
        line = self.p.stdout.readline()
        if not line:
            self.err.seek(0)
            raise RuntimeError("worker ended: " + self.err.read()[-2000:])
        return json.loads(line)

    def run(self):
        self.p.stdin.write("run\n")
        self.p.stdin.flush()
        return self._reply()

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.close()
        rc = self.p.wait(timeout=120)
        self.err.close()
        if rc != 0:
            raise RuntimeError(f"worker exit {rc}")


def existing_kernel_ab(args, parent):
    # control: a second process of THIS library, so that what two processes of one library differ by is on record beside the A/B
    new, old, ctl = Worker(args, None), Worker(args, parent), Worker(args, None)
    runs = {"this": [], "parent": [], "control": []}
    for run in range(args.ab_runs):                                           # alternating
        runs["parent"].append(old.run())
        runs["this"].append(new.run())
        runs["control"].append(ctl.run())
        print(f"A/B run {run}: parent {runs['parent'][-1]}, this {runs['this'][-1]}, control {runs['control'][-1]}", file=sys.stderr, flush=True)
    for w in (new, old, ctl):
        w.close()
    rec = {"rows": args.ab_rows, "queries_per_call": args.queries, "runs": args.ab_runs, "same_rows": runs["this"][0]["rows_checksum"] ==
           runs["parent"][0]["rows_checksum"], "ef_search": {}}
    for ef in args.ef:
        a, b = summary([r[str(ef)] for r in runs["this"]]), summary([r[str(ef)] for r in runs["parent"]])
        rec["ef_search"][str(ef)] = {"this_ms": a, "parent_ms": b, "control_this_library_again_ms": summary([r[str(ef)] for r in runs["control"]]),
                                     "difference_of_medians_ms": a["median"] - b["median"],
                                     "parent_spread_ms": b["max"] - b["min"],
                                     "inside_parent_spread": b["min"] <= a["median"] <= b["max"]}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--tasks", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--ef", type=int, nargs="*", default=[40, 100])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ab-rows", type=int, default=120_000)
    ap.add_argument("--ab-runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libvsrbac.so of the parent commit: adds the A/B of vsr_hnsw_search_device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_forest_search.json"))
    ap.add_argument("--ab-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ab_worker:
        return ab_worker(args)
    rec = {"probe": "hnsw_forest_search", "rows": args.rows, "dim": DIM, "partitions": args.partitions, "m": M, "ef_construction": EFC,
           "metric": "l2", "k": K, "queries_per_call": args.queries, "windows": args.windows, "window_s": args.window_s}
    if args.parent_lib and os.path.exists(args.parent_lib):                   # first: its processes end before the big corpus loads
        rec["existing_kernel_ab"] = existing_kernel_ab(args, os.path.abspath(args.parent_lib))
    rec["configs"] = legs(args)
    text = json.dumps(rec, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
