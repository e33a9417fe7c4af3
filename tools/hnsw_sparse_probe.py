"""HNSW over a sparse corpus (K4s) beside the exact scan (K1s) on the same queries, in one process.

Corpus: tools/sparse_probe.py's -- `--rows` rows of `--dim` dimensions with ~`--row-nnz` non-zeros (a SPLADE-like shape: indices
drawn with a Zipf-like skew, positive values; rows longer than the index's 1000 non-zeros are cut), queries of ~`--query-nnz`
non-zeros from the same index distribution.  The graphs come from vsr_hnsw_build_sparse (m = 16, ef_construction = 64), one per
operator.  Device-resident queries, `--queries` per call, k = 10, operators <#> and <->.  There is no parent kernel to compare
with and no number is fixed in advance; the yardstick is vsr_search_sparse_device on the same queries.

  build     vsr_hnsw_build_sparse per operator: seconds, elements
  k4s, k1s  vsr_hnsw_search_sparse_device at ef_search 40 / 100 / 400 and vsr_search_sparse_device: after a warm-up, `--reps` timed
            windows per leg, the two legs alternating; a window is as many back-to-back calls as fill ~0.25 s, closed by a
            synchronise; seconds per call = the median window / its calls (min and max recorded).  queries/s, mean visited
            elements, recall@10 against the exact scan (tie-aware: a returned row counts when it is no farther than the exact
            scan's 10th)
  ratio     k1s seconds per call / k4s seconds per call at each ef_search (above 1: the index is faster)
  bytes     vsr_corpus_device_bytes, vsr_hnsw_device_bytes

    python tools/hnsw_sparse_probe.py OUT_DIR [--rows 1000000] [--queries 1000] [--reps 9]

Writes OUT_DIR/hnsw_sparsevec.json and prints it."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from sparse_probe import sparse_rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out_dir")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=30522)
    ap.add_argument("--row-nnz", type=int, default=128)
    ap.add_argument("--query-nnz", type=int, default=32)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac

    os.makedirs(args.out_dir, exist_ok=True)
    n, dim, nq, k = args.rows, args.dim, args.queries, 10
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(args.seed)

    ip, ix, vx = sparse_rows(rng, n, dim, args.row_nnz)
    lens = np.diff(ip)
    if lens.max() > 1000:                                    # HNSW_MAX_NNZ: keep the first 1000 entries of a longer row
        keep = np.arange(ix.size) - np.repeat(ip[:-1], lens) < 1000
        ix, vx = ix[keep], vx[keep]
        ip = np.concatenate([[0], np.cumsum(np.minimum(lens, 1000))]).astype(np.int64)
    qp, qi, qv = sparse_rows(rng, nq, dim, args.query_nnz)
    max_q = int(np.diff(qp).max())

    ctx = vsrbac.Context(0)
    out = {"probe": "hnsw_sparsevec", "rows": n, "dim": dim, "row_nnz_mean": float(np.diff(ip).mean()),
           "query_nnz_mean": float(np.diff(qp).mean()), "queries": nq, "k": k, "reps": args.reps, "m": 16, "ef_construction": 64,
           "device": ctx.device_info()["name"], "operators": {}}
    corpus = ctx.load_corpus_sparse(ip, ix, vx, dim)
    out["corpus_device_bytes"] = corpus.device_bytes()
    d_qp, d_qi, d_qv = (torch.from_numpy(a).to(dev) for a in (qp, qi, qv))

    def outputs():
        return {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
                "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
                "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.zeros((nq,), dtype=torch.int64, device=dev)}

    for metric in ("ip", "l2"):
        ctx.synchronize()
        t0 = time.perf_counter()
        index = corpus.build_hnsw_sparse(16, 64, metric, seed=1)
        ctx.synchronize()
        res = {"build_seconds": time.perf_counter() - t0, "elements": index.info()[0], "index_device_bytes": index.device_bytes(),
               "k4s": {}, "ratio_k1s_over_k4s": {}}
        o_idx, o_scan = outputs(), outputs()

        def call(name, ef):
            if name == "k4s":
                return index.search_sparse_device(ptr(d_qp), ptr(d_qi), ptr(d_qv), nq, max_q, k, ef, metric, None, ptr(o_idx["blk"]),
                                                  ptr(o_idx["doc"]), ptr(o_idx["row"]), ptr(o_idx["dist"]), ptr(o_idx["cnt"]),
                                                  ptr(o_idx["vis"]))
            return corpus.search_sparse_device(ptr(d_qp), ptr(d_qi), ptr(d_qv), nq, max_q, k, metric, None, ptr(o_scan["blk"]),
                                               ptr(o_scan["doc"]), ptr(o_scan["row"]), ptr(o_scan["dist"]), ptr(o_scan["cnt"]))

        def window(name, ef, calls):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                call(name, ef)
            ctx.synchronize()
            return (time.perf_counter() - t0) / calls

        for ef in (40, 100, 400):
            calls = {}
            for name in ("k4s", "k1s"):                      # warm-up, and how many calls fill a window
                window(name, ef, 2)
                calls[name] = max(1, int(0.25 / window(name, ef, 2)))
            times = {"k4s": [], "k1s": []}
            for _ in range(args.reps):
                for name in times:                           # alternating: both legs see the same neighbours on the machine
                    times[name].append(window(name, ef, calls[name]))
            rows, dist, cnt = o_idx["row"].cpu().numpy(), o_idx["dist"].cpu().numpy(), o_idx["cnt"].cpu().numpy()
            e_dist, e_cnt = o_scan["dist"].cpu().numpy(), o_scan["cnt"].cpu().numpy()
            hits = total = 0
            for i in range(nq):                              # tie-aware: no farther than the exact scan's last row
                if e_cnt[i] > 0:
                    hits += int((dist[i, :max(cnt[i], 0)] <= e_dist[i, e_cnt[i] - 1]).sum())
                    total += int(e_cnt[i])
            stat = lambda t: {"seconds_per_call": float(np.median(t)), "seconds_per_call_min": float(min(t)),
                              "seconds_per_call_max": float(max(t)), "queries_per_s": nq / float(np.median(t))}
            res["k4s"][str(ef)] = dict(stat(times["k4s"]), calls_per_window=calls["k4s"], recall_at_10=hits / max(1, total),
                                       mean_visited=float(o_idx["vis"].cpu().numpy().mean()), overflowed=int((cnt < 0).sum()))
            res.setdefault("k1s", {})[str(ef)] = dict(stat(times["k1s"]), calls_per_window=calls["k1s"])
            res["ratio_k1s_over_k4s"][str(ef)] = res["k1s"][str(ef)]["seconds_per_call"] / res["k4s"][str(ef)]["seconds_per_call"]
        out["operators"][metric] = res
        index.free()
    out["guard"] = int(ctx.screening_check()[0])

    path = os.path.join(args.out_dir, "hnsw_sparsevec.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
