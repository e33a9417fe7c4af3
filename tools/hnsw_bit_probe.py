"""HNSW over a bit corpus (K4b) beside the scans it replaces and beside the fp32 K4 on the same graph, in one process.

Corpus: `--rows` x `--dim` real-valued rows around `--centres` centres (vsrbac.datasets.gaussian_corpus for the centres and
the noise), their binary_quantize as a bit corpus, the graph from vsr_hnsw_build_bit (Hamming, merging).  `--queries` queries
(corpus rows plus noise), device-resident; a call is timed by the host clock around the call and a synchronise, median of
`--reps`.

  build      vsr_hnsw_build_bit, merged and unmerged: seconds, elements
  k4b        vsr_hnsw_search_bit_device at ef_search 40 / 100 / 400: queries/s, recall@10 against vsr_search_bit (tie-aware:
             a returned row counts when it is no farther than the exact 10th), mean visited elements
  k1b        vsr_search_bit_device for the same queries (the exact scan of every row)
  k4_fp32    vsr_hnsw_search_device over the SAME graph loaded on the rows unpacked to 0 / 1 floats: the walk and the visited
             counts are the same (checked), so the difference is the row format and the lane mapping
  two_stage  vsr_hnsw_search_quantized_device against vsr_search_quantized_device at shortlist 100 / 400, time and recall@10
             against vsr_search, unfiltered and under the tree RBAC (bitmap filters) with the predicate-aware walk

    python tools/hnsw_bit_probe.py OUT_DIR [--rows 1000000] [--dim 768] [--queries 1000] [--reps 5]

Writes OUT_DIR/hnsw_bit.json and prints it."""
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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--centres", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20251121)
    ap.add_argument("--skip-fp32", action="store_true", help="leave out the fp32 K4 leg (it needs rows x dim x 4 bytes twice)")
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import gaussian_corpus, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    n, dim, nq, k = args.rows, args.dim, args.queries, 10
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(args.seed)

    centres, _, _ = gaussian_corpus(args.centres, dim, seed=args.seed + 1)
    x, blk, doc = gaussian_corpus(n, dim, seed=args.seed)
    x *= np.float32(0.6)
    x += centres[rng.integers(0, args.centres, n)]
    q = x[rng.integers(0, n, nq)] + np.float32(0.3) * rng.standard_normal((nq, dim)).astype(np.float32)

    ctx = vsrbac.Context(0)
    source = ctx.load_corpus(x, blk, doc)
    bits = source.binary_quantize()
    ndocs = int(doc.max())
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=ndocs, seed=args.seed)
    bits.load_rbac(rbac.user_roles, rbac.permissions)
    source.load_rbac(rbac.user_roles, rbac.permissions)
    users = rng.integers(1, 1001, nq)
    qb = ctx.binary_quantize(q)
    out = {"rows": n, "dim": dim, "queries": nq, "k": k, "reps": args.reps, "device": ctx.device_info()["name"]}

    def timed(fn):
        ts = []
        for _ in range(args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
            del keep
        return float(np.median(ts))

    def outputs(kk):
        return {"blk": torch.empty((nq, kk), dtype=torch.int64, device=dev), "doc": torch.empty((nq, kk), dtype=torch.int32, device=dev),
                "row": torch.empty((nq, kk), dtype=torch.int64, device=dev), "dist": torch.empty((nq, kk), dtype=torch.float32, device=dev),
                "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.zeros((nq,), dtype=torch.int64, device=dev)}

    # ---- builds ----
    out["build"] = {}
    index = None
    for name, merge in (("unmerged", False), ("merged", True)):
        t0 = time.perf_counter()
        h = bits.build_hnsw_bit(16, 64, "hamming", seed=1, merge_duplicates=merge)
        out["build"][name] = {"seconds": time.perf_counter() - t0, "elements": h.info()[0]}
        if merge:
            index = h
        else:
            h.free()

    # ---- K1b, K4b ----
    d_qb = torch.from_numpy(qb).to(dev)
    o = outputs(k)
    t = timed(lambda: bits.search_bit_device(ptr(d_qb), nq, k, "hamming", None, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]),
                                             ptr(o["cnt"])))
    exact_d = o["dist"].cpu().numpy().copy()
    out["k1b"] = {"seconds_per_call": t, "queries_per_s": nq / t}
    out["k4b"] = {}
    visited = {}
    for ef in (40, 100, 400):
        t = timed(lambda: index.search_bit_device(ptr(d_qb), nq, k, ef, "hamming", None, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]),
                                                  ptr(o["dist"]), ptr(o["cnt"]), ptr(o["vis"])))
        d, cnt = o["dist"].cpu().numpy(), o["cnt"].cpu().numpy()
        hits = sum(int((d[i, :max(cnt[i], 0)] <= exact_d[i, k - 1]).sum()) for i in range(nq))
        visited[ef] = o["vis"].cpu().numpy().copy()
        out["k4b"][str(ef)] = {"seconds_per_call": t, "queries_per_s": nq / t, "recall_at_10": hits / (nq * k),
                               "mean_visited": float(visited[ef].mean()), "overflowed": int((cnt < 0).sum())}

    # ---- the fp32 K4 over the same graph, rows unpacked to 0 / 1 floats ----
    if not args.skip_fp32:
        packed = np.concatenate([ctx.binary_quantize(x[i:i + 100_000]) for i in range(0, n, 100_000)])
        unpacked = np.unpackbits(packed, axis=1)[:, :dim].astype(np.float32)
        fcorpus = ctx.load_corpus(unpacked, blk, doc)
        findex = fcorpus.load_hnsw(index.export())
        d_qf = torch.from_numpy(np.unpackbits(qb, axis=1)[:, :dim].astype(np.float32)).to(dev)
        out["k4_fp32"] = {}
        for ef in (40, 100, 400):
            t = timed(lambda: findex.search_device(ptr(d_qf), nq, k, ef, "l2", None, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]),
                                                   ptr(o["dist"]), ptr(o["cnt"]), ptr(o["vis"])))
            same = bool((o["vis"].cpu().numpy() == visited[ef]).all())
            out["k4_fp32"][str(ef)] = {"seconds_per_call": t, "queries_per_s": nq / t, "same_visited_counts": same,
                                       "k4b_speedup": t / out["k4b"][str(ef)]["seconds_per_call"]}
        findex.free()
        fcorpus.free()
        del unpacked, packed

    # ---- two-stage: the indexed shortlist against the scanned one ----
    d_q = torch.from_numpy(q).to(dev)
    out["two_stage"] = {}
    for leg in ("unfiltered", "tree_rbac"):
        flt_b = None if leg == "unfiltered" else [bits.filter_for_user(int(u), vsrbac.BITMAP) for u in users]
        flt_s = None if leg == "unfiltered" else [source.filter_for_user(int(u), vsrbac.BITMAP) for u in users]
        truth = source.search(q, k, "l2", flt_s)
        index.set_predicate_aware(leg != "unfiltered")

        def recall():
            rows, cnt = o["row"].cpu().numpy(), o["cnt"].cpu().numpy()
            hits = sum(len(set(rows[i, :max(cnt[i], 0)].tolist()) & set(truth.rows[i, :truth.counts[i]].tolist())) for i in range(nq))
            return hits / max(1, int(truth.counts.sum()))

        out["two_stage"][leg] = {}
        for shortlist in (100, 400):
            e = {}
            t = timed(lambda: source.search_quantized_device(bits, ptr(d_q), nq, k, shortlist, "l2", flt_b, ptr(o["blk"]), ptr(o["doc"]),
                                                             ptr(o["row"]), ptr(o["dist"]), ptr(o["cnt"])))
            e["scanned"] = {"seconds_per_call": t, "recall_at_10": recall()}
            for ef in (40, 100, 400):
                if ef < shortlist and ef != 400:
                    continue                                 # a beam narrower than the shortlist cannot fill it
                t = timed(lambda: source.search_quantized_hnsw_device(index, ptr(d_q), nq, k, shortlist, ef, "l2", flt_b, ptr(o["blk"]),
                                                                      ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]), ptr(o["cnt"])))
                e[f"indexed_ef{ef}"] = {"seconds_per_call": t, "recall_at_10": recall()}
            out["two_stage"][leg][str(shortlist)] = e
    index.set_predicate_aware(False)

    path = os.path.join(args.out_dir, "hnsw_bit.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
