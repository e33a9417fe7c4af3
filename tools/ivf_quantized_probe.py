"""The two-stage search through the bit IVFFlat index (K3q + the shortlist re-rank) beside the forms it competes with, same corpus,
same device-resident queries, one process.

Corpus: the one of tools/hnsw_bit_probe.py / ivf_bit_probe.py -- `--rows` x `--dim` real-valued rows around `--centres` centres as
an fp32 corpus, its binary_quantize as a bit corpus, the tree RBAC of the benchmark on both.  Over the bit corpus: the IVFFlat
index as Corpus.build_ivf_bit builds it (`--lists` lists) and the merged Hamming HNSW graph of tools/hnsw_bit_probe.py (m 16,
ef_construction 64).  k = 10, L2.

  points     shortlist 100 / 400 x probes 1 / 10 / 32 x {unfiltered, tree RBAC} x {iterative scan off, relaxed_order with
             max_probes `--max-probes`}.  Per point, after a warm-up, `--reps` timed windows per leg, the legs alternating; a
             window is as many back-to-back calls as fill ~0.25 s; seconds per call = the median window / its calls (min and max
             recorded).  Legs:
               ivf_quantized   vsr_ivf_search_quantized_device                              (the new call)
               scanned         vsr_search_quantized_device                                  (K1b over all rows + re-rank)
               hnsw            vsr_hnsw_search_quantized_device at ef_search = shortlist    (K4b + re-rank; predicate-aware
                               walk under the RBAC, bitmap filters, as tools/hnsw_bit_probe.py)
               ivf_stage1      vsr_ivf_search_bit_device at k = shortlist and the point's probes: stage 1 by the shared passes
                               with NO re-rank -- a lower bound of what chaining the existing calls could reach
             and recall@10 of the first three against vsr_search over the source under the same filter, mean count, mean lists
             scanned.
  ratio_*    yardstick seconds per call / ivf_quantized seconds per call (above 1: the new call is faster).  No threshold.

    python tools/ivf_quantized_probe.py OUT_DIR [--rows 1000000] [--dim 768] [--lists 1000] [--queries 1000] [--reps 9]

Writes OUT_DIR/ivf_quantized.json and prints it."""
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
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-probes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=20251121)
    ap.add_argument("--no-hnsw", action="store_true", help="leave out the graph leg (and its build)")
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import gaussian_corpus, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    n, dim, nq, k, lists = args.rows, args.dim, args.queries, 10, args.lists
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
    packed = np.concatenate([ctx.binary_quantize(x[i:i + 100_000]) for i in range(0, n, 100_000)])
    del x
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=int(doc.max()), seed=args.seed)
    bits.load_rbac(rbac.user_roles, rbac.permissions)
    source.load_rbac(rbac.user_roles, rbac.permissions)
    users = rng.integers(1, 1001, nq)
    qb = ctx.binary_quantize(q)
    out = {"probe": "ivf_quantized", "rows": n, "dim": dim, "lists": lists, "queries": nq, "k": k, "reps": args.reps, "metric": "l2",
           "max_probes": args.max_probes, "device": ctx.device_info()["name"]}

    t0 = time.perf_counter()
    index, _, row_list = bits.build_ivf_bit(packed, lists, seed=1)
    sizes = np.bincount(row_list, minlength=lists)
    out["build"] = {"ivf_seconds": time.perf_counter() - t0, "empty_lists": int((sizes == 0).sum()), "largest_list": int(sizes.max())}
    del packed
    graph = None
    if not args.no_hnsw:
        t0 = time.perf_counter()
        graph = bits.build_hnsw_bit(16, 64, "hamming", seed=1, merge_duplicates=True)
        out["build"]["hnsw_seconds"] = time.perf_counter() - t0
    print(json.dumps({"build": out["build"]}), flush=True)

    d_q, d_qb = torch.from_numpy(q).to(dev), torch.from_numpy(qb).to(dev)
    ranges = [bits.filter_for_user(int(u), vsrbac.RANGES) for u in users]
    bitmaps = [bits.filter_for_user(int(u), vsrbac.BITMAP) for u in users]
    filters = {"none": None, "tree_rbac": bits.pack_filters(ranges)}
    graph_filters = {"none": None, "tree_rbac": bits.pack_filters(bitmaps)}
    truth = {"none": source.search(q, k, "l2"),
             "tree_rbac": source.search(q, k, "l2", [source.filter_for_user(int(u), vsrbac.RANGES) for u in users])}

    def outputs(kk):
        return {"blk": torch.empty((nq, kk), dtype=torch.int64, device=dev), "doc": torch.empty((nq, kk), dtype=torch.int32, device=dev),
                "row": torch.empty((nq, kk), dtype=torch.int64, device=dev), "dist": torch.empty((nq, kk), dtype=torch.float32, device=dev),
                "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "probes": torch.zeros((nq,), dtype=torch.int32, device=dev)}

    legs = ["ivf_quantized", "scanned"] + ([] if graph is None else ["hnsw"]) + ["ivf_stage1"]
    o = {name: outputs(k) for name in legs}
    wide = {s: outputs(s) for s in (100, 400)}                 # stage 1 alone returns the whole shortlist

    def call(name, point):
        shortlist, probes, filt, mode = point
        w = o[name]
        res = (ptr(w["blk"]), ptr(w["doc"]), ptr(w["row"]), ptr(w["dist"]), ptr(w["cnt"]))
        if name == "ivf_quantized":
            source.search_quantized_ivf_device(index, ptr(d_q), nq, k, shortlist, probes, "l2", filters[filt], mode, args.max_probes, *res,
                                               ptr(w["probes"]))
        elif name == "scanned":
            source.search_quantized_device(bits, ptr(d_q), nq, k, shortlist, "l2", filters[filt], *res)
        elif name == "hnsw":
            source.search_quantized_hnsw_device(graph, ptr(d_q), nq, k, shortlist, shortlist, "l2", graph_filters[filt], *res)
        else:
            w = wide[shortlist]
            index.search_bit_device(ptr(d_qb), nq, shortlist, probes, "hamming", filters[filt], ptr(w["blk"]), ptr(w["doc"]), ptr(w["row"]),
                                    ptr(w["dist"]), ptr(w["cnt"]))

    def window(name, point, calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call(name, point)
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls

    def recall(name, filt):
        rows, cnt = o[name]["row"].cpu().numpy(), o[name]["cnt"].cpu().numpy()
        ex = truth[filt]
        hits = sum(len(set(rows[i, :max(cnt[i], 0)].tolist()) & set(ex.rows[i, :ex.counts[i]].tolist())) for i in range(nq))
        return hits / max(1, int(ex.counts.sum())), float(cnt.mean())

    out["points"] = {}
    for filt in ("none", "tree_rbac"):
        if graph is not None:
            graph.set_predicate_aware(filt != "none")
        for shortlist in (100, 400):
            for probes in (1, 10, 32):
                for mode in ("off", "relaxed_order"):
                    point = (shortlist, probes, filt, mode)
                    label = f"shortlist{shortlist}_probes{probes}_{filt}_{'off' if mode == 'off' else 'relaxed'}"
                    rec = {"exact_mean_count": float(truth[filt].counts.mean())}
                    calls = {}
                    for name in legs:                        # warm-up (a filter's view-order bitmap is built on first use), window size
                        window(name, point, 2)
                        calls[name] = max(1, int(0.25 / window(name, point, 2)))
                    for name in legs[:-1]:
                        r, c = recall(name, filt)
                        rec[name] = {"recall_at_10": r, "mean_count": c}
                    rec["ivf_quantized"]["mean_lists_scanned"] = float(o["ivf_quantized"]["probes"].cpu().numpy().mean())
                    rec["ivf_stage1"] = {"mean_count": float(wide[shortlist]["cnt"].cpu().numpy().mean())}
                    times = {name: [] for name in legs}
                    for _ in range(args.reps):
                        for name in legs:                    # alternating: every leg sees the same neighbours on the machine
                            times[name].append(window(name, point, calls[name]))
                    for name in legs:
                        t = float(np.median(times[name]))
                        rec[name].update({"seconds_per_call": t, "seconds_per_call_min": float(min(times[name])),
                                          "seconds_per_call_max": float(max(times[name])), "calls_per_window": calls[name],
                                          "queries_per_s": nq / t})
                    for name in legs[1:]:
                        rec[f"ratio_{name}_over_ivf_quantized"] = rec[name]["seconds_per_call"] / rec["ivf_quantized"]["seconds_per_call"]
                    out["points"][label] = rec
                    print(json.dumps({label: rec}), flush=True)
    if graph is not None:
        graph.set_predicate_aware(False)

    path = os.path.join(args.out_dir, "ivf_quantized.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
