"""IVFFlat over a halfvec corpus (K3h) beside the fp32 K3 / K3i over the widened rows, same lists, same queries, one process.

Corpus: `--rows` x `--dim` real-valued rows around `--centres` centres (the generator of tools/hnsw_half_probe.py), rounded to
binary16 and loaded as a halfvec corpus, 100 rows per document, the tree RBAC of the benchmark on top.  The index is built the way
Corpus.build_ivf_half builds it (its sampling rule, vsr_ivf_kmeans_half, vsr_ivf_assign_half, vsr_ivf_load_half; lists = `--lists`,
L2), the two GPU steps timed.  The yardstick is the fp32 index over the WIDENED rows, loaded with the widened centres and the SAME
row_list; the queries (corpus rows plus noise) are rounded to binary16 first, so both see the same values.

  build      seconds of the k-means and of the assignment pass (half form; and of vsr_ivf_assign over the widened rows)
  bytes      vsr_corpus_device_bytes + vsr_ivf_device_bytes, both ways
  points     vsr_ivf_search_device, `--queries` device-resident queries per call, k = 10, L2, probes 1 / 10 / 32, unfiltered and
             under the tree RBAC (role pre-filters); vsr_ivf_search_iterative_device at probes 1 / max_probes 1000 under the tree
             RBAC.  First rows and counts of the two forms are compared for every query (recorded).  Then, after a warm-up,
             `--reps` timed windows per form, the two alternating; a window is as many back-to-back calls as fill ~0.25 s;
             seconds per call = the median window / its calls (min and max recorded)
  ratio      fp32 seconds per call / half seconds per call at each point (above 1: the half form is faster)

    python tools/ivf_half_probe.py OUT_DIR [--rows 1000000] [--dim 128] [--lists 1000] [--queries 1000] [--reps 9]

Writes OUT_DIR/ivf_halfvec_<dim>.json and prints it; `--merge A.json B.json ...` joins such files into OUT_DIR/ivf_halfvec.json."""
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--centres", type=int, default=2000)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=20260117)
    ap.add_argument("--merge", nargs="+", default=None, help="join per-shape files into OUT_DIR/ivf_halfvec.json and stop")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.merge:
        shapes = [json.load(open(p)) for p in args.merge]
        out = {"probe": "ivf_halfvec", "device": shapes[0]["device"], "shapes": {f'{s["rows"]}x{s["dim"]}': s for s in shapes}}
        with open(os.path.join(args.out_dir, "ivf_halfvec.json"), "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out, indent=1))
        return

    import torch
    import vsrbac
    from vsrbac.datasets import gaussian_corpus, sample_queries, tree_rbac

    n, dim, nq, k, lists = args.rows, args.dim, args.queries, 10, args.lists
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(args.seed)

    centres, _, _ = gaussian_corpus(args.centres, dim, seed=args.seed + 1)
    x, blk, doc = gaussian_corpus(n, dim, seed=args.seed, blocks_per_doc=100)
    x *= np.float32(0.6)
    x += centres[rng.integers(0, args.centres, n)]
    xh = x.astype(np.float16)
    del x
    q = xh[rng.integers(0, n, nq)].astype(np.float32) + np.float32(0.3) * rng.standard_normal((nq, dim)).astype(np.float32)
    q = q.astype(np.float16).astype(np.float32)              # what `$1::halfvec` holds: K3 gets the query K3h makes of it
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
    _, quser = sample_queries(nq, n, 1000, seed=args.seed)

    ctx = vsrbac.Context(0)
    out = {"rows": n, "dim": dim, "lists": lists, "queries": nq, "k": k, "reps": args.reps, "metric": "l2",
           "device": ctx.device_info()["name"]}

    half = ctx.load_corpus_half(xh, blk, doc)
    half.load_rbac(rbac.user_roles, rbac.permissions)
    pick = np.sort(np.random.default_rng(1).choice(n, size=min(n, max(lists * 50, 10000)), replace=False))   # build_ivf_half's rule
    samples = np.ascontiguousarray(xh[pick])
    ctx.synchronize()
    t0 = time.perf_counter()
    c16, iterations = ctx.ivf_kmeans_half(samples, lists, "l2", 1)
    t1 = time.perf_counter()
    row_list = half.ivf_assign_half(c16, "l2")
    t2 = time.perf_counter()
    hindex = half.load_ivf_half(c16, row_list)
    out["build"] = {"samples": int(len(pick)), "kmeans_seconds": t1 - t0, "kmeans_iterations": int(iterations),
                    "assign_seconds": t2 - t1, "empty_lists": int(lists - len(np.unique(row_list)))}
    print(json.dumps({"build": out["build"]}), flush=True)

    full = ctx.load_corpus(xh.astype(np.float32), blk, doc)
    full.load_rbac(rbac.user_roles, rbac.permissions)
    c32 = c16.astype(np.float32)
    t0 = time.perf_counter()
    row_list32 = full.ivf_assign(c32, "l2")
    out["build"]["fp32_assign_seconds"] = time.perf_counter() - t0
    out["build"]["fp32_assign_agrees"] = bool((row_list32 == row_list).all())
    findex = full.load_ivf(c32, row_list)
    out["device_bytes"] = {"half_corpus": half.device_bytes(), "half_index": hindex.device_bytes(),
                           "fp32_corpus": full.device_bytes(), "fp32_index": findex.device_bytes()}
    out["device_bytes"]["half_total"] = out["device_bytes"]["half_corpus"] + out["device_bytes"]["half_index"]
    out["device_bytes"]["fp32_total"] = out["device_bytes"]["fp32_corpus"] + out["device_bytes"]["fp32_index"]
    print(json.dumps({"device_bytes": out["device_bytes"]}), flush=True)

    d_q = torch.from_numpy(q).to(dev)

    def outputs():
        return {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
                "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
                "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "probes": torch.zeros((nq,), dtype=torch.int32, device=dev)}

    legs = {}
    for name, corpus, index in (("half", half, hindex), ("fp32", full, findex)):
        legs[name] = (index, outputs(), {"none": None,
                                         "tree_rbac": corpus.pack_filters([corpus.filter_for_user(int(u), vsrbac.RANGES) for u in quser])})

    def call(name, point):
        index, o, filters = legs[name]
        kind, probes, filt, max_probes = point
        if kind == "search":
            index.search_device(ptr(d_q), nq, k, probes, "l2", filters[filt], ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]),
                                ptr(o["cnt"]))
        else:
            index.search_iterative_device(ptr(d_q), nq, k, probes, "l2", filters[filt], "relaxed_order", max_probes, ptr(o["blk"]),
                                          ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]), ptr(o["cnt"]), ptr(o["probes"]))

    def window(name, point, calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call(name, point)
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls

    points = [("search", p, f, 0) for f in ("none", "tree_rbac") for p in (1, 10, 32)] + [("iterative", 1, "tree_rbac", 1000)]
    out["points"] = {}
    for point in points:
        kind, probes, filt, max_probes = point
        label = f"{kind}_probes{probes}_{filt}" + (f"_max{max_probes}" if kind == "iterative" else "")
        got = {}
        for name in legs:                                    # first: do the two forms answer alike, every query
            call(name, point)
            ctx.synchronize()
            o = legs[name][1]
            got[name] = (o["row"].cpu().numpy().copy(), o["cnt"].cpu().numpy().copy(), o["probes"].cpu().numpy().copy())
        cnt = got["half"][1]
        valid = np.arange(k)[None, :] < cnt[:, None]
        same_rows = ((got["half"][0] == got["fp32"][0]) | ~valid).all(axis=1)
        rec = {"counts_agree": bool((got["half"][1] == got["fp32"][1]).all()), "queries_with_the_same_rows": int(same_rows.sum()),
               "mean_count": float(cnt.mean())}
        if kind == "iterative":
            rec["lists_scanned_agree"] = bool((got["half"][2] == got["fp32"][2]).all())
            rec["mean_lists_scanned"] = float(got["half"][2].mean())
        calls = {}
        for name in legs:                                    # warm-up, and how many calls fill a window
            window(name, point, 2)
            calls[name] = max(1, int(0.25 / window(name, point, 2)))
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name in legs:                                # alternating: both forms see the same neighbours on the machine
                times[name].append(window(name, point, calls[name]))
        for name in legs:
            t = float(np.median(times[name]))
            rec[name] = {"seconds_per_call": t, "seconds_per_call_min": float(min(times[name])),
                         "seconds_per_call_max": float(max(times[name])), "calls_per_window": calls[name], "queries_per_s": nq / t}
        rec["ratio_fp32_over_half"] = rec["fp32"]["seconds_per_call"] / rec["half"]["seconds_per_call"]
        out["points"][label] = rec
        print(json.dumps({label: rec}), flush=True)

    path = os.path.join(args.out_dir, f"ivf_halfvec_{dim}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
