"""HNSW over a halfvec corpus (K4h) beside the fp32 K4 on the identical graph and queries, in one process.

Corpus: `--rows` x `--dim` real-valued rows around `--centres` centres (vsrbac.datasets.gaussian_corpus for the centres and
the noise), rounded to binary16 and loaded as a halfvec corpus; the graph from vsr_hnsw_build_half (m = 16, ef_construction =
64, L2).  The same graph is exported and loaded over an fp32 corpus of the WIDENED rows, so both kernels walk the same lists
over the same values; the queries (corpus rows plus noise) are rounded to binary16 first, so both see the same query too.
Device-resident queries, `--queries` per call, k = 10.

  build      vsr_hnsw_build_half and vsr_hnsw_build over the widened rows: seconds
  k4h, k4    vsr_hnsw_search_device at ef_search 40 / 100 / 400: after a warm-up, `--reps` timed windows per kernel, the two
             kernels alternating; a window is as many back-to-back calls as fill ~0.25 s, closed by a synchronise; seconds per
             call = the median window / its calls (min and max recorded).  queries/s, mean visited elements, recall@10 against
             vsr_search on the half corpus, and whether rows and visited counts of the two kernels agree
  ratio      k4 seconds per call / k4h seconds per call at each ef_search (above 1: K4h is faster)
  bytes      vsr_corpus_device_bytes + vsr_hnsw_device_bytes, both ways

    python tools/hnsw_half_probe.py OUT_DIR [--rows 1000000] [--dim 128] [--queries 1000] [--reps 9]

Writes OUT_DIR/hnsw_halfvec_<dim>.json and prints it; `--merge A.json B.json ...` joins such files into OUT_DIR/hnsw_halfvec.json."""
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
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=20260117)
    ap.add_argument("--merge", nargs="+", default=None, help="join per-shape files into OUT_DIR/hnsw_halfvec.json and stop")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.merge:
        shapes = [json.load(open(p)) for p in args.merge]
        out = {"probe": "hnsw_halfvec", "device": shapes[0]["device"], "shapes": {f'{s["rows"]}x{s["dim"]}': s for s in shapes}}
        with open(os.path.join(args.out_dir, "hnsw_halfvec.json"), "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out, indent=1))
        return

    import torch
    import vsrbac
    from vsrbac.datasets import gaussian_corpus

    n, dim, nq, k = args.rows, args.dim, args.queries, 10
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.default_rng(args.seed)

    centres, _, _ = gaussian_corpus(args.centres, dim, seed=args.seed + 1)
    x, blk, doc = gaussian_corpus(n, dim, seed=args.seed)
    x *= np.float32(0.6)
    x += centres[rng.integers(0, args.centres, n)]
    xh = x.astype(np.float16)
    del x
    q = xh[rng.integers(0, n, nq)].astype(np.float32) + np.float32(0.3) * rng.standard_normal((nq, dim)).astype(np.float32)
    q = q.astype(np.float16).astype(np.float32)              # what `$1::halfvec` holds: K4 gets the query K4h makes of it

    ctx = vsrbac.Context(0)
    out = {"rows": n, "dim": dim, "queries": nq, "k": k, "reps": args.reps, "m": 16, "ef_construction": 64,
           "device": ctx.device_info()["name"]}

    half = ctx.load_corpus_half(xh, blk, doc)
    ctx.synchronize()
    t0 = time.perf_counter()
    hindex = half.build_hnsw_half(16, 64, "l2", seed=1)
    ctx.synchronize()
    out["build"] = {"half_seconds": time.perf_counter() - t0, "elements": hindex.info()[0]}
    graph = hindex.export()
    truth = half.search(q, k, "l2")

    full = ctx.load_corpus(xh.astype(np.float32), blk, doc)
    ctx.synchronize()
    t0 = time.perf_counter()
    built = full.build_hnsw(16, 64, "l2", seed=1)
    ctx.synchronize()
    out["build"]["fp32_seconds"] = time.perf_counter() - t0
    built.free()
    findex = full.load_hnsw(graph)
    out["device_bytes"] = {"half_corpus": half.device_bytes(), "half_index": hindex.device_bytes(),
                           "fp32_corpus": full.device_bytes(), "fp32_index": findex.device_bytes()}
    out["device_bytes"]["half_total"] = out["device_bytes"]["half_corpus"] + out["device_bytes"]["half_index"]
    out["device_bytes"]["fp32_total"] = out["device_bytes"]["fp32_corpus"] + out["device_bytes"]["fp32_index"]

    d_q = torch.from_numpy(q).to(dev)

    def outputs():
        return {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
                "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
                "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "vis": torch.zeros((nq,), dtype=torch.int64, device=dev)}

    legs = {"k4h": (hindex, outputs()), "k4": (findex, outputs())}

    def call(name, ef):
        index, o = legs[name]
        return index.search_device(ptr(d_q), nq, k, ef, "l2", None, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]), ptr(o["dist"]),
                                   ptr(o["cnt"]), ptr(o["vis"]))

    def window(name, ef, calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call(name, ef)
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls

    out["k4h"], out["k4"], out["ratio_k4_over_k4h"] = {}, {}, {}
    for ef in (40, 100, 400):
        calls = {}
        for name in legs:                                    # warm-up, and how many calls fill a window
            window(name, ef, 3)
            calls[name] = max(1, int(0.25 / window(name, ef, 3)))
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name in legs:                                # alternating: both kernels see the same neighbours on the machine
                times[name].append(window(name, ef, calls[name]))
        res = {}
        for name, (index, o) in legs.items():
            rows, cnt, vis = o["row"].cpu().numpy(), o["cnt"].cpu().numpy(), o["vis"].cpu().numpy()
            hits = sum(len(set(rows[i, :max(cnt[i], 0)].tolist()) & set(truth.rows[i, :truth.counts[i]].tolist())) for i in range(nq))
            t = float(np.median(times[name]))
            res[name] = (rows, vis)
            out[name][str(ef)] = {"seconds_per_call": t, "seconds_per_call_min": float(min(times[name])),
                                  "seconds_per_call_max": float(max(times[name])), "calls_per_window": calls[name],
                                  "queries_per_s": nq / t, "recall_at_10": hits / max(1, int(truth.counts.sum())),
                                  "mean_visited": float(vis.mean()), "overflowed": int((cnt < 0).sum())}
        out["k4h"][str(ef)]["same_rows_as_k4"] = float((res["k4h"][0] == res["k4"][0]).mean())
        out["k4h"][str(ef)]["same_visited_counts_as_k4"] = float((res["k4h"][1] == res["k4"][1]).mean())
        out["ratio_k4_over_k4h"][str(ef)] = out["k4"][str(ef)]["seconds_per_call"] / out["k4h"][str(ef)]["seconds_per_call"]

    path = os.path.join(args.out_dir, f"hnsw_halfvec_{dim}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
