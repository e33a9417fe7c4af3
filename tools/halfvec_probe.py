"""halfvec corpora (vsr_corpus_load_half, K1h) beside the fp32 exact kernels over the same rows, in one process.

The same rows are loaded twice, as fp32 (vsr_corpus_load) and as binary16 (vsr_corpus_load_half).  The fp32 legs run in a
session with screening disabled (vsr_set_screening(ctx, 0)) and the int8 one-query kernel off (VSR_NO_SCAN8=1 at vsr_open), so
both sides run exact kernels over their rows: K1 / K1m over 4 bytes per element against K1h over 2.  Queries and results are
device-resident; a call is timed by the host clock around the call and a synchronise, the sides alternating.  The shared-pass
legs also run the fp32 rows with K1m switched off (VSR_NO_MQ=1, `fp32_exact_k1`): K1 with four queries per sub-batch, the
kernel K1h is an instantiation of -- the like-for-like comparison, where `fp32_exact` (K1m) is the library's best exact path.

  (a) 10M x 128 integer-valued rows, unfiltered, one query per call, k = 100
  (b) the same rows, 1000-query calls under the benchmark's tree RBAC (role pre-filter), k = 100
  (c) 1M x 768 real-valued rows (normal, rounded to binary16), 1000 unfiltered queries per call, k = 100

Per leg and side: median / min / max of the repetitions' time per call, the main scan launch's own device time
(vsr_profiling level 2, a second set of repetitions), the algorithmic bytes of that launch (vsr_stats.scan_bytes: rows*dim*4,
or *2 for the half corpus, + bitmap bytes + k*12) over that device time, the kernel that ran, and device_bytes of both
corpora.  `default` entries are the fp32 corpus as the library runs it when nothing is switched off (screening planes, int8
planes under the u8 query hint): not the yardstick, but what a user of an fp32 corpus of such rows gets today.  Results of
the two sides are compared on the first call of every leg.

    python tools/halfvec_probe.py OUT_DIR [--rows 10000000] [--wide-rows 1000000] [--queries 1000] [--reps 11]

Writes OUT_DIR/halfvec.json and prints it."""
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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--singles", type=int, default=20, help="one-query calls per repetition of leg (a)")
    ap.add_argument("--seed", type=int, default=20251121)
    args = ap.parse_args()

    import torch
    import vsrbac
    from vsrbac.datasets import sample_queries, sift_like_corpus, sift_like_rows_at, tree_rbac

    os.makedirs(args.out_dir, exist_ok=True)
    k, nq, reps = args.k, args.queries, max(args.reps, 11)
    dev = torch.device("cuda", 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    ctx = vsrbac.Context(0)                                   # owns the corpora; the `default` legs run in it
    ctx.set_query_hint(True)
    os.environ["VSR_NO_SCAN8"] = "1"
    exact = vsrbac.Context(0)                                 # fp32 yardstick: exact kernels over the fp32 rows
    del os.environ["VSR_NO_SCAN8"]
    exact.set_screening(False)
    os.environ["VSR_NO_SCAN8"] = os.environ["VSR_NO_MQ"] = "1"
    exact_k1 = vsrbac.Context(0)                              # ... with shared passes on K1 instead of K1m
    del os.environ["VSR_NO_SCAN8"], os.environ["VSR_NO_MQ"]
    exact_k1.set_screening(False)
    half_s = vsrbac.Context(0)                                # the half legs' session (nothing to switch off)

    def outputs(n):
        o = {"blk": torch.empty((n, k), dtype=torch.int64, device=dev), "doc": torch.empty((n, k), dtype=torch.int32, device=dev),
             "row": torch.empty((n, k), dtype=torch.int64, device=dev), "dist": torch.empty((n, k), dtype=torch.float32, device=dev),
             "cnt": torch.empty((n,), dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        return o

    def measure(sides, calls_per_rep):
        """sides: name -> (session, call(i)); the sides alternate inside every repetition."""
        for _, (s, call) in sides.items():                    # warm-up: code objects, workspaces, cached filters
            for i in range(min(calls_per_rep, 3)):
                call(i)
            s.synchronize()
        secs = {name: [] for name in sides}
        for _ in range(reps):
            for name, (s, call) in sides.items():
                t = time.perf_counter()
                for i in range(calls_per_rep):
                    call(i)
                s.synchronize()
                secs[name].append((time.perf_counter() - t) / calls_per_rep)
        out = {}
        for name, (s, call) in sides.items():
            ms = sorted(v * 1e3 for v in secs[name])
            s.profiling(2)
            s.stats_reset()
            for _ in range(reps):
                for i in range(calls_per_rep):
                    call(i)
            st = s.stats()
            s.profiling(False)
            cls = 0 if st["scan_launches"][0] else 1
            launches, kms, nbytes = st["scan_launches"][cls], st["scan_ms"][cls], st["scan_bytes"][cls]
            out[name] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
                         "calls_per_rep": calls_per_rep, "kernel": s.last_scan_kernel(),
                         "scan_kernel_ms_per_call": round(kms / (reps * calls_per_rep), 4), "scan_launches_per_call": launches / (reps * calls_per_rep),
                         "scan_bytes_per_call": int(nbytes // (reps * calls_per_rep)),
                         "scan_TB_per_s": round(nbytes / (kms * 1e-3) / 1e12, 3) if kms > 0 else None}
        return out

    def same(a, b, exact_values):
        """results of two sides on the same call"""
        ca, cb = a["cnt"].cpu().numpy(), b["cnt"].cpu().numpy()
        ra, rb = a["row"].cpu().numpy(), b["row"].cpu().numpy()
        da, db = a["dist"].cpu().numpy(), b["dist"].cpu().numpy()
        if exact_values:
            return {"identical": bool((ca == cb).all() and (ra == rb).all() and (da.view(np.uint32) == db.view(np.uint32)).all())}
        common = np.mean([len(set(ra[i].tolist()) & set(rb[i].tolist())) / k for i in range(len(ca))])
        return {"rows_in_common": round(float(common), 5), "max_abs_distance_difference": float(np.abs(da - db).max())}

    report = {"device": ctx.device_info()["name"], "k": k, "reps": reps,
              "timing": "host clock around the call(s) and a synchronise, device-resident queries and results, sides alternating; "
                        "scan_kernel_ms: HIP events around the main scan launch (vsr_profiling level 2) in a second set of repetitions"}

    # ---- (a), (b): 10M x 128 integer-valued rows ---------------------------------------------------------------------
    n, dim = args.rows, 128
    x, blk, doc = sift_like_corpus(n, dim, seed=args.seed)    # integers 0..255: exact in binary16, fp32 sums exact
    full = ctx.load_corpus(x, blk, doc)
    half = ctx.load_corpus_half(x.astype(np.float16), blk, doc)
    del x
    rbac = tree_rbac(num_users=1000, num_roles=100, num_docs=n // 100, seed=args.seed)
    full.load_rbac(rbac.user_roles, rbac.permissions)
    half.load_rbac(rbac.user_roles, rbac.permissions)
    qrow, quser = sample_queries(nq, n, 1000, seed=args.seed)
    d_q = torch.from_numpy(sift_like_rows_at(qrow, dim, seed=args.seed)).to(dev)
    report["rows_128"] = {"rows": n, "dim": dim, "device_bytes_fp32": full.device_bytes(), "device_bytes_half": half.device_bytes()}
    print(json.dumps({"rows_128": report["rows_128"]}), flush=True)

    o1 = {name: outputs(1) for name in ("fp32_exact", "half", "fp32_default")}
    single = lambda c, s, o: (lambda i: c.search_device(ptr(d_q[i:i + 1]), 1, k, "l2", None, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]),
                                                        ptr(o["dist"]), ptr(o["cnt"]), session=s))
    sides = {"fp32_exact": (exact, single(full, exact, o1["fp32_exact"])), "half": (half_s, single(half, half_s, o1["half"])),
             "fp32_default": (ctx, single(full, ctx, o1["fp32_default"]))}
    for name, (s, call) in sides.items():
        call(0)
        s.synchronize()
    leg = {"what": "unfiltered, one query per call", "same_results": same(o1["fp32_exact"], o1["half"], True)}
    leg.update(measure(sides, args.singles))
    leg["half_over_fp32_exact_median"] = round(leg["half"]["median_ms"] / leg["fp32_exact"]["median_ms"], 3)
    report["a"] = leg
    print(json.dumps({"a": leg}), flush=True)

    ob = {name: outputs(nq) for name in ("fp32_exact", "half", "fp32_default", "fp32_exact_k1")}
    batch = lambda c, s, o, fl: (lambda i: c.search_device(ptr(d_q), nq, k, "l2", fl, ptr(o["blk"]), ptr(o["doc"]), ptr(o["row"]),
                                                           ptr(o["dist"]), ptr(o["cnt"]), session=s))
    fl_full = full.pack_filters([full.filter_for_user(int(u), vsrbac.RANGES) for u in quser])
    fl_half = half.pack_filters([half.filter_for_user(int(u), vsrbac.RANGES) for u in quser])
    sides = {"fp32_exact": (exact, batch(full, exact, ob["fp32_exact"], fl_full)), "half": (half_s, batch(half, half_s, ob["half"], fl_half)),
             "fp32_default": (ctx, batch(full, ctx, ob["fp32_default"], fl_full)),
             "fp32_exact_k1": (exact_k1, batch(full, exact_k1, ob["fp32_exact_k1"], fl_full))}
    for name, (s, call) in sides.items():
        call(0)
        s.synchronize()
    leg = {"what": f"{nq} queries per call, tree RBAC role pre-filter", "same_results": same(ob["fp32_exact"], ob["half"], True)}
    leg.update(measure(sides, 1))
    leg["half_over_fp32_exact_median"] = round(leg["half"]["median_ms"] / leg["fp32_exact"]["median_ms"], 3)
    leg["half_over_fp32_exact_k1_median"] = round(leg["half"]["median_ms"] / leg["fp32_exact_k1"]["median_ms"], 3)
    report["b"] = leg
    print(json.dumps({"b": leg}), flush=True)
    del fl_full, fl_half
    full.free()
    half.free()

    # ---- (c): 1M x 768 real-valued rows ------------------------------------------------------------------------------
    n, dim = args.wide_rows, 768
    rng = np.random.default_rng([args.seed, 23])
    h = rng.standard_normal((n, dim), dtype=np.float32).astype(np.float16)
    full = ctx.load_corpus(h.astype(np.float32))              # the same rows, widened
    half = ctx.load_corpus_half(h)
    q = (h[rng.integers(0, n, nq)].astype(np.float32) + 0.05 * rng.standard_normal((nq, dim), dtype=np.float32))
    d_q = torch.from_numpy(q.astype(np.float16).astype(np.float32)).to(dev)      # already what `$1::halfvec` holds: both sides see it
    del h
    report["rows_768"] = {"rows": n, "dim": dim, "device_bytes_fp32": full.device_bytes(), "device_bytes_half": half.device_bytes()}
    sides = {"fp32_exact": (exact, batch(full, exact, ob["fp32_exact"], None)), "half": (half_s, batch(half, half_s, ob["half"], None)),
             "fp32_default": (ctx, batch(full, ctx, ob["fp32_default"], None)),
             "fp32_exact_k1": (exact_k1, batch(full, exact_k1, ob["fp32_exact_k1"], None))}
    for name, (s, call) in sides.items():
        call(0)
        s.synchronize()
    leg = {"what": f"{nq} unfiltered queries per call, real-valued rows", "same_results": same(ob["fp32_exact"], ob["half"], False)}
    leg.update(measure(sides, 1))
    leg["half_over_fp32_exact_median"] = round(leg["half"]["median_ms"] / leg["fp32_exact"]["median_ms"], 3)
    leg["half_over_fp32_exact_k1_median"] = round(leg["half"]["median_ms"] / leg["fp32_exact_k1"]["median_ms"], 3)
    report["c"] = leg
    print(json.dumps({"c": leg}), flush=True)
    full.free()
    half.free()

    with open(os.path.join(args.out_dir, "halfvec.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    for s in (half_s, exact_k1, exact, ctx):
        s.close()


if __name__ == "__main__":
    main()
