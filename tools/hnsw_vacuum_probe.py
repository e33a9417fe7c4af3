"""Cost of vacuuming an HNSW graph (vsr_hnsw_vacuum) against building it again over the live rows.

The two shapes of tools/hnsw_extend_probe.py (120 000 x 128 fp32, 1M x 128 halfvec; m = 16, ef_construction = 64, L2), 10 %, 30 % and
50 % of the rows deleted at random.  For each, alternately and --runs times after one warm-up of each call:

  (a) vsr_hnsw_vacuum of the exported graph of all rows -- the whole call: the host's validation and pass 1, the uploads, the
      edge-distance launch, the repair batches (every attempt, when the call restarts with larger arrays), the compaction;
  (b) vsr_hnsw_build* over a corpus of the live rows alone: existing code, the yardstick.

Medians with min and max, the call's attempts and batches, the repairs it ran in the global-memory form and the bytes of their
workspace pool (HnswIndex.vacuum_spill_info), and recall@10 at ef_search 40 of both graphs against the exact scan over the live
rows.  Whether (a) beats (b) at 50 % is the open question; the record says which way it went.

    python tools/hnsw_vacuum_probe.py [--shapes f32 half] [--shares 10 30 50] [--out profiles/hnsw_vacuum.json]

The legs of a shape that are not measured again (--shares) stay in the file as they are.

Prints one JSON record and writes it to --out (an existing "build_vs_parent" entry, tools/hnsw_build_probe.py's comparison with the
parent commit's library, is kept)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

M, EFC, DIM, K, EF, NQ = 16, 64, 128, 10, 40, 200


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def recall(index, exact_rows, q, to_exact=None):
    got, _ = index.search(q, K, EF, "l2")
    hit = 0
    for i in range(len(q)):
        rows = got.rows[i, :got.counts[i]]
        rows = rows if to_exact is None else to_exact[rows]
        hit += len(set(rows.tolist()) & set(exact_rows[i, :K].tolist()))
    return hit / (len(q) * K)


def measure(ctx, shape, runs, seed, shares, rec, save):
    import vsrbac
    from hnsw_extend_probe import rows_of
    x = rows_of(shape, seed)
    n = len(x)
    load = ctx.load_corpus if shape == "f32" else ctx.load_corpus_half
    build = (lambda c: c.build_hnsw(M, EFC, "l2", seed=1)) if shape == "f32" else (lambda c: c.build_hnsw_half(M, EFC, "l2", seed=1))
    rng = np.random.default_rng(seed + 5)
    q = np.asarray(x[rng.integers(0, n, NQ)], dtype=np.float32) + rng.standard_normal((NQ, DIM)).astype(np.float32) * 0.05
    full = load(x)
    idx = build(full)
    graph = idx.export()
    idx.free()
    print(f"{shape}: graph of {n} rows exported", file=sys.stderr, flush=True)
    rec.update({"rows": n, "dim": DIM, "format": "fp32" if shape == "f32" else "halfvec"})
    for share in (10, 30, 50):
        # (10 and 50 draw what they always drew; 30 has a stream of its own)
        dead = np.sort((rng if share != 30 else np.random.default_rng(seed + 30)).choice(n, n * share // 100, replace=False))
        if share not in shares:
            continue
        live = np.setdiff1d(np.arange(n), dead)
        part = load(x[live])
        exact = part.search(q, K, "l2").rows                   # live-corpus row indices

        def timed(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            return time.perf_counter() - t0, out

        try:
            _, (v, st) = timed(lambda: full.vacuum_hnsw(graph, dead, EFC, "l2"))
        except vsrbac.VsrError as err:                         # a graph too dead for the LDS ladders: the call says so
            dt, b = timed(lambda: build(part))
            dt, b2 = timed(lambda: build(part))
            rec[f"delete_{share}pct"] = {"dead_rows": int(len(dead)), "vacuum_refused": str(err), "status": err.status,
                                         "rebuild_live_rows_s": dt, f"recall_at_{K}_ef{EF}": {"rebuilt": recall(b2, exact, q)}}
            b.free()
            b2.free()
            part.free()
            save()
            continue
        new_of = np.full(n, -1, dtype=np.int64)
        new_of[live] = np.arange(len(live))
        r_vac = recall(v, exact, q, new_of)
        assert v.info()[0] == len(live)
        spilled, ws_bytes = v.vacuum_spill_info()
        v.free()
        _, b = timed(lambda: build(part))
        r_build = recall(b, exact, q)
        b.free()
        t_vac, t_build, attempts, batches = [], [], [], []
        for run in range(runs):
            dt, (v, st) = timed(lambda: full.vacuum_hnsw(graph, dead, EFC, "l2"))
            v.free()
            t_vac.append(dt)
            attempts.append(st["attempts"])
            batches.append(st["batches"])
            dt, b = timed(lambda: build(part))
            b.free()
            t_build.append(dt)
            print(f"{shape} {share} %: run {run + 1} of {runs}", file=sys.stderr, flush=True)
        part.free()
        rec[f"delete_{share}pct"] = {
            "dead_rows": int(len(dead)), "vacuum_s": stats(t_vac), "rebuild_live_rows_s": stats(t_build),
            "vacuum_over_rebuild": statistics.median(t_vac) / statistics.median(t_build),
            "attempts_per_call": max(attempts), "batches": max(batches), "elements_repaired": st["elements_repaired"],
            "spilled_repairs": spilled, "workspace_bytes": ws_bytes,
            f"recall_at_{K}_ef{EF}": {"vacuumed": r_vac, "rebuilt": r_build},
        }
        save()                                                 # after every leg: the long ones come last
    full.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=["f32", "half"], choices=["f32", "half"])
    ap.add_argument("--shares", nargs="+", type=int, default=[10, 30, 50], choices=[10, 30, 50], help="per cent of the rows deleted")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20260117)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_vacuum.json"))
    args = ap.parse_args()
    import vsrbac
    rec = {"probe": "hnsw_vacuum", "m": M, "ef_construction": EFC, "metric": "l2", "runs": args.runs}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        for key in ("build_vs_parent", "f32", "half"):
            if key in old:
                rec[key] = old[key]
    ctx = vsrbac.Context(0)
    rec["device"] = ctx.device_info()["name"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")

    for shape in args.shapes:
        measure(ctx, shape, args.runs, args.seed, args.shares, rec.setdefault(shape, {}), save)
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
