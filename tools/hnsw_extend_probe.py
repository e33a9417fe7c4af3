"""Cost of extending an HNSW graph (vsr_hnsw_extend) against building it again.

Two shapes, m = 16, ef_construction = 64, L2: the 120 000 x 128 fp32 SIFT-like rows of tools/hnsw_build_probe.py, and the rows of
tools/hnsw_half_probe.py's 1M x 128 halfvec corpus (with default document ids, so that the prefix of the rows is the prefix of the
insertion order).  For each, alternately and --runs times after one warm-up of each call:

  (a) vsr_hnsw_build* over all rows: existing code, the yardstick;
  (b) vsr_hnsw_extend of the exported graph of a 90 % prefix and of a 99 % prefix over all rows -- the whole call: the host's
      validation of the prior arrays, their upload, the edge-distance launch, the batches.

Medians with min and max, and the edge-distance launch alone from the library's device events (VSR_HNSW_EXTEND_TIMING=1).  The
expectation to confirm or refute: (b) is near the appended share of (a) plus one pass over the prior graph's edges.

    python tools/hnsw_extend_probe.py [--shapes f32 half] [--out profiles/hnsw_extend.json]

Prints one JSON record and writes it to --out (an existing "build_vs_parent" entry, tools/hnsw_build_probe.py's comparison with the
parent commit's library, is kept)."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vectorsearch-rbac_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

M, EFC, DIM = 16, 64, 128


def rows_of(shape, seed):
    if shape == "f32":
        from hnsw_build_probe import corpus_rows
        return corpus_rows(120_000, "clean", 7)
    from vsrbac.datasets import gaussian_corpus
    n, centres_n = 1_000_000, 2000
    rng = np.random.default_rng(seed)
    centres, _, _ = gaussian_corpus(centres_n, DIM, seed=seed + 1)
    x, _, _ = gaussian_corpus(n, DIM, seed=seed)
    x *= np.float32(0.6)
    x += centres[rng.integers(0, centres_n, n)]
    return x.astype(np.float16)


class Stderr:
    """What the library writes to file descriptor 2 while the block runs."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def measure(ctx, shape, runs, seed):
    x = rows_of(shape, seed)
    n = len(x)
    load = ctx.load_corpus if shape == "f32" else ctx.load_corpus_half
    build = (lambda c: c.build_hnsw(M, EFC, "l2", seed=1)) if shape == "f32" else (lambda c: c.build_hnsw_half(M, EFC, "l2", seed=1))

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        idx = fn()
        dt = time.perf_counter() - t0
        ne = idx.info()[0]
        idx.free()
        return dt, ne

    prior = {}
    for share in (90, 99):
        n0 = n * share // 100
        part = load(x[:n0])
        idx = build(part)
        prior[share] = idx.export()
        idx.free()
        part.free()
        print(f"{shape}: prefix graph of {n0} rows exported", file=sys.stderr, flush=True)
    full = load(x)
    os.environ["VSR_HNSW_EXTEND_TIMING"] = "1"
    timed(lambda: build(full))
    for share in (90, 99):
        with Stderr():
            timed(lambda: full.extend_hnsw(prior[share], EFC, "l2", seed=1))
    t_build, t_ext, edge_ms, attempts = [], {90: [], 99: []}, {90: [], 99: []}, {90: [], 99: []}
    for run in range(runs):
        dt, ne = timed(lambda: build(full))
        assert ne == n
        t_build.append(dt)
        for share in (90, 99):
            with Stderr() as err:
                dt, ne = timed(lambda: full.extend_hnsw(prior[share], EFC, "l2", seed=1))
            assert ne == n
            t_ext[share].append(dt)
            found = re.findall(r"vsr_hnsw_extend: prior_elements=(\d+) new_elements=(\d+) batches=(\d+) edge_dist_ms=([\d.]+)", err.text)
            # one line per attempt: a layer search that fills its visited table makes the call start again, as a build does
            assert found and int(found[-1][0]) == n * share // 100, err.text[-500:]
            attempts[share].append(len(found))
            edge_ms[share].append(float(found[-1][3]))
        print(f"{shape}: run {run + 1} of {runs}", file=sys.stderr, flush=True)
    os.environ.pop("VSR_HNSW_EXTEND_TIMING", None)
    full.free()
    rec = {"rows": n, "dim": DIM, "format": "fp32" if shape == "f32" else "halfvec", "build_all_s": stats(t_build)}
    for share in (90, 99):
        appended = 1.0 - share / 100.0
        med = statistics.median(t_ext[share])
        rec[f"extend_from_{share}pct"] = {
            "prior_rows": n * share // 100, "appended_share": appended, "extend_s": stats(t_ext[share]),
            "edge_distance_launch_ms": stats(edge_ms[share]), "attempts_per_call": max(attempts[share]),
            "share_of_build": med / statistics.median(t_build),
            "appended_share_of_build_s": appended * statistics.median(t_build),
        }
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=["f32", "half"], choices=["f32", "half"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20260117)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_extend.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vsrbac
    rec = {"probe": "hnsw_extend", "m": M, "ef_construction": EFC, "metric": "l2", "runs": args.runs}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        for key in ("build_vs_parent", "f32", "half"):
            if key in old:
                rec[key] = old[key]
    ctx = vsrbac.Context(0)
    rec["device"] = ctx.device_info()["name"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for shape in args.shapes:
        rec[shape] = measure(ctx, shape, args.runs, args.seed)
        with open(args.out, "w") as f:                        # after every shape: the long one comes last
            f.write(json.dumps(rec, indent=1) + "\n")
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
