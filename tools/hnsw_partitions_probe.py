"""One call for the HNSW graphs of many partitions (vsr_hnsw_build_partitions) against building them one after the other.

1M x 128 SIFT-like fp32 rows, m = 16, ef_construction = 64, L2, split into disjoint random partitions: 100 of 10 000 rows, 10 of
100 000, 1000 of 1000.

  - forest: this library, the corpus resident once, Corpus.build_hnsw_partitions -- the whole call (host pass, rounds, split);
  - sequential: the library given with --parent-lib (the parent commit's; without it this library), one corpus and one
    vsr_hnsw_build per partition, each freed before the next: the builds alone, and the builds with the loads of the
    per-partition corpora included (the host-side gather of a partition's rows is not timed);
  - device bytes of both forms: the resident corpus plus the graphs, against the resident corpus plus a copy of every partition's
    rows plus the graphs (the sum over partitions, as if all were kept, which is what serving them needs).

One resident process per arm, the arms alternating, --runs each after a small warm-up; medians, min and max.

    python tools/hnsw_partitions_probe.py [--parent-lib PATH] [--runs 5] [--out profiles/hnsw_partitions.json]

Prints one JSON record and writes it to --out; progress goes to stderr."""
import argparse
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

M, EFC, DIM = 16, 64, 128
SHAPES = [(100, 10_000), (10, 100_000), (1000, 1000)]       # (partitions, rows each)
NEW_SYMBOLS = ("vsr_hnsw_build_partitions", "vsr_hnsw_extend_partitions")   # what an older library given with --parent-lib may lack


def corpus_rows(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.abs(rng.normal(0, 45, (n, DIM)))), 0, 255).astype(np.float32)


def partitions(n, n_parts, size, seed):
    """n_parts disjoint row lists of `size` rows each, in random order (n_parts * size <= n)."""
    perm = np.random.default_rng([seed, n_parts]).permutation(n)[:n_parts * size]
    return [perm[g * size:(g + 1) * size].astype(np.int64) for g in range(n_parts)]


def worker(args):
    """A resident process: `forest P S` or `seq P S` on stdin, one JSON line each."""
    import ctypes
    from vsrbac import _ffi
    lib = ctypes.CDLL(_ffi.library_path())
    for name in NEW_SYMBOLS:
        if not hasattr(lib, name):
            _ffi.SYMBOLS.pop(name, None)
    import vsrbac
    ctx = vsrbac.Context(0)
    x = corpus_rows(args.rows, args.seed)
    corpus = ctx.load_corpus(x)                               # resident in both arms: the rows the partitions are subsets of
    print(json.dumps({"ready": True, "lib": _ffi.library_path(), "corpus_bytes": corpus.device_bytes()}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        parts = partitions(args.rows, int(word[1]), int(word[2]), args.seed)
        ctx.synchronize()
        if word[0] == "forest":
            t0 = time.perf_counter()
            indexes = corpus.build_hnsw_partitions(parts, M, EFC, "l2", args.seed)
            dt = time.perf_counter() - t0
            rec = {"call_s": dt, "graph_bytes": sum(h.device_bytes() for h in indexes), "elements": sum(h.info()[0] for h in indexes)}
            for h in indexes:
                h.free()
        else:
            load_s = build_s = 0.0
            graph_bytes = copy_bytes = elements = 0
            for p in parts:
                sub = np.ascontiguousarray(x[p])
                t0 = time.perf_counter()
                c = ctx.load_corpus(sub)
                t1 = time.perf_counter()
                h = c.build_hnsw(M, EFC, "l2", seed=args.seed)
                t2 = time.perf_counter()
                load_s += t1 - t0
                build_s += t2 - t1
                graph_bytes += h.device_bytes()
                copy_bytes += c.device_bytes()
                elements += h.info()[0]
                h.free()
                c.free()
            rec = {"build_s": build_s, "load_s": load_s, "graph_bytes": graph_bytes, "copy_bytes": copy_bytes, "elements": elements}
        print(json.dumps(rec), flush=True)
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
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(args.rows), "--seed", str(args.seed)],
                                  env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=self.err, text=True)
        self.ready = self._reply()

    def _reply(self):
        line = self.p.stdout.readline()
        if not line:
            self.err.seek(0)
            raise RuntimeError("worker ended: " + self.err.read()[-2000:])
        return json.loads(line)

    def ask(self, what, n_parts, size):
        self.p.stdin.write(f"{what} {n_parts} {size}\n")
        self.p.stdin.flush()
        return self._reply()

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.close()
        rc = self.p.wait(timeout=120)
        self.err.seek(0)
        text = self.err.read()
        self.err.close()
        if rc != 0:
            raise RuntimeError(f"worker exit {rc}: {text[-2000:]}")


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indexes into the three partitionings (default: all)")
    ap.add_argument("--parent-lib", default=None, help="libvsrbac.so of the parent commit (VSRBAC_LIB of the sequential arm)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_partitions.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    parent = os.path.abspath(args.parent_lib) if args.parent_lib and os.path.exists(args.parent_lib) else None
    rec = {"probe": "hnsw_partitions", "rows": args.rows, "dim": DIM, "m": M, "ef_construction": EFC, "metric": "l2", "runs": args.runs,
           "sequential_library": "parent commit" if parent else "this commit (no --parent-lib)", "partitionings": []}
    new, old = Worker(args, None), Worker(args, parent)
    rec["corpus_bytes"] = new.ready["corpus_bytes"]
    new.ask("forest", 4, 2000)                                # warm-up: code objects, hipCUB's first launches
    old.ask("seq", 4, 2000)
    shapes = SHAPES if args.shapes is None else [SHAPES[i] for i in args.shapes]
    for n_parts, size in shapes:
        if n_parts * size > args.rows:
            continue
        forest, seq = [], []
        for run in range(args.runs):                          # the arms alternate
            seq.append(old.ask("seq", n_parts, size))
            forest.append(new.ask("forest", n_parts, size))
            print(f"{n_parts} x {size} run {run}: forest {forest[-1]['call_s']:.3f} s, sequential builds {seq[-1]['build_s']:.3f} s "
                  f"+ loads {seq[-1]['load_s']:.3f} s", file=sys.stderr, flush=True)
        assert forest[0]["elements"] == seq[0]["elements"] == n_parts * size
        f_s = summary([r["call_s"] for r in forest])
        b_s = summary([r["build_s"] for r in seq])
        bl_s = summary([r["build_s"] + r["load_s"] for r in seq])
        rec["partitionings"].append({
            "partitions": n_parts, "rows_each": size,
            "forest_call_s": f_s, "sequential_builds_s": b_s, "sequential_builds_and_loads_s": bl_s,
            "speedup_over_builds": b_s["median"] / f_s["median"], "speedup_over_builds_and_loads": bl_s["median"] / f_s["median"],
            "device_bytes": {"forest": rec["corpus_bytes"] + forest[0]["graph_bytes"],
                             "sequential": rec["corpus_bytes"] + seq[0]["copy_bytes"] + seq[0]["graph_bytes"],
                             "graphs": forest[0]["graph_bytes"], "row_copies": seq[0]["copy_bytes"]},
        })
        assert forest[0]["graph_bytes"] == seq[0]["graph_bytes"]
    new.close()
    old.close()
    text = json.dumps(rec, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
