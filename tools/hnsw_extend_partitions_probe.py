"""One call that extends the HNSW graphs of many partitions (vsr_hnsw_extend_partitions) against extending them one by one.

1M x 128 SIFT-like fp32 rows, m = 16, ef_construction = 64, L2, split into disjoint random partitions -- 100 of 10 000 rows, 1000 of
1000 -- of which every partition holds all but a share of its rows in its graph and takes that share (0.1 %, 1 %, 10 %) as new rows.

  - forest: this library, the corpus resident once, the prior graphs from Corpus.build_hnsw_partitions (not timed),
    Corpus.extend_hnsw_partitions -- the whole call (host pass, join, edge distances, rounds, split);
  - sequential: the only route the parent commit offers, through the library given with --parent-lib (without it this library): per
    partition a corpus of its rows, old and new, and one vsr_hnsw_extend of the prior graph's export with its TIDs mapped into that
    corpus; the extensions alone, and with the loads of the per-partition corpora included (the host-side gather of a partition's
    rows, the export of the priors and the mapping of their TIDs are not timed);
  - device bytes of both routes: the resident corpus plus the new graphs (and, while the call runs, the priors), against the resident
    corpus plus a copy of every partition's rows plus the graphs.

One resident process per arm, the arms alternating, --runs each after a small warm-up; medians, min and max.

    python tools/hnsw_extend_partitions_probe.py [--parent-lib PATH] [--runs 5] [--out profiles/hnsw_extend_partitions.json]

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
SHAPES = [(100, 10_000), (1000, 1000)]                        # (partitions, rows each)
SHARES = [0.001, 0.01, 0.1]                                   # of a partition's rows: new
NEW_SYMBOLS = ("vsr_hnsw_extend_partitions",)                 # what the parent commit's library does not export


def corpus_rows(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.abs(rng.normal(0, 45, (n, DIM)))), 0, 255).astype(np.float32)


def partitions(n, n_parts, size, share, seed):
    """n_parts disjoint row lists of `size` rows each, split into (old, new): new holds max(1, share * size) rows.  Both ascend."""
    perm = np.random.default_rng([seed, n_parts]).permutation(n)[:n_parts * size]
    k = max(1, int(round(share * size)))
    parts = [perm[g * size:(g + 1) * size].astype(np.int64) for g in range(n_parts)]
    return [np.sort(p[:size - k]) for p in parts], [np.sort(p[size - k:]) for p in parts]


def worker(args):
    """A resident process: `forest P S SHARE` or `seq P S SHARE` on stdin, one JSON line each.  The prior graphs of a (P, S, SHARE) are
    made on first use and kept until another one is asked for."""
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
    have, priors, exports = None, [], []
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        key = (int(word[1]), int(word[2]), float(word[3]))
        old, new = partitions(args.rows, key[0], key[1], key[2], args.seed)
        if key != have:
            for h in priors:
                h.free()
            priors = corpus.build_hnsw_partitions(old, M, EFC, "l2", args.seed)
            exports = []
            if word[0] == "seq":                              # the per-graph route takes host arrays; a partition's old rows come first
                for h, o in zip(priors, old):                 # in its corpus, ascending, so element e's TID there is e's rank among them
                    g = h.export()
                    g["tids"] = np.where(g["tids"] >= 0, np.searchsorted(o, np.maximum(g["tids"], 0)), -1)
                    exports.append(g)
                for h in priors:
                    h.free()
                priors = []
            have = key
        ctx.synchronize()
        if word[0] == "forest":
            t0 = time.perf_counter()
            out = corpus.extend_hnsw_partitions(priors, new, EFC, "l2", args.seed)
            dt = time.perf_counter() - t0
            rec = {"call_s": dt, "graph_bytes": sum(h.device_bytes() for h in out), "prior_bytes": sum(h.device_bytes() for h in priors),
                   "elements": sum(h.info()[0] for h in out)}
            for h in out:
                h.free()
        else:
            load_s = extend_s = 0.0
            graph_bytes = copy_bytes = elements = 0
            for g, o, nw in zip(exports, old, new):
                sub = np.ascontiguousarray(x[np.concatenate([o, nw])])
                t0 = time.perf_counter()
                c = ctx.load_corpus(sub)
                t1 = time.perf_counter()
                h = c.extend_hnsw(g, EFC, "l2", args.seed)
                t2 = time.perf_counter()
                load_s += t1 - t0
                extend_s += t2 - t1
                graph_bytes += h.device_bytes()
                copy_bytes += c.device_bytes()
                elements += h.info()[0]
                h.free()
                c.free()
            rec = {"extend_s": extend_s, "load_s": load_s, "graph_bytes": graph_bytes, "copy_bytes": copy_bytes, "elements": elements}
        print(json.dumps(rec), flush=True)
    for h in priors:
        h.free()
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

    def ask(self, what, n_parts, size, share):
        self.p.stdin.write(f"{what} {n_parts} {size} {share}\n")
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
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indexes into the two partitionings (default: all)")
    ap.add_argument("--shares", type=float, nargs="*", default=None, help="shares of new rows (default: 0.001 0.01 0.1)")
    ap.add_argument("--parent-lib", default=None, help="libvsrbac.so of the parent commit (VSRBAC_LIB of the sequential arm)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_extend_partitions.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    parent = os.path.abspath(args.parent_lib) if args.parent_lib and os.path.exists(args.parent_lib) else None
    rec = {"probe": "hnsw_extend_partitions", "rows": args.rows, "dim": DIM, "m": M, "ef_construction": EFC, "metric": "l2", "runs": args.runs,
           "sequential_library": "parent commit" if parent else "this commit (no --parent-lib)", "cases": []}
    new, old = Worker(args, None), Worker(args, parent)
    rec["corpus_bytes"] = new.ready["corpus_bytes"]
    new.ask("forest", 4, 2000, 0.01)                          # warm-up: code objects, hipCUB's first launches
    old.ask("seq", 4, 2000, 0.01)
    shapes = SHAPES if args.shapes is None else [SHAPES[i] for i in args.shapes]
    for n_parts, size in shapes:
        if n_parts * size > args.rows:
            continue
        for share in (SHARES if args.shares is None else args.shares):
            forest, seq = [], []
            for run in range(args.runs):                      # the arms alternate
                seq.append(old.ask("seq", n_parts, size, share))
                forest.append(new.ask("forest", n_parts, size, share))
                print(f"{n_parts} x {size} + {share:g} run {run}: one call {forest[-1]['call_s']:.3f} s, sequential extends "
                      f"{seq[-1]['extend_s']:.3f} s + loads {seq[-1]['load_s']:.3f} s", file=sys.stderr, flush=True)
            assert forest[0]["elements"] == seq[0]["elements"] == n_parts * size
            assert forest[0]["graph_bytes"] == seq[0]["graph_bytes"]
            f_s = summary([r["call_s"] for r in forest])
            e_s = summary([r["extend_s"] for r in seq])
            el_s = summary([r["extend_s"] + r["load_s"] for r in seq])
            rec["cases"].append({
                "partitions": n_parts, "rows_each": size, "new_share": share, "new_rows_each": max(1, int(round(share * size))),
                "one_call_s": f_s, "sequential_extends_s": e_s, "sequential_extends_and_loads_s": el_s,
                "speedup_over_extends": e_s["median"] / f_s["median"], "speedup_over_extends_and_loads": el_s["median"] / f_s["median"],
                "device_bytes": {"one_call": rec["corpus_bytes"] + forest[0]["graph_bytes"],
                                 "one_call_with_priors": rec["corpus_bytes"] + forest[0]["graph_bytes"] + forest[0]["prior_bytes"],
                                 "sequential": rec["corpus_bytes"] + seq[0]["copy_bytes"] + seq[0]["graph_bytes"],
                                 "graphs": forest[0]["graph_bytes"], "row_copies": seq[0]["copy_bytes"]},
            })
    new.close()
    old.close()
    text = json.dumps(rec, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
