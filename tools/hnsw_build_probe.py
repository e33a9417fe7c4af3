"""Cost of the merging HNSW build's pre-pass, and the unmerged build against another build of the library.

120 000 SIFT-like 128-d rows, m = 16, ef_construction = 64, over a clean copy and over a copy in which 5 % of the rows are
copies of other rows.

  - pre-pass: milliseconds of hash / sort / resolve / element table from the library's device events
    (VSR_HNSW_DEDUP_TIMING=1), and the hash kernel's bytes / time against the 8 TB/s HBM specification;
  - merged build: whole-build wall time (the call synchronises) and n_elem;
  - unmerged build (flags = 0) of this library against the library given with --parent-lib (the parent commit's, built
    separately): one resident process per library, builds alternating, --runs each after a warm-up build; medians, and the
    spread (max - min) / median of the parent's own runs, which is the noise the comparison has to be read against.

    python tools/hnsw_build_probe.py [--parent-lib PATH] [--out profiles/hnsw_build_dedup.json]

Prints one JSON record and writes it to --out."""
import argparse
import json
import os
import re
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
HBM_SPEC_BYTES_PER_S = 8e12
NEW_SYMBOLS = ("vsr_hnsw_build_ex", "vsr_hnsw_export_shape", "vsr_hnsw_export", "vsr_hnsw_extend", "vsr_hnsw_vacuum",
               "vsr_hnsw_vacuum_spill_info", "vsr_hnsw_build_partitions", "vsr_hnsw_extend_partitions")


def corpus_rows(n, kind, seed):
    rng = np.random.default_rng(seed)
    x = np.clip(np.rint(np.abs(rng.normal(0, 45, (n, DIM)))), 0, 255).astype(np.float32)
    if kind == "dup5":                                    # 5 % of the rows become copies of rows outside that 5 %
        pick = rng.permutation(n)
        dup, rest = pick[:n // 20], pick[n // 20:]
        x[dup] = x[rng.choice(rest, size=len(dup))]
    return x


def worker(args):
    """A resident process: loads the corpus once, then answers `build <merge>` lines on stdin with one JSON line each."""
    import ctypes
    from vsrbac import _ffi
    lib = ctypes.CDLL(_ffi.library_path())
    for name in NEW_SYMBOLS:                              # an older library: bind what it has, the unmerged build is all it is asked
        if not hasattr(lib, name):
            _ffi.SYMBOLS.pop(name, None)
    import vsrbac
    ctx = vsrbac.Context(0)
    corpus = ctx.load_corpus(corpus_rows(args.rows, args.corpus, args.seed))
    print(json.dumps({"ready": True, "lib": _ffi.library_path()}), flush=True)
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        merge = word[1] == "1"
        ctx.synchronize()
        t0 = time.perf_counter()
        idx = corpus.build_hnsw(M, EFC, "l2", seed=args.seed, merge_duplicates=merge)
        dt = time.perf_counter() - t0
        n_elem = idx.info()[0]
        idx.free()
        print(json.dumps({"build_s": dt, "n_elem": n_elem, "merge": merge}), flush=True)
    corpus.free()
    ctx.close()


class Worker:
    def __init__(self, args, lib, corpus, timing=False):
        env = dict(os.environ)
        if lib:
            env["VSRBAC_LIB"] = lib
        else:
            env.pop("VSRBAC_LIB", None)
        self.err = tempfile.TemporaryFile(mode="w+")
        if timing:
            env["VSR_HNSW_DEDUP_TIMING"] = "1"
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--corpus", corpus, "--rows", str(args.rows),
                                   "--seed", str(args.seed)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=self.err,
                                  text=True)
        self.ready = self._reply()

    def _reply(self):
        line = self.p.stdout.readline()
        if not line:
            self.err.seek(0)
            raise RuntimeError("worker ended: " + self.err.read()[-2000:])
        return json.loads(line)

    def build(self, merge):
        self.p.stdin.write(f"build {int(merge)}\n")
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
        return text


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=120_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="libvsrbac.so of the parent commit (VSRBAC_LIB of its worker)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_build_dedup.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--corpus", default="clean", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    n = args.rows
    rec = {"probe": "hnsw_build_dedup", "rows": n, "dim": DIM, "m": M, "ef_construction": EFC, "runs": args.runs,
           "hbm_spec_bytes_per_s": HBM_SPEC_BYTES_PER_S}

    # ---- merged builds and the pre-pass, on both corpora ----
    row_bytes = n * ((DIM + 3) // 4) * 16
    for kind in ("clean", "dup5"):
        w = Worker(args, None, kind, timing=True)
        w.build(True)                                     # warm-up: code objects, hipCUB's first launches
        merged = [w.build(True) for _ in range(args.runs)]
        plain = [w.build(False) for _ in range(args.runs)]
        lines = re.findall(r"vsr_hnsw_dedup: rows=(\d+) elements=(\d+) rounds=(\d+) hash_ms=([\d.]+) sort_ms=([\d.]+) "
                           r"resolve_ms=([\d.]+) table_ms=([\d.]+)", w.close())[1:]
        assert len(lines) == args.runs, lines
        med = lambda i: statistics.median(float(t[i]) for t in lines)       # noqa: E731
        hash_ms = med(3)
        rec[kind] = {
            "n_elem_merged": merged[0]["n_elem"], "n_elem_unmerged": plain[0]["n_elem"], "dedup_rounds": int(lines[0][2]),
            "prepass_ms": {"hash": hash_ms, "sort": med(4), "resolve": med(5), "element_table": med(6)},
            "hash_kernel_bytes": row_bytes, "hash_kernel_bytes_per_s": row_bytes / (hash_ms * 1e-3),
            "hash_kernel_share_of_hbm_spec": row_bytes / (hash_ms * 1e-3) / HBM_SPEC_BYTES_PER_S,
            "merged_build_s_median": statistics.median(b["build_s"] for b in merged),
            "merged_build_s": [b["build_s"] for b in merged],
            "unmerged_build_s_median": statistics.median(b["build_s"] for b in plain),
        }

    # ---- the unmerged build: this library and the parent's, alternating ----
    if args.parent_lib and os.path.exists(args.parent_lib):
        new, old = Worker(args, None, "clean"), Worker(args, os.path.abspath(args.parent_lib), "clean")
        new.build(False)
        old.build(False)
        t_new, t_old = [], []
        for _ in range(args.runs):
            t_old.append(old.build(False)["build_s"])
            t_new.append(new.build(False)["build_s"])
        new.close()
        old.close()
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        rec["unmerged_vs_parent"] = {
            "this_build_s": t_new, "parent_build_s": t_old, "this_median_s": m_new, "parent_median_s": m_old,
            "parent_spread": spread(t_old), "this_spread": spread(t_new), "slowdown": m_new / m_old - 1.0,
            "within_parent_spread": bool(m_new / m_old - 1.0 <= spread(t_old)),
        }
    else:
        rec["unmerged_vs_parent"] = None                  # not measured: no parent library given

    text = json.dumps(rec, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
