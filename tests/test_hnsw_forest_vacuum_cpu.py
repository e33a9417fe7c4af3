"""The schedule of vsr_hnsw_vacuum_partitions (hnsw_forest_vacuum_plan, csrc/vsr_hnsw_forest.h, compiled alone with the host C++
compiler) and the call's surface.  Nothing here needs a GPU.

Every graph must keep exactly the batches vsr_hnsw_vacuum cuts for it alone -- the entry phase's batches of one first, then its
repair list in batches of min(batch_max, left) -- however the rounds pack them: one batch a graph a round, in order, a round within
the cap unless it holds one oversized batch."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "vsr_hnsw_forest.h"
// stdin: batch_max cap n_graphs, then "n_entry n_repair" per graph.  stdout: per round "R", then "graph entry_step first count" per piece
int main()
{
    unsigned batch_max = 0, cap = 0;
    int n = 0;
    if (scanf("%u %u %d", &batch_max, &cap, &n) != 3) return 2;
    std::vector<int32_t> n_entry((size_t) n);
    std::vector<int64_t> n_repair((size_t) n);
    for (int g = 0; g < n; ++g) {
        long long r = 0;
        if (scanf("%d %lld", &n_entry[(size_t) g], &r) != 2) return 2;
        n_repair[(size_t) g] = r;
    }
    vsr::HnswVacuumRounds plan;
    vsr::hnsw_forest_vacuum_plan(n, n_entry.data(), n_repair.data(), batch_max, cap, plan);
    for (size_t r = 0; r + 1 < plan.round_first.size(); ++r) {
        printf("R\n");
        for (size_t k = plan.round_first[r]; k < plan.round_first[r + 1]; ++k)
            printf("%d %d %lld %u\n", plan.pieces[k].graph, plan.pieces[k].entry_step, (long long) plan.pieces[k].first, plan.pieces[k].count);
    }
    return plan.round_first.back() == plan.pieces.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("forest_vacuum")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(graphs, batch_max, cap):
        text = f"{batch_max} {cap} {len(graphs)}\n" + " ".join(f"{e} {r}" for e, r in graphs) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("R\n")[1:]
        return [[tuple(int(v) for v in ln.split()) for ln in rnd.splitlines()] for rnd in out]
    return run


def alone(n_entry, n_repair, batch_max):
    """The batches of one graph's vacuum: (entry_step, first, count), the entry phase first."""
    return [(s, 0, 1) for s in range(n_entry)] + [(-1, at, min(batch_max, n_repair - at)) for at in range(0, n_repair, batch_max)]


REPAIRS = [0, 1, 63, 64, 65, 5000]


@pytest.mark.parametrize("batch_max", [64, 4096])
@pytest.mark.parametrize("cap", [1, 5, 4096])
def test_every_graph_keeps_its_own_batches(planner, cap, batch_max):
    graphs = [(e, r) for e in (0, 1, 2) for r in REPAIRS] + [(0, 0)]            # every entry phase with every list; one graph with nothing
    rounds = planner(graphs, batch_max, cap)
    got = [[] for _ in graphs]
    for pieces in rounds:
        assert pieces, "an empty round"
        served = [p[0] for p in pieces]
        assert served == sorted(set(served)), "a graph twice in one round, or graphs out of order"
        assert len(pieces) == 1 or sum(p[3] for p in pieces) <= cap, "a round of several batches exceeds the cap"
        for g, step, first, count in pieces:
            got[g].append((step, first, count))
    for g, (e, r) in enumerate(graphs):
        assert got[g] == alone(e, r, batch_max), f"graph {g}: not the batches of its vacuum alone"
    if cap == 4096:
        # what the packing is for: as many rounds as the longest vacuum has batches (the 4096-element batches go one a round)
        assert len(rounds) <= max(len(b) for b in got) + 3 < sum(len(b) for b in got) / 2


def test_symbol_declared_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    name, n_args = "vsr_hnsw_vacuum_partitions", 11
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsrbac.h")).read(), flags=re.S)
    found = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
    assert found, f"{name} is not declared in include/vsrbac.h"
    assert len(found.group(1).split(",")) == n_args
    assert hasattr(ctypes.CDLL(vsrbac.library_path()), name)                   # the built library; never touches the GPU
    assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == n_args


def test_python_surface():
    from vsrbac.engine import Corpus
    from vsrbac.harness import Deployment
    sig = inspect.signature(Corpus.vacuum_hnsw_partitions)
    assert list(sig.parameters)[1:] == ["priors", "dead_rows_per_partition", "ef_construction", "metric", "flags"]
    assert (sig.parameters["ef_construction"].default, sig.parameters["metric"].default, sig.parameters["flags"].default) == (64, None, 0)
    assert list(inspect.signature(Deployment.vacuum_partition_hnsw).parameters)[1:4] == ["graphs", "removed_docs", "deleted_docs"]
