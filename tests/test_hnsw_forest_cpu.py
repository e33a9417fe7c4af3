"""The schedule of vsr_hnsw_build_partitions (csrc/vsr_hnsw_forest.h, compiled alone with the host C++ compiler) and the call's
Python surface.  Nothing here needs a GPU.

The rounds are checked against what the contract says of every partition ON ITS OWN, not against a copy of the packing loop: a
partition's batches are the build's schedule (hnsw_extend_model.schedule, pinned to the serial model by test_hnsw_extend_cpu.py),
its entry points follow the build's rule, and a round is within the cap, ascending, and never starves the first unfinished
partition.  One rule is the header's own and is written down there: a batch larger than the cap (VSR_HNSW_FOREST_BATCH below the
build's batch size) takes a round of its own, because half a batch would see the other half and change the graph.  So "no round
exceeds the cap" reads: a round of more than one batch is within the cap, and a round of one batch is within HB_BATCH_MAX."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from hnsw_extend_model import BATCH_MAX, level_stream, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorsearch-rbac_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "vsr_hnsw_forest.h"
// stdin: m cap n_parts, the sizes, then every element's level.  stdout: "R count rec_cap batches" per round followed by its
// slots "elem entry entry_level", then "F" and every partition's final entry point
int main()
{
    int m = 0, n_parts = 0;
    unsigned cap = 0;
    if (scanf("%d %u %d", &m, &cap, &n_parts) != 3) return 2;
    std::vector<int64_t> base(1, 0);
    for (int g = 0; g < n_parts; ++g) {
        long long n = 0;
        if (scanf("%lld", &n) != 1) return 2;
        base.push_back(base.back() + n);
    }
    std::vector<int32_t> level((size_t) base.back());
    for (auto& l : level)
        if (scanf("%d", &l) != 1) return 2;
    vsr::HnswForestPlan plan;
    if (!vsr::hnsw_forest_plan(n_parts, base.data(), level.data(), m, cap, plan)) return 3;
    for (const auto& r : plan.rounds) {
        printf("R %u %u %u\n", r.count, r.rec_cap, r.batches);
        for (uint64_t s = r.first_slot; s < r.first_slot + r.count; ++s) printf("%d %d %d\n", plan.elems[s], plan.entry[s], plan.entry_level[s]);
    }
    printf("F");
    for (int32_t e : plan.final_entry) printf(" %d", e);
    printf("\n");
    return plan.elems.size() == level.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("forest")
    src, exe = d / "forest.cpp", d / "forest"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(sizes, levels, m, cap):
        text = f"{m} {cap} {len(sizes)}\n" + " ".join(map(str, sizes)) + "\n" + " ".join(map(str, levels)) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        rounds, i = [], 0
        while out[i].startswith("R"):
            _, count, rec_cap, batches = out[i].split()
            slots = [tuple(int(v) for v in ln.split()) for ln in out[i + 1:i + 1 + int(count)]]
            rounds.append((int(rec_cap), int(batches), slots))
            i += 1 + int(count)
        assert out[i].startswith("F")
        return rounds, [int(v) for v in out[i].split()[1:]]
    return run


def _entries(levels, n):
    """The build's entry-point rule over its own schedule: (entry, its level) when each batch begins, and after the last."""
    entry, elev, out = -1, -1, []
    for first, count in schedule(0, n):
        out.append((entry, elev))
        for e in range(first, first + count):
            if entry < 0 or levels[e] > elev:
                entry, elev = e, levels[e]
    return out, entry


SIZES = [[0, 1, 2, 16, 17, 5000], [5000, 17, 0, 16, 2, 1, 0], [17, 17, 17], [40, 3, 1, 0, 2, 16, 17, 200, 2], [0], []]


@pytest.mark.parametrize("cap", [1, 5, 4096])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)) or "none")
def test_rounds_are_every_partitions_own_schedule(planner, sizes, cap):
    m, seed = 4, 11                                                            # m = 4: several levels among 5000 draws
    stream = level_stream(seed, m, max(sizes, default=0))
    assert max(stream, default=0) >= 3 or max(sizes, default=0) < 5000
    base = [0]
    for n in sizes:
        base.append(base[-1] + n)
    levels = [lv for n in sizes for lv in stream[:n]]                          # the stream starts afresh for every partition
    rounds, final = planner(sizes, levels, m, cap)
    part_of = [g for g, n in enumerate(sizes) for _ in range(n)]
    got = [[] for _ in sizes]                                                  # per partition: (first, count, entry, entry level) per batch
    done = [0] * len(sizes)
    waited = 0
    for rec_cap, batches, slots in rounds:
        elems = [s[0] for s in slots]
        assert elems == sorted(set(elems)), "a round's elements do not ascend"
        assert rec_cap == sum(2 * m + levels[e] * m for e in elems)
        in_round = sorted(set(part_of[e] for e in elems))
        assert batches == len(in_round) >= 1
        assert len(elems) <= cap or batches == 1, "a round of several batches exceeds the cap"
        assert len(elems) <= BATCH_MAX
        unfinished = [g for g, n in enumerate(sizes) if done[g] < n]
        assert in_round[0] == unfinished[0], "the first unfinished partition was not served"
        for g in unfinished:
            nxt = max(1, min(done[g] // 8, BATCH_MAX, sizes[g] - done[g]))
            if g not in in_round:
                # it waited: only because its batch did not fit behind what the partitions before it had taken
                before = sum(1 for e in elems if part_of[e] < g)
                assert before > 0 and before + nxt > cap, (g, before, nxt, cap)
                waited += 1
        for g in in_round:
            mine = [s for s in slots if part_of[s[0]] == g]
            first = mine[0][0] - base[g]
            assert [s[0] - base[g] for s in mine] == list(range(first, first + len(mine)))
            assert len(set((s[1], s[2]) for s in mine)) == 1, "one batch, two entry points"
            ent = mine[0][1]
            got[g].append((first, len(mine), ent - base[g] if ent >= 0 else -1, mine[0][2]))
            done[g] += len(mine)
    for g, n in enumerate(sizes):
        want_entries, want_final = _entries(levels[base[g]:base[g + 1]], n)
        assert [(f, c) for f, c, _, _ in got[g]] == schedule(0, n), f"partition {g}: not the build's schedule"
        assert [(e, lv) for _, _, e, lv in got[g]] == want_entries, f"partition {g}: not the build's entry points"
        assert final[g] == (base[g] + want_final if n else -1)
    assert sum(len(s) for _, _, s in rounds) == base[-1]
    if sum(1 for n in sizes if n > 0) > cap:                                   # the first round cannot hold a batch of each
        assert waited > 0, "no partition ever waited: the cap was not exercised"
    if cap == 4096 and sizes == SIZES[0]:
        # what the packing is for: the six builds take 6 + ... batches one after the other, the forest as many rounds as the longest
        assert len(rounds) == len(schedule(0, 5000)) < sum(len(schedule(0, n)) for n in sizes)


def test_symbol_declared_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    name, n_args = "vsr_hnsw_build_partitions", 10
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsrbac.h")).read(), flags=re.S)
    found = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
    assert found, f"{name} is not declared in include/vsrbac.h"
    assert len(found.group(1).split(",")) == n_args
    assert hasattr(ctypes.CDLL(vsrbac.library_path()), name)                   # the built library; never touches the GPU
    assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == n_args


def test_python_surface():
    from vsrbac.engine import Corpus
    from vsrbac.harness import Deployment
    sig = inspect.signature(Corpus.build_hnsw_partitions)
    assert list(sig.parameters)[1:] == ["parts", "m", "ef_construction", "metric", "seed"]
    assert (sig.parameters["m"].default, sig.parameters["ef_construction"].default, sig.parameters["seed"].default) == (16, 64, 1)
    sig = inspect.signature(Deployment.build_partition_hnsw)
    assert list(sig.parameters)[1:] == ["partition_docs", "m", "ef_construction", "metric", "seed"]
