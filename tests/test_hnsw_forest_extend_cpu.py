"""The schedule of vsr_hnsw_extend_partitions (hnsw_forest_plan_from, csrc/vsr_hnsw_forest.h, compiled alone with the host C++
compiler) and the call's Python surface.  Nothing here needs a GPU.

hnsw_forest_plan_from is hnsw_forest_plan for graphs that are partly there: per partition the `done` to start from and the entry
point and entry level to start with.  As in tests/test_hnsw_forest_cpu.py the rounds are checked against what the contract says
of every partition ON ITS OWN: its batches are the build's schedule from its start (hnsw_extend_model.schedule), its entry points
follow the build's rule from the entry it started with, and a round holds one batch, or several that sum to at most the cap."""
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
// stdin: mode m cap n_parts, per partition "size start entry entry_level" (entry: a GLOBAL element or -1), then every element's
// level.  mode 0: hnsw_forest_plan (the starts are not read); 1: hnsw_forest_plan_from; 2: the same with nullptr start arrays.
// stdout: "R count rec_cap batches" per round followed by its slots "elem entry entry_level", then "F" and every partition's final
// entry point
int main()
{
    int mode = 0, m = 0, n_parts = 0;
    unsigned cap = 0;
    if (scanf("%d %d %u %d", &mode, &m, &cap, &n_parts) != 4) return 2;
    std::vector<int64_t> base(1, 0), start;
    std::vector<int32_t> entry, entry_level;
    for (int g = 0; g < n_parts; ++g) {
        long long n = 0, s = 0;
        int e = -1, l = -1;
        if (scanf("%lld %lld %d %d", &n, &s, &e, &l) != 4) return 2;
        base.push_back(base.back() + n);
        start.push_back(s);
        entry.push_back(e);
        entry_level.push_back(l);
    }
    std::vector<int32_t> level((size_t) base.back());
    for (auto& l : level)
        if (scanf("%d", &l) != 1) return 2;
    vsr::HnswForestPlan plan;
    bool ok;
    if (mode == 0) ok = vsr::hnsw_forest_plan(n_parts, base.data(), level.data(), m, cap, plan);
    else if (mode == 1) ok = vsr::hnsw_forest_plan_from(n_parts, base.data(), level.data(), m, cap, start.data(), entry.data(), entry_level.data(), plan);
    else ok = vsr::hnsw_forest_plan_from(n_parts, base.data(), level.data(), m, cap, nullptr, nullptr, nullptr, plan);
    if (!ok) return 3;
    for (const auto& r : plan.rounds) {
        printf("R %u %u %u\n", r.count, r.rec_cap, r.batches);
        for (uint64_t s = r.first_slot; s < r.first_slot + r.count; ++s) printf("%d %d %d\n", plan.elems[s], plan.entry[s], plan.entry_level[s]);
    }
    printf("F");
    for (int32_t e : plan.final_entry) printf(" %d", e);
    printf("\n");
    return plan.elems.size() == plan.entry.size() && plan.elems.size() == plan.entry_level.size() ? 0 : 4;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("forest_extend")
    src, exe = d / "forest.cpp", d / "forest"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(mode, parts, levels, m, cap):
        """parts: per partition (size, start, entry, entry_level).  Returns the program's output, parsed."""
        text = (f"{mode} {m} {cap} {len(parts)}\n" + " ".join(" ".join(map(str, p)) for p in parts) + "\n" + " ".join(map(str, levels)) + "\n")
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


SIZES = [[0, 1, 2, 16, 17, 5000], [5000, 17, 0, 16, 2, 1, 0], [40, 3, 1, 0, 2, 16, 17, 200, 2], [0], []]


def _levels(sizes, m, seed=11):
    stream = level_stream(seed, m, max(sizes, default=0))
    return [lv for n in sizes for lv in stream[:n]]


@pytest.mark.parametrize("cap", [1, 5, 4096])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)) or "none")
def test_from_nothing_it_is_the_partition_builds_plan(planner, sizes, cap):
    m = 4
    levels = _levels(sizes, m)
    nothing = [(n, 0, -1, -1) for n in sizes]
    want = planner(0, nothing, levels, m, cap)
    assert planner(1, nothing, levels, m, cap) == want                          # zeros and -1
    assert planner(2, nothing, levels, m, cap) == want                          # no start arrays at all
    assert sum(len(s) for _, _, s in want[0]) == sum(sizes)


# (size, start): nothing there yet, nothing to add, one element, a start off every boundary, most of the graph there already
STARTS = [[(0, 0), (17, 0), (2, 1), (129, 2), (129, 129), (1500, 700), (1503, 1500)],
          [(5000, 4990), (5000, 0), (40, 39), (300, 100), (9, 9), (5000, 2500)],
          [(64, 8), (64, 9), (64, 16), (64, 63)]]


@pytest.mark.parametrize("cap", [1, 5, 64, 4096])
@pytest.mark.parametrize("parts", STARTS, ids=lambda p: "-".join(f"{s}>{n}" for n, s in p))
def test_every_partition_keeps_its_own_schedule_from_its_start(planner, parts, cap):
    m = 4
    sizes = [n for n, _ in parts]
    levels = _levels(sizes, m)
    base = [0]
    for n in sizes:
        base.append(base[-1] + n)
    # a prior graph's entry point: the first element of its highest level, as the build leaves it
    start_entry = []
    for g, (n, s) in enumerate(parts):
        mine = levels[base[g]:base[g] + s]
        e = mine.index(max(mine)) if s else -1
        start_entry.append((base[g] + e, mine[e]) if s else (-1, -1))
    rounds, final = planner(1, [(n, s, e, lv) for (n, s), (e, lv) in zip(parts, start_entry)], levels, m, cap)
    part_of = [g for g, n in enumerate(sizes) for _ in range(n)]
    done = [s for _, s in parts]
    got = [[] for _ in parts]
    entry = [list(e) for e in start_entry]                                      # in force now
    for rec_cap, batches, slots in rounds:
        elems = [s[0] for s in slots]
        assert elems == sorted(set(elems)), "a round's elements do not ascend"
        assert rec_cap == sum(2 * m + levels[e] * m for e in elems)
        in_round = sorted(set(part_of[e] for e in elems))
        assert batches == len(in_round) >= 1
        assert batches == 1 or len(elems) <= cap, "a round of several batches exceeds the cap"
        assert len(elems) <= BATCH_MAX
        unfinished = [g for g, n in enumerate(sizes) if done[g] < n]
        assert in_round[0] == unfinished[0], "the first unfinished partition was not served"
        for g in unfinished:
            if g not in in_round:
                nxt = max(1, min(done[g] // 8, BATCH_MAX, sizes[g] - done[g]))
                before = sum(1 for e in elems if part_of[e] < g)
                assert before > 0 and before + nxt > cap, (g, before, nxt, cap)
        for g in in_round:
            mine = [s for s in slots if part_of[s[0]] == g]
            first = mine[0][0] - base[g]
            assert first == done[g], "a batch that does not begin where the graph ends"
            assert [s[0] - base[g] for s in mine] == list(range(first, first + len(mine)))
            # the entry point in force when the round began, for every slot of the batch
            assert all((s[1], s[2]) == tuple(entry[g]) for s in mine), (g, mine[0], entry[g])
            got[g].append((first, len(mine)))
        for g in in_round:                                                      # the entry points move when the round is over
            mine = [s[0] for s in slots if part_of[s[0]] == g]
            for e in mine:
                if entry[g][0] < 0 or levels[e] > entry[g][1]:
                    entry[g] = [e, levels[e]]
            done[g] += len(mine)
    for g, (n, s) in enumerate(parts):
        assert got[g] == schedule(s, n), f"partition {g}: not the build's schedule from {s}"
        assert final[g] == entry[g][0]
        assert done[g] == n
    assert sum(len(s) for _, _, s in rounds) == sum(n - s for n, s in parts)    # only the elements behind the prior ones have slots
    if cap == 4096 and parts == STARTS[0]:
        # what the packing is for: as many rounds as the longest extension has batches
        assert len(rounds) == max(len(schedule(s, n)) for n, s in parts) < sum(len(schedule(s, n)) for n, s in parts)


def test_symbol_declared_exported_and_bound():
    import vsrbac
    from vsrbac import _ffi
    name, n_args = "vsr_hnsw_extend_partitions", 10
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsrbac.h")).read(), flags=re.S)
    found = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
    assert found, f"{name} is not declared in include/vsrbac.h"
    assert len(found.group(1).split(",")) == n_args
    assert hasattr(ctypes.CDLL(vsrbac.library_path()), name)                   # the built library; never touches the GPU
    assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == n_args


def test_python_surface():
    from vsrbac.engine import Corpus
    from vsrbac.harness import Deployment
    sig = inspect.signature(Corpus.extend_hnsw_partitions)
    assert list(sig.parameters)[1:] == ["indexes", "new_parts", "ef_construction", "metric", "seed"]
    assert (sig.parameters["ef_construction"].default, sig.parameters["metric"].default, sig.parameters["seed"].default) == (64, None, 1)
    sig = inspect.signature(Deployment.extend_partition_hnsw)
    assert list(sig.parameters)[1:4] == ["graphs", "added_docs", "ef_construction"]
    doc = inspect.getdoc(Deployment.extend_partition_hnsw)
    assert "frees" in doc and "use_partition_hnsw" in doc
