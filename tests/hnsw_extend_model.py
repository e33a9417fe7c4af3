"""What tests of vsr_hnsw_extend restate of the batched HNSW build (vsr_hnsw_build_rt.hip: hnsw_build_once; vsr_hnsw_sizing.h): its batch schedule and its
seeded level stream.  tests/test_hnsw_extend_cpu.py pins both to oracle.HnswIndex.batched before a GPU test leans on them."""
import math

BATCH_MAX = 4096                                          # HB_BATCH_MAX (vsr_hnsw_sizing.h)
_M64 = (1 << 64) - 1


def schedule(start, n):
    """The batches (first, count) that take a graph of `start` elements to n: max(1, min(done / 8, BATCH_MAX, n - done))."""
    out, done = [], start
    while done < n:
        b = max(1, min(done // 8, BATCH_MAX, n - done))
        out.append((done, b))
        done += b
    return out


def boundaries(start, n):
    """Every `done` at which a batch of the schedule from `start` to n begins or ends, ascending."""
    return [start] + [first + count for first, count in schedule(start, n)]


def boundary_near(n, target, start=0):
    """The boundary of the schedule start -> n closest to `target`, strictly inside (start, n)."""
    inner = [b for b in boundaries(start, n) if start < b < n]
    return min(inner, key=lambda b: abs(b - target))


def level_stream(seed, m, count):
    """The levels of draws 0 .. count - 1: xorshift64* seeded as the build seeds it, level = floor(-ln(u) / ln(m)), capped like
    HnswGetMaxLevel."""
    rs = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & _M64
    if rs == 0:
        rs = 1

    def draw():
        nonlocal rs
        x = rs
        x ^= x >> 12
        x ^= (x << 25) & _M64
        x ^= x >> 27
        rs = x
        return (x * 0x2545F4914F6CDD1D) & _M64

    draw()
    cap = min((8192 - 24 - 8 - 4 - 4) // 6 // m - 2, 255)
    ml = 1.0 / math.log(m)
    out = []
    for _ in range(count):
        u = (draw() >> 11) * (1.0 / 9007199254740992.0)
        out.append(cap if u == 0.0 else min(int(-math.log(u) * ml), cap))
    return out


def empty_graph(m):
    """The export of a graph without elements: what extending from nothing starts from."""
    import numpy as np
    return {"m": m, "entry": -1, "max_level": 1, "level": np.zeros(0, np.int32), "nbr0": np.zeros((0, 2 * m), np.int32),
            "tid_count": np.zeros(0, np.int32), "tids": np.zeros((0, 10), np.int64), "up_slot": np.zeros(0, np.int32),
            "up_nbr": np.full((1, 1, m), -1, np.int32)}
