"""vsr_hnsw_vacuum restated in numpy / Python (include/vsrbac.h), on the dicts HnswIndex.export() returns.

pgvector's hnswvacuum.c under the batched schedule the GPU runs: pass 1 drops the dead heap TIDs, the entry phase repairs the
highest live element and the entry point one at a time, the main phase repairs every live element that names a deleted one (or
whose layer-0 list is not full) in batches against the graph as the batch found it, and the deleted elements are squeezed out.

The pieces are pgvector's, literally: HnswSearchLayer with its two heaps and CountElement's rule (only live elements count
towards ef, deleted ones and the repaired element itself are walked and stay in W), RemoveElements before SelectNeighbors,
UpdateNeighborOnDisk's cases before HnswUpdateConnection.  Heap keys are (distance, element id), the tie rule of the build.
Distances are float64 from float32 rows: on integer-valued rows they equal the GPU's fp32 sums exactly.  A bit graph is modelled
on its rows unpacked to 0 / 1 with metric "l2", which is the Hamming distance.

Run as an insertion -- no deleted elements, skip=False, ef not incremented -- the same pieces are the serial build's
(tests/test_hnsw_vacuum_cpu.py pins them to oracle.HnswIndex.batched(batch_limit=1)).
"""
import heapq

import numpy as np

from hnsw_iterative_model import rank_values

BATCH_MAX = 4096                                          # HB_BATCH_MAX (vsr_hnsw_sizing.h)


class Graph:
    """The export() arrays as per-element, per-layer Python lists of neighbour ids (the repair rewrites them)."""

    def __init__(self, g, rows, metric, extra_levels=()):
        self.m = int(g["m"])
        self.metric = metric
        self.entry = int(g["entry"])
        self.level = np.asarray(g["level"]).tolist() + list(extra_levels)
        self.n = len(self.level)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        tc = np.asarray(g["tid_count"]).tolist()
        self.tids = [list(t[:c]) for t, c in zip(np.asarray(g["tids"]).tolist(), tc)]
        self.up_slot = np.asarray(g["up_slot"]).tolist()
        nbr0, up_nbr = np.asarray(g["nbr0"]), np.asarray(g["up_nbr"])
        self.lists = []
        for e in range(len(tc)):
            ls = [[i for i in nbr0[e].tolist() if i >= 0]]
            for lc in range(1, self.level[e] + 1):
                ls.append([i for i in up_nbr[self.up_slot[e], lc - 1].tolist() if i >= 0])
            self.lists.append(ls)
        # an element's vector is its first TID's row, for the whole repair (a deleted element keeps it)
        self.elem_row = [t[0] for t in self.tids]
        for lv in extra_levels:                             # insertion: element len(tc) + i holds row len(tc) + i alone
            e = len(self.lists)
            self.lists.append([[] for _ in range(lv + 1)])
            self.tids.append([e])
            self.elem_row.append(e)
            self.up_slot.append(-1)
        self._vec = self.rows[np.asarray(self.elem_row, dtype=np.int64)]

    def dists_from(self, e):
        return rank_values(self.metric, self._vec, self._vec[e])


def search_layer(g, dist, ep, ef, lc, live, skip):
    """HnswSearchLayer (hnswutils.c:813-976).  ep: [(d, e)]; skip: CountElement's rule is on (a repair) -- only live elements
    count towards ef.  Returns W nearest first: with skip it can be longer than ef."""
    visited = set()
    C, W, wlen = [], [], 0
    for d, e in ep:
        visited.add(e)
        heapq.heappush(C, (d, e))
        heapq.heappush(W, (-d, -e))
        if not skip or live[e]:
            wlen += 1
    while C:
        cd, ce = heapq.heappop(C)
        if cd > -W[0][0]:
            break
        unvisited = []
        for e in g.lists[ce][lc]:
            if e in visited:
                continue
            visited.add(e)
            unvisited.append(e)
        for e in unvisited:
            ed = dist[e]
            if not (ed < -W[0][0] or wlen < ef):
                continue
            heapq.heappush(C, (ed, e))
            heapq.heappush(W, (-ed, -e))
            if not skip or live[e]:
                wlen += 1
                if wlen > ef:
                    heapq.heappop(W)                        # the furthest, deleted or live
    return sorted((-d, -e) for d, e in W)


def select(g, cand, lm):
    """SelectNeighbors (hnswutils.c:1053-1154).  cand: [(d, e)] nearest first.  Returns (selected in pgvector's order, pruned):
    a short list comes back as it came, furthest first, and prunes nobody (None)."""
    if len(cand) <= lm:
        return list(reversed(cand)), None
    sel, wd, i = [], [], 0
    while i < len(cand) and len(sel) < lm:
        d, e = cand[i]
        i += 1
        closer = True
        if sel:
            de = rank_values(g.metric, g._vec[[x[1] for x in sel]], g._vec[e])
            closer = not np.any(de <= d)                    # CheckElementCloser's <=
        (sel if closer else wd).append((d, e))
    wo = 0
    while wo < len(wd) and len(sel) < lm:                   # keep pruned connections
        sel.append(wd[wo])
        wo += 1
    return sel, (wd[wo] if wo < len(wd) else cand[-1])


def find_neighbours(g, me, entry, ef, live, skip):
    """HnswFindElementNeighbors: the new lists of `me`, [[(id, distance)] per layer], searched from `entry` (-1: all empty)."""
    lv = g.level[me]
    new = [[] for _ in range(lv + 1)]
    if entry < 0:
        return new
    dist = g.dists_from(me)
    ep = [(dist[entry], entry)]
    el = g.level[entry]
    for lc in range(el, lv, -1):
        ep = search_layer(g, dist, ep, 1, lc, live, skip)
    for lc in range(min(lv, el), -1, -1):
        w = search_layer(g, dist, ep, ef, lc, live, skip)
        lw = [(d, e) for d, e in w if e != me and live[e]] if skip else w      # RemoveElements
        sel, _ = select(g, lw, 2 * g.m if lc == 0 else g.m)
        new[lc] = [(e, d) for d, e in sel]
        ep = w                                              # W, whole, is the next layer's entry set
    return new


def link(g, src, lc, tgt, d, live):
    """One reverse edge src -> tgt's layer-lc list: UpdateNeighborOnDisk's cases, then HnswUpdateConnection."""
    lst = g.lists[tgt][lc]
    lm = 2 * g.m if lc == 0 else g.m
    if src in lst:
        return
    if len(lst) < lm:
        lst.append(src)
        return
    for j, i in enumerate(lst):
        if not live[i]:
            lst[j] = src
            return
    dt = g.dists_from(tgt)
    cand = sorted([(dt[i], i) for i in lst] + [(d, src)])
    _, pruned = select(g, cand, lm)
    if pruned[1] != src:
        lst[lst.index(pruned[1])] = src


def repair_batch(g, elems, entry, ef, live, skip=True):
    """One batch: every element against the graph as the batch found it, the new lists installed together, then the reverse
    edges in (layer, target, index in the batch) order."""
    news = [find_neighbours(g, e, entry, ef, live, skip) for e in elems]
    for e, nw in zip(elems, news):
        g.lists[e] = [[i for i, _ in ls] for ls in nw]
    recs = [(lc, i, bi, e, d) for bi, (e, nw) in enumerate(zip(elems, news)) for lc, ls in enumerate(nw) for i, d in ls]
    recs.sort(key=lambda r: r[:3])
    for lc, tgt, _, e, d in recs:
        link(g, e, lc, tgt, d, live)


def needs(g, e, live):
    """NeedsUpdated: a list names a deleted element, or the layer-0 list is not full."""
    return any(not live[i] for ls in g.lists[e] for i in ls) or len(g.lists[e][0]) < 2 * g.m


def export(g, keep=None, max_level=None):
    """The graph as export() arrays.  keep: the elements that stay, ascending (None: all), renumbered in that order; upper
    slots in ascending old slot."""
    keep = list(range(g.n)) if keep is None else keep
    new_of = {e: k for k, e in enumerate(keep)}
    m, ne = g.m, len(keep)
    entry = new_of[g.entry] if g.entry >= 0 and ne else -1
    if max_level is None:
        max_level = max(1, g.level[g.entry]) if entry >= 0 else 1
    uppers = sorted((e for e in keep if g.level[e] >= 1), key=lambda e: g.up_slot[e])
    slot_of = {e: s for s, e in enumerate(uppers)}
    level = np.array([g.level[e] for e in keep], dtype=np.int32).reshape(ne)
    nbr0 = np.full((ne, 2 * m), -1, dtype=np.int32)
    tid_count = np.zeros(ne, dtype=np.int32)
    tids = np.full((ne, 10), -1, dtype=np.int64)
    up_slot = np.full(ne, -1, dtype=np.int32)
    up_nbr = np.full((max(len(uppers), 1), max_level, m), -1 if uppers else 0, dtype=np.int32)
    for k, e in enumerate(keep):
        ids = [new_of[i] for i in g.lists[e][0]]
        nbr0[k, :len(ids)] = ids
        tid_count[k] = len(g.tids[e])
        tids[k, :len(g.tids[e])] = g.tids[e]
        if g.level[e] >= 1:
            up_slot[k] = slot_of[e]
            for lc in range(1, g.level[e] + 1):
                ids = [new_of[i] for i in g.lists[e][lc]]
                up_nbr[slot_of[e], lc - 1, :len(ids)] = ids
    return {"level": level, "nbr0": nbr0, "tid_count": tid_count, "tids": tids, "up_slot": up_slot, "up_nbr": up_nbr,
            "max_level": max_level, "entry": entry, "m": m}


def vacuum(graph, rows, metric, dead_rows, ef_construction, batch=BATCH_MAX):
    """(export of the vacuumed graph, stats with "elem_map") -- what Corpus.vacuum_hnsw returns, attempts aside."""
    g = Graph(graph, rows, metric)
    dead = set(int(r) for r in np.asarray(dead_rows).ravel())
    before = sum(len(t) for t in g.tids)
    g.tids = [[t for t in ts if t not in dead] for ts in g.tids]
    live = [len(t) > 0 for t in g.tids]
    kept = sum(len(t) for t in g.tids)
    entry, ef = g.entry, ef_construction + 1
    hp, hl = -1, -1
    for e in range(g.n):                                    # RemoveHeapTids' scan: strict >, the lowest id of the top level
        if live[e] and e != entry and g.level[e] > hl:
            hp, hl = e, g.level[e]
    repaired = batches = 0
    if hp >= 0 and needs(g, hp, live):
        repair_batch(g, [hp], entry, ef, live)
        repaired, batches = repaired + 1, batches + 1
    if entry >= 0:
        if not live[entry]:
            entry = hp
        elif needs(g, entry, live):
            repair_batch(g, [entry], hp, ef, live)
            repaired, batches = repaired + 1, batches + 1
    todo = [e for e in range(g.n) if live[e] and e != entry and needs(g, e, live)]
    for at in range(0, len(todo), batch):
        repair_batch(g, todo[at:at + batch], entry, ef, live)
        repaired, batches = repaired + len(todo[at:at + batch]), batches + 1
    g.entry = entry
    keep = [e for e in range(g.n) if live[e]]
    elem_map = np.full(g.n, -1, dtype=np.int32)
    elem_map[keep] = np.arange(len(keep), dtype=np.int32)
    stats = {"tuples_removed": before - kept, "tuples_kept": kept, "elements_removed": g.n - len(keep),
             "elements_repaired": repaired, "batches": batches, "elem_map": elem_map}
    return export(g, keep), stats


def check_invariants(graph, n_rows_dead=()):
    """What holds after any vacuum: ids in range, lists packed, a neighbour on layer lc lives there, no element lists itself
    twice, the entry on the top level, upper slots distinct, no TID among the dead rows."""
    m, ne = int(graph["m"]), len(graph["level"])
    level, nbr0, up_slot, up_nbr = graph["level"], graph["nbr0"], graph["up_slot"], graph["up_nbr"]
    if ne == 0:
        assert graph["entry"] == -1
        return
    assert 0 <= graph["entry"] < ne and level[graph["entry"]] == level.max()
    assert graph["max_level"] == max(1, int(level.max()))
    slots = up_slot[level >= 1]
    assert (up_slot[level == 0] == -1).all() and sorted(slots.tolist()) == list(range(len(slots)))
    dead = set(int(r) for r in n_rows_dead)
    for e in range(ne):
        tc = int(graph["tid_count"][e])
        assert 1 <= tc <= 10 and not (set(graph["tids"][e, :tc].tolist()) & dead), e
        for lc in range(int(level[e]) + 1):
            ls = nbr0[e] if lc == 0 else up_nbr[up_slot[e], lc - 1]
            k = int((ls >= 0).sum())
            assert (ls[:k] >= 0).all() and (ls[k:] == -1).all(), (e, lc)            # packed
            assert (ls[:k] < ne).all() and len(set(ls[:k].tolist())) == k, (e, lc)
            assert (level[ls[:k]] >= lc).all(), (e, lc)
