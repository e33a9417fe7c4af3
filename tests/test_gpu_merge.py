"""The multi-GPU merge at its limits.

A. merge_lists_kernel (vsr_merge_topk_device / vsr_merge_topk_packed_device) on synthetic per-part lists against a plain
   sort (tests/merge_model.py): both signs of the monotone map, -0, +-Inf, NaN, FLT_MAX, distance ties ordered by the global
   row across parts, empty and full parts, the padding cases, the API's size limit and the launches that need more than
   64 KB of LDS.  No search kernel is involved: a failure here points at the merge alone.  Everything is exact equality.
B. The keys a search emits (d_out_keys of vsr_search_device) and merges of real search output for every metric, against
   the CPU oracle."""
import ctypes

import numpy as np
import pytest

import merge_model as mm
from helpers import assert_valid_topk, sift_like
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import vsrbac
    c = vsrbac.Context(0)
    yield c
    c.close()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _seed(n_parts, k, nq):
    return n_parts * 10007 + k * 13 + nq


def _outputs(torch, dev, nq, k):
    """Output buffers with a tail of k + 3 extra elements, everything pre-filled with a sentinel."""
    tail = k + 3
    return {"block": torch.full((nq * k + tail,), SENT64, dtype=torch.int64, device=dev),
            "doc": torch.full((nq * k + tail,), SENT32, dtype=torch.int32, device=dev),
            "dist": torch.full((nq * k + tail,), SENT32, dtype=torch.int32, device=dev),      # (bit patterns)
            "keys": torch.full((nq * k + tail,), SENT64, dtype=torch.int64, device=dev),
            "counts": torch.full((nq + tail,), SENT32, dtype=torch.int32, device=dev)}


def _run_merge(ctx, case, layout, with_keys):
    """One launch on device copies of the case's inputs.  Returns the outputs as numpy (body and tail apart) after
    checking that the launch left its inputs alone."""
    import torch
    dev = torch.device("cuda", 0)
    n_parts, k, nq = case["n_parts"], case["k"], case["nq"]
    if layout == "packed":
        rec = ctx.packed_result_bytes(nq, k)
        assert rec == nq * k * 24
        host = mm.packed_records(case)
        assert host.size == n_parts * rec
        inputs = [torch.from_numpy(host.copy()).to(dev)]
    else:
        inputs = [torch.from_numpy(case["keys"].view(np.int64)).to(dev), torch.from_numpy(case["block"]).to(dev),
                  torch.from_numpy(case["doc"]).to(dev), torch.from_numpy(case["dist"].view(np.int32)).to(dev)]
    before = [t.clone() for t in inputs]
    o = _outputs(torch, dev, nq, k)
    torch.cuda.synchronize()                                  # the library runs on its own stream
    okeys = _p(o["keys"]) if with_keys else None
    if layout == "packed":
        ctx.merge_topk_packed_device(_p(inputs[0]), n_parts, nq, k, _p(o["block"]), _p(o["doc"]), _p(o["dist"]), okeys,
                                     _p(o["counts"]))
    else:
        ctx.merge_topk_device(_p(inputs[0]), _p(inputs[1]), _p(inputs[2]), _p(inputs[3]), n_parts, nq, k, _p(o["block"]),
                              _p(o["doc"]), _p(o["dist"]), okeys, _p(o["counts"]))
    ctx.synchronize()
    for a, b in zip(inputs, before):
        assert torch.equal(a, b), "the merge wrote to its inputs"
    got, tails = {}, {}
    for name, t in o.items():
        body = nq if name == "counts" else nq * k
        h = t.cpu().numpy()
        got[name], tails[name] = h[:body], h[body:]
    return got, tails


def _check_against_sort(case, got, tails, with_keys):
    nq, k, ref = case["nq"], case["k"], case["ref"]
    np.testing.assert_array_equal(got["counts"], ref["counts"])
    np.testing.assert_array_equal(got["block"].reshape(nq, k), ref["block"])
    np.testing.assert_array_equal(got["doc"].reshape(nq, k), ref["doc"])
    np.testing.assert_array_equal(got["dist"].view(np.uint32).reshape(nq, k), ref["dist"].view(np.uint32))
    if with_keys:
        np.testing.assert_array_equal(got["keys"].view(np.uint64).reshape(nq, k), ref["keys"])
    else:
        assert (got["keys"] == SENT64).all()
    past = np.arange(k)[None, :] >= ref["counts"][:, None]     # slots past the count: -1 / -1 / +Inf (/ KEY_EMPTY)
    assert (got["block"].reshape(nq, k)[past] == -1).all() and (got["doc"].reshape(nq, k)[past] == -1).all()
    assert (got["dist"].view(np.uint32).reshape(nq, k)[past] == 0x7F800000).all()
    for name, t in tails.items():
        assert (t == (SENT64 if t.dtype == np.int64 else SENT32)).all(), f"{name}: written past the end"


def _cases():
    out = []
    for n_parts, k in mm.SHAPES:
        for nq in (1, 7) + ((1000,) if (n_parts, k) == (8, 100) else ()):
            for layout in ("strided", "packed"):
                out.append(pytest.param(n_parts, k, nq, layout, id=f"{n_parts}x{k}-nq{nq}-{layout}"))
    return out


@pytest.mark.parametrize("n_parts,k,nq,layout", _cases())
def test_merge_equals_plain_sort(ctx, n_parts, k, nq, layout):
    """Ids, distances (bit patterns), counts and keys of the merged lists equal the sorted concatenation of the parts' real
    keys; slots past the count hold -1 / -1 / +Inf / KEY_EMPTY; out_keys = NULL changes nothing else; nothing is written
    past the end of an output or into an input."""
    case = mm.make_case(n_parts, k, nq, _seed(n_parts, k, nq))
    got, tails = _run_merge(ctx, case, layout, with_keys=True)
    _check_against_sort(case, got, tails, True)
    bare, tails = _run_merge(ctx, case, layout, with_keys=False)
    _check_against_sort(case, bare, tails, False)
    for name in ("block", "doc", "dist", "counts"):
        assert got[name].tobytes() == bare[name].tobytes(), name


@pytest.mark.parametrize("n_parts,k", mm.SHAPES, ids=[f"{p}x{k}" for p, k in mm.SHAPES])
def test_merge_layouts_give_identical_bytes(ctx, n_parts, k):
    case = mm.make_case(n_parts, k, 7, _seed(n_parts, k, 7))
    a, _ = _run_merge(ctx, case, "strided", with_keys=True)
    b, _ = _run_merge(ctx, case, "packed", with_keys=True)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_small_merge_after_a_large_lds_launch():
    """The > 64 KB launch raises the kernel's dynamic-LDS attribute, and the attribute stays: a small launch on the same
    context afterwards is still right (and so is a second large one)."""
    import vsrbac
    c = vsrbac.Context(0)
    try:
        for n_parts, k in ((8, 513), (3, 5), (4, 2048), (3, 5)):
            for layout in ("strided", "packed"):
                case = mm.make_case(n_parts, k, 7, _seed(n_parts, k, 7) + 1)
                got, tails = _run_merge(c, case, layout, with_keys=True)
                _check_against_sort(case, got, tails, True)
    finally:
        c.close()


def test_merge_argument_checks(ctx):
    """Status codes only: nothing here reaches a launch, and the sentinel-filled outputs stay as they were."""
    import torch
    import vsrbac
    from vsrbac import _ffi
    dev = torch.device("cuda", 0)
    small = mm.make_case(2, 4, 3, 1)
    keys = torch.from_numpy(small["keys"].view(np.int64)).to(dev)
    blk, doc = torch.from_numpy(small["block"]).to(dev), torch.from_numpy(small["doc"]).to(dev)
    dist = torch.from_numpy(small["dist"]).to(dev)
    packed = torch.from_numpy(mm.packed_records(small).copy()).to(dev)
    o = _outputs(torch, dev, 3, 4)
    torch.cuda.synchronize()

    def strided(n_parts, nq, k, keys_p=_p(keys), out_blk=_p(o["block"]), cnt=_p(o["counts"])):
        ctx.merge_topk_device(keys_p, _p(blk), _p(doc), _p(dist), n_parts, nq, k, out_blk, _p(o["doc"]), _p(o["dist"]),
                              _p(o["keys"]), cnt)

    def pack(n_parts, nq, k, in_p=_p(packed), out_blk=_p(o["block"]), cnt=_p(o["counts"])):
        ctx.merge_topk_packed_device(in_p, n_parts, nq, k, out_blk, _p(o["doc"]), _p(o["dist"]), _p(o["keys"]), cnt)

    for call in (strided, pack):
        for n_parts, k in ((8193, 1), (5, 2048)):                       # n_parts * k = 8193 / 10240 > 8192
            with pytest.raises(vsrbac.VsrError) as e:
                call(n_parts, 3, k)
            assert e.value.status == _ffi.ERR_UNSUPPORTED
        for n_parts, nq, k in ((0, 3, 4), (2, 3, 0), (2, -1, 4)):
            with pytest.raises(vsrbac.VsrError) as e:
                call(n_parts, nq, k)
            assert e.value.status == _ffi.ERR_INVALID
        for kw in ({"out_blk": None}, {"cnt": None}, {"keys_p": None} if call is strided else {"in_p": None}):
            with pytest.raises(vsrbac.VsrError) as e:
                call(2, 3, 4, **kw)
            assert e.value.status == _ffi.ERR_INVALID
        call(2, 0, 4)                                                   # nq = 0: VSR_OK, nothing to do
    ctx.synchronize()
    for name, t in o.items():
        h = t.cpu().numpy()
        assert (h == (SENT64 if h.dtype == np.int64 else SENT32)).all(), name


# ---------------------------------------------------------------------------------------------
# B. the keys a search emits, and merges of real search output for every metric
# ---------------------------------------------------------------------------------------------
def _search_into_record(torch, corpus, d_q, nq, k, metric, filters, pack, base):
    """vsr_search_device_exact with its four per-row outputs aimed into one packed record at byte `base` of `pack`."""
    nk = nq * k
    view = lambda lo, hi, dt: pack[base + lo:base + hi].view(dt)
    keys, blk = view(0, nk * 8, torch.int64), view(nk * 8, nk * 16, torch.int64)
    doc, dist = view(nk * 16, nk * 20, torch.int32), view(nk * 20, nk * 24, torch.float32)
    cnt = torch.empty((nq,), dtype=torch.int32, device=pack.device)
    corpus.search_device_exact(_p(d_q), nq, k, metric, filters, _p(blk), _p(doc), None, _p(dist), _p(cnt), _p(keys))
    return cnt


def _merge_records(torch, ctx, pack, parts, nq, k):
    dev = pack.device
    o = {"block": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
         "dist": torch.empty((nq, k), dtype=torch.float32, device=dev), "counts": torch.empty((nq,), dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    ctx.merge_topk_packed_device(_p(pack), parts, nq, k, _p(o["block"]), _p(o["doc"]), _p(o["dist"]), None, _p(o["counts"]))
    ctx.synchronize()
    return {name: t.cpu().numpy() for name, t in o.items()}


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine", "l1"])
def test_emitted_keys_order_and_global_rows(oracle, metric):
    """d_out_keys of vsr_search_device: strictly ascending up to the count, KEY_EMPTY after it; the low 32 bits are
    row_offset + the row's rank in (document_id, block_id) order (identities arrive shuffled, so this is not the caller's
    row index); sorting the returned rows by monotone_keys(the oracle's value, global row) reproduces the returned order.
    Small integer components: every sum is exact in fp32 and float32(sqrt(s)) is strictly monotone in the L2 sum s
    (s < 2^15: neighbouring roots differ by > 2^-9, their ulp is <= 2^-16), so the oracle's operator value orders like
    the kernel's ranking value.  Screening is off on this context: no query can come back flagged."""
    import torch
    import vsrbac
    from vsrbac.sharded import monotone_keys
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    n, dim, k, nq = 3000, 32, 64, 5
    x = rng.integers(-15, 16, (n, dim)).astype(np.float32)
    zero_rows = np.array([5, 1200, 1700, 2400])
    if metric == "cosine":
        x[zero_rows] = 0                                        # NaN distance
    doc = rng.integers(1, 40, n).astype(np.int32)
    blk = rng.permutation(n).astype(np.int64)
    q = rng.integers(-15, 16, (nq, dim)).astype(np.float32)
    half = (rng.random(n) < 0.5).astype(np.uint8)
    few = np.zeros(n, dtype=np.uint8)
    few[rng.choice(n, 40, replace=False)] = 1
    few[zero_rows] = 1
    masks = [None, half, few, half, None]
    c = vsrbac.Context(0)
    try:
        c.set_screening(False)
        d_q = torch.from_numpy(q).to(dev)
        for lo, hi, row_offset in ((0, n, 0), (1000, 2500, 1_000_000)):
            xs, ds, bs = x[lo:hi], doc[lo:hi], blk[lo:hi]
            corpus = c.load_corpus(xs, bs, ds, row_offset=row_offset)
            rank = np.empty(hi - lo, dtype=np.int64)
            rank[np.lexsort((bs, ds))] = np.arange(hi - lo)     # position in (document_id, block_id) order
            filters = [None if m is None else corpus.filter_from_bytemask(m[lo:hi]) for m in masks]
            o = {"blk": torch.empty((nq, k), dtype=torch.int64, device=dev), "doc": torch.empty((nq, k), dtype=torch.int32, device=dev),
                 "row": torch.empty((nq, k), dtype=torch.int64, device=dev), "dist": torch.empty((nq, k), dtype=torch.float32, device=dev),
                 "cnt": torch.empty((nq,), dtype=torch.int32, device=dev), "keys": torch.empty((nq, k), dtype=torch.int64, device=dev)}
            torch.cuda.synchronize()
            keep = corpus.search_device(_p(d_q), nq, k, metric, filters, _p(o["blk"]), _p(o["doc"]), _p(o["row"]), _p(o["dist"]),
                                        _p(o["cnt"]), _p(o["keys"]))
            c.synchronize()
            del keep
            keys, rows, cnt = o["keys"].cpu().numpy().view(np.uint64), o["row"].cpu().numpy(), o["cnt"].cpu().numpy()
            for i in range(nq):
                allowed = hi - lo if masks[i] is None else int(masks[i][lo:hi].sum())
                m = int(cnt[i])
                assert m == min(k, allowed), (i, m, allowed)
                assert (keys[i, 1:m] > keys[i, :m - 1]).all(), "keys are strictly ascending"
                assert (keys[i, m:] == mm.KEY_EMPTY).all()
                grow = row_offset + rank[rows[i, :m]]
                np.testing.assert_array_equal(keys[i, :m] & np.uint64(0xFFFFFFFF), grow.astype(np.uint64))
                val = np.array([oracle.distance(metric, xs[r], q[i]) for r in rows[i, :m]], dtype=np.float64).astype(np.float32)
                want = monotone_keys(val, grow)
                np.testing.assert_array_equal(np.argsort(want, kind="stable"), np.arange(m))
                if metric in ("ip", "l1"):                      # the ranking value IS the operator's value: the whole key
                    np.testing.assert_array_equal(keys[i, :m], want)
            if metric == "cosine":                              # the permitted zero rows came back, as NaN, last
                assert np.isnan(o["dist"].cpu().numpy()[2, :cnt[2]]).sum() == np.isin(zero_rows, np.arange(lo, hi)).sum() > 0
            corpus.free()
    finally:
        c.close()


def _merge_corpus(parts_max=8):
    """Integer rows with components in -31 .. 31 (fp32 sums exact: 31^2 * 768 < 2^24), three vectors planted once in every
    one of `parts_max` equal segments (so every shard of a 2-, 3- or 8-way split holds each: distance ties across shards)
    and one all-zero row per segment for the cosine case."""
    rng = np.random.default_rng(41)
    n, dim = 4800, 64
    x = rng.integers(-31, 32, (n, dim)).astype(np.float32)
    planted = rng.integers(-31, 32, (3, dim)).astype(np.float32)
    seg = n // parts_max
    zero_rows = []
    for s in range(parts_max):
        at = s * seg + rng.choice(seg, 4, replace=False)
        x[at[:3]] = planted
        zero_rows.append(int(at[3]))
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 12 + 1).astype(np.int32)
    return rng, x, planted, np.array(zero_rows), blk, doc


@pytest.mark.parametrize("metric", ["ip", "cosine", "l1"])
@pytest.mark.parametrize("parts", [2, 3, 8])
def test_sharded_merge_all_metrics(ctx, oracle, parts, metric):
    """Row-range shards, per-shard vsr_search_device_exact into packed records laid end to end like an all-gather, merged:
    inner product and L1 equal the oracle bit for bit (the negative half of the monotone map: the rank values straddle
    zero), cosine is a valid top-k of the oracle's float64 distances with its NaN rows last in (document, block) order,
    and all three equal the unsharded search on the same context."""
    import torch
    from vsrbac.sharded import shard_bounds
    dev = torch.device("cuda", 0)
    rng, x, planted, zero_rows, blk, doc = _merge_corpus()
    n, k, nq = len(x), 100, 6
    if metric != "cosine":
        zero_rows = zero_rows[:0]
    else:
        x[zero_rows] = 0
    q = np.concatenate([planted[:2], rng.integers(-31, 32, (nq - 2, x.shape[1])).astype(np.float32)])
    half = (rng.random(n) < 0.5).astype(np.uint8)
    few = np.zeros(n, dtype=np.uint8)
    few[rng.choice(n, 60, replace=False)] = 1
    few[zero_rows] = 1                                          # fewer than k rows permitted: the NaN rows are inside the top-k
    masks = [None, half, few, half, None, few]
    d_q = torch.from_numpy(q).to(dev)
    rec = ctx.packed_result_bytes(nq, k)
    pack = torch.empty((parts * rec,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    shards = []
    for r in range(parts):
        lo, hi = shard_bounds(n, parts, r, align=12)
        c = ctx.load_corpus(x[lo:hi], blk[lo:hi], doc[lo:hi], row_offset=lo)
        filters = [None if m is None else c.filter_from_bytemask(m[lo:hi]) for m in masks]
        _search_into_record(torch, c, d_q, nq, k, metric, filters, pack, r * rec)
        shards.append((c, filters))
    got = _merge_records(torch, ctx, pack, parts, nq, k)
    whole = ctx.load_corpus(x, blk, doc)
    res = whole.search(q, k, metric, [None if m is None else whole.filter_from_bytemask(m) for m in masks])
    np.testing.assert_array_equal(got["counts"], res.counts)
    np.testing.assert_array_equal(got["block"], res.block_ids)
    np.testing.assert_array_equal(got["doc"], res.doc_ids)
    np.testing.assert_array_equal(got["dist"].view(np.uint32), res.dist.view(np.uint32))
    saw_nan = 0
    for i in range(nq):
        m = int(got["counts"][i])
        allowed = np.arange(n) if masks[i] is None else np.flatnonzero(masks[i])
        assert m == min(k, allowed.size)
        assert (got["block"][i, m:] == -1).all() and (got["doc"][i, m:] == -1).all() and np.isposinf(got["dist"][i, m:]).all()
        if metric != "cosine":
            idx, dist = oracle.filtered_topk(metric, x, q[i], k, doc, blk, masks[i])
            assert m == idx.size
            np.testing.assert_array_equal(got["block"][i, :m], blk[idx])
            np.testing.assert_array_equal(got["doc"][i, :m], doc[idx])
            np.testing.assert_array_equal(got["dist"][i, :m], dist.astype(np.float32))
            continue
        rows = got["block"][i, :m] - 1
        np.testing.assert_array_equal(got["doc"][i, :m], doc[rows])
        ref = np.array([oracle.distance("cosine", x[r], q[i]) for r in range(n)], dtype=np.float64)
        assert_valid_topk(rows, got["dist"][i, :m], ref, k, TOL, candidates=allowed)
        isnan = np.isnan(got["dist"][i, :m])
        t = int(isnan.sum())
        assert not isnan[:m - t].any(), "NaN distances come after every finite one"
        if allowed.size <= k:
            assert t == np.isin(zero_rows, allowed).sum()
        assert (np.diff(rows[m - t:]) > 0).all(), "NaN rows among themselves: (document, block) order"
        saw_nan += t
    if metric == "cosine":
        assert saw_nan >= 2 * len(zero_rows), "the NaN rows must be inside the top-k of the few-rows queries"
    else:
        vals = got["dist"][np.isfinite(got["dist"])]
        assert metric != "ip" or ((vals < 0).any() and (vals > 0).any()), "inner products of both signs"
    whole.free()
    for c, _ in shards:
        c.free()


def test_large_k_merge_of_real_search_output(ctx, oracle):
    """k = 1024 over 8 shards: 8192 keys per query, the launch that needs more than 64 KB of LDS, fed by real search
    output.  L2 on SIFT-like rows; the RBAC filter leaves some shards with fewer than k permitted rows (one with none),
    and one user with fewer than k over all shards.  Equals the oracle exactly."""
    import torch
    import vsrbac
    from vsrbac.sharded import shard_bounds
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(52)
    parts, per, k = 8, 3000, 1024
    n = parts * per
    x = sift_like(rng, n)
    blk = (np.arange(n) + 1).astype(np.int64)
    doc = (np.arange(n) // 12 + 1).astype(np.int32)
    dps = per // 12                                             # documents per shard
    first = lambda s: s * dps + 1
    role1 = [d for s in (0, 1, 2) for d in range(first(s), first(s) + dps, 2)]          # 1500 rows per shard: >= k
    role1 += list(range(first(3), first(3) + 20))                                        # 240 rows: < k
    role1 += [d for s in (5, 6, 7) for d in range(first(s) + 7, first(s) + 57)]          # 600 rows: < k; shard 4: none
    role2 = [first(s) + 3 * j for s in (1, 4, 6) for j in range(10)]                     # 360 rows over all shards: < k
    perms = [(1, d) for d in role1] + [(2, d) for d in role2]
    ur = [(1, 1), (2, 2), (3, 1), (3, 2)]
    users = [1, 2, 3, 1]
    nq = len(users)
    q = x[rng.integers(0, n, nq)] + rng.integers(0, 2, (nq, x.shape[1])).astype(np.float32)
    d_q = torch.from_numpy(q).to(dev)
    rec = ctx.packed_result_bytes(nq, k)
    pack = torch.empty((parts * rec,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    shards, short = [], 0
    for r in range(parts):
        lo, hi = shard_bounds(n, parts, r, align=12)
        assert (lo, hi) == (r * per, (r + 1) * per)
        c = ctx.load_corpus(x[lo:hi], blk[lo:hi], doc[lo:hi], row_offset=lo)
        c.load_rbac(ur, perms)
        cnt = _search_into_record(torch, c, d_q, nq, k, "l2", [c.filter_for_user(u, vsrbac.RANGES) for u in users], pack, r * rec)
        short += int(cnt.cpu().numpy()[0] < k)
        shards.append(c)
    assert 3 <= short < parts, "user 1: some shards contribute fewer than k rows, some all k"
    got = _merge_records(torch, ctx, pack, parts, nq, k)
    for i, u in enumerate(users):
        mask = oracle.user_row_mask(u, ur, perms, doc)
        idx, dist = oracle.filtered_topk("l2", x, q[i], k, doc, blk, mask)
        m = int(got["counts"][i])
        assert m == idx.size == min(k, int(mask.sum()))
        np.testing.assert_array_equal(got["block"][i, :m], blk[idx])
        np.testing.assert_array_equal(got["doc"][i, :m], doc[idx])
        np.testing.assert_array_equal(got["dist"][i, :m], dist.astype(np.float32))
        assert (got["block"][i, m:] == -1).all() and np.isposinf(got["dist"][i, m:]).all()
    assert int(got["counts"][1]) == 360 and int(got["counts"][0]) == k
    for c in shards:
        c.free()
