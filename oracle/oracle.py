"""ctypes binding of the CPU oracle (oracle/vsr_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg — never by the product package (vectorsearch-rbac_amd/vsrbac).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

L2, IP, COSINE, L1 = 0, 1, 2, 3
JACCARD = 4                      # index paths only: bit_jaccard_ops over rows unpacked to 0 / 1 (HnswIndex.batched)
METRICS = {"l2": L2, "ip": IP, "cosine": COSINE, "l1": L1, "jaccard": JACCARD}

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


def build(force=False):
    """Compile the oracle with gcc (oracle/Makefile). Building the checker is not using it."""
    targets = ["liboracle.so", "liboracle_pgflags.so"]
    have = all(os.path.exists(os.path.join(_HERE, t)) for t in targets)
    if force:
        subprocess.check_call(["make", "-C", _HERE, "-B", "all"], stdout=subprocess.DEVNULL)
    else:
        # make decides (the libraries depend on the sources): a stale library must never check a newer header's functions;
        # where no compiler is at hand the prebuilt libraries are used as they are
        # (one process at a time: the ranks of a multi-GPU bench all come through here at once)
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                rc = subprocess.call(["make", "-C", _HERE, "all"], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL if have else None)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
        if rc != 0 and not have:
            raise RuntimeError("oracle: make failed and no prebuilt library is present")
    if os.path.isdir("/root/reference"):
        # optional reference-derived secondary oracle (vendored hnswlib, compiled in place)
        subprocess.call(["make", "-C", _HERE, "ref"], stdout=subprocess.DEVNULL,
                        stderr=subprocess.DEVNULL)


def _bind(lib):
    d, f, i, i64, vp = C.c_double, C.c_float, C.c_int, C.c_int64, C.c_void_p
    sig = {
        "orc_l2_squared": (f, [i, _f32p, _f32p]),
        "orc_inner_product_f32": (f, [i, _f32p, _f32p]),
        "orc_cosine_similarity": (d, [i, _f32p, _f32p]),
        "orc_l1_f32": (f, [i, _f32p, _f32p]),
        "orc_l2_distance": (d, [i, _f32p, _f32p]),
        "orc_l2_squared_distance": (d, [i, _f32p, _f32p]),
        "orc_inner_product": (d, [i, _f32p, _f32p]),
        "orc_negative_inner_product": (d, [i, _f32p, _f32p]),
        "orc_cosine_distance": (d, [i, _f32p, _f32p]),
        "orc_l1_distance": (d, [i, _f32p, _f32p]),
        "orc_spherical_distance": (d, [i, _f32p, _f32p]),
        "orc_vector_norm": (d, [i, _f32p]),
        "orc_l2_normalize": (i, [i, _f32p, _f32p]),
        "orc_distance": (d, [i, i, _f32p, _f32p]),
        "orc_check_dims": (i, [i, i, C.c_char_p, i]),
        "orc_user_row_mask": (None, [C.c_int32, _i32p, _i32p, i64, _i32p, _i32p, i64, _i32p, i64, _u8p]),
        "orc_filtered_topk": (i64, [i, _f32p, i64, i, vp, vp, vp, _f32p, i64, _i64p, _f64p]),
        "orc_merge_dedup": (i64, [_f64p, _i32p, _i64p, i64, i64, _i64p]),
        "orc_recall": (d, [_i32p, _i64p, i64, _i32p, _i64p, i64]),
        "orc_search_ranges": (None, [i, _f32p, i64, i, vp, vp, _f32p, i64, i64, _i64p, _i64p,
                                     _i64p, _f64p, _i64p]),
        "orc_ivf_kmeans": (i, [i, i, _f32p, i64, i, C.c_uint64, _f32p]),
        "orc_ivf_assign": (None, [i, i, _f32p, i64, _f32p, i, _i32p]),
        "orc_ivf_probe": (i, [i, i, _f32p, i, _f32p, i, _i32p]),
        "orc_hnsw_build": (vp, [i, _f32p, i64, i, i, i, C.c_uint64]),
        "orc_hnsw_build_batched": (vp, [i, _f32p, i64, i, i, i, C.c_uint64, C.c_int32, _i32p, _i32p, _i64p, i]),
        "orc_hnsw_free": (None, [vp]),
        "orc_hnsw_info": (None, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "orc_hnsw_export": (None, [vp, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p, C.c_int32]),
        "orc_hnsw_search": (i64, [vp, _f32p, i, _i64p, _f64p, _i32p, C.POINTER(i64)]),
        "orc_hnsw_search_pa": (i64, [vp, _f32p, i, _u8p, _i64p, _f64p, _i32p, C.POINTER(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


class Oracle:
    """The CPU oracle. variant='strict' is the parity checker; 'pgflags' the timed baseline."""

    def __init__(self, variant="strict"):
        build()
        name = {"strict": "liboracle.so", "pgflags": "liboracle_pgflags.so"}[variant]
        self.lib = _bind(C.CDLL(os.path.join(_HERE, name)))
        self.variant = variant

    # ---- pair distances -------------------------------------------------------------------
    @staticmethod
    def _v(x):
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32))

    def check_dims(self, da, db):
        buf = C.create_string_buffer(128)
        rc = self.lib.orc_check_dims(da, db, buf, 128)
        return rc, buf.value.decode()

    def pair(self, fn, a, b):
        a, b = self._v(a), self._v(b)
        rc, msg = self.check_dims(a.size, b.size)
        if rc:
            raise ValueError(msg)
        return getattr(self.lib, "orc_" + fn)(a.size, a, b)

    def distance(self, metric, a, b):
        a, b = self._v(a), self._v(b)
        rc, msg = self.check_dims(a.size, b.size)
        if rc:
            raise ValueError(msg)
        return self.lib.orc_distance(METRICS[metric], a.size, a, b)

    def vector_norm(self, a):
        a = self._v(a)
        return self.lib.orc_vector_norm(a.size, a)

    def l2_normalize(self, a):
        a = self._v(a)
        out = np.zeros_like(a)
        if self.lib.orc_l2_normalize(a.size, a, out):
            raise OverflowError("value out of range: overflow")
        return out

    # ---- RBAC ----------------------------------------------------------------------------
    def user_row_mask(self, user_id, user_roles, perms, row_doc):
        ur = np.ascontiguousarray(np.asarray(user_roles, dtype=np.int32).reshape(-1, 2))
        pa = np.ascontiguousarray(np.asarray(perms, dtype=np.int32).reshape(-1, 2))
        row_doc = np.ascontiguousarray(row_doc, dtype=np.int32)
        mask = np.zeros(row_doc.size, dtype=np.uint8)
        self.lib.orc_user_row_mask(int(user_id),
                                   np.ascontiguousarray(ur[:, 0]), np.ascontiguousarray(ur[:, 1]), len(ur),
                                   np.ascontiguousarray(pa[:, 0]), np.ascontiguousarray(pa[:, 1]), len(pa),
                                   row_doc, row_doc.size, mask)
        return mask

    # ---- exact filtered top-k ------------------------------------------------------------
    def filtered_topk(self, metric, rows, q, k, row_doc=None, row_block=None, mask=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        q = self._v(q)
        n, dim = rows.shape
        rc, msg = self.check_dims(dim, q.size)
        if rc:
            raise ValueError(msg)
        keep = []

        def ptr(arr, dt):
            if arr is None:
                return None
            a = np.ascontiguousarray(arr, dtype=dt)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)

        out_rows = np.full(max(k, 1), -1, dtype=np.int64)
        out_dist = np.full(max(k, 1), np.inf, dtype=np.float64)
        m = self.lib.orc_filtered_topk(METRICS[metric], rows, n, dim, ptr(row_doc, np.int32),
                                       ptr(row_block, np.int64), ptr(mask, np.uint8), q, k,
                                       out_rows, out_dist)
        return out_rows[:m], out_dist[:m]

    def search_ranges(self, metric, rows, queries, k, range_lists, row_doc=None, row_block=None):
        """range_lists[i] = [(start, count), ...] scanned for query i (one thread)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        n, dim = rows.shape
        nq = queries.shape[0]
        off = np.zeros(nq + 1, dtype=np.int64)
        flat = []
        for i, rl in enumerate(range_lists):
            flat.extend(rl)
            off[i + 1] = len(flat)
        ranges = np.ascontiguousarray(np.asarray(flat, dtype=np.int64).reshape(-1, 2))
        if ranges.size == 0:
            ranges = np.zeros((1, 2), dtype=np.int64)
        rd = None if row_doc is None else np.ascontiguousarray(row_doc, dtype=np.int32)
        rb = None if row_block is None else np.ascontiguousarray(row_block, dtype=np.int64)
        out_rows = np.full((nq, k), -1, dtype=np.int64)
        out_dist = np.full((nq, k), np.inf, dtype=np.float64)
        counts = np.zeros(nq, dtype=np.int64)
        self.lib.orc_search_ranges(METRICS[metric], rows, n, dim,
                                   None if rd is None else rd.ctypes.data_as(C.c_void_p),
                                   None if rb is None else rb.ctypes.data_as(C.c_void_p),
                                   queries, nq, k, off, ranges, out_rows, out_dist, counts)
        return out_rows, out_dist, counts

    # ---- merge / recall ------------------------------------------------------------------
    def merge_dedup(self, dist, doc, block, k):
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        doc = np.ascontiguousarray(doc, dtype=np.int32)
        block = np.ascontiguousarray(block, dtype=np.int64)
        out = np.zeros(max(k, 1), dtype=np.int64)
        m = self.lib.orc_merge_dedup(dist, doc, block, dist.size, k, out)
        return out[:m]

    def recall(self, gt, pred):
        """gt, pred: iterables of (document_id, block_id)."""
        g = np.asarray(list(gt), dtype=np.int64).reshape(-1, 2)
        p = np.asarray(list(pred), dtype=np.int64).reshape(-1, 2)
        return self.lib.orc_recall(np.ascontiguousarray(g[:, 0], dtype=np.int32),
                                   np.ascontiguousarray(g[:, 1]), len(g),
                                   np.ascontiguousarray(p[:, 0], dtype=np.int32),
                                   np.ascontiguousarray(p[:, 1]), len(p))


class IvfIndex:
    """pgvector's IVFFlat restated (vsr_index_oracle.c): k-means on a sample, every row in its nearest list, probes."""

    def __init__(self, oracle, metric, rows, lists=100, seed=1, sample=None):
        self.orc, self.metric = oracle, metric
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = self.rows.shape
        self.lists = int(lists)
        # ivfbuild.c:404-445: max(lists * 50, 10000) sampled rows (all of them when the table is smaller)
        want = max(self.lists * 50, 10000) if sample is None else int(sample)
        rng = np.random.default_rng(seed)
        pick = np.sort(rng.choice(n, size=min(n, want), replace=False)) if n else np.zeros(0, dtype=np.int64)
        samples = np.ascontiguousarray(self.rows[pick])
        self.centers = np.zeros((self.lists, dim), dtype=np.float32)
        rc = oracle.lib.orc_ivf_kmeans(METRICS[metric], dim, samples, len(samples), self.lists, int(seed), self.centers)
        assert rc == 0
        self.assign = np.zeros(n, dtype=np.int32)
        oracle.lib.orc_ivf_assign(METRICS[metric], dim, self.rows, n, self.centers, self.lists, self.assign)

    @classmethod
    def from_centers(cls, oracle, metric, rows, centers):
        """An index over given centres (no k-means): the assignment pass of ivfbuild.c:141-227 only."""
        self = cls.__new__(cls)
        self.orc, self.metric = oracle, metric
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.centers = np.ascontiguousarray(centers, dtype=np.float32)
        n, dim = self.rows.shape
        self.lists = len(self.centers)
        self.assign = np.zeros(n, dtype=np.int32)
        oracle.lib.orc_ivf_assign(METRICS[metric], dim, self.rows, n, self.centers, self.lists, self.assign)
        return self

    def probe(self, q, probes):
        q = np.ascontiguousarray(q, dtype=np.float32)
        out = np.zeros(min(probes, self.lists), dtype=np.int32)
        m = self.orc.lib.orc_ivf_probe(METRICS[self.metric], self.rows.shape[1], self.centers, self.lists, q, int(probes), out)
        return out[:m]

    def search(self, q, k, probes, row_doc=None, row_block=None, mask=None):
        """ivfscan.c:112-176 + the executor's filter: the k nearest permitted rows among the probed lists."""
        lists = self.probe(q, probes)
        m = np.isin(self.assign, lists).astype(np.uint8)
        if mask is not None:
            m &= np.asarray(mask, dtype=np.uint8)
        return self.orc.filtered_topk(self.metric, self.rows, q, k, row_doc, row_block, m)


class HnswIndex:
    """pgvector's HNSW restated (vsr_index_oracle.c): serial in-memory build, GetScanItems search."""

    def __init__(self, oracle, metric, rows, m=16, ef_construction=64, seed=1):
        self.orc, self.metric, self.m = oracle, metric, int(m)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = self.rows.shape
        self._h = oracle.lib.orc_hnsw_build(METRICS[metric], self.rows, n, dim, int(m), int(ef_construction), int(seed))
        self._read_info()

    def _read_info(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.orc.lib.orc_hnsw_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self.n_elem, self.entry, self.entry_level, self.n_upper = a.value, b.value, c.value, d.value

    @classmethod
    def batched(cls, oracle, metric, rows, m=16, ef_construction=64, seed=1, elements=None, batch_limit=0):
        """The GPU's batched build restated serially (vsr_index_oracle.c: orc_hnsw_build_batched).  elements: None -- element e
        is row e -- or a list of row tuples, one per element in element order (an element's vector is its first row's; the
        merging build's canonical grouping).  metric may be "jaccard" (rows unpacked to 0 / 1; "l2" on such rows is Hamming).
        batch_limit > 0 caps every batch (1: the serial build)."""
        self = cls.__new__(cls)
        self.orc, self.metric, self.m = oracle, metric, int(m)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = self.rows.shape
        if elements is None:
            elements = [(r,) for r in range(n)]
        ne = len(elements)
        elem_row = np.array([t[0] for t in elements] + [0], dtype=np.int32)
        tid_count = np.array([len(t) for t in elements] + [0], dtype=np.int32)
        tids = np.full((ne + 1, 10), -1, dtype=np.int64)
        for e, t in enumerate(elements):
            tids[e, :len(t)] = t
        assert tid_count[:ne].min(initial=1) >= 1 and tid_count.max(initial=1) <= 10
        self._h = oracle.lib.orc_hnsw_build_batched(METRICS[metric], self.rows, n, dim, int(m), int(ef_construction), int(seed),
                                                    ne, elem_row, tid_count, tids.reshape(-1), int(batch_limit))
        self._read_info()
        return self

    def __del__(self):
        try:
            if self._h:
                self.orc.lib.orc_hnsw_free(self._h)
                self._h = None
        except Exception:
            pass

    def search(self, q, ef):
        """Rows in the order hnswgettuple would emit their TIDs, index distances (float8), elements, visited count."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        rows = np.zeros(ef * 10 + 10, dtype=np.int64)
        dist = np.zeros(ef * 10 + 10, dtype=np.float64)
        elems = np.zeros(ef + 2, dtype=np.int32)
        nv = C.c_int64()
        n = self.orc.lib.orc_hnsw_search(self._h, q, int(ef), rows, dist, elems, C.byref(nv))
        return rows[:n], dist[:n], elems, nv.value

    def search_predicate_aware(self, q, ef, allowed_rows):
        """The predicate-aware layer-0 walk (vsr_index_oracle.c: search_layer_pa): rows (unfiltered: apply allowed_rows),
        index distances, elements, marked-element count."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        al = np.ascontiguousarray(allowed_rows, dtype=np.uint8)
        rows = np.zeros(ef * 10 + 10, dtype=np.int64)
        dist = np.zeros(ef * 10 + 10, dtype=np.float64)
        elems = np.zeros(ef + 2, dtype=np.int32)
        nv = C.c_int64()
        n = self.orc.lib.orc_hnsw_search_pa(self._h, q, int(ef), al, rows, dist, elems, C.byref(nv))
        return rows[:n], dist[:n], elems, nv.value

    def export(self):
        """Flat arrays for the GPU graph search: level, nbr0 [n_elem][2m], tid_count, tids [n_elem][10], up_slot,
        up_nbr [n_upper][max_level][m], max_level."""
        ne, m = self.n_elem, self.m
        max_level = max(self.entry_level, 1)
        level = np.zeros(ne, dtype=np.int32)
        nbr0 = np.zeros((ne, 2 * m), dtype=np.int32)
        tid_count = np.zeros(ne, dtype=np.int32)
        tids = np.zeros((ne, 10), dtype=np.int64)
        up_slot = np.zeros(ne, dtype=np.int32)
        up_nbr = np.zeros((max(self.n_upper, 1), max_level, m), dtype=np.int32)
        self.orc.lib.orc_hnsw_export(self._h, level, nbr0.reshape(-1), tid_count, tids.reshape(-1), up_slot,
                                     up_nbr.reshape(-1), max_level)
        return {"level": level, "nbr0": nbr0, "tid_count": tid_count, "tids": tids, "up_slot": up_slot, "up_nbr": up_nbr,
                "max_level": max_level, "entry": self.entry, "m": m}
