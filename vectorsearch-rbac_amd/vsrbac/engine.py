"""Object wrappers over the C ABI: Context (one GPU), Corpus (resident rows + identity + RBAC), Filter."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _ffi
from ._ffi import VsrError, check, load_library

L2, IP, COSINE, L1 = 0, 1, 2, 3
HAMMING, JACCARD = 4, 5                              # bit corpora only (Corpus.search_bit)
METRICS = {"l2": L2, "<->": L2, "ip": IP, "<#>": IP, "cosine": COSINE, "<=>": COSINE, "l1": L1, "<+>": L1,
           "hamming": HAMMING, "<~>": HAMMING, "jaccard": JACCARD, "<%>": JACCARD}
RANGES, BITMAP = 0, 1
MAX_K = 2048                                         # VSR_MAX_K: the largest k, and the longest shortlist of search_quantized
BUILD_MERGE_DUPLICATES = 1                           # VSR_HNSW_BUILD_MERGE_DUPLICATES

SearchResult = namedtuple("SearchResult", "block_ids doc_ids rows dist counts")


def _metric(m):
    return METRICS[m] if isinstance(m, str) else int(m)


# hnsw.iterative_scan's values (hnsw.c:21-31) -> vsr_hnsw_iterative
ITERATIVE_MODES = {"off": 0, "relaxed_order": 1, "strict_order": 2}


def _iterative_mode(m):
    if isinstance(m, str):
        if m not in ITERATIVE_MODES:
            raise ValueError(f"invalid value for parameter \"hnsw.iterative_scan\": \"{m}\"")
        return ITERATIVE_MODES[m]
    return int(m)


# ivfflat.iterative_scan's values (ivfflat.c:20-30) -> vsr_ivf_iterative; IVFFlat has no strict order
IVF_ITERATIVE_MODES = {"off": 0, "relaxed_order": 1}


def _ivf_iterative_mode(m):
    if isinstance(m, str):
        if m not in IVF_ITERATIVE_MODES:
            raise ValueError(f"invalid value for parameter \"ivfflat.iterative_scan\": \"{m}\"")
        return IVF_ITERATIVE_MODES[m]
    return int(m)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as_f16(a, what):
    """`a` as np.float16.  The halfvec index entry points take halfvec values: an array of another type is refused rather than
    rounded silently (round it with astype(np.float16), as load_corpus_half documents)."""
    a = np.asarray(a)
    if a.dtype != np.float16:
        raise ValueError(f"{what} must be a np.float16 array (halfvec values), got {a.dtype}")
    return a


def _packed_bits(a, dim, what):
    """`a` as packed uint8 [n, (dim + 7) // 8] in varbit order: a bool [n, dim] array is packed with np.packbits (element i
    -> bit 7 - i % 8 of byte i // 8); a uint8 array is taken as packed already, then `dim` must be given."""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = np.atleast_2d(a)
        if dim is not None and int(dim) != a.shape[1]:
            raise ValueError(f"{what}: a bool array of {a.shape[1]} columns cannot have dim {dim}")
        dim = a.shape[1]
        packed = np.packbits(a, axis=1) if dim else np.zeros((a.shape[0], 0), dtype=np.uint8)
        return np.ascontiguousarray(packed), int(dim)
    if a.dtype != np.uint8:
        raise ValueError(f"{what}: bit strings are bool [n, dim] or packed uint8 [n, (dim + 7) // 8] arrays")
    if dim is None:
        raise ValueError(f"{what}: packed uint8 rows need dim (the bit length)")
    a = np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 else a)
    if a.ndim != 2 or a.shape[1] != (int(dim) + 7) // 8:
        raise ValueError(f"{what}: packed rows of {int(dim)} bits are [n, {(int(dim) + 7) // 8}] bytes")
    return a, int(dim)


def _csr(indptr, indices=None, values=None, dim=None, what="sparse rows"):
    """Sparse rows as (indptr int64 [n + 1], indices int32 [nnz] zero-based, values float32 [nnz], dim): three arrays plus `dim`,
    or any object with .indptr / .indices / .data / .shape (a scipy.sparse CSR matrix; scipy itself is not needed)."""
    if indices is None and values is None and hasattr(indptr, "indptr"):
        m = indptr
        indptr, indices, values = m.indptr, m.indices, m.data
        if dim is None:
            dim = m.shape[1]
    if indices is None or values is None or dim is None:
        raise ValueError(f"{what}: give indptr, indices, values and dim, or an object with .indptr / .indices / .data / .shape")
    ip = np.ascontiguousarray(indptr, dtype=np.int64).reshape(-1)
    ix = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    vx = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if ip.size < 1 or ix.size != vx.size or (ip.size > 1 and (int(ip.max()) > ix.size or int(ip.min()) < 0)):
        raise ValueError(f"{what}: indptr has n + 1 entries addressing indices / values of equal length")
    return ip, ix, vx, int(dim)


class Context:
    """One MI355X.  Fails loudly (VsrError) when there is no gfx950 device."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        check(self._lib.vsr_open(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vsr_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_int64()
        check(self._lib.vsr_device_info(self._h, name, 256, C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    def set_stream(self, stream_handle):
        """A hipStream_t handle (torch: `stream.cuda_stream`).  None: the context's own stream.  0 is what torch reports
        for the device's null stream: it is passed as VSR_STREAM_NULL, so that work the caller orders on that stream
        (events, copies, collectives) really is ordered against the searches."""
        if stream_handle is None:
            handle = 0
        else:
            handle = int(stream_handle) or 1
        check(self._lib.vsr_set_stream(self._h, C.c_void_p(handle)))

    def set_query_hint(self, u8_queries=True):
        """Promise that the device-resident queries of this context are integers 0..255 (SIFT): L2 searches over a
        corpus of such integers then screen on its int8 planes.  Verified on the device; a violation flags the query."""
        check(self._lib.vsr_set_query_hint(self._h, 1 if u8_queries else 0))

    def synchronize(self):
        check(self._lib.vsr_synchronize(self._h))

    def profiling(self, enable=True):
        """True / 1: HIP events around every launch class; 2: around the main scan launch only; False: off."""
        check(self._lib.vsr_profiling(self._h, int(enable)))

    def stats(self):
        st = _ffi.Stats()
        check(self._lib.vsr_stats_get(self._h, C.byref(st)))
        out = {}
        for f, _ in st._fields_:
            v = getattr(st, f)
            out[f] = list(v) if hasattr(v, "__len__") else v
        return out

    def stats_reset(self):
        check(self._lib.vsr_stats_reset(self._h))

    def last_scan_kernel(self):
        """Kernel instantiation the main scan launch of this session's last search resolved to."""
        buf = C.create_string_buffer(512)                # (a class-view int8 plan names three kernels and their variants: > 200 characters)
        check(self._lib.vsr_last_scan_kernel(self._h, buf, 512))
        return buf.value.decode()

    def set_screening(self, enable=True):
        """Allow the MFMA screening + exact re-rank path for shared passes (K2 / K2w / K2g over an fp32 corpus, K2h over a
        halfvec corpus; K5r behind them).  False: exact kernels only (K1 / K1m, K1h), and no search of this context flags."""
        check(self._lib.vsr_set_screening(self._h, int(bool(enable))))

    def screening_check(self, nq=0):
        """(flagged queries since open, flags of the last vsr_search_device call).  Synchronises."""
        total = C.c_int64()
        flags = np.zeros(max(nq, 1), dtype=np.int32)
        check(self._lib.vsr_screening_check(self._h, C.byref(total), _ptr(flags) if nq else None, int(nq)))
        return total.value, flags[:nq]

    def tune(self, block_budget=-1, min_rows_per_block=0, max_queries_per_pass=0):
        check(self._lib.vsr_tune(self._h, block_budget, min_rows_per_block, max_queries_per_pass))

    def load_corpus(self, rows, block_ids=None, doc_ids=None, row_offset=0):
        return Corpus(self, rows, block_ids, doc_ids, row_offset)

    def load_corpus_half(self, rows, block_ids=None, doc_ids=None, row_offset=0):
        """A halfvec corpus (vsr_corpus_load_half): `rows` np.float16, resident as they are -- 2 bytes per element.  An fp32
        array is rounded to binary16 as Float4ToHalf does (round to nearest even); a finite element that would become
        +-Inf raises VsrError('"<v>" is out of range for type halfvec').  Searches go through the same Corpus methods."""
        rows = np.asarray(rows)
        if rows.dtype != np.float16:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            bad = np.isfinite(rows) & (np.abs(rows) >= np.float32(65520.0))
            if bad.any():
                raise VsrError(_ffi.ERR_INVALID, f'"{float(rows[bad].ravel()[0]):.9g}" is out of range for type halfvec')
            with np.errstate(over="ignore"):
                rows = rows.astype(np.float16)
        return Corpus(self, rows, block_ids, doc_ids, row_offset, half=True)

    def load_corpus_bit(self, rows, dim=None, block_ids=None, doc_ids=None, row_offset=0):
        """A bit corpus (vsr_corpus_load_bit): `rows` packed uint8 [n, (dim + 7) // 8] in varbit order, or a bool [n, dim]
        array (packed here with np.packbits; dim may then be omitted).  Searches go through Corpus.search_bit."""
        packed, dim = _packed_bits(rows, dim, "load_corpus_bit")
        return Corpus(self, packed, block_ids, doc_ids, row_offset, bit_dim=dim)

    def load_corpus_sparse(self, indptr, indices=None, values=None, dim=None, block_ids=None, doc_ids=None, row_offset=0):
        """A sparse corpus (vsr_corpus_load_sparse, pgvector's sparsevec): CSR rows as three arrays plus `dim` (zero-based
        indices), or any object with .indptr / .indices / .data / .shape.  Rows are validated as sparsevec_recv validates a
        value (VsrError in pgvector's words).  Searches go through Corpus.search_sparse."""
        ip, ix, vx, dim = _csr(indptr, indices, values, dim, "load_corpus_sparse")
        return Corpus(self, None, block_ids, doc_ids, row_offset, sparse=(ip, ix, vx, dim))

    def sparse_pair_distances(self, metric, a, b):
        """sparsevec's <->, <#>, <=>, <+> for pairs (a[i], b[i]): a, b are (indptr, indices, values, dim) tuples or objects with
        .indptr / .indices / .data / .shape, of equally many rows.  The operator's float8, bit for bit (one thread per pair runs
        sparsevec.c's own merge).  Raises VsrError('different sparsevec dimensions %d and %d') on a mismatch."""
        pa = _csr(*a, what="sparse_pair_distances") if isinstance(a, (tuple, list)) else _csr(a, what="sparse_pair_distances")
        pb = _csr(*b, what="sparse_pair_distances") if isinstance(b, (tuple, list)) else _csr(b, what="sparse_pair_distances")
        n = pa[0].size - 1
        if pb[0].size - 1 != n:
            raise ValueError("sparse_pair_distances: a and b must hold equally many rows")
        out = np.empty(n, dtype=np.float64)
        check(self._lib.vsr_sparse_pair_distances(self._h, _metric(metric), _ptr(pa[0]), _ptr(pa[1]), _ptr(pa[2]), _ptr(pb[0]),
                                                  _ptr(pb[1]), _ptr(pb[2]), n, pa[3], pb[3], _ptr(out)))
        return out

    def sparse_norms(self, a, indices=None, values=None, dim=None):
        """l2_norm of every sparse row (sparsevec.c:1044-1055): `a` as load_corpus_sparse takes rows.  float64 [n]."""
        ip, _, vx, _ = _csr(a, indices, values, dim, "sparse_norms")
        n = ip.size - 1
        out = np.empty(n, dtype=np.float64)
        check(self._lib.vsr_sparse_norms(self._h, _ptr(ip), _ptr(vx), n, _ptr(out)))
        return out

    def sparse_l2_normalize(self, a, indices=None, values=None, dim=None):
        """l2_normalize of every sparse row (sparsevec.c:1060-1120): (indptr, indices, values, dim) of the unit rows.  An entry
        whose quotient rounds to 0 is dropped, as pgvector drops it, so the result is a legal sparsevec; a row of zero norm stays
        as it is; raises VsrError('value out of range: overflow')."""
        ip, ix, vx, dim = _csr(a, indices, values, dim, "sparse_l2_normalize")
        n = ip.size - 1
        out = np.empty_like(vx)
        zeros = C.c_int64(0)
        check(self._lib.vsr_sparse_l2_normalize(self._h, _ptr(ip), _ptr(vx), n, _ptr(out), C.byref(zeros)))
        lo, hi = int(ip[0]), int(ip[-1])
        ix, out, ip = ix[lo:hi], out[:hi - lo], ip - lo     # (the library writes the entries it read, rebased to 0)
        if zeros.value:
            keep = out != 0
            kept = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
            ix, out, ip = ix[keep], out[keep], kept[ip]
        return ip, np.ascontiguousarray(ix), np.ascontiguousarray(out), dim

    def bit_pair_distances(self, metric, a, b, dim=None, dim_b=None):
        """hamming_distance / jaccard_distance for pairs (a[i], b[i]) of bit strings, bool or packed uint8 (then with `dim`;
        `dim_b` when b's length differs); b may be a single string (broadcast).  Raises VsrError('different bit lengths %u
        and %u') like pgvector's CheckDims."""
        bcast = np.asarray(b).ndim == 1
        pa, da = _packed_bits(a, dim, "bit_pair_distances")
        pb, db = _packed_bits(b, dim if dim_b is None else dim_b, "bit_pair_distances")
        out = np.empty(pa.shape[0], dtype=np.float64)
        check(self._lib.vsr_bit_pair_distances(self._h, _metric(metric), _ptr(pa), _ptr(pb), pa.shape[0], da, db, int(bcast),
                                               _ptr(out)))
        return out

    def binary_quantize(self, a):
        """binary_quantize of every row (vector.c:941-968): packed uint8 [n, (dim + 7) // 8], bit set where the element > 0."""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        out = np.zeros((a.shape[0], (a.shape[1] + 7) // 8), dtype=np.uint8)
        check(self._lib.vsr_binary_quantize(self._h, _ptr(a), a.shape[0], a.shape[1], _ptr(out)))
        return out

    def pair_distances(self, metric, a, b):
        """Operator value for pairs (a[i], b[i]); b may be a single vector (broadcast).
        Raises VsrError('different vector dimensions %d and %d') like pgvector's CheckDims."""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
        bcast = b.ndim == 1
        b2 = np.atleast_2d(b)
        out = np.empty(a.shape[0], dtype=np.float64)
        check(self._lib.vsr_pair_distances(self._h, _metric(metric), _ptr(a), _ptr(b2), a.shape[0],
                                           a.shape[1], b2.shape[1], int(bcast), _ptr(out)))
        return out

    def vector_norms(self, a):
        """vector_norm of every row (vector.c:756-769)."""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        out = np.empty(a.shape[0], dtype=np.float64)
        check(self._lib.vsr_vector_norms(self._h, _ptr(a), a.shape[0], a.shape[1], _ptr(out)))
        return out

    def l2_normalize(self, a):
        """l2_normalize of every row (vector.c:774-808); raises VsrError('value out of range: overflow')."""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        out = np.empty_like(a)
        check(self._lib.vsr_l2_normalize(self._h, _ptr(a), a.shape[0], a.shape[1], _ptr(out)))
        return out

    def spherical_distances(self, a, b):
        """vector_spherical_distance(a[i], b[i]) (vector.c:692-711); b may be a single vector."""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float32)))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
        bcast = b.ndim == 1
        b2 = np.atleast_2d(b)
        out = np.empty(a.shape[0], dtype=np.float64)
        check(self._lib.vsr_spherical_distances(self._h, _ptr(a), _ptr(b2), a.shape[0], a.shape[1], b2.shape[1], int(bcast),
                                                _ptr(out)))
        return out

    def ivf_kmeans(self, samples, lists, metric="l2", seed=1):
        """IVFFlat build, step 1 (ivfkmeans.c): k-means++ + Elkan's k-means over the sampled rows on the GPU.
        Returns (centers[lists, dim], iterations)."""
        s = np.ascontiguousarray(np.atleast_2d(np.asarray(samples, dtype=np.float32)))
        ns, dim = (0, s.shape[1]) if s.size == 0 else s.shape
        out = np.zeros((int(lists), dim), dtype=np.float32)
        it = C.c_int(0)
        check(self._lib.vsr_ivf_kmeans(self._h, _metric(metric), dim, _ptr(s), ns, int(lists), C.c_uint64(int(seed)), _ptr(out),
                                       C.byref(it)))
        return out, it.value

    def ivf_kmeans_half(self, samples_f16, lists, metric="l2", seed=1):
        """ivf_kmeans for the halfvec opclasses (vsr_ivf_kmeans_half): `samples_f16` np.float16; the centres are halfvec
        values, rounded to binary16 wherever the float build stores one.  Returns (centers[lists, dim] np.float16, iterations)."""
        s = np.ascontiguousarray(np.atleast_2d(_as_f16(samples_f16, "samples")))
        ns, dim = (0, s.shape[1]) if s.size == 0 else s.shape
        out = np.zeros((int(lists), dim), dtype=np.float16)
        it = C.c_int(0)
        check(self._lib.vsr_ivf_kmeans_half(self._h, _metric(metric), dim, _ptr(s), ns, int(lists), C.c_uint64(int(seed)),
                                            _ptr(out), C.byref(it)))
        return out, it.value

    def ivf_kmeans_bit(self, samples, lists, dim=None, seed=1):
        """ivf_kmeans for bit_hamming_ops (vsr_ivf_kmeans_bit): `samples` bool [n, dim] or packed uint8 [n, (dim + 7) // 8] with
        `dim`; the distance is the Hamming count and the centres are bit strings (bit i set where more than half of a centre's
        members have it).  Returns (centers packed uint8 [lists, (dim + 7) // 8], iterations)."""
        s, dim = _packed_bits(samples, dim, "ivf_kmeans_bit")
        out = np.zeros((int(lists), (dim + 7) // 8), dtype=np.uint8)
        it = C.c_int(0)
        check(self._lib.vsr_ivf_kmeans_bit(self._h, dim, _ptr(s), s.shape[0], int(lists), C.c_uint64(int(seed)), _ptr(out),
                                           C.byref(it)))
        return out, it.value

    def merge_topk_device(self, keys, block_ids, doc_ids, dist, n_parts, nq, k, out_block, out_doc, out_dist,
                          out_keys, out_counts):
        """Device pointers (ints).  Layout [n_parts][nq][k]."""
        check(self._lib.vsr_merge_topk_device(self._h, keys, block_ids, doc_ids, dist, n_parts, nq, k,
                                              out_block, out_doc, out_dist, out_keys, out_counts))


    def packed_result_bytes(self, nq, k):
        return self._lib.vsr_packed_result_bytes(int(nq), int(k))

    def merge_topk_packed_device(self, packed, n_parts, nq, k, out_block, out_doc, out_dist, out_keys, out_counts):
        """`packed`: device pointer to n_parts records of packed_result_bytes(nq, k) bytes (one all-gather)."""
        check(self._lib.vsr_merge_topk_packed_device(self._h, packed, n_parts, nq, k, out_block, out_doc, out_dist,
                                                     out_keys, out_counts))


class Filter:
    def __init__(self, corpus, handle, owned):
        self.corpus = corpus
        self._h = handle
        self._owned = owned

    @property
    def allowed_rows(self):
        return self.corpus._lib.vsr_filter_allowed_rows(self._h)

    @property
    def scanned_rows(self):
        return self.corpus._lib.vsr_filter_scanned_rows(self._h)

    def free(self):
        if self._owned and self._h:
            self.corpus._lib.vsr_filter_free(self._h)
        self._h = None

    def __del__(self):
        try:
            if self.corpus._h and self.corpus.ctx._h:   # (vsr_filter_free reaches through the corpus to its context)
                self.free()
        except Exception:
            pass


class Corpus:
    """Rows resident in HBM, identified as (document_id, block_id) like the reference's documentblocks table."""

    def __init__(self, ctx, rows, block_ids=None, doc_ids=None, row_offset=0, half=False, bit_dim=None, sparse=None):
        self.ctx = ctx
        self._lib = ctx._lib
        if sparse is not None:                       # (indptr, indices, values, dim) as _csr returns them (Context.load_corpus_sparse)
            ip, ix, vx, dim = sparse
            n = ip.size - 1
            blk = None if block_ids is None else np.ascontiguousarray(block_ids, dtype=np.int64)
            doc = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
            if (blk is not None and blk.size != n) or (doc is not None and doc.size != n):
                raise ValueError("block_ids / doc_ids must have one entry per row")
            h = C.c_void_p()
            check(self._lib.vsr_corpus_load_sparse(ctx._h, _ptr(ip), _ptr(ix), _ptr(vx), n, dim, _ptr(blk), _ptr(doc),
                                                   int(row_offset), C.byref(h)))
            self._h = h
            self.n, self.dim = n, dim
            self.row_offset = int(row_offset)
            self._user_filters = {}
            return
        bit = bit_dim is not None                    # rows: packed uint8 [n, (bit_dim + 7) // 8] (Context.load_corpus_bit)
        rows = np.ascontiguousarray(rows, dtype=np.uint8 if bit else np.float16 if half else np.float32)
        if rows.ndim != 2:
            raise ValueError("rows must be [n, dim]")
        n, dim = rows.shape
        if bit:
            dim = int(bit_dim)
        blk = None if block_ids is None else np.ascontiguousarray(block_ids, dtype=np.int64)
        doc = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
        if (blk is not None and blk.size != n) or (doc is not None and doc.size != n):
            raise ValueError("block_ids / doc_ids must have one entry per row")
        h = C.c_void_p()
        load = self._lib.vsr_corpus_load_bit if bit else self._lib.vsr_corpus_load_half if half else self._lib.vsr_corpus_load
        check(load(ctx._h, _ptr(rows), n, dim, _ptr(blk), _ptr(doc), int(row_offset), C.byref(h)))
        self._h = h
        self.n, self.dim = n, dim
        self.row_offset = int(row_offset)
        self._user_filters = {}

    @property
    def is_half(self):
        """True for a halfvec corpus (Context.load_corpus_half)."""
        return bool(self._lib.vsr_corpus_is_half(self._h))

    @property
    def is_bit(self):
        """True for a bit corpus (Context.load_corpus_bit, Corpus.binary_quantize)."""
        return bool(self._lib.vsr_corpus_is_bit(self._h))

    @property
    def is_sparse(self):
        """True for a sparse corpus (Context.load_corpus_sparse)."""
        return bool(self._lib.vsr_corpus_is_sparse(self._h))

    def binary_quantize(self):
        """A bit corpus of this corpus's resident rows, quantized on the device (vsr_corpus_binary_quantize): same context,
        row identity and internal order.  RBAC tables are not inherited: call load_rbac on the result."""
        h = C.c_void_p()
        check(self._lib.vsr_corpus_binary_quantize(self._h, C.byref(h)))
        out = Corpus.__new__(Corpus)
        out.ctx, out._lib, out._h = self.ctx, self._lib, h
        out.n, out.dim, out.row_offset = self.n, self.dim, self.row_offset
        out._user_filters = {}
        return out

    def device_bytes(self):
        """Device bytes holding vector data: rows, norms and every screening plane (vsr_corpus_device_bytes)."""
        return int(self._lib.vsr_corpus_device_bytes(self._h))

    def free(self):
        if getattr(self, "_h", None):
            self._lib.vsr_corpus_free(self._h)
            self._h = None

    def __del__(self):
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass

    # ---- RBAC -------------------------------------------------------------------------------
    def load_rbac(self, user_roles, permissions):
        """user_roles: (user_id, role_id) pairs; permissions: (role_id, document_id) pairs."""
        ur = np.ascontiguousarray(np.asarray(user_roles, dtype=np.int32).reshape(-1, 2))
        pa = np.ascontiguousarray(np.asarray(permissions, dtype=np.int32).reshape(-1, 2))
        u, r = np.ascontiguousarray(ur[:, 0]), np.ascontiguousarray(ur[:, 1])
        pr, pd = np.ascontiguousarray(pa[:, 0]), np.ascontiguousarray(pa[:, 1])
        check(self._lib.vsr_rbac_load(self._h, _ptr(u), _ptr(r), len(ur), _ptr(pr), _ptr(pd), len(pa)))
        self._user_filters = {}

    def filter_for_user(self, user_id, mode=RANGES):
        key = (int(user_id), int(mode))
        f = self._user_filters.get(key)
        if f is None:
            h = C.c_void_p()
            check(self._lib.vsr_filter_for_user(self._h, int(user_id), int(mode), C.byref(h)))
            f = self._user_filters[key] = Filter(self, h, owned=False)
        return f

    def filter_for_roles(self, role_ids, mode=RANGES):
        r = np.ascontiguousarray(role_ids, dtype=np.int32)
        h = C.c_void_p()
        check(self._lib.vsr_filter_for_roles(self._h, _ptr(r), r.size, int(mode), C.byref(h)))
        return Filter(self, h, owned=False)

    def filter_from_bytemask(self, allowed, mode=BITMAP):
        m = np.ascontiguousarray(allowed, dtype=np.uint8)
        if m.size != self.n:
            raise ValueError("mask must have one byte per row")
        h = C.c_void_p()
        check(self._lib.vsr_filter_from_bytemask(self._h, _ptr(m), int(mode), C.byref(h)))
        return Filter(self, h, owned=True)

    def filter_from_documents(self, doc_ids, user_id=-1):
        d = np.ascontiguousarray(doc_ids, dtype=np.int32)
        h = C.c_void_p()
        check(self._lib.vsr_filter_from_documents(self._h, _ptr(d), d.size, int(user_id), C.byref(h)))
        return Filter(self, h, owned=True)

    # ---- indexes -----------------------------------------------------------------------------
    def load_ivf(self, centers, row_list):
        """IVFFlat index over this corpus: centres [lists, dim] and the list of every row (caller row order)."""
        return IvfIndex(self, centers, row_list)

    def build_ivf(self, rows, lists=100, metric="l2", seed=1, sample=None):
        """CREATE INDEX ... USING ivfflat on the GPU (ivfbuild.c:998-1019): sample max(lists * 50, 10000) of `rows` (this
        corpus's rows in the caller's order, host array), k-means on the sample (vsr_ivf_kmeans), every row into its
        nearest list (vsr_ivf_assign), list-ordered image (vsr_ivf_load).  Returns (IvfIndex, centers, row_list)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = rows.shape[0]
        want = max(int(lists) * 50, 10000) if sample is None else int(sample)
        rng = np.random.default_rng(seed)
        pick = np.sort(rng.choice(n, size=min(n, want), replace=False)) if n else np.zeros(0, dtype=np.int64)
        centers, _ = self.ctx.ivf_kmeans(rows[pick], lists, metric, seed)
        row_list = self.ivf_assign(centers, metric)
        return IvfIndex(self, centers, row_list), centers, row_list

    def load_ivf_half(self, centers_f16, row_list):
        """load_ivf over this halfvec corpus (vsr_ivf_load_half): centres np.float16 [lists, dim]; the list-ordered image and the
        centres stay binary16 on the device.  The index answers IvfIndex.search* / probe like any float index."""
        return IvfIndex(self, centers_f16, row_list, half=True)

    def build_ivf_half(self, rows_f16, lists=100, metric="l2", seed=1, sample=None):
        """CREATE INDEX ... USING ivfflat (col halfvec_l2_ops | halfvec_ip_ops | halfvec_cosine_ops) over this halfvec corpus:
        build_ivf's sampling rule on `rows_f16` (this corpus's rows in the caller's order, np.float16), vsr_ivf_kmeans_half,
        vsr_ivf_assign_half, vsr_ivf_load_half.  Returns (IvfIndex, centers np.float16, row_list)."""
        rows = np.ascontiguousarray(_as_f16(rows_f16, "rows"))
        n = rows.shape[0]
        want = max(int(lists) * 50, 10000) if sample is None else int(sample)
        rng = np.random.default_rng(seed)
        pick = np.sort(rng.choice(n, size=min(n, want), replace=False)) if n else np.zeros(0, dtype=np.int64)
        centers, _ = self.ctx.ivf_kmeans_half(rows[pick], lists, metric, seed)
        row_list = self.ivf_assign_half(centers, metric)
        return IvfIndex(self, centers, row_list, half=True), centers, row_list

    def load_ivf_bit(self, centers, row_list):
        """load_ivf over this bit corpus (vsr_ivf_load_bit, bit_hamming_ops): centres bool [lists, dim] or packed uint8
        [lists, (dim + 7) // 8]; image and centres stay packed on the device.  The index answers IvfIndex.probe_bit /
        search_bit*."""
        return IvfIndex(self, centers, row_list, bit=True)

    def build_ivf_bit(self, rows, lists=100, seed=1, sample=None):
        """CREATE INDEX ... USING ivfflat (col bit_hamming_ops) over this bit corpus: build_ivf's sampling rule on `rows` (this
        corpus's rows in the caller's order, bool or packed uint8), vsr_ivf_kmeans_bit, vsr_ivf_assign_bit, vsr_ivf_load_bit.
        Returns (IvfIndex, centers packed uint8, row_list)."""
        rows, dim = _packed_bits(rows, self.dim, "build_ivf_bit")
        n = rows.shape[0]
        want = max(int(lists) * 50, 10000) if sample is None else int(sample)
        rng = np.random.default_rng(seed)
        pick = np.sort(rng.choice(n, size=min(n, want), replace=False)) if n else np.zeros(0, dtype=np.int64)
        centers, _ = self.ctx.ivf_kmeans_bit(rows[pick], lists, dim, seed)
        row_list = self.ivf_assign_bit(centers)
        return IvfIndex(self, centers, row_list, bit=True), centers, row_list

    def build_hnsw(self, m=16, ef_construction=64, metric="l2", seed=1, merge_duplicates=False):
        """CREATE INDEX ... USING hnsw on the GPU (vsr_hnsw_build): batched insertion, recall parity with the serial build.
        merge_duplicates: byte-identical rows share an element of up to 10 heap TIDs, as in pgvector (vsr_hnsw_build_ex)."""
        h = C.c_void_p()
        if merge_duplicates:
            check(self._lib.vsr_hnsw_build_ex(self._h, int(m), int(ef_construction), _metric(metric), int(seed),
                                              BUILD_MERGE_DUPLICATES, C.byref(h)))
        else:
            check(self._lib.vsr_hnsw_build(self._h, int(m), int(ef_construction), _metric(metric), int(seed), C.byref(h)))
        return HnswIndex(self, h)

    def build_hnsw_partitions(self, parts, m=16, ef_construction=64, metric=None, seed=1):
        """One HNSW index per row subset -- a role table, a dynamic partition -- built in one call over this corpus, whose rows
        stay resident once (vsr_hnsw_build_partitions).  `parts`: a sequence of row-index sequences of this corpus; they may
        overlap, come in any order and be empty, but a partition names a row once.  Returns a list of HnswIndex, one per
        partition, each the graph build_hnsw / build_hnsw_half / build_hnsw_bit (the row format is this corpus's) with the same
        m, ef_construction, metric and seed makes of a corpus holding only that partition's rows, its heap TIDs being row indices
        of THIS corpus.  metric: None is "l2", or "hamming" on a bit corpus, where it also becomes the indexes' opclass.  On an
        error no index is left behind."""
        if metric is None:
            metric = "hamming" if self.is_bit else "l2"
        rows = [np.ascontiguousarray(np.asarray(p, dtype=np.int64).ravel()) for p in parts]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([r.size for r in rows])
        flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, dtype=np.int64)
        handles = (C.c_void_p * max(len(rows), 1))()
        check(self._lib.vsr_hnsw_build_partitions(self._h, len(rows), _ptr(off), _ptr(flat), int(m), int(ef_construction),
                                                  _metric(metric), int(seed), 0, handles))
        return [HnswIndex(self, C.c_void_p(handles[g])) for g in range(len(rows))]

    def extend_hnsw_partitions(self, indexes, new_parts, ef_construction=64, metric=None, seed=1):
        """extend_hnsw for many graphs of this corpus in one call (vsr_hnsw_extend_partitions): graph g, `indexes[g]`, takes the
        rows `new_parts[g]` (row indices of this corpus; may be empty).  `indexes`: HnswIndex objects over this corpus -- what
        build_hnsw_partitions or an earlier call of this method returned, or any others of one m -- or None for an empty graph; at
        least one must be an index, because m is theirs.  Partitions may share rows and an index may be named twice; a row a graph
        holds already is refused.  Returns a list of NEW HnswIndex, one per partition: each the graph extend_hnsw with the same
        ef_construction, metric and seed makes of that graph alone over a corpus of its own rows.  The indexes passed in stay as
        they are and stay the caller's to free.  metric: None is "l2", or "hamming" on a bit corpus, where it must be the indexes'
        opclass.  On an error no index is left behind."""
        if metric is None:
            metric = "hamming" if self.is_bit else "l2"
        if len(indexes) != len(new_parts):
            raise ValueError(f"{len(indexes)} indexes but {len(new_parts)} row lists")
        rows = [np.ascontiguousarray(np.asarray(p, dtype=np.int64).ravel()) for p in new_parts]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([r.size for r in rows])
        flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, dtype=np.int64)
        for g, h in enumerate(indexes):
            if h is not None and not getattr(h, "_h", None):
                raise ValueError(f"indexes[{g}] has been freed")          # NULL would quietly mean an empty graph
        prior = (C.c_void_p * max(len(rows), 1))(*[None if h is None else h._h for h in indexes])
        handles = (C.c_void_p * max(len(rows), 1))()
        check(self._lib.vsr_hnsw_extend_partitions(self._h, len(rows), prior, _ptr(off), _ptr(flat), int(ef_construction),
                                                   _metric(metric), int(seed), 0, handles))
        return [HnswIndex(self, C.c_void_p(handles[g])) for g in range(len(rows))]

    def hnsw_forest(self, indexes):
        """HnswForest over indexes of this corpus (the list build_hnsw_partitions returns, or any others of one row format and one
        m): their graphs searched as a set, one search launch and one merge launch per call (vsr_hnsw_forest_open)."""
        return HnswForest(indexes, corpus=self)

    def load_hnsw(self, graph):
        """HNSW graph over this corpus; `graph`: dict with m, entry, level, nbr0, tid_count, tids, up_slot, up_nbr,
        max_level (include/vsrbac.h, vsr_hnsw_load: what a dump of pgvector's in-memory build holds)."""
        return HnswIndex(self, graph)

    def extend_hnsw(self, graph, ef_construction=64, metric=None, seed=1):
        """INSERT for a batch of rows (vsr_hnsw_extend): `graph` is the dict HnswIndex.export() returns for a graph over SOME of
        this corpus's rows -- its TIDs are row indices of this corpus -- and the rows no TID names are inserted by build_hnsw's own
        batches, in internal row order, with levels from the build's seeded stream (the i-th new row takes the draw after those of
        the covered rows).  fp32, halfvec and bit corpora; metric: None is "l2", or "hamming" on a bit corpus, where it also becomes
        the index's opclass.  Extending a prefix build at one of the build's batch boundaries gives the one-shot build's graph.
        Recipe: load the corpus again with the new rows (old rows at their old indices, or map the TIDs), extend_hnsw(old.export()),
        then free the old index and the old corpus."""
        if metric is None:
            metric = "hamming" if self.is_bit else "l2"
        a = lambda name, dt: np.ascontiguousarray(graph[name], dtype=dt)
        level, nbr0, tc, tids = a("level", np.int32), a("nbr0", np.int32), a("tid_count", np.int32), a("tids", np.int64)
        up_slot, up_nbr = a("up_slot", np.int32), a("up_nbr", np.int32)
        n_upper = int((up_slot >= 0).sum())
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_extend(self._h, int(graph["m"]), level.size, int(graph["entry"]), _ptr(level), _ptr(nbr0), _ptr(tc),
                                        _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper, int(graph["max_level"]),
                                        int(ef_construction), _metric(metric), int(seed), 0, C.byref(h)))
        return HnswIndex(self, h)

    def vacuum_hnsw(self, graph, dead_rows, ef_construction=64, metric=None):
        """VACUUM after DELETE (vsr_hnsw_vacuum): `graph` is the dict HnswIndex.export() returns for a graph over this corpus,
        `dead_rows` the row indices of this corpus that were deleted (duplicates allowed, rows no TID names ignored).  The rows
        stay in this corpus: the repair walks through deleted elements.  Every live element that pointed at a deleted one, or
        whose layer-0 list is not full, is repaired on the GPU with the build's search and selection; the deleted elements are
        then squeezed out and the live ones renumbered in ascending old id.  fp32, halfvec and bit corpora; metric: None is
        "l2", or "hamming" on a bit corpus.  Returns (HnswIndex, stats): stats has tuples_removed, tuples_kept,
        elements_removed, elements_repaired, batches, attempts and "elem_map", the new id of every old element (-1: deleted).
        No dead rows: the graph is loaded as it is.  Everything dead: an empty index whose searches return nothing.
        Recipe to drop the rows from the corpus as well: vacuum, export() the result, formats.remap_hnsw_rows(export,
        new_index_of_old_row), reload the corpus without the dead rows, load_hnsw(remapped) on it, free the old pair.
        UPDATE is vacuum followed by extend_hnsw: remap onto a corpus of the live rows plus the new versions (the extension
        inserts every row no TID names, so the dead rows must be gone from it) and extend there."""
        if metric is None:
            metric = "hamming" if self.is_bit else "l2"
        a = lambda name, dt: np.ascontiguousarray(graph[name], dtype=dt)
        level, nbr0, tc, tids = a("level", np.int32), a("nbr0", np.int32), a("tid_count", np.int32), a("tids", np.int64)
        up_slot, up_nbr = a("up_slot", np.int32), a("up_nbr", np.int32)
        n_upper = int((up_slot >= 0).sum())
        dead = np.ascontiguousarray(np.asarray(dead_rows, dtype=np.int64).ravel())
        elem_map = np.full(level.size, -1, dtype=np.int32)
        st = _ffi.HnswVacuumStats()
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_vacuum(self._h, int(graph["m"]), level.size, int(graph["entry"]), _ptr(level), _ptr(nbr0), _ptr(tc),
                                        _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper, int(graph["max_level"]),
                                        int(ef_construction), _metric(metric), _ptr(dead), dead.size, 0, _ptr(elem_map),
                                        C.byref(st), C.byref(h)))
        stats = {name: int(getattr(st, name)) for name, _ in st._fields_}
        stats["elem_map"] = elem_map
        return HnswIndex(self, h), stats

    def build_hnsw_bit(self, m=16, ef_construction=64, metric="hamming", seed=1, merge_duplicates=False):
        """CREATE INDEX ... USING hnsw (col bit_hamming_ops | bit_jaccard_ops) over this bit corpus (vsr_hnsw_build_bit):
        build_hnsw's batched insertion on the packed rows.  merge_duplicates: byte-identical rows share an element -- the
        build to use on a quantized corpus, which is full of duplicates."""
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_build_bit(self._h, int(m), int(ef_construction), _metric(metric), int(seed),
                                           BUILD_MERGE_DUPLICATES if merge_duplicates else 0, C.byref(h)))
        return HnswIndex(self, h)

    def load_hnsw_bit(self, graph, metric="hamming"):
        """load_hnsw over this bit corpus (vsr_hnsw_load_bit): `metric` is the opclass the graph was built for, "hamming" or
        "jaccard"; the index then answers HnswIndex.search_bit* with that metric only."""
        return HnswIndex(self, graph, bit_metric=_metric(metric))

    def build_hnsw_half(self, m=16, ef_construction=64, metric="l2", seed=1, merge_duplicates=False):
        """CREATE INDEX ... USING hnsw (col halfvec_l2_ops | halfvec_ip_ops | halfvec_cosine_ops) over this halfvec corpus
        (vsr_hnsw_build_half): build_hnsw's batched insertion on the binary16 rows.  merge_duplicates: rows whose binary16 bytes
        are identical share an element.  The index answers HnswIndex.search* like any float index."""
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_build_half(self._h, int(m), int(ef_construction), _metric(metric), int(seed),
                                            BUILD_MERGE_DUPLICATES if merge_duplicates else 0, C.byref(h)))
        return HnswIndex(self, h)

    def load_hnsw_half(self, graph):
        """load_hnsw over this halfvec corpus (vsr_hnsw_load_half): the graph kernels read the binary16 rows themselves."""
        return HnswIndex(self, graph, half=True)

    def build_hnsw_sparse(self, m=16, ef_construction=64, metric="l2", seed=1, merge_duplicates=False):
        """CREATE INDEX ... USING hnsw (col sparsevec_l2_ops | sparsevec_ip_ops | sparsevec_cosine_ops | sparsevec_l1_ops) over
        this sparse corpus (vsr_hnsw_build_sparse): build_hnsw's batched insertion on the CSR rows, at most 1000 non-zeros per
        row.  Cosine: load unit rows (Context.sparse_l2_normalize).  merge_duplicates is refused (VsrError).  The index answers
        HnswIndex.search_sparse*."""
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_build_sparse(self._h, int(m), int(ef_construction), _metric(metric), int(seed),
                                              BUILD_MERGE_DUPLICATES if merge_duplicates else 0, C.byref(h)))
        return HnswIndex(self, h)

    def load_hnsw_sparse(self, graph):
        """load_hnsw over this sparse corpus (vsr_hnsw_load_sparse); the index answers HnswIndex.search_sparse*, metric per call."""
        return HnswIndex(self, graph, sparse=True)

    # ---- search ------------------------------------------------------------------------------
    def pack_filters(self, filters):
        """One filter per query as a reusable C array (build it once when the same batch shape repeats)."""
        arr = (C.c_void_p * len(filters))(*[(f._h if f is not None else None) for f in filters])
        arr._keep = list(filters)                    # the handles must outlive the array
        return arr

    def _filter_array(self, filters, nq):
        if filters is None:
            return None, None
        if isinstance(filters, C.Array):
            if len(filters) != nq:
                raise ValueError("one filter per query")
            return filters, filters
        if isinstance(filters, Filter):
            filters = [filters] * nq
        if len(filters) != nq:
            raise ValueError("one filter per query")
        arr = (C.c_void_p * nq)(*[(f._h if f is not None else None) for f in filters])
        return arr, filters

    def search(self, queries, k, metric="l2", filters=None):
        """Host buffers in and out.  Returns SearchResult of [nq, k] arrays (+ counts[nq])."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = self._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_search(self._h, _ptr(q), nq, dim, int(k), _metric(metric), farr, _ptr(blk), _ptr(doc),
                                   _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_bit(self, queries, k, metric="hamming", filters=None, dim=None):
        """Corpus.search over a bit corpus: `queries` bool [nq, dim] or packed uint8 [nq, (dim + 7) // 8] (dim: the corpus's
        unless given), metric "hamming" / "<~>" or "jaccard" / "<%>".  Exact; never flags."""
        q, qdim = _packed_bits(queries, self.dim if dim is None else dim, "search_bit")
        nq = q.shape[0]
        farr, keep = self._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_search_bit(self._h, _ptr(q), nq, qdim, int(k), _metric(metric), farr, _ptr(blk), _ptr(doc),
                                       _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_sparse(self, queries, k, metric="l2", filters=None, indices=None, values=None, dim=None):
        """Corpus.search over a sparse corpus: `queries` as CSR -- an object with .indptr / .indices / .data / .shape, or the
        indptr array with `indices`, `values` (dim: the corpus's unless given).  metric "l2", "ip", "cosine" or "l1".
        Exact; never flags."""
        if indices is None and hasattr(queries, "indptr"):
            ip, ix, vx, qdim = _csr(queries, dim=dim, what="search_sparse")
        else:
            ip, ix, vx, qdim = _csr(queries, indices, values, self.dim if dim is None else dim, "search_sparse")
        nq = ip.size - 1
        farr, keep = self._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_search_sparse(self._h, _ptr(ip), _ptr(ix), _ptr(vx), nq, qdim, int(k), _metric(metric), farr,
                                          _ptr(blk), _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_sparse_device(self, d_indptr, d_indices, d_values, nq, max_query_nnz, k, metric, filters, d_block, d_doc, d_rows,
                             d_dist, d_counts, d_keys=None, dim=None, session=None):
        """search_device over a sparse corpus (vsr_search_sparse_device_on): the queries' CSR arrays in device memory (int64,
        int32, float32) and the largest non-zero count of any of them; a longer query fails screening_check."""
        farr, keep = self._filter_array(filters, nq)
        check(self._lib.vsr_search_sparse_device_on(session._h if session is not None else None, self._h, d_indptr, d_indices,
                                                    d_values, nq, self.dim if dim is None else dim, int(max_query_nnz), int(k),
                                                    _metric(metric), farr, d_block, d_doc, d_rows, d_dist, d_counts, d_keys))
        return keep

    def search_bit_device(self, d_queries, nq, k, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_keys=None,
                          dim=None, session=None):
        """search_device over a bit corpus (vsr_search_bit_device_on): d_queries addresses nq x (dim + 7) // 8 packed bytes,
        any alignment."""
        farr, keep = self._filter_array(filters, nq)
        check(self._lib.vsr_search_bit_device_on(session._h if session is not None else None, self._h, d_queries, nq,
                                                 self.dim if dim is None else dim, int(k), _metric(metric), farr, d_block,
                                                 d_doc, d_rows, d_dist, d_counts, d_keys))
        return keep

    def search_device(self, d_queries, nq, k, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_keys=None,
                      dim=None, session=None):
        """Device pointers (ints); enqueues on the context's stream, does not synchronise.  `session`: another Context
        of the same GPU whose stream and workspaces the search uses (two batches in flight over one corpus)."""
        farr, keep = self._filter_array(filters, nq)
        check(self._lib.vsr_search_device_on(session._h if session is not None else None, self._h, d_queries, nq,
                                             self.dim if dim is None else dim, int(k), _metric(metric), farr, d_block,
                                             d_doc, d_rows, d_dist, d_counts, d_keys))
        return keep

    def search_quantized(self, bits, queries, k, shortlist, metric="l2", filters=None):
        """Two-stage search (vsr_search_quantized): the `shortlist` nearest permitted rows of `bits` -- this corpus's
        binary_quantize() -- by Hamming distance to binary_quantize(query), re-ranked by the exact `metric` distance to this
        corpus's rows; the first k.  `filters` are filters of `bits`.  k <= shortlist <= MAX_K; "l2", "ip" or "cosine"."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = bits._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_search_quantized(self._h, bits._h, _ptr(q), nq, dim, int(k), int(shortlist), _metric(metric), farr,
                                             _ptr(blk), _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_quantized_device(self, bits, d_queries, nq, k, shortlist, metric, filters, d_block, d_doc, d_rows, d_dist,
                                d_counts, d_keys=None, session=None):
        """search_quantized with device pointers (ints): d_queries addresses nq x dim floats.  Both stages are enqueued on the
        stream of `session` (None: the context of `bits`); nothing synchronises (vsr_search_quantized_device_on)."""
        farr, keep = bits._filter_array(filters, nq)
        check(self._lib.vsr_search_quantized_device_on(session._h if session is not None else None, self._h, bits._h, d_queries,
                                                       nq, self.dim, int(k), int(shortlist),
                                                       _metric(metric), farr, d_block, d_doc, d_rows, d_dist, d_counts, d_keys))
        return keep

    def search_quantized_hnsw(self, bit_index, queries, k, shortlist, ef_search=40, metric="l2", filters=None):
        """search_quantized with the shortlist taken from an index (vsr_hnsw_search_quantized): `bit_index` is a Hamming
        HnswIndex over this corpus's binary_quantize(); the shortlist is its search_bit answer for k = shortlist and
        ef_search (it may be shorter than `shortlist`), the re-rank is search_quantized's.  `filters` are filters of the bit
        corpus."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = bit_index.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_hnsw_search_quantized(self._h, bit_index._h, _ptr(q), nq, dim, int(k), int(shortlist), int(ef_search),
                                                  _metric(metric), farr, _ptr(blk), _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_quantized_hnsw_device(self, bit_index, d_queries, nq, k, shortlist, ef_search, metric, filters, d_block, d_doc,
                                     d_rows, d_dist, d_counts, d_keys=None):
        """search_quantized_hnsw with device pointers (ints): d_queries addresses nq x dim floats.  Both stages are enqueued on
        the bit corpus context's stream; nothing synchronises (vsr_hnsw_search_quantized_device)."""
        farr, keep = bit_index.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_quantized_device(self._h, bit_index._h, d_queries, nq, self.dim, int(k), int(shortlist),
                                                         int(ef_search), _metric(metric), farr, d_block, d_doc, d_rows, d_dist,
                                                         d_counts, d_keys))
        return keep

    def search_quantized_ivf(self, bit_index, queries, k, shortlist, probes=1, metric="l2", filters=None, mode="off",
                             max_probes=32768):
        """search_quantized with the shortlist taken from the lists of an index (vsr_ivf_search_quantized): `bit_index` is an
        IvfIndex over this corpus's binary_quantize() (load_ivf_bit / build_ivf_bit); the shortlist is its search_bit_iterative
        answer for k = shortlist, `probes`, `mode` ("off": search_bit's, max_probes ignored) and `max_probes`, the re-rank is
        search_quantized's.  `filters` are filters of the bit corpus.  Returns SearchResult and the lists each scan had taken."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = bit_index.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        scanned = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_ivf_search_quantized(self._h, bit_index._h, _ptr(q), nq, dim, int(k), int(shortlist), int(probes),
                                                 _metric(metric), farr, _ivf_iterative_mode(mode), int(max_probes), _ptr(blk),
                                                 _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt), _ptr(scanned)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), scanned

    def search_quantized_ivf_device(self, bit_index, d_queries, nq, k, shortlist, probes, metric, filters, mode, max_probes,
                                    d_block, d_doc, d_rows, d_dist, d_counts, d_probes=None, d_keys=None):
        """search_quantized_ivf with device pointers (ints): d_queries addresses nq x dim floats.  Both stages are enqueued on
        the bit corpus context's stream; nothing synchronises (vsr_ivf_search_quantized_device)."""
        farr, keep = bit_index.corpus._filter_array(filters, nq)
        check(self._lib.vsr_ivf_search_quantized_device(self._h, bit_index._h, d_queries, nq, self.dim, int(k), int(shortlist),
                                                        int(probes), _metric(metric), farr, _ivf_iterative_mode(mode),
                                                        int(max_probes), d_block, d_doc, d_rows, d_dist, d_counts, d_probes,
                                                        d_keys))
        return keep

    def ivf_assign(self, centers, metric="l2"):
        """The pass of the ivfflat build that touches every row (ivfbuild.c:404-445): the nearest centre of each row, in
        the caller's row order -- the `row_list` IvfIndex / vsr_ivf_load take."""
        c = np.ascontiguousarray(centers, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] != self.dim:
            raise VsrError(_ffi.ERR_INVALID, f"centers must be (lists, {self.dim})")
        out = np.zeros(self.n, dtype=np.int32)
        check(self._lib.vsr_ivf_assign(self._h, _ptr(c), int(c.shape[0]), _metric(metric), _ptr(out)))
        return out

    def ivf_assign_half(self, centers_f16, metric="l2"):
        """ivf_assign over this halfvec corpus (vsr_ivf_assign_half): centres np.float16, compared with the binary16 rows where
        they lie."""
        c = np.ascontiguousarray(_as_f16(centers_f16, "centers"))
        if c.ndim != 2 or c.shape[1] != self.dim:
            raise VsrError(_ffi.ERR_INVALID, f"centers must be (lists, {self.dim})")
        out = np.zeros(self.n, dtype=np.int32)
        check(self._lib.vsr_ivf_assign_half(self._h, _ptr(c), int(c.shape[0]), _metric(metric), _ptr(out)))
        return out

    def ivf_assign_bit(self, centers):
        """ivf_assign over this bit corpus (vsr_ivf_assign_bit): the centre of the lowest (Hamming count, list id) for each row."""
        c, _ = _packed_bits(centers, self.dim, "ivf_assign_bit")
        out = np.zeros(self.n, dtype=np.int32)
        check(self._lib.vsr_ivf_assign_bit(self._h, _ptr(c), int(c.shape[0]), _ptr(out)))
        return out

    def search_device_exact(self, d_queries, nq, k, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_keys=None,
                            dim=None, session=None):
        """search_device + wait + exact re-run of whatever the screening flagged (vsr_search_device_exact): returns the
        number of queries that were re-run; every row of the outputs is proven exact when it returns."""
        farr, keep = self._filter_array(filters, nq)
        n = C.c_int32(0)
        check(self._lib.vsr_search_device_exact(session._h if session is not None else None, self._h, d_queries, nq,
                                                self.dim if dim is None else dim, int(k), _metric(metric), farr, d_block,
                                                d_doc, d_rows, d_dist, d_counts, d_keys, C.byref(n)))
        del keep
        return int(n.value)


class IvfIndex:
    """pgvector's ivfflat scan (ivfscan.c) on the GPU: probe the nearest lists, scan them, keep the permitted top-k."""

    def __init__(self, corpus, centers, row_list, half=False, bit=False):
        self.corpus, self._lib = corpus, corpus._lib
        rl = np.ascontiguousarray(row_list, dtype=np.int32)
        if bit:                                                                     # (Corpus.load_ivf_bit)
            c, _ = _packed_bits(centers, corpus.dim, "centers")
            if rl.size != corpus.n:
                raise ValueError("row_list must have one entry per row")
        else:
            c = np.ascontiguousarray(_as_f16(centers, "centers")) if half else np.ascontiguousarray(centers, dtype=np.float32)
            if c.ndim != 2 or c.shape[1] != corpus.dim or rl.size != corpus.n:
                raise ValueError("centers must be [lists, dim] and row_list must have one entry per row")
        h = C.c_void_p()
        load = self._lib.vsr_ivf_load_bit if bit else self._lib.vsr_ivf_load_half if half else self._lib.vsr_ivf_load   # (half: Corpus.load_ivf_half)
        check(load(corpus._h, _ptr(c), c.shape[0], _ptr(rl), C.byref(h)))
        self._h, self.lists = h, c.shape[0]

    def device_bytes(self):
        """Device memory of the index in bytes (vsr_ivf_device_bytes): the list-ordered image of the rows with norms and rank
        map, the centres, the list offsets; the corpus itself: Corpus.device_bytes."""
        return int(self._lib.vsr_ivf_device_bytes(self._h))

    def free(self):
        if getattr(self, "_h", None):
            self._lib.vsr_ivf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            if self.corpus._h and self.corpus.ctx._h:
                self.free()
        except Exception:
            pass

    def search_device(self, d_queries, nq, k, probes, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts):
        """Device pointers (ints); returns when every query is proven exact over its lists (vsr_ivf_search_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_ivf_search_device(self._h, d_queries, nq, self.corpus.dim, int(k), int(probes), _metric(metric),
                                              farr, d_block, d_doc, d_rows, d_dist, d_counts))
        del keep

    def probe(self, queries, probes, metric="l2"):
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        p = min(int(probes), self.lists)
        out = np.zeros((q.shape[0], p), dtype=np.int32)
        check(self._lib.vsr_ivf_probe(self._h, _ptr(q), q.shape[0], q.shape[1], int(probes), _metric(metric), _ptr(out)))
        return out

    def search(self, queries, k, probes, metric="l2", filters=None):
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = self.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_ivf_search(self._h, _ptr(q), nq, dim, int(k), int(probes), _metric(metric), farr, _ptr(blk),
                                       _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_iterative_device(self, d_queries, nq, k, probes, metric, filters, mode, max_probes, d_block, d_doc, d_rows,
                                d_dist, d_counts, d_probes=None):
        """Device pointers (ints); returns when every query is proven exact (vsr_ivf_search_iterative_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_ivf_search_iterative_device(self._h, d_queries, nq, self.corpus.dim, int(k), int(probes),
                                                        _metric(metric), farr, _ivf_iterative_mode(mode), int(max_probes),
                                                        d_block, d_doc, d_rows, d_dist, d_counts, d_probes))
        del keep

    def search_iterative(self, queries, k, probes, metric="l2", filters=None, mode="relaxed_order", max_probes=32768):
        """pgvector's iterative index scan (ivfflat.iterative_scan = mode, ivfflat.max_probes): batches of `probes` lists,
        nearest lists first, until k permitted rows are out or max_probes lists are scanned.  SearchResult (rows in stream
        order: sorted inside a batch, not across batches) plus, as a second value, the lists each query's scan had taken
        when it stopped (so->listIndex)."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = self.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        scanned = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_ivf_search_iterative(self._h, _ptr(q), nq, dim, int(k), int(probes), _metric(metric), farr,
                                                 _ivf_iterative_mode(mode), int(max_probes), _ptr(blk), _ptr(doc), _ptr(row),
                                                 _ptr(dist), _ptr(cnt), _ptr(scanned)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), scanned

    # ---- an index over a bit corpus (Corpus.load_ivf_bit / build_ivf_bit, bit_hamming_ops) ----
    def probe_bit(self, queries, probes, dim=None):
        """IvfIndex.probe for a bit index (vsr_ivf_probe_bit): `queries` bool [nq, dim] or packed uint8 [nq, (dim + 7) // 8]; the
        lists in (Hamming count to the centre, list id) order."""
        q, qdim = _packed_bits(queries, self.corpus.dim if dim is None else dim, "probe_bit")
        p = min(int(probes), self.lists)
        out = np.zeros((q.shape[0], p), dtype=np.int32)
        check(self._lib.vsr_ivf_probe_bit(self._h, _ptr(q), q.shape[0], qdim, int(probes), _ptr(out)))
        return out

    def _results(self, nq, k):
        kk = max(int(k), 1)
        return (np.full((nq, kk), -1, dtype=np.int64), np.full((nq, kk), -1, dtype=np.int32), np.full((nq, kk), -1, dtype=np.int64),
                np.full((nq, kk), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.int32))

    def search_bit(self, queries, k, probes, metric="hamming", filters=None, dim=None):
        """IvfIndex.search for a bit index (vsr_ivf_search_bit): queries as in probe_bit, metric "hamming" / "<~>"; rows rank as
        Corpus.search_bit ranks them."""
        q, qdim = _packed_bits(queries, self.corpus.dim if dim is None else dim, "search_bit")
        nq = q.shape[0]
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        check(self._lib.vsr_ivf_search_bit(self._h, _ptr(q), nq, qdim, int(k), int(probes), _metric(metric), farr, _ptr(blk),
                                           _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt)

    def search_bit_device(self, d_queries, nq, k, probes, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, dim=None):
        """search_device for a bit index (vsr_ivf_search_bit_device): d_queries addresses nq x (dim + 7) // 8 packed bytes, any
        alignment; returns when the results are complete."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_ivf_search_bit_device(self._h, d_queries, nq, self.corpus.dim if dim is None else dim, int(k),
                                                  int(probes), _metric(metric), farr, d_block, d_doc, d_rows, d_dist, d_counts))
        del keep

    def search_bit_iterative(self, queries, k, probes, metric="hamming", filters=None, mode="relaxed_order", max_probes=32768,
                             dim=None):
        """search_iterative for a bit index (vsr_ivf_search_bit_iterative): SearchResult and the lists each scan had taken."""
        q, qdim = _packed_bits(queries, self.corpus.dim if dim is None else dim, "search_bit_iterative")
        nq = q.shape[0]
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        scanned = np.zeros(nq, dtype=np.int32)
        check(self._lib.vsr_ivf_search_bit_iterative(self._h, _ptr(q), nq, qdim, int(k), int(probes), _metric(metric), farr,
                                                     _ivf_iterative_mode(mode), int(max_probes), _ptr(blk), _ptr(doc),
                                                     _ptr(row), _ptr(dist), _ptr(cnt), _ptr(scanned)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), scanned

    def search_bit_iterative_device(self, d_queries, nq, k, probes, metric, filters, mode, max_probes, d_block, d_doc, d_rows,
                                    d_dist, d_counts, d_probes=None, dim=None):
        """search_iterative_device for a bit index (vsr_ivf_search_bit_iterative_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_ivf_search_bit_iterative_device(self._h, d_queries, nq, self.corpus.dim if dim is None else dim,
                                                            int(k), int(probes), _metric(metric), farr,
                                                            _ivf_iterative_mode(mode), int(max_probes), d_block, d_doc, d_rows,
                                                            d_dist, d_counts, d_probes))
        del keep


class HnswIndex:
    """pgvector's hnsw scan (hnswscan.c) on the GPU: greedy descent, ef_search beam on layer 0, TIDs, filter, LIMIT."""

    def __init__(self, corpus, g, bit_metric=None, half=False, sparse=False):
        self.corpus, self._lib = corpus, corpus._lib
        if isinstance(g, C.c_void_p):                # a handle vsr_hnsw_build* returned (Corpus.build_hnsw, build_hnsw_bit)
            self._h = g
            return
        a = lambda name, dt: np.ascontiguousarray(g[name], dtype=dt)
        level, nbr0, tc, tids = a("level", np.int32), a("nbr0", np.int32), a("tid_count", np.int32), a("tids", np.int64)
        up_slot, up_nbr = a("up_slot", np.int32), a("up_nbr", np.int32)
        n_upper = int((up_slot >= 0).sum())
        h = C.c_void_p()
        if bit_metric is not None:                   # Corpus.load_hnsw_bit: the opclass travels with the graph
            check(self._lib.vsr_hnsw_load_bit(corpus._h, int(bit_metric), int(g["m"]), level.size, int(g["entry"]), _ptr(level),
                                              _ptr(nbr0), _ptr(tc), _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper,
                                              int(g["max_level"]), C.byref(h)))
        elif half:                                   # Corpus.load_hnsw_half
            check(self._lib.vsr_hnsw_load_half(corpus._h, int(g["m"]), level.size, int(g["entry"]), _ptr(level), _ptr(nbr0),
                                               _ptr(tc), _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper, int(g["max_level"]),
                                               C.byref(h)))
        elif sparse:                                 # Corpus.load_hnsw_sparse
            check(self._lib.vsr_hnsw_load_sparse(corpus._h, int(g["m"]), level.size, int(g["entry"]), _ptr(level), _ptr(nbr0),
                                                 _ptr(tc), _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper, int(g["max_level"]),
                                                 C.byref(h)))
        else:
            check(self._lib.vsr_hnsw_load(corpus._h, int(g["m"]), level.size, int(g["entry"]), _ptr(level), _ptr(nbr0), _ptr(tc),
                                          _ptr(tids), _ptr(up_slot), _ptr(up_nbr), n_upper, int(g["max_level"]), C.byref(h)))
        self._h = h

    def free(self):
        if getattr(self, "_h", None):
            self._lib.vsr_hnsw_free(self._h)
            self._h = None

    def __del__(self):
        try:
            if self.corpus._h and self.corpus.ctx._h:
                self.free()
        except Exception:
            pass

    def set_predicate_aware(self, on=True):
        """The layer-0 walk applies the query's filter itself (ACORN-1 style two-hop expansion) instead of leaving the
        filtering of the results to the caller's side (vsr_hnsw_set_predicate_aware)."""
        check(self._lib.vsr_hnsw_set_predicate_aware(self._h, 1 if on else 0))

    def info(self):
        """(elements, entry point, its level, highest level) of the graph."""
        v = [C.c_int32() for _ in range(4)]
        check(self._lib.vsr_hnsw_info(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def device_bytes(self):
        """Device memory of the graph arrays in bytes (vsr_hnsw_device_bytes); the corpus: Corpus.device_bytes."""
        return int(self._lib.vsr_hnsw_device_bytes(self._h))

    def export(self):
        """The graph as the dict Corpus.load_hnsw takes (vsr_hnsw_export): level, nbr0 [n_elem][2m], tid_count,
        tids [n_elem][10] (caller row indices), up_slot, up_nbr [n_upper][max_level][m], max_level, entry, m."""
        v = [C.c_int32() for _ in range(5)]
        check(self._lib.vsr_hnsw_export_shape(self._h, *[C.byref(x) for x in v]))
        m, ne, entry, n_upper, max_level = (int(x.value) for x in v)
        level = np.zeros(ne, dtype=np.int32)
        nbr0 = np.zeros((ne, 2 * m), dtype=np.int32)
        tid_count = np.zeros(ne, dtype=np.int32)
        tids = np.zeros((ne, 10), dtype=np.int64)
        up_slot = np.zeros(ne, dtype=np.int32)
        up_nbr = np.zeros((max(n_upper, 1), max_level, m), dtype=np.int32)
        check(self._lib.vsr_hnsw_export(self._h, _ptr(level), _ptr(nbr0), _ptr(tid_count), _ptr(tids), _ptr(up_slot),
                                        _ptr(up_nbr)))
        return {"level": level, "nbr0": nbr0, "tid_count": tid_count, "tids": tids, "up_slot": up_slot, "up_nbr": up_nbr,
                "max_level": max_level, "entry": entry, "m": m}

    def extended_over(self, corpus, ef_construction=64, metric=None, seed=1):
        """A new index over `corpus` -- this index's rows at their row indices plus new rows -- made by export() and
        Corpus.extend_hnsw: the graph is kept, only the new rows are inserted.  This index and its corpus stay as they are: free
        the old pair once the new one serves."""
        return corpus.extend_hnsw(self.export(), ef_construction, metric, seed)

    def vacuumed(self, dead_rows, ef_construction=64, metric=None):
        """(HnswIndex, stats): this index without `dead_rows`, repaired and compacted -- Corpus.vacuum_hnsw over export().  The
        rows stay in the corpus and this index stays as it is: free it once the new one serves.  To drop the rows from the
        corpus too: export() the result, formats.remap_hnsw_rows, reload the corpus without the dead rows, load_hnsw, free
        the old pair.  UPDATE is vacuum followed by extend_hnsw."""
        return self.corpus.vacuum_hnsw(self.export(), dead_rows, ef_construction, metric)

    def vacuum_spill_info(self):
        """(spilled_repairs, workspace_bytes) of the vacuum that made this index (vsr_hnsw_vacuum_spill_info): the repairs whose
        working set outgrew the LDS and ran in the global-memory form, and the bytes of the workspace pool they shared.
        (0, 0) for an index any other call made."""
        n, b = C.c_int32(), C.c_int64()
        check(self._lib.vsr_hnsw_vacuum_spill_info(self._h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def search_device(self, d_queries, nq, k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts,
                      d_visited=None):
        """Device pointers (ints); ONE launch on the corpus context's stream, no synchronisation (vsr_hnsw_search_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_device(self._h, d_queries, nq, self.corpus.dim, int(k), int(ef_search), _metric(metric),
                                               farr, d_block, d_doc, d_rows, d_dist, d_counts, d_visited))
        return keep

    def search(self, queries, k, ef_search=40, metric="l2", filters=None):
        """SearchResult plus, as a second value, the number of elements each query visited on layer 0."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = self.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        vis = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search(self._h, _ptr(q), nq, dim, int(k), int(ef_search), _metric(metric), farr, _ptr(blk),
                                        _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt), _ptr(vis)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), vis

    def search_iterative_device(self, d_queries, nq, k, ef_search, metric, filters, mode, max_scan_tuples, d_block, d_doc,
                                d_rows, d_dist, d_counts, d_tuples=None):
        """Device pointers (ints); launches on the corpus context's stream, no synchronisation
        (vsr_hnsw_search_iterative_device).  A query whose discarded set outgrew its buffer reports count -1."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_iterative_device(self._h, d_queries, nq, self.corpus.dim, int(k), int(ef_search),
                                                         _metric(metric), farr, _iterative_mode(mode), int(max_scan_tuples),
                                                         d_block, d_doc, d_rows, d_dist, d_counts, d_tuples))
        return keep

    def search_iterative(self, queries, k, ef_search=40, metric="l2", filters=None, mode="relaxed_order",
                         max_scan_tuples=20000):
        """pgvector's iterative index scan (hnsw.iterative_scan = mode, hnsw.max_scan_tuples): rounds of the layer-0 search
        resumed from the discarded candidates until k permitted rows are out.  SearchResult (rows in stream order) plus, as a
        second value, the tuples each query's scan counted (so->tuples) when it stopped."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        nq, dim = q.shape
        farr, keep = self.corpus._filter_array(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        tup = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search_iterative(self._h, _ptr(q), nq, dim, int(k), int(ef_search), _metric(metric), farr,
                                                  _iterative_mode(mode), int(max_scan_tuples), _ptr(blk), _ptr(doc), _ptr(row),
                                                  _ptr(dist), _ptr(cnt), _ptr(tup)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), tup

    # ---- a bit index (Corpus.load_hnsw_bit / build_hnsw_bit): queries are bit strings, the metric is the index's -------------
    def _results(self, nq, k):
        kk = max(int(k), 1)
        return (np.full((nq, kk), -1, dtype=np.int64), np.full((nq, kk), -1, dtype=np.int32), np.full((nq, kk), -1, dtype=np.int64),
                np.full((nq, kk), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.int32))

    def search_bit(self, queries, k, ef_search=40, metric="hamming", filters=None, dim=None):
        """HnswIndex.search over a bit index (vsr_hnsw_search_bit): `queries` bool [nq, dim] or packed uint8
        [nq, (dim + 7) // 8] (dim: the corpus's unless given), as Corpus.search_bit takes them; `metric` must be the index's.
        SearchResult (dist: the Hamming count or the Jaccard distance) plus the elements each query visited on layer 0."""
        q, qdim = _packed_bits(queries, self.corpus.dim if dim is None else dim, "search_bit")
        nq = q.shape[0]
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        vis = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search_bit(self._h, _ptr(q), nq, qdim, int(k), int(ef_search), _metric(metric), farr, _ptr(blk),
                                            _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt), _ptr(vis)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), vis

    def search_bit_device(self, d_queries, nq, k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts,
                          d_visited=None, dim=None):
        """Device pointers (ints): d_queries addresses nq x (dim + 7) // 8 packed bytes, any alignment; query staging and ONE
        search launch on the corpus context's stream, no synchronisation (vsr_hnsw_search_bit_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_bit_device(self._h, d_queries, nq, self.corpus.dim if dim is None else dim, int(k),
                                                   int(ef_search), _metric(metric), farr, d_block, d_doc, d_rows, d_dist, d_counts,
                                                   d_visited))
        return keep

    def search_bit_iterative(self, queries, k, ef_search=40, metric="hamming", filters=None, mode="relaxed_order",
                             max_scan_tuples=20000, dim=None):
        """search_iterative over a bit index (vsr_hnsw_search_bit_iterative): SearchResult in stream order plus the tuples
        each query's scan counted when it stopped."""
        q, qdim = _packed_bits(queries, self.corpus.dim if dim is None else dim, "search_bit_iterative")
        nq = q.shape[0]
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        tup = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search_bit_iterative(self._h, _ptr(q), nq, qdim, int(k), int(ef_search), _metric(metric), farr,
                                                      _iterative_mode(mode), int(max_scan_tuples), _ptr(blk), _ptr(doc), _ptr(row),
                                                      _ptr(dist), _ptr(cnt), _ptr(tup)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), tup

    # ---- a sparse index (Corpus.load_hnsw_sparse / build_hnsw_sparse): queries are CSR, the metric is given per call -----------
    def _csr_queries(self, queries, indices, values, dim, what):
        """The forms Corpus.search_sparse accepts: an object with .indptr / .indices / .data / .shape, or three arrays."""
        if indices is None and hasattr(queries, "indptr"):
            return _csr(queries, dim=dim, what=what)
        return _csr(queries, indices, values, self.corpus.dim if dim is None else dim, what)

    def search_sparse(self, queries, k, ef_search=40, metric="l2", filters=None, indices=None, values=None, dim=None):
        """HnswIndex.search over a sparse index (vsr_hnsw_search_sparse): `queries` as Corpus.search_sparse takes them (up to
        16000 non-zeros each), metric "l2", "ip", "cosine" (unit rows and unit queries) or "l1".  SearchResult plus the
        elements each query visited on layer 0."""
        ip, ix, vx, qdim = self._csr_queries(queries, indices, values, dim, "search_sparse")
        nq = ip.size - 1
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        vis = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search_sparse(self._h, _ptr(ip), _ptr(ix), _ptr(vx), nq, qdim, int(k), int(ef_search),
                                               _metric(metric), farr, _ptr(blk), _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt),
                                               _ptr(vis)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), vis

    def search_sparse_device(self, d_indptr, d_indices, d_values, nq, max_query_nnz, k, ef_search, metric, filters, d_block, d_doc,
                             d_rows, d_dist, d_counts, d_visited=None, dim=None):
        """Device pointers (ints): the queries' CSR arrays in device memory (int64, int32, float32) and the largest non-zero
        count of any of them (a longer query fails screening_check); query staging and ONE search launch on the corpus
        context's stream, no synchronisation (vsr_hnsw_search_sparse_device)."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_sparse_device(self._h, d_indptr, d_indices, d_values, nq,
                                                      self.corpus.dim if dim is None else dim, int(max_query_nnz), int(k),
                                                      int(ef_search), _metric(metric), farr, d_block, d_doc, d_rows, d_dist,
                                                      d_counts, d_visited))
        return keep

    def search_sparse_iterative(self, queries, k, ef_search=40, metric="l2", filters=None, mode="relaxed_order",
                                max_scan_tuples=20000, indices=None, values=None, dim=None):
        """search_iterative over a sparse index (vsr_hnsw_search_sparse_iterative): SearchResult in stream order plus the
        tuples each query's scan counted when it stopped."""
        ip, ix, vx, qdim = self._csr_queries(queries, indices, values, dim, "search_sparse_iterative")
        nq = ip.size - 1
        farr, keep = self.corpus._filter_array(filters, nq)
        blk, doc, row, dist, cnt = self._results(nq, k)
        tup = np.zeros(nq, dtype=np.int64)
        check(self._lib.vsr_hnsw_search_sparse_iterative(self._h, _ptr(ip), _ptr(ix), _ptr(vx), nq, qdim, int(k), int(ef_search),
                                                         _metric(metric), farr, _iterative_mode(mode), int(max_scan_tuples),
                                                         _ptr(blk), _ptr(doc), _ptr(row), _ptr(dist), _ptr(cnt), _ptr(tup)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), tup

    def search_sparse_iterative_device(self, d_indptr, d_indices, d_values, nq, max_query_nnz, k, ef_search, metric, filters, mode,
                                       max_scan_tuples, d_block, d_doc, d_rows, d_dist, d_counts, d_tuples=None, dim=None):
        """Device pointers (ints); no synchronisation (vsr_hnsw_search_sparse_iterative_device).  A query whose discarded set
        outgrew its buffer reports count -1."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_sparse_iterative_device(self._h, d_indptr, d_indices, d_values, nq,
                                                                self.corpus.dim if dim is None else dim, int(max_query_nnz),
                                                                int(k), int(ef_search), _metric(metric), farr,
                                                                _iterative_mode(mode), int(max_scan_tuples), d_block, d_doc,
                                                                d_rows, d_dist, d_counts, d_tuples))
        return keep

    def search_bit_iterative_device(self, d_queries, nq, k, ef_search, metric, filters, mode, max_scan_tuples, d_block, d_doc,
                                    d_rows, d_dist, d_counts, d_tuples=None, dim=None):
        """Device pointers (ints); no synchronisation (vsr_hnsw_search_bit_iterative_device).  A query whose discarded set
        outgrew its buffer reports count -1."""
        farr, keep = self.corpus._filter_array(filters, nq)
        check(self._lib.vsr_hnsw_search_bit_iterative_device(self._h, d_queries, nq, self.corpus.dim if dim is None else dim,
                                                             int(k), int(ef_search), _metric(metric), farr, _iterative_mode(mode),
                                                             int(max_scan_tuples), d_block, d_doc, d_rows, d_dist, d_counts,
                                                             d_tuples))
        return keep


def _task_table(tasks, nq):
    """(q_off int64 [nq + 1], q_graph int32 [q_off[nq]]) from one sequence of graph ids per query, or from a (q_off, q_graph) pair of
    numpy arrays passed through as it is (the library checks it)."""
    if isinstance(tasks, tuple) and len(tasks) == 2 and isinstance(tasks[0], np.ndarray):
        off = np.ascontiguousarray(tasks[0], dtype=np.int64).reshape(-1)
        if off.size != nq + 1:
            raise ValueError("q_off has one entry per query and one more")
        return off, np.ascontiguousarray(tasks[1], dtype=np.int32).reshape(-1)
    if len(tasks) != nq:
        raise ValueError("one sequence of graph ids per query")
    lists = [np.asarray(t, dtype=np.int32).reshape(-1) for t in tasks]
    off = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([t.size for t in lists], out=off[1:])
    flat = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)
    return off, np.ascontiguousarray(flat, dtype=np.int32)


class HnswForest:
    """Many HnswIndex over one corpus searched as a set (vsr_hnsw_forest_*): per query the graphs named in `tasks`, every
    (query, graph) pair a wave of ONE search launch, the per-graph results merged on the GPU by (distance, document_id, block_id),
    repeated rows dropped, the first k kept -- what HnswIndex.search on each graph plus a host merge gives.  `tasks`: one sequence
    of graph ids (positions in `indexes`) per query, or a (q_off, q_graph) pair of arrays.  The forest keeps the indexes alive;
    free() it before freeing them."""

    def __init__(self, indexes, corpus=None):
        self.indexes = list(indexes)
        self.corpus = corpus if corpus is not None else (self.indexes[0].corpus if self.indexes else None)
        self._lib = self.corpus._lib if self.corpus is not None else load_library()
        arr = (C.c_void_p * max(len(self.indexes), 1))(*[h._h for h in self.indexes])
        h = C.c_void_p()
        check(self._lib.vsr_hnsw_forest_open(arr if self.indexes else None, len(self.indexes), C.byref(h)))
        self._h = h

    def free(self):
        if getattr(self, "_h", None):
            self._lib.vsr_hnsw_forest_free(self._h)
            self._h = None

    def __del__(self):
        try:
            if self.corpus is None or (self.corpus._h and self.corpus.ctx._h):
                self.free()
        except Exception:
            pass

    def set_predicate_aware(self, on=True):
        """HnswIndex.set_predicate_aware for the searches of this forest (the indexes' own flags are not read)."""
        check(self._lib.vsr_hnsw_forest_set_predicate_aware(self._h, 1 if on else 0))

    def _filters(self, filters, nq):
        return self.corpus._filter_array(filters, nq) if self.corpus is not None else (None, None)

    def _host(self, fn, q, qdim, k, ef_search, metric, tasks, filters):
        nq = q.shape[0]
        off, graph = _task_table(tasks, nq)
        farr, keep = self._filters(filters, nq)
        kk = max(int(k), 1)
        blk = np.full((nq, kk), -1, dtype=np.int64)
        doc = np.full((nq, kk), -1, dtype=np.int32)
        row = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.int32)
        vis = np.zeros(max(int(off[-1]), 0), dtype=np.int64)
        check(fn(self._h, _ptr(q), nq, qdim, int(k), int(ef_search), _metric(metric), _ptr(off), _ptr(graph), farr, _ptr(blk), _ptr(doc),
                 _ptr(row), _ptr(dist), _ptr(cnt), _ptr(vis)))
        del keep
        return SearchResult(blk, doc, row, dist, cnt), vis

    def search(self, queries, tasks, k, ef_search=40, metric="l2", filters=None):
        """SearchResult plus the elements every TASK visited on layer 0, [q_off[nq]] (vsr_hnsw_forest_search)."""
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(queries, dtype=np.float32)))
        return self._host(self._lib.vsr_hnsw_forest_search, q, q.shape[1], k, ef_search, metric, tasks, filters)

    def search_bit(self, queries, tasks, k, ef_search=40, metric="hamming", filters=None, dim=None):
        """search over a forest of bit indexes (vsr_hnsw_forest_search_bit): `queries` as HnswIndex.search_bit takes them."""
        cdim = self.corpus.dim if self.corpus is not None else None
        q, qdim = _packed_bits(queries, cdim if dim is None else dim, "search_bit")
        return self._host(self._lib.vsr_hnsw_forest_search_bit, q, qdim, k, ef_search, metric, tasks, filters)

    def _device(self, fn, d_queries, nq, dim, tasks, k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_visited):
        off, graph = _task_table(tasks, nq)
        farr, keep = self._filters(filters, nq)
        check(fn(self._h, d_queries, nq, dim, int(k), int(ef_search), _metric(metric), _ptr(off), _ptr(graph), farr, d_block, d_doc,
                 d_rows, d_dist, d_counts, d_visited))
        return keep

    def search_device(self, d_queries, nq, tasks, k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts,
                      d_visited=None):
        """Device pointers (ints) for the queries and the outputs, `tasks` and `filters` on the host; one search launch and one
        merge launch on the corpus context's stream, no synchronisation (vsr_hnsw_forest_search_device).  A query that owns a task
        whose visited table overflowed reports count -1."""
        return self._device(self._lib.vsr_hnsw_forest_search_device, d_queries, nq, self.corpus.dim if self.corpus is not None else 0, tasks,
                            k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_visited)

    def search_bit_device(self, d_queries, nq, tasks, k, ef_search, metric, filters, d_block, d_doc, d_rows, d_dist, d_counts,
                          d_visited=None, dim=None):
        """search_device over a forest of bit indexes: d_queries addresses nq x (dim + 7) // 8 packed bytes; one staging launch over
        the queries in front of the two (vsr_hnsw_forest_search_bit_device)."""
        cdim = self.corpus.dim if self.corpus is not None else 0
        return self._device(self._lib.vsr_hnsw_forest_search_bit_device, d_queries, nq, cdim if dim is None else dim, tasks, k, ef_search,
                            metric, filters, d_block, d_doc, d_rows, d_dist, d_counts, d_visited)
