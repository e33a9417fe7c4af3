"""Data formats on either side of the search path: what the reference's callers hold when they reach
`vsr_corpus_load` / `vsr_search`.  Host-side only; nothing here touches the GPU.

  * pgvector text form   `[a,b,...]`   vector_in / vector_out   (pgvector/src/vector.c:165-270, 278-315)
  * pgvector binary form  int16 dim, int16 unused (= 0), float4[dim] big-endian   vector_recv / vector_send  (:363-411)
  * the same two forms of halfvec (pgvector/src/halfvec.c:165-320 text, :356-404 binary: big-endian uint16 binary16 elements);
    arrays are np.float16, what Context.load_corpus_half takes
  * PostgreSQL's bit / varbit, the operand type of pgvector's <~> and <%> (bitvec.c): '0' / '1' digit text; binary form int32
    bit length, big-endian, then the packed bytes.  Values are bool arrays, what Context.load_corpus_bit packs
  * pgvector's sparsevec (sparsevec.c:187-565): text `{i:v,...}/dim` with one-based indices; binary int32 dim, nnz, unused,
    then the zero-based indices and the float4 values.  Values are (indices, values, dim) rows of a CSR corpus
  * shared_vectors.bin (+ .meta) of the C++ benches   SharedVectorTable::save_vectors / load_vectors
    (logical_partition_benchmark/benchmark/src/shared_vector_table.cpp:169-201): int32 dim, int64 count, float32[count*dim];
    .meta = int32 dim, int64 count, (int32 document_id, int32 block_id)[count]

Errors are ValueError with pgvector's message texts (the shim maps them to ereport).
"""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

VECTOR_MAX_DIM = 16000                                    # vector.h:4
_SPACE = " \t\n\r\v\f"                                    # vector_isspace, vector.c:144-158

_libc = ctypes.CDLL(ctypes.util.find_library("c") or None, use_errno=True)
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
_ERANGE = 34


def _check_element(v, kind="vector"):
    if math.isnan(v):
        raise ValueError(f"NaN not allowed in {kind}")                        # vector.c:101-113, halfvec.c:101-113
    if math.isinf(v):
        raise ValueError(f"infinite value not allowed in {kind}")


def _check_dim(dim, kind="vector"):
    if dim < 1:
        raise ValueError(f"{kind} must have at least 1 dimension")            # vector.c:85-96, halfvec.c:84-96
    if dim > VECTOR_MAX_DIM:
        raise ValueError(f"{kind} cannot have more than {VECTOR_MAX_DIM} dimensions")


def _check_expected(expected_dim, dim):
    if expected_dim is not None and expected_dim != -1 and dim != expected_dim:
        raise ValueError(f"expected {expected_dim} dimensions, not {dim}")    # CheckExpectedDim, vector.c:72-80


def vector_from_text(lit, expected_dim=None):
    """vector_in: same grammar, same number parser (libc strtof: no double rounding), same error texts."""
    return np.asarray(_elements_from_text(lit, expected_dim, "vector"), dtype=np.float32)


def _elements_from_text(lit, expected_dim, kind):
    """The grammar vector_in and halfvec_in share (vector.c:165-270, halfvec.c:165-271); kind: the type named in the errors.
    halfvec: every element is the fp32 value of the binary16 it rounds to (Float4ToHalfUnchecked)."""
    if isinstance(lit, bytes):
        lit = lit.decode()
    raw = lit.encode()
    bad = f'invalid input syntax for type {kind}: "{lit}"'
    n = len(raw)
    pos = 0

    def skip(p):
        while p < n and chr(raw[p]) in _SPACE:
            p += 1
        return p

    pos = skip(pos)
    if pos >= n or raw[pos:pos + 1] != b"[":
        raise ValueError(bad + '\nDETAIL:  Vector contents must start with "[".')
    pos = skip(pos + 1)
    if raw[pos:pos + 1] == b"]":
        raise ValueError(f"{kind} must have at least 1 dimension")
    out = []
    buf = ctypes.create_string_buffer(raw + b"\0")
    base = ctypes.addressof(buf)
    while True:
        if len(out) == VECTOR_MAX_DIM:
            raise ValueError(f"{kind} cannot have more than {VECTOR_MAX_DIM} dimensions")
        pos = skip(pos)
        if pos >= n:
            raise ValueError(bad)
        end = ctypes.c_char_p()
        ctypes.set_errno(0)
        val = _libc.strtof(ctypes.c_char_p(base + pos), ctypes.byref(end))
        stop = ctypes.cast(end, ctypes.c_void_p).value - base
        if stop == pos:
            raise ValueError(bad)
        range_error = ctypes.get_errno() == _ERANGE and math.isinf(val)
        if kind == "halfvec":
            with np.errstate(over="ignore"):
                h = float(np.float32(val).astype(np.float16))     # round to nearest even, |v| >= 65520 -> +-Inf
            range_error = range_error or (math.isinf(h) and not math.isinf(val))
            val = h
        if range_error:
            raise ValueError(f'"{raw[pos:stop].decode()}" is out of range for type {kind}')
        _check_element(val, kind)
        out.append(val)
        pos = skip(stop)
        c = raw[pos:pos + 1]
        if c == b",":
            pos += 1
        elif c == b"]":
            pos += 1
            break
        else:
            raise ValueError(bad)
    pos = skip(pos)
    if pos != n:
        raise ValueError(bad + "\nDETAIL:  Junk after closing right brace.")
    _check_dim(len(out), kind)
    _check_expected(expected_dim, len(out))
    return out


def _float4_shortest(v):
    """float_to_shortest_decimal_bufn for float4 (PostgreSQL's Ryu f2s): shortest round-trip digits, fixed notation for
    decimal exponents in [-4, 6), else d.ddde+XX with at least two exponent digits."""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    sign = "-" if np.signbit(v) else ""
    a = abs(v)
    if a == 0:
        return sign + "0"
    sci = np.format_float_scientific(a, unique=True, trim="-", exp_digits=1)   # e.g. '1.5e+38', '1.e+00' -> trimmed
    mant, exp = sci.split("e")
    exp = int(exp)
    digits = mant.replace(".", "")
    if -4 <= exp < 6:
        if exp >= 0:
            whole = digits[:exp + 1].ljust(exp + 1, "0")
            frac = digits[exp + 1:]
        else:
            whole = "0"
            frac = "0" * (-exp - 1) + digits
        return sign + whole + ("." + frac if frac else "")
    body = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
    return f"{sign}{body}e{'+' if exp >= 0 else '-'}{abs(exp):02d}"


def vector_to_text(v):
    """vector_out."""
    v = np.asarray(v, dtype=np.float32).ravel()
    return "[" + ",".join(_float4_shortest(x) for x in v) + "]"


def vector_from_binary(b, expected_dim=None):
    """vector_recv."""
    if len(b) < 4:
        raise ValueError("insufficient data left in message")
    dim, unused = struct.unpack(">hh", b[:4])
    _check_dim(dim)
    _check_expected(expected_dim, dim)
    if unused != 0:
        raise ValueError(f"expected unused to be 0, not {unused}")
    if len(b) != 4 + 4 * dim:
        raise ValueError("insufficient data left in message" if len(b) < 4 + 4 * dim else "incorrect binary data format")
    x = np.frombuffer(b, dtype=">f4", count=dim, offset=4).astype(np.float32)
    for e in x:
        _check_element(float(e))
    return x


def vector_to_binary(v):
    """vector_send."""
    v = np.asarray(v, dtype=np.float32).ravel()
    _check_dim(v.size)
    return struct.pack(">hh", v.size, 0) + v.astype(">f4").tobytes()


def _check_halfvec_typmod(expected_dim):
    if expected_dim is None or expected_dim == -1:
        return
    if expected_dim < 1:
        raise ValueError("dimensions for type halfvec must be at least 1")    # halfvec_typmod_in, halfvec.c:325-351
    if expected_dim > VECTOR_MAX_DIM:                                         # (HALFVEC_MAX_DIM is 16000 too, halfvec.h)
        raise ValueError(f"dimensions for type halfvec cannot exceed {VECTOR_MAX_DIM}")


def halfvec_from_text(lit, expected_dim=None):
    """halfvec_in (halfvec.c:165-271): vector_in's grammar; every element rounded to binary16 (round to nearest even), one
    that overflows is `"<text>" is out of range for type halfvec`.  Returns np.float16."""
    _check_halfvec_typmod(expected_dim)
    return np.asarray(_elements_from_text(lit, expected_dim, "halfvec"), dtype=np.float16)


def halfvec_to_text(v):
    """halfvec_out (halfvec.c:279-320): the shortest float4 decimal of every widened element."""
    v = np.asarray(v, dtype=np.float16).ravel()
    return "[" + ",".join(_float4_shortest(np.float32(x)) for x in v) + "]"


def halfvec_from_binary(b, expected_dim=None):
    """halfvec_recv (halfvec.c:356-385): int16 dim, int16 unused (= 0), dim big-endian uint16 binary16 bit patterns."""
    _check_halfvec_typmod(expected_dim)
    if len(b) < 4:
        raise ValueError("insufficient data left in message")
    dim, unused = struct.unpack(">hh", b[:4])
    _check_dim(dim, "halfvec")
    _check_expected(expected_dim, dim)
    if unused != 0:
        raise ValueError(f"expected unused to be 0, not {unused}")
    if len(b) != 4 + 2 * dim:
        raise ValueError("insufficient data left in message" if len(b) < 4 + 2 * dim else "incorrect binary data format")
    x = np.frombuffer(b, dtype=">u2", count=dim, offset=4).astype(np.uint16).view(np.float16)
    for e in x:
        _check_element(float(e), "halfvec")
    return x


def halfvec_to_binary(v):
    """halfvec_send (halfvec.c:390-404)."""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float16).ravel())
    _check_dim(v.size, "halfvec")
    return struct.pack(">hh", v.size, 0) + v.view(np.uint16).astype(">u2").tobytes()


# ---- PostgreSQL's bit / varbit, the type pgvector's <~> and <%> take (bitvec.c).  A value here is a bool array: element i is
# bit i of the string; on the wire and in a corpus it is bit 7 - i % 8 of byte i // 8, pad bits zero (np.packbits' order).
def bit_from_text(lit):
    """bit_in / varbit_in for binary digits: '0' / '1' characters with an optional B (or b) prefix, any length including 0.
    (The hexadecimal X form is not taken.)  Returns a bool array."""
    s = lit[1:] if lit[:1] in ("B", "b") else lit
    for ch in s:
        if ch not in "01":
            raise ValueError(f'"{ch}" is not a valid binary digit')
    return np.frombuffer(s.encode("ascii"), dtype=np.uint8) == ord("1")


def bit_to_text(v):
    """bit_out / varbit_out: one '0' / '1' digit per element, no prefix."""
    return "".join("1" if x else "0" for x in np.asarray(v, dtype=np.bool_).ravel())


def bit_from_binary(b):
    """varbit_recv: int32 bit length, big-endian, then (length + 7) // 8 bytes; pad bits in the last byte are dropped, as
    varbit_recv clears them.  Returns a bool array."""
    if len(b) < 4:
        raise ValueError("insufficient data left in message")
    (bitlen,) = struct.unpack(">i", b[:4])
    if bitlen < 0:
        raise ValueError("invalid length in external bit string")
    nbytes = (bitlen + 7) // 8
    if len(b) != 4 + nbytes:
        raise ValueError("insufficient data left in message" if len(b) < 4 + nbytes else "incorrect binary data format")
    bits = np.unpackbits(np.frombuffer(b, dtype=np.uint8, count=nbytes, offset=4))
    return bits[:bitlen].astype(np.bool_)


def bit_to_binary(v):
    """varbit_send: int32 bit length, big-endian, then the packed bytes with zero pad bits."""
    v = np.asarray(v, dtype=np.bool_).ravel()
    return struct.pack(">i", v.size) + np.packbits(v).tobytes()


# ---- pgvector's sparsevec (sparsevec.c).  A value here is (indices int32 zero-based ascending, values float32, dim): one row of
# the CSR arrays Context.load_corpus_sparse takes.  Text is `{i:v,...}/dim` with ONE-based indices; the binary form is
# sparsevec_send's: int32 dim, int32 nnz, int32 unused (= 0), nnz int32 zero-based indices, nnz float4, all big-endian.
SPARSEVEC_MAX_DIM = 1000000000                            # sparsevec.h
SPARSEVEC_MAX_NNZ = 16000
_INT_MAX, _INT_MIN = 2147483647, -2147483648


def _check_sparsevec_dim(dim):
    if dim < 1:
        raise ValueError("sparsevec must have at least 1 dimension")          # CheckDim, sparsevec.c:53-65
    if dim > SPARSEVEC_MAX_DIM:
        raise ValueError(f"sparsevec cannot have more than {SPARSEVEC_MAX_DIM} dimensions")


def _check_sparsevec_typmod(expected_dim):
    if expected_dim is None or expected_dim == -1:
        return
    if expected_dim < 1:
        raise ValueError("dimensions for type sparsevec must be at least 1")  # sparsevec_typmod_in, sparsevec.c:461-487
    if expected_dim > SPARSEVEC_MAX_DIM:
        raise ValueError(f"dimensions for type sparsevec cannot exceed {SPARSEVEC_MAX_DIM}")


def _check_sparsevec_indices(indices, dim):
    for i, index in enumerate(indices):                                       # CheckIndex, sparsevec.c:92-116
        if index < 0 or index >= dim:
            raise ValueError("sparsevec index out of bounds")
        if i > 0 and index < indices[i - 1]:
            raise ValueError("sparsevec indices must be in ascending order")
        if i > 0 and index == indices[i - 1]:
            raise ValueError("sparsevec indices must not contain duplicates")


def _strtol(raw, pos):
    """strtol(base 10) at raw[pos:]: (value, end), end == pos when no digits were read."""
    p, n = pos, len(raw)
    while p < n and chr(raw[p]) in _SPACE:
        p += 1
    q = p + 1 if raw[p:p + 1] in (b"+", b"-") else p
    e = q
    while e < n and 48 <= raw[e] <= 57:
        e += 1
    if e == q:
        return 0, pos
    return int(raw[p:e]), e


def sparsevec_from_text(lit, expected_dim=None):
    """sparsevec_in (sparsevec.c:187-389): same grammar, same number parsers, same error texts; zero values are dropped, the
    entries sorted by index.  Returns (indices int32 zero-based, values float32, dim)."""
    _check_sparsevec_typmod(expected_dim)
    if isinstance(lit, bytes):
        lit = lit.decode()
    raw = lit.encode()
    bad = f'invalid input syntax for type sparsevec: "{lit}"'
    n = len(raw)
    if raw.count(b",") + 1 > SPARSEVEC_MAX_NNZ:
        raise ValueError(f"sparsevec cannot have more than {SPARSEVEC_MAX_NNZ} non-zero elements")

    def skip(p):
        while p < n and chr(raw[p]) in _SPACE:
            p += 1
        return p

    pos = skip(0)
    if raw[pos:pos + 1] != b"{":
        raise ValueError(bad + '\nDETAIL:  Vector contents must start with "{".')
    pos = skip(pos + 1)
    elements = []
    if raw[pos:pos + 1] == b"}":
        pos += 1
    else:
        buf = ctypes.create_string_buffer(raw + b"\0")
        base = ctypes.addressof(buf)
        while True:
            pos = skip(pos)
            if pos >= n:
                raise ValueError(bad)
            index, stop = _strtol(raw, pos)
            if stop == pos:
                raise ValueError(bad)
            index = min(max(index, _INT_MIN + 1), _INT_MAX)               # "keep in int range for correct error message later"
            pos = skip(stop)
            if raw[pos:pos + 1] != b":":
                raise ValueError(bad)
            pos = skip(pos + 1)
            end = ctypes.c_char_p()
            ctypes.set_errno(0)
            val = _libc.strtof(ctypes.c_char_p(base + pos), ctypes.byref(end))
            stop = ctypes.cast(end, ctypes.c_void_p).value - base
            if stop == pos:
                raise ValueError(bad)
            if ctypes.get_errno() == _ERANGE and (val == 0 or math.isinf(val)):
                raise ValueError(f'"{raw[pos:stop].decode()}" is out of range for type sparsevec')
            _check_element(val, "sparsevec")
            if val != 0:                                                      # zero values are not stored
                elements.append((index - 1, val))                             # 1-based (SQL) -> 0-based
            pos = skip(stop)
            c = raw[pos:pos + 1]
            if c == b",":
                pos += 1
            elif c == b"}":
                pos += 1
                break
            else:
                raise ValueError(bad)
    pos = skip(pos)
    if raw[pos:pos + 1] != b"/":
        raise ValueError(bad + "\nDETAIL:  Unexpected end of input.")
    pos = skip(pos + 1)
    dim, stop = _strtol(raw, pos)
    if stop == pos:
        raise ValueError(bad)
    dim = min(max(dim, _INT_MIN), _INT_MAX)
    pos = skip(stop)
    if pos != n:
        raise ValueError(bad + "\nDETAIL:  Junk after closing.")
    _check_sparsevec_dim(dim)
    _check_expected(expected_dim, dim)
    elements.sort(key=lambda e: e[0])
    _check_sparsevec_indices([e[0] for e in elements], dim)
    return (np.asarray([e[0] for e in elements], dtype=np.int32), np.asarray([e[1] for e in elements], dtype=np.float32), dim)


def sparsevec_to_text(indices, values, dim):
    """sparsevec_out (sparsevec.c:408-456): one-based indices, the shortest float4 decimal of every value."""
    indices = np.asarray(indices, dtype=np.int64).ravel()
    values = np.asarray(values, dtype=np.float32).ravel()
    return "{" + ",".join(f"{int(i) + 1}:{_float4_shortest(v)}" for i, v in zip(indices, values)) + "}/" + str(int(dim))


def sparsevec_from_binary(b, expected_dim=None):
    """sparsevec_recv (sparsevec.c:492-539).  Returns (indices int32 zero-based, values float32, dim)."""
    _check_sparsevec_typmod(expected_dim)
    if len(b) < 12:
        raise ValueError("insufficient data left in message")
    dim, nnz, unused = struct.unpack(">iii", b[:12])
    _check_sparsevec_dim(dim)
    if nnz < 0:                                                               # CheckNnz, sparsevec.c:70-87
        raise ValueError("sparsevec cannot have negative number of elements")
    if nnz > SPARSEVEC_MAX_NNZ:
        raise ValueError(f"sparsevec cannot have more than {SPARSEVEC_MAX_NNZ} non-zero elements")
    if nnz > dim:
        raise ValueError("sparsevec cannot have more elements than dimensions")
    _check_expected(expected_dim, dim)
    if unused != 0:
        raise ValueError(f"expected unused to be 0, not {unused}")
    if len(b) < 12 + 4 * nnz:
        raise ValueError("insufficient data left in message")
    indices = np.frombuffer(b, dtype=">i4", count=nnz, offset=12).astype(np.int32)
    _check_sparsevec_indices([int(i) for i in indices], dim)
    if len(b) != 12 + 8 * nnz:
        raise ValueError("insufficient data left in message" if len(b) < 12 + 8 * nnz else "incorrect binary data format")
    values = np.frombuffer(b, dtype=">f4", count=nnz, offset=12 + 4 * nnz).astype(np.float32)
    for v in values:
        _check_element(float(v), "sparsevec")
        if v == 0:
            raise ValueError("binary representation of sparsevec cannot contain zero values")
    return indices, values, dim


def sparsevec_to_binary(indices, values, dim):
    """sparsevec_send (sparsevec.c:544-565)."""
    indices = np.asarray(indices, dtype=np.int32).ravel()
    values = np.asarray(values, dtype=np.float32).ravel()
    if indices.size != values.size:
        raise ValueError("sparsevec: one value per index")
    return struct.pack(">iii", int(dim), indices.size, 0) + indices.astype(">i4").tobytes() + values.astype(">f4").tobytes()


def write_shared_vectors(path, rows, doc_ids, block_ids):
    """SharedVectorTable::save_vectors (shared_vector_table.cpp:169-201); used to make test inputs."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<iq", dim, n))
        f.write(rows.tobytes())
    ids = np.empty((n, 2), dtype="<i4")
    ids[:, 0] = doc_ids
    ids[:, 1] = block_ids
    with open(path + ".meta", "wb") as f:
        f.write(struct.pack("<iq", dim, n))
        f.write(ids.tobytes())


def read_shared_vectors(path, mmap=True):
    """SharedVectorTable::load_vectors: (rows float32 [n, dim], document_ids int32 [n], block_ids int32 [n]).
    Rows are memory-mapped by default (a 10M x 128 table is 5 GB); `vsr_corpus_load` copies them once."""
    with open(path, "rb") as f:
        head = f.read(12)
    if len(head) != 12:
        raise ValueError(f"Malformed shared vector file: {path}")
    dim, n = struct.unpack("<iq", head)
    if dim < 1 or n < 0:
        raise ValueError(f"Malformed shared vector file: {path}")
    if mmap and n:
        rows = np.memmap(path, dtype="<f4", mode="r", offset=12, shape=(n, dim))
    else:
        rows = np.fromfile(path, dtype="<f4", offset=12, count=n * dim).reshape(n, dim)
    if rows.shape != (n, dim):
        raise ValueError(f"Malformed shared vector file: {path}")
    with open(path + ".meta", "rb") as f:
        mdim, mn = struct.unpack("<iq", f.read(12))
        if (mdim, mn) != (dim, n):
            raise ValueError(f"Metadata mismatch for {path}")
        ids = np.frombuffer(f.read(8 * n), dtype="<i4")
    if ids.size != 2 * n:
        raise ValueError(f"Malformed shared vector metadata: {path}.meta")
    ids = ids.reshape(n, 2)
    return rows, np.ascontiguousarray(ids[:, 0]), np.ascontiguousarray(ids[:, 1])


# ---- an HNSW graph on disk: the dict Corpus.load_hnsw takes and HnswIndex.export returns, as one .npz ----
_HNSW_ARRAYS = (("level", np.int32), ("nbr0", np.int32), ("tid_count", np.int32), ("tids", np.int64), ("up_slot", np.int32),
                ("up_nbr", np.int32))
_HNSW_SCALARS = ("max_level", "entry", "m")


def save_hnsw(path, graph):
    """Write an exported graph (HnswIndex.export, or any dict Corpus.load_hnsw takes) to `path` as one uncompressed .npz."""
    fields = {name: np.ascontiguousarray(graph[name], dtype=dt) for name, dt in _HNSW_ARRAYS}
    fields.update({name: np.asarray(int(graph[name]), dtype=np.int64) for name in _HNSW_SCALARS})
    with open(path, "wb") as f:                         # (a file object: np.savez appends ".npz" to a bare name)
        np.savez(f, **fields)


def load_hnsw(path):
    """The dict save_hnsw wrote: arrays with their dtypes and shapes, max_level / entry / m as ints."""
    with np.load(path, allow_pickle=False) as z:
        missing = [name for name, _ in _HNSW_ARRAYS if name not in z.files] + [name for name in _HNSW_SCALARS if name not in z.files]
        if missing:
            raise ValueError(f"{path}: not an HNSW graph file (missing {', '.join(missing)})")
        graph = {name: np.ascontiguousarray(z[name], dtype=dt) for name, dt in _HNSW_ARRAYS}
        graph.update({name: int(z[name]) for name in _HNSW_SCALARS})
    return graph


def remap_hnsw_rows(graph, new_index_of_old_row):
    """Move an exported graph onto a corpus whose rows were renumbered: every heap TID t becomes new_index_of_old_row[t].
    The step between Corpus.vacuum_hnsw and a corpus loaded without the dead rows: vacuum, export() the result,
    remap_hnsw_rows(export, new_index_of_old_row), reload the corpus, Corpus.load_hnsw(remapped), free the old pair.
    new_index_of_old_row: an integer array over the OLD corpus's rows, -1 for a row that is gone.  A TID that names such a
    row, or a row outside the array, is a ValueError: the graph was not vacuumed of it.  Returns a new dict; the -1 padding of
    `tids` past tid_count stays."""
    new_of = np.asarray(new_index_of_old_row, dtype=np.int64).ravel()
    tids = np.array(graph["tids"], dtype=np.int64, copy=True)
    tc = np.asarray(graph["tid_count"], dtype=np.int64)
    if tids.ndim != 2 or tids.shape[0] != tc.size:
        raise ValueError("remap_hnsw_rows: tids must be [n_elem][10] beside tid_count [n_elem]")
    used = np.arange(tids.shape[1])[None, :] < tc[:, None]
    old = tids[used]
    if old.size and (old.min() < 0 or old.max() >= new_of.size):
        raise ValueError("remap_hnsw_rows: a heap TID names a row outside new_index_of_old_row")
    new = new_of[old]
    if new.size and new.min() < 0:
        bad = int(old[np.argmin(new)])
        raise ValueError(f"remap_hnsw_rows: row {bad} is named by a heap TID but has no new index (vacuum it first)")
    tids[used] = new
    tids[~used] = -1
    out = dict(graph)
    out["tids"] = tids
    return out
