"""numpy restatement of pgvector's bit distances and of the library's filtered top-k over them (the expected answer of
tests/test_gpu_bitvec.py; pinned against pgvector's own known answers by tests/test_bit_formats.py).

  hamming_distance  popcount(a ^ b)                                                      (bitutils.c:34-61)
  jaccard_distance  ab == 0 ? 1 : 1 - ab / (double) (aa + bb - ab), ab = |a & b| ...     (bitutils.c:96-129)
  binary_quantize   bit = x > 0                                                          (vector.c:941-968)

Bit strings are packed uint8 rows in varbit order (np.packbits: element i -> bit 7 - i % 8 of byte i // 8); bits past `dim`
never count, whatever they hold."""
import numpy as np


def pack(bits):
    """bool [n, dim] -> packed uint8 [n, (dim + 7) // 8], pad bits zero."""
    bits = np.atleast_2d(np.asarray(bits, dtype=np.bool_))
    if bits.shape[1] == 0:
        return np.zeros((bits.shape[0], 0), dtype=np.uint8)
    return np.packbits(bits, axis=1)


def unpack(packed, dim):
    """packed uint8 [n, (dim + 7) // 8] -> bool [n, dim]; the pad bits are dropped."""
    packed = np.atleast_2d(np.asarray(packed, dtype=np.uint8))
    if dim == 0:
        return np.zeros((packed.shape[0], 0), dtype=np.bool_)
    return np.unpackbits(packed, axis=1)[:, :dim].astype(np.bool_)


def set_pad_bits(packed, dim):
    """The same strings with every bit past `dim` set to 1."""
    out = np.array(packed, dtype=np.uint8, copy=True)
    if dim % 8:
        out[:, -1] |= np.uint8(0xFF >> (dim % 8))
    return out


class BitModel:
    """A corpus of packed rows with its identity: distances to many queries at once and the library's order."""

    def __init__(self, rows, dim, doc=None, blk=None):
        n = np.asarray(rows).shape[0]
        self.dim = dim
        self.doc = np.zeros(n, dtype=np.int32) if doc is None else np.asarray(doc)
        self.blk = np.arange(n, dtype=np.int64) if blk is None else np.asarray(blk)
        self.bits = unpack(rows, dim).astype(np.float32)                  # 0 / 1: products and sums below are exact integers
        self.pop = self.bits.sum(axis=1, dtype=np.float64)                # popcount of every row
        self.by_id = np.lexsort((self.blk, self.doc))                     # the tie order, computed once

    def distances(self, metric, queries):
        """float64 operator values [nq, n] of the packed queries against every row."""
        q = unpack(queries, self.dim).astype(np.float32)
        ab = (q @ self.bits.T).astype(np.float64)                         # |a & b|: integers < 2^24, exact in fp32
        bb = q.sum(axis=1, dtype=np.float64)[:, None]
        aa = self.pop[None, :]
        if metric == "hamming":
            return aa + bb - 2.0 * ab                                     # popcount(a ^ b)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = 1.0 - ab / (aa + bb - ab)
        return np.where(ab == 0, 1.0, d)

    def topk(self, dist_row, k, mask=None):
        """(caller row indices, float32 distances) of the k nearest permitted rows by ((float) distance, document_id,
        block_id): np.lexsort((blk, doc, dist32)), as a stable sort by distance of the rows in id order."""
        dist32 = np.asarray(dist_row).astype(np.float32)
        ids = self.by_id if mask is None else self.by_id[np.asarray(mask, dtype=bool)[self.by_id]]
        order = ids[np.argsort(dist32[ids], kind="stable")][:k]
        return order, dist32[order]


def distances(metric, rows, q, dim):
    """float64 operator values of every packed row against the packed query `q`."""
    return BitModel(rows, dim).distances(metric, q)[0]


def topk(metric, rows, q, dim, k, doc=None, blk=None, mask=None):
    """(caller row indices, float32 distances) of the k nearest permitted rows, ordered by ((float) distance, document_id,
    block_id) -- vsr_search_bit's contract."""
    m = BitModel(rows, dim, doc, blk)
    return m.topk(m.distances(metric, q)[0], k, mask)


def binary_quantize(x):
    """packed uint8 [n, (dim + 7) // 8]: bit set where the element > 0 (NaN, -0.0 and 0 give 0)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        return pack(x > 0)


def user_row_mask(user, user_roles, permissions, doc):
    """rows visible to `user`: some role of the user is permitted the row's document."""
    roles = {r for u, r in user_roles if u == user}
    docs = np.asarray(sorted({d for r, d in permissions if r in roles}), dtype=np.int64)
    return np.isin(np.asarray(doc), docs)
