"""numpy model of the two-stage search (vsr_search_quantized, include/vsrbac.h): a Hamming shortlist on the quantized rows,
then the exact operator distance on the source rows of the shortlist.

  stage 1   qb = binary_quantize(q) from the fp32 query as given; S = the `shortlist` nearest permitted rows by
            (Hamming, document_id, block_id)                                   -- tests/bit_model.py
  stage 2   the oracle's exact filtered top-k with S as the mask, in the library's order: (fp32 distance, NaN last,
            document_id, block_id); a halfvec source sees the query rounded to binary16

Everything is in caller row indices, like the oracle."""
import numpy as np

import bit_model


def round_half(q):
    """The query `$1::halfvec` holds, widened."""
    with np.errstate(over="ignore"):
        return np.asarray(q, dtype=np.float32).astype(np.float16).astype(np.float32)


class QuantizedModel:
    def __init__(self, oracle, x, doc=None, blk=None, half=False):
        """x: the source rows as fp32 [n, dim] (a halfvec source: its binary16 rows widened)."""
        self.orc = oracle
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        n, self.dim = self.x.shape
        self.doc = np.zeros(n, dtype=np.int32) if doc is None else np.asarray(doc, dtype=np.int32)
        self.blk = np.arange(n, dtype=np.int64) if blk is None else np.asarray(blk, dtype=np.int64)
        self.half = half
        self.bits = bit_model.BitModel(bit_model.binary_quantize(self.x), self.dim, self.doc, self.blk)

    def hamming(self, queries):
        """[nq, n] Hamming distances of binary_quantize(queries) to every quantized row."""
        return self.bits.distances("hamming", bit_model.binary_quantize(queries))

    def shortlist(self, ham_row, shortlist, mask=None):
        """S: caller row indices in (Hamming, document_id, block_id) order."""
        return self.bits.topk(ham_row, shortlist, mask)[0]

    def exact(self, metric, q, k, mask=None):
        """The exact search over the source: (rows, float64 distances)."""
        qq = round_half(q) if self.half else np.asarray(q, dtype=np.float32)
        return self.orc.filtered_topk(metric, self.x, qq, k, self.doc, self.blk, mask)

    def rerank(self, metric, q, k, S):
        """The first k rows of S by (fp32 distance, NaN last, document_id, block_id): (rows, float64 distances).  The
        distances are the oracle's; the ORDER is the library's contract (include/vsrbac.h, vsr_topk.h: keys carry the
        monotone image of the fp32 value), which differs from the oracle's float8 order exactly where two float8 values
        round to the same fp32 one -- then the ids decide."""
        m = np.zeros(self.x.shape[0], dtype=np.uint8)
        m[S] = 1
        idx, dist = self.exact(metric, q, len(S), m)             # every row of S with its float8 distance
        d32 = dist.astype(np.float32)
        nan = np.isnan(d32)
        order = np.lexsort((self.blk[idx], self.doc[idx], np.where(nan, np.float32(0), d32), nan))[:k]
        return idx[order], dist[order]

    def search(self, metric, queries, k, shortlist, masks=None):
        """Per query (rows, float64 distances, S)."""
        queries = np.atleast_2d(np.asarray(queries, dtype=np.float32))
        ham = self.hamming(queries)
        out = []
        for i, q in enumerate(queries):
            S = self.shortlist(ham[i], shortlist, None if masks is None else masks[i])
            idx, dist = self.rerank(metric, q, k, S)
            out.append((idx, dist, S))
        return out


def recall(found, exact_rows):
    """|found & exact| / |exact| (1 when the exact answer is empty)."""
    exact_rows = np.asarray(exact_rows)
    return 1.0 if exact_rows.size == 0 else np.intersect1d(found, exact_rows).size / exact_rows.size
