"""numpy model of the two-stage search through the bit IVFFlat index (vsr_ivf_search_quantized, include/vsrbac.h).  No new
arithmetic: two models that exist are chained.

  stage 1   qb = binary_quantize(q); S = tests/ivf_bit_model.IvfBit.search (iterative scan off) or .iterative (relaxed_order)
            at k = shortlist over the index of the quantized rows, with the lists the scan had taken
  stage 2   tests/quantized_model.QuantizedModel.rerank of S on the source rows

Everything is in caller row indices.  The index is given by its centres and, optionally, by a row -> list assignment of the
test's choosing (Corpus.load_ivf_bit takes the same), so list shapes are not left to k-means."""
import numpy as np

import bit_model
from ivf_bit_model import IvfBit
from quantized_model import QuantizedModel


class IvfQuantizedModel:
    def __init__(self, oracle, x, centers, row_list=None, doc=None, blk=None, half=False):
        """x: the source rows as fp32 [n, dim] (a halfvec source: its binary16 rows widened); centers: packed [lists, bytes]."""
        self.qm = QuantizedModel(oracle, x, doc, blk, half=half)
        self.dim = self.qm.dim
        self.doc, self.blk = self.qm.doc, self.qm.blk
        self.ivf = IvfBit(bit_model.binary_quantize(self.qm.x), self.dim, centers, self.doc, self.blk)
        if row_list is not None:
            self.ivf.assign = np.asarray(row_list, dtype=np.int32)
        self.lists = self.ivf.lists

    def shortlist(self, q, shortlist, probes, mode="off", max_probes=32768, mask=None):
        """(S in stage-1 order, lists scanned)."""
        qb = bit_model.binary_quantize(q)[0]
        if mode == "off":
            return self.ivf.search(qb, shortlist, probes, mask)[0], min(int(probes), self.lists)
        rows, _, scanned = self.ivf.iterative(qb, shortlist, probes, max_probes, mask)
        return rows, scanned

    def search(self, metric, q, k, shortlist, probes, mode="off", max_probes=32768, mask=None):
        """(rows, float64 distances, S, lists scanned) of one query."""
        S, scanned = self.shortlist(q, shortlist, probes, mode, max_probes, mask)
        if len(S) == 0:                                          # (nothing to re-rank)
            return np.zeros(0, np.int64), np.zeros(0, np.float64), S, scanned
        idx, dist = self.qm.rerank(metric, q, k, S)
        return idx, dist, S, scanned
