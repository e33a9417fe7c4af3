"""Corpora whose permission classes put the number of allowed rows of a query on the edges of the final selection
(vsr_kernels.hip: select_emit_wave_kernel, select_rerank_kernel, K5 + rerank_kernel, rerank_body).  Shared by
test_gpu_select_wave.py (the int8 planes), test_screen_edges.py (the bf16, fp32-MFMA and f16 screening tiers) and
test_gpu_exact_shared.py (K1m, whose edges are those of its candidate buffers).

A World is ~n rows x d in documents of at most 100 rows, dealt in random order over the classes.  The RBAC is a tree as
vsrbac.datasets.tree_rbac makes it (a role is permitted its own documents and its ancestors'; a user holds one role): the
root role owns ONE row and child c one row less than classes[c] says, so the queries of child c's user have exactly that
many allowed rows.  Inside a class every vector occurs one to three times, at scattered rows, so equal distances straddle
the k-th place of most queries; they must come out in row order.

All values are integers; exact_bound() asserts from the rows and queries themselves that every partial sum of a squared L2
distance or an inner product is an integer below 2^24, so the oracle's fp32 sums are exact in any order and results are
compared bit for bit."""
import numpy as np

from helpers import sift_like

# test_gpu_select_wave.py's classes: (allowed rows of the class's queries, queries its user asks); the root comes last and
# owns the one row everybody sees
CLASSES = ((2, 1), (9, 15), (10, 16), (11, 17), (99, 64), (100, 65), (101, 1), (127, 15), (128, 16), (129, 17), (130, 1),
           (255, 1), (256, 15), (257, 1), (511, 15), (512, 16), (513, 17), (1023, 15), (1024, 16), (1025, 17), (16384, 64), (40001, 65), (1, 1))


def small_signed(rng, n, d):
    """Integers -15 .. 15: exact bf16 values with zero mean (the coarse screen's products are exact; distances spread widely
    against |x|^2 + |q|^2)."""
    return rng.integers(-15, 16, (n, d)).astype(np.float32)


class World:
    """classes: (allowed rows, queries) per child role, the root last; role 1 = the root, role 2 + c = child c, user u holds
    role u.  rows(rng, n, d): the row generator; q_range: the values that replace a query's first five coordinates;
    k_ref: how many results ref() keeps; round_query: what the corpus's query type does to a query before the distance
    (halfvec: binary16 rounding), applied by ref()."""

    def __init__(self, classes, d=128, seed=20261019, rows=sift_like, q_range=(0, 256), k_ref=513, round_query=None):
        rng = np.random.default_rng(seed)
        self.classes = classes
        self.k_ref = k_ref
        self.round_query = round_query
        root = len(classes) - 1
        assert classes[root][0] == 1
        sizes = [a - 1 for a, _ in classes[:root]] + [1]
        doc_rows, doc_class = [], []
        for cls, size in enumerate(sizes):
            parts = [100] * (size // 100) + ([size % 100] if size % 100 else [])
            doc_rows += parts
            doc_class += [cls] * len(parts)
        order = rng.permutation(len(doc_rows))                         # every class scattered over the whole corpus
        self.doc_rows = np.asarray(doc_rows)[order]
        self.doc_class = np.asarray(doc_class)[order]
        self.doc = np.repeat(np.arange(1, len(order) + 1), self.doc_rows).astype(np.int32)
        self.n = int(self.doc.size)
        assert self.n == sum(sizes)
        self.blk = (np.arange(self.n) + 1).astype(np.int64)
        row_class = np.repeat(self.doc_class, self.doc_rows)
        self.x = np.empty((self.n, d), dtype=np.float32)
        for cls, size in enumerate(sizes):                             # every vector one to three times, at scattered rows
            base = rows(rng, size, d)
            copies = np.repeat(np.arange(size), rng.integers(1, 4, size))[:size]
            self.x[row_class == cls] = base[rng.permutation(copies)]
        self.role_of_class = [2 + c for c in range(root)] + [1]
        self.quser = np.concatenate([np.full(w, self.role_of_class[c]) for c, (_, w) in enumerate(classes)])
        rng.shuffle(self.quser)
        self.nq = int(self.quser.size)
        q = self.x[rng.integers(0, self.n, self.nq)].copy()
        q[:, :5] = rng.integers(q_range[0], q_range[1], (self.nq, 5)).astype(np.float32)
        self.q = q
        self._ref = {}
        self._rows = {}

    def rbac(self):
        perms = []
        for d, cls in enumerate(self.doc_class):
            role = self.role_of_class[int(cls)]
            perms += [(role, d + 1)] if role != 1 else [(r, d + 1) for r in range(1, len(self.classes) + 1)]
        user_roles = [(r, r) for r in range(1, len(self.classes) + 1)]
        return np.asarray(user_roles, dtype=np.int32), np.asarray(perms, dtype=np.int32)

    def allowed_rows(self, oracle, user):
        if user not in self._rows:
            ur, perms = self.rbac()
            self._rows[user] = np.flatnonzero(oracle.user_row_mask(user, ur, perms, self.doc))
        return self._rows[user]

    def allowed_of_query(self):
        """Allowed rows per query, from the class list (test_candidate_counts_sit_on_the_edges checks it against the oracle)."""
        by_role = {self.role_of_class[c]: a for c, (a, _) in enumerate(self.classes)}
        return np.asarray([by_role[int(u)] for u in self.quser])

    def rq(self, q):
        return q if self.round_query is None else self.round_query(q)

    def ref(self, oracle, i, metric="l2"):
        """The oracle's top k_ref of query i (computed once per metric; a smaller k is its head: same order), over the allowed
        rows only."""
        i = int(i)
        if (metric, i) not in self._ref:
            rows = self.allowed_rows(oracle, int(self.quser[i]))
            idx, dist = oracle.filtered_topk(metric, self.x[rows], self.rq(self.q[i]), self.k_ref, self.doc[rows], self.blk[rows])
            self._ref[(metric, i)] = (rows[idx], dist)
        return self._ref[(metric, i)]

    def exact_bound(self, l1=False):
        """max over rows and queries of (|x| + |q|)^2: bounds every partial sum of |x - q|^2, of |x|^2 + |q|^2 - 2 x.q and of
        x.q -- and with them the three sums of a cosine distance, x.q, |x|^2 and |q|^2.  l1: also |x|_1 + |q|_1, which bounds
        every partial sum of sum |x_i - q_i|; the larger of the two is returned.  Asserts that the values are integers and the
        bound is below 2^24."""
        q = np.stack([self.rq(v) for v in self.q])
        assert (self.x == np.rint(self.x)).all() and (q == np.rint(q)).all()
        nx = float((self.x.astype(np.float64) ** 2).sum(1).max())
        nq = float((q.astype(np.float64) ** 2).sum(1).max())
        bound = (np.sqrt(nx) + np.sqrt(nq)) ** 2
        assert bound < 2 ** 24, (nx, nq, bound)
        if l1:
            ax = float(np.abs(self.x.astype(np.float64)).sum(1).max())
            aq = float(np.abs(q.astype(np.float64)).sum(1).max())
            assert ax + aq < 2 ** 24, (ax, aq)
            bound = max(bound, ax + aq)
        return bound
