"""Corpus format x entry point: what the library answers when the two do not match.

Four corpora of 16 rows (vector d = 8, halfvec d = 8, bit d = 16, sparsevec d = 8 with 2 non-zeros per row) against every entry
point of the Python bindings that takes a corpus.  A mismatching cell must give exactly the status and the message below (the
texts are the library's, written out; `{who}` is the C entry point the binding calls); a matching cell must simply succeed.  A
refusal returns before any launch."""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 16, 3
INVALID, DIM_MISMATCH, UNSUPPORTED = 1, 2, 6
FORMATS = ("vector", "halfvec", "bit", "sparsevec")
DIM = {"vector": 8, "halfvec": 8, "bit": 16, "sparsevec": 8}

NOT_BIT = (INVALID, "{who}: the corpus is not a bit corpus")
NOT_SPARSE = (INVALID, "{who}: the corpus is not a sparse corpus")
NOT_HALF = (INVALID, "{who}: the corpus is not a halfvec corpus")
BIT_SEARCH = (UNSUPPORTED, "{who}: a bit corpus is searched with vsr_search_bit* (<~> / <%>), its graphs with vsr_hnsw_search_bit*")
SPARSE_SEARCH = (UNSUPPORTED, "{who}: a sparsevec corpus is searched with vsr_search_sparse* (<->, <#>, <=>, <+>) and has no index path yet")
SPARSE_NO_INDEX = (UNSUPPORTED, "{who}: a sparsevec corpus has no index path yet (the sparsevec_*_ops HNSW opclasses)")
BIT_NO_IVF = (UNSUPPORTED, "{who}: a bit corpus has no index path yet (the bit_hamming_ops / bit_jaccard_ops opclasses)")
HALF_IVF = (UNSUPPORTED, "{who}: a halfvec corpus is indexed with vsr_ivf_kmeans_half / vsr_ivf_assign_half / vsr_ivf_load_half "
                         "(the halfvec_*_ops opclasses)")
HALF_HNSW = (UNSUPPORTED, "{who}: the graph of a halfvec corpus is loaded with vsr_hnsw_load_half and built with vsr_hnsw_build_half "
                          "(the halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops opclasses)")
BIT_HNSW_LOAD = (UNSUPPORTED, "{who}: the graph of a bit corpus is loaded with vsr_hnsw_load_bit (the bit_hamming_ops / bit_jaccard_ops opclasses)")
BIT_HNSW_BUILD = (UNSUPPORTED, "{who}: the graph of a bit corpus is built with vsr_hnsw_build_bit (the bit_hamming_ops / bit_jaccard_ops opclasses)")
BIT_ALREADY = (INVALID, "vsr_corpus_binary_quantize: the corpus is a bit corpus already")
SPARSE_NO_QUANTIZE = (UNSUPPORTED, "vsr_corpus_binary_quantize: a sparsevec corpus has no binary_quantize (pgvector defines none)")
SPARSE_NO_TWO_STAGE = (UNSUPPORTED, "{who}: a sparsevec corpus has no two-stage search (pgvector defines no binary_quantize for sparsevec)")
SOURCE_IS_BIT = (INVALID, "{who}: the source corpus is a bit corpus (the re-rank needs the fp32 or halfvec rows)")
BITS_NOT_BIT = (INVALID, "{who}: the bits corpus is not a bit corpus")
OK = None

# entry point of the bindings -> (the C entry point it reaches, the answer per corpus format in FORMATS order)
TABLE = {
    "search":               ("vsr_search",               (OK, OK, BIT_SEARCH, SPARSE_SEARCH)),
    "search_bit":           ("vsr_search_bit",           (NOT_BIT, NOT_BIT, OK, SPARSE_SEARCH)),
    "search_sparse":        ("vsr_search_sparse",        (NOT_SPARSE, NOT_SPARSE, NOT_SPARSE, OK)),
    "search_device":        ("vsr_search_device",        (OK, OK, BIT_SEARCH, SPARSE_SEARCH)),
    "search_bit_device":    ("vsr_search_bit_device",    (NOT_BIT, NOT_BIT, OK, SPARSE_SEARCH)),
    "search_sparse_device": ("vsr_search_sparse_device", (NOT_SPARSE, NOT_SPARSE, NOT_SPARSE, OK)),
    "load_ivf":             ("vsr_ivf_load",             (OK, HALF_IVF, BIT_NO_IVF, SPARSE_NO_INDEX)),
    "load_ivf_half":        ("vsr_ivf_load_half",        (NOT_HALF, OK, NOT_HALF, NOT_HALF)),
    "ivf_assign":           ("vsr_ivf_assign",           (OK, HALF_IVF, BIT_NO_IVF, SPARSE_NO_INDEX)),
    "ivf_assign_half":      ("vsr_ivf_assign_half",      (NOT_HALF, OK, NOT_HALF, NOT_HALF)),
    "load_hnsw":            ("vsr_hnsw_load",            (OK, HALF_HNSW, BIT_HNSW_LOAD, SPARSE_NO_INDEX)),
    "load_hnsw_bit":        ("vsr_hnsw_load_bit",        (NOT_BIT, NOT_BIT, OK, NOT_BIT)),
    "load_hnsw_half":       ("vsr_hnsw_load_half",       (NOT_HALF, OK, NOT_HALF, NOT_HALF)),
    "build_hnsw":           ("vsr_hnsw_build",           (OK, HALF_HNSW, BIT_HNSW_BUILD, SPARSE_NO_INDEX)),
    "build_hnsw_bit":       ("vsr_hnsw_build_bit",       (NOT_BIT, NOT_BIT, OK, NOT_BIT)),
    "build_hnsw_half":      ("vsr_hnsw_build_half",      (NOT_HALF, OK, NOT_HALF, NOT_HALF)),
    "binary_quantize":      ("vsr_corpus_binary_quantize", (OK, OK, BIT_ALREADY, SPARSE_NO_QUANTIZE)),
    "search_quantized":     ("vsr_search_quantized",     (OK, OK, SOURCE_IS_BIT, SPARSE_NO_TWO_STAGE)),   # the format is the SOURCE corpus's
}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class Env:
    """The four corpora, a 16-row graph per indexable format, and the arguments every call takes."""

    def __init__(self):
        import torch
        import vsrbac
        self.ctx = vsrbac.Context(0)
        rng = np.random.default_rng(7)
        blk = (np.arange(N) + 1).astype(np.int64)
        doc = (np.arange(N) // 4 + 1).astype(np.int32)
        x = rng.standard_normal((N, 8)).astype(np.float32)
        bits = rng.integers(0, 2, (N, 16)).astype(bool)
        sp_idx = np.sort(np.stack([rng.choice(8, 2, replace=False) for _ in range(N)]), axis=1).astype(np.int32).reshape(-1)
        sp_val = rng.uniform(0.5, 1.5, 2 * N).astype(np.float32)
        self.c = {"vector": self.ctx.load_corpus(x, blk, doc),
                  "halfvec": self.ctx.load_corpus_half(x.astype(np.float16), blk, doc),
                  "bit": self.ctx.load_corpus_bit(np.packbits(bits, axis=1), 16, blk, doc),
                  "sparsevec": self.ctx.load_corpus_sparse(np.arange(0, 2 * N + 1, 2), sp_idx, sp_val, 8, blk, doc)}
        self.index = {"vector": self.c["vector"].build_hnsw(4, 8, "l2"), "halfvec": self.c["halfvec"].build_hnsw_half(4, 8, "l2"),
                      "bit": self.c["bit"].build_hnsw_bit(4, 8, "hamming")}
        self.graph = {f: ix.export() for f, ix in self.index.items()}
        self.quantized = {f: self.c[f].binary_quantize() for f in ("vector", "halfvec")}
        self.centers = rng.standard_normal((4, 16)).astype(np.float32)
        self.row_list = (np.arange(N) % 4).astype(np.int32)
        dev = torch.device("cuda", 0)
        self.d_q = torch.from_numpy(rng.standard_normal((1, 16)).astype(np.float32)).to(dev)
        self.d_qb = torch.zeros(4, dtype=torch.uint8, device=dev)
        self.d_ptr = torch.tensor([0, 1], dtype=torch.int64, device=dev)
        self.d_idx = torch.tensor([0], dtype=torch.int32, device=dev)
        self.d_val = torch.tensor([1.0], dtype=torch.float32, device=dev)
        self.out = [torch.empty((1, K), dtype=t, device=dev) for t in (torch.int64, torch.int32, torch.int64, torch.float32)]
        self.out.append(torch.empty((1,), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()                              # the library runs on its own stream

    def q(self, dim):
        return np.linspace(0.0, 1.0, dim, dtype=np.float32).reshape(1, dim)

    def qbits(self, dim):
        return (np.arange(dim) % 3 == 0).reshape(1, dim)

    def call(self, entry, f, dim=None):
        """`entry` on the corpus of format `f`, with queries of `dim` (the corpus's unless given).  Indexes and corpora it makes are freed."""
        c, dim = self.c[f], DIM[f] if dim is None else dim
        outs = [_p(t) for t in self.out]
        made = None
        if entry == "search":
            c.search(self.q(dim), K, "l2")
        elif entry == "search_bit":
            c.search_bit(self.qbits(dim), K, "hamming", dim=dim)
        elif entry == "search_sparse":
            c.search_sparse(np.array([0, 1]), K, "l2", indices=np.array([0]), values=np.array([1.0]), dim=dim)
        elif entry == "search_device":
            c.search_device(_p(self.d_q), 1, K, "l2", None, *outs, dim=dim)
        elif entry == "search_bit_device":
            c.search_bit_device(_p(self.d_qb), 1, K, "hamming", None, *outs, dim=dim)
        elif entry == "search_sparse_device":
            c.search_sparse_device(_p(self.d_ptr), _p(self.d_idx), _p(self.d_val), 1, 1, K, "l2", None, *outs, dim=dim)
        elif entry == "load_ivf":
            made = c.load_ivf(self.centers[:, :c.dim], self.row_list)
        elif entry == "load_ivf_half":
            made = c.load_ivf_half(self.centers[:, :c.dim].astype(np.float16), self.row_list)
        elif entry == "ivf_assign":
            c.ivf_assign(self.centers[:, :c.dim], "l2")
        elif entry == "ivf_assign_half":
            c.ivf_assign_half(self.centers[:, :c.dim].astype(np.float16), "l2")
        elif entry == "load_hnsw":
            made = c.load_hnsw(self.graph.get(f, self.graph["vector"]))
        elif entry == "load_hnsw_bit":
            made = c.load_hnsw_bit(self.graph.get(f, self.graph["vector"]), "hamming")
        elif entry == "load_hnsw_half":
            made = c.load_hnsw_half(self.graph.get(f, self.graph["vector"]))
        elif entry == "build_hnsw":
            made = c.build_hnsw(4, 8, "l2")
        elif entry == "build_hnsw_bit":
            made = c.build_hnsw_bit(4, 8, "hamming")
        elif entry == "build_hnsw_half":
            made = c.build_hnsw_half(4, 8, "l2")
        elif entry == "binary_quantize":
            made = c.binary_quantize()
        elif entry == "search_quantized":
            c.search_quantized(self.quantized.get(f, self.c["bit"]), self.q(dim), K, 4, "l2")
        else:
            raise KeyError(entry)
        self.ctx.synchronize()
        if made is not None:
            made.free()

    def close(self):
        for ix in self.index.values():
            ix.free()
        for c in list(self.quantized.values()) + list(self.c.values()):
            c.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def refused(expected, who, fn, *a, **kw):
    from vsrbac import VsrError
    status, text = expected
    with pytest.raises(VsrError) as e:
        fn(*a, **kw)
    assert (e.value.status, str(e.value)) == (status, text.format(who=who))


@pytest.mark.parametrize("f", FORMATS)
@pytest.mark.parametrize("entry", list(TABLE))
def test_format_against_entry_point(env, entry, f):
    who, answers = TABLE[entry]
    expected = answers[FORMATS.index(f)]
    if expected is OK:
        env.call(entry, f)
    else:
        refused(expected, who, env.call, entry, f)


def test_search_quantized_refuses_bits_that_are_not_the_sources(env):
    """The second corpus of the two-stage search: not a bit corpus, a sparse one, or a bit corpus that was loaded instead of
    quantized from the source -- the message names the source's type.  (Corpus serial numbers depend on what the process made
    before: any number matches.)"""
    from vsrbac import VsrError
    who, q = "vsr_search_quantized", env.q(8)
    for f in ("vector", "halfvec"):
        src = env.c[f]
        refused(BITS_NOT_BIT, who, src.search_quantized, env.c["vector"], q, K, 4, "l2")
        refused(BITS_NOT_BIT, who, src.search_quantized, env.c["halfvec"], q, K, 4, "l2")
        refused(SPARSE_NO_TWO_STAGE, who, src.search_quantized, env.c["sparsevec"], q, K, 4, "l2")
        with pytest.raises(VsrError) as e:
            src.search_quantized(env.c["bit"], q, K, 4, "l2")
        text = (f"vsr_search_quantized: bits corpus #N (16 rows of 16 bits) was not made from source corpus #N ({f}, 16 rows of 8 dimensions) "
                "by vsr_corpus_binary_quantize: it was loaded with vsr_corpus_load_bit")
        pattern = r"#\d+".join(re.escape(part) for part in text.split("#N"))
        assert e.value.status == INVALID and re.fullmatch(pattern, str(e.value)), str(e.value)


def test_graph_search_against_index_format(env):
    """HnswIndex.search / search_bit on a float index (over vector and over halfvec rows) and on a bit index."""
    not_bit_index = (INVALID, "{who}: the index is not over a bit corpus (it is searched with vsr_hnsw_search*)")
    bit_index = (UNSUPPORTED, "{who}: the index is over a bit corpus: it is searched with vsr_hnsw_search_bit* (<~> / <%>)")
    for f in ("vector", "halfvec"):
        env.index[f].search(env.q(8), K, 8, "l2")
        refused(not_bit_index, "vsr_hnsw_search_bit", env.index[f].search_bit, env.qbits(8), K, 8, "hamming")
    env.index["bit"].search_bit(env.qbits(16), K, 8, "hamming")
    refused(bit_index, "vsr_hnsw_search", env.index["bit"].search, env.q(16), K, 8, "l2")


def test_wrong_format_wins_over_wrong_dim(env):
    """Both at once: the format refusal is reported; the dimension alone: CheckDims' message, with the type's name."""
    refused(BIT_SEARCH, "vsr_search", env.call, "search", "bit", 17)
    refused(SPARSE_SEARCH, "vsr_search", env.call, "search", "sparsevec", 9)
    refused(NOT_BIT, "vsr_search_bit", env.call, "search_bit", "vector", 9)
    refused(SPARSE_SEARCH, "vsr_search_bit_device", env.call, "search_bit_device", "sparsevec", 9)
    refused(NOT_SPARSE, "vsr_search_sparse", env.call, "search_sparse", "bit", 17)
    refused(SOURCE_IS_BIT, "vsr_search_quantized", env.call, "search_quantized", "bit", 17)
    refused((UNSUPPORTED, "{who}: the index is over a bit corpus: it is searched with vsr_hnsw_search_bit* (<~> / <%>)"), "vsr_hnsw_search",
            env.index["bit"].search, env.q(17), K, 8, "l2")
    refused((DIM_MISMATCH, "different vector dimensions 8 and 9"), "", env.call, "search", "vector", 9)
    refused((DIM_MISMATCH, "different halfvec dimensions 8 and 9"), "", env.call, "search_device", "halfvec", 9)
    refused((DIM_MISMATCH, "different bit lengths 16 and 17"), "", env.call, "search_bit", "bit", 17)
    refused((DIM_MISMATCH, "different sparsevec dimensions 8 and 9"), "", env.call, "search_sparse", "sparsevec", 9)
    refused((DIM_MISMATCH, "different halfvec dimensions 8 and 9"), "", env.call, "search_quantized", "halfvec", 9)
