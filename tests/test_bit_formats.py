"""pgvector's bit type on the CPU: the numpy model of tests/bit_model.py reproduces every known answer of pgvector's own
regression output (tests/golden/pgvector_bit_known_answers.json), which pins the model the GPU tests compare against; the
varbit text / binary codecs of vsrbac.formats round-trip in PostgreSQL's bit order."""
import json
import os
import struct

import numpy as np
import pytest

import bit_model
from vsrbac import formats

LENGTHS = [0, 1, 7, 8, 9, 1025]


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_bit_known_answers.json")) as f:
        return json.load(f)


def test_fixture_covers_the_regression_file(known):
    fns = [c["fn"] for c in known["distances"]]
    assert fns.count("hamming_distance") == 12 and fns.count("jaccard_distance") == 14
    errors = [c["error"] for c in known["distances"] if "error" in c]
    assert errors == ["different bit lengths 3 and 2", "different bit lengths 3 and 4", "different bit lengths 4 and 3",
                      "different bit lengths 4 and 5"]
    assert any(len(c["a"]) > 512 for c in known["distances"]) and any(len(c["a"]) == 0 for c in known["distances"])
    assert len(known["binary_quantize"]) == 3


def test_model_reproduces_every_known_answer(known):
    for c in known["distances"]:
        a, b = formats.bit_from_text(c["a"]), formats.bit_from_text(c["b"])
        if "error" in c:
            assert a.size != b.size and c["error"] == f"different bit lengths {a.size} and {b.size}"
            continue
        assert a.size == b.size
        metric = "hamming" if c["fn"] == "hamming_distance" else "jaccard"
        got = bit_model.distances(metric, bit_model.pack(a), bit_model.pack(b), a.size)
        assert got.shape == (1,) and got[0] == c["expected"], (c, got)      # exact float8
        # pad bits never count
        if a.size:
            got = bit_model.distances(metric, bit_model.set_pad_bits(bit_model.pack(a), a.size),
                                      bit_model.set_pad_bits(bit_model.pack(b), a.size), a.size)
            assert got[0] == c["expected"]


def test_model_topk_order_and_mask():
    """A self-check of tests/bit_model.py alone (it touches no library symbol and passes without the feature): the order the GPU
    tests expect is np.lexsort((blk, doc, dist32)) restricted to the mask."""
    rows = bit_model.pack(np.asarray([[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 0, 0]], dtype=bool))
    q = bit_model.pack(np.asarray([[1, 1, 0, 0]], dtype=bool))
    doc = np.asarray([2, 1, 1, 1, 1], dtype=np.int32)
    blk = np.asarray([1, 9, 8, 7, 3], dtype=np.int64)
    idx, dist = bit_model.topk("hamming", rows, q, 4, 5, doc, blk)
    assert idx.tolist() == [4, 2, 0, 1, 3] and dist.tolist() == [0, 0, 0, 1, 4] and dist.dtype == np.float32
    idx, dist = bit_model.topk("jaccard", rows, q, 4, 3, doc, blk, mask=[1, 1, 0, 1, 0])
    assert idx.tolist() == [0, 1, 3] and dist.tolist() == [0.0, 0.5, 1.0]
    rng = np.random.default_rng(0)
    rows = bit_model.pack(rng.random((500, 12)) < 0.5)
    doc, blk = rng.integers(1, 9, 500).astype(np.int32), rng.permutation(500).astype(np.int64)
    idx, dist = bit_model.topk("hamming", rows, rows[:1], 12, 500, doc, blk)
    d32 = bit_model.distances("hamming", rows, rows[:1], 12).astype(np.float32)
    assert idx.tolist() == np.lexsort((blk, doc, d32)).tolist() and (dist == d32[idx]).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_codec_round_trips(n):
    rng = np.random.default_rng(n)
    v = rng.random(n) < 0.5
    text = formats.bit_to_text(v)
    assert len(text) == n and set(text) <= {"0", "1"}
    for lit in (text, "B" + text, "b" + text):
        back = formats.bit_from_text(lit)
        assert back.dtype == np.bool_ and back.shape == (n,) and (back == v).all()
    wire = formats.bit_to_binary(v)
    assert len(wire) == 4 + (n + 7) // 8 and struct.unpack(">i", wire[:4])[0] == n
    back = formats.bit_from_binary(wire)
    assert back.dtype == np.bool_ and back.shape == (n,) and (back == v).all()
    assert wire[4:] == bit_model.pack(v)[0].tobytes()                       # the corpus layout is the wire layout


def test_bit_order_and_padding():
    assert formats.bit_to_binary(formats.bit_from_text("10000000")) == struct.pack(">i", 8) + b"\x80"
    assert formats.bit_to_binary(formats.bit_from_text("00000001")) == struct.pack(">i", 8) + b"\x01"
    assert formats.bit_to_binary(formats.bit_from_text("1")) == struct.pack(">i", 1) + b"\x80"
    assert formats.bit_to_binary(formats.bit_from_text("000000001")) == struct.pack(">i", 9) + b"\x00\x80"
    assert formats.bit_to_binary(formats.bit_from_text("")) == struct.pack(">i", 0)
    for n in LENGTHS:
        wire = formats.bit_to_binary(np.ones(n, dtype=bool))               # pad bits are zero on output
        if n % 8:
            assert wire[-1] == (0xFF00 >> (n % 8)) & 0xFF
    # ... and ignored on input, as varbit_recv clears them
    assert formats.bit_from_binary(struct.pack(">i", 3) + b"\xff").tolist() == [True, True, True]
    for bad in ("102", "x01", "B0 1"):
        with pytest.raises(ValueError):
            formats.bit_from_text(bad)
    with pytest.raises(ValueError):
        formats.bit_from_binary(b"\x00\x00")
    with pytest.raises(ValueError):
        formats.bit_from_binary(struct.pack(">i", 9) + b"\x00")
    with pytest.raises(ValueError):
        formats.bit_from_binary(struct.pack(">i", -1))


def test_binary_quantize_known_answers(known):
    for c in known["binary_quantize"]:
        v = np.asarray(c["vector"], dtype=np.float32)
        packed = bit_model.binary_quantize(v)
        assert formats.bit_to_text(bit_model.unpack(packed, v.size)[0]) == c["expected"]
        assert (bit_model.unpack(packed, 8 * packed.shape[1])[0, v.size:] == 0).all()          # pad bits zero
    edge = np.asarray([[0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, 2.0]], dtype=np.float32)
    assert formats.bit_to_text(bit_model.unpack(bit_model.binary_quantize(edge), 9)[0]) == "000101011"
    # a halfvec quantizes like its widened value: positive exactly when the half is
    h = np.asarray([6e-8, -6e-8, 0.0, 65504.0], dtype=np.float16)
    assert formats.bit_to_text(bit_model.unpack(bit_model.binary_quantize(h.astype(np.float32)), 4)[0]) == "1001"


def test_ffi_declares_the_bit_entry_points():
    from vsrbac import _ffi
    for name in ("vsr_corpus_load_bit", "vsr_corpus_is_bit", "vsr_search_bit", "vsr_search_bit_device", "vsr_search_bit_device_on",
                 "vsr_bit_pair_distances", "vsr_binary_quantize", "vsr_corpus_binary_quantize"):
        assert name in _ffi.SYMBOLS, name
