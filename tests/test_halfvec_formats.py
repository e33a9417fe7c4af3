"""halfvec on the host side: the text and binary codecs of vsrbac/formats.py against pgvector's own expectations
(tests/golden/pgvector_halfvec_io.json, transcribed from pgvector/test/expected/halfvec.out:1-164), the wire image of
halfvec_send / halfvec_recv (halfvec.c:356-404), and the claim every GPU halfvec test rests on: pgvector computes a halfvec
distance by widening both operands to fp32 and doing vector.c's arithmetic (halfutils.c), so the existing fp32 oracle on the
widened operands reproduces every distance of halfvec.out:355-499 (tests/golden/pgvector_halfvec_known_answers.json)."""
import json
import math
import os
import struct

import numpy as np
import pytest

from vsrbac import formats


@pytest.fixture(scope="module")
def io_cases(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_halfvec_io.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_halfvec_known_answers.json")) as f:
        return json.load(f)


def widen(v):
    """What a halfvec operand is to the distance functions: rounded to binary16 (nearest even), widened to fp32."""
    return np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)


def test_text_known_answers(io_cases):
    for lit, out in io_cases["text_ok"]:
        v = formats.halfvec_from_text(lit)
        assert v.dtype == np.float16
        assert formats.halfvec_to_text(v) == out, lit
    for lit, msg in io_cases["text_error"]:
        with pytest.raises(ValueError) as e:
            formats.halfvec_from_text(lit)
        assert str(e.value).split("\n")[0] == msg, lit
        if lit in io_cases["details"]:
            assert str(e.value).split("\n")[1] == "DETAIL:  " + io_cases["details"][lit]
    for lit, dim, out in io_cases["typmod"]:
        if out.startswith("["):
            assert formats.halfvec_to_text(formats.halfvec_from_text(lit, dim)) == out
        else:
            with pytest.raises(ValueError) as e:
                formats.halfvec_from_text(lit, dim)
            assert str(e.value) == out


def test_text_rounding_and_limits(io_cases):
    lim = io_cases["dim_limit"]
    top = "[" + ",".join(["1"] * lim["max_dim"]) + "]"
    assert formats.halfvec_from_text(top).size == lim["max_dim"]
    with pytest.raises(ValueError) as e:
        formats.halfvec_from_text(top[:-1] + ",1]")
    assert str(e.value) == lim["too_many"]
    with pytest.raises(ValueError) as e:
        formats.halfvec_to_binary(np.zeros(0, dtype=np.float16))
    assert str(e.value) == lim["too_few"]
    # round to nearest even at the binary16 grid (1 + 2^-10 steps), ties to even; the largest finite value; subnormals
    got = formats.halfvec_from_text("[1.0004,1.00048828125,1.00146484375,65504,6e-8,5.96e-8,2.9e-8]")
    want = np.asarray([1.0, 1.0, 1.001953125, 65504.0, 2.0 ** -24, 2.0 ** -24, 0.0], dtype=np.float16)
    np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))
    # every finite binary16 value survives text and binary round trips bit for bit
    every = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(np.float16)
    every = every[np.isfinite(every)]
    for part in np.array_split(every, 8):
        np.testing.assert_array_equal(formats.halfvec_from_text(formats.halfvec_to_text(part)).view(np.uint16), part.view(np.uint16))
        np.testing.assert_array_equal(formats.halfvec_from_binary(formats.halfvec_to_binary(part)).view(np.uint16), part.view(np.uint16))


def test_binary_layout_and_checks():
    # a hand-built halfvec_send image: int16 dim, int16 unused = 0, dim big-endian uint16 (1.5 = 0x3E00, -2 = 0xC000, 0.5 = 0x3800)
    image = bytes([0x00, 0x03, 0x00, 0x00, 0x3E, 0x00, 0xC0, 0x00, 0x38, 0x00])
    v = formats.halfvec_from_binary(image)
    assert v.dtype == np.float16
    np.testing.assert_array_equal(v, np.asarray([1.5, -2.0, 0.5], dtype=np.float16))
    assert formats.halfvec_to_binary(v) == image
    assert formats.halfvec_to_binary(np.asarray([1.5, -2.0, 0.5], dtype=np.float32)) == image
    with pytest.raises(ValueError, match="expected unused to be 0, not 7"):
        formats.halfvec_from_binary(struct.pack(">hh", 3, 7) + image[4:])
    with pytest.raises(ValueError, match="NaN not allowed in halfvec"):
        formats.halfvec_from_binary(struct.pack(">hhH", 1, 0, 0x7E00))
    with pytest.raises(ValueError, match="infinite value not allowed in halfvec"):
        formats.halfvec_from_binary(struct.pack(">hhH", 1, 0, 0xFC00))
    with pytest.raises(ValueError, match="halfvec must have at least 1 dimension"):
        formats.halfvec_from_binary(struct.pack(">hh", 0, 0))
    with pytest.raises(ValueError, match="expected 2 dimensions, not 3"):
        formats.halfvec_from_binary(image, expected_dim=2)
    with pytest.raises(ValueError, match="insufficient data left in message"):
        formats.halfvec_from_binary(image[:-2])
    with pytest.raises(ValueError, match="incorrect binary data format"):
        formats.halfvec_from_binary(image + b"\0\0")


def test_numpy_float16_cast_is_float4_to_half():
    """The GPU tests take `q.astype(np.float16).astype(np.float32)` as the query `$1::halfvec` holds: round to nearest even
    and overflow to Inf from 65520 on, as Float4ToHalf (halfutils.h:146-261)."""
    with np.errstate(over="ignore"):
        h = np.asarray([65519.996, 65520.0, -65520.0, 1.00048828125, 1.00146484375, 2.98e-8, 2.99e-8], dtype=np.float32).astype(np.float16)
    want = np.asarray([65504.0, np.inf, -np.inf, 1.0, 1.001953125, 0.0, 2.0 ** -24], dtype=np.float16)
    np.testing.assert_array_equal(h, want)


@pytest.mark.parametrize("variant", ["strict", "pgflags"])
def test_oracle_on_widened_operands_reproduces_halfvec_distances(known, variant):
    from oracle.oracle import Oracle
    orc = Oracle(variant)
    seen = set()
    for fn, a, b, want in known["distances"]:
        seen.add(fn)
        if isinstance(want, str) and want.startswith("ERROR:"):
            # the oracle speaks of the vector type; the text the library must produce for a halfvec corpus is the fixture's
            with pytest.raises(ValueError) as e:
                orc.pair(fn, widen(a), widen(b))
            assert str(e.value).replace("vector", "halfvec") == known["dim_error"] and want == "ERROR:  " + known["dim_error"]
            continue
        got = orc.pair(fn, widen(a), widen(b))
        if want == "NaN":
            assert math.isnan(got)
        else:
            assert got == want, (fn, a, b, got, want)      # the regress outputs are exact
    assert seen == {"l2_distance", "inner_product", "negative_inner_product", "cosine_distance", "l1_distance"}
    assert any(len(a) == 9 for _, a, _, _ in known["distances"])          # cases that cross an 8-wide chunk
