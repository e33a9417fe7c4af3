"""pgvector's sparsevec text and binary forms (vsrbac.formats.sparsevec_*): every '...'::sparsevec statement of pgvector's
test/expected/sparsevec.out with its output or error (tests/golden/pgvector_sparsevec_known_answers.json, text_io), and binary
values laid out by hand from sparsevec_send (the fixture's `binary`).  CPU only."""
import json
import os

import numpy as np
import pytest

from vsrbac import formats


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "pgvector_sparsevec_known_answers.json")) as f:
        return json.load(f)


def test_text_io_known_answers(known):
    cases = known["text_io"]
    assert len(cases) == 55 and sum("error" in c for c in cases) >= 35
    for c in cases:
        if "error" in c:
            with pytest.raises(ValueError) as e:
                formats.sparsevec_from_text(c["input"], c.get("typmod"))
            assert str(e.value) == c["error"], c
        else:
            ix, vx, dim = formats.sparsevec_from_text(c["input"], c.get("typmod"))
            assert ix.dtype == np.int32 and vx.dtype == np.float32
            assert formats.sparsevec_to_text(ix, vx, dim) == c["output"], c


def test_text_round_trip_and_limits():
    rng = np.random.default_rng(1)
    for dim in (1, 7, 30522, 1000000000):
        nnz = min(dim, 50)
        ix = np.sort(rng.choice(min(dim, 10**6), size=nnz, replace=False)).astype(np.int32)
        if dim > 1:
            ix[-1] = dim - 1                                    # the top of the range
        vx = rng.normal(size=nnz).astype(np.float32)
        vx[vx == 0] = 1
        text = formats.sparsevec_to_text(ix, vx, dim)
        jx, wx, d2 = formats.sparsevec_from_text(text)
        assert d2 == dim and (jx == ix).all() and (wx.view(np.uint32) == vx.view(np.uint32)).all()
    many = "{" + ",".join(f"{i + 1}:1" for i in range(16001)) + "}/20000"
    with pytest.raises(ValueError, match="sparsevec cannot have more than 16000 non-zero elements"):
        formats.sparsevec_from_text(many)
    ix, vx, dim = formats.sparsevec_from_text("{" + ",".join(f"{i + 1}:1" for i in range(16000)) + "}/16000")
    assert ix.size == 16000 and dim == 16000


def test_binary_known_answers(known):
    for c in known["binary"]:
        b = bytes.fromhex(c["hex"])
        if "error" in c:
            with pytest.raises(ValueError) as e:
                formats.sparsevec_from_binary(b, c.get("typmod"))
            assert str(e.value) == c["error"], c
        else:
            ix, vx, dim = formats.sparsevec_from_binary(b)
            assert formats.sparsevec_to_text(ix, vx, dim) == c["text"]
            assert formats.sparsevec_to_binary(ix, vx, dim) == b
            jx, wx, d2 = formats.sparsevec_from_text(c["text"])
            assert formats.sparsevec_to_binary(jx, wx, d2) == b


def test_binary_truncated_and_trailing():
    b = formats.sparsevec_to_binary([0, 2], [1.5, 3.5], 5)
    for cut in (0, 11, 12, 19, len(b) - 1):
        with pytest.raises(ValueError, match="insufficient data left in message"):
            formats.sparsevec_from_binary(b[:cut])
    with pytest.raises(ValueError, match="incorrect binary data format"):
        formats.sparsevec_from_binary(b + b"\0")
