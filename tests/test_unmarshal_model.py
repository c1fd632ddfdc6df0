"""The unmarshal tests' model (tests/unmarshal_model.py) against outsiders: the
hand-written bytes of tests/test_marshal_flat.py read backwards, Python's
json.loads plus a flatten on every document the model accepts, and the
oracle's marshaller on seeded trees.  No library, no GPU."""
import json

import pytest

import unmarshal_cases as C
import unmarshal_model as M
from reflow_oracle import OFileset
from test_marshal_flat import HAND, STRINGS


def test_hand_tables_backwards():
    for v, doc in HAND:
        assert M.parse(doc) == (M.canon(v), 0)
    assert M.parse(b'{"Fileset":{"b":{"ID":"sha256:' + C.HEX1 + b'","Size":0},"B":{"ID":"sha256:' + C.HEX1 +
                   b'","Size":0}}}')[1] == M.ORDER


@pytest.mark.parametrize("s,quoted", STRINGS)
def test_strings_backwards(s, quoted):
    value, why = M.parse(C.one(quoted))
    assert why == 0
    # what Go's decoder gives for the encoder's bytes: invalid input bytes came out as U+FFFD
    want = json.loads(quoted.decode()).encode()
    assert value == ((), ((want, C.ID1, 1),))
    if b"\\ufffd" not in quoted:
        assert want == s
    else:  # one replacement per bad byte
        assert want == b"\xef\xbf\xbd" * len(s)


def test_ufffd_escape_and_raw_ufffd():
    assert M.parse(C.one(b'"\\ufffd"'))[0][1][0][0] == "\ufffd".encode()
    assert M.parse(C.one(b'"' + "\ufffd".encode() + b'"'))[0][1][0][0] == "\ufffd".encode()


def test_refusal_table():
    for doc, bit in C.REFUSALS:
        assert M.parse(doc) == (None, bit), doc[:120]
    for doc in C.ACCEPTED:
        assert M.parse(doc)[1] == 0, doc[:120]


def test_every_accepted_document_decodes_the_same_outside_the_model():
    docs = [t.json() for t in C.random_trees(0xB0B, 300)] + [t.json() for t in C.random_trees(0xA11, 200, False)]
    docs += C.mutation_batch() + C.ACCEPTED[:3] + C.ACCEPTED[4:]  # (json.loads recurses: not the 4096-deep chain)
    accepted = 0
    for d in docs:
        value, why = C.model(d)
        if why:
            continue
        accepted += 1
        assert M.from_loads(json.loads(d.decode("utf-8", "surrogatepass"))) == value, d[:200]
    assert accepted > 500


def test_round_trip_of_valid_utf8_trees_is_the_identity():
    for t in C.random_trees(0xB0B, 300):
        assert M.parse(t.json()) == (M.canon(t), 0)
    assert M.parse(OFileset(map={}, list=[]).json()) == (((), ()), 0)
