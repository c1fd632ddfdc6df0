"""Documents the unmarshal tests share (CPU and GPU): builders for canonical
bytes, the refusal table with the reason bit each case must give, the mutation
batch, and the comparison of a forest with the model (tests/unmarshal_model.py)."""
import random

import unmarshal_model as M
from reflow_amd import capi
from reflow_oracle import OFileset

ID1 = bytes(range(1, 33))
HEX1 = ID1.hex().encode()


def ent(qpath, size=b"1", hexid=HEX1):
    """One Map entry from an already quoted path."""
    return qpath + b':{"ID":"sha256:' + hexid + b'","Size":' + (size if isinstance(size, bytes) else str(size).encode()) + b'}'


def one(qpath, size=b"1", hexid=HEX1):
    return b'{"Fileset":{' + ent(qpath, size, hexid) + b'}}'


def chain(depth):
    """A List chain whose deepest node has this depth (the root is 0)."""
    return b'{"List":[' * depth + b'{}' + b']}' * depth


S, STR, IDB, SZ, ORD, DEP, LEN = M.STRUCTURE, M.STRING, M.ID, M.SIZE, M.ORDER, M.DEPTH, M.LENGTH
E = ent(b'"a"')
REFUSALS = [
    # whitespace anywhere
    (b' {}', S), (b'{} ', S), (b'{ }', S), (b'{"Fileset": {' + E + b'}}', S), (b'{"Fileset":{' + E + b' }}', S),
    (b'{"Fileset":{"a" :{"ID":"sha256:' + HEX1 + b'","Size":1}}}', S),
    (b'{"Fileset":{"a":{"ID": "sha256:' + HEX1 + b'","Size":1}}}', S),
    (b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'", "Size":1}}}', S),
    (b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'","Size": 1}}}', SZ),
    (b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'","Size":1 }}}', SZ),
    (b'{"Fileset":{"a":{"ID":"sha256: ' + HEX1[1:] + b'","Size":1}}}', IDB),
    (b'{"List":[ {}]}', S), (b'{"List":[{} ]}', S), (b'{"List":[{}, {}]}', S), (b'{\n}', S), (b'{\t"List":[{}]}', S),
    # key case, order, duplicates, empties, unknown fields
    (b'{"Fileset":{"a":{"Id":"sha256:' + HEX1 + b'","Size":1}}}', S),
    (b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'","size":1}}}', S),
    (b'{"fileset":{' + E + b'}}', S), (b'{"list":[{}]}', S),
    (b'{"Fileset":{' + E + b'},"List":[{}]}', S),
    (b'{"Fileset":{"a":{"Size":1,"ID":"sha256:' + HEX1 + b'"}}}', S),
    (b'{"Fileset":{' + E + b',' + E + b'}}', ORD),
    (b'{"Fileset":{' + ent(b'"b"') + b',' + ent(b'"a"') + b'}}', ORD),
    (b'{"Fileset":{' + ent(b'"a\\u0000"') + b',' + ent(b'"a"') + b'}}', ORD),
    (b'{"Fileset":{}}', S), (b'{"List":[]}', S), (b'{"List":[{}],"Fileset":{}}', S),
    (b'{"Fileset":{' + E + b'},"X":1}', S), (b'{"X":1}', S), (b'{"List":[{}],"X":{}}', S),
    (b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'","Size":1,"X":1}}}', SZ),
    (b'{"Fileset":{' + E + b'},"Fileset":{' + E + b'}}', S), (b'{"List":[{}],"List":[{}]}', S),
    # escapes the encoder never emits, raw bytes it always escapes
    (one(b'"\\u0041"'), STR), (one(b'"\\u003C"'), STR), (one(b'"\\/"'), STR), (one(b'"\\b"'), STR),
    (one(b'"\\f"'), STR), (one(b'"\\u000a"'), STR), (one(b'"\\u0022"'), STR), (one(b'"\\u005c"'), STR),
    (one(b'"\\uFFFD"'), STR), (one(b'"\\u00e9"'), STR), (one(b'"\\ud83d\\ude00"'), STR),
    (one(b'"<"'), STR), (one(b'">"'), STR), (one(b'"&"'), STR), (one(b'"\x01"'), STR), (one(b'"\n"'), STR),
    (one(b'"\xff"'), STR), (one(b'"\xe2\x82"'), STR), (one(b'"\xed\xa0\x80"'), STR), (one(b'"\xc0\xaf"'), STR),
    (one(b'"\xf4\x90\x80\x80"'), STR), (one(b'"\xe2\x80\xa8"'), STR), (one(b'"\xe2\x80\xa9"'), STR),
    # IDs
    (one(b'"a"', hexid=HEX1[:63]), IDB), (one(b'"a"', hexid=HEX1 + b"0"), IDB), (one(b'"a"', hexid=HEX1.upper()), IDB),
    (one(b'"a"', hexid=b"0A" + HEX1[2:]), IDB), (one(b'"a"', hexid=b"0" * 64), IDB),
    (b'{"Fileset":{"a":{"ID":"sha512:' + HEX1 + b'","Size":1}}}', IDB),
    (b'{"Fileset":{"a":{"ID":"' + HEX1 + b'","Size":1}}}', IDB),
    # sizes
    (one(b'"a"', b"-0"), SZ), (one(b'"a"', b"01"), SZ), (one(b'"a"', b"1.0"), SZ), (one(b'"a"', b"1e3"), SZ),
    (one(b'"a"', b""), SZ), (one(b'"a"', b"9223372036854775808"), SZ), (one(b'"a"', b"-9223372036854775809"), SZ),
    (one(b'"a"', b"-"), SZ), (one(b'"a"', b"+1"), SZ), (one(b'"a"', b'"1"'), SZ), (one(b'"a"', b"9" * 40), SZ),
    # structure at the ends
    (b'{}}', S), (b'{}{}', S), (b'{},{}', S), (b'', LEN), (b'}}}}', S), (b'{"List":[{}}}', S), (b'{"List":[{}]]', S),
    (b'[{}]', S), (b'{"List":[{}],}', S), (b'{"List":[{},]}', S), (b'{"Fileset":{' + E + b',}}', S),
    (b'{', LEN), (b'{"List":[{}]', LEN), (one(b'"a"')[:-1], LEN), (b'{"Fileset":{"abc', LEN),
    (chain(4097), DEP),
]
ACCEPTED = [b'{}', one(b'"a"', b"-9223372036854775808"), one(b'"a"', b"9223372036854775807"), chain(4096),
            one(b'"Fileset"'), one(b'"ID"'), one(b'""'), b'{"List":[{},{"List":[{}]}],"Fileset":{' + E + b'}}',
            b'{"Fileset":{' + ent(b'"a"') + b',' + ent(b'"a\\u0000"') + b'}}']

MUTATION_DOCS = [
    b'{}', b'{"List":[{}]}', b'{"List":[{},{}]}', one(b'"a"'), one(b'"a\\"b\\\\"', b"-10"),
    one(b'"\\u003c\xc3\xa9"', b"0"), one(b'"\\n\\ufffd\\u2028"', b"7"), one(b'""', b"12"),
    b'{"List":[{}],"Fileset":{' + ent(b'"ID"') + b',' + ent(b'"Size"', b"2") + b'}}',
    b'{"List":[{"Fileset":{' + ent(b'"Fileset"', b"5") + b'}},{"List":[{}]}]}',
    b'{"Fileset":{' + ent(b'"List"') + b',' + ent(b'"a"', b"22") + b',' + ent(b'"b"', b"333") + b'}}',
    b'{"List":[{"List":[{"List":[{}]}]}]}', b'{"List":[{},{},{}],"Fileset":{' + ent(b'"x/y"', b"-1") + b'}}',
    one(b'"\xf0\x9f\x98\x80"'), one(b'"sha256:"'), one(b'"\\\\\\\\"'), one(b'"0"', b"100"),
    b'{"Fileset":{' + ent(b'"a"') + b',' + ent(b'"aa"') + b'}}', b'{"List":[{"Fileset":{' + E + b'}}]}',
    b'{"List":[{"List":[{}],"Fileset":{' + E + b'}},{}]}',
]
SUBS = b'"\\{}[],:0a '


def mutation_batch():
    """Every single-byte deletion of MUTATION_DOCS and every substitution by a byte of SUBS."""
    out = []
    for d in MUTATION_DOCS:
        for k in range(len(d)):
            out.append(d[:k] + d[k + 1:])
            for c in SUBS:
                if c != d[k]:
                    out.append(d[:k] + bytes([c]) + d[k + 1:])
    return out


def random_tree(rng, depth=0, valid_utf8=True):
    """tests/test_marshal_flat.py's generator shape; valid_utf8 keeps every path
    a valid UTF-8 string (the round trip's condition)."""
    def path():
        n = rng.randint(0, 12)
        if valid_utf8:
            p = "".join(rng.choice(["a", "/", '"', "\\", "\n", "<", "&", "\x00", "\x7f", "\u00e9", "\u65e5", "\u2028",
                                    "\U0001F600", "\ufffd", "z", "\t"]) for _ in range(n)).encode()
        else:
            p = bytes(rng.randrange(256) for _ in range(n))
            if rng.random() < 0.3:
                p += rng.choice(["\u00e9", "\u65e5", "\u2028", "\U0001F600"]).encode()
        return p
    m = None
    if rng.random() < 0.8:
        m = {}
        for _ in range(rng.randint(0, 6)):
            m[path()] = (bytes(rng.randrange(1, 256) for _ in range(32)), rng.randint(-(1 << 63), (1 << 63) - 1))
    lst = None
    if depth < 3 and rng.random() < 0.4:
        lst = [random_tree(rng, depth + 1, valid_utf8) for _ in range(rng.randint(0, 3))]
    return OFileset(map=m, list=lst)


def random_trees(seed, n, valid_utf8=True):
    rng = random.Random(seed)
    return [random_tree(rng, 0, valid_utf8) for _ in range(n)]


_MODEL = {}


def model(doc):
    """parse(doc), remembered: the reference is computed once per document."""
    r = _MODEL.get(doc)
    if r is None:
        r = _MODEL[doc] = M.parse(doc)
    return r


def check_forest(f, docs, label=""):
    """Status, reason, counts and value of every document against the model."""
    status, reason, ncnt, ecnt = f.status()
    values = f.values()
    want = [model(d) for d in docs]
    assert reason.tolist() == [w[1] for w in want], label
    assert status.tolist() == [capi.RF_ENOTCANONICAL if w[1] else capi.RF_OK for w in want], label
    for d, v, w, nn, ne in zip(docs, values, want, ncnt, ecnt):
        if w[0] is None:
            assert v is None and nn == 0 and ne == 0, (label, d)
        else:
            assert v is not None and v.flat() == M.flat(w[0]), (label, d)
    assert f.n_accepted == sum(1 for w in want if w[0] is not None) and f.n_docs == len(docs)
    assert f.n_entries == int(ecnt.sum()) and f.n_nodes == int(ncnt.sum())
