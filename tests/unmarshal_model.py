"""A strict recursive-descent parser of the canonical Fileset JSON, in plain
Python, written from the grammar and the refusal rules of include/reflow_hip.h
and independent of the C++: the model the unmarshal tests compare status,
reason and value with.

    parse(doc) -> (value, 0)  or  (None, reason bit)

A value is (children, entries): a tuple of child values and a tuple of
(path bytes, id32, size) in document order; flat() gives capi.Fileset.flat()'s form.
The reason is that of the first thing wrong reading left to right; where the
document ends while more must follow it is LENGTH."""
import sys

STRUCTURE, STRING, ID, SIZE, ORDER, DEPTH, LENGTH = 1, 2, 4, 8, 16, 32, 64
MAX_DEPTH = 4096
HEX = b"0123456789abcdef"


class Refuse(Exception):
    def __init__(self, bit):
        super().__init__(bit)
        self.bit = bit


class _Parser:
    def __init__(self, b):
        self.b, self.i, self.n = b, 0, len(b)

    def peek(self, ahead=0):
        if self.i + ahead >= self.n:
            raise Refuse(LENGTH)
        return self.b[self.i + ahead]

    def lit(self, text, bit):
        for ch in text:
            if self.peek() != ch:
                raise Refuse(bit)
            self.i += 1

    def node(self, depth):
        self.lit(b"{", STRUCTURE)
        if depth > MAX_DEPTH:
            raise Refuse(DEPTH)
        kids, entries = [], ()
        if self.peek() == 0x22:
            if self.peek(1) == ord("L"):
                self.lit(b'"List":[', STRUCTURE)
                while True:
                    kids.append(self.node(depth + 1))
                    c = self.peek()
                    if c == ord("]"):
                        break
                    if c != ord(","):
                        raise Refuse(STRUCTURE)
                    self.i += 1
                self.i += 1
                if self.peek() == ord(","):
                    self.i += 1
                    entries = self.map()
            else:
                entries = self.map()
        self.lit(b"}", STRUCTURE)
        return (tuple(kids), entries)

    def map(self):
        self.lit(b'"Fileset":{', STRUCTURE)
        out, prev = [], None
        while True:
            if self.peek() != 0x22:
                raise Refuse(STRUCTURE)
            self.i += 1
            path = self.string()
            if prev is not None and not prev < path:
                raise Refuse(ORDER)
            prev = path
            self.lit(b':{"ID":"', STRUCTURE)
            self.lit(b"sha256:", ID)
            for k in range(64):
                if self.peek(k) not in HEX:
                    self.i += k
                    raise Refuse(ID)
            fid = bytes.fromhex(self.b[self.i:self.i + 64].decode())
            self.i += 64
            self.lit(b'"', ID)
            if fid == bytes(32):
                raise Refuse(ID)
            self.lit(b',"Size":', STRUCTURE)
            size = self.int()
            self.lit(b"}", SIZE)
            out.append((path, fid, size))
            c = self.peek()
            self.i += 1
            if c == ord("}"):
                return tuple(out)
            if c != ord(","):
                raise Refuse(STRUCTURE)

    def int(self):
        neg = self.i < self.n and self.b[self.i] == ord("-")
        if neg:
            self.i += 1
        c = self.peek()
        if not 0x30 <= c <= 0x39:
            raise Refuse(SIZE)
        if c == 0x30:
            self.i += 1
            if neg:
                raise Refuse(SIZE)
            return 0
        j = self.i
        while j < self.n and 0x30 <= self.b[j] <= 0x39:
            j += 1
        v = int(self.b[self.i:j])
        self.i = j
        v = -v if neg else v
        if not -(1 << 63) <= v < (1 << 63):
            raise Refuse(SIZE)
        return v

    def string(self):
        out = bytearray()
        while True:
            c = self.peek()
            if c == 0x22:
                self.i += 1
                return bytes(out)
            if c == 0x5C:
                e = self.peek(1)
                if e in b'"\\':
                    out.append(e)
                    self.i += 2
                elif e in b"nrt":
                    out.append({ord("n"): 10, ord("r"): 13, ord("t"): 9}[e])
                    self.i += 2
                elif e == ord("u"):
                    self.peek(5)
                    h = self.b[self.i + 2:self.i + 6]
                    if h == b"fffd":
                        out += b"\xef\xbf\xbd"
                    elif h in (b"2028", b"2029"):
                        out += chr(int(h, 16)).encode()
                    elif h[:2] == b"00" and h[2] in HEX and h[3] in HEX:
                        v = int(h, 16)
                        if not ((v < 0x20 and v not in (9, 10, 13)) or v in b"<>&"):
                            raise Refuse(STRING)
                        out.append(v)
                    else:
                        raise Refuse(STRING)
                    self.i += 6
                else:
                    raise Refuse(STRING)
            elif c < 0x80:
                if c < 0x20 or c in b"<>&":
                    raise Refuse(STRING)
                out.append(c)
                self.i += 1
            else:
                want = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 0
                seq = self.b[self.i:self.i + want]
                try:
                    ch = seq.decode("utf-8") if want and len(seq) == want else ""
                except UnicodeDecodeError:
                    ch = ""
                if len(ch) != 1 or ord(ch) in (0x2028, 0x2029):
                    raise Refuse(STRING)
                out += seq
                self.i += want


def parse(doc):
    p = _Parser(bytes(doc))
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 3 * MAX_DEPTH + 1000))
    try:
        if p.n == 0:
            raise Refuse(LENGTH)
        v = p.node(0)
        if p.i != p.n:
            raise Refuse(STRUCTURE)
        return v, 0
    except Refuse as r:
        return None, r.bit
    finally:
        sys.setrecursionlimit(old)


def flat(value):
    """A value as [(depth, entries)] per node in closing order: capi.Fileset.flat()'s
    form, without recursion (a 4096-deep value compares)."""
    out, stack = [], [(value, 0, False)]
    while stack:
        v, d, seen = stack.pop()
        if seen:
            out.append((d, v[1]))
            continue
        stack.append((v, d, True))
        stack.extend((c, d + 1, False) for c in reversed(v[0]))
    return out


def canon(fs):
    """An OFileset / capi.Fileset-shaped object in the model's value form: Maps
    in key order, empty Lists and Maps absent."""
    def key(k):
        return k.encode("utf-8", "surrogateescape") if isinstance(k, str) else bytes(k)
    ents = sorted((key(k), bytes(v[0]), int(v[1])) for k, v in (fs.map or {}).items())
    return (tuple(canon(c) for c in fs.list or ()), tuple(ents))


def from_loads(obj):
    """json.loads' result in the model's value form (the outsider's decode)."""
    ents = sorted((k.encode("utf-8", "surrogatepass"), bytes.fromhex(v["ID"][len("sha256:"):]), v["Size"])
                  for k, v in obj.get("Fileset", {}).items())
    return (tuple(from_loads(c) for c in obj.get("List", [])), tuple(ents))
