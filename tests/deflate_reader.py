"""A plain inflater for one raw DEFLATE block (RFC 1951) that reports what
it saw: block type, HLIT / HDIST / HCLEN, the header's code-length symbols
with their extra values, the three code-length arrays, the tokens and the
output.  tests/deflate_cases.py uses it to prove that a case reaches the edge
it is named for (a 15-bit code, a run of 138 zeros, a match 32,768 back); it
is not a second check of zlib, which tests/test_deflate_cases.py holds it to
once, on the cases themselves."""
from dataclasses import dataclass, field

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


@dataclass
class Block:
    btype: int                      # 0 stored, 1 fixed, 2 dynamic
    bfinal: int
    hlit: int = 0
    hdist: int = 0
    hclen: int = 0
    header: list = field(default_factory=list)      # (code-length symbol, extra value), extra 0 for 0..15
    cl_len: list = field(default_factory=list)      # [19] by symbol
    lit_len: list = field(default_factory=list)     # [HLIT + 257]
    dist_len: list = field(default_factory=list)    # [HDIST + 1]
    tokens: list = field(default_factory=list)      # int (a literal) or (length, distance)
    len_syms: set = field(default_factory=set)      # 257..285 as read
    dist_syms: set = field(default_factory=set)     # 0..29 as read
    out: bytes = b""
    end_bit: int = 0                # first bit after the block

    @property
    def stored(self):
        return self.btype == 0

    def matches(self):
        return [t for t in self.tokens if not isinstance(t, int)]


class _Bits:
    def __init__(self, data):
        self.d = bytes(data)
        self.p = 0                  # bit position

    def get(self, nb):
        p = self.p
        assert p + nb <= 8 * len(self.d), "past the end of the stream"
        r = (int.from_bytes(self.d[p >> 3:(p >> 3) + 3], "little") >> (p & 7)) & ((1 << nb) - 1)    # nb <= 16
        self.p = p + nb
        return r


def _decoder(lengths):
    """{(length, canonical code): symbol} (RFC 1951 3.2.2)."""
    count = [0] * 16
    for L in lengths:
        count[L] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for L in range(1, 16):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    table = {}
    for sym, L in enumerate(lengths):
        if L:
            table[(L, nxt[L])] = sym
            nxt[L] += 1
    return table


def _sym(bits, table):
    p = bits.p
    w = int.from_bytes(bits.d[p >> 3:(p >> 3) + 3], "little") >> (p & 7)
    code = 0
    for L in range(1, 16):
        code = (code << 1) | ((w >> (L - 1)) & 1)       # Huffman codes are packed most significant bit first
        s = table.get((L, code))
        if s is not None:
            assert p + L <= 8 * len(bits.d), "past the end of the stream"
            bits.p = p + L
            return s
    raise AssertionError("no such code")


def read_block(raw):
    """The first DEFLATE block of `raw` (a member's bytes 18 .. -8)."""
    bits = _Bits(raw)
    b = Block(bfinal=bits.get(1), btype=bits.get(2))
    assert b.btype != 3
    if b.btype == 0:
        bits.p = (bits.p + 7) & ~7
        n, nn = bits.get(16), bits.get(16)
        assert n ^ nn == 0xffff
        at = bits.p // 8
        b.out = bytes(raw[at:at + n])
        assert len(b.out) == n
        b.tokens = list(b.out)
        b.end_bit = bits.p + 8 * n
        return b
    if b.btype == 1:
        b.lit_len = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        b.dist_len = [5] * 30
    else:
        b.hlit, b.hdist, b.hclen = bits.get(5), bits.get(5), bits.get(4)
        b.cl_len = [0] * 19
        for i in range(b.hclen + 4):
            b.cl_len[CL_ORDER[i]] = bits.get(3)
        cl = _decoder(b.cl_len)
        lens, total = [], b.hlit + 257 + b.hdist + 1
        while len(lens) < total:
            s = _sym(bits, cl)
            if s < 16:
                b.header.append((s, 0))
                lens.append(s)
            elif s == 16:
                e = bits.get(2)
                b.header.append((16, e))
                assert lens, "repeat with nothing before it"
                lens += [lens[-1]] * (3 + e)
            elif s == 17:
                e = bits.get(3)
                b.header.append((17, e))
                lens += [0] * (3 + e)
            else:
                e = bits.get(7)
                b.header.append((18, e))
                lens += [0] * (11 + e)
        assert len(lens) == total, "a run crosses the end of the lengths"
        b.lit_len, b.dist_len = lens[:b.hlit + 257], lens[b.hlit + 257:]
    lit, dist = _decoder(b.lit_len), _decoder(b.dist_len)
    out = bytearray()
    while True:
        s = _sym(bits, lit)
        if s < 256:
            b.tokens.append(s)
            out.append(s)
        elif s == 256:
            break
        else:
            assert s <= 285
            b.len_syms.add(s)
            length = LEN_BASE[s - 257] + bits.get(LEN_EXTRA[s - 257])
            d = _sym(bits, dist)
            assert d < 30
            b.dist_syms.add(d)
            distance = DIST_BASE[d] + bits.get(DIST_EXTRA[d])
            assert distance <= len(out), "distance before the start"
            b.tokens.append((length, distance))
            for _ in range(length):
                out.append(out[-distance])
    b.out = bytes(out)
    b.end_bit = bits.p
    return b


def read_member(member):
    """The one block of a BGZF member made by the compressor."""
    b = read_block(member[18:-8])
    assert b.bfinal == 1 and (b.end_bit + 7) // 8 == len(member) - 26, "one final block fills the member"
    return b
