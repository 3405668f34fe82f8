"""A bit-exact DEFLATE (RFC 1951) writer for tests: it writes exactly the
blocks, code lengths, header symbols and tokens a test asks for, so that the
device inflater (csrc/dcr_inflate.hip) meets streams no compressor would
choose.  Pure Python; zlib is used for CRC32 only.

A token is an ``int`` (a literal byte) or ``(length, distance)``.  Negative
cases may also use ``("lsym", s)`` / ``("dsym", s)`` (the code of a
literal/length or distance symbol with no extra bits) and
``("raw", value, nbits)`` (bits written as they are, LSB first).
"""
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32

# length 3..258 -> (symbol, extra bits, extra value); 258 is symbol 285
_LEN_SYM = [None] * 259
for _s in range(28):
    for _v in range(1 << LEN_EXTRA[_s]):
        _LEN_SYM[LEN_BASE[_s] + _v] = (257 + _s, LEN_EXTRA[_s], _v)
_LEN_SYM[258] = (285, 0, 0)
# distance 1..32768 -> symbol, by the distance's top bits
_DIST_SYM = [0] * 32769
for _s in range(30):
    for _v in range(1 << DIST_EXTRA[_s]):
        _DIST_SYM[DIST_BASE[_s] + _v] = _s


def len_symbol(length):
    return _LEN_SYM[length]


def dist_symbol(dist):
    s = _DIST_SYM[dist]
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def kraft(lengths):
    """Sum of 2^(15 - l) over the nonzero lengths: 32768 for a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1)
        c >>= 1
    return r


def canonical(lengths):
    """Per symbol (code as written LSB first, length), None without a code:
    the canonical code of RFC 1951 3.2.2.  Completeness is not checked."""
    maxl = max(lengths, default=0)
    cnt = [0] * (maxl + 2)
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((_rev(nxt[l] & ((1 << l) - 1), l), l))
            nxt[l] += 1
    return out


class BitWriter:
    """Bits LSB first into bytes (Huffman codes are handed in bit-reversed)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        if self.n >= 64:
            self._spill()

    def _spill(self):
        nb = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
        self.acc >>= 8 * nb
        self.n -= 8 * nb

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def align(self):
        self.n = (self.n + 7) & ~7
        self._spill()

    def write(self, data):
        assert self.n % 8 == 0
        self._spill()
        self.buf += data

    def getvalue(self):
        w = BitWriter()
        w.buf, w.acc, w.n = bytearray(self.buf), self.acc, self.n
        w.align()
        return bytes(w.buf)


# ---- code lengths from frequencies ------------------------------------------------
def huffman_lengths(freqs, maxbits=15):
    """Complete code lengths (Kraft sum 1, at most ``maxbits``) for the symbols
    with a nonzero frequency; with fewer than two such symbols the lowest unused
    ones join, so the code is complete."""
    n = len(freqs)
    used = [s for s in range(n) if freqs[s] > 0]
    for s in range(n):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    f = {s: max(freqs[s], 1) for s in used}
    heap = [(f[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    # limit the lengths: move codes up from the longest level until the Kraft sum fits
    cnt = [0] * (maxbits + 1)
    for s in used:
        cnt[min(depth[s], maxbits)] += 1
    total = sum(cnt[l] << (maxbits - l) for l in range(1, maxbits + 1))
    while total > 1 << maxbits:
        cnt[maxbits] -= 1
        for l in range(maxbits - 1, 0, -1):
            if cnt[l]:
                cnt[l] -= 1
                cnt[l + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (-f[s], s))
    lens, k = [0] * n, 0
    for l in range(1, maxbits + 1):
        for _ in range(cnt[l]):
            lens[order[k]] = l
            k += 1
    assert kraft(lens) == 32768
    return lens


def stretched_lengths(freqs, maxbits=15):
    """As huffman_lengths, but the rarest symbols are pushed down to
    ``maxbits`` bits: the k rarest share one subtree whose leaves descend as
    a stair to two ``maxbits``-bit codes, and the others are shortened to
    keep the Kraft sum at exactly 1 (their Huffman code with the k merged
    into one symbol).  Codes beyond a decoder's root tables then appear by
    construction.  A code with a ``maxbits``-bit member has more than
    ``maxbits`` symbols; with fewer in use the plain lengths are returned."""
    n = len(freqs)
    lens = huffman_lengths(freqs, maxbits)
    used = sorted((s for s in range(n) if lens[s]), key=lambda s: (freqs[s], -s))     # rarest first
    for k in range(2, len(used)):
        group = used[:k]
        f = [0 if s in group else (max(freqs[s], 1) if lens[s] else 0) for s in range(n)]
        red = huffman_lengths(f + [sum(max(freqs[s], 1) for s in group)], maxbits)
        top = red[-1]                               # the depth of the merged symbol
        if top >= maxbits or k < maxbits + 1 - top or k > 1 << (maxbits - top):
            continue
        depths = list(range(top + 1, maxbits)) + [maxbits, maxbits]
        while len(depths) < k:                      # split the shallowest leaf
            i = depths.index(min(depths))
            depths[i] += 1
            depths.append(depths[i])
        depths.sort(reverse=True)
        out = red[:-1]
        for s, dep in zip(group, depths):
            out[s] = dep
        assert kraft(out) == 32768 and max(out) == maxbits
        return out
    return lens


def token_freqs(tokens, eob=True):
    """(literal/length frequencies [286], distance frequencies [30])."""
    ll, d = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            ll[t] += 1
        else:
            ll[_LEN_SYM[t[0]][0]] += 1
            d[_DIST_SYM[t[1]]] += 1
    if eob:
        ll[256] += 1
    return ll, d


def replay(tokens, prefix=b""):
    """The bytes the tokens stand for (after ``prefix``, which matches may reach)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            if not (3 <= length <= 258 and 1 <= dist <= len(out)):
                raise ValueError(f"replay: match {t} at {len(out)}")
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out[len(prefix):])


def rle_lengths(parts, allow=(16, 17, 18)):
    """Run-length code the code lengths as the code-length alphabet:
    [(symbol, extra value, index of the first length, lengths covered)].
    ``parts`` are coded one after the other, each on its own: hand in
    [ll + d] for runs that may cross from the literal lengths into the
    distance lengths, [ll, d] to forbid that."""
    out, base = [], 0
    for seq in parts:
        i, n = 0, len(seq)
        while i < n:
            v, r = seq[i], 1
            while i + r < n and seq[i + r] == v:
                r += 1
            if v == 0 and r >= 11 and 18 in allow:
                k = min(r, 138)
                out.append((18, k - 11, base + i, k))
            elif v == 0 and r >= 3 and 17 in allow:
                k = min(r, 10)
                out.append((17, k - 3, base + i, k))
            elif v != 0 and r >= 4 and 16 in allow:
                out.append((v, 0, base + i, 1))
                k = min(r - 1, 6)
                out.append((16, k - 3, base + i + 1, k))
                k += 1
            else:
                k = 1
                out.append((v, 0, base + i, 1))
            i += k
        base += n
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Stream:
    """One raw DEFLATE stream, block by block."""

    def __init__(self):
        self.w = BitWriter()

    @property
    def bitpos(self):
        return self.w.bitpos

    def bits(self, v, k):
        self.w.put(v, k)

    def getvalue(self):
        return self.w.getvalue()

    def stored(self, data, final=False, nlen=None, length=None):
        """A stored block; ``length`` overrides LEN (the data is written as
        given), ``nlen`` overrides NLEN."""
        w = self.w
        w.put(int(final), 1)
        w.put(0, 2)
        w.align()
        n = len(data) if length is None else length
        assert 0 <= n <= 65535
        w.put(n, 16)
        w.put((n ^ 0xffff) if nlen is None else nlen, 16)
        w.write(data)

    def block_header(self, btype, final=False):
        self.w.put(int(final), 1)
        self.w.put(btype, 2)

    def fixed(self, tokens, final=False, eob=True):
        self.block_header(1, final)
        self.tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)

    def dynamic(self, tokens, ll, d, final=False, eob=True, allow=(16, 17, 18), cross=True, cl_lens=None,
                hlit=None, hdist=None):
        """A dynamic block with the given literal/length and distance code
        lengths (trailing zero lengths are cut unless hlit / hdist say
        otherwise).  The header's code-length code is a Huffman code of the
        run-length symbols unless ``cl_lens`` (19 lengths by symbol) is given.
        Returns the run-length symbols (rle_lengths)."""
        ll, d = list(ll), list(d)
        if hlit is None:
            hlit = max(257, max((i + 1 for i, l in enumerate(ll) if l), default=0))
        if hdist is None:
            hdist = max(1, max((i + 1 for i, l in enumerate(d) if l), default=0))
        ll = (ll + [0] * hlit)[:hlit]
        d = (d + [0] * hdist)[:hdist]
        runs = rle_lengths([ll + d] if cross else [ll, d], allow)
        if cl_lens is None:
            f = [0] * 19
            for r in runs:
                f[r[0]] += 1
            cl_lens = huffman_lengths(f, 7)
        hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
        self.raw_header(hlit - 257, hdist - 1, hclen, [cl_lens[CL_ORDER[i]] for i in range(hclen)],
                        [(r[0], r[1]) for r in runs], final)
        self.tokens(tokens, canonical(ll), canonical(d), eob)
        return runs

    def raw_header(self, hlit_field, hdist_field, hclen, cl_lens_in_order, syms, final=False):
        """A dynamic block header written field by field: the 5/5/4-bit
        counts, ``hclen`` 3-bit lengths in the header's order, then the
        code-length symbols [(symbol, extra value)] with the canonical code of
        those lengths ((``"raw"``, value, nbits) writes bits as they are)."""
        assert 4 <= hclen <= 19 and len(cl_lens_in_order) == hclen
        w = self.w
        self.block_header(2, final)
        w.put(hlit_field, 5)
        w.put(hdist_field, 5)
        w.put(hclen - 4, 4)
        by_sym = [0] * 19
        for i, l in enumerate(cl_lens_in_order):
            w.put(l, 3)
            by_sym[CL_ORDER[i]] = l
        codes = canonical(by_sym)
        for t in syms:
            if t[0] == "raw":
                w.put(t[1], t[2])
                continue
            sym, extra = t
            if codes[sym] is None:
                raise ValueError(f"code-length symbol {sym} has no code")
            w.put(*codes[sym])
            if sym >= 16:
                w.put(extra, _CL_EXTRA[sym])

    def tokens(self, tokens, ll_codes, d_codes, eob=True):
        w = self.w
        put = w.put
        for t in tokens:
            if isinstance(t, int):
                c = ll_codes[t]
                if c is None:
                    raise ValueError(f"literal {t} has no code")
                put(c[0], c[1])
                continue
            if t[0] == "raw":
                put(t[1], t[2])
                continue
            if t[0] == "lsym" or t[0] == "dsym":
                c = (ll_codes if t[0] == "lsym" else d_codes)[t[1]]
                if c is None:
                    raise ValueError(f"symbol {t} has no code")
                put(c[0], c[1])
                continue
            ls, lx, lv = _LEN_SYM[t[0]]
            ds = _DIST_SYM[t[1]]
            c = ll_codes[ls] if ls < len(ll_codes) else None
            dc = d_codes[ds] if ds < len(d_codes) else None
            if c is None or dc is None:
                raise ValueError(f"match {t} has no code")
            put(c[0] | lv << c[1], c[1] + lx)
            put(dc[0] | (t[1] - DIST_BASE[ds]) << dc[1], dc[1] + DIST_EXTRA[ds])
        if eob:
            c = ll_codes[256]
            if c is None:
                raise ValueError("no code for the end of block")
            put(c[0], c[1])


def member(deflate_bytes, data, crc=None, isize=None):
    """The stream as a BGZF member (SAM spec 4.1); crc / isize override the trailer."""
    bsize = 18 + len(deflate_bytes) + 8
    assert bsize <= 65536
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1)
    return hdr + deflate_bytes + struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                                             len(data) if isize is None else isize)


def tokenize(data, max_dist=32768, chain=8, far=False):
    """A greedy hash matcher: minimum match 3, maximum 258, distances up to
    ``max_dist`` (<= 32768); the longest of up to ``chain`` candidates, and
    with ``far`` the farthest among equally long ones."""
    assert 1 <= max_dist <= 32768
    n = len(data)
    head, prev = {}, [-1] * n
    out, i = [], 0

    def insert(p):
        if p + 3 <= n:
            k = data[p:p + 3]
            prev[p] = head.get(k, -1)
            head[k] = p

    while i < n:
        best_len, best_pos = 0, -1
        if i + 3 <= n:
            c, depth = head.get(data[i:i + 3], -1), 0
            lim = min(258, n - i)
            while c >= 0 and i - c <= max_dist and depth < chain:
                m = 3
                while m < lim and data[c + m] == data[i + m]:
                    m += 1
                if m > best_len or (far and m == best_len):
                    best_len, best_pos = m, c
                c = prev[c]
                depth += 1
        if best_len >= 3:
            out.append((best_len, i - best_pos))
            for p in range(i, min(i + best_len, i + 16)):
                insert(p)
            i += best_len
        else:
            out.append(data[i])
            insert(i)
            i += 1
    return out
