"""Hand-built DEFLATE streams for the device inflater's tests, written with
tests/deflate_builder.py at the smallest shapes that reach each edge of
``k_inflate`` (csrc/dcr_inflate.hip): codes beyond the root tables, literal
pairs around the 63-literal flush, the three match-copy paths and their
limits (64, kRingDist = 4032), the 2,048-byte output pieces, stored blocks at
every bit position, 256-byte input windows, and the streams zlib rejects.

``groups()`` builds the list once per process.  tests/test_deflate_builder.py
checks every case against zlib on the CPU (so the expected verdicts are
zlib's); tests/test_gpu_inflate_streams.py runs them on the device.

A case's ``kind``:
  "ok"       zlib inflates ``stream`` to ``data``; the trailer is right
  "stream"   zlib raises on ``stream``
  "trailer"  zlib inflates ``stream`` to ``data``, but ISIZE or CRC32 (what
             the members table hands the kernel) is made wrong
"""
import functools
import zlib

import numpy as np

from tests import deflate_builder as db

STAIR = list(range(1, 15)) + [15, 15]          # a complete code with every length 1..15


class Case:
    def __init__(self, name, stream, data=None, kind="ok", isize=None, crc=None, tail=b"", in_mod=None):
        assert kind in ("ok", "stream", "trailer")
        assert (data is None) == (kind == "stream")
        self.name, self.stream, self.data, self.kind = name, bytes(stream), data, kind
        self.isize = len(data) if isize is None else isize
        self.crc = (zlib.crc32(data) if data is not None else 0) if crc is None else crc
        self.tail = tail        # bytes that follow the stream in the input buffer
        self.in_mod = in_mod    # the in_off mod 256 this case was laid out for (None: any)
        if kind == "ok":
            assert isize is None and crc is None
        if kind == "trailer":
            assert self.isize != len(data) or self.crc != zlib.crc32(data)

    def __repr__(self):
        return f"Case({self.name})"


def rnd(n, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def text(n, seed=0):
    """Record-like text: plenty of matches at many distances."""
    out, i = bytearray(), seed * 1000
    while len(out) < n:
        out += b"read%07d\tMI:Z:%d/A\tRX:Z:ACGT-TTGA\tq%s\n" % (i, i // 8, bytes([33 + (i * 7 + k * k) % 40
                                                                                   for k in range(i % 23)]))
        i += 1
    return bytes(out[:n])


def lens_at(n, pairs):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


def auto_lens(toks, stretch=False, eob=True):
    fl, fd = db.token_freqs(toks, eob)
    pick = db.stretched_lengths if stretch else db.huffman_lengths
    return pick(fl), (pick(fd) if any(fd) else [0])


class Member:
    """A member under construction: the stream and the bytes it stands for."""

    def __init__(self):
        self.s = db.Stream()
        self.out = bytearray()

    def stored(self, data, **kw):
        self.s.stored(data, **kw)
        self.out += data

    def fixed(self, toks, **kw):
        self.s.fixed(toks, **kw)
        self.out += db.replay(toks, bytes(self.out))

    def dynamic(self, toks, ll=None, d=None, stretch=False, **kw):
        if ll is None:
            ll, d = auto_lens(toks, stretch)
        runs = self.s.dynamic(toks, ll, d, **kw)
        self.out += db.replay(toks, bytes(self.out))
        return runs

    def case(self, name, **kw):
        return Case(name, self.s.getvalue(), bytes(self.out), **kw)


def one_block(name, toks, mode="dyn", **kw):
    m = Member()
    if mode == "fixed":
        m.fixed(toks, final=True)
    else:
        m.dynamic(toks, stretch=mode == "stretch", final=True)
    return m.case(name, **kw)


# ---- valid members ----------------------------------------------------------------
def g_code_lengths():
    out = []
    # every literal/length code length 1..15 in one block; 'a'..'g' have the 10..15-bit codes
    syms = [65 + i for i in range(8)] + [256] + [97 + i for i in range(7)]
    ll = lens_at(257, zip(syms, STAIR))
    lits = [s for s in syms if s != 256]
    toks = [lits[i] for i in np.random.default_rng(1).integers(0, 15, 90)] + lits[::-1] + lits
    m = Member()
    m.dynamic(toks, ll, [0], final=True)
    out.append(m.case("ll_lengths_1_to_15"))
    # distance codes of 9..15 bits (symbols 8..15), all used
    d = STAIR[:]
    pre = list(rnd(300, 2))
    toks = pre[:]
    for k, s in enumerate(range(16)):
        toks += [(3 + 5 * k, db.DIST_BASE[s] + (k % (1 << db.DIST_EXTRA[s]))), pre[k]]
    m = Member()
    ll2, _ = auto_lens(toks)
    m.dynamic(toks, ll2, d, final=True)
    out.append(m.case("dist_lengths_9_to_15"))
    # a length symbol on the slow path, then a distance on the slow path
    syms = [65 + i for i in range(13)] + [256, 258, 285]
    ll = lens_at(286, zip(syms, STAIR))
    toks = [65 + int(v) for v in np.random.default_rng(3).integers(0, 13, 300)]
    for k, s in enumerate(range(9, 16)):
        toks += [(4 if k % 2 else 258, db.DIST_BASE[s] + k % 3), 65 + k]
    m = Member()
    m.dynamic(toks, ll, d, final=True)
    out.append(m.case("slow_length_then_slow_distance"))
    # HLIT = 286 with HDIST = 30, every symbol with a code
    ll = [8] * 226 + [9] * 60
    d30 = [4, 4] + [5] * 28
    m = Member()
    m.stored(rnd(24600, 4))
    toks = list(rnd(40, 5)) + [(258, 24582), 7, (3, 1), (230, 30), 255, (10, 24000), (115, 4097)]
    runs = m.dynamic(toks, ll, d30, final=True)
    assert sum(r[3] for r in runs) == 316
    out.append(m.case("hlit_286_hdist_30"))
    # HLIT = 257, HDIST = 1, a zero distance length
    toks = [int(v) for v in rnd(80, 6, 48, 53)]
    m = Member()
    m.dynamic(toks, auto_lens(toks)[0], [0], final=True)
    out.append(m.case("hlit_257_hdist_1_zero"))
    # a distance code that is one 1-bit code (zlib and libdeflate accept it)
    toks = [1, 2, 3, (20, 1), 4, (3, 1), 5, (258, 1)]
    m = Member()
    m.dynamic(toks, auto_lens(toks)[0], [1], final=True)
    out.append(m.case("one_code_distance_sym0"))
    toks = list(rnd(9, 7)) + [(10, 7), 9, (30, 8), (258, 7)]
    m = Member()
    m.dynamic(toks, auto_lens(toks)[0], [0, 0, 0, 0, 0, 1], final=True)
    out.append(m.case("one_code_distance_sym5"))
    # a literal/length code that is one 1-bit code, on symbol 256: an empty block
    m = Member()
    m.dynamic([], lens_at(257, [(256, 1)]), [0], final=True)
    out.append(m.case("one_code_eob_only"))
    return out


def g_header_runs():
    out = []
    # symbol 16 repeating from the literal lengths into the distance lengths
    ll = lens_at(259, [(65, 3), (66, 3), (256, 2), (257, 2), (258, 2)])     # HLIT = 259
    m = Member()
    runs = m.dynamic([65, 66, 65, (3, 1), (4, 2), (3, 3), (4, 4), 66], ll, [2, 2, 2, 2], final=True)
    assert any(r[0] == 16 and r[2] < 259 < r[2] + r[3] for r in runs)
    out.append(m.case("rep16_crosses_hlit"))
    # the same lengths with the run cut at the boundary
    m = Member()
    runs = m.dynamic([65, 66, 66, 65, (3, 1), (4, 4)], ll, [2, 2, 2, 2], final=True, cross=False)
    assert not any(r[2] < 259 < r[2] + r[3] for r in runs)
    out.append(m.case("rep16_cut_at_hlit"))
    # symbol 18 with 138 zeros
    toks = [int(v) for v in rnd(60, 8, 200, 208)]
    m = Member()
    runs = m.dynamic(toks, auto_lens(toks)[0], [0], final=True)
    assert (18, 127) in [(r[0], r[1]) for r in runs]
    out.append(m.case("rep18_138_zeros"))
    # symbol 17 (18 forbidden)
    toks = [10 + 6 * int(v) for v in rnd(120, 9, 0, 30)]
    m = Member()
    runs = m.dynamic(toks, auto_lens(toks)[0], [0], final=True, allow=(17,))
    assert {r[0] for r in runs if r[0] >= 16} == {17}
    out.append(m.case("rep17_only"))
    # no repeat symbols at all
    toks = list(rnd(50, 10, 60, 70)) + [(5, 3), (9, 40)]
    m = Member()
    ll, d = auto_lens(toks)
    runs = m.dynamic(toks, ll, d, final=True, allow=())
    assert all(r[0] < 16 for r in runs)
    out.append(m.case("no_repeat_symbols"))
    return out


# two common literals with 2-bit codes, more with 3..4 bits: most root entries are pairs;
# 121 ('y', 8 bits) never pairs, so it shifts the phase of a run by one literal
PAIR_LL = lens_at(258, [(97, 2), (98, 2), (99, 3), (100, 4), (101, 4), (102, 4), (256, 4), (257, 4), (103, 5),
                        (104, 6), (120, 7), (121, 8), (122, 8)])


def g_pairs():
    assert db.kraft(PAIR_LL) == 32768
    out = []
    for n in (61, 62, 63, 64, 65, 126, 127):
        for phase in (0, 1):
            run = [121] * phase + [97 + int(v) for v in rnd(n - phase, n, 0, 6)]
            for end in ("eob", "match"):
                m = Member()
                m.dynamic(run + ([(3, 2), 104] if end == "match" else []), PAIR_LL, [1, 1], final=True)
                out.append(m.case(f"pairs_{n}_phase{phase}_{end}"))
    # a single literal (the 8-bit one) takes the buffer from 62 to 63 inside a run
    m = Member()
    m.dynamic([97 + int(v) for v in rnd(62, 3, 0, 6)] + [121] + [97 + int(v) for v in rnd(37, 4, 0, 6)], PAIR_LL,
              [1, 1], final=True)
    out.append(m.case("pairs_100_single62_eob"))
    return out


def g_short_dist():
    out = []
    for k, (lo, hi, mode) in enumerate(((1, 22, "stretch"), (22, 43, "fixed"), (43, 64, "dyn"))):
        toks = []
        for dist in range(lo, hi):
            toks += list(rnd(dist, 100 + dist))                 # the period's content: fresh bytes
            toks += [(ln, dist) for ln in (3, 4, 63, 64, 65, 257, 258)]
        out.append(one_block(f"short_dist_{lo}_{hi - 1}", toks, mode))
    return out


RING_D = (64, 65, 127, 128, 4031, 4032)


def g_ring():
    out = []
    # directly after a 1-literal flush / directly after a 3-byte match
    for place in ("lit", "match3"):
        toks = list(rnd(4100, 20))
        for k, (dist, ln) in enumerate((d, ln) for d in RING_D for ln in (3, 258)):
            toks += list(rnd(300, 21 + k)) + [(3, 9)]
            if place == "lit":
                toks.append(k)
            toks.append((ln, dist))
        out.append(one_block(f"ring_after_{place}", toks, "stretch"))
    # directly after a stored block
    m = Member()
    m.stored(rnd(4100, 40))
    for k, (dist, ln) in enumerate((d, ln) for d in RING_D for ln in (3, 258)):
        m.stored(rnd(300, 41 + k))
        if k % 2:
            m.fixed([(ln, dist)])
        else:
            m.dynamic([(ln, dist)])
    m.stored(b"", final=True)
    out.append(m.case("ring_after_stored"))
    return out


HBM_D = (4033, 4095, 4096, 4097, 8192, 32767, 32768)


def g_hbm():
    out = []
    toks = []
    for k, (dist, ln) in enumerate((d, ln) for d in HBM_D for ln in (3, 258)):
        toks += list(rnd(5, 60 + k)) + [(ln, dist)]
    m = Member()
    m.stored(rnd(32768, 50))
    m.dynamic(toks, final=True)
    out.append(m.case("hbm_after_stored_prefix"))
    out.append(one_block("hbm_after_literal_prefix", list(rnd(32768, 51)) + toks, "dyn"))
    # opos == dist: the source is the member's first byte
    for dist in HBM_D:
        for ln in (258, 3) if dist in (4033, 32768) else (258,):
            m = Member()
            m.stored(rnd(dist, 52 + dist % 7))
            m.fixed([(ln, dist)], final=True)
            out.append(m.case(f"hbm_first_byte_{dist}_{ln}"))
    # a 65,536-byte member that ends with the match
    m = Member()
    m.stored(rnd(65536 - 258, 53))
    m.dynamic([(258, 32768)], final=True)
    assert len(m.out) == 65536
    out.append(m.case("hbm_ends_64k_member"))
    return out


SIZES = [0, 1, 31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536] + \
        [2048 * k + r for k in (1, 3) for r in (1, 31, 32, 33) if (k, r) != (1, 1)]


def match_run(n, seed):
    """n bytes as a few literals and one long run of matches."""
    pre = min(n, 70) if n >= 73 or n < 4 else 1
    toks = list(rnd(pre, seed))
    left, k = n - pre, 0
    dists = (70, 7, 65, 1, 33) if pre == 70 else (1,)
    while left:
        ln = min(258, left)
        if 0 < left - ln < 3:
            ln -= 3
        toks.append((ln, dists[k % len(dists)]))
        left -= ln
        k += 1
    return toks


def g_sizes():
    out = []
    for k, n in enumerate(SIZES):
        out.append(one_block(f"size_{n}_literals", list(rnd(n, 70 + k, 64, 80)), "stretch" if k % 2 else "dyn"))
        out.append(one_block(f"size_{n}_matches", match_run(n, 90 + k), "dyn" if k % 2 else "fixed"))
    return out


def g_blocks():
    out = []
    ta = list(rnd(40, 110, 65, 91)) + [(20, 11), (258, 1)]
    # a stored block of LEN 0 as first, middle and last block
    m = Member()
    m.stored(b"")
    m.fixed(ta)
    m.stored(b"")
    m.dynamic(ta, stretch=True)
    m.stored(b"", final=True)
    out.append(m.case("stored_len0_first_middle_last"))
    m = Member()
    m.stored(rnd(65535, 111), final=True)
    out.append(m.case("stored_len_65535"))
    # stored -> dynamic -> fixed -> stored with every bit position before a stored block
    pos_first, pos_last = set(), set()
    for lead in (0, 1):
        for k in range(8):
            m = Member()
            if lead:
                m.fixed([200] * k + [65])
                pos_first.add(m.s.bitpos % 8)
            m.stored(rnd(37 + k, 112 + k))
            m.dynamic(ta + [(30, 60)], stretch=bool(lead))      # the same bits for every k
            m.fixed([66, 67, (5, 2)] + [200] * k)
            if not lead:
                pos_last.add(m.s.bitpos % 8)
            m.stored(rnd(29 + k, 130 + k), final=True)
            out.append(m.case(f"stored_dynamic_fixed_stored_{lead}_{k}"))
    assert pos_first == set(range(8)) and pos_last == set(range(8))
    m = Member()
    m.fixed([], final=True)
    out.append(m.case("empty_fixed_block"))
    # 200 blocks of one token each
    m = Member()
    for i in range(200):
        tok = (3 + i % 20, 1 + i % 10) if len(m.out) >= 10 and i % 4 == 0 else (i * 37) % 256
        final = i == 199
        if i % 3 == 0:
            m.dynamic([tok], final=final)
        elif i % 3 == 1 or not isinstance(tok, int):
            m.fixed([tok], final=final)
        else:
            m.stored(bytes([tok]), final=final)
    out.append(m.case("200_one_token_blocks"))
    # a match whose source lies in an earlier stored block
    m = Member()
    m.stored(rnd(500, 140))
    m.fixed([(100, 400), 65, (258, 500)], final=True)
    out.append(m.case("match_into_stored_block"))
    return out


def fill(bits, seed):
    """Fixed-block literals that take exactly ``bits`` bits (8-bit codes below 144, 9-bit above)."""
    nine = bits % 8
    eight = (bits - 9 * nine) // 8
    assert eight >= 0
    toks = list(rnd(eight, seed, 32, 128)) + list(rnd(nine, seed + 1, 144, 256))
    order = np.random.default_rng(seed + 2).permutation(len(toks))
    return [toks[i] for i in order]


def g_align():
    """Members for the placement test (every in_off mod 4 and out_off mod 4)."""
    out = []
    t = text(5000, 1)
    m = Member()
    m.dynamic(db.tokenize(t[:2000]), stretch=True)
    m.stored(t[2000:3001])
    m.fixed(list(t[3001:3100]))
    m.dynamic([(258, 3000)] * 7 + list(t[:94]), final=True)
    assert len(m.out) == 5000
    out.append(m.case("align_multi_block_5000"))
    # a stored block after an odd number of bits
    m = Member()
    m.fixed(list(t[:11]))
    m.stored(t[100:233])
    m.fixed([(40, 100), 200, 201], final=True)
    out.append(m.case("align_stored_data_start"))
    # the 256-byte input window boundary (bit 2048 of a member at in_off = 0 mod 4) ...
    # ... inside a match's length extra bits: the token starts at bit 2038, extra bits [2046, 2051)
    for name, start, in_extra in (("len_extra", 2038, 8), ("dist_extra", 2027, 18)):
        m = Member()
        toks = fill(start - 3, 150)
        m.s.block_header(1, True)
        codes = db.canonical(db.FIXED_LL), db.canonical(db.FIXED_D)
        m.s.tokens(toks, *codes, eob=False)
        assert m.s.bitpos == start and start + in_extra < 2048 < start + in_extra + 5
        more = [(138, 150), 65, 66, (258, 190), 67]
        m.s.tokens(more, *codes)
        m.out += db.replay(toks + more)
        out.append(m.case(f"window_in_{name}", in_mod=0))
    # ... inside a stored header: LEN in bytes 255 and 256; and the 3 header bits across bit 2048
    for name, end in (("stored_len", 2036), ("stored_type", 2047)):
        m = Member()
        m.fixed(fill(end - 7 - 3, 160))
        assert m.s.bitpos == end
        m.stored(rnd(300, 161))
        m.fixed([(258, 300), 65], final=True)
        out.append(m.case(f"window_in_{name}", in_mod=0))
    return out


REUSE_KINDS = ("dyn_long", "fixed", "stored", "empty", "dyn_one_dist")


def g_reuse():
    """kind -> variants of a tiny member, for launches in which a wave decodes several in turn."""
    out = {k: [] for k in REUSE_KINDS}
    syms = [65 + i for i in range(8)] + [256] + [97 + i for i in range(7)]
    ll = lens_at(257, zip(syms, STAIR))
    lits = [s for s in syms if s != 256]
    for v in range(6):
        m = Member()
        m.dynamic([lits[(i * (v + 1) + v) % 15] for i in range(24)] + lits[9:], ll, [0], final=True)
        out["dyn_long"].append(m.case(f"reuse_dyn_long_{v}"))
        out["fixed"].append(one_block(f"reuse_fixed_{v}", list(rnd(12 + v, 170 + v)) + [(7 + v, 3 + v)], "fixed"))
        m = Member()
        m.stored(rnd(10 + v, 180 + v), final=True)
        out["stored"].append(m.case(f"reuse_stored_{v}"))
        m = Member()
        if v % 2:
            m.fixed([], final=True)
        else:
            m.stored(b"", final=True)
        out["empty"].append(m.case(f"reuse_empty_{v}"))
        toks = [v, v + 1, (9 + v, 1), 200 + v, (3, 1)]
        m = Member()
        m.dynamic(toks, auto_lens(toks)[0], [1], final=True)
        out["dyn_one_dist"].append(m.case(f"reuse_dyn_one_dist_{v}"))
    return out


def good_neighbours():
    return [one_block("good_dynamic", db.tokenize(text(900, 3)), "dyn"),
            one_block("good_fixed", db.tokenize(text(300, 4)), "fixed")]


# ---- invalid members --------------------------------------------------------------
def g_invalid():
    out = []
    fixed_codes = db.canonical(db.FIXED_LL), db.canonical(db.FIXED_D)

    def bad(name, s, isize, **kw):
        out.append(Case(name, s.getvalue() if isinstance(s, db.Stream) else s, None, "stream", isize=isize, **kw))

    # header errors
    s = db.Stream()
    s.block_header(3, True)
    s.bits(0, 29)
    bad("block_type_3", s, 10)
    s = db.Stream()
    s.stored(b"0123456789", final=True, nlen=10)
    bad("nlen_mismatch", s, 10, crc=zlib.crc32(b"0123456789"))
    whole = rnd(100, 200)
    s = db.Stream()
    s.stored(whole[:50], final=True, length=100)
    bad("stored_len_past_member", s, 100, crc=zlib.crc32(whole), tail=whole[50:])
    m = Member()
    m.stored(whole, final=True)
    out.append(m.case("stored_len_past_isize", kind="trailer", isize=99, crc=zlib.crc32(whole[:99])))
    # HLIT = 287 / 288 and HDIST = 31 / 32 in otherwise whole blocks: the extra lengths are 0, the codes
    # complete, the data valid, so that only the count itself is wrong
    toks = db.tokenize(text(300, 7))
    ll, d = auto_lens(toks)
    for name, kw in (("hlit_287", {"hlit": 287}), ("hlit_288", {"hlit": 288}), ("hdist_31", {"hdist": 31}),
                     ("hdist_32", {"hdist": 32})):
        s = db.Stream()
        s.dynamic(toks, ll, d, final=True, **kw)
        bad(name, s, 300, crc=zlib.crc32(text(300, 7)))
    # over-subscribed by one code: a complete code with one length shortened, the block whole
    # behind it (a decoder that does not check the Kraft sum reads most of it)
    def shorten(lens):
        lens = list(lens)
        lens[max(range(len(lens)), key=lambda i: lens[i])] -= 1
        assert db.kraft(lens) > 32768
        return lens
    f = [0] * 19
    for r in db.rle_lengths([(ll + [0] * 286)[:max(257, max(i + 1 for i, l in enumerate(ll) if l))] +
                             d[:max(i + 1 for i, l in enumerate(d) if l)]]):
        f[r[0]] += 1
    for name, kw in (("oversubscribed_code_length_code", {"cl_lens": shorten(db.huffman_lengths(f, 7))}),
                     ("oversubscribed_literal_code", {"ll": shorten(ll)}),
                     ("oversubscribed_distance_code", {"d": shorten(d)})):
        s = db.Stream()
        s.dynamic(toks, kw.pop("ll", ll), kw.pop("d", d), final=True, **kw)
        bad(name, s, 300, crc=zlib.crc32(text(300, 7)))
    # symbol 16 first, in an otherwise whole block: with "the previous length" read as 0 the lengths
    # are 65: 1 bit, 256: 1 bit, no distance code, and the data behind them decodes to AAA
    s = db.Stream()
    cl = lens_at(19, [(16, 2), (18, 2), (0, 2), (1, 2)])
    s.raw_header(0, 0, 18, [cl[db.CL_ORDER[i]] for i in range(18)],
                 [(16, 0), (18, 51), (1, 0), (18, 127), (18, 41), (1, 0), (0, 0)], final=True)
    s.tokens([65, 65, 65], db.canonical(lens_at(257, [(65, 1), (256, 1)])), db.canonical([0]))
    bad("repeat_first", s, 3, crc=zlib.crc32(b"AAA"))
    # a repeat that overruns HLIT + HDIST = 258: 138 + 109 zeros, ten 8s, then 11 more zeros
    s = db.Stream()
    s.raw_header(0, 0, 5, [0, 0, 1, 2, 2], [(18, 127), (18, 98)] + [(8, 0)] * 10 + [(18, 0)], final=True)
    s.bits(0, 32)
    bad("repeat_overruns_total", s, 10)
    s = db.Stream()
    s.dynamic([65, 66, 65], lens_at(257, [(65, 1), (66, 1)]), [0], final=True, eob=False)
    s.bits(0, 32)
    bad("no_code_for_end_of_block", s, 3, crc=zlib.crc32(b"ABA"))

    # incomplete codes whose unused codes never occur
    s = db.Stream()
    s.dynamic([65] * 5, lens_at(257, [(65, 1), (256, 2)]), [0], final=True)
    bad("incomplete_literal_code", s, 5, crc=zlib.crc32(b"AAAAA"))
    toks = db.tokenize(text(600, 5))
    ll, d = auto_lens(toks)
    longest = max(range(len(ll)), key=lambda i: (ll[i] < 15, ll[i]))
    ll[longest] += 1
    assert db.kraft(ll) < 32768
    s = db.Stream()
    s.dynamic(toks, ll, d, final=True)
    bad("incomplete_literal_code_text", s, 600, crc=zlib.crc32(text(600, 5)))
    for name, dl, toks in (("incomplete_distance_one_2bit_code", [2], [1, 2, 3, (5, 1)]),
                           ("incomplete_distance_two_codes", [1, 2], [1, 2, 3, (5, 1), (5, 2)])):
        s = db.Stream()
        s.dynamic(toks, auto_lens(toks)[0], dl, final=True)
        bad(name, s, len(db.replay(toks)), crc=zlib.crc32(db.replay(toks)))
    ll = [8] * 255 + [0, 8]
    assert db.kraft(ll) == 32768
    s = db.Stream()
    s.dynamic([1, 2, 3, 254], ll, [0], final=True, allow=(), cl_lens=lens_at(19, [(8, 1), (0, 2)]))
    bad("incomplete_code_length_code", s, 4, crc=zlib.crc32(bytes([1, 2, 3, 254])))

    # symbol errors
    for sym in (286, 287):
        s = db.Stream()
        s.fixed([65, ("lsym", sym), 66], final=True)
        bad(f"fixed_symbol_{sym}", s, 2)
    for sym in (30, 31):
        s = db.Stream()
        s.fixed([65, 66, 67, ("lsym", 257), ("dsym", sym), 68], final=True)
        bad(f"fixed_distance_symbol_{sym}", s, 7)
    s = db.Stream()
    s.dynamic([65, ("lsym", 257), ("raw", 1, 1)], lens_at(258, [(65, 1), (256, 2), (257, 2)]), [1], final=True)
    bad("unused_code_of_one_code_distance", s, 4)

    # a distance one more than the bytes produced
    for opos in (0, 1, 63, 64, 4096):
        s = db.Stream()
        s.fixed(list(rnd(opos, 210 + opos % 9)) + [(3, opos + 1)], final=True)
        bad(f"distance_too_far_at_{opos}", s, opos + 3)

    # output one byte longer than ISIZE, ending in a literal, a pair, a match; one byte shorter
    m = Member()
    m.fixed(list(b"ACGTACGTA"), final=True)
    out.append(m.case("isize_short_by_literal", kind="trailer", isize=8, crc=zlib.crc32(b"ACGTACGT")))
    m = Member()
    m.dynamic([97, 98] * 5, PAIR_LL, [1, 1], final=True)
    out.append(m.case("isize_short_by_pair", kind="trailer", isize=9, crc=zlib.crc32(b"ab" * 4 + b"a")))
    m = Member()
    m.fixed(list(b"ACGTN") + [(10, 3)], final=True)
    out.append(m.case("isize_short_by_match", kind="trailer", isize=14, crc=zlib.crc32(bytes(m.out[:14]))))
    m = Member()
    m.fixed(list(b"ACGTN") + [(10, 3)], final=True)
    out.append(m.case("isize_long_by_one", kind="trailer", isize=16))

    # truncations: the cut-off bytes follow in the buffer, so only in_len tells
    t = text(1200, 6)
    whole = one_block("whole", db.tokenize(t), "dyn").stream
    n = len(whole)
    for cut in [n - k for k in range(1, 9)] + [n // 4, n // 2, 3 * n // 4]:
        bad(f"truncated_at_{cut}_of_{n}", whole[:cut], 1200, crc=zlib.crc32(t), tail=whole[cut:])
    # a good stream, a wrong CRC32 (2,049 bytes: the short last piece)
    c = one_block("x", list(rnd(2049, 220, 64, 96)), "dyn")
    out.append(Case("wrong_crc_2049", c.stream, c.data, "trailer", crc=c.crc ^ 1))
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """name -> cases, built once per process."""
    return {
        "code_lengths": g_code_lengths(),
        "header_runs": g_header_runs(),
        "pairs": g_pairs(),
        "short_dist": g_short_dist(),
        "ring": g_ring(),
        "hbm": g_hbm(),
        "sizes": g_sizes(),
        "blocks": g_blocks(),
        "align": g_align(),
        "reuse": [c for k in REUSE_KINDS for c in g_reuse()[k]],
        "invalid": g_invalid(),
    }


VALID_GROUPS = ("code_lengths", "header_runs", "pairs", "short_dist", "ring", "hbm", "sizes", "blocks", "align",
                "reuse")
