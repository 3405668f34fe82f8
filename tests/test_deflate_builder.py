"""The DEFLATE writer (tests/deflate_builder.py) and the inflate case list
(tests/inflate_cases.py) against zlib alone, without a GPU: every valid case
inflates to the bytes its tokens stand for and the whole stream is consumed,
every invalid stream makes zlib raise, every wrong trailer is wrong.  So the
verdict the device test (tests/test_gpu_inflate_streams.py) expects of a case
is zlib's, not the builder's."""
import zlib

import numpy as np
import pytest

from tests import deflate_builder as db
from tests import inflate_cases as ic


def zlib_inflate(stream):
    """(bytes, whole stream consumed and ended) of a raw DEFLATE stream."""
    o = zlib.decompressobj(-15)
    out = o.decompress(stream)
    return out, o.eof and o.unused_data == b"" and o.unconsumed_tail == b""


def all_cases():
    return [c for g in ic.groups().values() for c in g] + ic.good_neighbours()


def test_case_names_are_unique_and_every_group_has_cases():
    names = [c.name for c in all_cases()]
    assert len(set(names)) == len(names)
    assert all(len(g) > 0 for g in ic.groups().values())
    assert {c.kind for c in ic.groups()["invalid"]} == {"stream", "trailer"}
    assert all(c.kind == "ok" for name in ic.VALID_GROUPS for c in ic.groups()[name])


def test_valid_cases_inflate_to_their_tokens():
    n = 0
    for c in all_cases():
        if c.kind == "stream":
            continue
        out, whole = zlib_inflate(c.stream)
        assert out == c.data, c.name
        assert whole, c.name
        n += 1
        if c.kind == "ok":
            assert c.isize == len(out) and c.crc == zlib.crc32(out), c.name
        else:
            assert c.isize != len(out) or c.crc != zlib.crc32(out), c.name
    assert n > 150


def test_invalid_streams_make_zlib_raise():
    n = 0
    for c in all_cases():
        if c.kind != "stream":
            continue
        with pytest.raises(zlib.error):
            zlib.decompress(c.stream, -15)
        # with the cut-off bytes behind it, a truncated stream is whole again
        if c.name.startswith("truncated_at_"):
            out, whole = zlib_inflate(c.stream + c.tail)
            assert whole and len(out) == c.isize and zlib.crc32(out) == c.crc, c.name
        n += 1
    assert n >= 35


def test_the_accepted_incomplete_codes_are_zlibs():
    """One 1-bit literal/length or distance code and an empty distance code
    pass; any other incomplete code is rejected at the block header, used or
    not (the rule of build_table in csrc/dcr_inflate.hip)."""
    by = {c.name: c for c in all_cases()}
    for name in ("one_code_distance_sym0", "one_code_distance_sym5", "one_code_eob_only", "hlit_257_hdist_1_zero"):
        assert by[name].kind == "ok"
    for name in ("incomplete_literal_code", "incomplete_literal_code_text", "incomplete_distance_one_2bit_code",
                 "incomplete_distance_two_codes", "incomplete_code_length_code"):
        with pytest.raises(zlib.error, match="invalid (literal/lengths|distances|code lengths) set"):
            zlib.decompress(by[name].stream, -15)


def test_length_assigners():
    rng = np.random.default_rng(0)
    for trial in range(40):
        n = int(rng.integers(3, 287))
        f = [int(v) for v in rng.integers(0, 50, n) ** 3 * (rng.random(n) < 0.7)]
        f[int(rng.integers(0, n))] += 1
        for limit in (7, 15):
            if limit == 7 and sum(1 for v in f if v) > 19:
                continue
            lens = db.huffman_lengths(f, limit)
            assert db.kraft(lens) == 32768 and max(lens) <= limit
            assert all(l > 0 for l, v in zip(lens, f) if v)
        if sum(1 for v in f if v) >= 16:        # a 15-bit code needs 16 symbols
            lens = db.stretched_lengths(f)
            assert db.kraft(lens) == 32768 and max(lens) == 15, trial
            assert all(l > 0 for l, v in zip(lens, f) if v)
            rare = sorted((s for s in range(n) if lens[s]), key=lambda s: (f[s], -s))[0]
            assert lens[rare] == 15


def test_stretched_blocks_use_long_codes():
    """The cases meant to reach the slow path do: literal/length codes beyond
    the 9-bit root and distance codes beyond the 8-bit root are used."""
    toks = list(ic.rnd(4100, 20))
    ll, _ = ic.auto_lens(toks, stretch=True)
    assert max(ll) == 15 and db.kraft(ll) == 32768
    assert any(ll[t] > 9 for t in toks)


def test_pair_cases_reach_the_flush_edges():
    """The literal-pair members reach the edges they are meant for, whatever
    the seeds: with the kernel's greedy pairing (two literals share a 9-bit
    root entry when their codes fit it) and its flush at 63 or more pending
    literals, a pair takes the buffer from 62 to 64 inside a run and at a
    member's end, a single literal takes it to 63, and members end with 62
    pending and with a flush exactly at ISIZE."""
    events, ends = set(), set()
    for c in ic.groups()["pairs"]:
        _, n, _, end = c.name.split("_")
        run, nlit, i = c.data[:int(n)], 0, 0
        while i < len(run):
            n1 = ic.PAIR_LL[run[i]]
            two = i + 1 < len(run) and n1 + ic.PAIR_LL[run[i + 1]] <= 9
            nlit += 2 if two else 1
            i += 2 if two else 1
            if nlit >= 63:
                events.add((nlit, "pair" if two else "single", "end" if i == len(run) else "inside"))
                if end == "eob" and i == len(run):
                    ends.add(("flush_at_isize", nlit))
                nlit = 0
        if end == "eob":
            ends.add(("pending", nlit))
    assert {(64, "pair", "inside"), (64, "pair", "end"), (63, "single", "inside"), (63, "pair", "inside")} <= events
    assert {("pending", 62), ("flush_at_isize", 63), ("flush_at_isize", 64)} <= ends


def test_bit_writer_and_canonical_codes_round_trip():
    # fixed codes: RFC 1951 3.2.6 gives literal 0 = 00110000, 144 = 110010000, 256 = 0000000, 280 = 11000000
    codes = db.canonical(db.FIXED_LL)
    def msb(c):
        return format(int(format(c[0], f"0{c[1]}b")[::-1], 2), f"0{c[1]}b")
    assert [msb(codes[s]) for s in (0, 144, 256, 280)] == ["00110000", "110010000", "0000000", "11000000"]
    w = db.BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    w.put(0b1011, 4)
    assert w.bitpos == 7
    assert w.getvalue() == bytes([0b1011_01_1])
    assert db.len_symbol(258) == (285, 0, 0) and db.len_symbol(3) == (257, 0, 0) and db.len_symbol(257)[0] == 284
    assert db.dist_symbol(32768) == (29, 13, 8191) and db.dist_symbol(1) == (0, 0, 0)


def test_tokenizer_replays_and_respects_the_window():
    data = ic.text(20_000, 2) + ic.rnd(3000, 1) + ic.text(20_000, 2)
    for max_dist, far in ((32768, True), (4096, False), (1, False)):
        toks = db.tokenize(data, max_dist, far=far)
        assert db.replay(toks) == data
        m = [t for t in toks if not isinstance(t, int)]
        assert m and all(3 <= t[0] <= 258 and 1 <= t[1] <= max_dist for t in m)
    assert max(t[1] for t in db.tokenize(data, 32768, far=True) if not isinstance(t, int)) > 20_000


def test_member_wraps_as_bgzf():
    import gzip
    c = ic.good_neighbours()[0]
    blob = db.member(c.stream, c.data)
    assert gzip.decompress(blob) == c.data
    bad = db.member(c.stream, c.data, crc=c.crc ^ 1)
    with pytest.raises(gzip.BadGzipFile):
        gzip.decompress(bad)
    assert db.member(c.stream, c.data, isize=7)[-4:] == (7).to_bytes(4, "little")
