"""``k_inflate`` (csrc/dcr_inflate.hip) against zlib on DEFLATE streams that
zlib never emits: the hand-built members of tests/inflate_cases.py, handed to
``dcr_inflater_run`` with a members table made here, so that ``in_off`` and
``out_off`` are the test's.  The oracle is zlib: where it inflates a member,
rc is 0 and the member's bytes are zlib's; where it raises, or the trailer
is made wrong, rc is the index + 1 of the first such member and the members
around it are intact.  tests/test_deflate_builder.py checks the same list
on the CPU (reference: the BAM read under ``samfile.fetch``,
DuplexUMIConsensusReads.py:1476, :1519, through htslib, which accepts any
RFC 1951 stream)."""
import zlib

import numpy as np
import pytest

from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu

_WANT = {}


def want(c):
    """zlib's verdict on a case: its bytes, or None where zlib raises."""
    if c.name not in _WANT:
        try:
            _WANT[c.name] = zlib.decompress(c.stream, -15)      # raises on a truncated stream too
        except zlib.error:
            _WANT[c.name] = None
        assert (_WANT[c.name] is None) == (c.kind == "stream"), c.name
    return _WANT[c.name]


def fails(c):
    return c.kind != "ok"


def lay_out(cases, in_mod4=None, out_offs=None, out_bytes=None):
    """(input buffer, members table, output bytes): the streams one after the
    other with 0-3 bytes of junk between them (``in_mod4``: each member's
    in_off mod 4), nothing behind the last one; outputs back to back unless
    ``out_offs`` says where."""
    from duplexumiconsensusreads_amd import _lib
    buf, rows, o = bytearray(), [], 0
    for i, c in enumerate(cases):
        if c.in_mod is not None:
            buf += b"\xd7" * ((c.in_mod - len(buf)) % 256)
        else:
            r = in_mod4[i] if in_mod4 is not None else (i * 3 + 1) % 4
            buf += b"\xd7" * ((r - len(buf)) % 4)
        oo = o if out_offs is None else out_offs[i]
        rows.append((len(buf), oo, len(c.stream), c.isize, c.crc, 0))
        buf += c.stream + c.tail
        o = oo + c.isize
    return bytes(buf), np.array(rows, dtype=_lib.BGZF_MEMBER_DTYPE), (o if out_bytes is None else out_bytes)


def check(cases, m, rc, out, label=""):
    """rc names the first member zlib (or its trailer) rejects; every member
    zlib accepts has zlib's bytes, whatever failed beside it."""
    bad = [i for i, c in enumerate(cases) if fails(c)]
    assert rc == (bad[0] + 1 if bad else 0), (label, rc, cases[rc - 1].name if rc else None)
    out = out.tobytes()
    for c, row in zip(cases, m):
        if not fails(c):
            o = int(row["out_off"])
            assert out[o:o + c.isize] == want(c), (label, c.name)


def launch(inf, buf, m, n):
    """One dcr_inflater_run; a HIP runtime error (not a member's verdict)
    ends the session, so that nothing more is started on a device that has
    faulted.  An argument error (a mistake in a test's layout, refused on the
    host before anything is launched) fails the test like any other."""
    from duplexumiconsensusreads_amd import _lib
    try:
        return inf.run(np.frombuffer(buf, np.uint8), m, n)
    except _lib.DcrError as e:
        if "outside the buffers" in str(e) or "bad arguments" in str(e):
            raise
        pytest.exit(f"device runtime error, session ended: {e}", 1)


def run(inf, cases, label="", **kw):
    from duplexumiconsensusreads_amd import _lib
    buf, m, n = lay_out(cases, **kw)
    rc, out = launch(inf, buf, m, n)
    if rc and not any(fails(c) for c in cases):
        print("inflate:", label, _lib.load().dcr_last_error().decode())
    check(cases, m, rc, out, label)
    return m, out


@pytest.fixture(scope="module")
def inf():
    from duplexumiconsensusreads_amd import _lib
    h = _lib.Inflater(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def groups():
    g = ic.groups()
    for cases in g.values():
        for c in cases:
            want(c)
    return g


@pytest.mark.parametrize("group", ic.VALID_GROUPS)
def test_valid_members(inf, groups, group):
    cases = groups[group]
    assert cases and all(c.kind == "ok" and want(c) == c.data for c in cases)
    for c in cases:                       # one member per launch: a failure names its case
        run(inf, [c], c.name)
    run(inf, cases, group)                # then all in one launch


def test_invalid_members(inf, groups):
    """Each invalid member between two good ones: reported by index, the
    neighbours' outputs intact."""
    good = ic.good_neighbours()
    bad = groups["invalid"]
    assert all(fails(c) for c in bad) and not any(fails(c) for c in good)
    for c in bad:
        run(inf, [good[0], c, good[1]], c.name)
    every = [good[0]]
    for i, c in enumerate(bad):
        every += [c, good[i % 2]]
    run(inf, every, "all invalid members")
    # the first failing member is the one reported, wherever it stands
    run(inf, [good[0], good[1], good[0]] + bad[::-1] + [good[1]], "invalid members last")


def test_alignment_placements(inf, groups):
    """The same multi-block member at every in_off mod 4 and out_off mod 4 in
    one launch, the stored-block variant at every byte alignment of its data,
    the window-boundary members where they were laid out for, and the last
    member ending at the last byte of the input buffer."""
    by = {c.name: c for c in groups["align"]}
    a, b = by["align_multi_block_5000"], by["align_stored_data_start"]
    cases, in_mod4, out_offs, o = [], [], [], 0
    for i in range(4):
        for j in range(4):
            for c in (a, b):
                cases.append(c)
                in_mod4.append(i)
                o += (j - o) % 4
                out_offs.append(o)
                o += c.isize
    windows = [c for c in groups["align"] if c.in_mod is not None]
    assert len(windows) == 4
    for c in windows:
        cases.append(c)
        in_mod4.append(0)
        out_offs.append(o)
        o += c.isize + 3
    cases.append(a)
    in_mod4.append(3)
    out_offs.append(o)
    buf, m, n = lay_out(cases, in_mod4=in_mod4, out_offs=out_offs)
    assert {(int(r["in_off"]) % 4, int(r["out_off"]) % 4) for r, c in zip(m, cases) if c is a} == \
        {(i, j) for i in range(4) for j in range(4)}
    assert all(int(r["in_off"]) % 256 == 0 for r, c in zip(m, cases) if c.in_mod is not None)
    assert int(m[-1]["in_off"]) + int(m[-1]["in_len"]) == len(buf)
    rc, out = launch(inf, buf, m, n)
    check(cases, m, rc, out, "placements")


def test_wave_reuse(inf, groups):
    """More members than the launch has waves (16 workgroups per CU), so a
    wave decodes several in turn with the previous member's tables in LDS:
    every kind of member follows every other kind on some wave."""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = 16 * cu
    n = max(5000, grid + grid // 2)
    kinds = {k: [c for c in groups["reuse"] if c.name.startswith(f"reuse_{k}_")] for k in ic.REUSE_KINDS}
    assert all(len(v) == 6 for v in kinds.values())
    rng = np.random.default_rng(11)
    order = rng.permutation(np.arange(n) % len(ic.REUSE_KINDS))
    cases = [kinds[ic.REUSE_KINDS[k]][i % 6] for i, k in enumerate(order)]
    followed = {(int(order[i]), int(order[i + grid])) for i in range(n - grid)}
    assert len(followed) == len(ic.REUSE_KINDS) ** 2
    run(inf, cases, "wave reuse")


def test_nothing_written_outside_a_members_output(inf, groups):
    """A launch of stored members of 0xA5 fills out[0, N); the device output
    buffer persists, so after a second launch that places every valid and
    invalid member with gaps of 1-67 bytes, every gap byte and the 16 bytes at
    either end are still 0xA5: a member, failing or not, writes only its own
    [out_off, out_off + isize)."""
    from tests.deflate_builder import Stream
    cases = [c for g in ic.VALID_GROUPS for c in groups[g]]
    bad = groups["invalid"]
    step = len(cases) // len(bad)
    for i, c in enumerate(bad):                      # spread the invalid ones among the valid
        cases.insert(1 + i * (step + 1), c)
    out_offs, o = [], 16
    for i, c in enumerate(cases):
        out_offs.append(o)
        o += c.isize + 1 + (i * 13) % 67
    n = out_offs[-1] + cases[-1].isize + 16
    # first launch: 0xA5 over [0, n)
    fill = []
    for p in range(0, n, 65535):
        k = min(65535, n - p)
        s = Stream()
        s.stored(b"\xa5" * k, final=True)
        fill.append(ic.Case(f"fill_{p}", s.getvalue(), b"\xa5" * k))
    _, out = run(inf, fill, "fill")
    assert len(out) == n and out.tobytes() == b"\xa5" * n
    # second launch, the same out_bytes
    buf, m, nn = lay_out(cases, out_offs=out_offs, out_bytes=n)
    assert nn == n
    rc, out = launch(inf, buf, m, n)
    check(cases, m, rc, out, "gaps")
    own = np.zeros(n, bool)
    for c, oo in zip(cases, out_offs):
        own[oo:oo + c.isize] = True
    assert not own[:16].any() and not own[-16:].any()
    gaps = np.asarray(out)[~own]
    assert len(gaps) >= 32 + len(cases) - 1
    wrong = np.flatnonzero(gaps != 0xA5)
    assert len(wrong) == 0, ("bytes outside every member's output changed", np.flatnonzero(~own)[wrong][:8])
