"""Named inputs for the BGZF block compressor (csrc/dcr_deflate.h, k_deflate):
each is one block of at most 0xff00 bytes (STREAMS: many blocks) built from a
seeded generator, with the property it claims, which `claim(member, block)`
asserts on the emulation's member and on what tests/deflate_reader.py reads
back from it.  tests/test_deflate_cases.py checks the claims on the CPU;
tests/test_gpu_deflate_blocks.py runs the same list through the kernel.

What the code cannot reach, whatever the input (asserted over all cases in
test_deflate_cases.py):
  - kMaxDeflate (65,510 deflate bytes): a block is stored as soon as its
    deflate bytes exceed n + 5 <= 65,285.
  - match length 258 / length symbol 285, and length 3 / symbol 257: a lane
    parses a sub-block of ceil(n / 256) <= 255 bytes, matches end at its end,
    and the parse takes no match shorter than 4.
  - a stored block with dbytes == n + 6 can be told from one with more only by
    its neighbour: both are n + 31 bytes (see stored_edge_*)."""
from dataclasses import dataclass, field

import numpy as np

from tests import deflate_reader as dr
from tests.test_deflate_emulation import record_text

N = 0xff00
STAGE = 57344           # sizeof(Shared::stage): a member of at most this many bytes is assembled in LDS


@dataclass
class Case:
    name: str
    data: bytes
    claims: list = field(default_factory=list)      # callables (member, block), each asserts
    says: str = ""

    def claim(self, member, block):
        for f in self.claims:
            f(member, block)


_MEMBERS = {}


def member(data):
    """dcr_deflate_emulate's member of one block, computed once per content."""
    from duplexumiconsensusreads_amd import native_io
    if data not in _MEMBERS:
        _MEMBERS[data] = native_io.deflate_emulate(data)
    return _MEMBERS[data]


# ---- contents ---------------------------------------------------------------------
def text4(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def noise(n, seed, alphabet=256, base=0):
    return (np.random.default_rng(seed).integers(0, alphabet, n, dtype=np.int64) + base).astype(np.uint8).tobytes()


def noise_then_zeros(seed, alphabet, L, n=N):
    """The first L bytes of one noise sequence per (seed, alphabet), zeros up to n."""
    return noise(n, seed, alphabet)[:L] + bytes(n - L)


# ---- claims -----------------------------------------------------------------------
def stored(m, b):
    assert b.stored and len(m) == len(b.out) + 31, (b.btype, len(m))


def dynamic(m, b):
    assert b.btype == 2, b.btype


def size_is(want):
    def f(m, b):
        assert len(m) == want, (len(m), want)
    return f


def global_path(m, b):       # dynamic and too large for stage[]: BitOut into the slot, atomic-or stitching
    assert b.btype == 2 and len(m) > STAGE, (b.btype, len(m))


def staged_path(m, b):
    assert b.btype == 2 and len(m) <= STAGE, (b.btype, len(m))


def header_has(sym, extra=None):
    def f(m, b):
        assert any(s == sym and (extra is None or e == extra) for s, e in b.header), (sym, extra, b.header)
    return f


def no_far_distance(m, b):
    assert all(d <= 32768 for _, d in b.matches())


def has_distance(d):
    def f(m, b):
        assert any(dd == d for _, dd in b.matches()), sorted({dd for _, dd in b.matches()})[-5:]
    return f


def lacks_distance(d):
    def f(m, b):
        assert all(dd != d for _, dd in b.matches())
    return f


def has_match(length, distance):
    def f(m, b):
        assert (length, distance) in b.matches(), (length, distance)
    return f


def longest_match(want):
    def f(m, b):
        assert max(l for l, _ in b.matches()) == want
    return f


def max_lit_len(want):
    def f(m, b):
        assert max(b.lit_len) == want, max(b.lit_len)
    return f


def max_cl_len(want):
    def f(m, b):
        assert max(b.cl_len) == want, b.cl_len
    return f


def no_match(m, b):          # HDIST = 0 and the lone distance code of one bit (p3c_assign, m_dist == 0)
    assert b.btype == 2 and not b.matches() and b.hdist == 0 and b.dist_len == [1], (b.hdist, b.dist_len)


def dist_syms_are(want):
    def f(m, b):
        assert b.dist_syms == set(want), sorted(b.dist_syms)
    return f


def len_syms_cover(want):
    def f(m, b):
        assert b.len_syms >= set(want), sorted(set(want) - b.len_syms)
    return f


# ---- the cases ----------------------------------------------------------------------
CASES = []


def add(name, data, *claims, says=""):
    assert 0 < len(data) <= N, name
    CASES.append(Case(name, bytes(data), list(claims), says))


# paths
for a in (150, 200, 240):
    add(f"global_{a}", noise(N, a, a), global_path, says="dynamic, member above 57,344 bytes: the global BitOut path")
add("stored_full", noise(N, 256, 256), stored, size_is(N + 31))
add("staged_noise", noise(N, 128, 128), staged_path, says="the largest staged members: BitOut2 and p6_copy near full")
add("noise_then_zeros", noise(N - 300, 7, 256) + bytes(300), global_path)

# The two boundaries, found by bisecting L with the emulation (noise_then_zeros(seed, alphabet, L)); the sizes
# these constants give are asserted.  Both sides of use_stage are hit exactly.
STAGE_EDGE = dict(seed=11, alphabet=140, last_staged_L=63931, first_global_L=63932)
# dbytes = len(member) - 26 == n + 5 is the largest block kept compressed.  A stored block holds n + 5 deflate
# bytes too, so both members are n + 31 bytes; the stored one is the same noise one byte longer (every byte
# added one byte to the member up to there), so its dynamic form would have been n + 6, which no output shows.
STORED_EDGE = dict(seed=12, alphabet=256, kept_L=65225, stored_L=65226)
add("stage_last", noise_then_zeros(STAGE_EDGE["seed"], STAGE_EDGE["alphabet"], STAGE_EDGE["last_staged_L"]),
    staged_path, size_is(STAGE), says="57,344 bytes: the last size assembled in stage[]")
add("stage_first_global", noise_then_zeros(STAGE_EDGE["seed"], STAGE_EDGE["alphabet"], STAGE_EDGE["first_global_L"]),
    global_path, size_is(STAGE + 1), says="57,345 bytes: the first size written straight to the slot")
add("stored_edge_keep", noise_then_zeros(STORED_EDGE["seed"], STORED_EDGE["alphabet"], STORED_EDGE["kept_L"]),
    global_path, size_is(N + 31), says="dbytes == n + 5 stays compressed")
add("stored_edge_drop", noise_then_zeros(STORED_EDGE["seed"], STORED_EDGE["alphabet"], STORED_EDGE["stored_L"]),
    stored, size_is(N + 31), says="one noise byte more: stored")

# sizes: lane_range with n < 256 (empty lanes), n just over a multiple of 256, n % 16 != 0 (the staging
# tail mask), the largest blocks
SIZES = list(range(1, 10)) + [15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 4097, N - 17, N - 3, N - 1, N]
for n in SIZES:
    small = [stored] if n <= 5 else []
    add(f"text_{n}", text4(n, n), *small)
    add(f"zeros_{n}", bytes(n), *small, *([dynamic, size_is(39)] if n == 8 else []),
        *([dynamic, size_is(70)] if n in (255, 256, 257) else []))
    add(f"random_{n}", noise(n, n), *small, *([stored] if n in (255, 256, 257) else []))


# matches
def _period(p, n=N, seed=0):
    unit = noise(p, 1000 + p + seed, 26, 65)
    while len(set(unit)) < min(p, 2):        # a unit of one repeated value has a shorter period
        seed += 1
        unit = noise(p, 1000 + p + seed, 26, 65)
    return (unit * (n // p + 1))[:n]


for p in (1, 2, 3, 4, 5):
    # every sub-block of 255 bytes: at most one literal, then one match of the distance p that runs to its end
    add(f"run_period_{p}", _period(p), dynamic, has_distance(p), longest_match(255),
        says="distance 1..4 candidates / the lane's table; the longest match there is, 255")
add("run_period_300", _period(300), dynamic, has_distance(300),
    says="a long match cut at every sub-block end (255 bytes)")


def _all_lengths():
    """6-bit noise; in lane 3 + i's sub-block a run of LEN + 1 equal bytes >= 64 (a literal, then a match of
    distance 1 and exactly LEN) for the first and the last length of every length symbol 258..284."""
    d = bytearray(noise(N, 21, 64))
    lens = []
    for i in range(1, 28):                   # symbols 258 .. 284
        lo = dr.LEN_BASE[i]
        hi = min(dr.LEN_BASE[i] + (1 << dr.LEN_EXTRA[i]) - 1, 250)
        lens += [lo] if hi == lo else [lo, hi]
    for k, L in enumerate(lens):
        at = 255 * (3 + k) + 2
        d[at:at + L + 1] = bytes([64 + k]) * (L + 1)
    return bytes(d), lens


_d, _lens = _all_lengths()
add("all_length_symbols", _d, dynamic, len_syms_cover(range(258, 285)), *[has_match(L, 1) for L in _lens],
    says="every length symbol the parse can emit, 258..284, first and last length of each")


def _far(d, at=100, n=N, plen=200, seed=31):
    x = bytearray(noise(n, seed, 64))
    pat = noise(plen, seed + 1, 192, 64)
    x[at:at + plen] = pat
    x[at + d:at + d + plen] = pat
    assert len(x) == n
    return bytes(x)


# A 200-byte pattern at 100 and again at 100 + d.  The copy lies in the second 32 KiB half, where the block-wide
# candidates are the earliest second-half position and the latest first-half position with the same hash: about
# 16 noise positions share each of the 2,048 hashes, so the pattern at 100 is not a candidate and no match of
# distance d is made (asserted).  dist_*_late put the pattern at the end of the first half instead, where it is
# the latest position of its hashes: 32,768 is used, 32,769 must not be.
for d in (32767, 32768, 32769, 40000):
    add(f"dist_{d}", _far(d), dynamic, no_far_distance, lacks_distance(d))
add("dist_32767_late", _far(32767, at=32256), dynamic, no_far_distance, has_distance(32767))
add("dist_32768_late", _far(32768, at=32256), dynamic, no_far_distance, has_distance(32768))
add("dist_32769_late", _far(32769, at=32256), dynamic, no_far_distance, lacks_distance(32769))

for k in range(1, 41):
    add(f"text_then_{k}_zeros", text4(1000 + 7 * k, k) + bytes(k), dynamic,
        says="match_len runs from the last bytes into the zero padding; only lim stops it")
for n in (1100, 4111, N - 5):
    add(f"zeros_to_end_{n}", text4(37, n) + bytes(n - 37), dynamic, has_distance(1))


# codes and header
add("two_values", (np.random.default_rng(41).integers(0, 2, N) * 255).astype(np.uint8).tobytes(), dynamic,
    header_has(18, 127), says="literal lengths 1..254 unused: symbol 18 with a run of 138")


def _flat_literals():
    rng = np.random.default_rng(42)
    body = b"".join(rng.permutation(256).astype(np.uint8).tobytes() for _ in range(16))
    return body + bytes(3000)


# 256 equiprobable literals and nothing else cannot stay dynamic (8 bits a byte and the header exceed n + 5),
# so a zero run pays for the header: one more literal zero and a few matches, the literal code stays flat
add("flat_literals", _flat_literals(), dynamic, header_has(16),
    says="every literal present and equally frequent: repeat-previous (16) runs in the header")


def _weighted(weights, n, seed):
    rng = np.random.default_rng(seed)
    w = np.asarray(weights, np.float64)
    cnt = np.maximum(1, np.floor(w / w.sum() * n)).astype(np.int64)
    vals = rng.permutation(256)[:len(w)]
    x = np.repeat(vals, cnt)[:n]
    return rng.permutation(x).astype(np.uint8).tobytes()


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


# Fibonacci weights scaled to the block, every weight below one byte counted as one: the shuffled bytes make
# some 13,000 matches, which flatten the code, and 22 weights stop at 14 bits; 30 reach 15, 36 also the 7-bit
# limit of the code-length code
add("fibonacci", _weighted(_fib(30), N, 43), dynamic, max_lit_len(15),
    says="a literal/length code at the 15-bit limit")
add("fibonacci_cl7", _weighted(_fib(36), N, 43), dynamic, max_lit_len(15), max_cl_len(7),
    says="... and a code-length code at the 7-bit limit")
add("no_match_64", noise(4096, 45, 64, 32), no_match, says="no match in a dynamic block: HDIST = 0, one 1-bit code")
add("one_distance_symbol", bytes([7]) * 5000, dynamic, dist_syms_are({0}))


def _all_distances():
    """Distances 65 and up: 16-byte patterns of bytes >= 64 at the block's start, where they are the earliest
    positions of their hashes (a_min), each copied (first distance of its symbol) + 1 later, the farthest
    first so that no copy lands on a pattern.  Distances 1 to 49: a stretch of that period (the lane's table)."""
    rng = np.random.default_rng(45)
    n = 30000
    x = bytearray(noise(n, 46, 64))
    for k in range(12, 30):
        s, d = 16 * (29 - k), dr.DIST_BASE[k] + 1
        pat = noise(16, 500 + k, 192, 64)
        x[s:s + 16] = pat
        x[s + d:s + d + 16] = pat
    at = 26000
    for k in range(0, 12):
        p = dr.DIST_BASE[k]
        unit = bytes(rng.permutation(192)[:p].astype(np.uint8) + 64)
        L = 3 * p + 24
        x[at:at + L] = (unit * (L // p + 1))[:L]
        at += L + 8
    assert len(x) == n
    return bytes(x)


add("all_distance_symbols", _all_distances(), dynamic, dist_syms_are(range(30)))


# ---- multi-block streams ------------------------------------------------------------------
def _cycle(c):
    return [noise(N, 7000 + c, 200), noise(N, 7100 + c, 256), bytes(N), record_text(N, 7200 + c),
            noise(N, 7300 + c, 128)]


_BODY = b"".join(b"".join(_cycle(c)) for c in range(8))       # 40 full blocks
STREAMS = {
    "cycle_then_7": _BODY + text4(7, 71),
    "cycle_then_257": _BODY + text4(257, 72),
}


def blocks_of(stream):
    return [stream[i:i + N] for i in range(0, len(stream), N)]
