"""The named compressor inputs of tests/deflate_cases.py on the host emulation
(dcr_deflate_emulate): every block gives one valid BGZF member, the plain
reader (tests/deflate_reader.py) agrees with zlib on it, and the case reaches
the edge it is named for: the path (stored, staged in LDS, written straight
to the slot), the member sizes at the two boundaries, code lengths of 15 and
7 bits, the header's run-length symbols, the distance limit, HDIST = 0.  A
change of the parse that moves a case off its edge fails here, on the CPU;
tests/test_gpu_deflate_blocks.py holds the kernel to the same members."""
import zlib

import pytest

from tests import deflate_cases as dc
from tests import deflate_reader as dr
from tests.test_deflate_emulation import check_member

_BLOCKS = {}


def read(data):
    if data not in _BLOCKS:
        _BLOCKS[data] = dr.read_member(dc.member(data))
    return _BLOCKS[data]


def check_block(data):
    m = dc.member(data)
    check_member(m, data)
    b = read(data)
    assert b.out == zlib.decompress(m[18:-8], -15) == data
    assert b.bfinal == 1
    return m, b


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_is_valid_and_on_its_edge(case):
    m, b = check_block(case.data)
    case.claim(m, b)


def test_case_names_are_unique():
    names = [c.name for c in dc.CASES]
    assert len(names) == len(set(names))


def test_boundary_constants_give_the_stated_sizes():
    s = dc.STAGE_EDGE
    size = lambda L: len(dc.member(dc.noise_then_zeros(s["seed"], s["alphabet"], L)))      # noqa: E731
    assert size(s["last_staged_L"]) == dc.STAGE == 57344
    assert size(s["first_global_L"]) == dc.STAGE + 1
    s = dc.STORED_EDGE
    kept = dc.member(dc.noise_then_zeros(s["seed"], s["alphabet"], s["kept_L"]))
    drop = dc.member(dc.noise_then_zeros(s["seed"], s["alphabet"], s["stored_L"]))
    assert len(kept) - 26 == dc.N + 5 and kept[18] & 7 == 5          # BFINAL, dynamic
    assert len(drop) - 26 == dc.N + 5 and drop[18] & 7 == 1          # BFINAL, stored
    assert s["stored_L"] == s["kept_L"] + 1
    # one member byte per noise byte up to the edge: the next would have been n + 6
    before = dc.member(dc.noise_then_zeros(s["seed"], s["alphabet"], s["kept_L"] - 1))
    assert len(before) == len(kept) - 1


def test_every_path_is_among_the_cases():
    kinds = {"stored": 0, "staged": 0, "global": 0}
    for c in dc.CASES:
        m, b = dc.member(c.data), read(c.data)
        kinds["stored" if b.stored else "staged" if len(m) <= dc.STAGE else "global"] += 1
    assert kinds["stored"] >= 20 and kinds["staged"] >= 60 and kinds["global"] >= 6, kinds


def test_what_no_input_reaches():
    """Lanes parse sub-blocks of at most 255 bytes and take no match under 4
    bytes: no length 3 (symbol 257) and none above 255 (symbol 285 = 258);
    no distance above 32,768; no member near kMaxDeflate + 26."""
    for c in dc.CASES:
        b = read(c.data)
        if not b.stored:
            assert all(4 <= l <= 255 and 1 <= d <= 32768 for l, d in b.matches()), c.name
        assert len(dc.member(c.data)) <= dc.N + 31, c.name


@pytest.mark.parametrize("name", list(dc.STREAMS))
def test_stream_blocks(name):
    blocks = dc.blocks_of(dc.STREAMS[name])
    assert len(blocks) == 41 and all(len(x) == dc.N for x in blocks[:-1])
    assert len(blocks[-1]) == {"cycle_then_7": 7, "cycle_then_257": 257}[name]
    kinds = []
    for data in blocks:
        m, b = check_block(data)
        kinds.append("stored" if b.stored else "staged" if len(m) <= dc.STAGE else "global")
    # large and incompressible next to small and compressible, eight times over
    assert kinds[:40] == ["global", "stored", "staged", "staged", "staged"] * 8
    sizes = [len(dc.member(x)) for x in blocks[:5]]
    assert sizes[2] < 300 and sizes[3] < 30000 and sizes[4] > 57000, sizes
