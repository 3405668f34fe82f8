"""``k_deflate`` (csrc/dcr_writer.hip, csrc/dcr_deflate.h) alone on the named
blocks of tests/deflate_cases.py, through the test entry
``dcr_deflate_blocks`` of libdcr.so: the input padded with 0xff to 16 bytes,
every slot and a guard slot behind the last pre-filled, the grid capped and
the block-claim counter switched on request.  Record streams compress about
threefold and never take the stored block, the bit writer into global memory
(members above 57,344 bytes), blocks under 256 bytes or code lengths at their
limits; these do (tests/test_deflate_cases.py proves it on the CPU).  Every
member is a valid BGZF block that zlib inflates to the input, equals the host
emulation's (``dcr_deflate_emulate``) byte for byte, and nothing is written
behind it."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc

pytestmark = pytest.mark.gpu

FILL = 0xA7
SLOT = 65536


@pytest.fixture(scope="module")
def ctx():
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.params import ConsensusParams
    c = _lib.Context(ConsensusParams(), device=0)
    fn = _lib.load().dcr_deflate_blocks
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p]
    yield c
    c.close()


def deflate(ctx, data, max_wg=0, claim=False):
    """(slots [blocks + 1, 65536], sizes [blocks]) of one launch.  A HIP
    runtime error ends the session: nothing more is started on a device that
    has faulted."""
    from duplexumiconsensusreads_amd import _lib
    nb = (len(data) + dc.N - 1) // dc.N
    src = np.frombuffer(data, np.uint8)
    slots = np.zeros((nb + 1, SLOT), np.uint8)
    sizes = np.zeros(nb, np.int64)
    rc = _lib.load().dcr_deflate_blocks(ctx._ctx, src.ctypes.data, len(data), max_wg, int(claim), FILL,
                                        slots.ctypes.data, sizes.ctypes.data)
    if rc:
        pytest.exit(f"device runtime error, session ended: {_lib.load().dcr_last_error().decode()}", 1)
    return slots, sizes


def check_slot(slot, size, data, label):
    want = dc.member(data)
    assert 26 < size <= SLOT, (label, size)
    got = slot[:size].tobytes()
    assert size == struct.unpack_from("<H", got, 16)[0] + 1, label                     # 1: BSIZE + 1
    assert got[:16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", label           # 2: the BGZF header
    assert zlib.decompress(got[18:-8], -15) == data, label                             # 3
    assert struct.unpack_from("<II", got, size - 8) == (zlib.crc32(data), len(data)), label    # 4: CRC32, ISIZE
    if got != want:                                                                     # 5: the emulation's member
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError(f"{label}: member differs from the emulation's: {len(got)} bytes against "
                             f"{len(want)}, first at {at}")
    rest = slot[4 * ((size + 3) // 4):]                                                 # 6: nothing behind it
    stray = np.flatnonzero(rest != FILL)
    assert not len(stray), (f"{label}: {len(stray)} bytes written behind the member of {size} bytes, the first at "
                            f"{4 * ((size + 3) // 4) + int(stray[0])} = {int(rest[stray[0]]):#x}, the last at "
                            f"{4 * ((size + 3) // 4) + int(stray[-1])}")


def check_run(slots, sizes, blocks, label):
    assert len(sizes) == len(blocks)
    for i, data in enumerate(blocks):
        check_slot(slots[i], int(sizes[i]), data, f"{label} block {i}")
    assert (slots[len(blocks)] == FILL).all(), f"{label}: guard slot written"            # 7


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_block(ctx, case):
    slots, sizes = deflate(ctx, case.data)
    check_run(slots, sizes, [case.data], case.name)


@pytest.mark.parametrize("name", list(dc.STREAMS))
def test_stream_on_every_grid(ctx, name):
    """One workgroup takes every block in turn (cap 1), two alternate, the
    default grid takes one each; fixed stride and claim counter: the same
    slots, each right.  With one workgroup a 7-byte block follows 40 full ones
    on the same LDS: stage[] (a union with the hash tables), the padding of
    in[] and the token buffer are what the block before left."""
    stream = dc.STREAMS[name]
    blocks = dc.blocks_of(stream)
    first = None
    for max_wg in (1, 2, 0):
        for claim in (False, True):
            label = f"{name} cap {max_wg} claim {claim}"
            slots, sizes = deflate(ctx, stream, max_wg, claim)
            check_run(slots, sizes, blocks, label)
            if first is None:
                first = (slots, sizes)
            else:
                assert np.array_equal(sizes, first[1]), label
                assert np.array_equal(slots, first[0]), label
