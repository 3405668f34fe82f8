"""The smallest and the awkward batch sizes through all three entry points of
one context (dcr_submit_write, dcr_submit, dcr_run_batch_host), in an order
that shows every device-buffer planner an empty batch before anything was
allocated, then minimal, grown and shrunk buffers: an empty batch (E), one
family (B) and 299 families (A), run as E, B, A, B, E, A.  Both streams
rotate over the context's slots 0 and 1.  Per batch the device writer's record
stream must equal the host writer's over the plain path's outputs, and the
host-pointer path must equal the C oracle."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from duplexumiconsensusreads_amd import native_io, synth
from duplexumiconsensusreads_amd.params import ConsensusParams

pytestmark = pytest.mark.gpu

SCALARS = ("status", "pos", "mapq", "len", "n_cig", "n_de", "D", "M", "E")


def members(blob):
    """Split concatenated BGZF blocks; check each one; return the data."""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", blob, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", blob, p + bsize - 8)
        data = zlib.decompress(blob[p + 18:p + bsize - 8], -15)
        assert len(data) == isize and zlib.crc32(data) == crc
        out.append(data)
        p += bsize
    return b"".join(out)


def one_batch(path, params, min_reads):
    ing = native_io.Ingest(path, params.min_map_quality, min_reads, params.max_reads, params.min_base_quality)
    hb = native_io.HostBatch(reads=50_000, side_bytes=1 << 24)
    ing.next(hb)
    assert hb.end_kind == native_io.END_EOF, "the whole file is one batch"
    ing.close()
    return hb


def test_empty_minimal_grown_and_shrunk_batches(tmp_path):
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    from oracle import dcr_oracle_c
    params = ConsensusParams()
    paths = {}
    for n in (1, 300):
        paths[n] = str(tmp_path / f"in{n}.bam")
        synth.write_config_bam(paths[n], synth.SynthConfig("t", n, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                           softclip_frac=0.3))
    hbs = {"B": one_batch(paths[1], params, params.min_reads), "A": one_batch(paths[300], params, params.min_reads),
           "E": one_batch(paths[300], params, 1000)}
    sizes = {k: (hb.n_fam, hb.s.n_reads, hb.s.n_bases) for k, hb in hbs.items()}
    assert sizes == {"B": (1, 27, 4050), "A": (299, 5900, 885000), "E": (0, 0, 0)}
    oracle = {k: dcr_oracle_c.run(hb.packed(), params) for k, hb in hbs.items()}

    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    host = DeviceStream(ctx, device_writer=False)
    for step, k in enumerate("EBABEA"):
        hb = hbs[k]
        F = hb.n_fam
        # device writer
        res = dev.result(dev.submit(hb))
        got = members(res.bgzf.tobytes())
        fam_fail, ds_len = res.fam_fail.copy(), res.ds_len.copy()
        # plain path, then the host writer over its outputs
        slot = host.next_slot
        ss, ds, rs = host.result(host.submit(hb))
        assert native_io.first_failure(hb, ss, ds, F, rs)[0] == F, (step, k)
        out = str(tmp_path / f"host_{step}.bam")
        w = native_io.BgzfWriter(out, b"")
        w.write_consensus(hb, ss, ds, F)
        w.close()
        want = gzip.decompress(open(out, "rb").read())
        assert got == want, (step, k)
        assert res.record_bytes == len(want), (step, k)
        assert not fam_fail.any(), (step, k)
        assert np.array_equal(ds_len, host.outs[slot].arr["ds"]["len"][:2 * F]), (step, k)
        if F == 0:
            # k_compact writes zero totals for an empty stream
            assert want == b"" and res.record_bytes == 0 and res.bgzf_bytes == 0, (step, k)
        # host-pointer path against the oracle, as smoke() compares them
        packed = hb.packed()
        ss_g, ds_g, _ = ctx.run_host(packed)
        ss_o, ds_o, _ = oracle[k]
        for name, col_off, a, b in (("ss", packed.ss_col_off, ss_g, ss_o), ("ds", packed.ds_col_off, ds_g, ds_o)):
            for f in SCALARS:
                assert np.array_equal(getattr(a, f), getattr(b, f)), (step, k, name, f)
            for i in range(a.n_rec):
                if a.status[i] == 0:
                    assert a.record(i, col_off) == b.record(i, col_off), (step, k, name, i)
    dev.close()
    host.close()
    ctx.close()
