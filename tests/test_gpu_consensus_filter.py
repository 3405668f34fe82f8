"""The consensus filters on the GPU (dcr_set_filter: k_filter, then k_fmt_size /
k_fmt_size_ss skipping the dropped families) against the host path
(dcr_fmt_filter and the host formatter's masked entries over the kernel
outputs of dcr_submit) on the same batches, byte for byte: record bytes, BGZF
members and fam_filt, for the duplex stream and the single-strand stream; and
``--filter_*`` through the GPU CLI against the model (tests/filter_model.py)
over the reference's records."""
import gzip

import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, native_io, synth
from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from duplexumiconsensusreads_amd.records import AlignedSegment
from tests import filter_model as fm
from tests.test_consensus_filter import FILTERS, WANT_DS, WANT_SS, summary_lines
from tests.test_gpu_writer import members
from tests.test_ss_output import DEFAULT, assert_records, failing_input, records, run, side_files, write_bam

pytestmark = pytest.mark.gpu


def batches(path, params, reads, ss_meta):
    ing = native_io.Ingest(path, params.min_map_quality, params.min_reads, params.max_reads,
                           params.min_base_quality, ss_meta=ss_meta)
    while True:
        hb = native_io.HostBatch(reads=reads, side_bytes=1 << 24, ss_meta=ss_meta)
        ing.next(hb)
        yield hb
        if hb.end_kind != native_io.END_FULL:
            break
    ing.close()


def host_streams(tmp_path, hb, ss, ds, n_fam, fam_filt, ss_output):
    """The host formatter's record bytes of the kept families of [0, n_fam):
    (duplex, single-strand or None)."""
    out = []
    for k in range(2 if ss_output else 1):
        path = str(tmp_path / f"host{k}.bam")
        w = native_io.BgzfWriter(path, b"")
        if k == 0:
            w.write_consensus(hb, ss, ds, n_fam, fam_filt)
        else:
            w.write_consensus_ss(hb, ss, n_fam, fam_filt)
        w.close()
        out.append(gzip.decompress(open(path, "rb").read()))
    return out[0], out[1] if ss_output else None


def check_stream(blocks, fetched, want, n_blocks, n_record_bytes):
    got = members(blocks)                                   # checks every member's CRC32 and ISIZE
    assert len(got) == n_record_bytes
    assert got == want
    assert fetched == want
    emu = b"".join(native_io.deflate_emulate(fetched[i:i + 0xff00]) for i in range(0, len(fetched), 0xff00))
    assert emu == blocks
    assert n_blocks == -(-len(want) // 0xff00)


def check_batches(tmp_path, path, params, reads, flt, ss_output, n_slots=2):
    """Every batch of ``path`` through the filtering device writer and through
    dcr_submit + the host filter and formatter; returns the batches' fam_filt."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter = ss_output, flt
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = ss_output
    seen = []
    for hb in batches(path, params, reads, ss_output):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        assert not res.fam_fail.any(), "these inputs have no failing family"
        fetched = res.record_bytes_of(F).tobytes()          # before the slot is submitted again
        blocks, fam_filt = res.bgzf.tobytes(), res.fam_filt.copy()
        if ss_output:
            ss_fetched, ss_blocks = res.ss_record_bytes_of(F).tobytes(), res.ss_bgzf.tobytes()
        ss, ds, rs = host.result(host.submit(hb))
        assert native_io.first_failure(hb, ss, ds, F, rs)[0] == F
        want_filt = native_io.apply_filter(hb, ss, ds, flt, F)      # masks the host copies in place
        assert np.array_equal(fam_filt, want_filt)
        want, want_ss = host_streams(tmp_path, hb, ss, ds, F, want_filt, ss_output)
        check_stream(blocks, fetched, want, res.blocks, res.record_bytes)
        if ss_output:
            check_stream(ss_blocks, ss_fetched, want_ss, res.ss_blocks, res.ss_record_bytes)
        seen.append(fam_filt)
    dev.close()
    host.close()
    ctx.close()
    return seen


# one masked base in 150 stays under both bounds, three do not
SYNTH_FILTER = ConsensusFilter(min_base_quality=60, min_reads=(8, 4, 2), max_read_error_rate=(0.03, 0.25),
                               max_no_call_fraction=0.02, min_mean_base_quality=59.0)


@pytest.mark.parametrize("kind,ss_output", [("c1", False), ("indel_clip", True)])
def test_device_streams_are_the_host_paths(tmp_path, kind, ss_output):
    path = str(tmp_path / "in.bam")
    cfg = synth.SynthConfig("t", 400, sub_size="poisson5", seed=9,
                            indel_frac=0.3 if kind == "indel_clip" else 0.0,
                            softclip_frac=0.3 if kind == "indel_clip" else 0.0)
    synth.write_config_bam(path, cfg)
    seen = check_batches(tmp_path, path, ConsensusParams(), 2000, SYNTH_FILTER, ss_output)
    assert len(seen) > 2                                    # several batches: both slots are reused
    words = np.concatenate(seen)
    assert 390 <= len(words) <= 400
    kept = (words & 0xff) == 0
    assert kept.any() and (~kept).any() and (words[kept] >> 8).sum() > 0
    assert all(((words & b) != 0).any() for b in (1, 2, 4, 8))


def test_every_base_masked_meets_the_bounds_exactly(tmp_path):
    """Q above every quality masks every base: all 'N' at quality <= 2.  A
    no-call bound of 1.0 and a mean-quality bound at the masked mean are then
    met with equality; the records with a quality below 2 miss the second."""
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 400, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                   softclip_frac=0.3))
    flt = ConsensusFilter(min_base_quality=61, max_no_call_fraction=1.0, min_mean_base_quality=2.0)
    words = np.concatenate(check_batches(tmp_path, path, ConsensusParams(), 2000, flt, False))
    assert ((words & 0xff) == 0).sum() > 300 and set(np.unique(words & 0xff)) == {0, 8}


# ---- edge shapes: duplex lengths around the 64-lane dword stride (a wave covers
# 256 bases per step) and the partial last word; dropped families first, last
# and on both sides of a kept one
EDGE_LEN = [1, 63, 64, 65, 150, 151, 300]
EDGE_SMALL = [True, False, True, False, False, False, True]     # one read per subfamily: dropped by min_reads


def edge_bam(path):
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    hdr = BamHeader("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])
    with AlignmentFile(path, "wb", header=hdr) as out:
        for f, (L, small) in enumerate(zip(EDGE_LEN, EDGE_SMALL)):
            ins = L + 40
            tmpl = acgt[rng.integers(0, 4, ins + 8)]
            P = 10_000 + 1_000 * f
            spec = [(99, "A", 0), (163, "B", 0), (83, "B", ins - L), (147, "A", ins - L)]    # A1 B2 B1 A2
            for k, (flag, strand, start) in enumerate(spec):
                for j in range(1 if small else 2):
                    r = AlignedSegment()
                    r.query_name = f"e{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = P + start
                    r.mapping_quality = 20 + (7 * j + k) % 41
                    r.cigartuples = [(0, L)]
                    seq = tmpl[start:start + L].copy()
                    if j == 1:                        # the second read dissents: columns of low consensus quality
                        seq[(k + 2) % 5::5] = acgt[(np.searchsorted(acgt, seq[(k + 2) % 5::5]) + 1) % 4]
                    r.query_sequence = seq.tobytes().decode()
                    # qualities 20..39 in a pattern that differs between reads and is no multiple of 4 long
                    r.query_qualities = [20 + (3 * i + 5 * j + k) % 20 if i % 7 else 37 for i in range(L)]
                    r.set_tags([("MI", f"{f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)
    return path


def test_edge_shapes(tmp_path):
    path = edge_bam(str(tmp_path / "edge.bam"))
    params = ConsensusParams()
    # the duplex qualities of this input, to put the masking bound inside them
    from oracle import dcr_oracle_c
    hb = next(iter(batches(path, params, 1 << 12, True)))
    assert hb.n_fam == len(EDGE_LEN)
    _, ds, _ = dcr_oracle_c.run(hb.packed(), params)
    assert ds.len.tolist() == [L for L in EDGE_LEN for _ in range(2)]
    quals = np.concatenate([ds.qual[int(o):int(o) + int(n)] for o, n in zip(hb.a["ds_col_off"], ds.len)])
    Q = int(np.median(quals))
    assert quals.min() < Q <= quals.max()
    flt = ConsensusFilter(min_base_quality=Q, min_reads=(3, 1, 1))
    (words,) = check_batches(tmp_path, path, params, 1 << 12, flt, True)
    assert [bool(w & 0xff) for w in words] == EDGE_SMALL
    masked = [int(w) >> 8 for w in words]
    assert all(0 < m < 2 * L for m, L in zip(masked[1:], EDGE_LEN[1:])) and masked[0] in (0, 1, 2)


def test_a_batch_with_every_family_dropped_then_the_slot_again(tmp_path):
    """An empty record stream: zero blocks through the scans, k_deflate,
    k_compact, the wait, the slot fetches and the BGZF writer; then the same
    slot takes a batch whose filter keeps everything."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 120, sub_size="poisson5", seed=5))
    params = ConsensusParams()
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=1, device_writer=True)
    dev.ss_output = True
    hb = next(iter(batches(path, params, 1 << 16, True)))
    F = hb.n_fam
    assert F == 120
    res = dev.result(dev.submit(hb))                        # no filter: the reference point
    assert res.fam_filt is None
    want = (res.bgzf.tobytes(), res.ss_bgzf.tobytes(), res.record_bytes, res.ss_record_bytes)
    assert want[2] > 0xff00
    dev.filter = ConsensusFilter(min_reads=(1000, 1, 1))
    res = dev.result(dev.submit(hb))
    assert ((res.fam_filt & 0xff) == 1).all() and not res.fam_fail.any()
    assert (res.bgzf_bytes, res.record_bytes, res.blocks) == (0, 0, 0)
    assert (res.ss_bgzf_bytes, res.ss_record_bytes, res.ss_blocks) == (0, 0, 0)
    assert len(res.record_bytes_of(F)) == 0 and len(res.ss_record_bytes_of(F)) == 0
    out = str(tmp_path / "empty.bam")
    w = native_io.BgzfWriter(out, b"BAM\1")
    w.put_blocks(res.bgzf, res.record_bytes)
    w.close()
    assert gzip.decompress(open(out, "rb").read()) == b"BAM\1"
    dev.filter = ConsensusFilter(min_reads=(1, 1, 1), max_read_error_rate=(1.0, 1.0))
    res = dev.result(dev.submit(hb))
    assert not res.fam_filt.any()
    assert (res.bgzf.tobytes(), res.ss_bgzf.tobytes(), res.record_bytes, res.ss_record_bytes) == want
    dev.close()
    ctx.close()


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_filt") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.mark.parametrize("batch_reads", ["1048576", "300"])
def test_gpu_cli_golden_families(tmp_path, golden_bam, batch_reads):
    be = cli.default_backend(ConsensusParams())
    flt = FILTERS["all"]
    want, words = fm.apply(flt, WANT_DS)
    out, ss, plain = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam"), str(tmp_path / "plain.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads,
                       *flt.argv()], backend=be)
    assert exc is None
    assert_records(records(out), want, "ds")
    assert_records(records(ss), fm.keep_ss(words, WANT_SS), "ss")
    # the same backend, kept by the process, without the options: the filter does not stay on its context
    stdout0, exc0 = run(["-i", golden_bam, "-o", plain, "--batch_reads", batch_reads], backend=be)
    assert exc0 is None and stdout == stdout0 + summary_lines(words)
    assert_records(records(plain), WANT_DS, "ds")
    assert side_files(plain) == side_files(out)


def test_gpu_cli_failing_family_in_mid_batch(tmp_path):
    """The reference raises IndexError at the 21st family; the 20 before it
    are filtered, and what is left comes from the slot's record stream
    (record_bytes_of honours the dropped families' zero sizes)."""
    path, out, ss = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    first = failing_input(path)
    ds20 = [r for c in first for r in c["expect"]["ds"]]
    totals = sorted(sum(fm.scalars(r)[:2]) for r in ds20)
    flt = fm.Filter(min_base_quality=FILTERS["mask"].min_base_quality, min_reads=(totals[len(totals) // 2], 1, 1))
    want, words = fm.apply(flt, ds20)
    assert 0 < len(want) < 40
    stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, *flt.argv()],
                      backend=cli.default_backend(ConsensusParams()))
    assert exc == "IndexError"
    assert_records(records(out), want, "ds")
    assert_records(records(ss), fm.keep_ss(words, [r for c in first for r in c["expect"]["ss"]]), "ss")
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "plain.bam")], backend=cli.default_backend(ConsensusParams()))
    assert (stdout0, exc0) == (stdout, exc)
