"""The single-strand records on the GPU (dcr_submit_write_ss: k_fmt_size_ss,
k_fmt_write_ss and a second k_deflate / k_compact pass) against the host
formatter (dcr_fmt_write_ss over the kernel outputs of dcr_submit) on the
same batches, byte for byte; the duplex stream of the same submit against a
plain dcr_submit_write; and ``--single_strand_output`` through the GPU CLI
against the reference's records (tests/golden/families.json.gz)."""
import gzip

import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, native_io, synth
from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from duplexumiconsensusreads_amd.params import ConsensusParams
from duplexumiconsensusreads_amd.records import AlignedSegment
from oracle import dcr_oracle_c
from tests.test_gpu_writer import members
from tests.test_ss_output import (DEFAULT, PROCESSED, assert_records, failing_input, records, run, side_files,
                                  write_bam)

pytestmark = pytest.mark.gpu


def batches(path, params, reads):
    ing = native_io.Ingest(path, params.min_map_quality, params.min_reads, params.max_reads,
                           params.min_base_quality, ss_meta=True)
    while True:
        hb = native_io.HostBatch(reads=reads, side_bytes=1 << 24, ss_meta=True)
        ing.next(hb)
        yield hb
        if hb.end_kind != native_io.END_FULL:
            break
    ing.close()


def host_stream(tmp_path, hb, ss, n_fam):
    """The host formatter's single-strand record bytes of families [0, n_fam)."""
    out = str(tmp_path / "host_ss.bam")
    w = native_io.BgzfWriter(out, b"")
    w.write_consensus_ss(hb, ss, n_fam)
    w.close()
    return gzip.decompress(open(out, "rb").read())


def check_batches(tmp_path, path, params, reads):
    """Every batch of ``path`` through the three submits; returns the batches'
    (families, single-strand BGZF blocks)."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    dev.ss_output = True
    plain = DeviceStream(ctx, device_writer=True)
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = True
    seen = []
    for hb in batches(path, params, reads):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        fetched = res.ss_record_bytes_of(F).tobytes()       # before the slot is submitted again
        ds_fetched = res.record_bytes_of(F).tobytes()
        ss_blocks, ds_blocks = res.ss_bgzf.tobytes(), res.bgzf.tobytes()
        fam_fail = res.fam_fail.copy()
        assert not fam_fail.any(), "these inputs have no failing family"
        # the duplex stream of the same submit is a plain dcr_submit_write's
        res0 = plain.result(plain.submit(hb))
        assert res0.ss_bgzf is None
        assert ds_blocks == res0.bgzf.tobytes()
        assert ds_fetched == res0.record_bytes_of(F).tobytes()
        assert (res.bgzf_bytes, res.record_bytes, res.blocks) == (res0.bgzf_bytes, res0.record_bytes, res0.blocks)
        assert np.array_equal(fam_fail, res0.fam_fail)
        # the single-strand stream is the host formatter's over dcr_submit's outputs
        ss, ds, rs = host.result(host.submit(hb))
        assert native_io.first_failure(hb, ss, ds, F, rs)[0] == F
        want = host_stream(tmp_path, hb, ss, F)
        got = members(ss_blocks)                            # checks every member's CRC32 and ISIZE
        assert len(got) == res.ss_record_bytes
        assert got == want
        assert fetched == want
        emu = b"".join(native_io.deflate_emulate(fetched[i:i + 0xff00]) for i in range(0, len(fetched), 0xff00))
        assert emu == ss_blocks
        assert res.ss_blocks == -(-len(want) // 0xff00)
        seen.append((F, res.ss_blocks))
    dev.close()
    plain.close()
    host.close()
    ctx.close()
    return seen


@pytest.mark.parametrize("kind", ["c1", "indel_clip"])
def test_device_stream_is_the_host_formatters(tmp_path, kind):
    path = str(tmp_path / "in.bam")
    cfg = synth.SynthConfig("t", 400, sub_size="poisson5", seed=9,
                            indel_frac=0.3 if kind == "indel_clip" else 0.0,
                            softclip_frac=0.3 if kind == "indel_clip" else 0.0)
    synth.write_config_bam(path, cfg)
    seen = check_batches(tmp_path, path, ConsensusParams(), 2000)
    assert len(seen) > 2                                    # several batches: both slots are reused
    assert 390 <= sum(f for f, _ in seen) <= 400            # a clipped family may fall to the filters
    assert all(nb > 1 for _, nb in seen[:-1])               # every full batch's stream spans blocks


# ---- edge shapes: subfamily sizes around the 64-lane chunks of the sQ array and the
# general kernel (> 64 reads), list lengths 1 / 150 / 151 around the 64-entry
# chunks of the sd / se text, depths of 1, 2 and 3 digits, sD >= 256 (type S)
EDGE = [((1, 63, 64, 65), 151), ((100, 128, 129, 2), 150), ((260, 1, 1, 1), 1)]
EDGE_ARGS = ["--max_reads", "300"]


def edge_bam(path):
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    hdr = BamHeader("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])
    with AlignmentFile(path, "wb", header=hdr) as out:
        for f, (sizes, L) in enumerate(EDGE):
            ins = L + 40
            tmpl = acgt[rng.integers(0, 4, ins + 8)]
            P = 10_000 + 1_000 * f
            spec = [(99, "A", 0), (163, "B", 0), (83, "B", ins - L), (147, "A", ins - L)]    # A1 B2 B1 A2
            for k, (flag, strand, start) in enumerate(spec):
                for j in range(sizes[k]):
                    seq, cig = tmpl[start:start + L].copy(), [(0, L)]
                    if L >= 150 and j % 5 == 1:       # one inserted base, two deleted ones
                        seq = np.concatenate([tmpl[start:start + 40], acgt[j % 4:j % 4 + 1], tmpl[start + 40:start + 89],
                                              tmpl[start + 91:start + 91 + L - 90]])
                        cig = [(0, 40), (1, 1), (0, 49), (2, 2), (0, L - 90)]
                    r = AlignedSegment()
                    r.query_name = f"e{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = P + start
                    r.mapping_quality = 20 + (7 * j + k) % 41
                    r.cigartuples = cig
                    r.query_sequence = seq.tobytes().decode()
                    r.query_qualities = [37 if (i + j) % 11 else 25 for i in range(L)]
                    r.set_tags([("MI", f"{f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)
    return path


def test_edge_shapes(tmp_path):
    path = edge_bam(str(tmp_path / "edge.bam"))
    params = ConsensusParams(max_reads=300)
    seen = check_batches(tmp_path, path, params, 1 << 12)
    assert [f for f, _ in seen] == [3]
    # the decoded records: the GPU CLI's are the oracle-backend CLI's
    got_ss, want_ss = str(tmp_path / "g_ss.bam"), str(tmp_path / "o_ss.bam")
    out_g, exc_g = run(["-i", path, "-o", str(tmp_path / "g.bam"), "--single_strand_output", got_ss, *EDGE_ARGS],
                       backend=cli.default_backend(params))
    out_o, exc_o = run(["-i", path, "-o", str(tmp_path / "o.bam"), "--single_strand_output", want_ss, *EDGE_ARGS],
                       backend=dcr_oracle_c.run)
    assert (out_g, exc_g) == (out_o, exc_o) and exc_o is None
    want = records(want_ss)
    assert_records(records(got_ss), want, "ss")
    assert_records(records(str(tmp_path / "g.bam")), records(str(tmp_path / "o.bam")), "ds")
    # the shapes this input is for
    assert [r["qname"] for r in want] == [f"consensus_family{f}_{s}" for f in range(3) for s in ("A1", "B2", "B1", "A2")]
    tags = [{t[0]: t for t in r["tags"]} for r in want]
    assert [len(t["sQ"][2]) for t in tags] == [n for sizes, _ in EDGE for n in sizes]
    assert [t["sD"][1:] for t in tags][8] == ["S", 260] and tags[0]["sD"][1:] == ["C", 1]
    assert {1, 150, 151} <= {len(r["seq"]) for r in want}       # odd and even lengths are 4-bit packed
    assert any("I" in r["cigar"] or "D" in r["cigar"] for r in want)
    assert "100" in tags[4]["sd"][2] and "64" in tags[2]["sd"][2]


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_ss") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.mark.parametrize("batch_reads", ["1048576", "300"])
def test_gpu_cli_golden_families(tmp_path, golden_bam, batch_reads):
    be = cli.default_backend(ConsensusParams())
    out, ss, plain = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam"), str(tmp_path / "plain.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads],
                      backend=be)
    assert exc is None
    assert_records(records(ss), [r for c in PROCESSED for r in c["expect"]["ss"]], "ss")
    assert_records(records(out), [r for c in PROCESSED for r in c["expect"]["ds"]], "ds")
    # the same backend, kept by the process, without the option: the same other outputs
    stdout0, exc0 = run(["-i", golden_bam, "-o", plain, "--batch_reads", batch_reads], backend=be)
    assert (stdout0, exc0) == (stdout, exc)
    assert records(plain) == records(out) and side_files(plain) == side_files(out)


def test_gpu_cli_failing_family_in_mid_batch(tmp_path):
    """The reference raises IndexError at the 21st family: reported through
    fam_fail, the batch's records before it come from the slot's record
    stream (ss_record_bytes_of)."""
    path, out, ss = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    first = failing_input(path)
    _, exc = run(["-i", path, "-o", out, "--single_strand_output", ss], backend=cli.default_backend(ConsensusParams()))
    assert exc == "IndexError"
    assert_records(records(ss), [r for c in first for r in c["expect"]["ss"]], "ss")
    assert_records(records(out), [r for c in first for r in c["expect"]["ds"]], "ds")
    assert len(records(ss)) == 80 and len(records(out)) == 40


def test_blocks_larger_than_the_host_buffer_are_fetched_again(tmp_path):
    """dcr_wait_write_ss with a cap_bgzf too small for a stream returns
    DCR_ECAPACITY with both totals set; DeviceStream grows that stream's
    buffer and fetches its blocks from the slot (dcr_slot_fetch 2 and 5)."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 200, sub_size="poisson5", seed=5))
    params = ConsensusParams()
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    dev.ss_output = True
    hb = next(iter(batches(path, params, 1 << 16)))
    assert hb.n_fam == 200
    res = dev.result(dev.submit(hb))
    want_ds, want_ss = res.bgzf.tobytes(), res.ss_bgzf.tobytes()
    assert len(want_ds) > 1000 and len(want_ss) > 1000
    for small in (("ds", "ss"), ("ss",), ("ds",)):
        h = dev.submit(hb)
        outs = {"ds": dev.wouts[h[0]], "ss": dev.wouts_ss[h[0]]}
        for k in small:
            outs[k].cap_b = 1000                # what the next dcr_wait_write_ss is told
        res = dev.result(h)
        assert (res.bgzf.tobytes(), res.ss_bgzf.tobytes()) == (want_ds, want_ss), small
        assert all(outs[k].cap_b >= len(w) for k, w in (("ds", want_ds), ("ss", want_ss)))
    dev.close()
    ctx.close()
