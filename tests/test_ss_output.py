"""``--single_strand_output FILE``: the four single-strand consensus records
(A1, B2, B1, A2) of every family whose duplex records are written, in a BAM
of their own, against the records the reference's ``make_consensus_read(
method="single_strand")`` returned for the golden families
(tests/golden/families.json.gz ``expect["ss"]``).

CPU: every run uses the C oracle as the batch backend (test infrastructure);
the records are formatted by the native host formatter (dcr_fmt_write_ss)."""
import contextlib
import ctypes
import io
import os
import random
import subprocess

import pytest

from duplexumiconsensusreads_amd import bam, cli, native_io, synth
from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from oracle import dcr_oracle_c
from tests.golden_io import input_record, load_families

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAM = load_families()
HEADER = BamHeader("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:chr{i + 1}\tLN:248956422\n" for i in range(4)),
                   [f"chr{i + 1}" for i in range(4)], [248956422] * 4)


def inner_soft_clip(case):
    """pass_filters exits on a soft clip inside the CIGAR (:1163-1165)."""
    return any(op == 4 for r in case["reads"] for op, _ in r["cigar"][1:-1])


# the golden families a run of main() with the default flags gets through
DEFAULT = [c for c in FAM["cases"] if c["params"] == "default" and c["expect"]["status"] in ("ok", "filtered")
           and not inner_soft_clip(c)]
PROCESSED = [c for c in DEFAULT if c["expect"]["status"] == "ok"]
BIG = "scores_minreads2_max6"
BIG_FLAGS = ["--min_base_quality", "25", "--min_reads", "2", "--max_reads", "6", "--max_base_quality", "50",
             "--base_quality_shift", "2", "--deletion_score", "15", "--no_insertion_score", "45"]


def subfamily_sizes(case):
    """Reads per subfamily A1 B2 B1 A2 (split_family :132-154) among the reads that pass -q 20."""
    n = [0, 0, 0, 0]
    for r in case["reads"]:
        if r["mapq"] < 20:
            continue
        rev, r1, r2 = r["flag"] & 16, r["flag"] & 64, r["flag"] & 128
        k = 0 if (not rev and r1) else 1 if (not rev and r2) else 2 if (rev and r1) else 3 if (rev and r2) else -1
        if k >= 0:
            n[k] += 1
    return n


SAMPLED = [c for c in FAM["cases"] if c["params"] == BIG and c["kind"] == "big" and c["expect"]["status"] == "ok"
           and max(subfamily_sizes(c)) > 6 and not inner_soft_clip(c)]


def write_bam(path, cases):
    with AlignmentFile(path, "wb", header=HEADER) as out:
        for c in cases:
            for r in c["reads"]:
                out.write(input_record(r))


def records(path):
    with AlignmentFile(path, "rb") as f:
        return [r.to_dict() for r in f]


def run(argv, rng=None, backend=dcr_oracle_c.run):
    """(stdout, exception name or None) of cli.main."""
    buf, exc = io.StringIO(), None
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(argv, backend=backend, rng=rng or random.Random(1))
    except SystemExit as e:
        exc = f"SystemExit({e.code})"
    except Exception as e:  # noqa: BLE001 - the reference's outcome
        exc = type(e).__name__
    return buf.getvalue(), exc


def side_files(out):
    return [records(out[:-4] + s) for s in ("_filteredreads.bam", "_filteredfamilies.bam")]


def assert_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, i, {k: (g.get(k), w.get(k)) for k in w if g.get(k) != w.get(k)})


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ss") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


def test_golden_selection_is_the_one_checked():
    assert (len(DEFAULT), len(PROCESSED), len(SAMPLED)) == (983, 877, 39)


def test_default_is_no_single_strand_file(tmp_path, golden_bam):
    assert cli.parse_args(["-i", "x.bam"]).single_strand_output is None
    out = str(tmp_path / "cons.bam")
    _, exc = run(["-i", golden_bam, "-o", out])
    assert exc is None
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cons.bam", "cons_filteredfamilies.bam",
                                                          "cons_filteredreads.bam"]


@pytest.mark.parametrize("batch_reads", ["1048576", "100"])
def test_golden_families(tmp_path, golden_bam, batch_reads):
    out, ss, plain = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam"), str(tmp_path / "plain.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads])
    stdout0, exc0 = run(["-i", golden_bam, "-o", plain, "--batch_reads", batch_reads])
    assert exc is None and exc0 is None
    want_ss = [r for c in PROCESSED for r in c["expect"]["ss"]]
    assert len(want_ss) == 3508
    assert_records(records(ss), want_ss, "ss")
    assert_records(records(out), [r for c in PROCESSED for r in c["expect"]["ds"]], "ds")
    assert stdout == stdout0
    assert side_files(out) == side_files(plain)
    assert records(out) == records(plain)
    with AlignmentFile(ss, "rb") as f, AlignmentFile(golden_bam, "rb") as g:
        assert f.header.encode() == g.header.encode()


def test_downsampled_families(tmp_path):
    """Flag, MI, RX and the sQ order are those of the sample's first read and of the sample."""
    for c in SAMPLED:
        path, out, ss = (str(tmp_path / f"in{c['fam']}.bam"), str(tmp_path / f"c{c['fam']}.bam"),
                         str(tmp_path / f"s{c['fam']}.bam"))
        write_bam(path, [c])
        _, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, *BIG_FLAGS],
                     rng=random.Random(c["expect"]["seed"]))
        assert exc is None, c["fam"]
        assert_records(records(ss), c["expect"]["ss"], ("ss", c["fam"]))
        assert_records(records(out), c["expect"]["ds"], ("ds", c["fam"]))


def failing_input(path):
    """20 families, then the golden family the reference raises IndexError on."""
    crash = [c for c in FAM["cases"] if c["fam"] == 996]
    assert len(crash) == 1 and crash[0]["params"] == "default" and crash[0]["expect"]["status"] == "crash:IndexError"
    assert not inner_soft_clip(crash[0])
    write_bam(path, PROCESSED[:20] + crash)
    return PROCESSED[:20]


@pytest.mark.parametrize("batch_reads", ["1048576", "40"])
def test_failing_family_ends_both_files(tmp_path, batch_reads):
    path, out, ss = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    first = failing_input(path)
    stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads])
    assert exc == "IndexError"
    assert_records(records(ss), [r for c in first for r in c["expect"]["ss"]], "ss")
    assert_records(records(out), [r for c in first for r in c["expect"]["ds"]], "ds")
    assert len(records(ss)) == 80 and len(records(out)) == 40
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "plain.bam"), "--batch_reads", batch_reads])
    assert (stdout0, exc0) == (stdout, exc)


def test_bad_output_name(tmp_path, golden_bam, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", golden_bam, "-o", str(tmp_path / "cons.bam"), "--single_strand_output",
                  str(tmp_path / "sscs.sam")], backend=dcr_oracle_c.run)
    assert e.value.code == 1
    assert ("ERROR: output file is not specified in the right format. \n Please specify the file name of a valid "
            ".bam file. Include the format in the file name.") in capsys.readouterr().out
    assert not (tmp_path / "sscs.sam").exists()


def test_native_stream_is_the_python_codecs(tmp_path, golden_bam):
    """dcr_fmt_write_ss writes the uncompressed stream bam.encode_record gives for the same records."""
    ss = str(tmp_path / "sscs.bam")
    _, exc = run(["-i", golden_bam, "-o", str(tmp_path / "cons.bam"), "--single_strand_output", ss])
    assert exc is None
    with AlignmentFile(ss, "rb") as f:
        recs = list(f)
        hdr = f.header.encode()
    assert len(recs) == 3508
    assert bam.bgzf_stream(ss) == hdr + b"".join(bam.encode_record(r) for r in recs)


def test_two_gloo_ranks_write_the_same_four_files(tmp_path):
    from tests.test_cli_shard import _outcome, run_sharded
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 600, sub_size="poisson5", seed=11, low_mapq_frac=0.1,
                                                   indel_frac=0.1, softclip_frac=0.1))
    extra = ["--min_reads", "3", "--max_reads", "5"]

    def argv(tag):
        return ["-i", path, "-o", str(tmp_path / f"{tag}.bam"), "--single_strand_output",
                str(tmp_path / f"{tag}_ss.bam"), *extra]

    def files(tag):
        return [records(str(tmp_path / f"{tag}{s}.bam")) for s in ("", "_filteredreads", "_filteredfamilies", "_ss")]
    out1, exc1, st1 = _outcome(argv("one"), 7)
    part_dir = tmp_path / "parts"
    part_dir.mkdir()
    os.environ["DCR_PART_DIR"] = str(part_dir)
    try:
        got = run_sharded(argv("many"), 7, 2)
    finally:
        del os.environ["DCR_PART_DIR"]
    assert exc1 is None and got[0][:3] == (out1, exc1, st1)
    one, many = files("one"), files("many")
    assert len(one[0]) > 0 and len(one[2]) > 0 and len(one[3]) == 2 * len(one[0])
    for a, b in zip(many, one):
        assert a == b
    assert list(part_dir.iterdir()) == []
    # the input has filtered families and subfamilies that are downsampled
    ing = native_io.Ingest(path, 20, 3, 5, 20)
    hb = native_io.HostBatch(reads=1 << 16)
    ing.next(hb)
    assert len(ing.sample_calls()) > 0 and hb.s.n_tab > hb.n_fam
    ing.close()


def _c_values(header, exprs, tmp_path):
    src = (f'#include "{header}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{'
           + "".join(f'printf("%zu\\n", (size_t)({e}));' for e in exprs) + "return 0;}\n")
    exe = str(tmp_path / "ss_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]


def test_ctypes_layouts_match_headers(tmp_path):
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import WMeta, WMetaSs, WRes
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"),
                    ["sizeof(dcr_wmeta_ss)", "offsetof(dcr_wmeta_ss, sub_flag)", "offsetof(dcr_wmeta_ss, sub_mi)",
                     "offsetof(dcr_wmeta_ss, sub_rx)", "sizeof(dcr_wmeta)", "sizeof(dcr_wres)",
                     "offsetof(dcr_wres, totals)", "DCR_ABI_VERSION"], tmp_path)
    assert got == [ctypes.sizeof(WMetaSs), WMetaSs.sub_flag.offset, WMetaSs.sub_mi.offset, WMetaSs.sub_rx.offset,
                   ctypes.sizeof(WMeta), ctypes.sizeof(WRes), WRes.totals.offset, 1]
    S = native_io.HostBatchStruct
    got = _c_values(os.path.join(ROOT, "include", "dcr_io.h"),
                    ["sizeof(dcr_host_batch)", "offsetof(dcr_host_batch, side_filt)",
                     "offsetof(dcr_host_batch, sub_flag)", "offsetof(dcr_host_batch, sub_mi)",
                     "offsetof(dcr_host_batch, sub_rx)", "offsetof(dcr_host_batch, n_fam)", "DCR_INGEST_SS_META",
                     "DCR_IO_ABI_VERSION"], tmp_path)
    assert got == [ctypes.sizeof(S), S.side_filt.offset, S.sub_flag.offset, S.sub_mi.offset, S.sub_rx.offset,
                   S.n_fam.offset, native_io.INGEST_SS_META, 1]
    assert {"dcr_submit_write_ss", "dcr_wait_write_ss"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dcr_submit_write_ss") and hasattr(lib, "dcr_wait_write_ss") and lib.dcr_abi_version() == 1
    assert hasattr(native_io.load(), "dcr_fmt_write_ss") and native_io.load().dcr_io_abi_version() == 1


def test_ss_metadata_only_under_the_flag(tmp_path, golden_bam):
    """Without DCR_INGEST_SS_META, or with NULL arrays, the ingest writes no
    extra string into the names arena."""
    def names_bytes(ingest_flag, batch_flag):
        ing = native_io.Ingest(golden_bam, ss_meta=ingest_flag)
        hb = native_io.HostBatch(reads=1 << 16, ss_meta=batch_flag)
        ing.next(hb)
        ing.close()
        return hb.s.n_names, hb
    n0, _ = names_bytes(False, False)
    assert names_bytes(True, False)[0] == n0 and names_bytes(False, True)[0] == n0
    n1, hb = names_bytes(True, True)
    assert n1 > n0
    assert hb.name(hb.a["sub_mi"][1]) == PROCESSED[0]["expect"]["ss"][1]["tags"][0][2]
    assert int(hb.a["sub_flag"][1]) == PROCESSED[0]["expect"]["ss"][1]["flag"]
