"""``--mate_overlap mask|consensus``: the two duplex reads of a family
reconciled where they cover the same reference position (include/dcr.h
``dcr_set_mate_overlap``), through the CLI against the spec restated in
tests/mate_overlap_model.py, applied to the records of a run without the
option.

CPU: every run uses the C oracle as the batch backend (test infrastructure);
the step is the native host one (dcr_fmt_mate_overlap)."""
import contextlib
import ctypes
import io
import os
import random

import pytest

from duplexumiconsensusreads_amd import bam, cli, native_io, params, synth
from oracle import dcr_oracle_c
from tests import filter_model as fm
from tests import mate_overlap_cases as mc
from tests import mate_overlap_model as mm
from tests.test_ss_output import (PROCESSED, DEFAULT, _c_values, assert_records, failing_input, records, run,
                                  side_files, write_bam)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_DS = [r for c in PROCESSED for r in c["expect"]["ds"]]
MODES = ("mask", "consensus")
# the 877 golden families, counted with the model's rules
GOLDEN_CENSUS = dict(overlapping=761, with_disagreement=227, disagree=1244, equal_q=404, mate1_higher=213,
                     mate2_higher=627, agree=12827, agree_sum_le_93=1458, skipped_n=2248, shifted=224)


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ovl") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.fixture(scope="module")
def plain(tmp_path_factory, golden_bam):
    """The runs without the option, one per batch size: (output, single-strand file, stdout)."""
    d = tmp_path_factory.mktemp("ovl_plain")
    out = {}
    for batch_reads in ("1048576", "100"):
        o, ss = str(d / f"plain{batch_reads}.bam"), str(d / f"plain{batch_reads}_ss.bam")
        stdout, exc = run(["-i", golden_bam, "-o", o, "--single_strand_output", ss, "--batch_reads", batch_reads])
        assert exc is None
        out[batch_reads] = (o, ss, stdout)
    return out


def test_the_golden_input_is_not_vacuous():
    assert len(WANT_DS) == 2 * 877
    assert mm.census(WANT_DS) == GOLDEN_CENSUS
    # no golden pair has mate 2 starting left of mate 1: the hand-built families cover that
    assert all(WANT_DS[2 * f + 1]["pos"] >= WANT_DS[2 * f]["pos"] for f in range(877))


@pytest.mark.parametrize("batch_reads", ["1048576", "100"])
@pytest.mark.parametrize("mode", MODES)
def test_golden_families(tmp_path, golden_bam, plain, mode, batch_reads):
    p_out, p_ss, p_stdout = plain[batch_reads]
    before = records(p_out)
    assert_records(before, WANT_DS, "plain")
    want, counts = mm.apply(mode, before)
    tot = mm.totals(counts)
    c = GOLDEN_CENSUS
    assert tot[:2] == (c["agree"] + c["disagree"], c["disagree"])
    if mode == "mask":
        assert tot[2] == 2 * c["disagree"]
    else:
        assert tot[2] > 2 * c["disagree"]
    out, ss = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    stats = {}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["-i", golden_bam, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads,
                  "--mate_overlap", mode], backend=dcr_oracle_c.run, rng=random.Random(1), stats=stats)
    got = records(out)
    assert_records(got, want, "ds")
    assert got != before
    # nothing but seq and qual moved
    for g, b in zip(got, before):
        assert {k for k in b if g[k] != b[k]} <= {"seq", "qual"}
    assert side_files(out) == side_files(p_out)
    assert open(ss, "rb").read() == open(p_ss, "rb").read()
    assert buf.getvalue() == p_stdout + mc.summary_lines(tot)
    assert (stats["overlap_compared"], stats["overlap_disagree"], stats["overlap_changed"]) == tot
    assert stats["consensus_records"] == len(want) and "filter_dropped_families" not in stats


@pytest.fixture(scope="module")
def hand_built(tmp_path_factory):
    """The hand-built families' input and the plain run's duplex records."""
    d = tmp_path_factory.mktemp("ovl_cases")
    path = mc.write_families(str(d / "in.bam"), mc.families())
    out = str(d / "plain.bam")
    stdout, exc = run(["-i", path, "-o", out])
    assert exc is None
    return path, records(out), stdout


@pytest.mark.parametrize("name", list(mc.CASES))
def test_hand_built_shapes(hand_built, name):
    """The plain run's pos and CIGAR of both records, and what the pair holds."""
    f = list(mc.CASES).index(name)
    want = mc.CASES[name][2]
    pair = hand_built[1][2 * f:2 * f + 2]
    assert tuple(r["pos"] - 1000 * f for r in pair) == want["pos"]
    assert tuple(r["cigar"] for r in pair) == want["cigar"]
    census = mm.census(pair)
    assert {k: census[k] for k in want["census"]} == want["census"]


@pytest.mark.parametrize("mode", MODES)
def test_hand_built_families(tmp_path, hand_built, mode):
    path, before, stdout0 = hand_built
    want, counts = mm.apply(mode, before)
    by_name = dict(zip(mc.CASES, counts))
    assert by_name["disjoint"] == by_name["adjacent"] == (0, 0, 0)
    assert by_name["one_base"] == (1, 1, 2)
    assert by_name["n_either_side"][:2] == (10, 1)
    assert by_name["quality_sums"] == ((12, 0, 0) if mode == "mask" else (12, 0, 24))
    out = str(tmp_path / "cons.bam")
    stdout, exc = run(["-i", path, "-o", out, "--mate_overlap", mode])
    assert exc is None
    got = records(out)
    assert_records(got, want, "ds")
    assert stdout == stdout0 + mc.summary_lines(mm.totals(counts))
    # spot checks of the rules themselves, on the records as read back
    f = list(mc.CASES).index("pos1<pos0")
    a, b = got[2 * f], got[2 * f + 1]
    if mode == "consensus":
        # mate 2 (quality 60) overrules mate 1 (51) at the first and the last overlapping base
        assert a["seq"][0] == b["seq"][8] == before[2 * f + 1]["seq"][8] and a["qual"][0] == b["qual"][8] == 9
        assert a["seq"][3] == b["seq"][11] and a["qual"][3] == b["qual"][11] == 9
        assert a["qual"][1] == b["qual"][9] == 93
    else:
        assert (a["seq"][0], b["seq"][8], a["qual"][0], b["qual"][8]) == ("N", "N", 2, 2)
        assert a["qual"][1:3] == before[2 * f]["qual"][1:3]
    f = list(mc.CASES).index("quality_sums")
    if mode == "consensus":
        assert got[2 * f]["qual"] == got[2 * f + 1]["qual"] == [93] * 4 + [42] * 8
    f = list(mc.CASES).index("identical")
    assert got[2 * f]["seq"][0] == got[2 * f]["seq"][11] == "N"         # equal qualities: masked in both modes
    assert got[2 * f + 1]["qual"][0] == got[2 * f + 1]["qual"][11] == 2


@pytest.mark.parametrize("mode", MODES)
def test_composition_with_the_filters(tmp_path, golden_bam, plain, mode):
    """fam_filt and the records with the option are what the filter model
    gives on the records the overlap model returns."""
    before = records(plain["1048576"][0])
    step, counts = mm.apply(mode, before)
    quals = sorted(q for r in step for q in r["qual"])
    Q = quals[len(quals) // 10] + 1
    masked = [fm.mask(fm.Filter(min_base_quality=Q), r)[0] for r in step]
    fractions = sorted(r["seq"].count("N") / len(r["seq"]) for r in masked)
    flt = fm.Filter(min_base_quality=Q, max_no_call_fraction=fractions[3 * len(fractions) // 4])
    want, words = fm.apply(flt, step)
    want0, words0 = fm.apply(flt, before)
    kept = [w & 0xff == 0 for w in words]
    assert 0 < sum(kept) < len(words)
    assert words != words0, "the step does not move the filter's outcome"
    out, ss = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    stats = {}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["-i", golden_bam, "-o", out, "--single_strand_output", ss, "--mate_overlap", mode, *flt.argv()],
                 backend=dcr_oracle_c.run, rng=random.Random(1), stats=stats)
    assert_records(records(out), want, "ds")
    assert_records(records(ss), fm.keep_ss(words, records(plain["1048576"][1])), "ss")
    from tests.test_consensus_filter import summary_lines
    tot = mm.totals(counts, kept)                        # only the families written count
    assert tot != mm.totals(counts)
    assert buf.getvalue() == plain["1048576"][2] + summary_lines(words) + mc.summary_lines(tot)
    assert (stats["overlap_compared"], stats["overlap_disagree"], stats["overlap_changed"]) == tot
    assert stats["filter_dropped_families"] == len(words) - sum(kept)


@pytest.mark.parametrize("batch_reads", ["1048576", "40"])
def test_failing_family(tmp_path, batch_reads):
    """The families before the failing one are reconciled as any other; the
    failure and everything printed for it stay as they are."""
    path, out, ss = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    first = failing_input(path)
    ds20 = [r for c in first for r in c["expect"]["ds"]]
    want, counts = mm.apply("consensus", ds20)
    assert mm.totals(counts)[1] > 0
    stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads,
                       "--mate_overlap", "consensus"])
    assert exc == "IndexError"
    assert_records(records(out), want, "ds")
    assert_records(records(ss), [r for c in first for r in c["expect"]["ss"]], "ss")
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "plain.bam"), "--batch_reads", batch_reads])
    assert (stdout0, exc0) == (stdout, exc)
    assert side_files(out) == side_files(str(tmp_path / "plain.bam"))


def test_default_is_off(tmp_path, golden_bam, plain):
    assert cli.parse_args(["-i", "x.bam"]).mate_overlap is None
    a = cli.parse_args(["-i", "x.bam", "--mate_overlap", "mask"])
    assert a.mate_overlap == params.OVL_MASK and params.ConsensusFilter.from_args(a) is None
    assert cli.parse_args(["-i", "x.bam", "--mate_overlap", "consensus"]).mate_overlap == params.OVL_CONSENSUS
    out = str(tmp_path / "again.bam")
    stats = {}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["-i", golden_bam, "-o", out], backend=dcr_oracle_c.run, rng=random.Random(1), stats=stats)
    assert buf.getvalue() == plain["1048576"][2]
    assert open(out, "rb").read() == open(plain["1048576"][0], "rb").read()
    assert not any(k.startswith("overlap_") for k in stats)


BAD = [["--mate_overlap", ""], ["--mate_overlap", "Mask"], ["--mate_overlap", "1"], ["--mate_overlap", "clip"],
       ["--mate_overlap", "mask,consensus"], ["--mate_overlap"]]


@pytest.mark.parametrize("bad", BAD, ids=[" ".join(b) or "-" for b in BAD])
def test_malformed_values_exit_at_parse_time(tmp_path, bad, capsys):
    missing = str(tmp_path / "never_opened.bam")
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", missing, "-o", str(tmp_path / "out.bam"), *bad], backend=lambda *a: None)
    assert e.value.code == 2                                 # argparse's error, not the reference's exit(1)
    assert "--mate_overlap" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_host_entry_point_rejects_other_modes(tmp_path):
    hb = native_io.HostBatch(reads=64)
    ds = native_io.FmtOut()
    for mode in (0, 3, -1):
        with pytest.raises(native_io.IOError_):
            native_io.apply_overlap(hb, None, ds, mode, 0)


def test_two_gloo_ranks_write_the_same_files_and_summary(tmp_path):
    from tests.test_cli_shard import _outcome, run_sharded
    synth.write_config_bam(str(tmp_path / "synth.bam"),
                           synth.SynthConfig("t", 600, sub_size="poisson5", seed=11, low_mapq_frac=0.1,
                                             indel_frac=0.1, softclip_frac=0.1))
    # the generator's mates read one template: make mate 2 dissent
    path = mc.dissenting_copy(str(tmp_path / "synth.bam"), str(tmp_path / "in.bam"))
    base = ["--min_reads", "3", "--max_reads", "5"]

    def argv(tag, extra):
        return ["-i", path, "-o", str(tmp_path / f"{tag}.bam"), "--single_strand_output",
                str(tmp_path / f"{tag}_ss.bam"), *base, *extra]

    def files(tag):
        return [records(str(tmp_path / f"{tag}{s}.bam")) for s in ("", "_filteredreads", "_filteredfamilies", "_ss")]
    _, exc0, _ = _outcome(argv("all", []), 7)
    assert exc0 is None
    every = files("all")
    want, counts = mm.apply("consensus", every[0])
    tot = mm.totals(counts)
    assert all(t > 0 for t in tot)
    out1, exc1, st1 = _outcome(argv("one", ["--mate_overlap", "consensus"]), 7)
    part_dir = tmp_path / "parts"
    part_dir.mkdir()
    os.environ["DCR_PART_DIR"] = str(part_dir)
    try:
        got = run_sharded(argv("many", ["--mate_overlap", "consensus"]), 7, 2)
    finally:
        del os.environ["DCR_PART_DIR"]
    assert exc1 is None and got[0][:3] == (out1, exc1, st1)
    one, many = files("one"), files("many")
    for a, b in zip(many, one):
        assert a == b
    # the BAM streams byte for byte (the ranks' parts are compressed apart, so the BGZF blocks are cut elsewhere)
    for tag in ("", "_ss"):
        assert bam.bgzf_stream(str(tmp_path / f"many{tag}.bam")) == bam.bgzf_stream(str(tmp_path / f"one{tag}.bam"))
    assert list(part_dir.iterdir()) == []
    assert_records(one[0], want, "ds")
    assert one[1:] == every[1:]
    assert out1.endswith(mc.summary_lines(tot))


def test_ctypes_layouts_match_headers(tmp_path):
    from duplexumiconsensusreads_amd import _lib
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"), ["DCR_OVL_MASK", "DCR_OVL_CONSENSUS", "DCR_ABI_VERSION"],
                    tmp_path)
    assert got == [params.OVL_MASK, params.OVL_CONSENSUS, 1]
    assert {"dcr_set_mate_overlap", "dcr_slot_overlap_out"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dcr_set_mate_overlap") and hasattr(lib, "dcr_slot_overlap_out") and lib.dcr_abi_version() == 1
    assert hasattr(native_io.load(), "dcr_fmt_mate_overlap") and native_io.load().dcr_io_abi_version() == 1
