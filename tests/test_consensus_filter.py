"""``--filter_*``: masking of weak duplex bases and the family filters
(include/dcr.h ``dcr_filter``), through the CLI against the spec restated in
tests/filter_model.py, applied to the records the reference returned for the
golden families (tests/golden/families.json.gz ``expect["ds"]`` / ``["ss"]``).

CPU: every run uses the C oracle as the batch backend (test infrastructure);
the filter is the native host one (dcr_fmt_filter) and the records come from
the host formatter's masked entries (dcr_fmt_write_filt / _ss_filt)."""
import contextlib
import ctypes
import io
import os
import random
import statistics

import pytest

from duplexumiconsensusreads_amd import cli, native_io, params, synth
from oracle import dcr_oracle_c
from tests import filter_model as fm
from tests.test_ss_output import (PROCESSED, DEFAULT, _c_values, assert_records, failing_input, records, run,
                                  side_files, write_bam)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_DS = [r for c in PROCESSED for r in c["expect"]["ds"]]
WANT_SS = [r for c in PROCESSED for r in c["expect"]["ss"]]


def pct(values, p):
    v = sorted(values)
    return v[int(len(v) * p)]


def no_call_fraction(r):
    return r["seq"].count("N") / len(r["seq"])


def mean_quality(r):
    return sum(r["qual"]) / len(r["qual"])


def golden_filters():
    """Thresholds taken from the expected records themselves: each rule at
    the median of its own value, and all rules together at the quartile that
    lets three quarters of the records through."""
    sc = [fm.scalars(r) for r in WANT_DS]
    quals = sorted(q for r in WANT_DS for q in r["qual"])
    Q = quals[len(quals) // 10] + 1                      # masks at least a tenth of the bases
    masked = [fm.mask(fm.Filter(min_base_quality=Q), r)[0] for r in WANT_DS]
    tot, hi, lo = [a + b for a, b, *_ in sc], [max(a, b) for a, b, *_ in sc], [min(a, b) for a, b, *_ in sc]
    cE, sE = [s[4] for s in sc], [max(s[2], s[3]) for s in sc]
    med = statistics.median_high
    A, B = max(med(hi), med(lo)), med(lo)
    return {
        "mask": fm.Filter(min_base_quality=Q),
        "min_reads": fm.Filter(min_reads=(max(med(tot), A), A, B)),
        "error_rate": fm.Filter(max_read_error_rate=(med(cE), med(sE))),
        "no_call": fm.Filter(min_base_quality=Q, max_no_call_fraction=med(no_call_fraction(r) for r in masked)),
        "mean_qual": fm.Filter(min_base_quality=Q, min_mean_base_quality=med(mean_quality(r) for r in masked)),
        "all": fm.Filter(min_base_quality=Q, min_reads=(pct(tot, .25), pct(hi, .25), pct(lo, .25)),
                         max_read_error_rate=(pct(cE, .75), pct(sE, .75)),
                         max_no_call_fraction=pct([no_call_fraction(r) for r in masked], .75),
                         min_mean_base_quality=pct([mean_quality(r) for r in masked], .25)),
    }


FILTERS = golden_filters()
RULE_BIT = {"min_reads": fm.MIN_READS, "error_rate": fm.ERROR_RATE, "no_call": fm.NO_CALL, "mean_qual": fm.MEAN_QUAL}


def summary_lines(words):
    """What the CLI prints after the reference's four summary lines."""
    dropped = [w for w in words if w & 0xff]
    per = ", ".join("%s %d" % (name, sum(1 for w in dropped if w & bit))
                    for bit, name in ((1, "min_reads"), (2, "max_read_error_rate"), (4, "max_no_call_fraction"),
                                      (8, "min_mean_base_quality")))
    return ("\n A total of %d families (%.2f %%) were removed by the consensus filters.\n"
            "\n Families removed per rule: %s\n"
            "\n A total of %d bases were masked in the consensus reads that were written.\n"
            % (len(dropped), len(dropped) / len(words) * 100, per, sum(w >> 8 for w in words if not w & 0xff)))


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("filt") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.fixture(scope="module")
def plain(tmp_path_factory, golden_bam):
    """The unfiltered run, made before this module sets any filter."""
    out = str(tmp_path_factory.mktemp("filt_plain") / "plain.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out])
    assert exc is None
    return out, stdout


def files_bytes(out):
    return [open(out[:-4] + s, "rb").read() for s in (".bam", "_filteredreads.bam", "_filteredfamilies.bam")]


@pytest.mark.parametrize("name", list(FILTERS))
def test_golden_families(tmp_path, golden_bam, plain, name):
    flt = FILTERS[name]
    want, words = fm.apply(flt, WANT_DS)
    # the run is not vacuous
    dropped = [f for f, w in enumerate(words) if w & 0xff]
    if name == "mask":
        assert not dropped
    else:
        assert dropped and len(dropped) < len(words)
        one_only = [f for f in dropped
                    if sum(1 for r in WANT_DS[2 * f:2 * f + 2] if fm.reasons(flt, fm.mask(flt, r)[0])) == 1]
        assert one_only, "no family is dropped for one record alone"
        bits = RULE_BIT[name] if name in RULE_BIT else 15
        assert {b for b in (1, 2, 4, 8) if any(w & b for w in words)} == {b for b in (1, 2, 4, 8) if bits & b}
    if flt.min_base_quality is not None:
        assert sum(w >> 8 for w in words if not w & 0xff) > 0
    out, ss = str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    stats = {}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["-i", golden_bam, "-o", out, "--single_strand_output", ss, *flt.argv()], backend=dcr_oracle_c.run,
                 rng=random.Random(1), stats=stats)
    got = records(out)
    assert_records(got, want, "ds")
    # masking changed a base of a record that was written
    if flt.min_base_quality is not None:
        by_name = {r["qname"]: r for r in WANT_DS}
        assert any(g["seq"] != by_name[g["qname"]]["seq"] for g in got)
    assert_records(records(ss), fm.keep_ss(words, WANT_SS), "ss")
    assert side_files(out) == side_files(plain[0])
    assert buf.getvalue() == plain[1] + summary_lines(words)
    assert stats["consensus_records"] == len(want) and stats["consensus_bases"] == sum(len(r["seq"]) for r in want)
    assert stats["filter_dropped_families"] == len(dropped)
    assert stats["filter_masked_bases"] == sum(w >> 8 for w in words if not w & 0xff)


def test_thresholds_at_a_records_own_values_keep_it(tmp_path, golden_bam):
    """Equality passes: X = n / L as Python computes it, C = cE, S = the larger
    of aE and bE, T = aD + bD, Q = the mean quality, each the larger (smaller)
    of a family's two records so that the pair rule keeps the family."""
    assert any(no_call_fraction(r) not in (0.0, 1.0) for r in WANT_DS)
    cases = 0
    for f in range(0, len(WANT_DS) // 2, 61):
        pair = WANT_DS[2 * f:2 * f + 2]
        sc = [fm.scalars(r) for r in pair]
        if max(max(s[2:]) for s in sc) > 1.0:                # a single-strand E above 1: no option value reaches it
            continue
        flt = fm.Filter(min_reads=(min(a + b for a, b, *_ in sc), min(max(a, b) for a, b, *_ in sc),
                                   min(min(a, b) for a, b, *_ in sc)),
                        max_read_error_rate=(max(s[4] for s in sc), max(max(s[2], s[3]) for s in sc)),
                        max_no_call_fraction=max(no_call_fraction(r) for r in pair),
                        min_mean_base_quality=min(mean_quality(r) for r in pair))
        want, words = fm.apply(flt, WANT_DS)
        assert words[f] == 0
        out = str(tmp_path / f"eq{f}.bam")
        _, exc = run(["-i", golden_bam, "-o", out, *flt.argv()])
        assert exc is None
        got = records(out)
        assert_records(got, want, ("ds", f))
        assert pair[0]["qname"] in {r["qname"] for r in got}
        cases += 1
    assert cases >= 9


def test_batch_size_does_not_change_the_files(tmp_path, golden_bam):
    flt = FILTERS["all"]
    outs = []
    for tag, extra in (("a", []), ("b", ["--batch_reads", "300"])):
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        stdout, exc = run(["-i", golden_bam, "-o", out, "--single_strand_output", ss, *flt.argv(), *extra])
        assert exc is None
        outs.append((stdout, records(out), records(ss), side_files(out)))
    assert outs[0] == outs[1]
    assert len(outs[0][1]) == len(fm.apply(flt, WANT_DS)[0])


def test_default_is_off(tmp_path, golden_bam, plain):
    """Without a filter option: the same bytes in every output and the same
    stdout as before any filter was set in this process; no new stats key."""
    a = cli.parse_args(["-i", "x.bam"])
    assert params.ConsensusFilter.from_args(a) is None
    out, mid = str(tmp_path / "again.bam"), str(tmp_path / "mid.bam")
    _, exc = run(["-i", golden_bam, "-o", mid, *FILTERS["all"].argv()])
    assert exc is None
    stats = {}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["-i", golden_bam, "-o", out], backend=dcr_oracle_c.run, rng=random.Random(1), stats=stats)
    assert buf.getvalue() == plain[1]
    assert files_bytes(out) == files_bytes(plain[0])
    assert not any(k.startswith("filter_") for k in stats)
    assert stats["consensus_records"] == len(WANT_DS)
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("again")) == [
        "again.bam", "again_filteredfamilies.bam", "again_filteredreads.bam"]


@pytest.mark.parametrize("batch_reads", ["1048576", "40"])
def test_failing_family(tmp_path, batch_reads):
    """The families before the failing one are filtered as any other; the
    failure and everything printed for it stay as they are."""
    path, out, ss = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "sscs.bam")
    first = failing_input(path)
    ds20 = [r for c in first for r in c["expect"]["ds"]]
    sc = [fm.scalars(r) for r in ds20]
    flt = fm.Filter(min_base_quality=FILTERS["mask"].min_base_quality,
                    min_reads=(statistics.median_high(a + b for a, b, *_ in sc), 1, 1))
    want, words = fm.apply(flt, ds20)
    assert 0 < len(want) < 40
    stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, "--batch_reads", batch_reads, *flt.argv()])
    assert exc == "IndexError"
    assert_records(records(out), want, "ds")
    assert_records(records(ss), fm.keep_ss(words, [r for c in first for r in c["expect"]["ss"]]), "ss")
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "plain.bam"), "--batch_reads", batch_reads])
    assert (stdout0, exc0) == (stdout, exc)
    assert side_files(out) == side_files(str(tmp_path / "plain.bam"))


BAD = [["--filter_min_base_quality", "-1"], ["--filter_min_base_quality", "2.5"], ["--filter_min_base_quality", "x"],
       ["--filter_min_reads", "3,4"], ["--filter_min_reads", "5,3,4"], ["--filter_min_reads", "1,1,1,1"],
       ["--filter_min_reads", ""], ["--filter_min_reads", "2,"], ["--filter_min_reads", "2.0"],
       ["--filter_max_read_error_rate", "1.5"], ["--filter_max_read_error_rate", "-0.1"],
       ["--filter_max_read_error_rate", "0.1,0.2,0.3"], ["--filter_max_read_error_rate", "nan"],
       ["--filter_max_read_error_rate", "0.1,2"], ["--filter_max_no_call_fraction", "1.01"],
       ["--filter_max_no_call_fraction", "0.1,0.2"], ["--filter_max_no_call_fraction", "nan"],
       ["--filter_min_mean_base_quality", "-1"], ["--filter_min_mean_base_quality", "inf"],
       ["--filter_min_mean_base_quality", "nan"], ["--filter_min_mean_base_quality", "q"]]


@pytest.mark.parametrize("bad", BAD, ids=[" ".join(b) for b in BAD])
def test_malformed_values_exit_at_parse_time(tmp_path, bad, capsys):
    missing = str(tmp_path / "never_opened.bam")
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", missing, "-o", str(tmp_path / "out.bam"), *bad], backend=lambda *a: None)
    assert e.value.code == 2                                 # argparse's error, not the reference's exit(1)
    assert bad[0] in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_well_formed_values():
    a = cli.parse_args(["-i", "x.bam", "--filter_min_reads", "5", "--filter_max_read_error_rate", "0.25",
                        "--filter_min_base_quality", "0", "--filter_max_no_call_fraction", "1",
                        "--filter_min_mean_base_quality", "0"])
    f = params.ConsensusFilter.from_args(a)
    assert f.min_reads == (5, 5, 5) and f.max_read_error_rate == (0.25, 0.25) and f.active == 31
    assert cli.parse_args(["-i", "x.bam", "--filter_min_reads", "5,2"]).filter_min_reads == (5, 2, 2)
    assert params.ConsensusFilter.from_args(cli.parse_args(["-i", "x.bam", "--filter_min_base_quality", "0"])).active \
        == params.FILT_MASK_BASES                            # any one option turns the filter on


def test_two_gloo_ranks_write_the_same_files_and_summary(tmp_path):
    from tests.test_cli_shard import _outcome, run_sharded
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 600, sub_size="poisson5", seed=11, low_mapq_frac=0.1,
                                                   indel_frac=0.1, softclip_frac=0.1))
    base = ["--min_reads", "3", "--max_reads", "5"]

    def argv(tag, extra):
        return ["-i", path, "-o", str(tmp_path / f"{tag}.bam"), "--single_strand_output",
                str(tmp_path / f"{tag}_ss.bam"), *base, *extra]

    def files(tag):
        return [records(str(tmp_path / f"{tag}{s}.bam")) for s in ("", "_filteredreads", "_filteredfamilies", "_ss")]
    # thresholds from the unfiltered run's own records
    _, exc0, _ = _outcome(argv("all", []), 7)
    assert exc0 is None
    every = files("all")
    sc = [fm.scalars(r) for r in every[0]]
    Q = max(q for r in every[0] for q in r["qual"])          # masks every base below the commonest quality
    fractions = [no_call_fraction(fm.mask(fm.Filter(Q), r)[0]) for r in every[0]]
    flt = fm.Filter(min_base_quality=Q, min_reads=(pct([a + b for a, b, *_ in sc], .3), 1, 1),
                    max_read_error_rate=(pct([s[4] for s in sc], .8), 1.0),
                    max_no_call_fraction=statistics.median_low(x for x in fractions if x > 0))
    want, words = fm.apply(flt, every[0])
    assert 0 < len(want) < 2 * len(words)
    assert 0 < sum(w >> 8 for w in words if not w & 0xff) < sum(len(r["seq"]) for r in want)
    # (the masked records all hold one 'N' in 150 bases: the no-call bound sits exactly there and keeps them)
    assert all(any(w & b for w in words) for b in (1, 2))
    out1, exc1, st1 = _outcome(argv("one", flt.argv()), 7)
    part_dir = tmp_path / "parts"
    part_dir.mkdir()
    os.environ["DCR_PART_DIR"] = str(part_dir)
    try:
        got = run_sharded(argv("many", flt.argv()), 7, 2)
    finally:
        del os.environ["DCR_PART_DIR"]
    assert exc1 is None and got[0][:3] == (out1, exc1, st1)
    one, many = files("one"), files("many")
    for a, b in zip(many, one):
        assert a == b
    assert list(part_dir.iterdir()) == []
    assert_records(one[0], want, "ds")
    assert_records(one[3], fm.keep_ss(words, every[3]), "ss")
    assert one[1:3] == every[1:3]
    assert out1.endswith(summary_lines(words))


def test_ctypes_layouts_match_headers(tmp_path):
    from duplexumiconsensusreads_amd import _lib
    S = params.DcrFilter
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"),
                    ["sizeof(dcr_filter)", "offsetof(dcr_filter, active)", "offsetof(dcr_filter, min_base_quality)",
                     "offsetof(dcr_filter, min_reads)", "offsetof(dcr_filter, max_error_rate)",
                     "offsetof(dcr_filter, max_no_call_fraction)", "offsetof(dcr_filter, min_mean_base_quality)",
                     "DCR_FILT_MIN_READS", "DCR_FILT_ERROR_RATE", "DCR_FILT_NO_CALL", "DCR_FILT_MEAN_QUAL",
                     "DCR_FILT_MASK_BASES", "sizeof(dcr_wres)", "sizeof(dcr_wmeta)", "sizeof(dcr_out)",
                     "DCR_ABI_VERSION"], tmp_path)
    from duplexumiconsensusreads_amd.batch import DcrOut
    from duplexumiconsensusreads_amd.stream import WMeta, WRes
    assert got == [ctypes.sizeof(S), S.active.offset, S.min_base_quality.offset, S.min_reads.offset,
                   S.max_error_rate.offset, S.max_no_call_fraction.offset, S.min_mean_base_quality.offset,
                   params.FILT_MIN_READS, params.FILT_ERROR_RATE, params.FILT_NO_CALL, params.FILT_MEAN_QUAL,
                   params.FILT_MASK_BASES, ctypes.sizeof(WRes), ctypes.sizeof(WMeta), ctypes.sizeof(DcrOut), 1]
    assert [fm.MIN_READS, fm.ERROR_RATE, fm.NO_CALL, fm.MEAN_QUAL] == got[7:11]
    assert {"dcr_set_filter", "dcr_slot_filter_out"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dcr_set_filter") and hasattr(lib, "dcr_slot_filter_out") and lib.dcr_abi_version() == 1
    io_lib = native_io.load()
    assert all(hasattr(io_lib, n) for n in ("dcr_fmt_filter", "dcr_fmt_write_filt", "dcr_fmt_write_ss_filt"))
    assert io_lib.dcr_io_abi_version() == 1
