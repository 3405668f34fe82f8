"""The per-base consensus filters on the CPU: the model
(tests/base_filter_model.py) against maps written out by hand for hand-built
families (tests/base_filter_cases.py), the rules on those families, the
command line options, the backends that cannot apply them, and the struct's
layout.  The device is compared against the model in
tests/test_gpu_base_filter.py."""
import ctypes
import os

import pytest

from duplexumiconsensusreads_amd import cli, params
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from oracle import dcr_oracle as O
from oracle import dcr_oracle_c
from tests import base_filter_model as bm
from tests.base_filter_cases import FAMILIES, MAPS, write_families
from tests.test_ss_output import _c_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.Params()
CORES = {name: bm.family(subs, P) for name, subs in FAMILIES.items()}


def test_every_family_is_called():
    assert set(MAPS) == set(FAMILIES) and all(res is not None for res in CORES.values())


@pytest.mark.parametrize("name", list(FAMILIES))
def test_map_of_the_hand_built_family(name):
    res = CORES[name]
    assert bm.base_map(res["ss"][0], res["ss"][1], res["ds"][0]) == MAPS[name]
    # duplex record 1 is called from two plain 10M subfamilies
    assert bm.base_map(res["ss"][2], res["ss"][3], res["ds"][1]) == [(c, c, c, c, c) for c in range(10)]


def test_the_shapes_are_the_ones_named():
    """The consensus strings the hand-written maps were derived from."""
    cons = {name: (res["ss"][0]["cons"], res["ss"][1]["cons"], res["ds"][0]["cons"]) for name, res in CORES.items()}
    assert cons["ends"] == ("NNGTTGCAAGCN", "ACGTTGCAAGCT", "ACGTTGCAAGCT")
    assert cons["5M2D5M"] == ("ACGTT--AAG", "ACGTT--AAG", "ACGTT--A")
    assert cons["ins_every_read"][0] == "ACGTTTGCAAG" and cons["ins_half"][0] == "ACGTTnGCAAG"
    assert cons["5M1I1D5M"] == ("ACGTTt-CAAG", "ACGTTt-CAAG", "ACGTTTCAAG")
    assert cons["5M1D1I5M"] == ("ACGTT-tCAAG", "ACGTT-tCAAG", "ACGTTTCAAG")
    assert CORES["5M1I1D5M"]["ss"][0]["cigar"] == [(0, 10)] and CORES["5M1D1I5M"]["ss"][0]["cigar"] == [(0, 10)]
    assert cons["a_del_b_not"] == ("ACGTT--AAG", "ACGTTGCAAGCT", "ACGTTGCAAGCT")
    assert cons["pos_a=pos_b+3"][2] == "ACGTTGCAAGCTT" and CORES["pos_a=pos_b+3"]["ss"][0]["pos"] == 103
    assert cons["a_weak_ins"] == ("ACGTTnGCAAG", "ACGTTGCAAG", "ACGTT+GCAAG")
    assert cons["ins_5_and_6"] == ("ACGTTtGCAAG", "ACGTTGnCAAG", "ACGTTtG+CAA")
    assert cons["ins_6_and_5"] == ("ACGTTnGCAAG", "ACGTTGtCAAG", "ACGTT+GtCAA")


def test_level_one_columns():
    assert bm.columns("NNGTTGCAAGCN") == (list(range(2, 11)), list(range(2, 11)), 12)
    assert bm.columns("ACGTTt-CAAG")[0] == [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]
    assert bm.columns("ACGTT-tCAAG")[0] == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    # a '+' column has no d-index: the bases after it keep consecutive d-indices, not alignment columns
    assert bm.columns("ACGTT+GtCAA") == (list(range(10)), [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], 10)
    # only upper-case N is trimmed; an all-N consensus has no base
    assert bm.columns("nACN")[0] == [0, 1, 2] and bm.columns("NNN") == ([], [], 3)


def masked(name, **rules):
    res = CORES[name]
    return bm.family_masks(bm.BaseFilter(**rules), res)[0]


def test_min_base_reads():
    # pos_a=pos_b+3: strand a has two reads on columns 3..12, strand b three on columns 0..9
    assert masked("pos_a=pos_b+3", min_base_reads=(4, 1, 0)) == [0, 1, 2, 10, 11, 12]
    assert masked("pos_a=pos_b+3", min_base_reads=(3, 3, 0)) == [10, 11, 12]
    assert masked("pos_a=pos_b+3", min_base_reads=(2, 2, 2)) == [0, 1, 2, 10, 11, 12]
    assert masked("pos_a=pos_b+3", min_base_reads=(5, 3, 2)) == [0, 1, 2, 10, 11, 12]
    assert masked("pos_a=pos_b+3", min_base_reads=(6, 1, 1)) == list(range(13))
    # a_del_b_not: strand a (two reads) has no base where it has the deletion and past its end;
    # its own '-' columns carry depth but are not the duplex bases' source
    assert masked("a_del_b_not", min_base_reads=(4, 1, 1)) == [5, 6, 10, 11]
    # ends: the two masked 5' columns and the undecided last column of strand a are outside its window
    assert masked("ends", min_base_reads=(4, 2, 2)) == [0, 1, 11]
    # the merged M: base 6 reads its strands' column 7 (depth 4 + 4), not column 6
    assert masked("5M1I1D5M", min_base_reads=(8, 4, 4)) == [5]          # the insertion column itself: 3 + 3
    assert masked("5M1D1I5M", min_base_reads=(8, 4, 4)) == [5]          # base 5 is the insertion here (column 6)
    # ins_half, base 5: aD = 2 of four reads, bD = 1 of two
    assert masked("ins_half", min_base_reads=(4, 2, 1)) == [5]


def test_max_base_error_rate_and_agreement():
    # ins_half, base 5: aE + bE = 4 + 2 over aD + bD = 2 + 1
    assert masked("ins_half", max_base_error_rate=1.0) == [5]
    assert masked("ins_half", max_base_error_rate=0.0) == [5]
    # exactly at the bound is kept: 1 + 1 errors over 3 + 3 reads
    assert masked("5M1I1D5M", max_base_error_rate=2 / 6) == [] and masked("5M1I1D5M", max_base_error_rate=0.33) == [5]
    # no reads and no errors: 0 > X * 0 is false
    assert masked("ends", max_base_error_rate=0.0) == []
    assert masked("pos_a=pos_b+3", require_strand_agreement=True) == [0, 1, 2, 10, 11, 12]
    assert masked("a_del_b_not", require_strand_agreement=True) == [5, 6, 10, 11]
    assert masked("ins_5_and_6", require_strand_agreement=True) == [5]
    assert masked("ins_6_and_5", require_strand_agreement=True) == [6]
    assert masked("5M2D5M", require_strand_agreement=True) == []


def test_union_with_the_quality_mask_counts_once():
    res = CORES["pos_a=pos_b+3"]
    rec = [dict(seq=r["seq"], qual=list(r["qual"]), tags=[("aD", "i", 2), ("bD", "i", 3), ("aE", "f", 0.0),
                                                           ("bE", "f", 0.0), ("cE", "f", 0.0)]) for r in res["ds"]]
    rec[0]["qual"][0], rec[0]["qual"][5] = 1, 7
    masks = [bm.family_masks(bm.BaseFilter(require_strand_agreement=True), res)]
    flt = bm.fm.Filter(min_base_quality=10, max_no_call_fraction=0.5)
    kept, words = bm.apply(flt, rec, masks)
    # bases 0 1 2 10 11 12 by the rule, 0 and 5 by quality: seven distinct bases, quality min(q, 2)
    assert words == [(7 << 8) | bm.fm.NO_CALL] and kept == []
    m, n = bm.mask_record(flt, rec[0], masks[0][0])
    assert n == 7 and m["seq"] == "NNNTTNCAAGNNN" and m["qual"][:3] == [1, 2, 2] and m["qual"][5] == 2
    # without the record rule the family stays, masked
    kept, words = bm.apply(bm.fm.Filter(min_base_quality=10), rec, masks)
    assert words == [7 << 8] and kept[0]["seq"] == "NNNTTNCAAGNNN" and kept[1] == rec[1]


# ---- the command line
def parse(*extra):
    return cli.parse_args(["-i", "x.bam", *extra])


def test_without_the_options_nothing_is_on():
    args = parse()
    assert args.filter_min_base_reads is None and args.filter_max_base_error_rate is None
    assert args.filter_require_strand_agreement is False
    assert ConsensusFilter.from_args(args) is None
    assert ConsensusFilter(min_reads=(3, 2, 1)).as_base_struct() is None


def test_option_parsing():
    f = ConsensusFilter.from_args(parse("--filter_min_base_reads", "6,3"))
    assert f.min_base_reads == (6, 3, 3) and f.active == 0 and f.base_active == params.BF_MIN_READS
    f = ConsensusFilter.from_args(parse("--filter_min_base_reads", "6,3,1", "--filter_max_base_error_rate", "0.125",
                                        "--filter_require_strand_agreement", "--filter_min_base_quality", "30"))
    assert (f.min_base_reads, f.max_base_error_rate, f.require_strand_agreement) == ((6, 3, 1), 0.125, True)
    assert f.base_active == 7 and f.active == params.FILT_MASK_BASES
    s = f.as_base_struct()
    assert (s.active, list(s.min_reads), s.max_error_rate) == (7, [6, 3, 1], 0.125)
    f = ConsensusFilter.from_args(parse("--filter_require_strand_agreement"))
    assert f is not None and f.base_active == params.BF_AGREEMENT and f.as_struct().active == 0
    assert bm.BaseFilter((6, 3, 1), 0.125, True).argv() == ["--filter_min_base_reads", "6,3,1",
                                                            "--filter_max_base_error_rate", "0.125",
                                                            "--filter_require_strand_agreement"]


@pytest.mark.parametrize("argv", [["--filter_min_base_reads", "3,4"], ["--filter_min_base_reads", "3,2,1,0"],
                                  ["--filter_min_base_reads", "x"], ["--filter_min_base_reads", ""],
                                  ["--filter_min_base_reads", "2.5"], ["--filter_max_base_error_rate", "1.5"],
                                  ["--filter_max_base_error_rate", "-0.1"], ["--filter_max_base_error_rate", "nan"],
                                  ["--filter_max_base_error_rate", "0.1,0.2"],
                                  ["--filter_require_strand_agreement", "1"]])
def test_malformed_values(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(*argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_backends_without_the_device_writer_refuse():
    flt = ConsensusFilter(min_base_reads=(3, 1, 1))
    with pytest.raises(ValueError, match="this backend cannot apply the per-base filters"):
        cli._as_backend(dcr_oracle_c.run, ConsensusParams(), flt=flt)

    class HostPath:                      # a stream backend whose records the host formats
        device_writer, filter, ss_output, metrics = False, None, False, False

        def submit(self, hb):
            raise AssertionError
    with pytest.raises(ValueError, match="this backend cannot apply the per-base filters"):
        cli._as_backend(HostPath(), ConsensusParams(), flt=flt)
    # the record rules alone are still taken
    be = cli._as_backend(HostPath(), ConsensusParams(), flt=ConsensusFilter(min_reads=(3, 1, 1)))
    assert be.filter == ConsensusFilter(min_reads=(3, 1, 1))


def test_oracle_backend_cli_refuses_before_any_output(tmp_path):
    path, out = write_families(str(tmp_path / "in.bam"), [FAMILIES["ends"]]), str(tmp_path / "cons.bam")
    with pytest.raises(ValueError, match="this backend cannot apply the per-base filters"):
        cli.main(["-i", path, "-o", out, "--filter_require_strand_agreement"], backend=dcr_oracle_c.run)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam"]
    # the same input without the option runs
    assert cli.main(["-i", path, "-o", out], backend=dcr_oracle_c.run) in (0, None)
    assert os.path.exists(out)


def test_struct_layout(tmp_path):
    S = params.DcrBaseFilter
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"),
                    ["sizeof(dcr_base_filter)", "offsetof(dcr_base_filter, active)",
                     "offsetof(dcr_base_filter, min_reads)", "offsetof(dcr_base_filter, max_error_rate)",
                     "DCR_BF_MIN_READS", "DCR_BF_ERROR_RATE", "DCR_BF_AGREEMENT", "sizeof(dcr_filter)",
                     "DCR_ABI_VERSION"], tmp_path)
    assert got == [ctypes.sizeof(S), S.active.offset, S.min_reads.offset, S.max_error_rate.offset,
                   params.BF_MIN_READS, params.BF_ERROR_RATE, params.BF_AGREEMENT, ctypes.sizeof(params.DcrFilter), 1]
    from duplexumiconsensusreads_amd import _lib
    assert "dcr_set_base_filter" in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "dcr_set_base_filter")
