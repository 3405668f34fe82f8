"""``--metrics_output FILE.json``: the consensus QC tables (include/dcr.h
``dcr_metrics``) through the CLI against the restatement in
tests/metrics_model.py over the records the reference returned for the golden
families (tests/golden/families.json.gz ``expect["ds"]`` / ``["ss"]``).

CPU: every run uses the C oracle as the batch backend (test infrastructure);
the tables are counted by the native host path (dcr_fmt_metrics)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, native_io, params, synth
from oracle import dcr_oracle_c
from tests import metrics_model as mm
from tests.test_consensus_filter import FILTERS, WANT_DS, WANT_SS, files_bytes
from tests.test_ss_output import (BIG_FLAGS, DEFAULT, SAMPLED, _c_values, failing_input, records, run, side_files,
                                  subfamily_sizes, write_bam)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("met") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.fixture(scope="module")
def want():
    """The model over the reference's own records, computed once."""
    t = mm.tables(WANT_DS, WANT_SS)
    return t, mm.file_bytes(mm.document(t))


@pytest.fixture(scope="module")
def plain(tmp_path_factory, golden_bam):
    out = str(tmp_path_factory.mktemp("met_plain") / "plain.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out])
    assert exc is None
    return out, stdout


def test_the_golden_run_is_not_vacuous(want):
    t, _ = want
    assert t["n"][0] == 877 and all(v > 0 for v in t["n"][:6])
    for name in ("err_c", "err_s", "ss_qual", "ds_qual"):
        assert sum(1 for v in t[name] if v) >= 2, name
    assert all(sum(1 for v in row if v) >= 2 for row in t["ss_reads"])
    assert sum(1 for row in t["ds_depth"] for v in row if v) >= 2
    assert all(sum(1 for v in row if v) >= 2 for kind in t["col"] for row in kind)
    assert t["err_s"] != t["err_c"]
    # forward and reverse records both have columns
    for recs in (WANT_SS, WANT_DS):
        assert 0 < sum(1 for r in recs if r["flag"] & 16) < len(recs)


@pytest.mark.parametrize("batch_reads", ["1048576", "300"])
def test_golden_families(tmp_path, golden_bam, plain, want, batch_reads):
    out, met = str(tmp_path / "cons.bam"), str(tmp_path / "metrics.json")
    stdout, exc = run(["-i", golden_bam, "-o", out, "--metrics_output", met, "--batch_reads", batch_reads])
    assert exc is None
    got = open(met, "rb").read()
    assert json.loads(got) == mm.document(want[0])
    assert got == want[1]                       # the same bytes at every batch size
    # the flag changes nothing else (BGZF block boundaries follow the batches: records, not bytes)
    assert stdout == plain[1] and records(out) == records(plain[0]) and side_files(out) == side_files(plain[0])


def test_host_counters_word_for_word(golden_bam, want):
    """native_io.metrics over one batch of all the golden families: every one of the 10,716 words."""
    p = params.ConsensusParams()
    ing = native_io.Ingest(golden_bam, p.min_map_quality, p.min_reads, p.max_reads, p.min_base_quality)
    hb = native_io.HostBatch(reads=1 << 20)
    ing.next(hb)
    ing.close()
    assert hb.n_fam == 877
    ss, ds, _ = dcr_oracle_c.run(hb.packed(), p)
    words = native_io.metrics(hb, native_io.fmt_out(ss), native_io.fmt_out(ds), hb.n_fam)
    assert words.dtype == np.uint64 and words.tolist() == mm.flat(want[0])
    f = params.metrics_fields(words)
    assert f["col"].shape == (2, 3, 512) and f["ds_depth"].shape == (64, 64) and f["ss_reads"].shape == (4, 256)
    # fam_fail skips families: the first 10 alone, then everything but them
    ff = np.ones(hb.n_fam, np.int32)
    ff[:10] = 0
    a = native_io.metrics(hb, native_io.fmt_out(ss), native_io.fmt_out(ds), hb.n_fam, ff)
    b = native_io.metrics(hb, native_io.fmt_out(ss), native_io.fmt_out(ds), hb.n_fam, 1 - ff)
    assert a.tolist() == mm.flat(mm.tables(WANT_DS[:20], WANT_SS[:40])) and np.array_equal(a + b, words)
    assert np.array_equal(native_io.metrics(hb, native_io.fmt_out(ss), native_io.fmt_out(ds), 10), a)


def test_downsampled_families(tmp_path):
    """``ss_reads`` shows the sample sizes (--max_reads 6), not the input sizes."""
    c = SAMPLED[0]
    path, out, met = str(tmp_path / "in.bam"), str(tmp_path / "c.bam"), str(tmp_path / "m.json")
    write_bam(path, [c])
    _, exc = run(["-i", path, "-o", out, "--metrics_output", met, *BIG_FLAGS], rng=random.Random(c["expect"]["seed"]))
    assert exc is None
    doc = json.load(open(met))
    assert doc == mm.document(mm.tables(c["expect"]["ds"], c["expect"]["ss"]))
    sizes = [len(v) - 1 for v in doc["ss_reads"].values()]
    assert max(sizes) == 6 and max(subfamily_sizes(c)) > 6


@pytest.mark.parametrize("extra", ["filter", "ss_output", "both"])
def test_filters_and_single_strand_output_do_not_change_the_tables(tmp_path, golden_bam, want, extra):
    """The tables describe the consensus as called: counted before the filter masks and drops."""
    out, met = str(tmp_path / "cons.bam"), str(tmp_path / "metrics.json")
    argv = ["-i", golden_bam, "-o", out, "--metrics_output", met]
    if extra in ("filter", "both"):
        argv += FILTERS["all"].argv()
    if extra in ("ss_output", "both"):
        argv += ["--single_strand_output", str(tmp_path / "sscs.bam")]
    _, exc = run(argv)
    assert exc is None
    assert open(met, "rb").read() == want[1]
    if extra != "ss_output":
        assert len(records(out)) < len(WANT_DS)         # the filter did drop families


def test_default_is_no_metrics_file(tmp_path, golden_bam, plain):
    assert cli.parse_args(["-i", "x.bam"]).metrics_output is None
    out = str(tmp_path / "cons.bam")
    stdout, exc = run(["-i", golden_bam, "-o", out])
    assert exc is None and stdout == plain[1] and files_bytes(out) == files_bytes(plain[0])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cons.bam", "cons_filteredfamilies.bam",
                                                          "cons_filteredreads.bam"]


@pytest.mark.parametrize("batch_reads", ["1048576", "40"])
def test_failing_family_leaves_no_metrics_file(tmp_path, batch_reads):
    path, out, met = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam"), str(tmp_path / "metrics.json")
    failing_input(path)
    stdout, exc = run(["-i", path, "-o", out, "--metrics_output", met, "--batch_reads", batch_reads])
    assert exc == "IndexError" and not os.path.exists(met)
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "plain.bam"), "--batch_reads", batch_reads])
    assert (stdout0, exc0) == (stdout, exc)
    assert files_bytes(out) == files_bytes(str(tmp_path / "plain.bam"))


def test_bad_names(tmp_path, golden_bam, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", golden_bam, "-o", str(tmp_path / "cons.bam"), "--metrics_output", str(tmp_path / "m.txt")],
                 backend=dcr_oracle_c.run)
    assert e.value.code == 1
    assert cli.OUTPUT_FORMAT_ERROR in capsys.readouterr().out
    assert list(tmp_path.iterdir()) == []
    # a path that cannot be created fails before any output is written
    with pytest.raises(OSError):
        cli.main(["-i", golden_bam, "-o", str(tmp_path / "cons.bam"), "--metrics_output",
                  str(tmp_path / "no_such_dir" / "m.json")], backend=dcr_oracle_c.run)
    assert list(tmp_path.iterdir()) == []


def test_two_gloo_ranks_write_the_same_bytes(tmp_path):
    from tests.test_cli_shard import _outcome, run_sharded
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 600, sub_size="poisson5", seed=11, low_mapq_frac=0.1,
                                                   indel_frac=0.1, softclip_frac=0.1))

    def argv(tag):
        return ["-i", path, "-o", str(tmp_path / f"{tag}.bam"), "--metrics_output", str(tmp_path / f"{tag}.json"),
                "--single_strand_output", str(tmp_path / f"{tag}_ss.bam"), "--min_reads", "3", "--max_reads", "5"]
    out1, exc1, st1 = _outcome(argv("one"), 7)
    part_dir = tmp_path / "parts"
    part_dir.mkdir()
    os.environ["DCR_PART_DIR"] = str(part_dir)
    try:
        got = run_sharded(argv("many"), 7, 2)
    finally:
        del os.environ["DCR_PART_DIR"]
    assert exc1 is None and got[0][:3] == (out1, exc1, st1)
    one, many = open(tmp_path / "one.json", "rb").read(), open(tmp_path / "many.json", "rb").read()
    assert one == many
    # and they are the model's over the records this run wrote
    doc = mm.document(mm.tables(records(str(tmp_path / "one.bam")), records(str(tmp_path / "one_ss.bam"))))
    assert json.loads(one) == doc and doc["families"] > 100 and max(len(v) for v in doc["ss_reads"].values()) == 6


def test_struct_layout_matches_the_header(tmp_path):
    from duplexumiconsensusreads_amd import _lib
    M = params.DcrMetrics
    names = [n for n, _ in M._fields_]
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"),
                    ["sizeof(dcr_metrics)"] + [f"offsetof(dcr_metrics, {n})" for n in names]
                    + [f"sizeof(((dcr_metrics *)0)->{n})" for n in names]
                    + ["DCR_MET_READS_BINS", "DCR_MET_DEPTH_BINS", "DCR_MET_ERR_BINS", "DCR_MET_QUAL_BINS",
                       "DCR_MET_COL_BINS", "DCR_ABI_VERSION"], tmp_path)
    assert got == ([ctypes.sizeof(M)] + [getattr(M, n).offset for n in names] + [getattr(M, n).size for n in names]
                   + [params.MET_READS_BINS, params.MET_DEPTH_BINS, params.MET_ERR_BINS, params.MET_QUAL_BINS,
                      params.MET_COL_BINS, 1])
    assert ctypes.sizeof(M) == 85728 and params.MET_WORDS == 10716
    assert {"dcr_set_metrics", "dcr_slot_metrics_out"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dcr_set_metrics") and hasattr(lib, "dcr_slot_metrics_out")
    assert hasattr(native_io.load(), "dcr_fmt_metrics")
