"""``--genome`` / ``--genome_metrics_output``: the consensus as called against a
reference FASTA (include/dcr.h ``dcr_genome_metrics``): the FASTA loader, the
native host count (dcr_fmt_genome_metrics) against the spec restated in
tests/genome_metrics_model.py, and the CLI through the C oracle as the batch
backend (test infrastructure).  Every comparison is between integers or bytes:
exact equality throughout."""
import contextlib
import ctypes
import io
import json
import os
import random

import numpy as np
import pytest

from duplexumiconsensusreads_amd import _lib, cli, native_io, params
from oracle import dcr_oracle_c
from tests import genome_metrics_cases as gc
from tests import genome_metrics_model as gm
from tests.test_ss_output import PROCESSED, _c_values, failing_input, records, run, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQS = list(zip(gc.NAMES, gc.LENGTHS))


def codes_of(s):
    return [gm.base_code(c) for c in s]


def genome_object(strings=gc.GENOME):
    off = np.zeros(len(strings) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return params.Genome(np.array([c for s in strings for c in codes_of(s)], np.uint8), off,
                         tuple("s%d" % i for i in range(len(strings))))


def same_tables(words, t):
    got = params.genome_metrics_fields(words)
    for k in ("n", "sub", "tri", "cyc", "qual"):
        assert np.array_equal(got[k], t[k]), (k, np.argwhere(got[k] != t[k])[:8])
    assert np.array_equal(np.asarray(words), gm.words(t))


# ---- the FASTA loader
@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return gc.write_fasta(str(tmp_path_factory.mktemp("gm_fa") / "genome.fa"))


def check_loaded(g):
    assert g.codes.dtype == np.uint8 and g.ref_off.dtype == np.int64
    assert g.ref_off.tolist() == [0, gc.LENGTHS[0], gc.LENGTHS[0] + gc.LENGTHS[1], gc.LENGTHS[0] + gc.LENGTHS[1]]
    assert g.codes.tolist() == codes_of(gc.GENOME[0]) + codes_of(gc.GENOME[1])
    assert g.names == tuple(gc.NAMES) and g.load_s >= 0


def test_loader_keeps_the_header_sequences_in_header_order(fasta):
    g = params.load_genome(fasta, SEQS)
    check_loaded(g)                                         # chrC, which the file lacks, is absent: length 0
    assert set(np.unique(g.codes).tolist()) == {0, 1, 2, 3, 4}                  # lower case and IUPAC letters
    assert "n" in gc.GENOME[0] and "a" in gc.GENOME[0] and "R" in gc.GENOME[0]


@pytest.mark.parametrize("kw", [dict(width=7), dict(width=61, newline="\r\n"), dict(last_newline=False),
                                dict(width=100000, newline="\r\n", last_newline=False), dict(extra=False)],
                         ids=["short_lines", "crlf", "no_trailing_newline", "one_line_crlf", "no_extra_sequence"])
def test_loader_line_shapes(tmp_path, kw):
    check_loaded(params.load_genome(gc.write_fasta(str(tmp_path / "g.fa"), **kw), SEQS))


def test_loader_lines_of_varying_length(tmp_path):
    rng = random.Random(3)
    with open(tmp_path / "g.fa", "w") as f:
        for name, s in zip(gc.NAMES[:2], gc.GENOME[:2]):
            f.write(">%s\n" % name)
            i = 0
            while i < len(s):
                n = rng.randint(1, 90)
                f.write(s[i:i + n] + "\n")
                i += n
    check_loaded(params.load_genome(str(tmp_path / "g.fa"), SEQS))


def test_loader_with_and_without_a_fai(tmp_path, fasta):
    path = gc.write_fasta(str(tmp_path / "g.fa"))
    with open(path + ".fai", "w") as f:
        f.write("chrB\t%d\t6\t60\t61\n" % gc.LENGTHS[1])
    a, b = params.load_genome(path, SEQS), params.load_genome(fasta, SEQS)
    assert np.array_equal(a.codes, b.codes) and np.array_equal(a.ref_off, b.ref_off)


def test_loader_errors(tmp_path, fasta):
    with pytest.raises(ValueError, match="chrA.*header says %d" % (gc.LENGTHS[0] + 1)):
        params.load_genome(fasta, [("chrA", gc.LENGTHS[0] + 1), SEQS[1]])
    text = open(fasta).read()
    (tmp_path / "twice.fa").write_text(text + ">chrB again\nACGT\n")
    with pytest.raises(ValueError, match="'chrB' occurs twice"):
        params.load_genome(str(tmp_path / "twice.fa"), SEQS)
    for name in ("g.fa.gz", "g.fa.bgz"):
        (tmp_path / name).write_text(text)
        with pytest.raises(ValueError, match="compressed"):
            params.load_genome(str(tmp_path / name), SEQS)
    # a header sequence only: nothing of the file is kept
    g = params.load_genome(fasta, [("chrC", 700)])
    assert len(g.codes) == 0 and g.ref_off.tolist() == [0, 0]


def test_header_sequences():
    assert params.header_sequences(gc.HEADER.encode()) == SEQS


# ---- the host path against the model
def oracle_batch(path, reads=1 << 20):
    p = params.ConsensusParams()
    ing = native_io.Ingest(path, p.min_map_quality, p.min_reads, p.max_reads, p.min_base_quality)
    hb = native_io.HostBatch(reads=reads)
    ing.next(hb)
    ing.close()
    ss, ds, _ = dcr_oracle_c.run(hb.packed(), p)
    return hb, ss, ds


def host_words(hb, ss, ds, genome, n_fam, fam_fail=None):
    return native_io.genome_metrics(hb, native_io.fmt_out(ss), native_io.fmt_out(ds), genome, n_fam, fam_fail)


def model_of_arrays(hb, ss, ds, strings, n_fam, fam_fail=None):
    return gm.tables_of_arrays(ss, ds, hb.a["ss_col_off"], hb.a["ds_col_off"], hb.a["fam_tid"], n_fam, strings, fam_fail)


@pytest.fixture(scope="module")
def hand_built(tmp_path_factory):
    d = tmp_path_factory.mktemp("gm_cases")
    path = str(d / "in.bam")
    names = gc.write_all(path)
    return path, names, oracle_batch(path)


def test_hand_built_families_host_path_is_the_model(hand_built):
    path, names, (hb, ss, ds) = hand_built
    assert hb.n_fam == len(names) and not np.asarray(ss.status).any() and not np.asarray(ds.status).any()
    g = genome_object()
    same_tables(host_words(hb, ss, ds, g, hb.n_fam), model_of_arrays(hb, ss, ds, gc.GENOME, hb.n_fam))
    # family by family: fam_fail selects one
    for f, name in enumerate(names):
        ff = np.ones(hb.n_fam, np.int32)
        ff[f] = 0
        t = model_of_arrays(hb, ss, ds, gc.GENOME, hb.n_fam, ff)
        same_tables(host_words(hb, ss, ds, g, hb.n_fam, ff), t)
        assert t["n"][:, 0].tolist() == [4, 2], name


def cigar_text(rec):
    return "".join("%d%s" % (n, gm.OPS[op]) for op, n in rec["cigar"])


def family_tables(hand_built, name):
    path, names, (hb, ss, ds) = hand_built
    ff = np.ones(hb.n_fam, np.int32)
    ff[names.index(name)] = 0
    return model_of_arrays(hb, ss, ds, gc.GENOME, hb.n_fam, ff)


@pytest.mark.parametrize("name", list(gc.EDGES))
def test_edge_families_keep_their_shape(hand_built, name):
    path, names, (hb, ss, ds) = hand_built
    f = names.index(name)
    pos, cigar = gc.EDGES[name][1]
    for j in range(2):
        rec = ds.record(2 * f + j, hb.a["ds_col_off"])
        assert (rec["pos"], cigar_text(rec)) == (pos[j], cigar[j]), name


def test_edge_families_count_what_they_are_about(hand_built):
    path, names, (hb, ss, ds) = hand_built
    t = {name: family_tables(hand_built, name) for name in gc.EDGES}
    # the substitutions written into the reads are the mismatches, where the genome has a base; by cycle
    for name, L, sub in (("len63", (63, 63), ((62,), (0,))), ("len64", (64, 64), ((63,), (0,))),
                         ("len65", (65, 65), ((64,), (0, 64))), ("len130", (130, 130), ((64, 129), (127, 128))),
                         ("long", (600, 650), ((3, 510, 511, 512, 599), (0, 70, 138, 139, 140, 649)))):
        pos = gc.EDGES[name][1][0]
        n = t[name]["n"][1]
        want = np.zeros((2, 512), np.uint64)
        for j in range(2):
            for i in sub[j]:
                if gc.GENOME[0][pos[j] + i] in "ACGTacgt":
                    want[j, min(i if j == 0 else L[j] - 1 - i, 511)] += 1
        assert np.array_equal(t[name]["cyc"][1, :, 1], want), name
        assert n[3] == want.sum() >= len(sub[0]) + len(sub[1]) - 2 and n[1] == n[2] + n[3] + n[4] + n[5], (name, n)
    assert t["len1"]["n"][1, 1] == 2 and t["len1"]["n"][0, 1] == 4
    # the clamp: a whole 64-base step of both long mates lies at or past cycle 511
    cyc = t["long"]["cyc"][1]
    assert cyc[:, 0, 511].min() > 64 and cyc[0, 1, 511] >= 1 and cyc[1, 1, 511] >= 1
    # absent sequence: every base is genome_unknown; nothing in sub
    assert t["absent"]["n"][1, 5] == t["absent"]["n"][1, 1] == 100 and not t["absent"]["sub"].any()
    # past the end: exactly the ten positions past the last base
    assert t["past_end"]["n"][1, 5] - sum(c not in "ACGTacgt" for c in gc.GENOME[0][-50:-10]) - \
        sum(c not in "ACGTacgt" for c in gc.GENOME[0][-30:]) == 10
    # the first position has no 5' neighbour, the last no 3' neighbour: counted in sub, not in tri
    for name in ("pos0", "last_base"):
        assert t[name]["sub"].sum() > t[name]["tri"].sum() > 0
    assert t["second"]["n"][1, 3] == 2
    d = t["two_deletions"]["n"][1]
    assert d[8] == 2 and d[9] == 8 and d[3] == 1
    i = t["ins_first"]["n"]
    assert i[:, 6].tolist() == [1, 1] and i[:, 7].tolist() == [2, 2]       # the first operation of both levels' record


def random_records(hb, ss, ds, seed, n_ref):
    """Overwrite the result arrays with random records: every operation code
    (the unused ones too), len and n_cig below, at and above the region,
    negative pos, runs that pass a sequence's end, tid absent and out of range."""
    rng = random.Random(seed)
    for o, off in ((ss, hb.a["ss_col_off"]), (ds, hb.a["ds_col_off"])):
        for r in range(o.n_rec):
            ro, room = int(off[r]), int(off[r + 1]) - int(off[r])
            o.len[r] = rng.choice([room, room, room, rng.randint(0, room), room + rng.randint(1, 50), -3])
            ncig = rng.randint(0, min(room, 8))
            o.n_cig[r] = rng.choice([ncig, ncig, ncig, room + 7, -1])
            o.pos[r] = rng.choice([rng.randint(0, 400), rng.randint(0, 400), -rng.randint(1, 30), rng.randint(380, 460)])
            for i in range(room):
                op = rng.choice([0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15])
                o.cigar[ro + i] = (rng.choice([1, 2, 3, 30, 70, 200]) << 4) | op
                o.seq[ro + i] = ord(rng.choice("ACGTACGTACGTNacgtn*"))
                o.qual[ro + i] = rng.choice([0, 2, 20, 35, 41, 93, 255])
    for f in range(hb.n_fam):
        hb.a["fam_tid"][f] = rng.choice([0, 0, 1, 1, 2, n_ref, -1, 3])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_records_host_path_is_the_model(hand_built, seed):
    path, names, _ = hand_built
    hb, ss, ds = oracle_batch(path)
    rng = random.Random(100 + seed)
    strings = ["".join(rng.choice("ACGTNacgt") for _ in range(n)) for n in (430, 0, 395, 420)]
    random_records(hb, ss, ds, seed, len(strings))
    t = model_of_arrays(hb, ss, ds, strings, hb.n_fam)
    same_tables(host_words(hb, ss, ds, genome_object(strings), hb.n_fam), t)
    for lv in range(2):
        assert all(int(v) > 0 for v in t["n"][lv][:10]), t["n"][lv]
    assert t["tri"].any() and t["cyc"][:, :, 1].any() and t["qual"][:, 1, 255].any()


def test_host_entry_point_rejects_bad_arguments(hand_built):
    path, names, (hb, ss, ds) = hand_built
    g = genome_object()
    for off in ([1, 5, 6, 6], [0, 5, 4, 6]):
        bad = params.Genome(g.codes, np.array(off, np.int64), g.names)
        with pytest.raises(native_io.IOError_):
            host_words(hb, ss, ds, bad, hb.n_fam)
    with pytest.raises(native_io.IOError_):
        host_words(hb, ss, ds, g, hb.n_fam + 1)
    # the single-strand results without pos / n_cig / cigar
    so = native_io.fmt_out(ss)
    so.cigar = None
    with pytest.raises(native_io.IOError_):
        native_io.genome_metrics(hb, so, native_io.fmt_out(ds), g, hb.n_fam)


# ---- the CLI through the oracle backend
@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory, hand_built, fasta):
    """One run with the option and --single_strand_output, one without the option."""
    d = tmp_path_factory.mktemp("gm_cli")
    path = hand_built[0]
    out = {}
    for tag, extra in (("with", ["--genome", fasta, "--genome_metrics_output", str(d / "with.json")]), ("plain", [])):
        stdout, exc = run(["-i", path, "-o", str(d / f"{tag}.bam"), "--single_strand_output", str(d / f"{tag}_ss.bam"),
                           *extra])
        assert exc is None
        out[tag] = (stdout, str(d / f"{tag}.bam"), str(d / f"{tag}_ss.bam"))
    return d, out


def test_cli_json_is_the_model_over_the_written_records(cli_runs):
    d, out = cli_runs
    t = gm.tables(records(out["plain"][2]), records(out["plain"][1]), gc.GENOME)
    text = open(str(d / "with.json")).read()
    assert json.loads(text) == gm.document(t)
    assert text == params.genome_metrics_json(gm.words(t)) and text.endswith("}\n")
    assert not any(isinstance(v, float) for v in _leaves(json.loads(text)))
    assert t["n"][1, 3] > 20 and t["n"][0, 3] > 40 and t["n"][1, 8] > 0 and t["n"][0, 6] > 0
    # the summary gains one line; stdout before it is unchanged
    assert out["with"][0] == out["plain"][0] + gm.summary_line(t)


def _leaves(doc):
    if isinstance(doc, dict):
        doc = list(doc.values())
    if isinstance(doc, list):
        for v in doc:
            yield from _leaves(v)
    else:
        yield doc


def test_cli_changes_no_other_output_byte(cli_runs):
    d, out = cli_runs
    for k in (1, 2):
        assert open(out["with"][k], "rb").read() == open(out["plain"][k], "rb").read()
    for s in ("_filteredreads.bam", "_filteredfamilies.bam"):
        assert open(out["with"][1][:-4] + s, "rb").read() == open(out["plain"][1][:-4] + s, "rb").read()
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("plain")) == [
        "plain.bam", "plain_filteredfamilies.bam", "plain_filteredreads.bam", "plain_ss.bam"]


def test_cli_counts_the_single_strand_level_without_the_single_strand_file(tmp_path, cli_runs, hand_built, fasta):
    d, out = cli_runs
    stdout, exc = run(["-i", hand_built[0], "-o", str(tmp_path / "o.bam"), "--genome", fasta,
                       "--genome_metrics_output", str(tmp_path / "o.json"), "--batch_reads", "60",
                       "--mate_overlap", "mask", "--filter_min_reads", "4,2,2", "--metrics_output",
                       str(tmp_path / "m.json")])
    assert exc is None
    # several batches, the overlap step and a filter: the consensus as called, the same bytes
    assert open(str(tmp_path / "o.json"), "rb").read() == open(str(d / "with.json"), "rb").read()
    assert len(records(str(tmp_path / "o.bam"))) < len(records(out["plain"][1]))


def test_cli_default_is_off(tmp_path, hand_built):
    a = cli.parse_args(["-i", "x.bam"])
    assert (a.genome, a.genome_metrics_output) == (None, None)
    stats = {}
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        cli.main(["-i", hand_built[0], "-o", str(tmp_path / "o.bam")], backend=dcr_oracle_c.run,
                 rng=random.Random(1), stats=stats)
    assert "Against the genome" not in buf.getvalue() and "genome_load_s" not in stats
    assert sorted(p.name for p in tmp_path.iterdir()) == ["o.bam", "o_filteredfamilies.bam", "o_filteredreads.bam"]


def test_cli_reports_the_load_time(tmp_path, hand_built, fasta):
    stats = {}
    with contextlib.redirect_stdout(io.StringIO()):
        cli.main(["-i", hand_built[0], "-o", str(tmp_path / "o.bam"), "--genome", fasta, "--genome_metrics_output",
                  str(tmp_path / "o.json")], backend=dcr_oracle_c.run, rng=random.Random(1), stats=stats)
    assert stats["genome_load_s"] > 0


def test_cli_bad_options_open_nothing(tmp_path, hand_built, fasta, capsys):
    path, out = hand_built[0], str(tmp_path / "out.bam")
    js = str(tmp_path / "g.json")
    for extra in (["--genome", fasta], ["--genome_metrics_output", js]):
        with pytest.raises(ValueError, match="need each other"):
            cli.main(["-i", path, "-o", out, *extra], backend=dcr_oracle_c.run)
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", path, "-o", out, "--genome", fasta, "--genome_metrics_output", str(tmp_path / "g.txt")],
                 backend=dcr_oracle_c.run)
    assert e.value.code == 1 and cli.OUTPUT_FORMAT_ERROR in capsys.readouterr().out
    with pytest.raises(OSError):
        cli.main(["-i", path, "-o", out, "--genome", fasta, "--genome_metrics_output",
                  str(tmp_path / "missing" / "g.json")], backend=dcr_oracle_c.run)
    # a compressed FASTA, a wrong length, a name twice: before any output file exists
    text = open(fasta).read()
    (tmp_path / "short.fa").write_text(text.replace(">chrA", ">chrA_renamed") + ">chrA\nACGT\n")
    (tmp_path / "twice.fa").write_text(text + ">chrA\nACGT\n")
    (tmp_path / "g.fa.gz").write_text(text)
    for name, word in (("short.fa", "chrA"), ("twice.fa", "twice"), ("g.fa.gz", "compressed")):
        with pytest.raises(ValueError, match=word):
            cli.main(["-i", path, "-o", out, "--genome", str(tmp_path / name), "--genome_metrics_output", js,
                      "--metrics_output", str(tmp_path / "m.json")], backend=dcr_oracle_c.run)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["g.fa.gz", "short.fa", "twice.fa"]


@pytest.mark.parametrize("batch_reads", ["1048576", "40"])
def test_cli_a_reference_failure_leaves_no_file(tmp_path, batch_reads):
    """The golden families lie on chr1 .. chr4, which this FASTA lacks: every
    sequence absent, the run as far as the failing family, no JSON."""
    path = str(tmp_path / "in.bam")
    failing_input(path)
    (tmp_path / "other.fa").write_text(">chrOther\nACGTACGT\n")
    js = str(tmp_path / "g.json")
    stdout, exc = run(["-i", path, "-o", str(tmp_path / "o.bam"), "--genome", str(tmp_path / "other.fa"),
                       "--genome_metrics_output", js, "--batch_reads", batch_reads])
    assert exc == "IndexError" and not os.path.exists(js) and len(records(str(tmp_path / "o.bam"))) == 40
    stdout0, exc0 = run(["-i", path, "-o", str(tmp_path / "p.bam"), "--batch_reads", batch_reads])
    assert (stdout0, exc0) == (stdout, exc)
    # without the failing family the same FASTA gives a file: every base on an absent sequence
    write_bam(path, PROCESSED[:20])
    stdout, exc = run(["-i", path, "-o", str(tmp_path / "o.bam"), "--genome", str(tmp_path / "other.fa"),
                       "--genome_metrics_output", js])
    doc = json.loads(open(js).read())
    assert exc is None and doc["duplex"]["records"] == 40 and doc["single_strand"]["records"] == 80
    assert doc["duplex"]["genome_unknown"] == doc["duplex"]["aligned_bases"] > 0 and doc["duplex"]["matches"] == 0


def test_two_gloo_ranks_write_the_same_json(tmp_path, fasta):
    from tests.test_cli_shard import _outcome, run_sharded
    names, fams = gc.overlap_families()
    path = gc.write_families(str(tmp_path / "in.bam"), fams * 2 + gc.edge_families(),
                             moved=set(range(2 * len(fams))))

    def argv(tag):
        return ["-i", path, "-o", str(tmp_path / f"{tag}.bam"), "--genome", fasta, "--genome_metrics_output",
                str(tmp_path / f"{tag}.json"), "--single_strand_output", str(tmp_path / f"{tag}_ss.bam")]
    out1, exc1, st1 = _outcome(argv("one"), 7)
    part_dir = tmp_path / "parts"
    part_dir.mkdir()
    os.environ["DCR_PART_DIR"] = str(part_dir)
    try:
        got = run_sharded(argv("many"), 7, 2)
    finally:
        del os.environ["DCR_PART_DIR"]
    assert exc1 is None and got[0][:3] == (out1, exc1, st1)
    one = open(str(tmp_path / "one.json"), "rb").read()
    assert open(str(tmp_path / "many.json"), "rb").read() == one
    t = gm.tables(records(str(tmp_path / "one_ss.bam")), records(str(tmp_path / "one.bam")), gc.GENOME)
    assert one.decode() == params.genome_metrics_json(gm.words(t)) and out1.endswith(gm.summary_line(t))
    assert records(str(tmp_path / "many.bam")) == records(str(tmp_path / "one.bam"))
    assert list(part_dir.iterdir()) == []


def test_ctypes_layouts_match_headers(tmp_path):
    got = _c_values(os.path.join(ROOT, "include", "dcr.h"),
                    ["DCR_GMET_CYC_BINS", "DCR_GMET_QUAL_BINS", "sizeof(dcr_genome_metrics)",
                     "offsetof(dcr_genome_metrics, sub)", "offsetof(dcr_genome_metrics, tri)",
                     "offsetof(dcr_genome_metrics, cyc)", "offsetof(dcr_genome_metrics, qual)"], tmp_path)
    G = params.DcrGenomeMetrics
    assert got == [params.GMET_CYC_BINS, params.GMET_QUAL_BINS, ctypes.sizeof(G), G.sub.offset, G.tri.offset,
                   G.cyc.offset, G.qual.offset]
    assert params.GMET_WORDS == 6232 == len(gm.words(gm.new_tables()))
    assert {"dcr_set_genome", "dcr_slot_genome_metrics_out"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dcr_set_genome") and hasattr(lib, "dcr_slot_genome_metrics_out")
    assert hasattr(native_io.load(), "dcr_fmt_genome_metrics")
    assert params.GMET_N_NAMES == gm.N_NAMES and params.GMET_LEVELS == gm.LEVELS
