"""The errors against a genome on the GPU (dcr_set_genome: k_genome_metrics once
per level in k_base_metrics' place, into the slot's block) against the host
path (dcr_fmt_genome_metrics over the kernel outputs of dcr_submit) and against
the model (tests/genome_metrics_model.py) on the same batches, integer for
integer; the record bytes and BGZF members against a pass without the option,
byte for byte; and ``--genome`` through the GPU CLI."""
import json
import types

import numpy as np
import pytest

from duplexumiconsensusreads_amd import _lib, cli, native_io, params as params_mod, synth
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams, Genome
from duplexumiconsensusreads_amd.stream import DeviceStream
from tests import genome_metrics_cases as gc
from tests import genome_metrics_model as gm
from tests.test_genome_metrics import genome_object, same_tables
from tests.test_gpu_consensus_filter import batches
from tests.test_ss_output import FAM, PROCESSED, records, run, write_bam

pytestmark = pytest.mark.gpu


def random_genome(lengths, seed):
    """(params.Genome, the model's strings) of random codes, some of them 4."""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    codes = rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), size=int(off[-1]), p=[0.24, 0.24, 0.24, 0.24, 0.04])
    letters = np.frombuffer(b"ACGTN", np.uint8)[codes].tobytes().decode()
    return (Genome(codes, off, tuple("s%d" % i for i in range(len(lengths)))),
            [letters[int(off[t]):int(off[t + 1])] for t in range(len(lengths))])


def check_run(path, genome, strings, reads, n_slots=2, may_fail=False, model=True, **opts):
    """Every batch of ``path`` through the device writer without and with the
    genome set (``opts``: the other options of both passes), and through
    dcr_submit + the host count.  The streams of both device passes must be
    the same bytes; every batch's device block must be the host's and the
    model's.  Returns (the sum of the blocks, the batches' fam_fail)."""
    params = ConsensusParams()
    ss_output = opts.get("ss_output", False)
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    for k, v in opts.items():
        if k == "allele":
            dev.set_allele_sites(*v)
        else:
            setattr(dev, k, v)
    host = DeviceStream(ctx, device_writer=False)
    host.genome = genome                                    # the single-strand pos, n_cig and cigar come back too
    plain = []
    for hb in batches(path, params, reads, ss_output):
        res = dev.result(dev.submit(hb))
        assert res.genome_metrics is None
        plain.append((res.bgzf.tobytes(), res.record_bytes_of(hb.n_fam).tobytes(),
                      res.ss_bgzf.tobytes() if ss_output else None, res.fam_fail.copy()))
    if "allele" in opts:
        dev.set_allele_sites(*opts["allele"])               # a fresh table for the second pass
    dev.genome = genome
    total, fails = np.zeros(params_mod.GMET_WORDS, np.uint64), []
    for b, hb in enumerate(batches(path, params, reads, ss_output)):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        block, fam_fail = res.genome_metrics.copy(), res.fam_fail.copy()
        assert may_fail or not fam_fail.any(), "these inputs have no failing family"
        assert np.array_equal(fam_fail, plain[b][3])
        assert (res.bgzf.tobytes(), res.record_bytes_of(F).tobytes(),
                res.ss_bgzf.tobytes() if ss_output else None) == plain[b][:3]
        slot = host.submit(hb)
        ss, ds, rs = host.result(slot)
        want = native_io.genome_metrics(hb, ss, ds, genome, F, fam_fail)
        assert np.array_equal(block, want), np.flatnonzero(block != want)[:10]
        if model:
            arr = host.outs[slot].arr
            same_tables(block, gm.tables_of_arrays(types.SimpleNamespace(**arr["ss"]), types.SimpleNamespace(**arr["ds"]),
                                                   hb.a["ss_col_off"], hb.a["ds_col_off"], hb.a["fam_tid"], F, strings,
                                                   fam_fail))
        total += block
        fails.append(fam_fail)
    assert ctx.genome is genome
    dev.close()
    assert ctx.genome is None                               # set per run: closing frees the device copy
    host.close()
    ctx.close()
    return total, fails


@pytest.mark.parametrize("ss_output", [False, True])
def test_hand_built_families(tmp_path, ss_output):
    """Record lengths 1, 63, 64, 65, 130, 600 and 650; position 0, the last
    base of a sequence and a run past it; the second sequence and an absent
    one; an insertion first; deletions: one batch."""
    path = str(tmp_path / "in.bam")
    names = gc.write_all(path)
    total, fails = check_run(path, genome_object(), gc.GENOME, 1 << 14, ss_output=ss_output)
    assert len(fails) == 1 and len(fails[0]) == len(names)
    f = params_mod.genome_metrics_fields(total)
    assert f["n"][:, 0].tolist() == [4 * len(names), 2 * len(names)]
    assert all(int(v) > 0 for lv in range(2) for v in f["n"][lv][:10])
    assert f["cyc"][1, :, 0, 511].min() > 64 and f["n"][1, 8] >= 2 and f["n"][1, 5] >= 110


def test_a_failing_family_between_two_good_ones(tmp_path):
    crash = [c for c in FAM["cases"] if c["fam"] == 996]
    cases = PROCESSED[:3] + crash + PROCESSED[3:6]
    path = str(tmp_path / "in.bam")
    write_bam(path, cases)
    ends = [0] * 4
    for c in cases:
        for r in c["reads"]:
            ends[r["tid"]] = max(ends[r["tid"]], r["pos"] + 400)
    assert sum(ends) < 1 << 24
    genome, strings = random_genome(ends, 3)
    total, (fam_fail,) = check_run(path, genome, strings, 1 << 14, may_fail=True)
    assert fam_fail[3] != 0 and not fam_fail[:3].any() and not fam_fail[4:].any()
    assert params_mod.genome_metrics_fields(total)["n"][:, 0].tolist() == [24, 12]


def test_300_copies_of_one_family_in_one_batch(tmp_path):
    """Every add meets others on the same LDS bins; the totals are exact."""
    fams = gc.edge_families(["len130"]) * 300
    path = gc.write_families(str(tmp_path / "in.bam"), fams, moved=set())
    total, fails = check_run(path, genome_object(), gc.GENOME, 1 << 15, model=False)
    assert len(fails) == 1 and len(fails[0]) == 300
    one = gc.write_families(str(tmp_path / "one.bam"), fams[:1], moved=set())
    single, _ = check_run(one, genome_object(), gc.GENOME, 1 << 12)
    assert np.array_equal(total, 300 * single) and single[12 + 3] > 0      # n[1][3]: the duplex mismatches


@pytest.fixture(scope="module")
def synth_bam(tmp_path_factory):
    """600 generator families on 50 loci below position 1.5 M: no failing
    family on the oracle (checked on the CPU), several batches of 2000 reads."""
    d = tmp_path_factory.mktemp("gpu_gm_synth")
    path = str(d / "synth.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 600, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                   softclip_frac=0.3, n_loci=50))
    return path, random_genome([1_600_000], 7)


def test_generator_families_fill_every_bin_over_batches_and_slots(synth_bam):
    path, (genome, strings) = synth_bam
    total, fails = check_run(path, genome, strings, 2000, ss_output=True)
    assert len(fails) > 2 and sum(len(f) for f in fails) > 590       # both slots are reused
    f = params_mod.genome_metrics_fields(total)
    assert f["sub"].all() and f["tri"].all()
    # the duplex records of these families keep no insertion or deletion; the single-strand ones do
    assert all(int(v) > 0 for v in f["n"][0][:10]) and all(int(v) > 0 for v in f["n"][1][:6])
    used = f["qual"][:, 0] > 0
    assert used.sum(axis=1).min() >= 8 and ((f["qual"][:, 1] > 0) == used).all()    # every quality that occurs


def test_every_other_option_on_at_once(tmp_path, synth_bam):
    """The tables describe the consensus as called: the overlap step, the
    filters, the tags, the other tables and the allele counts change none of
    them."""
    path, (genome, strings) = synth_bam
    alone, _ = check_run(path, genome, strings, 2000, model=False)
    keys = (np.arange(1_000_000, 1_000_400, 3, dtype=np.int64), 20)
    flt = ConsensusFilter(min_base_quality=40, max_no_call_fraction=0.02, min_base_reads=(4, 2, 1))
    both, _ = check_run(path, genome, strings, 2000, model=False, ss_output=True, filter=flt,
                        mate_overlap=params_mod.OVL_CONSENSUS, base_tags=True, metrics=True, base_metrics=True,
                        allele=keys)
    assert np.array_equal(alone, both) and alone.any()


def test_set_clear_set(tmp_path):
    path = str(tmp_path / "in.bam")
    gc.write_all(path)
    params = ConsensusParams()
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    (hb,) = list(batches(path, params, 1 << 14, False))
    g = genome_object()
    dev.genome = g
    a = dev.result(dev.submit(hb)).genome_metrics.copy()
    assert a.any()
    # bad genomes are DCR_EARG and leave the state as it was
    lib = _lib.load()
    codes = np.ascontiguousarray(g.codes)
    for off, cs in (([0, 9, 5, 9], codes), ([1, 5, 9, 9], codes), ([0, 5, 9, 9], np.full(16, 5, np.uint8))):
        off = np.array(off, np.int64)
        assert lib.dcr_set_genome(ctx._ctx, cs.ctypes.data, off.ctypes.data, 3) != 0
    assert np.array_equal(dev.result(dev.submit(hb)).genome_metrics, a)
    dev.genome = None
    res = dev.result(dev.submit(hb))
    plain = res.bgzf.tobytes()
    assert res.genome_metrics is None and ctx.genome is None
    # another genome, then the first again: each batch's block is its own
    other = Genome(np.ascontiguousarray(g.codes[::-1]), g.ref_off, g.names)
    dev.genome = other
    res = dev.result(dev.submit(hb))
    b = res.genome_metrics.copy()
    assert res.bgzf.tobytes() == plain and not np.array_equal(a, b) and b[:2].tolist() == a[:2].tolist()
    dev.genome = g
    assert np.array_equal(dev.result(dev.submit(hb)).genome_metrics, a)
    assert np.array_equal(dev.result(dev.submit(hb)).genome_metrics, a)    # not a running total
    dev.close()
    ctx.close()


# ---- the GPU CLI
def out_files(out, ss):
    return [open(p, "rb").read() for p in (out, out[:-4] + "_filteredreads.bam", out[:-4] + "_filteredfamilies.bam", ss)]


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_gm_cli")
    names, fams = gc.overlap_families()
    path = gc.write_families(str(d / "in.bam"), fams * 2 + gc.edge_families(), moved=set(range(2 * len(fams))))
    return path, gc.write_fasta(str(d / "genome.fa"))


def test_gpu_cli_on_the_device_writer(tmp_path, cli_input):
    path, fasta = cli_input
    be = cli.default_backend(ConsensusParams())
    outs = {}
    for tag, opts in (("with", []), ("without", []),
                      ("all", ["--mate_overlap", "mask", "--per_base_tags", "--filter_min_base_reads", "4,2,1",
                               "--filter_max_no_call_fraction", "0.05", "--batch_reads", "100"])):
        extra = [] if tag == "without" else ["--genome", fasta, "--genome_metrics_output", str(tmp_path / f"{tag}.json")]
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, *opts, *extra], backend=be)
        assert exc is None
        outs[tag] = (stdout, out_files(out, ss))
    assert outs["with"][1] == outs["without"][1]
    t = gm.tables(records(str(tmp_path / "without_ss.bam")), records(str(tmp_path / "without.bam")), gc.GENOME)
    text = open(str(tmp_path / "with.json")).read()
    assert json.loads(text) == gm.document(t) and text == params_mod.genome_metrics_json(gm.words(t))
    assert outs["with"][0] == outs["without"][0] + gm.summary_line(t)
    # with the overlap step, the tags and the filters, in several batches: the same bytes
    assert open(str(tmp_path / "all.json")).read() == text and outs["all"][0].endswith(gm.summary_line(t))
    assert be.ctx.genome is None                            # the kept backend does not keep the genome


def test_gpu_cli_two_ranks_against_one_process(tmp_path, cli_input):
    from tests.test_gpu_base_filter import _run_process
    path, fasta = cli_input
    one, many = str(tmp_path / "one.bam"), str(tmp_path / "many.bam")
    rc1, out1 = _run_process(["-i", path, "-o", one, "--genome", fasta, "--genome_metrics_output",
                              str(tmp_path / "one.json")])
    rc2, out2 = _run_process(["--gpus", "2", "-i", path, "-o", many, "--genome", fasta, "--genome_metrics_output",
                              str(tmp_path / "many.json")])
    assert rc1 == 0 and rc2 == 0 and out1 == out2
    text = open(str(tmp_path / "one.json"), "rb").read()
    assert open(str(tmp_path / "many.json"), "rb").read() == text
    assert records(many) == records(one)
    doc = json.loads(text)
    assert doc["duplex"]["records"] == len(records(one)) and doc["duplex"]["mismatches"] > 20
    assert "Against the genome" in out1
