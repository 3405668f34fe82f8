"""The allele counts at given sites on the GPU (dcr_set_allele_sites:
k_allele_counts after the filters and before the formatters, into a table on
the context) against the host path (dcr_fmt_allele_counts over the kernel
outputs of dcr_submit, after the host overlap step and filter) and against the
model (tests/allele_counts_model.py) on the same batches, integer for integer;
the record bytes and BGZF members against a pass without the option, byte for
byte; and ``--allele_sites`` through the GPU CLI."""
import numpy as np
import pytest

from duplexumiconsensusreads_amd import _lib, bam, cli, native_io, params as params_mod, synth
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from duplexumiconsensusreads_amd.stream import DeviceStream
from tests import allele_counts_cases as ac
from tests import allele_counts_model as am
from tests import mate_overlap_cases as mc
from tests.test_gpu_mate_overlap import batches, check_stream, host_records, host_streams
from tests.test_ss_output import records, run

pytestmark = pytest.mark.gpu


def keys_of(sites):
    return np.array([(tid << 32) | pos for tid, pos in sorted(sites)], np.int64)


def written_records(hb, host, slot, n, fam_filt):
    """The duplex records of the kept families of [0, n) of a host result, as the model's dicts."""
    recs = host_records(hb, host.outs[slot].arr["ds"], n)
    out = []
    for f in range(n):
        if fam_filt is None or fam_filt[f] & 0xff == 0:
            out += [dict(r, tid=int(hb.a["fam_tid"][f])) for r in recs[2 * f:2 * f + 2]]
    return out


def check_run(tmp_path, path, sites, reads, min_q=0, ss_output=False, flt=None, mode=0, n_slots=2, fetch_after=None):
    """Every batch of ``path`` through the device writer without and with the
    sites set, and through dcr_submit + the host overlap step, filter and
    counter.  The streams of both device passes must be the same bytes (and
    the host formatter's); the device table must be the host's and the
    model's.  ``fetch_after``: also fetch after that many batches; the table
    so far must be the host's so far, and the run goes on.  Returns (the
    table, the records counted, the number of batches)."""
    params = ConsensusParams()
    sites = sorted(sites)
    keys = keys_of(sites)
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter, dev.mate_overlap = ss_output, flt, mode
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = ss_output
    with pytest.raises(_lib.DcrError):
        ctx.allele_counts()                                 # DCR_EARG without sites
    plain = []
    for hb in batches(path, params, reads, ss_output):
        res = dev.result(dev.submit(hb))
        plain.append((res.bgzf.tobytes(), res.record_bytes_of(hb.n_fam).tobytes(),
                      res.ss_bgzf.tobytes() if ss_output else None))
    dev.set_allele_sites(keys, min_q)
    assert not dev.allele_counts().any()                    # a fresh table
    want = np.zeros((len(keys), 8), np.uint64)
    counted = []
    n_batches = 0
    for b, hb in enumerate(batches(path, params, reads, ss_output)):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        assert not res.fam_fail.any(), "these inputs have no failing family"
        blocks, fetched = res.bgzf.tobytes(), res.record_bytes_of(F).tobytes()
        assert (blocks, fetched, res.ss_bgzf.tobytes() if ss_output else None) == plain[b]
        fam_filt = res.fam_filt.copy() if flt is not None else None
        n_blocks, n_bytes = res.blocks, res.record_bytes
        slot = host.submit(hb)
        ss, ds, rs = host.result(slot)
        assert native_io.first_failure(hb, ss, ds, F, rs)[0] == F
        if mode:
            native_io.apply_overlap(hb, ss, ds, mode, F)
        want_filt = native_io.apply_filter(hb, ss, ds, flt, F) if flt is not None else None
        if flt is not None:
            assert np.array_equal(fam_filt, want_filt)
        native_io.allele_counts(hb, ds, keys, min_q, F, want_filt, want)
        counted += written_records(hb, host, slot, F, want_filt)
        check_stream(blocks, fetched, host_streams(tmp_path, hb, ss, ds, F, want_filt, False)[0], n_blocks, n_bytes)
        n_batches += 1
        if fetch_after == n_batches:
            assert np.array_equal(dev.allele_counts(), want)        # and the table goes on accumulating
    got = dev.allele_counts()
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert np.array_equal(dev.allele_counts(), got)         # a fetch does not disturb the table
    assert got.tolist() == am.table(sites, counted, min_q)
    dev.set_allele_sites(None)
    with pytest.raises(_lib.DcrError):
        ctx.allele_counts()
    dev.close()
    host.close()
    ctx.close()
    return got, counted, n_batches


@pytest.mark.parametrize("shift", [0, 1000])
def test_hand_built_families(tmp_path, shift):
    path = ac.write_families(str(tmp_path / "in.bam"), ac.families(), shift)
    sites = ac.dense_sites(len(ac.ALL), shift)
    got, recs, n = check_run(tmp_path, path, sites, 1 << 12, ss_output=shift == 0)
    assert n == 1 and len(recs) == 2 * len(ac.ALL)
    tot = got.sum(axis=0)
    assert all(int(t) > 0 for t in tot), tot                # every column, both included
    # a quality threshold between the weak mate's and the others'
    got_q, _, _ = check_run(tmp_path, path, sites, 1 << 12, min_q=52)
    assert int(got_q[:, am.DISCORDANT].sum()) < int(got[:, am.DISCORDANT].sum())
    assert np.array_equal(got_q[:, :7].sum(axis=1), got[:, :7].sum(axis=1))


def test_many_families_on_the_same_sites(tmp_path):
    """300 copies of two families stacked on 20 sites in one batch: every
    update of a site's counters meets others; the totals are exact."""
    fams = ac.families(["identical", "deletion"]) * 300
    path = ac.write_families(str(tmp_path / "in.bam"), fams, shift=0)
    sites = [(0, p) for p in range(98, 118)]
    got, recs, n = check_run(tmp_path, path, sites, 1 << 14)
    assert n == 1 and len(recs) == 1200
    by_pos = {p: got[i].tolist() for i, (_, p) in enumerate(sites)}
    assert by_pos[98] == by_pos[99] == [0] * 8
    assert sum(by_pos[101][:7]) == 600 and by_pos[101][am.BOTH] == 600
    assert by_pos[100][am.DISCORDANT] == 300                # `identical` dissents at its first base
    assert by_pos[106][am.DISCORDANT] == 300 and by_pos[106][am.BOTH] == 600   # `deletion`: del against a base
    assert sum(by_pos[113][:7]) == 300 and by_pos[113][am.BOTH] == 0            # only `deletion`'s 16M mate
    assert by_pos[116] == by_pos[117] == [0] * 8


@pytest.fixture(scope="module")
def synth_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_ac_synth")
    synth.write_config_bam(str(d / "synth.bam"), synth.SynthConfig("t", 400, sub_size="poisson5", seed=9,
                                                                    indel_frac=0.3, softclip_frac=0.3))
    # the generator's mates read one template and never disagree: mate 2's reads are made to dissent
    path = mc.dissenting_copy(str(d / "synth.bam"), str(d / "in.bam"))
    # the span: every reference position an input read's alignment touches (the families lie
    # far apart, a few hundred positions each; the positions between them belong to no record)
    span = set()
    with bam.AlignmentFile(path, "rb") as f:
        refs = f.header.references
        for r in f:
            rec = r.to_dict()
            n = sum(int(n) for n, op in am.CIGAR_OP.findall(rec["cigar"] or "") if op in "M=XDN")
            span.update(range(rec["pos"], rec["pos"] + n))
    return path, sorted(span), refs


def longest_m_run(recs):
    return max(int(n) for r in recs for n, op in am.CIGAR_OP.findall(r["cigar"]) if op in "M=X")


@pytest.mark.parametrize("step", [7, 1])
def test_the_table_accumulates_over_batches_and_slots(tmp_path, synth_bam, step):
    path, span, _ = synth_bam
    sites = [(0, p) for p in span[::step]]
    got, recs, n = check_run(tmp_path, path, sites, 2000, ss_output=step == 7, fetch_after=2)
    assert n > 2                                            # both slots are reused
    assert 2 * 390 <= len(recs) <= 2 * 400
    # with every position a site, one M run holds more than 64 sites: the lanes stride more than once
    assert (longest_m_run(recs) > 64) and (step == 1 or longest_m_run(recs) // step < 64)
    tot = got.sum(axis=0)
    assert int(tot[am.DISCORDANT]) > 0 and int(tot[am.BOTH]) > 0 and int(tot[am.N]) > 0
    assert all(int(tot[c]) > 0 for c in (am.A, am.C, am.G, am.T))


def test_with_the_overlap_step_and_a_filter(tmp_path, synth_bam):
    """The table counts the records as they are written: after the overlap
    step, and without the families the filter drops."""
    path, span, _ = synth_bam
    sites = [(0, p) for p in span[::3]]
    flt = ConsensusFilter(min_base_quality=40, max_no_call_fraction=0.02)
    got, recs, n = check_run(tmp_path, path, sites, 2000, flt=flt, mode=params_mod.OVL_MASK)
    assert n > 2 and 0 < len(recs) < 2 * 390                # some families dropped, some kept
    plain, _, _ = check_run(tmp_path, path, sites, 2000)
    assert int(got[:, am.DISCORDANT].sum()) < int(plain[:, am.DISCORDANT].sum())
    assert int(got[:, :7].sum()) < int(plain[:, :7].sum())


def test_sparse_sites(tmp_path, synth_bam):
    path, span, _ = synth_bam
    # one site, well inside a read
    inside = set(span)
    one = next(p for p in span[len(span) // 2:] if p - 30 in inside and p + 30 in inside)
    got, recs, _ = check_run(tmp_path, path, [(0, one)], 2000)
    assert int(got[0, :7].sum()) > 0
    # sites no record touches: left of, between and right of the families, and the span on another reference id
    lo, hi, inside = span[0], span[-1], set(span)
    sites = [(0, p) for p in range(0, lo, max(lo // 50, 1))] + [(0, hi + 1 + p) for p in range(50)] + \
            [(0, p) for p in range(lo, hi, max((hi - lo) // 500, 1)) if p not in inside] + [(1, p) for p in span[::10]]
    assert len(sites) > 500
    got, _, _ = check_run(tmp_path, path, sites, 2000)
    assert not got.any()


def test_set_clear_set_gives_a_fresh_table(tmp_path):
    path = ac.write_families(str(tmp_path / "in.bam"), ac.families(), 1000)
    params = ConsensusParams()
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    (hb,) = list(batches(path, params, 1 << 12, False))
    first = keys_of(ac.dense_sites(len(ac.ALL), 1000))
    dev.set_allele_sites(first)
    dev.result(dev.submit(hb))
    a = dev.allele_counts()
    assert a.shape == (len(first), 8) and a.any()
    # bad keys are DCR_EARG and leave the table as it was
    for bad in ([5, 5], [9, 3], [-1], [1 << 31]):
        with pytest.raises(_lib.DcrError):
            ctx.set_allele_sites(np.array(bad, np.int64))
    with pytest.raises(_lib.DcrError):
        ctx.set_allele_sites(first, -1)
    assert np.array_equal(dev.allele_counts(), a)
    dev.set_allele_sites(None)
    plain = dev.result(dev.submit(hb)).bgzf.tobytes()
    with pytest.raises(_lib.DcrError):
        ctx.allele_counts()
    second = first[::2]
    dev.set_allele_sites(second)
    assert dev.allele_counts().shape == (len(second), 8) and not dev.allele_counts().any()
    assert dev.result(dev.submit(hb)).bgzf.tobytes() == plain
    assert np.array_equal(dev.allele_counts(), a[::2])
    # the same keys again: a fresh table again, and twice the batch gives twice the counts
    dev.set_allele_sites(second)
    assert not dev.allele_counts().any()
    dev.result(dev.submit(hb))
    dev.result(dev.submit(hb))
    assert np.array_equal(dev.allele_counts(), 2 * a[::2])
    dev.close()
    ctx.close()


# ---- the GPU CLI
def out_files(out, ss):
    return [open(p, "rb").read() for p in (out, out[:-4] + "_filteredreads.bam", out[:-4] + "_filteredfamilies.bam", ss)]


def test_gpu_cli_with_everything_on(tmp_path, synth_bam):
    """--mate_overlap consensus, --per_base_tags, a per-base filter and
    --single_strand_output: the table is the model's on the records as
    written, and every other output is the bytes of the run without the option."""
    from tests.test_allele_counts import read_tsv
    path, span, refs = synth_bam
    sites = [(0, p) for p in span[::2]]
    bed = ac.write_sites(str(tmp_path / "sites.bed"), sites, refs)
    be = cli.default_backend(ConsensusParams())
    opts = ["--mate_overlap", "consensus", "--per_base_tags", "--filter_min_base_reads", "4,2,1",
            "--filter_max_no_call_fraction", "0.05", "--batch_reads", "2000"]
    outs = {}
    for tag, extra in (("with", ["--allele_sites", bed, "--allele_counts_output", str(tmp_path / "with.tsv")]),
                       ("without", []), ("again", ["--allele_sites", bed, "--allele_counts_output",
                                                   str(tmp_path / "again.tsv"), "--allele_min_base_quality", "30"])):
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, *opts, *extra], backend=be)
        assert exc is None
        outs[tag] = (stdout, out_files(out, ss))
    assert outs["with"][1] == outs["without"][1] == outs["again"][1]
    written = records(str(tmp_path / "with.bam"))
    assert 0 < len(written) <= 2 * 400
    for tag, q in (("with", 0), ("again", 30)):
        got_sites, rows = read_tsv(str(tmp_path / f"{tag}.tsv"), refs)
        want = am.table(sites, written, q)
        assert got_sites == sites and rows == want
        assert open(str(tmp_path / f"{tag}.tsv")).read() == am.tsv(sites, want, refs)
        assert outs[tag][0] == outs["without"][0] + am.summary_line(want)
    assert not be.ctx.allele_sites                          # the kept backend does not keep the table


def test_gpu_cli_two_ranks_against_one_process(tmp_path, synth_bam):
    from tests.test_gpu_base_filter import _run_process
    path, span, refs = synth_bam
    sites = [(0, p) for p in span[::3]]
    bed = ac.write_sites(str(tmp_path / "sites.bed"), sites, refs)
    one, many = str(tmp_path / "one.bam"), str(tmp_path / "many.bam")
    opts = ["--allele_sites", bed, "--filter_max_no_call_fraction", "0.01"]
    rc1, out1 = _run_process(["-i", path, "-o", one, *opts, "--allele_counts_output", str(tmp_path / "one.tsv")])
    rc2, out2 = _run_process(["--gpus", "2", "-i", path, "-o", many, *opts, "--allele_counts_output",
                              str(tmp_path / "many.tsv")])
    assert rc1 == 0 and rc2 == 0 and out1 == out2
    tsv = open(str(tmp_path / "one.tsv"), "rb").read()
    assert open(str(tmp_path / "many.tsv"), "rb").read() == tsv
    written = records(one)
    assert records(many) == written
    rows = am.table(sites, written)
    assert tsv.decode() == am.tsv(sites, rows, refs) and out1.endswith(am.summary_line(rows))
    assert sum(r[am.DISCORDANT] for r in rows) > 0
