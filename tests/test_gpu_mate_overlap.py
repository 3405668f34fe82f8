"""The overlapping mates on the GPU (dcr_set_mate_overlap: k_mate_overlap after
the QC tables and before the filters) against the host path
(dcr_fmt_mate_overlap, then the host filter and formatter over the kernel
outputs of dcr_submit) on the same batches, byte for byte: record bytes, BGZF
members and fam_ovl; and ``--mate_overlap`` through the GPU CLI against the
model (tests/mate_overlap_model.py), alone and composed with the filters, the
per-base tags and the QC tables."""
import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, native_io, params as params_mod, synth
from duplexumiconsensusreads_amd.bam import AlignmentFile
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from duplexumiconsensusreads_amd.records import AlignedSegment
from tests import base_filter_model as bm
from tests import mate_overlap_cases as mc
from tests import mate_overlap_model as mm
from tests.golden_io import input_record
from tests.test_gpu_consensus_filter import batches, check_stream, host_streams
from tests.test_ss_output import (DEFAULT, FAM, HEADER, PROCESSED, assert_records, failing_input, records, run,
                                  side_files, write_bam)

pytestmark = pytest.mark.gpu

MODES = {"mask": params_mod.OVL_MASK, "consensus": params_mod.OVL_CONSENSUS}
WANT_DS = [r for c in PROCESSED for r in c["expect"]["ds"]]
CIGAR_OPS = "MIDNSHP=X"


def host_records(hb, arr, n_fam):
    """The duplex records of families [0, n_fam) of host result arrays as the model's dicts."""
    off = hb.a["ds_col_off"]
    out = []
    for k in range(2 * n_fam):
        ro, n, nc = int(off[k]), int(arr["len"][k]), int(arr["n_cig"][k])
        out.append(dict(pos=int(arr["pos"][k]), seq=arr["seq"][ro:ro + n].tobytes().decode("latin-1"),
                        qual=arr["qual"][ro:ro + n].tolist(),
                        cigar="".join("%d%s" % (int(v) >> 4, CIGAR_OPS[int(v) & 15]) for v in arr["cigar"][ro:ro + nc])))
    return out


def check_batches(tmp_path, path, params, reads, mode, ss_output=False, flt=None, n_slots=2, last_fails=False):
    """Every batch of ``path`` through the device writer with the mode set, and
    through dcr_submit + the host step, filter and formatter.  Without a filter
    the single-strand stream must be the one of a pass without the mode.
    ``last_fails``: the input's last family fails; it must come back untouched.
    Returns per batch (fam_ovl [F, 3], fam_filt or None, the census of the
    batch's pairs before the step)."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter = ss_output, flt
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = ss_output
    plain_ss = []
    if ss_output and flt is None:
        for hb in batches(path, params, reads, ss_output):
            res = dev.result(dev.submit(hb))
            assert res.fam_ovl is None
            plain_ss.append((res.ss_bgzf.tobytes(), res.ss_record_bytes))
    dev.mate_overlap = MODES[mode]
    seen = []
    for b, hb in enumerate(batches(path, params, reads, ss_output)):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        n = F
        if last_fails and hb.end_kind != native_io.END_FULL:
            n = F - 1
            assert res.fam_fail[n] != 0 and res.fam_ovl[3 * n:].tolist() == [0, 0, 0]
        assert not res.fam_fail[:n].any()
        fetched = res.record_bytes_of(F).tobytes()          # before the slot is submitted again
        blocks, fam_ovl = res.bgzf.tobytes(), res.fam_ovl.copy()
        fam_filt = res.fam_filt.copy() if flt is not None else None
        if ss_output:
            ss_fetched, ss_blocks = res.ss_record_bytes_of(F).tobytes(), res.ss_bgzf.tobytes()
        slot = host.submit(hb)
        ss, ds, rs = host.result(slot)
        assert native_io.first_failure(hb, ss, ds, F, rs)[0] == n
        before = host_records(hb, host.outs[slot].arr["ds"], n)
        want_ovl = native_io.apply_overlap(hb, ss, ds, MODES[mode], n)      # rewrites the host copies in place
        assert np.array_equal(fam_ovl[:3 * n], want_ovl), np.flatnonzero(fam_ovl[:3 * n] != want_ovl)[:10]
        # the host step is the model's
        after, counts = mm.apply(mode, before)
        assert host_records(hb, host.outs[slot].arr["ds"], n) == after
        assert want_ovl.reshape(-1, 3).tolist() == [list(c) for c in counts]
        want_filt = native_io.apply_filter(hb, ss, ds, flt, n) if flt is not None else None
        if flt is not None:
            assert np.array_equal(fam_filt[:n], want_filt)
        want, want_ss = host_streams(tmp_path, hb, ss, ds, n, want_filt, ss_output)
        check_stream(blocks, fetched, want, res.blocks, res.record_bytes)
        if ss_output:
            check_stream(ss_blocks, ss_fetched, want_ss, res.ss_blocks, res.ss_record_bytes)
            if flt is None:
                assert (ss_blocks, res.ss_record_bytes) == plain_ss[b]
        seen.append((fam_ovl.reshape(-1, 3)[:n], None if fam_filt is None else fam_filt[:n], mm.census(before)))
    dev.close()
    host.close()
    ctx.close()
    return seen


@pytest.fixture(scope="module")
def synth_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_ovl_synth")
    synth.write_config_bam(str(d / "synth.bam"), synth.SynthConfig("t", 400, sub_size="poisson5", seed=9,
                                                                    indel_frac=0.3, softclip_frac=0.3))
    # the generator's mates read one template and never disagree: mate 2's reads are made to dissent
    return mc.dissenting_copy(str(d / "synth.bam"), str(d / "in.bam"))


@pytest.mark.parametrize("ss_output", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_streams_are_the_host_paths(tmp_path, synth_bam, mode, ss_output):
    seen = check_batches(tmp_path, synth_bam, ConsensusParams(), 2000, mode, ss_output)
    assert len(seen) > 2                                    # several batches: both slots are reused
    ovl = np.concatenate([s[0] for s in seen])
    assert 390 <= len(ovl) <= 400
    compared, disagree, changed = (int(v) for v in ovl.sum(axis=0))
    assert compared > 0 and disagree > 0 and changed > 0
    assert changed == 2 * disagree if mode == "mask" else changed > 2 * disagree
    for key in ("equal_q", "mate1_higher", "mate2_higher", "agree_sum_le_93", "skipped_n"):
        assert sum(s[2][key] for s in seen) > 0, key


def test_hand_built_families(tmp_path):
    path = mc.write_families(str(tmp_path / "in.bam"), mc.families())
    for mode in MODES:
        (got,) = check_batches(tmp_path, path, ConsensusParams(), 1 << 12, mode, ss_output=mode == "mask")
        ovl, _, census = got
        by_name = dict(zip(mc.CASES, ovl.tolist()))
        assert by_name["disjoint"] == by_name["adjacent"] == [0, 0, 0] and by_name["one_base"] == [1, 1, 2]
        assert census["shifted"] == 3 and census["mate1_higher"] == census["mate2_higher"] == 2


# ---- edge shapes: duplex lengths around the 64-lane stride with the mates at the same position and 1, 2, 3
# apart (the two records' words misaligned against each other); disagreements at the first and the last
# overlapping base and on both sides of the dword and the wave boundaries of either record; a family the
# filter drops and the family the reference fails next to kept ones
EDGE_LEN = [1, 63, 64, 65, 150, 151, 300]
EDGE_DELTA = [0, 1, 2, 3]


def edge_bam(path, failing_last):
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    spec = [(99, "A"), (163, "B"), (83, "B"), (147, "A")]                   # A1 B2 B1 A2
    fams = [(L, d, False) for L in EDGE_LEN for d in EDGE_DELTA]
    fams.insert(len(fams) // 2, (150, 2, True))                            # a dissenting read in A1: dropped by the error rate
    with AlignmentFile(path, "wb", header=HEADER) as out:
        for f, (L, delta, noisy) in enumerate(fams):
            tmpl = acgt[rng.integers(0, 4, L + 8)]
            P = 10_000 + 1_000 * f
            n_ov = L - delta
            flips = {i for i in (0, 3, 4, 63, 64, n_ov - 1, 3 - delta, 4 - delta, 63 - delta, 64 - delta)
                     if 0 <= i < n_ov}
            for k, (flag, strand) in enumerate(spec):
                start = delta if k >= 2 else 0
                for j in range(2 if noisy and k == 0 else 1):
                    r = AlignedSegment()
                    r.query_name = f"e{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = P + start
                    r.mapping_quality = 30
                    r.cigartuples = [(0, L)]
                    seq = tmpl[start:start + L].copy()
                    if k >= 2:                            # mate 2 dissents
                        idx = np.array(sorted(flips), np.int64)
                        seq[idx] = acgt[(np.searchsorted(acgt, seq[idx]) + 1) % 4]
                    if j == 1:
                        seq[2::5] = acgt[(np.searchsorted(acgt, seq[2::5]) + 1) % 4]
                    r.query_sequence = seq.tobytes().decode()
                    # one weak read per strand keeps the duplex qualities below the cap; the mates' follow
                    # different patterns: higher, lower and equal at the flips
                    r.query_qualities = [20 + ((3 * i) % 5 if k < 2 else (7 * i + 2) % 5) for i in range(L)]
                    r.set_tags([("MI", f"{5000 + f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)
        if failing_last:
            crash = [c for c in FAM["cases"] if c["fam"] == 996]
            assert len(crash) == 1 and crash[0]["expect"]["status"] == "crash:IndexError"
            for r in crash[0]["reads"]:
                out.write(input_record(r))
    return fams


@pytest.mark.parametrize("mode", list(MODES))
def test_edge_shapes(tmp_path, mode):
    path = str(tmp_path / "edge.bam")
    fams = edge_bam(path, failing_last=True)
    flt = ConsensusFilter(max_read_error_rate=(1.0, 0.0))
    (got,) = check_batches(tmp_path, path, ConsensusParams(), 1 << 13, mode, ss_output=True, flt=flt, last_fails=True)
    ovl, filt, census = got
    assert len(ovl) == len(fams)
    assert [bool(w & 0xff) for w in filt] == [noisy for _, _, noisy in fams]
    for (L, delta, _), (compared, disagree, changed) in zip(fams, ovl.tolist()):
        n_ov = max(L - delta, 0)
        flips = {i for i in (0, 3, 4, 63, 64, n_ov - 1, 3 - delta, 4 - delta, 63 - delta, 64 - delta) if 0 <= i < n_ov}
        assert compared <= n_ov and disagree <= len(flips)
        if n_ov == 0:
            assert (compared, disagree, changed) == (0, 0, 0)
    assert int(ovl[:, 1].sum()) > 100
    assert all(census[k] > 0 for k in ("equal_q", "mate1_higher", "mate2_higher"))


def test_edge_shapes_have_their_lengths(tmp_path):
    """The edge input gives the duplex lengths and positions it is built for (the oracle, no GPU work)."""
    from oracle import dcr_oracle_c
    path = str(tmp_path / "edge.bam")
    fams = edge_bam(path, failing_last=False)
    hb = next(iter(batches(path, ConsensusParams(), 1 << 13, False)))
    assert hb.n_fam == len(fams)
    _, ds, _ = dcr_oracle_c.run(hb.packed(), ConsensusParams())
    assert ds.len.tolist() == [L for L, _, _ in fams for _ in range(2)]
    assert [int(ds.pos[2 * f + 1] - ds.pos[2 * f]) for f in range(len(fams))] == [d for _, d, _ in fams]
    assert all(int(n) == 1 for n in ds.n_cig)


# ---- the GPU CLI
@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_ovl") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


def out_files(out):
    return [open(out[:-4] + s, "rb").read() for s in (".bam", "_filteredreads.bam", "_filteredfamilies.bam")]


@pytest.mark.parametrize("batch_reads", ["1048576", "300"])
@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_cli_golden_families(tmp_path, golden_bam, mode, batch_reads):
    be = cli.default_backend(ConsensusParams())
    want, counts = mm.apply(mode, WANT_DS)
    tot = mm.totals(counts)
    assert tot[1] == 1244
    out, plain, again = (str(tmp_path / f"{t}.bam") for t in ("cons", "plain", "again"))
    stdout, exc = run(["-i", golden_bam, "-o", out, "--batch_reads", batch_reads, "--mate_overlap", mode], backend=be)
    assert exc is None
    assert_records(records(out), want, "ds")
    # the same backend, kept by the process, without the option: the mode does not stay on its context
    stdout0, exc0 = run(["-i", golden_bam, "-o", plain, "--batch_reads", batch_reads], backend=be)
    assert exc0 is None and stdout == stdout0 + mc.summary_lines(tot)
    assert_records(records(plain), WANT_DS, "ds")
    assert side_files(plain) == side_files(out)
    # and with it again
    stdout2, exc2 = run(["-i", golden_bam, "-o", again, "--batch_reads", batch_reads, "--mate_overlap", mode],
                        backend=be)
    assert (stdout2, exc2) == (stdout, exc) and out_files(again) == out_files(out)


def test_gpu_cli_failing_family_in_mid_batch(tmp_path):
    path, out = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam")
    first = failing_input(path)
    want, counts = mm.apply("consensus", [r for c in first for r in c["expect"]["ds"]])
    assert mm.totals(counts)[1] > 0
    be = cli.default_backend(ConsensusParams())
    stdout, exc = run(["-i", path, "-o", out, "--mate_overlap", "consensus"], backend=be)
    assert exc == "IndexError"
    assert_records(records(out), want, "ds")
    assert (stdout, exc) == run(["-i", path, "-o", str(tmp_path / "plain.bam")], backend=be)


@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_cli_with_the_filters_the_tags_and_the_tables(tmp_path, mode):
    """Sequential composition: the per-base rules' masks come from the
    alignment (the model over the cores), the quality rule and the record rules
    see the bases as the step left them, the tags and both QC tables describe
    the consensus as called."""
    from tests.test_gpu_base_filter import _CASE_CORES, P, base_rules
    from tests.test_gpu_base_tags import tagged
    from tests import base_tags_model as tm
    from oracle import dcr_oracle as O
    cases = PROCESSED[:120]
    path = str(tmp_path / "in.bam")
    write_bam(path, cases)
    flt = ConsensusFilter(min_base_quality=40, min_base_reads=(5, 3, 1), max_no_call_fraction=0.3)
    opts = base_rules(flt).argv() + ["--filter_min_base_quality", "40", "--filter_max_no_call_fraction", "0.3",
                                     "--per_base_tags"]
    masks, tags = [], []
    for c in cases:
        if c["fam"] not in _CASE_CORES:
            _CASE_CORES[c["fam"]] = bm.family(O.split_family([r for r in c["reads"] if r["mapq"] >= 20]), P)
        masks.append(bm.family_masks(base_rules(flt), _CASE_CORES[c["fam"]]))
        tags += tm.family_tags(_CASE_CORES[c["fam"]])[0]
    called = [r for c in cases for r in c["expect"]["ds"]]
    step, counts = mm.apply(mode, called)
    assert mm.totals(counts)[1] > 0
    rules = bm.fm.Filter(flt.min_base_quality, flt.min_reads, flt.max_read_error_rate, flt.max_no_call_fraction,
                         flt.min_mean_base_quality)
    want, words = bm.apply(rules, [tagged(r, t) for r, t in zip(step, tags)], masks)
    want0, words0 = bm.apply(rules, [tagged(r, t) for r, t in zip(called, tags)], masks)
    kept = [w & 0xff == 0 for w in words]
    assert any(kept) and not all(kept) and words != words0
    be = cli.default_backend(ConsensusParams())
    files = {}
    for tag, extra in (("with", ["--mate_overlap", mode]), ("without", [])):
        out = str(tmp_path / f"{tag}.bam")
        met, bmet = str(tmp_path / f"{tag}_met.json"), str(tmp_path / f"{tag}_bmet.json")
        stdout, exc = run(["-i", path, "-o", out, "--batch_reads", "500", "--metrics_output", met,
                           "--base_metrics_output", bmet, *opts, *extra], backend=be)
        assert exc is None
        files[tag] = (stdout, records(out), open(met).read(), open(bmet).read())
    assert_records(files["with"][1], want, "ds")
    assert_records(files["without"][1], want0, "ds")
    assert files["with"][2:] == files["without"][2:] and len(files["with"][3]) > 100
    assert files["with"][0].endswith(mc.summary_lines(mm.totals(counts, kept)))


def test_gpu_cli_two_ranks_against_one_process(tmp_path, synth_bam):
    from tests.test_gpu_base_filter import _run_process
    one, many = str(tmp_path / "one.bam"), str(tmp_path / "many.bam")
    opts = ["--mate_overlap", "consensus", "--filter_max_no_call_fraction", "0.01"]
    rc1, out1 = _run_process(["-i", synth_bam, "-o", one, *opts])
    rc2, out2 = _run_process(["--gpus", "2", "-i", synth_bam, "-o", many, *opts])
    assert rc1 == 0 and rc2 == 0 and out1 == out2
    line = [ln for ln in out1.splitlines() if "held two different bases" in ln]
    assert len(line) == 1 and int(line[0].split()[3]) > 0
    for s in ("", "_filteredreads", "_filteredfamilies"):
        a, b = records(one[:-4] + s + ".bam"), records(many[:-4] + s + ".bam")
        assert len(a) == len(b) and a == b
    # the records are the model's over a run without the option, the dropped families' counters left out
    _, exc0 = run(["-i", synth_bam, "-o", str(tmp_path / "plain.bam")], backend=cli.default_backend(ConsensusParams()))
    assert exc0 is None
    step, counts = mm.apply("consensus", records(str(tmp_path / "plain.bam")))
    from tests import filter_model as fm
    want, words = fm.apply(fm.Filter(max_no_call_fraction=0.01), step)
    assert_records(records(one), want, "ds")
    assert out1.endswith(mc.summary_lines(mm.totals(counts, [w & 0xff == 0 for w in words])))
