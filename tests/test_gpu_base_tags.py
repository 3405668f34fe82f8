"""The per-base tags on the GPU (dcr_set_base_tags: k_fmt_size_tags /
k_fmt_write_tags and the _ss pair over the column maps
k_consensus_general_map stores) against the model
(tests/base_tags_model.py over the oracle's alignment), byte for byte: the
host formatter's records of the kernel outputs of dcr_submit, retagged with
the model's tags, must be the device writer's record bytes, and its BGZF
members the emulation's, for the duplex and the single-strand stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

from duplexumiconsensusreads_amd import bam, cli, native_io, stream, synth
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from oracle import dcr_oracle as O
from tests import base_filter_model as bm
from tests import base_tags_model as tm
from tests.base_filter_cases import FAMILIES, batch_subfamilies, write_families
from tests.test_gpu_base_filter import edge_bam, EDGE_LEN, out_files, run_cli
from tests.test_gpu_consensus_filter import batches, check_stream, host_streams
from tests.test_ss_output import DEFAULT, PROCESSED, assert_records, failing_input, records, write_bam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.Params()


def batch_tags(pk, n_fam, cache, key0, params=P):
    """``family_tags`` of families [0, n_fam) of a packed batch; the cores are kept in ``cache``."""
    out = []
    for f in range(n_fam):
        if key0 + f not in cache:
            cache[key0 + f] = bm.family(batch_subfamilies(pk, f), params)
        assert cache[key0 + f] is not None
        out.append(tm.family_tags(cache[key0 + f]))
    return out


def check_batches(tmp_path, path, params, reads, ss_output=True, n_slots=2, cache=None, flt=None, metrics=False,
                  oracle_params=P):
    """Every batch of ``path`` through the device writer with the tags on, and
    through the same writer without them (with ``flt`` and ``metrics`` as
    given) or, without a filter, dcr_submit + the host formatter; the second
    stream retagged with the model's tags must be the first.  Returns per batch
    (stored-map flags, fam_filt or None, metrics words or None, the decoded
    duplex records' tags)."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter, dev.metrics, dev.base_tags = ss_output, flt, metrics, True
    if flt is None:
        other = DeviceStream(ctx, device_writer=False)
    else:
        other = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
        other.filter, other.metrics = flt, metrics
    other.ss_output = ss_output
    cache = {} if cache is None else cache
    seen, key0 = [], 0
    for hb in batches(path, params, reads, ss_output):
        F = hb.n_fam
        handle = dev.submit(hb)
        res = dev.result(handle)
        assert not res.fam_fail.any(), "these inputs have no failing family"
        fetched, blocks = res.record_bytes_of(F).tobytes(), res.bgzf.tobytes()
        flags = np.zeros(6 * F, np.uint8)
        _lib._check(dev.lib.dcr_slot_fetch(ctx._ctx, handle[0], 6, 0, 6 * F, flags.ctypes.data))
        fam_filt = res.fam_filt.copy() if flt is not None else None
        words = res.metrics.copy() if metrics else None
        if ss_output:
            ss_fetched, ss_blocks = res.ss_record_bytes_of(F).tobytes(), res.ss_bgzf.tobytes()
        if flt is None:
            ss, ds, rs = other.result(other.submit(hb))
            assert native_io.first_failure(hb, ss, ds, F, rs)[0] == F
            want, want_ss = host_streams(tmp_path, hb, ss, ds, F, None, ss_output)
            kept = np.ones(F, bool)
        else:
            plain = other.result(other.submit(hb))
            want = plain.record_bytes_of(F).tobytes()
            want_ss = plain.ss_record_bytes_of(F).tobytes() if ss_output else None
            assert np.array_equal(plain.fam_filt, fam_filt)
            assert not metrics or np.array_equal(plain.metrics, words)
            kept = (fam_filt & 0xff) == 0
        tags = batch_tags(hb.packed(), F, cache, key0, oracle_params)
        want = tm.retag_stream(want, [t for f in range(F) if kept[f] for t in tags[f][0]])
        check_stream(blocks, fetched, want, res.blocks, res.record_bytes)
        if ss_output:
            want_ss = tm.retag_stream(want_ss, [t for f in range(F) if kept[f] for t in tags[f][1]])
            check_stream(ss_blocks, ss_fetched, want_ss, res.ss_blocks, res.ss_record_bytes)
        seen.append((flags, fam_filt, words, [tags[f][0] for f in range(F) if kept[f]]))
        key0 += F
    dev.close()
    other.close()
    ctx.close()
    return seen


def test_hand_built_families(tmp_path):
    path = write_families(str(tmp_path / "in.bam"), list(FAMILIES.values()))
    (got,) = check_batches(tmp_path, path, ConsensusParams(), 1 << 12)
    flags = got[0]
    assert len(flags) == 6 * len(FAMILIES) and flags.any() and not flags.all()      # stored maps and derived ones


def test_single_runs_at_the_dword_and_wave_boundaries(tmp_path):
    path = edge_bam(str(tmp_path / "edge.bam"))
    (got,) = check_batches(tmp_path, path, ConsensusParams(), 1 << 12)
    flags, _, _, tags = got
    assert not flags.any() and [len(t[0]["ad"]) for t in tags] == EDGE_LEN
    # duplex 1: three columns of strand a alone, then both, then three of strand b alone
    for t, L in zip(tags, EDGE_LEN):
        assert len(t[1]["ac"]) == L + 3 and t[1]["bc"][:3] == "NNN" and t[1]["ac"][-3:] == "NNN"
        assert t[1]["bd"][:3] == [0, 0, 0] and t[1]["ad"][-3:] == [0, 0, 0]
        assert min(t[1]["ad"][:min(L, 3)] + t[1]["bd"][-min(L, 3):]) > 0


_GOLDEN_CORES = {}


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_tags") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.mark.parametrize("batch_reads", [1 << 20, 300])
def test_golden_families(tmp_path, golden_bam, batch_reads):
    seen = check_batches(tmp_path, golden_bam, ConsensusParams(), batch_reads, cache=_GOLDEN_CORES)
    assert (len(seen) > 2) == (batch_reads == 300)
    flags = np.concatenate([s[0] for s in seen])
    tags = [t for s in seen for fam in s[3] for t in fam]
    assert len(tags) == 2 * 877 and flags.any() and not flags.all()
    assert any(t["ad"] != t["bd"] for t in tags)


def test_with_the_filters_and_the_metrics(tmp_path):
    """No filter touches what the tags are computed from: the tags of the
    families kept are the unfiltered run's, and fam_filt and the QC tables are
    those of a run without the tags (compared inside check_batches)."""
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 300, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                   softclip_frac=0.3))
    flt = ConsensusFilter(min_base_quality=60, min_base_reads=(8, 4, 2), require_strand_agreement=True,
                          min_reads=(8, 4, 2))
    cache = {}
    seen = check_batches(tmp_path, path, ConsensusParams(), 2000, flt=flt, metrics=True, cache=cache)
    free = check_batches(tmp_path, path, ConsensusParams(), 2000, cache=cache)
    assert len(seen) > 2 and len(seen) == len(free)
    dropped = masked = 0
    for a, b in zip(seen, free):
        kept = (a[1] & 0xff) == 0
        assert a[3] == [t for t, k in zip(b[3], kept) if k] and a[2].any()
        assert np.array_equal(a[0], b[0])
        dropped += int((~kept).sum())
        masked += int((a[1][kept] >> 8).sum())
    assert dropped > 0 and masked > 0 and sum(len(a[3]) for a in seen) > 0


# ---- the GPU CLI
def tagged(rec, tags):
    """A decoded record (AlignedSegment.to_dict) with the model's tags in place of its own."""
    return dict(rec, tags=[[t, "Z" if isinstance(tags[t], str) else "Bs", tags[t]] if t in tags else [t, c, v]
                           for t, c, v in rec["tags"]])


_CASE_CORES = {}


def model_records(cases):
    """(duplex, single-strand) records the reference wrote for the golden ``cases``, with the model's tags."""
    ds, ss = [], []
    for c in cases:
        if c["fam"] not in _CASE_CORES:
            _CASE_CORES[c["fam"]] = bm.family(O.split_family([r for r in c["reads"] if r["mapq"] >= 20]), P)
        t_ds, t_ss = tm.family_tags(_CASE_CORES[c["fam"]])
        ds += [tagged(r, t) for r, t in zip(c["expect"]["ds"], t_ds)]
        ss += [tagged(r, t) for r, t in zip(c["expect"]["ss"], t_ss)]
    return ds, ss


def test_cli_on_off_on_for_one_backend(tmp_path):
    cases = PROCESSED[:120]
    path = str(tmp_path / "in.bam")
    write_bam(path, cases)
    be = cli.default_backend(ConsensusParams())
    runs = {}
    for tag, extra in (("never", []), ("on", ["--per_base_tags"]), ("off", []), ("on_again", ["--per_base_tags"])):
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        stdout, exc = run_cli(["-i", path, "-o", out, "--single_strand_output", ss, "--batch_reads", "500", *extra], be)
        assert exc is None
        runs[tag] = (stdout, out_files(out, ss))
    assert runs["off"] == runs["never"] and runs["on_again"] == runs["on"]
    assert runs["on"][0] == runs["never"][0] and runs["on"][1][1:3] == runs["never"][1][1:3]      # stdout, side files
    want_ds, want_ss = model_records(cases)
    assert_records(records(str(tmp_path / "on.bam")), want_ds, "ds")
    assert_records(records(str(tmp_path / "on_ss.bam")), want_ss, "ss")
    assert_records(records(str(tmp_path / "off.bam")), [r for c in cases for r in c["expect"]["ds"]], "ds")


def test_cli_failing_family_in_mid_batch(tmp_path):
    """The reference raises IndexError at the 21st family; the 20 before it are written with their tags."""
    path, out = str(tmp_path / "in.bam"), str(tmp_path / "cons.bam")
    first = failing_input(path)
    be = cli.default_backend(ConsensusParams())
    stdout, exc = run_cli(["-i", path, "-o", out, "--per_base_tags"], be)
    assert exc == "IndexError"
    assert_records(records(out), model_records(first)[0], "ds")
    assert len(records(out)) == 40
    assert (stdout, exc) == run_cli(["-i", path, "-o", str(tmp_path / "plain.bam")], be)


def _run_process(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("DCR_SHARD", None)
    p = subprocess.run([sys.executable, "-m", "duplexumiconsensusreads_amd.cli", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    return p.returncode, p.stdout


def test_cli_two_ranks_against_one_process(tmp_path):
    path = str(tmp_path / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 1500, sub_size="poisson5", seed=21, low_mapq_frac=0.1,
                                                   indel_frac=0.2, softclip_frac=0.1))
    files = {}
    for tag, extra in (("one", []), ("many", ["--gpus", "2"])):
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        rc, stdout = _run_process([*extra, "-i", path, "-o", out, "--single_strand_output", ss, "--min_reads", "3",
                                   "--per_base_tags"])
        assert rc == 0
        files[tag] = (stdout, [bam.bgzf_stream(p) for p in (out, out[:-4] + "_filteredreads.bam",
                                                            out[:-4] + "_filteredfamilies.bam", ss)])
    assert files["one"] == files["many"]
    recs = records(str(tmp_path / "one.bam"))
    assert len(recs) > 0
    for r in recs:
        codes = {t: c for t, c, _ in r["tags"]}
        assert all(codes[t] == ("Z" if t[1] in "cq" else "Bs") for t in tm.DUPLEX_TAGS)
        assert all(len(v) == len(r["seq"]) for t, _, v in r["tags"] if t in tm.DUPLEX_TAGS)


# ---- capacity (csrc/dcr_capi.hip stream_bound): the record stream's bound holds for every batch whose
# records stay inside their regions, so the device buffers cannot be exceeded; the caller's pinned BGZF
# buffer is checked against the compressed size, and tagged records that do not fit take the refetch path
def bound(hb, ss_output):
    a, F = hb.a, hb.n_fam
    td = np.diff(a["ds_col_off"][:2 * F + 1]).astype(np.int64)
    ts = np.diff(a["ss_col_off"][:4 * F + 1]).astype(np.int64)
    nr = np.diff(a["sub_off"][:4 * F + 1]).astype(np.int64)
    lc = np.array([len(hb.name(a["fam_code"][f])) for f in range(F)])
    lr = np.array([len(hb.name(a["fam_rx"][k])) for k in range(2 * F)])
    ds = 400 * 2 * F + 4 * lc.sum() + lr.sum() + 22 * td.sum() + nr.sum()
    if not ss_output:
        return int(ds), None
    lm = sum(len(hb.name(a["sub_mi"][s])) + len(hb.name(a["sub_rx"][s])) for s in range(4 * F))
    return int(ds), int(160 * 4 * F + 4 * lc.sum() + lm + 10 * ts.sum() + nr.sum())


def test_pinned_capacity_takes_the_refetch_path(tmp_path, monkeypatch):
    path = edge_bam(str(tmp_path / "edge.bam"))
    real, asked = stream._WriterOut.ensure, []

    def small(self, n_fam, bgzf_bytes, *rest):
        # submit asks for its floor of 64 MiB: claim 256 bytes of it; the refetch asks for the real size
        asked.append(bgzf_bytes)
        real(self, n_fam, bgzf_bytes, *rest)
        if bgzf_bytes >= 64 << 20:
            self.cap_b = 256
    monkeypatch.setattr(stream._WriterOut, "ensure", small)
    (got,) = check_batches(tmp_path, path, ConsensusParams(), 1 << 12, n_slots=1)
    refetched = [n for n in asked if n < 64 << 20]
    assert len(refetched) == 2 and all(n > 256 for n in refetched)          # both streams, once each
    monkeypatch.setattr(stream._WriterOut, "ensure", real)
    # the device's own bound: every tagged stream is inside it
    from duplexumiconsensusreads_amd import _lib
    ctx = _lib.Context(ConsensusParams(), device=0)
    dev = stream.DeviceStream(ctx, device_writer=True)
    dev.ss_output = dev.base_tags = True
    for hb in batches(path, ConsensusParams(), 1 << 12, True):
        res = dev.result(dev.submit(hb))
        b_ds, b_ss = bound(hb, True)
        assert 0 < res.record_bytes <= b_ds and 0 < res.ss_record_bytes <= b_ss
    dev.close()
    ctx.close()


# ---- the clamp: a depth above the int16 range
def test_depth_above_the_int16_range_clamps(tmp_path):
    """One family whose A1 subfamily has 33,000 two-base reads (--max_reads 40000): valid on the CPU
    oracle, handled by the default path on the device, and its ad / sd entries clamp to 32767."""
    from oracle import dcr_oracle_c
    from tests.base_filter_cases import PLAIN, read
    from tests.test_ss_output import run
    fam = [[read(100, [(0, 2)])] * 33000, [read(100, [(0, 2)])] * 2, PLAIN, PLAIN]
    path = write_families(str(tmp_path / "in.bam"), [fam])
    flags = ["--max_reads", "40000", "--batch_reads", "65536"]
    outs = {}
    for tag, be in (("oracle", dcr_oracle_c.run), ("device", cli.default_backend(ConsensusParams(max_reads=40000)))):
        out, ss = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam")
        stdout, exc = run(["-i", path, "-o", out, "--single_strand_output", ss, *flags], backend=be)
        assert exc is None
        outs[tag] = (stdout, records(out), records(ss))
    assert outs["device"] == outs["oracle"] and len(outs["oracle"][1]) == 2            # the default path handles it
    assert ["ad", "Z", "[33000, 33000]"] in outs["oracle"][1][0]["tags"]
    (got,) = check_batches(tmp_path, path, ConsensusParams(max_reads=40000), 1 << 16)
    assert got[3][0][0]["ad"] == [32767, 32767] and got[3][0][0]["bd"] == [2, 2]
