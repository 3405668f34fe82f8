"""The native ingest's run path on the CPU: the scanner pool cuts every
chunk's record index into runs (consecutive plain records of one MI prefix,
summed as a family; any other record a run of its own, marked slow) and the
walk takes a run that is a whole family in one step.  Each case is the
smallest input that reaches one seam of that path, read through the native
ingest and through the Python restatement of the same steps
(tests/test_native_io.py ``python_ingest``): every ``BATCH_FIELDS`` array,
both side streams, the counters and the generator state must be equal.

* excluded reads inside families: the runs are cut by slow records, the
  family arrives as several runs and goes through the per-record path;
* families of one read back to back, filtered and processed ones in turn;
* a family across the first chunk boundary (the first chunk holds 4 MiB of
  inflated bytes), at two block alignments, and a 1,000-read subfamily
  across it: the last run of an index is never taken as a whole family (its
  end is not known), or the family would come out in two pieces here;
* a batch that is full at a run: nothing of the run is consumed;
* families that sample between plain ones: the draws stay in input order;
* a family whose UMI check fails on the packer after families of the run
  path: the batch is cut where the per-record path cuts it.
"""
import random
import struct

import numpy as np
import pytest

from duplexumiconsensusreads_amd import bam, native_io, synth
from duplexumiconsensusreads_amd.batch import BATCH_FIELDS
from duplexumiconsensusreads_amd.params import ConsensusParams
from duplexumiconsensusreads_amd.records import AlignedSegment

from .test_native_io import concat, legacy_pass_filters, python_ingest

FIRST_CHUNK = 4 << 20          # inflated bytes the inflater asks for first (whole blocks, 64 KiB kept free)
HDR = bam.BamHeader("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])


def run_native(path, P, seed, reads):
    """Every batch of the native ingest: concat()'s tuples, and per batch
    (n_tab, n_reads, table); then the generator, the counters, the error."""
    rng = random.Random(seed)
    ing = native_io.Ingest(path, P.min_map_quality, P.min_reads, P.max_reads, P.min_base_quality, 4)
    ing.set_rng_state(rng.getstate())
    out, extra = [], []
    while True:
        hb = native_io.HostBatch(reads=reads, side_bytes=1 << 22)
        ing.next(hb)
        pk = hb.packed()
        out.append((hb.s.n_reads, hb.s.n_bases, hb.s.n_cigar, hb.s.ss_cols, hb.s.ds_cols,
                    {k: getattr(pk, k).copy() for k in BATCH_FIELDS}, hb.side("exc").tobytes(),
                    hb.side("filt").tobytes()))
        extra.append((hb.s.n_tab, hb.s.n_reads, [(k, s, c) for k, _, s, c, _, _ in hb.table()]))
        if hb.end_kind != native_io.END_FULL:
            break
    rng.setstate(ing.rng_state(rng.getstate()))
    counters = ing.counters()
    err = (hb.end_kind, *hb.error())
    ing.close()
    return out, extra, rng, counters, err


def assert_same(native, ref):
    out, _, rng2, counters, err = native
    pk, exc, filt, rng1 = ref
    assert err[0] == native_io.END_EOF
    got = concat(out)
    for k in BATCH_FIELDS:
        assert np.array_equal(got[k], getattr(pk, k)), k
    assert b"".join(o[6] for o in out) == b"".join(bam.encode_record(r) for r in exc)
    assert b"".join(o[7] for o in out) == b"".join(bam.encode_record(r) for r in filt)
    assert rng1.getstate() == rng2.getstate()
    assert counters["excluded"] == len(exc) and counters["processed"] == pk.n_fam
    assert counters["filtered"] == sum(k == native_io.FAM_FILTERED for _, _, tab in native[1] for k, _, _ in tab)
    if not any(s for _, _, tab in native[1] for _, s, _ in tab):     # no family sampled: every passing read is kept
        assert counters["passed"] == pk.n_reads + len(filt)
    assert counters["records"] == counters["passed"] + counters["excluded"]


def families(path, q=20):
    """[(passing reads, [excluded?, per record in input order])] per MI
    prefix of the file (the synthetic inputs keep a family's records together)."""
    fams, code = [], None
    with bam.AlignmentFile(path, "rb") as f:
        for r in f:
            c = r.get_tag("MI").split("/")[0]
            if c != code:
                fams.append([0, []])
                code = c
            fams[-1][0] += bool(legacy_pass_filters(r, q))
            fams[-1][1].append(not legacy_pass_filters(r, q))
    return fams


# -- excluded reads inside families, sampling between plain families ---------------
@pytest.fixture(scope="module", params=[0.02, 0.5])
def lowmapq(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("runs") / "p5.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 300, sub_size="poisson5", indel_frac=0.1, softclip_frac=0.1,
                                                   low_mapq_frac=request.param, seed=13))
    return path, request.param, {}


def cached_ref(cache, path, P, seed):
    key = (P.max_reads, P.min_reads, seed)
    if key not in cache:
        cache[key] = python_ingest(path, P, seed)
    return cache[key]


def test_excluded_reads_cut_the_runs(lowmapq):
    path, frac, cache = lowmapq
    if frac == 0.5:
        ex = [e for n, e in families(path) if n]
        assert any(e[0] for e in ex) and any(e[-1] for e in ex)
        assert any(any(e[1:-1]) for e in ex)
        assert any(any(a and b for a, b in zip(e, e[1:])) for e in ex)
    P = ConsensusParams()
    ref = cached_ref(cache, path, P, 3)
    for reads in (1 << 16, 300):
        assert_same(run_native(path, P, 3, reads), ref)


@pytest.mark.parametrize("max_reads", [3, 7])
def test_sampling_families_between_plain_ones(lowmapq, max_reads):
    path, _, cache = lowmapq
    P = ConsensusParams(max_reads=max_reads)
    ref = cached_ref(cache, path, P, 21)
    native = run_native(path, P, 21, 1 << 16)
    kinds = [s != 0 for _, _, tab in native[1] for _, s, _ in tab]
    assert any(kinds) and (max_reads == 3 or not all(kinds))     # at 3 nearly every poisson5 family samples
    assert_same(native, ref)
    assert_same(run_native(path, P, 21, 256), ref)


# -- hand-made families ---------------------------------------------------------------
def rec(name, flag, mi, rx, pos=100):
    r = AlignedSegment()
    r.query_name, r.flag, r.reference_id, r.reference_start = name, flag, 0, pos
    r.mapping_quality = 60
    r.cigartuples = [(0, 20)]
    r.query_sequence = "ACGT" * 5
    r.query_qualities = [30] * 20
    r.next_reference_id, r.next_reference_start = 0, pos
    r.set_tags([("MI", mi), ("RX", rx)])
    return r


def family(code, per_sub, rx=("AC", "GT"), bad=None):
    """per_sub reads in each of A1 (99), B2 (163), B1 (83), A2 (147); bad: index of a read with another RX"""
    out = []
    for flag in (99, 163, 83, 147)[:4 if per_sub else 1]:
        strand = "A" if flag in (99, 147) else "B"
        for j in range(max(per_sub, 1)):
            u = f"{rx[0]}-{rx[1]}" if strand == "A" else f"{rx[1]}-{rx[0]}"
            out.append(rec(f"{code}_{flag}_{j}", flag, f"{code}/{strand}", u, pos=100 + len(out)))
    if bad is not None:
        out[bad].set_tags([("MI", out[bad].get_tag("MI")), ("RX", "TT-TT")])
    return out


def write_bam(path, fams):
    with bam.AlignmentFile(path, "wb", header=HDR) as out:
        for fam in fams:
            for r in fam:
                out.write(r)
    return path


@pytest.mark.parametrize("min_reads", [1, 3])
def test_runs_of_length_one_back_to_back(tmp_path, min_reads):
    """Families of a single read (three subfamilies empty: filtered at any
    min_reads) back to back, between families of 4 x 1 and 4 x 3 reads."""
    fams = []
    for k in range(40):
        fams += [family(f"s{k}a", 0), family(f"s{k}b", 0), family(f"f{k}", 3 if k % 2 else 1), family(f"s{k}c", 0)]
    path = write_bam(str(tmp_path / "ones.bam"), fams)
    P = ConsensusParams(min_reads=min_reads)
    ref = python_ingest(path, P, 1)
    assert ref[0].n_fam == (20 if min_reads == 3 else 40)
    for reads in (1 << 12, 16):
        native = run_native(path, P, 1, reads)
        assert_same(native, ref)
        kinds = [k for _, _, tab in native[1] for k, _, _ in tab]
        assert len(kinds) == 160 and len(set(kinds[:8])) == 2     # filtered and processed in turn


def test_failing_family_after_run_path_families(tmp_path):
    """A family with one mismatched RX in the middle of the input: its check
    fails on the packer, after the families before it were queued.  The batch
    holds exactly those families (the restatement of the input cut before the
    failing family), the counters stand after the failing family's reads, and
    kind and message are those of the same family at the head of an input."""
    good = [family(f"g{k}", 2, rx=("AC", "GT")) for k in range(31)]
    bad = family("bad", 2, bad=5)
    mid = write_bam(str(tmp_path / "mid.bam"), good[:15] + [bad] + good[15:])
    head = write_bam(str(tmp_path / "head.bam"), [bad] + good)
    prefix = write_bam(str(tmp_path / "prefix.bam"), good[:15])
    P = ConsensusParams()
    pk, _, _, _ = python_ingest(prefix, P, 1)
    res = {}
    for name, path in (("mid", mid), ("head", head)):
        for reads in (1 << 12, 64):
            out, extra, _, counters, err = run_native(path, P, 1, reads)
            res[name, reads] = (out, extra, counters, err)
            assert err[0] == native_io.END_ERROR and err[1] == "exit"
            assert "ERROR: family bad has different UMI tags" in err[2]
    assert len({r[3] for r in res.values()}) == 1                  # one kind, one message
    for reads in (1 << 12, 64):
        out, extra, counters, _ = res["mid", reads]
        got = concat(out)
        for k in BATCH_FIELDS:
            assert np.array_equal(got[k], getattr(pk, k)), k
        assert sum(e[0] for e in extra) == 15
        assert [counters[k] for k in ("passed", "records", "processed", "filtered", "excluded")] == [128, 128, 15, 0, 0]
        out, extra, counters, _ = res["head", reads]
        assert [e[0] for e in extra] == [0] and out[0][0] == 0
        assert [counters[k] for k in ("passed", "records", "processed", "filtered", "excluded")] == [8, 8, 0, 0, 0]


# -- the first chunk boundary, batches full at a run -------------------------------------
def record_starts(stream):
    """offsets of the records of an inflated BAM stream, and where they end"""
    l_text, = struct.unpack_from("<i", stream, 4)
    n_ref, = struct.unpack_from("<i", stream, 8 + l_text)
    p = 12 + l_text
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    starts = []
    while p < len(stream):
        starts.append(p)
        p += 4 + struct.unpack_from("<i", stream, p)[0]
    return starts, p


def rewrite(path, header, records):
    w = bam.BGZFWriter(path, level=1)
    w.write(header)
    w.write(records)
    w.close()
    return path


def first_boundary(path):
    """inflated bytes in the ingest's first chunk: whole BGZF blocks while 64 KiB more would fit"""
    total = 0
    data = open(path, "rb").read()
    p = 0
    while p < len(data) and total + 0x10000 <= FIRST_CHUNK:
        bsize, = struct.unpack_from("<H", data, p + 16)
        total += struct.unpack_from("<I", data, p + bsize + 1 - 4)[0]
        p += bsize + 1
    return total


@pytest.fixture(scope="module")
def fixed8(tmp_path_factory):
    """640 fixed8 families of 2 x 150 bp (20,480 reads, ~6 MB inflated: one
    chunk boundary inside), as records; the restatement's result for them;
    and the records of one family of 4 x 1,000 reads."""
    d = tmp_path_factory.mktemp("fixed8")
    src = str(d / "src.bam")
    synth.write_packed_bam(src, synth.packed_fixed_size(640, seed=9), seed=9, level=1)
    stream = bam.bgzf_stream(src)
    starts, end = record_starts(stream)
    assert len(starts) == 640 * 32 and end == len(stream)
    big = str(d / "big.bam")
    synth.write_packed_bam(big, synth.packed_fixed_size(1, sub_size=1000, seed=4), seed=4, level=1, fam_id0=100_000)
    bstream = bam.bgzf_stream(big)
    bstarts, bend = record_starts(bstream)
    assert len(bstarts) == 4000
    fx = {"dir": d, "src": src, "header": stream[:starts[0]], "records": stream[starts[0]:], "starts": starts,
          "big": bstream[bstarts[0]:bend], "ref": python_ingest(src, ConsensusParams(), 5), "pad": {}}
    # the same records behind a header `pad` bytes longer: the chunk boundary
    # falls into another family, in the middle of it
    offs = np.array(starts) - starts[0]
    for pad in (0, 4800):
        text = HDR.text + ("@CO\t" + "x" * (pad - 5) + "\n" if pad else "")
        header = bam.BamHeader(text, HDR.references, HDR.lengths).encode()
        path = rewrite(str(d / f"pad{pad}.bam"), header, fx["records"])
        cut = first_boundary(path) - len(header)                  # offset in the records
        i = int(np.searchsorted(offs, cut, side="right")) - 1     # the record the boundary falls into
        assert 0 < cut < len(fx["records"]) and 2 <= i % 32 <= 29, (cut, i)
        fx["pad"][pad] = (path, i // 32)
    assert fx["pad"][0][1] != fx["pad"][4800][1]
    return fx


@pytest.mark.parametrize("pad", [0, 4800])
def test_family_across_the_first_chunk_boundary(fixed8, pad):
    path, _ = fixed8["pad"][pad]
    for reads in (1 << 16, 5000):
        assert_same(run_native(path, ConsensusParams(), 5, reads), fixed8["ref"])


def test_thousand_read_subfamily_across_the_boundary(fixed8):
    offs = np.array(fixed8["starts"]) - fixed8["starts"][0]
    at = int(offs[380 * 32])                                     # the large family after 380 families
    records = fixed8["records"][:at] + fixed8["big"] + fixed8["records"][at:]
    path = rewrite(str(fixed8["dir"] / "big_mid.bam"), fixed8["header"], records)
    cut = first_boundary(path) - len(fixed8["header"])
    assert at + 4096 < cut < at + len(fixed8["big"]) - 4096        # well inside the large family
    P = ConsensusParams()
    ref = python_ingest(path, P, 8)
    native = run_native(path, P, 8, 8192)
    assert [s for _, _, tab in native[1] for _, s, _ in tab].count(15) == 1     # all four subfamilies sampled
    assert_same(native, ref)


@pytest.mark.parametrize("reads", [200, 256, 5000])
def test_batch_full_at_a_run(fixed8, lowmapq, reads):
    """Every batch but the last ends because the next family's reads would
    not have fitted, and the batches together are the restatement's."""
    p5, frac, cache = lowmapq
    for path, ref, seed in ((fixed8["src"], fixed8["ref"], 5), (p5, cached_ref(cache, p5, ConsensusParams(), 3), 3)):
        if path == fixed8["src"] and frac != 0.02:
            continue                                              # once is enough
        native = run_native(path, ConsensusParams(), seed, reads)
        assert_same(native, ref)
        sizes = [n for n, _ in families(path)] if path == p5 else [32] * 640
        t = 0
        for n_tab, n_reads, _ in native[1][:-1]:
            t += n_tab
            assert n_tab > 0 and n_reads <= reads < n_reads + sizes[t], (t, n_reads, sizes[t])
        assert t + native[1][-1][0] == len(sizes)
        whole = run_native(path, ConsensusParams(), seed, 1 << 16)
        assert [x for e in native[1] for x in e[2]] == [x for e in whole[1] for x in e[2]]
