"""The consensus QC tables on the GPU (dcr_set_metrics: k_metrics between the
failure scan and the filter) against the host path (dcr_fmt_metrics over the
kernel outputs of dcr_submit) on the same batches, word for word over all
10,716 counters; and ``--metrics_output`` through the GPU CLI against the model
(tests/metrics_model.py) over the reference's records."""
import json

import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, native_io, params, synth
from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from duplexumiconsensusreads_amd.params import ConsensusParams
from duplexumiconsensusreads_amd.records import AlignedSegment
from tests import metrics_model as mm
from tests.test_consensus_filter import WANT_DS, WANT_SS
from tests.test_gpu_consensus_filter import SYNTH_FILTER, batches
from tests.test_ss_output import DEFAULT, failing_input, run, write_bam

pytestmark = pytest.mark.gpu


def run_batches(path, prm, reads, ss_output=False, flt=None, metrics=True, n_slots=2):
    """Every batch of ``path`` through the device writer, and through
    dcr_submit + the host counters: per batch (device words or None, host
    words, fam_fail, duplex record bytes, single-strand record bytes or None)."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(prm, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter, dev.metrics = ss_output, flt, metrics
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = ss_output
    out = []
    for hb in batches(path, prm, reads, ss_output):
        F = hb.n_fam
        res = dev.result(dev.submit(hb))
        got = res.metrics.copy() if metrics else None       # the slot's block: copied before the slot is reused
        assert (res.metrics is None) == (not metrics)
        rec = res.record_bytes_of(F).tobytes()
        ss_rec = res.ss_record_bytes_of(F).tobytes() if ss_output else None
        fam_fail = res.fam_fail.copy()
        ss, ds, _ = host.result(host.submit(hb))
        out.append((got, native_io.metrics(hb, ss, ds, F, fam_fail), fam_fail, rec, ss_rec))
    dev.close()
    host.close()
    ctx.close()
    return out


def assert_words(got, want):
    assert got.dtype == np.uint64 and got.shape == (params.MET_WORDS,)
    if not np.array_equal(got, want):
        g, w = params.metrics_fields(got), params.metrics_fields(want)
        bad = {k: [(tuple(int(x) for x in i), int(g[k][tuple(i)]), int(w[k][tuple(i)]))
                   for i in np.argwhere(g[k] != w[k])[:5]] for k in g if not np.array_equal(g[k], w[k])}
        raise AssertionError(f"device counters differ from the host's (index, device, host): {bad}")


@pytest.fixture(scope="module")
def synth_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_met") / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 400, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                   softclip_frac=0.3))
    return path


_RUNS = {}


def synth_run(path, ss_output, filtered, metrics):
    """Each configuration of the 400 synthetic families runs once per module."""
    key = (ss_output, filtered, metrics)
    if key not in _RUNS:
        _RUNS[key] = run_batches(path, ConsensusParams(), 2000, ss_output, SYNTH_FILTER if filtered else None, metrics)
    return _RUNS[key]


@pytest.mark.parametrize("ss_output", [False, True])
@pytest.mark.parametrize("filtered", [False, True])
def test_device_equals_host(synth_bam, ss_output, filtered):
    seen = synth_run(synth_bam, ss_output, filtered, True)
    assert len(seen) > 2                                     # several batches on two slots: reused and zeroed
    for got, want, fam_fail, _, _ in seen:
        assert not fam_fail.any()
        assert_words(got, want)
    total = sum(s[0] for s in seen)
    f = params.metrics_fields(total)
    assert 390 <= int(f["n"][0]) <= 400 and int(f["n"][3]) > 0
    for name in ("ss_reads", "ds_depth", "err_c", "err_s", "ss_qual", "ds_qual", "col"):
        assert np.count_nonzero(f[name]) >= 2, name
    # the filter masks and drops after the count: the same counters with and without it
    plain = synth_run(synth_bam, ss_output, False, True)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(seen, plain)) and len(seen) == len(plain)
    # and counting changes no record
    off = synth_run(synth_bam, ss_output, filtered, False)
    assert [(s[3], s[4]) for s in seen] == [(s[3], s[4]) for s in off]
    if filtered:
        assert sum(len(s[3]) for s in seen) < sum(len(s[3]) for s in plain)     # the filter did drop families


# ---- edge shapes: read lengths around the wave's strides (64 lanes of 16
# quality bytes / 8 columns) and the 512-column clamp; sub-family sizes at the
# clamps of ds_depth (63) and ss_reads (255, with the deep-record kernels)
EDGE_LEN = [1, 63, 64, 65, 150, 511, 512, 513, 600]
EDGE_FAMILIES = [(L, (2, 2, 2, 2)) for L in EDGE_LEN] + [(20, (62, 63, 64, 65)), (20, (254, 255, 256, 300))]


def edge_bam(path):
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    hdr = BamHeader("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])
    with AlignmentFile(path, "wb", header=hdr) as out:
        for f, (L, sizes) in enumerate(EDGE_FAMILIES):
            ins = L + 40
            tmpl = acgt[rng.integers(0, 4, ins + 8)]
            P = 10_000 + 2_000 * f
            spec = [(99, "A", 0), (163, "B", 0), (83, "B", ins - L), (147, "A", ins - L)]    # A1 B2 B1 A2
            for k, (flag, strand, start) in enumerate(spec):
                for j in range(sizes[k]):
                    r = AlignedSegment()
                    r.query_name = f"e{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = P + start
                    r.mapping_quality = 20 + (7 * j + k) % 41
                    r.cigartuples = [(0, L)]
                    seq = tmpl[start:start + L].copy()
                    if j % 8 == 1 and L > 4:          # some reads dissent: columns with errors and lower quality
                        seq[(k + 2) % 5::5] = acgt[(np.searchsorted(acgt, seq[(k + 2) % 5::5]) + 1) % 4]
                    r.query_sequence = seq.tobytes().decode()
                    r.query_qualities = [20 + (3 * i + 5 * j + k) % 20 if i % 7 else 37 for i in range(L)]
                    r.set_tags([("MI", f"{f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)
    return path


def test_edge_shapes(tmp_path):
    path = edge_bam(str(tmp_path / "edge.bam"))
    prm = ConsensusParams(max_reads=300)
    # the oracle on the CPU: these inputs give the intended lengths, columns and depths
    from oracle import dcr_oracle_c
    hb = next(iter(batches(path, prm, 1 << 12, True)))
    assert hb.n_fam == len(EDGE_FAMILIES)
    ss, ds, _ = dcr_oracle_c.run(hb.packed(), prm)
    assert not ss.status.any() and not ds.status.any()
    assert ds.n_de.tolist() == [L for L, _ in EDGE_FAMILIES for _ in range(2)]
    assert ss.n_de.tolist() == [L for L, _ in EDGE_FAMILIES for _ in range(4)]
    assert (ss.len < ss.n_de).any()                         # trimmed records: fewer bases than columns
    assert ss.D.tolist() == [n for _, sizes in EDGE_FAMILIES for n in sizes]
    for ss_output in (False, True):
        ((got, want, fam_fail, _, _),) = run_batches(path, prm, 1 << 12, ss_output)
        assert not fam_fail.any()
        assert_words(got, want)
    f = params.metrics_fields(got)
    assert int(f["n"][0]) == len(EDGE_FAMILIES)
    assert f["ds_depth"][63, 62] == 1 and f["ds_depth"][63, 63] == 3 and f["ds_depth"][2, 2] == 2 * len(EDGE_LEN)
    assert [int(f["ss_reads"][k, 255]) for k in range(4)] == [0, 1, 1, 1] and f["ss_reads"][0, 254] == 1
    # columns past 511 fall into the last bin: the records of 513 and 600 columns
    assert f["col"][0, 0, 511] == 4 * (1 + 2 + 89) and f["col"][1, 0, 511] == 2 * (1 + 2 + 89)
    assert f["col"][0, 0, 510] == 4 * 4 and f["col"][0, 0, 0] == 4 * len(EDGE_FAMILIES)


def test_one_hot_bin(tmp_path):
    """3,000 families of eight reads per sub-family in one batch: almost every
    quality and depth in one bin (the contention and no-wrap case)."""
    path = str(tmp_path / "hot.bam")
    synth.write_packed_bam(path, synth.packed_fixed_size(3000, sub_size=8, read_len=150, seed=2))
    ((got, want, fam_fail, _, _),) = run_batches(path, ConsensusParams(), 1 << 17)
    assert len(fam_fail) == 3000 and not fam_fail.any()
    assert_words(got, want)
    f = params.metrics_fields(got)
    assert [int(f["ss_reads"][k, 8]) for k in range(4)] == [3000] * 4 and f["ds_depth"][8, 8] == 6000
    assert f["ss_qual"].max() > int(f["n"][1]) // 2 and f["col"][0, 1].max() > 65535


def test_failing_family_in_mid_batch(tmp_path):
    path = str(tmp_path / "in.bam")
    first = failing_input(path)
    ((got, want, fam_fail, _, _),) = run_batches(path, ConsensusParams(), 1 << 16, True)
    assert len(fam_fail) == len(first) + 1 and np.flatnonzero(fam_fail).tolist() == [len(first)]
    assert_words(got, want)
    assert int(got[0]) == len(first)
    assert got.tolist() == mm.flat(mm.tables([r for c in first for r in c["expect"]["ds"]],
                                             [r for c in first for r in c["expect"]["ss"]]))


def test_on_off_on_for_one_slot(synth_bam):
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    prm = ConsensusParams()
    ctx = _lib.Context(prm, device=0)
    dev = DeviceStream(ctx, n_slots=1, device_writer=True)
    hb = next(iter(batches(synth_bam, prm, 2000, False)))
    dev.metrics = True
    res = dev.result(dev.submit(hb))
    first, blocks = res.metrics.copy(), res.bgzf.tobytes()
    assert int(first[0]) == hb.n_fam
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    dev.wouts[0].metrics[:] = sentinel
    dev.metrics = False
    res = dev.result(dev.submit(hb))
    assert res.metrics is None and res.bgzf.tobytes() == blocks
    assert (dev.wouts[0].metrics == sentinel).all()          # while off the destination is not written
    dev.metrics = True
    res = dev.result(dev.submit(hb))
    assert np.array_equal(res.metrics, first) and res.bgzf.tobytes() == blocks
    dev.close()
    ctx.close()


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_met_golden") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


def test_gpu_cli_golden_families(tmp_path, golden_bam):
    be = cli.default_backend(ConsensusParams())
    want = mm.document(mm.tables(WANT_DS, WANT_SS))
    seen = []
    for batch_reads in ("1048576", "300"):
        out, met = str(tmp_path / f"cons{batch_reads}.bam"), str(tmp_path / f"met{batch_reads}.json")
        stdout, exc = run(["-i", golden_bam, "-o", out, "--metrics_output", met, "--batch_reads", batch_reads],
                          backend=be)
        assert exc is None
        seen.append((open(met, "rb").read(), stdout))
        assert json.loads(seen[-1][0]) == want
    assert seen[0][0] == seen[1][0] == mm.file_bytes(want)
    # the same backend, kept by the process, without the option: the setting does not stay on its context
    before = sorted(p.name for p in tmp_path.iterdir())
    stdout0, exc0 = run(["-i", golden_bam, "-o", str(tmp_path / "cons300.bam"), "--batch_reads", "300"], backend=be)
    assert exc0 is None and stdout0 == seen[1][1]
    assert sorted(p.name for p in tmp_path.iterdir()) == before and be.metrics is False and be.ctx.metrics is False
