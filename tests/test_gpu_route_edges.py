"""The routing-edge cases (tests/route_cases.py: records on both sides of every
limit that decides a record's kernels) through the three entry points, bit for
bit against the C oracle: dcr_run_batch_host (each case alone, all of them in
two shuffles, the k_recmeta work-split batches; with and without read info),
dcr_run_batch on device pointers, and the slot path (dcr_submit /
dcr_submit_write), whose host-side hint skips k_prep_big and k_decide_deep for
batches without deep records.  No route is asserted: tests/test_route_cases.py
shows on the CPU that the inputs sit where the table says."""
import gzip

import numpy as np
import pytest

from duplexumiconsensusreads_amd import _lib, native_io
from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from duplexumiconsensusreads_amd.batch import BATCH_FIELDS, OUT_COLS, OUT_SCALARS, OutArrays, pack_families
from duplexumiconsensusreads_amd.records import AlignedSegment
from oracle import dcr_oracle_c
from tests import route_cases as rc
from tests.test_gpu_parity import assert_same
from tests.test_gpu_writer import members

pytestmark = pytest.mark.gpu

CASES = rc.cases()
IDS = [c.name for c in CASES]
INFO = ("seq_start", "len", "status", "has_ins")
_ORACLE = {}


def oracle(key, packed, params):
    """The C oracle's result of a batch, computed once per module."""
    if key not in _ORACLE:
        _ORACLE[key] = dcr_oracle_c.run(packed, params, n_threads=8)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(rc.PARAMS, device=0, want_info=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_noinfo():
    c = _lib.Context(rc.PARAMS, device=0, want_info=False)
    yield c
    c.close()


def check_host(c, key, packed, params, info):
    c.set_params(params)
    got = c.run_host(packed, want_info=info)
    want = oracle(key, packed, params)
    assert_same(packed, got, want)
    if info:
        for k in INFO:
            assert np.array_equal(got[2][k], want[2][k]), k


# ---- dcr_run_batch_host
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_alone(ctx, case):
    """a one-family batch (behind its pad family where the case fixes lo & 15):
    the record is the first and the last entry of whichever list it lands in"""
    packed, _ = rc.build_batch([case])
    check_host(ctx, case.name, packed, rc.PARAMS_MIN0 if case.min0 else rc.PARAMS, True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_alone_without_read_info(ctx_noinfo, case):
    packed, _ = rc.build_batch([case])
    check_host(ctx_noinfo, case.name, packed, rc.PARAMS_MIN0 if case.min0 else rc.PARAMS, False)


@pytest.mark.parametrize("info", [True, False], ids=["info", "noinfo"])
@pytest.mark.parametrize("seed", sorted(rc.COMBINED))
def test_all_cases_shuffled(ctx, ctx_noinfo, seed, info):
    packed, _ = rc.build_batch(rc.shuffled(seed))
    check_host(ctx if info else ctx_noinfo, ("shuffle", seed), packed, rc.combined_params(seed), info)


@pytest.mark.parametrize("info", [True, False], ids=["info", "noinfo"])
@pytest.mark.parametrize("name", sorted(rc.RPW_BATCHES))
def test_work_split_batches(ctx, ctx_noinfo, name, info):
    check_host(ctx if info else ctx_noinfo, name, rc.rpw_batch(name), rc.PARAMS, info)


# ---- dcr_run_batch with device pointers
def test_all_cases_device_pointers(ctx):
    from duplexumiconsensusreads_amd.device import DeviceBatch
    packed, _ = rc.build_batch(rc.shuffled(2))          # the shuffle with the empty subfamily
    packed.bases, packed.quals = packed.bases.copy(), packed.quals.copy()      # writable, as the upload wants them
    ctx.set_params(rc.combined_params(2))
    db = DeviceBatch(packed)
    ctx.reserve(db.batch_struct)
    ctx.run_device(db.batch_struct, db.ss_struct, db.ds_struct)
    ctx.sync()
    got = db.download()
    assert_same(packed, (got[0], got[1]), oracle(("shuffle", 2), packed, rc.combined_params(2)))


# ---- the slot path and its hint
def write_bam(path, fams):
    """as tests/test_gpu_ss_output.edge_bam writes its families"""
    hdr = BamHeader("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])
    with AlignmentFile(path, "wb", header=hdr) as out:
        for f, fam in enumerate(fams):
            for k, (flag, strand) in enumerate(((99, "A"), (163, "B"), (83, "B"), (147, "A"))):     # A1 B2 B1 A2
                for j, x in enumerate(fam[k]):
                    r = AlignedSegment()
                    r.query_name = f"c{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = x.reference_start
                    r.mapping_quality = x.mapping_quality
                    r.cigartuples = x.cigartuples
                    r.query_sequence = x.query_sequence
                    r.query_qualities = x.query_qualities
                    r.set_tags([("MI", f"{f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)


def one_batch(path, params):
    """as tests/test_gpu_slot_sizes.one_batch, with the single-strand metadata"""
    ing = native_io.Ingest(path, params.min_map_quality, params.min_reads, params.max_reads, params.min_base_quality,
                           ss_meta=True)
    hb = native_io.HostBatch(reads=50_000, side_bytes=1 << 24, ss_meta=True)
    ing.next(hb)
    assert hb.end_kind == native_io.END_EOF, "the whole file is one batch"
    ing.close()
    return hb


def out_arrays(arr, n_rec, n_cols):
    o = OutArrays(n_rec, n_cols)
    for k in OUT_SCALARS:
        getattr(o, k)[:] = arr[k][:n_rec]
    for k in OUT_COLS:
        getattr(o, k)[:n_cols] = arr[k][:n_cols]
    return o


def test_slot_path_with_and_without_deep_records(tmp_path):
    from duplexumiconsensusreads_amd.stream import DeviceStream
    params = rc.PARAMS
    hbs, want_max = {}, {"r63": 63, "r64": 64}
    for g, sel in rc.slot_groups().items():
        fams, _ = rc.families(sel)
        path = str(tmp_path / f"{g}.bam")
        write_bam(path, fams)
        hbs[g] = hb = one_batch(path, params)
        # the ingest hands on exactly the families the table built (the geometry checked on the CPU)
        packed, want = hb.packed(), pack_families(fams)
        for k in BATCH_FIELDS:
            assert np.array_equal(getattr(packed, k), getattr(want, k)), (g, k)
        deepest = int(np.diff(packed.sub_off).max())
        assert deepest == want_max[g] if g in want_max else deepest >= 65, (g, deepest)
    ctx = _lib.Context(params, device=0)
    dev = DeviceStream(ctx, device_writer=True)
    host = DeviceStream(ctx, device_writer=False)
    host.ss_output = True               # pos, n_cig and cigar of the single-strand records come back too
    failing = 0
    # a batch that launches k_prep_big / k_decide_deep is followed by one that skips them, and the reverse:
    # on the context (65 63 64 63 65 first) and, the slots alternating, on slot 0 (65 64 65 63 65) and on
    # slot 1 (63 63 65 63) each
    order = ("r65", "r63", "r64", "r63", "r65", "r65", "r63", "r63", "r65")
    for step, g in enumerate(order):
        hb = hbs[g]
        F, packed = hb.n_fam, hb.packed()
        # device writer
        res = dev.result(dev.submit(hb))
        blocks = members(res.bgzf.tobytes())            # checks every member
        nz = np.flatnonzero(res.fam_fail)
        f_dev = int(nz[0]) if len(nz) else F
        fetched = res.record_bytes_of(f_dev).tobytes()  # before the slot is submitted again
        record_bytes = res.record_bytes
        # plain path: its arrays against the oracle, field by field and record by record
        slot = host.next_slot
        ss, ds, rs = host.result(host.submit(hb))
        arr = host.outs[slot].arr
        got = (out_arrays(arr["ss"], 4 * F, packed.ss_cols), out_arrays(arr["ds"], 2 * F, packed.ds_cols))
        assert_same(packed, got, oracle(g, packed, params))
        # the device writer's stream is the host writer's over those arrays, up to the first failing family
        f_host = native_io.first_failure(hb, ss, ds, F, rs)[0]
        assert f_dev == f_host, (step, g)
        out = str(tmp_path / f"host_{step}.bam")
        w = native_io.BgzfWriter(out, b"")
        w.write_consensus(hb, ss, ds, f_host)
        w.close()
        want = gzip.decompress(open(out, "rb").read()) if f_host else b""
        assert fetched == want, (step, g)
        assert blocks[:len(want)] == want, (step, g)
        if f_host == F:
            assert blocks == want and record_bytes == len(want), (step, g)
        else:
            failing += 1
            n_fail = sum(c.fails for c in rc.slot_groups()[g])
            assert f_host == F - n_fail and len(nz) == n_fail, (step, g, f_host, nz)
    assert failing == order.count("r65"), "the group of 65 and more reads holds the failing families"
    dev.close()
    host.close()
    ctx.close()
