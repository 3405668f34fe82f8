"""The per-base duplex QC tables on the GPU (dcr_set_base_metrics:
k_base_metrics over the column maps k_consensus_general_map stores) against
the model (tests/base_metrics_model.py over the oracle's alignment): every one
of the 12,068 words, for equality.  Every table is an integer sum, so the sum
over the batches of a run is the one-batch total."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from duplexumiconsensusreads_amd import cli, params, synth
from duplexumiconsensusreads_amd.params import ConsensusFilter, ConsensusParams
from oracle import dcr_oracle as O
from tests import base_filter_model as bm
from tests import base_metrics_model as mm
from tests.base_filter_cases import batch_subfamilies, read, write_families
from tests.test_base_metrics import ALL
from tests.test_gpu_base_filter import EDGE_LEN, edge_bam, out_files, run_cli
from tests.test_gpu_consensus_filter import batches
from tests.test_ss_output import DEFAULT, PROCESSED, failing_input, write_bam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.Params()
ZERO = np.zeros(params.BMET_WORDS, np.uint64)


def device_batches(path, prm, reads, base_metrics=True, ss_output=False, flt=None, metrics=False, base_tags=False,
                   n_slots=2, streams=True):
    """Every batch of ``path`` through the device writer, two batches in flight
    on ``n_slots`` > 1.  Per batch a dict: F, fam_fail, words (base metrics),
    flags (stored maps), fam_filt, metrics, records / ss_records (with
    ``streams``), bgzf, pk."""
    from duplexumiconsensusreads_amd import _lib
    from duplexumiconsensusreads_amd.stream import DeviceStream
    ctx = _lib.Context(prm, device=0)
    dev = DeviceStream(ctx, n_slots=n_slots, device_writer=True)
    dev.ss_output, dev.filter, dev.metrics, dev.base_tags = ss_output, flt, metrics, base_tags
    dev.base_metrics = base_metrics
    maps = base_metrics or base_tags or (flt is not None and flt.base_active)
    out = []

    def take(hb, handle):
        F = hb.n_fam
        res = dev.result(handle)
        d = dict(F=F, fam_fail=res.fam_fail.copy(), pk=hb.packed(), bgzf=res.bgzf.tobytes(),
                 words=res.base_metrics.copy() if base_metrics else None,
                 fam_filt=res.fam_filt.copy() if flt is not None else None,
                 metrics=res.metrics.copy() if metrics else None)
        assert (res.base_metrics is None) == (not base_metrics)
        if streams:
            d["records"] = res.record_bytes_of(F).tobytes()
            d["ss_records"] = res.ss_record_bytes_of(F).tobytes() if ss_output else None
        flags = np.zeros(6 * F, np.uint8)
        rc = dev.lib.dcr_slot_fetch(ctx._ctx, handle[0], 6, 0, 6 * F, flags.ctypes.data)
        assert rc == (0 if maps else 1)                    # dcr_slot_fetch what 6 serves a base-metrics batch too
        d["flags"] = flags
        out.append(d)

    pending = None
    for hb in batches(path, prm, reads, ss_output):
        handle = dev.submit(hb)
        if pending is not None and n_slots == 1:
            raise AssertionError("one slot cannot hold two batches")
        if pending is not None:
            take(*pending)
        if n_slots > 1:
            pending = (hb, handle)
        else:
            take(hb, handle)
    if pending is not None:
        take(*pending)
    dev.close()
    ctx.close()
    return out


def model_words(batch, cache=None, key0=0, prm=P):
    """The model's block of one device batch; failing families (fam_fail != 0) are not counted."""
    fams = []
    for f in range(batch["F"]):
        if cache is not None and key0 + f in cache:
            res = cache[key0 + f]
        else:
            res = bm.family(batch_subfamilies(batch["pk"], f), prm)
            if cache is not None:
                cache[key0 + f] = res
        assert (res is None) <= (batch["fam_fail"][f] != 0)
        fams.append(res if batch["fam_fail"][f] == 0 else None)
    return mm.tables(fams)


def assert_words(got, want):
    bad = np.flatnonzero(got != want)
    assert got.dtype == np.uint64 and len(got) == params.BMET_WORDS == 12068
    assert len(bad) == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:10]]


def check(path, prm, reads, **kw):
    """Device words against the model for every batch; returns the batches."""
    seen = device_batches(path, prm, reads, **kw)
    for b in seen:
        assert_words(b["words"], model_words(b))
    return seen


def test_hand_built_families(tmp_path):
    path = write_families(str(tmp_path / "in.bam"), list(ALL.values()))
    (b,) = check(path, ConsensusParams(), 1 << 12)
    assert b["F"] == len(ALL) and not b["fam_fail"].any()
    assert b["flags"].any() and not b["flags"].all()         # the stored-map and the derived-map paths both run
    s = mm.sparse(b["words"])
    assert s["n"][0] == 2 * len(ALL) and s["n"][5] == 5 and s["n"][6] >= 1
    assert s["pair"][(0, 0, 3)] == 1                         # "differ": a calls A where b calls T


def test_single_runs_at_the_dword_and_wave_boundaries(tmp_path):
    path = edge_bam(str(tmp_path / "edge.bam"))
    (b,) = check(path, ConsensusParams(), 1 << 12)
    assert not b["flags"].any()
    s = mm.sparse(b["words"])
    # duplex 1 has three columns of one strand alone at either end
    assert s["n"][1] == sum(2 * L + 3 for L in EDGE_LEN) and min(s["n"][3], s["n"][4]) >= 2 * len(EDGE_LEN)
    assert s["n"][6] > 0 and max(i for (j, w, i) in s["cyc"]) == max(EDGE_LEN) + 2


def long_families(lengths, seed=3):
    """Per length: duplex 0 of two strands at one position, duplex 1 of strands three columns apart; the
    last family's reads all carry an insertion (stored maps).  Every second read dissents here and there."""
    rng = np.random.default_rng(seed)
    fams = []
    for n, L in enumerate(lengths):
        tmpl = "".join("ACGT"[i] for i in rng.integers(0, 4, L + 8))
        ins = n == len(lengths) - 1
        subs = []
        for k, start in enumerate((0, 0, 2, 5)):
            sub = []
            for j in range(2 + k % 2):
                if ins:
                    cig = [(0, 40 + k), (1, 1), (0, L - 41 - k)]
                    seq = tmpl[start:start + 40 + k] + "T" + tmpl[start + 40 + k:start + L - 1]
                else:
                    cig, seq = [(0, L)], tmpl[start:start + L]
                if j == 1:
                    seq = "".join("ACGT"[("ACGT".index(ch) + 1) % 4] if i % 11 == k and 5 < i < len(seq) - 5 else ch
                                  for i, ch in enumerate(seq))
                sub.append(dict(pos=100 + start, mapq=40, cigar=cig, seq=seq,
                                qual=[25 + (3 * i + 7 * j + k) % 15 for i in range(L)]))
            subs.append(sub)
        fams.append(subs)
    return fams


def test_the_cycle_clamp_and_its_tail(tmp_path):
    lengths = [511, 512, 513, 600, 600]
    path = write_families(str(tmp_path / "long.bam"), long_families(lengths), shift=5000)
    (b,) = check(path, ConsensusParams(), 1 << 14)
    assert not b["fam_fail"].any() and b["flags"].any() and not b["flags"].all()
    m = params.base_metrics_fields(b["words"])
    for j in range(2):
        assert m["cyc"][j, 0, :511].tolist() == [len(lengths)] * 511       # every record has cycles 0 .. 510
        assert m["cyc"][j, 0, 511] > 89 and m["cyc"][j, 4, 511] > m["cyc"][j, 0, 511]      # the bases past them
    assert int(m["cyc"][:, 0].sum()) == int(m["n"][1]) > 2 * sum(lengths) - 10


def test_the_depth_clamp_and_depths_above_255(tmp_path):
    """Subfamilies of 300 and 62 reads (duplex 0) and of 70 and 64 (duplex 1): depth bins clamp at 63, the
    sums of cyc do not clamp at 255."""
    def sub(n, dissent):
        return [read(100, [(0, 12)], last="A" if i % dissent == 0 else None) for i in range(n)]
    path = write_families(str(tmp_path / "deep.bam"), [[sub(300, 7), sub(62, 5), sub(70, 3), sub(64, 9)]])
    (b,) = check(path, ConsensusParams(max_reads=400), 1 << 12)
    assert not b["fam_fail"].any()
    s = mm.sparse(b["words"])
    assert set(s["depth"]) == {(63, 62), (63, 63)} and s["cyc"][(0, 4, 0)] == 362 and s["cyc"][(1, 4, 0)] == 134
    assert sum(v for (j, w, i), v in s["cyc"].items() if w == 5) > 0


_GOLDEN = {}


@pytest.fixture(scope="module")
def golden_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_bmet") / "golden.bam")
    write_bam(path, DEFAULT)
    return path


@pytest.mark.parametrize("batch_reads", [1 << 20, 300])
def test_golden_families(golden_bam, batch_reads):
    seen = device_batches(golden_bam, ConsensusParams(), batch_reads, streams=False)
    assert (len(seen) > 2) == (batch_reads == 300) and sum(b["F"] for b in seen) == 877
    if "want" not in _GOLDEN:                                # the model over the 877 families, once
        cache, key0, total = {}, 0, ZERO.copy()
        for b in seen:
            total += model_words(b, cache, key0)
            key0 += b["F"]
        _GOLDEN["want"] = total
    want = _GOLDEN["want"]
    assert_words(sum((b["words"] for b in seen), ZERO.copy()), want)       # the sum over batches is the one-batch total
    flags = np.concatenate([b["flags"] for b in seen])
    assert flags.any() and not flags.all()
    s = mm.sparse(want)
    assert s["n"][:7] == [1754, 112607, 98528, 7115, 6964, 0, 24177]
    assert sum(v for (j, x, y), v in s["pair"].items() if x != y) == 24177
    assert {c for c, q in s["qual"]} == {0, 1, 2} and len(s["depth"]) == 461 and len(s["err"]) == 416
    assert max(i for (j, w, i) in s["cyc"]) == 152


# ---- with everything else on, and the identities between the tables and the other outputs
@pytest.fixture(scope="module")
def synth_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_bmet_synth") / "in.bam")
    synth.write_config_bam(path, synth.SynthConfig("t", 300, sub_size="poisson5", seed=9, indel_frac=0.3,
                                                   softclip_frac=0.3))
    return path


@pytest.fixture(scope="module")
def synth_plain(synth_bam):
    """The run with nothing else on; its first batch (indels and soft clips in a third of the reads) against
    the model."""
    seen = device_batches(synth_bam, ConsensusParams(), 2000)
    assert len(seen) > 2 and seen[0]["flags"].any() and not seen[0]["flags"].all()
    assert_words(seen[0]["words"], model_words(seen[0]))
    return seen


def test_with_the_filters_the_metrics_the_tags_and_the_single_strand_stream(synth_bam, synth_plain):
    flt = ConsensusFilter(min_base_quality=60, min_base_reads=(8, 4, 2), require_strand_agreement=True,
                          min_reads=(8, 4, 2))
    opts = dict(ss_output=True, flt=flt, metrics=True, base_tags=True)
    full = device_batches(synth_bam, ConsensusParams(), 2000, **opts)
    without = device_batches(synth_bam, ConsensusParams(), 2000, base_metrics=False, **opts)
    assert len(full) == len(without) == len(synth_plain)
    for a, b, p in zip(full, without, synth_plain):
        assert_words(a["words"], p["words"])                 # the consensus as called: no option changes a word
        assert a["records"] == b["records"] and a["ss_records"] == b["ss_records"] and a["bgzf"] == b["bgzf"]
        assert np.array_equal(a["fam_filt"], b["fam_filt"]) and np.array_equal(a["metrics"], b["metrics"])
        assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["flags"], p["flags"])
        assert b["words"] is None
    assert sum(int((a["fam_filt"] >> 8).sum()) for a in full) > 0
    assert any((a["fam_filt"] & 0xff).any() for a in full)


def test_the_tables_give_what_the_per_base_rules_mask(synth_bam, synth_plain):
    total = sum((b["words"] for b in synth_plain), ZERO.copy())
    by_depth = device_batches(synth_bam, ConsensusParams(), 2000, flt=ConsensusFilter(min_base_reads=(8, 4, 2)))
    masked = sum(int((b["fam_filt"] >> 8).sum()) for b in by_depth)
    assert masked == mm.masked_by_min_reads(total, 8, 4, 2) > 0
    by_agreement = device_batches(synth_bam, ConsensusParams(), 2000,
                                  flt=ConsensusFilter(require_strand_agreement=True))
    assert sum(int((b["fam_filt"] >> 8).sum()) for b in by_agreement) == int(total[7]) > 0
    for b in by_depth + by_agreement:
        assert not (b["fam_filt"] & 0xff).any()              # a per-base rule alone drops nothing


def test_identities_with_the_record_level_tables(synth_bam, synth_plain):
    seen = device_batches(synth_bam, ConsensusParams(), 2000, metrics=True, streams=False)
    for b, p in zip(seen, synth_plain):
        assert_words(b["words"], p["words"])
        m, r = params.base_metrics_fields(b["words"]), params.metrics_fields(b["metrics"])
        assert m["n"][0] == 2 * r["n"][0] > 0 and m["n"][1] == r["n"][2] > 0
        assert int(m["cyc"][:, 1].sum()) == int(r["n"][3])
        assert np.array_equal(m["qual"].sum(axis=0), r["ds_qual"])
        assert int(m["cyc"][:, 0].sum()) == int(m["n"][1]) == int(m["depth"].sum()) == int(m["err"].sum())
        assert int(m["pair"].sum()) == int(m["n"][2]) and int(m["n"][2:6].sum()) == int(m["n"][1])
        assert int(m["cyc"][:, 2].sum()) == int(m["n"][6]) == int(m["qual"][1].sum())


# ---- a failing family
def test_a_failing_family_in_mid_batch_is_not_counted(tmp_path):
    path = str(tmp_path / "in.bam")
    failing_input(path)
    (b,) = device_batches(path, ConsensusParams(), 1 << 20, streams=False)
    assert b["fam_fail"][20] != 0 and not b["fam_fail"][:20].any()
    assert_words(b["words"], model_words(b))
    ok = int((b["fam_fail"] == 0).sum())
    assert int(b["words"][0]) == 2 * ok and ok < b["F"]
    # the CLI: the run ends as the reference's does and leaves no table file
    out, js = str(tmp_path / "cons.bam"), str(tmp_path / "b.json")
    be = cli.default_backend(ConsensusParams())
    stdout, exc = run_cli(["-i", path, "-o", out, "--base_metrics_output", js], be)
    assert exc == "IndexError" and not os.path.exists(js)
    plain = run_cli(["-i", path, "-o", str(tmp_path / "plain.bam")], be)
    assert (stdout, exc) == plain and out_files(out) == out_files(str(tmp_path / "plain.bam"))


# ---- the GPU CLI
_CASE_CORES = {}


def test_cli_end_to_end_and_on_off_on_for_one_backend(tmp_path):
    cases = PROCESSED[:120]
    path = str(tmp_path / "in.bam")
    write_bam(path, cases)
    be = cli.default_backend(ConsensusParams())
    runs = {}
    for tag, on in (("never", False), ("on", True), ("off", False), ("on_again", True)):
        out, ss, js = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}_ss.bam"), str(tmp_path / f"{tag}.json")
        extra = ["--base_metrics_output", js] if on else []
        stdout, exc = run_cli(["-i", path, "-o", out, "--single_strand_output", ss, "--batch_reads", "500", *extra], be)
        assert exc is None and os.path.exists(js) == on
        runs[tag] = (stdout, out_files(out, ss), open(js, "rb").read() if on else None)
    # the option changes no output byte and no stdout line; switching it off leaves the default run
    assert runs["off"] == runs["never"] and runs["on_again"] == runs["on"]
    assert runs["on"][:2] == runs["never"][:2]
    for c in cases:
        if c["fam"] not in _CASE_CORES:
            _CASE_CORES[c["fam"]] = bm.family(O.split_family([r for r in c["reads"] if r["mapq"] >= 20]), P)
    want = mm.tables([_CASE_CORES[c["fam"]] for c in cases])
    assert runs["on"][2] == params.base_metrics_json(want).encode()
    doc = json.loads(runs["on"][2])
    assert doc["records"] == 240 and doc["bases"] > 0 and doc["disagree"] > 0 and doc["version"] == 1


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
    got = {}
    for tag, extra in (("one", []), ("many", ["--gpus", "2"])):
        out, js, mj = str(tmp_path / f"{tag}.bam"), str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}_m.json")
        rc, stdout = _run_process([*extra, "-i", path, "-o", out, "--min_reads", "3", "--base_metrics_output", js,
                                   "--metrics_output", mj])
        assert rc == 0
        got[tag] = (stdout, open(js, "rb").read(), open(mj, "rb").read())
    assert got["one"] == got["many"]
    doc, met = json.loads(got["one"][1]), json.loads(got["one"][2])
    assert doc["records"] == 2 * met["families"] > 200 and doc["bases"] == met["ds_bases"]
