"""bench.py --dump-outputs: bench.dump_outputs turns the three BAMs of a CLI
pass into arrays.  A small pass with the C oracle backend on CPU: the arrays
hold the files' record counts and, for the sampled records, the fixed fields
and every byte that ``bam`` decodes from the same files; a second dump of the
same files is identical; a file without records gives its summary alone."""
import contextlib
import io
import os
import random
import struct

import numpy as np
import pytest

from duplexumiconsensusreads_amd import bam, cli
from oracle import dcr_oracle_c

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _records(path):
    with bam.AlignmentFile(path, "rb") as f:
        return [bam.encode_record(r) for r in f]


def test_dump_outputs_holds_the_output_records(tmp_path, monkeypatch):
    import bench
    # 240 consensus records, 57 filtered reads, no filtered family: a sampled, a whole and an empty file
    inp, out = os.path.join(GOLDEN, "e2e_c1_small.bam"), str(tmp_path / "cons3.bam")
    random.seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        cli.main(["-i", inp, "-o", out], backend=dcr_oracle_c.run)
    monkeypatch.setattr(bench, "DUMP_RECORDS", 60)          # fewer than the consensus records: a real sample
    bench.dump_outputs(str(tmp_path / "d1"), out)
    bench.dump_outputs(str(tmp_path / "d2"), out)
    assert sorted(os.listdir(tmp_path / "d1")) == sorted(os.listdir(tmp_path / "d2"))
    assert all(np.load(tmp_path / "d1" / f).size for f in os.listdir(tmp_path / "d1"))
    counts = {}
    for name, path in (("consensus", out), ("filteredreads", out[:-4] + "_filteredreads.bam"),
                       ("filteredfamilies", out[:-4] + "_filteredfamilies.bam")):
        recs = _records(path)
        if not recs:            # no empty array is written
            assert np.load(tmp_path / "d1" / f"{name}_summary.npy").tolist() == [0, 0]
            assert not (tmp_path / "d1" / f"{name}_core.npy").exists()
            assert not (tmp_path / "d1" / f"{name}_bytes.npy").exists()
            counts[name] = 0
            continue
        got = {k: np.load(tmp_path / "d1" / f"{name}_{k}.npy") for k in ("summary", "core", "bytes")}
        for k, v in got.items():
            assert v.dtype == (np.float32 if k == "bytes" else np.float64)
            assert np.array_equal(v, np.load(tmp_path / "d2" / f"{name}_{k}.npy"))
        assert got["summary"].tolist() == [len(recs), sum(len(r) for r in recs)]
        core = got["core"]
        assert core.shape == (min(len(recs), 60), 1 + len(bench.CORE_FIELDS))
        idx = core[:, 0].astype(int)
        assert np.all(np.diff(idx) > 0) and idx[-1] < len(recs)
        want_bytes = []
        for row, i in zip(core, idx):
            assert tuple(row[1:]) == struct.unpack_from("<iiiBBHHHiiii", recs[i], 0)
            want_bytes.append(np.frombuffer(recs[i], np.uint8)[36:])
        assert np.array_equal(got["bytes"], np.concatenate(want_bytes))
        counts[name] = len(recs)
    assert counts["consensus"] > 60 > counts["filteredreads"] > 0 == counts["filteredfamilies"]


@pytest.mark.parametrize("extra", [["--kernel-only"], ["--steps", "0"]])
def test_dump_outputs_needs_a_timed_cli_pass(tmp_path, monkeypatch, extra):
    """Nothing to dump without a timed CLI pass: refused while parsing, before any work."""
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--dump-outputs", str(tmp_path / "d"), *extra])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and not (tmp_path / "d").exists()


def test_bam_records_fails_on_a_truncated_stream(tmp_path):
    import bench
    whole = bam.bgzf_stream(os.path.join(GOLDEN, "e2e_c1_small.bam"))
    n = sum(1 for _ in bench.bam_records(os.path.join(GOLDEN, "e2e_c1_small.bam")))
    assert n == len(_records(os.path.join(GOLDEN, "e2e_c1_small.bam")))
    for cut, what in ((len(whole) - 5, "record"), (6, "header")):
        w = bam.open_bgzf_writer(str(tmp_path / f"{what}.bam"))
        w.write(whole[:cut])
        w.close()
        with pytest.raises(ValueError, match=f"truncated BAM {what}"):
            list(bench.bam_records(str(tmp_path / f"{what}.bam")))
