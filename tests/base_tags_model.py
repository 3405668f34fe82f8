"""The per-base tags (include/dcr.h ``dcr_set_base_tags``, ``--per_base_tags``)
restated in plain Python over the per-base filters' map
(tests/base_filter_model.py ``base_map`` / ``columns``), and ``retag``, which
puts them into a record the host formatter wrote.

    tags = duplex_tags(a, b, r)        # the ten tags of duplex core r, called from cores a and b
    tags = ss_tags(core)               # sd, se of a single-strand core
    rec = retag(record_bytes, tags)    # the same record with those tags in the new encodings

A list value is a ``B:s`` array, a str value a ``Z`` string.
"""
import struct

from tests import base_filter_model as bm

CLAMP = 32767
DUPLEX_TAGS = ("ad", "bd", "cd", "ae", "be", "ce", "ac", "bc", "aq", "bq")
SS_TAGS = ("sd", "se")


def duplex_tags(a, b, r):
    out = {t: [] for t in DUPLEX_TAGS}
    for c, ia, ib, ca, cb in bm.base_map(a, b, r):
        for s, core, i, col in (("a", a, ia, ca), ("b", b, ib, cb)):
            out[s + "d"].append(0 if col is None else min(core["d"][col], CLAMP))
            out[s + "e"].append(0 if col is None else min(core["e"][col], CLAMP))
            out[s + "c"].append("N" if i is None else core["seq"][i])
            out[s + "q"].append("!" if i is None else chr(core["qual"][i] + 33))
        out["cd"].append(min(r["d"][c], CLAMP))
        out["ce"].append(min(r["e"][c], CLAMP))
    for t in ("ac", "bc", "aq", "bq"):
        out[t] = "".join(out[t])
    return out


def ss_tags(core):
    col = bm.columns(core["cons"])[0]
    assert len(col) == len(core["seq"])
    return {"sd": [min(core["d"][c], CLAMP) for c in col], "se": [min(core["e"][c], CLAMP) for c in col]}


def family_tags(res):
    """The tags of the six records of ``base_filter_model.family``'s cores:
    ([duplex 0, duplex 1], [A1, B2, B1, A2])."""
    return ([duplex_tags(res["ss"][2 * j], res["ss"][2 * j + 1], res["ds"][j]) for j in range(2)],
            [ss_tags(c) for c in res["ss"]])


_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}


def _aux_end(buf, off):
    """The end of the aux field whose two-letter tag starts at ``off``."""
    t = chr(buf[off + 2])
    if t in _FIXED:
        return off + 3 + _FIXED[t]
    if t in "ZH":
        return buf.index(b"\x00", off + 3) + 1
    if t == "B":
        n = struct.unpack_from("<i", buf, off + 4)[0]
        return off + 8 + n * _FIXED[chr(buf[off + 3])]
    raise ValueError(f"bad tag type {t}")


def encode(tag, value):
    if isinstance(value, str):
        return tag.encode() + b"Z" + value.encode() + b"\x00"
    return tag.encode() + b"Bs" + struct.pack(f"<i{len(value)}h", len(value), *value)


def retag(rec, tags):
    """``rec``: one formatted BAM record, block_size included.  The aux fields
    named in ``tags`` are replaced where they stand and block_size is fixed;
    every other byte stays."""
    rec = bytes(rec)
    size, l_rn, n_cig, l_seq = (struct.unpack_from("<i", rec, 0)[0], rec[12], struct.unpack_from("<H", rec, 16)[0],
                                struct.unpack_from("<i", rec, 20)[0])
    assert size + 4 == len(rec)
    off = 36 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    out, seen = [rec[4:off]], set()
    while off < len(rec):
        end, name = _aux_end(rec, off), rec[off:off + 2].decode()
        if name in tags:
            out.append(encode(name, tags[name]))
            seen.add(name)
        else:
            out.append(rec[off:end])
        off = end
    assert off == len(rec) and seen == set(tags), (sorted(seen), sorted(tags))
    body = b"".join(out)
    return struct.pack("<i", len(body)) + body


def split_records(stream):
    """The records of an uncompressed record stream, block_size included."""
    out, off = [], 0
    while off < len(stream):
        n = struct.unpack_from("<i", stream, off)[0] + 4
        out.append(bytes(stream[off:off + n]))
        off += n
    assert off == len(stream)
    return out


def retag_stream(stream, tags):
    """``retag`` over a record stream; ``tags``: one dict per record, in order."""
    recs = split_records(stream)
    assert len(recs) == len(tags), (len(recs), len(tags))
    return b"".join(retag(r, t) for r, t in zip(recs, tags))
