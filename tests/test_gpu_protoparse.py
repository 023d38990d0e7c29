"""tfgpu_proto_parser_parse against the row-wise restatement (tests/protoparse_ref.py), cell for cell after download: values, nil bits, src_row,
part_id, the `unparsed` list and event_base.  Shapes are the smallest at which a path changes: message counts around a wave, events per message that
cross a wave in the scan, events around the 8-byte read window."""
import os
import struct

import numpy as np
import pytest

import protoparse_ref as R
from transferia_amd import abi, lib

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protoparser", "gotest")
KIND_CODE = {"unmarshal": abi.ROW_PROTO_UNMARSHAL, "required": abi.ROW_PROTO_REQUIRED, "corrupted": abi.ROW_PROTO_FRAME_CORRUPTED,
             "incomplete": abi.ROW_PROTO_FRAME_INCOMPLETE, "short": abi.ROW_PROTO_FRAME_SHORT, "wrapper": abi.ROW_PROTO_WRAPPER, "host": abi.ROW_HOST_FALLBACK}
FDS = R.device_cases_fds()
FDS_PLAIN = R.device_cases_fds(foreign=False)  # without `deep`: every field may be a column
BIG = (R.PROTOSEQ_MAX_RECORD + 1).to_bytes(4, "little")
EV = R.parse_fds(FDS).by_full[".t.Ev"]
COLS = [(c, False) for c in R.DEVICE_COLUMNS]
FRAMINGS = ["PackageTypeSingleMsg", "PackageTypeProtoseq", "PackageTypeRepeated"]


def norm(cell):
    g, v = cell
    if g == "float32":
        return (g, np.float32(v).tobytes())
    if g == "float64":
        return (g, struct.pack("<d", v))
    if g in ("string", "bytes", "json"):
        return (g, bytes(v))
    return (g, v)


def frame(pkg, events):
    """one queue message holding `events` (their wire bytes) in the framing"""
    if pkg == "PackageTypeProtoseq":
        return b"".join(R.protoseq_frame(e) for e in events)
    if pkg == "PackageTypeRepeated":
        return b"".join(R.enc_bytes(1, e) for e in events)
    assert len(events) == 1
    return events[0]


def check(desc_file, message, values, pkg="PackageTypeSingleMsg", offsets=None, write_times=None, create_times=None, topic="a/b@c", partition=3, host_events=(),
          **cfg):
    """device against restatement over one batch; returns (rows, unparsed) of the restatement.  host_events: (msg, idx) of events the reference decodes
    and the device hands to the host (a field outside its subset that is no column)"""
    ref = R.Parser(desc_file, message, pkg, **cfg)
    par = lib.ProtoParser.create(desc_file, message, pkg, **cfg)
    assert [(c.name, c.dtype, c.key, c.required) for c in par.schema().cols] == ref.schema
    n = len(values)
    offsets = list(offsets) if offsets is not None else [100 + i for i in range(n)]
    write_times = list(write_times) if write_times is not None else [1_700_000_000_123_456_789 + i for i in range(n)]
    batch = abi.message_batch(topic, partition, [(offsets[i], write_times[i], None, values[i], None) for i in range(n)])
    dev, un, base = par.parse(batch, create_time_ns=create_times)
    got = dev.download()
    rows, want_un, want_base = ref.do_batch(values)
    if host_events:
        want_un = sorted(want_un + [(e, m, idx, "host", None) + next((s, n) for s, n, i, _ in ref.events(values[m]) if i == idx) for e, m, idx, _ in rows if (m, idx) in host_events])
        rows = [r for r in rows if (r[1], r[2]) not in host_events]
    assert list(base) == want_base
    starts = np.concatenate([[0], np.cumsum([len(v) for v in values])]) if n else np.zeros(1, np.int64)
    assert [(int(u["event"]), int(u["msg"]), int(u["idx"]), int(u["code"]), int(u["start"]), int(u["len"])) for u in un] == \
        [(e, m, idx, KIND_CODE[kind], int(starts[m]) + s, ln) for e, m, idx, kind, col, s, ln in want_un]
    names = [s[0] for s in ref.schema]
    assert [int(u["column"]) for u in un] == [names.index(col) if kind == "required" else -1 for e, m, idx, kind, col, s, ln in want_un]
    assert got.nrows == len(rows) and dev.table_id() == ("", "a_b_c") and [c.name for c in got.cols] == names
    assert list(got.src_row) == [r[0] for r in rows] and list(got.part_id) == [r[1] for r in rows]
    nfield = len(ref.included) + len(ref.extra)
    for j in range(nfield):
        want = [norm(r[3][j]) for r in rows]
        have = [norm(got.cols[j].pyvalue(i)) for i in range(got.nrows)]
        assert have == want, (names[j], [(i, h, w) for i, (h, w) in enumerate(zip(have, want)) if h != w][:3])
    for j in range(nfield, len(names)):
        c = got.cols[j]
        for i, (e, m, idx, _) in enumerate(rows):
            want = {"_partition": ["string", ('{"partition":%d,"topic":"%s"}' % (partition, topic)).encode()], "_offset": ["uint64", offsets[m]], "_idx": ["uint64", idx],
                    "_lb_ctime": ["time", divmod(create_times[m] if create_times is not None else 0, 10**9)],
                    "_lb_wtime": ["time", divmod(write_times[m], 10**9)]}[names[j]]
            assert norm(c.pyvalue(i)) == norm(want), (names[j], i)
    par.free()
    return rows, want_un


def small_event(i):
    return R.encode(EV, [("i32", i - 3), ("s", "é%d" % i), ("ri", list(range(i % 4))), ("m", [("s", "x" * (i % 3)), ("i", i)]), ("mi", {"k%d" % (i % 2): i})])


@pytest.mark.parametrize("nmsg", [0, 1, 63, 64, 65, 257])
def test_message_counts_single(nmsg):
    values = [small_event(i) if i % 7 != 5 else b"" for i in range(nmsg)]  # (an empty message yields no event)
    rows, un = check(FDS, "Ev", values, include_columns=COLS)
    assert len(rows) == sum(1 for v in values if v) and not un


@pytest.mark.parametrize("pkg", FRAMINGS[1:])
@pytest.mark.parametrize("nmsg", [0, 1, 65])
def test_events_per_message(pkg, nmsg):
    """0, 1, 2 and 130 events a message: the counts cross a wave in the scan"""
    per = [0, 1, 2, 130]
    values = [frame(pkg, [small_event(m * 131 + k) for k in range(per[m % 4])]) for m in range(nmsg)]
    rows, un = check(FDS_PLAIN, "EvList" if pkg == "PackageTypeRepeated" else "Ev", values, pkg, include_columns=COLS, add_synthetic_keys=True, add_system_columns=True,
                     create_times=[5 * m - 7 for m in range(nmsg)])
    assert len(rows) == sum(per[m % 4] for m in range(nmsg)) and not un


@pytest.mark.parametrize("pkg", FRAMINGS)
def test_event_sizes(pkg):
    """an event of 0 bytes (every field at its zero value), events of 7 / 8 / 9 bytes (the 8-byte read window) and one of about 2 KiB"""
    evs = [b"", R.encode(EV, [("s", "abcde")]), R.encode(EV, [("s", "abcdef")]), R.encode(EV, [("s", "abcdefg")]),
           R.encode(EV, [("s", "й" * 400), ("rb", [bytes(range(256))] * 4), ("rs", ["z" * 100] * 2), ("by", b"\xff" * 33)])]
    assert [len(e) for e in evs[:4]] == [0, 7, 8, 9] and 2000 < len(evs[4]) < 2300
    if pkg == "PackageTypeSingleMsg":
        values = [e for e in evs]
    else:
        values = [frame(pkg, evs), frame(pkg, evs[:1]), frame(pkg, evs[1:3])]
    rows, un = check(FDS, "EvList" if pkg == "PackageTypeRepeated" else "Ev", values, pkg, include_columns=COLS)
    assert not un and len(rows) == (4 if pkg == "PackageTypeSingleMsg" else 8)


@pytest.fixture(scope="module")
def metrika():
    with open(os.path.join(GOLD, "metrika-data", "metrika_hit_log.desc"), "rb") as f:
        desc = f.read()
    with open(os.path.join(GOLD, "metrika-data", "metrika_hit_log_data.bin"), "rb") as f:
        data = f.read()
    return desc, data


def test_metrika_fixture_three_framings(metrika):
    """the reference's own fixture whole: 162 events of 92 columns as the repeated wrapper; its elements re-framed as protoseq and as single messages
    give the same columns"""
    desc, data = metrika
    rows, un = check(desc, "CloudTransferHitList", [data], "PackageTypeRepeated")
    assert len(rows) == 162 and len(rows[0][3]) == 92 and not un
    elements = [data[v[0]:v[0] + v[1]] for num, wt, v in R.wire_fields(data) if num == 1]
    rows2, _ = check(desc, "CloudTransferHit", [frame("PackageTypeProtoseq", elements[:100]), frame("PackageTypeProtoseq", elements[100:])], "PackageTypeProtoseq")
    rows3, _ = check(desc, "CloudTransferHit", elements, "PackageTypeSingleMsg")
    assert [r[3] for r in rows2] == [r[3] for r in rows] == [r[3] for r in rows3]


def test_protoseq_framing():
    e = [small_event(i) for i in range(6)]
    F, M = R.protoseq_frame, R.PROTOSEQ_MAGIC
    flipped = F(e[1])[:-1] + b"\x00"
    values = [
        F(e[0]) + BIG + b"junk" + M + F(e[1]),  # a size of 64 MiB + 1: resynchronised
        F(e[0]) + flipped + F(e[2]),                      # a flipped sync byte with a later magic: e[1] + broken magic + e[2]'s frame up to its magic are ONE corrupted event
        F(e[0]) + flipped,                                # ... and without one: the rest is dropped silently
        F(e[0]) + b"\x01", F(e[0]) + b"\x01\x02", F(e[0]) + b"\x01\x02\x03",   # 1-3 trailing bytes
        F(e[0]) + F(e[3])[:10],                           # a frame cut inside the payload
        F(e[0]) + F(e[3])[:-5],                           # ... and inside the magic
        F(M + e[4] + M) + F(e[5]),                        # magic bytes inside a payload: the size field decides where the frame ends, the payload is not searched
        BIG,                                     # nothing but an oversized size: no magic, dropped
        b"",
    ]
    rows, un = check(FDS, "Ev", values, "PackageTypeProtoseq", include_columns=COLS, add_synthetic_keys=True)
    kinds = [(u[1], u[3]) for u in un]
    assert (0, "corrupted") in kinds and (1, "corrupted") in kinds and (3, "short") in kinds and (6, "incomplete") in kinds and (7, "incomplete") in kinds
    assert not any(m == 2 for m, _ in kinds) and sum(1 for r in rows if r[1] == 2) == 1 and not any(r[1] in (9, 10) for r in rows)


def test_repeated_wrapper():
    e = [small_event(i) for i in range(4)]
    el = lambda b: R.enc_bytes(1, b)  # noqa: E731
    values = [
        el(e[0]) + el(e[1])[:-3],                                   # cut mid-element: one item, the whole value, counter 1
        el(e[0]) + R.enc_varint(7, 5) + R.enc_bytes(9, b"zz") + el(e[1]) + R.enc_fixed32(3, b"abcd"),   # unknown fields beside the elements
        el(e[2]) + el(R.enc_bytes(14, b"\xff\xfe")) + el(e[3]),     # an element with invalid UTF-8 fails the WRAPPER
        el(e[2]),
        R.enc_varint(1, 5) + el(e[0]),                              # the wrapper's field as a varint: the host decides
        el(e[0]) + el(R.tag(3, 3)),                                 # a group inside an element: the host takes the message whole
        b"",
    ]
    rows, un = check(FDS, "EvList", values, "PackageTypeRepeated", include_columns=COLS, add_synthetic_keys=True)
    assert [(u[1], u[2], u[3]) for u in un] == [(0, 1, "wrapper"), (2, 1, "wrapper"), (4, 0, "host"), (5, 0, "host")]
    assert [r[1] for r in rows] == [1, 1, 3]


def test_typing_extremes():
    """every scalar kind at its extremes, zigzag, enum as int32, float32 inside an `any`, base64 of 0 / 1 / 2 / 3 bytes, packed and unpacked runs"""
    i32, i64, u32, u64 = [-2**31, 2**31 - 1, -1], [-2**63, 2**63 - 1, -1], [0, 2**32 - 1], [0, 2**64 - 1]
    evs = []
    for k in range(3):
        evs.append(R.encode(EV, [("d", [1.7976931348623157e308, 5e-324, -1.5][k]), ("f", [3.4028234663852886e38, 1e-45, 0.1][k]), ("i32", i32[k]), ("i64", i64[k]),
                                 ("u32", u32[k % 2]), ("u64", u64[k % 2]), ("s32", i32[k]), ("s64", i64[k]), ("fx32", u32[k % 2]), ("fx64", u64[k % 2]),
                                 ("sf32", i32[k]), ("sf64", i64[k]), ("b", k != 1), ("s", 'q"\\<\n\u2028' * k), ("by", b"\x00\xff" * k), ("en", i32[k]),
                                 ("ri", i32), ("rz", i64), ("rx", u64), ("re", [0, 1, -1]), ("rf", [0.1, 2.2, 1e21, 1e-7, 16777216.0, -0.0]),
                                 ("rd", [0.1, 1e21, 1e-7, 123456789.125]), ("rb", [b"", b"a", b"ab", b"abc"]), ("rs", ["", "é", "<>&"]),
                                 ("m", [("f", 0.3), ("b", b"a" * k), ("e", -1 - k), ("s", "s\t")]), ("mf", {"b": 0.7, "a": 1e-7}), ("mb", {"k": b"ab"})], packed=k != 1))
    # int32 fields carrying more than 32 bits on the wire are truncated as Go's int32(v) does; duplicate map keys: the last one wins
    evs.append(R.enc_varint(3, (1 << 40) + 5) + R.enc_varint(5, (1 << 33) + 7) + R.enc_varint(13, 2)
               + R.encode(EV, [("mi", {"a": 1})]) + R.encode(EV, [("mi", {"b": 2})]) + R.encode(EV, [("mi", {"a": 3})]) + R.encode(EV, [("i32", 1), ("i32", 2)]))
    rows, un = check(FDS, "Ev", evs, include_columns=COLS)
    assert len(rows) == 4 and not un
    c = R.DEVICE_COLUMNS.index
    assert rows[3][3][c("mi")] == ["json", b'{"a":3,"b":2}'] and rows[3][3][c("i32")] == ["int32", 2] and rows[0][3][c("en")] == ["int32", -2**31]
    assert rows[0][3][c("rb")] == ["json", b'["","YQ==","YWI=","YWJj"]'] and rows[0][3][c("rf")] == ["json", b"[0.1,2.2,1e+21,1e-7,16777216,-0]"]


@pytest.mark.parametrize("pkg", ["PackageTypeSingleMsg", "PackageTypeRepeated"])
def test_not_fill_empty_fields(pkg):
    """the flag in each of its places: a top-level field that is not set; inside a message only the set members; a message none of whose members is set
    and a message type without fields; nil elements of a repeated message field keep their slot as null; `_lb_extra_` columns skip the top-level rule"""
    evs = [
        R.encode(EV, [("i32", 0), ("s", ""), ("oi", 0), ("os", ""), ("ua", 0), ("m", [("i", 0), ("s", "x"), ("oi", 0)]), ("rm", [[("i", 1)], [], [("s", "")]]),
                      ("em", []), ("rem", [[], []]), ("ri", []), ("mi", {"z": 0})]),
        R.encode(EV, [("m", [("i", 0), ("f", 0.0)]), ("ub", ""), ("b", True), ("mf", {}), ("rs", [""]), ("d", 2.5)]),
        b"",
    ]
    values = evs if pkg == "PackageTypeSingleMsg" else [frame(pkg, evs)]
    msgname = "EvList" if pkg == "PackageTypeRepeated" else "Ev"
    for nfe in (True, False):
        rows, un = check(FDS, msgname, values, pkg, include_columns=COLS, not_fill_empty_fields=nfe)
        assert not un
        # the same fields as `_lb_extra_` columns: makeValues' second loop has no top-level Has() check, the inner rules stay
        rows2, un2 = check(FDS_PLAIN, msgname, values, pkg, include_columns=[("d", False)], add_system_columns=True, not_fill_empty_fields=nfe)
        assert not un2
    c = R.DEVICE_COLUMNS.index
    rows, _ = check(FDS, msgname, values, pkg, include_columns=COLS, not_fill_empty_fields=True)
    r0 = rows[0][3]
    assert r0[c("i32")] == ["nil", None] and r0[c("oi")] == ["int32", 0] and r0[c("os")] == ["string", b""] and r0[c("ua")] == ["int32", 0]
    assert r0[c("m")] == ["json", b'{"oi":0,"s":"x"}'] and r0[c("rm")] == ["json", b'[{"i":1},null,null]'] and r0[c("em")] == ["nil", None]
    assert r0[c("rem")] == ["json", b"[null,null]"] and r0[c("mi")] == ["json", b'{"z":0}'] and r0[c("ri")] == ["nil", None]
    assert rows[1][3][c("m")] == ["nil", None] and rows[1][3][c("ub")] == ["string", b""] and rows[1][3][c("ua")] == ["nil", None]


def test_required_columns():
    """Required on a present and an absent optional field, a oneof member and a message; a plain proto3 scalar has no presence and never fails"""
    evs = [R.encode(EV, [("oi", 0), ("m", []), ("ub", "")]), R.encode(EV, [("oi", 1), ("ub", "x")]), R.encode(EV, [("m", [("i", 1)]), ("ub", "y")]),
           R.encode(EV, [("oi", 1), ("m", [])])]
    rows, un = check(FDS, "Ev", evs, include_columns=[("i32", True), ("oi", True), ("m", True), ("ub", True), ("s", False)], primary_keys=["i32"])
    assert [(u[1], u[3], u[4]) for u in un] == [(1, "required", "m"), (2, "required", "oi"), (3, "required", "ub")] and len(rows) == 1
    rows, un = check(FDS, "EvList", [frame("PackageTypeRepeated", evs)], "PackageTypeRepeated", include_columns=[("oi", True)])
    assert [(u[2], u[3]) for u in un] == [(3, "required")] and len(rows) == 3


def test_field_outside_the_subset_that_is_no_column():
    """`deep` (nesting of two levels) is left out of IncludeColumns: only the event that carries it goes to the host"""
    evs = [small_event(1), small_event(2) + R.enc_bytes(40, R.enc_bytes(1, R.enc_varint(2, 5))), small_event(3)]
    rows, un = check(FDS, "Ev", evs, include_columns=COLS, host_events={(1, 1)})
    assert [(u[1], u[3]) for u in un] == [(1, "host")] and [r[1] for r in rows] == [0, 2]
    par = lib.ProtoParser.create(FDS, "Ev", include_columns=COLS + [("deep", False)])
    code, why, name, ncol = par.info()
    assert code == abi.ROW_HOST_FALLBACK and "deep" in why and "nesting deeper than one level" in why and name == "t.Ev"
    batch = abi.message_batch("t", 0, [(0, 0, None, e, None) for e in evs])
    dev, un, base = par.parse(batch)
    assert dev.nrows == 0 and [int(u["code"]) for u in un] == [abi.ROW_HOST_FALLBACK] * 3 and list(base) == [0, 1, 2, 3]


def test_what_does_not_unmarshal_and_what_the_host_decides():
    ok = small_event(1)
    evs = [
        ok + R.enc_bytes(14, b"ab\xc0"),                  # invalid UTF-8 in a proto3 string fails the unmarshal ...
        ok + R.enc_bytes(15, b"ab\xc0"),                  # ... bytes may hold anything
        ok + R.enc_bytes(28, R.enc_bytes(1, b"\xed\xa0\x80")),        # a member string (a surrogate)
        ok + R.enc_bytes(31, R.enc_bytes(1, b"k") + R.enc_bytes(2, b"\x80")),   # a map value
        ok + R.enc_bytes(22, b"\xf5"),                    # an element of a repeated string
        ok + R.enc_bytes(77, b"\xff") + R.enc_varint(78, 1),          # unknown fields hold anything
        ok + R.tag(3, 0),                                 # a varint cut off
        ok + R.enc_bytes(21, b"\x80"),                    # a packed run cut inside a varint
        ok + R.enc_bytes(27, b"1234567"),                 # a packed fixed64 run of 7 bytes
        ok + R.tag(14, 2) + b"\x05ab",                    # a length beyond the event
        ok + R.tag(50, 3) + R.tag(50, 4),                 # a group: the host decides
        ok + R.enc_varint((1 << 29), 1),                  # a field number above 2^29 - 1
        ok + R.enc_varint(14, 5),                         # a known field with a foreign wire type
        ok + R.enc_fixed32(3, b"abcd"),
        R.encode(EV, [("rd", [1.0, float("nan")])]),      # NaN inside an `any` has no JSON text
        R.encode(EV, [("mf", {"a": float("inf")})]),
        R.encode(EV, [("d", float("nan")), ("f", float("-inf"))]),   # ... as a cell of its own it is a value
    ]
    rows, un = check(FDS, "Ev", evs, include_columns=COLS)
    assert [(u[1], u[3]) for u in un] == [(0, "unmarshal"), (2, "unmarshal"), (3, "unmarshal"), (4, "unmarshal"), (6, "unmarshal"), (7, "unmarshal"),
                                          (8, "unmarshal"), (9, "unmarshal"), (10, "host"), (11, "host"), (12, "host"), (13, "host"), (14, "host"), (15, "host")]
    assert [r[1] for r in rows] == [1, 5, 16]
    # Has() of -0.0 under NotFillEmptyFields is not pinned: the host
    rows, un = check(FDS, "Ev", [R.encode(EV, [("d", -0.0)]), R.encode(EV, [("m", [("f", -0.0)])]), ok], include_columns=COLS, not_fill_empty_fields=True)
    assert [(u[1], u[3]) for u in un] == [(0, "host"), (1, "host")] and len(rows) == 1
