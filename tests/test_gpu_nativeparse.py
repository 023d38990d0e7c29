"""The native parser on the device (tf_nativeparse.hip, through tfgpu_native_parse) against the plain-Python restatement (tests/nativeparse_ref.py),
exactly: the group order and each group's identity, every cell, nil bit and kind, OldKeys with presence, the meta arrays, part and keytypes, the item
map and the fallback list with reason, item and column.

The sizes are the smallest at which the kernels can go wrong: the cut's 64-byte step (messages and backslash runs around bytes 62 / 63 / 64), a wave
and a workgroup of items (63 .. 257), the text sinks' 8-byte word (0 / 7 / 8 / 9), every integer type at its limits, the scanner's depth limit."""
import json
import os

import numpy as np
import pytest

import nativeparse_ref as R
from transferia_amd import abi

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debezium_emitter")


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def col(name, typ, key=False, ot="", **more):
    d = {"table_schema": "", "table_name": "", "path": "", "name": name, "type": typ, "key": key, "fake_key": False, "required": False, "expression": "", "original_type": ot}
    d.update(more)
    return d


def ts_text(cols) -> str:
    return json.dumps(cols, separators=(",", ":"))


def ci(kind="insert", names=("id",), values=("1",), cols=(col("id", "int32", True),), table="t", schema="public", part="", oldkeys="{}", id=1, lsn=2, commit=3, pos=0,
       tx="", query="", ts=None, extra="") -> bytes:
    """one ChangeItem as MarshalJSON orders it; names None = `null`; values are JSON texts"""
    cn = "null" if names is None else "[" + ",".join(json.dumps(n) for n in names) + "]"
    s = '{"id":%d,"nextlsn":%d,"commitTime":%d,"txPosition":%d,"kind":%s,"schema":%s,"table":%s,"part":%s,"columnnames":%s' % (
        id, lsn, commit, pos, json.dumps(kind), json.dumps(schema), json.dumps(table), json.dumps(part), cn)
    if values:
        s += ',"columnvalues":[' + ",".join(values) + "]"
    s += ',"table_schema":' + (ts if ts is not None else ts_text(list(cols)))
    s += ',"oldkeys":%s,"tx_id":%s,"query":%s%s}' % (oldkeys, json.dumps(tx), json.dumps(query), extra)
    return s.encode("utf-8")


def arr(*items) -> bytes:
    return b"[" + b",".join(items) + b"]"


def cell(c: abi.Column, r: int):
    g, v = c.pyvalue(r)
    return (g, tuple(v) if g == "time" else v)


def norm(c):
    g, v = c
    return (g, tuple(v) if g == "time" else bytes(v) if isinstance(v, (bytes, bytearray)) else v)


def check(tf, msgs, ctx=""):
    """the device against the restatement over one message batch; returns (restatement's result, device result)"""
    want = R.parse(msgs)
    got = tf.native_parse(abi.message_batch("tp", 0, [(i, 0, None, m, None) for i, m in enumerate(msgs)]))
    ni, ng, nf = got.info()
    assert got.fallback() == want.fallback, (ctx, "fallback")
    msg, grp, row = got.items()
    assert [(int(a), int(b), int(c)) for a, b, c in zip(msg, grp, row)] == want.items, (ctx, "item map")
    assert (ni, ng, nf) == (len(want.items), len(want.groups), len(want.fallback)), ctx
    for g, W in enumerate(want.groups):
        D = got.group(g)
        wb, wschema, wmeta = R.group_batch(W)
        b = D.batch.download()
        assert (b.table_ns, b.table_name, D.part) == (W.ns, W.table, W.part), (ctx, g)
        assert [k.decode() for k in D.key_types] == W.key_types, (ctx, g)
        assert D.schema == wschema, (ctx, g, "TableSchema")
        assert D.table_schema_json == W.table_schema_json, (ctx, g)
        dts = D.batch.table_schema()
        assert (dts.triples() if dts else []) == wschema.triples(), (ctx, g)
        assert b.nrows == len(W.rows), (ctx, g)
        assert [(c.name, c.dtype, c.repr) for c in b.cols] == [(c.name, c.dtype, c.repr) for c in wb.cols], (ctx, g, "columns")
        assert all(c.absent is None for c in b.cols) and getattr(b, "col_order", None) is None, (ctx, g)
        assert list(b.kind) == list(wb.kind), (ctx, g, "kinds")
        for r, (_, values, old, _m) in enumerate(W.rows):
            assert [cell(c, r) for c in b.cols] == [norm(v) for v in values], (ctx, g, "row", r)
        wold = getattr(wb, "old_keys", None) or []
        dold = getattr(b, "old_keys", None) or []
        assert [(c.name, c.dtype, c.repr) for c in dold] == [(c.name, c.dtype, c.repr) for c in wold], (ctx, g, "OldKeys columns")
        if wold:
            assert list(b.old_present) == list(wb.old_present), (ctx, g, "old_keys_present")
            for r, (_, _v, old, _m) in enumerate(W.rows):
                if old is not None:
                    assert [cell(c, r) for c in dold] == [norm(v) for v in old], (ctx, g, "OldKeys row", r)
        m = D.meta_host()
        assert int(D.meta.n) == len(W.rows)
        for k in ("id", "lsn", "commit_time", "counter", "names_form"):
            assert [int(x) for x in m[k]] == wmeta[k], (ctx, g, k)
        assert m["tx_id"] == wmeta["tx_id"] and m["query"] == wmeta["query"], (ctx, g)
    return want, got


def parsed(want, n_groups=None):
    assert not want.fallback, want.fallback
    if n_groups is not None:
        assert len(want.groups) == n_groups
    return want


# ---- 1. round trip through the NATIVE queue format ------------------------------------------------------------------------------------------------------
RT_COLS = [col("i8", "int8"), col("i16", "int16"), col("i32", "int32", True), col("i64", "int64"), col("u8", "uint8"), col("u16", "uint16"), col("u32", "uint32"),
           col("u64", "uint64"), col("d", "double"), col("b", "boolean"), col("s", "utf8"), col("by", "string", ot="pg:bytea"), col("t", "timestamp"),
           col("iv", "interval"), col("a", "any", ot="pg:jsonb")]
RT_ROWS = [
    ["-128", "-32768", "1", "-9223372036854775808", "255", "65535", "4294967295", "18446744073709551615", "1.5", "true", '"hello"', '"AQID"', '"2024-02-29T23:59:59.123456789Z"',
     "-5", '{"a":1,"b":[1,2]}'],
    ["127", "32767", "2", "9223372036854775807", "0", "0", "0", "0", "1E5", "false", '"\\u003ctag\\u003e \\" \\\\ \\u2028"', '""', '"1970-01-01T00:00:00Z"', "0", '"text"'],
    ["null"] * 15,
]


def test_round_trip(tf):
    names = [c["name"] for c in RT_COLS]
    old = '{"keynames":["i32"],"keytypes":["integer"],"keyvalues":[%s]}'
    # Updates and Deletes with OldKeys: rows that carry keyvalues are written with keynames / keytypes, rows without are written `"oldkeys":{}` — another group key
    items = [ci("update", names, RT_ROWS[0], RT_COLS, oldkeys=old % "3", id=7, lsn=100, commit=1700000000000000000, pos=3, tx="tx<1>", query="select 1", part="p0"),
             ci("update", names, RT_ROWS[1], RT_COLS, oldkeys=old % "1", id=8, part="p0"),
             ci("delete", names, RT_ROWS[2], RT_COLS, oldkeys=old % "-7", id=9, part="p0"),
             ci("update", names, RT_ROWS[0], RT_COLS, oldkeys=old % "null", id=10, part="p0"),
             ci("delete", names, RT_ROWS[1], RT_COLS, oldkeys=old % "2", id=11, part="p0")]
    want, got = check(tf, [arr(*items)])
    parsed(want, 1)
    D = got.group(0)
    # the parsed group goes straight back into the serializer, under three batchings; parsing THAT gives the same group again
    for kw in ({}, {"enabled": True, "max_change_items": 3}, {"enabled": True, "max_message_size": 2 * len(items[1])}):
        o = abi.queue_options(abi.QFMT_NATIVE, table_schema_json=D.table_schema_json, old_key_types=D.key_types, group_part_ids=[D.part], group_rows=[D.batch.nrows], **kw)
        msgs = tf.queue_serialize(o, D.batch, D.meta).messages()
        assert sum(len(R.cut(m)) for m in msgs) == 5
        if not kw:
            assert len(msgs) == 5
        w2, g2 = check(tf, msgs, str(kw))
        parsed(w2, 1)
        assert [r[1:] for r in w2.groups[0].rows] == [r[1:] for r in want.groups[0].rows] and w2.groups[0].key == want.groups[0].key
        D2 = g2.group(0)
        o2 = abi.queue_options(abi.QFMT_NATIVE, table_schema_json=D2.table_schema_json, old_key_types=D2.key_types, group_part_ids=[D2.part], group_rows=[D2.batch.nrows], **kw)
        assert tf.queue_serialize(o2, D2.batch, D2.meta).messages() == msgs, kw   # the bytes the device wrote are the bytes it writes from its own parse


# ---- 2. the reference's ChangeItem fixtures --------------------------------------------------------------------------------------------------------------------
def fixture(name) -> bytes:
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read().strip()


def test_replica_identity_fixtures(tf):
    upd, dele = fixture("emitter_replica_identity__canon_change_item_update.txt"), fixture("emitter_replica_identity__canon_change_item_delete.txt")
    other = ci("insert", ("k", "v"), ("5", '"five"'), (col("k", "int64", True), col("v", "utf8")), table="second")
    parsed(check(tf, [arr(upd)], "update")[0], 1)
    parsed(check(tf, [arr(dele)], "delete")[0], 1)
    want, _ = check(tf, [arr(other, upd, other, dele, upd, other)], "interleaved")
    parsed(want)
    assert [g for _, g, _ in want.items] == [0, 1, 0, 2, 1, 0] and [r for _, _, r in want.items] == [0, 0, 1, 0, 1, 2]


# ---- 3. the cut at its edges -----------------------------------------------------------------------------------------------------------------------------------
def padded(n: int) -> bytes:
    """a one-item message of exactly n bytes (white space in front of the closing bracket)"""
    m = arr(ci())
    assert len(m) <= n
    return m[:-1] + b" " * (n - len(m)) + b"]"


def test_cut_message_sizes(tf):
    base = len(arr(ci()))
    sizes = [base, base + 1] + [k * 64 + d for k in (5, 6) for d in (-1, 0, 1)]
    msgs = [b"", b"[]", None, b" [ ] ", b"[", b"]"] + [padded(n) for n in sizes if n >= base]
    for n in (63, 64, 65, 127, 128, 129):   # short messages of exactly these sizes: an unknown member pads the item
        m = b'[{"kind":"insert","pad":"' + b"x" * (n - 28) + b'"}]'
        assert len(m) == n
        msgs.append(m)
    want, _ = check(tf, msgs)
    assert [f[:2] for f in want.fallback] == [(0, "SYNTAX"), (4, "SYNTAX"), (5, "SYNTAX")]


@pytest.mark.parametrize("end", [62, 63, 64])
def test_cut_backslash_runs(tf, end):
    msgs = []
    for run in (1, 2, 3, 64):
        # a string value whose backslash run ends at byte `end` of a 64-byte step, in front of a quote
        head = b'[{"kind":"insert","x":"'
        fill = (end + 1 + 128 - run - len(head)) % 64
        m = head + b"a" * (fill + 64) + b"\\" * run + b'"' + (b'' if run % 2 == 0 else b'}]"') + b'}]'
        assert (m.index(b'\\' * run) + run - 1) % 64 == end % 64
        msgs.append(m)
    want, _ = check(tf, msgs)
    assert not want.fallback and len(want.items) == 4


def test_cut_strings_white_space_and_counts(tf):
    tricky = ci(names=("id", "s"), values=("1", '"[ ] { } , \\" \\\\"'), cols=(col("id", "int32", True), col("s", "utf8")), tx="}]", query="[{")
    spaced = b' \t\r\n[ \n' + tricky.replace(b'"table":"t"', b'"table":"t2"').replace(b',"', b' ,\n "').replace(b'":', b'" : ') + b' ,\t' + tricky + b'\r\n] \n'
    msgs = [spaced]
    for n in (63, 64, 65, 256, 257):
        msgs.append(arr(*[ci(id=i) for i in range(n)]))
    msgs += [arr(ci(id=i)) for i in range(257)]
    want, _ = check(tf, msgs)
    parsed(want)
    assert len(want.items) == 2 + 63 + 64 + 65 + 256 + 257 + 257


def nested(depth: int) -> str:
    return "[" * depth + "]" * depth


def test_depth_limit(tf):
    cols = (col("id", "int32", True), col("a", "any"))
    ok = ci(names=("id", "a"), values=("1", nested(126)), cols=cols)       # the item, columnvalues and 126 arrays: 128 containers
    deep = ci(names=("id", "a"), values=("1", nested(127)), cols=cols)
    uns = ci(names=("id", "a"), values=("1", nested(15) [:15] + '{"b":1,"a":2}' + "]" * 15), cols=cols)    # unsorted keys 16 deep under the value
    uns17 = ci(names=("id", "a"), values=("1", "[" * 16 + '{"b":1,"a":2}' + "]" * 16), cols=cols)
    want, _ = check(tf, [arr(ok), arr(deep), arr(uns), arr(uns17)])
    assert want.fallback == [(1, "DEPTH", 0, -1), (3, "DEPTH", 0, 1)]


# ---- 4. cells ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cells(tf):
    cols = [col("s", "utf8"), col("b0", "string", ot="pg:bytea"), col("b1", "utf8", ot="mysql:varbinary(8)"), col("b2", "string", ot="ydb:String"),
            col("d", "double"), col("f", "float"), col("t", "datetime"), col("dt", "date"), col("a", "any"), col("pj", "any", ot="pg:json"), col("iv", "interval")]
    names = [c["name"] for c in cols]
    rows = [
        ['""', '""', '"QQ=="', '"QUI="', "1.45e-10", "-0", '"2020-01-02T03:04:05Z"', '"2020-01-02T00:00:00.5Z"', '{"z":1,"a":{"y":[],"b":null},"z":2}', '"plain"', "-0"],
        ['"1234567"', '"QUJD"', '"QUJDRA=="', '"+/+/"', "1E5", "123456789012345678901234567890", '"2020-01-02T03:04:05.123456Z"', '"0000-01-01T00:00:00.000000001Z"',
         '[1.0,true,null,{"b":"<&>","a":"\\u00e9"}]', '"\\u003cx\\u003e"', "9223372036854775807"],
        ['"12345678"', "null", "null", "null", "0", "-1.5E-3", '"9999-12-31T23:59:59.999999999Z"', "null", "12.50", "null", "-9223372036854775808"],
        ['"123456789"', '"//8="', '"AA=="', '""', "null", "null", "null", "null", "true", '["s",["t"]]', "null"],
        ['"\\" \\\\ \\/ \\b \\f \\n \\r \\t \\u0041 \\ud83d\\ude00 \\ud800 \\udc00x \\u00e9 é"', "null", "null", "null", "1", "1", "null", "null", "false", "{}", "1"],
    ]
    want, _ = check(tf, [arr(*[ci(names=names, values=r, cols=cols, id=i) for i, r in enumerate(rows)])])
    parsed(want, 1)
    vals = want.groups[0].rows
    assert vals[4][1][0] == ("string", '" \\ / \b \f \n \r \t A 😀 � �x é é'.encode("utf-8"))
    assert vals[0][1][8] == ("json", b'{"a":{"b":null,"y":[]},"z":2}') and vals[1][1][8] == ("json", b'[1.0,true,null,{"a":"\xc3\xa9","b":"\\u003c\\u0026\\u003e"}]')
    assert vals[1][1][5] == ("jsonnum", b"123456789012345678901234567890") and vals[0][1][4] == ("jsonnum", b"1.45e-10")
    assert vals[3][1][1] == ("bytes", b"\xff\xff") and vals[0][1][2] == ("bytes", b"A") and vals[0][1][3] == ("bytes", b"AB")


INT_TYPES = list(R.INT_RANGE)


def test_integer_limits(tf):
    msgs, expect = [], []
    for t in INT_TYPES:
        lo, hi = R.INT_RANGE[t]
        c = (col("v", t),)
        msgs.append(arr(*[ci(names=("v",), values=(str(v),), cols=c, table=t) for v in (lo, hi, 0)] + [ci(names=("v",), values=("-0",), cols=c, table=t)]))
        for v in (lo - 1, hi + 1):
            msgs.append(arr(ci(names=("v",), values=(str(v),), cols=c, table=t)))
            expect.append((len(msgs) - 1, "INT_FORM", 0, 0))
    want, _ = check(tf, msgs)
    assert want.fallback == expect and len(want.groups) == len(INT_TYPES)


# ---- 5. all or nothing ----------------------------------------------------------------------------------------------------------------------------------------------
def bad_items():
    """(reason, column, item) for every fallback reason an item can carry"""
    c2 = (col("id", "int32", True), col("x", "utf8"))
    one = lambda typ, v, ot="": ci(names=("id", "x"), values=("1", v), cols=(col("id", "int32", True), col("x", typ, ot=ot)), table="bad")  # noqa: E731
    ok = ci(names=("id", "x"), values=("1", '"v"'), cols=c2, table="bad")
    return [
        ("UTF8", -1, ok.replace(b'"v"', b'"\xff"')), ("SYNTAX", -1, ok.replace(b'"v"', b'"\\x"')), ("KEY_FORM", -1, ok.replace(b'"kind"', b'"k\\u0069nd"')),
        ("DUP_MEMBER", -1, ok[:-1] + b',"id":5}'), ("HEADER_VALUE", -1, ok.replace(b'"id":1', b'"id":-1')), ("HEADER_VALUE", -1, ok.replace(b'"nextlsn":2', b'"nextlsn":"2"')),
        ("HEADER_VALUE", -1, ok.replace(b'"oldkeys":{}', b'"oldkeys":{"KeyNames":["id"]}')), ("KIND", -1, ok.replace(b'"insert"', b'"truncate"')),
        ("KIND", -1, ok.replace(b'"kind":"insert",', b'')), ("LENGTHS", -1, ok.replace(b'[1,"v"]', b'[1]')),
        ("LENGTHS", -1, ok.replace(b'"insert"', b'"update"').replace(b'"oldkeys":{}', b'"oldkeys":{"keynames":["id"]}')),
        ("INSERT_KEYVALUES", -1, ok.replace(b'"oldkeys":{}', b'"oldkeys":{"keynames":["id"],"keyvalues":[1]}')),
        ("SCHEMA_COLUMN", 1, ci(names=("id", "nope"), values=("1", '"v"'), cols=c2, table="bad")), ("SCHEMA_COLUMN", 1, one("decimal", '"v"')),
        ("SCHEMA_COLUMN", -1, ok.replace(b'"name":"x"', b'"Name":"x"')),
        ("INT_FORM", 1, one("int32", "1.0")), ("INT_FORM", 1, one("int64", "1e3")), ("INT_FORM", 1, one("interval", "1.5")), ("NUM_STRING", 1, one("int32", '"1"')),
        ("NUM_STRING", 1, one("double", '"1.5"')), ("VALUE_TYPE", 1, one("boolean", "1")), ("VALUE_TYPE", 1, one("int32", "[1]")), ("VALUE_TYPE", 1, one("double", "true")),
        ("TIME_ZONE", 1, one("timestamp", '"2020-01-02T03:04:05+04:00"')), ("TIME_FORM", 1, one("timestamp", '"2020-01-02 03:04:05"')),
        ("TIME_FORM", 1, one("date", '"2020-02-30T00:00:00Z"')), ("TIME_FORM", 1, one("datetime", "1577934245")), ("TIME_FORM", 1, one("timestamp", '"2020-01-02T03:04:05.1234567890Z"')),
        ("BASE64", 1, one("string", '"QQ="', "pg:bytea")), ("BASE64", 1, one("string", '"\\/\\/8="', "pg:bytea")),
        ("TIME_FORM", 1, one("timestamp", '"2020-01-02T03:04:05\\u005a"')), ("BASE64", 1, one("string", '"Q Q="', "pg:bytea")), ("ANY_STRING", 1, one("any", '"{}"')),
        ("ANY_STRING", 1, one("any", '[["{}"]]')), ("ANY_PG_TIMESTAMP", 1, one("any", '"2020-01-02T03:04:05Z"', "pg:timestamp without time zone")),
        ("MYSQL_BIT", 1, one("utf8", "5", "mysql:bit(8)")), ("STRING_NONSTRING", 1, one("utf8", "5")), ("STRING_NONSTRING", 1, one("string", "5", "pg:bytea")),
        ("MONGO_BSON", 1, one("any", "{}", "mongo:bson")),
        ("INT_FORM", 2, ok.replace(b'"insert"', b'"delete"').replace(b'"oldkeys":{}', b'"oldkeys":{"keynames":["id"],"keyvalues":[1.5]}')),
    ]


def test_all_or_nothing(tf):
    good = [ci(id=i) for i in range(64)]
    msgs, expect = [], []
    for reason, column, item in bad_items():
        msgs += [arr(*good), arr(*(good + [item])), arr(*good)]
        expect.append((len(msgs) - 2, reason, 64, column))
    # a later item of the same table whose table_schema differs: Restore reads the first one's
    differs = ci(cols=(col("id", "int64", True),))
    msgs.append(arr(*(good + [differs])))
    expect.append((len(msgs) - 1, "SCHEMA_DIFFERS", 64, -1))
    want, _ = check(tf, msgs)
    assert want.fallback == expect
    flagged = {m for m, *_ in expect}
    assert all((g == -1) == (m in flagged) for m, g, _ in want.items) and len(want.groups) == 1


# ---- 6. garbage ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_garbage(tf):
    one = arr(ci())
    msgs = [b"not json", one[:-1], one[: len(one) // 2], ci(), one + b"x", b"[1]", b'["a"]', b"[[]]", b"[{}{}]", b"[{},]", b"[,{}]", b"[{}],", b'[{"a":"]}', b"\xff\xfe", b"[{]}",
            b'[{"a":[}]', arr(ci(names=("id", "x")))]
    want, _ = check(tf, msgs + [one])
    assert [f[0] for f in want.fallback] == list(range(len(msgs))) and want.fallback[-1][1] == "LENGTHS"
    assert [i for i in want.items if i[1] >= 0] == [(len(msgs), 0, 0)]


# ---- 7. the empty and the one-row batch ----------------------------------------------------------------------------------------------------------------------------
def test_empty_and_one_row(tf):
    want, got = check(tf, [])
    assert got.info() == (0, 0, 0)
    want, got = check(tf, [None, b"[]"])
    assert got.info() == (0, 0, 0)
    want, got = check(tf, [arr(ci("delete", None, (), oldkeys='{"keynames":["id"],"keytypes":["integer"],"keyvalues":[4]}'))])
    parsed(want, 1)
    G = want.groups[0]
    assert G.names == [] and G.names_form == 1 and G.rows[0][2] == [("int32", 4)]


def child(body: str, **env):
    """runs `body` in a process of its own (settings the library reads once per process), bound to the same build of the library; it must print ok"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from transferia_amd import abi, lib\nimport os\n"
            "emu = os.environ.get('TFGPU_TEST_EMU_LIB')\n"
            "if emu: lib._LIBPATH = emu\n"
            "lib.init()\nimport test_gpu_nativeparse as T\n" % (here, os.path.dirname(here))) + body + "\nprint('ok')\n"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_weak_hash_groups_by_the_texts(tf):
    # almost every group key collides: the spans decide
    child("msgs = [T.arr(*[T.ci(table='t%d' % (i % 7), id=i) for i in range(100)])]\n"
          "want, _ = T.check(lib, msgs)\nassert len(want.groups) == 7", TFGPU_NATIVE_WEAK_HASH="1")


# ---- 8. many groups; the whole-call refusals ---------------------------------------------------------------------------------------------------------------------
def slim(name, typ):
    return {"name": name, "type": typ}


def batch_of(msgs):
    return abi.message_batch("tp", 0, [(i, 0, None, m, None) for i, m in enumerate(msgs)])


def test_thousands_of_groups(tf):
    """3000 tables in one batch: the descriptor tables, the programs and the scans' totals of one call take megabytes of the library's 8 MiB read-back
    ring, and a few calls take it round more than once — nothing read back may be read again behind a later read-back"""
    n = 3000
    cols = (slim("id", "int32"), slim("s", "utf8"))
    items = [ci(names=("id", "s"), values=(str(i), '"v%d"' % i), cols=cols, table="t%d" % i, id=i) for i in range(n)]
    items += [ci(names=("id", "s"), values=(str(-i), '"second row of %d"' % i), cols=cols, table="t%d" % i, id=n + i) for i in range(0, n, 7)]
    msgs = [arr(*items[:1000]), arr(*items[1000:2500]), arr(*items[2500:])]
    want, got = check(tf, msgs)
    parsed(want, n)
    assert [len(g.rows) for g in want.groups] == [2 if i % 7 == 0 else 1 for i in range(n)]
    info, (m0, g0, r0) = got.info(), got.items()
    for _ in range(4):
        again = tf.native_parse(batch_of(msgs))
        m, g, r = again.items()
        assert again.info() == info and (m == m0).all() and (g == g0).all() and (r == r0).all()
        for k in (0, n // 2, n - 1):
            b = again.group(k).batch.download()
            assert [cell(c, 0) for c in b.cols] == [norm(v) for v in want.groups[k].rows[0][1]], k
        again.free()


def test_too_many_columns_is_refused_by_name(tf):
    n = 65536
    big = ci(names=["c%d" % i for i in range(n)], values=["1"] * n, cols=(slim("c0", "int32"),), table="wide")
    with pytest.raises(tf.TfgpuError) as ex:
        tf.native_parse(batch_of([arr(ci()), arr(big), arr(ci(id=2))]))
    assert ex.value.code == tf.ERR_UNSUPPORTED and "more than 65 535 columns" in str(ex.value) and "wide" in str(ex.value)
    fits = ci(names=["c%d" % i for i in range(n - 1)], values=["1"] * (n - 1), cols=(slim("c0", "int32"),), table="wide")   # one fewer: the device's own answer
    got = tf.native_parse(batch_of([arr(fits)]))
    assert got.fallback() == [(0, "SCHEMA_COLUMN", 0, 1)]
    parsed(check(tf, [arr(ci()), arr(ci(id=2))])[0], 1)   # the library goes on


def test_text_column_limit_is_refused_by_name(tf):
    # TFGPU_TEST_TEXT_LIMIT lowers the 4 GiB bound of a text column (read once per process)
    child("c2 = (T.col('id', 'int32', True), T.col('s', 'utf8'))\n"
          "long = T.arr(T.ci(names=('id', 's'), values=('1', '\"' + 'x' * 100 + '\"'), cols=c2, table='wide'))\n"
          "for msg, what in ((long, 'column s of table wide'), (T.arr(T.ci(tx='t' * 100)), 'tx_id of table t'), (T.arr(T.ci(query='q' * 100)), 'query of table t')):\n"
          "    try:\n"
          "        lib.native_parse(T.batch_of([T.arr(T.ci()), msg]))\n"
          "    except lib.TfgpuError as e:\n"
          "        assert e.code == lib.ERR_UNSUPPORTED and what in str(e) and 'reaches 4 GiB of text' in str(e), str(e)\n"
          "    else:\n"
          "        raise AssertionError('not refused: ' + what)\n"
          "    want, _ = T.check(lib, [T.arr(T.ci(names=('id', 's'), values=('1', '\"short\"'), cols=c2))])\n"
          "    assert not want.fallback and len(want.groups) == 1", TFGPU_TEST_TEXT_LIMIT="64")
