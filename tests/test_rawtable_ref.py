"""raw_to_table without a device: the reference's own test vectors (tests/golden/raw_to_table.json) through the plain-Python restatement
(tests/rawtable_ref.py), and the host half of the C ABI pinned to the same file — create / free, Validate's two error texts, both schemas field by
field, the table names with the suffix that is appended as it stands — plus the size refusals, which are judged before a byte is read."""
import numpy as np
import pytest

import rawtable_ref as ref
from transferia_amd import abi, lib
from util import golden

G = golden("raw_to_table.json")


def test_plan_create():
    """The parser exists (before it did, the library had no tfgpu_raw_to_table_create)."""
    p = lib.RawToTable.create("t", "string")
    assert p._h
    p.free()
    assert p._h is None
    for cfg in ({"TableName": "t", "ValueType": "json", "IsTimestampEnabled": True, "IsHeadersEnabled": True, "DLQSuffix": ""},   # ParserConfigRawToTableLb
                {"TableName": "", "IsKeyEnabled": True, "KeyType": "bytes", "ValueType": "string", "IsTimestampEnabled": False, "IsHeadersEnabled": False, "DLQSuffix": "_x"}):
        q = lib.RawToTable.from_config(cfg)
        assert [c[:2] for c in q.schema().triples()] == [c[:2] for c in ref.schema(ref.config(cfg), False)]
        q.free()


def test_golden_file_is_whole():
    assert [d["test"] for d in G["do"]].count("TestDo_ValidMessages") == 6
    assert [d["test"] for d in G["do"]].count("TestDo_SendsToDLQ") == 4
    assert len(G["do"]) == 14 and len(G["validate"]) == 3 and len(G["schema"]) == 1


@pytest.mark.parametrize("case", G["validate"], ids=lambda c: c["name"])
def test_validate(case):
    c = case["config"]
    if case["error"] is None:
        ref.config(c)
        lib.RawToTable.from_config(c).free()
        return
    with pytest.raises(ref.ConfigError) as ri:
        ref.config(c)
    assert str(ri.value) == case["error"]
    for make in (lambda: lib.RawToTable.from_config(c),
                 lambda: lib.RawToTable.create(value_type=c["ValueType"], key_type=c["KeyType"], is_key_enabled=c["IsKeyEnabled"])):
        with pytest.raises(lib.TfgpuError) as ei:
            make()
        assert ei.value.code == lib.ERR_CONFIG and str(ei.value).endswith(": " + case["error"])


def test_key_type_is_judged_only_with_the_key():
    c = {"IsKeyEnabled": False, "KeyType": "blablabla", "ValueType": "bytes"}
    assert ref.config(c)["ValueType"] == "bytes"
    lib.RawToTable.from_config(c).free()
    lib.RawToTable.from_config({"ValueType": "string"}).free()   # the Lb form: no key fields at all
    with pytest.raises(lib.TfgpuError) as ei:
        lib.RawToTable.from_config({"TableName": "t"})
    assert ei.value.code == lib.ERR_CONFIG and "invalid parser config - unsupported value type: " in str(ei.value)


def _schema_rows(s: abi.Schema):
    for c in s.cols:   # newColSchema leaves every other field empty
        assert (c.path, c.original_type, c.table_schema, c.table_name, c.expression, c.fake_key, c.properties_json) == ("", "", "", "", "", False, "")
    return [[c.name, c.dtype, c.key, c.required] for c in s.cols]


def test_schema_golden():
    for case in G["schema"]:
        c = ref.config(case["config"])
        assert ref.schema(c, case["dlq"]) == case["columns"]
        p = lib.RawToTable.from_config(case["config"])
        assert _schema_rows(p.schema(abi.RTT_DLQ if case["dlq"] else abi.RTT_MAIN)) == case["columns"]


@pytest.mark.parametrize("vt", ref.TYPES)
@pytest.mark.parametrize("kt", (None,) + ref.TYPES)
def test_both_schemas_field_by_field(kt, vt):
    for ts in (False, True):
        for hd in (False, True):
            cfg = {"ValueType": vt, "IsKeyEnabled": kt is not None, "KeyType": kt or "", "IsTimestampEnabled": ts, "IsHeadersEnabled": hd}
            c = ref.config(cfg)
            p = lib.RawToTable.create("", vt, kt, ts, hd)
            assert _schema_rows(p.schema(abi.RTT_MAIN)) == ref.schema(c, False)
            dlq = _schema_rows(p.schema(abi.RTT_DLQ))
            assert dlq == ref.schema(c, True)
            # the dead-letter table does not depend on the flags: always timestamp, headers, key and value as bytes, and the reason
            assert dlq == [["topic", "utf8", True, True], ["partition", "uint32", True, True], ["offset", "uint32", True, True], ["timestamp", "timestamp", False, True],
                           ["headers", "any", False, False], ["key", "string", False, False], ["value", "string", False, False], ["failure_reason", "utf8", False, False]]


@pytest.mark.parametrize("table,suffix,topic,main,dlq", [
    ("base", "", "tp", "base", "base_dlq"),
    ("base", "errors", "tp", "base", "baseerrors"),      # appended as it stands: the code and its test decide, not the doc comment
    ("base", "_errors", "tp", "base", "base_errors"),
    ("", "", "test_topic", "test_topic", "test_topic_dlq"),
    ("", "x", "", "", "x"),
])
def test_table_names(table, suffix, topic, main, dlq):
    c = ref.config({"TableName": table, "ValueType": "bytes", "DLQSuffix": suffix})
    assert (ref.table_name(c, False, topic), ref.table_name(c, True, topic)) == (main, dlq)
    p = lib.RawToTable.create(table, "bytes", dlq_suffix=suffix)
    assert (p.table_name(abi.RTT_MAIN, topic), p.table_name(abi.RTT_DLQ, topic)) == (main, dlq)


@pytest.mark.parametrize("case", G["do"], ids=lambda c: c["name"])
def test_restatement_against_golden(case):
    c = ref.config(case["config"])
    main, dlq, fb = ref.do_batch(c, case["topic"], case["partition"], [ref.golden_message(case["message"])])
    assert fb == []
    rows = dlq if case["dlq"] else main
    assert len(main) + len(dlq) == 1 and len(rows) == 1
    assert rows[0][1] == [ref.golden_cell(v) for v in case["values"]]
    assert ref.table_name(c, case["dlq"], case["topic"]) == case["table"]
    assert len(rows[0][1]) == len(ref.schema(c, case["dlq"]))


def test_restatement_json_grammar():
    ok = [b"1", b" 1 ", b"-0", b"1E5", b"1e+5", b"0.5", b'"a"', b"null", b"[1,2]", b'{"a":{"b":[]}}', b'"\\ud800"', b'"\xff"', b"\t[ ]\n"]
    bad = [b"", b" ", b"01", b"1.", b".5", b"-", b"1e", b'"\\x"', b'"a\nb"', b"[1,", b'{"a"}', b'{"a":1,}', b"[1 2]", b"1 2", b"nul", b"NaN", b"Infinity", b"'a'", b'{"a":1}x']
    for b in ok:
        assert ref.json_decode(b)[0], b
    for b in bad:
        assert not ref.json_decode(b)[0], b
    assert ref.marshal(ref.json_decode(b'{"b":1E5,"a":"<\\u00e9\xff>","b":[2 , {"z":null,"y":"\\ud800\\udc00"}]}')[1]) == \
        b'{"a":"\\u003c\xc3\xa9\xef\xbf\xbd\\u003e","b":[2,{"y":"\xf0\x90\x80\x80","z":null}]}'
    assert ref.marshal_headers({"b": "x", "a": b"\xff<"}) == b'{"a":"\\ufffd\\u003c","b":"x"}'
    assert ref.marshal_headers({}) == b"{}" and ref.marshal_headers(None) == b"null"
    with pytest.raises(ref.HostFallback):
        ref.json_decode(b"[" * 129 + b"]" * 129)
    assert ref.json_decode(b"[" * 128 + b"]" * 128)[2] == 128


# ---- the refusals that are judged from the stated sizes alone ---------------------------------------------------------------------------------------------
def _empty_batch(n=0):
    b = abi.CMessageBatch()
    start = np.zeros(n + 1, np.uint64)
    b.topic, b.mem, b.nmsg, b.value_start = b"t", abi.MEM_HOST, n, start.ctypes.data
    b._keep = (start,)
    return b, start


def test_refusals_by_name_need_no_byte():
    b, start = _empty_batch(2)
    lib.raw_to_table_check_sizes(b)
    # offsets that claim 4 GiB of values: refused before `values` (NULL here) is looked at
    start[2] = 1 << 32
    b.values_len = 1 << 32
    for which in ("values_len", "start"):
        with pytest.raises(lib.TfgpuError) as ei:
            lib.raw_to_table_check_sizes(b)
        assert ei.value.code == lib.ERR_UNSUPPORTED and "the values reach 4 GiB" in str(ei.value)
        b.values_len = 16   # the second turn: only the last start claims it
    b, start = _empty_batch(2)
    b.keys_len = (1 << 32) - 1
    with pytest.raises(lib.TfgpuError) as ei:
        lib.raw_to_table_check_sizes(b)
    assert ei.value.code == lib.ERR_UNSUPPORTED and "the keys reach 4 GiB" in str(ei.value)
    b, start = _empty_batch(2)
    b.nmsg = 1 << 31
    with pytest.raises(lib.TfgpuError) as ei:
        lib.raw_to_table_check_sizes(b)
    assert ei.value.code == lib.ERR_UNSUPPORTED and "more than 2^31-1 messages" in str(ei.value)
    b, start = _empty_batch(2)
    b.nmsg, b.topic, b.value_start = (1 << 31) - 1, b"x" * 8, None   # 16 GiB of topic text (no start array: none is read)
    with pytest.raises(lib.TfgpuError) as ei:
        lib.raw_to_table_check_sizes(b)
    assert ei.value.code == lib.ERR_UNSUPPORTED and "the topic column reaches 4 GiB" in str(ei.value)


def test_geometry_accessors():
    chunk, long_ = lib.rawtt_geometry()
    assert chunk >= 4 and long_ >= 2 * chunk   # a chunk looks back three bytes; a long message has more than one chunk
