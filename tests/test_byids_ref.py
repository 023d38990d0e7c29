"""filter_rows_by_ids without a device: the plan-level C ABI (the factory with its three config errors, Type, Description, ResultSchema, Suitable), the
plain-Python restatement (tests/byids_ref.py) against the reference's own e2e cases (tests/golden/filter_rows_by_ids.json), and encoding/json's
unquote as the restatement writes it."""
import base64
import json

import numpy as np
import pytest

import byids_ref as ref
from transferia_amd import abi, lib
from util import golden

T = ref.T
G = golden("filter_rows_by_ids.json")


def test_plan_create():
    """The device plan exists (before it did, this raised ERR_UNSUPPORTED: `has no device plan`)."""
    t = lib.Transformer(T, G["pg2pg"]["config"])
    assert t.type() == T
    assert t.description() == ref.DESCRIPTION == "Row filter by allowed IDs"
    assert T not in lib.registry() and len(lib.registry()) == 10
    # its neighbours in the reference's registry stay where they were
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer("mongo_pk_extender", {})
    assert ei.value.code == lib.ERR_UNSUPPORTED and "no device plan" in str(ei.value)


def test_config_errors():
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"tables": {"includeTables": ["("]}, "allowedIDs": ["a"]})
    assert ei.value.code == lib.ERR_CONFIG and "unable to create tables filter: " in str(ei.value)
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"columns": {"excludeColumns": ["[a"]}, "allowedIDs": ["a"]})
    assert ei.value.code == lib.ERR_CONFIG and "unable to create columns filter: " in str(ei.value)
    for cfg in ({}, {"allowedIDs": []}, {"tables": {"includeTables": ["t"]}, "columns": {"includeColumns": ["c"]}, "allowedIDs": None}):
        with pytest.raises(lib.TfgpuError) as ei:
            lib.Transformer(T, cfg)
        assert ei.value.code == lib.ERR_CONFIG and "list of allowed IDs shouldn't be empty" in str(ei.value)
        with pytest.raises(ValueError) as ri:
            ref.factory(cfg)
        assert str(ri.value) == "list of allowed IDs shouldn't be empty"
    # the order of the reference: tables, then columns, then the IDs
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"tables": {"includeTables": ["("]}, "columns": {"includeColumns": ["("]}})
    assert "unable to create tables filter: " in str(ei.value)
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"columns": {"includeColumns": ["("]}})
    assert "unable to create columns filter: " in str(ei.value)
    with pytest.raises(ValueError) as ri:
        ref.factory({"tables": {"includeTables": ["("]}, "allowedIDs": ["a"]})
    assert str(ri.value).startswith("unable to create tables filter: ")
    # an empty ID, duplicates, bytes that are no UTF-8 in the JSON escapes' reach: all fine
    lib.Transformer(T, {"allowedIDs": ["", "a", "a", "\u0000x", "é"]})
    assert ref.factory({"allowedIDs": ["", "a", "a", "é"]}) == {0: {b""}, 1: {b"a"}, 2: {"é".encode()}}


def test_result_schema_is_the_input_schema():
    schema = abi.Schema([abi.ColSchema("id", "utf8", True, "p.id", "pg:text", True, "public", "src", "", False, ""),
                         abi.ColSchema("body", "any", False, "p.body", "pg:jsonb", False, "public", "src", "lower(body)", True, '{"a":1}'),
                         abi.ColSchema("n", "int32", False)])
    rs = lib.Transformer(T, {"allowedIDs": ["x"], "columns": {"includeColumns": ["id"]}}).result_schema(schema)

    def full(s):
        return [[c.name, c.dtype, c.key, c.path, c.original_type, c.required, c.table_schema, c.table_name, c.expression, c.fake_key, c.properties_json] for c in s.cols]
    assert full(rs) == full(schema)


SUITABLE = [
    # (config, ns, table, schema, expect)
    ({"allowedIDs": ["a"]}, "db", "t", [["a", "utf8", True]], True),
    ({"allowedIDs": ["a"]}, "db", "t", [["a", "string", False]], True),
    ({"allowedIDs": ["a"]}, "db", "t", [["a", "any", False]], True),
    ({"allowedIDs": ["a"]}, "db", "t", [["a", "int64", True], ["b", "double", False], ["c", "timestamp", False], ["d", "boolean", False]], False),
    ({"allowedIDs": ["a"]}, "db", "t", [], False),
    ({"allowedIDs": ["a"], "columns": {"includeColumns": ["^id$"]}}, "db", "t", [["id", "int64", True], ["name", "utf8", False]], False),
    ({"allowedIDs": ["a"], "columns": {"includeColumns": ["^id$"]}}, "db", "t", [["x", "int64", True], ["id", "utf8", False]], True),
    ({"allowedIDs": ["a"], "columns": {"excludeColumns": ["name"]}}, "db", "t", [["name", "utf8", False]], False),
    # `document` of `any`: suitable whatever the column filter says; `document` of another type is an ordinary column
    ({"allowedIDs": ["a"], "columns": {"excludeColumns": ["document"]}}, "db", "t", [["_id", "int64", True], ["document", "any", False]], True),
    ({"allowedIDs": ["a"], "columns": {"includeColumns": ["^nested_id$"]}}, "db", "t", [["_id", "int64", True], ["document", "any", False]], True),
    ({"allowedIDs": ["a"], "columns": {"excludeColumns": ["document"]}}, "db", "t", [["document", "utf8", False]], False),
    ({"allowedIDs": ["a"], "columns": {"excludeColumns": ["Document"]}}, "db", "t", [["Document", "any", False]], False),
    # the table: namespace.name and the quoted form; a table that does not match
    ({"allowedIDs": ["a"], "tables": {"includeTables": ["^other$"]}}, "db", "t", [["a", "utf8", True]], False),
    ({"allowedIDs": ["a"], "tables": {"includeTables": ["^other$"]}}, "db", "t", [["document", "any", False]], False),
    ({"allowedIDs": ["a"], "tables": {"includeTables": ["^t$"]}}, "db", "t", [["a", "utf8", True]], False),
    ({"allowedIDs": ["a"], "tables": {"includeTables": ["^t$"]}}, "", "t", [["a", "utf8", True]], True),
    ({"allowedIDs": ["a"], "tables": {"includeTables": ["^db\\.t$"]}}, "db", "t", [["a", "utf8", True]], True),
    ({"allowedIDs": ["a"], "tables": {"includeTables": ['^"db"\\."t"$']}}, "db", "t", [["a", "utf8", True]], True),
    ({"allowedIDs": ["a"], "tables": {"excludeTables": ["t"]}}, "db", "t", [["a", "utf8", True]], False),
]


def test_suitable():
    for cfg, ns, table, spec, want in SUITABLE:
        schema = abi.Schema.of(spec)
        assert ref.suitable(cfg, ns, table, schema) == want, (cfg, ns, table, spec)
        assert lib.Transformer(T, cfg).suitable(ns, table, schema) == want, (cfg, ns, table, spec)
    for name in ("pg2pg", "mongo2mongo"):
        g = G[name]
        schema = abi.Schema.of(g["schema"])
        assert ref.suitable(g["config"], g["ns"], g["table"], schema) and lib.Transformer(T, g["config"]).suitable(g["ns"], g["table"], schema)
    g = G["ydb2ydb"]
    assert lib.Transformer(T, g["config"]).suitable("", g["table"], abi.Schema.of(g["schema"]))


# ---- the reference's e2e cases through the restatement ------------------------------------------------------------------------------------------------
def rows_batch(spec, rows, ns, table, kinds=None):
    schema = abi.Schema.of(spec)
    gotype = {"utf8": "string", "string": "bytes", "int32": "int32", "uint64": "uint64"}
    vals = [[[gotype[c[1]], v] for c, v in zip(spec, row)] for row in rows]
    b = abi.batch_from_rows(schema, [c[0] for c in spec], vals, ns, table, kinds)
    b.schema = schema
    return b


def test_golden_pg2pg():
    g = G["pg2pg"]
    snap = rows_batch(g["schema"], g["snapshot_rows"], g["ns"], g["table"])
    target = {}
    kept, idx = ref.apply(g["config"], snap)
    assert idx == [1, 2]                                            # ID1 by `id`, ID2 by the prefix ID2_2 of `id2`
    for i in range(kept.nrows):
        target[kept.col("id").get_bytes(i).decode()] = int(kept.col("val").values[i])
    rep = rows_batch(g["schema"], [r["row"] for r in g["replicated"]], g["ns"], g["table"], [r["kind"] for r in g["replicated"]])
    kept, idx = ref.apply(g["config"], rep)
    assert idx == [1, 2, 4] and kept.kind.tolist() == [abi.K_UPDATE, abi.K_UPDATE, abi.K_INSERT]   # Updates are judged like Inserts
    for i in range(kept.nrows):
        target[kept.col("id").get_bytes(i).decode()] = int(kept.col("val").values[i])
    assert len(target) == g["expect_target_rows"] and target == g["expect_target"]


def test_golden_ydb2ydb():
    g = G["ydb2ydb"]
    table = {}
    for push in g["pushes"]:
        b = rows_batch(g["schema"], push, "", g["table"])
        kept, _ = ref.apply(g["config"], b)
        for i in range(kept.nrows):
            table[int(kept.col("id").values[i])] = [int(kept.col("id").values[i]), base64.b64encode(kept.col("id2").get_bytes(i)).decode(), kept.col("id3").get_bytes(i).decode(),
                                                    int(kept.col("value").values[i])]
    assert [table[k] for k in sorted(table)] == [c["columnvalues"] for c in g["canon_kept"]]


def test_golden_mongo_what_a_device_batch_can_say():
    """the documents as a device batch could hold them — `_id` and the document as JSON text: `_id` is judged as everywhere, the `document` column is
    skipped by the restatement (no DValue) where the reference would look inside, so the device refuses the batch by name (tests/test_gpu_byids.py)"""
    g = G["mongo2mongo"]
    n = len(g["documents"])
    docs = [json.dumps(d, separators=(",", ":")).encode() for d in g["documents"]]
    b = abi.Batch([abi.column_from_values("_id", "utf8", [["string", d["_id"]] for d in g["documents"]]),
                   abi.column_from_values("document", "any", [["json", x] for x in docs])], n, g["ns"], g["table"])
    b.schema = abi.Schema.of(g["schema"])
    _, idx = ref.apply(g["config"], b)
    by_id_alone = [g["documents"][i]["_id"] for i in idx]
    assert by_id_alone == ["ID1", "ID4"] and set(by_id_alone) < set(g["expect_target_ids"])
    assert ref.MONGO_REFUSAL == "Mongo `document` columns stay with the stock transformer"


# ---- the restatement's own corners --------------------------------------------------------------------------------------------------------------------
def test_is_id_allowed():
    by_len = ref.factory({"allowedIDs": ["ab", "abc", "x", "ab"]})
    assert by_len == {2: {b"ab"}, 3: {b"abc"}, 1: {b"x"}}
    for v, want in ((b"", False), (b"a", False), (b"ab", True), (b"abd", True), (b"abc", True), (b"xyz", True), (b"y", False), (b"ba", False), (b"aB", False)):
        assert ref.is_id_allowed(by_len, v) == want, v
    with_empty = ref.factory({"allowedIDs": ["", "zz"]})
    assert ref.is_id_allowed(with_empty, b"") and ref.is_id_allowed(with_empty, b"anything")
    assert ref.is_id_allowed(ref.factory({"allowedIDs": ["\xff".encode("latin-1").decode("latin-1")]}), "ÿ".encode())   # bytes, not runes: the ID's UTF-8


def test_go_unquote():
    for text in ['"plain"', '""', '"q\\"b\\\\s\\/"', '"\\b\\f\\n\\r\\t"', '"\\u00e9\\u4e16"', '"\\ud83d\\ude00"', '"é世😀"', '"a\\u0000b"']:
        assert ref.go_unquote(text.encode()) == json.loads(text).encode("utf-8"), text
    rep = "�".encode()
    assert ref.go_unquote(b'"\\ud800"') == rep and ref.go_unquote(b'"\\udc00x"') == rep + b"x"
    assert ref.go_unquote(b'"\\ud800\\u0041"') == rep + b"A"           # the escape behind a lone surrogate is read on its own
    assert ref.go_unquote(b'"\\ud800\\ud800\\udc00"') == rep + "\U00010000".encode()
    assert ref.go_unquote(b'"\\udc00\\ud800"') == rep + rep
    assert ref.go_unquote(b'"a\xffb\xc3"') == b"a" + rep + b"b" + rep  # raw bytes that are no UTF-8 are coerced
    assert ref.go_unquote(b'"\xed\xa0\x80"') == rep * 3 and ref.go_unquote(b'"\xc0\x80"') == rep * 2
    assert ref.go_unquote(b'"\\x"') is None and ref.go_unquote(b'"\\u12"') is None and ref.go_unquote(b'"a') is None
    assert ref.json_text_as_string(b' "s" ') == b"s"
    for text in (b'{"a":"s"}', b'["s"]', b"17", b"true", b"false", b"null", b"-1.5e3", b""):
        assert ref.json_text_as_string(text) is None


def test_should_keep_walks_the_schema_and_reads_as_map():
    cfg = {"allowedIDs": ["ID"], "columns": {"excludeColumns": ["^skip$"]}}
    cols = [abi.column_from_values("a", "utf8", [["string", "x"], ["string", "IDa"], ["nil", None], ["string", "x"], ["string", "x"], ["string", "x"]]),
            abi.column_from_values("skip", "utf8", [["string", "ID"]] * 6),
            abi.column_from_values("n", "utf8", [["jsonnum", "1"], ["jsonnum", "2"], ["jsonnum", "3"], ["jsonnum", "4"], ["jsonnum", "5"], ["jsonnum", "6"]]),
            abi.column_from_values("j", "any", [["json", '"IDj"'], ["json", "{}"], ["json", '"id"'], ["json", '["ID"]'], ["json", "null"], ["json", '"I\\u0044"']]),
            abi.column_from_values("a", "utf8", [["string", "x"], ["string", "x"], ["string", "IDlast"], ["string", "x"], ["string", "ID"], ["string", "ID"]])]
    b = abi.Batch(cols, 6, "db", "t")
    b.kind = np.array([0, 0, 1, 0, 2, 3], np.uint8)
    assert ref.kept_rows(cfg, b) == [0, 2]          # row 1: the LAST `a` is read; rows 4, 5: a Delete and a non-row kind have no ColumnNames
    b.cols[4].absent = np.array([False, False, True, False, False, False])
    assert ref.kept_rows(cfg, b) == [0]             # row 2 does not list the last `a`: the first one, a nil there, is the entry
    b.schema = abi.Schema.of([["j", "int64", False], ["a", "utf8", False], ["gone", "utf8", False]])
    b.cols[4].absent = None
    assert ref.kept_rows(cfg, b) == [2]             # the schema's DataType decides: `j` is no text column there
