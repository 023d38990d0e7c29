"""raw_doc_grouper without a device: the reference's own cases (tests/golden/raw_doc_grouper.json) through the plain-Python restatement
(tests/rawdoc_ref.py), and the plan-level C ABI pinned to the same file — the factory with both of its config errors, the shouldUpdateOldKeys refusal,
Suitable, Description, ResultSchema with the pg: stubs and the kept ColSchema fields — and the entries a raw_doc_grouper may not go through."""
import ctypes as C
import json

import numpy as np
import pytest

import rawdoc_ref as ref
from transferia_amd import abi, lib
from util import golden, item_to_batch

T = "raw_doc_grouper"
G = golden("raw_doc_grouper.json")


def test_plan_create():
    """The device plan exists (before it did, this raised ERR_UNSUPPORTED: `has no device plan`)."""
    t = lib.Transformer(T, {"keys": ["watchid"], "tables": {"includeTables": ["^hits$"]}})
    assert t.type() == T
    assert T not in lib.registry() and len(lib.registry()) == 10


def test_factory_rules():
    assert len(G["configs"]) == 3 and sum(c["error"] is not None for c in G["configs"]) == 2
    for c in G["configs"]:
        if c["error"] is None:
            assert ref.factory(c["config"]) == (c["keys"], c["fields"])
            assert lib.Transformer(T, c["config"]).description() == ref.description(c["config"])
            continue
        with pytest.raises(ValueError) as ri:
            ref.factory(c["config"])
        assert str(ri.value) == c["error"]
        with pytest.raises(lib.TfgpuError) as ei:
            lib.Transformer(T, c["config"])
        assert ei.value.code == lib.ERR_CONFIG and c["error"] in str(ei.value), c["name"]
    # etl_updated_at / doc are appended only where neither list names them
    assert ref.factory({"keys": ["a", "etl_updated_at"], "fields": ["doc", "b"]}) == (["a", "etl_updated_at"], ["doc", "b"])
    assert ref.factory({"keys": ["a"]}) == (["a"], ["etl_updated_at", "doc"])
    # ... so `doc` as a key AND a field is the second rule
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"keys": ["doc"], "fields": ["doc"]})
    assert ei.value.code == lib.ERR_CONFIG and "Can't use same column as key and non-key : doc" in str(ei.value)
    # a bad table regexp, with the reference's wrapping
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"keys": ["a"], "tables": {"includeTables": ["("]}})
    assert ei.value.code == lib.ERR_CONFIG and "unable to init table filter: unable to compile include regexp: (" in str(ei.value)
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"keys": ["a"], "tables": {"excludeTables": ["[a"]}})
    assert ei.value.code == lib.ERR_CONFIG and "unable to init table filter: unable to compile exclude regexp: [a" in str(ei.value)


def test_description():
    assert lib.Transformer(T, {"keys": ["col1", "col2"], "fields": ["col3"]}).description() == "Return item as primary keys col1, col2 and json, containing the rest"
    assert lib.Transformer(T, {}).description() == "Return item as primary keys  and json, containing the rest"


def test_should_update_old_keys_is_refused_by_name():
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"keys": ["col1", "col2"], "shouldUpdateOldKeys": True})
    assert ei.value.code == lib.ERR_UNSUPPORTED and "shouldUpdateOldKeys" in str(ei.value) and T in str(ei.value) and "ragged OldKeys" in str(ei.value)
    lib.Transformer(T, {"keys": ["col1", "col2"], "shouldUpdateOldKeys": False})
    # the factory's own errors come first, as in the reference (the flag is only stored there)
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"keys": ["k", "k"], "shouldUpdateOldKeys": True})
    assert ei.value.code == lib.ERR_CONFIG


def test_cdc_grouper_stays_refused():
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer("raw_cdc_doc_grouper", {"keys": ["a"]})
    assert ei.value.code == lib.ERR_UNSUPPORTED and "no device plan" in str(ei.value)


def test_suitable():
    s = G["suitable"]
    assert [c["expect"] for c in s["cases"]] == [True, False, True, False, False, False]
    t = lib.Transformer(T, s["config"])
    for c in s["cases"]:
        _b, schema = item_to_batch(c["item"])
        assert ref.suitable(s["config"], c["item"]["ns"], c["item"]["table"], schema) == c["expect"], c["item"]["params"]
        assert t.suitable(c["item"]["ns"], c["item"]["table"], schema) == c["expect"], c["item"]["params"]
    # 'Wrong columns fail transfer': unsuitable whatever the table
    w = G["wrong_columns"]
    t = lib.Transformer(T, w["config"])
    for it in w["items"]:
        _b, schema = item_to_batch(it)
        assert not t.suitable("", "", schema) and not ref.suitable(w["config"], "", "", schema)
    # etl_updated_at / doc need not be in the schema, wherever they are configured
    schema = abi.Schema.of([["a", "int64", True], ["b", "utf8", False]])
    for cfg in ({"keys": ["a", "etl_updated_at"]}, {"keys": ["a"], "fields": ["doc", "b"]}):
        assert lib.Transformer(T, cfg).suitable("db", "t", schema) and ref.suitable(cfg, "db", "t", schema)
    assert not lib.Transformer(T, {"keys": ["a"], "fields": ["c"]}).suitable("db", "t", schema)
    # the table filter sees namespace.name and the quoted form (TableFqtnVariants: the bare name only where there is no namespace)
    for inc, want in ((["^t$"], False), (["t$"], True), (["^db\\.t$"], True), (['^"db"\\."t"$'], True), (["^x$"], False)):
        cfg = {"keys": ["a"], "tables": {"includeTables": inc}}
        assert lib.Transformer(T, cfg).suitable("db", "t", schema) == want == ref.suitable(cfg, "db", "t", schema)
    assert not lib.Transformer(T, {"keys": ["a"], "tables": {"excludeTables": ["t"]}}).suitable("db", "t", schema)


def full(schema):
    return [[c.name, c.dtype, c.key, c.path, c.original_type, c.required, c.table_schema, c.table_name, c.expression, c.fake_key, c.properties_json] for c in schema.cols]


def test_result_schema():
    v = G["values_are_parsed"]
    t = lib.Transformer(T, v["config"])
    for c in v["cases"]:
        _b, schema = item_to_batch(c["item"])
        rs = t.result_schema(schema)
        assert [[x.name, x.key] for x in rs.cols] == v["result_schema"]
        assert full(rs) == full(ref.result_schema(v["config"], schema))
        assert [x.dtype for x in rs.cols][3:] == ["timestamp", "any"] and [x.original_type for x in rs.cols][3:] == ["", ""]
    # 'System events schema fixed'
    se = G["system_events"]
    for cols in se["schemas"]:
        rs = lib.Transformer(T, se["config"]).result_schema(abi.Schema.of(cols))
        assert [x.name for x in rs.cols] == se["expect_schema_columns"] and [x.key for x in rs.cols] == [True, True, False, False]
    # an existing column keeps every other ColSchema field; keys in CONFIG order; a key that was none, a field that was one; pg: stubs
    schema = abi.Schema([abi.ColSchema("id", "int64", True, "p.id", "pg:bigint", True, "public", "src", "", False, ""),
                         abi.ColSchema("body", "utf8", False, "p.body", "pg:text", False, "public", "src", "lower(body)", True, '{"a":1}'),
                         abi.ColSchema("skipped", "double", False),
                         abi.ColSchema("ts", "datetime", True, "", "pg:timestamp without time zone")])
    cfg = {"keys": ["body", "etl_updated_at", "id"], "fields": ["ts"]}
    rs = lib.Transformer(T, cfg).result_schema(schema)
    assert full(rs) == full(ref.result_schema(cfg, schema))
    assert full(rs) == [["body", "utf8", True, "p.body", "pg:text", False, "public", "src", "lower(body)", True, '{"a":1}'],
                        ["etl_updated_at", "timestamp", True, "", "pg:timestamp without time zone", False, "", "", "", False, ""],
                        ["id", "int64", True, "p.id", "pg:bigint", True, "public", "src", "", False, ""],
                        ["ts", "datetime", False, "", "pg:timestamp without time zone", False, "", "", "", False, ""],
                        ["doc", "any", False, "", "pg:json", False, "", "", "", False, ""]]
    # "contains", not "starts with"
    rs = lib.Transformer(T, {"keys": ["a"]}).result_schema(abi.Schema.of([["a", "utf8", False, "", "mysql:xpg:y"]]))
    assert [x.original_type for x in rs.cols] == ["mysql:xpg:y", "pg:timestamp without time zone", "pg:json"]
    # a configured name the schema lacks is left out (Suitable is what answers for it)
    rs = lib.Transformer(T, {"keys": ["a", "nosuch"], "fields": ["gone"]}).result_schema(abi.Schema.of([["a", "utf8", False]]))
    assert [[x.name, x.key] for x in rs.cols] == [["a", True], ["etl_updated_at", False], ["doc", False]]


def test_golden_values_through_the_restatement(oracle):
    v = G["values_are_parsed"]
    for c in v["cases"]:
        b, _schema = item_to_batch(c["item"])
        out, errs = ref.apply(oracle, v["config"], b, [c["item"]["commit_time"]])
        assert errs == [] and out.nrows == 1
        assert sorted(x.name for x in out.cols) == sorted(v["result_columns"])
        assert [x.name for x in out.cols][-2:] == ["etl_updated_at", "doc"]
        assert out.col("doc").get_bytes(0) == c["expect_doc"].encode(), c["item"]["params"]
        assert (int(out.col("etl_updated_at").values[0]), int(out.col("etl_updated_at").nanos[0])) == tuple(G["etl_updated_at"])
        for name in ("col1", "col2", "col3"):   # the kept values are the item's own
            assert out.col(name).pyvalue(0) == b.col(name).pyvalue(0)
        assert [[x.name, x.key] for x in out.schema.cols] == v["result_schema"]
        assert out.kind.tolist() == [abi.KIND_ID["update"]]


def test_golden_schemas_and_unsuitable_items_through_the_restatement(oracle):
    d = G["different_schemas"]
    by_input = {}   # the reference keeps one target schema per input schema hash: the result is a function of the input schema
    for it in d["items"]:
        b, schema = item_to_batch(it)
        out, errs = ref.apply(oracle, d["config"], b, [it["commit_time"]])
        assert errs == [] and sorted(x.name for x in out.cols) == sorted(d["result_columns"])
        assert by_input.setdefault(json.dumps(full(schema)), full(out.schema)) == full(out.schema)
    assert len(by_input) == d["distinct_schemas"]
    assert len({json.dumps(v) for v in by_input.values()}) == 2   # (col1 as string, col1 as int32: two of the three results read alike)
    w = G["wrong_columns"]
    for it in w["items"]:
        b, _schema = item_to_batch(it)
        out, errs = ref.apply(oracle, w["config"], b, [it["commit_time"]])
        assert out.nrows == w["expect_transformed"] and len(errs) == w["expect_errors"]


def test_restatement_details(oracle):
    """what the golden cases do not reach: the overwrite order around `_rest`, a `_rest` that is no map, ABSENT cells, the string escapes, the times"""
    schema = abi.Schema.of([["b", "utf8", False], ["_rest", "any", False], ["a", "int64", False]])
    rows = [[["string", "x"], ["json", '{"a":"rest","b":"rest","m":[1,{"z":null}]}'], ["int64", 7]],
            [["string", "y"], ["json", "[1]"], ["int64", 8]],
            [["string", "z"], ["nil", None], ["int64", 9]]]
    b = abi.batch_from_rows(schema, ["b", "_rest", "a"], rows, "db", "t")
    out, _ = ref.apply(oracle, {"keys": ["a"]}, b, None)
    assert [out.col("doc").get_bytes(i) for i in range(3)] == [b'{"a":7,"b":"rest","m":[1,{"z":null}]}', b'{"_rest":[1],"a":8,"b":"y"}', b'{"_rest":null,"a":9,"b":"z"}']
    assert [c.name for c in out.cols] == ["a", "etl_updated_at", "doc"] and out.col("etl_updated_at").values.tolist() == [0, 0, 0]
    b.col("a").absent = np.array([True, False, False])
    b.col("b").absent = np.array([False, True, False])
    out, _ = ref.apply(oracle, {"keys": ["a"]}, b, None)
    assert [out.col("doc").get_bytes(i) for i in range(2)] == [b'{"a":"rest","b":"rest","m":[1,{"z":null}]}', b'{"_rest":[1],"a":8}']
    assert ref.json_string(b'a"\\\x01\n<>&\xff\xe2\x80\xa8\xf0\x9f\x98\x80\xed\xa0\x80') == b'"a\\"\\\\\\u0001\\n<>&\\ufffd\\u2028\xf0\x9f\x98\x80\\ufffd\\ufffd\\ufffd"'
    assert [ref.etl_time(x) for x in (0, 1, 999999999, 10**9, 1 << 63, (1 << 64) - 1)] == [(0, 0), (0, 1), (0, 999999999), (1, 0), (-9223372037, 145224192), (-1, 999999999)]
    assert ref.rfc3339nano(1677510100, 0) == b"2023-02-27T15:01:40Z" and ref.rfc3339nano(-1, 500) == b"1969-12-31T23:59:59.0000005Z"


def test_where_a_raw_doc_grouper_may_not_go():
    L = lib.load()
    grp, flt = lib.Transformer(T, {"keys": ["a"]}), lib.Transformer("filter_rows", {"filter": "a > 1"})
    split = lib.Transformer("table_splitter_transformer", {"columns": ["a"]})
    # tfgpu_apply / tfgpu_apply_split: refused from the plans alone, naming the entry that runs it
    for chain in ([grp], [flt, grp], [grp, flt]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        out, nerr = C.c_void_p(), C.c_int64(0)
        rc = L.tfgpu_apply(arr, len(chain), None, C.byref(out), None, 0, C.byref(nerr))
        assert rc == lib.ERR_UNSUPPORTED and "tfgpu_apply_meta" in L.tfgpu_last_error().decode() and T in L.tfgpu_last_error().decode()
    for chain in ([grp, split], [flt, grp, split]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        out, nerr = C.c_void_p(), C.c_int64(0)
        rc = L.tfgpu_apply_split(arr, len(chain), None, C.byref(out), None, 0, C.byref(nerr))
        assert rc == lib.ERR_UNSUPPORTED and "tfgpu_apply_meta" in L.tfgpu_last_error().decode() and T in L.tfgpu_last_error().decode()
    # tfgpu_apply_meta itself sends a table splitter where it belongs, and still checks its arguments
    arr = (C.c_void_p * 2)(grp._h, split._h)
    out, nerr = C.c_void_p(), C.c_int64(0)
    assert L.tfgpu_apply_meta(arr, 2, None, None, C.byref(out), None, 0, C.byref(nerr)) == lib.ERR_UNSUPPORTED and "tfgpu_apply_split" in L.tfgpu_last_error().decode()
    arr = (C.c_void_p * 1)(grp._h)
    assert L.tfgpu_apply_meta(arr, 1, None, None, C.byref(out), None, 0, C.byref(nerr)) == lib.ERR_INVALID
    # tfgpu_transformation_create / _from_config
    for chain in ([grp], [flt, grp]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        h = C.c_void_p()
        rc = L.tfgpu_transformation_create(arr, len(chain), C.byref(h))
        assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    L.tfgpu_transformation_from_config.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.tfgpu_transformation_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    cfg = {"transformers": [{"filterRows": {"tables": {}, "filter": "id > 1"}}, {"rawDocGrouper": {"keys": ["id"]}, "transformerId": "t-2"}]}
    rc = L.tfgpu_transformation_from_config(json.dumps(cfg).encode(), None, 0, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    extra = (C.c_void_p * 1)(grp._h)
    rc = L.tfgpu_transformation_from_config(json.dumps({"transformers": cfg["transformers"][:1]}).encode(), extra, 1, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    cfg["transformers"][1]["rawDocGrouper"]["keys"] = ["id", "id"]
    rc = L.tfgpu_transformation_from_config(json.dumps(cfg).encode(), None, 0, C.byref(h))
    assert rc == lib.ERR_CONFIG and "unable to init: " + T in L.tfgpu_last_error().decode() and "Can't use same keys column names twice: id, id" in L.tfgpu_last_error().decode()
    # the chain without it still builds
    assert L.tfgpu_transformation_from_config(json.dumps({"transformers": cfg["transformers"][:1]}).encode(), None, 0, C.byref(h)) == 0
    L.tfgpu_transformation_destroy(h)

