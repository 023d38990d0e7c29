"""table_splitter_transformer without a device: the reference's own cases through the plain-Python restatement (tests/table_split_ref.py), and the
plan-level C ABI — Type, Description with the reference's two quirks, Suitable, ResultSchema, the useLegacyLf refusal, and the entries a splitter may
not go through."""
import ctypes as C
import json

import pytest

import table_split_ref as ref
from transferia_amd import abi, lib
from util import golden, item_to_batch

T = "table_splitter_transformer"
G = golden("table_splitter.json")


def test_plan_create():
    """The device plan exists (before it did, this raised ERR_UNSUPPORTED: `has no device plan`)."""
    t = lib.Transformer(T, {"columns": ["eventdate", "regionid"], "splitter": "/", "tables": {"includeTables": ["^hits$"]}})
    assert t.type() == T


def test_golden_names_through_the_restatement(oracle):
    assert len(G["replacement"]) == 7
    for case in G["replacement"]:
        b, _schema = item_to_batch(case["item"])
        cfg = {"columns": case["columns"], "splitter": case["splitter"]}
        assert ref.table_names(oracle, cfg, b) == [case["expect"].encode()], case["expect"]
        names, ids, rows = ref.split(oracle, cfg, b)
        assert names == [case["expect"].encode()] and ids.tolist() == [0] and [r.tolist() for r in rows] == [[0]]
    assert [c["expect"] for c in G["replacement"]][5:] == ["table6/helloworld/234", "table7__2.71828__2023-08-31"]


def test_restatement_layout(oracle):
    """what the golden cases do not reach: names outside the schema, repeated names, values the row does not have, first-appearance order"""
    schema = abi.Schema.of([["b", "utf8", False], ["a", "int64", False], ["gone", "any", False], ["gone2", "int32", False]])
    rows = [[["int64", 2], ["string", "x"]], [["int64", 1], ["string", "y"]], [["int64", 2], ["string", "x"]], [["nil", None], ["string", "x"]]]
    b = abi.batch_from_rows(schema, ["a", "b"], rows, "db", "t")
    b.schema = schema
    cfg = {"columns": ["a", "nosuch", "b", "a", "gone", "gone2"], "splitter": ""}
    assert ref.table_names(oracle, cfg, b) == [b"t/2/x/2/null/<nil>", b"t/1/y/1/null/<nil>", b"t/2/x/2/null/<nil>", b"t/<nil>/x/<nil>/null/<nil>"]
    names, ids, groups = ref.split(oracle, cfg, b)
    assert names == [b"t/2/x/2/null/<nil>", b"t/1/y/1/null/<nil>", b"t/<nil>/x/<nil>/null/<nil>"] and ids.tolist() == [0, 1, 0, 2]
    assert [g.tolist() for g in groups] == [[0, 2], [1], [3]]
    b.table_name = ""
    assert ref.table_names(oracle, {"columns": ["b", "a"], "splitter": "é"}, b)[:2] == ["xé2".encode(), "yé1".encode()]
    assert ref.table_names(oracle, {"columns": ["nosuch"]}, b) == [b""] * 4
    # two value tuples, one name
    rows = [[["string", "a/b"], ["string", "c"]], [["string", "a"], ["string", "b/c"]]]
    b = abi.batch_from_rows(abi.Schema.of([["p", "utf8", False], ["q", "utf8", False]]), ["p", "q"], rows, "db", "t")
    assert ref.split(oracle, {"columns": ["p", "q"]}, b)[0] == [b"t/a/b/c"]


def test_type_description_and_registry():
    t = lib.Transformer(T, {"splitter": "_"})
    assert t.type() == T
    assert t.description() == "Table splitter for tables=(include: , exclude: ); columns=(); splitter=_"
    # `columns=(...)` is built from the tables' ExcludeRegexp (joined with ","), not from `columns`; the splitter prints as configured (empty, not "/")
    t = lib.Transformer(T, {"columns": ["a", "b"], "tables": {"includeTables": ["^i1$", "^i2$"], "excludeTables": ["^e1$", "^e2$"]}})
    assert t.description() == "Table splitter for tables=(include: ^i1$|^i2$, exclude: ^e1$|^e2$); columns=(^e1$,^e2$); splitter="
    # trimStr cuts only where the cut form is shorter than the value: 150 characters are cut to 100 + "... and 50 more", 101 stay (114 > 101)
    long150, long101 = "^" + "a" * 149, "^" + "b" * 100
    t = lib.Transformer(T, {"tables": {"includeTables": [long150], "excludeTables": [long101]}, "splitter": "::"})
    assert t.description() == "Table splitter for tables=(include: %s... and 50 more, exclude: %s); columns=(%s); splitter=::" % (long150[:100], long101, long101)
    assert T not in lib.registry() and len(lib.registry()) == 10


def test_suitable_and_result_schema():
    assert len(G["suitable"]) == 8
    empty = abi.Schema.of([])
    for s in G["suitable"]:
        t = lib.Transformer(T, {"tables": {"includeTables": s["include"], "excludeTables": s["exclude"]}})
        assert t.suitable(s["ns"], s["table"], empty) == s["expect"], s
    schema = abi.Schema.of([["id", "int64", True], ["s", "utf8", False, "", "pg:text"], ["d", "date", False]])
    t = lib.Transformer(T, {"columns": ["s", "d"], "splitter": "/"})
    assert t.suitable("db", "anything", schema)
    rs = t.result_schema(schema)
    assert [[c.name, c.dtype, c.key, c.original_type] for c in rs.cols] == [[c.name, c.dtype, c.key, c.original_type] for c in schema.cols]


def test_legacy_lf_is_refused_by_name():
    with pytest.raises(lib.TfgpuError) as ei:
        lib.Transformer(T, {"columns": ["a"], "useLegacyLf": True})
    assert ei.value.code == lib.ERR_UNSUPPORTED and "useLegacyLf" in str(ei.value) and T in str(ei.value)
    lib.Transformer(T, {"columns": ["a"], "useLegacyLf": False})


def test_where_a_splitter_may_not_go():
    L = lib.load()
    split, flt = lib.Transformer(T, {"columns": ["a"]}), lib.Transformer("filter_rows", {"filter": "a > 1"})
    # tfgpu_apply: refused from the plans alone, naming the entry that runs it
    for chain in ([split], [flt, split], [split, flt]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        out, nerr = C.c_void_p(), C.c_int64(0)
        rc = L.tfgpu_apply(arr, len(chain), None, C.byref(out), None, 0, C.byref(nerr))
        assert rc == lib.ERR_UNSUPPORTED and "tfgpu_apply_split" in L.tfgpu_last_error().decode()
    # tfgpu_apply_split: a splitter that is not last, or two of them
    for chain in ([split, flt], [split, split], [flt, split, split]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        out, nerr = C.c_void_p(), C.c_int64(0)
        rc = L.tfgpu_apply_split(arr, len(chain), None, C.byref(out), None, 0, C.byref(nerr))
        assert rc == lib.ERR_UNSUPPORTED and "tfgpu_tablesplit_batch" in L.tfgpu_last_error().decode() and "tfgpu_apply" in L.tfgpu_last_error().decode()
    # tfgpu_transformation_create
    for chain in ([split], [flt, split]):
        arr = (C.c_void_p * len(chain))(*[t._h for t in chain])
        h = C.c_void_p()
        rc = L.tfgpu_transformation_create(arr, len(chain), C.byref(h))
        assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    # tfgpu_transformation_from_config: by its config key, as an extra transformer, and with the key the plan itself refuses
    L.tfgpu_transformation_from_config.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.tfgpu_transformation_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    cfg = {"transformers": [{"filterRows": {"tables": {}, "filter": "id > 1"}}, {"tableSplitterTransformer": {"columns": ["a"], "splitter": "/"}, "transformerId": "t-2"}]}
    rc = L.tfgpu_transformation_from_config(json.dumps(cfg).encode(), None, 0, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    extra = (C.c_void_p * 1)(split._h)
    rc = L.tfgpu_transformation_from_config(json.dumps({"transformers": cfg["transformers"][:1]}).encode(), extra, 1, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and L.tfgpu_last_error().decode().startswith("unable to init: " + T + ": ")
    cfg["transformers"][1]["tableSplitterTransformer"]["useLegacyLf"] = True
    rc = L.tfgpu_transformation_from_config(json.dumps(cfg).encode(), None, 0, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and "unable to init: " + T in L.tfgpu_last_error().decode() and "useLegacyLf" in L.tfgpu_last_error().decode()
    # the chain without it still builds
    assert L.tfgpu_transformation_from_config(json.dumps({"transformers": cfg["transformers"][:1]}).encode(), None, 0, C.byref(h)) == 0
    L.tfgpu_transformation_destroy(h)
