"""The protobuf parser without a GPU: the restatement (tests/protoparse_ref.py) against the reference's own canon texts, and the host half of the C ABI
(tfgpu_proto_parser_create / _create_json / _schema / _info: descriptor set → compiled parser) against the restatement."""
import base64
import json
import os
import struct

import pytest

import protoparse_ref as R
from transferia_amd import abi, lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protoparser", "gotest")
STD = R.std_data_types_fds()
STD_DESC = R.parse_fds(STD).by_full[".StdDataTypesMsg"]
STD_FIELDS = [f.name for f in STD_DESC.fields]

# proto_parser_test.go's stdDataTypesFilled / stdDataTypesEmpty, restated as data (proto.Marshal writes fields in number order)
FILLED = R.encode(STD_DESC, [
    ("doubleField", 1.11), ("floatField", 2.2), ("int32Field", 2), ("int64Field", 3), ("uint32Field", 4), ("uint64Field", 5), ("sint32Field", 6), ("sint64Field", 7),
    ("fixed32Field", 8), ("fixed64Field", 9), ("sfixed32Field", 10), ("sfixed64Field", 11), ("boolField", True), ("stringField", "string"), ("bytesField", b"bytes"),
    ("mapField", {"key1": 23, "key2": 12}), ("repeatedField", ["1", "2", "3"]), ("msgField", [("stringField", "stringField"), ("int32Field", 2), ("enumField", 1)]),
    ("structField", [("fields", {"key1": [("string_value", "value1")], "key2": [("number_value", 2.2)]})]), ("one", [("int32Field", 52)])])
EMPTY = R.encode(STD_DESC, [("doubleField", 2.223)])


def metrika_desc(name="metrika_hit_log.desc"):
    with open(os.path.join(GOLD, "metrika-data", name), "rb") as f:
        return f.read()


def canon(name):
    with open(os.path.join(GOLD, "canondata", "TestCheckNotFillEmptyFields_%s.json" % name)) as f:
        return f.read()


def schema_of(par):
    return [(c.name, c.dtype, c.key, c.required) for c in par.schema().cols]


# ---- the restatement against the reference's canon data --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,required,nfe,value", [("not_fill_empty_fields", True, True, FILLED), ("fill_empty_fields", True, False, FILLED),
                                                     ("not_fill_column_with_nil_value", False, True, EMPTY)])
def test_canon_items(name, required, nfe, value):
    """TestCheckNotFillEmptyFields' three items, structField and `one` included (which only the restatement decodes)"""
    text = canon(name)
    item = json.loads(text)
    p = R.Parser(STD, "StdDataTypesMsg", include_columns=[(n, required) for n in STD_FIELDS], not_fill_empty_fields=nfe)
    m = R.unmarshal(p.desc, value)
    vals, err, _ = p.make_values(m)
    assert err is None and item["columnnames"] == [s[0] for s in p.schema]
    got = "[" + ",".join(R.go_json(v, html=True) for v in vals) + "]"
    a = text.index('"columnvalues":') + len('"columnvalues":')
    assert text[a:text.index(',"table_schema"')] == got
    assert [(c["name"], c["type"], c["key"], c["required"]) for c in item["table_schema"]] == p.schema


def test_go_json_floats():
    f32 = lambda x: R.F32(struct.unpack("<f", struct.pack("<f", x))[0])  # noqa: E731
    assert [R.go_json(v) for v in (0.1, 1e21, 1e20, 1e-6, 1e-7, 123456789.125, -2.5, f32(2.2), f32(0.1), f32(1e21), f32(16777216.0), f32(1e-7))] == \
        ["0.1", "1e+21", "100000000000000000000", "0.000001", "1e-7", "123456789.125", "-2.5", "2.2", "0.1", "1e+21", "16777216", "1e-7"]


def test_protoseq_scanner():
    F, M = R.protoseq_frame, R.PROTOSEQ_MAGIC
    assert R.protoseq_scan(F(b"ab") + F(b"")) == [(4, 2, None), (42, 0, None)]
    assert R.protoseq_scan(F(b"ab") + b"\x01\x02") == [(4, 2, None), (38, 2, "last incomplete protoseq message: expected size len = 4, got size len = 2")]
    assert R.protoseq_scan(F(b"abcd")[:-1]) == [(0, 39, "last incomplete protoseq message")]
    big = (R.PROTOSEQ_MAX_RECORD + 1).to_bytes(4, "little")
    assert R.protoseq_scan(big + b"xy" + M + F(b"q")) == [(4, 2, "frame corrupted"), (42, 1, None)]
    assert R.protoseq_scan(big + b"xy") == []  # no magic: the rest is dropped silently
    assert R.protoseq_scan(F(b"ab")[:-1] + b"\x00" + F(b"cd")) == [(4, 2 + 32 + 4 + 2, "frame corrupted")]


# ---- the C ABI's host half -----------------------------------------------------------------------------------------------------------------------------------
def test_extract_message_across_two_files():
    """extract_message.desc: MessageOne (1.proto) holds MessageTwo (2.proto) as a field, a oneof member and a repeated field"""
    with open(os.path.join(GOLD, "extract_message.desc"), "rb") as f:
        desc = f.read()
    ref = R.Parser(desc, "MessageOne")
    par = lib.ProtoParser.create(desc, "MessageOne")
    assert schema_of(par) == ref.schema and dict((s[0], s[1]) for s in ref.schema)["message_two"] == "any"
    code, why, name, ncol = par.info()
    assert (code, why, name, ncol) == (abi.ROW_OK, "", "MessageOne", 7)
    assert schema_of(lib.ProtoParser.create(desc, "MessageTwo")) == R.Parser(desc, "MessageTwo").schema
    with pytest.raises(lib.TfgpuError) as e:
        lib.ProtoParser.create(desc, "EnumOne")
    assert e.value.code == lib.ERR_CONFIG and "message with provided name 'EnumOne' not found" in str(e.value)


def test_message_defined_by_two_files_is_refused_by_name():
    two = R.fds([R.file_("a.proto", "a", messages=[R.msg("M", [R.field("x", 1, "int32")])]), R.file_("b.proto", "b", messages=[R.msg("M", [R.field("y", 1, "string")])])])
    with pytest.raises(lib.TfgpuError) as e:
        lib.ProtoParser.create(two, "M")
    assert e.value.code == lib.ERR_UNSUPPORTED and "'M' is defined by more than one file" in str(e.value)
    assert R.Parser(two, "M").defined_in == ["a.proto", "b.proto"]


def test_column_splits():
    """TestPrepareFieldDescriptors' splits as a config reaches them: only included fields, included + `_lb_extra_`, no column at all.  (Its fourth split,
    `_lb_extra_` columns alone, is no config's: an empty IncludeColumns means every field.)"""
    a = lib.ProtoParser.create(STD, "StdDataTypesMsg", include_columns=[("doubleField", False), ("stringField", False), ("int32Field", False)])
    assert schema_of(a) == [("doubleField", "double", False, False), ("stringField", "utf8", False, False), ("int32Field", "int32", False, False)]
    cfg = dict(include_columns=[("doubleField", False), ("stringField", False)], add_system_columns=True, skip_dedup_keys=True)
    b, rb = lib.ProtoParser.create(STD, "StdDataTypesMsg", **cfg), R.Parser(STD, "StdDataTypesMsg", **cfg)
    names = [s[0] for s in schema_of(b)]
    assert schema_of(b) == rb.schema and names[:2] == ["doubleField", "stringField"] and names[2:4] == ["_lb_extra_floatField", "_lb_extra_int32Field"]
    assert names[-2:] == ["_lb_ctime", "_lb_wtime"] and len(names) == 2 + 18 + 2 and [f.name for f in rb.extra] == [n[len("_lb_extra_"):] for n in names[2:-2]]
    none = R.fds([R.file_("e.proto", messages=[R.msg("Nothing")])])
    assert schema_of(lib.ProtoParser.create(none, "Nothing")) == [] == R.Parser(none, "Nothing").schema


S_IDX, S_OFF, S_PART, CT, WT = "_idx", "_offset", "_partition", "_lb_ctime", "_lb_wtime"
REQUIRED_SET_CASES = [  # makeRequiredSetTestCases: (config, required columns, key columns)
    (dict(), [], []),
    (dict(primary_keys=["doubleField", "floatField"]), ["doubleField", "floatField"], ["doubleField", "floatField"]),
    (dict(primary_keys=["doubleField", "floatField"], null_keys_allowed=True), [], ["doubleField", "floatField"]),
    (dict(primary_keys=["doubleField", "floatField"], include_columns=[("doubleField", True)], null_keys_allowed=True), ["doubleField"], ["doubleField", "floatField"]),
    (dict(primary_keys=["doubleField", "floatField"], include_columns=[("doubleField", False)], null_keys_allowed=True), [], ["doubleField", "floatField"]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", False), ("doubleField", False)], null_keys_allowed=True), [], ["doubleField"]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True), ("doubleField", False)], null_keys_allowed=True), ["floatField"], ["doubleField"]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True), ("doubleField", True)]), ["floatField", "doubleField"], ["doubleField"]),
    (dict(primary_keys=["doubleField"], add_synthetic_keys=True, null_keys_allowed=True), [], ["doubleField", S_IDX, S_OFF, S_PART]),
    (dict(primary_keys=["doubleField"], add_synthetic_keys=True), ["doubleField", S_IDX, S_OFF, S_PART], ["doubleField", S_IDX, S_OFF, S_PART]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True)], add_synthetic_keys=True),
     ["doubleField", "floatField", S_IDX, S_OFF, S_PART], ["doubleField", S_IDX, S_OFF, S_PART]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True)], add_synthetic_keys=True, add_system_columns=True, skip_dedup_keys=True),
     ["doubleField", "floatField", S_IDX, S_OFF, S_PART], ["doubleField", S_IDX, S_OFF, S_PART]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True)], add_synthetic_keys=True, add_system_columns=True),
     ["doubleField", "floatField", S_IDX, S_OFF, S_PART, CT, WT], ["doubleField", S_IDX, S_OFF, S_PART, CT, WT]),
    (dict(primary_keys=["doubleField"], include_columns=[("floatField", True)], add_synthetic_keys=True, add_system_columns=True, null_keys_allowed=True),
     ["floatField"], ["doubleField", S_IDX, S_OFF, S_PART, CT, WT]),
]


@pytest.mark.parametrize("case", range(len(REQUIRED_SET_CASES)))
def test_required_and_keys_set(case):
    """TestDoStdDataTypesRequiredAndPKSet: one item, nothing unparsed, and exactly these columns Required / PrimaryKey"""
    cfg, required, keys = REQUIRED_SET_CASES[case]
    ref, par = R.Parser(STD, "StdDataTypesMsg", **cfg), lib.ProtoParser.create(STD, "StdDataTypesMsg", **cfg)
    assert schema_of(par) == ref.schema
    assert {s[0] for s in ref.schema if s[3]} == set(required) and {s[0] for s in ref.schema if s[2]} == set(keys)
    rows, un, base = ref.do_batch([FILLED])
    assert len(rows) == 1 and not un and base == [0, 1]


def test_required_not_set():
    """TestDoRequiredNotSet: msgField as a key of a message that does not hold it: exactly one unparsed item"""
    ref = R.Parser(STD, "StdDataTypesMsg", primary_keys=["msgField"])
    rows, un, base = ref.do_batch([EMPTY])
    assert not rows and [(u[2], u[3], u[4]) for u in un] == [(1, "required", "msgField")]
    vals, err, col = ref.make_values(R.unmarshal(ref.desc, EMPTY))
    assert err == "required field 'msgField' was not populated"


def test_config_error_texts():
    def err(**cfg):
        kw = dict(desc_file=STD, message_name="StdDataTypesMsg")
        kw.update(cfg)
        with pytest.raises(lib.TfgpuError) as e:
            lib.ProtoParser.create(**kw)
        try:
            R.Parser(kw["desc_file"], kw["message_name"], **{k: v for k, v in kw.items() if k not in ("desc_file", "message_name", "desc_resource_name")})
            ref = None
        except (R.ConfigError, R.UnmarshalError) as x:
            ref = str(x)
        return e.value.code, str(e.value).split(": ", 1)[1], ref

    for cfg, text in [
        (dict(desc_file=b""), "desc file and desc resource are both empty"),
        (dict(message_name="Nope"), "SetDescriptors error: error extracting message descriptor from desc file: message with provided name 'Nope' not found"),
        (dict(package_type="PackageTypeRepeated"), "SetDescriptors error: can't extract embedded repeated message descriptor while provided package type is repeated"),
        (dict(include_columns=[("int32Field", False), ("int32Field", True)]), "duplicate column name 'int32Field'"),
        (dict(primary_keys=["nope"]), "given key field 'nope' not found in proto message desc"),
        (dict(primary_keys=["int32Field"], include_columns=[("int32Field", False)]), "key param 'int32Field' must be set as required"),
        (dict(include_columns=[("nope", False)]), "requested column nope not found in proto descriptor"),
    ]:
        code, got, ref = err(**cfg)
        assert (code, got) == (lib.ERR_CONFIG, text) and ref == text, cfg
    code, got, _ = err(desc_file=b"\x0a\x05abc")
    assert code == lib.ERR_CONFIG and got.startswith("SetDescriptors error: error extracting message descriptor from desc file: error unmarshaling proto desc file content: ")
    code, got, _ = err(desc_resource_name="res")
    assert code == lib.ERR_UNSUPPORTED and "DescResourceName" in got
    # a wrapper needs exactly one field, and that field a repeated message
    assert schema_of(lib.ProtoParser.create(STD, "StdDataTypesMsgList", "PackageTypeRepeated")) == R.Parser(STD, "StdDataTypesMsgList", "PackageTypeRepeated").schema


@pytest.mark.parametrize("desc_name,message,nfields", [("metrika_hit_log.desc", "CloudTransferHit", 92), ("metrika_hit_protoseq.desc", "CloudTransferHit", 116)])
def test_metrika_schema_under_both_configs(desc_name, message, nfields):
    desc = metrika_desc(desc_name)
    common = dict(DescFile=base64.b64encode(desc).decode(), DescResourceName="", MessageName="CloudTransferHitList", IncludeColumns=None, PrimaryKeys=None,
                  PackageType="PackageTypeRepeated", NullKeysAllowed=False, NotFillEmptyFields=False)
    par = lib.ProtoParser.from_config(common)  # json.Marshal(ParserConfigProtoCommon)
    ref = R.Parser(desc, "CloudTransferHitList", "PackageTypeRepeated")
    assert schema_of(par) == ref.schema and len(ref.schema) == nfields and par.info() == (abi.ROW_OK, "", ref.desc.full, nfields) and ref.desc.name == message
    names = [f.name for f in ref.desc.fields]
    for keys in ([], names[1:3]):
        for sys_cols in (False, True):
            for synth in (False, True):
                for nka in (False, True):
                    inc = [dict(Name=names[3], Required=True), dict(Name=names[1], Required=True), dict(Name=names[4], Required=False)] if keys else None
                    lb = dict(common, MessageName=message, PackageType="PackageTypeProtoseq", IncludeColumns=inc, PrimaryKeys=keys or None, NullKeysAllowed=nka,
                              AddSystemColumns=sys_cols, SkipDedupKeys=synth and sys_cols, AddSyntheticKeys=synth)
                    ref = R.Parser(desc, message, "PackageTypeProtoseq", include_columns=[(c["Name"], c["Required"]) for c in inc or []], primary_keys=keys,
                                   null_keys_allowed=nka, add_system_columns=sys_cols, skip_dedup_keys=synth and sys_cols, add_synthetic_keys=synth)
                    par = lib.ProtoParser.from_config(json.dumps(lb))
                    assert schema_of(par) == ref.schema, lb
                    assert par.info()[0] == abi.ROW_OK and par.info()[3] == len(ref.schema)


def test_info_names_each_refused_construct():
    def why(files, message="M", **cfg):
        par = lib.ProtoParser.create(R.fds(files), message, **cfg)
        code, text, _, _ = par.info()
        return code, text

    f, m, L = R.field, R.msg, R.LABEL_REPEATED
    leaf = m("Leaf", [f("x", 1, "int32")])
    for fields, extra, needle in [
        ([f("c", 1, "message", type_name=".Mid")], [m("Mid", [f("l", 1, "message", type_name=".Leaf")]), leaf], "nesting deeper than one level (Mid.l)"),
        ([f("c", 1, "message", type_name=".Mid")], [m("Mid", [f("a", 1, "int32", oneof_index=0), f("b", 2, "string", oneof_index=0)], oneofs=["o"])], "a oneof inside the nested message Mid"),
        ([f("c", 1, "message", type_name=".Mid")], [m("Mid", [f("r", 1, "int32", L)])], "a repeated or map field inside the nested message Mid"),
        ([f("c", 1, "group", type_name=".Leaf")], [leaf], "a group field"),
        ([f("c", 1, "message", type_name=".google.protobuf.Struct")], [], "google.protobuf.Struct"),
    ]:
        code, text = why([R.struct_file(), R.file_("m.proto", messages=[m("M", fields)] + extra)])
        assert code == abi.ROW_HOST_FALLBACK and text == "column c: " + needle, text
    for key, val, tn, needle in [("int32", "int32", "", "a map keyed by other than a string"), ("string", "message", ".Leaf", "a map with message values")]:
        mf, me = R.map_field("M", "c", 1, key, val, tn)
        assert why([R.file_("m.proto", messages=[m("M", [mf], nested=[me]), leaf])]) == (abi.ROW_HOST_FALLBACK, "column c: " + needle)
    assert why([R.file_("m.proto", syntax="proto2", messages=[m("M", [f("x", 1, "int32")])])]) == (abi.ROW_HOST_FALLBACK, "a proto2 file defines M")
    # the reference's own StdDataTypesMsg: structField and `one` are outside the subset; IncludeColumns that leave them out keep the device
    par = lib.ProtoParser.create(STD, "StdDataTypesMsg")
    assert par.info()[0] == abi.ROW_HOST_FALLBACK and par.info()[1] == "column structField: google.protobuf.Struct"
    par = lib.ProtoParser.create(STD, "StdDataTypesMsg", include_columns=[(n, False) for n in STD_FIELDS if n not in ("structField", "one")])
    assert par.info()[:2] == (abi.ROW_OK, "")


# ---- the restatement's decode against the protobuf library -----------------------------------------------------------------------------------------------------
def test_decode_against_the_protobuf_library():
    pytest.importorskip("google.protobuf")
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    fds_bytes = R.device_cases_fds()
    s = descriptor_pb2.FileDescriptorSet()
    s.ParseFromString(fds_bytes)
    pool = descriptor_pool.DescriptorPool()
    for fd in s.file:
        pool.Add(fd)
    cls = message_factory.GetMessageClass(pool.FindMessageTypeByName("t.Ev"))
    ev = R.parse_fds(fds_bytes).by_full[".t.Ev"]

    def tree(m):  # the restatement's message as {name: value} of the fields that are set, as ListFields gives them
        out = {}
        for f in m.desc.fields:
            if not m.has(f):
                continue
            v = m.get(f)
            conv = (lambda x: tree(x)) if f.type == R.T_MESSAGE and not f.is_map else (lambda x: x)
            if f.is_map:
                out[f.name] = dict(v)
            elif f.label == R.LABEL_REPEATED:
                out[f.name] = [conv(x) for x in v]
            else:
                out[f.name] = conv(v)
        return out

    def lib_tree(m):
        out = {}
        for fd, v in m.ListFields():
            if fd.message_type is not None and fd.message_type.GetOptions().map_entry:
                out[fd.name] = dict(v)
            elif fd.is_repeated:
                out[fd.name] = [lib_tree(x) if fd.message_type is not None else x for x in v]
            else:
                out[fd.name] = lib_tree(v) if fd.message_type is not None else v
        return out

    cases = [
        R.encode(ev, [("d", 1.5), ("i32", -7), ("s", "é"), ("by", b"\xff"), ("en", 3), ("oi", 0), ("ua", 1), ("ub", "z"), ("ri", [1, -2, 3]), ("rs", ["a", ""]),
                      ("rz", [-1, 2**40]), ("rx", [1, 2**64 - 1]), ("m", [("s", "q"), ("i", 5), ("oi", 0)]), ("rm", [[("i", 1)], []]), ("mi", {"a": 1, "b": 2}),
                      ("ms", {"k": "v"}), ("em", []), ("big", 9)], packed=True),
        R.encode(ev, [("ri", [1, 2]), ("rf", [0.5]), ("re", [1, 0])], packed=False) + R.encode(ev, [("ri", [3]), ("rf", [1.5, 2.5])], packed=True),   # packed and unpacked runs mix
        R.encode(ev, [("mi", {"a": 1})]) + R.encode(ev, [("mi", {"b": 2})]) + R.encode(ev, [("mi", {"a": 3})]),   # duplicate map keys: the last one wins
        R.encode(ev, [("m", [("s", "a"), ("i", 1)])]) + R.encode(ev, [("m", [("i", 2)])]),    # occurrences of a message field merge
        R.encode(ev, [("ub", "x")]) + R.encode(ev, [("ua", 0)]),                              # the last oneof member stays, set to its zero value
        R.enc_varint(3, (1 << 40) + 5) + R.enc_varint(13, 7),                                 # int32 truncates, bool is != 0
        R.enc_bytes(99, b"\xff") + R.encode(ev, [("i64", -1)]),                               # unknown fields are skipped
        b"",
    ]
    for data in cases:
        want = cls()
        want.ParseFromString(data)
        assert tree(R.unmarshal(ev, data)) == lib_tree(want), data
    for bad in [R.enc_bytes(14, b"\xc0\xaf"), R.enc_bytes(22, b"\xff"), R.enc_bytes(28, R.enc_bytes(1, b"\xed\xa0\x80")), R.enc_bytes(31, R.enc_bytes(2, b"\x80")),
                R.tag(3, 0), R.enc_bytes(21, b"\x80"), R.tag(14, 2) + b"\x05ab", R.enc_bytes(27, b"1234567")]:
        with pytest.raises(Exception):
            cls().ParseFromString(bad)   # invalid UTF-8 in a proto3 string and cut wire forms: both must fail
        with pytest.raises(R.UnmarshalError):
            R.unmarshal(ev, bad)
