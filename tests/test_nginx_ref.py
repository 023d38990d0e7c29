"""nginx access-log ingest without a GPU: the plain-Python restatement (tests/nginx_ref.py) and the library's host ABI
(tfgpu_nginx_format_*, tfgpu_nginx_resolve_schema) both reproduce the cases of the reference's own tests
(tests/golden/nginx_format.json, transcribed from nginx_format_test.go and data_error_matrix_test.go)."""
import pytest

import nginx_ref as ref
from transferia_amd import abi, lib
from util import golden

CASES = golden("nginx_format.json")["cases"]


def _of(kind):
    return [c for c in CASES if c["kind"] == kind]


def _id(c):
    return c["cite"].rsplit("/", 1)[-1] + ("-" + c["name"] if "name" in c else "")


# ---- the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _of("tokenize"), ids=_id)
def test_ref_tokenize(c):
    assert ref.tokenize_format(c["format"].encode()) == [(bool(v), s.encode()) for v, s in c["tokens"]]


@pytest.mark.parametrize("c", _of("compile"), ids=_id)
def test_ref_compile(c):
    if c["error"]:
        with pytest.raises(ValueError):
            ref.compile_format(c["format"].encode())
        return
    f = ref.compile_format(c["format"].encode())
    if "fields" in c:
        assert [x.decode() for x in f.fields] == c["fields"]
    if "nfields" in c:
        assert len(f.fields) == c["nfields"]
    assert [(s.name, s.dtype, s.path, s.original_type) for s in f.schema()] == [(x.decode(), "utf8", str(i), "nginx:utf8") for i, x in enumerate(f.fields)]


def _check_entry(c, pe):
    if c.get("error"):
        assert pe is None
        return
    assert pe is not None
    values, consumed = pe
    if "values" in c:
        assert values == [v.encode() for v in c["values"]]
    if "nvalues" in c:
        assert len(values) == c["nvalues"]
    for k, v in c.get("values_at", {}).items():
        assert values[int(k)] == v.encode(), k
    if "consumed" in c:
        assert consumed == c["consumed"]
    if c.get("consumed_less_than_len"):
        assert consumed < len(c["input"].encode())


@pytest.mark.parametrize("c", _of("parse_entry") + _of("unexpected"), ids=_id)
def test_ref_parse_entry(c):
    f = ref.compile_format(c["format"].encode())
    pe = ref.parse_entry(f, c["input"].encode())
    _check_entry(c, pe)
    if c["kind"] == "unexpected":
        assert ref.has_unexpected_fields(c["input"].encode(), pe[1]) == c["error_with_error_behavior"]
    if "dash_fields" in c:
        names = [x.decode() for x in f.fields]
        assert all(pe[0][names.index(n)] == b"-" for n in c["dash_fields"])


@pytest.mark.parametrize("c", _of("match_literal") + _of("find_delimiter"), ids=_id)
def test_ref_literals(c):
    if c["kind"] == "match_literal":
        assert ref.match_literal(c["input"].encode(), c["literal"].encode()) == c["result"]
    else:
        assert ref.find_delimiter(c["input"].encode(), c["delimiter"].encode()) == c["result"]


def _typed_chunk(oracle, c):
    f = ref.compile_format(b'"$v"')
    schema = abi.Schema([abi.ColSchema("v", c["dtype"], False, "0")])
    return ref.parse_chunk(oracle, f, schema, b'"' + c["value"].encode() + b'"\n')


@pytest.mark.parametrize("c", _of("convert"), ids=lambda c: "%s-%s" % (c["dtype"], c["value"]))
def test_ref_convert(oracle, c):
    """convertNginxValue, seen through a one-column line; a value that stays a string goes on through Strictify"""
    r = _typed_chunk(oracle, c)
    if c["result"] == "error":
        assert r.errors == [(1, "CAST", 0)] and not r.rows
    elif c["result"] == "nil":
        assert r.rows == [[("nil", None)]] and not r.errors
    elif c["result"] == "time":
        assert r.rows == [[("time", (c["unix"], 0))]]
    else:
        want = {"int64": ("int64", 200), "double": ("jsonnum", b"0.042")}[c["dtype"]]
        assert r.rows == [[want]]


@pytest.mark.parametrize("c", _of("reader_line"), ids=_id)
def test_ref_reader_lines(oracle, c):
    f = ref.compile_format(c["format"].encode())
    r = ref.parse_chunk(oracle, f, ref.resolve_schema(f), c["body"].encode())
    assert (r.errors == [(1, "NGINX_FORMAT", -1)]) == c["error"] and r.consumed == len(c["body"]) and r.next_row_number == 2


def test_ref_line_loop(oracle):
    f = ref.compile_format(b"$a $b")
    data = b"1 2\n\n  \t\r\n\xc2\xa0\xe2\x80\x83\n3 4\r\nbad\n5 6"
    schema = ref.resolve_schema(f)
    r = ref.parse_chunk(oracle, f, schema, data, file_name="f.log", row_number_base=10)
    assert r.consumed == len(data) - 3 and r.next_row_number == 13 and r.errors == [(12, "NGINX_FORMAT", -1)]
    assert r.rows == [[("string", b"f.log"), ("uint64", 10), ("string", b"1"), ("string", b"2")], [("string", b"f.log"), ("uint64", 11), ("string", b"3"), ("string", b"4")]]
    r = ref.parse_chunk(oracle, f, schema, data, row_number_base=10, last_chunk=True, hide_system_cols=True)
    assert r.consumed == len(data) and r.next_row_number == 14 and r.rows[-1] == [("nil", None), ("nil", None), ("string", b"5"), ("string", b"6")]
    r = ref.parse_chunk(oracle, f, schema, b"1 2")
    assert r.consumed == 0 and r.next_row_number == 1 and not r.rows and not r.errors


# ---- the library's host ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _of("tokenize"), ids=_id)
def test_abi_tokens(c):
    assert lib.NginxFormat(c["format"]).tokens == [(bool(v), s.encode()) for v, s in c["tokens"]]


@pytest.mark.parametrize("c", _of("compile") + _of("parse_entry") + _of("reader_line"), ids=_id)
def test_abi_compile_matches_ref(c):
    if c.get("kind") == "compile" and c["error"]:
        with pytest.raises(lib.TfgpuError) as e:
            lib.NginxFormat(c["format"])
        assert e.value.code == lib.ERR_CONFIG
        return
    f, r = lib.NginxFormat(c["format"]), ref.compile_format(c["format"].encode())
    assert f.tokens == r.tokens and f.fields == [x.decode() for x in r.fields]
    if "fields" in c:
        assert f.fields == c["fields"]
    if "nfields" in c:
        assert len(f.fields) == c["nfields"]


def test_abi_collapse_and_dollar_edges():
    for fmt in ["$a \t\n\t $b", "$a\n\n$b", "$a \n \n $b", "  $a$b \"x\" $ $$c $-d \xc2\xa0", "\xe2\x80\x83$a\xe3\x80\x80", "$a\t \n"]:
        assert lib.NginxFormat(fmt).tokens == ref.tokenize_format(fmt.encode()), fmt


def _schema_tuple(s):
    return [(c.name, c.dtype, c.key, c.path, c.original_type) for c in s.cols]


def test_abi_resolve_schema_empty_output_schema():
    f, r = lib.NginxFormat('"$host" "$status" "$host"'), ref.compile_format(b'"$host" "$status" "$host"')
    got = f.resolve_schema()
    assert _schema_tuple(got) == _schema_tuple(ref.resolve_schema(r))
    assert _schema_tuple(got) == [("__file_name", "utf8", True, "", ""), ("__row_index", "uint64", True, "", ""), ("host", "utf8", False, "0", "nginx:utf8"),
                                  ("status", "utf8", False, "1", "nginx:utf8"), ("host_2", "utf8", False, "2", "nginx:utf8")]
    assert _schema_tuple(f.resolve_schema(abi.Schema([]), hide_system_cols=True)) == _schema_tuple(got)[2:]


@pytest.mark.parametrize("c", _of("resolve_names"), ids=_id)
def test_abi_resolve_schema_name_matching(c):
    f, r = lib.NginxFormat(c["format"]), ref.compile_format(c["format"].encode())
    out = abi.Schema([abi.ColSchema(n, "utf8") for n in c["columns"]])
    got = f.resolve_schema(out, hide_system_cols=True)
    assert _schema_tuple(got) == _schema_tuple(ref.resolve_schema(r, out, True))
    assert [(x.name, x.path) for x in got.cols] == [(n, p) for n, p in zip(c["columns"], c["paths"]) if p is not None]  # an unknown column is dropped


def test_abi_resolve_schema_keys_types_and_paths():
    f, r = lib.NginxFormat("$remote_addr [$time_local] $status"), ref.compile_format(b"$remote_addr [$time_local] $status")
    out = abi.Schema([abi.ColSchema("status", "int32", True), abi.ColSchema("when", "datetime", False, "1"), abi.ColSchema("gone", "utf8"),
                      abi.ColSchema("remote_addr", "utf8", False, "", "my:type"), abi.ColSchema("far", "boolean", False, "99")])
    for hide in (False, True):
        got = f.resolve_schema(out, hide_system_cols=hide)
        assert _schema_tuple(got) == _schema_tuple(ref.resolve_schema(r, out, hide))
    got = f.resolve_schema(out)
    assert _schema_tuple(got) == [("__file_name", "utf8", False, "", ""), ("__row_index", "uint64", False, "", ""), ("status", "int32", True, "2", "nginx:int32"),
                                  ("when", "datetime", False, "1", "nginx:datetime"), ("remote_addr", "utf8", False, "0", "my:type"), ("far", "boolean", False, "99", "nginx:boolean")]


def test_abi_rowerr_names():
    assert abi.ROWERR[abi.ROW_NGINX_FORMAT] == "NGINX_FORMAT" and abi.ROWERR[abi.ROW_NGINX_EXTRA] == "NGINX_EXTRA"


def test_nginx_parse_needs_a_device():
    import ctypes
    n = ctypes.c_int(0)
    if lib.load().tfgpu_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    f = lib.NginxFormat("$a $b")
    with pytest.raises(lib.TfgpuError) as e:
        lib.nginx_parse(f, lib.nginx_options(), f.resolve_schema(), b"1 2\n")
    assert e.value.code == lib.ERR_DEVICE
