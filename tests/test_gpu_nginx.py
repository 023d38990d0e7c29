"""Parity of the HIP nginx access-log ingest (tfgpu_nginx_parse: line index, token walk, cell conversion, compaction) with the
plain-Python restatement of the reference's reader (tests/nginx_ref.py, typed by oracle.strictify).  Needs an MI355X."""
import random

import pytest

import nginx_ref as ref
from transferia_amd import abi
from util import golden

pytestmark = pytest.mark.gpu

CASES = golden("nginx_format.json")["cases"]
CDN = next(c for c in CASES if c.get("name") == "cdn")
CDN_DASH = next(c for c in CASES if c.get("name") == "cdn_dash")
COMBINED = '$remote_addr - $remote_user [$time_local] "$request" $status $body_bytes_sent "$http_referer" "$http_user_agent"'
QUOTED = '"$remote_addr" "-" "$remote_user" "[$time_local]" "$request" "$status" "$body_bytes_sent" "$request_time" "$upstream_response_time" "$host"'


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def run_both(tf, oracle, fmt: str, schema, data: bytes, ctx="", src=None, **kw):
    """the chunk through the library and through the restatement; everything the call returns is compared, row by row"""
    f, r = tf.NginxFormat(fmt), ref.compile_format(fmt.encode())
    if schema is None:
        schema = f.resolve_schema(hide_system_cols=bool(kw.get("hide_system_cols")))
    want = ref.parse_chunk(oracle, r, schema, data, **kw)
    db, consumed, nxt, errs = tf.nginx_parse(f, tf.nginx_options(**kw), schema, data if src is None else src, max_errors=1 << 16)
    out = db.download()
    assert consumed == want.consumed, ctx
    assert nxt == want.next_row_number, ctx
    assert [(e[0], e[1], e[3]) for e in errs] == want.errors, ctx
    assert not [e for e in want.errors if e[1] == "HOST_FALLBACK"], ctx
    assert [c.name for c in out.cols] == [c.name for c in schema.cols], ctx
    got = abi.batch_rows(out)
    assert len(got) == len(want.rows), (ctx, len(got), len(want.rows))
    for i, (a, b) in enumerate(zip(got, want.rows)):
        assert a == b, (ctx, i, a, b)
    return db, out, want


# ---- 1. the reference's own parseEntry cases, one line per call ----------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] in ("parse_entry", "unexpected")], ids=lambda c: c["cite"].rsplit(":", 1)[-1] + c.get("name", ""))
def test_golden_parse_entry(tf, oracle, c):
    line = c["input"].encode()
    assert b"\n" not in line
    for extra in (False, True):
        db, out, want = run_both(tf, oracle, c["format"], None, line, ctx=c["cite"], last_chunk=True, hide_system_cols=True, unexpected_field_error=extra)
        ok_expected = not c.get("error") and not (extra and c.get("error_with_error_behavior"))
        assert (out.nrows == 1) == ok_expected and len(want.errors) == (0 if ok_expected else 1)
        if not ok_expected:
            assert want.errors[0][1] == ("NGINX_FORMAT" if c.get("error") else "NGINX_EXTRA")
            continue
        vals = [v[1] for v in abi.batch_rows(out)[0]]
        if "values" in c:
            assert [b"-" if v is None else v for v in vals] == [v.encode() for v in c["values"]]
        for k, v in c.get("values_at", {}).items():
            assert vals[int(k)] == (None if v == "-" else v.encode())
    # consumed, seen through the unexpected-field check: a byte appended behind what parseEntry consumed is an extra field
    if not c.get("error") and "consumed" in c and c["consumed"] == len(line):
        _, out, want = run_both(tf, oracle, c["format"], None, line + b" x", last_chunk=True, unexpected_field_error=True)
        last_has_delim = ref.compile_format(c["format"].encode()).tokens[-1][0] is False
        assert out.nrows == (0 if last_has_delim else 1)


@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] == "reader_line"], ids=lambda c: c["cite"].rsplit(":", 1)[-1])
def test_golden_reader_lines(tf, oracle, c):
    _, out, want = run_both(tf, oracle, c["format"], None, c["body"].encode())
    assert out.nrows == 0 and want.errors == [(1, "NGINX_FORMAT", -1)]


# ---- 2. the 47-field CDN line and its dash variant under a typed schema ----------------------------------------------------
def cdn_schema(tf):
    f = tf.NginxFormat(CDN["format"])
    out = abi.Schema([abi.ColSchema("remote_addr", "utf8"), abi.ColSchema("status", "int32", True), abi.ColSchema("body_bytes_sent", "uint64"),
                      abi.ColSchema("request_time", "double"), abi.ColSchema("time_local", "datetime"), abi.ColSchema("day", "date", False, "2"),
                      abi.ColSchema("flag", "boolean", False, "1"), abi.ColSchema("far", "int16", False, "99"), abi.ColSchema("far_text", "utf8", False, "99"),
                      abi.ColSchema("upstream_response_time", "double"), abi.ColSchema("ts", "timestamp", False, "2"), abi.ColSchema("request", "string"),
                      abi.ColSchema("geoip2_region", "utf8"), abi.ColSchema("no_such_field", "utf8")])
    return f.resolve_schema(out)


def test_cdn_lines_typed(tf, oracle):
    schema = cdn_schema(tf)
    assert "no_such_field" not in [c.name for c in schema.cols]
    data = (CDN["input"] + "\n" + CDN_DASH["input"] + "\n").encode()
    # the timestamp column reads "28/Nov/2025:10:04:24 +0000" as a plain string: none of cast's layouts takes it, as oracle.strictify says
    _, out, want = run_both(tf, oracle, CDN["format"], schema, data, file_name="cdn.log")
    assert out.nrows == 0 and [e[1:] for e in want.errors] == [("CAST", [c.name for c in schema.cols].index("ts"))] * 2
    schema = abi.Schema([c for c in schema.cols if c.name != "ts"])
    _, out, want = run_both(tf, oracle, CDN["format"], schema, data, file_name="cdn.log")
    assert out.nrows == 2
    row = dict(zip([c.name for c in schema.cols], want.rows[0]))
    assert row["status"] == ("int32", 403) and row["flag"] == ("nil", None) and row["far"] == ("int16", 0) and row["time_local"] == ("time", (1764324264, 0))
    assert dict(zip([c.name for c in schema.cols], want.rows[1]))["upstream_response_time"] == ("nil", None)


def test_timestamp_column_is_a_plain_string(tf, oracle):
    """the CSV reader's integer shortcut (parse_cell) does not apply: "1700000000" under `timestamp` is what cast.ToTimeE makes of the string"""
    schema = abi.Schema([abi.ColSchema("t", "timestamp", False, "0"), abi.ColSchema("u", "timestamp", False, "1")])
    data = b"1700000000 2024-05-06T07:08:09Z\n2024-05-06 2024-05-06 07:08:09\n- 20240506\n"
    run_both(tf, oracle, "$a $b", schema, data)


# one value per layout of spf13/cast's StringToDate list, in its order (a zone abbreviation is UTC: Go gives any other one a fabricated zero offset) ...
CAST_LAYOUT_CELLS = [
    "2024-05-06", "2024-05-06T07:08:09+02:00", "2024-05-06T07:08:09", "Mon, 06 May 2024 07:08:09 +0200", "Mon, 06 May 2024 07:08:09 UTC",
    "06 May 24 07:08 +0200", "06 May 24 07:08 UTC", "Monday, 06-May-24 07:08:09 UTC", "2024-05-06 07:08:09.123456789 +0000 UTC",
    "2024-05-06T07:08:09+0200", "2024-05-06 07:08:09+0200", "2024-05-06 07:08:09", "Mon May  6 07:08:09 2024", "Mon May  6 07:08:09 UTC 2024",
    "Mon May 06 07:08:09 +0200 2024", "2024-05-06 07:08:09+02:00", "06 May 2024", "2024-05-06 07:08:09 +02:00", "2024-05-06 07:08:09 +0200",
    "7:08PM", "May  6 07:08:09", "May  6 07:08:09.123", "May  6 07:08:09.123456", "May  6 07:08:09.123456789"]
# ... and the shapes the fixed-shape fast path in front of that list (parse_datetime, tf_strictcell.hpp) decides by itself
FAST_PATH_CELLS = [
    "2024-05-06T07:08:09.5", "2024-05-06T07:08:09,5", "2024-05-06 07:08:09.25", "2024-05-06 07:08:09,25", "2024-05-06T07:08:09.1234567891234Z",
    "2024-05-06T07:08:09Z", "2024-05-06T07:08:09.5+02:00", "2024-05-06T07:08:09-05:30", "2024-05-06T07:08:09+25:00", "2024-05-06T7:08:09", "2024-05-06 7:08:09",
    "2023-02-30", "2024-02-29", "2024-05-06T24:00:00", "2024-05-06T07:08:60", "2024-05-06T07:08:09 Z", "2024-05-06 07:08:09 Z", "2024-05-06 07:08:09Z", "-", ""]


def test_timestamp_cells_take_the_fast_path_and_every_cast_layout(tf, oracle):
    """a `timestamp` cell is cast.ToTimeE of the string: the fixed shapes through the fast path, everything else through the 24 layouts, and both
    say what oracle.strictify says (run_both also asserts that no line is a HOST_FALLBACK row of the oracle)"""
    cells = CAST_LAYOUT_CELLS + FAST_PATH_CELLS
    data = "".join('"%s"\n' % c for c in cells).encode()
    _, out, want = run_both(tf, oracle, '"$t"', abi.Schema([abi.ColSchema("t", "timestamp", False, "0")]), data)
    # Go's range rules: an offset hour above 24, a day the month does not have, hour 24, second 60; a space in front of "Z" and "" fit no layout
    bad = ["2024-05-06T07:08:09+25:00", "2023-02-30", "2024-05-06T24:00:00", "2024-05-06T07:08:60", "2024-05-06T07:08:09 Z", "2024-05-06 07:08:09 Z", ""]
    assert want.errors == [(1 + cells.index(c), "CAST", 0) for c in bad] and len(want.rows) == len(cells) - len(bad)
    assert list(want.rows[0]) == [("time", (1714953600, 0))] and list(want.rows[1]) == [("time", (1714972089, 0))], want.rows[:2]


# ---- 3. shapes where the kernel can go wrong ---------------------------------------------------------------------------------
def _line(i, pad=0):
    return b'"10.0.%d.%d" "%d" "%s"' % (i // 256 % 256, i % 256, 200 + i % 300, b"x" * pad + b"/p%d" % i)


SHAPE_FMT = '"$addr" "$status" "$path"'


def shape_schema():
    return abi.Schema([abi.ColSchema("__file_name", "utf8", True), abi.ColSchema("__row_index", "uint64", True), abi.ColSchema("addr", "utf8", False, "0"),
                       abi.ColSchema("status", "int32", False, "1"), abi.ColSchema("path", "string", False, "2"), abi.ColSchema("path_again", "utf8", False, "2"),
                       abi.ColSchema("status_text", "utf8", False, "1")])


def _padded(n):
    """a line of exactly n bytes"""
    base = _line(7)
    return _line(7, n - len(base))


def shape_chunks(tf):
    tile, wg = tf.nginx_tile()
    out = {}
    out["0 lines"] = (b"", {})
    out["0 bytes, last chunk"] = (b"", {"last_chunk": True})  # one empty line, blank: no row, nothing counted
    out["only a blank line"] = (b"\n", {})
    for n in sorted({1, 63, 64, 65, wg - 1, wg, wg + 1, 3 * wg + 5}):
        out["%d lines" % n] = (b"".join(_line(i) + b"\n" for i in range(n)), {})
    for n in (tile - 17, tile - 16, tile - 15, tile, tile + 1):
        out["a line of %d bytes" % n] = (_line(1) + b"\n" + _padded(n) + b"\n" + _line(2) + b"\n", {})
    out["3 tiles between short ones"] = (b"".join(_line(i) + b"\n" for i in range(5)) + _padded(3 * tile) + b"\n" + b"".join(_line(i) + b"\n" for i in range(5, 9)), {})
    # lines that end exactly where a tile staged from a 16-byte boundary ends, and one byte either side of it
    for d in (-1, 0, 1):
        first = _padded(32 * 7 - 1)  # with its '\n': 224 bytes, so the next line starts on a 16-byte boundary
        fill = [_padded(255) for _ in range((tile - 224) // 256 - 1)]
        used = 224 + 256 * len(fill)
        out["a line ending %+d of the tile end" % d] = (b"\n".join([first] + fill + [_padded(tile - used + d), _line(3), _line(4)]) + b"\n", {})
    out["CRLF"] = (b"".join(_line(i) + b"\r\n" for i in range(70)) + _line(70) + b"\r\r\n", {"unexpected_field_error": True})
    blank = [b"", b"   ", b"\t \r", b"\xc2\xa0", b"\xc2\xa0\xe2\x80\x83\xe3\x80\x80 \xe2\x81\x9f", b"\xe2\x80\xa8"]
    mixed = []
    for i in range(3 * wg):
        mixed.append(_line(i))
        mixed += [blank[(i + k) % len(blank)] for k in range(i % 3)]
    mixed += [blank[i % len(blank)] for i in range(2 * wg + 3)] + [_line(9999), b"\xc2", b"\xe2\x80", _line(10000)]  # (a cut rune is no white space)
    out["blank lines interleaved"] = (b"\n".join(mixed) + b"\n", {"row_number_base": 1000})
    body = b"".join(_line(i) + b"\n" for i in range(10))
    out["no trailing newline"] = (body + _line(10), {})
    out["no trailing newline, last chunk"] = (body + _line(10), {"last_chunk": True})
    out["blank tail, last chunk"] = (body + b"  \t", {"last_chunk": True})
    out["no newline at all"] = (_line(1), {})
    out["no newline at all, last chunk"] = (_line(1), {"last_chunk": True})
    out["backslash last"] = (b'"1.2.3.4" "200" "/p\\\n' + _line(1) + b'\n"1.2.3.4" "200" "/p\\"\n"1.2.3.4" "200" "/p\\\\"\n', {})
    out["escaped quotes"] = (b'"1.2.3.4" "200" "GET /p?q=\\"hello\\" HTTP/1.1"\n"1.2.3.4" "200" "a\\\\" "b"\n"1.2.3.4" "200" "a\\\\\\" "b"\n', {"unexpected_field_error": True})
    out["leading space"] = (b" " + _line(1) + b"\n" + _line(2) + b"\n\t" + _line(3) + b"\n", {})
    out["tabs for spaces, extra and trailing"] = (b'"1.2.3.4"\t "200" \t"/a"\n"1.2.3.4" "200" "/b" \t \n"1.2.3.4" "200" "/c" "more"\n"1.2.3.4" "200" "/d"\xc2\xa0\n',
                                                  {"unexpected_field_error": True})
    out["bad cells"] = (b'"1.2.3.4" "abc" "/a"\n"1.2.3.4" "2147483648" "/b"\n"1.2.3.4" "-" "-"\n"-" "12.00" "/c"\n"1.2.3.4" "" ""\n', {"row_number_base": 7, "hide_system_cols": True})
    return out


def test_shapes(tf, oracle):
    schema = shape_schema()
    for name, (data, kw) in shape_chunks(tf).items():
        kw = dict({"file_name": "a/b.log"}, **kw)
        run_both(tf, oracle, SHAPE_FMT, schema, data, ctx=name, **kw)


def test_last_variable_and_adjacent_variables(tf, oracle):
    run_both(tf, oracle, "$a $b", None, b"1 2\r3\n4 5\r\n6  7 8\n9\n 1 2\n", ctx="\\r inside a last variable without delimiter", unexpected_field_error=True)
    run_both(tf, oracle, '$a$b "$c" $d$e', None, b'ab "c" de\n "c" \nab"c" de\nab "c"\n', ctx="adjacent variables")
    run_both(tf, oracle, "$a", abi.Schema([abi.ColSchema("a", "utf8", False, "0"), abi.ColSchema("n", "int64", False, "0")]), b"12\nx y\n-\n  7\n", ctx="one variable")


def test_float32_interval_and_default_double(tf, oracle):
    """the kinds the other cases leave out: float32 (values Go's fast path decides), interval, and a `double` column whose index no field has
    (DefaultValue float64(0): the json.Number "0", a cell that is no byte range of the chunk) beside one that is a view"""
    schema = abi.Schema([abi.ColSchema("f", "float", False, "0"), abi.ColSchema("d", "interval", False, "1"), abi.ColSchema("far", "double", False, "99"),
                         abi.ColSchema("x", "double", False, "0"), abi.ColSchema("far_f", "float", False, "99"), abi.ColSchema("far_d", "interval", False, "99")])
    data = b"1.5 1h30m\n0.25 250ms\n- -\n3 abc\nzz 1s\n-7 1.5h\n1e3 -2m3.5s\n12.00 90\n"
    _, out, want = run_both(tf, oracle, "$a $b", schema, data, ctx="float32 / interval / default double")
    # ("90" is a duration: cast.ToDurationE reads a string without a unit as nanoseconds)
    assert out.nrows == 6 and [(e[0], e[1]) for e in want.errors] == [(4, "CAST"), (5, "CAST")]
    sent = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, _).download()
    assert sent == oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, want.batch, schema)


def test_refused_path(tf):
    f = tf.NginxFormat("$a $b")
    with pytest.raises(tf.TfgpuError) as e:
        tf.nginx_parse(f, tf.nginx_options(), abi.Schema([abi.ColSchema("a", "utf8", False, "a.b")]), b"1 2\n")
    assert e.value.code == tf.ERR_CONFIG


# ---- 4. random parity --------------------------------------------------------------------------------------------------------
MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]


def gen_lines(rng, quoted: bool, n: int) -> bytes:
    def sp():
        return rng.choice([" ", " ", " ", "\t", "  ", " \t"])

    def num():
        k = rng.randrange(6)
        if k == 0:
            return "-"
        if k == 1:
            return str(rng.randrange(0, 10 ** rng.randrange(1, 10)))
        whole, frac = rng.randrange(0, 10 ** rng.randrange(1, 7)), rng.randrange(0, 10 ** 6)
        return "%d.%0*d" % (whole, rng.randrange(1, 7), frac)  # at most 12 significant digits

    lines = []
    for i in range(n):
        addr = "%d.%d.%d.%d" % tuple(rng.randrange(256) for _ in range(4))
        user = rng.choice(["-", "frank", "a\\\"b", "u%d" % i])
        t = "%02d/%s/%04d:%02d:%02d:%02d %s%02d%02d" % (rng.randrange(1, 29), rng.choice(MONTHS), rng.randrange(1971, 2100), rng.randrange(24), rng.randrange(60),
                                                          rng.randrange(60), rng.choice("+-"), rng.randrange(0, 15), rng.choice([0, 30, 45]))
        req = rng.choice(["GET /i%d HTTP/1.1" % i, "POST /a?q=\\\"x\\\" HTTP/2.0", "-", "GET /\\\\ HTTP/1.0", "HEAD /%s HTTP/1.1" % ("p" * rng.randrange(0, 300))])
        status = str(rng.choice([200, 204, 301, 302, 400, 403, 404, 499, 500, 502]))
        size = rng.choice(["-", str(rng.randrange(0, 1 << 40)), "0"])
        bad = rng.random() < 0.05 and rng.randrange(7)
        if bad == 1:
            status = rng.choice(["abc", "20x", "4 04", ""])
        elif bad == 2:
            status = str(rng.choice([2147483648, -2147483649, 10 ** 12]))
        elif bad == 3:
            t = rng.choice(["32/Jan/2024:00:00:00 +0000", "01/Foo/2024:00:00:00 +0000", "2024-01-01T00:00:00Z", "01/Jan/2024:24:00:00 +0000", ""])
        if quoted:
            parts = ['"%s"' % addr, '"-"', '"%s"' % user, '"[%s]"' % t, '"%s"' % req, '"%s"' % status, '"%s"' % size, '"%s"' % num(), '"%s"' % num(), '"h%d.example"' % (i % 7)]
            line = parts[0]
            for p in parts[1:]:
                line += sp() + p
        else:
            line = addr + sp() + "-" + sp() + user + sp() + "[" + t + "]" + sp() + '"' + req + '"' + sp() + status + sp() + size + sp() + '"-"' + sp() + '"Mozilla/5.0 (X11; %d)"' % i
        if bad == 4:
            line = line[:rng.randrange(1, len(line))]
        elif bad == 5:
            k = rng.randrange(len(line))
            line = line[:k] + "#" + line[k + 1:]
        elif bad == 6:
            line += rng.choice([' "extra"', " x", "\t\t", " \xa0"])
        lines.append(line)
        if rng.random() < 0.02:
            lines.append(rng.choice(["", " ", "\t", "\xa0"]))
    return ("\n".join(lines) + "\n").encode("utf-8")


def random_schema(tf, quoted):
    f = tf.NginxFormat(QUOTED if quoted else COMBINED)
    cols = [abi.ColSchema("remote_addr", "utf8"), abi.ColSchema("remote_user", "string"), abi.ColSchema("time_local", "datetime"), abi.ColSchema("day", "date", False, "2"),
            abi.ColSchema("request", "utf8"), abi.ColSchema("status", "int32", True), abi.ColSchema("status_u", "uint16", False, "4"), abi.ColSchema("body_bytes_sent", "uint64")]
    if quoted:
        cols += [abi.ColSchema("request_time", "double"), abi.ColSchema("upstream_response_time", "double"), abi.ColSchema("host", "utf8")]
    else:
        cols += [abi.ColSchema("http_user_agent", "utf8"), abi.ColSchema("far", "boolean", False, "40")]
    return f.resolve_schema(abi.Schema(cols))


@pytest.mark.parametrize("quoted", [False, True], ids=["combined", "quoted"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_parity(tf, oracle, seed, quoted):
    rng = random.Random(seed * 2 + int(quoted))
    data = gen_lines(rng, quoted, 4096)
    schema = random_schema(tf, quoted)
    # the restatement alone first: the generator yields nothing the reference cannot decide, and it does break lines
    want = ref.parse_chunk(oracle, ref.compile_format((QUOTED if quoted else COMBINED).encode()), schema, data, file_name="r.log", unexpected_field_error=True)
    kinds = {e[1] for e in want.errors}
    assert "HOST_FALLBACK" not in kinds and {"NGINX_FORMAT", "NGINX_EXTRA", "CAST", "RANGE"} <= kinds and 100 < len(want.errors) < 400
    run_both(tf, oracle, QUOTED if quoted else COMBINED, schema, data, ctx="seed %d" % seed, file_name="r.log", unexpected_field_error=True)


# ---- 5. memory kinds ---------------------------------------------------------------------------------------------------------
def test_memory_kinds(tf, oracle):
    data = gen_lines(random.Random(11), True, 300)
    schema = random_schema(tf, True)
    host = tf.HostBuffer(data)
    dev = tf.DeviceBuffer.upload(data)
    rows = []
    for src in (None, host, dev):
        db, out, _ = run_both(tf, oracle, QUOTED, schema, data, src=src, file_name="m.log")
        rows.append(abi.batch_rows(out))
    dev.free()  # the batch keeps the text alive itself
    assert rows[0] == rows[1] == rows[2] and abi.batch_rows(db.download()) == rows[0]
    host.free()


# ---- 6. the batch flows on -----------------------------------------------------------------------------------------------------
def test_downstream_filter_and_serialize(tf, oracle):
    data = gen_lines(random.Random(5), True, 500)
    schema = random_schema(tf, True)
    db, _, want = run_both(tf, oracle, QUOTED, schema, data, file_name="d.log")
    cfg = {"filter": "status >= 400"}
    got = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, tf.apply_chain([tf.Transformer("filter_rows", cfg)], db).transformed).download()
    kept = oracle.apply_chain([oracle.Transformer("filter_rows", cfg)], want.batch, schema)
    exp = oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, kept.batch, kept.schema)
    assert exp is not None and 0 < kept.batch.nrows < want.batch.nrows
    assert got == exp
