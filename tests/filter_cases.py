"""The batches and the filters that tests/test_filter_ref.py (model against oracle, no device) and tests/test_gpu_filter_rows.py (device against
model) both run: one batch of 257 rows per column family — one row past a 256-thread workgroup — whose cells are the family's edge values in
rotation, so that rows 0, 255 and 256 hold edge values too, with nil cells among them; a variant of every batch whose rows list their own columns
(ABSENT bitmaps, and one row that lists nothing); per column every constant type it can meet under every operator, with constants on and beside
the edge values.

A family built for a fallback class (`fallback`: text under a numeric constant, `any` scalars, texts under a time constant that are none of the
fixed shapes, floats outside the int64 range under an int list) is the only place where the model may say MAY_FALL_BACK or IMPL_DEFINED and the
device HOST_FALLBACK; test_filter_ref.py asserts the first half of that, test_gpu_filter_rows.py the second."""
import numpy as np

from transferia_amd import abi

N = 257
NIL_EVERY, NIL_AT = 11, 7            # rows 7, 18, 29, ... are nil: not 0, 255 or 256
ABSENT_EVERY, ABSENT_AT = 13, 5      # the variant: rows 5, 18, 31, ... do not list the tested columns (18 is nil as well)
LISTS_NOTHING = 100                  # ... and this row lists no column at all
CMP = ["=", "!=", "<", "<=", ">", ">="]
MIN_I64, MAX_I64 = -(1 << 63), (1 << 63) - 1


class Family:
    def __init__(self, name, batch, filters, fallback=False):
        """filters: [config dict]; fallback: built for a fallback class"""
        self.name, self.batch, self.filters, self.fallback = name, batch, filters, fallback

    def schema(self):
        return abi.Schema.of([[c.name, c.dtype, False] for c in self.batch.cols])

    def variant(self):
        """the same cells in rows that list their own columns"""
        cols = []
        for c in self.batch.cols:
            d = abi.Column(c.name, c.dtype, c.repr, values=c.values, offsets=c.offsets, data=c.data, nanos=c.nanos, validity=c.validity)
            d.absent = np.array([i % ABSENT_EVERY == ABSENT_AT or i == LISTS_NOTHING for i in range(N)], bool)
            cols.append(d)
        cols.append(fixed("always", "int32", abi.R_INT32, list(range(N)), nils=False))      # what the other rows still list
        cols[-1].absent = np.array([i == LISTS_NOTHING for i in range(N)], bool)
        b = abi.Batch(cols, N, self.batch.table_ns, self.batch.table_name)
        b.kind = self.batch.kind
        return Family(self.name + "/absent", b, self.filters[::7], self.fallback)          # 7: prime to the operators' and the constants' counts


def rotate(vals, nils=True):
    return [None if nils and i % NIL_EVERY == NIL_AT else vals[i % len(vals)] for i in range(N)]


def fixed(name, dtype, repr_, vals, nils=True, nanos=None):
    cells = rotate(vals, nils)
    valid = np.array([v is not None for v in cells], bool)
    if repr_ == abi.R_TIME:
        a = np.array([0 if v is None else v[0] for v in cells], np.int64)
        nn = np.array([0 if v is None else v[1] for v in cells], np.int32)
        return abi.Column(name, dtype, repr_, values=a, nanos=nn, validity=None if valid.all() else valid)
    a = np.array([0 if v is None else v for v in cells], dtype=abi.REPR_NP[repr_])
    return abi.Column(name, dtype, repr_, values=a, validity=None if valid.all() else valid)


def text(name, dtype, repr_, vals, nils=True):
    cells = rotate(vals, nils)
    off = np.zeros(N + 1, np.uint32)
    off[1:] = np.cumsum([len(c or b"") for c in cells])
    valid = np.array([c is not None for c in cells], bool)
    return abi.Column(name, dtype, repr_, offsets=off, data=np.frombuffer(b"".join(c or b"" for c in cells), np.uint8).copy(),
                      validity=None if valid.all() else valid)


def one(flt):
    return {"filter": flt}


def quoted(b: bytes, q="'"):
    """a filter string constant for these bytes (valid UTF-8)"""
    return q + b.decode("utf-8").replace("\\", "\\\\").replace(q, "\\" + q) + q


def other_types(col, skip):
    """one constant of every type but `skip` against `col`, and the NULL terms"""
    consts = {"int": ["= 1", "IN (1, 2)"], "float": ["= 1.5", "NOT IN (1.5)"], "bool": ["= TRUE", "!= false"], "string": ["= 'a'", "~ 'a'", "IN ('a')"],
              "time": ["= 1970-01-01", "< 1970-01-01T00:00:00Z", "IN (1970-01-01T00:00)"]}
    out = [one("%s %s" % (col, c)) for ty, cs in consts.items() if ty not in skip for c in cs]
    return out + [one("%s = NULL" % col), one("%s != nil" % col)]


# ---- integers ---------------------------------------------------------------------------------------------------------------------------------------
INT_COLS = [("i8", "int8", abi.R_INT8), ("i16", "int16", abi.R_INT16), ("i32", "int32", abi.R_INT32), ("i64", "int64", abi.R_INT64),
            ("u8", "uint8", abi.R_UINT8), ("u16", "uint16", abi.R_UINT16), ("u32", "uint32", abi.R_UINT32), ("u64", "uint64", abi.R_UINT64)]
INT_POINTS = [0, 1, -1, 2**53 - 1, 2**53, 2**53 + 1, 2**53 + 2, 2**53 + 3, 2**63 - 513, 2**63 - 512, 2**63 - 1, 2**63, 2**64 - 1]


def int_edges(repr_):
    info = np.iinfo(abi.REPR_NP[repr_])
    return sorted({int(info.min), int(info.max)} | {p for p in INT_POINTS if info.min <= p <= info.max})


def int_constants(edges):
    return sorted({c for e in edges for c in (e - 1, e, e + 1) if MIN_I64 <= c <= MAX_I64})


def integers(which):
    name, dtype, repr_ = next(c for c in INT_COLS if c[0] == which)
    edges = int_edges(repr_)
    b = abi.Batch([fixed(name, dtype, repr_, edges)], N, "db", "t")
    fl = []
    for c in int_constants(edges):
        for op in CMP:
            fl.append(one("%s %s %d" % (name, op, c)))
            fl.append(one("%s%s%+d.0" % (name, op, c)))                       # the float form of the same number, its sign glued to the operator
    some = edges[len(edges) // 2]
    for lst in ("(%d)" % some, "(%d, %d)" % (edges[0], edges[-1] if edges[-1] <= MAX_I64 else 7), "(-9223372036854775808, 9223372036854775807)", "(5, 6)",
                "(%d.0, 0.0)" % some, "(-0.0)", "(0.0, 0.5)", "(9223372036854775807.0)", "(9007199254740993.0)"):
        fl += [one("%s IN %s" % (name, lst)), one("%s NOT IN %s" % (name, lst))]
    fl += [one("%s ~ 1" % name), one("%s !~ 1.0" % name)]                     # "Unknown operation"
    return Family("integers/" + name, b, fl + other_types(name, ("int", "float")))


# ---- floats -----------------------------------------------------------------------------------------------------------------------------------------
F32 = [float(np.float32(0.1)), 16777216.0, float(np.float32(16777217)), float(np.float32(1e-45)), float(np.finfo(np.float32).max), 0.0, -0.0,
       float("inf"), float("-inf"), float("nan"), 0.5, 1.5, -2.5, 3.0, -1.0]
F64 = [0.1, 2.0**53, 2.0**53 + 2, 9223372036854775807.0, 1e19, -1e19, 1e300, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 5e-324, 1.5, -2.0,
       3.0, -9223372036854775808.0, 9223372036854774784.0]
FLOAT_CONSTS = ["0.1", "0.10000000149011612", "0.10000000149011611", "16777216.0", "16777217.0", "0.0", "-0.0", "0.5", "1.5", "1.50000000000000022", "-2.5",
                "340282346638528859811704183484516925440.0", "340282346638528859811704183484516925441.0", "9007199254740992.0", "9007199254740994.0",
                "9223372036854775807.0", "10000000000000000000.0", "-10000000000000000000.0", "0.000000000000000000000000000000000000000000001",
                "1" + "0" * 300 + ".0", "3.0"]
FLOAT_INT_CONSTS = ["0", "1", "-1", "3", "16777216", "16777217", "9007199254740992", "9007199254740993", "9223372036854775807", "-9223372036854775808", "2"]


def floats(which, in_range_only=False):
    name, dtype, repr_, vals = ("f", "float", abi.R_FLOAT32, F32) if which == "float" else ("d", "double", abi.R_FLOAT64, F64)
    if in_range_only:
        vals = [v for v in vals if -9223372036854775808.0 <= v < 9223372036854775808.0 or v != v]
    b = abi.Batch([fixed(name, dtype, repr_, vals)], N, "db", "t")
    int_lists = ["(0)", "(3, 1)", "(-9223372036854775808)", "(9223372036854775807)", "(-9223372036854775808, 9223372036854775807, 16777216)", "(-2, -1)"]
    lists = [one("%s %s %s" % (name, op, lst)) for lst in int_lists for op in ("IN", "NOT IN")]
    if in_range_only:
        return Family("floats/%s/int lists, every float inside the int64 range" % which, b, lists)
    fl = [one("%s %s %s" % (name, op, c)) for c in FLOAT_CONSTS + FLOAT_INT_CONSTS for op in CMP]
    for lst in ("(0.0)", "(-0.0)", "(0.1, 1.5)", "(0.10000000149011612, -2.5)", "(16777216.0)", "(5.5)"):
        fl += [one("%s IN %s" % (name, lst)), one("%s NOT IN %s" % (name, lst))]
    fl += [one("%s ~ 1.5" % name), one("%s !~ 1" % name)]
    return [Family("floats/" + which, b, fl + other_types(name, ("int", "float"))),
            Family("floats/%s/int lists" % which, b, lists, fallback=True)]


def booleans():
    b = abi.Batch([fixed("b", "boolean", abi.R_BOOL, [1, 0, 1, 1, 0])], N, "db", "t")
    fl = [one("b %s %s" % (op, c)) for c in ("TRUE", "false", "True", "0", "1", "2", "-1", "0.0", "1.0", "0.5") for op in CMP]
    for lst in ("(1)", "(0, 2)", "(1.0)", "(0.5, 0.0)"):
        fl += [one("b IN %s" % lst), one("b NOT IN %s" % lst)]
    fl += [one("b ~ TRUE"), one("b !~ false"), one("b ~ 1")]
    return Family("bool", b, fl + other_types("b", ("int", "float", "bool")))


# ---- times ------------------------------------------------------------------------------------------------------------------------------------------
YEAR1, YEAR9999 = -62135596800, 253402300799
TIME_CONSTS = ["1970-01-01T00:00:00Z", "1969-12-31T23:59:59Z", "1969-12-31T23:59:59.999999Z", "1969-12-31T23:59:59.000001Z", "1970-01-01T00:00:00.000001Z",
               "1970-01-01T00:00:00.0000019Z", "1970-01-01T00:00:01Z", "0001-01-01T00:00:00Z", "0001-01-01T00:00:00.999999Z", "0001-01-01",
               "9999-12-31T23:59:59Z", "9999-12-31T23:59:59.999999Z", "9999-12-31", "1970-01-01", "1970-01-01T00:00", "1970-01-01T03:00:00+03:00",
               "1969-12-31T21:00-03", "1970-01-02T00:00:00+24:00", "1970-01-01T00:00:00-00:60"]


def times():
    pts = [(s, n) for s in (-1, 0, YEAR1, YEAR9999, 1) for n in (0, 999, 1000, 999_999_999)]
    days = [(s, 0) for s in (0, -86400, YEAR1, YEAR9999 - 86399, 86400)]
    b = abi.Batch([fixed("ts", "timestamp", abi.R_TIME, pts), fixed("dt", "datetime", abi.R_TIME, [p for p in pts if p[1] == 0]), fixed("day", "date", abi.R_TIME, days)], N, "db", "t")
    fl = []
    for col in ("ts", "dt", "day"):
        fl += [one("%s %s %s" % (col, op, c)) for c in TIME_CONSTS for op in CMP]
        for lst in ("(1970-01-01)", "(1969-12-31T23:59:59Z, 0001-01-01)", "(1970-01-01T00:00:00.000001Z, 9999-12-31T23:59:59.999999Z)", "(2020-02-29)"):
            fl += [one("%s IN %s" % (col, lst)), one("%s NOT IN %s" % (col, lst))]
        fl += [one("%s ~ 1970-01-01" % col), one("%s !~ 1970-01-01T00:00:00Z" % col)]
        fl += other_types(col, ("time",))
    return Family("times", b, fl)


# ---- text -------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = [b"", b"ab", b"abc", b"abcd", "é".encode(), b"\xff\xfe", b"a\xc3", b"aaab", b"ababab", b"aab", b"abab", b"z", b"abc\x00", b"\x7f", "日本".encode(), b"b"]
TEXT_CONSTS = [b"", b"abc", b"ab", b"abcd", b"aab", b"aaa", b"aaabb", b"abab", b"babab", b"abababa", b"b", b"a", b"z", "é".encode(), b"\x7f", "日".encode(),
               b"abc\x00"]


def texts():
    b = abi.Batch([text("s", "utf8", abi.R_STRING, TEXTS), text("y", "string", abi.R_BYTES, TEXTS[::-1])], N, "db", "t")
    fl = []
    for col in ("s", "y"):
        for c in TEXT_CONSTS:
            q = quoted(c) if b"\x00" not in c and c != "é".encode() else ("'abc\\x00'" if b"\x00" in c else '"\\u00e9"')
            fl += [one("%s %s %s" % (col, op, q)) for op in CMP + ["~", "!~"]]
        for lst in ("('abc')", "('', 'ab')", "('aab', \"abab\", 'nope')", "('é', 'z')", "('abcde')"):
            fl += [one("%s IN %s" % (col, lst)), one("%s NOT IN %s" % (col, lst))]
    fl += other_types("s", ("int", "float", "string", "time")) + other_types("y", ("string",))
    return Family("text", b, fl)


NUMBER_TEXTS = [b"12.5", b"1e3", b"0x10", b"1_0", b"abc", b"inf", b"NaN", b"", b"-0", b"+7", b"0x1p4", b"1e400", b" 1", b"9223372036854775808", b"-Infinity", b".5", b"5."]
NUMERIC_TERMS = ["> 10", "= 10", "<= 12.5", "!= 1000.0", ">= 16", "< 0.5", "= 0.0", "IN (10, 16)", "NOT IN (12.5, 1000.0)", "IN (9223372036854775807)", "NOT IN (7)", "~ 1"]


def number_texts():
    b = abi.Batch([text("s", "utf8", abi.R_STRING, NUMBER_TEXTS), text("n", "utf8", abi.R_JSONNUM, [t for t in NUMBER_TEXTS if t not in (b"", b" 1")])], N, "db", "t")
    return Family("text that holds numbers", b, [one("%s %s" % (col, t)) for col in ("s", "n") for t in NUMERIC_TERMS], fallback=True)


def json_numbers():
    b = abi.Batch([text("n", "utf8", abi.R_JSONNUM, [b"1", b"12.5", b"-3", b"1e3"])], N, "db", "t")
    return Family("json.Number", b, other_types("n", ("int", "float")))           # no string, no time, no bool to matchValue; not nil


FIXED_TIME_TEXTS = [b"1970-01-01", b"1970-01-01 00:00:00", b"1970-01-01T00:00:00", b"1970-01-01T00:00:00Z", b"1970-01-01T03:00:00+03:00", b"1969-12-31 23:59:59.999999",
                    b"1969-12-31T23:59:59,999999", b"1970-01-01T00:00:00.0000019Z", b"1970-01-01 00:00:00,000001", b"1970-01-01T00:00:00.000001999-00:00",
                    b"2020-02-29", b"2019-02-29", b"2020-02-30 00:00:00", b"1970-01-01T24:00:00", b"1970-01-01 00:00:60", b"1970-01-01T00:60:00Z",
                    b"1970-01-02T00:00:00+24:00", b"1970-01-01T00:00:00-00:60", b"1970-01-01T00:00:00+25:00", b"1970-01-01T00:00:00+00:61", b"1970-13-01", b"1970-00-10",
                    b"1970-01-00", b"0000-01-01T00:00:00Z", b"9999-12-31T23:59:59.999999999Z", b"0001-01-01"]
OTHER_TIME_TEXTS = [b"2020-01-01 10:00:00 +0300 MSK", b"2020-01-01T10:00:00.123+0300", b"Mon Jan  2 15:04:05 2006", b"10:00:00", b"abc", b"", b"1970-01-01 00:00:00Z",
                    b"1970-01-01T00:00:00.", b"1970-01-01T00:00", b"1970-1-1", b"02 Jan 06 15:04 MST", b"1970-01-01", b"3:04PM"]
TIME_TERMS = ["%s %s" % (op, c) for c in ("1970-01-01T00:00:00Z", "1969-12-31T23:59:59.999999Z", "1970-01-01T00:00:00.000001Z", "2020-02-29", "1970-01-02T00:00", "0001-01-01") for op in CMP] + \
             ["IN (1970-01-01, 2020-02-29)", "NOT IN (1970-01-01T00:00:00.000001Z)", "IN (1970-01-01T00:01:00Z)", "~ 1970-01-01"]


def time_texts(fixed_shapes):
    vals = FIXED_TIME_TEXTS if fixed_shapes else OTHER_TIME_TEXTS
    b = abi.Batch([text("s", "utf8", abi.R_STRING, vals)], N, "db", "t")
    return Family("text that holds times/" + ("fixed shapes" if fixed_shapes else "other layouts"), b, [one("s " + t) for t in TIME_TERMS], fallback=not fixed_shapes)


# ---- any, interval ----------------------------------------------------------------------------------------------------------------------------------
ANY_SCALARS = [b'"abc"', b'"x"', b'""', b'"ab\\u0063d"', b'"12.5"', b'"1970-01-01"', b"12.5", b"10", b"-0.0", b"1e19", b"true", b"false", b' "abc"', b'{"k":1}', b"[1]", b"3"]
ANY_CONTAINERS = [b'{"k":1}', b"[]", b"{}", b' [ "abc" ]', b'\n{"abc":"abc"}']
ANY_TERMS = ["= \"abc\"", "!= 'abc'", "< 'b'", "~ 'bc'", "!~ 'x'", "IN ('abc', 'x')", "NOT IN ('')", "> 10", "= 12.5", "<= 3", "IN (10, 3)", "NOT IN (12.5)", "IN (-9223372036854775808)",
             "= TRUE", "!= false", "> FALSE", "= 1970-01-01", "IN (1970-01-01T00:00)", "= NULL", "!= NULL"]


def anys(containers):
    b = abi.Batch([text("a", "any", abi.R_JSON, ANY_CONTAINERS if containers else ANY_SCALARS)], N, "db", "t")
    return Family("any/" + ("containers" if containers else "scalars"), b, [one("a " + t) for t in ANY_TERMS], fallback=not containers)


def intervals():
    b = abi.Batch([fixed("iv", "interval", abi.R_DURATION, [0, 1, -1, 10**15, MIN_I64, MAX_I64])], N, "db", "t")
    return Family("interval", b, other_types("iv", ()) + [one("iv %s 0" % op) for op in CMP] + [one("iv IN (0, 1)"), one("iv NOT IN (0.0)")])


# ---- AND / OR, kinds, tables --------------------------------------------------------------------------------------------------------------------------
def logic():
    """each failing class behind a false term, behind an expression that matched, and the mirror of each"""
    n = N
    i = fixed("i", "int64", abi.R_INT64, [5, -5, 0, 7, -7, 100])
    u = fixed("u", "uint64", abi.R_UINT64, [1, 2**63, 2**64 - 1, 2**63 - 1])
    iv = fixed("iv", "interval", abi.R_DURATION, [0, 1])
    m = fixed("m", "int32", abi.R_INT32, [1, 2, 3], nils=False)
    m.absent = np.array([r % 5 == 2 for r in range(n)], bool)
    b = abi.Batch([i, u, iv, m], n, "db", "t")
    fails = {"INT_OVERFLOW": "u > 0", "TYPE_PAIR": "iv = 0", "COLUMN_NOT_FOUND": "m >= 1", "COLUMN_NOT_FOUND (no such name)": "nosuch = 1", "INT_OVERFLOW before NULL": "u = NULL"}
    fl = []
    for f in fails.values():
        fl += [one("i > 0 AND %s" % f), one("%s AND i > 0" % f), {"filters": ["i > 0", f]}, {"filters": [f, "i > 0"]},
               one("i > 0 AND i < 50 AND %s AND i != 7" % f), {"filters": ["i > 50 AND i < 0", "i = 5 AND %s" % f, "i <= 0"]},
               {"filters": ["i < 0 AND %s" % f, "i > 6 AND %s AND i > 50" % f, f]}]
    fl += [{"filters": ["u > 0", "iv = 0", "m >= 1"]}, one("m >= 1 AND iv = 0 AND u > 0"), one(""), {"filters": ["", "u > 0"]}, one("  "),
           {"filters": ["i = NULL", "i > 6"]}, one("i != NULL AND i >= 0 AND i <= 7 AND i IN (0, 7)")]
    return Family("logic", b, fl)


def kinds():
    b = abi.Batch([fixed("i", "int64", abi.R_INT64, [5, -5, 0, 7])], N, "db", "t")
    b.kind = np.array([(r * 3) % 5 if r % 3 else 0 for r in range(N)], np.uint8)    # Update / Delete / other / Synchronize rows among the Inserts
    fl = [one("i > 0"), one("nosuch = 1"), {"filter": "i > 0", "tables": {"excludeTables": ["^db\\.t$"]}}, {"filter": "i > 0", "tables": {"includeTables": ["^db\\.t$"]}},
          {"filter": "i > 0", "tables": {"includeTables": ["other"]}}]
    sysb = abi.Batch(b.cols, N, "db", "__wal")
    sysb.kind = b.kind
    plain = abi.Batch(b.cols, N, "db", "__wal")                                      # a system table, every row an Insert: passed through whole
    return [Family("kinds", b, fl), Family("kinds/system table", sysb, fl[:2]), Family("system table", plain, fl[:2])]


def families():
    out = [integers(c[0]) for c in INT_COLS]
    out += floats("float") + floats("double") + [floats("float", True), floats("double", True)]
    out += [booleans(), times(), texts(), number_texts(), json_numbers(), time_texts(True), time_texts(False), anys(False), anys(True), intervals(), logic()]
    out += kinds()
    return out


def all_cases():
    """every family and its ABSENT variant"""
    fams = families()
    return fams + [f.variant() for f in fams if not f.name.startswith(("kinds", "system"))]
