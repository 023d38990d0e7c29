"""Plain-Python restatement of the native parser (pkg/parsers/registry/native/parser_native.go): abstract.UnmarshalChangeItems + ValidateChangeItems +
RestoreChangeItems (pkg/abstract/restore.go:320-373, validator.go:9-39, changeitem/change_item.go:618-678) over message bytes, together with the line
include/tfgpu.h draws between what the device takes and what it leaves to the stock parser (tfgpu_native_reason).  tests/test_nativeparse_ref.py pins
it to the reference's own vectors, tests/test_gpu_nativeparse.py holds the device to it.  Nothing here imports the library.

The JSON grammar, UseNumber decoding and json.Marshal come from tests/rawtable_ref.py (Python's json is not encoding/json); the cell conversions come
from oracle/dbz_emitter.restore where it says the same thing, and are restated here where it leaves something out: integer ranges, the strictness of
base64, the time forms, `any` (whose cells the ABI carries as json.Marshal text, HTML escaping on, as every producer of TFGPU_R_JSON writes it)."""
import base64
import re

from oracle import dbz_emitter as E
from rawtable_ref import CANON_DEPTH, HostFallback, Num, WS, _Bad, _Scanner, go_string_html, marshal, utf8_valid
from transferia_amd import abi

DTYPES = abi.DTYPES[1:]
INT_RANGE = {"int8": (-2**7, 2**7 - 1), "int16": (-2**15, 2**15 - 1), "int32": (-2**31, 2**31 - 1), "int64": (-2**63, 2**63 - 1),
             "uint8": (0, 2**8 - 1), "uint16": (0, 2**16 - 1), "uint32": (0, 2**32 - 1), "uint64": (0, 2**64 - 1)}
MEMBERS = ("id", "nextlsn", "commitTime", "txPosition", "kind", "schema", "table", "part", "columnnames", "columnvalues", "table_schema", "oldkeys", "tx_id", "query")
COL_TAGS = ("name", "type", "key", "fake_key", "required", "path", "original_type", "table_schema", "table_name", "expression", "properties")
_INT = re.compile(r"-?[0-9]+\Z")
_TIME = re.compile(r"^(\d{4})-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d)(?:\.(\d{1,9}))?(Z|[+-]\d\d:\d\d)\Z", re.A)
_B64 = re.compile(rb"^(?:[A-Za-z0-9+/]{4})*(?:[A-Za-z0-9+/]{2}==|[A-Za-z0-9+/]{3}=)?\Z")


class Fallback(Exception):
    def __init__(self, reason, column=-1):
        Exception.__init__(self, reason)
        self.reason, self.column = reason, column


class Pairs(list):
    """an object as its (key, value) pairs in source order"""


class _PairScanner(_Scanner):
    def obj(self):
        out = Pairs()
        self.ws()
        if self.b[self.p:self.p + 1] == b"}":
            self.p += 1
            return out
        while True:
            self.ws()
            if self.b[self.p:self.p + 1] != b'"':
                raise _Bad()
            k = self.string()
            self.ws()
            if self.b[self.p:self.p + 1] != b":":
                raise _Bad()
            self.p += 1
            out.append((k, self.value()))
            self.ws()
            d = self.b[self.p:self.p + 1]
            self.p += 1
            if d == b"}":
                return out
            if d != b",":
                raise _Bad()


def plain(v):
    """a value with its objects as dicts again (the last of a repeated key stands)"""
    if isinstance(v, Pairs):
        return {k: plain(x) for k, x in v}
    if isinstance(v, list):
        return [plain(x) for x in v]
    return v


# ---- the cut: `[` objects `]` between white space -----------------------------------------------------------------------------------------------------------
def cut(msg: bytes):
    """the items' (start, end) spans, or None where the message is not an array of objects by its brackets, quotes and commas alone"""
    n, p = len(msg), 0

    def ws():
        nonlocal p
        while p < n and msg[p] in WS:
            p += 1
    ws()
    if p >= n or msg[p] != 0x5B:
        return None
    p += 1
    spans = []
    ws()
    if p < n and msg[p] == 0x5D:
        p += 1
    else:
        while True:
            ws()
            if p >= n or msg[p] != 0x7B:
                return None
            s, depth, instr = p, 0, False
            while p < n:
                c = msg[p]
                if instr:
                    if c == 0x5C:
                        p += 1
                    elif c == 0x22:
                        instr = False
                elif c == 0x22:
                    instr = True
                elif c in (0x7B, 0x5B):
                    depth += 1
                elif c in (0x7D, 0x5D):
                    depth -= 1
                    if depth == 0:
                        break
                p += 1
            if p >= n or msg[p] != 0x7D:
                return None
            p += 1
            spans.append((s, p))
            ws()
            if p < n and msg[p] == 0x2C:
                p += 1
                continue
            if p < n and msg[p] == 0x5D:
                p += 1
                break
            return None
    ws()
    return spans if p == n else None


# ---- one item's own form ---------------------------------------------------------------------------------------------------------------------------------------
class Header:
    def __init__(self):
        self.raw = {}      # member -> the value's text (absent and null: not there)
        self.val = {}      # member -> the decoded value
        self.id = self.lsn = self.commit = self.counter = 0
        self.kind = None
        self.old = {}      # keynames / keytypes / keyvalues -> (text, value)


def _members(span: bytes, start: int, scanner):
    """(key, plain key?, value text, value) of the object that starts at span[start], in source order"""
    sc = scanner(span)
    sc.p = start + 1
    while True:
        sc.ws()
        if span[sc.p:sc.p + 1] == b"}":
            return
        ks = sc.p
        key = sc.string()
        rawkey = span[ks + 1:sc.p - 1]
        sc.ws()
        sc.p += 1
        sc.ws()
        vs = sc.p
        v = sc.value()
        yield key, (b"\\" not in rawkey and all(c < 0x80 for c in rawkey)), span[vs:sc.p], v
        sc.ws()
        if span[sc.p:sc.p + 1] == b",":
            sc.p += 1


def _unsigned(v, bits):
    return isinstance(v, Num) and _INT.match(v) and not v.startswith("-") and int(v) < 2**bits


def read_header(span: bytes) -> Header:
    if not utf8_valid(span):
        raise Fallback("UTF8")
    sc = _Scanner(span)
    try:
        sc.value()
        sc.ws()
        if sc.p != len(span):
            raise _Bad()
    except _Bad:
        raise Fallback("SYNTAX")
    except HostFallback:
        raise Fallback("DEPTH")
    h, seen = Header(), set()
    for key, is_plain, text, v in _members(span, 0, _Scanner):
        if not is_plain:
            raise Fallback("KEY_FORM")
        if key not in MEMBERS:
            continue
        if key in seen:
            raise Fallback("DUP_MEMBER")
        seen.add(key)
        if v is None:
            continue   # Decode(null) leaves the field as it is
        if key in ("id", "nextlsn", "commitTime"):
            if not _unsigned(v, 32 if key == "id" else 64):
                raise Fallback("HEADER_VALUE")
            setattr(h, {"id": "id", "nextlsn": "lsn", "commitTime": "commit"}[key], int(v))
        elif key == "txPosition":
            if not (isinstance(v, Num) and _INT.match(v) and -2**63 <= int(v) < 2**63):
                raise Fallback("HEADER_VALUE")
            h.counter = int(v)
        elif key == "kind":
            if not isinstance(v, str) or isinstance(v, Num):
                raise Fallback("HEADER_VALUE")
            h.kind = {b'"insert"': "insert", b'"update"': "update", b'"delete"': "delete"}.get(text)
        elif key in ("schema", "table", "part", "tx_id", "query"):
            if not isinstance(v, str) or isinstance(v, Num):
                raise Fallback("HEADER_VALUE")
            h.raw[key], h.val[key] = text, v
        elif key == "columnnames":
            if not isinstance(v, list) or any(not isinstance(x, str) or isinstance(x, Num) for x in v):
                raise Fallback("HEADER_VALUE")
            h.raw[key], h.val[key] = text, v
        elif key in ("columnvalues", "table_schema"):
            if not isinstance(v, list):
                raise Fallback("HEADER_VALUE")
            h.raw[key], h.val[key] = text, v
        elif key == "oldkeys":
            if not isinstance(v, dict):
                raise Fallback("HEADER_VALUE")
            oseen = set()
            for ok, opl, otext, ov in _members(text, 0, _Scanner):
                if not opl:
                    raise Fallback("KEY_FORM")
                if ok not in ("keynames", "keytypes", "keyvalues"):
                    raise Fallback("HEADER_VALUE")
                if ok in oseen:
                    raise Fallback("DUP_MEMBER")
                oseen.add(ok)
                if ov is None:
                    continue
                if not isinstance(ov, list) or (ok != "keyvalues" and any(not isinstance(x, str) or isinstance(x, Num) for x in ov)):
                    raise Fallback("HEADER_VALUE")
                h.old[ok] = (otext, ov)
    if h.kind is None:
        raise Fallback("KIND")
    ncn, ncv = len(h.val.get("columnnames", [])), len(h.val.get("columnvalues", []))
    nkn, nkv = len(h.old.get("keynames", (b"", []))[1]), len(h.old.get("keyvalues", (b"", []))[1])
    if ncn != ncv:
        raise Fallback("LENGTHS")
    if h.kind == "insert":
        if nkv:
            raise Fallback("INSERT_KEYVALUES")
    elif nkn != nkv:
        raise Fallback("LENGTHS")
    return h


# ---- a group's columns ---------------------------------------------------------------------------------------------------------------------------------------------
class Column:
    def __init__(self, name, col):
        self.name, self.col = name, col   # col: the table_schema entry of that name (a dict of its tags), or None


def read_schema(text: bytes):
    """table_schema as the host reads it: [dict of the known tags], or None where only encoding/json decides (a repeated tag, a tag in another letter
    case, a value of another type)"""
    if not text:
        return []
    sc = _PairScanner(text)
    cols = []
    for c in sc.value():
        if not isinstance(c, Pairs):
            return None
        d, keys = {}, [k for k, _ in c]
        if len(set(keys)) != len(keys):
            return None
        for k, v in c:
            if k in ("name", "type", "path", "original_type", "table_schema", "table_name", "expression"):
                if v is not None and (not isinstance(v, str) or isinstance(v, Num)):
                    return None
                d[k] = v or ""
            elif k in ("key", "fake_key", "required"):
                if v is not None and not isinstance(v, bool):
                    return None
                d[k] = bool(v)
            elif k == "properties":
                if v is not None and not isinstance(v, Pairs):
                    return None
                d[k] = plain(v) if v else None
            elif k.lower() in COL_TAGS:
                return None
        cols.append(d)
    return cols


def group_columns(h: Header):
    """(value columns, OldKeys columns, schema) of the item's group, or None where the host does not read its texts"""
    texts = [h.raw.get(k, b"") for k in ("schema", "table", "part", "columnnames", "table_schema")] + [h.old.get(k, (b"",))[0] for k in ("keynames", "keytypes")]
    if any(re.search(rb"\\u[dD]", t) for t in texts):
        return None
    schema = read_schema(h.raw.get("table_schema", b""))
    if schema is None:
        return None
    by_name = {}
    for c in schema:
        by_name[c.get("name", "")] = c   # a later column of the same name stands
    return ([Column(n, by_name.get(n)) for n in h.val.get("columnnames", [])], [Column(n, by_name.get(n)) for n in h.old.get("keynames", (b"", []))[1]], schema)


def is_binary(ot: str) -> bool:
    return E.trim_mysql_type(ot) in E.MYSQL_BINARY or ot in ("pg:bytea", "ydb:String") or ot.startswith("mysql:binary") or ot.startswith("mysql:blob")


def repr_of(col) -> int:
    d, ot = col["type"], col.get("original_type", "")
    if d in INT_RANGE:
        return getattr(abi, "R_" + d.upper())
    return {"float": abi.R_JSONNUM, "double": abi.R_JSONNUM, "boolean": abi.R_BOOL, "date": abi.R_TIME, "datetime": abi.R_TIME, "timestamp": abi.R_TIME,
            "interval": abi.R_DURATION, "any": abi.R_JSON}.get(d, abi.R_BYTES if is_binary(ot) else abi.R_STRING)


def _has_string(v) -> bool:
    return (isinstance(v, str) and not isinstance(v, Num)) or (isinstance(v, list) and any(_has_string(x) for x in v))


def _depth_unsorted(v):
    """(container depth, some object's keys not strictly ascending) of a value whose objects are Pairs"""
    if isinstance(v, Pairs):
        keys = [k for k, _ in v]
        uns = any(not a.encode("utf-8") < b.encode("utf-8") for a, b in zip(keys, keys[1:]))
        sub = [_depth_unsorted(x) for _, x in v]
    elif isinstance(v, list):
        uns, sub = False, [_depth_unsorted(x) for x in v]
    else:
        return 0, False
    return 1 + max([d for d, _ in sub] or [0]), uns or any(u for _, u in sub)


def restore_cell(column: Column, text: bytes):
    """Restore(column, value) as an ABI cell (gotype, value), or Fallback(reason)"""
    col = column.col
    if col is None or col.get("type") not in DTYPES:
        raise Fallback("SCHEMA_COLUMN")
    d, ot = col["type"], col.get("original_type", "")
    if d == "any" and ot.startswith("mongo:bson"):
        raise Fallback("MONGO_BSON")
    v = _PairScanner(text).value()
    if v is None:
        return ("nil", None)
    is_str, is_num = isinstance(v, str) and not isinstance(v, Num), isinstance(v, Num)
    if isinstance(v, list) and d != "any":
        raise Fallback("VALUE_TYPE")
    ecol = E.Col(column.name, d, False, ot)
    if d in INT_RANGE or d == "interval":
        if is_str:
            raise Fallback("NUM_STRING" if d != "interval" else "VALUE_TYPE")
        if not is_num:
            raise Fallback("VALUE_TYPE")
        lo, hi = INT_RANGE["int64" if d == "interval" else d]
        if not _INT.match(v) or not (lo <= int(v) <= hi or (v.startswith("-") and int(v) == 0)):
            raise Fallback("INT_FORM")
        g, x = E.restore(ecol, E.JN(v))
        return ("duration", x) if d == "interval" else (g, x)
    if d in ("float", "double"):
        if not is_num:
            raise Fallback("NUM_STRING" if is_str else "VALUE_TYPE")
        return ("jsonnum", v.encode("ascii")) if d == "float" else E.restore(ecol, E.JN(v))   # no case "float" in Restore: the json.Number stays
    if d == "boolean":
        if not isinstance(v, bool):
            raise Fallback("VALUE_TYPE")
        return ("bool", v)
    if d in ("string", "utf8"):
        if is_binary(ot):
            if is_num and ot.startswith("mysql:bit"):
                raise Fallback("MYSQL_BIT")
            if not is_str:
                raise Fallback("STRING_NONSTRING")
            if not _B64.match(text[1:-1]):   # as it is spelled: an escaped spelling is left to the host
                raise Fallback("BASE64")
            return ("bytes", base64.b64decode(v))
        if not is_str:
            raise Fallback("STRING_NONSTRING")
        return E.restore(ecol, v)
    if d in ("date", "datetime", "timestamp"):
        if is_num:
            raise Fallback("TIME_FORM")
        if not is_str:
            raise Fallback("VALUE_TYPE")
        m = _TIME.match(text[1:-1].decode("latin-1"))   # as it is spelled: an escaped spelling is left to the host
        if not m:
            raise Fallback("TIME_FORM")
        if m.group(8) != "Z":
            raise Fallback("TIME_ZONE")
        y, mo, dd, hh, mi, ss = (int(m.group(i)) for i in range(1, 7))
        if not (1 <= mo <= 12 and 1 <= dd <= E._days_in_month(y, mo) and hh < 24 and mi < 60 and ss < 60):
            raise Fallback("TIME_FORM")
        g, (sec, ns, _off) = E.restore(ecol, v)
        return (g, (sec, ns))
    # any
    string_ok = ot == "mysql:json" or ot.startswith("ch:Decimal(") or ot.startswith("ch:Nullable(Decimal(") or (ot.startswith("pg:") and not ot.startswith("pg:timestamp"))
    if _has_string(v) and not string_ok:
        raise Fallback("ANY_PG_TIMESTAMP" if ot.startswith("pg:timestamp") else "ANY_STRING")
    if isinstance(v, (Pairs, list)):
        depth, uns = _depth_unsorted(v)
        if uns and depth > CANON_DEPTH:
            raise Fallback("DEPTH")
    return ("json", go_string_html(v) if is_str else marshal(plain(v)))


def _elements(text: bytes):
    """the texts of an array's elements"""
    sc = _Scanner(text)
    sc.p = 1
    out = []
    while True:
        sc.ws()
        if text[sc.p:sc.p + 1] == b"]":
            return out
        s = sc.p
        sc.value()
        out.append(text[s:sc.p])
        sc.ws()
        if text[sc.p:sc.p + 1] == b",":
            sc.p += 1


def restore_item(h: Header):
    """(value cells, OldKeys cells or None, schema) of one item; Fallback with the column"""
    cols = group_columns(h)
    if cols is None:
        raise Fallback("SCHEMA_COLUMN")
    vcols, kcols, schema = cols
    values, old = [], None
    for k, (c, t) in enumerate(zip(vcols, _elements(h.raw["columnvalues"]) if "columnvalues" in h.raw else [])):
        try:
            values.append(restore_cell(c, t))
        except Fallback as f:
            raise Fallback(f.reason, k)
    if h.kind != "insert" and "keyvalues" in h.old and kcols:
        old = []
        for k, (c, t) in enumerate(zip(kcols, _elements(h.old["keyvalues"][0]))):
            try:
                old.append(restore_cell(c, t))
            except Fallback as f:
                raise Fallback(f.reason, len(vcols) + k)
    return values, old, schema


# ---- the parser ----------------------------------------------------------------------------------------------------------------------------------------------------
class Group:
    def __init__(self, key, h: Header, schema):
        self.key = key
        self.ns, self.table, self.part = h.val.get("schema", ""), h.val.get("table", ""), h.val.get("part", "")
        self.names, self.key_names = list(h.val.get("columnnames", [])), list(h.old.get("keynames", (b"", []))[1])
        self.key_types = list(h.old.get("keytypes", (b"", []))[1])
        self.names_form = 1 if "columnnames" not in h.raw else 2 if not self.names else 0
        self.schema = schema              # [dict of tags]
        self.table_schema_json = h.raw.get("table_schema")
        self.rows = []                    # (kind, value cells, OldKeys cells or None, meta dict)

    def reprs(self):
        by_name = {}
        for c in self.schema:
            by_name[c.get("name", "")] = c
        return [repr_of(by_name[n]) for n in self.names], [repr_of(by_name[n]) for n in self.key_names], [by_name[n]["type"] for n in self.names + self.key_names]


class Result:
    def __init__(self):
        self.groups, self.items, self.fallback = [], [], []   # items: (message, group or -1, row or -1); fallback: (message, reason, item, column)


def parse(messages) -> Result:
    """messages: [bytes, or None for a nil value]"""
    res = Result()
    by_key = {}
    for m, msg in enumerate(messages):
        if msg is None:
            continue
        spans = cut(bytes(msg))
        if spans is None:
            res.fallback.append((m, "SYNTAX", -1, -1))
            continue
        parsed, problem, first_schema = [], None, {}
        for i, (s, e) in enumerate(spans):
            try:
                h = read_header(msg[s:e])
                tid = (h.val.get("schema", ""), h.val.get("table", ""))
                ts = h.raw.get("table_schema", b"")
                if first_schema.setdefault(tid, ts) != ts:
                    raise Fallback("SCHEMA_DIFFERS")
                values, old, schema = restore_item(h)
                parsed.append((h, values, old, schema))
            except Fallback as f:
                if problem is None:
                    problem = (m, f.reason, i, f.column)
                parsed.append(None)
        if problem:
            res.fallback.append(problem)
            res.items += [(m, -1, -1)] * len(spans)
            continue
        for h, values, old, schema in parsed:
            key = (h.val.get("schema", ""), h.val.get("table", ""), h.val.get("part", ""), h.raw.get("columnnames"), h.raw.get("table_schema"),
                   h.old.get("keynames", (None,))[0], h.old.get("keytypes", (None,))[0])
            if key not in by_key:
                by_key[key] = len(res.groups)
                res.groups.append(Group(key, h, schema))
            g = by_key[key]
            G = res.groups[g]
            res.items.append((m, g, len(G.rows)))
            G.rows.append((h.kind, values, old, {"id": h.id, "lsn": h.lsn, "commit_time": h.commit, "counter": h.counter,
                                                 "tx_id": h.val.get("tx_id", "").encode("utf-8"), "query": h.val.get("query", "").encode("utf-8")}))
    return res


# ---- a group as an abi.Batch ---------------------------------------------------------------------------------------------------------------------------------------
_GOTYPE = {abi.R_INT8: "int8", abi.R_INT16: "int16", abi.R_INT32: "int32", abi.R_INT64: "int64", abi.R_UINT8: "uint8", abi.R_UINT16: "uint16", abi.R_UINT32: "uint32",
           abi.R_UINT64: "uint64", abi.R_BOOL: "bool", abi.R_STRING: "string", abi.R_BYTES: "bytes", abi.R_JSONNUM: "jsonnum", abi.R_JSON: "json", abi.R_TIME: "time",
           abi.R_DURATION: "duration"}


def _column(name, dtype, r, cells):
    typed = [c if c[0] != "nil" else ["nil", None] for c in cells]
    if all(c[0] == "nil" for c in typed):   # column_from_values types a column by its cells: give it one of the right Go type, then cut it off
        filler = {"time": (0, 0)}.get(_GOTYPE[r], b"" if r in abi.VAR_REPRS else 0)
        col = abi.column_from_values(name, dtype, typed + [[_GOTYPE[r], filler]])
        n = len(typed)
        if r in abi.VAR_REPRS:
            col.offsets = col.offsets[:n + 1]
        else:
            col.values = col.values[:n]
            if col.nanos is not None:
                col.nanos = col.nanos[:n]
        col.validity = col.validity[:n]
        return col
    return abi.column_from_values(name, dtype, typed)


def group_batch(G: Group):
    """(abi.Batch with OldKeys, abi.Schema, meta dict of lists)"""
    vr, kr, dts = G.reprs()
    n = len(G.rows)
    cols = [_column(nm, dts[k], vr[k], [row[1][k] for row in G.rows]) for k, nm in enumerate(G.names)]
    b = abi.Batch(cols, n, G.ns, G.table)
    b.kind = __import__("numpy").array([abi.KIND_ID[row[0]] for row in G.rows], dtype="uint8")
    if G.key_names:
        nil = [("nil", None)] * len(G.key_names)
        b.old_keys = [_column(nm, dts[len(G.names) + k], kr[k], [(row[2] or nil)[k] for row in G.rows]) for k, nm in enumerate(G.key_names)]
        b.old_present = __import__("numpy").array([row[2] is not None for row in G.rows], dtype=bool)
    schema = abi.Schema([abi.ColSchema(c.get("name", ""), c.get("type", ""), c.get("key", False), c.get("path", ""), c.get("original_type", ""), c.get("required", False),
                                       c.get("table_schema", ""), c.get("table_name", ""), c.get("expression", ""), c.get("fake_key", False),
                                       marshal(c["properties"]).decode("utf-8") if c.get("properties") else "") for c in G.schema])
    b.schema = schema
    meta = {k: [row[3][k] for row in G.rows] for k in ("id", "lsn", "commit_time", "counter", "tx_id", "query")}
    meta["names_form"] = [G.names_form] * n
    return b, schema, meta
