"""raw_doc_grouper restated in plain Python (pkg/transformer/registry/raw_doc_grouper/raw_doc_grouper.go, raw_data_utils.go) over abi.Batch rows:
NewRawDocGroupTransformer's rules, Suitable, resultSchema / CollectFieldsForTransformer, collectParsedData, inPlaceRemoveOldKeys on Update rows, and a
json.Marshal of docData without HTML escaping that matches the ABI's `any` text (compact, members in byte order of the key).

A cell's JSON text is written out here, repr by repr, as encoding/json prints the Go value the ABI says the cell holds; floats go through the oracle's
floatEncoder, which is pinned to the serializer goldens.  A `_rest` cell held as `any` text that starts with '{' is the map[string]interface{} the
reference splices: its members are read with Python's json scanner, kept as their source text, and written into the same map the columns go into — so the
overwrite order on equal keys is the reference's own loop over ColumnNames, not a rule of this file."""
import base64
import datetime
import json
import re

import numpy as np

from transferia_amd import abi

ETL, DOC, REST = "etl_updated_at", "doc", "_rest"
SPECIAL = {ETL: "timestamp", DOC: "any"}
K_INSERT, K_UPDATE, K_DELETE = 0, 1, 2


# ---- NewRawDocGroupTransformer (raw_doc_grouper.go:195-236) ------------------------------------------------------------------------------------------
def factory(config):
    """-> (keys, fields); ValueError with the reference's text for what the constructor rejects"""
    keys = list(config.get("keys") or [])
    fields = list(config.get("fields") or [])
    for name in (ETL, DOC):
        if name not in keys and name not in fields:
            fields.append(name)
    if len(set(keys)) != len(keys):
        raise ValueError("Can't use same keys column names twice: " + ", ".join(keys))
    for k in keys:
        if k in fields:
            raise ValueError("Can't use same column as key and non-key : " + k)
    for rx in (config.get("tables") or {}).get("includeTables", []) + (config.get("tables") or {}).get("excludeTables", []):
        re.compile(rx)
    return keys, fields


def description(config):
    return "Return item as primary keys %s and json, containing the rest" % ", ".join(factory(config)[0])


def contains_all_fields(config, names):
    keys, fields = factory(config)
    return all(n in SPECIAL or n in names for n in keys + fields)   # allFieldsPresent (raw_data_utils.go:144-152)


def table_matches(config, ns, table):
    """MatchAnyTableNameVariant over filter.Filter (transformer_common.go:9-33, filter.go:27-44)"""
    t = config.get("tables") or {}
    inc, exc = t.get("includeTables") or [], t.get("excludeTables") or []
    if not inc and not exc:
        return True

    def dq(s):
        return '"' + s.replace('"', '""') + '"'

    def match(v):
        if any(re.search(x, v) for x in exc):
            return False
        return not inc or any(re.search(x, v) for x in inc)
    full = table if not ns else ns + "." + table
    fqtn = (dq(ns) + "." if ns else "") + (table if table == "*" else dq(table))
    return match(full) or match(fqtn)


def suitable(config, ns, table, schema):
    return table_matches(config, ns, table) and contains_all_fields(config, [c.name for c in schema.cols])


def result_schema(config, schema):
    """resultSchema (raw_doc_grouper.go:129-152): keys in config order with PrimaryKey set, then fields with it cleared; an existing column keeps every
    other ColSchema field; a stub's OriginalType is pg's when any input column's holds "pg:" """
    keys, fields = factory(config)
    pg = any("pg:" in c.original_type for c in schema.cols)
    index = {c.name: i for i, c in enumerate(schema.cols)}   # MakeMapColNameToIndex: the last of a repeated name
    out = []
    for names, is_key in ((keys, True), (fields, False)):
        for name in names:
            if name in index:
                c = schema.cols[index[name]]
                out.append(abi.ColSchema(c.name, c.dtype, is_key, c.path, c.original_type, c.required, c.table_schema, c.table_name, c.expression, c.fake_key, c.properties_json))
            elif name in SPECIAL:
                orig = "" if not pg else ("pg:json" if SPECIAL[name] == "any" else "pg:timestamp without time zone")
                out.append(abi.ColSchema(name, SPECIAL[name], is_key, "", orig))
    return abi.Schema(out)


# ---- json.Marshal without HTML escaping ----------------------------------------------------------------------------------------------------------------
def json_string(b: bytes) -> bytes:
    """encoding/json appendString(escapeHTML = false) of the Go string with these bytes"""
    out = bytearray(b'"')
    i, n = 0, len(b)
    short = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}
    while i < n:
        c = b[i]
        if c < 0x80:
            if c in short:
                out += short[c]
            elif c < 0x20:
                out += b"\\u00%02x" % c
            else:
                out.append(c)
            i += 1
            continue
        width = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 0
        try:
            ch = b[i:i + width].decode("utf-8") if width and i + width <= n else None   # (strict: no surrogates, no overlongs, nothing above U+10FFFF)
        except UnicodeDecodeError:
            ch = None
        if ch is None or len(ch) != 1:
            out += b"\\ufffd"
            i += 1
        elif ch in ("\u2028", "\u2029"):
            out += b"\\u%04x" % ord(ch)
            i += width
        else:
            out += b[i:i + width]
            i += width
    out += b'"'
    return bytes(out)


def rfc3339nano(sec: int, nsec: int) -> bytes:
    d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=int(sec))
    frac = ("." + ("%09d" % nsec).rstrip("0")) if nsec else ""
    return ("%04d-%02d-%02dT%02d:%02d:%02d%sZ" % (d.year, d.month, d.day, d.hour, d.minute, d.second, frac)).encode()


def cell_json(oracle, col, i) -> bytes:
    """json.Marshal of the Go value in row i of `col`: what emit_json_cell(any_as_string = 0, html = false) stands for"""
    if col.validity is not None and not col.validity[i]:
        return b"null"
    r = col.repr
    if r == abi.R_STRING:
        return json_string(col.get_bytes(i))
    if r == abi.R_BYTES:
        return b'"' + base64.b64encode(col.get_bytes(i)) + b'"'
    if r == abi.R_JSONNUM:
        return col.get_bytes(i) or b"0"
    if r == abi.R_JSON:
        return col.get_bytes(i)
    if r == abi.R_TIME:
        return b'"' + rfc3339nano(int(col.values[i]), int(col.nanos[i]) if col.nanos is not None else 0) + b'"'
    if r == abi.R_BOOL:
        return b"true" if col.values[i] else b"false"
    if r in (abi.R_FLOAT32, abi.R_FLOAT64):
        return oracle.json_float(float(col.values[i]), 32 if r == abi.R_FLOAT32 else 64).encode()
    return str(int(col.values[i])).encode()   # the integers and time.Duration (an int64)


def rest_members(text: bytes):
    """[(decoded key, the member's value as its source text)] of a JSON object text, in source order"""
    s = text.decode("utf-8")
    dec = json.JSONDecoder()
    ws = re.compile(r"[ \t\r\n]*")
    pos = ws.match(s, 1).end()
    out = []
    if s[pos] == "}":
        return out
    while True:
        key, pos = dec.raw_decode(s, pos)
        assert isinstance(key, str)
        pos = ws.match(s, pos).end()
        assert s[pos] == ":"
        pos = ws.match(s, pos + 1).end()
        _, end = dec.raw_decode(s, pos)
        out.append((key, s[pos:end].encode("utf-8")))
        pos = ws.match(s, end).end()
        if s[pos] == "}":
            return out
        assert s[pos] == ","
        pos = ws.match(s, pos + 1).end()


def listed(col, i) -> bool:
    return col.absent is None or not col.absent[i]


def doc_of_row(oracle, batch, i) -> bytes:
    """json.Marshal(docData) of row i (collectParsedData, raw_doc_grouper.go:158-193): the loop over the row's ColumnNames in batch order"""
    doc = {}
    for col in batch.cols:
        if not listed(col, i):
            continue
        valid = col.validity is None or col.validity[i]
        if col.name == REST and col.repr == abi.R_JSON and valid and col.get_bytes(i)[:1] == b"{":   # restMap, ok := colValue.(map[string]interface{})
            for k, v in rest_members(col.get_bytes(i)):
                doc[k.encode("utf-8")] = v
        else:
            doc[col.name.encode("utf-8")] = cell_json(oracle, col, i)
    return b"{" + b",".join(json_string(k) + b":" + doc[k] for k in sorted(doc)) + b"}"


# ---- Apply ---------------------------------------------------------------------------------------------------------------------------------------
def etl_time(commit_time: int):
    """time.Unix(0, int64(atime)) as (seconds, nanoseconds)"""
    v = int(commit_time) & 0xFFFFFFFFFFFFFFFF
    if v >= 1 << 63:
        v -= 1 << 64
    return v // 1000000000, v % 1000000000


def batch_schema(batch):
    s = getattr(batch, "schema", None)
    return s if s is not None else abi.Schema([abi.ColSchema(c.name, c.dtype) for c in batch.cols])


def apply(oracle, config, batch, commit_time=None):
    """Apply over the rows of `batch` -> (the transformed rows as a Batch with .schema, the indices of the rows that became errors).
    commit_time: uint64 per INPUT row (row i reads entry src_row[i]), None = zero."""
    keys, fields = factory(config)
    n = batch.nrows
    schema = batch_schema(batch)
    if not contains_all_fields(config, [c.name for c in schema.cols]):
        empty = abi.Batch([], 0, batch.table_ns, batch.table_name)
        return empty, list(range(n))
    kept = [c for c in batch.cols if c.name in keys or c.name in fields]
    src = batch.src_row if batch.src_row is not None else np.arange(n, dtype=np.int32)
    times = [etl_time(0 if commit_time is None else commit_time[int(src[i])]) for i in range(n)]
    etl = abi.Column(ETL, "timestamp", abi.R_TIME, values=np.array([t[0] for t in times], np.int64), nanos=np.array([t[1] for t in times], np.int32))
    docs = [doc_of_row(oracle, batch, i) for i in range(n)]
    off = np.zeros(n + 1, np.uint32)
    if n:
        off[1:] = np.cumsum([len(d) for d in docs])
    doc = abi.Column(DOC, "any", abi.R_JSON, offsets=off, data=np.frombuffer(b"".join(docs), np.uint8).copy())
    out = abi.Batch(kept + [etl, doc], n, batch.table_ns, batch.table_name, batch.kind, src.astype(np.int32), batch.part_id)
    out.schema = result_schema(config, schema)
    # inPlaceRemoveOldKeys(&item.OldKeys, item.ColumnNames) for Update rows (raw_data_utils.go:87-95, 127-142); shouldUpdateOldKeys is off
    old = list(getattr(batch, "old_keys", None) or [])
    if old:
        pres = np.asarray(getattr(batch, "old_present", None), bool) if getattr(batch, "old_present", None) is not None else np.ones(n, bool)
        kinds = batch.kind if batch.kind is not None else np.zeros(n, np.uint8)
        names_after = [c.name for c in kept] + [ETL, DOC]
        per_row = [[c.name for c in old if (kinds[i] != K_UPDATE or c.name in names_after)] if pres[i] else None for i in range(n)]
        lists = {tuple(x) for x in per_row if x is not None}
        if len(lists) > 1:
            raise NotImplementedError("ragged OldKeys: rows of one batch would carry different KeyNames")
        names = list(lists.pop()) if lists else [c.name for c in old]
        out.old_keys = [c for c in old if c.name in names]
        if out.old_keys:
            out.old_present = pres
    return out, []
