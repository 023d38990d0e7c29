"""filter_rows_by_ids restated in plain Python (pkg/transformer/registry/filter_rows_by_ids/filter_rows_by_ids.go) over abi.Batch rows: the
constructor's rules, Suitable, shouldKeep and isIDAllowed.  Written from the Go, line by line, with no eye on the device code.

What a cell is to the Go code: R_STRING a `string`, R_BYTES a `[]byte`, R_JSON the value encoding/json decoded from the text (a `string` only where
the text is a JSON string: go_unquote below is encoding/json's unquote), R_JSONNUM a json.Number (no case of the type switch), everything else a
number, bool or time.  A nil has no case either; an ABSENT cell has no entry in AsMap().  A device batch cannot hold a provider_mongo.DValue, so
the `document` branch always `continue`s here — the device refuses such a batch by name instead (MONGO_REFUSAL)."""
import re

import numpy as np

from transferia_amd import abi

T = "filter_rows_by_ids"
DESCRIPTION = "Row filter by allowed IDs"
DOCUMENT = "document"
MONGO_REFUSAL = "Mongo `document` columns stay with the stock transformer"
K_INSERT, K_UPDATE = 0, 1


# ---- NewFilterRowsByIDsTransformer (:42-72) ------------------------------------------------------------------------------------------------------
def _raw(s):
    return s if isinstance(s, bytes) else s.encode("utf-8")


def factory(config):
    """-> AllowedIDPrefixesByLength {length: set of ids}; ValueError with the reference's text for what the constructor rejects"""
    for part, inc, exc, what in (("tables", "includeTables", "excludeTables", "tables"), ("columns", "includeColumns", "excludeColumns", "columns")):
        f = config.get(part) or {}
        for rx in (f.get(inc) or []) + (f.get(exc) or []):
            try:
                re.compile(rx)
            except re.error as e:
                raise ValueError("unable to create %s filter: %s" % (what, e))
    ids = config.get("allowedIDs") or []
    if len(ids) == 0:
        raise ValueError("list of allowed IDs shouldn't be empty")
    by_len = {}
    for i in ids:
        by_len.setdefault(len(_raw(i)), set()).add(_raw(i))
    return by_len


def _match(inc, exc, v):   # filter.Filter.Match (filter.go:27-44)
    if any(re.search(x, v) for x in exc):
        return False
    return not inc or any(re.search(x, v) for x in inc)


def column_matches(config, name):
    c = config.get("columns") or {}
    return _match(c.get("includeColumns") or [], c.get("excludeColumns") or [], name)


def table_matches(config, ns, table):
    """MatchAnyTableNameVariant (transformer_common.go:9-33)"""
    t = config.get("tables") or {}
    inc, exc = t.get("includeTables") or [], t.get("excludeTables") or []
    if not inc and not exc:
        return True

    def dq(s):
        return '"' + s.replace('"', '""') + '"'
    full = table if not ns else ns + "." + table
    fqtn = (dq(ns) + "." if ns else "") + (table if table == "*" else dq(table))
    return _match(inc, exc, full) or _match(inc, exc, fqtn)


def is_mongo_document(name, dtype):       # :186-188
    return name == DOCUMENT and dtype == "any"


def column_suitable(config, name, dtype):  # :190-196 (ytschema: TypeString "utf8", TypeBytes "string", TypeAny "any")
    return dtype in ("utf8", "string", "any") and column_matches(config, name)


def suitable(config, ns, table, schema):   # :170-184
    if not table_matches(config, ns, table):
        return False
    return any(column_suitable(config, c.name, c.dtype) or is_mongo_document(c.name, c.dtype) for c in schema.cols)


# ---- isIDAllowed (:156-168) ------------------------------------------------------------------------------------------------------------------------
def is_id_allowed(by_len, value: bytes) -> bool:
    for length, prefixes in by_len.items():
        if length > len(value):
            continue
        if value[:length] in prefixes:
            return True
    return False


# ---- encoding/json unquote (decode.go unquoteBytes) ---------------------------------------------------------------------------------------------------
def _getu4(s, r):
    if len(s) - r < 6 or s[r:r + 2] != b"\\u":
        return -1
    h = s[r + 2:r + 6]
    return int(h, 16) if re.fullmatch(rb"[0-9a-fA-F]{4}", h) else -1


def _decode_rune(s, r):
    """utf8.DecodeRune -> (rune, size); (0xFFFD, 1) for what is not well-formed"""
    c = s[r]
    if c < 0x80:
        return c, 1
    for size in (2, 3, 4):
        try:
            ch = s[r:r + size].decode("utf-8")   # strict: no surrogates, no overlongs, nothing past U+10FFFF
        except UnicodeDecodeError:
            continue
        if len(ch) == 1:
            return ord(ch), size
    return 0xFFFD, 1


def go_unquote(text: bytes):
    """the bytes of the Go string the JSON string `text` (quotes included) decodes to; None where unquote gives up"""
    if len(text) < 2 or text[:1] != b'"' or text[-1:] != b'"':
        return None
    s = text[1:-1]
    out = bytearray()
    r = 0
    short = {ord('"'): b'"', ord("\\"): b"\\", ord("/"): b"/", ord("'"): b"'", ord("b"): b"\b", ord("f"): b"\f", ord("n"): b"\n", ord("r"): b"\r", ord("t"): b"\t"}
    while r < len(s):
        c = s[r]
        if c == ord("\\"):
            r += 1
            if r >= len(s):
                return None
            if s[r] == ord("u"):
                r -= 1
                rr = _getu4(s, r)
                if rr < 0:
                    return None
                r += 6
                if 0xD800 <= rr < 0xE000:                       # utf16.IsSurrogate
                    rr1 = _getu4(s, r)
                    if rr < 0xDC00 and 0xDC00 <= rr1 < 0xE000:  # utf16.DecodeRune gives a rune
                        r += 6
                        out += chr(0x10000 + ((rr - 0xD800) << 10) + (rr1 - 0xDC00)).encode("utf-8")
                        continue
                    rr = 0xFFFD                                 # invalid surrogate; fall back to replacement rune
                out += chr(rr).encode("utf-8")
                continue
            if s[r] not in short:
                return None
            out += short[s[r]]
            r += 1
        elif c == ord('"') or c < 0x20:
            return None
        elif c < 0x80:
            out.append(c)
            r += 1
        else:                                                   # coerce to well-formed UTF-8
            rr, size = _decode_rune(s, r)
            r += size
            out += chr(rr).encode("utf-8")
    return bytes(out)


def json_text_as_string(text: bytes):
    """the Go string inside an `any` decoded from this JSON text, or None where the value is no string"""
    t = text.strip(b" \t\r\n")
    if t[:1] != b'"':
        return None
    return go_unquote(t)


# ---- shouldKeep (:92-130) --------------------------------------------------------------------------------------------------------------------------
def batch_schema(batch):
    s = getattr(batch, "schema", None)
    return s if s is not None else abi.Schema([abi.ColSchema(c.name, c.dtype) for c in batch.cols])


def as_map(batch, i):
    """ChangeItem.AsMap() of row i: {name: column}; the last column listing a name wins; a row without ColumnNames (a Delete, a non-row kind) has none"""
    kind = K_INSERT if batch.kind is None else int(batch.kind[i])
    if kind not in (K_INSERT, K_UPDATE):
        return {}
    return {c.name: c for c in batch.cols if c.absent is None or not c.absent[i]}


def cell_string(col, i):
    """the value as the type switch of shouldKeep sees it: its bytes for a string / []byte, None for everything that `continue`s"""
    if col.validity is not None and not col.validity[i]:
        return None
    if col.repr in (abi.R_STRING, abi.R_BYTES):
        return col.get_bytes(i)
    if col.repr == abi.R_JSON:
        return json_text_as_string(col.get_bytes(i))
    return None


def should_keep(config, by_len, batch, schema, i) -> bool:
    m = as_map(batch, i)
    for cs in schema.cols:
        if is_mongo_document(cs.name, cs.dtype):
            continue                       # processMongoDocument: no DValue in a device batch
        if not column_suitable(config, cs.name, cs.dtype):
            continue
        col = m.get(cs.name)
        if col is None:
            continue
        v = cell_string(col, i)
        if v is None:
            continue
        if is_id_allowed(by_len, v):
            return True
    return False


def kept_rows(config, batch):
    """Apply: the indices of the rows of `batch` that stay, ascending"""
    by_len = factory(config)
    schema = batch_schema(batch)
    return [i for i in range(batch.nrows) if should_keep(config, by_len, batch, schema, i)]


# ---- the kept rows as a batch (what the device's result downloads to) -------------------------------------------------------------------------------
def take_column(c, idx):
    idx = np.asarray(idx, dtype=np.int64)
    o = abi.Column(c.name, c.dtype, c.repr)
    if c.repr in abi.VAR_REPRS:
        cells = [c.get_bytes(int(i)) for i in idx]
        o.offsets = np.zeros(len(idx) + 1, np.uint32)
        if len(idx):
            o.offsets[1:] = np.cumsum([len(x) for x in cells])
        o.data = np.frombuffer(b"".join(cells), np.uint8).copy()
    else:
        o.values = np.asarray(c.values)[idx]
        if c.nanos is not None:
            o.nanos = np.asarray(c.nanos)[idx]
    if c.validity is not None:
        o.validity = np.asarray(c.validity, bool)[idx]
    if c.absent is not None:
        o.absent = np.asarray(c.absent, bool)[idx]
    return o


def take_rows(batch, idx):
    idx = [int(i) for i in idx]
    out = abi.Batch([take_column(c, idx) for c in batch.cols], len(idx), batch.table_ns, batch.table_name)
    src = batch.src_row if batch.src_row is not None else np.arange(batch.nrows, dtype=np.int32)
    out.src_row = np.asarray(src, np.int32)[idx] if idx else np.zeros(0, np.int32)
    out.kind = None if batch.kind is None else np.asarray(batch.kind, np.uint8)[idx]
    out.part_id = None if batch.part_id is None else np.asarray(batch.part_id, np.uint32)[idx]
    old = list(getattr(batch, "old_keys", None) or [])
    if old:
        out.old_keys = [take_column(c, idx) for c in old]
        pres = getattr(batch, "old_present", None)
        out.old_present = (np.asarray(pres, bool) if pres is not None else np.ones(batch.nrows, bool))[idx]
    if getattr(batch, "schema", None) is not None:
        out.schema = batch.schema
    return out


def apply(config, batch):
    """-> (the kept rows as a Batch, their indices in `batch`)"""
    idx = kept_rows(config, batch)
    return take_rows(batch, idx), idx
