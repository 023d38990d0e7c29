"""Plain-Python restatement of the raw_to_table parser (pkg/parsers/registry/raw_to_table/engine/parser.go, pkg/util/raw_to_table_common,
pkg/util/dlq_maker/queue_dlq_maker) — what tests/test_rawtable_ref.py checks against the reference's own test vectors and tests/test_gpu_rawtable.py holds
the device to.  Nothing here imports the library.

Python's json is not encoding/json (it takes NaN / Infinity, refuses invalid UTF-8, has its own depth limit), so the scanner grammar, the decode
(UseNumber, the last of a repeated key, invalid UTF-8 -> U+FFFD) and json.Marshal are written out."""
import json

from rawdoc_ref import json_string  # encoding/json appendString without HTML escaping

TYPES = ("bytes", "string", "json")
MAX_DEPTH, CANON_DEPTH = 128, 16   # include/tfgpu.h: deeper JSON / deeper JSON with unsorted keys is left to the stock parser
KEYS = ("TableName", "IsKeyEnabled", "KeyType", "ValueType", "IsTimestampEnabled", "IsHeadersEnabled", "DLQSuffix")


class ConfigError(ValueError):
    pass


class HostFallback(Exception):
    """the device does not decide this message"""


def config(c: dict) -> dict:
    """CommonConfig from either parser config (the Lb form has no key) + Validate"""
    out = {"TableName": c.get("TableName", ""), "IsKeyEnabled": bool(c.get("IsKeyEnabled", False)), "KeyType": c.get("KeyType", ""),
           "ValueType": c.get("ValueType", ""), "IsTimestampEnabled": bool(c.get("IsTimestampEnabled", False)),
           "IsHeadersEnabled": bool(c.get("IsHeadersEnabled", False)), "DLQSuffix": c.get("DLQSuffix", "")}
    if out["IsKeyEnabled"] and out["KeyType"] not in TYPES:
        raise ConfigError("invalid parser config - unsupported key type: %s" % out["KeyType"])
    if out["ValueType"] not in TYPES:
        raise ConfigError("invalid parser config - unsupported value type: %s" % out["ValueType"])
    return out


def dlq_config(c: dict) -> dict:
    return dict(c, IsKeyEnabled=True, KeyType="bytes", ValueType="bytes", IsTimestampEnabled=True, IsHeadersEnabled=True)


def schema(c: dict, dlq: bool):
    """BuildTableSchemaAndColumnNames: [name, DataType, PrimaryKey, Required]"""
    if dlq:
        c = dlq_config(c)
    yt = {"bytes": "string", "string": "utf8", "json": "any"}
    cols = [["topic", "utf8", True, True], ["partition", "uint32", True, True], ["offset", "uint32", True, True]]
    if c["IsTimestampEnabled"]:
        cols.append(["timestamp", "timestamp", False, True])
    if c["IsHeadersEnabled"]:
        cols.append(["headers", "any", False, False])
    if c["IsKeyEnabled"]:
        cols.append(["key", yt[c["KeyType"]], False, False])
    cols.append(["value", yt[c["ValueType"]], False, False])
    if dlq:
        cols.append(["failure_reason", "utf8", False, False])
    return cols


def table_name(c: dict, dlq: bool, topic: str) -> str:
    base = c["TableName"] or topic
    return base + (c["DLQSuffix"] or "_dlq") if dlq else base   # a suffix without '_' is appended as it stands


def utf8_valid(b: bytes) -> bool:
    try:
        b.decode("utf-8")   # strict: no overlongs, no surrogates, nothing above U+10FFFF, nothing cut short
        return True
    except UnicodeDecodeError:
        return False


# ---- encoding/json: scanner.go's grammar, decode.go's unquote, UseNumber -----------------------------------------------------------------------------
class Num(str):
    """json.Number: the literal's text"""


class _Bad(Exception):
    pass


WS = b" \t\r\n"


class _Scanner:
    def __init__(self, b: bytes):
        self.b, self.p, self.depth, self.maxdepth, self.sorted = b, 0, 0, 0, True

    def ws(self):
        while self.p < len(self.b) and self.b[self.p] in WS:
            self.p += 1

    def value(self):
        self.ws()
        if self.p >= len(self.b):
            raise _Bad()
        c = self.b[self.p:self.p + 1]
        if c in (b"{", b"["):
            if self.depth == MAX_DEPTH:
                raise HostFallback()
            self.depth += 1
            self.maxdepth = max(self.maxdepth, self.depth)
            self.p += 1
            v = self.obj() if c == b"{" else self.arr()
            self.depth -= 1
            return v
        if c == b'"':
            return self.string()
        if c == b"-" or c.isdigit():
            return self.number()
        for lit, v in ((b"true", True), (b"false", False), (b"null", None)):
            if self.b.startswith(lit, self.p):
                self.p += len(lit)
                return v
        raise _Bad()

    def obj(self):
        out, prev = {}, None
        self.ws()
        if self.b[self.p:self.p + 1] == b"}":
            self.p += 1
            return out
        while True:
            self.ws()
            if self.b[self.p:self.p + 1] != b'"':
                raise _Bad()
            k = self.string()
            if prev is not None and not prev < k:   # (code point order = the order of the UTF-8 bytes)
                self.sorted = False
            prev = k
            self.ws()
            if self.b[self.p:self.p + 1] != b":":
                raise _Bad()
            self.p += 1
            v = self.value()
            out.pop(k, None)
            out[k] = v   # the last of a repeated key stays
            self.ws()
            d = self.b[self.p:self.p + 1]
            self.p += 1
            if d == b"}":
                return out
            if d != b",":
                raise _Bad()

    def arr(self):
        out = []
        self.ws()
        if self.b[self.p:self.p + 1] == b"]":
            self.p += 1
            return out
        while True:
            out.append(self.value())
            self.ws()
            d = self.b[self.p:self.p + 1]
            self.p += 1
            if d == b"]":
                return out
            if d != b",":
                raise _Bad()

    def number(self):
        b, s = self.b, self.p

        def digits():
            q = self.p
            while self.p < len(b) and 0x30 <= b[self.p] <= 0x39:
                self.p += 1
            return self.p > q
        if b[self.p:self.p + 1] == b"-":
            self.p += 1
        if b[self.p:self.p + 1] == b"0":
            self.p += 1
        elif not digits():
            raise _Bad()
        if b[self.p:self.p + 1] == b".":
            self.p += 1
            if not digits():
                raise _Bad()
        if b[self.p:self.p + 1] in (b"e", b"E"):
            self.p += 1
            if b[self.p:self.p + 1] in (b"+", b"-"):
                self.p += 1
            if not digits():
                raise _Bad()
        return Num(b[s:self.p].decode("ascii"))

    def hex4(self, at):
        h = self.b[at:at + 4]
        if len(h) != 4 or any(x not in b"0123456789abcdefABCDEF" for x in h):
            return None
        return int(h, 16)

    def string(self) -> str:
        b = self.b
        self.p += 1
        out = []
        while True:
            if self.p >= len(b):
                raise _Bad()
            c = b[self.p]
            if c == 0x22:
                self.p += 1
                return "".join(out)
            if c < 0x20:
                raise _Bad()
            if c == 0x5C:
                e = b[self.p + 1:self.p + 2]
                if e == b"u":
                    r = self.hex4(self.p + 2)
                    if r is None:
                        raise _Bad()
                    self.p += 6
                    if 0xD800 <= r < 0xE000:
                        r2 = self.hex4(self.p + 2) if b[self.p:self.p + 2] == b"\\u" else None
                        if r < 0xDC00 and r2 is not None and 0xDC00 <= r2 < 0xE000:
                            self.p += 6
                            r = 0x10000 + ((r - 0xD800) << 10) + (r2 - 0xDC00)
                        else:
                            r = 0xFFFD
                    out.append(chr(r))
                    continue
                m = {b'"': '"', b"\\": "\\", b"/": "/", b"b": "\b", b"f": "\f", b"n": "\n", b"r": "\r", b"t": "\t"}
                if e not in m:
                    raise _Bad()
                out.append(m[e])
                self.p += 2
                continue
            if c < 0x80:
                out.append(chr(c))
                self.p += 1
                continue
            w = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 0
            try:
                ch = b[self.p:self.p + w].decode("utf-8") if w and self.p + w <= len(b) else None
            except UnicodeDecodeError:
                ch = None
            if ch is None or len(ch) != 1:
                out.append(chr(0xFFFD))
                self.p += 1
            else:
                out.append(ch)
                self.p += w


def json_decode(b: bytes):
    """(valid, value, max container depth, every object's keys strictly ascending) — json.Valid + jsonx.Unmarshal into `any`.
    Raises HostFallback for nesting beyond MAX_DEPTH."""
    s = _Scanner(b)
    try:
        v = s.value()
        s.ws()
        if s.p != len(b):
            raise _Bad()
    except _Bad:
        return False, None, 0, True
    return True, v, s.maxdepth, s.sorted


def go_string_html(s: str) -> bytes:
    """encoding/json appendString with escapeHTML (json.Marshal's default) of a VALID string"""
    t = json_string(s.encode("utf-8"))
    return t.replace(b"<", b"\\u003c").replace(b">", b"\\u003e").replace(b"&", b"\\u0026")


def go_bytes_html(b: bytes) -> bytes:
    """the same for a Go string holding any bytes: an invalid byte is the escape \\ufffd (rawdoc_ref.json_string)"""
    return json_string(b).replace(b"<", b"\\u003c").replace(b">", b"\\u003e").replace(b"&", b"\\u0026")


def marshal(v) -> bytes:
    """json.Marshal of a value decoded by json_decode: compact, map keys ascending"""
    if v is None:
        return b"null"
    if v is True:
        return b"true"
    if v is False:
        return b"false"
    if isinstance(v, Num):
        return v.encode("ascii")
    if isinstance(v, str):
        return go_string_html(v)
    if isinstance(v, list):
        return b"[" + b",".join(marshal(x) for x in v) + b"]"
    return b"{" + b",".join(go_string_html(k) + b":" + marshal(v[k]) for k in sorted(v)) + b"}"


def marshal_headers(h) -> bytes:
    """json.Marshal(map[string]string): keys in byte order; a nil map is `null`"""
    if h is None:
        return b"null"
    raw = lambda x: x.encode("utf-8") if isinstance(x, str) else bytes(x)  # noqa: E731
    m = {}
    for k, v in (h.items() if isinstance(h, dict) else h):
        m[raw(k)] = raw(v)   # the later pair of a repeated key stands
    return b"{" + b",".join(go_bytes_html(k) + b":" + go_bytes_html(m[k]) for k in sorted(m)) + b"}"


# ---- the parser ----------------------------------------------------------------------------------------------------------------------------------------
def dlq_reason(c: dict, key, value) -> str:
    """sendToDLQReason; raises HostFallback"""
    parts, fallback = [], False

    def check(want, b, who):
        nonlocal fallback
        if want == "string" and not utf8_valid(b or b""):
            parts.append(who + " is configured as string, but it isn't valid UTF-8")
        elif want == "json" and b is not None:
            try:
                ok, _, depth, srt = json_decode(b)
            except HostFallback:
                fallback = True
                return
            if not ok:
                parts.append(who + " is configured as JSON, but it isn't valid JSON")
            elif not srt and depth > CANON_DEPTH:
                fallback = True
    if c["IsKeyEnabled"]:
        check(c["KeyType"], key, "key")
    check(c["ValueType"], value, "value")
    if fallback:
        raise HostFallback()
    return "|".join(parts)


def cell(kind: str, b):
    """appendProperType as a typed cell: None, ("utf8", bytes), ("bytes", bytes), ("any", json.Marshal text)"""
    if b is None:
        return None
    if kind == "string":
        return ("utf8", bytes(b))
    if kind == "bytes":
        return ("bytes", bytes(b))
    v = json_decode(b)[1]
    return None if v is None else ("any", marshal(v))   # a nil interface


def row(c: dict, topic: str, partition: int, msg, reason=None):
    """BuildColumnValues (+ failure_reason): the cells in column order"""
    off, wt, key, value, headers = msg
    out = [("utf8", topic.encode("utf-8")), ("u32", partition), ("u32", off & 0xFFFFFFFF)]
    if c["IsTimestampEnabled"]:
        out.append(("time", (wt // 10**9, wt % 10**9)))
    if c["IsHeadersEnabled"]:
        out.append(("any", marshal_headers(headers)))
    if c["IsKeyEnabled"]:
        out.append(cell(c["KeyType"], key))
    out.append(cell(c["ValueType"], value))
    if reason is not None:
        out.append(("utf8", reason.encode("utf-8")))
    return out


def do_batch(c: dict, topic: str, partition: int, msgs):
    """DoBatch: (main [(message index, cells)], dead-letter [(message index, cells)], [message indexes left to the stock parser])"""
    main, dlq, fb = [], [], []
    for i, m in enumerate(msgs):
        try:
            why = dlq_reason(c, m[2], m[3])
        except HostFallback:
            fb.append(i)
            continue
        if why:
            dlq.append((i, row(dlq_config(c), topic, partition, m, why)))
        else:
            main.append((i, row(c, topic, partition, m)))
    return main, dlq, fb


# ---- the golden file's notation --------------------------------------------------------------------------------------------------------------------------
def golden_message(m: dict):
    unhex = lambda x: None if x is None else bytes.fromhex(x)  # noqa: E731
    return (m["offset"], m["write_time_ns"], unhex(m["key"]), unhex(m["value"]), m["headers"])


def golden_cell(v):
    if v is None:
        return None
    (k, x), = v.items()
    if k == "utf8":
        return ("utf8", x.encode("utf-8"))
    if k == "bytes":
        return ("bytes", bytes.fromhex(x))
    if k == "u32":
        return ("u32", x)
    if k == "time_ns":
        return ("time", (x // 10**9, x % 10**9))
    if k == "headers":
        return ("any", marshal_headers(x))
    assert k == "any"
    return ("any", x.encode("utf-8"))


def load_golden(path):
    with open(path, encoding="utf-8") as f:
        return json.load(f)
