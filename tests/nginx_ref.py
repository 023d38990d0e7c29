"""A plain-Python restatement of the reference's nginx access-log reader (pkg/providers/s3/reader/registry/nginx): tokenizeFormat,
compileFormat, parseEntry, matchLiteral, findDelimiter (nginx_format.go), the line loop of Read (reader_nginx.go:101-189),
checkUnexpectedFields, convertNginxValue (reader_nginx_funcs.go), constructCI (reader_nginx.go:217-279) and the schema resolver
(nginx_schema_resolver.go:52-101).  Everything works on bytes, so offsets agree with Go's.  The time layout is oracle.time_parse's and
the typing is oracle.strictify's; nothing here is shared with the product."""
import re

from transferia_amd import abi

TIME_LOCAL_LAYOUT = "02/Jan/2006:15:04:05 -0700"
_VAR_RE = re.compile(rb"\$([A-Za-z0-9_]+)")
_COLLAPSE_RE = re.compile(rb"[ \t]*\n[ \t]*")
# unicode.IsSpace (White_Space property)
_SPACE_RUNES = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | set(range(0x2000, 0x200B))


def _rune_at(b: bytes, i: int):
    """utf8.DecodeRune(b[i:]) -> (rune, width); an invalid sequence is (0xFFFD, 1)"""
    c = b[i]
    if c < 0x80:
        return c, 1
    w = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 0
    if w and i + w <= len(b):
        try:
            return ord(b[i:i + w].decode("utf-8")), w
        except UnicodeDecodeError:
            pass
    return 0xFFFD, 1


def _last_rune(b: bytes, end: int):
    """utf8.DecodeLastRune(b[:end])"""
    for w in range(1, 5):
        s = end - w
        if s < 0:
            break
        if (b[s] & 0xC0) != 0x80:  # a start byte
            r, wd = _rune_at(b[:end], s)
            if s + wd == end:
                return r, wd
            break
    return 0xFFFD, 1


def trim_space(b: bytes) -> bytes:
    """strings.TrimSpace"""
    a, e = 0, len(b)
    while a < e:
        r, w = _rune_at(b, a)
        if r not in _SPACE_RUNES:
            break
        a += w
    while e > a:
        r, w = _last_rune(b, e)
        if r not in _SPACE_RUNES or e - w < a:
            break
        e -= w
    return b[a:e]


def tokenize_format(fmt: bytes):
    fmt = _COLLAPSE_RE.sub(b" ", trim_space(fmt))
    tokens, last = [], 0
    for m in _VAR_RE.finditer(fmt):
        if m.start() > last:
            tokens.append((False, fmt[last:m.start()]))
        tokens.append((True, m.group(1)))
        last = m.end()
    if last < len(fmt):
        tokens.append((False, fmt[last:]))
    return tokens


class Compiled:
    def __init__(self, tokens, fields):
        self.tokens, self.fields = tokens, fields

    def next_delimiter(self, after: int) -> bytes:
        for isv, v in self.tokens[after + 1:]:
            if not isv and len(v):
                return v
        return b""

    def schema(self):
        return [abi.ColSchema(f.decode(), "utf8", False, str(i), "nginx:utf8") for i, f in enumerate(self.fields)]


def compile_format(fmt: bytes) -> Compiled:
    tokens = tokenize_format(fmt)
    if not tokens:
        raise ValueError("No tokens found in format")
    if not any(isv for isv, _ in tokens):
        raise ValueError("No variable found in format")
    fields, used = [], {}
    for isv, v in tokens:
        if not isv:
            continue
        used[v] = used.get(v, 0) + 1
        fields.append(v if used[v] == 1 else v + b"_%d" % used[v])
    return Compiled(tokens, fields)


def match_literal(inp: bytes, lit: bytes) -> int:
    p = 0
    for lch in lit:
        if p >= len(inp):
            return -1
        if lch == 0x20:
            if inp[p] not in (0x20, 0x09):
                return -1
            while p < len(inp) and inp[p] in (0x20, 0x09):
                p += 1
        else:
            if inp[p] != lch:
                return -1
            p += 1
    return p


def find_delimiter(inp: bytes, delim: bytes) -> int:
    i = 0
    while i < len(inp):
        if inp[i] == 0x5C and not (i + 1 < len(inp) and inp[i + 1] == 0x0A):
            i += 2
            continue
        if match_literal(inp[i:], delim) >= 0:
            return i
        i += 1
    return -1


def index_of_newline(s: bytes) -> int:
    for i, c in enumerate(s):
        if c in (0x0A, 0x0D):
            return i
    return -1


def parse_entry(c: Compiled, inp: bytes):
    """-> (values, consumed), or None on a format error"""
    values, pos = [], 0
    for i, (isv, v) in enumerate(c.tokens):
        if not isv:
            n = match_literal(inp[pos:], v)
            if n < 0:
                return None
            pos += n
            continue
        d = c.next_delimiter(i)
        if d == b"":
            end = index_of_newline(inp[pos:])
            if end < 0:
                end = len(inp) - pos
        else:
            end = find_delimiter(inp[pos:], d)
            if end < 0:
                return None
        values.append(inp[pos:pos + end])
        pos += end
    return values, pos


def has_unexpected_fields(line: bytes, consumed: int) -> bool:
    return consumed < len(line) and trim_space(line[consumed:]) != b""


def resolve_schema(c: Compiled, output_schema=None, hide_system_cols=False) -> abi.Schema:
    if not output_schema or not output_schema.cols:
        cols = c.schema()
    else:
        index = {}
        for i, f in enumerate(c.fields):
            index[f.decode()] = i  # (a later duplicate cannot exist: the names are unique)
        cols = []
        for col in output_schema.cols:
            col = abi.ColSchema(**col.__dict__)
            if col.path == "":
                if col.name not in index:
                    continue
                col.path = "%d" % index[col.name]
            if col.original_type == "":
                col.original_type = "nginx:" + col.dtype
            cols.append(col)
    if not hide_system_cols:
        key = not any(x.key for x in cols)
        cols = [abi.ColSchema("__file_name", "utf8", key), abi.ColSchema("__row_index", "uint64", key)] + cols
    return abi.Schema(cols)


_INT_TYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")


def _default_value(col):
    """abstract.DefaultValue (change_item_builders.go:88-109)"""
    if col.dtype in _INT_TYPES:
        return [col.dtype, 0]
    if col.dtype == "float":
        return ["float32", 0.0]
    if col.dtype == "double":
        return ["float64", 0.0]
    if col.dtype in ("string", "utf8"):
        return ["string", b""]
    if col.dtype == "boolean":
        return ["bool", False]
    if col.dtype in ("date", "datetime", "timestamp"):
        return ["time", (0, 0)]
    if col.dtype == "interval":
        return ["duration", 0]
    raise NotImplementedError(col.dtype)


class Parsed:
    """batch / rows: the ChangeItems after Strictify; errors: [(lineCounter, code name, column index or -1)] in line order"""

    def __init__(self):
        self.batch, self.rows, self.errors, self.consumed, self.next_row_number = None, [], [], 0, 0


def parse_chunk(ora, c: Compiled, schema: abi.Schema, data: bytes, file_name="", row_number_base=1, hide_system_cols=False,
                unexpected_field_error=False, last_chunk=False) -> Parsed:
    """One round of NginxReader.Read over `data` (reader_nginx.go:101-189) with every data error collected instead of handled."""
    out = Parsed()
    counter = row_number_base
    last_nl = data.rfind(b"\n")
    if last_nl >= 0:
        processable, out.consumed = data[:last_nl + 1], last_nl + 1
    elif last_chunk:
        processable = data
    else:
        out.next_row_number = counter
        out.batch = abi.batch_from_rows(schema, [x.name for x in schema.cols], [])
        return out
    if last_chunk:
        out.consumed = len(data)
        processable = data
    items = []  # (lineCounter, values before Strictify)
    for line in processable.split(b"\n"):
        line = line.rstrip(b"\r")
        if trim_space(line) == b"":
            continue
        pe = parse_entry(c, line)
        if pe is None:
            out.errors.append((counter, "NGINX_FORMAT", -1))
            counter += 1
            continue
        fields, consumed = pe
        if unexpected_field_error and has_unexpected_fields(line, consumed):
            out.errors.append((counter, "NGINX_EXTRA", -1))
            counter += 1
            continue
        vals, bad = [], None
        for i, col in enumerate(schema.cols):  # constructCI
            if col.name in ("__file_name", "__row_index"):
                if hide_system_cols:
                    vals.append(["nil", None])
                else:
                    vals.append(["string", file_name.encode()] if col.name == "__file_name" else ["uint64", counter])
                continue
            idx = int(col.path)  # strconv.Atoi: the resolver only produces integers
            if idx < 0 or idx >= len(fields):
                vals.append(_default_value(col))
                continue
            v = fields[idx]
            if v == b"-":  # convertNginxValue
                vals.append(["nil", None])
            elif col.dtype in ("datetime", "date"):
                t = ora.time_parse(TIME_LOCAL_LAYOUT, v.decode("utf-8", "surrogateescape")) if _is_utf8(v) else None
                if t is None:
                    bad = i
                    break
                vals.append(["time", t])
            else:
                vals.append(["string", v])
        if bad is not None:
            out.errors.append((counter, "CAST", bad))
        else:
            items.append((counter, vals))
        counter += 1
    out.next_row_number = counter
    names = [x.name for x in schema.cols]
    # strictify.Strictify item by item: rows are independent, so one call over all of them and a second over the ones that pass
    # is the same thing; a failing row is looked at column by column for the first value that fails
    while True:
        pre = abi.batch_from_rows(schema, names, [v for _, v in items])
        res = ora.strictify(pre, schema) if items else None
        if res is None or not res.errors:
            break
        failed = {}
        for row, code, _msg in res.errors:
            failed.setdefault(row, code)
        for row in sorted(failed):
            counter_r, vals = items[row]
            col_idx, code = -1, failed[row]
            for i, col in enumerate(schema.cols):
                one = abi.batch_from_rows(abi.Schema([col]), [col.name], [[vals[i]]])
                r1 = ora.strictify(one, abi.Schema([col]))
                if r1.errors:
                    col_idx, code = i, r1.errors[0][1]
                    break
            out.errors.append((counter_r, abi.ROWERR[code], col_idx))
        items = [it for k, it in enumerate(items) if k not in failed]
    out.errors.sort(key=lambda e: e[0])
    if items:
        out.batch = res.batch
    else:
        out.batch = pre
    out.rows = abi.batch_rows(out.batch) if items else []
    return out


def _is_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False
