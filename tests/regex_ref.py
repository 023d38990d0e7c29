"""regex_replace_transformer restated in plain Python (pkg/transformer/registry/regex_replace/transformer.go), independent of the
library's own regex compiler: Go's Regexp.replaceAll loop and Regexp.expand, driven by Python's `re` as the match engine (a
backtracking engine that, like Go's, reports the leftmost match and prefers the first alternative), plus the transformer's batch
rules (the schema type by position, the Go-type gate, the dropped table).

Text is decoded with `surrogateescape`: a byte that is not part of a valid UTF-8 sequence becomes one code point, as
utf8.DecodeRune makes it one rune of width 1 — `.` and negated classes match it in both.

re.sub is NOT used: it replaces an empty match right behind a non-empty one ([a-c]* over "abcdef" gives "xxdxexfx"), Go does not."""
import re

import numpy as np

from transferia_amd import abi

GO_SPACE = "\\t\\n\\f\\r "


def translate(pattern: str) -> str:
    """The mandatory subset of Go's syntax in Python's: \\s is [\\t\\n\\f\\r ] (no \\v), `$` and \\z are the end of the text."""
    out = []
    i, n = 0, len(pattern)
    in_class = class_first = False
    while i < n:
        c = pattern[i]
        if c == "\\" and i + 1 < n:
            e = pattern[i + 1]
            i += 2
            class_first = False
            if e == "s":
                out.append(GO_SPACE if in_class else "[" + GO_SPACE + "]")
            elif e == "S":
                if in_class:
                    raise ValueError("\\S inside a class has no plain translation")
                out.append("[^" + GO_SPACE + "]")
            elif e == "z" and not in_class:
                out.append("\\Z")
            elif e == "B" and not in_class:
                # syntax.EmptyOpContext(-1, -1) is "no word boundary": \B matches in the empty text.  Python before 3.14 says no there.
                out.append("(?:\\B|(?<![\\s\\S])(?![\\s\\S]))")
            else:
                out.append("\\" + e)
            continue
        if in_class:
            if c == "]" and not class_first:
                in_class = False
            class_first = False
            out.append("\\[" if c == "[" else c)  # (a bare [ inside a class is a FutureWarning in Python)
            i += 1
            continue
        if c == "[":
            in_class, class_first = True, True
            out.append(c)
            i += 1
            if i < n and pattern[i] == "^":
                out.append("^")
                i += 1
            continue
        out.append("\\Z" if c == "$" else c)
        i += 1
    return "".join(out)


def compile_go(pattern: str):
    return re.compile(translate(pattern), re.ASCII)


def _extract(s: str):
    """regexp.extract: s starts behind the '$'.  -> (name, num, rest) or None"""
    brace = s.startswith("{")
    if brace:
        s = s[1:]
    i = 0
    while i < len(s) and (s[i].isalpha() or s[i].isdigit() or s[i] == "_"):
        i += 1
    if i == 0:
        return None
    name = s[:i]
    if brace:
        if i >= len(s) or s[i] != "}":
            return None
        i += 1
    num = 0
    for ch in name:
        if not ("0" <= ch <= "9") or num >= 10 ** 8:
            num = -1
            break
        num = num * 10 + ord(ch) - 48
    if name[0] == "0" and len(name) > 1:
        num = -1
    return name, num, s[i:]


def expand(template: str, m) -> str:
    """Regexp.expand over a match of Python's engine (no named groups: a name expands to nothing)"""
    out = []
    while template:
        k = template.find("$")
        if k < 0:
            break
        out.append(template[:k])
        template = template[k + 1:]
        if template.startswith("$"):
            out.append("$")
            template = template[1:]
            continue
        ex = _extract(template)
        if ex is None:
            out.append("$")
            continue
        _, num, template = ex
        if 0 <= num <= m.re.groups and m.start(num) >= 0:
            out.append(m.group(num))
    out.append(template)
    return "".join(out)


def replace_all(pattern, rule: str, data: bytes) -> bytes:
    """Regexp.ReplaceAll(data, rule) (regexp.go replaceAll)"""
    rx = compile_go(pattern) if isinstance(pattern, str) else pattern
    src = data.decode("utf-8", "surrogateescape")
    out = []
    last_end = search = 0
    while search <= len(src):
        m = rx.search(src, search)  # (pos keeps the context: ^ and \b see what lies before it)
        if not m:
            break
        out.append(src[last_end:m.start()])
        if m.end() > last_end or m.start() == 0:  # no copy for an empty match right behind another match
            out.append(expand(rule, m))
        last_end = m.end()
        width = 1 if search < len(src) else 0
        if search + width > m.end():
            search += width
        elif search + 1 > m.end():
            search += 1
        else:
            search = m.end()
    out.append(src[last_end:])
    return "".join(out).encode("utf-8", "surrogateescape")


class NameFilter:
    """filter.Filter (pkg/transformer/registry/filter/filter.go)"""

    def __init__(self, include=None, exclude=None):
        self.include = [re.compile(x) for x in include or []]
        self.exclude = [re.compile(x) for x in exclude or []]

    def match(self, v: str) -> bool:
        if any(r.search(v) for r in self.exclude):
            return False
        return not self.include or any(r.search(v) for r in self.include)


def replace_column(rx, rule: str, c: abi.Column) -> abi.Column:
    n = c.nrows()
    cells = [replace_all(rx, rule, c.get_bytes(i)) if c.is_valid(i) else c.get_bytes(i) for i in range(n)]
    off = np.zeros(n + 1, np.uint32)
    if n:
        off[1:] = np.cumsum([len(x) for x in cells])
    return abi.Column(c.name, c.dtype, c.repr, offsets=off, data=np.frombuffer(b"".join(cells), np.uint8).copy(), validity=c.validity)


def apply_batch(config: dict, b: abi.Batch, schema: abi.Schema = None):
    """Transformer.Apply over a columnar batch.  None: the table does not match and the items are dropped (the loop `continue`s).
    The type that gates the i-th value is the i-th column of the TableSchema (transformer.go:110), whatever its name."""
    tables = NameFilter((config.get("tables") or {}).get("includeTables"), (config.get("tables") or {}).get("excludeTables"))
    columns = NameFilter((config.get("columns") or {}).get("includeColumns"), (config.get("columns") or {}).get("excludeColumns"))
    if not tables.match(b.table_name):
        return None
    schema = schema if schema is not None else getattr(b, "schema", None)
    if schema is not None and len(b.cols) > len(schema.cols):
        raise IndexError("item.TableSchema.Columns()[i]: more ColumnNames than schema columns (the stock transformer panics)")
    rx = compile_go(config.get("regexMatch", ""))
    rule = config.get("replaceRule", "")
    cols = []
    for i, c in enumerate(b.cols):
        typ = schema.cols[i].dtype if schema is not None else c.dtype
        if columns.match(c.name) and ((typ == "utf8" and c.repr == abi.R_STRING) or (typ == "string" and c.repr == abi.R_BYTES)):
            cols.append(replace_column(rx, rule, c))
        else:
            cols.append(c)
    out = abi.Batch(cols, b.nrows, b.table_ns, b.table_name, b.kind, b.src_row, b.part_id)
    if getattr(b, "schema", None) is not None:
        out.schema = b.schema
    return out
