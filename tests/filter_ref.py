"""filter_rows restated in plain Python over abi.Batch rows, from pkg/transformer/registry/filter_rows/{filter_rows,util}.go and
library/go/yandex/cloud/filter/{grammar/grammar.go,filters.go}, line by line, with no eye on the device code or on oracle/.  Python integers and
Python floats only (a Python float is Go's float64).

The lexer is the reference's own regular expression (grammar.go:257-264), applied with re's .match(s, pos): Python's alternation is leftmost-first
as Go's is.  Two things are Go's and not Python's: `\\d` means [0-9] (re.ASCII), and `\\s` means [\\t\\n\\f\\r ] — no vertical tab — so that one
class is spelled out.

What this model does not decide (the third-party sources are not part of the reference tree, so nothing here guesses at them):
  * a quoted string whose unquoted text is one of the grammar's literals (AND, IN, NOT, TRUE, FALSE, NULL, NIL, the three punctuation marks) where
    the grammar expects that literal: participle compares literals by token value.  parse() raises OutOfModel for such a filter.
  * what participle's Unquote makes of `\\x80`..`\\xff` and `\\200`..`\\377` (a byte or a rune).  unquote() raises OutOfModel for them.

A cell, as the Go code sees it (go_value): R_INT8.. a sized integer, R_FLOAT32/64 a float, R_BOOL a bool, R_STRING a string, R_BYTES a []byte,
R_JSONNUM a json.Number, R_TIME a time.Time, R_DURATION a time.Duration, R_JSON what encoding/json decodes from the text into an interface{}
(string, float64, bool, map, slice), a nil cell nil.  An ABSENT cell is not in the row's ColumnNames at all.

match_value answers True / False (the reference decides, this is its answer), an error class (INT_OVERFLOW, TYPE_PAIR), IMPL_DEFINED (Go's
int64(float) outside the int64 range, which the Go spec leaves to the implementation: amd64 gives MinInt64, arm64 saturates), or UNDECIDED (a text
under a time constant that is none of the fixed shapes below: stringToTime's other layouts are not restated).  Beside the answer it says whether
the device may hand the row back to the host path instead of answering (may_fall_back):
  * R_STRING and R_JSONNUM cells under a numeric constant (strconv.ParseFloat of a text),
  * R_JSON scalar cells,
  * R_STRING cells under a time constant whose text is none of the fixed shapes.
The fixed shapes are syntactic — digits and punctuation, whatever the fields' values:
  2006-01-02 | 2006-01-02 15:04:05[.frac] | 2006-01-02T15:04:05[.frac] | 2006-01-02T15:04:05[.frac](Z|±hh:mm)      (frac behind `.` or `,`)
A text of such a shape whose fields are out of range (Feb 30, 24:00, :60, +25:00) is parsed by no layout of stringToTime: every other layout
fails on its first punctuation mark.  The reference then reports "Unsupported type pair", and so does the model: TYPE_PAIR, no fallback."""
import json
import math
import re

from transferia_amd import abi

import byids_ref

INT_OVERFLOW, TYPE_PAIR, COLUMN_NOT_FOUND, UNSUPPORTED_KIND = "INT_OVERFLOW", "TYPE_PAIR", "COLUMN_NOT_FOUND", "UNSUPPORTED_KIND"
IMPL_DEFINED, UNDECIDED = "IMPL_DEFINED", "UNDECIDED"
EQ, NE, LT, LE, GT, GE, IN, NOT_IN, MATCH, NOT_MATCH = "=", "!=", "<", "<=", ">", ">=", "IN", "NOT IN", "~", "!~"
OPERATORS = (EQ, NE, LT, LE, GT, GE, IN, NOT_IN, MATCH, NOT_MATCH)
MIN_I64, MAX_I64 = -(1 << 63), (1 << 63) - 1


class Refused(Exception):
    """the reference's constructor returns an error for this filter"""


class OutOfModel(Exception):
    """see the module docstring: the model has no answer of its own"""


# ---- the lexer (grammar.go:255-265) -------------------------------------------------------------------------------------------------------------
GO_LEXER = (r"""(?P<Operator>!=|<=|>=|!~|[=<>~])"""
            r"""|(?P<String>'((\\'|[^']))*'|"(\\"|[^"])*")"""
            r"""|(?P<DateTime>\d{4}-\d{2}-\d{2}(T\d{2}:\d{2}(:\d{2}(\.\d+)?)?(Z|[+-]\d+(:\d+)?)?)?)"""
            r"""|(?P<Ident>[a-zA-Z][a-zA-Z0-9_.]*)"""
            r"""|(?P<Float>[-+]?\d+\.\d+)"""
            r"""|(?P<Int>[-+]?\d+)"""
            r"""|(?P<Punctuation>[(),])"""
            r"""|(?P<WS>\s+)""")
_LEXER = re.compile(GO_LEXER.replace(r"\s", r"[\t\n\f\r ]"), re.ASCII | re.DOTALL)   # Go's \s; Go's [^'] takes a newline too


def lex(s: str):
    """-> [(token type, text)]; Refused where no alternative matches (the lexer's error)"""
    out, pos = [], 0
    while pos < len(s):
        m = _LEXER.match(s, pos)
        if m is None or m.end() == pos:
            raise Refused("invalid token at %d" % pos)
        out.append((m.lastgroup, m.group()))
        pos = m.end()
    return out


# ---- participle.Unquote("String"): a strconv.UnquoteChar loop (strconv/quote.go) ----------------------------------------------------------------
_SIMPLE = {"a": 7, "b": 8, "f": 12, "n": 10, "r": 13, "t": 9, "v": 11, "\\": 0x5C}


def unquote(tok: str) -> bytes:
    quote, s = tok[0], tok[1:-1]
    out = bytearray()
    i = 0
    while i < len(s):
        c = s[i]
        if c == quote:
            raise Refused("unescaped quote")
        if c != "\\":
            out += c.encode("utf-8")
            i += 1
            continue
        if i + 1 >= len(s):
            raise Refused("lone backslash")
        e = s[i + 1]
        i += 2
        if e in _SIMPLE:
            out.append(_SIMPLE[e])
        elif e in "xuU":
            n = {"x": 2, "u": 4, "U": 8}[e]
            h = s[i:i + n]
            if len(h) < n or not re.fullmatch(r"[0-9a-fA-F]+", h):
                raise Refused("bad hex escape")
            v = int(h, 16)
            i += n
            if e == "x":
                if v >= 0x80:
                    raise OutOfModel("\\x%02x" % v)
                out.append(v)
            else:
                if v > 0x10FFFF or 0xD800 <= v < 0xE000:       # !utf8.ValidRune
                    raise Refused("invalid rune")
                out += chr(v).encode("utf-8")
        elif e in "01234567":
            d = s[i:i + 2]
            if len(d) < 2 or not re.fullmatch(r"[0-7]{2}", d):
                raise Refused("bad octal escape")
            v = int(e + d, 8)
            i += 2
            if v > 255:
                raise Refused("octal escape above 255")
            if v >= 0x80:
                raise OutOfModel("\\%o" % v)
            out.append(v)
        elif e in "'\"":
            if e != quote:
                raise Refused("the other quote, escaped")
            out += e.encode()
        else:
            raise Refused("unknown escape")
    return bytes(out)


# ---- time.Parse of a DateTime token under findTimeLayout's layout (grammar.go:114-144, 171-182) -------------------------------------------------
def days_from_civil(y, m, d):
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def _days_in(m, y):
    if m == 2:
        return 29 if y % 4 == 0 and (y % 100 != 0 or y % 400 == 0) else 28
    return 30 if m in (4, 6, 9, 11) else 31


def unix_micro(y, mo, d, h, mi, se, frac, sign, zh, zm):
    """time.Date(...).UnixMicro() of fields as time.Parse read them, or None where Parse reports a field out of range.  frac: the digits behind the
    mark, as text (parseNanoseconds keeps nine); sign: -1, +1, or 0 for UTC"""
    if not (1 <= mo <= 12 and 1 <= d <= 31 and d <= _days_in(mo, y) and h < 24 and mi < 60 and se < 60):
        return None
    if zh > 24 or zm > 60:               # "some people do write offsets of 24 hours or 60 minutes": > and not >=
        return None
    ns = int((frac[:9]).ljust(9, "0")) if frac else 0
    sec = days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + se - sign * (zh * 3600 + zm * 60)
    return sec * 1000000 + ns // 1000


def parse_datetime_token(v: str) -> int:
    """UnixMicro of a DateTime token, Refused where time.Parse(findTimeLayout(v), v) fails"""
    t = v.find("T")
    with_seconds, tz = False, None
    if t > 0:
        time_part = v[t:]
        z = next((k for k, ch in enumerate(time_part) if ch in "+-Z"), -1)
        pure = time_part if z < 0 else time_part[:z]
        with_seconds = pure.count(":") == 2
        if z >= 0:
            tz = "Z07:00" if ":" in time_part[z:] else "Z07"
    m = re.match(r"(\d{4})-(\d{2})-(\d{2})", v, re.ASCII)
    y, mo, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
    rest = v[10:]
    h = mi = se = 0
    frac, sign, zh, zm = "", 0, 0, 0
    if t > 0:
        m = re.match(r"T(\d{2}):(\d{2})", rest, re.ASCII)
        h, mi = int(m.group(1)), int(m.group(2))
        rest = rest[6:]
        if with_seconds:
            m = re.match(r":(\d{2})(?:[.,](\d+))?", rest, re.ASCII)          # the fraction behind "05" is read though the layout has none
            se, frac = int(m.group(1)), m.group(2) or ""
            rest = rest[m.end():]
        if tz is not None:
            if rest[:1] == "Z":
                rest = rest[1:]
            elif tz == "Z07:00":
                m = re.match(r"([+-])(\d{2}):(\d{2})", rest, re.ASCII)
                if m is None:
                    raise Refused("zone")
                sign, zh, zm = (-1 if m.group(1) == "-" else 1), int(m.group(2)), int(m.group(3))
                rest = rest[6:]
            else:
                m = re.match(r"([+-])(\d{2})", rest, re.ASCII)
                if m is None:
                    raise Refused("zone")
                sign, zh = (-1 if m.group(1) == "-" else 1), int(m.group(2))
                rest = rest[3:]
    if rest:
        raise Refused("extra text")
    us = unix_micro(y, mo, d, h, mi, se, frac, sign, zh, zm)
    if us is None:
        raise Refused("field out of range")
    return us


# ---- the grammar (grammar.go:16-61) and validateTerm (filters.go:246-274) --------------------------------------------------------------------------
class Term:
    """attr; op; vtype in int/float/string/time/bool/null; values: a list for IN / NOT IN, else one value (int: int, float: float, string: bytes,
    time: UnixMicro, bool: bool, null: None)"""

    def __init__(self, attr, op, vtype, value):
        self.attr, self.op, self.vtype, self.value = attr, op, vtype, value

    def __repr__(self):
        return "Term(%s %s %s %r)" % (self.attr, self.op, self.vtype, self.value)


class _Parser:
    def __init__(self, toks):
        self.t, self.p = toks, 0

    def peek(self):
        return self.t[self.p] if self.p < len(self.t) else ("EOF", "")

    def ws(self):
        if self.peek()[0] == "WS":
            self.p += 1

    def lit(self, *words):
        """a literal of the grammar: compared by value, without regard to case for an Ident token"""
        ty, v = self.peek()
        if ty == "String":
            try:
                u = unquote(v).decode("utf-8", "replace")
            except (Refused, OutOfModel):
                return None
            if u in words:
                raise OutOfModel("a quoted %r where the grammar expects the literal" % u)
            return None
        hit = next((w for w in words if (v.upper() == w if ty == "Ident" else v == w)), None)
        if hit is not None:
            self.p += 1
        return hit

    def value(self):
        ty, v = self.peek()
        if ty == "String":
            self.p += 1
            return ("string", unquote(v))
        if ty == "DateTime":
            self.p += 1
            return ("datetime", v)
        w = self.lit("TRUE", "FALSE")
        if w:
            return ("bool", w == "TRUE")
        if ty == "Float":
            self.p += 1
            return ("float", v)
        if ty == "Int":
            self.p += 1
            return ("int", v)
        if self.lit("NULL", "NIL"):
            return ("null", None)
        if self.lit("("):
            items = []
            self.ws()
            items.append(self.value())
            self.ws()
            while True:
                self.ws()
                if not self.lit(","):
                    break
                self.ws()
                items.append(self.value())
                self.ws()
            if not self.lit(")"):
                raise Refused("unexpected token %r" % (self.peek()[1],))
            return ("list", items)
        raise Refused("unexpected token %r" % (v,))

    def term(self):
        ty, v = self.peek()
        if ty != "Ident":
            raise Refused("unexpected token %r" % (v,))
        attr = v
        self.p += 1
        self.ws()
        ty, v = self.peek()
        if ty == "Operator":
            op = v
            self.p += 1
        elif self.lit("IN"):
            op = IN
        elif self.lit("NOT"):
            while self.peek()[0] == "WS":
                self.p += 1
            if not self.lit("IN"):
                raise Refused("unexpected token %r" % (self.peek()[1],))
            op = NOT_IN
        else:
            raise Refused("unexpected token %r" % (v,))
        self.ws()
        val = self.value()
        self.ws()
        return attr, op, val


def _delayed(v):
    """Value.delayedParse: the constant's own value, Refused where strconv / time.Parse report an error"""
    ty, x = v
    if ty == "datetime":
        return parse_datetime_token(x)
    if ty == "float":
        f = float(x)
        if math.isinf(f):
            raise Refused("value out of range")
        return f
    if ty == "int":
        i = int(x)
        if not MIN_I64 <= i <= MAX_I64:
            raise Refused("value out of range")
        return i
    return x


def parse(s: str):
    """filter.Parse -> [Term], Refused where the reference's constructor gives an error (prepareTermValues' included)"""
    if s == "":
        return []
    p = _Parser(lex(s))
    p.ws()
    raw = []
    if p.peek()[0] != "EOF":
        raw.append(p.term())
        while True:
            save = p.p
            p.ws()
            if not p.lit("AND"):
                p.p = save
                break
            p.ws()
            raw.append(p.term())
    if p.peek()[0] != "EOF":
        raise Refused("unexpected token %r" % (p.peek()[1],))
    terms = []
    for attr, op, (ty, x) in raw:
        if ty == "list":                                             # validateTerm
            head = x[0][0]
            if any(i[0] != head for i in x):
                raise Refused("list items should have same type")
            if head == "list":
                raise Refused("nested list are not supported")
            if op not in (IN, NOT_IN):
                raise Refused("list values require [ NOT ] IN operator")
            vals = [_delayed(i) for i in x]
            if head in ("bool", "null"):                             # valuesListToSet (util.go:81-112)
                raise Refused("not appropriate type of list values")
            terms.append(Term(attr, op, "time" if head == "datetime" else head, vals))
        else:
            if op in (IN, NOT_IN):
                raise Refused("%s operator expect list value" % op)
            if ty == "null" and op not in (EQ, NE):
                raise Refused("NULL expects = or !=")
            terms.append(Term(attr, op, "time" if ty == "datetime" else ty, _delayed((ty, x))))
    return terms


def expressions(config):
    """Config.expressions (filter_rows.go:47-70)"""
    flt, many = config.get("filter", "") or "", config.get("filters") or []
    if flt != "" and many:
        raise Refused("Settings 'filters' and 'filter' cannot be enabled at the same time")
    return [parse(f) for f in (many if many else [flt])]


# ---- strconv.ParseFloat(s, 64) as cast.ToFloat64E calls it ------------------------------------------------------------------------------------------
_DEC = re.compile(r"[+-]?(?:[0-9_]+\.?[0-9_]*|\.[0-9_]+)(?:[eE][+-]?[0-9_]+)?", re.ASCII)
_HEX = re.compile(r"[+-]?0[xX](?:[0-9a-fA-F_]+\.?[0-9a-fA-F_]*|\.[0-9a-fA-F_]+)[pP][+-]?[0-9_]+", re.ASCII)


def _underscore_ok(s):
    """strconv's underscoreOK: an underscore only between digits, or between a base prefix and a digit"""
    i = 1 if s[:1] in "+-" else 0
    saw, hexa = "^", False
    if len(s) - i >= 2 and s[i] == "0" and s[i + 1] in "bBoOxX":
        hexa = s[i + 1] in "xX"
        i += 2
        saw = "0"
    for ch in s[i:]:
        if ch.isdigit() or (hexa and ch in "abcdefABCDEF"):
            saw = "0"
        elif ch == "_":
            if saw != "0":
                return False
            saw = "_"
        else:
            if saw == "_":
                return False
            saw = "!"
    return saw != "_"


def go_parse_float(b: bytes):
    """-> float, or None where ParseFloat returns an error (a range error too: cast then fails the conversion)"""
    try:
        s = b.decode("ascii")
    except UnicodeDecodeError:
        return None
    m = re.fullmatch(r"([+-]?)(inf|infinity)", s, re.I)
    if m:
        return -math.inf if m.group(1) == "-" else math.inf
    if s.lower() == "nan":
        return math.nan
    if _HEX.fullmatch(s):
        if not _underscore_ok(s):                                    # (also what refuses a mantissa without a digit: "0x_p1")
            return None
        try:
            return float.fromhex(s.replace("_", ""))
        except (OverflowError, ValueError):
            return None
    if _DEC.fullmatch(s):
        if not _underscore_ok(s):
            return None
        t = s.replace("_", "")
        if not re.search(r"[0-9]", re.split(r"[eE]", t)[0]) or (("e" in t.lower()) and not re.search(r"[0-9]", re.split(r"[eE]", t)[1])):
            return None
        f = float(t)
        return None if math.isinf(f) else f
    return None


# ---- a cell as a Go value ---------------------------------------------------------------------------------------------------------------------------
SIGNED = {abi.R_INT8, abi.R_INT16, abi.R_INT32, abi.R_INT64}
UNSIGNED = {abi.R_UINT8, abi.R_UINT16, abi.R_UINT32, abi.R_UINT64}


def go_value(col, i):
    """(kind, value): int | uint | f32 | f64 | bool | string | bytes | jsonnum | time | duration | nil | map | slice"""
    if col.validity is not None and not col.validity[i]:
        return ("nil", None)
    r = col.repr
    if r in SIGNED:
        return ("int", int(col.values[i]))
    if r in UNSIGNED:
        return ("uint", int(col.values[i]))
    if r in (abi.R_FLOAT32, abi.R_FLOAT64):
        return ("f32" if r == abi.R_FLOAT32 else "f64", float(col.values[i]))
    if r == abi.R_BOOL:
        return ("bool", bool(col.values[i]))
    if r == abi.R_TIME:
        return ("time", (int(col.values[i]), int(col.nanos[i]) if col.nanos is not None else 0))
    if r == abi.R_DURATION:
        return ("duration", int(col.values[i]))
    raw = col.get_bytes(i)
    if r == abi.R_STRING:
        return ("string", raw)
    if r == abi.R_BYTES:
        return ("bytes", raw)
    if r == abi.R_JSONNUM:
        return ("jsonnum", raw)
    v = json.loads(raw.decode("utf-8", "surrogateescape"))
    if isinstance(v, str):
        return ("string", byids_ref.json_text_as_string(raw))        # by its bytes: encoding/json's own unquote
    if isinstance(v, bool):
        return ("bool", v)
    if isinstance(v, (int, float)):
        return ("f64", float(v))
    if isinstance(v, dict):
        return ("map", None)
    if isinstance(v, list):
        return ("slice", None)
    raise OutOfModel("an `any` cell whose text is null")


# ---- matchValue (filter_rows.go:180-365) --------------------------------------------------------------------------------------------------------------
_FIXED = re.compile(r"(\d{4})-(\d\d)-(\d\d)(?:([ T])(\d\d):(\d\d):(\d\d)(?:[.,](\d+))?(?:(Z)|([+-])(\d\d):(\d\d))?)?", re.ASCII)


def fixed_shape_time(text: bytes):
    """-> (is one of the fixed shapes, UnixMicro or None where no layout parses it)"""
    try:
        m = _FIXED.fullmatch(text.decode("ascii"))
    except UnicodeDecodeError:
        return False, None
    if m is None or (m.group(4) == " " and (m.group(9) or m.group(10))):
        return False, None
    g = m.groups()
    if g[3] is None:
        return True, unix_micro(int(g[0]), int(g[1]), int(g[2]), 0, 0, 0, "", 0, 0, 0)
    sign = 0 if g[9] is None else (-1 if g[9] == "-" else 1)
    return True, unix_micro(int(g[0]), int(g[1]), int(g[2]), int(g[4]), int(g[5]), int(g[6]), g[7] or "", sign, int(g[10] or 0), int(g[11] or 0))


def _ordered(a, b, op):
    """matchOrderedValue; Go's float comparisons are IEEE's, as Python's are"""
    if op == EQ:
        return a == b
    if op == NE:
        return a != b
    if op == LT:
        return a < b
    if op == LE:
        return a <= b
    if op == GT:
        return a > b
    if op == GE:
        return a >= b
    return TYPE_PAIR                                                  # "Unknown operation": ~ and !~ on a number


def _in_set(v, values, op):
    """matchValueToSet: a Go map lookup — a NaN key is never found, -0.0 finds 0.0"""
    found = any(v == x for x in values)
    return found if op == IN else not found


def match_value(cell, term, from_json=False):
    """-> (answer, may_fall_back)"""
    kind, v = cell
    op, ty = term.op, term.vtype
    is_set = op in (IN, NOT_IN)
    is_int1 = is_float1 = False
    int1 = float1 = None
    fb = from_json and kind not in ("map", "slice", "nil")            # an R_JSON scalar
    if kind == "int":
        is_int1, int1 = True, v
    elif kind == "uint":                                               # toInt64E (util.go:49-79): only uint64 can overflow
        if v > MAX_I64:
            return INT_OVERFLOW, fb
        is_int1, int1 = True, v
    if not is_int1:                                                    # cast.ToFloat64E
        if kind in ("f32", "f64"):
            is_float1, float1 = True, v
        elif kind == "bool":
            is_float1, float1 = True, 1.0 if v else 0.0
        elif kind == "nil":
            is_float1, float1 = True, 0.0
        elif kind in ("string", "jsonnum"):
            f = go_parse_float(v)
            if f is not None:
                is_float1, float1 = True, f
    if ty in ("int", "float") and kind in ("string", "jsonnum"):
        fb = True
    if ty == "int":
        if is_int1:
            return (_in_set(int1, term.value, op) if is_set else _ordered(int1, term.value, op)), fb
        if is_float1:
            if is_set:
                if math.trunc(float1) == float1 if math.isfinite(float1) else not math.isnan(float1):
                    if not (-9223372036854775808.0 <= float1 < 9223372036854775808.0):
                        return IMPL_DEFINED, fb
                    return _in_set(int(float1), term.value, op), fb
                return False, fb                                        # isMatched = false for IN and for NOT IN
            return _ordered(float1, float(term.value), op), fb
    elif ty == "float":
        if is_int1:
            return (_in_set(float(int1), term.value, op) if is_set else _ordered(float(int1), term.value, op)), fb
        if is_float1:
            return (_in_set(float1, term.value, op) if is_set else _ordered(float1, term.value, op)), fb
    elif ty == "bool":
        if kind == "bool":
            return _ordered(int(v), int(term.value), op), fb
    elif ty == "string":
        if kind in ("bytes", "string"):
            if op == MATCH:
                return term.value in v, fb
            if op == NOT_MATCH:
                return term.value not in v, fb
            return (_in_set(v, term.value, op) if is_set else _ordered(v, term.value, op)), fb
    elif ty == "time":
        us = None
        if kind == "time":
            us = v[0] * 1000000 + v[1] // 1000                          # Time.UnixMicro
        elif kind == "string":
            fixed, us = fixed_shape_time(v)
            if not fixed:
                return UNDECIDED, True
        if us is not None:
            return (_in_set(us, term.value, op) if is_set else _ordered(us, term.value, op)), fb
    elif ty == "null":
        if op == EQ:
            return kind == "nil", fb
        if op == NE:
            return kind != "nil", fb
    return TYPE_PAIR, fb


# ---- Apply, matchItem, matchExpression (filter_rows.go:99-176) ----------------------------------------------------------------------------------------
SYSTEM_TABLES = {"__wal", "__table_transfer_progress", "__tm_gtid_keeper", "__tm_keeper", "__consumer_keeper", "__data_transfer_lsn",
                 "__data_transfer_signal_table", "__data_transfer", "__dt_cluster_time"}    # abstract.RegisterSystemTables of the providers


class Row:
    """outcome: "keep" | "drop" | an error class | IMPL_DEFINED | UNDECIDED; term: the flat index of the term that ended the row (errors, IMPL_DEFINED,
    UNDECIDED), else -1; fall_back: the flat indices of the terms at which the device may hand this row back instead"""

    def __init__(self, outcome, term=-1, fall_back=()):
        self.outcome, self.term, self.fall_back = outcome, term, tuple(fall_back)

    def __repr__(self):
        return "Row(%s, %d, %r)" % (self.outcome, self.term, self.fall_back)


def match_row(exprs, batch, i):
    names = [c for c in batch.cols if c.absent is None or not c.absent[i]]      # the row's own ColumnNames
    fall_back = []
    base = 0
    for terms in exprs:                                                           # matchItem: an OR, the first match ends it
        ok = True
        for k, term in enumerate(terms):                                          # matchExpression: an AND, the first false term ends it
            for j, col in enumerate(names):
                if col.name != term.attr:
                    if j < len(names) - 1:
                        continue
                    return Row(COLUMN_NOT_FOUND, base + k, fall_back)
                ans, fb = match_value(go_value(col, i), term, from_json=col.repr == abi.R_JSON)
                if fb:
                    fall_back.append(base + k)
                if ans is not True and ans is not False:
                    return Row(ans, base + k, fall_back)
                ok = ans
                break
            if not ok:
                break
        if ok:
            return Row("keep", -1, fall_back)
        base += len(terms)
    return Row("drop", -1, fall_back)


def apply(batch, config):
    """-> [Row] for every row of `batch`; Refused where the constructor fails"""
    exprs = expressions(config)
    applies = byids_ref.table_matches(config, batch.table_ns, batch.table_name) and batch.table_name not in SYSTEM_TABLES
    out = []
    for i in range(batch.nrows):
        kind = abi.K_INSERT if batch.kind is None else int(batch.kind[i])
        if kind in (abi.K_UPDATE, abi.K_DELETE):
            out.append(Row(UNSUPPORTED_KIND))
        elif not applies or kind != abi.K_INSERT:
            out.append(Row("keep"))
        else:
            out.append(match_row(exprs, batch, i))
    return out


def kept(rows):
    return [i for i, r in enumerate(rows) if r.outcome == "keep"]


def errors(rows):
    return sorted((i, r.outcome, r.term) for i, r in enumerate(rows) if r.outcome in (INT_OVERFLOW, TYPE_PAIR, COLUMN_NOT_FOUND, UNSUPPORTED_KIND))
