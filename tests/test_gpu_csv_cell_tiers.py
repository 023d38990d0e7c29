"""The cell tiers of csv_parse_regular against the oracle: the text cells that stay on the straight tier (plain at both ends, or
enclosed in quotes with any number of quotes between) and those that must leave it, the date / timestamp cells in every shape
their fixed-offset code accepts or refuses (slots of one length and mixed ones, as a tier of their own would tell them apart),
and the item → (column, line) division at the edges of a slot.

A tile's cells are dealt run by run (a run: the columns of one kind), items (column, line) with lines fastest, 64 items a slot.
The schema has three text columns, so with L lines item 63 and item 64 of the text run are cells (63 // L, 63 % L) and
(64 // L, 64 % L): the line counts 40, 64, 65 and 130 put a slot's edge inside a column, at a column's end and past it."""
import numpy as np
import pytest

from transferia_amd import abi
from test_gpu_csv import compare, tf  # noqa: F401  (tf: the module's library fixture)

pytestmark = pytest.mark.gpu

SCHEMA = abi.Schema.of([["t0", "utf8", False, "0"], ["t1", "utf8", False, "1"], ["t2", "utf8", False, "2"],
                        ["i", "int32", False, "3"], ["d", "date", False, "4"], ["ts", "timestamp", False, "5"]])
T0, T1, T2, INT, DATE, TS = range(6)
LINES = (40, 64, 65, 130)


def table(nlines, cells=None, ts="2013-07-15 10:47:34", date="2013-07-15"):
    """nlines lines of plain cells; cells: {(column, line): the cell's bytes as they stand in the file}."""
    cells = cells or {}
    out = []
    for j in range(nlines):
        row = [b"p%d" % j, b"word%d" % (j * 7), b"x", b"%d" % (j * 1000003 % 2000000), date.encode(), ts.encode()]
        for c in range(6):
            if (c, j) in cells:
                row[c] = cells[(c, j)]
        out.append(b",".join(row) + b"\n")
    return b"".join(out)


def text_item(nlines, it):
    """(column, line) of item `it` of the text run"""
    return it // nlines, it % nlines


# ---------------------------------------------------------------------------------------------------------------------------
# text cells
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlines", LINES)
def test_one_odd_cell_at_each_edge_of_a_slot(tf, oracle, nlines):
    for odd in (b'"a""b"', "plainй".encode(), "йplain".encode()):
        for it in (0, 63, 64):
            col, line = text_item(nlines, it)
            out, errs = compare(tf, oracle, {}, SCHEMA, table(nlines, {(col, line): odd}), "odd %r at item %d of %d lines" % (odd, it, nlines))
            assert not errs and out.nrows == nlines
            want = b'a"b' if odd[0:1] == b'"' else odd
            assert out.col("t%d" % col).get_bytes(line) == want


QUOTE_RUNS = [b'""', b'""""', b'""""""', b'"a""""b"', b'"""a"', b'"a"""', b'"a"b"c"', b'"a""b"', b'",,"', b'"a,""b"', b'""","""']


@pytest.mark.parametrize("nlines", LINES)
def test_quote_runs_inside_enclosed_cells(tf, oracle, nlines):
    cells = {}
    for k, q in enumerate(QUOTE_RUNS):  # every shape in every text column, on lines of their own
        for col in (T0, T1, T2):
            cells[(col, (3 * k + col) % nlines)] = q
    compare(tf, oracle, {}, SCHEMA, table(nlines, cells), "quote runs, %d lines" % nlines)
    # ... and every shape alone among plain cells
    for k, q in enumerate(QUOTE_RUNS):
        col, line = text_item(nlines, (61 + k) % (3 * nlines))
        compare(tf, oracle, {}, SCHEMA, table(nlines, {(col, line): q}), "quote run %r alone, %d lines" % (q, nlines))


@pytest.mark.parametrize("size", [33, 64, 100])
def test_pair_count_crosses_words_of_the_quote_bitmap(tf, oracle, size):
    """Enclosed cells of `size` bytes, one on every line, a "" pair sliding through them byte by byte (and a second pair and a lone
    quote run of three further on): the pairs land on every bit of the bitmap's 32-bit words, bits 31 / 32 included."""
    nlines = 130
    inner = size - 2
    cells = {}
    for j in range(nlines):
        body = bytearray(b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[k % 62] for k in range(inner))
        p = j % (inner - 1)
        body[p:p + 2] = b'""'
        p2 = (p + 9) % (inner - 3)
        if abs(p2 - p) > 4:
            body[p2:p2 + 4] = b'""""'
        cells[(T1, j)] = b'"' + bytes(body) + b'"'
    data = table(nlines, cells)
    # the input is what the docstring says: some pair starts on bit 31 of a bitmap word (tile positions are file offsets + 4096)
    starts = {m % 32 for m in range(len(data) - 1) if data[m:m + 2] == b'""'}
    assert {30, 31, 0} <= starts
    out, errs = compare(tf, oracle, {}, SCHEMA, data, "pairs across bitmap words, %d-byte cells" % size)
    assert not errs and out.nrows == nlines


LEAVERS = [
    b" a", b"a ", b" ", b"\ta", b"a\x7f",
    "\u00a0a\u00a0".encode(), "\u2003a\u2003".encode(), "\u3000a\u3000".encode(), "\u0085a\u0085".encode(),
    "\u1680".encode(), "a\u2028".encode(), "\u205fa".encode(),
    b"a\xc2", b"\xc2", b"\xe2\x80", b"a\xe2",                              # malformed ends
    "a\u200b".encode(), "\u200ba".encode(), "a\u0416".encode(), b"a\xe2\x80", b"a\x80\x80",  # E2 80 8B is no space; nor are these
]


@pytest.mark.parametrize("nlines", (40, 65))
def test_cells_that_leave_the_straight_tier(tf, oracle, nlines):
    """A space or a Unicode space at either end, a malformed end, a rune that only looks like a space's: each alone in a slot of
    plain cells, then all of them together; none may go back to the host."""
    for k, cell in enumerate(LEAVERS):
        col, line = text_item(nlines, (62 + k) % (3 * nlines))
        compare(tf, oracle, {}, SCHEMA, table(nlines, {(col, line): cell}), "leaver %r, %d lines" % (cell, nlines))
    cells = {((k + j) % 3, (2 * k + j) % nlines): cell for k, cell in enumerate(LEAVERS) for j in (0, 1)}
    compare(tf, oracle, {}, SCHEMA, table(nlines, cells), "all leavers, %d lines" % nlines)
    # a one-byte cell behind a field that ends in the lead byte of a three-byte space: the look two bytes back leaves the cell
    for lead in (b"\xe1", b"\xe2", b"\xe3", b"\xc2"):
        for last in (b"\x80", b"\x8b", b"\x9f", b"\xa0"):
            compare(tf, oracle, {}, SCHEMA, table(nlines, {(T0, 5): b"a" + lead, (T1, 5): last, (T2, 5): last + last}), "behind %r: %r" % (lead, last))


@pytest.mark.parametrize("cell", [b'"', b'"a', b'a"', b'a"b', b'a""b', b'"a"b', b'a"b"', b'""a'])
def test_quotes_that_do_not_enclose(tf, oracle, cell):
    """A quote at one end only, inside an unquoted cell, or alone: the line's quotes may not even balance (the tile then takes the
    general kernel).  Whatever the path, the answer is the oracle's."""
    for nlines in (40, 65):
        col, line = text_item(nlines, 63)
        compare(tf, oracle, {}, SCHEMA, table(nlines, {(col, line): cell}), "%r, %d lines" % (cell, nlines))


def test_double_quote_disabled(tf, oracle):
    for nlines in (40, 65):
        for it in (0, 63, 64):
            col, line = text_item(nlines, it)
            out, errs = compare(tf, oracle, dict(double_quote=0), SCHEMA, table(nlines, {(col, line): b'"a""b"', (T2, 7): b'"plain"', (T2, 8): b'""'}),
                                "double_quote=0, item %d of %d lines" % (it, nlines))
            assert line in [e[0] for e in errs]  # (error and kind were compared with the oracle's)


# ---------------------------------------------------------------------------------------------------------------------------
# date and timestamp cells
# ---------------------------------------------------------------------------------------------------------------------------
def test_time_slots_of_one_length_and_mixed(tf, oracle):
    for nlines in LINES:
        for sep in " T":
            compare(tf, oracle, {}, SCHEMA, table(nlines, ts="2013-07-15%s10:47:34" % sep), "all 19 bytes, %r" % sep)
        compare(tf, oracle, {}, SCHEMA, table(nlines, ts="2013-07-15"), "all 10 bytes")
        compare(tf, oracle, {}, SCHEMA, table(nlines, date="2013-07-15 10:47:34"), "a date column of 19-byte cells")
        mix = {(TS, j): [b"2013-07-15", b"2024-02-29T23:59:59", b"1999-12-31 00:00:00"][j % 3] for j in range(nlines)}
        mix.update({(DATE, j): [b"2013-07-15T10:47:34", b"2000-02-29"][j % 2] for j in range(0, nlines, 5)})
        compare(tf, oracle, {}, SCHEMA, table(nlines, mix), "mixed lengths")


def _invalid_times():
    good = "2013-07-15 10:47:34"
    out = ["2013-00-15 10:47:34", "2013-13-15 10:47:34", "2013-07-00 10:47:34", "2013-07-32 10:47:34",
           "2013-04-31 10:47:34", "2013-06-31 10:47:34", "2013-09-31 10:47:34", "2013-11-31 10:47:34", "2013-01-31 10:47:34",
           "2013-07-15 24:47:34", "2013-07-15 10:60:34", "2013-07-15 10:47:60", "2013-07-15 23:59:59", "2013-07-15 00:00:00"]
    for y in (1900, 2000, 2023, 2024, 2100, 2400):
        out += ["%04d-02-%02d 10:47:34" % (y, d) for d in (28, 29, 30)]
    for pos in range(19):  # a non-digit in each digit position, a wrong separator in each separator position
        for ch in ("x", "/", ":", " ", "\xb2", "-", "5"):
            if good[pos] != ch:
                out.append(good[:pos] + ch + good[pos + 1:])
    return out


def test_time_cells_invalid_one_at_a_time(tf, oracle):
    """Every shape the fixed-offset code must refuse (and a few it must take), one cell at a time in a slot of good cells, as a
    timestamp and as a date, in both lengths.  Results and row errors are the oracle's."""
    nlines = 40
    cases = _invalid_times()
    for k, s in enumerate(cases):
        b = s.encode("latin-1")
        line = k % nlines
        compare(tf, oracle, {}, SCHEMA, table(nlines, {(TS, line): b, (DATE, (line + 1) % nlines): b[:10]}), "time %r" % s)
    # ... and all of them in one column, T-separated too
    for sep in (b" ", b"T"):
        cells = {(TS, k): s.encode("latin-1").replace(b" ", sep) for k, s in enumerate(cases[:130])}
        compare(tf, oracle, {}, SCHEMA, table(130, cells), "every invalid shape, %r" % sep)
        cells = {(TS, k): s.encode("latin-1").replace(b" ", sep) for k, s in enumerate(cases[130:260])}
        compare(tf, oracle, {}, SCHEMA, table(130, cells), "every invalid shape (2), %r" % sep)


def test_time_cells_years_and_decimal_seconds(tf, oracle):
    for nlines in (40, 65):
        cells = {}
        for k, y in enumerate((0, 1, 1969, 1970, 9999, 400, 100, 4, 1600, 1700)):
            cells[(TS, 2 * k)] = b"%04d-12-31 23:59:59" % y
            cells[(TS, 2 * k + 1)] = b"%04d-01-01" % y
            cells[(DATE, 2 * k)] = b"%04d-03-01" % y
            cells[(DATE, 2 * k + 1)] = b"%04d-02-29" % y
        compare(tf, oracle, {}, SCHEMA, table(nlines, cells), "years")
        # plain decimal seconds among 19-byte cells (ten digits: the length of a date)
        for dec in (b"1374100000", b"0", b"-5", b"+7", b"1374100000123456789", b"0001374100", b"13741x0000", b"2013-07-1", b""):
            compare(tf, oracle, {}, SCHEMA, table(nlines, {(TS, 11): dec, (TS, nlines - 1): dec}), "decimal seconds %r" % dec)
        compare(tf, oracle, {}, SCHEMA, table(nlines, {(TS, j): b"%d" % (1374100000 + j) for j in range(nlines)}), "all decimal")


# ---------------------------------------------------------------------------------------------------------------------------
# items: the (column, line) of every lane
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols,nlines", [(6, 1), (6, 2), (6, 63), (6, 64), (6, 65), (16, 255), (120, 1), (120, 2), (120, 37), (120, 38), (120, 65)])
def test_every_item_finds_its_cell(tf, oracle, ncols, nlines):
    """Tiles of 1 … 255 lines (a tile indexes 4608 fields: 255 lines of 16 columns, 38 of 120): every cell carries its own
    (column, line), so a wrong quotient in the item division shows as a wrong value."""
    kinds = ["int32", "utf8", "int16", "int64"]
    schema = abi.Schema.of([["c%d" % c, kinds[c % 4] if ncols < 100 else kinds[(c // 30) % 4], False, str(c)] for c in range(ncols)])
    rows = []
    for j in range(nlines):
        rows.append(b",".join(b"%d" % ((c * 256 + j) % 32000) for c in range(ncols)) + b"\n")
    out, errs = compare(tf, oracle, {}, schema, b"".join(rows), "%d columns, %d lines" % (ncols, nlines))
    assert not errs and out.nrows == nlines
    for c in (0, ncols // 2, ncols - 1):
        col = out.col("c%d" % c)
        want = [(c * 256 + j) % 32000 for j in range(nlines)]
        if col.repr in abi.VAR_REPRS:
            assert [col.get_bytes(j) for j in range(nlines)] == [b"%d" % v for v in want]
        else:
            assert np.array_equal(col.values[:nlines], np.array(want, dtype=col.values.dtype))


def test_tiles_of_exactly_64_lines(tf, oracle):
    """Two tiles' worth of 448-byte lines: 28 KiB / 448 = 64 lines end in every tile."""
    schema = abi.Schema.of([["a", "int32", False, "0"], ["pad", "utf8", False, "1"], ["b", "int16", False, "2"], ["t", "utf8", False, "3"]])
    rows = []
    for j in range(160):
        head = b"%d," % (j * 77)
        tail = b",%d,t%d\n" % (j, j)
        rows.append(head + b"p" * (448 - len(head) - len(tail)) + tail)
    data = b"".join(rows)
    assert all(len(r) == 448 for r in rows)
    out, errs = compare(tf, oracle, {}, schema, data, "448-byte lines")
    assert not errs and np.array_equal(out.col("b").values[:160], np.arange(160, dtype=np.int16))
