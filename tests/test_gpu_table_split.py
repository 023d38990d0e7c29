"""table_splitter_transformer on the device (tf_tablesplit.hip) against the plain-Python restatement (tests/table_split_ref.py), exactly: the names as
bytes, their count and order of first appearance, every row's table, and every per-table batch cell for cell — values, nils, ABSENT bits, kinds,
OldKeys with presence, part_id, src_row, namespace, table name, TableSchema.

The sizes at which the code takes another path: a wave and a workgroup of rows (63 / 64 / 65 / 256 / 257), one table (no sort) against two, more
tables than a wave, every row a table of its own, and the 8-byte word of the name hash (text cells of 7 / 8 / 9 bytes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import table_split_ref as ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
T = "table_splitter_transformer"


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def text_column(name, dtype, repr_, cells):
    """cells: bytes, or None for nil"""
    n = len(cells)
    off = np.zeros(n + 1, np.uint32)
    if n:
        off[1:] = np.cumsum([len(c or b"") for c in cells])
    valid = np.array([c is not None for c in cells], dtype=bool)
    return abi.Column(name, dtype, repr_, offsets=off, data=np.frombuffer(b"".join(c or b"" for c in cells), np.uint8).copy(),
                      validity=None if valid.all() else valid)


def fixed_column(name, dtype, repr_, vals, nanos=None):
    """vals: numbers, or None for nil"""
    valid = np.array([v is not None for v in vals], dtype=bool)
    a = np.array([0 if v is None else v for v in vals], dtype=abi.REPR_NP[repr_])
    return abi.Column(name, dtype, repr_, values=a, nanos=None if nanos is None else np.array(nanos, np.int32), validity=None if valid.all() else valid)


def assert_same_batch(got: abi.Batch, want: abi.Batch, ctx=""):
    assert got.nrows == want.nrows, ctx
    assert (got.table_ns, got.table_name) == (want.table_ns, want.table_name), ctx

    def cols_equal(gc, wc, what):
        assert [c.name for c in gc] == [c.name for c in wc], (ctx, what)
        for a, b in zip(gc, wc):
            assert (a.dtype, a.repr) == (b.dtype, b.repr), (ctx, what, a.name)
            va = a.validity if a.validity is not None else np.ones(got.nrows, bool)
            vb = b.validity if b.validity is not None else np.ones(want.nrows, bool)
            ab = a.absent if a.absent is not None else np.zeros(got.nrows, bool)
            bb = b.absent if b.absent is not None else np.zeros(want.nrows, bool)
            assert np.array_equal(ab, bb), (ctx, what, a.name, "absent")
            assert np.array_equal(va & ~ab, vb & ~bb), (ctx, what, a.name, "validity")   # (an ABSENT cell reads nil whatever its validity bit said)
            if a.repr in abi.VAR_REPRS:
                assert [a.get_bytes(i) for i in range(got.nrows)] == [b.get_bytes(i) for i in range(want.nrows)], (ctx, what, a.name)
            else:
                ok = va & ~ab
                assert np.array_equal(a.values[ok].view(np.uint8), b.values[ok].view(np.uint8)), (ctx, what, a.name, "values")
                if a.repr == abi.R_TIME:   # (no nanos array = every one of them zero)
                    an = a.nanos if a.nanos is not None else np.zeros(got.nrows, np.int32)
                    bn = b.nanos if b.nanos is not None else np.zeros(want.nrows, np.int32)
                    assert np.array_equal(an[ok], bn[ok]), (ctx, what, a.name, "nanos")
    cols_equal(got.cols, want.cols, "cols")
    cols_equal(getattr(got, "old_keys", None) or [], getattr(want, "old_keys", None) or [], "old_keys")
    if getattr(want, "old_keys", None):
        assert np.array_equal(got.old_present, want.old_present), (ctx, "old_present")
    wk = want.kind if want.kind is not None else np.zeros(want.nrows, np.uint8)
    gk = got.kind if got.kind is not None else np.zeros(got.nrows, np.uint8)
    assert np.array_equal(gk, wk), (ctx, "kind")
    wp = want.part_id if want.part_id is not None else np.zeros(want.nrows, np.uint32)   # (no part_id array = PartID 0 everywhere: the oracle always writes one)
    gp = got.part_id if got.part_id is not None else np.zeros(got.nrows, np.uint32)
    assert np.array_equal(gp, wp), (ctx, "part_id")
    assert np.array_equal(got.src_row, want.src_row), (ctx, "src_row")


def compare(ts, oracle, config, batch, ctx=""):
    """`ts`: the device's split of `batch` (a host batch: what the splitter saw) under `config`"""
    names, ids, groups = ref.split(oracle, config, batch)
    assert ts.nrows == batch.nrows, ctx
    assert ts.count == len(names), (ctx, ts.names()[:5], names[:5])
    assert ts.names() == names, ctx
    assert np.array_equal(ts.row_tables(), ids), ctx
    for t, rows in enumerate(groups):
        assert ts.table_rows(t) == len(rows), (ctx, t)
        db = ts.batch(t)
        want = ref.take_rows(batch, rows)
        want.table_name = names[t].split(b"\0")[0].decode("utf-8", "surrogateescape")   # (the view's table name is a C string: a name holding a NUL byte is cut there)
        assert_same_batch(db.download(), want, (ctx, names[t]))
        if getattr(batch, "schema", None) is not None:
            assert db.table_schema().triples() == batch.schema.triples(), ctx
    return names


def check(tf, oracle, config, batch, ctx=""):
    ts = tf.table_split(tf.Transformer(T, config), tf.DeviceBatch.upload(batch))
    return compare(ts, oracle, config, batch, ctx)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
WORDS = [b"click", b"view", b"", b"scroll/down", None, "нажатие".encode(), b"x" * 9]


def mixed_batch(n, ntables=7):
    k = np.arange(n) * 5 % max(ntables, 1)
    cols = [fixed_column("id", "int64", abi.R_INT64, [int(i) * 1000003 for i in range(n)]),
            fixed_column("day", "date", abi.R_TIME, [1370044800 + 86400 * int(x % 3) + 3600 * (i % 24) for i, x in enumerate(k)]),
            text_column("event", "utf8", abi.R_STRING, [WORDS[int(x) % len(WORDS)] for x in k]),
            fixed_column("region", "uint32", abi.R_UINT32, [int(x) // 3 for x in k]),
            text_column("payload", "any", abi.R_JSON, [b'{"i":%d}' % i for i in range(n)])]
    b = abi.Batch(cols, n, "db", "events")
    b.schema = abi.Schema.of([["id", "int64", True], ["day", "date", False], ["event", "utf8", False], ["region", "uint32", False], ["payload", "any", False]])
    return b


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1000])
def test_row_counts(tf, oracle, n):
    b = mixed_batch(n)
    names = check(tf, oracle, {"columns": ["day", "event", "region"], "splitter": "/"}, b, "n=%d" % n)
    assert len(names) == min(n, 7)
    if n:
        assert names[0] == b"events/2013-06-01/click/0"


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def keyed_batch(keys):
    """one uint32 key per row whose VALUE order is unrelated to its order of appearance, and a text copy of it"""
    n = len(keys)
    vals = [(int(k) * 2654435761 + 12345) % (1 << 32) for k in keys]
    cols = [fixed_column("k", "uint32", abi.R_UINT32, vals), text_column("s", "utf8", abi.R_STRING, [b"key-%d" % v for v in vals]),
            fixed_column("row", "int32", abi.R_INT32, list(range(n)))]
    return abi.Batch(cols, n, "db", "t")


@pytest.mark.parametrize("ntables,n", [(1, 130), (2, 130), (65, 300), (300, 300)])
def test_table_counts(tf, oracle, ntables, n):
    b = keyed_batch([i * 7 % ntables for i in range(n)])
    for columns in (["k"], ["s"], ["s", "k"]):
        names = check(tf, oracle, {"columns": columns, "splitter": "_"}, b, (ntables, columns))
        assert len(names) == ntables


def test_interleaved_first_appearances(tf, oracle):
    """257 tables over 4 096 rows, new names turning up between repeats all along: id order != slot order != value order"""
    rng = np.random.RandomState(257)
    keys = rng.randint(0, 257, 4096)
    first = [int(np.flatnonzero(keys == k)[0]) for k in range(257)]
    assert len(set(keys.tolist())) == 257 and max(first) > 1000
    names = check(tf, oracle, {"columns": ["k"]}, keyed_batch(keys))
    assert len(names) == 257
    vals = [int(nm.split(b"/")[1]) for nm in names]
    assert vals != sorted(vals)


# ---- component types ------------------------------------------------------------------------------------------------------------------
I64_MIN, U64_MAX = -(1 << 63), (1 << 64) - 1


def typed_batch():
    n = 8
    t0 = 1693490347   # 2023-08-31T13:59:07Z = 16:59:07+03:00
    secs = [t0, t0, 0, -1, 253402300799, t0 + 86400, None, t0]
    nanos = [0, 123456789, 0, 999999999, 0, 500000000, 0, 1000]
    cols = [fixed_column("i8", "int8", abi.R_INT8, [-128, 127, 0, -1, 5, 5, None, 7]),
            fixed_column("i16", "int16", abi.R_INT16, [-32768, 32767, 0, -1, 5, 5, None, 7]),
            fixed_column("i32", "int32", abi.R_INT32, [-(1 << 31), (1 << 31) - 1, 0, -1, 5, 5, None, 7]),
            fixed_column("i64", "int64", abi.R_INT64, [I64_MIN, (1 << 63) - 1, 0, -1, 1000000000, 999999999999, None, I64_MIN]),
            fixed_column("u8", "uint8", abi.R_UINT8, [0, 255, 1, 1, 5, 5, None, 7]),
            fixed_column("u16", "uint16", abi.R_UINT16, [0, 65535, 1, 1, 5, 5, None, 7]),
            fixed_column("u32", "uint32", abi.R_UINT32, [0, (1 << 32) - 1, 1, 1, 5, 5, None, 7]),
            fixed_column("u64", "uint64", abi.R_UINT64, [0, U64_MAX, 1 << 63, 10000000000000000000, 5, 5, None, U64_MAX]),
            fixed_column("b", "boolean", abi.R_BOOL, [True, False, True, True, False, False, None, True]),
            fixed_column("f32", "float", abi.R_FLOAT32, [2.71828, 1e21, 1e-5, 0.0, -0.0, 16777216.0, None, 2.71828]),
            fixed_column("f64", "double", abi.R_FLOAT64, [3.14, 1e21, 1e-5, 1e20, -0.0, 123456789.125, None, 3.14]),
            text_column("s", "utf8", abi.R_STRING, [b"hello", b"", b"hello", "мир".encode(), b"a/b", b"<nil>", None, b"hello"]),
            text_column("by", "string", abi.R_BYTES, [b"\x00\x01", b"", b"raw", b"\xff\xfe", b"a/b", b"<nil>", None, b"\x00\x01"]),
            text_column("num", "double", abi.R_JSONNUM, [b"1.50", b"-0", b"1e400", b"12345678901234567890", b"0", b"0", None, b"1.50"]),
            text_column("js", "any", abi.R_JSON, [b'{"a":1}', b"[]", b"null", b'"s"', b"1", b"1", None, b'{"a":1}']),
            fixed_column("d", "date", abi.R_TIME, secs, nanos), fixed_column("dt", "datetime", abi.R_TIME, secs, nanos),
            fixed_column("ts", "timestamp", abi.R_TIME, secs, nanos), fixed_column("tstr", "utf8", abi.R_TIME, secs, nanos),
            fixed_column("iv", "interval", abi.R_DURATION, [0, 1, 1500000000, -90000000000, 3600000000000, I64_MIN, None, 0]),
            fixed_column("anyint", "any", abi.R_INT64, [1, 2, 1, None, 2, 1, None, 1])]
    return abi.Batch(cols, n, "db", "typed")


def test_component_types(tf, oracle):
    b = typed_batch()
    db = tf.DeviceBatch.upload(b)
    seen = {}
    for c in b.cols:
        cfg = {"columns": [c.name], "splitter": "|"}
        ts = tf.table_split(tf.Transformer(T, cfg), db)
        seen[c.name] = compare(ts, oracle, cfg, b, c.name)
    # the forms that are easy to get wrong, as the reference prints them
    assert seen["i64"][0] == b"typed|-9223372036854775808" and b"typed|18446744073709551615" in seen["u64"]
    assert seen["f32"][:3] == [b"typed|2.71828", b"typed|1e+21", b"typed|1e-05"] and seen["f64"][:4] == [b"typed|3.14", b"typed|1e+21", b"typed|1e-05", b"typed|1e+20"]
    assert seen["d"][0] == b"typed|2023-08-31" and seen["ts"][1] == b"typed|2023-08-31T13:59:07.123456789Z"
    assert seen["tstr"][0] == b"typed|2023-08-31 13:59:07 +0000 UTC" and b"typed|1.5s" in seen["iv"]
    assert b"typed|<nil>" in seen["s"] and b"typed|null" in seen["js"] and b"typed|null" in seen["anyint"] and b"typed|<nil>" not in seen["anyint"]
    assert len(seen["d"]) == 6   # rows 0, 1 and 7 share a day; nil, the epoch, its eve, year 9999 and the next day are their own
    # all of them in one name
    check(tf, oracle, {"columns": [c.name for c in b.cols], "splitter": ""}, b, "all")


def test_refused_value_forms(tf):
    n = 3
    for col in (text_column("x", "utf8", abi.R_BYTES, [b"a"] * n), text_column("x", "any", abi.R_STRING, [b"a"] * n),
                fixed_column("x", "any", abi.R_FLOAT64, [1.5] * n)):
        with pytest.raises(tf.TfgpuError) as ei:
            tf.table_split(tf.Transformer(T, {"columns": ["x"]}), tf.DeviceBatch.upload(abi.Batch([col], n, "db", "t")))
        assert ei.value.code == tf.ERR_UNSUPPORTED and T in str(ei.value) and "column x" in str(ei.value)
        # a column the name does not read is not looked at
        assert tf.table_split(tf.Transformer(T, {"columns": ["y"]}), tf.DeviceBatch.upload(abi.Batch([col], n, "db", "t"))).names() == [b"t"]


# ---- name layout ------------------------------------------------------------------------------------------------------------------------
def layout_batch():
    lens = [0, 7, 8, 9, 255, 256, 257, 7, 0, 8]
    cells = [bytes((65 + (i + j) % 26) for j in range(ln)) for i, ln in enumerate(lens)]
    cells[7], cells[8], cells[9] = cells[1], cells[0], b"\xff\xfe/\xc3"   # repeats of the 7-byte and the empty cell; invalid UTF-8
    n = len(cells)
    cols = [text_column("txt", "utf8", abi.R_STRING, cells), fixed_column("a", "int32", abi.R_INT32, [i % 2 for i in range(n)]),
            fixed_column("z", "int64", abi.R_INT64, list(range(n)))]
    b = abi.Batch(cols, n, "db", "layout")
    # the TableSchema's order differs from the batch's, and it has two columns the batch lacks
    b.schema = abi.Schema.of([["z", "int64", True], ["lost", "utf8", False], ["a", "int32", False], ["lostany", "any", False], ["txt", "utf8", False]])
    return b


@pytest.mark.parametrize("config", [
    {"columns": ["txt"]},                                              # cells of 0 / 7 / 8 / 9 / 255 / 256 / 257 bytes, an invalid-UTF-8 cell; no splitter given
    {"columns": ["a", "nosuch", "txt"], "splitter": ""},              # a configured name the schema lacks: nothing, not even a splitter; the empty splitter is "/"
    {"columns": ["lost", "a", "lostany"], "splitter": "_"},           # schema columns the batch lacks: <nil>, and null under any
    {"columns": ["a", "txt", "a", "a"], "splitter": "€"},             # a repeated name; a three-byte splitter
    {"columns": ["txt", "a"], "splitter": "€€"},
    {"columns": [], "splitter": "_"},                                  # no columns: one table, the batch's own name
    {"columns": ["nosuch"]},
], ids=lambda c: ",".join(c["columns"]) + "|" + c.get("splitter", "-"))
def test_name_layout(tf, oracle, config):
    b = layout_batch()
    names = check(tf, oracle, config, b)
    b.table_name = ""                                                   # an empty table name is no component
    names0 = check(tf, oracle, config, b, "no table name")
    sp = (config.get("splitter") or "/").encode()
    assert all(nm.startswith(b"layout") for nm in names)
    assert names0 == [nm[len(b"layout" + sp):] if nm != b"layout" else b"" for nm in names]


def test_a_batch_without_a_table_schema(tf, oracle):
    """no TableSchema: the batch's own columns stand in for it (names and DataTypes)"""
    b = layout_batch()
    b.schema = None
    names = check(tf, oracle, {"columns": ["z", "lost", "a"], "splitter": "."}, b)
    assert names[0] == b"layout.0.0" and len(names) == b.nrows


# ---- two value tuples, one name ---------------------------------------------------------------------------------------------------------
def ambiguous_batch():
    p = [b"a/b", b"a", b"a/b", b"a", b"x", b"", b"/", b"a/b/c"]
    q = [b"c", b"b/c", b"c", b"b/c", b"y", b"/", b"", b""]
    return abi.Batch([text_column("p", "utf8", abi.R_STRING, p), text_column("q", "utf8", abi.R_STRING, q), fixed_column("i", "int32", abi.R_INT32, list(range(8)))], 8, "db", "t")


def test_ambiguous_joins_land_in_one_table(tf, oracle):
    names = check(tf, oracle, {"columns": ["p", "q"], "splitter": "/"}, ambiguous_batch())
    assert names == [b"t/a/b/c", b"t/x/y", b"t///", b"t/a/b/c/"]          # rows 0-3 are ONE table, and so are rows 5 and 6
    # a nil and a text cell that reads "<nil>"
    b = abi.Batch([text_column("p", "utf8", abi.R_STRING, [None, b"<nil>", b"nil", None])], 4, "db", "t")
    assert check(tf, oracle, {"columns": ["p"]}, b) == [b"t/<nil>", b"t/nil"]
    # seconds of one day under DataType date, and bools held as other non-zero bytes
    day = fixed_column("d", "date", abi.R_TIME, [86400 * 19000 + s for s in (0, 1, 86399, 86400)])
    flag = abi.Column("f", "boolean", abi.R_BOOL, values=np.array([1, 2, 255, 0], np.uint8))
    b = abi.Batch([day, flag], 4, "db", "t")
    assert len(check(tf, oracle, {"columns": ["d"]}, b)) == 2
    ts = tf.table_split(tf.Transformer(T, {"columns": ["f"]}), tf.DeviceBatch.upload(b))
    assert ts.names() == [b"t/true", b"t/false"] and ts.row_tables().tolist() == [0, 0, 0, 1]


def test_ambiguous_joins_across_integer_columns(tf, oracle):
    """A component that prints injectively does not make the JOINED name injective: rows whose integer columns differ can still print one name.
    Only a difference in exactly one such column, everything else equal, settles "another table" without the texts."""
    b = abi.Batch([text_column("b", "utf8", abi.R_STRING, [b"x", b"x/5", b"x", b"x", b"x/5"]), fixed_column("a", "int64", abi.R_INT64, [5, 6, 5, 7, 6]),
                   text_column("c", "utf8", abi.R_STRING, [b"6/y", b"y", b"6/y", b"6/y", b"y"])], 5, "db", "t")
    assert check(tf, oracle, {"columns": ["b", "a", "c"], "splitter": "/"}, b) == [b"t/x/5/6/y", b"t/x/7/6/y"]
    # two integer columns and a splitter that is a digit: (1, 11) and (11, 1) both print t11111
    b = abi.Batch([fixed_column("a", "int32", abi.R_INT32, [1, 11, 1, 2, 11]), fixed_column("c", "uint16", abi.R_UINT16, [11, 1, 11, 11, 2])], 5, "db", "t")
    assert check(tf, oracle, {"columns": ["a", "c"], "splitter": "1"}, b) == [b"t11111", b"t12111", b"t11112"]
    # a name configured twice over a differing integer: two differing components, still two names
    assert check(tf, oracle, {"columns": ["a", "a"], "splitter": "1"}, b) == [b"t1111", b"t111111", b"t1212"]
    # an integer against a nil in another column
    b = abi.Batch([fixed_column("a", "int32", abi.R_INT32, [1, 2, 1, None]), text_column("s", "utf8", abi.R_STRING, [None, b"<nil>", b"<nil>", b"1"])], 4, "db", "t")
    assert check(tf, oracle, {"columns": ["a", "s"], "splitter": "/"}, b) == [b"t/1/<nil>", b"t/2/<nil>", b"t/<nil>/1"]


def test_forty_tables_over_300_rows(tf, oracle):
    b = keyed_batch([(i * i + 3 * i) % 40 for i in range(300)])
    want = len({(i * i + 3 * i) % 40 for i in range(300)})
    assert len(check(tf, oracle, {"columns": ["s"]}, b)) == want
    assert len(check(tf, oracle, {"columns": ["k", "s"], "splitter": "-"}, b)) == want


def test_equal_hashes_are_settled_by_the_name_texts():
    """With TFGPU_TABLESPLIT_WEAK_HASH=1 the 128-bit hash keeps two bits: nearly every pair of names collides and only the raw-value and text compares
    keep the tables apart — the results must still be the restatement's (own process: the switch is read once)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFGPU_TABLESPLIT_WEAK_HASH="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "ambiguous_joins or forty_tables"], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "3 passed" in r.stdout, r.stdout[-500:]


# ---- what a row carries along -----------------------------------------------------------------------------------------------------------
def cdc_batch(n=130):
    b = mixed_batch(n)
    b.kind = np.array([i % 3 for i in range(n)], np.uint8)                # inserts, updates, deletes
    b.part_id = np.array([i * 7 % 11 for i in range(n)], np.uint32)
    b.old_keys = [fixed_column("id", "int64", abi.R_INT64, [None if i % 5 == 0 else i * 3 for i in range(n)])]
    b.old_present = np.array([i % 3 != 0 for i in range(n)], bool)
    return b


def test_kinds_oldkeys_part_id_travel_with_the_rows(tf, oracle):
    check(tf, oracle, {"columns": ["event", "region"], "splitter": "/"}, cdc_batch())


def test_absent_cells_read_nil_and_keep_their_bit(tf, oracle):
    b = cdc_batch(70)
    ab = np.array([i % 4 == 1 for i in range(70)], bool)
    b.col("event").absent = ab
    b.col("region").absent = np.array([i % 10 == 3 for i in range(70)], bool)
    cfg = {"columns": ["event", "region"], "splitter": "/"}
    ts = tf.table_split(tf.Transformer(T, cfg), tf.DeviceBatch.upload(b))
    names = compare(ts, oracle, cfg, b)
    ids = ts.row_tables()
    assert all(names[ids[i]].startswith(b"events/<nil>/") for i in np.flatnonzero(ab))
    t = int(ids[1])
    got = ts.batch(t).download()
    assert got.col("event").absent is not None and got.col("event").absent.any()


def test_input_that_is_still_a_selection(tf, oracle):
    b = mixed_batch(257)
    flt = ("filter_rows", {"filter": "id > 100000000"})
    kept = oracle.apply_chain([oracle.Transformer(*flt)], b, b.schema).batch
    kept.schema = b.schema
    assert 0 < kept.nrows < b.nrows and kept.src_row is not None
    sel = tf.Transformer(*flt).apply(tf.DeviceBatch.upload(b)).transformed   # the kept rows, not gathered yet
    cfg = {"columns": ["region", "event"], "splitter": "/"}
    ts = tf.table_split(tf.Transformer(T, cfg), sel)
    compare(ts, oracle, cfg, kept)
    # the per-table batches outlive the handle
    parts = [ts.batch(t) for t in range(ts.count)]
    names = ts.names()
    ts.free()
    assert [p.table_id() for p in parts] == [("db", nm.decode()) for nm in names]
    assert sum(p.download().nrows for p in parts) == kept.nrows


def test_apply_split_behind_filter_rows_and_mask_field(tf, oracle):
    b = mixed_batch(257)
    b.col("region").absent = np.array([i in (5, 200) for i in range(257)], bool)   # filter_rows fails the rows that do not list its column
    front = [("filter_rows", {"filter": "region >= 1"}), ("mask_field", {"maskFunctionHash": {"userDefinedSalt": "salt"}, "columns": ["event"]})]
    cfg = {"columns": ["day", "event"], "splitter": "/"}
    want = oracle.apply_chain([oracle.Transformer(*f) for f in front], b, b.schema)
    seen = want.batch
    seen.schema = want.schema
    assert 0 < seen.nrows < b.nrows
    ts = tf.apply_split([tf.Transformer(*f) for f in front] + [tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b))
    names = compare(ts, oracle, cfg, seen)                                          # src_row points into the original batch
    assert len(names[0]) == len(b"events/2013-06-01/") + 64                         # the masked event: a hex digest
    assert sorted((e[0], e[1]) for e in ts.errors) == sorted((e[0], abi.ROWERR[e[1]]) for e in want.errors) and len(ts.errors) == 2
    assert {e[2] for e in ts.errors} == {0}
    # each table's batch goes on through tfgpu_apply like any other
    first = ts.batch(0)
    out = tf.Transformer("convert_to_string", {"columns": {"includeColumns": ["^id$"]}}).apply(first).transformed.download()
    assert out.nrows == ts.table_rows(0) and out.table_name == names[0].decode() and out.col("id").repr == abi.R_STRING


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(tf, fn):
    with pytest.raises(tf.TfgpuError) as ei:
        fn()
    assert ei.value.code == tf.ERR_UNSUPPORTED, str(ei.value)
    return str(ei.value)


def test_refusals(tf):
    split = tf.Transformer(T, {"columns": ["event"]})
    flt = tf.Transformer("filter_rows", {"filter": "id >= 0"})
    b = mixed_batch(65)
    for kind in (abi.K_OTHER, abi.K_SYNCHRONIZE):
        b.kind = np.zeros(65, np.uint8)
        b.kind[64] = kind
        assert "non-row kinds" in _refused(tf, lambda: tf.table_split(split, tf.DeviceBatch.upload(b)))
    b.kind = None
    db = tf.DeviceBatch.upload(b)
    assert "tfgpu_apply_split" in _refused(tf, lambda: tf.apply_chain([flt, split], db))
    assert "tfgpu_apply_split" in _refused(tf, lambda: split.apply(db))
    assert "tfgpu_tablesplit_batch" in _refused(tf, lambda: tf.apply_split([split, flt], db))
    assert "tfgpu_tablesplit_batch" in _refused(tf, lambda: tf.apply_split([flt, split, split], db))
    with pytest.raises(tf.TfgpuError) as ei:
        tf.apply_split([flt], db)
    assert ei.value.code == tf.ERR_INVALID
    with pytest.raises(tf.TfgpuError) as ei:
        tf.table_split(flt, db)
    assert ei.value.code == tf.ERR_INVALID
    # rows that carry their own ColumnNames order (a collapsed TOAST batch)
    from collapse_cases import batch_from_items
    items = [{"kind": "update", "keys": ["id"], "names": ["id", "b"], "values": [["int64", 1], ["string", "b0"]]},
             {"kind": "update", "keys": ["id"], "names": ["id", "s"], "values": [["int64", 1], ["string", "a1"]]}]
    ordered = tf.collapse(tf.DeviceBatch.upload(batch_from_items(items, names=["id", "s", "b"])[0]))
    assert ordered.download().col_order is not None
    assert "col_order" in _refused(tf, lambda: tf.table_split(tf.Transformer(T, {"columns": ["s"]}), ordered))
