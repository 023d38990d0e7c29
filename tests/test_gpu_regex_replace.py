"""regex_replace_transformer on the device (tf_regex.hip) against the plain-Python restatement (tests/regex_ref.py), cell for cell:
bytes, offsets, validity, dtype and repr.

The kernel stages no text tile: a lane walks its cell in HBM.  The sizes at which its code takes another path are the 8-byte word of
the copies (7 / 8 / 9), a wave and a workgroup of cells (63 / 64 / 65 / 257 rows), and where the lanes' thread lists live: in LDS with 256,
128 or 64 lanes per workgroup, or in the HBM workspace (long programs, many capture slots).  The cell lengths 63 / 64 / 65 / 255 / 256 /
257 and one of 1000 bytes stand where the issue's tile-1 / tile / tile+1 / longer-than-a-tile cells would."""
import ctypes as C
import random

import numpy as np
import pytest

import regex_ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
T = "regex_replace_transformer"


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


def assert_same(got: abi.Batch, want: abi.Batch, ctx=""):
    assert got.nrows == want.nrows, ctx
    assert [c.name for c in got.cols] == [c.name for c in want.cols], ctx
    for a, b in zip(got.cols, want.cols):
        assert (a.dtype, a.repr) == (b.dtype, b.repr), (ctx, a.name)
        va = a.validity if a.validity is not None else np.ones(got.nrows, bool)
        vb = b.validity if b.validity is not None else np.ones(want.nrows, bool)
        assert np.array_equal(va, vb), (ctx, a.name, "validity")
        if a.repr in abi.VAR_REPRS:
            if not np.array_equal(a.offsets, b.offsets) or bytes(a.data[: int(a.offsets[-1])]) != bytes(b.data[: int(b.offsets[-1])]):
                for i in range(got.nrows):
                    assert a.get_bytes(i) == b.get_bytes(i), (ctx, a.name, "row %d" % i)
                assert np.array_equal(a.offsets, b.offsets), (ctx, a.name, "offsets")
        else:
            assert np.array_equal(a.values[va], b.values[vb]), (ctx, a.name, "values")


def device_copy(tf, db):
    """the same batch uploaded again from DEVICE memory (tfgpu_batch.mem = TFGPU_MEM_DEVICE)"""
    v = db.view()
    h = C.c_void_p()
    tf._check(tf.load().tfgpu_batch_upload(C.byref(v), C.byref(h)))
    return tf.DeviceBatch(h)


def run(tf, config, batch, from_device=False):
    t = tf.Transformer(T, config)
    db = tf.DeviceBatch.upload(batch)
    if from_device:
        db = device_copy(tf, db)
    res = t.apply(db)
    assert not res.errors
    return res.transformed.download()


def check(tf, config, batch, ctx="", from_device=False):
    want = regex_ref.apply_batch(config, batch)
    got = run(tf, config, batch, from_device)
    assert_same(got, want, (ctx, config.get("regexMatch"), config.get("replaceRule")))
    return got


def one_column(cells, dtype="utf8", repr_=abi.R_STRING):
    return abi.Batch([text_column("s", dtype, repr_, cells)], len(cells), "db", "t")


LONG = (b"ab_c@" * 200)                       # 1000 bytes, matches all along, one of them across every 8 / 64 / 256-byte boundary
CELLS = [b"", None, b"a", b"_", b"\xff", b"abc", b"abcdef", b"def", "日".encode(), b"value_1", b"a@b#c&d_", b"_start", b"end_", b"no match here",
         b"x" * 6 + b"_", b"x" * 7 + b"_", b"x" * 8 + b"_",                                  # 7 / 8 / 9 bytes, the match in the last byte
         b"x" * 62 + b"_", b"x" * 63 + b"_", b"x" * 64 + b"_", b"_" + b"x" * 254, b"x" * 255 + b"_", b"x" * 256 + b"_",   # 63 / 64 / 65 / 255 / 256 / 257
         b"x" * 60 + b"____" + b"x" * 3, b"x" * 62 + b"12345" + b"y" * 190 + b"678",            # matches across the 64- and 256-byte marks
         LONG, "é_ü".encode(), "a€b_\U0001F600@".encode(), b"\x80_\xbf", b"\xe2\x82_", b"\xf0\x9f\x98_", b"_\xc3", b"\xed\xa0\x80_\xc0\x80",
         b"John Doe", b"https://yandex.ru/games/app/99348", b"test123", b"banana", b"a b\tc\nd\x0be\x0cf\rg", b"ab ab a", b"aaa", b"a\na"]
RULES = [("[_@#&]", "-"), ("\\d+", "NUM"), ("a", "b"), ("(\\w+)\\s(\\w+)", "$2, $1"), (".*?/app/(\\d+).*", "$1"),
         ("[a-c]*", "x"), ("b*", "x"), ("", "x"),                                                # Go's documented empty-match behaviour
         ("a|ab", "<$0>"), ("ab|a", "<$0>"),                                                     # priority
         ("a+", "<$0>"), ("a+?", "<$0>"), ("x{2,5}", "<$0>"), ("x{2,5}?", "<$0>"), ("a.*b", "!"), ("a.*?b", "!"),   # greedy against lazy
         ("(a)|(b)", "[$1|$2]"), ("(x)?_", "[${1}]"),                                            # a group that takes no part in the match
         ("(\\w)(\\w)?", "$0${1}$$$1x$2$"), ("_", "$"), ("_", "a longer rule than the match $0 $0"), ("\\w+", ""),   # rule forms; longer and shorter
         (".", "<$0>"), ("[^a]", "."), ("\\W", "<$0>"), ("é|\\xff|€|\U0001F600", "#"),         # runes: multi-byte, and bytes that are none
         ("^a", "^"), ("a$", "$$"), ("\\Aa|a\\z", "E"), ("\\ba", "B"), ("\\Ba", "b"), ("\\s", "_"), ("\\S+", "w"), ("[\\s\\d]+", "_"), ("\\D\\d", "!")]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts(tf, n):
    cells = [CELLS[i % len(CELLS)] for i in range(n)]
    for pat, rule in RULES[:5] + RULES[5:8]:
        check(tf, {"regexMatch": pat, "replaceRule": rule}, one_column(cells), "n=%d" % n)


@pytest.mark.parametrize("k", range(len(RULES)))
def test_rules_over_the_cell_pool(tf, k):
    pat, rule = RULES[k]
    check(tf, {"regexMatch": pat, "replaceRule": rule}, one_column(CELLS))


def test_golden_vectors(tf):
    from util import golden, item_to_batch
    g = golden("regex_replace.json")
    for v in g["empty_match"]:
        out = run(tf, {"regexMatch": v["pattern"], "replaceRule": v["rule"]}, one_column([v["value"].encode()]))
        assert out.cols[0].get_bytes(0).decode() == v["expect"], v
    for v in g["go_semantics"]:   # lazy loops around groups, counted repeats of bodies that can match nothing: Go's answers, derived by hand
        out = run(tf, {"regexMatch": v["pattern"], "replaceRule": v["rule"]}, one_column([v["value"].encode()]))
        assert out.cols[0].get_bytes(0).decode() == v["expect"], v
    for v in g["replace"]:
        if v["value"][0] == "int64" and v["typ"] == "utf8":
            continue  # an int64 under a utf8 column: no such column form
        schema = abi.Schema.of([["c", v["typ"], False]])
        b = abi.batch_from_rows(schema, ["c"], [[v["value"]]], "db", "t")
        out = run(tf, {"regexMatch": v["pattern"], "replaceRule": v["rule"]}, b)
        assert abi.batch_rows(out) == [[abi.norm_value(v["expect"])]], v["name"]
    for case in g["batch"]:
        b, schema = item_to_batch(case["item"])
        out = run(tf, case["config"], b)
        if case["expect_values"] is None:
            assert out.nrows == 0
        else:
            assert abi.batch_rows(out) == [[abi.norm_value(x) for x in case["expect_values"]]], case["name"]


def mixed_batch(n):
    cells = [CELLS[i % len(CELLS)] for i in range(n)]
    some = [c for c in cells]
    cols = [text_column("s", "utf8", abi.R_STRING, some), text_column("b", "string", abi.R_BYTES, some), text_column("a", "any", abi.R_STRING, some),
            text_column("u8b", "utf8", abi.R_BYTES, some), text_column("other", "utf8", abi.R_STRING, some),
            abi.Column("i", "int64", abi.R_INT64, values=np.arange(n, dtype=np.int64) * 1234567),
            text_column("j", "any", abi.R_JSON, [b'{"a_b":1}'] * n)]
    return abi.Batch(cols, n, "db", "t")


CFG = {"regexMatch": "[_@#&]|\\d+", "replaceRule": "<$0>", "columns": {"includeColumns": ["^s$", "^b$", "^a$", "^u8b$", "^i$", "^j$"]}}


def test_column_gate(tf):
    """utf8 + Go string and string + []byte are rewritten; `any`, utf8 held as []byte, unmatched names and integers pass through untouched"""
    b = mixed_batch(65)
    got = check(tf, CFG, b)
    for name in ("a", "u8b", "other", "i", "j"):
        c, o = b.col(name), got.col(name)
        if c.repr in abi.VAR_REPRS:
            assert bytes(c.data) == bytes(o.data[: len(c.data)]) and np.array_equal(c.offsets, o.offsets)
    assert bytes(got.col("s").data) != bytes(b.col("s").data) and bytes(got.col("s").data[: int(got.col("s").offsets[-1])]) == bytes(got.col("b").data[: int(got.col("b").offsets[-1])])
    # a column in which nothing matches keeps its bytes
    check(tf, {"regexMatch": "ZZZ", "replaceRule": "-"}, b)


def test_host_and_device_uploads(tf):
    b = mixed_batch(64)
    check(tf, CFG, b, "host")
    check(tf, CFG, b, "device", from_device=True)


def test_typ_is_taken_by_position(tf):
    """item.TableSchema.Columns()[i]: the i-th SCHEMA column's type gates the i-th value, whatever the names say"""
    cells = [b"a_b", b"c_d", None, b"_"]
    b = abi.Batch([text_column("p", "any", abi.R_STRING, cells), text_column("q", "utf8", abi.R_STRING, cells)], len(cells), "db", "t")
    b.schema = abi.Schema.of([["q", "utf8", False], ["p", "any", False]])
    cfg = {"regexMatch": "_", "replaceRule": "-"}
    got = check(tf, cfg, b)
    assert got.col("p").get_bytes(0) == b"a-b" and got.col("q").get_bytes(0) == b"a_b"   # by name it would be the other way round
    # string / utf8 swapped by position: neither Go type fits the type it is judged by
    b = abi.Batch([text_column("x", "utf8", abi.R_STRING, cells), text_column("y", "string", abi.R_BYTES, cells)], len(cells), "db", "t")
    b.schema = abi.Schema.of([["y", "string", False], ["x", "utf8", False]])
    got = check(tf, cfg, b)
    assert got.col("x").get_bytes(0) == b"a_b" and got.col("y").get_bytes(0) == b"a_b"


def test_more_columns_than_the_schema_is_refused(tf):
    cells = [b"a_b"]
    b = abi.Batch([text_column("p", "utf8", abi.R_STRING, cells), text_column("q", "utf8", abi.R_STRING, cells)], 1, "db", "t")
    b.schema = abi.Schema.of([["p", "utf8", False]])
    with pytest.raises(IndexError):
        regex_ref.apply_batch({"regexMatch": "_", "replaceRule": "-"}, b)
    with pytest.raises(tf.TfgpuError) as ei:
        run(tf, {"regexMatch": "_", "replaceRule": "-"}, b)
    assert ei.value.code == tf.ERR_UNSUPPORTED and "more columns than its TableSchema" in str(ei.value)


def test_unmatched_table_gives_no_rows(tf):
    b = mixed_batch(65)
    for tables in ({"excludeTables": ["^t$"]}, {"includeTables": ["^db\\.t$"]}):   # (the name alone is matched: "db.t" is not it)
        cfg = dict(CFG, tables=tables)
        assert regex_ref.apply_batch(cfg, b) is None
        t = tf.Transformer(T, cfg)
        res = t.apply(tf.DeviceBatch.upload(b))
        assert res.transformed.nrows == 0 and not res.errors
        assert res.transformed.download().nrows == 0


def test_input_that_is_still_a_selection(tf, oracle):
    b = mixed_batch(257)
    schema = abi.Schema.of([[c.name, c.dtype, False] for c in b.cols])
    flt = ("filter_rows", {"filter": "i > 100000000"})
    kept = oracle.apply_chain([oracle.Transformer(*flt)], b, schema).batch
    assert 0 < kept.nrows < b.nrows
    want = regex_ref.apply_batch(CFG, kept)
    f, t = tf.Transformer(*flt), tf.Transformer(T, CFG)
    sel = f.apply(tf.DeviceBatch.upload(b)).transformed   # the kept rows, not gathered yet
    assert_same(t.apply(sel).transformed.download(), want, "apply on a selection")
    assert_same(tf.apply_chain([f, t], tf.DeviceBatch.upload(b)).transformed.download(), want, "chain")


def test_rows_with_their_own_column_names_are_refused(tf):
    """The rule is positional (the i-th value against the i-th schema column): a batch with an ABSENT cell, and one whose rows carry their own
    ColumnNames order, are refused by name before anything is computed (apply_plan's entry protocol) — mask_field, which walks each row's
    own names, still takes the first and refuses only the second."""
    from collapse_cases import batch_from_items
    col = text_column("s", "utf8", abi.R_STRING, [b"ab", None, b"cd"])
    col.absent = np.array([False, True, False])   # row 1 does not list the column (it reads nil)
    ragged = tf.DeviceBatch.upload(abi.Batch([col], 3, "db", "t"))
    items = [{"kind": "update", "keys": ["id"], "names": ["id", "b"], "values": [["int64", 1], ["string", "b0"]]},
             {"kind": "update", "keys": ["id"], "names": ["id", "s"], "values": [["int64", 1], ["string", "a1"]]}]
    ordered = tf.collapse(tf.DeviceBatch.upload(batch_from_items(items, names=["id", "s", "b"])[0]))   # merged names id, b, s: not the batch's order
    assert ordered.download().col_order.tolist() == [[0, 2, 1]]
    rx, mask = tf.Transformer(T, CFG), tf.Transformer("mask_field", {"columns": ["s"], "maskFunctionHash": {"userDefinedSalt": "salt"}})
    for db in (ragged, ordered):
        with pytest.raises(tf.TfgpuError, match="ABSENT cells") as e:
            rx.apply(db)
        assert e.value.code == tf.ERR_UNSUPPORTED
    got = mask.apply(ragged).transformed.download()
    assert got.nrows == 3 and got.cols[0].absent.tolist() == [False, True, False] and [len(got.cols[0].get_bytes(i)) for i in (0, 2)] == [64, 64]
    with pytest.raises(tf.TfgpuError, match="ABSENT cells") as e:
        mask.apply(ordered)
    assert e.value.code == tf.ERR_UNSUPPORTED


def test_chain_to_json_each_row(tf, oracle):
    n = 257
    cells = [CELLS[i % len(CELLS)] for i in range(n)]
    cells = [c if c is None else c.decode("utf-8", "replace").encode() for c in cells]   # (JSON output: valid UTF-8 in, so that the serializers agree on it)
    b = abi.Batch([abi.Column("i", "int64", abi.R_INT64, values=np.arange(n, dtype=np.int64)), text_column("s", "utf8", abi.R_STRING, cells),
                   text_column("keep", "utf8", abi.R_STRING, cells)], n, "db", "t")
    schema = abi.Schema.of([["i", "int64", True], ["s", "utf8", False], ["keep", "utf8", False]])
    flt = ("filter_rows", {"filter": "i >= 3 AND i < 250"})
    cfg = {"regexMatch": "(\\w+)\\s(\\w+)|[_@#&]", "replaceRule": "$2-$1", "columns": {"includeColumns": ["^s$"]}}
    kept = oracle.apply_chain([oracle.Transformer(*flt)], b, schema)
    want = oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, regex_ref.apply_batch(cfg, kept.batch), kept.schema)
    res = tf.apply_chain([tf.Transformer(*flt), tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b))
    assert not res.errors
    assert bytes(tf.serialize(abi.FMT_CH_JSON_EACH_ROW, res.transformed).download()) == bytes(want)


def test_both_homes_of_the_thread_lists(tf):
    """short programs keep the lanes' thread lists in LDS (256, 128 or 64 lanes a workgroup), long ones or many capture slots in the HBM workspace"""
    cells = [CELLS[i % len(CELLS)] for i in range(130)]
    for pat, rule in [("_", "-"),                                                       # 2 instructions: 256 lanes
                      ("(\\w+)\\s(\\w+)", "$2, $1"),                                    # 6 slots: 128 lanes or fewer
                      ("(a)(b)?(c)?(d)?(e)?(f)?(x+)(_)?", "$8$7$6$5$4$3$2$1"),          # 18 slots: 64 lanes
                      ("(?:ab_c@|x{10,40}_|[a-c]{1,20}\\d)+", "<$0>"),                  # a long program: the HBM workspace
                      ("(a)?(b)?(c)?(d)?(e)?(f)?(g)?(h)?(i)?(j)?(k)?(l)?(m)?(n)?(o)?(\\w)", "$16$15$14$13$12$11$10$9$8$7$6$5$4$3$2$1")]:   # 34 slots
        check(tf, {"regexMatch": pat, "replaceRule": rule}, one_column(cells))


def _refusal(tf, config, batch):
    t = tf.Transformer(T, config)
    with pytest.raises(tf.TfgpuError) as ei:
        t.apply(tf.DeviceBatch.upload(batch))
    assert ei.value.code == tf.ERR_UNSUPPORTED, str(ei.value)
    return str(ei.value)


def test_a_result_column_of_4gib_is_refused(tf):
    """`.` with a 1 KiB rule multiplies the text by 1024: 4100 cells of 1 KiB would be a 4.2 GB column.  Refused after the length pass
    (which sums in 64 bits), before anything is allocated or written."""
    cells = [b"y" * 1024] * 4100
    assert "split the batch" in _refusal(tf, {"regexMatch": ".", "replaceRule": "r" * 1024}, one_column(cells))
    # (the same rule over three such cells goes through)
    check(tf, {"regexMatch": ".", "replaceRule": "r" * 1024}, one_column([b"y" * 1024] * 3))


def test_cell_length_cap(tf):
    """one lane walks a cell: a cell above TFGPU_REGEX_MAX_CELL (1 MiB) sends the batch to the stock transformer; one of exactly 1 MiB is rewritten"""
    assert "TFGPU_REGEX_MAX_CELL" in _refusal(tf, {"regexMatch": "_", "replaceRule": "-"}, one_column([b"a_b", b"x" * (1 << 20) + b"_"]))
    got = run(tf, {"regexMatch": "_", "replaceRule": "--"}, one_column([b"a_b", b"x" * ((1 << 20) - 1) + b"_"]))
    assert got.cols[0].get_bytes(0) == b"a--b" and got.cols[0].get_bytes(1)[-3:] == b"x--" and len(got.cols[0].get_bytes(1)) == (1 << 20) + 1


def test_search_step_budget(tf):
    """a(?:.*c)? restarts a search that runs to the end of the cell from every `a`: quadratic, in Go as here.  A cell may take
    (len + 1) * (program size + 16) + 1024 search steps; past that the batch is refused by name.  Short cells and linear patterns are far below it."""
    cfg = {"regexMatch": "a(?:.*c)?", "replaceRule": "<$0>"}
    check(tf, cfg, one_column([b"a" * 30, b"aaac" * 5, b""]))
    assert "search steps" in _refusal(tf, cfg, one_column([b"a" * 30, b"a" * 4000]))
    check(tf, cfg, one_column([b"a" * 4000 + b"c"]))                     # one search, to the end
    check(tf, {"regexMatch": "x{10,40}_", "replaceRule": "!"}, one_column([b"x" * 4000 + b"_"]))   # bounded look-ahead from every position: len * 41 steps


# ---- the seeded random leg --------------------------------------------------------------------------------------------------------------
ATOMS = ["a", "b", "c", "é", "\\xff", " ", ".", "[ab]", "[^a ]", "[a-cé]", "\\w", "\\s", "\\S", "\\d", "[^\\xff]"]


def gen(rng, depth=0):
    """One pattern of the mandatory subset -> (text, can match the empty string, holds a capturing group).  What it never emits, and why:
    - a * + {n,} whose body can match the empty string (refused by the device: engines differ);
    - a counted repeat {n,m} of such a body: Go unrolls x{1,3} to x(x(x)?)?, Python's engine runs a counted loop and leaves it at the first
      iteration that matched nothing — the captures of the two differ and the restatement could not arbitrate;
    - a lazy loop around a capturing group: CPython's engine reports inverted group spans there (re.search(r'((.*\\B.)+?) ', 'é  b').span(2)
      is (3, 2)), so its answer is no reference;
    - patterns past the program cap (nesting two levels deep, short concatenations)."""
    anchors = ("^", "$", "\\b", "\\B", "\\A", "\\z")

    def atom():
        r = rng.random()
        if depth < 2 and r < 0.25:
            inner, e, _ = gen(rng, depth + 1)
            cap = rng.random() < 0.6
            return ("(" if cap else "(?:") + inner + ")", e, cap or _
        if r < 0.30:
            return rng.choice(anchors), True, False
        return rng.choice(ATOMS), False, False

    def piece():
        a, e, cap = atom()
        if rng.random() < 0.45 or a in anchors:
            return a, e, cap
        if e:
            q = "?"
        elif a[0] == "(":
            q = rng.choice(["?", "*", "+", "{1,3}"])
        else:
            q = rng.choice(["?", "*", "+", "{1,3}", "{2}", "{0,2}", "{2,}"])
        lazy = "?" if rng.random() < 0.35 and not (cap and q in ("*", "+", "{2,}")) else ""
        return a + q + lazy, e or q in ("?", "*", "{0,2}"), cap

    def concat():
        parts = [piece() for _ in range(rng.randint(1, 3 if depth == 0 else 2))]
        return "".join(p[0] for p in parts), all(p[1] for p in parts), any(p[2] for p in parts)

    alts = [concat() for _ in range(1 if rng.random() < 0.65 else rng.randint(2, 3 if depth == 0 else 2))]
    return "|".join(a[0] for a in alts), any(a[1] for a in alts), any(a[2] for a in alts)


def test_seeded_random_patterns(tf):
    rng = random.Random(20240614)
    alphabet = [b"a", b"b", b"c", "é".encode(), b"\xff", b" "]
    cells = [b"".join(rng.choice(alphabet) for _ in range(rng.randint(0, 12))) for _ in range(63)] + [None]
    col = one_column(cells)
    db = tf.DeviceBatch.upload(col)
    refused, wrong = [], []
    for k in range(200):
        pat = gen(rng)[0]
        rule = rng.choice(["x", "", "<$0>", "[$1|$2]", "$2$1", "${1}y"])
        cfg = {"regexMatch": pat, "replaceRule": rule}
        want = regex_ref.apply_batch(cfg, col)
        try:
            t = tf.Transformer(T, cfg)
        except tf.TfgpuError as e:
            refused.append((pat, str(e)))
            continue
        got = t.apply(db).transformed.download()
        try:
            assert_same(got, want, (pat, rule))
        except AssertionError as e:
            wrong.append(str(e)[:600])
    print("random leg: %d patterns, %d refused, %d mismatches" % (200, len(refused), len(wrong)))
    assert not refused, refused[:5]       # the grammar emits the mandatory subset only: the device may refuse none
    assert not wrong, wrong[:5]
