"""filter_rows_by_ids on the device (tf_byids.hip) against the plain-Python restatement (tests/byids_ref.py), row for row after download: which rows
stay, their src_row, kinds, OldKeys with presence, part_id, and every column cell for cell with its nil and ABSENT bits.

The sizes at which the code takes another path: a wave and a workgroup of rows (63 / 64 / 65 / 255 / 256 / 257, and 1025 = five workgroups), cells
around every allowed length (and around the four-byte steps of the hash walk), ID tables on either side of the LDS budget (the two kernels are also
run over the same batch and compared), the JSON string decoder's escapes at and across the last compared byte."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import byids_ref as ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
T = ref.T
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------------
def text_column(name, dtype, repr_, cells):
    """cells: bytes, or None for nil"""
    n = len(cells)
    off = np.zeros(n + 1, np.uint32)
    if n:
        off[1:] = np.cumsum([len(c or b"") for c in cells])
    valid = np.array([c is not None for c in cells], dtype=bool)
    return abi.Column(name, dtype, repr_, offsets=off, data=np.frombuffer(b"".join(c or b"" for c in cells), np.uint8).copy(),
                      validity=None if valid.all() else valid)


def fixed_column(name, dtype, repr_, vals):
    valid = np.array([v is not None for v in vals], dtype=bool)
    a = np.array([0 if v is None else v for v in vals], dtype=abi.REPR_NP[repr_])
    return abi.Column(name, dtype, repr_, values=a, validity=None if valid.all() else valid)


def assert_same_batch(got: abi.Batch, want: abi.Batch, ctx=""):
    """tests/test_gpu_rawdoc.py's comparison; a batch without src_row reads the identity"""
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
            assert np.array_equal(va & ~ab, vb & ~bb), (ctx, what, a.name, "validity")
            ok = va & ~ab
            if a.repr in abi.VAR_REPRS:
                for i in range(got.nrows):
                    if ok[i]:
                        assert a.get_bytes(i) == b.get_bytes(i), (ctx, what, a.name, i)
            else:
                assert np.array_equal(a.values[ok].view(np.uint8), b.values[ok].view(np.uint8)), (ctx, what, a.name, "values")
    cols_equal(got.cols, want.cols, "cols")
    cols_equal(getattr(got, "old_keys", None) or [], getattr(want, "old_keys", None) or [], "old_keys")
    if getattr(want, "old_keys", None):
        assert np.array_equal(got.old_present, want.old_present), (ctx, "old_present")
    wk = want.kind if want.kind is not None else np.zeros(want.nrows, np.uint8)
    gk = got.kind if got.kind is not None else np.zeros(got.nrows, np.uint8)
    assert np.array_equal(gk, wk), (ctx, "kind")
    wp = want.part_id if want.part_id is not None else np.zeros(want.nrows, np.uint32)
    gp = got.part_id if got.part_id is not None else np.zeros(got.nrows, np.uint32)
    assert np.array_equal(gp, wp), (ctx, "part_id")
    ident = np.arange(want.nrows, dtype=np.int32)
    assert np.array_equal(got.src_row if got.src_row is not None else ident, want.src_row if want.src_row is not None else ident), (ctx, "src_row")


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------------
def config_json(config) -> bytes:
    """the config as JSON text; an allowed ID given as bytes goes in byte for byte (json.dumps cannot say 0xFF)"""
    rest = {k: v for k, v in config.items() if k != "allowedIDs"}
    parts = []
    for i in config["allowedIDs"]:
        raw = i if isinstance(i, bytes) else i.encode("utf-8")
        parts.append(b'"' + b"".join(b"\\u%04x" % c if c < 0x20 else b"\\" + bytes([c]) if c in (0x22, 0x5C) else bytes([c]) for c in raw) + b'"')
    return json.dumps(rest).encode()[:-1] + (b", " if rest else b"") + b'"allowedIDs": [' + b", ".join(parts) + b"]}"


def transformer(tf, config):
    t = tf.Transformer.__new__(tf.Transformer)
    t._h = None
    h = C.c_void_p()
    tf._check(tf.load().tfgpu_plan_create(T.encode(), config_json(config), C.byref(h)))
    t._h = h
    return t


def lds_budget():
    with open(os.path.join(ROOT, "transferia_amd", "csrc", "tf_byids.hpp")) as f:
        m = re.search(r"constexpr uint32_t BYIDS_LDS_BUDGET = (\d+)u << (\d+);", f.read())
    return int(m.group(1)) << int(m.group(2))


def image_bytes(ids):
    """the size of the device table of these IDs (tf_byids.hpp): the distinct lengths, three words per slot of a power-of-two table at most half full, the bytes"""
    ids = {i if isinstance(i, bytes) else i.encode() for i in ids}
    cap = 4
    while cap < 2 * len(ids):
        cap *= 2
    return 4 * (len({len(i) for i in ids}) + 3 * cap + (sum(len(i) for i in ids) + 3) // 4)


def kept_on_device(tf, config, db, lds):
    old = os.environ.get("TFGPU_BYIDS_LDS")
    os.environ["TFGPU_BYIDS_LDS"] = "1" if lds else "0"
    try:
        res = tf.apply_chain([transformer(tf, config)], db)
    finally:
        if old is None:
            del os.environ["TFGPU_BYIDS_LDS"]
        else:
            os.environ["TFGPU_BYIDS_LDS"] = old
    assert res.errors == []
    return res.transformed


def check(tf, config, batch, ctx="", device_batch=None, seen=None):
    """the device's Apply of `config` over `batch` against the restatement's, through both kernels.  `seen`: the host batch the filter read, where
    `device_batch` is not simply the upload of `batch`"""
    db = device_batch if device_batch is not None else tf.DeviceBatch.upload(batch)
    want, idx = ref.apply(config, seen if seen is not None else batch)
    got = kept_on_device(tf, config, db, True).download()
    assert_same_batch(got, want, (ctx, "lds"))
    hbm = kept_on_device(tf, config, db, False).download()
    assert_same_batch(hbm, want, (ctx, "hbm"))
    assert np.array_equal(got.src_row, hbm.src_row), ctx
    return got, idx


IDS3 = ["ID1", "ID2_2", "ID4"]


PATTERNS = [b"ID1", b"ID0", b"ID2_2_suffix", b"ID2-", b"", None, b"ID4x", b"id4", b"xID1"]   # IDS3 lets rows 0, 2 and 6 of every nine through


def ids_batch(n):
    cells = [None if PATTERNS[i % 9] is None else PATTERNS[i % 9] + (b"%d" % (i % 7) if PATTERNS[i % 9] else b"") for i in range(n)]
    return abi.Batch([fixed_column("n", "int64", abi.R_INT64, list(range(n))), text_column("id", "utf8", abi.R_STRING, cells)], n, "db", "t")


# ---- row counts ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts(tf, n):
    b = ids_batch(n)
    got, idx = check(tf, {"allowedIDs": IDS3}, b, "n=%d" % n)
    assert idx == [i for i in range(n) if i % 9 in (0, 2, 6)]
    assert got.col("n").values.tolist() == idx


# ---- cell lengths -------------------------------------------------------------------------------------------------------------------------------------
def around(ident: bytes):
    """cells around one ID: empty, one byte short, the ID, one byte more, the ID with its last byte changed, the ID behind another byte"""
    L = len(ident)
    return [b"", ident[:L - 1], ident, ident + b"z", ident[:L - 1] + bytes([ident[L - 1] ^ 1]), b"q" + ident, ident[:L - 1] + b"\x00", ident * 3]


SPECIAL_IDS = [b"a", b"\x00", b"\xff", b"abc", b"a\x00c", b"\xff\xfe\xfd", "é!".encode(), b"abcde", b"ab\x00\xffe", "日é".encode(), "😀".encode() + b"x"]


@pytest.mark.parametrize("L", [1, 3, 5])
def test_cell_lengths_around_an_allowed_length(tf, L):
    ids = [i for i in SPECIAL_IDS if len(i) == L]
    assert len(ids) >= 3
    cells = [c for i in ids for c in around(i)] + [None, b"abcdefgh", b"abc", b"ab", b"a"]
    b = abi.Batch([text_column("s", "utf8", abi.R_STRING, cells), text_column("y", "string", abi.R_BYTES, cells[::-1])], len(cells), "db", "t")
    for cols in (["^s$"], ["^y$"], []):
        cfg = {"allowedIDs": ids, "columns": {"includeColumns": cols}}
        _, idx = check(tf, cfg, b, (L, cols))
        assert 0 < len(idx) < len(cells)
    # ... and with the other lengths allowed beside it: 1, 3 and 5 in one table
    check(tf, {"allowedIDs": SPECIAL_IDS, "columns": {"includeColumns": ["^s$"]}}, b, (L, "all lengths"))
    # an ID longer than every cell
    _, idx = check(tf, {"allowedIDs": [b"abcdefgh" * 40]}, b, (L, "long id"))
    assert idx == []
    _, idx = check(tf, {"allowedIDs": [b"abcdefgh" * 40, b"abcdefgh"]}, b, (L, "long id and a short one"))
    assert len(idx) == 2                                     # the one cell that holds it, in `s` and in `y`


def test_the_empty_id(tf):
    n = 70
    s = text_column("s", "utf8", abi.R_STRING, [None if i % 5 == 0 else b"" if i % 5 == 1 else b"v%d" % i for i in range(n)])
    s.absent = np.array([i % 7 == 3 for i in range(n)], bool)
    b = abi.Batch([s, fixed_column("n", "int32", abi.R_INT32, list(range(n))), text_column("num", "utf8", abi.R_JSONNUM, [b"1"] * n)], n, "db", "t")
    for ids in ([""], ["", "zz"], ["zz", "", "v1"]):
        got, idx = check(tf, {"allowedIDs": ids}, b, ids)
        assert idx == [i for i in range(n) if i % 5 != 0 and i % 7 != 3]      # every string, the empty one too; no nil, no ABSENT cell, no number


# ---- ID counts ------------------------------------------------------------------------------------------------------------------------------------------
def test_id_counts_and_both_kernels(tf):
    budget = lds_budget()
    n = 300
    prefix = b"tenant-0000-0000-0000-"                      # IDs that share a long common prefix
    pool = [prefix + b"%05d" % k for k in range(3000)]
    cells = [pool[(i * 37) % 3000] + b"/suffix" if i % 3 else pool[(i * 37) % 3000][:-1] for i in range(n)]
    b = abi.Batch([text_column("s", "utf8", abi.R_STRING, cells)], n, "db", "t")
    small = [x for x in range(1, 600) if image_bytes(pool[:x]) <= budget]
    below, above = max(small), max(small) + 1                # one count on each side of the LDS budget
    assert image_bytes(pool[:below]) <= budget < image_bytes(pool[:above])
    for count in (1, 3, below, above, 1000, 3000):
        _, idx = check(tf, {"allowedIDs": pool[:count]}, b, count)
        assert idx == [i for i in range(n) if i % 3 and (i * 37) % 3000 < count]
    # 17 distinct lengths in one table
    ids = [b"L" * k + b"%d" % k for k in range(17)]
    assert len({len(i) for i in ids}) == 17
    cells = [ids[i % 17][: len(ids[i % 17]) - (i % 2)] + (b"tail" if i % 4 == 0 else b"") for i in range(n)]
    _, idx = check(tf, {"allowedIDs": ids}, abi.Batch([text_column("s", "string", abi.R_BYTES, cells)], n, "db", "t"), "17 lengths")
    assert 0 < len(idx) < n


def profiled(tf, fn):
    """{timer name: launches} of the library's filter_rows_by_ids timers while fn() runs"""
    tf.synchronize()
    tf.prof_reset()
    tf.prof_enable(True)
    try:
        fn()
        tf.synchronize()
    finally:
        tf.prof_enable(False)
    return {k: n for k, n, _ms in tf.prof_get() if k.startswith("filter_rows_by_ids")}


def test_which_kernel_runs_and_the_table_is_uploaded_once(tf, monkeypatch):
    monkeypatch.delenv("TFGPU_BYIDS_LDS", raising=False)
    budget = lds_budget()
    pool = [b"tenant-0000-0000-0000-%05d" % k for k in range(600)]
    below = max(x for x in range(1, 600) if image_bytes(pool[:x]) <= budget)
    db = tf.DeviceBatch.upload(ids_batch(300))
    for count, kernel in ((1, "filter_rows_by_ids_lds"), (below, "filter_rows_by_ids_lds"), (below + 1, "filter_rows_by_ids_hbm"), (600, "filter_rows_by_ids_hbm")):
        t = transformer(tf, {"allowedIDs": pool[:count]})
        first = profiled(tf, lambda: tf.apply_chain([t], db))
        assert first == {kernel: 1, "filter_rows_by_ids_table_upload": 1}, (count, first)       # the kernel the table's size asks for; the lane's first batch uploads
        again = profiled(tf, lambda: [tf.apply_chain([t], db) for _ in range(3)])
        assert again == {kernel: 3}, (count, again)                                             # ... and the later ones find the table
        other = transformer(tf, {"allowedIDs": pool[:count]})                                   # another plan is another table, whatever it holds
        assert profiled(tf, lambda: tf.apply_chain([other], db)) == {kernel: 1, "filter_rows_by_ids_table_upload": 1}
    monkeypatch.setenv("TFGPU_BYIDS_LDS", "0")                                                  # the switch the comparisons of check() rest on
    t = transformer(tf, {"allowedIDs": pool[:1]})
    assert profiled(tf, lambda: tf.apply_chain([t], db)) == {"filter_rows_by_ids_hbm": 1, "filter_rows_by_ids_table_upload": 1}
    # a lane keeps at most 16 tables: the one used longest ago is uploaded again when its plan comes back
    monkeypatch.delenv("TFGPU_BYIDS_LDS")
    plans = [transformer(tf, {"allowedIDs": [b"id-%d" % k]}) for k in range(17)]
    assert profiled(tf, lambda: [tf.apply_chain([q], db) for q in plans]) == {"filter_rows_by_ids_lds": 17, "filter_rows_by_ids_table_upload": 17}
    assert profiled(tf, lambda: tf.apply_chain([plans[16]], db)) == {"filter_rows_by_ids_lds": 1}
    assert profiled(tf, lambda: tf.apply_chain([plans[0]], db)) == {"filter_rows_by_ids_lds": 1, "filter_rows_by_ids_table_upload": 1}


# ---- reprs ----------------------------------------------------------------------------------------------------------------------------------------------
JSON_CELLS = [b'"ID1"', b'"ID1 and more"', b'"ID"', b'""', b' "ID1"', b'"I\\u00441"', b'"\\u0049\\u0044\\u0031"', b'"ID\\u0031x"',        # plain, \u escapes
              b'"\\"q"', b'"\\\\b"', b'"\\/s"', b'"\\bx"', b'"\\fx"', b'"\\nx"', b'"\\rx"', b'"\\tx"',                                  # each short escape
              b'"\\ud83d\\ude00x"', "\"😀x\"".encode(), b'"\\ud83dx"', b'"\\ude00x"', b'"\\ud83d\\u0041"', b'"\\ud800\\ud83d\\ude00"',       # a pair, lone surrogates
              b'"a\\u00e9x"', "\"aéx\"".encode(), b'"a\\u00e9"', b'"a\\u4e16"', b'"a\xffb"', b'"a\xc3"',                                # the escape straddles the L-th byte
              b'{"ID1":1}', b'["ID1"]', b"17", b"true", b"false", b"null", b"-1.5e3", b"", None]                                               # no string
JSON_IDS = [b"ID1", b"ID", b'"q', b"\\b", b"/s", b"\bx", b"\fx", b"\nx", b"\rx", b"\tx", "😀".encode(), "😀".encode()[:2], "�".encode() + b"x", "�".encode() + b"A",
            "�😀".encode()[:5], b"a\xc3", "aé".encode(), b"a\xe4", "a�".encode()]


def test_reprs(tf):
    cells = [b"ID1", b"ID1x", b"ID", b"", None, b"xID1", b"ID4", b"ID2_2"]
    n = len(cells)
    for dtype in ("utf8", "string", "any"):
        for repr_ in (abi.R_STRING, abi.R_BYTES):
            _, idx = check(tf, {"allowedIDs": IDS3}, abi.Batch([text_column("c", dtype, repr_, cells)], n, "db", "t"), (dtype, repr_))
            assert idx == [0, 1, 6, 7]
    # a json.Number under utf8 never matches, an int column under `string` is skipped, text under a DataType that is none of the three too
    b = abi.Batch([text_column("num", "utf8", abi.R_JSONNUM, [b"ID1", b"1", b"ID4", b"", b"2", b"3", b"4", b"5"]),
                   fixed_column("i", "string", abi.R_INT64, [1, 2, 3, 4, 5, 6, 7, 8]),
                   text_column("d", "int64", abi.R_STRING, cells), fixed_column("t", "utf8", abi.R_BOOL, [1] * n)], n, "db", "t")
    _, idx = check(tf, {"allowedIDs": IDS3 + ["1", "true"]}, b, "never strings")
    assert idx == []


def test_json_cells(tf):
    n = len(JSON_CELLS)
    b = abi.Batch([text_column("j", "any", abi.R_JSON, JSON_CELLS), fixed_column("n", "int32", abi.R_INT32, list(range(n)))], n, "db", "t")
    for dtype in ("any", "utf8", "string"):
        b.cols[0].dtype = dtype
        _, idx = check(tf, {"allowedIDs": [b"ID1"]}, b, dtype)
        assert idx == [0, 1, 4, 5, 6, 7]
    b.cols[0].dtype = "any"
    hits = set()
    for ident in JSON_IDS:                                   # one ID at a time: which cells it lets through is the restatement's to say
        _, idx = check(tf, {"allowedIDs": [ident]}, b, ident)
        assert idx, ident
        hits |= set(idx)
    assert hits == set(range(n - 9)) - {3}                   # every string cell but the empty one was reached by some ID; the non-strings by none
    _, idx = check(tf, {"allowedIDs": JSON_IDS + [b""]}, b, "all, and the empty ID")
    assert idx == list(range(n - 9))
    # the compared text is the decoded string, not the JSON text
    _, idx = check(tf, {"allowedIDs": [b'"ID1', b"I\\u0044", b'{"ID1"', b"nul", b"17", b"tru"]}, b, "json text")
    assert idx == []


# ---- columns --------------------------------------------------------------------------------------------------------------------------------------------
def test_which_column_decides(tf):
    n = 130
    miss = [b"nothing%d" % i for i in range(n)]
    cols = [text_column("a", "utf8", abi.R_STRING, miss), text_column("b", "string", abi.R_BYTES, [b"ID1" if i % 4 == 1 else b"x" for i in range(n)]),
            fixed_column("n", "int64", abi.R_INT64, list(range(n))), text_column("c", "any", abi.R_JSON, [b'"ID4"' if i % 4 == 2 else b"{}" for i in range(n)]),
            text_column("z", "utf8", abi.R_STRING, [b"ID2_2!" if i % 8 == 3 else b"" for i in range(n)])]
    b = abi.Batch(cols, n, "db", "t")
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "second, fourth and last column")
    assert idx == [i for i in range(n) if i % 4 in (1, 2) or i % 8 == 3]
    _, idx = check(tf, {"allowedIDs": IDS3, "columns": {"excludeColumns": ["^b$"]}}, b, "the filter excludes b")
    assert idx == [i for i in range(n) if i % 4 == 2 or i % 8 == 3]
    _, idx = check(tf, {"allowedIDs": ["ID1"], "columns": {"excludeColumns": ["^b$"]}}, b, "... the one column that would match")
    assert idx == []
    _, idx = check(tf, {"allowedIDs": IDS3, "columns": {"includeColumns": ["^z$", "^gone$"]}}, b, "only the last")
    assert idx == [i for i in range(n) if i % 8 == 3]
    # a schema column the batch lacks; the schema in another order than the columns, with other DataTypes than the columns'
    b.schema = abi.Schema.of([["gone", "utf8", True], ["z", "utf8", False], ["c", "int64", False], ["b", "any", False], ["a", "utf8", False]])
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "schema order")
    assert idx == [i for i in range(n) if i % 4 == 1 or i % 8 == 3]
    b.schema = abi.Schema.of([["b", "string", False]])                               # ... a schema that lists one of them
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "short schema")
    assert idx == [i for i in range(n) if i % 4 == 1]
    b.schema = None                                                                  # schema NULL: the batch's own columns
    _, idx = check(tf, {"allowedIDs": IDS3, "columns": {"includeColumns": ["^[cz]$"]}}, b, "no schema")
    assert idx == [i for i in range(n) if i % 4 == 2 or i % 8 == 3]


def test_a_name_listed_twice_the_last_wins(tf):
    n = 67
    first = text_column("a", "utf8", abi.R_STRING, [b"ID1" if i % 2 == 0 else b"x" for i in range(n)])
    last = text_column("a", "utf8", abi.R_STRING, [b"ID4" if i % 3 == 0 else b"y" for i in range(n)])
    b = abi.Batch([first, fixed_column("n", "int32", abi.R_INT32, list(range(n))), last], n, "db", "t")
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "twice")
    assert idx == [i for i in range(n) if i % 3 == 0]
    last.absent = np.array([i % 5 == 0 for i in range(n)], bool)                     # a row that does not list the last one reads the one before it
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "twice, the last ABSENT in some rows")
    assert idx == [i for i in range(n) if (i % 5 == 0 and i % 2 == 0) or (i % 5 != 0 and i % 3 == 0)]
    b.cols[0] = fixed_column("a", "utf8", abi.R_INT64, list(range(n)))              # ... which is no string
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "twice, a number first")
    assert idx == [i for i in range(n) if i % 5 != 0 and i % 3 == 0]
    b.schema = abi.Schema.of([["a", "utf8", True], ["a", "utf8", False]])            # the schema lists the name twice as well
    check(tf, {"allowedIDs": IDS3}, b, "twice in the schema")


# ---- cell states ----------------------------------------------------------------------------------------------------------------------------------------
def test_nils_and_absent_cells(tf):
    n = 131
    s = text_column("s", "utf8", abi.R_STRING, [None if i % 3 == 0 else b"ID1-%d" % i for i in range(n)])
    s.absent = np.array([i % 4 == 1 for i in range(n)], bool)
    other = text_column("o", "utf8", abi.R_STRING, [b"o%d" % i for i in range(n)])
    other.absent = np.array([i % 6 == 2 for i in range(n)], bool)
    b = abi.Batch([s, other, fixed_column("n", "int64", abi.R_INT64, [None if i % 10 == 0 else i for i in range(n)])], n, "db", "t")
    got, idx = check(tf, {"allowedIDs": ["ID1"]}, b, "nil and ABSENT in the only matching column")
    assert idx == [i for i in range(n) if i % 3 != 0 and i % 4 != 1]
    assert got.col("o").absent is not None and got.col("o").absent.tolist() == [i % 6 == 2 for i in idx]      # the output carries the bitmaps
    assert got.col("n").validity is not None and got.col("n").validity.tolist() == [i % 10 != 0 for i in idx]


# ---- kinds ----------------------------------------------------------------------------------------------------------------------------------------------
def test_kinds(tf):
    n = 135
    kinds = [i % 5 for i in range(n)]                                                 # Insert, Update, Delete, K_OTHER, K_SYNCHRONIZE
    b = ids_batch(n)
    b.cols[1] = text_column("id", "utf8", abi.R_STRING, [b"ID1" if i % 2 == 0 else b"no" for i in range(n)])
    b.kind = np.array(kinds, np.uint8)
    b.part_id = np.array([i * 7 % 11 for i in range(n)], np.uint32)
    b.old_keys = [fixed_column("n", "int64", abi.R_INT64, [None if i % 9 == 0 else i * 3 for i in range(n)])]
    b.old_present = np.array([k in (1, 2) for k in kinds], bool)
    got, idx = check(tf, {"allowedIDs": IDS3}, b, "kinds")
    assert idx == [i for i in range(n) if i % 2 == 0 and i % 5 in (0, 1)]             # Updates like Inserts; the rest dropped where their cells match
    assert set(got.kind.tolist()) == {abi.K_INSERT, abi.K_UPDATE} and [c.name for c in got.old_keys] == ["n"]
    b.kind = None                                                                     # kind == NULL: every row an Insert
    b.old_keys, b.old_present = None, None
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "no kinds")
    assert idx == [i for i in range(n) if i % 2 == 0]
    b.kind = np.full(n, abi.K_DELETE, np.uint8)                                       # nothing stays
    _, idx = check(tf, {"allowedIDs": IDS3 + [""]}, b, "deletes")
    assert idx == []


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------------------
def upload_device(tf, host, prefix=5, slack=9):
    """`host` through a TFGPU_MEM_DEVICE upload whose text columns sit `prefix` bytes into their buffers (offsets[0] != 0) and state a data_len `slack`
    bytes past offsets[nrows] (tests/test_gpu_batch_plumbing.py's pattern)"""
    db = tf.DeviceBatch.upload(host)
    v = db.view()
    keep = []
    for i, c in enumerate(host.cols):
        if c.repr not in abi.VAR_REPRS:
            continue
        o = np.asarray(c.offsets, np.int64)
        off = (o - o[0] + prefix).astype(np.uint32)
        data = b"ID1" * 2 + b"X" * (prefix - 6) + bytes(np.asarray(c.data, np.uint8)[int(o[0]): int(o[-1])]) + b"ID1" * (slack // 3)
        bo, bd = tf.DeviceBuffer.upload(off.tobytes()), tf.DeviceBuffer.upload(data)
        keep += [bo, bd]
        v.cols[i].offsets, v.cols[i].data, v.cols[i].data_len = bo.ptr, bd.ptr, len(data)
    h = C.c_void_p()
    tf._check(tf.load().tfgpu_batch_upload(C.byref(v), C.byref(h)))   # (synchronises: the buffers may go)
    return tf.DeviceBatch(h)


def test_offsets_that_do_not_start_at_zero_or_end_at_data_len(tf):
    n = 129
    b = ids_batch(n)
    b.cols.append(text_column("j", "any", abi.R_JSON, [b'"ID4"' if i % 9 == 1 else b"[]" for i in range(n)]))
    want_idx = [i for i in range(n) if i % 9 in (0, 1, 2, 6)]
    _, idx = check(tf, {"allowedIDs": IDS3}, b, "device upload", device_batch=upload_device(tf, b, 6, 9))
    assert idx == want_idx
    # a host batch whose offsets start behind a prefix of the data
    shifted = abi.Batch(list(b.cols), n, "db", "t")
    c = b.col("id")
    shifted.cols[1] = abi.Column("id", "utf8", abi.R_STRING, offsets=(c.offsets + np.uint32(3)), data=np.concatenate([np.frombuffer(b"ID1", np.uint8), c.data]), validity=c.validity)
    _, idx = check(tf, {"allowedIDs": IDS3}, shifted, "host shift")
    assert idx == want_idx


def test_behind_a_filter_rows_the_input_is_a_selection(tf, oracle):
    n = 257
    b = ids_batch(n)
    flt = ("filter_rows", {"filter": "n > 100"})
    kept = oracle.apply_chain([oracle.Transformer(*flt)], b, ref.batch_schema(b)).batch
    assert 0 < kept.nrows < n
    cfg = {"allowedIDs": IDS3}
    res = tf.apply_chain([tf.Transformer(*flt), transformer(tf, cfg)], tf.DeviceBatch.upload(b))
    want, idx = ref.apply(cfg, kept)
    assert res.errors == [] and res.transformed.nrows == len(idx) > 0
    assert_same_batch(res.transformed.download(), want, "selection in")
    assert want.src_row.tolist() == [i for i in range(101, n) if i % 9 in (0, 2, 6)]   # src_row names rows of the chain's input


def test_straight_from_csv_parse(tf, oracle):
    from transferia_amd import workload
    n = 300
    schema, data, opts = workload.hits_schema(), workload.hits_csv(n), workload.hits_csv_options()
    host = tf.csv_parse(opts, schema, data)[0].download()
    urls = [host.col("url").get_bytes(i) for i in range(n)]
    ids = sorted({u[:14] for u in urls[::7] if len(u) >= 14})[:5] + [urls[1]]
    cfg = {"allowedIDs": ids, "columns": {"includeColumns": ["^url$"]}}
    db, consumed, errs = tf.csv_parse(opts, schema, data)                               # its text columns have not been scanned yet
    assert consumed == len(data) and not errs
    res = tf.apply_chain([transformer(tf, cfg)], db)
    want, idx = ref.apply(cfg, host)
    assert 0 < len(idx) < n and res.transformed.nrows == len(idx)                       # tfgpu_dbatch_nrows alone: the result is still a selection
    text = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, res.transformed).download()            # ... then a serializer reads it
    assert text == oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, want, schema)
    assert_same_batch(res.transformed.download(), want, "csv")


def chain_batch(n):
    b = ids_batch(n)
    b.cols.append(text_column("secret", "utf8", abi.R_STRING, [b"s%d" % i for i in range(n)]))
    b.schema = abi.Schema.of([["n", "int64", True], ["id", "utf8", False], ["secret", "utf8", False]])
    return b


def test_chain_with_mask_field_into_json_each_row(tf, oracle):
    n = 260
    b = chain_batch(n)
    cfg = {"allowedIDs": IDS3, "columns": {"includeColumns": ["^id$"]}}
    mask = ("mask_field", {"maskFunctionHash": {"userDefinedSalt": "salt"}, "columns": ["secret"]})
    res = tf.apply_chain([transformer(tf, cfg), tf.Transformer(*mask)], tf.DeviceBatch.upload(b))
    kept, idx = ref.apply(cfg, b)
    want = oracle.apply_chain([oracle.Transformer(*mask)], kept, b.schema)
    text = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, res.transformed).download()
    expect = oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, want.batch, want.schema)
    assert expect is not None and text == expect and text.count(b"\n") == len(idx) > 0


def test_transformation_push_and_apply_split(tf, oracle):
    n = 140
    b = chain_batch(n)
    cfg = {"allowedIDs": IDS3, "tables": {"includeTables": ["^db\\.t$"]}}
    mask = ("mask_field", {"maskFunctionHash": {"userDefinedSalt": "salt"}, "columns": ["secret"]})
    kept, idx = ref.apply(cfg, b)
    want = oracle.apply_chain([oracle.Transformer(*mask)], kept, b.schema).batch
    tn = tf.Transformation([transformer(tf, cfg), tf.Transformer(*mask)])
    assert tn.table_plan("db", "t", b.schema) == [0, 1] and tn.table_plan("db", "other", b.schema) == [1]
    out = tn.push_run(tf.DeviceBatch.upload(b), b.schema)
    assert out.errors == [] and out.error_batches == []
    got = out.transformed.download()
    assert got.nrows == len(idx) and got.src_row.tolist() == idx
    assert [got.col("secret").get_bytes(i) for i in range(got.nrows)] == [want.col("secret").get_bytes(i) for i in range(want.nrows)]
    # tfgpu_transformation_from_config knows the type by its config name
    L = tf.load()
    L.tfgpu_transformation_from_config.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.tfgpu_transformation_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    text = json.dumps({"transformers": [{"filterRowsByIds": cfg, "transformerId": "t-1"}]}).encode()
    assert L.tfgpu_transformation_from_config(text, None, 0, C.byref(h)) == 0, L.tfgpu_last_error()
    L.tfgpu_transformation_destroy(h)
    # in front of a table splitter: the rows the filter keeps are the rows that are split
    split = tf.Transformer("table_splitter_transformer", {"columns": ["id"]})
    ts = tf.apply_split([transformer(tf, cfg), split], tf.DeviceBatch.upload(b))
    alone = tf.table_split(split, tf.DeviceBatch.upload(kept))
    assert ts.nrows == len(idx) and ts.names() == alone.names() and [ts.table_rows(t) for t in range(ts.count)] == [alone.table_rows(t) for t in range(alone.count)]
    # tfgpu_apply_meta runs it as tfgpu_apply does
    res = tf.apply_meta([transformer(tf, cfg)], tf.DeviceBatch.upload(b), np.arange(n, dtype=np.uint64))
    assert res.transformed.download().src_row.tolist() == idx


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tf):
    cfg = {"allowedIDs": IDS3}
    b = ids_batch(10)
    b.cols.append(text_column("document", "any", abi.R_JSON, [b'{"nested_id":"ID1"}'] * 10))
    for schema in (None, abi.Schema.of([["id", "utf8", True], ["document", "any", False]])):
        b.schema = schema
        with pytest.raises(tf.TfgpuError) as ei:
            tf.apply_chain([transformer(tf, cfg)], tf.DeviceBatch.upload(b))
        assert ei.value.code == tf.ERR_UNSUPPORTED and T in str(ei.value) and ref.MONGO_REFUSAL in str(ei.value)
    b.schema = abi.Schema.of([["id", "utf8", True], ["document", "utf8", False]])    # `document` of another DataType is an ordinary column
    b.cols[2].dtype = "utf8"
    check(tf, cfg, b, "document as utf8")
    assert transformer(tf, cfg).suitable("db", "t", abi.Schema.of([["document", "any", False]]))   # Suitable still answers as the reference does
    # rows that carry their own ColumnNames order (a collapsed TOAST batch)
    from collapse_cases import batch_from_items
    items = [{"kind": "update", "keys": ["id"], "names": ["id", "b"], "values": [["int64", 1], ["string", "b0"]]},
             {"kind": "update", "keys": ["id"], "names": ["id", "s"], "values": [["int64", 1], ["string", "a1"]]}]
    ordered = tf.collapse(tf.DeviceBatch.upload(batch_from_items(items, names=["id", "s", "b"])[0]))
    assert ordered.download().col_order is not None
    with pytest.raises(tf.TfgpuError) as ei:
        tf.apply_chain([transformer(tf, cfg)], ordered)
    assert ei.value.code == tf.ERR_UNSUPPORTED and T in str(ei.value) and "col_order" in str(ei.value)


# ---- a seeded random sweep: 200 batches of at most 300 rows ---------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "I", "D", "1", "\x00", "é", "日", "😀", '"', "\\", "/", "\n", "\t", "\x7f"]
RAW_BYTES = [b"a", b"b", b"I", b"D", b"1", b"\x00", b"\xff", b"\xc3", b"\xa9", "é".encode(), "😀".encode()]


def random_json_string(rng, text: str) -> bytes:
    out = bytearray(b'"')
    short = {'"': b'\\"', "\\": b"\\\\", "/": b"\\/", "\n": b"\\n", "\t": b"\\t"}
    for ch in text:
        how = rng.integers(0, 3)
        cp = ord(ch)
        if ch in short and (how != 1 or ch in '"\\\n\t'):
            out += short[ch]
        elif how == 1 or cp < 0x20:
            if cp >= 0x10000:
                v = cp - 0x10000
                out += b"\\u%04x\\u%04x" % (0xD800 + (v >> 10), 0xDC00 + (v & 0x3FF))
            else:
                out += b"\\u%04X" % cp if how == 1 and cp > 0xFF else b"\\u%04x" % cp
        else:
            out += ch.encode("utf-8")
        if rng.random() < 0.04:
            out += [b"\\ud800", b"\\udc00", b"\xff", b"\xe6\x97"][rng.integers(0, 4)]       # a lone surrogate, raw bytes that are no UTF-8
    return bytes(out + b'"')


def random_case(rng):
    n = int(rng.choice([0, 1, 17, 64, 65, 130, 257, 300]))
    nid = int(rng.choice([1, 2, 3, 8, 40, 700]))
    ids = set()
    while len(ids) < nid:
        k = int(rng.choice([0, 1, 1, 2, 3, 3, 4, 5, 6, 9])) if nid < 100 else int(rng.integers(2, 7))
        ids.add(b"".join(RAW_BYTES[rng.integers(0, len(RAW_BYTES))] for _ in range(k))[:k] if rng.random() < 0.5 else
                "".join(ALPHABET[rng.integers(0, len(ALPHABET))] for _ in range(k)).encode()[:k])
        if nid >= 100 and len(ids) < nid:
            ids.add(b"id-%04d" % rng.integers(0, 5000))
    ids = sorted(ids)
    pick = lambda: ids[rng.integers(0, len(ids))]   # noqa: E731
    names = ["c0", "c1", "c2", "c3"]
    cols = []
    for _ in range(int(rng.integers(1, 6))):
        name = names[rng.integers(0, 4)]
        form = int(rng.choice([abi.R_STRING, abi.R_STRING, abi.R_BYTES, abi.R_JSON, abi.R_JSONNUM, abi.R_INT64]))
        dtype = str(rng.choice(["utf8", "utf8", "string", "any", "int64"]))
        if form == abi.R_INT64:
            c = fixed_column(name, dtype, form, [None if rng.random() < 0.1 else int(rng.integers(0, 99)) for _ in range(n)])
        else:
            cells = []
            for _ in range(n):
                u = rng.random()
                if u < 0.08:
                    cells.append(None)
                elif form == abi.R_JSON:
                    if u < 0.2:
                        cells.append([b"{}", b'["a"]', b"1", b"null", b"true"][rng.integers(0, 5)])
                    else:
                        base = pick().decode("utf-8", "replace").replace("�", "") if u < 0.6 else ""
                        cells.append(random_json_string(rng, base + "".join(ALPHABET[rng.integers(0, len(ALPHABET))] for _ in range(int(rng.integers(0, 5))))))
                elif form == abi.R_JSONNUM:
                    cells.append(b"%d" % rng.integers(0, 99))
                else:
                    tail = b"".join(RAW_BYTES[rng.integers(0, len(RAW_BYTES))] for _ in range(int(rng.integers(0, 4))))
                    base = pick() if u < 0.5 else b""
                    cells.append((base[: len(base) - 1] if u < 0.2 else base) + tail)
            c = text_column(name, dtype, form, cells)
        if rng.random() < 0.3:
            c.absent = rng.random(n) < 0.25
        cols.append(c)
    b = abi.Batch(cols, n, "db", "t")
    if rng.random() < 0.6:
        b.kind = rng.integers(0, 5, n).astype(np.uint8) if rng.random() < 0.5 else rng.integers(0, 2, n).astype(np.uint8)
    if rng.random() < 0.5:
        spec = [[nm, str(rng.choice(["utf8", "string", "any", "int64"])), False] for nm in rng.permutation(names + ["gone"])][: int(rng.integers(1, 6))]
        b.schema = abi.Schema.of(spec)
    cfg = {"allowedIDs": ids}
    u = rng.random()
    if u < 0.3:
        cfg["columns"] = {"includeColumns": ["^c[%s]$" % "".join(str(d) for d in rng.permutation(4)[:2])]}
    elif u < 0.5:
        cfg["columns"] = {"excludeColumns": ["^c%d$" % rng.integers(0, 4)]}
    return cfg, b


@pytest.mark.parametrize("part", range(4))
def test_random_sweep(tf, part):
    rng = np.random.default_rng(20260 + part)
    kept = total = 0
    for k in range(50):
        cfg, b = random_case(rng)
        _, idx = check(tf, cfg, b, ("part %d batch %d" % (part, k), cfg.get("columns")))
        kept += len(idx)
        total += b.nrows
    assert 0 < kept < total
