"""raw_doc_grouper on the device (tf_rawdoc.hip, through tfgpu_apply_meta) against the plain-Python restatement (tests/rawdoc_ref.py), exactly: every
output column cell for cell — values, nils, ABSENT bits, kinds, OldKeys with presence, part_id, src_row, namespace, table, TableSchema with its keys —
and `doc` byte for byte.

The sizes at which the code takes another path: a wave and a workgroup of rows (63 / 64 / 65 / 256 / 257), the sink's 8-byte word (text cells of
0 / 7 / 8 / 9 bytes), batches with and without a `_rest` column (two kernels), rows that splice `_rest` next to rows that do not."""
import numpy as np
import pytest

import rawdoc_ref as ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
T = "raw_doc_grouper"
EPOCH = 1677510100000000000   # the reference tests' updateTime


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
    """tests/test_gpu_table_split.py's comparison; a batch without src_row reads the identity"""
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
            if a.repr in abi.VAR_REPRS:
                for i in range(got.nrows):
                    if (va & ~ab)[i]:
                        assert a.get_bytes(i) == b.get_bytes(i), (ctx, what, a.name, i)
            else:
                ok = va & ~ab
                assert np.array_equal(a.values[ok].view(np.uint8), b.values[ok].view(np.uint8)), (ctx, what, a.name, "values")
                if a.repr == abi.R_TIME:
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
    wp = want.part_id if want.part_id is not None else np.zeros(want.nrows, np.uint32)
    gp = got.part_id if got.part_id is not None else np.zeros(got.nrows, np.uint32)
    assert np.array_equal(gp, wp), (ctx, "part_id")
    ident = np.arange(want.nrows, dtype=np.int32)
    assert np.array_equal(got.src_row if got.src_row is not None else ident, want.src_row if want.src_row is not None else ident), (ctx, "src_row")


def docs_of(b):
    return [b.col("doc").get_bytes(i) for i in range(b.nrows)]


def check(tf, oracle, config, batch, commit_time=None, ctx="", device_batch=None, seen=None):
    """the device's Apply of `config` over `batch` against the restatement's.  `seen`: the host batch the grouper read, where `device_batch` is not
    simply the upload of `batch`"""
    db = device_batch if device_batch is not None else tf.DeviceBatch.upload(batch)
    res = tf.apply_meta([tf.Transformer(T, config)], db, commit_time)
    want, werrs = ref.apply(oracle, config, seen if seen is not None else batch, commit_time)
    assert werrs == [] and res.errors == [], ctx
    got = res.transformed.download()
    assert_same_batch(got, want, ctx)
    assert docs_of(got) == docs_of(want), ctx
    assert res.transformed.table_schema().triples() == want.schema.triples(), ctx
    return got


# ---- rows and reprs -------------------------------------------------------------------------------------------------------------------------------
I64_MIN, U64_MAX = -(1 << 63), (1 << 64) - 1
TEXTS = [b"", b"seven77", b"eight888", b"nine99999", b'quote " and \\ backslash', b"ctl \x00\x01\x1f\n\r\t\b\f end", b"bad \xff\xfe\xc3 utf8 \xed\xa0\x80",
         "sep \u2028\u2029 нажатие 😀".encode(), b"<html> & 'apos' stay", b"x" * 300]


def every_repr_batch(n):
    """the eight integers, both floats, bool, string, bytes, json.Number, `any`, time with nanos, duration: nils in each column (row i is nil in column
    i % 19 when i % 3 == 0), names whose byte order differs from the batch's and one that needs escaping"""
    def nil(c, i, v):
        return None if (i % 3 == 0 and i % 19 == c) else v
    r = range(n)
    t0 = 1693490347
    cols = [fixed_column("zeta", "int8", abi.R_INT8, [nil(0, i, (i * 37) % 256 - 128) for i in r]),
            fixed_column("i16", "int16", abi.R_INT16, [nil(1, i, (i * 9973) % 65536 - 32768) for i in r]),
            fixed_column("Alpha", "int32", abi.R_INT32, [nil(2, i, [-(1 << 31), (1 << 31) - 1, 0, -1, 99999999, 100000000, -100000000][i % 7]) for i in r]),
            fixed_column("i64", "int64", abi.R_INT64, [nil(3, i, [I64_MIN, (1 << 63) - 1, 0, -1, 10**16, -(10**8), 99999999 + i][i % 7]) for i in r]),
            fixed_column("u8", "uint8", abi.R_UINT8, [nil(4, i, i % 256) for i in r]),
            fixed_column("u16", "uint16", abi.R_UINT16, [nil(5, i, (i * 257) % 65536) for i in r]),
            fixed_column("u32", "uint32", abi.R_UINT32, [nil(6, i, [0, (1 << 32) - 1, 100000000, 99999999][i % 4]) for i in r]),
            fixed_column("u64", "uint64", abi.R_UINT64, [nil(7, i, [0, U64_MAX, 1 << 63, 10**19, 10**16 - 1, i][i % 6]) for i in r]),
            fixed_column("f32", "float", abi.R_FLOAT32, [nil(8, i, [2.71828, 1e21, 1e-7, 0.0, -0.0, 16777216.0, 1e20, i * 0.25][i % 8]) for i in r]),
            fixed_column("f64", "double", abi.R_FLOAT64, [nil(9, i, [3.14, 1e21, 1e-7, 1e20, -0.0, 123456789.125, 5e-324, i / 3.0][i % 8]) for i in r]),
            fixed_column("b", "boolean", abi.R_BOOL, [nil(10, i, i % 2 == 0) for i in r]),
            text_column('na"me\n', "utf8", abi.R_STRING, [nil(11, i, TEXTS[i % len(TEXTS)]) for i in r]),
            text_column("by", "string", abi.R_BYTES, [nil(12, i, TEXTS[(i + 1) % len(TEXTS)][: i % 11]) for i in r]),
            text_column("num", "double", abi.R_JSONNUM, [nil(13, i, [b"1.50", b"-0", b"1e400", b"12345678901234567890", b""][i % 5]) for i in r]),
            text_column("js", "any", abi.R_JSON, [nil(14, i, [b'{"a":1}', b"[]", b"null", b'"s<>"', b"1", b'{"k":[1,{"z":null}]}'][i % 6]) for i in r]),
            fixed_column("ts", "timestamp", abi.R_TIME, [nil(15, i, [t0, 0, -1, 253402300799, t0 + i][i % 5]) for i in r], [[0, 123456789, 999999999, 1000, 500000000][i % 5] for i in r]),
            fixed_column("dt", "datetime", abi.R_TIME, [nil(16, i, t0 + 86400 * i) for i in r]),
            fixed_column("iv", "interval", abi.R_DURATION, [nil(17, i, [0, 1, 1500000000, -90000000000, I64_MIN][i % 5]) for i in r]),
            text_column("étoile", "utf8", abi.R_STRING, [nil(18, i, b"r%d" % i) for i in r])]
    b = abi.Batch(cols, n, "db", "typed")
    b.schema = abi.Schema([abi.ColSchema(c.name, c.dtype, c.name == "i64") for c in cols])
    return b


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_row_counts_and_every_repr(tf, oracle, n):
    b = every_repr_batch(n)
    ct = np.array([EPOCH + i * 1000000007 for i in range(n)], np.uint64)
    got = check(tf, oracle, {"keys": ["u32", "Alpha"], "fields": ["js", 'na"me\n']}, b, ct, "n=%d" % n)   # keys that are not the source's, a `fields` list
    assert [c.name for c in got.cols] == ["Alpha", "u32", 'na"me\n', "js", "etl_updated_at", "doc"]          # the kept columns in INPUT order
    if n > 1:
        d = docs_of(got)[1]
        assert d.startswith(b'{"Alpha":2147483647,"b":false,"by":"')                                          # byte order: upper case first
        assert b'"na\\"me\\n":"seven77"' in d and d.endswith(b',"zeta":-91,"\xc3\xa9toile":"r1"}')
    if n > 9:
        assert b'"<html> & \'apos\' stay"' in docs_of(got)[8] and b"\\u2028\\u2029" in docs_of(got)[7] and b"\\ufffd\\ufffd\\ufffd utf8 \\ufffd\\ufffd\\ufffd" in docs_of(got)[6]
        assert b"ctl \\u0000\\u0001\\u001f\\n\\r\\t\\b\\f end" in docs_of(got)[5]


def test_text_cell_lengths_around_the_sink_word(tf, oracle):
    cells = [b"", b"1234567", b"12345678", b"123456789", None, b"\n234567", b'"2345678', b"12345678\\"]
    for name in ("s", "a_longer_name_"):   # (the literal in front moves the cell against the word)
        b = abi.Batch([text_column(name, "utf8", abi.R_STRING, cells), fixed_column("k", "int32", abi.R_INT32, list(range(len(cells))))], len(cells), "db", "t")
        got = check(tf, oracle, {"keys": ["k"]}, b, None, name)

        def doc(i, text, name=name):   # two members, in byte order of their names
            m = sorted([(b"k", b"%d" % i), (name.encode(), text)])
            return b"{" + b",".join(b'"' + k + b'":' + v for k, v in m) + b"}"
        texts = [b'""', b'"1234567"', b'"12345678"', b'"123456789"', b"null", b'"\\n234567"', b'"\\"2345678"', b'"12345678\\\\"']
        assert docs_of(got) == [doc(i, t) for i, t in enumerate(texts)]


# ---- keys and fields ------------------------------------------------------------------------------------------------------------------------------
def test_key_and_field_choices(tf, oracle):
    b = every_repr_batch(20)
    ct = [EPOCH] * 20
    got = check(tf, oracle, {"keys": ["etl_updated_at", "i64"]}, b, ct)                       # etl_updated_at as a key: first in the schema, still behind the kept columns
    assert [c.name for c in got.cols] == ["i64", "etl_updated_at", "doc"]
    got = check(tf, oracle, {"keys": [], "fields": ["doc"]}, b, ct)                           # nothing kept
    assert [c.name for c in got.cols] == ["etl_updated_at", "doc"]
    got = check(tf, oracle, {"keys": ["étoile"], "fields": ["doc", "etl_updated_at", "zeta"]}, b, ct)
    assert [c.name for c in got.cols] == ["zeta", "étoile", "etl_updated_at", "doc"]
    b.schema = None                                                                             # no TableSchema: the batch's own columns stand in for it
    check(tf, oracle, {"keys": ["u8"], "fields": ["b"]}, b, ct)


# ---- ABSENT ---------------------------------------------------------------------------------------------------------------------------------------
def test_absent_cells(tf, oracle):
    n = 70
    b = every_repr_batch(n)
    b.col("f64").absent = np.array([i % 4 == 1 for i in range(n)], bool)
    b.col("js").absent = np.array([i % 5 == 2 for i in range(n)], bool)
    b.col("u32").absent = np.array([i % 6 == 3 for i in range(n)], bool)         # a key column
    for c in b.cols:                                                             # rows 10 and 64 list nothing
        ab = c.absent if c.absent is not None else np.zeros(n, bool)
        ab[[10, 64]] = True
        c.absent = ab
    got = check(tf, oracle, {"keys": ["u32"], "fields": ["js"]}, b, None)
    d = docs_of(got)
    assert d[10] == b"{}" and d[64] == b"{}" and b'"f64"' not in d[1] and b'"f64"' in d[2] and b'"u32"' not in d[3]
    assert got.col("u32").absent is not None and got.col("u32").absent[3] and got.col("js").absent[2]


# ---- _rest ----------------------------------------------------------------------------------------------------------------------------------------
def rest_batch(rests, rest_repr=abi.R_JSON, rest_dtype="any"):
    """columns b, m (before `_rest`), `_rest`, a, n (behind it)"""
    n = len(rests)
    cols = [text_column("b", "utf8", abi.R_STRING, [b"col-b%d" % i for i in range(n)]), fixed_column("m", "int32", abi.R_INT32, list(range(n))),
            text_column("_rest", rest_dtype, rest_repr, rests),
            fixed_column("a", "int64", abi.R_INT64, [100 + i for i in range(n)]), text_column("n", "utf8", abi.R_STRING, [b"col-n%d" % i for i in range(n)])]
    return abi.Batch(cols, n, "db", "t")


RESTS = [b"{}", b'{"k":1}', b'{"0first":null}', b'{"c":[1,2,{"x":"}"}]}', b'{"zz":"last"}', b'{"0":0,"aa":{"n":{"n":[]}},"c":"\\u00e9","zz":true}',
         b'{"b":"rest wins"}', b'{"a":"column wins"}', b'{"a":1,"b":2,"m":3,"n":4}', b'{"_rest":"inner"}', b'{"\xc3\xa9":1}',
         None, b"[1,2]", b'"text"', b"17", b"null", b'{"ab":1,"b":2,"ba":3}', b'{"innerKey1":"1","innerKey2":2,"innerKey3":true}']


@pytest.mark.parametrize("n", [len(RESTS), 130])
def test_rest_is_spliced(tf, oracle, n):
    rests = [RESTS[i % len(RESTS)] for i in range(n)]
    b = rest_batch(rests)
    got = check(tf, oracle, {"keys": ["a"], "fields": ["_rest"]}, b, None)
    d = docs_of(got)
    assert d[0] == b'{"a":100,"b":"col-b0","m":0,"n":"col-n0"}' and d[1] == b'{"a":101,"b":"col-b1","k":1,"m":1,"n":"col-n1"}'
    assert d[2].startswith(b'{"0first":null,"a":102') and d[4].endswith(b'"n":"col-n4","zz":"last"}')
    assert d[6] == b'{"a":106,"b":"rest wins","m":6,"n":"col-n6"}' and d[7] == b'{"a":107,"b":"col-b7","m":7,"n":"col-n7"}'
    assert d[8] == b'{"a":108,"b":2,"m":3,"n":"col-n8"}' and d[9] == b'{"_rest":"inner","a":109,"b":"col-b9","m":9,"n":"col-n9"}'
    assert d[11].startswith(b'{"_rest":null,') and d[12].startswith(b'{"_rest":[1,2],') and d[13].startswith(b'{"_rest":"text",')
    # the column behind `_rest` ABSENT in the row: nothing overwrites the rest member
    b.col("a").absent = np.array([i % len(RESTS) in (7, 8) for i in range(n)], bool)
    b.col("_rest").absent = np.array([i % len(RESTS) == 1 for i in range(n)], bool)
    got = check(tf, oracle, {"keys": ["a"], "fields": ["_rest"]}, b, None)
    assert docs_of(got)[7] == b'{"a":"column wins","b":"col-b7","m":7,"n":"col-n7"}' and docs_of(got)[1] == b'{"a":101,"b":"col-b1","m":1,"n":"col-n1"}'


def test_rest_held_otherwise_is_a_member(tf, oracle):
    # a Go string, and bytes: `_rest` like any column (the batch runs the kernel without the merge)
    b = rest_batch([b'{"k":1}', None, b"plain"], abi.R_STRING, "utf8")
    got = check(tf, oracle, {"keys": ["a"]}, b, None)
    assert docs_of(got)[0] == b'{"_rest":"{\\"k\\":1}","a":100,"b":"col-b0","m":0,"n":"col-n0"}'
    check(tf, oracle, {"keys": ["a"]}, rest_batch([b'{"k":1}', None], abi.R_BYTES, "string"), None)


# ---- CommitTime -----------------------------------------------------------------------------------------------------------------------------------
TIMES = [0, 1, 999999999, 10**9, EPOCH, 1 << 63, (1 << 64) - 1, (1 << 63) - 1]


def test_commit_times(tf, oracle):
    n = len(TIMES)
    b = every_repr_batch(n)
    ct = np.array(TIMES, np.uint64)
    got = check(tf, oracle, {"keys": ["i64"]}, b, ct)
    e = got.col("etl_updated_at")
    assert (e.dtype, e.repr) == ("timestamp", abi.R_TIME)
    assert list(zip(e.values.tolist(), e.nanos.tolist()))[:6] == [(0, 0), (0, 1), (0, 999999999), (1, 0), (1677510100, 0), (-9223372037, 145224192)]
    # meta NULL, and a meta without commit times: the Go zero value in every row
    got = check(tf, oracle, {"keys": ["i64"]}, b, None)
    assert got.col("etl_updated_at").values.tolist() == [0] * n
    res = tf.apply_meta([tf.Transformer(T, {"keys": ["i64"]})], tf.DeviceBatch.upload(b), abi.row_meta(n, ids=np.arange(n)))
    assert res.transformed.download().col("etl_updated_at").values.tolist() == [0] * n
    # meta on the device
    dev = tf.DeviceBuffer.upload(ct.tobytes())
    res = tf.apply_meta([tf.Transformer(T, {"keys": ["i64"]})], tf.DeviceBatch.upload(b), dev)
    want, _ = ref.apply(oracle, {"keys": ["i64"]}, b, ct)
    assert_same_batch(res.transformed.download(), want, "device meta")
    # too few entries
    for short in (ct[:n - 1], tf.DeviceBuffer.upload(ct[:n - 1].tobytes())):
        with pytest.raises(tf.TfgpuError) as ei:
            tf.apply_meta([tf.Transformer(T, {"keys": ["i64"]})], tf.DeviceBatch.upload(b), short)
        assert ei.value.code == tf.ERR_INVALID and "meta->n" in str(ei.value)


def test_behind_filter_rows_the_times_follow_their_rows(tf, oracle):
    n = 257
    b = every_repr_batch(n)
    ct = np.array([EPOCH + 1000000007 * i for i in range(n)], np.uint64)
    flt = ("filter_rows", {"filter": "u16 > 20000"})
    kept = oracle.apply_chain([oracle.Transformer(*flt)], b, b.schema).batch
    kept.schema = b.schema
    assert 0 < kept.nrows < n and kept.src_row is not None and not np.array_equal(kept.src_row, np.arange(kept.nrows))
    cfg = {"keys": ["i64"], "fields": ["u16"]}
    res = tf.apply_meta([tf.Transformer(*flt), tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b), ct)   # the grouper reads a batch that is still a selection
    want, _ = ref.apply(oracle, cfg, kept, ct)
    got = res.transformed.download()
    assert_same_batch(got, want)
    assert docs_of(got) == docs_of(want) and res.errors == []
    assert got.col("etl_updated_at").values[0] == (EPOCH + 1000000007 * int(kept.src_row[0])) // 10**9
    # meta->n covers the batch's rows and not the input's
    with pytest.raises(tf.TfgpuError) as ei:
        tf.apply_meta([tf.Transformer(*flt), tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b), ct[:kept.nrows])
    assert ei.value.code == tf.ERR_INVALID and "src_row" in str(ei.value)
    # every other chain runs through this entry as through tfgpu_apply
    a = tf.apply_meta([tf.Transformer(*flt)], tf.DeviceBatch.upload(b), ct).transformed.download()
    assert_same_batch(a, tf.apply_chain([tf.Transformer(*flt)], tf.DeviceBatch.upload(b)).transformed.download())


# ---- kinds and OldKeys ----------------------------------------------------------------------------------------------------------------------------
def cdc_batch(n, kinds, old_names, present):
    b = every_repr_batch(n)
    b.kind = np.array(kinds, np.uint8)
    b.part_id = np.array([i * 7 % 11 for i in range(n)], np.uint32)
    b.old_keys = [fixed_column(nm, "int64", abi.R_INT64, [None if i % 5 == 0 else i * 3 for i in range(n)]) for nm in old_names]
    b.old_present = np.array(present, bool)
    return b


def test_kinds_oldkeys_part_id_are_carried(tf, oracle):
    n = 130
    kinds = [i % 3 for i in range(n)]                                           # inserts, updates, deletes
    b = cdc_batch(n, kinds, ["i64"], [k != 0 for k in kinds])
    got = check(tf, oracle, {"keys": ["i64"]}, b, None)                         # every OldKeys name is a result column
    assert [c.name for c in got.old_keys] == ["i64"] and got.kind.tolist() == kinds


def test_oldkeys_the_result_does_not_list(tf, oracle):
    n = 66
    cfg = {"keys": ["u32"]}
    upd = [1 if i % 2 else 0 for i in range(n)]                                 # OldKeys on the Updates only: the unlisted column goes (inPlaceRemoveOldKeys)
    got = check(tf, oracle, cfg, cdc_batch(n, upd, ["i64", "u32"], [k == 1 for k in upd]), None, "updates")
    assert [c.name for c in got.old_keys] == ["u32"]
    got = check(tf, oracle, cfg, cdc_batch(n, upd, ["i64"], [k == 1 for k in upd]), None, "updates, nothing left")
    assert not getattr(got, "old_keys", None)
    dele = [2 if i % 2 else 0 for i in range(n)]                                # ... on Deletes only: kept as it is
    got = check(tf, oracle, cfg, cdc_batch(n, dele, ["i64", "u32"], [k == 2 for k in dele]), None, "deletes")
    assert [c.name for c in got.old_keys] == ["i64", "u32"]
    mixed = [i % 3 for i in range(n)]                                           # ... on both: per-row KeyNames
    b = cdc_batch(n, mixed, ["i64", "u32"], [k != 0 for k in mixed])
    with pytest.raises(NotImplementedError):
        ref.apply(oracle, cfg, b, None)
    assert "ragged OldKeys" in _refused(tf, cfg, b)
    # the same mix where only the Updates carry OldKeys is no mix
    got = check(tf, oracle, cfg, cdc_batch(n, mixed, ["i64", "u32"], [k == 1 for k in mixed]), None, "present on updates")
    assert [c.name for c in got.old_keys] == ["u32"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def _refused(tf, config, batch, commit_time=None):
    with pytest.raises(tf.TfgpuError) as ei:
        tf.apply_meta([tf.Transformer(T, config)], batch if isinstance(batch, tf.DeviceBatch) else tf.DeviceBatch.upload(batch), commit_time)
    assert ei.value.code == tf.ERR_UNSUPPORTED and T in str(ei.value), str(ei.value)
    return str(ei.value)


def test_refusals(tf):
    cfg = {"keys": ["i64"]}
    for bad, col in ((float("nan"), "f64"), (float("inf"), "f32"), (float("-inf"), "f64")):
        b = every_repr_batch(70)
        b.col(col).values[67] = bad
        b.col(col).values[69] = bad
        msg = _refused(tf, cfg, b)
        assert "NaN" in msg and "column " + col in msg and "row 67" in msg
        b.col(col).absent = np.array([i in (67, 69) for i in range(70)], bool)       # a cell the row does not list is not looked at
        tf.apply_meta([tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b))
    for kind in (abi.K_OTHER, abi.K_SYNCHRONIZE):
        b = every_repr_batch(65)
        b.kind = np.zeros(65, np.uint8)
        b.kind[64] = kind
        assert "non-row kinds" in _refused(tf, cfg, b)
    for name in ("doc", "etl_updated_at"):
        b = every_repr_batch(3)
        b.cols.append(text_column(name, "utf8", abi.R_STRING, [b"x"] * 3))
        b.schema = None
        assert "a column named " + name in _refused(tf, cfg, b)
    # a spliced `_rest` member key with a backslash escape
    b = rest_batch([b'{"k":1}', b'{"a\\u0062":1}', b"{}"])
    assert "backslash" in _refused(tf, {"keys": ["a"]}, b)
    b = rest_batch([b'{"k":1}', b'{"k":1', b"{}"])                                   # ... and a text that is no object
    assert "`_rest`" in _refused(tf, {"keys": ["a"]}, b)
    # the entries that do not see CommitTime
    db = tf.DeviceBatch.upload(every_repr_batch(3))
    with pytest.raises(tf.TfgpuError) as ei:
        tf.Transformer(T, cfg).apply(db)
    assert ei.value.code == tf.ERR_UNSUPPORTED and "tfgpu_apply_meta" in str(ei.value)
    # rows that carry their own ColumnNames order (a collapsed TOAST batch)
    from collapse_cases import batch_from_items
    items = [{"kind": "update", "keys": ["id"], "names": ["id", "b"], "values": [["int64", 1], ["string", "b0"]]},
             {"kind": "update", "keys": ["id"], "names": ["id", "s"], "values": [["int64", 1], ["string", "a1"]]}]
    ordered = tf.collapse(tf.DeviceBatch.upload(batch_from_items(items, names=["id", "s", "b"])[0]))
    assert ordered.download().col_order is not None
    assert "col_order" in _refused(tf, {"keys": ["id"]}, ordered)


def test_unsuitable_schema_is_a_row_error_per_row(tf, oracle):
    n = 65
    b = every_repr_batch(n)
    for cfg in ({"keys": ["i64", "nosuch"]}, {"keys": ["i64"], "fields": ["gone"]}):
        res = tf.apply_meta([tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b), [EPOCH] * n)
        want, werrs = ref.apply(oracle, cfg, b, [EPOCH] * n)
        assert res.transformed.download().nrows == 0 == want.nrows
        assert [e[0] for e in res.errors] == werrs == list(range(n)) and {e[1] for e in res.errors} == {"COLUMN_NOT_FOUND"} and {e[2] for e in res.errors} == {0}
    # the TableSchema decides, not the batch's columns: a schema column the batch lacks is enough
    b.schema = abi.Schema(b.schema.cols + [abi.ColSchema("gone", "utf8")])
    got = check(tf, oracle, {"keys": ["i64"], "fields": ["gone"]}, b, None)
    assert [c.name for c in got.cols] == ["i64", "etl_updated_at", "doc"]
    assert got.nrows == n


# ---- downstream -----------------------------------------------------------------------------------------------------------------------------------
def test_output_feeds_clickhouse_json_each_row(tf, oracle):
    n = 66
    b = rest_batch([RESTS[i % len(RESTS)] for i in range(n)])
    b.schema = abi.Schema.of([["b", "utf8", False], ["m", "int32", True], ["_rest", "any", False], ["a", "int64", False], ["n", "utf8", False]])
    cfg = {"keys": ["a"], "fields": ["n"]}
    ct = np.array([EPOCH + i for i in range(n)], np.uint64)
    res = tf.apply_meta([tf.Transformer(T, cfg)], tf.DeviceBatch.upload(b), ct)
    want, _ = ref.apply(oracle, cfg, b, ct)
    text = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, res.transformed).download()
    expect = oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, want, want.schema)
    assert expect is not None and text == expect and text.count(b"\n") == n
    # (JSONEachRow carries an `any` value as a string and a timestamp as nanoseconds)
    assert text.split(b"\n")[0] == b'{"a":100,"n":"col-n0","etl_updated_at":1677510100000000000,"doc":"{\\"a\\":100,\\"b\\":\\"col-b0\\",\\"m\\":0,\\"n\\":\\"col-n0\\"}"}'
