"""raw_to_table on the device (tf_rawtable.hip, through tfgpu_raw_to_table_parse) against the plain-Python restatement (tests/rawtable_ref.py), exactly:
both tables cell for cell — values, nils, the `any` and headers texts byte for byte — with their names, schemas, keys, src_row and kinds, and the
messages left to the stock parser.

The sizes are the smallest at which the kernels can go wrong: the validator's 8-byte word (lengths 0 / 1 / 7 / 8 / 9), its chunk and its short / long
switch (both read from the library), a wave and a workgroup of messages (63 .. 257), the emitters' depth limits on both sides."""
import numpy as np
import pytest

import rawtable_ref as ref
from transferia_amd import abi
from util import golden

pytestmark = pytest.mark.gpu
G = golden("raw_to_table.json")
TS = 1700000000123456789


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def cells_of(b: abi.Batch, r: int):
    out = []
    for c in b.cols:
        k, v = c.pyvalue(r)
        out.append(None if k == "nil" else ("utf8", v) if k == "string" else ("any", v) if k == "json" else ("u32", v) if k == "uint32" else (k, v))
    return out


def compare_table(dev, want, c, dlq, topic, ctx):
    b = dev.download()
    cols = ref.schema(c, dlq)
    assert [[x.name, x.dtype] for x in b.cols] == [x[:2] for x in cols], ctx   # typed columns, also with zero rows
    assert dev.table_schema().triples() == [x[:3] for x in cols], ctx
    assert (b.table_ns, b.table_name) == ("", ref.table_name(c, dlq, topic)), ctx
    assert b.nrows == len(want), (ctx, "rows", b.nrows, len(want))
    assert list(b.src_row) == [i for i, _ in want], (ctx, "src_row")
    assert b.kind is None or not b.kind.any(), ctx   # every row an Insert
    for r, (i, cells) in enumerate(want):
        assert cells_of(b, r) == cells, (ctx, "dlq" if dlq else "main", "message", i)
    return b


def check(tf, cfg, msgs, topic="tp", partition=7, ctx=""):
    """the device's DoBatch against the restatement's; returns (main, dead-letter, fallback list) as the restatement has them"""
    c = ref.config(cfg)
    p = tf.RawToTable.from_config(cfg)
    dm, dd, fb = p.parse(abi.message_batch(topic, partition, msgs))
    wm, wd, wfb = ref.do_batch(c, topic, partition, msgs)
    assert fb == wfb, (ctx, "fallback")
    compare_table(dm, wm, c, False, topic, ctx)
    compare_table(dd, wd, c, True, topic, ctx)
    return wm, wd, wfb


def msg(i, value, key=None, headers=None, wt=TS):
    return (1000 + i, wt + i, key, value, headers)


# ---- 1. the reference's own cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["do"], ids=lambda c: c["name"])
def test_golden_through_the_device(tf, case):
    m = ref.golden_message(case["message"])
    wm, wd, _ = check(tf, case["config"], [m], case["topic"], case["partition"], case["name"])
    rows = wd if case["dlq"] else wm
    assert len(rows) == 1 and rows[0][1] == [ref.golden_cell(v) for v in case["values"]]


# ---- 2. utf8.Valid ------------------------------------------------------------------------------------------------------------------------------------------
BAD_UTF8 = [b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf",
            b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\xfe", b"\x80", b"\xbf", b"\xc2", b"\xe0\xa0", b"\xf0\x90\x80", b"\xf0\x90", b"\xc2\x41", b"\xe1\x80\x41"]
GOOD_UTF8 = [b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xef\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf"]
FILL_BAD = b"\x80\x80\x80 starts with continuation bytes and ends in a lead \xf0\x90"   # what a neighbour must not lend or borrow
FILL_GOOD = "plain text, zwölf Boxkämpfer 😀".encode()


def utf8_items():
    items = []
    for L in (0, 1, 7, 8, 9):
        items.append(b"a" * L)
    for s in BAD_UTF8 + GOOD_UTF8:
        for pre in (0, 1, 7, 8, 9):   # the sequence at the start, behind one byte, across and behind the first word
            items += [b"a" * pre + s, b"a" * pre + s + b"z"]
    return items


def both_types(who, v):
    """`v` as the value or as the key of a message, the other one plain"""
    return {"value": v, "key": b"k"} if who == "value" else {"value": b"v", "key": v}


def utf8_cfg(who):
    return {"TableName": "t", "ValueType": "string" if who == "value" else "bytes", "IsKeyEnabled": True, "KeyType": "string" if who == "key" else "bytes"}


@pytest.mark.parametrize("who", ["value", "key"])
def test_utf8_edges_first_middle_last(tf, who):
    """every edge as the first, a middle and the last of 200 messages whose neighbours start with continuation bytes and end in a lead byte"""
    n = 200
    for item in utf8_items():
        vals = [FILL_BAD if (i % 2 == 1 or i == n - 2) else FILL_GOOD for i in range(n)]
        for at in (0, n // 2, n - 1):
            vals[at] = item
        msgs = [msg(i, **both_types(who, v)) for i, v in enumerate(vals)]
        wm, wd, _ = check(tf, utf8_cfg(who), msgs, ctx=(who, item))
        assert ({0, n // 2, n - 1} <= {i for i, _ in wm}) == ref.utf8_valid(item), item


@pytest.mark.parametrize("who", ["value", "key"])
def test_utf8_lead_at_the_end_is_not_completed_by_the_next_message(tf, who):
    pairs = [(b"ab\xc2", b"\x80cd"), (b"\xe0\xa0", b"\x80"), (b"\xf0", b"\x90\x80\x80"), (b"\xf0\x90\x80", b"\x80"), (b"x" * 7 + b"\xc3", b"\xa9" + b"y" * 7)]
    vals = [x for p in pairs for x in p]
    wm, wd, _ = check(tf, utf8_cfg(who), [msg(i, **both_types(who, v)) for i, v in enumerate(vals)])
    assert wm == [] and len(wd) == len(vals)


@pytest.mark.parametrize("who", ["value", "key"])
def test_utf8_chunk_and_long_switch(tf, who):
    """a multi-byte sequence across every offset around the wave validator's chunk size and around the short / long switch, in messages long enough for
    the wave path and in messages of exactly those lengths; valid, with a bad last continuation byte, and cut short by the message's end"""
    chunk, long_ = tf.rawtt_geometry()
    seqs = ["😀".encode(), "€".encode(), "é".encode(), b"\xf0\x9f\x98\x41", b"\xf0\x80\x80\x80", b"\xed\xa0\x80"]
    vals = []
    for L in (chunk - 1, chunk, chunk + 1, long_ - 1, long_, long_ + 1):
        for s in seqs:
            for pos in range(L - 4, L + 2):
                if pos < 0:
                    continue
                vals.append(b"a" * pos + s + b"b" * (long_ + 3 * chunk + 5 - pos))   # the wave path, the sequence around offset L
                vals.append(FILL_BAD)
            if L > len(s):
                vals += [b"a" * (L - len(s)) + s, FILL_BAD, b"a" * (L - len(s) + 1) + s[:-1], FILL_BAD]   # exactly L bytes: whole, and cut short by the end
    # continuation bytes at a chunk's start that belong to no sequence, and a chunk of nothing but continuation bytes
    vals += [b"a" * (2 * chunk) + b"\x80" + b"a" * long_, b"a" * (2 * chunk - 1) + b"\xc3\xa9\x80" + b"a" * long_, b"a" * long_ + b"\x80" * chunk + b"a" * chunk,
             "é".encode() * long_, "😀".encode() * long_, b"a" + "😀".encode() * long_ + b"\xf0"]
    msgs = [msg(i, **both_types(who, v)) for i, v in enumerate(vals)]
    wm, wd, _ = check(tf, utf8_cfg(who), msgs)
    assert len(wm) > 50 and len(wd) > 50


# ---- 3. json.Valid, the decode and json.Marshal ---------------------------------------------------------------------------------------------------------------
def nested_unsorted(depth):
    """`depth` objects inside one another, each with its keys in descending order"""
    s = b"1"
    for _ in range(depth):
        s = b'{"b":2,"a":' + s + b"}"
    return s


def json_values():
    cd, md = ref.CANON_DEPTH, ref.MAX_DEPTH
    good = [b" {} ", b"\t[1, 2 ,3]\r\n", b"1", b"-0.5e-3", b"1E5", b"true", b"false", b"null", b'"top level string <&> \\u00e9"', b'"\xff stray"', b'"\\ud800"',
            b'"\\ud83d\\ude00 pair"', b'{"a":1,"a":2,"b":{"x":1,"x":[1,{"k":1,"k":2}]}}', b'{"b":1,"a":2}', b'{"a":{"z":1,"y":2},"c":[{"q":1,"p":2}]}',
            b'{"k\\u0061":1,"ka":2}', b'{"a\xff":1,"a":2}', b'{"":""}', b'{"a":"\\u2028\\u2029\\b\\f\\n\\r\\t\\"\\\\\\/"}', b"[" * md + b"]" * md,
            b"[" * (cd - 1) + nested_unsorted(1) + b"]" * (cd - 1), nested_unsorted(cd), b'{"seven77":"1234567","eight888":"12345678","nine99999":"123456789"}']
    bad = [b"", b" ", b"{} x", b"[1] 2", b"01", b"1.", b"-", b'"\\x"', b'"a\x01b"', b'"raw\nnewline"', b"[1,2", b'{"a":1', b'{"a":[1,{"b":2}', b'"open', b"nul",
           b"NaN", b"{'a':1}", b'{"a":1,}', b"[,1]", b'"\\u12g4"']
    fallback = [nested_unsorted(cd + 1), b"[" * (cd) + nested_unsorted(1) + b"]" * cd, b"[" * (md + 1) + b"]" * (md + 1), b"[" * (md + 1)]
    return good, bad, fallback


@pytest.mark.parametrize("who", ["value", "key"])
def test_json_edges(tf, who):
    good, bad, fallback = json_values()
    vals = [x for t in zip(good, bad + bad) for x in t] + fallback + [None]
    cfg = {"TableName": "j", "ValueType": "json" if who == "value" else "bytes", "IsKeyEnabled": True, "KeyType": "json" if who == "key" else "bytes"}
    msgs = [msg(i, **both_types(who, v)) for i, v in enumerate(vals)]
    wm, wd, wfb = check(tf, cfg, msgs)
    text = "%s is configured as JSON, but it isn't valid JSON" % who
    at = {v: i for i, v in enumerate(vals)}
    assert {i for i, _ in wd} == {i for i, v in enumerate(vals) if v in bad}
    assert all(cells[-1] == ("utf8", text.encode()) for _, cells in wd)
    assert wfb == [at[v] for v in fallback]   # in neither batch
    col = -1 if who == "value" else -2
    main = dict(wm)
    assert main[at[b"null"]][col] is None and main[at[None]][col] is None          # a nil cell both ways
    assert main[at[b"1E5"]][col] == ("any", b"1E5")                                   # json.Number keeps its text
    assert main[at[b'{"b":1,"a":2}']][col] == ("any", b'{"a":2,"b":1}')              # the sorting emitter
    assert main[at[b'"\xff stray"']][col] == ("any", b'"\xef\xbf\xbd stray"')        # one U+FFFD
    assert main[at[b'"\\ud800"']][col] == ("any", b'"\xef\xbf\xbd"')
    assert main[at[b'{"a":1,"a":2,"b":{"x":1,"x":[1,{"k":1,"k":2}]}}']][col] == ("any", b'{"a":2,"b":{"x":[1,{"k":2}]}}')


def test_json_empty_against_nil(tf):
    wm, wd, _ = check(tf, {"ValueType": "json", "IsKeyEnabled": True, "KeyType": "json"},
                      [msg(0, None, None), msg(1, b"", None), msg(2, None, b""), msg(3, b"", b""), msg(4, b"{}", b"[]")])
    assert [i for i, _ in wm] == [0, 4] and [c[-1][1] for _, c in wd] == [b"value is configured as JSON, but it isn't valid JSON",
                                                                          b"key is configured as JSON, but it isn't valid JSON",
                                                                          b"key is configured as JSON, but it isn't valid JSON|value is configured as JSON, but it isn't valid JSON"]


# ---- 4. the split -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("pattern", ["good", "bad", "alternating"])
def test_split_patterns(tf, n, pattern):
    vals = [b"ok %d" % i if pattern == "good" or (pattern == "alternating" and i % 2 == 0) else b"bad \xff %d" % i for i in range(n)]
    wm, wd, _ = check(tf, {"TableName": "", "ValueType": "string", "IsTimestampEnabled": True}, [msg(i, v, b"k%d" % i, {"i": str(i)}) for i, v in enumerate(vals)], topic="split")
    assert len(wm) + len(wd) == n
    if pattern == "alternating":
        assert [i for i, _ in wm] == list(range(0, n, 2)) and [i for i, _ in wd] == list(range(1, n, 2))


def test_all_eight_reasons(tf):
    """one config knows three of the eight texts (key, value, key|value): the four pairs of checked types together give all eight"""
    seen = set()
    bad = {"string": b"\xc0", "json": b"{"}
    good = {"string": b"fine", "json": b"[1]"}
    for kt in ("string", "json"):
        for vt in ("string", "json"):
            msgs = [msg(0, good[vt], good[kt]), msg(1, good[vt], bad[kt]), msg(2, bad[vt], good[kt]), msg(3, bad[vt], bad[kt]), msg(4, None, None), msg(5, bad[vt], None)]
            wm, wd, _ = check(tf, {"ValueType": vt, "IsKeyEnabled": True, "KeyType": kt, "DLQSuffix": "errors"}, msgs)
            assert [i for i, _ in wm] == [0, 4] and [i for i, _ in wd] == [1, 2, 3, 5]
            seen |= {c[-1][1] for _, c in wd}
            assert b"|" in wd[2][1][-1][1]
    assert len(seen) == 8


# ---- 5. the columns ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_offset_truncates_and_times(tf):
    times = [0, 1, -1, 999999999, 1000000000, -999999999, -1000000000, -1000000001, TS, -TS, (1 << 63) - 1, -(1 << 63)]
    msgs = [((1 << 32) + 5, t, None, b"v", None) for t in times] + [((1 << 64) - 1, 0, None, b"v", None), (1 << 63, 0, None, b"v", None)]
    wm, _, _ = check(tf, {"ValueType": "bytes", "IsTimestampEnabled": True}, msgs)
    assert wm[0][1][2] == ("u32", 5) and wm[2][1][3] == ("time", (-1, 999999999)) and wm[-2][1][2] == ("u32", 0xFFFFFFFF)


def test_headers(tf):
    five = [("k%d" % i, "v%d" % i) for i in (5, 4, 3, 2, 1)]   # descending: the device sorts
    hs = [{}, {"only": "one"}, five, None, {"esc": 'quote " back \\ <html> & \n\t\x01', "é": "ü ", b"bad\xff": b"\xc0\x80", "": ""},
          [("dup", "first"), ("a", "x"), ("dup", "last")], {"k": "v" * 300}, [("b", "2"), ("ab", "1"), ("a", "0"), ("abc", "3")]]
    msgs = [msg(i, b"good" if i % 2 else b"bad \xff", b"k", h) for i, h in enumerate(hs + hs[:1] + hs)]
    wm, wd, _ = check(tf, {"ValueType": "string", "IsHeadersEnabled": True}, msgs)
    texts = {i: c[3][1] for i, c in wm}
    assert texts[1] == b'{"only":"one"}' and texts[3] == b"null" and texts[5] == b'{"a":"x","dup":"last"}' and texts[7] == b'{"a":"0","ab":"1","abc":"3","b":"2"}'
    assert wd[0][1][4] == ("any", b"{}") and wd[1][1][4] == ("any", b'{"k1":"v1","k2":"v2","k3":"v3","k4":"v4","k5":"v5"}')
    # a batch without any header arrays: every map is nil
    p = tf.RawToTable.create("t", "bytes", headers=True)
    b = abi.message_batch("tp", 0, [msg(0, b"v"), msg(1, b"w")])
    b.header_pair_start, b.header_pairs, b.npairs, b.headers_nil = None, None, 0, None
    dm, _, _ = p.parse(b)
    assert [cells_of(dm.download(), r)[3] for r in range(2)] == [("any", b"null")] * 2


@pytest.mark.parametrize("vt", ref.TYPES)
def test_every_flag_combination(tf, vt):
    """key on / off, timestamp, headers and a table name of its own or the topic's, for every value type, the key type going round; 64 messages with nil
    and empty keys / values, valid and not"""
    pool = {"bytes": [b"\x00\xff raw", b"", None, b"x" * 9], "string": ["grüße".encode(), b"", None, b"\xe2\x82", b"abcdefgh"],
            "json": [b'{"b":[1,2],"a":null}', b"", None, b"[1", b" 17 ", b'"s"', b"null"]}
    k = 0
    for key in (False, True):
        for ts in (False, True):
            for hd in (False, True):
                for named in (False, True):
                    kt = ref.TYPES[k % 3]
                    k += 1
                    cfg = {"TableName": "named" if named else "", "ValueType": vt, "IsKeyEnabled": key, "KeyType": kt, "IsTimestampEnabled": ts, "IsHeadersEnabled": hd}
                    msgs = [msg(i, pool[vt][i % len(pool[vt])], pool[kt][(i // 2) % len(pool[kt])], None if i % 5 == 0 else {"n": str(i)}) for i in range(64)]
                    check(tf, cfg, msgs, topic="flags", ctx=cfg)


# ---- 6. the results are ordinary batches ----------------------------------------------------------------------------------------------------------------------
def test_results_are_ordinary_batches(tf):
    msgs = [msg(i, [b'{"b":%d,"a":"x"}' % i, b"[", b"null", b'"s"'][i % 4], b"key %d" % i, {"h": str(i)}) for i in range(100)]
    p = tf.RawToTable.create("ordinary", "json", "string", timestamp=True, headers=True)
    dm, dd, fb = p.parse(abi.message_batch("tp", 3, msgs))
    assert fb == [] and dm.nrows == 75 and dd.nrows == 25
    for dev in (dm, dd):
        again = tf.DeviceBatch.upload(dev.download())
        assert tf.serialize(abi.FMT_CH_JSON_EACH_ROW, dev).download() == tf.serialize(abi.FMT_CH_JSON_EACH_ROW, again).download()
        assert tf.deepsizeof(dev) == tf.deepsizeof(again)
    text = tf.serialize(abi.FMT_CH_JSON_EACH_ROW, dm).download()
    assert text.count(b"\n") == 75 and b'{\\"a\\":\\"x\\",\\"b\\":0}' in text   # (an `any` goes out as its text in a string)


def test_device_memory_batch(tf):
    """the same batch with every array in HBM (mem = TFGPU_MEM_DEVICE)"""
    msgs = [msg(i, [b"v\xc3\xa9", b"\xff", None, b""][i % 4], [b'{"z":1,"a":2}', None, b"1"][i % 3], None if i % 7 == 0 else {"h%d" % i: "v"}) for i in range(130)]
    hb = abi.message_batch("dev", 1, msgs)
    n = len(msgs)
    keep = []

    def up(ptr, nbytes):
        if not ptr or not nbytes:
            return None
        import ctypes as C
        d = tf.DeviceBuffer.upload(C.string_at(ptr, nbytes))
        keep.append(d)
        return d.ptr
    db = abi.CMessageBatch()
    db.topic, db.partition, db.mem, db.nmsg, db.npairs = hb.topic, hb.partition, abi.MEM_DEVICE, n, hb.npairs
    db.values_len, db.keys_len, db.header_bytes_len = hb.values_len, hb.keys_len, hb.header_bytes_len
    db.values, db.keys, db.header_bytes = up(hb.values, hb.values_len), up(hb.keys, hb.keys_len), up(hb.header_bytes, hb.header_bytes_len)
    db.value_start, db.key_start, db.header_pair_start = up(hb.value_start, 8 * (n + 1)), up(hb.key_start, 8 * (n + 1)), up(hb.header_pair_start, 8 * (n + 1))
    db.offset, db.write_time_ns, db.header_pairs = up(hb.offset, 8 * n), up(hb.write_time_ns, 8 * n), up(hb.header_pairs, 16 * hb.npairs)
    db.value_nil, db.key_nil, db.headers_nil = (up(x, (n + 7) // 8) for x in (hb.value_nil, hb.key_nil, hb.headers_nil))
    cfg = {"ValueType": "string", "IsKeyEnabled": True, "KeyType": "json", "IsTimestampEnabled": True, "IsHeadersEnabled": True}
    c = ref.config(cfg)
    dm, dd, fb = tf.RawToTable.from_config(cfg).parse(db)
    wm, wd, wfb = ref.do_batch(c, "dev", 1, msgs)
    assert fb == wfb
    compare_table(dm, wm, c, False, "dev", "device")
    compare_table(dd, wd, c, True, "dev", "device")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_entry(tf):
    p = tf.RawToTable.create("t", "string")
    start = np.array([0, 5, 1 << 32], np.uint64)
    b = abi.CMessageBatch()
    b.topic, b.mem, b.nmsg, b.value_start, b.values_len = b"t", abi.MEM_HOST, 2, start.ctypes.data, 1 << 32   # `values` stays NULL: nothing may read it
    with pytest.raises(tf.TfgpuError) as ei:
        p.parse(b)
    assert ei.value.code == tf.ERR_UNSUPPORTED and "the values reach 4 GiB" in str(ei.value)
    b.nmsg, b.values_len = 1 << 31, 0
    import ctypes as C
    m, d = C.c_void_p(), C.c_void_p()
    assert tf.load().tfgpu_raw_to_table_parse(p._h, C.byref(b), C.byref(m), C.byref(d), None, None) == tf.ERR_UNSUPPORTED
    assert b"more than 2^31-1 messages" in tf.load().tfgpu_last_error()
    # offsets that run backwards or past the buffer are an error of the call, found before a byte of the messages is read
    for starts in ([0, 4, 2], [0, 2, 9]):
        hb = abi.message_batch("t", 0, [msg(0, b"ab"), msg(1, b"cd")])
        bad = np.array(starts, np.uint64)
        hb.value_start = bad.ctypes.data
        with pytest.raises(tf.TfgpuError) as ei:
            p.parse(hb)
        assert ei.value.code == tf.ERR_INVALID and "ascending and inside" in str(ei.value)
