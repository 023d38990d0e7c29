"""CSV text columns in the LENGTHS state (TextView::lens, tf_common.hpp): the tile parser leaves a text column's lengths unscanned, a row
filter's gather carries them on, and materialize() (ensure_text_offsets, tf_rows.hip) scans them when the first reader asks for offsets.

Every expected value comes from the oracle (csv_parse / apply_chain / deepsizeof / serialize) or from numpy over a download; the device's
own eager form (TFGPU_CSV_SCAN_EAGER=1) is never the reference.

The input: 400 rows of six columns (id int32, s1 utf8, n int64, d date, s2 utf8, k uint8), about 100 KB, which is four 28 KiB tiles of
csv_parse_regular.  The text cells hold empty cells, "quoted" cells, quoted cells with a doubled quote inside (the has_special case) and, in
the rows that straddle the first three tile boundaries, a cell of s1 whose last byte is the last byte of its tile.  The same rows are also
parsed behind one header line (skip_rows=1), with the boundary cells fitted again.

Case 8 (one handle read from two lanes) is the ORDERED hand-over of tests/test_gpu_lane_handover.py case a, without that file's hold switch:
two lanes that call materialize() on one handle AT THE SAME MOMENT race on the host side on TextView::packed and on the handle's own
DColumn fields (nothing orders `packed` between lanes: DESIGN §2, "what orders a shared view"), which this change does not widen itself to
fix; a test that provokes that race would test the finding, not the lengths state."""
import threading

import numpy as np
import pytest

from transferia_amd import abi
from test_gpu_transformers import assert_batches_equal

pytestmark = pytest.mark.gpu

TILE = 28 * 1024   # csv_parse_regular's tile (CT_T)
NROWS = 400
SCHEMA = abi.Schema.of([["id", "int32", True, "0"], ["s1", "utf8", False, "1"], ["n", "int64", False, "2"], ["d", "date", False, "3"],
                        ["s2", "utf8", False, "4"], ["k", "uint8", False, "5"]])
TEXT = ("s1", "s2")
HEADER = b"id,s1,n,d,s2,k\n"


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def make_csv(nrows=NROWS, header=False, bad_rows=(), seed=11):
    """-> bytes.  Row r: id r, n = a permutation value in [0, nrows), so `n >= c` keeps a known share; bad_rows get a word where n stands"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nrows)
    words = [b"alpha", b"be ta", b"g\xc3\xa4mma", b"d'elta", b"eps;lon"]
    out = bytearray(HEADER if header else b"")
    boundary = TILE
    for r in range(nrows):
        kind = r % 8
        w = words[r % len(words)]
        if kind == 0:
            s1 = b""                                                # empty cell
        elif kind == 1:
            s1 = b'"' + w + b", quoted" + b'"'                       # quoted cell (a delimiter inside)
        elif kind == 2:
            s1 = b'"' + w + b' ""twice"" ' + w + b'"'                # doubled quote inside quotes
        else:
            s1 = w * int(rng.integers(1, 80))                      # plain, 5 .. 550 bytes
        s2 = [b"", b'""', b'"x"', w, b'"a""b"', w * 12][int(rng.integers(0, 6))] + (b"p" * int(rng.integers(0, 400)) if kind >= 3 else b"")
        if s2.startswith(b'"') and not s2.endswith(b'"'):
            s2 = w
        n_cell = b"%d" % int(perm[r]) if r not in bad_rows else b"12x"
        head = b"%d," % r
        tail = b",%s,2013-07-%02d,%s,%d\n" % (n_cell, 1 + r % 28, s2, r % 200)
        # the row that would cross the next tile boundary: its s1 cell (plain bytes) is stretched or cut to END at the boundary
        if kind >= 3 and len(out) + len(head) < boundary - 8 and len(out) + len(head) + len(s1) + len(tail) > boundary:
            s1 = (s1 * 4)[: boundary - len(out) - len(head)]
            boundary += TILE
        out += head + s1 + tail
    return bytes(out)


def boundary_cells(data):
    """how many tile boundaries fall directly behind the last byte of an unquoted s1 cell (the byte AT the boundary is its delimiter)"""
    hits = 0
    for b in range(TILE, len(data), TILE):
        line0 = data.rfind(b"\n", 0, b) + 1
        first = data.index(b",", line0)
        if data[b:b + 1] == b"," and data.find(b",", first + 1) == b and b'"' not in data[first + 1:b]:
            hits += 1
    return hits


def opts_for(header):
    return abi.csv_options(skip_rows=1 if header else 0)


def parse(tf, data, header=False):
    db, consumed, errs = tf.csv_parse(opts_for(header), SCHEMA, data, max_errors=1 << 12)
    return db, consumed, errs


def check_download(db, ref_batch, ctx):
    """offsets, bytes and data_len of the text columns (and every other column) against the oracle's batch"""
    v = db.view()
    dl = {v.cols[i].name.decode(): int(v.cols[i].data_len) for i in range(v.ncols)}
    out = db.download()
    if ref_batch.nrows == 0:
        assert out.nrows == 0, ctx
        for name in TEXT:
            assert dl[name] == 0 and np.array_equal(out.col(name).offsets, np.zeros(1, np.uint32)), (ctx, name)
        return out
    assert_batches_equal(out, ref_batch, ctx)
    for name in TEXT:
        assert dl[name] == int(ref_batch.col(name).offsets[-1]), (ctx, name, "data_len")
    return out


@pytest.fixture(scope="module")
def inputs(oracle):
    """{header: (csv bytes, the oracle's parse of them)}: computed once, read by every case, changed by none"""
    res = {}
    for header in (False, True):
        data = make_csv(header=header)
        assert len(data) >= 3 * TILE + 1024, len(data)          # four tiles
        assert boundary_cells(data) >= 2, boundary_cells(data)  # cells that end where a tile ends
        ref = oracle.csv_parse(opts_for(header), SCHEMA, data, "", "")
        assert ref.batch.nrows == NROWS and not ref.errors
        res[header] = (data, ref)
    return res


def chain_for(mod, const):
    return [mod.Transformer("filter_rows", {"filter": "n >= %d" % const})]


def scans(tf):
    tf.synchronize()
    return sum(n for name, n, _ms in tf.prof_get() if name == "scan_u32_segments")


@pytest.mark.parametrize("header", [False, True])
def test_parse_download(tf, oracle, inputs, header):
    """1. parse -> download"""
    data, ref = inputs[header]
    db, consumed, errs = parse(tf, data, header)
    assert consumed == ref.consumed and not errs
    check_download(db, ref.batch, "parse, header=%s" % header)


@pytest.mark.parametrize("header", [False, True])
@pytest.mark.parametrize("const,what", [(NROWS // 2, "half"), (NROWS, "none"), (0, "all")])
def test_filter_download(tf, oracle, inputs, header, const, what):
    """2. parse -> filter_rows keeping about half / none / all (the shallow copy) -> download"""
    data, ref = inputs[header]
    db, _, _ = parse(tf, data, header)
    got = tf.apply_chain(chain_for(tf, const), db).transformed
    want = oracle.apply_chain(chain_for(oracle, const), ref.batch, ref.schema).batch
    assert got.nrows == want.nrows == {"half": NROWS - NROWS // 2, "none": 0, "all": NROWS}[what]
    out = check_download(got, want, "filter %s, header=%s" % (what, header))
    if want.nrows:
        assert np.array_equal(out.src_row, want.src_row)
    check_download(db, ref.batch, "the parsed batch behind its filter, %s" % what)   # the source of the selection, read afterwards


def test_no_data_rows(tf, oracle):
    """2, "none": a CSV of zero data rows (a header alone, and nothing at all) through parse -> filter -> download"""
    for data, header in ((HEADER, True), (b"", False)):
        ref = oracle.csv_parse(opts_for(header), SCHEMA, data, "", "")
        db, consumed, errs = parse(tf, data, header)
        assert db.nrows == ref.batch.nrows == 0 and consumed == ref.consumed and not errs
        got = tf.apply_chain(chain_for(tf, 1), db).transformed
        assert got.nrows == 0
        check_download(got, ref.batch, "zero data rows, filtered")
        check_download(db, ref.batch, "zero data rows")


def test_malformed_lines(tf, oracle):
    """3. three lines that fail, in three different tiles: nobody zeroes their lengths any more — compact_rows reads the kept rows' only"""
    bad = (40, 190, 350)
    data = make_csv(bad_rows=bad, seed=12)
    starts = [0] + [i + 1 for i, ch in enumerate(data) if ch == 10]
    assert len({starts[r] // TILE for r in bad}) == 3
    ref = oracle.csv_parse(opts_for(False), SCHEMA, data, "", "")
    assert sorted(e[0] for e in ref.errors) == list(bad)
    db, consumed, errs = parse(tf, data)
    assert consumed == ref.consumed
    assert sorted((e[0], e[1]) for e in errs) == sorted((e[0], abi.ROWERR[e[1]]) for e in ref.errors)
    out = check_download(db, ref.batch, "three malformed lines")
    assert np.array_equal(out.src_row, ref.batch.src_row)


def test_sized_ahead_second_parse(tf, oracle, inputs):
    """4. two parses on one lane: the second is sized from the first one's bytes per line and holds about 5 % fewer rows, so its
    buffers (and the stride between the columns' lengths) are larger than its true row count"""
    data, ref = inputs[False]
    first, _, _ = parse(tf, data)
    n2 = NROWS * 95 // 100
    data2 = make_csv(nrows=n2, seed=13)
    assert len(data2) >= 2 * TILE
    ref2 = oracle.csv_parse(opts_for(False), SCHEMA, data2, "", "")
    second, consumed, errs = parse(tf, data2)
    assert consumed == ref2.consumed and not errs and second.nrows == n2
    check_download(second, ref2.batch, "the second, sized-ahead parse")
    check_download(first, ref.batch, "the first parse, read behind the second")
    got = tf.apply_chain(chain_for(tf, n2 // 2), parse(tf, data2)[0]).transformed
    want = oracle.apply_chain(chain_for(oracle, n2 // 2), ref2.batch, ref2.schema).batch
    check_download(got, want, "a sized-ahead parse, filtered")


def test_deepsizeof_scans_nothing(tf, oracle, inputs):
    """5. DeepSizeof of a parsed and of a filtered batch reads the lengths themselves: the oracle's value, the same value once a download
    has made offsets, and no scan_u32_segments launch in between"""
    data, ref = inputs[False]
    want_parsed = oracle.deepsizeof(ref.batch, ref.schema)[0]
    fb = oracle.apply_chain(chain_for(oracle, NROWS // 2), ref.batch, ref.schema)
    want_filtered = oracle.deepsizeof(fb.batch, fb.schema)[0]
    tf.prof_enable(True)
    try:
        db, _, _ = parse(tf, data)
        flt = tf.apply_chain(chain_for(tf, NROWS // 2), db).transformed
        tf.prof_reset()
        a, b = tf.deepsizeof(db), tf.deepsizeof(flt)
        assert scans(tf) == 0
    finally:
        tf.prof_enable(False)
    assert (a, b) == (want_parsed, want_filtered)
    db.download(); flt.download()
    assert (tf.deepsizeof(db), tf.deepsizeof(flt)) == (want_parsed, want_filtered)


def test_scan_counts(tf, oracle, inputs):
    """6. parse -> filter -> drop (the benchmark's path): no scan_u32_segments launch at all; parse -> download twice: one"""
    data, ref = inputs[False]
    tf.prof_enable(True)
    try:
        tf.prof_reset()
        db, _, _ = parse(tf, data)
        flt = tf.apply_chain(chain_for(tf, NROWS // 2), db).transformed
        assert flt.nrows == NROWS - NROWS // 2
        flt.free(); db.free()
        assert scans(tf) == 0
        tf.prof_reset()
        db, _, _ = parse(tf, data)
        one = db.download()
        two = db.download()
        assert scans(tf) == 1
    finally:
        tf.prof_enable(False)
    assert_batches_equal(one, ref.batch, "first download")
    assert_batches_equal(two, ref.batch, "second download")


def np_rows(b, idx):
    """rows idx of a downloaded batch's columns: plain numpy"""
    idx = np.asarray(idx, np.int64)
    cols = []
    for c in b.cols:
        o = abi.Column(c.name, c.dtype, c.repr)
        if c.repr in abi.VAR_REPRS:
            off = c.offsets.astype(np.int64)
            lens = (off[1:] - off[:-1])[idx]
            no = np.zeros(len(idx) + 1, np.int64); no[1:] = np.cumsum(lens)
            byte = np.repeat(off[:-1][idx] - no[:-1], lens) + np.arange(int(no[-1]), dtype=np.int64)
            o.offsets, o.data = no.astype(np.uint32), np.asarray(c.data, np.uint8)[byte]
        else:
            o.values = c.values[idx]
            if c.nanos is not None:
                o.nanos = c.nanos[idx]
        if c.validity is not None:
            o.validity = c.validity[idx]
        cols.append(o)
    return abi.Batch(cols, len(idx), b.table_ns, b.table_name)


def test_slice_concat_to_lane(tf, oracle, inputs):
    """7. slice, concat with a second parsed batch and to_lane of batches still in the lengths state, against numpy slicing and
    concatenation of the originals' downloads (taken AFTER the operation: a download would make the offsets first)"""
    data, ref = inputs[False]
    data2 = make_csv(nrows=300, seed=14)
    try:
        a, _, _ = parse(tf, data)
        sl = a.slice(8, 200).download()
        assert_batches_equal(sl, np_rows(a.download(), np.arange(8, 208)), "slice")

        a, _, _ = parse(tf, data)
        b, _, _ = parse(tf, data2)
        both = tf.DeviceBatch.concat([a, b], row_base=[0, NROWS]).download()
        da, db_ = a.download(), b.download()
        assert_batches_equal(da, ref.batch, "the first part")
        for c in da.cols:   # one host batch of both parts' rows
            d = db_.col(c.name)
            if c.repr in abi.VAR_REPRS:
                c.offsets = np.concatenate([c.offsets, d.offsets[1:] + c.offsets[-1]]).astype(np.uint32)
                c.data = np.concatenate([c.data[: int(da.col(c.name).offsets[NROWS])], d.data])
            else:
                c.values = np.concatenate([c.values, d.values])
                if c.nanos is not None or d.nanos is not None:
                    c.nanos = np.concatenate([c.nanos if c.nanos is not None else np.zeros(NROWS, np.int32), d.nanos if d.nanos is not None else np.zeros(300, np.int32)])
            if c.validity is not None or d.validity is not None:
                c.validity = np.concatenate([c.validity if c.validity is not None else np.ones(NROWS, bool), d.validity if d.validity is not None else np.ones(300, bool)])
        da.nrows = NROWS + 300
        assert_batches_equal(both, da, "concat")
        assert np.array_equal(both.src_row, np.concatenate([np.arange(NROWS), np.arange(300) + NROWS]))

        a, _, _ = parse(tf, data)
        flt = tf.apply_chain(chain_for(tf, NROWS // 2), a).transformed
        moved = flt.to_lane(1)
        tf.lane_use(1)
        got = moved.download()
        tf.lane_use(0)
        want = oracle.apply_chain(chain_for(oracle, NROWS // 2), ref.batch, ref.schema).batch
        assert_batches_equal(got, want, "to_lane of a filtered batch")
        assert_batches_equal(flt.download(), want, "the filtered batch behind to_lane")
    finally:
        tf.lane_use(0)
        tf.synchronize()


def test_one_handle_two_lanes(tf, oracle, inputs):
    """8. lane 1 parses and filters (a selection over columns in the lengths state); lane 2 makes it dense and downloads it; then lane 1
    serializes the same handle — and the other way round.  Ordered by host events, no device synchronize between the lanes (module docstring)."""
    data, ref = inputs[False]
    want = oracle.apply_chain(chain_for(oracle, NROWS // 2), ref.batch, ref.schema)
    want_json = oracle.serialize(abi.FMT_JSON, want.batch, want.schema)
    assert want_json is not None
    errs = []
    try:
        for first in ("download", "serialize"):
            made, read = threading.Event(), threading.Event()
            box, got = {}, {}

            def reader(h, what):
                if what == "download":
                    h.dense()
                    return h.download()
                return tf.serialize(abi.FMT_JSON, h).download()

            def maker():
                try:
                    tf.lane_use(1)
                    db, _, _ = parse(tf, data)
                    box["db"] = db
                    box["h"] = tf.apply_chain(chain_for(tf, NROWS // 2), db).transformed
                    made.set()
                    assert read.wait(120)
                    got["maker"] = reader(box["h"], "serialize" if first == "download" else "download")
                except BaseException as e:  # noqa: BLE001 (reported to the main thread)
                    errs.append(repr(e))
                    made.set()

            def other():
                try:
                    tf.lane_use(2)
                    assert made.wait(120)
                    got["other"] = reader(box["h"], first)
                except BaseException as e:  # noqa: BLE001
                    errs.append(repr(e))
                finally:
                    read.set()
            ts = [threading.Thread(target=f, daemon=True) for f in (maker, other)]
            for t in ts:
                t.start()
            for t in ts:
                t.join(300)
            assert not any(t.is_alive() for t in ts) and errs == [], errs
            dl, js = (got["other"], got["maker"]) if first == "download" else (got["maker"], got["other"])
            assert_batches_equal(dl, want.batch, "two lanes, %s first: the download" % first)
            assert js == want_json, "two lanes, %s first: the serializer" % first
    finally:
        tf.lane_use(0)
        tf.synchronize()
