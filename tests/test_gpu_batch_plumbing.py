"""tfgpu_dbatch_slice, tfgpu_shard_rows, tfgpu_dbatch_concat and the Bufferer's flush (tf_shard.hip, tf_pipeline.cpp) against a numpy model of the
same operations (tests/batch_ref.py): exact equality of every row — cells, nils, ABSENT bits, kinds, part ids, OldKeys with presence — and of src_row.

What the cases are after
  * shard_splice_bits is a read-modify-write of bitmap bytes that consecutive parts share: part boundaries at every row mod 8, seventeen 1-row parts
    (three or more launches rewrite one byte), parts around a wave and a workgroup, parts without rows in every position;
  * a part that lacks an optional array next to one that has it (validity, nanos, absent, kind, part_id, src_row, old_keys_present, OldKeys
    validity) must read as that array's default;
  * a text column's offsets are absolute into its data (include/tfgpu.h): offsets[0] may be non-zero and data_len may exceed offsets[nrows].  concat
    once took a part's text from 0 and data_len instead: the row in front of such a part grew by the part's offsets[0] bytes.  The consumer matrix
    holds every other entry to the same contract;
  * the bits behind the last row of a slice's bitmaps are the FOLLOWING rows' bits: no consumer may read them."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import batch_ref as ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
SEED0 = int(os.environ.get("TFGPU_TEST_SEED", "0"))
FULL = ref.ATTRS
SIZES = (0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)
SWEEP_SEED = 4248


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


# ---- comparing -----------------------------------------------------------------------------------------------------------------------
def assert_rows(got, want, ctx=""):
    """got: a download; want: the model's batch"""
    assert got.nrows == want.nrows, (ctx, "nrows", got.nrows, want.nrows)
    assert ref.shape(got) == ref.shape(want), (ctx, ref.shape(got), ref.shape(want))
    g, w = ref.rows(got), ref.rows(want)
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, (ctx, "row %d of %d" % (i, got.nrows), a, b)
    for c in got.cols:   # an ABSENT cell also reads nil
        if c.absent is not None and c.absent.any():
            assert c.validity is not None and not c.validity[c.absent].any(), (ctx, c.name, "validity under ABSENT")


def has_src_row(db):
    return bool(db.view().src_row)


def assert_src_row(db, got, want_src, ctx=""):
    """the device batch carries a src_row exactly where the model does, and the same one"""
    if got.nrows:
        assert has_src_row(db) == (want_src is not None), (ctx, "src_row present", has_src_row(db))
    if want_src is not None:
        assert np.array_equal(got.src_row, want_src), (ctx, "src_row", got.src_row[:20], want_src[:20])


def check_concat(tf, hosts, dbs=None, row_base=None, ctx=""):
    dbs = dbs if dbs is not None else [tf.DeviceBatch.upload(h) for h in hosts]
    merged = tf.DeviceBatch.concat(dbs, row_base=row_base)
    got = merged.download()
    want = ref.concat_batches(hosts, row_base)
    assert_rows(got, want, ctx)
    assert_src_row(merged, got, want.src_row, ctx)
    return merged, got, want


def parts_of(sizes, attrs_of=lambda g: FULL):
    out, start = [], 0
    for g, k in enumerate(sizes):
        out.append(ref.part(k, start, attrs_of(g)))
        start += k + 3
    return out


# ---- concat, by part sizes -----------------------------------------------------------------------------------------------------------
BOUNDARIES = [(3, 5, 1, 13), (7, 9), (9, 7, 64, 2), (1,) * 17, (63, 64, 65), (255, 1, 256, 257)]


@pytest.mark.parametrize("sizes", BOUNDARIES, ids=lambda s: "17x1" if len(s) == 17 else "-".join(map(str, s)))
@pytest.mark.parametrize("mix", ["all", "alternate"])
def test_concat_part_boundaries(tf, sizes, mix):
    """every alignment of a part boundary inside a bitmap byte; `alternate`: every second part carries no optional array at all, so the splice of
    all-ones (validity, presence) and the skipped splice (ABSENT) meet the copied bits in one byte"""
    hosts = parts_of(sizes, (lambda g: FULL) if mix == "all" else (lambda g: FULL if g % 2 == 0 else ()))
    assert {sum(sizes[:g]) % 8 for g in range(1, len(sizes))} - {0}, "no boundary inside a byte"
    check_concat(tf, hosts, ctx=(sizes, mix))
    check_concat(tf, hosts, row_base=[1000 * g for g in range(len(sizes))], ctx=(sizes, mix, "row_base"))


EMPTIES = [(0, 3, 0, 2, 0), (2, 0, 0, 3), (0,), (0, 0)]


@pytest.mark.parametrize("sizes", EMPTIES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("how", ["upload", "slice"])
@pytest.mark.parametrize("mix", ["all", "empties_only"])
def test_concat_parts_without_rows(tf, sizes, how, mix):
    """parts without rows first, in the middle, last, doubled and on their own: uploaded, or the (0, 0) slice of an 8-row batch (which still `has`
    every optional array of that batch); `empties_only`: only the parts without rows carry the optional arrays — they must decide nothing about
    src_row, and the others' rows read the defaults"""
    hosts = parts_of(sizes, (lambda g: FULL) if mix == "all" else (lambda g: FULL if sizes[g] == 0 else ()))
    dbs, keep = [], []
    for g, h in enumerate(hosts):
        if h.nrows or how == "upload":
            dbs.append(tf.DeviceBatch.upload(h))
        else:
            eight = tf.DeviceBatch.upload(ref.part(8, 500 + 10 * g, FULL))
            keep.append(eight)
            dbs.append(eight.slice(0, 0))
    check_concat(tf, hosts, dbs, ctx=(sizes, how, mix))
    check_concat(tf, hosts, dbs, row_base=[100 * g for g in range(len(sizes))], ctx=(sizes, how, mix, "row_base"))


# ---- concat, by which optional arrays a part carries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("attr", ref.ATTRS)
def test_concat_optional_array_in_one_part_only(tf, attr):
    """the array in the first part only, the last only, a middle one only, and in none; the other arrays in every part or in no part"""
    sizes = (5, 9, 3, 12)   # boundaries at rows 5, 14, 17: three alignments, none on a byte
    for others in ((), tuple(a for a in FULL if a != attr)):
        for where in (0, 3, 1, None):
            hosts = parts_of(sizes, lambda g: others + ((attr,) if g == where else ()))
            for rb in (None, [0, 40, 80, 120]):
                _, got, want = check_concat(tf, hosts, row_base=rb, ctx=(attr, where, bool(others), rb))
                if attr == "absent" and where is not None:   # the merged ABSENT bits come down, and only that part's rows have any
                    a = got.col("opt").absent
                    lo = sum(sizes[:where])
                    assert a is not None and a.any() and np.array_equal(a, want.col("opt").absent) and not a[:lo].any() and not a[lo + sizes[where]:].any()
                if attr.startswith("validity.") and where is not None and not others:   # a part without validity next to one with it reads all-valid
                    v = got.col(attr.split(".")[1]).validity
                    lo = sum(sizes[:where])
                    assert v is not None and not v.all() and v[:lo].all() and v[lo + sizes[where]:].all()
                if attr == "src_row":
                    exp = []
                    for g, k in enumerate(sizes):
                        exp.append((hosts[g].src_row.astype(np.int64) if g == where else np.arange(k)) + (rb[g] if rb else 0))
                    if where is None and rb is None and "src_row" not in others:
                        assert want.src_row is None
                    elif "src_row" not in others:
                        assert np.array_equal(got.src_row, np.concatenate(exp))


# ---- concat, a seeded random sweep -----------------------------------------------------------------------------------------------------
def sweep_trials(seed):
    """40 trials of 1-6 parts with sizes from SIZES, a random set of optional arrays per part and, half the time, a row_base.  How many of them cut
    inside a bitmap byte does not hang on the seed: only the first three draws of ONE part stand (a later one is drawn again from 2-6), and a trial
    of several parts whose boundaries all fall on multiples of 8 rows draws its sizes again.  At least 37 of the 40 therefore have such a boundary
    whatever TFGPU_TEST_SEED is."""
    rng = np.random.default_rng(seed)
    out, single = [], 0
    for _ in range(40):
        nparts = int(rng.integers(1, 7))
        if nparts == 1 and single == 3:
            nparts = int(rng.integers(2, 7))
        single += nparts == 1
        for _draw in range(1000):
            sizes = [int(rng.choice(SIZES)) for _ in range(nparts)]
            if sum(sizes) == 0:
                sizes.append(3)
            if nparts == 1 or inside_a_byte(sizes):
                break
        else:
            raise AssertionError("no part-size list with a boundary inside a byte in 1000 draws")
        attrs = [tuple(a for a in FULL if rng.integers(0, 2)) for _ in sizes]
        rb = [int(x) for x in np.cumsum(rng.integers(0, 500, len(sizes)))] if rng.integers(0, 2) else None
        out.append((sizes, attrs, rb))
    return out


def inside_a_byte(sizes):
    return any(sum(sizes[:g]) % 8 for g in range(1, len(sizes)) if sum(sizes[g:]))


def test_concat_random_sweep(tf):
    trials = sweep_trials(SEED0 + SWEEP_SEED)
    hit = 0
    for t, (sizes, attrs, rb) in enumerate(trials):
        hosts = parts_of(sizes, lambda g: attrs[g])
        check_concat(tf, hosts, row_base=rb, ctx=("trial %d" % t, sizes, attrs, rb))
        hit += inside_a_byte(sizes)
    assert hit >= 35, "only %d of 40 trials had a part boundary inside a bitmap byte" % hit


# ---- text offsets that do not start at 0 or end at data_len -------------------------------------------------------------------------------
def upload_device(tf, host, prefix=5, slack=9, short=0):
    """`host` through a TFGPU_MEM_DEVICE upload whose text columns sit `prefix` bytes into their buffers and state a data_len `slack` bytes past
    offsets[nrows] (tests/test_gpu_regex_replace.py::device_copy is the pattern: the view of an uploaded batch, handed to tfgpu_batch_upload).  `short`: the stated
    data_len is that many bytes LESS than the buffer holds (with slack = 0: less than offsets[nrows] — a column concat must refuse)"""
    db = tf.DeviceBatch.upload(host)
    v = db.view()
    keep = []
    for i, c in enumerate(host.cols):
        if c.repr not in abi.VAR_REPRS:
            continue
        o = np.asarray(c.offsets, np.int64)
        off = (o - o[0] + prefix).astype(np.uint32)
        data = b"X" * prefix + bytes(np.asarray(c.data, np.uint8)[int(o[0]): int(o[-1])]) + b"Y" * slack
        bo, bd = tf.DeviceBuffer.upload(off.tobytes()), tf.DeviceBuffer.upload(data)
        keep += [bo, bd]
        v.cols[i].offsets, v.cols[i].data, v.cols[i].data_len = bo.ptr, bd.ptr, len(data) - short
    h = C.c_void_p()
    tf._check(tf.load().tfgpu_batch_upload(C.byref(v), C.byref(h)))   # (synchronises: the buffers may go)
    return tf.DeviceBatch(h)


def upload_as(tf, host, how):
    if how == "plain":
        return tf.DeviceBatch.upload(host)
    if how == "host_shift":
        return tf.DeviceBatch.upload(ref.shift_text(host))
    if how == "device_shift":
        return upload_device(tf, host, prefix=5, slack=0)
    if how == "device_slack":
        return upload_device(tf, host, prefix=0, slack=9)
    assert how == "device_both"
    return upload_device(tf, host)


ODD = ["host_shift", "device_shift", "device_slack", "device_both"]
# where the odd part(s) stand among parts of 4, 6, 3 (and 0) rows
PLACES = {"second": ((4, 6, 3), (1,)), "first": ((4, 6, 3), (0,)), "last": ((4, 6, 3), (2,)), "twice_in_a_row": ((4, 6, 3), (1, 2)), "all": ((4, 6, 3), (0, 1, 2)),
          "behind_an_empty_part": ((4, 0, 6, 3), (2,)), "before_an_empty_part": ((4, 6, 0, 3), (1,)), "an_empty_odd_part": ((4, 0, 3), (1,)), "an_empty_odd_part_last": ((4, 6, 0), (2,))}


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("how", ODD)
def test_concat_text_offsets_anywhere_in_data(tf, how, place):
    sizes, odd = PLACES[place]
    hosts = parts_of(sizes, lambda g: ("validity.js", "nanos", "kind"))   # (no nil in `text`: every part ends on a text cell with bytes)
    for h in hosts:
        if h.nrows:
            assert len(h.col("text").get_bytes(h.nrows - 1)) > 0 and h.col("text").is_valid(h.nrows - 1)
    dbs = [upload_as(tf, h, how if g in odd else "plain") for g, h in enumerate(hosts)]
    for g in odd:   # the part itself reads back as its rows
        assert_rows(dbs[g].download(), hosts[g], (how, place, "part %d" % g))
    merged, got, want = check_concat(tf, hosts, dbs, ctx=(how, place))
    for name in ("text", "js"):   # and the merged column is packed: nothing but the cells' bytes
        c = got.col(name)
        assert int(c.offsets[0]) == 0 and int(merged.view().cols[ref.NAMES.index(name)].data_len) == int(c.offsets[-1]) == len(want.col(name).data), (how, place, name)


# ---- the consumer matrix: a shifted upload gives what the normalised upload of the same rows gives ---------------------------------------------
M_ATTRS = ("validity.text", "validity.opt", "validity.js", "nanos")
PG = {"id": "pg:bigint", "text": "pg:text", "ts": "pg:timestamp without time zone", "opt": "pg:integer", "flag": "pg:boolean", "js": "pg:jsonb"}


def _rows_src(db):
    b = db.download()
    return ref.shape(b), ref.rows(b), [int(x) for x in b.src_row]


def _apply(t, cfg):
    return lambda tf, db: _rows_src(tf.apply_chain([tf.Transformer(t, cfg)], db).transformed)


def _filter(tf, db):
    out = tf.apply_chain([tf.Transformer("filter_rows", {"filter": "text > 'b' AND opt > -40000"})], db).transformed
    assert 0 < out.nrows < db.nrows   # (the comparison reads the text cells: some rows go, some stay)
    return _rows_src(out)


def _sharded(tf, db):
    return tf.Transformer("sharder_transformer", {"shardsCount": "7", "columns": {"includeColumns": ["^text$"]}}).apply(db).transformed


def _partition(tf, db):
    p, counts = tf.partition(_sharded(tf, db), 7)
    return _rows_src(p), counts


def _table_split(tf, db):
    ts = tf.table_split(tf.Transformer("table_splitter_transformer", {"columns": ["flag", "text"], "splitter": "/"}), db)
    return ts.names(), [int(x) for x in ts.row_tables()], [_rows_src(ts.batch(t)) for t in range(ts.count)]


def _parquet(tf, db):
    import pyarrow.parquet as pq
    raw = tf.parquet_write(db, ref.SCHEMA)
    assert pq.read_table(io.BytesIO(raw)).num_rows == db.nrows
    return raw


def _dbz(tf, db):
    schema = abi.Schema([abi.ColSchema(c.name, c.dtype, c.key, "", PG[c.name]) for c in ref.SCHEMA.cols])
    params = {"database.dbname": "pguser", "topic.prefix": "fullfillment", "dt.add.original.type.info": "false", "dt.source.type": "pg"}
    return tf.debezium_emit(abi.dbz_emit_options(params, schema), db).messages()


CONSUMERS = {
    "download": lambda tf, db: _rows_src(db),
    "json": lambda tf, db: tf.serialize(abi.FMT_JSON, db).download(),
    "csv": lambda tf, db: tf.serialize(abi.FMT_CSV, db).download(),
    "jsoneachrow": lambda tf, db: tf.serialize(abi.FMT_CH_JSON_EACH_ROW, db).download(),
    "queue_native": lambda tf, db: tf.queue_serialize(abi.queue_options(abi.QFMT_NATIVE, table_schema=ref.SCHEMA), db).messages(),
    "deepsizeof": lambda tf, db: (lambda r: (r[0], [int(x) for x in r[1]]))(tf.deepsizeof(db, per_row=True)),
    "mask_field": _apply("mask_field", {"columns": ["text"], "maskFunctionHash": {"userDefinedSalt": "s"}}),
    "convert_to_string": _apply("convert_to_string", {}),
    "filter_rows": _filter,
    "sharder_transformer": lambda tf, db: _rows_src(_sharded(tf, db)),
    "slice": lambda tf, db: _rows_src(db.slice(8, 13)),
    "to_lane": lambda tf, db: _rows_src(db.to_lane(1)),
    "partition": _partition,
    "collapse": lambda tf, db: _rows_src(tf.collapse(db)),
    "parquet_write": _parquet,
    "ch_native_block": lambda tf, db: tf.ch_native_block(db, [("id", "Int64"), ("text", "Nullable(String)"), ("opt", "Nullable(Int32)")]).download(),
    "regex_replace_transformer": _apply("regex_replace_transformer", {"regexMatch": "[a7]|\\d\\d", "replaceRule": "<$0>", "columns": {"includeColumns": ["^text$", "^js$"]}}),
    "table_split": _table_split,
    "raw_doc_grouper": lambda tf, db: _rows_src(tf.apply_meta([tf.Transformer("raw_doc_grouper", {"keys": ["id"]})], db).transformed),
    "debezium_emit": _dbz,
}


@pytest.fixture(scope="module")
def matrix_batches():
    plain = ref.part(29, 100, M_ATTRS, old=False)
    cdc = ref.part(29, 100, M_ATTRS + ("kind", "old_present"))
    return plain, cdc


@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("how", ["host_shift", "device_both"])
def test_consumer_reads_text_through_its_offsets(tf, matrix_batches, consumer, how):
    host = matrix_batches[1 if consumer == "collapse" else 0]
    try:
        want = CONSUMERS[consumer](tf, tf.DeviceBatch.upload(host))
        got = CONSUMERS[consumer](tf, upload_as(tf, host, how))
    finally:
        tf.lane_use(0)
    assert want is not None and len(want) > 0
    assert got == want, (consumer, how)


# ---- producers' outputs as parts --------------------------------------------------------------------------------------------------------
def _csv(tf, n, row0):
    from transferia_amd import workload
    data = workload.hits_csv(n, row0=row0)
    db, consumed, errs = tf.csv_parse(workload.hits_csv_options(), workload.hits_schema(), data)
    assert consumed == len(data) and not errs and db.nrows == n
    return db


def _filtered(tf, n, start):
    db = tf.DeviceBatch.upload(ref.part(n, start, M_ATTRS))
    out = tf.apply_chain([tf.Transformer("filter_rows", {"filter": "opt > -40000"})], db).transformed
    assert 13 < out.nrows < n and out.nrows % 8, out.nrows
    return out


def _transformed(t, cfg):
    def make(tf, n, start):
        return tf.apply_chain([tf.Transformer(t, cfg)], tf.DeviceBatch.upload(ref.part(n, start, M_ATTRS, old=False))).transformed
    return make


def _parquet_read(tf, n, start):
    import pyarrow as pa
    import pyarrow.parquet as pq
    k = list(range(start, start + n))
    t = pa.table({"k": pa.array(k, pa.int64()), "s": pa.array([None if i % 3 == 0 else "s%d" % i * (i % 4) for i in k]), "d": pa.array([None if i % 5 == 0 else i / 4 for i in k], pa.float64()),
                  "b": pa.array([None if i % 7 == 0 else bool(i & 1) for i in k])})
    buf = io.BytesIO()
    pq.write_table(t, buf)
    return tf.parquet_read(buf.getvalue(), None, "ns", "tbl")


NGINX = '$remote_addr - $remote_user [$time_local] "$request" $status $body_bytes_sent "$http_referer" "$http_user_agent"'


def _nginx(tf, n, start):
    lines = b"".join(b'10.0.%d.%d - %s [19/Oct/2026:10:%02d:00 +0000] "GET /p/%d HTTP/1.1" %d %d "-" "agent/%d"\n' % (i % 200, i % 7, b"-" if i % 3 else b"bob", i % 60, i, 200 + i % 5, i * 37, i % 11)
                     for i in range(start, start + n))
    f = tf.NginxFormat(NGINX)
    db, consumed, _nxt, errs = tf.nginx_parse(f, tf.nginx_options(last_chunk=True), f.resolve_schema(), lines)
    assert consumed == len(lines) and not errs and db.nrows == n
    return db


PRODUCERS = {"csv_parse": _csv, "filter_rows": _filtered, "mask_field": _transformed("mask_field", {"columns": ["text"], "maskFunctionHash": {"userDefinedSalt": "s"}}),
             "convert_to_string": _transformed("convert_to_string", {}), "parquet_read": _parquet_read, "nginx_parse": _nginx}


def kernels_of(tf, call):
    """(what call() returned, the names under which the library timed device work on this lane while it ran)"""
    tf.prof_enable(True)
    try:
        tf.prof_reset()
        out = call()
        tf.synchronize()
        return out, {name for name, launches, _ms in tf.prof_get() if launches}
    finally:
        tf.prof_enable(False)


# what the library must still have to do when it first reads a producer's output: pack text that is a view into the source (csv_copy_words), gather
# the rows a filter kept (compact_gather).  If a producer came to finish that work itself, its case here would stop covering the hand-over.
LEFT_TO_DO = {"csv_parse": "csv_copy_words", "nginx_parse": "csv_copy_words", "filter_rows": "compact_gather"}


def _laid_end_to_end(tf, parts, ctx, ran=()):
    """concat(parts) against the parts' own downloads laid end to end (the parts are downloaded AFTER the merge: it sees them as their producer left
    them, text still a view into the source, rows still a selection).  `ran`: what handling the parts before the merge has run already."""
    merged, during = kernels_of(tf, lambda: tf.DeviceBatch.concat(parts))
    todo = LEFT_TO_DO.get(ctx.split(",")[0])
    if todo:
        assert todo in set(ran) | during, (ctx, "the parts were complete before anything read them", sorted(during))
    got = merged.download()
    had = [has_src_row(p) for p in parts]
    downs = [p.download() for p in parts]
    for d, h in zip(downs, had):
        if not h:
            d.src_row = None   # (a download spells the identity out)
    if ctx.split(",")[0] == "filter_rows":   # kept rows, not all rows: the parts count in their sources
        assert all(had) and not any(np.array_equal(d.src_row, np.arange(d.nrows)) for d in downs), ctx
    want = ref.concat_batches(downs)
    assert_rows(got, want, ctx)
    assert_src_row(merged, got, want.src_row, ctx)


@pytest.mark.parametrize("producer", PRODUCERS)
def test_concat_of_producers_outputs(tf, producer):
    make = PRODUCERS[producer]
    a, b = make(tf, 53, 0), make(tf, 29, 1000)
    assert a.nrows % 8 and b.nrows % 8 and a.nrows != b.nrows
    _laid_end_to_end(tf, [a, b, a], producer)   # (nrows touches no column: the merge is the first to read them)
    a2, b2 = make(tf, 53, 0), make(tf, 29, 1000)   # fresh ones: the slice reads them as the producer left them
    (sa, sb), ran = kernels_of(tf, lambda: (a2.slice(8, a2.nrows - 11), b2.slice(8, 5)))
    if producer in LEFT_TO_DO:
        assert LEFT_TO_DO[producer] in ran, (producer, "slice", sorted(ran))
    assert sa.nrows % 8
    _laid_end_to_end(tf, [sa, sb, sa], producer + ", slices", ran)


# ---- slice ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slice_sources(tf):
    """an uploaded batch and a merged one of 45 rows with every optional array, and their ABSENT-free twins (the serializers compute on values and
    refuse ABSENT cells by name)"""
    out = {}
    for name, attrs in (("full", FULL), ("values", tuple(a for a in FULL if a != "absent"))):
        host = ref.part(45, 7, attrs)
        hosts = parts_of((13, 5, 27), lambda g: attrs)
        out[name] = [("uploaded", host, tf.DeviceBatch.upload(host)), ("merged", ref.concat_batches(hosts), tf.DeviceBatch.concat([tf.DeviceBatch.upload(h) for h in hosts]))]
    return out


@pytest.mark.parametrize("row0", [0, 8, 16, 32])
@pytest.mark.parametrize("nrows", [0, 1, 7, 8, 13, 23, None], ids=lambda n: "to_the_end" if n is None else str(n))
def test_slice_is_the_rows_it_names(tf, oracle, slice_sources, row0, nrows):
    for what, host, db in slice_sources["full"]:
        n = host.nrows - row0 if nrows is None else nrows
        if row0 + n > host.nrows:
            with pytest.raises(tf.TfgpuError):
                db.slice(row0, n)
            continue
        s = db.slice(row0, n)
        got, want = s.download(), ref.slice_batch(host, row0, n)
        assert_rows(got, want, (what, row0, n))
        assert_src_row(s, got, want.src_row, (what, row0, n))
    for what, host, db in slice_sources["values"]:
        n = host.nrows - row0 if nrows is None else nrows
        if row0 + n > host.nrows or n % 8 == 0:
            continue
        # the bits behind the slice's last row are the following rows' bits: what the serializers and deepsizeof give is the numpy slice's
        s, want = db.slice(row0, n), ref.slice_batch(host, row0, n)
        assert_rows(s.download(), want, (what, row0, n, "values"))
        exp = oracle.serialize(abi.FMT_CH_JSON_EACH_ROW, want, ref.SCHEMA)
        assert exp is not None and tf.serialize(abi.FMT_CH_JSON_EACH_ROW, s).download() == exp, (what, row0, n, "JSONEachRow")
        assert tf.deepsizeof(s) == oracle.deepsizeof(want, ref.SCHEMA)[0], (what, row0, n, "deepsizeof")


def test_slice_refuses_a_row0_inside_a_byte(tf, slice_sources):
    for _what, _host, db in slice_sources["full"]:
        with pytest.raises(tf.TfgpuError, match="multiple of 8"):
            db.slice(3, 1)


# ---- shard_rows, then concat --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g", [(1, 3), (65, 8), (64, 3), (130, 4)])
def test_shard_rows_then_concat_is_the_identity(tf, n, g):
    """shards that come out empty or ragged (cuts at multiples of 64 rows), all lanes on one device"""
    host = ref.part(n, 11, FULL)
    db = tf.DeviceBatch.upload(host)
    try:
        parts, row0 = db.shard_rows(g, lanes=list(range(g)))
        assert row0[0] == 0 and all(r % 64 == 0 or r == n for r in row0) and sum(p.nrows for p in parts) == n
        assert any(p.nrows == 0 for p in parts) or len({p.nrows for p in parts}) > 1
        at = 0
        for p in parts:   # each shard is the rows it names
            assert_rows(p.download(), ref.slice_batch(host, at, p.nrows), (n, g, at))
            at += p.nrows
        merged = tf.DeviceBatch.concat(parts)
        got = merged.download()
        assert_rows(got, host, (n, g))
        assert_src_row(merged, got, host.src_row, (n, g))
        # with the shards' first rows as row_base, parts that carry no src_row of their own come back with the rows of the batch that was cut
        bare = ref.part(n, 11, tuple(a for a in FULL if a != "src_row"))
        parts, row0 = tf.DeviceBatch.upload(bare).shard_rows(g, lanes=list(range(g)))
        back = tf.DeviceBatch.concat(parts, row_base=row0)
        got = back.download()
        assert_rows(got, bare, (n, g, "row_base"))
        assert_src_row(back, got, np.arange(n, dtype=np.int32), (n, g, "row_base"))
    finally:
        tf.lane_use(0)


# ---- the Bufferer's flush ---------------------------------------------------------------------------------------------------------------
FLUSH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_uint64)


@pytest.mark.parametrize("known", [True, False], ids=["row_base_known", "row_base_unknown"])
def test_bufferer_flush_is_the_concat_of_what_was_pushed(tf, known):
    """tests/test_pipeline.py::test_bufferer_flush_is_one_device_concat over the mixed schema: parts of 3, 5, 1 and 13 rows, count trigger 22, the flushed
    batch compared whole.  With every part's source extent stated (async_push_meta) src_row is shifted per part; with one push that does not state
    it (async_push) the merged batch carries none."""
    L = tf.load()
    got, errs = [], []

    def flush(user, merged, parts, nparts, nrows, size):
        try:
            view = tf.DeviceBatch(C.c_void_p(merged))
            got.append((nparts, nrows, has_src_row(view), view.download()))
            view._h = None   # the handle stays the bufferer's
        except BaseException as e:  # noqa: BLE001 (reported to the main thread)
            errs.append(repr(e))
            return 1
        return 0
    cb = FLUSH(flush)
    L.tfgpu_bufferer_create.argtypes = [C.c_int64, C.c_uint64, C.c_int64, C.c_int, FLUSH, C.c_void_p, C.POINTER(C.c_void_p)]
    L.tfgpu_bufferer_async_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.tfgpu_bufferer_async_push_meta.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int64, C.POINTER(C.c_uint64)]
    L.tfgpu_bufferer_wait.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L.tfgpu_bufferer_close.argtypes = [C.c_void_p]
    L.tfgpu_bufferer_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.tfgpu_bufferer_create(22, 0, 0, 1, cb, None, C.byref(h)) == 0
    sizes, source_rows = (3, 5, 1, 13), (10, 20, 5, 40)   # (src_row of part() runs to 3 k - 1 < the stated source rows)
    hosts = parts_of(sizes, lambda g: FULL if g != 2 else tuple(a for a in FULL if a not in ("src_row", "nanos", "absent")))
    dbs, tickets = [], []
    for g, host in enumerate(hosts):
        db = tf.DeviceBatch.upload(host)
        dbs.append(db)
        t = C.c_uint64(0)
        if known or g != 1:
            assert L.tfgpu_bufferer_async_push_meta(h, db._h, host.nrows, 64, 0, source_rows[g], C.byref(t)) == 0
        else:
            assert L.tfgpu_bufferer_async_push(h, db._h, host.nrows, 64, 0, C.byref(t)) == 0
        tickets.append(t.value)
    assert [L.tfgpu_bufferer_wait(h, t, 60000) for t in tickets] == [0] * 4, errs
    L.tfgpu_bufferer_close(h)
    L.tfgpu_bufferer_destroy(h)
    assert errs == [] and [(x[0], x[1]) for x in got] == [(4, 22)]
    base = [0, 10, 30, 35]
    want = ref.concat_batches(hosts, base)
    assert_rows(got[0][3], want, known)
    assert [int(x) for x in got[0][3].col("id").values] == [int(x) for x in want.col("id").values]
    if known:
        assert got[0][2] and np.array_equal(got[0][3].src_row, want.src_row)
        assert np.array_equal(want.src_row[8:9], [30]) and want.src_row[9] == 35 + 2   # (the part without a src_row counts from its base)
    else:
        assert not got[0][2], "a merged batch whose parts' source rows cannot be lined up carries no src_row"


# ---- refusals stay named -----------------------------------------------------------------------------------------------------------------
def test_concat_refusals(tf):
    a = ref.part(5, 0, FULL)
    da = tf.DeviceBatch.upload(a)

    def refused(other, match):
        with pytest.raises(tf.TfgpuError, match=match):
            tf.DeviceBatch.concat([da, tf.DeviceBatch.upload(other)])
    fewer = ref.part(3, 9, FULL)
    fewer.cols = fewer.cols[:-1]
    refused(fewer, "different columns")
    renamed = ref.part(3, 9, FULL)
    renamed.cols[1].name = "other"
    refused(renamed, "column text differs")
    other_repr = ref.part(3, 9, FULL)
    other_repr.cols[5].repr = abi.R_STRING
    refused(other_repr, "column js differs")
    no_old = ref.part(3, 9, FULL, old=False)
    refused(no_old, "different columns")
    refused(ref.part(3, 9, FULL, table="u"), "different tables")
    other_schema = ref.part(3, 9, FULL)
    other_schema.schema = abi.Schema.of([["id", "int64", True], ["text", "utf8", True], ["ts", "timestamp"], ["opt", "int32"], ["flag", "boolean"], ["js", "any"]])
    refused(other_schema, "different tables / schemas")
    # a text column whose offsets run past the data_len its device upload stated: refused before a byte of it is read
    short = upload_device(tf, ref.part(3, 9, FULL), prefix=0, slack=0, short=2)
    with pytest.raises(tf.TfgpuError, match="offsets outside its data"):
        tf.DeviceBatch.concat([da, short])
    # a null part
    hs = (C.c_void_p * 2)(da._h, None)
    out = C.c_void_p()
    assert tf.load().tfgpu_dbatch_concat(hs, 2, None, C.byref(out)) != 0 and not out.value
    with pytest.raises(tf.TfgpuError, match="null part"):
        tf._check(tf.load().tfgpu_dbatch_concat(hs, 2, None, C.byref(out)))


def test_a_batch_with_its_own_column_order_is_not_cut_or_merged(tf):
    """col_order is an output of tfgpu_collapse: two Updates of one key that list different columns merge into a row whose names are not in batch order"""
    from collapse_cases import batch_from_items
    items = [{"kind": "update", "keys": ["id"], "names": ["id", "b"], "values": [["int64", 1], ["string", "b0"]]},
             {"kind": "update", "keys": ["id"], "names": ["id", "s"], "values": [["int64", 1], ["string", "a1"]]}]
    ordered = tf.collapse(tf.DeviceBatch.upload(batch_from_items(items, names=["id", "s", "b"])[0]))
    assert ordered.view().col_order
    with pytest.raises(tf.TfgpuError, match="ColumnNames order"):
        tf.DeviceBatch.concat([ordered, ordered])
    with pytest.raises(tf.TfgpuError, match="ColumnNames order"):
        ordered.slice(0, 1)
