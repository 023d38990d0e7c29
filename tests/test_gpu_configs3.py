"""BASELINE.json configs[3] end to end from its real source format: a hits-shaped Parquet object (tests/hits_parquet.py) →
mask_field(clientip) + sharder_transformer(userid) + convert_to_string + convert_to_datetime → ClickHouse JSONEachRow.

Each stage has tests of its own; these check the seams between them.  (a) the object, under the user OutputSchema, decodes to the
same columns as the CSV parse of the same rows, for every writer shape; (b) the composite against the oracle (ora_parquet.read →
oracle chain → oracle serializer), byte for byte, with row errors and PartIDs; (c) the same under the schema the reference resolves
from the footer; (d) the ways into the reader give the same bytes; (e) three lanes side by side give each object's own bytes.
The chain is the bench's own (bench.wl_configs3.Configs3Workload.CH), so the two cannot drift apart."""
import hashlib
import io
import os
import re
import sys
import threading

import numpy as np
import pytest

from transferia_amd import abi, workload

pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hits_parquet as hp  # noqa: E402
from bench.wl_configs3 import Configs3Workload  # noqa: E402
from oracle import ora_parquet  # noqa: E402

pytestmark = pytest.mark.gpu
CH = Configs3Workload.CH
FMT = abi.FMT_CH_JSON_EACH_ROW
# the CPU emulator's pre-flight (tools/hipemu/run_gpu_tests.py, which sets TFGPU_TEST_EMU_LIB) runs the kernels a thousand times slower:
# there the same tests run on fewer rows, still over several row groups; the MI355X run is the one at these sizes
EMU = bool(os.environ.get("TFGPU_TEST_EMU_LIB"))
N_A = 7001 if EMU else 20011
N_B = 4099 if EMU else 65536 + 13
N_E = 1201 if EMU else 6007
COMPOSITE = dict(codec="SNAPPY", dictionary_pagesize_limit=4096, row_group_size=N_B // 4 + 1)  # dictionary → PLAIN partway, four row groups


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def csv_columns(tf, n, row0=0):
    """the device's CSV parse of hits rows [row0, row0 + n) under hp.SCHEMA, downloaded"""
    db, consumed, errs = tf.csv_parse(workload.hits_csv_options(), hp.SCHEMA, workload.hits_csv(n, row0=row0))
    assert not errs and db.nrows == n
    host = db.download()
    db.free()
    return host


def columns_diff(got: abi.Batch, want: abi.Batch):
    """None when the two batches hold the same cells: names, dtype AND repr, validity, values of valid cells, the bytes of text cells,
    nanoseconds (0 where a side has none); else what differs first"""
    if got.nrows != want.nrows:
        return "rows %d vs %d" % (got.nrows, want.nrows)
    if [c.name for c in got.cols] != [c.name for c in want.cols]:
        return "column names"
    n = got.nrows
    for a, b in zip(got.cols, want.cols):
        if (a.dtype, a.repr) != (b.dtype, b.repr):
            return "column %s: dtype / repr %s vs %s" % (a.name, (a.dtype, a.repr), (b.dtype, b.repr))
        va = np.ones(n, bool) if a.validity is None else np.asarray(a.validity, bool)
        vb = np.ones(n, bool) if b.validity is None else np.asarray(b.validity, bool)
        if not np.array_equal(va, vb):
            return "column %s: validity (first at row %d)" % (a.name, int(np.flatnonzero(va != vb)[0]))
        if a.repr in abi.VAR_REPRS:
            la, lb = np.diff(np.asarray(a.offsets, np.int64))[va], np.diff(np.asarray(b.offsets, np.int64))[vb]
            if not np.array_equal(la, lb):
                return "column %s: lengths (first at valid row %d)" % (a.name, int(np.flatnonzero(la != lb)[0]))
            ta = b"".join(a.get_bytes(i) for i in np.flatnonzero(va)) if not va.all() else bytes(a.data[: int(a.offsets[-1])])
            tb = b"".join(b.get_bytes(i) for i in np.flatnonzero(vb)) if not vb.all() else bytes(b.data[: int(b.offsets[-1])])
            if ta != tb:
                return "column %s: text bytes" % a.name
        else:
            x, y = np.asarray(a.values)[va], np.asarray(b.values)[vb]
            if x.dtype != y.dtype or not np.array_equal(x, y):
                return "column %s: values %s vs %s" % (a.name, x.dtype, y.dtype)
            if a.repr == abi.R_TIME:
                na = np.zeros(n, np.int32) if a.nanos is None else np.asarray(a.nanos)
                nb = np.zeros(n, np.int32) if b.nanos is None else np.asarray(b.nanos)
                if not np.array_equal(na[va], nb[vb]):
                    return "column %s: nanoseconds" % a.name
    return None


def device_json(tf, db, plans=None, free=True):
    """(JSONEachRow text, row errors, PartIDs) of the chain over a device batch"""
    tr = tf.apply_chain(plans if plans is not None else [tf.Transformer(t, c) for t, c in CH], db)
    out = tf.serialize(FMT, tr.transformed)
    text = bytes(out.download())
    part = tr.transformed.download().part_id
    out.free(); tr.transformed.free()
    if free:
        db.free()
    return text, sorted(e[0] for e in tr.errors), part


def oracle_json(oracle, obj, schema: abi.Schema, file_name=""):
    """the same from the oracle: ora_parquet.read → rows as the reference's constructCI makes them → the oracle's chain and serializer"""
    rows = ora_parquet.read(obj, [(c.name, c.dtype) for c in schema.cols], file_name)
    b = abi.batch_from_rows(schema, [c.name for c in schema.cols], rows)
    r = oracle.apply_chain([oracle.Transformer(t, c) for t, c in CH], b, schema)
    return bytes(oracle.serialize(FMT, r.batch, r.schema)), sorted(e[0] for e in r.errors), r.batch.part_id


@pytest.fixture(scope="module")
def csv_a(tf):
    return csv_columns(tf, N_A)


# ---- (a) ----

@pytest.mark.parametrize("shape", sorted(hp.SHAPES))
def test_object_decodes_to_the_csv_columns(tf, csv_a, shape):
    """Under the user OutputSchema (int16 columns stored as INT32 + INT(16)), the Parquet read equals the CSV parse cell for cell —
    the int16 columns come back as int16, as Restore's cast.ToInt16 makes them (restore.go:127-131)."""
    obj, held = hp.write(csv_a, **hp.SHAPES[shape])
    got = tf.parquet_read(obj, hp.SCHEMA).download()
    why = columns_diff(got, held)
    assert why is None, "%s: %s" % (shape, why)


# ---- (b), (c) ----

@pytest.fixture(scope="module")
def csv_b(oracle):
    r = oracle.csv_parse(workload.hits_csv_options(), hp.SCHEMA, workload.hits_csv(N_B))
    assert not r.errors and r.batch.nrows == N_B
    return r.batch


@pytest.mark.parametrize("knobs", [{}, dict(nulls=0.05, subsecond=True)], ids=["plain", "nulls_subsecond"])
def test_composite_against_the_oracle(tf, oracle, csv_b, knobs):
    """Parquet read → chain → JSONEachRow on the device = ora_parquet.read → oracle chain → oracle serializer, byte for byte; with
    nulls, nil cells go through mask, sharder and both casts, and fractional seconds into JSONEachRow."""
    obj, _ = hp.write(csv_b, **COMPOSITE, **knobs)
    text, errs, part = device_json(tf, tf.parquet_read(obj, hp.SCHEMA))
    want, werrs, wpart = oracle_json(oracle, obj, hp.SCHEMA)
    assert len(want) > 1000 * N_B and len(pq.ParquetFile(io.BytesIO(obj)).metadata.to_dict()["row_groups"]) == 4
    assert text == want, "JSONEachRow differs (%d vs %d bytes)" % (len(text), len(want))
    assert errs == werrs
    assert np.array_equal(part, wpart)
    if knobs:  # the leg did carry nil cells (JSONEachRow leaves their keys out) and sub-second times (nanoseconds in the text)
        lines = want.split(b"\n")[:-1]
        assert len(lines) == N_B and sum(b'"userid":' not in x for x in lines) > N_B // 40
        assert any(not t.endswith(b"000000000") for t in re.findall(rb'"eventtime":(\d+)', want[:1 << 20]))


def test_composite_under_the_resolved_schema(tf, oracle, csv_b):
    """parquet_resolve_schema (system columns __file_name / __row_index, INT(16) → int64) against ora_parquet.resolve_schema, then the
    same chain and JSONEachRow, device against oracle."""
    obj, _ = hp.write(csv_b, **COMPOSITE)
    s = tf.parquet_resolve_schema(obj)
    ref = ora_parquet.resolve_schema(obj)
    assert [(c.name, c.dtype, c.original_type, c.key) for c in s.cols] == [(n, t, ot, k) for n, t, ot, k, _ in ref]
    assert s.dtype_of("javaenable") == "int64" and s.cols[0].name == "__file_name"
    fname = "hits/part-00000.parquet"
    text, errs, part = device_json(tf, tf.parquet_read(obj, s, file_name=fname))
    want, werrs, wpart = oracle_json(oracle, obj, abi.Schema.of([[n, t, k, "", ot, req] for n, t, ot, k, req in ref]), fname)
    assert text == want, "JSONEachRow differs (%d vs %d bytes)" % (len(text), len(want))
    assert errs == werrs
    assert np.array_equal(part, wpart)


# ---- (d) ----

@pytest.mark.parametrize("codec", ["SNAPPY", "LZ4_RAW"])
def test_ways_in_give_the_same_bytes(tf, csv_a, codec, monkeypatch):
    """TFGPU_PQ_DEVICE_INFLATE 1 / 0 / unset, parquet_read_staged and a read from a pinned HostBuffer: the bytes of the default read."""
    obj, _ = hp.write(csv_a, codec=codec, data_page_size=16384, row_group_size=N_A // 3 + 1)
    monkeypatch.delenv("TFGPU_PQ_DEVICE_INFLATE", raising=False)
    want = device_json(tf, tf.parquet_read(obj, hp.SCHEMA))
    for mode in ("1", "0"):
        monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", mode)
        assert device_json(tf, tf.parquet_read(obj, hp.SCHEMA))[0] == want[0], mode
    monkeypatch.delenv("TFGPU_PQ_DEVICE_INFLATE")
    staged = tf.DeviceBuffer.alloc(tf.parquet_staging_size(obj))
    staged.write(0, np.frombuffer(obj, np.uint8), len(obj))
    got = device_json(tf, tf.parquet_read_staged(obj, staged, hp.SCHEMA))
    staged.free()
    assert got[0] == want[0], "staged"
    pinned = tf.HostBuffer(obj)
    got = device_json(tf, tf.parquet_read(pinned, hp.SCHEMA))
    pinned.free()
    assert got[0] == want[0], "pinned"
    assert np.array_equal(got[2], want[2]) and got[1] == want[1]


# ---- (e) ----

def test_three_lanes_give_each_objects_own_bytes(tf):
    """Three lanes read, transform and serialize three different objects at once (host-inflated ZSTD pages in the per-thread
    pre-inflate arena, SNAPPY and LZ4_RAW pages, reads from pinned memory): each lane's bytes are its object's single-lane bytes."""
    assert tf.lane_count() >= 3
    objs = [hp.write(csv_columns(tf, N_E, row0=r0), **kw)[0] for r0, kw in ((0, dict(codec="ZSTD")), (50000, dict(codec="SNAPPY", row_group_size=N_E // 3)),
                                                                             (90001, dict(codec="LZ4_RAW", data_page_size=4096, nulls=0.05, subsecond=True)))]
    single = [device_json(tf, tf.parquet_read(o, hp.SCHEMA))[0] for o in objs]
    assert len(set(single)) == 3
    rounds = 4
    go = threading.Barrier(3)
    got, errs = {}, []

    def lane(j):
        try:
            tf.lane_use(j)
            plans = [tf.Transformer(t, c) for t, c in CH]
            pinned = tf.HostBuffer(objs[j])
            go.wait()
            for k in range(rounds):
                got[(j, k)] = device_json(tf, tf.parquet_read(pinned if k % 2 else objs[j], hp.SCHEMA), plans)[0]
            tf.synchronize()
            pinned.free()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            go.abort()
    ths = [threading.Thread(target=lane, args=(j,)) for j in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    tf.lane_use(0)
    assert not errs, errs
    for (j, k), text in sorted(got.items()):
        assert hashlib.sha256(text).digest() == hashlib.sha256(single[j]).digest(), (j, k)
    assert len(got) == 3 * rounds


# ---- the `any` column and integer narrowing ----

def test_any_column_over_byte_array(tf, oracle):
    """`hitcolor` is `any` in the hits schema.  Read here (restore.go:217-252): parquet-go hands a BYTE_ARRAY leaf over as []byte, and
    Restore's `any` branch unmarshals only a string, so the []byte comes back as it is — R_BYTES on the device and in the oracle."""
    pa = pytest.importorskip("pyarrow")
    vals = ["C", "E", None, "", '{"a":1}', "F"] * 50
    buf = io.BytesIO()
    pq.write_table(pa.table({"hitcolor": pa.array(vals, pa.string()), "k": pa.array(range(len(vals)), pa.int32())}), buf, compression="SNAPPY")
    obj = buf.getvalue()
    s = abi.Schema.of([["hitcolor", "any"], ["k", "int16"]])
    got = tf.parquet_read(obj, s).download()
    want = abi.batch_from_rows(s, ["hitcolor", "k"], ora_parquet.read(obj, [("hitcolor", "any"), ("k", "int16")], ""))
    assert got.col("hitcolor").repr == want.col("hitcolor").repr == abi.R_BYTES
    assert got.col("k").repr == want.col("k").repr == abi.R_INT16
    assert abi.batch_rows(got) == abi.batch_rows(want)
