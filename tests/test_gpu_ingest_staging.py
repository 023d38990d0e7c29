"""What the ingest entries share between the C ABI and their first launch, and between their last launch and the returned batch (tf_ingest.cpp):
the refusals of the message starts and of a misaligned device pointer, entry by entry with the entry's own prefix; the lowered 4 GiB bound of a
text column (TFGPU_TEST_TEXT_LIMIT) in the protobuf parser and in raw_to_table; the empty and the one-row batch of the text-column finish."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import protoparse_ref as R
from transferia_amd import abi, confluent_sr, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SR_PROTO = b'syntax = "proto3"; package a.b.c; message V { int32 id = 1; string s = 2; P p = 3; message P { double x = 1; } }'
SR_JSON_PROPS = [("a", abi.SRT_INTEGER, False), ("s", abi.SRT_STRING, False)]
DBZ_FIELDS = [("a", abi.DBZ_INT32, False, 0)]
JSON_FIELDS = [("a", "int64")]
PP_FDS = R.fds([R.file_("t.proto", "t", messages=[R.msg("Ev", [R.field("id", 1, "int32"), R.field("s", 2, "string"), R.field("by", 3, "bytes")])])])
PP_COLS = [("id", False), ("s", False), ("by", False)]


@pytest.fixture(scope="module")
def tf():
    lib.init()
    return lib


@pytest.fixture(scope="module")
def proto_schema(tf):
    s = confluent_sr.ProtoSchema(tf, SR_PROTO)
    assert s.code == abi.ROW_OK, s.why
    return s


def messages_at(starts):
    """tfgpu_messages with the starts as given (abi.messages derives them from the values)"""
    n = len(starts) - 1
    st, off, wt = np.asarray(starts, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int64)
    m = abi.CMessages()
    m.nmsg, m.start, m.offset, m.write_time_ns = n, st.ctypes.data, off.ctypes.data, wt.ctypes.data
    m._keep = (st, off, wt)
    return m


def starts_entries(tf, proto_schema):
    """(who, call(data, msgs)) of every entry that takes message starts"""
    return [
        ("confluent SR", lambda d, m: tf.sr_frames(d, m)),
        ("confluent SR", lambda d, m: tf.sr_json_parse(abi.sr_json_options(7, SR_JSON_PROPS, "ns", "t"), d, m)),
        ("confluent SR protobuf", lambda d, m: proto_schema.parse(1, d, m)),
        ("debezium", lambda d, m: tf.debezium_unpack(d, m)),
        ("debezium", lambda d, m: tf.debezium_parse((1, 2), DBZ_FIELDS, d, np.zeros(int(m.nmsg), abi.DBZ_FRAME_DTYPE), m)),
        ("json", lambda d, m: tf.json_parse(abi.json_options(topic="t"), abi.Schema.of(JSON_FIELDS), d, m)),
    ]


# ---- 1. message starts ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("starts", [[0, 5, 3], [0, 9]], ids=["descending", "past_the_end"])
def test_message_starts_are_refused(tf, proto_schema, starts):
    data = b"\0" * 8
    entries = starts_entries(tf, proto_schema)
    assert len(entries) == 6
    for who, call in entries:
        with pytest.raises(tf.TfgpuError) as ex:
            call(data, messages_at(starts))
        assert ex.value.code == tf.ERR_INVALID, who
        assert str(ex.value).endswith(who + ": message offsets must be ascending and inside the buffer"), (who, str(ex.value))


# ---- 2. device pointer --------------------------------------------------------------------------------------------------------------------------------------
def test_misaligned_device_pointer_is_refused(tf, proto_schema):
    """a window at ptr + 1 of a block the library owns is refused before any launch; the same block at ptr is taken"""
    L = tf.load()
    buf = tf.DeviceBuffer.upload(b'{"a":1}\n' * 32)
    assert buf.size == 256 and buf.ptr % 16 == 0
    P = C.c_void_p
    opts, cs = abi.json_options(topic="t"), abi.Schema.of(JSON_FIELDS).to_c()
    L.tfgpu_sr_proto_parse.argtypes = [P, C.c_uint32, C.c_int32, P, C.c_uint64, C.c_int, P, C.POINTER(P), P, C.c_int64, C.POINTER(C.c_int64)]

    def sr_frames(p):
        arr, nf = (abi.CSrFrame * 64)(), C.c_int64(0)
        return L.tfgpu_sr_frames(p, 64, abi.MEM_DEVICE, None, arr, 64, C.byref(nf))

    def debezium_unpack(p):
        frames = np.zeros(1, abi.DBZ_FRAME_DTYPE)
        return L.tfgpu_debezium_unpack(p, 64, abi.MEM_DEVICE, None, frames.ctypes.data)

    def json_parse(p):
        out, nerr, errs = P(), C.c_int64(0), (abi.CRowError * 64)()
        rc = L.tfgpu_json_parse(C.byref(opts), C.byref(cs), p, 64, abi.MEM_DEVICE, None, C.byref(out), errs, 64, C.byref(nerr))
        if rc == 0:
            L.tfgpu_dbatch_free(out)
        return rc

    def sr_proto_parse(p):
        out, ne, errs = P(), C.c_int64(0), (abi.CRowError * 64)()
        rc = L.tfgpu_sr_proto_parse(proto_schema._h, 1, 1, p, 64, abi.MEM_DEVICE, None, C.byref(out), errs, 64, C.byref(ne))
        if rc == 0:
            L.tfgpu_dbatch_free(out)
        return rc

    for who, call in [("confluent SR", sr_frames), ("debezium", debezium_unpack), ("json", json_parse), ("confluent SR protobuf", sr_proto_parse)]:
        assert call(buf.ptr + 1) == tf.ERR_INVALID, who
        assert (L.tfgpu_last_error() or b"").decode() == who + ": device buffer must be 16-byte aligned", who
        assert call(buf.ptr) == 0, (who, (L.tfgpu_last_error() or b"").decode())


# ---- 3. the lowered text limit ------------------------------------------------------------------------------------------------------------------------------
TEXT_LIMIT_CODE = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import protoparse_ref as R
from transferia_amd import abi, lib
if os.environ.get("TFGPU_TEST_EMU_LIB"):
    lib._LIBPATH = os.environ["TFGPU_TEST_EMU_LIB"]
lib.init()
fds = R.fds([R.file_("t.proto", "t", messages=[R.msg("Ev", [R.field("s", 1, "string")])])])
values = [R.enc_bytes(1, bytes([97 + i %% 26]) * 100) for i in range(64)]
def run(name, call, text):
    try:
        print(name, "PARSED", call())
    except lib.TfgpuError as ex:
        print(name, "REFUSED", ex.code == lib.ERR_UNSUPPORTED, str(ex).endswith(text), str(ex))
par = lib.ProtoParser.create(fds, "Ev", include_columns=[("s", False)])
run("protoparse", lambda: par.parse(abi.message_batch("tp", 0, [(i, 0, None, v, None) for i, v in enumerate(values)]))[0].nrows,
    "column s holds 4 GiB of text or more: split the batch")
raw = lib.RawToTable.create()
run("rawtable", lambda: raw.parse(abi.message_batch("tp", 0, [(i, 0, None, b"v" * 100, None) for i in range(64)]))[0].nrows,
    "column value of table " + raw.table_name(abi.RTT_MAIN, "tp") + " reaches 4 GiB of text (32-bit offsets): split the batch")
""" % (ROOT, ROOT)


@pytest.fixture(scope="module")
def text_limit_runs():
    """TFGPU_TEST_TEXT_LIMIT is read once per process: a subprocess per value.  64 events / messages of 100 bytes are 6400 bytes of text in one column."""
    def run(limit):
        r = subprocess.run([sys.executable, "-c", TEXT_LIMIT_CODE], capture_output=True, text=True, timeout=600, env=dict(os.environ, TFGPU_TEST_TEXT_LIMIT=limit))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in r.stdout.strip().splitlines() if ln.startswith(("protoparse ", "rawtable "))}
        assert set(lines) == {"protoparse", "rawtable"}, r.stdout[-2000:] + r.stderr[-2000:]
        return lines
    return {"4096": run("4096"), "": run("")}


@pytest.mark.parametrize("entry", ["protoparse", "rawtable"])
def test_lowered_text_limit_refuses_the_column(text_limit_runs, entry):
    assert text_limit_runs["4096"][entry].startswith("REFUSED True True"), text_limit_runs["4096"][entry]
    assert text_limit_runs[""][entry] == "PARSED 64"


# ---- 4. the empty and the one-row batch ---------------------------------------------------------------------------------------------------------------------
def text_columns(b: abi.Batch):
    return {c.name: ([int(x) for x in c.offsets], bytes(c.data[: int(c.offsets[-1])])) for c in b.cols if c.repr in abi.VAR_REPRS}


def test_sr_protobuf_empty_and_single_row(tf, proto_schema):
    data, m = abi.messages([b""])
    db, errs = proto_schema.parse(1, data, m)
    b = db.download()
    assert b.nrows == 0 and errs == SR_EMPTY_ERRORS
    assert text_columns(b) == {"s": ([0], b""), "p": ([0], b"")}
    one = b"\0\0\0\0\x01\0" + R.enc_varint(1, 5) + R.enc_bytes(2, b"hello") + R.enc_bytes(3, R.enc_scalar(1, R.T_DOUBLE, 1.5))
    data, m = abi.messages([one])
    db, errs = proto_schema.parse(1, data, m)
    b = db.download()
    assert b.nrows == 1 and errs == {} and list(b.src_row) == [0]
    assert [c.pyvalue(0) for c in b.cols] == SR_ONE_ROW
    assert text_columns(b) == SR_ONE_TEXT


def test_protobuf_parser_empty_and_single_row(tf):
    par = tf.ProtoParser.create(PP_FDS, "Ev", "PackageTypeProtoseq", include_columns=PP_COLS)
    dev, un, base = par.parse(abi.message_batch("tp", 0, [(0, 0, None, b"", None)]))
    b = dev.download()
    assert b.nrows == 0 and len(un) == 0 and list(base) == [0, 0]
    assert text_columns(b) == {"s": ([0], b""), "by": ([0], b"")}
    ev = R.enc_varint(1, 5) + R.enc_bytes(2, b"hello") + R.enc_bytes(3, b"\x01\x02")
    dev, un, base = par.parse(abi.message_batch("tp", 0, [(0, 0, None, R.protoseq_frame(ev), None)]))
    b = dev.download()
    assert b.nrows == 1 and len(un) == 0 and list(base) == [0, 1] and list(b.src_row) == PP_ONE_SRC_ROW
    assert [c.pyvalue(0) for c in b.cols] == PP_ONE_ROW
    assert text_columns(b) == PP_ONE_TEXT


# what the commit before the shared finish returned for the bytes above
SR_EMPTY_ERRORS = {}
SR_ONE_ROW = [["int32", 5], ["string", b"hello"], ["json", b'{"x":1.5}']]
SR_ONE_TEXT = {"s": ([0, 5], b"hello"), "p": ([0, 9], b'{"x":1.5}')}
PP_ONE_SRC_ROW = [0]
PP_ONE_ROW = [["int32", 5], ["string", b"hello"], ["bytes", b"\x01\x02"]]
PP_ONE_TEXT = {"s": ([0, 5], b"hello"), "by": ([0, 2], b"\x01\x02")}
