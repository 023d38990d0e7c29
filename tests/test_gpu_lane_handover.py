"""One batch read from two lanes: the selection -> dense hand-over of tf::dense / tf::dense_locked (tf_rows.hip).

filter_rows and skip_events hand their kept rows on as a selection (tfgpu_dbatch::pending); the first reader gathers them in place, and the
gather is only QUEUED on the gathering lane's stream.  A reader on another lane has to order its stream behind it (the lane's dense_event).
Every case here lets two host threads on two lanes read ONE pending handle and compares what each of them got with a reference that does not
come from that path:

  * kept rows, validity, kind, src_row, part_id: the input's numpy columns under a numpy boolean mask (the filter is `i64 > constant` behind
    skip_events(update): `(kind != update) & (i64 > constant)`), src_row = np.flatnonzero(mask);
  * serialized bytes: at the small size the oracle's serializer over those numpy rows; at every size the bytes the device gives for the
    numpy-gathered rows uploaded DENSE on one lane behind a synchronize (no selection, no second lane; tests/test_serializers.py pins that
    path to the oracle);
  * mask_field: Python's hmac / hashlib over the numpy-kept rows' text.

What makes a missing wait visible
  * The gather must last many kernel-launch latencies.  Measured once on the commit before this file (rocprofv3 --kernel-trace --stats, a run of
    its own, MI355X), the compact_gather kernels of ONE selection -> dense transition that keeps 31-44 % of the rows (the trace also shows
    skip_events' own, larger gather in front of each):
        mixed table, 2^20 rows:  about 0.1 ms (gather_bytes_all 38 us, gather_fixed_all 19 us, gather_len_all and gather_bitmap_all 4 us each)
        fixed table, 2^21 rows:  about 0.1 ms (ONE gather_fixed_all launch of 88 us, gather_bitmap_all 5 us)
        wide table,  2^23 rows:  2.0-2.2 ms (ONE gather_fixed_all launch of 1 999 / 2 168 / 2 240 us over 149 columns, gather_bitmap_all 9-23 us);
                                 3.9-4.1 ms between the library's own events around the call
    The first two are UNDER the ~0.3 ms such a test needs, and they cannot show a missing wait: on the parent commit with only the hold knob
    added, cases b, c and e PASS on them.  They stay as cases of the hand-over's values over every consumer; the `wide` table (the fixed table plus
    128 int64 columns, 1.2 KB a row) is the one sized for the race, and on it the same library FAILS b, c and e (below).  None of these figures is
    a pass/fail threshold.
  * A table with text columns cannot show a missing wait at any size: gather_batch reads the packed text lengths back to the host (a stream
    synchronize) before it returns, so that gather is complete, not queued, when the lock is released.  The `fixed` and `wide` tables have no such
    read-back: their gather IS only queued.
  * Between a lane's look at the handle and its first read of the columns there must be no slow host work either: a hipMalloc for every column
    of a reader's result outlasts a short gather.  On the wide table the readers are row windows (tfgpu_dbatch_slice: the last rows first) and a
    second filter_rows, and a rehearsal on OTHER rows of the same count fills every lane's block cache with buffers of the race's sizes first
    (_wide_case).  Case e queues sixteen more gathers in front of the one under test: 36 ms of backlog against the 16 ms that making a lane
    took (a stream and 8 MiB of pinned memory; both printed by the case).
  * The HBM block cache hands a freed buffer back to the next request of its size: a repeat of the same batch would find the previous, correct
    gather in the stale buffers and pass falsely.  Every repetition therefore filters with another constant (other rows are kept: a stale buffer
    holds another answer), the previous repetition's handles stay alive until the next one has been compared (its buffers cannot be handed out
    meanwhile), the references' own dense uploads stay alive until the comparison is over, and the wide table's rehearsal leaves in the caches
    the answer for rows the race does not keep.
  * TFGPU_DENSE_HOLD_MS=n (read once per process, tests only) makes a caller that has seen a selection sleep n ms before it asks for the gather,
    with no lock held: two threads behind one barrier then both see `pending`, one gathers, the other certainly arrives behind it.  Such knobs
    are latched at first use, so these cases run in a child Python process of their own (never a re-exec of one that opened the GPU).

The CPU emulator pre-flight (tools/hipemu/run_gpu_tests.py) runs the small size of every case; its streams run in order, so there it proves
the tests' logic and references, not the waits.  The full-size cases (`fullsize` in their names) need the MI355X.

That the cases bite: on the parent commit plus only the hold knob (one MI355X visit), at full size on the wide table,
  b  failed: ('b: wide 8388608 rows, 2516080 kept: row windows on lane 1, window 0 of (last rows, middle, first rows)', 'i8', 'values',
              '1532 of 4096 rows differ, rows 208 .. 3983')
  c  failed: ('c: wide 8388608 rows, 2516880 kept: row windows on lane 1, window 0 of (last rows, middle, first rows)', 'i8', 'values',
              '1224 of 4096 rows differ, rows 1456 .. 4095')
  e  failed: ('e: wide 8388608 rows, 2516696 kept: row windows read from a lane bound after the gather was queued, window 0 of (last rows, middle,
              first rows)', 'i8', 'values', '4079 of 4096 rows differ, rows 0 .. 4095')
(value mismatches: no crash, no hang), case a passed, and with the waits in place all of them pass."""
import ctypes as C
import gc
import hashlib
import hmac
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":  # a child process of cases b-e and g (see _child): the same import roots a pytest run has
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)

from transferia_amd import abi  # noqa: E402

SEED0 = int(os.environ.get("TFGPU_TEST_SEED", "0"))  # 0 = the committed seeds; other values: soak runs

pytestmark = pytest.mark.gpu

SMALL = 3000
FULL = {"mixed": 1 << 20, "fixed": 1 << 21, "wide": 1 << 23}
TABLES = ("mixed", "fixed")
RACE_TABLES = TABLES + ("wide",)   # cases b, c, e: the table whose gather is long enough to be caught unfinished
WIDE_COLS = 128
DECOYS = 16
HOLD_MS = 200       # far above a barrier's skew (tens of microseconds)
WAIT_S = 300        # every wait between threads and every join gives up after this
CHILD_S = 900
UPDATE = 1          # tfgpu kind of an Update row (skip_events drops them; filter_rows takes Inserts only)
NPARTS = 3


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


# ---- the table and its numpy reference ---------------------------------------------------------------------------------------------
def _table(rng, n, table):
    """tests/test_gpu_transformers.py::_random_batch (every fixed-width repr, two text columns, times, nils) with kinds and part ids;
    `fixed`: without the text columns and with sixteen more int64 columns (a gather that is never read back); `wide`: with WIDE_COLS more
    (derived from i64 by arithmetic: 8 GiB at 2^23 rows would take long to draw), a gather of milliseconds."""
    def strs(maxlen, alphabet=b"abcxyz0123 ,\"'\\\xd0\xb9", valid=None):
        lens = rng.integers(0, maxlen, n)
        if valid is not None:
            lens = lens * valid  # canonical batches carry no payload under nil values
        off = np.zeros(n + 1, np.uint32); off[1:] = np.cumsum(lens)
        data = rng.choice(np.frombuffer(alphabet, np.uint8), int(off[-1])).astype(np.uint8)
        return off, data
    cols = []
    for name, r, dt, lo, hi in [("i8", abi.R_INT8, "int8", -128, 128), ("i16", abi.R_INT16, "int16", -2**15, 2**15),
                                ("i32", abi.R_INT32, "int32", -2**31, 2**31), ("i64", abi.R_INT64, "int64", -2**62, 2**62),
                                ("u8", abi.R_UINT8, "uint8", 0, 256), ("u16", abi.R_UINT16, "uint16", 0, 2**16),
                                ("u32", abi.R_UINT32, "uint32", 0, 2**32), ("u64", abi.R_UINT64, "uint64", 0, 2**63)]:
        cols.append(abi.Column(name, dt, r, values=rng.integers(lo, hi, n).astype(abi.REPR_NP[r])))
    edge = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1][: min(4, n)]
    cols[3].values[: len(edge)] = edge
    cols.append(abi.Column("b", "boolean", abi.R_BOOL, values=rng.integers(0, 2, n).astype(np.uint8)))
    if table == "mixed":
        sv = rng.random(n) > 0.1
        o, d = strs(40, valid=sv)
        cols.append(abi.Column("s", "utf8", abi.R_STRING, offsets=o, data=d, validity=sv))
        o, d = strs(150)
        cols.append(abi.Column("by", "string", abi.R_BYTES, offsets=o, data=d))
    else:
        for k in range(16):
            cols.append(abi.Column("w%d" % k, "int64", abi.R_INT64, values=rng.integers(-2**62, 2**62, n)))
        for k in range(WIDE_COLS if table == "wide" else 0):
            cols.append(abi.Column("x%d" % k, "int64", abi.R_INT64, values=cols[3].values * np.int64(2 * k + 3) + np.int64(k)))   # (wraps: any bits do)
    secs = rng.integers(-62135596800, 253402300799, n)
    cols.append(abi.Column("ts", "timestamp", abi.R_TIME, values=secs, nanos=rng.integers(0, 10**9, n).astype(np.int32) * (rng.random(n) > 0.5)))
    cols.append(abi.Column("d", "date", abi.R_TIME, values=(secs // 86400) * 86400, nanos=np.zeros(n, np.int32)))
    cols.append(abi.Column("dt", "datetime", abi.R_TIME, values=secs.copy(), validity=rng.random(n) > 0.05))
    cols.append(abi.Column("iv", "interval", abi.R_DURATION, values=rng.integers(-10**15, 10**15, n) * rng.integers(0, 2, n)))
    b = abi.Batch(cols, n, "db", "tbl")
    b.kind = rng.choice(np.array([0, 0, 0, UPDATE], np.uint8), n)
    b.part_id = rng.integers(0, NPARTS, n).astype(np.uint32)
    schema = abi.Schema.of([[c.name, c.dtype, c.name == "i64"] for c in cols])
    return b, schema


def _constants(b, k):
    """k filter constants around the median of i64: each keeps about half the rows, no two keep the same ones"""
    v = np.sort(b.col("i64").values)
    n = len(v)
    return [int(v[n // 2 + (j - k // 2) * max(n // (4 * k), 1)]) for j in range(k)]


def _kept_mask(b, const):
    return (b.kind != UPDATE) & (b.col("i64").values > const)


def _take(b, idx):
    """rows idx (an index array, in that order) of a host batch: plain numpy"""
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
    out = abi.Batch(cols, len(idx), b.table_ns, b.table_name)
    out.kind = b.kind[idx] if b.kind is not None else None
    out.part_id = b.part_id[idx] if b.part_id is not None else None
    out.src_row = (b.src_row[idx] if b.src_row is not None else idx).astype(np.int32)
    return out


def _expected(b, const):
    return _take(b, np.flatnonzero(_kept_mask(b, const)))


def _first_diff(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    m = min(len(a), len(b))
    d = np.flatnonzero(a[:m] != b[:m])
    return "lengths %d / %d, %d of the common %d bytes differ, first at %s" % (len(a), len(b), len(d), m, int(d[0]) if len(d) else None)


def _rows_diff(x, y):
    d = np.flatnonzero(np.asarray(x) != np.asarray(y))
    return "%d of %d rows differ, rows %d .. %d" % (len(d), len(x), int(d[0]), int(d[-1])) if len(d) else "equal"


def assert_batches_equal(a: abi.Batch, b: abi.Batch, ctx=""):
    """every column (values, nanos, offsets, bytes), validity, kind, src_row and part_id of `a` (from the device) against `b` (the reference)"""
    assert a.nrows == b.nrows, (ctx, "nrows", a.nrows, b.nrows)
    assert [c.name for c in a.cols] == [c.name for c in b.cols], ctx
    n = a.nrows
    for ca, cb in zip(a.cols, b.cols):
        va = ca.validity if ca.validity is not None else np.ones(n, bool)
        vb = cb.validity if cb.validity is not None else np.ones(n, bool)
        assert ca.dtype == cb.dtype and ca.repr == cb.repr, (ctx, ca.name, ca.dtype, cb.dtype, ca.repr, cb.repr)
        assert np.array_equal(va, vb), (ctx, ca.name, "validity", _rows_diff(va, vb))
        if ca.repr in abi.VAR_REPRS:
            assert np.array_equal(ca.offsets, cb.offsets), (ctx, ca.name, "offsets", _rows_diff(ca.offsets, cb.offsets))
            da, db = bytes(ca.data[: int(ca.offsets[-1])]), bytes(cb.data[: int(cb.offsets[-1])])
            assert da == db, (ctx, ca.name, "data", _first_diff(da, db))
        else:
            assert np.array_equal(ca.values[va], cb.values[vb]), (ctx, ca.name, "values", _rows_diff(np.where(va, ca.values, 0), np.where(vb, cb.values, 0)))
            if ca.repr == abi.R_TIME:
                na = ca.nanos if ca.nanos is not None else np.zeros(n, np.int32)
                nb = cb.nanos if cb.nanos is not None else np.zeros(n, np.int32)
                assert np.array_equal(na[va], nb[vb]), (ctx, ca.name, "nanos", _rows_diff(np.where(va, na, 0), np.where(vb, nb, 0)))
    for f in ("kind", "src_row", "part_id"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (ctx, f, "present", x is not None, y is not None)
        if x is not None:
            assert np.array_equal(x, y), (ctx, f, _rows_diff(x, y))


def _same(got, want, ctx):
    if isinstance(want, abi.Batch):
        assert_batches_equal(got, want, ctx)
    elif isinstance(want, tuple):
        assert len(got) == len(want), ctx
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s [%d]" % (ctx, k))
    elif isinstance(want, (bytes, bytearray)):
        assert got == want, (ctx, _first_diff(got, want))
    else:
        assert got == want, (ctx, got, want)


# ---- the consumers that call tf::dense: what each returns for a handle, and the reference for it -------------------------------------
FORMATS = {"json": abi.FMT_JSON, "csv": abi.FMT_CSV, "jsoneachrow": abi.FMT_CH_JSON_EACH_ROW}
READERS = ("json", "csv", "jsoneachrow", "queue", "download", "concat", "slice", "deepsizeof", "partition")


def _read(tf, name, h, nsrc):
    """reader `name` on handle h, on the calling thread's lane; everything it made is downloaded before it returns"""
    if name in FORMATS:
        return tf.serialize(FORMATS[name], h).download()
    if name == "queue":
        return tf.queue_serialize(abi.queue_options(abi.QFMT_JSON, enabled=False), h).values.download()
    if name == "download":
        return h.download()
    if name == "concat":
        return tf.DeviceBatch.concat([h, h], row_base=[0, nsrc]).download()
    if name == "slice":
        return h.slice(8, h.nrows // 2).download()
    if name == "deepsizeof":
        return tf.deepsizeof(h)
    if name == "partition":
        p, counts = tf.partition(h, NPARTS)
        return (p.download(), list(counts))
    raise KeyError(name)


class Want:
    """the references for one set of kept rows.  `exp`: the numpy rows; `dense`: the same rows uploaded dense on the calling lane (the device
    bytes of the serializers come from it, behind a synchronize, before any second lane touches anything)."""

    def __init__(self, tf, oracle, exp, schema, nsrc, names, small):
        self.exp, self.by = exp, {}
        dense = tf.DeviceBatch.upload(exp)
        m = exp.nrows
        for name in names:
            if name in FORMATS or name == "queue" or name == "deepsizeof":
                w = _read(tf, name, dense, nsrc)
                if small and name in FORMATS:  # ... and those bytes are the oracle's
                    ob = oracle.serialize(FORMATS[name], exp, schema)
                    assert ob is not None and w == ob, (name, "dense device bytes against the oracle's serializer")
                if small and name == "queue":
                    msgs = oracle.queue_serialize(abi.queue_options(abi.QFMT_JSON, enabled=False), exp, schema)
                    assert msgs is not None and w == b"".join(msgs), "dense device queue messages against the oracle's"
                if small and name == "deepsizeof":
                    assert w == oracle.deepsizeof(exp, schema)[0], "dense device deepsizeof against the oracle's"
            elif name == "download":
                w = exp
            elif name == "concat":
                two = _take(exp, np.concatenate([np.arange(m), np.arange(m)]))
                two.src_row = np.concatenate([exp.src_row, exp.src_row + nsrc]).astype(np.int32)
                w = two
            elif name == "slice":
                w = _take(exp, np.arange(8, 8 + m // 2))
                w.src_row = exp.src_row[8: 8 + m // 2]
            elif name == "partition":
                order = np.argsort(exp.part_id, kind="stable")
                w = _take(exp, order)
                w.src_row = exp.src_row[order]
                w = (w, [int(x) for x in np.bincount(exp.part_id, minlength=NPARTS)])
            self.by[name] = w
        tf.synchronize()
        self._dense = dense   # alive until the comparison is over: its buffers, which hold the ANSWER, are not handed to the gather under test


def _chain(tf, const, op=">"):
    return [tf.Transformer("skip_events", {"events": ["update"]}), tf.Transformer("filter_rows", {"filter": "i64 %s %d" % (op, const)})]


def _run_threads(fns):
    """each fn on a thread of its own; exceptions are collected, every join has a timeout"""
    errs = []

    def wrap(f):
        def run():
            try:
                f()
            except BaseException as e:  # noqa: BLE001 (reported to the main thread)
                import traceback
                errs.append("%s: %r\n%s" % (f.__name__, e, traceback.format_exc()))
        return run
    ts = [threading.Thread(target=wrap(f), daemon=True) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(WAIT_S)
    assert not any(t.is_alive() for t in ts), "a thread did not finish in %d s; errors so far: %s" % (WAIT_S, errs)
    assert errs == [], "\n".join(errs)


def _wait(ev):
    if not ev.wait(WAIT_S):
        raise TimeoutError("the other thread never signalled")


# ---- a. ordered hand-over ---------------------------------------------------------------------------------------------------------------
def _ordered_handover(tf, oracle, n, table, readers=READERS, small=True, seed=1):
    rng = np.random.default_rng(SEED0 + 7100 + seed)
    b, schema = _table(rng, n, table)
    tf.lane_use(1)
    src = tf.DeviceBatch.upload(b)     # lane 1 makes the batch and the selection
    tf.lane_use(0)
    combos = [(r, who) for r in readers for who in ("other", "maker")]
    prev = []
    try:
        for const, (r, who) in zip(_constants(b, len(combos)), combos):
            second = "download" if r != "download" else "json"
            want = Want(tf, oracle, _expected(b, const), schema, n, (r, second), small)
            assert 0 < want.exp.nrows < n
            made, read = threading.Event(), threading.Event()
            box, got = {}, {}

            def maker():
                tf.lane_use(1)
                h = box["h"] = tf.apply_chain(_chain(tf, const), src).transformed
                assert h.nrows == want.exp.nrows     # (no column was touched)
                if who == "maker":                   # the maker gathers on its stream; the other lane reads behind it
                    got["maker"] = _read(tf, r, h, n)
                made.set()                           # NO synchronize: the other lane has to order itself
                _wait(read)
                got["maker2"] = _read(tf, second, h, n)   # at once, the same handle

            def other():
                tf.lane_use(2)
                _wait(made)
                try:
                    got["other"] = _read(tf, r if who == "other" else second, box["h"], n)   # who == "other": this lane gathers
                finally:
                    read.set()
            _run_threads([maker, other])
            ctx = "%s %d rows, reader %s, gathered by the %s lane" % (table, n, r, who)
            if who == "maker":
                _same(got["maker"], want.by[r], ctx + ": the gathering lane's result")
                _same(got["other"], want.by[second], ctx + ": the other lane's result")
            else:
                _same(got["other"], want.by[r], ctx + ": the gathering lane's result")
            _same(got["maker2"], want.by[second], ctx + ": the maker's read behind the other lane's")
            for h in prev:
                h.free()
            prev = [box["h"]]   # stays alive over the next repetition: its buffers are not handed to it
    finally:
        tf.lane_use(0)
        tf.synchronize()


@pytest.mark.parametrize("table", TABLES)
def test_ordered_handover(tf, oracle, table):
    """a. lane 1 filters and leaves the selection; without a synchronize lane 2 reads it (and gathers), then lane 1 reads — and the same with
    lane 1 gathering first — for every consumer that calls tf::dense"""
    _ordered_handover(tf, oracle, SMALL, table)


@pytest.mark.parametrize("table", TABLES)
def test_ordered_handover_fullsize(tf, oracle, table):
    _ordered_handover(tf, oracle, FULL[table], table, small=False, seed=2)


# ---- b, c, e on the wide table: cheap readers over a gather of milliseconds -----------------------------------------------------------------
def _const_for_count(b, m, op):
    """the constant c for which `(kind != update) & (i64 op c)` keeps exactly m rows (i64 is distinct among the rows that count)"""
    v = np.sort(b.col("i64").values[b.kind != UPDATE])
    assert len(np.unique(v)) == len(v) and 0 < m < len(v)
    return int(v[len(v) - m - 1]) if op == ">" else int(v[m])


def _windows(m):
    """three row windows of a kept batch, the LAST rows first (a gather writes them last): [(row0, nrows)], row0 a multiple of 8"""
    w = max(min(4096, m // 4) // 8 * 8, 8)
    return [((m - w) // 8 * 8, m - (m - w) // 8 * 8), (m // 2 // 8 * 8, w), (0, w)]


def _read_windows(h):
    """tfgpu_dbatch_slice calls tf::dense and reads the columns; the whole 3 GiB batch is never brought to the host"""
    out = []
    for r0, k in _windows(h.nrows):
        sl = h.slice(r0, k)
        out.append(sl.download())
        sl.free()
    return out


def _want_windows(b, idx):
    return [_take(b, idx[r0: r0 + k]) for r0, k in _windows(len(idx))]


def _same_windows(got, want, ctx):
    assert len(got) == len(want), ctx
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, "%s, window %d of (last rows, middle, first rows)" % (ctx, j))


def _wide_case(tf, case, n):
    """Cases b, c and e where a missing wait cannot hide.  The table's gather is ONE gather_fixed_all launch over 149 columns that lasts milliseconds
    at full size; the readers are row windows (tfgpu_dbatch_slice) and, for c, a second filter_rows pushed through a Transformation, whose first
    device work follows tf::dense at once.  A REHEARSAL first runs the same calls on a selection of the same row count over OTHER rows
    (`i64 < c`, disjoint from the race's `i64 > c`): every lane's block cache then holds buffers of exactly the sizes the race asks for — no
    hipMalloc between a lane's look at the handle and its first read — and what those buffers hold is the answer for rows the race does not keep."""
    rng = np.random.default_rng(SEED0 + 7800 + ord(case))
    b, _schema = _table(rng, n, "wide")
    live = int(np.count_nonzero(b.kind != UPDATE))
    m = live * 2 // 5 // 8 * 8
    c_gt, c_lt = _const_for_count(b, m, ">"), _const_for_count(b, m, "<")
    idx = np.flatnonzero(_kept_mask(b, c_gt))
    assert len(idx) == m
    c2 = 12345
    idx2 = idx[b.col("i32").values[idx] > c2]
    second = tf.Transformation([tf.Transformer("filter_rows", {"filter": "i32 > %d" % c2})])

    def transform(h):   # c: a transformer that must gather, entering through tfgpu_transformation_push (tf::dense, then its own copy of the handle)
        out = second.push_run(h).transformed
        try:
            return [out.nrows] + _read_windows(out)
        finally:
            out.free()
    want = _want_windows(b, idx)
    want2 = [len(idx2)] + _want_windows(b, idx2)
    ctx = "%s: wide %d rows, %d kept" % (case, n, m)
    if case in ("b", "c"):
        tf.lane_use(1)
        src = tf.DeviceBatch.upload(b)
        on2 = transform if case == "c" else _read_windows
        h0 = [tf.apply_chain(_chain(tf, c_lt, "<"), src).transformed for _ in range(2)]   # the rehearsal's selections: the race's row count, other rows
        assert h0[0].nrows == m
        tf.lane_use(0)
        _run_threads([lambda: (tf.lane_use(1), _read_windows(h0[0]))])
        _run_threads([lambda: (tf.lane_use(2), on2(h0[1]))])
        for x in h0:
            x.free()
        tf.lane_use(1)
        tf.synchronize()
        h = tf.apply_chain(_chain(tf, c_gt), src).transformed
        tf.lane_use(0)
        g1, g2 = _racing_pair(tf, h, _read_windows, on2)
        _same_windows(g1, want, ctx + ": row windows on lane 1")
        if case == "c":
            assert g2[0] == want2[0], (ctx + ": rows a second filter_rows keeps, on lane 2", g2[0], want2[0])
            _same_windows(g2[1:], want2[1:], ctx + ": filter_rows on lane 2")
        else:
            _same_windows(g2, want, ctx + ": row windows on lane 2")
        _same_windows(_read_windows(h), want, ctx + ": the handle afterwards")
        return
    # e: only lane 0 exists while the gather is queued, behind a backlog of DECOYS gathers that outlasts the making of a lane
    src = tf.DeviceBatch.upload(b)
    h0 = [tf.apply_chain(_chain(tf, c_lt, "<"), src).transformed for _ in range(DECOYS + 1)]
    for x in h0:
        x.dense()
    tf.synchronize()
    for x in h0:
        x.free()
    c_dec = _const_for_count(b, m - 8, ">")
    decoys = [tf.apply_chain(_chain(tf, c_dec), src).transformed for _ in range(DECOYS)]   # (they stay alive: their buffers are nobody else's)
    h = tf.apply_chain(_chain(tf, c_gt), src).transformed
    go = threading.Event()
    got, errs = {}, []

    def late():
        try:
            _wait(go)
            t0 = time.perf_counter()
            tf.lane_use(1)   # the lane is made HERE, after the gather was queued
            got["bind_ms"] = (time.perf_counter() - t0) * 1e3
            got["windows"] = _read_windows(h)
        except BaseException as e:  # noqa: BLE001 (reported to the main thread)
            errs.append(repr(e))
    t = threading.Thread(target=late, daemon=True)
    t.start()
    t0 = time.perf_counter()
    for x in decoys:
        x.dense()
    h.dense()
    queued_ms = (time.perf_counter() - t0) * 1e3
    go.set()
    tf.synchronize()
    drained_ms = (time.perf_counter() - t0) * 1e3
    t.join(WAIT_S + 5)
    assert not t.is_alive(), "the late lane's thread did not finish"
    assert errs == [], errs
    print("e: %d gathers queued in %.2f ms, drained after %.2f ms; binding the new lane took %.2f ms" % (DECOYS + 1, queued_ms, drained_ms, got["bind_ms"]))
    _same_windows(got["windows"], want, ctx + ": row windows read from a lane bound after the gather was queued")


# ---- b-e, g: child processes ---------------------------------------------------------------------------------------------------------------
def _child(case, n, table, hold=True):
    """the case in a fresh Python process (a child: the knob is latched at first use, and cases e and g need a process without lanes)"""
    env = dict(os.environ)
    env.pop("TFGPU_DENSE_HOLD_MS", None)
    if hold:
        env["TFGPU_DENSE_HOLD_MS"] = str(HOLD_MS)
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), case, str(n), table]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_S, cwd=ROOT)
    assert r.returncode == 0, "child `%s %d %s` exit %s\n%s\n%s" % (case, n, table, r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    assert "child ok" in r.stdout, r.stdout[-3000:]


def _racing_pair(tf, h, first, second, delay_second=0.0):
    """two threads on lanes 1 and 2 call their reader on h from behind one barrier; -> [result of first, result of second]"""
    bar = threading.Barrier(2, timeout=WAIT_S)
    got = [None, None]

    def on_lane_1():
        tf.lane_use(1)
        bar.wait()
        got[0] = first(h)

    def on_lane_2():
        tf.lane_use(2)
        bar.wait()
        if delay_second:
            time.sleep(delay_second)
        got[1] = second(h)
    _run_threads([on_lane_1, on_lane_2])
    return got


def case_b(tf, oracle, n, table):
    """b. the loser of the race: both lanes have seen `pending` (the hold) before either gathers; whoever arrives second finds it gone"""
    if table == "wide":
        return _wide_case(tf, "b", n)
    small = n <= SMALL
    rng = np.random.default_rng(SEED0 + 7200)
    b, schema = _table(rng, n, table)
    tf.lane_use(1)
    src = tf.DeviceBatch.upload(b)
    tf.lane_use(0)
    pairs = [("download", "download")] + [(READERS[i], READERS[(i + 1) % len(READERS)]) for i in range(len(READERS))]
    prev = []
    for const, (r1, r2) in zip(_constants(b, len(pairs)), pairs):
        want = Want(tf, oracle, _expected(b, const), schema, n, (r1, r2), small)
        tf.lane_use(1)
        h = tf.apply_chain(_chain(tf, const), src).transformed
        tf.lane_use(0)
        g1, g2 = _racing_pair(tf, h, lambda x: _read(tf, r1, x, n), lambda x: _read(tf, r2, x, n))
        ctx = "b: %s %d rows, %s on lane 1 beside %s on lane 2" % (table, n, r1, r2)
        _same(g1, want.by[r1], ctx + ": lane 1")
        _same(g2, want.by[r2], ctx + ": lane 2")
        for x in prev:
            x.free()
        prev = [h]


def case_c(tf, oracle, n, table):
    """c. a transformer entering beside a reader: lane 2 applies a second filter_rows / convert_to_string to the handle lane 1 is reading.  Through
    tfgpu_apply the transformer works on its own copy of the handle, taken under the transition's lock (a selection: it gathers for itself; dense
    already: it waits for the gathering lane's event); through a Transformation's push it enters by tf::dense like any reader and can be the loser
    of case b.  (apply_plan itself never sees a handle somebody else can change.)"""
    if table == "wide":
        return _wide_case(tf, "c", n)
    small = n <= SMALL
    rng = np.random.default_rng(SEED0 + 7300)
    b, schema = _table(rng, n, table)
    tf.lane_use(1)
    src = tf.DeviceBatch.upload(b)
    tf.lane_use(0)
    c2 = 12345
    steps = [("push", "filter_rows"), ("apply", "filter_rows"), ("push", "convert_to_string"), ("apply", "convert_to_string")]
    prev = []
    for const, (route, kind) in zip(_constants(b, len(steps)), steps):
        exp = _expected(b, const)
        want = Want(tf, oracle, exp, schema, n, ("download",), small)
        cfg = {"filter": "i32 > %d" % c2} if kind == "filter_rows" else {}
        if kind == "filter_rows":
            want2 = _take(exp, np.flatnonzero(exp.col("i32").values > c2))   # (src_row: rows of the first filter's input, as the device counts them)
        else:  # the same transformer over the numpy rows uploaded dense on one lane, behind a synchronize; the oracle's at the small size
            d = tf.DeviceBatch.upload(exp)
            want2 = tf.apply_chain([tf.Transformer(kind, cfg)], d).transformed.download()
            tf.synchronize()
            d.free()
            if small:
                ref = oracle.apply_chain([oracle.Transformer(kind, cfg)], exp, schema)
                want2o = ref.batch
                want2o.kind, want2o.part_id = want2.kind, want2.part_id   # (the oracle's result carries neither)
                assert_batches_equal(want2, want2o, "c: dense %s against the oracle" % kind)
        tr = tf.Transformer(kind, cfg)
        tn = tf.Transformation([tr])

        def transform(x):
            out = tn.push_run(x).transformed if route == "push" else tf.apply_chain([tr], x).transformed
            return out.download()
        tf.lane_use(1)
        h = tf.apply_chain(_chain(tf, const), src).transformed
        tf.lane_use(0)
        g1, g2 = _racing_pair(tf, h, lambda x: x.download(), transform)
        ctx = "c: %s %d rows, download on lane 1 beside %s (%s) on lane 2" % (table, n, kind, route)
        _same(g1, want.by["download"], ctx + ": lane 1")
        _same(g2, want2, ctx + ": lane 2")
        _same(h.download(), want.by["download"], ctx + ": the handle afterwards")
        for x in prev:
            x.free()
        prev = [h]


def case_d(tf, oracle, n, table):
    """d. mask_field reads THROUGH the selection (its own copy of it) while another lane gathers the handle and resets `pending`: the serializer's
    lane enters first and holds, mask_field's lane takes its copy half a hold later and holds, the serializer gathers, mask_field hashes"""
    small = n <= SMALL
    rng = np.random.default_rng(SEED0 + 7400)
    b, schema = _table(rng, n, table)
    tf.lane_use(1)
    src = tf.DeviceBatch.upload(b)
    tf.lane_use(0)
    salt = "handover"
    masked = ["i32", "by"] if table == "mixed" else ["i32", "u8"]
    cfg = {"maskFunctionHash": {"userDefinedSalt": salt}, "columns": masked}
    prev = []
    for const, fmt in zip(_constants(b, 2), ("json", "csv")):
        exp = _expected(b, const)
        want = Want(tf, oracle, exp, schema, n, (fmt, "download"), small)
        wm = _take(exp, np.arange(exp.nrows))
        wm.src_row = exp.src_row
        for name in masked:
            c = exp.col(name)
            text = [c.get_bytes(i) for i in range(exp.nrows)] if c.repr in abi.VAR_REPRS else [b"%d" % int(v) for v in c.values]
            hexd = "".join(hmac.new(salt.encode(), t, hashlib.sha256).hexdigest() for t in text).encode()
            k = [x.name for x in wm.cols].index(name)
            wm.cols[k] = abi.Column(name, "utf8", abi.R_STRING, offsets=(np.arange(exp.nrows + 1, dtype=np.uint64) * 64).astype(np.uint32), data=np.frombuffer(hexd, np.uint8))
        mask = tf.Transformer("mask_field", cfg)
        tf.lane_use(1)
        h = tf.apply_chain(_chain(tf, const), src).transformed
        tf.lane_use(0)
        # the serializer (lane 1) is first in time: mask_field (lane 2) starts half a hold behind the barrier
        g_ser, g_mask = _racing_pair(tf, h, lambda x: _read(tf, fmt, x, n), lambda x: tf.apply_chain([mask], x).transformed.download(), delay_second=HOLD_MS / 2000.0)
        ctx = "d: %s %d rows, %s beside mask_field" % (table, n, fmt)
        _same(g_ser, want.by[fmt], ctx + ": the serializer")
        _same(g_mask, wm, ctx + ": mask_field through the selection")
        _same(h.download(), want.by["download"], ctx + ": the handle afterwards")
        for x in prev:
            x.free()
        prev = [h]


def case_e(tf, oracle, n, table):
    """e. a lane born after the gather was queued: only lane 0 exists while it gathers (behind a backlog of other gathers on its stream); at once
    a new thread binds lane 1 and reads the handle"""
    if table == "wide":
        return _wide_case(tf, "e", n)
    small = n <= SMALL
    rng = np.random.default_rng(SEED0 + 7500)
    b, schema = _table(rng, n, table)
    src = tf.DeviceBatch.upload(b)
    consts = _constants(b, 49)
    want = Want(tf, oracle, _expected(b, consts[0]), schema, n, ("download", "json"), small)
    h = tf.apply_chain(_chain(tf, consts[0]), src).transformed
    decoys = [tf.apply_chain(_chain(tf, c), src).transformed for c in consts[1:]]
    go = threading.Event()
    got, errs = {}, []

    def late():
        try:
            _wait(go)
            tf.lane_use(1)   # the lane is made HERE, after the gather was queued
            got["download"] = h.download()
            got["json"] = _read(tf, "json", h, n)
        except BaseException as e:  # noqa: BLE001 (reported to the main thread)
            errs.append(repr(e))
    t = threading.Thread(target=late, daemon=True)
    t.start()
    for x in decoys:
        x.dense()        # queued on lane 0's stream (tfgpu_dbatch_dense returns without a synchronize where no text length is read back)
    h.dense()
    go.set()
    t.join(WAIT_S + 5)
    assert not t.is_alive(), "the late lane's thread did not finish"
    assert errs == [], errs
    ctx = "e: %s %d rows, read from a lane bound after the gather was queued" % (table, n)
    _same(got["download"], want.by["download"], ctx)
    _same(got["json"], want.by["json"], ctx + " (json)")


def case_g(tf, oracle, n, table):
    """g. twenty init .. dense transition across two lanes .. shutdown rounds in one process: every round's results are the reference's and no
    call fails (a lane's event is made again after destroy_lane)"""
    rng = np.random.default_rng(SEED0 + 7600)
    b, schema = _table(rng, n, table)
    consts = _constants(b, 20)
    for k in range(20):
        tf.init()
        who = ("other", "maker")[k % 2]
        const = consts[k]
        want = Want(tf, oracle, _expected(b, const), schema, n, ("download", "csv"), n <= SMALL and k == 0)
        made, read = threading.Event(), threading.Event()
        box, got = {}, {}

        def maker():
            tf.lane_use(1)
            box["src"] = tf.DeviceBatch.upload(b)
            box["tr"] = _chain(tf, const)
            h = box["h"] = tf.apply_chain(box["tr"], box["src"]).transformed
            if who == "maker":
                got["maker"] = _read(tf, "csv", h, n)
            made.set()
            _wait(read)
            got["maker2"] = h.download()

        def other():
            tf.lane_use(2)
            _wait(made)
            try:
                got["other"] = _read(tf, "csv" if who == "other" else "download", box["h"], n)
            finally:
                read.set()
        _run_threads([maker, other])
        ctx = "g: round %d, %s %d rows, gathered by the %s lane" % (k, table, n, who)
        _same(got["maker2"], want.by["download"], ctx)
        _same(got["other"], want.by["csv" if who == "other" else "download"], ctx)
        if who == "maker":
            _same(got["maker"], want.by["csv"], ctx)
        box["h"].free(); box["src"].free(); want._dense.free()   # nothing of this round outlives its lanes
        box.clear(); got.clear()
        gc.collect()
        tf.shutdown()


CHILD_CASES = {"b": case_b, "c": case_c, "d": case_d, "e": case_e, "g": case_g}


@pytest.mark.parametrize("table", RACE_TABLES)
def test_loser_of_the_race(table):
    _child("b", SMALL, table)


@pytest.mark.parametrize("table", RACE_TABLES)
def test_loser_of_the_race_fullsize(table):
    _child("b", FULL[table], table)


@pytest.mark.parametrize("table", RACE_TABLES)
def test_transformer_beside_a_reader(table):
    _child("c", SMALL, table)


@pytest.mark.parametrize("table", RACE_TABLES)
def test_transformer_beside_a_reader_fullsize(table):
    _child("c", FULL[table], table)


@pytest.mark.parametrize("table", TABLES)
def test_mask_field_through_the_selection_while_another_lane_gathers(table):
    _child("d", SMALL, table)


@pytest.mark.parametrize("table", TABLES)
def test_mask_field_through_the_selection_while_another_lane_gathers_fullsize(table):
    _child("d", FULL[table] // 4, table)   # (Python's hmac over the kept rows is the slow part: a quarter of the rows)


@pytest.mark.parametrize("table", RACE_TABLES)
def test_lane_born_after_the_gather(table):
    _child("e", SMALL, table, hold=False)


@pytest.mark.parametrize("table", RACE_TABLES)
def test_lane_born_after_the_gather_fullsize(table):
    _child("e", FULL[table], table, hold=False)


def test_init_shutdown_cycles():
    _child("g", SMALL, "mixed", hold=False)


def test_init_shutdown_cycles_fullsize():   # (twenty uploads and references: an eighth of the fixed table's rows; the fixed table, whose gather stays queued)
    _child("g", FULL["fixed"] // 8, "fixed", hold=False)


# ---- f. the Bufferer at size ---------------------------------------------------------------------------------------------------------------
FLUSH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_uint64)


def _bufferer_at_size(tf, oracle, n, table):
    """the shape of tests/test_pipeline.py::test_bufferer_merged_src_row_lines_up_with_the_parts_sources with two filtered batches of n rows:
    the collector's thread concatenates the pushed handles (still selections) while the pushing thread serializes them on its lane"""
    L = tf.load()
    small = n <= SMALL
    rng = np.random.default_rng(SEED0 + 7700)
    merged_got, errs = [], []

    def flush(user, merged, parts, nparts, nrows, size):
        try:
            view = tf.DeviceBatch(C.c_void_p(merged))
            merged_got.append((nparts, view.download()))
            view._h = None
        except BaseException as e:  # noqa: BLE001 (reported to the main thread)
            errs.append(repr(e))
            return 1
        return 0
    cb = FLUSH(flush)
    L.tfgpu_bufferer_create.argtypes = [C.c_int64, C.c_uint64, C.c_int64, C.c_int, FLUSH, C.c_void_p, C.POINTER(C.c_void_p)]
    L.tfgpu_bufferer_async_push_meta.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int64, C.POINTER(C.c_uint64)]
    L.tfgpu_bufferer_wait.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L.tfgpu_bufferer_close.argtypes = [C.c_void_p]
    L.tfgpu_bufferer_destroy.argtypes = [C.c_void_p]
    tf.lane_use(1)
    try:
        parts, wants, held, tickets, bytes_got = [], [], [], [], []
        for k in range(2):
            b, schema = _table(rng, n, table)
            const = _constants(b, 3)[k]
            tf.lane_use(0)
            wants.append(Want(tf, oracle, _expected(b, const), schema, n, ("json", "download"), small))
            tf.lane_use(1)
            src = tf.DeviceBatch.upload(b)
            parts.append(tf.apply_chain(_chain(tf, const), src).transformed)
            held.append(src)
        total = sum(w.exp.nrows for w in wants)
        h = C.c_void_p()
        assert L.tfgpu_bufferer_create(total, 0, 0, 1, cb, None, C.byref(h)) == 0
        for k in range(2):
            t = C.c_uint64(0)
            assert L.tfgpu_bufferer_async_push_meta(h, parts[k]._h, parts[k].nrows, 64, 0, n, C.byref(t)) == 0
            tickets.append(t.value)
            bytes_got.append(_read(tf, "json", parts[k], n))   # the pusher reads its handle while the collector may be merging it
        L.tfgpu_bufferer_close(h)
        assert [L.tfgpu_bufferer_wait(h, t, WAIT_S * 1000) for t in tickets] == [0, 0], errs
        L.tfgpu_bufferer_destroy(h)
        assert errs == []
        ctx = "f: %s, two batches of %d rows" % (table, n)
        for k in range(2):
            _same(bytes_got[k], wants[k].by["json"], "%s: part %d serialized on the pusher's lane" % (ctx, k))
            _same(parts[k].download(), wants[k].by["download"], "%s: part %d afterwards" % (ctx, k))
        assert [np_ for np_, _ in merged_got] == [2], merged_got and [x[0] for x in merged_got]
        m0 = wants[0].exp.nrows
        both = merged_got[0][1]
        assert both.nrows == total
        _same(_take(both, np.arange(m0)), _with_src(wants[0].exp, both.src_row[:m0], 0), ctx + ": merged, part 0")
        _same(_take(both, np.arange(m0, total)), _with_src(wants[1].exp, both.src_row[m0:], n), ctx + ": merged, part 1")
        for x in held + parts:
            x.free()
    finally:
        tf.lane_use(0)
        tf.synchronize()


def _with_src(exp, got_src, shift):
    """exp as _take() of the merged download shows it: _take keeps the merged batch's src_row, which must be exp's shifted by the source rows of
    the parts in front"""
    assert np.array_equal(got_src, exp.src_row + shift), ("merged src_row", _rows_diff(got_src, exp.src_row + shift))
    w = _take(exp, np.arange(exp.nrows))
    w.src_row = (exp.src_row + shift).astype(np.int32)
    return w


@pytest.mark.parametrize("table", TABLES)
def test_bufferer_at_size(tf, oracle, table):
    _bufferer_at_size(tf, oracle, SMALL, table)


@pytest.mark.parametrize("table", TABLES)
def test_bufferer_at_size_fullsize(tf, oracle, table):
    _bufferer_at_size(tf, oracle, 1 << 18, table)


if __name__ == "__main__":
    from transferia_amd import lib as _lib
    if os.environ.get("TFGPU_TEST_EMU_LIB"):  # the CPU pre-flight's build of the kernels, as tests/conftest.py binds it for a pytest child
        _lib._LIBPATH = os.environ["TFGPU_TEST_EMU_LIB"]
    from oracle import oracle as _ora
    _ora.build()
    _lib.init()
    try:
        CHILD_CASES[sys.argv[1]](_lib, _ora, int(sys.argv[2]), sys.argv[3])
    finally:
        sys.stdout.flush()
    print("child ok")
