"""A hits-shaped Parquet object for the configs[3] tests (TEST INFRASTRUCTURE, not product code).

`write(batch, ...)` takes the rows of workload.hits_csv as parsed columns (the oracle's parse, or a device batch's download())
and writes them with pyarrow, typed the way a real writer types hits:

  int16 → INT32 + INT(16, true)      int32 → INT32      int64 → INT64      utf8 → BYTE_ARRAY + STRING
  timestamp → INT64 + TIMESTAMP(MICROS, UTC) = seconds × 10^6 (+ the sub-second micros below)      date → INT32 + DATE

`hitcolor` is `any` in the hits schema.  The device reads a BYTE_ARRAY under `any` as []byte (Restore's `any` branch hands a
non-string value back as it is), so the configs[3] tests read the object under SCHEMA, where `hitcolor` is `utf8`: every column
then has one reading that the device, the oracle and the CSV parse share.  test_gpu_configs3 pins the `any` reading on its own.

Knobs: codec (NONE / SNAPPY / ZSTD / LZ4_RAW), dictionary on or off, dictionary_pagesize_limit (a small one makes a chunk fall back
from dictionary to PLAIN partway), data_page_size, row_group_size, data_page_version, nulls=p (cells of NULL_COLUMNS made null at
rate p) and subsecond (per-row micros added to the timestamps).  `write` returns the object and the batch it holds: the input with
those nulls and micros applied, which is what a read of the object must give back."""
from __future__ import annotations

import dataclasses
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from transferia_amd import abi, workload

# every column the configs[3] chain reads, one timestamp, the date and two text columns
NULL_COLUMNS = ("clientip", "userid", "regionid", "counterid", "ipnetworkid", "eventtime", "eventdate", "title", "url")

_ARROW = {"int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64(), "utf8": pa.string(), "timestamp": pa.timestamp("us", tz="UTC"), "date": pa.date32()}
_CODEC = {"NONE": "NONE", "SNAPPY": "SNAPPY", "ZSTD": "ZSTD", "LZ4_RAW": "LZ4"}  # (pyarrow's "LZ4" writes the LZ4_RAW codec)


def schema() -> abi.Schema:
    """the hits schema with `hitcolor` typed utf8 (see the module's docstring)"""
    return abi.Schema([dataclasses.replace(c, dtype="utf8") if c.name == "hitcolor" else c for c in workload.hits_schema().cols])


SCHEMA = schema()


def _valid(c: abi.Column, n: int) -> np.ndarray:
    return np.ones(n, bool) if c.validity is None else np.asarray(c.validity, bool)


def _apply(b: abi.Batch, nulls: float, subsecond: bool, seed: int) -> abi.Batch:
    """the batch with NULL_COLUMNS' cells made null at rate `nulls` and micros added to every timestamp (nanos = micros × 1000)"""
    rng = np.random.default_rng(seed)
    n = b.nrows
    cols = []
    for c in b.cols:
        valid = c.validity
        if nulls and c.name in NULL_COLUMNS:
            valid = _valid(c, n) & (rng.random(n) >= nulls)
        nanos = c.nanos
        if subsecond and c.dtype == "timestamp":
            nanos = (rng.integers(0, 10**6, n) * 1000).astype(np.int32)
        if c.repr in abi.VAR_REPRS and valid is not None and not valid.all():
            # a null text cell holds no bytes (what every reader gives back for it)
            lens = np.diff(np.asarray(c.offsets, np.int64))
            keep = np.repeat(valid, lens)
            off = np.zeros(n + 1, np.uint32)
            np.cumsum(np.where(valid, lens, 0), out=off[1:])
            cols.append(dataclasses.replace(c, offsets=off, data=np.asarray(c.data[: int(c.offsets[-1])])[keep], validity=valid))
        elif c.repr not in abi.VAR_REPRS and valid is not None:
            vals = np.where(valid, c.values, 0).astype(c.values.dtype)
            cols.append(dataclasses.replace(c, values=vals, nanos=None if nanos is None else np.where(valid, nanos, 0).astype(np.int32), validity=valid))
        else:
            cols.append(dataclasses.replace(c, nanos=nanos))
    return abi.Batch(cols, n, b.table_ns, b.table_name)


def _arrow(c: abi.Column, n: int, dtype: str) -> pa.Array:
    valid = _valid(c, n)
    vbuf = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    nulls = int(n - valid.sum())
    if dtype == "utf8":
        assert c.repr in abi.VAR_REPRS, c.name
        off = np.asarray(c.offsets, np.int32)
        return pa.Array.from_buffers(pa.string(), n, [vbuf, pa.py_buffer(off.tobytes()), pa.py_buffer(bytes(np.asarray(c.data[: int(off[-1])])))], null_count=nulls)
    if dtype == "timestamp":
        assert c.repr == abi.R_TIME, c.name
        ns = np.zeros(n, np.int64) if c.nanos is None else np.asarray(c.nanos, np.int64)
        us = np.asarray(c.values, np.int64) * 10**6 + ns // 1000
        return pa.Array.from_buffers(_ARROW[dtype], n, [vbuf, pa.py_buffer(us.tobytes())], null_count=nulls)
    if dtype == "date":
        assert c.repr == abi.R_TIME and (c.nanos is None or not np.asarray(c.nanos)[valid].any()), c.name
        days = (np.asarray(c.values, np.int64) // 86400).astype(np.int32)
        return pa.Array.from_buffers(_ARROW[dtype], n, [vbuf, pa.py_buffer(days.tobytes())], null_count=nulls)
    want = np.dtype({"int16": np.int16, "int32": np.int32, "int64": np.int64}[dtype])
    return pa.Array.from_buffers(_ARROW[dtype], n, [vbuf, pa.py_buffer(np.ascontiguousarray(np.asarray(c.values).astype(want)).tobytes())], null_count=nulls)


def write(b: abi.Batch, codec: str = "SNAPPY", dictionary: bool = True, dictionary_pagesize_limit: int | None = None, data_page_size: int | None = None,
          row_group_size: int | None = None, data_page_version: str = "1.0", nulls: float = 0.0, subsecond: bool = False, seed: int = 3):
    """(the Parquet object, the batch it holds) for the hits rows of `b` (columns named and typed as SCHEMA)"""
    held = _apply(b, nulls, subsecond, seed)
    dt = {c.name: c.dtype for c in SCHEMA.cols}
    n = held.nrows
    tab = pa.table([_arrow(c, n, dt[c.name]) for c in held.cols], names=[c.name for c in held.cols])
    kw = dict(compression=_CODEC[codec], use_dictionary=dictionary, data_page_version=data_page_version, row_group_size=row_group_size or max(n, 1))
    if dictionary_pagesize_limit is not None:
        kw["dictionary_pagesize_limit"] = dictionary_pagesize_limit
    if data_page_size is not None:
        kw["data_page_size"] = data_page_size
    buf = io.BytesIO()
    pq.write_table(tab, buf, **kw)
    return buf.getvalue(), held


# the writer shapes test 2a reads: every knob at least once
SHAPES = {
    "none_dict": dict(codec="NONE"),
    "snappy_dict_plain_fallback": dict(codec="SNAPPY", dictionary_pagesize_limit=4096),
    "zstd_plain": dict(codec="ZSTD", dictionary=False),
    "lz4raw_small_pages": dict(codec="LZ4_RAW", data_page_size=2048),
    "snappy_row_groups": dict(codec="SNAPPY", row_group_size=3001),
    "zstd_v2_pages": dict(codec="ZSTD", data_page_version="2.0", dictionary_pagesize_limit=8192),
    "snappy_nulls_subsecond": dict(codec="SNAPPY", nulls=0.05, subsecond=True, row_group_size=2999),
}
