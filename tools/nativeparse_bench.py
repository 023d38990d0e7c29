#!/usr/bin/env python3
"""Stand-alone measurement of the native parser on the GPU.  --rows `hits` rows (2^20; 105 columns), taken --chunk-rows at a time (a ChangeItem carries
its whole table_schema, about 15 KB for this table: 2^16 items are about a GiB of JSON and the ABI's offsets hold 4 GiB), are serialized by
tfgpu_queue_serialize (TFGPU_QFMT_NATIVE) into three message shapes — batching off (an item a message), 64 items a message, messages of about 1 MiB —
and each shape is parsed back by tfgpu_native_parse, everything resident in HBM.  One process.  Prints one JSON line: per shape the messages and
bytes, the serializer pass that produced them, ms per parse and items/s (host clock around calls that end in a device synchronise), per-kernel ms
(HIP events on the library's stream, tfgpu_prof_*), the cut's bytes per second (both of its runs together read the values twice) and its share of the
HBM peak and of the pass.  Beside it, as the comparison that matters — the same rows in the other wire form — tfgpu_debezium_emit's envelopes of the
same rows through the Debezium parser.  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench.common import HBM_PEAK_GBS  # noqa: E402
from transferia_amd import abi, lib, workload  # noqa: E402

SHAPES = [("batching_off", {}), ("items_64", {"enabled": True, "max_change_items": 64}), ("about_1MiB", {"enabled": True, "max_message_size": 1 << 20})]
PG = {"int16": "pg:smallint", "int32": "pg:integer", "int64": "pg:bigint", "utf8": "pg:text", "timestamp": "pg:timestamp without time zone", "date": "pg:date", "any": "pg:json"}


def hits_chunk(n, row0):
    buf = lib.DeviceBuffer.upload(workload.hits_csv(n, row0=row0, header=False))
    db, _, errs = lib.csv_parse(workload.hits_csv_options(header=False), workload.hits_schema(), buf)
    assert not errs and db.nrows == n
    db.dense()
    buf.free()
    return db


def device_messages(values: "lib.DeviceBuffer", starts: np.ndarray):
    """a tfgpu_message_batch over message values that are already in HBM"""
    b = abi.CMessageBatch()
    st = lib.DeviceBuffer.upload(np.ascontiguousarray(starts, np.uint64).tobytes())
    b.topic, b.partition, b.mem, b.nmsg = b"bench", 0, abi.MEM_DEVICE, len(starts) - 1
    b.values, b.values_len, b.value_start = values.ptr, int(starts[-1]), st.ptr
    b._keep = (st, values)
    return b


def timed(fn):
    lib.synchronize()
    t0 = time.perf_counter()
    out = fn()
    lib.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--chunk-rows", type=int, default=1 << 16)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    lib.init(0)
    schema = workload.hits_schema()
    pg_schema = abi.Schema([abi.ColSchema(c.name, c.dtype, c.key, "", PG.get(c.dtype, "")) for c in schema.cols])
    res = {"workload": "native parser: hits rows written by the NATIVE queue serializer, parsed back", "rows": a.rows, "chunk_rows": a.chunk_rows, "columns": len(schema.cols),
           "hbm_peak_gbs": HBM_PEAK_GBS, "shapes": {}}
    acc = {name: {"messages": 0, "bytes": 0, "items": 0, "groups": 0, "fallback_messages": 0, "serialize_ms": 0.0, "parse_ms": 0.0, "kernel_ms": {}} for name, _ in SHAPES}
    dbz = {"messages": 0, "bytes": 0, "rows": 0, "emit_ms": 0.0, "parse_ms": 0.0, "kernel_ms": {}}
    from transferia_amd import debezium
    dparser = debezium.Parser(lib)
    for row0 in range(0, a.rows, a.chunk_rows):
        n = min(a.chunk_rows, a.rows - row0)
        print("rows %d .. %d" % (row0, row0 + n), file=sys.stderr, flush=True)
        db = hits_chunk(n, row0)
        meta = abi.row_meta(n, ids=np.arange(n) % 97, lsns=np.arange(n, dtype=np.uint64) + 5, commit_times=np.full(n, 1700000000000000000, np.uint64))
        for name, kw in SHAPES:
            s = acc[name]
            o = abi.queue_options(abi.QFMT_NATIVE, table_schema=pg_schema, **kw)   # (with the OriginalTypes a Postgres source states: the `any` column is pg:json)
            for _ in range(a.warmup if row0 == 0 else 0):
                lib.queue_serialize(o, db, meta).values.free()
            q, ms = timed(lambda: lib.queue_serialize(o, db, meta))
            s["serialize_ms"] += ms
            mb = device_messages(q.values, q.msg_start)
            for _ in range(a.warmup if row0 == 0 else 0):
                lib.native_parse(mb).free()
            lib.prof_reset()
            lib.prof_enable(True)
            p, ms = timed(lambda: lib.native_parse(mb))
            lib.prof_enable(False)
            s["parse_ms"] += ms
            for k, _n, kms in lib.prof_get():
                if k.startswith(("natp_", "scan_")):
                    s["kernel_ms"][k] = s["kernel_ms"].get(k, 0.0) + kms
            ni, ng, nf = p.info()
            s["messages"] += len(q); s["bytes"] += int(q.msg_start[-1]); s["items"] += ni; s["groups"] = max(s["groups"], ng); s["fallback_messages"] += nf
            if nf and "first_fallback" not in s:
                s["first_fallback"] = list(p.fallback()[0])
            p.free()
            q.values.free()
        # the same rows as Debezium envelopes
        try:
            dopts = abi.dbz_emit_options({"database.dbname": "db", "topic.prefix": "srv", "dt.source.type": "pg"}, pg_schema)
            em, ms = timed(lambda: lib.debezium_emit(dopts, db, meta))
            dbz["emit_ms"] += ms
            keep = np.flatnonzero(em.val_null == 0)
            starts = np.asarray(em.val_start, np.uint64)
            msgs = abi.CMessages()
            msgs.nmsg, msgs.start = len(em), starts.ctypes.data
            for _ in range(a.warmup if row0 == 0 else 0):
                for pb in dparser.parse(em.values, msgs)[0]:
                    pb.batch.free()
            lib.prof_reset()
            lib.prof_enable(True)
            (parsed, errors), ms = timed(lambda: dparser.parse(em.values, msgs))
            lib.prof_enable(False)
            dbz["parse_ms"] += ms
            for k, _n, kms in lib.prof_get():
                if k.startswith(("dbz_", "scan_")):
                    dbz["kernel_ms"][k] = dbz["kernel_ms"].get(k, 0.0) + kms
            dbz["messages"] += len(keep); dbz["bytes"] += int(starts[-1]); dbz["rows"] += sum(pb.batch.nrows for pb in parsed)
            dbz["errors"] = dbz.get("errors", 0) + len(errors)
            for pb in parsed:
                pb.batch.free()
            em.values.free(); em.keys.free()
        except lib.TfgpuError as e:   # the comparison is recorded as refused, by its own words
            dbz["refused"] = str(e)[:300]
        db.free()
    for name, _ in SHAPES:
        s = acc[name]
        cut = s["kernel_ms"].get("natp_cut_count", 0.0) + s["kernel_ms"].get("natp_cut_write", 0.0)
        s["kernel_ms"] = {k: round(v, 4) for k, v in s["kernel_ms"].items()}
        s["kernels_ms"] = round(sum(s["kernel_ms"].values()), 4)
        s["items_per_s"] = round(s["items"] / (s["parse_ms"] * 1e-3)) if s["parse_ms"] else None
        s["parse_gbs"] = round(s["bytes"] / (s["parse_ms"] * 1e-3) / 1e9, 3) if s["parse_ms"] else None
        if cut:
            s["cut_ms"] = round(cut, 4)
            s["cut_gbs"] = round(2 * s["bytes"] / (cut * 1e-3) / 1e9, 3)
            s["cut_fraction_of_hbm_peak"] = round(2 * s["bytes"] / (cut * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)
            s["cut_share_of_kernel_time"] = round(cut / s["kernels_ms"], 4)
            s["cut_share_of_parse_ms"] = round(cut / s["parse_ms"], 4)
        s["serialize_ms"], s["parse_ms"] = round(s["serialize_ms"], 3), round(s["parse_ms"], 3)
        res["shapes"][name] = s
    dbz["kernel_ms"] = {k: round(v, 4) for k, v in dbz["kernel_ms"].items()}
    if dbz["parse_ms"]:
        dbz["rows_per_s"] = round(dbz["rows"] / (dbz["parse_ms"] * 1e-3))
        dbz["parse_gbs"] = round(dbz["bytes"] / (dbz["parse_ms"] * 1e-3) / 1e9, 3)
    dbz["emit_ms"], dbz["parse_ms"] = round(dbz["emit_ms"], 3), round(dbz["parse_ms"], 3)
    res["debezium_parse_same_rows"] = dbz
    print(json.dumps(res))


if __name__ == "__main__":
    main()
