#!/usr/bin/env python3
"""Stand-alone measurement of table_splitter_transformer on the GPU: 2^20 `hits` rows, resident in HBM, split --steps times after --warmup calls
by (`eventdate`), (`eventdate`, `regionid`) and (`userid`) — with the generated table: 31 tables, a quarter of a million, and as many tables as rows.  One process.  Prints one JSON line:
per key set the number of tables, ms per pass and rows/s without and with materialising every per-table batch (host clock around calls that end in
a device synchronise; the batches are materialised only up to --max-batches tables: one gather and one synchronise per table is the caller's
loop, not the split), and per-kernel ms (HIP events on the library's stream, tfgpu_prof_*).  Beside it, as the nearest existing work and not as a
threshold: sharder_transformer over the same columns followed by tfgpu_partition(8).  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench.common import HBM_PEAK_GBS  # noqa: E402
from transferia_amd import lib, workload  # noqa: E402

KEYS = [("eventdate", ["eventdate"]), ("eventdate_regionid", ["eventdate", "regionid"]), ("userid", ["userid"])]


def hits_batch(rows: int, piece: int = 1 << 18) -> "lib.DeviceBatch":
    parts = []
    for row0 in range(0, rows, piece):
        n = min(piece, rows - row0)
        buf = lib.DeviceBuffer.upload(workload.hits_csv(n, row0=row0, header=False))
        db, _, errs = lib.csv_parse(workload.hits_csv_options(header=False), workload.hits_schema(), buf)
        assert not errs and db.nrows == n
        parts.append(db.dense())
        buf.free()
    out = lib.DeviceBatch.concat(parts) if len(parts) > 1 else parts[0]
    for p in parts:
        if p is not out:
            p.free()
    return out


def profiled(fn, steps, warmup, prefixes):
    for _ in range(warmup):
        fn()
    lib.synchronize()
    lib.prof_reset()
    lib.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    lib.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / steps
    lib.prof_enable(False)
    kms = {k: round(ms / steps, 4) for k, n, ms in lib.prof_get() if any(k.startswith(p) for p in prefixes)}
    return wall_ms, kms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batches", type=int, default=4096)
    a = ap.parse_args()
    lib.init(0)
    db = hits_batch(a.rows)
    widths = {c.name: c for c in db.download().cols if c.name in ("eventdate", "regionid", "userid")}
    res = {"workload": "table_splitter_transformer", "rows": a.rows, "columns_in_batch": len(db.column_names()), "steps": a.steps, "warmup": a.warmup,
           "hbm_peak_gbs": HBM_PEAK_GBS, "keys": {}}
    for name, cols in KEYS:
        plan = lib.Transformer("table_splitter_transformer", {"columns": cols, "splitter": "/"})
        state = {}

        def split_only():
            ts = lib.table_split(plan, db)
            state["tables"] = ts.count
            ts.free()

        def split_and_batches():
            ts = lib.table_split(plan, db)
            for t in range(ts.count):
                ts.batch(t).free()
            ts.free()

        wall, kms = profiled(split_only, a.steps, a.warmup, ["tsplit_"])
        key_bytes = sum(int(widths[c].values.itemsize if widths[c].values is not None else 0) * a.rows + (int(widths[c].offsets[-1]) + 4 * a.rows if widths[c].offsets is not None else 0)
                        for c in cols)
        entry = {"columns": cols, "tables": state["tables"], "split_ms_host_clock": round(wall, 4), "split_rows_per_s": round(a.rows / (wall * 1e-3)), "kernel_ms": kms,
                 "key_column_bytes": key_bytes,
                 "hash_fraction_of_hbm_peak": round((key_bytes + 16 * a.rows) / (kms["tsplit_hash"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 5) if kms.get("tsplit_hash") else None,
                 "intern_ns_per_row": round(kms["tsplit_intern"] * 1e6 / a.rows, 3) if kms.get("tsplit_intern") else None}
        if state["tables"] <= a.max_batches:
            wall2, kms2 = profiled(split_and_batches, max(1, a.steps // 2), 1, ["tsplit_", "compact_gather"])
            entry.update({"with_batches_ms_host_clock": round(wall2, 4), "with_batches_rows_per_s": round(a.rows / (wall2 * 1e-3)), "with_batches_kernel_ms": kms2})
        else:
            entry["with_batches_ms_host_clock"] = None  # one gather + one synchronise per table, about n of them: the caller's loop, not measured
        # the nearest existing work: CRC32 of the same columns' strings, then 8 parts (one pass and one host sync per part)
        shard = lib.Transformer("sharder_transformer", {"shardsCount": "8", "columns": {"includeColumns": ["^%s$" % c for c in cols]}})

        def shard_and_partition():
            out = shard.apply(db).transformed
            parts, _counts = lib.partition(out, 8)
            parts.free(); out.free()

        wall3, kms3 = profiled(shard_and_partition, max(1, a.steps // 2), 1, ["sharder_", "partition_", "compact_gather"])
        entry["sharder_partition8"] = {"ms_host_clock": round(wall3, 4), "rows_per_s": round(a.rows / (wall3 * 1e-3)), "kernel_ms": kms3}
        res["keys"][name] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
