#!/usr/bin/env python3
"""Stand-alone measurement of filter_rows_by_ids on the GPU: the `url` column of 2^20 `hits` rows, resident in HBM, filtered --steps times after
--warmup calls with 1, 64 and 65 536 allowed IDs, of one length (16 bytes) and of four (8, 12, 16 and 24).  The IDs are prefixes of the column's own
cells, topped up with IDs no cell starts with, so every table lets some rows through.  One process.  Prints one JSON line: per config the kernel's ms
(HIP events on the library's stream, tfgpu_prof_*), ms per call by the host clock (the call ends in a device synchronise and includes the
compaction of the keep flags), the rows kept, which kernel ran (by the library's own timer name: the table in LDS, or probed where it lies), the bytes the kernel moves — per row two offsets'
worth (4 bytes amortised), at most max_len cell bytes (fewer where the cell or the next allowed length is shorter: counted as the walk reads them)
and the 4-byte keep flag — and those bytes over the kernel's time as a fraction of the HBM peak bench/common.py uses.  filter_rows' kernel for one
string-equality term on the same column is taken in the same process, as the yardstick: an existing kernel on the same data.  No hardware counters
are collected here.  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench.common import HBM_PEAK_GBS  # noqa: E402
from regex_bench import url_column  # noqa: E402
from transferia_amd import lib  # noqa: E402

KERNELS = {"filter_rows_by_ids_lds": "lds", "filter_rows_by_ids_hbm": "hbm"}   # the library's timer names: which kernel ran is the library's to say
COUNTS = [1, 64, 65536]
LENGTHS = {"one_length": [16], "four_lengths": [8, 12, 16, 24]}


def allowed_ids(cells, count, lengths, rng):
    """`count` distinct ASCII IDs over `lengths`: prefixes of random cells first, then IDs no cell starts with"""
    ids, tries = set(), 0
    while len(ids) < count and tries < 4 * count:
        tries += 1
        c, L = cells[int(rng.integers(0, len(cells)))], lengths[tries % len(lengths)]
        if len(c) >= L and all(0x20 <= x < 0x7F and x not in (0x22, 0x5C) for x in c[:L]):
            ids.add(bytes(c[:L]).decode("ascii"))
    k = 0
    while len(ids) < count:
        L = lengths[k % len(lengths)]
        ids.add(("~id%0" + str(L - 3) + "d") % k)
        k += 1
    return sorted(ids)


def bytes_walked(lens, allowed_lengths):
    """the cell bytes the hash walk reads: up to the largest allowed length that is not longer than the cell"""
    al = np.array(sorted(allowed_lengths), np.int64)
    idx = np.searchsorted(al, lens, side="right")
    return int(np.where(idx > 0, al[np.maximum(idx - 1, 0)], 0).sum())


def timed(plan, db, steps, warmup, kernels):
    """-> (ms per call by the host clock, the one of `kernels` that ran, its ms per launch, rows kept)"""
    for _ in range(warmup):
        out = plan.apply(db).transformed
    kept = out.nrows
    lib.synchronize()
    lib.prof_reset()
    lib.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.apply(db).transformed.free()
    lib.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / steps
    lib.prof_enable(False)
    ran = [(k, ms / max(n, 1)) for k, n, ms in lib.prof_get() if k in kernels and n]
    assert len(ran) == 1, ran
    return wall_ms, ran[0][0], ran[0][1], kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib.init(0)
    b = url_column(a.rows)
    col = b.cols[0]
    db = lib.DeviceBatch.upload(b)
    lens = np.diff(col.offsets.astype(np.int64))
    rng = np.random.default_rng(7)
    sample = [col.get_bytes(int(i)) for i in rng.integers(0, a.rows, 1 << 17)]
    res = {"workload": "filter_rows_by_ids", "rows": a.rows, "column": "url", "bytes_in_column": int(col.offsets[-1]), "steps": a.steps, "warmup": a.warmup,
           "hbm_peak_gbs": HBM_PEAK_GBS, "configs": {}}
    for shape, lengths in LENGTHS.items():
        for count in COUNTS:
            ids = allowed_ids(sample, count, lengths, rng)
            plan = lib.Transformer("filter_rows_by_ids", {"columns": {"includeColumns": ["^url$"]}, "allowedIDs": ids})
            wall, name, k, kept = timed(plan, db, a.steps, a.warmup, KERNELS)
            moved = bytes_walked(lens, {len(i) for i in ids}) + 4 * (a.rows + 1) + 4 * a.rows
            res["configs"]["%s_%d_ids" % (shape, count)] = {
                "ids": count, "lengths": sorted({len(i) for i in ids}), "id_bytes": sum(len(i) for i in ids), "kernel": name, "table_in": KERNELS[name],
                "rows_kept": kept, "kernel_ms": round(k, 4) if k else None, "ms_per_call_host_clock": round(wall, 4), "bytes_moved": moved,
                "fraction_of_hbm_peak": round(moved / (k * 1e-3) / (HBM_PEAK_GBS * 1e9), 5) if k else None}
    # the yardstick: filter_rows, one string-equality term on the same column
    target = next(c for c in sample if c).decode("utf-8", "replace").replace("'", "").replace("\\", "")
    flt = lib.Transformer("filter_rows", {"filter": "url = '%s'" % target})
    wall, _name, k, kept = timed(flt, db, a.steps, a.warmup, ["filter_rows_eval"])
    res["filter_rows_string_equality"] = {"kernel": "filter_rows_eval", "rows_kept": kept, "kernel_ms": round(k, 4) if k else None, "ms_per_call_host_clock": round(wall, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
