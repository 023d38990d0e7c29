#!/usr/bin/env python3
"""Stand-alone measurement of regex_replace_transformer on the GPU: the `url` column of 2^20 `hits` rows, resident in HBM, rewritten
--steps times after --warmup calls by three rules — `[_@#&]` -> `-` (few matches), `\\d+` -> `NUM` (many) and the captures rule
`.*?/app/(\\d+).*` -> `$1`.  One process.  Prints one JSON line: per rule ms per pass (host clock around calls that end in a device
synchronise), per-kernel ms (HIP events on the library's stream, tfgpu_prof_*), bytes read (the cell bytes once per pass that ran: the write pass runs only
when something matched) and written, and those bytes over the two kernels' time as a fraction of the HBM peak bench/common.py uses.  mask_field and
convert_to_string over the same column are taken in the same process, as yardsticks.  No hardware counters are collected here (VALU
instructions per input byte need a rocprofv3 --pmc run of their own).  GPU only; it reads nothing outside the repository."""
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

RULES = [("few_matches", "[_@#&]", "-"), ("many_matches", "\\d+", "NUM"), ("captures", ".*?/app/(\\d+).*", "$1")]


def url_column(rows: int, piece: int = 1 << 18) -> abi.Batch:
    offs, datas, base = [np.zeros(1, np.uint32)], [], 0
    for row0 in range(0, rows, piece):
        n = min(piece, rows - row0)
        buf = lib.DeviceBuffer.upload(workload.hits_csv(n, row0=row0, header=False))
        db, _, errs = lib.csv_parse(workload.hits_csv_options(header=False), workload.hits_schema(), buf)
        assert not errs and db.nrows == n
        c = db.download().col("url")
        total = int(c.offsets[-1])
        offs.append(c.offsets[1:].astype(np.uint32) + np.uint32(base))
        datas.append(np.asarray(c.data[:total]))
        base += total
        db.free(); buf.free()
    col = abi.Column("url", "utf8", abi.R_STRING, offsets=np.concatenate(offs), data=np.concatenate(datas))
    return abi.Batch([col], rows, "", "hits")


def timed(plan, db, steps, warmup, kernels):
    for _ in range(warmup):
        out = plan.apply(db).transformed
    out_bytes = out.payload_bytes()
    lib.synchronize()
    lib.prof_reset()
    lib.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.apply(db).transformed.free()
    lib.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / steps
    lib.prof_enable(False)
    kms = {k: ms / max(n, 1) for k, n, ms in lib.prof_get() if any(k.startswith(p) for p in kernels)}
    return wall_ms, kms, out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib.init(0)
    b = url_column(a.rows)
    db = lib.DeviceBatch.upload(b)
    in_bytes = int(b.cols[0].offsets[-1])
    res = {"workload": "regex_replace_transformer", "rows": a.rows, "column": "url", "bytes_in": in_bytes, "steps": a.steps, "warmup": a.warmup, "hbm_peak_gbs": HBM_PEAK_GBS, "rules": {}}
    for name, pat, rule in RULES:
        t = lib.Transformer("regex_replace_transformer", {"regexMatch": pat, "replaceRule": rule, "columns": {"includeColumns": ["^url$"]}})
        wall, kms, out_bytes = timed(t, db, a.steps, a.warmup, ["regex_replace_"])
        k = sum(kms.values())
        wrote = "regex_replace_write" in kms   # a column in which nothing matched keeps its buffers: the length pass alone ran
        read, written = (2 if wrote else 1) * in_bytes, out_bytes if wrote else 0
        moved = read + written + (3 if wrote else 2) * 4 * a.rows  # + offsets read per pass, lengths written once
        res["rules"][name] = {"regexMatch": pat, "replaceRule": rule, "ms_per_pass_host_clock": round(wall, 4), "kernel_ms": {x: round(v, 4) for x, v in sorted(kms.items())},
                              "bytes_read": read, "bytes_written": written, "fraction_of_hbm_peak": round(moved / (k * 1e-3) / (HBM_PEAK_GBS * 1e9), 5) if k else None,
                              "input_bytes_per_us": round(in_bytes / (k * 1e3), 2) if k else None}
    yard = {}
    for name, plan, kernels in [("mask_field", lib.Transformer("mask_field", {"columns": ["url"], "maskFunctionHash": {"userDefinedSalt": "s"}}), ["mask_"]),
                                ("convert_to_string", lib.Transformer("convert_to_string", {"columns": {"includeColumns": ["^url$"]}, "convert_to_bytes": True}), ["to_string"])]:
        wall, kms, out_bytes = timed(plan, db, a.steps, a.warmup, kernels)
        yard[name] = {"ms_per_pass_host_clock": round(wall, 4), "kernel_ms": {x: round(v, 4) for x, v in sorted(kms.items())}, "bytes_read": in_bytes, "bytes_written": out_bytes}
    res["same_column"] = yard  # (convert_to_string over a text column without nils only changes the type tag: no kernel runs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
