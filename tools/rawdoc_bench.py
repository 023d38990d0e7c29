#!/usr/bin/env python3
"""Stand-alone measurement of raw_doc_grouper on the GPU: 2^20 `hits` rows, resident in HBM, keys = (watchid), every column folded into `doc`, run
--steps times after --warmup calls through tfgpu_apply_meta with one CommitTime per row.  One process.  Prints one JSON line: ms per pass and rows/s
(host clock around calls that end in a device synchronise), per-kernel ms (HIP events on the library's stream, tfgpu_prof_*), the doc bytes, and the
write kernel's bytes written per second as a share of the HBM peak.  Beside it, as the nearest existing work and not as a threshold: tfgpu_serialize in
the encoding/json row format over the same batch — the same values and nearly the same bytes.  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench.common import HBM_PEAK_GBS  # noqa: E402
from transferia_amd import abi, lib  # noqa: E402
from tools.table_split_bench import hits_batch, profiled  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    lib.init(0)
    db = hits_batch(a.rows)
    plan = lib.Transformer("raw_doc_grouper", {"keys": ["watchid"]})
    ct = lib.DeviceBuffer.upload((1677510100000000000 + np.arange(a.rows, dtype=np.uint64) * 1000).tobytes())
    meta = abi.row_meta_device(a.rows, commit_time=ct.ptr)
    state = {}

    def group():
        lib.apply_meta([plan], db, meta).transformed.free()

    def serialize():
        buf = lib.serialize(abi.FMT_JSON, db)
        state["ser"] = buf.size
        buf.free()

    res = {"workload": "raw_doc_grouper", "rows": a.rows, "columns_in_batch": len(db.column_names()), "keys": ["watchid"], "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "hbm_peak_gbs": HBM_PEAK_GBS, "grouper": [], "serialize_json": []}
    probe = lib.apply_meta([plan], db, meta).transformed.download()
    doc_bytes = int(probe.col("doc").offsets[-1])
    res["doc_bytes"] = doc_bytes
    del probe
    for _ in range(a.repeats):   # the two alternately, so that a drift of the clocks shows in both
        wall, kms = profiled(group, a.steps, a.warmup, ["rawdoc_"])
        g = {"ms_host_clock": round(wall, 4), "rows_per_s": round(a.rows / (wall * 1e-3)), "kernel_ms": kms,
             "len_plus_write_ms": round(kms.get("rawdoc_len", 0) + kms.get("rawdoc_write", 0), 4)}
        if kms.get("rawdoc_write"):
            g["write_gbs"] = round(doc_bytes / (kms["rawdoc_write"] * 1e-3) / 1e9, 2)
            g["write_fraction_of_hbm_peak"] = round(doc_bytes / (kms["rawdoc_write"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)
        res["grouper"].append(g)
        wall2, kms2 = profiled(serialize, a.steps, a.warmup, ["ser_"])
        res["serialize_json"].append({"ms_host_clock": round(wall2, 4), "rows_per_s": round(a.rows / (wall2 * 1e-3)), "kernel_ms": kms2, "bytes": state.get("ser"),
                                      "kernels_ms": round(sum(kms2.values()), 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
