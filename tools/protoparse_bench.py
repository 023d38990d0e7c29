#!/usr/bin/env python3
"""Stand-alone measurement of the protobuf parser on the GPU: the reference's metrika fixture (162 CloudTransferHit events of 92 columns, about 106 bytes
each) replicated to 2^20 events, resident in HBM, parsed --steps times after --warmup calls through tfgpu_proto_parser_parse in each of the three
framings — single (one event a message), protoseq and repeated (162 events a message).  One process.  Prints one JSON line: per framing ms per call
and events/s (host clock around calls that end in a device synchronise), per-kernel ms (HIP events on the library's stream, tfgpu_prof_*) and
pp_decode's bytes per second as a share of the HBM peak; the same for events of about 2 KiB, where one lane per event walks twenty times as many
bytes (and, beside it, events made long by one bytes field the walk jumps over).  Beside it, as the existing decoder's figure on its own input and not as a threshold:
tfgpu_sr_proto_parse over the sr_proto workload's 784-byte message.  GPU only; it reads nothing outside tests/golden/."""
import argparse
import base64
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import protoparse_ref as R  # noqa: E402
from bench.common import HBM_PEAK_GBS  # noqa: E402
from tools.table_split_bench import profiled  # noqa: E402
from transferia_amd import abi, confluent_sr, lib  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


class DeviceMessages:
    """a tfgpu_message_batch with every array in HBM: `values` repeated `reps` times"""

    def __init__(self, values, reps):
        self.keep = []
        lens = np.tile(np.array([len(v) for v in values], np.uint64), reps)
        n = len(lens)
        start = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=start[1:])
        data = b"".join(values) * reps
        b = abi.CMessageBatch()
        b.topic, b.partition, b.mem, b.nmsg = b"bench/topic", 3, abi.MEM_DEVICE, n
        b.values, b.values_len, b.value_start = self.up(data), len(data), self.up(start.tobytes())
        b.offset = self.up(np.arange(n, dtype=np.uint64).tobytes())
        b.write_time_ns = self.up((1700000000000000000 + np.arange(n, dtype=np.int64) * 1000).tobytes())
        self.c, self.input_bytes = b, len(data)

    def up(self, data):
        d = lib.DeviceBuffer.upload(data if len(data) else b"\0")
        self.keep.append(d)
        return d.ptr


def run(parser, batch, event_bytes, steps, warmup):
    state = {}

    def once():
        dev, un, _ = parser.parse(batch.c, cap=16, event_base=False)
        state["rows"], state["unparsed"] = dev.nrows, len(un)
        dev.free()
    wall, kms = profiled(once, steps, warmup, ["pp_", "scan_"])
    out = {"ms_host_clock": round(wall, 4), "events_per_s": round(state["rows"] / (wall * 1e-3)), "rows": state["rows"], "unparsed": state["unparsed"],
           "messages": int(batch.c.nmsg), "input_bytes": batch.input_bytes, "kernel_ms": kms, "kernels_ms": round(sum(kms.values()), 4)}
    d = kms.get("pp_decode")
    if d:
        out["decode_gbs"] = round(event_bytes / (d * 1e-3) / 1e9, 2)
        out["decode_fraction_of_hbm_peak"] = round(event_bytes / (d * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)
        out["decode_events_per_s"] = round(state["rows"] / (d * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sr-messages", type=int, default=1 << 18)
    a = ap.parse_args()
    lib.init(0)
    with open(os.path.join(GOLD, "protoparser", "gotest", "metrika-data", "metrika_hit_log.desc"), "rb") as f:
        desc = f.read()
    with open(os.path.join(GOLD, "protoparser", "gotest", "metrika-data", "metrika_hit_log_data.bin"), "rb") as f:
        wrapper = f.read()
    events = [wrapper[v[0]:v[0] + v[1]] for num, wt, v in R.wire_fields(wrapper) if num == 1]
    reps = (a.events + len(events) - 1) // len(events)
    ev_bytes = sum(len(e) for e in events) * reps
    res = {"workload": "protobuf parser, metrika fixture replicated", "events": len(events) * reps, "bytes_per_event": round(ev_bytes / (len(events) * reps), 1), "steps": a.steps,
           "warmup": a.warmup, "hbm_peak_gbs": HBM_PEAK_GBS, "framings": {}}
    single = lib.ProtoParser.create(desc, "CloudTransferHit", "PackageTypeSingleMsg")
    res["framings"]["single"] = run(single, DeviceMessages(events, reps), ev_bytes, a.steps, a.warmup)
    seq = lib.ProtoParser.create(desc, "CloudTransferHit", "PackageTypeProtoseq")
    res["framings"]["protoseq"] = run(seq, DeviceMessages([b"".join(R.protoseq_frame(e) for e in events)], reps), ev_bytes, a.steps, a.warmup)
    rep = lib.ProtoParser.create(desc, "CloudTransferHitList", "PackageTypeRepeated")
    res["framings"]["repeated"] = run(rep, DeviceMessages([wrapper], reps), ev_bytes, a.steps, a.warmup)

    # long events of about 2 KiB (the s3 test's event is 2 183 bytes), two ways.  "walked": an event's own bytes 21 times over — a valid message (the
    # last value of a scalar stands, lists grow) every tag of which the lane has to read.  "skipped": the event plus ONE bytes field of 2 KiB, which the
    # walk jumps over (bytes are not validated): the decode's bytes/s is nominal there
    title = R.enc_bytes(4, ("заголовок страницы / page title " * 80).encode()[:2070])
    nlong = max(1, a.events // 16)
    for name, longs in (("walked", [e * 21 for e in events]), ("skipped", [e + title for e in events])):
        lreps = (nlong + len(longs) - 1) // len(longs)
        lbytes = sum(len(e) for e in longs) * lreps
        r = run(single, DeviceMessages(longs, lreps), lbytes, a.steps, a.warmup)
        r["bytes_per_event"] = round(lbytes / (len(longs) * lreps), 1)
        res["long_events_single_" + name] = r

    # the existing decoder on its own input
    with open(os.path.join(GOLD, "sr_protobuf.json")) as f:
        case = json.load(f)["cases"][1]
    msg, sid, text = base64.b64decode(case["message_b64"]), int(case["schema_id"]), case["schema"].encode()
    n = a.sr_messages
    data, msgs = abi.messages([msg] * n)
    dbuf = lib.DeviceBuffer.upload(data)
    schema = confluent_sr.ProtoSchema(lib, text)

    def sr_once():
        batch, errors = schema.parse(sid, dbuf, msgs)
        batch.free()
    wall, kms = profiled(sr_once, a.steps, a.warmup, ["pb_", "scan_"])
    res["sr_proto_parse_own_input"] = {"messages": n, "bytes_per_message": len(msg), "ms_host_clock": round(wall, 4), "messages_per_s": round(n / (wall * 1e-3)), "kernel_ms": kms,
                                       "decode_gbs": round(len(data) / (kms["pb_decode"] * 1e-3) / 1e9, 2) if kms.get("pb_decode") else None}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
