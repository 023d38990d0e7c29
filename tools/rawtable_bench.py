#!/usr/bin/env python3
"""Stand-alone measurement of the raw_to_table parser on the GPU: 2^20 synthetic messages of a few hundred bytes, resident in HBM, parsed --steps times
after --warmup calls through tfgpu_raw_to_table_parse under three configs — string value / no key; bytes key + JSON value + headers; JSON key + JSON
value.  One process.  Prints one JSON line: per config ms per call, messages/s and input GB/s (host clock around calls that end in a device
synchronise), per-kernel ms (HIP events on the library's stream, tfgpu_prof_*), rawtt_utf8_valid's bytes per second as a share of the HBM peak, and the
validator alone over messages of 64 B .. 32 KiB with the short / long switch moved (TFGPU_RAWTT_LONG_BYTES).  Beside the JSON config, as the nearest
existing work and not as a threshold: tfgpu_sr_json_parse over the same payloads framed as Confluent messages, every member an `any` property — the
same scan and emit plus typing.  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench.common import HBM_PEAK_GBS  # noqa: E402
from transferia_amd import abi, lib  # noqa: E402
from tools.table_split_bench import profiled  # noqa: E402

WORDS = ["значение", "value", "größe", "数据", "payload", "météo", "x", "идентификатор", "row", "😀"]
NDISTINCT = 4096


def tile(msgs, n):
    """n messages out of the distinct ones, round robin: (bytes, uint64 starts[n + 1])"""
    reps = (n + len(msgs) - 1) // len(msgs)
    lens = np.tile(np.array([len(m) for m in msgs], np.uint64), reps)[:n]
    start = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=start[1:])
    data = (b"".join(msgs) * reps)[: int(start[n])]
    return data, start


def text_message(rng, lo=200, hi=400):
    want, out = int(rng.integers(lo, hi)), []
    while sum(len(w) + 1 for w in out) < want:
        out.append(WORDS[int(rng.integers(len(WORDS)))].encode())
    return b" ".join(out)[:want].decode("utf-8", "ignore").encode()


def json_message(rng, i):
    m = {"id": i, "user": "user-%d" % int(rng.integers(1 << 20)), "amount": round(float(rng.random()) * 1e4, 2), "ok": bool(i & 1), "tags": ["a", "b", WORDS[i % len(WORDS)]],
         "note": text_message(rng, 80, 160).decode(), "nested": {"lat": 55.75, "lon": 37.61, "z": None}}
    keys = sorted(m) if i % 8 else list(m)   # one in eight with its keys as written: the sorting emitter
    return json.dumps({k: m[k] for k in keys}, ensure_ascii=False, separators=(",", ":")).encode()


class DeviceMessages:
    """a tfgpu_message_batch with every array in HBM"""

    def __init__(self, n, values, vstart, keys=None, kstart=None, headers=False):
        self.keep = []
        b = abi.CMessageBatch()
        b.topic, b.partition, b.mem, b.nmsg = b"bench_topic", 3, abi.MEM_DEVICE, n
        b.values, b.values_len, b.value_start = self.up(values), len(values), self.up(vstart.tobytes())
        if keys is not None:
            b.keys, b.keys_len, b.key_start = self.up(keys), len(keys), self.up(kstart.tobytes())
        b.offset = self.up(np.arange(n, dtype=np.uint64).tobytes())
        b.write_time_ns = self.up((1700000000000000000 + np.arange(n, dtype=np.int64) * 1000).tobytes())
        if headers:   # two pairs a message: ("source", "bench"), ("trace", "<message index mod 4096, 8 hex digits>")
            traces = b"".join(b"%08x" % i for i in range(NDISTINCT))
            hb = b"sourcebenchtrace" + traces
            pairs = np.zeros((n, 2, 4), np.uint32)
            pairs[:, 0] = (0, 6, 6, 5)
            pairs[:, 1, 0], pairs[:, 1, 1], pairs[:, 1, 3] = 11, 5, 8
            pairs[:, 1, 2] = 16 + 8 * (np.arange(n, dtype=np.uint32) % NDISTINCT)
            b.header_bytes, b.header_bytes_len = self.up(hb), len(hb)
            b.header_pair_start, b.header_pairs, b.npairs = self.up((np.arange(n + 1, dtype=np.uint64) * 2).tobytes()), self.up(pairs.tobytes()), 2 * n
        self.c, self.input_bytes = b, len(values) + (len(keys) if keys is not None else 0)

    def up(self, data):
        d = lib.DeviceBuffer.upload(data if len(data) else b"\0")
        self.keep.append(d)
        return d.ptr


def run(parser, batch, steps, warmup):
    state = {}

    def once():
        m, d, fb = parser.parse(batch.c)
        state["rows"] = (m.nrows, d.nrows, len(fb))
        m.free()
        d.free()
    wall, kms = profiled(once, steps, warmup, ["rawtt_", "scan_"])
    n = int(batch.c.nmsg)
    return {"ms_host_clock": round(wall, 4), "messages_per_s": round(n / (wall * 1e-3)), "input_gb_per_s": round(batch.input_bytes / (wall * 1e-3) / 1e9, 3),
            "input_bytes": batch.input_bytes, "rows_main_dlq_fallback": state["rows"], "kernel_ms": kms, "kernels_ms": round(sum(kms.values()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep-mib", type=int, default=256)
    a = ap.parse_args()
    lib.init(0)
    n = a.messages
    rng = np.random.default_rng(7)
    chunk, long_ = lib.rawtt_geometry()
    res = {"workload": "raw_to_table", "messages": n, "steps": a.steps, "warmup": a.warmup, "hbm_peak_gbs": HBM_PEAK_GBS, "chunk_bytes": chunk, "long_bytes": long_, "configs": {}}
    texts = [text_message(rng) for _ in range(NDISTINCT)]
    texts[7] = texts[7][:50] + b"\xff" + texts[7][50:]   # a few for the dead-letter table
    jsons = [json_message(rng, i) for i in range(NDISTINCT)]
    jsons[9] = jsons[9][:-1]
    keys_b = [b"key-%06d" % i for i in range(NDISTINCT)]
    keys_j = [b'{"id":%d,"shard":"s%d"}' % (i, i % 16) for i in range(NDISTINCT)]
    tv, tvs = tile(texts, n)
    jv, jvs = tile(jsons, n)
    kb, kbs = tile(keys_b, n)
    kj, kjs = tile(keys_j, n)

    # 1. string value, no key
    batch = DeviceMessages(n, tv, tvs)
    r = run(lib.RawToTable.create("", "string"), batch, a.steps, a.warmup)
    u = r["kernel_ms"].get("rawtt_utf8_valid")
    if u:
        r["utf8_valid_gbs"] = round(len(tv) / (u * 1e-3) / 1e9, 2)
        r["utf8_valid_fraction_of_hbm_peak"] = round(len(tv) / (u * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)
    res["configs"]["string_value_no_key"] = r
    del batch
    # 2. bytes key + JSON value + headers
    batch = DeviceMessages(n, jv, jvs, kb, kbs, headers=True)
    res["configs"]["bytes_key_json_value_headers"] = run(lib.RawToTable.create("", "json", "bytes", headers=True), batch, a.steps, a.warmup)
    del batch
    # 3. JSON key + JSON value
    batch = DeviceMessages(n, jv, jvs, kj, kjs)
    rj = run(lib.RawToTable.create("", "json", "json"), batch, a.steps, a.warmup)
    res["configs"]["json_key_json_value"] = rj
    del batch

    # the comparison: the same JSON payloads as Confluent JSON-schema frames, every member an `any` property
    framed = [b"\0\0\0\0\x01" + j for j in jsons]
    fv, fvs = tile(framed, n)
    msgs = abi.CMessages()
    off, wt = np.zeros(n, np.uint64), np.zeros(n, np.int64)
    msgs.nmsg, msgs.start, msgs.offset, msgs.write_time_ns = n, fvs.ctypes.data, off.ctypes.data, wt.ctypes.data
    opts = abi.sr_json_options(1, [(k, 5, False) for k in sorted(["id", "user", "amount", "ok", "tags", "note", "nested"])], "", "bench")
    dev = lib.DeviceBuffer.upload(fv)

    def sr_once():
        lib.sr_json_parse(opts, dev, msgs).device_batch.free()
    wall, kms = profiled(sr_once, a.steps, a.warmup, ["sr_", "scan_"])
    res["sr_json_parse_same_payloads"] = {"ms_host_clock": round(wall, 4), "input_bytes": len(fv), "kernel_ms": kms, "kernels_ms": round(sum(kms.values()), 4),
                                          "kernels_ms_per_gb": round(sum(kms.values()) / (len(fv) / 1e9), 4)}
    jk = {k: v for k, v in rj["kernel_ms"].items()}
    res["json_key_json_value_kernels_ms_per_gb"] = round(sum(jk.values()) / (rj["input_bytes"] / 1e9), 4)
    del dev

    # the short / long switch: the validator alone over lengths 64 B .. 32 KiB (log-uniform, ~256 MiB), ASCII with a multi-byte word now and then
    lens = np.exp(rng.uniform(np.log(64), np.log(32768), 2048)).astype(int)
    base = (" ".join(WORDS) + " ").encode() * 1200
    longs = [base[:int(x)].decode("utf-8", "ignore").encode() for x in lens]
    nl = max(1, (a.sweep_mib << 20) // sum(len(x) for x in longs)) * len(longs)
    lv, lvs = tile(longs, nl)
    batch = DeviceMessages(nl, lv, lvs)
    sweep = {}
    p = lib.RawToTable.create("", "string")
    for lb in (2 * chunk, 256, 1024, 4096, 16384, 1 << 30):
        os.environ["TFGPU_RAWTT_LONG_BYTES"] = str(lb)
        r = run(p, batch, a.steps, a.warmup)
        u = r["kernel_ms"].get("rawtt_utf8_valid", 0)
        sweep[str(lb)] = {"utf8_valid_ms": u, "gbs": round(len(lv) / (u * 1e-3) / 1e9, 2) if u else None}
    os.environ.pop("TFGPU_RAWTT_LONG_BYTES", None)
    res["long_switch_sweep"] = {"messages": nl, "bytes": len(lv), "by_long_bytes": sweep}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
