#!/usr/bin/env python3
"""Stand-alone measurement of tfgpu_nginx_parse on the GPU: 2^20 lines of the 47-field CDN log_format, resident in a tfgpu_dbuf,
parsed --steps times after --warmup calls.  Prints one JSON line: rows/s, ms per call (host clock around calls that end in a device
synchronise), per-kernel ms (HIP events on the library's stream, tfgpu_prof_*), and (bytes in + bytes out) over the dominant kernel's
time as a fraction of the HBM peak bench/common.py uses.  The same figure for csv_parse_regular over `hits` rows is taken in the same
process, as the yardstick: both are text parsers over resident bytes.  GPU only; it reads nothing outside the repository."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench.common import HBM_PEAK_GBS  # noqa: E402
from transferia_amd import abi, lib, workload  # noqa: E402

FIELDS = ["remote_addr", "remote_user", "time_local", "request", "status", "body_bytes_sent", "http_referer", "http_user_agent", "bytes_sent", "edgename", "scheme", "host",
          "request_time", "upstream_response_time", "request_length", "http_range", "responding_node", "upstream_cache_status", "upstream_response_length", "upstream_addr",
          "gcdn_api_client_id", "gcdn_api_resource_id", "uid_got", "uid_set", "geoip_country_code", "geoip_city", "shield_type", "server_addr", "server_port", "upstream_status",
          "upstream_connect_time", "upstream_header_time", "shard_addr", "geoip2_data_asnumber", "connection", "connection_requests", "request_id", "http_x_forwarded_proto",
          "http_x_forwarded_request_id", "ssl_cipher", "ssl_session_id", "ssl_session_reused", "sent_http_content_type", "real_tcpinfo_rtt", "http_x_forwarded_http_ver",
          "vp_enabled", "geoip2_region"]
BRACKETED = {"time_local", "edgename", "responding_node"}
TYPES = {"status": "int32", "body_bytes_sent": "uint64", "bytes_sent": "uint64", "request_length": "uint32", "request_time": "double", "upstream_response_time": "double",
         "time_local": "datetime", "server_port": "uint16", "connection": "uint64"}


def cdn_format() -> str:
    parts = []
    for i, f in enumerate(FIELDS):
        parts.append('"[$%s]"' % f if f in BRACKETED else '"$%s"' % f)
        if i == 0 or f == "upstream_status":
            parts.append('"-"')
    return " ".join(parts)


def cdn_lines(n: int, distinct: int = 4096, seed: int = 7) -> bytes:
    rng = random.Random(seed)
    months = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]
    lines = []
    for i in range(distinct):
        v = {f: "-" for f in FIELDS}
        v.update(remote_addr="%d.%d.%d.%d" % tuple(rng.randrange(256) for _ in range(4)),
                 time_local="%02d/%s/2025:%02d:%02d:%02d +0000" % (rng.randrange(1, 29), rng.choice(months), rng.randrange(24), rng.randrange(60), rng.randrange(60)),
                 request="GET /%s HTTP/1.1" % "/".join("p%d" % rng.randrange(1000) for _ in range(rng.randrange(1, 6))), status=str(rng.choice([200, 200, 200, 206, 304, 403, 404, 502])),
                 body_bytes_sent=str(rng.randrange(1 << 24)), http_user_agent="Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 (KHTML, like Gecko) Chrome/%d.0.0.0 Safari/537.36" % rng.randrange(90, 140),
                 bytes_sent=str(rng.randrange(1 << 24)), edgename="edge-%d" % rng.randrange(64), scheme=rng.choice(["http", "https"]), host="cdn%d.example.com" % rng.randrange(100),
                 request_time="%d.%03d" % (rng.randrange(3), rng.randrange(1000)), request_length=str(rng.randrange(100, 2000)), responding_node="n%d" % rng.randrange(16),
                 upstream_cache_status=rng.choice(["HIT", "MISS", "-"]), geoip_country_code=rng.choice(["US", "DE", "RU", "BR"]), geoip_city=rng.choice(["St Louis", "Berlin", "Moscow"]),
                 shield_type="shield_no", server_addr="10.0.%d.%d" % (rng.randrange(256), rng.randrange(256)), server_port=str(rng.choice([80, 443, 10080])),
                 connection=str(rng.randrange(1 << 32)), connection_requests=str(rng.randrange(1, 100)), request_id="%032x" % rng.getrandbits(128), http_x_forwarded_proto="https",
                 sent_http_content_type=rng.choice(["text/html", "application/json", "image/png"]), real_tcpinfo_rtt=str(rng.randrange(200000)), http_x_forwarded_http_ver="HTTP/1.1",
                 vp_enabled="0", geoip2_region=rng.choice(["MO", "BE", "MOW"]))
        if rng.random() < 0.5:
            v["upstream_response_time"] = "%d.%03d" % (rng.randrange(2), rng.randrange(1000))
        parts = []
        for k, f in enumerate(FIELDS):
            parts.append('"[%s]"' % v[f] if f in BRACKETED else '"%s"' % v[f])
            if k == 0 or f == "upstream_status":
                parts.append('"-"')
        lines.append(" ".join(parts) + "\n")
    block = "".join(lines).encode()
    reps, rest = divmod(n, distinct)
    return block * reps + "".join(lines[:rest]).encode()


def kernel_ms(names):
    return {k: ms / max(n, 1) for k, n, ms in lib.prof_get() if any(k.startswith(p) for p in names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--csv-rows", type=int, default=1 << 18)
    a = ap.parse_args()
    lib.init(0)
    fmt = lib.NginxFormat(cdn_format())
    assert fmt.fields == FIELDS
    schema = fmt.resolve_schema(abi.Schema([abi.ColSchema(f, TYPES.get(f, "utf8")) for f in FIELDS]))
    cs = schema.to_c()
    data = cdn_lines(a.lines)
    buf = lib.DeviceBuffer.upload(data)
    opts = lib.nginx_options(file_name="bench.log")

    def step():
        db, consumed, nxt, errs = lib.nginx_parse(fmt, opts, cs, buf)
        assert consumed == len(data) and not errs and db.nrows == a.lines and nxt == a.lines + 1
        return db
    for _ in range(a.warmup):
        db = step()
    out_bytes = db.payload_bytes()
    lib.synchronize()
    lib.prof_reset()
    lib.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    lib.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    lib.prof_enable(False)
    kms = kernel_ms(["nginx_", "csv_count_newlines", "csv_line_index"])
    dom = max((k for k in kms if k.startswith("nginx_")), key=lambda k: kms[k])
    frac = (len(data) + out_bytes) / (kms[dom] * 1e-3) / (HBM_PEAK_GBS * 1e9)

    # the yardstick, same process: csv_parse_regular over `hits` rows
    csv_schema, csv_data, csv_opts = workload.hits_schema(), workload.hits_csv(a.csv_rows), workload.hits_csv_options()
    cbuf, ccs = lib.DeviceBuffer.upload(csv_data), csv_schema.to_c()
    for _ in range(a.warmup):
        cdb, _, _ = lib.csv_parse(csv_opts, ccs, cbuf)
    csv_out = cdb.payload_bytes()
    lib.prof_reset()
    lib.prof_enable(True)
    for _ in range(a.steps):
        lib.csv_parse(csv_opts, ccs, cbuf)
    lib.synchronize()
    lib.prof_enable(False)
    cms = kernel_ms(["csv_parse_regular"])["csv_parse_regular"]
    csv_frac = (len(csv_data) + csv_out) / (cms * 1e-3) / (HBM_PEAK_GBS * 1e9)
    print(json.dumps({"workload": "nginx_parse", "lines": a.lines, "bytes_in": len(data), "bytes_out": out_bytes, "steps": a.steps, "warmup": a.warmup,
                      "ms_per_call_host_clock": round(wall_ms, 4), "rows_per_s": round(a.lines / (wall_ms * 1e-3)), "kernel_ms": {k: round(v, 4) for k, v in sorted(kms.items())},
                      "dominant_kernel": dom, "hbm_peak_gbs": HBM_PEAK_GBS, "dominant_kernel_fraction_of_hbm_peak": round(frac, 4),
                      "csv_parse_regular": {"rows": a.csv_rows, "bytes_in": len(csv_data), "bytes_out": csv_out, "kernel_ms": round(cms, 4), "fraction_of_hbm_peak": round(csv_frac, 4)}}))


if __name__ == "__main__":
    main()
