// tf_protoparse.hip — the per-batch half of the generic protobuf parser (pkg/parsers/registry/protobuf; the compiled parser comes from tf_protodesc.cpp).
//
//   ProtoParser.DoBatch / do / processScanned       protoparser/proto_parser.go:76-146
//   makeValues, extractValueRecursive, …Leaf        protoparser/proto_parser.go:189-339
//   ProtoseqScanner, DoNotSplitScanner              pkg/parsers/scanner/protoseq_scanner.go, donotsplit_scanner.go
//   RepeatedScanner, SplitterScanner                protoscanner/repeated_scanner.go, splitter_scanner.go
//
// A queue message holds one event (single), a chain of protoseq frames, or a wrapper whose only field is a repeated message.  Kernels:
//   pp_check_batch   the batch's own offsets: ascending, inside the buffer (nothing below reads a byte before this has passed)
//   pp_frames<W>     lane = message: the framing walk.  W = false counts the message's events, (scan), W = true writes their spans
//                    (start, len, message, counter, framing code).  protoseq: size, payload, magic — a few reads per frame; an oversized size or
//                    a sync mismatch searches the next magic from behind the size field; the three failing forms are events with a code.
//                    repeated: the wrapper's top level through the shared wire walk; elements are the occurrences of its field.
//   pp_decode        lane = event: the wire walk over (start, len) keeping every field's LAST occurrence, nested messages walked, proto3 strings
//                    checked for UTF-8, then the Required columns.  One lane per event is latency-bound on long events.
//   pp_msg_final     lane = message: under `repeated` an element that does not unmarshal fails the WRAPPER — the message is one failed event
//   pp_keep / pp_rows  the kept events, their rows, src_row (the event's ordinal) and part_id (the message)
//   pp_cells<ANY, WIDE>, pp_text_copy, pp_text_any<WIDE>   as the SR branch's, with this parser's typing and NotFillEmptyFields
//   pp_aux, pp_const_text   _offset, _idx, _lb_ctime, _lb_wtime; _partition (one constant text)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "tf_common.hpp"
#include "tf_ingest.hpp"
#include "tf_devrow.hpp"
#include "tf_devfmt.hpp"
#include "tf_pbwire.hpp"
#include "tf_protodesc.hpp"
#include "tf_utf8.hpp"

namespace tf {
namespace ppd {

using pbd::DField;
using pbd::DMember;

constexpr uint32_t PROTOSEQ_MAX_RECORD = 64u << 20;  // maxRecordSize: "64mb - const from push-client"
__constant__ uint8_t PROTOSEQ_MAGIC[32] __attribute__((aligned(8))) = {31, 247, 247, 126, 190, 166, 94, 158, 55, 166, 246, 46, 254, 174, 71, 167,
                                                 183, 110, 191, 175, 22, 158, 159, 55, 246, 87, 247, 102, 167, 6, 175, 247};

struct Frames {
  const uint8_t *data; const uint64_t *start; int64_t nmsg;
  int32_t pkg, wrapper_number;
  uint32_t *nev;        // [nmsg + 1]: counts, then their exclusive scan
  uint32_t *msg_state;  // [nmsg]: 0, 1 = the host takes the whole message, 2 = the wrapper does not unmarshal
  uint32_t *ev_start, *ev_len, *ev_msg, *ev_idx; uint8_t *ev_code;
  uint32_t *nerr;
};

__global__ void __launch_bounds__(256) pp_check_batch(const uint64_t *start, uint64_t len, int64_t n, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i <= n) bad = start[i] > len || (i < n && start[i] > start[i + 1]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1u);
}

__device__ __forceinline__ bool magic_at(MemBytes &rd, uint32_t pos) {
  const uint64_t *m = reinterpret_cast<const uint64_t *>(PROTOSEQ_MAGIC);
  return rd.word(pos) == m[0] && rd.word(pos + 8) == m[1] && rd.word(pos + 16) == m[2] && rd.word(pos + 24) == m[3];
}
// ProtoseqScanner.Scan over [a, z): on(start, len, code) per event
template <class F> __device__ void protoseq_frames(MemBytes &rd, uint32_t a, uint32_t z, F on) {
  uint32_t pos = a;
  while (pos < z) {
    if (z - pos < 4) { on(pos, z - pos, (int)TFGPU_ROW_PROTO_FRAME_SHORT); return; }
    const uint32_t size = (uint32_t)rd.bytes(pos, 4);
    pos += 4;
    if (size <= PROTOSEQ_MAX_RECORD) {
      if ((uint64_t)(z - pos) < (uint64_t)size + 32u) { on(pos - 4, z - pos + 4, (int)TFGPU_ROW_PROTO_FRAME_INCOMPLETE); return; }
      if (magic_at(rd, pos + size)) { on(pos, size, 0); pos += size + 32u; continue; }
    }
    // handleCurrentCorrupted: bytes.Index(data, magic) from behind the size field; nothing found: the rest is dropped (do never reads sc.Err())
    uint32_t q = pos;
    bool found = false;
    for (; z - q >= 32u; q++) if (rd.at(q) == 31u && magic_at(rd, q)) { found = true; break; }
    if (!found) return;
    on(pos, q - pos, (int)TFGPU_ROW_PROTO_FRAME_CORRUPTED);
    pos = q + 32u;
  }
}

template <bool WRITE> __global__ void __launch_bounds__(128) pp_frames(Frames f) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= f.nmsg) return;
  if (WRITE && f.msg_state[m]) return;  // (counted as no event: a walk that stops half way has no slots to write to)
  const uint32_t a = (uint32_t)f.start[m], z = (uint32_t)f.start[m + 1];
  MemBytes rd(f.data);
  uint32_t n = 0;
  const uint32_t base = WRITE ? f.nev[m] : 0u;
  auto ev = [&](uint32_t s, uint32_t l, int code) {
    if constexpr (WRITE) { const uint32_t e = base + n; f.ev_start[e] = s; f.ev_len[e] = l; f.ev_msg[e] = (uint32_t)m; f.ev_idx[e] = n + 1; f.ev_code[e] = (uint8_t)code; }
    n++;
  };
  if (f.pkg == TFGPU_PROTO_PKG_SINGLE) { if (z > a) ev(a, z - a, 0); }
  else if (f.pkg == TFGPU_PROTO_PKG_PROTOSEQ) protoseq_frames(rd, a, z, ev);
  else {
    // the wrapper's own level: occurrences of its field are the elements; another number is an unknown field (kept aside, ignored); its field with
    // another wire type, a group, a number beyond 2^29 - 1: the stock code decides
    const int rc = pbd::walk(rd, a, z, [&](uint32_t num, uint32_t wt, uint64_t raw, uint32_t len) {
      if (num != (uint32_t)f.wrapper_number) return 0;
      if (wt != 2) return 2;
      ev((uint32_t)raw, len, 0);
      return 0;
    });
    if (rc) { n = 0; if constexpr (!WRITE) { f.msg_state[m] = rc == 1 ? 2u : 1u; atomicAdd(f.nerr, 1u); } }
  }
  if constexpr (!WRITE) f.nev[m] = n;
}

struct Params {
  const uint8_t *data;
  const DField *fields; const uint32_t *fflags; int32_t nfields; const DMember *members; const uint8_t *names;
  const int16_t *lut; int32_t lutn;
  const uint32_t *ev_start, *ev_len, *ev_msg, *ev_idx; uint8_t *ev_code; int32_t *ev_col; int64_t nev;
  uint64_t *rec; uint8_t *present;  // [nfields][nev]
  uint32_t *msg_state; uint32_t *nerr;
  const int32_t *req; int32_t nreq;  // (column, field) pairs: the columns whose absence fails the event
  int32_t pkg, nfe, schema_code;
  const uint32_t *row_ev; int64_t nrows;
};

// a nested message's (or a map entry's) bytes: its known members with their wire types, its strings valid UTF-8
__device__ __forceinline__ int check_members(MemBytes &d, const Params &p, const DField &fd, uint32_t a, uint32_t len) {
  return pbd::walk(d, a, a + len, [&](uint32_t n2, uint32_t w2, uint64_t r2, uint32_t l2) {
    for (int k = 0; k < fd.nmem; k++) {
      const DMember &mb = p.members[fd.mem_off + k];
      if ((uint32_t)mb.number != n2) continue;
      const int t = mb.ptype & MEMBER_TYPE;
      if ((int)w2 != pbd::want_wt(t)) return 2;
      if (t == TFGPU_PB_STRING && !utf8_valid_range(d, (uint32_t)r2, (uint32_t)r2 + l2, (uint32_t)r2 + l2)) return 1;
    }
    return 0;
  });
}

__global__ void __launch_bounds__(128) pp_decode(Params p) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.nev) return;
  const uint32_t msg = p.ev_msg[e];
  auto done = [&](int st, int col) {
    p.ev_code[e] = (uint8_t)st; p.ev_col[e] = col;
    if (st) atomicAdd(p.nerr, 1u);
  };
  const int framing = p.ev_code[e];
  if (framing) return done(framing, -1);
  if (p.schema_code) return done(p.schema_code, -1);
  MemBytes d(p.data);
  const uint32_t a = p.ev_start[e], z = a + p.ev_len[e];
  for (int f = 0; f < p.nfields; f++) p.present[(int64_t)f * p.nev + e] = 0;
  bool twice = false;
  const int rc = pbd::walk(d, a, z, [&](uint32_t num, uint32_t wt, uint64_t raw, uint32_t len) {
    int f = -1;
    if (num < (uint32_t)p.lutn) f = p.lut[num];
    else for (int k = 0; k < p.nfields; k++) if ((uint32_t)p.fields[k].number == num) { f = k; break; }
    if (f < 0) return 0;  // an unknown field: kept aside by the dynamic message, no column reads it
    if (p.fflags[f] & PF_FOREIGN) return 2;  // a field outside the device subset: the device cannot vouch that its bytes unmarshal
    const DField &fd = p.fields[f];
    const int64_t i = (int64_t)f * p.nev + e;
    if (fd.oneof) for (int k = 0; k < p.nfields; k++) if (k != f && p.fields[k].oneof == fd.oneof) p.present[(int64_t)k * p.nev + e] = 0;  // the LAST member on the wire stays
    if (fd.repeated) {
      const int ew = pbd::want_wt(fd.ptype);
      if (fd.ptype == TFGPU_PB_MESSAGE) {
        if (wt != 2) return 2;
        const int r2 = check_members(d, p, fd, (uint32_t)raw, len);
        if (r2) return r2;
        if (fd.repeated == 2 && (p.members[fd.mem_off + 1].ptype & MEMBER_TYPE) == TFGPU_PB_BYTES) {  // an entry without its bytes value holds a nil []byte (null in the text): the host's
          bool has_value = false;
          pbd::walk(d, (uint32_t)raw, (uint32_t)raw + len, [&](uint32_t n2, uint32_t, uint64_t, uint32_t) { if (n2 == 2) has_value = true; return 0; });
          if (!has_value) return 3;
        }
        if (fd.repeated == 2) { const uint64_t seen = p.present[i] ? p.rec[i] + 1 : 1; p.rec[i] = seen; if (seen > pbd::MAP_MAX_ENTRIES) return 3; }
        p.present[i] = 1;
        return 0;
      }
      if ((int)wt == ew) {
        if (fd.ptype == TFGPU_PB_STRING && !utf8_valid_range(d, (uint32_t)raw, (uint32_t)raw + len, (uint32_t)raw + len)) return 1;
        p.present[i] = 1;
        return 0;
      }
      if (wt != 2) return 2;
      uint32_t q = (uint32_t)raw; const uint32_t qe = q + len;  // a packed run
      while (q < qe) {
        if (ew == 0) { uint64_t v; if (!pbd::varint(d, q, qe, &v)) return 1; }
        else { const uint32_t w = ew == 1 ? 8u : 4u; if (qe - q < w) return 1; q += w; }
      }
      if (len) p.present[i] = 1;  // (an empty run adds no element: Has() of a list is Len() > 0)
      return 0;
    }
    if ((int)wt != pbd::want_wt(fd.ptype)) return 2;  // a known field with a foreign wire type
    if (fd.ptype == TFGPU_PB_MESSAGE) {
      if (p.present[i]) twice = true;  // protobuf merges the occurrences
      const int r2 = check_members(d, p, fd, (uint32_t)raw, len);
      if (r2) return r2;
    } else if (fd.ptype == TFGPU_PB_STRING && !utf8_valid_range(d, (uint32_t)raw, (uint32_t)raw + len, (uint32_t)raw + len)) return 1;
    p.rec[i] = wt == 2 ? (raw | ((uint64_t)len << 32)) : raw;
    p.present[i] = 1;
    return 0;
  });
  if (rc == 1) { if (p.pkg == TFGPU_PROTO_PKG_REPEATED) atomicMax(&p.msg_state[msg], 2u); return done(TFGPU_ROW_PROTO_UNMARSHAL, -1); }
  if (rc == 2) { if (p.pkg == TFGPU_PROTO_PKG_REPEATED) atomicMax(&p.msg_state[msg], 1u); return done(TFGPU_ROW_HOST_FALLBACK, -1); }
  if (rc == 3 || twice) return done(TFGPU_ROW_HOST_FALLBACK, -1);
  for (int k = 0; k < p.nreq; k++) if (!p.present[(int64_t)p.req[2 * k + 1] * p.nev + e]) return done(TFGPU_ROW_PROTO_REQUIRED, p.req[2 * k]);
  done(TFGPU_ROW_OK, -1);
}

// nfin[m]: the events message m counts for (a message the wrapper of which fails, or which the host takes whole, is ONE)
__global__ void __launch_bounds__(256) pp_msg_final(const uint32_t *nev_scan, const uint32_t *msg_state, int64_t nmsg, uint32_t *nfin) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m < nmsg) nfin[m] = msg_state[m] ? 1u : nev_scan[m + 1] - nev_scan[m];
}
__global__ void __launch_bounds__(256) pp_keep(Params p, uint32_t *keep) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < p.nev) keep[e] = p.ev_code[e] == 0 && p.msg_state[p.ev_msg[e]] == 0 ? 1u : 0u;
}
__global__ void __launch_bounds__(256) pp_rows(Params p, const uint32_t *keep_scan, const uint32_t *event_base, uint32_t *row_ev, int32_t *src_row, uint32_t *part_id) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.nev || keep_scan[e + 1] == keep_scan[e]) return;
  const uint32_t r = keep_scan[e], m = p.ev_msg[e];
  row_ev[r] = (uint32_t)e;
  src_row[r] = (int32_t)(event_base[m] + p.ev_idx[e] - 1u);
  part_id[r] = m;
}

struct OutCol {
  int32_t field;       // index into the field table
  int32_t nfe_top;     // NotFillEmptyFields applies to the column itself (not to an `_lb_extra_` column: makeValues' second loop)
  void *values;        // fixed-width kinds
  uint32_t *lens;      // text kinds: lengths, then offsets [nrows + 1]
  uint8_t *data;
  uint8_t *validity;   // bitmap, written 64 rows (one wave) at a time
};

// Has() of a proto3 field without explicit presence: the value is not the zero value.  minus_zero: −0.0, which the device leaves to the host
__device__ __forceinline__ bool nonzero(int t, uint64_t raw, bool &minus_zero) {
  switch (t) {
    case TFGPU_PB_STRING: case TFGPU_PB_BYTES: return (uint32_t)(raw >> 32) != 0;
    case TFGPU_PB_FLOAT: if ((uint32_t)raw == 0x80000000u) minus_zero = true; return ((uint32_t)raw & 0x7FFFFFFFu) != 0;
    case TFGPU_PB_DOUBLE: if (raw == 0x8000000000000000ull) minus_zero = true; return (raw & 0x7FFFFFFFFFFFFFFFull) != 0;
    default: return pbd::as_i64(t, raw) != 0;
  }
}

// extractValueExceptListRecursive of a message value: {"name":value,…} in name order.  Under NotFillEmptyFields only the members that are set, and
// false (nil) when none is; a message type without fields is nil in either mode (cntEmpty == Len() == 0).  host: NaN / Inf, or −0.0 under the flag
template <class S> __device__ bool emit_msg(S &s, const Params &p, const DField &fd, uint32_t a, uint32_t len, bool &host) {
  if (fd.nmem == 0) return false;
  MemBytes rd(p.data);
  bool any = false;
  for (int k = 0; k < fd.nmem; k++) {
    const DMember &mb = p.members[fd.mem_off + k];
    const int t = mb.ptype & MEMBER_TYPE;
    bool present = false; uint64_t raw = 0;
    pbd::walk(rd, a, a + len, [&](uint32_t n2, uint32_t w2, uint64_t r2, uint32_t l2) { if ((uint32_t)mb.number == n2) { present = true; raw = w2 == 2 ? (r2 | ((uint64_t)l2 << 32)) : r2; } return 0; });
    if (p.nfe) {
      bool has = present;
      if (present && !(mb.ptype & MEMBER_EXPLICIT)) { bool mz = false; has = nonzero(t, raw, mz); if (mz) host = true; }
      if (!has) continue;
    }
    s.put(any ? ',' : '{');
    any = true;
    emit_json_string(s, p.names + mb.name_off, mb.name_len, false);
    s.put(':');
    if (t == TFGPU_PB_BYTES && !present) put_lit(s, "null");  // Get of an unset bytes field is a nil []byte: json.Marshal writes null (a set, empty one is "")
    else if (!pbd::emit_member(s, p.data, t, present, raw)) host = true;
  }
  if (!any) return false;
  s.put('}');
  return true;
}
// a repeated message field: the elements in wire order, a nil element as null (items[i] stays nil)
template <class S> __device__ void emit_msg_array(S &s, const Params &p, const DField &fd, uint32_t a, uint32_t z, bool &host) {
  MemBytes rd(p.data);
  bool first = true;
  s.put('[');
  pbd::walk(rd, a, z, [&](uint32_t num, uint32_t wt, uint64_t raw, uint32_t len) {
    if (num != (uint32_t)fd.number || wt != 2) return 0;
    if (!first) s.put(',');
    first = false;
    if (!emit_msg(s, p, fd, (uint32_t)raw, len, host)) put_lit(s, "null");
    return 0;
  });
  s.put(']');
}

// one `any` cell into the sink; false: nil
template <bool WIDE, class S> __device__ bool any_cell(S &s, const Params &p, const OutCol &c, const DField &fd, uint32_t e, bool present, uint64_t raw, bool &host) {
  const uint32_t a = p.ev_start[e], z = a + p.ev_len[e];
  if (fd.repeated) {
    if (c.nfe_top && !present) return false;  // !Has: nil; without the flag an absent list is [] and an absent map {}
    if constexpr (WIDE) {
      if (fd.repeated == 2) { if (!pbd::emit_map(s, p, fd, a, z)) host = true; }
      else emit_msg_array(s, p, fd, a, z, host);
    } else if (!pbd::emit_array<false>(s, p, fd, a, z)) host = true;
    return true;
  }
  if (!present) return c.nfe_top ? false : emit_msg(s, p, fd, 0u, 0u, host);  // Get of an unset message field: the empty message
  return emit_msg(s, p, fd, (uint32_t)raw, (uint32_t)(raw >> 32), host);
}

// ANY = false: fixed-width values and string / bytes lengths; ANY = true: the `any` columns (the JSON emitter's registers); WIDE: maps and repeated
// messages (the key-order scan, an emitter inside the element walk) — the split tf_protobuf.hip measured
template <bool ANY, bool WIDE = false> __global__ void __launch_bounds__(256) pp_cells(Params p, const OutCol *cols, const int32_t *list, uint32_t *host_rows) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < p.nrows;
  const OutCol &c = cols[list[blockIdx.y]];
  const DField &fd = p.fields[c.field];
  bool valid = in;
  if (in) {
    const uint32_t e = p.row_ev[r];
    const int64_t i = (int64_t)c.field * p.nev + e;
    const bool present = p.present[i] != 0;
    uint64_t raw = present ? p.rec[i] : 0ull;
    if constexpr (ANY) {
      CountSink s;
      bool host = false;
      valid = any_cell<WIDE>(s, p, c, fd, e, present, raw, host);
      if (host) { host_rows[r] = 1; s.n = 0; }
      c.lens[r] = valid ? s.n : 0u;
    } else {
      if (c.nfe_top) {
        bool has = present, mz = false;
        if (present && !(p.fflags[c.field] & PF_EXPLICIT)) has = nonzero(fd.ptype, raw, mz);
        if (mz) host_rows[r] = 1;
        if (!has) { valid = false; raw = 0; }
      }
      switch (fd.ptype) {
        case TFGPU_PB_STRING: case TFGPU_PB_BYTES: c.lens[r] = (uint32_t)(raw >> 32); break;
        case TFGPU_PB_DOUBLE: case TFGPU_PB_INT64: case TFGPU_PB_UINT64: case TFGPU_PB_FIXED64: case TFGPU_PB_SFIXED64: case TFGPU_PB_SINT64:
          ((uint64_t *)c.values)[r] = (uint64_t)pbd::as_i64(fd.ptype, raw); break;
        case TFGPU_PB_BOOL: ((uint8_t *)c.values)[r] = raw != 0; break;
        default: ((uint32_t *)c.values)[r] = fd.ptype == TFGPU_PB_FLOAT ? (uint32_t)raw : (uint32_t)pbd::as_i64(fd.ptype, raw);
      }
    }
  }
  const uint64_t bal = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && in) reinterpret_cast<uint64_t *>(c.validity)[r >> 6] = bal;
}
__global__ void __launch_bounds__(256) pp_text_copy(Params p, const OutCol *cols, const int32_t *list) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  const OutCol &c = cols[list[blockIdx.y]];
  const uint32_t n = c.lens[r + 1] - c.lens[r];  // (offsets by now)
  if (!n) return;
  const uint64_t raw = p.rec[(int64_t)c.field * p.nev + p.row_ev[r]];
  WriteSink s{c.data + c.lens[r]};
  put_bytes(s, p.data + (uint32_t)raw, n);
  s.flush();
}
template <bool WIDE> __global__ void __launch_bounds__(256) pp_text_any(Params p, const OutCol *cols, const int32_t *list) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  const OutCol &c = cols[list[blockIdx.y]];
  if (c.lens[r + 1] == c.lens[r]) return;  // nil, or a row for the host: nothing was counted
  const uint32_t e = p.row_ev[r];
  const int64_t i = (int64_t)c.field * p.nev + e;
  const bool present = p.present[i] != 0;
  WriteSink s{c.data + c.lens[r]};
  bool host = false;
  any_cell<WIDE>(s, p, c, p.fields[c.field], e, present, present ? p.rec[i] : 0ull, host);
  s.flush();
}

struct Aux {
  const uint32_t *row_ev, *ev_msg, *ev_idx; int64_t nrows;
  const uint64_t *offset; const int64_t *wt, *ct;
  uint64_t *col_offset, *col_idx; int64_t *ct_sec, *wt_sec; int32_t *ct_nsec, *wt_nsec;
};
__global__ void __launch_bounds__(256) pp_aux(Aux x) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= x.nrows) return;
  const uint32_t e = x.row_ev[r], m = x.ev_msg[e];
  if (x.col_offset) x.col_offset[r] = x.offset ? x.offset[m] : 0ull;
  if (x.col_idx) x.col_idx[r] = x.ev_idx[e];
  if (x.ct_sec) { const int64_t t = x.ct ? x.ct[m] : 0, q = dev::floordiv(t, 1000000000ll); x.ct_sec[r] = q; x.ct_nsec[r] = (int32_t)(t - q * 1000000000ll); }
  if (x.wt_sec) { const int64_t t = x.wt ? x.wt[m] : 0, q = dev::floordiv(t, 1000000000ll); x.wt_sec[r] = q; x.wt_nsec[r] = (int32_t)(t - q * 1000000000ll); }
}
__global__ void __launch_bounds__(256) pp_const_text(const uint8_t *text, uint32_t tlen, int64_t nrows, uint32_t *off, uint8_t *data) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nrows) off[i] = (uint32_t)i * tlen;
  if (i < nrows * (int64_t)tlen) data[i] = text[i % tlen];
}

}  // namespace ppd
}  // namespace tf

using namespace tf;
using namespace tf::ppd;

extern "C" int tfgpu_proto_parser_parse(const tfgpu_proto_parser *h, const tfgpu_message_batch *b, const int64_t *create_time_ns, tfgpu_dbatch **out,
                                        tfgpu_proto_unparsed *unparsed, int64_t cap, int64_t *nunparsed, int64_t *event_base) {
  TF_API_BEGIN
  const char *T = "protobuf parser: ";
  if (!h || !b || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_parse: null argument");
  // the size refusals, from the stated lengths, before a byte is read
  if (b->nmsg < 0) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "negative message count");
  if (b->nmsg > 0x7FFFFFFFll) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "more than 2^31-1 messages: split the batch");
  if (b->values_len >= 0xFFFFFFF0ull) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the values reach 4 GiB (32-bit offsets): split the batch");
  if (b->mem != TFGPU_MEM_HOST && b->mem != TFGPU_MEM_DEVICE) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "bad mem");
  const int64_t n = b->nmsg, na = std::max<int64_t>(n, 1);
  if (n && !b->value_start) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "value_start is null");
  if (b->values_len && !b->values) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "a byte buffer is null");
  if (cap < 0 || (cap && !unparsed)) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "bad unparsed list");
  const int nf = (int)h->fields.size(), ncol = (int)h->cols.size();
  Context &cx = ctx();
  std::lock_guard<std::mutex> lk(cx.mu);
  hipStream_t st = cx.stream;
  std::string topic = b->topic ? b->topic : "";
  const std::string partition_text = "{\"partition\":" + std::to_string(b->partition) + ",\"topic\":\"" + topic + "\"}";  // Partition.String()
  for (auto &ch : topic) if (ch == '/' || ch == '@') ch = '_';  // tableName

  // ---- the batch in HBM ---------------------------------------------------------------------------------------------------------------------------------
  Buf vdata, vstart, boffset, bwt, bct;
  stage_bytes(b->values, b->values_len, b->mem, vdata);
  static const uint64_t ZERO1[1] = {0};
  const uint64_t *dstart = n ? stage_array<uint64_t>(b->value_start, (size_t)n + 1, b->mem, vstart) : stage_array<uint64_t>(ZERO1, 1, TFGPU_MEM_HOST, vstart);
  const uint64_t *doffset = stage_array<uint64_t>(b->offset, (size_t)n, b->mem, boffset);
  const int64_t *dwt = stage_array<int64_t>(b->write_time_ns, (size_t)n, b->mem, bwt);
  const int64_t *dct = stage_array<int64_t>(create_time_ns, (size_t)n, b->mem, bct);
  Buf status = dalloc_zero(16), nerr = dalloc_zero(16);
  { KernelTimer t("pp_check_batch", n); pp_check_batch<<<grid_for(n + 1, 256), 256, 0, st>>>(dstart, b->values_len, n, ptr<uint32_t>(status)); }
  {
    const uint32_t *hs = d2h_u32(status->p);
    tf::sync();
    if (*hs) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "message offsets must be ascending and inside the buffer");
  }

  // ---- framing → event spans --------------------------------------------------------------------------------------------------------------------------
  Buf nev = dalloc_zero((size_t)(na + 1) * 4 + 16), msg_state = dalloc_zero((size_t)na * 4 + 16);
  Frames fr{};
  fr.data = ptr<uint8_t>(vdata); fr.start = dstart; fr.nmsg = n; fr.pkg = h->pkg; fr.wrapper_number = h->wrapper_number;
  fr.nev = ptr<uint32_t>(nev); fr.msg_state = ptr<uint32_t>(msg_state); fr.nerr = ptr<uint32_t>(nerr);
  if (n) { KernelTimer t("pp_frames_count", (int64_t)b->values_len); pp_frames<false><<<grid_for(n, 128), 128, 0, st>>>(fr); }
  // (the counts are summed in 64 bits before the 32-bit scan: 2^31 events and more are refused)
  Buf tot64 = dalloc_zero(16);
  sum_u32_segments_u64(ptr<uint32_t>(nev), n, 1, na + 1, ptr<unsigned long long>(tot64));
  exclusive_scan_u32(ptr<uint32_t>(nev), ptr<uint32_t>(nev), n, true);
  const uint32_t *htot = d2h_u32(tot64->p, 2);
  tf::sync();
  const uint64_t nev64 = (uint64_t)htot[0] | (uint64_t)htot[1] << 32;
  if (nev64 > 0x7FFFFFFFull) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "more than 2^31-1 events: split the batch");
  const int64_t ne = (int64_t)nev64, nea = std::max<int64_t>(ne, 1);
  if ((uint64_t)std::max(nf, 1) * (uint64_t)nea * 9ull >= (1ull << 40)) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "fields x events need 1 TiB of records: split the batch");
  Buf ev_start = dalloc((size_t)nea * 4 + 16), ev_len = dalloc((size_t)nea * 4 + 16), ev_msg = dalloc((size_t)nea * 4 + 16), ev_idx = dalloc((size_t)nea * 4 + 16);
  Buf ev_code = dalloc_zero((size_t)nea + 16), ev_col = dalloc((size_t)nea * 4 + 16);
  fr.ev_start = ptr<uint32_t>(ev_start); fr.ev_len = ptr<uint32_t>(ev_len); fr.ev_msg = ptr<uint32_t>(ev_msg); fr.ev_idx = ptr<uint32_t>(ev_idx); fr.ev_code = ptr<uint8_t>(ev_code);
  if (n && ne) { KernelTimer t("pp_frames_write", (int64_t)b->values_len); pp_frames<true><<<grid_for(n, 128), 128, 0, st>>>(fr); }

  // ---- the events ---------------------------------------------------------------------------------------------------------------------------------------
  std::vector<DMember> members = h->members;
  if (members.empty()) members.push_back(DMember{0, 0, 0, 0});
  std::vector<DField> fields = h->fields;
  std::vector<uint32_t> fflags = h->fflags;
  if (fields.empty()) { fields.push_back(DField{}); fflags.push_back(0); }
  std::vector<int16_t> lut(1024, (int16_t)-1);
  for (int j = 0; j < nf; j++) if (h->fields[(size_t)j].number >= 0 && h->fields[(size_t)j].number < (int32_t)lut.size()) lut[(size_t)h->fields[(size_t)j].number] = (int16_t)j;
  std::vector<int32_t> req;
  for (int j = 0; j < ncol; j++) {
    const Col &c = h->cols[(size_t)j];
    if (c.field >= 0 && !c.extra && (c.flags & TFGPU_COL_REQUIRED) && (h->fflags[(size_t)c.field] & PF_EXPLICIT)) { req.push_back(j); req.push_back(c.field); }
  }
  const int32_t none = 0;
  Buf bfields = upload_const(fields.data(), fields.size() * sizeof(DField)), bflags = upload_const(fflags.data(), fflags.size() * 4);
  Buf bmembers = upload_const(members.data(), members.size() * sizeof(DMember)), bnames = upload_const(h->names.data(), h->names.size());
  Buf blut = upload_const(lut.data(), lut.size() * 2), breq = req.empty() ? upload_const(&none, 4) : upload_const(req.data(), req.size() * 4);
  Buf rec = dalloc((size_t)std::max(nf, 1) * (size_t)nea * 8 + 16), present = dalloc((size_t)std::max(nf, 1) * (size_t)nea + 16);
  Params p{};
  p.data = ptr<uint8_t>(vdata);
  p.fields = ptr<DField>(bfields); p.fflags = ptr<uint32_t>(bflags); p.nfields = nf; p.members = ptr<DMember>(bmembers); p.names = ptr<uint8_t>(bnames);
  p.lut = ptr<int16_t>(blut); p.lutn = (int32_t)lut.size();
  p.ev_start = fr.ev_start; p.ev_len = fr.ev_len; p.ev_msg = fr.ev_msg; p.ev_idx = fr.ev_idx; p.ev_code = fr.ev_code; p.ev_col = ptr<int32_t>(ev_col); p.nev = ne;
  p.rec = ptr<uint64_t>(rec); p.present = ptr<uint8_t>(present); p.msg_state = fr.msg_state; p.nerr = fr.nerr;
  p.req = ptr<int32_t>(breq); p.nreq = (int32_t)(req.size() / 2);
  p.pkg = h->pkg; p.nfe = h->not_fill_empty ? 1 : 0; p.schema_code = h->code;
  if (ne) { KernelTimer t("pp_decode", (int64_t)b->values_len); pp_decode<<<grid_for(ne, 128), 128, 0, st>>>(p); }
  Buf nfin = dalloc_zero((size_t)(na + 1) * 4 + 16), keep = dalloc_zero((size_t)(nea + 1) * 4 + 16);
  if (n) pp_msg_final<<<grid_for(n, 256), 256, 0, st>>>(ptr<uint32_t>(nev), fr.msg_state, n, ptr<uint32_t>(nfin));
  exclusive_scan_u32(ptr<uint32_t>(nfin), ptr<uint32_t>(nfin), n, true);  // → event_base
  if (ne) pp_keep<<<grid_for(ne, 256), 256, 0, st>>>(p, ptr<uint32_t>(keep));
  exclusive_scan_u32(ptr<uint32_t>(keep), ptr<uint32_t>(keep), ne, true);
  const uint32_t *hrows = d2h_u32(ptr<uint32_t>(keep) + ne), *hnerr = d2h_u32(p.nerr);
  tf::sync();
  const int64_t nrows = *hrows, nra = std::max<int64_t>(nrows, 1);
  const uint32_t nerr_total = *hnerr;

  // ---- the rows -----------------------------------------------------------------------------------------------------------------------------------------
  auto db = std::make_unique<tfgpu_dbatch>();
  db->nrows = nrows; db->table = topic;
  db->src_row = dalloc((size_t)nra * 4); db->part_id = dalloc((size_t)nra * 4);
  Buf row_ev = dalloc((size_t)nra * 4 + 16), host_rows = dalloc_zero((size_t)(nra + 1) * 4 + 16);
  p.row_ev = ptr<uint32_t>(row_ev); p.nrows = nrows;
  if (ne && nrows) pp_rows<<<grid_for(ne, 256), 256, 0, st>>>(p, ptr<uint32_t>(keep), ptr<uint32_t>(nfin), ptr<uint32_t>(row_ev), ptr<int32_t>(db->src_row), ptr<uint32_t>(db->part_id));
  std::vector<OutCol> oc((size_t)std::max(ncol, 1));
  std::memset(oc.data(), 0, oc.size() * sizeof(OutCol));
  std::vector<int32_t> text_cols, light_cols, any_cols, wide_cols;
  auto is_any = [&](const Col &c) { return c.field >= 0 && (h->fields[(size_t)c.field].repeated || h->fields[(size_t)c.field].ptype == TFGPU_PB_MESSAGE); };
  auto is_wide = [&](const Col &c) { const DField &f = h->fields[(size_t)c.field]; return f.repeated == 2 || (f.repeated && f.ptype == TFGPU_PB_MESSAGE); };
  int ntext = 0;
  bool has_any = false;
  for (auto &c : h->cols) if (c.field >= 0) { const int t = h->fields[(size_t)c.field].ptype; if (is_any(c) || t == TFGPU_PB_STRING || t == TFGPU_PB_BYTES) ntext++; if (is_any(c)) has_any = true; }
  TextSegments text(ntext, nrows);
  const ValidityBlock valid(ncol, nrows);
  Aux ax{};
  ax.row_ev = p.row_ev; ax.ev_msg = p.ev_msg; ax.ev_idx = p.ev_idx; ax.nrows = nrows; ax.offset = doffset; ax.wt = dwt; ax.ct = dct;
  bool has_aux = false;
  int ti = 0;
  for (int j = 0; j < ncol; j++) {
    const Col &c = h->cols[(size_t)j];
    DColumn d;
    d.name = c.name; d.dtype = c.dtype;
    OutCol &o = oc[(size_t)j];
    o.field = std::max(c.field, 0); o.nfe_top = h->not_fill_empty && !c.extra ? 1 : 0;
    auto fixed = [&](int repr, size_t w) { d.repr = repr; d.values = dalloc((size_t)nra * w + 8); o.values = d.values->p; };
    if (c.field < 0) {
      has_aux = has_aux || c.aux != AUX_PARTITION;
      switch (c.aux) {
        case AUX_PARTITION: {
          d.repr = TFGPU_R_STRING;
          d.data_len = (uint64_t)nrows * partition_text.size();
          if (text_total_exceeds(d.data_len)) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column _partition holds 4 GiB of text or more: split the batch");
          d.offsets = dalloc((size_t)(nrows + 1) * 4 + 16); d.data = dalloc((size_t)d.data_len + 16);
          Buf bt = upload_const(partition_text.data(), partition_text.size());
          pp_const_text<<<grid_for(std::max<int64_t>(nrows + 1, (int64_t)d.data_len), 256), 256, 0, st>>>(ptr<uint8_t>(bt), (uint32_t)partition_text.size(), nrows, ptr<uint32_t>(d.offsets), ptr<uint8_t>(d.data));
          break;
        }
        case AUX_OFFSET: fixed(TFGPU_R_UINT64, 8); ax.col_offset = (uint64_t *)o.values; break;
        case AUX_IDX: fixed(TFGPU_R_UINT64, 8); ax.col_idx = (uint64_t *)o.values; break;
        case AUX_CTIME: fixed(TFGPU_R_TIME, 8); d.nanos = dalloc((size_t)nra * 4 + 8); ax.ct_sec = (int64_t *)o.values; ax.ct_nsec = ptr<int32_t>(d.nanos); break;
        default: fixed(TFGPU_R_TIME, 8); d.nanos = dalloc((size_t)nra * 4 + 8); ax.wt_sec = (int64_t *)o.values; ax.wt_nsec = ptr<int32_t>(d.nanos); break;
      }
    } else if (is_any(c)) { d.repr = TFGPU_R_JSON; (is_wide(c) ? wide_cols : any_cols).push_back(j); }
    else {
      light_cols.push_back(j);
      switch (h->fields[(size_t)c.field].ptype) {  // extractLeafValue's Go types
        case TFGPU_PB_DOUBLE: fixed(TFGPU_R_FLOAT64, 8); break;
        case TFGPU_PB_FLOAT: fixed(TFGPU_R_FLOAT32, 4); break;
        case TFGPU_PB_INT64: case TFGPU_PB_SFIXED64: case TFGPU_PB_SINT64: fixed(TFGPU_R_INT64, 8); break;
        case TFGPU_PB_UINT64: case TFGPU_PB_FIXED64: fixed(TFGPU_R_UINT64, 8); break;
        case TFGPU_PB_INT32: case TFGPU_PB_SFIXED32: case TFGPU_PB_SINT32: case TFGPU_PB_ENUM: fixed(TFGPU_R_INT32, 4); break;  // EnumNumber → int32
        case TFGPU_PB_UINT32: case TFGPU_PB_FIXED32: fixed(TFGPU_R_UINT32, 4); break;
        case TFGPU_PB_BOOL: fixed(TFGPU_R_BOOL, 1); break;
        case TFGPU_PB_STRING: d.repr = TFGPU_R_STRING; break;
        case TFGPU_PB_BYTES: d.repr = TFGPU_R_BYTES; break;
        default: return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_parse: bad field type");  // (a foreign column: h->code sent every event to the host)
      }
    }
    if (c.field >= 0 && !d.values) {
      d.offsets = text.offsets(ti);
      o.lens = text.seg(ti);
      text_cols.push_back(j);
      ti++;
    }
    if (c.field >= 0) { d.validity = valid.col(j); o.validity = ptr<uint8_t>(d.validity); }
    db->schema.push_back({d.name, d.dtype});
    if (c.flags & TFGPU_COL_KEY) db->key_names.push_back(c.name);
    db->cols.push_back(std::move(d));
  }
  Buf boc = upload_small(oc.data(), oc.size() * sizeof(OutCol));
  if (nrows) {
    if (has_aux) { KernelTimer t("pp_aux", nrows); pp_aux<<<grid_for(nrows, 256), 256, 0, st>>>(ax); }
    KernelTimer t("pp_cells", nrows);
    auto list = [&](const std::vector<int32_t> &v) { return upload_small(v.data(), v.size() * 4); };
    if (!light_cols.empty()) { Buf l = list(light_cols); pp_cells<false><<<dim3(grid_for(nrows, 256), (unsigned)light_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l), ptr<uint32_t>(host_rows)); }
    if (!any_cols.empty()) { Buf l = list(any_cols); pp_cells<true><<<dim3(grid_for(nrows, 256), (unsigned)any_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l), ptr<uint32_t>(host_rows)); }
    if (!wide_cols.empty()) { Buf l = list(wide_cols); pp_cells<true, true><<<dim3(grid_for(nrows, 256), (unsigned)wide_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l), ptr<uint32_t>(host_rows)); }
  }
  if (ntext) {
    text.scan(true);
    tf::sync();
    for (int t = 0; t < ntext; t++) {
      const uint64_t bytes = text.total(t);
      DColumn &d = db->cols[(size_t)text_cols[(size_t)t]];
      if (text_total_exceeds(bytes)) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column " + d.name + " holds 4 GiB of text or more: split the batch");
      d.data_len = bytes;
      d.data = dalloc((size_t)d.data_len + 16);
      oc[(size_t)text_cols[(size_t)t]].data = ptr<uint8_t>(d.data);
    }
    boc = upload_small(oc.data(), oc.size() * sizeof(OutCol));
    if (nrows) {
      KernelTimer t("pp_text", nrows);
      std::vector<int32_t> copy_cols;
      for (int32_t j : text_cols) if (!is_any(h->cols[(size_t)j])) copy_cols.push_back(j);
      auto list = [&](const std::vector<int32_t> &v) { return upload_small(v.data(), v.size() * 4); };
      if (!copy_cols.empty()) { Buf l = list(copy_cols); pp_text_copy<<<dim3(grid_for(nrows, 256), (unsigned)copy_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l)); }
      if (!any_cols.empty()) { Buf l = list(any_cols); pp_text_any<false><<<dim3(grid_for(nrows, 256), (unsigned)any_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l)); }
      if (!wide_cols.empty()) { Buf l = list(wide_cols); pp_text_any<true><<<dim3(grid_for(nrows, 256), (unsigned)wide_cols.size()), 256, 0, st>>>(p, ptr<OutCol>(boc), ptr<int32_t>(l)); }
    }
  }

  // ---- rows for the host (a NaN / Inf inside an `any`, −0.0 under NotFillEmptyFields), the failed events ------------------------------------------------
  std::unique_ptr<tfgpu_dbatch> result = std::move(db);
  std::vector<uint32_t> host_events;
  if (nrows && (has_any || h->not_fill_empty)) host_events = split_host_rows(result, host_rows, row_ev, nrows);
  std::vector<uint32_t> hbase((size_t)n + 1, 0u);
  if (event_base || nerr_total || !host_events.empty()) {
    if (n) d2h(hbase.data(), nfin->p, (size_t)(n + 1) * 4);
    tf::sync();
    if (event_base) for (int64_t m = 0; m <= n; m++) event_base[m] = hbase[(size_t)m];
  }
  int64_t nu = 0;
  if (nerr_total || !host_events.empty()) {
    std::vector<uint32_t> hs((size_t)nea), hl((size_t)nea), hm((size_t)nea), hi((size_t)nea), hstate((size_t)na), hscan((size_t)n + 1, 0u), hstart32;
    std::vector<uint8_t> hc((size_t)nea);
    std::vector<int32_t> hcol((size_t)nea);
    std::vector<uint64_t> hstart((size_t)n + 1, 0ull);
    if (ne) {
      d2h(hs.data(), ev_start->p, (size_t)ne * 4); d2h(hl.data(), ev_len->p, (size_t)ne * 4); d2h(hm.data(), ev_msg->p, (size_t)ne * 4); d2h(hi.data(), ev_idx->p, (size_t)ne * 4);
      d2h(hc.data(), ev_code->p, (size_t)ne); d2h(hcol.data(), ev_col->p, (size_t)ne * 4);
    }
    if (n) { d2h(hstate.data(), msg_state->p, (size_t)n * 4); d2h(hscan.data(), nev->p, (size_t)(n + 1) * 4); d2h(hstart.data(), dstart, (size_t)(n + 1) * 8); }
    tf::sync();
    for (uint32_t e : host_events) { hc[e] = (uint8_t)TFGPU_ROW_HOST_FALLBACK; hcol[e] = -1; }
    auto add = [&](int64_t event, int64_t m, uint64_t start, uint32_t len, int32_t idx, int32_t code, int32_t col) {
      if (unparsed && nu < cap) unparsed[nu] = tfgpu_proto_unparsed{event, m, start, len, idx, code, col};
      nu++;
    };
    for (int64_t m = 0; m < n; m++) {
      if (hstate[(size_t)m]) {  // the message as one event: the wrapper fails (Counter 1), or the host takes it whole
        const bool fails = hstate[(size_t)m] == 2;
        add(hbase[(size_t)m], m, hstart[(size_t)m], (uint32_t)(hstart[(size_t)m + 1] - hstart[(size_t)m]), fails ? 1 : 0, fails ? TFGPU_ROW_PROTO_WRAPPER : TFGPU_ROW_HOST_FALLBACK, -1);
        continue;
      }
      for (uint32_t e = hscan[(size_t)m]; e < hscan[(size_t)m + 1]; e++)
        if (hc[e]) add((int64_t)hbase[(size_t)m] + hi[e] - 1, m, hs[e], hl[e], (int32_t)hi[e], hc[e], hc[e] == TFGPU_ROW_PROTO_REQUIRED ? hcol[e] : -1);
    }
  }
  if (nunparsed) *nunparsed = nu;
  tf::sync();  // (the staged copies of the batch go back to the pool behind the kernels that read them)
  *out = result.release();
  return TFGPU_OK;
  TF_API_END
}
