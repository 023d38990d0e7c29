// tf_pbwire.hpp — the protobuf wire walk and the `any` emitters both protobuf front ends share: the Confluent-SR branch (tf_protobuf.hip, schema from
// .proto text) and the generic protobuf parser (tf_protoparse.hip, schema from a FileDescriptorSet).  Both compile their schema into the same field
// table (DField / DMember); the emitters read it through any struct P that has `data`, `members` and `names`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tf_common.hpp"
#include "tf_devfloat.hpp"
#include "tf_devparse.hpp"
#include "tf_emit.hpp"
#include "tf_pbfields.hpp"

namespace tf {
namespace pbd {

constexpr uint32_t MAP_MAX_ENTRIES = 32;   // a map field with more entries than this is the stock code's (TFGPU_ROW_HOST_FALLBACK): the emitter below is quadratic in them
__device__ __forceinline__ int want_wt(int t) {
  switch (t) {
    case TFGPU_PB_DOUBLE: case TFGPU_PB_FIXED64: case TFGPU_PB_SFIXED64: return 1;
    case TFGPU_PB_FLOAT: case TFGPU_PB_FIXED32: case TFGPU_PB_SFIXED32: return 5;
    case TFGPU_PB_STRING: case TFGPU_PB_BYTES: case TFGPU_PB_MESSAGE: return 2;
    default: return 0;
  }
}
// a base-128 varint at [i, end): false = truncated / longer than ten bytes (proto.DecodeVarint's errors).  Bytes come through MemBytes'
// 8-byte window: one load per eight bytes of a message instead of one per byte.
__device__ __forceinline__ bool varint(MemBytes &rd, uint32_t &i, uint32_t end, uint64_t *v) {
  uint64_t x = 0;
  for (uint32_t s = 0; s < 70; s += 7) {
    if (i >= end) return false;
    const uint32_t c = rd.at(i++);
    x |= (uint64_t)(c & 0x7Fu) << s;   // (bits beyond 64 fall off: Go's uint64 shift does the same)
    if (!(c & 0x80u)) { *v = x; return true; }
  }
  return false;
}
__device__ __forceinline__ uint64_t le(MemBytes &rd, uint32_t i, int n) { return rd.bytes(i, n); }  // never past the word holding the value's last byte

// One message's fields over [a, z): calls on(number, wire type, raw value or start, len) for every field; 0 ok, 1 does not unmarshal, 2 host
template <class F> __device__ int walk(MemBytes &d, uint32_t a, uint32_t z, F on) {
  uint32_t i = a;
  while (i < z) {
    uint64_t tag;
    if (!varint(d, i, z, &tag)) return 1;
    const uint32_t wt = (uint32_t)tag & 7u;
    const uint64_t num = tag >> 3;
    if (num == 0 || num > 536870911ull) return 2;   // field number 0 / beyond 2^29 - 1: what the reference's decoder makes of it is not pinned
    uint64_t raw = 0; uint32_t len = 0;
    if (wt == 0) { if (!varint(d, i, z, &raw)) return 1; }
    else if (wt == 1) { if (z - i < 8) return 1; raw = le(d, i, 8); i += 8; }
    else if (wt == 5) { if (z - i < 4) return 1; raw = le(d, i, 4); i += 4; }
    else if (wt == 2) { uint64_t n; if (!varint(d, i, z, &n)) return 1; if (n > (uint64_t)(z - i)) return 1; raw = i; len = (uint32_t)n; i += (uint32_t)n; }
    else return 2;  // groups (and the reserved wire types: an error in one library, skipped by another — the stock code decides)
    const int r = on((uint32_t)num, wt, raw, len);
    if (r) return r;
  }
  return 0;
}

// the Go value of a scalar occurrence (unpackNotRepeatedVal's type assertions: int32 / int64 / uint32 / uint64 / float32 / float64 / bool)
__device__ __forceinline__ int64_t as_i64(int t, uint64_t raw) {
  switch (t) {
    case TFGPU_PB_INT32: case TFGPU_PB_ENUM: case TFGPU_PB_SFIXED32: return (int64_t)(int32_t)(uint32_t)raw;
    case TFGPU_PB_SINT32: { const uint32_t v = (uint32_t)raw; return (int64_t)(int32_t)((v >> 1) ^ (0u - (v & 1u))); }
    case TFGPU_PB_SINT64: return (int64_t)((raw >> 1) ^ (0ull - (raw & 1ull)));
    case TFGPU_PB_UINT32: case TFGPU_PB_FIXED32: return (int64_t)(uint32_t)raw;
    case TFGPU_PB_BOOL: return raw != 0;
    default: return (int64_t)raw;  // int64, sfixed64, uint64, fixed64: the bits
  }
}

// json.Marshal of one member's value.  false: NaN / Inf (json.Marshal fails: host)
template <class S> __device__ bool emit_member(S &s, const uint8_t *d, int t, bool present, uint64_t raw) {
  switch (t) {
    case TFGPU_PB_STRING: emit_json_string(s, d + (present ? (uint32_t)raw : 0u), present ? (uint32_t)(raw >> 32) : 0u, false); return true;
    case TFGPU_PB_BYTES: s.put('"'); emit_base64(s, d + (present ? (uint32_t)raw : 0u), present ? (uint32_t)(raw >> 32) : 0u); s.put('"'); return true;
    case TFGPU_PB_BOOL: { const char *w = present && raw ? "true" : "false"; while (*w) s.put((uint8_t)*w++); return true; }
    case TFGPU_PB_DOUBLE: case TFGPU_PB_FLOAT: {
      double v = 0;
      if (present) { if (t == TFGPU_PB_DOUBLE) v = __longlong_as_double((long long)raw); else v = (double)__uint_as_float((uint32_t)raw); }
      if (v != v || v == INFINITY || v == -INFINITY) return false;
      dev::fmt_json_float(s, v, t == TFGPU_PB_DOUBLE ? 64 : 32);
      return true;
    }
    case TFGPU_PB_UINT64: case TFGPU_PB_FIXED64: emit_u64(s, present ? raw : 0ull); return true;
    default: emit_i64(s, present ? as_i64(t, raw) : 0); return true;
  }
}
// a message field's map: {"name":value,…} over ALL its members in name order (the host sorted them), the last occurrence of each.
// (One walk of the field's bytes per member.  Collecting up to eight members' values in ONE walk — values in registers, unrolled loops —
//  was measured: pb_text 0.68 -> 1.08 ms on the reference's 60-column message, profiles/r08l_*; the walks are short and the registers dear.)
template <class S, class P> __device__ bool emit_message(S &s, const P &p, const DField &fd, uint32_t a, uint32_t len) {
  const uint8_t *d = p.data;
  MemBytes rd(p.data);
  s.put('{');
  for (int k = 0; k < fd.nmem; k++) {
    const DMember &mb = p.members[fd.mem_off + k];
    bool present = false; uint64_t raw = 0;
    walk(rd, a, a + len, [&](uint32_t n2, uint32_t w2, uint64_t r2, uint32_t l2) { if ((uint32_t)mb.number == n2) { present = true; raw = w2 == 2 ? (r2 | ((uint64_t)l2 << 32)) : r2; } return 0; });
    if (k) s.put(',');
    emit_json_string(s, p.names + mb.name_off, mb.name_len, false);
    s.put(':');
    if (!emit_member(s, d, mb.ptype, present, raw)) return false;
  }
  s.put('}');
  return true;
}

// a repeated field's []interface{}: the elements of every occurrence in wire order, packed runs unrolled.  false: a NaN / Inf element
// MSG: the instantiation that takes element MESSAGES too (the wide kernels below)
template <bool MSG, class S, class P> __device__ bool emit_array(S &s, const P &p, const DField &fd, uint32_t a, uint32_t z) {
  const uint8_t *d = p.data;
  MemBytes rd(p.data);
  const int ew = want_wt(fd.ptype);
  bool first = true, ok = true;
  s.put('[');
  walk(rd, a, z, [&](uint32_t num, uint32_t wt, uint64_t raw, uint32_t len) {
    if (num != (uint32_t)fd.number) return 0;
    if constexpr (MSG) if (fd.ptype == TFGPU_PB_MESSAGE) {  // an element message: its map, as a singular message field's (unpackRepeatedVal → unpackNotRepeatedVal over *dynamic.Message)
      if (!first) s.put(',');
      first = false;
      if (!emit_message(s, p, fd, (uint32_t)raw, len)) ok = false;
      return 0;
    }
    auto one = [&](uint64_t r) { if (!first) s.put(','); first = false; if (!emit_member(s, d, fd.ptype, true, r)) ok = false; };
    if ((int)wt == ew) one(wt == 2 ? (raw | ((uint64_t)len << 32)) : raw);
    else {  // packed (pb_decode let nothing else through)
      uint32_t q = (uint32_t)raw; const uint32_t qe = q + len;
      while (q < qe) {
        uint64_t v = 0;
        if (ew == 0) { if (!varint(rd, q, qe, &v)) break; }
        else { const int w = ew == 1 ? 8 : 4; v = le(rd, q, w); q += (uint32_t)w; }
        one(v);
      }
    }
    return 0;
  });
  s.put(']');
  return ok;
}

// a map<string, V> field's map[string]interface{} (types_protobuf.go:57-71) as json.Marshal writes it: keys in byte order, the LAST entry of a key
// (protobuf's map semantics), an entry without a key / value member under "" / the zero value.  No scratch list of the entries: the smallest key
// above the one just written is found by one scan of the field's occurrences a key (<= MAP_MAX_ENTRIES entries: pb_decode counted them).
struct MapKey { uint32_t at, len; };
__device__ __forceinline__ int key_cmp(const uint8_t *d, MapKey a, MapKey b) {
  const uint32_t n = min(a.len, b.len);
  for (uint32_t i = 0; i < n; i++) { const int x = (int)d[a.at + i] - (int)d[b.at + i]; if (x) return x; }
  return (a.len > b.len) - (a.len < b.len);
}
template <class S, class P> __device__ bool emit_map(S &s, const P &p, const DField &fd, uint32_t a, uint32_t z) {
  const uint8_t *d = p.data;
  MemBytes rd(p.data);
  const int vt = p.members[fd.mem_off + 1].ptype;
  bool ok = true, have_prev = false, first = true;
  MapKey prev{0, 0};
  s.put('{');
  for (uint32_t round = 0; round <= MAP_MAX_ENTRIES; round++) {
    bool found = false; MapKey best{0, 0}; bool vpresent = false; uint64_t vraw = 0;
    walk(rd, a, z, [&](uint32_t num, uint32_t wt, uint64_t raw, uint32_t len) {
      if (num != (uint32_t)fd.number || wt != 2) return 0;
      MapKey k{0, 0}; bool vp = false; uint64_t vr = 0;
      walk(rd, (uint32_t)raw, (uint32_t)raw + len, [&](uint32_t n2, uint32_t w2, uint64_t r2, uint32_t l2) {
        if (n2 == 1 && w2 == 2) k = MapKey{(uint32_t)r2, l2};
        else if (n2 == 2) { vp = true; vr = w2 == 2 ? (r2 | ((uint64_t)l2 << 32)) : r2; }
        return 0;
      });
      if (have_prev && key_cmp(d, k, prev) <= 0) return 0;          // written already (or a duplicate of one that was)
      const int c = found ? key_cmp(d, k, best) : -1;
      if (c <= 0) { found = true; best = k; vpresent = vp; vraw = vr; }  // a smaller key, or a LATER entry of the same one: the last one wins
      return 0;
    });
    if (!found) break;
    if (!first) s.put(',');
    first = false;
    emit_json_string(s, d + best.at, best.len, false);
    s.put(':');
    if (!emit_member(s, d, vt, vpresent, vraw)) ok = false;
    prev = best; have_prev = true;
  }
  s.put('}');
  return ok;
}

}  // namespace pbd
}  // namespace tf
