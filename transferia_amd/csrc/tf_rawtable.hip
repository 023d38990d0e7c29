// tf_rawtable.hip — the raw_to_table parser on device (pkg/parsers/registry/raw_to_table/engine/parser.go, pkg/util/raw_to_table_common,
// pkg/util/dlq_maker/queue_dlq_maker): a Kafka / YDS message batch becomes rows  topic, partition, offset[, timestamp][, headers][, key], value  of the
// main table; a message whose key / value does not fit the configured type (string: utf8.Valid, JSON: json.Valid) becomes a row of the dead-letter
// table instead, with key and value as bytes and the reason as text.
//
//   rawtt_check_batch     the batch's own offsets: ascending, inside their buffers (nothing below reads a byte before this has passed)
//   rawtt_utf8_valid      utf8.Valid per message: a lane per message below RAWTT_LONG_BYTES, the wave together over RAWTT_CHUNK_BYTES chunks above
//   rawtt_json_check      json.Valid per message (skip_value + only white space behind it), the top-level type and any_keys_order's answer
//   rawtt_split_flags     reason code (4 bits) -> keep flags of the two tables; (scan: exclusive_scan_u32_segments); rawtt_rows: the two row lists
//   rawtt_fixed           offset, partition, timestamp and the lengths of the byte cells, lane = row
//   rawtt_validity        the nil bitmaps of key / value
//   rawtt_any_len/_write  `any` cells: json.Marshal of the decoded value, <false> emit_any, <true> emit_any_canon (launched when some value needs it)
//   rawtt_headers<COUNT>  json.Marshal(map[string]string): keys ascending by selection, `null` for a nil map
//   rawtt_copy_cells      byte cells (key / value / failure_reason) through the segmented copy (tf_segcopy.hpp)
//   rawtt_topic           one constant repeated
//
// The JSON scanner with its container stacks lives in rawtt_json_check and rawtt_any_* only, which a config without a JSON-typed key or value never
// launches (the third compiler trap).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "tf_plan.hpp"
#include "tf_ingest.hpp"
#include "tf_devrow.hpp"
#include "tf_devfmt.hpp"
#include "tf_jsonscan.hpp"
#include "tf_segcopy.hpp"
#include "tf_utf8.hpp"

#define RAWTT_CHUNK_BYTES 64    // what one lane of the wave validator takes of a long message per step
#define RAWTT_LONG_BYTES 1024   // messages of this many bytes and more are validated by the wave together

struct tfgpu_raw_to_table {
  std::string table_name, dlq_suffix;
  bool key = false, ts = false, headers = false;
  int key_type = 0, value_type = 0;  // RT_BYTES / RT_STRING / RT_JSON
};

namespace tf {
namespace rawtt {

enum { RT_BYTES = 0, RT_STRING = 1, RT_JSON = 2 };
enum : uint32_t { R_KEY_UTF8 = 1u, R_KEY_JSON = 2u, R_VAL_UTF8 = 4u, R_VAL_JSON = 8u, R_MASK = 15u, R_FALLBACK = 0x80u };
enum : uint32_t { ST_BAD_OFFSETS = 1u, ST_CANON = 2u, ST_FALLBACK = 4u };
constexpr uint32_t INFO_CANON = 0x40u;  // beside the sr::VT_* type of the top-level value

struct Bytes {  // one of the batch's three byte buffers with its per-message ranges
  const uint8_t *data;    // padded copy in HBM, 8-byte aligned
  const uint64_t *start;  // [n + 1]
  const uint8_t *nil;     // bitmap or null
  uint64_t len;
};
__device__ __forceinline__ bool bit_of(const uint8_t *bm, int64_t i) { return bm && ((bm[i >> 3] >> (i & 7)) & 1); }

__global__ void __launch_bounds__(256) rawtt_check_batch(Bytes v, Bytes k, const uint64_t *pair_start, const tfgpu_header_pair *pairs, int64_t npairs, uint64_t hlen, int64_t n,
                                                         uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i <= n) {
    if (v.start[i] > v.len || (i < n && v.start[i] > v.start[i + 1])) bad = true;
    if (k.start && (k.start[i] > k.len || (i < n && k.start[i] > k.start[i + 1]))) bad = true;
    if (pair_start && (pair_start[i] > (uint64_t)npairs || (i < n && pair_start[i] > pair_start[i + 1]))) bad = true;
  }
  if (i < npairs) {
    const tfgpu_header_pair p = pairs[i];
    if ((uint64_t)p.key_off + p.key_len > hlen || (uint64_t)p.val_off + p.val_len > hlen) bad = true;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, (uint32_t)ST_BAD_OFFSETS);
}

// ---- utf8.Valid ------------------------------------------------------------------------------------------------------------------------------------
// Where the walk of chunk [cs, ..) starts, given that the bytes in front of it are valid (if they are not, the lane in front says so): behind the
// sequence that starts in the last three bytes of the chunk in front and reaches across cs.  cs - 3 >= the message's start.
__device__ __forceinline__ uint32_t utf8_chunk_start(MemBytes &rd, const uint32_t cs) {
  for (uint32_t k = 1; k <= 3; k++) {
    const uint32_t b = rd.at(cs - k);
    if (b >= 0x80 && b <= 0xBF) continue;
    const uint32_t need = b >= 0xF0 ? 3u : b >= 0xE0 ? 2u : b >= 0xC0 ? 1u : 0u;  // (an invalid lead is the other lane's finding)
    return need >= k ? cs - k + need + 1 : cs;
  }
  return cs;
}
// 64 messages a wave.  A short message is its lane's; then the wave takes the long ones among its 64 one after another, lane j of step t validating
// chunk 64 t + j.  `reason[m] |= bit` where the bytes are not valid UTF-8 (a nil message is valid: utf8.Valid(nil)).
__global__ void __launch_bounds__(256) rawtt_utf8_valid(Bytes b, int64_t n, uint32_t long_bytes, uint8_t *reason, uint32_t bit) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  uint32_t s = 0, e = 0;
  if (m < n && !bit_of(b.nil, m)) { s = (uint32_t)b.start[m]; e = (uint32_t)b.start[m + 1]; }
  MemBytes rd(b.data);
  const bool is_long = e - s >= long_bytes;
  bool ok = true;
  if (!is_long) ok = utf8_valid_range(rd, s, e, e);
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t ms = (uint32_t)__shfl((int)s, L), me = (uint32_t)__shfl((int)e, L);
    const uint32_t nchunk = (me - ms + RAWTT_CHUNK_BYTES - 1) / RAWTT_CHUNK_BYTES;
    bool good = true;
    for (uint32_t c = (uint32_t)lane; c < nchunk; c += 64) {
      const uint32_t cs = ms + c * RAWTT_CHUNK_BYTES, ce = me - cs > RAWTT_CHUNK_BYTES ? cs + RAWTT_CHUNK_BYTES : me;
      const uint32_t from = c ? utf8_chunk_start(rd, cs) : cs;
      if (from < ce && !utf8_valid_range(rd, from, ce, me)) good = false;
      else if (from > me) good = false;  // (a lead in front whose sequence the message's end cuts short: the lane in front reports it too)
    }
    const bool all_good = !__any(!good);
    if (lane == L) ok = all_good;
  }
  if (m < n && !ok) reason[m] |= (uint8_t)bit;
}

// ---- json.Valid, the top-level type, the key order ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(128) rawtt_json_check(Bytes b, int64_t n, uint8_t *reason, uint32_t bit, uint8_t *info, uint32_t *status) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  if (bit_of(b.nil, m)) { info[m] = (uint8_t)sr::VT_NULL; return; }  // `bytes != nil` guards the check: a nil cell
  const uint32_t s = (uint32_t)b.start[m], e = (uint32_t)b.start[m + 1];
  MemBytes rd(b.data);
  uint32_t pos = s, vt = 0;
  const int rc = sr::skip_value(rd, pos, e, vt);
  uint32_t flags = 0, r = 0, inf = vt & sr::VT_MASK;
  if (rc == 2) r = R_FALLBACK;
  else if (rc == 1) r = bit;
  else {
    while (pos < e && sr::is_ws(rd.at(pos))) pos++;
    if (pos != e) r = bit;  // checkValid: something behind the value
    else if (inf == sr::VT_OBJ || inf == sr::VT_ARR) {
      const int ord = sr::any_keys_order(rd, s, e - s);
      if (ord == 1) { inf |= INFO_CANON; flags |= ST_CANON; }
      else if (ord == 2) r = R_FALLBACK;
    }
  }
  info[m] = (uint8_t)inf;
  if (r) reason[m] |= (uint8_t)r;
  if (r == R_FALLBACK) flags |= ST_FALLBACK;
  if (flags & ~__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(status, flags);
}

// ---- the split --------------------------------------------------------------------------------------------------------------------------------------
// keep[0][m]: a main row, keep[1][m]: a dead-letter row; a message the device does not decide is in neither
__global__ void __launch_bounds__(256) rawtt_split_flags(const uint8_t *reason, int64_t n, uint32_t *keep, int64_t stride) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const uint32_t r = reason[m];
  keep[m] = r == 0 ? 1u : 0u;
  keep[stride + m] = (r & R_MASK) && !(r & R_FALLBACK) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) rawtt_rows(const uint8_t *reason, int64_t n, const uint32_t *scanned, int64_t stride, int32_t *rows_main, int32_t *rows_dlq, int32_t *codes) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const uint32_t r = reason[m];
  if (r == 0) rows_main[scanned[m]] = (int32_t)m;
  else if (!(r & R_FALLBACK)) rows_dlq[scanned[stride + m]] = (int32_t)m;
  if (codes) codes[m] = (r & R_FALLBACK) ? (int32_t)TFGPU_ROW_HOST_FALLBACK : (int32_t)TFGPU_ROW_OK;
}

// ---- the columns ---------------------------------------------------------------------------------------------------------------------------------------
struct Fixed {
  const int32_t *rows; int64_t nrows;
  const uint64_t *offset; const int64_t *wt;
  uint32_t partition;
  uint32_t *col_offset, *col_partition;
  int64_t *ts_sec; int32_t *ts_nsec;  // null without the timestamp column
  Bytes key, val;
  uint32_t *key_len, *val_len;        // null: no such byte column (absent, or an `any` column)
  const uint8_t *reason; const uint32_t *reason_off; uint32_t *reason_len;  // the dead-letter table's failure_reason
};
__global__ void __launch_bounds__(256) rawtt_fixed(Fixed f) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= f.nrows) return;
  const int64_t m = f.rows[r];
  f.col_offset[r] = f.offset ? (uint32_t)f.offset[m] : 0u;  // uint32(msg.Offset): truncating
  f.col_partition[r] = f.partition;
  if (f.ts_sec) {
    const int64_t t = f.wt ? f.wt[m] : 0, q = dev::floordiv(t, 1000000000ll);
    f.ts_sec[r] = q; f.ts_nsec[r] = (int32_t)(t - q * 1000000000ll);
  }
  if (f.key_len) f.key_len[r] = f.key.start && !bit_of(f.key.nil, m) ? (uint32_t)(f.key.start[m + 1] - f.key.start[m]) : 0u;
  if (f.val_len) f.val_len[r] = !bit_of(f.val.nil, m) ? (uint32_t)(f.val.start[m + 1] - f.val.start[m]) : 0u;
  if (f.reason_len) { const uint32_t c = f.reason[m] & R_MASK; f.reason_len[r] = f.reason_off[c + 1] - f.reason_off[c]; }
}
// bit r of the bitmap: the cell is not nil — the message has the key / value, and under JSON its top-level value is not `null`
__global__ void __launch_bounds__(256) rawtt_validity(const int32_t *rows, int64_t nrows, const uint8_t *nil, int absent, const uint8_t *info, uint8_t *bitmap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (nrows + 7) / 8) return;
  uint32_t v = 0;
  for (int q = 0; q < 8; q++) {
    const int64_t r = i * 8 + q;
    if (r >= nrows) break;
    const int64_t m = rows[r];
    if (!absent && !bit_of(nil, m) && !(info && (info[m] & sr::VT_MASK) == sr::VT_NULL)) v |= 1u << q;
  }
  bitmap[i] = (uint8_t)v;
}

// `any` cells.  CANON == false: the values whose objects hold their keys ascending; CANON == true: the others (a launch of its own, so that the
// kernel every cell runs through does not carry the sorting emitter's frames — as sr_cell_values / sr_cell_text)
template <bool CANON, class S> __device__ __forceinline__ void any_cell(S &s, const Bytes &b, const uint8_t *info, int64_t m) {
  const uint32_t inf = info[m];
  if ((inf & sr::VT_MASK) == sr::VT_NULL || ((inf & INFO_CANON) != 0) != CANON) return;
  MemBytes rd(b.data);
  uint32_t a = (uint32_t)b.start[m];
  const uint32_t e = (uint32_t)b.start[m + 1];
  if constexpr (CANON) {
    while (a < e && sr::is_ws(rd.at(a))) a++;
    sr::emit_any_canon(s, rd, a, e - a);
  } else sr::emit_any(s, rd, a, e - a);
}
template <bool CANON> __global__ void __launch_bounds__(256) rawtt_any_len(Bytes b, const uint8_t *info, const int32_t *rows, int64_t nrows, uint32_t *len) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const int64_t m = rows[r];
  if (CANON && !(info[m] & INFO_CANON)) return;
  sr::CountSink s;
  any_cell<CANON>(s, b, info, m);
  if (CANON || !(info[m] & INFO_CANON)) len[r] = s.n;
}
template <bool CANON> __global__ void __launch_bounds__(256) rawtt_any_write(Bytes b, const uint8_t *info, const int32_t *rows, int64_t nrows, const uint32_t *off, uint8_t *data) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  sr::ByteSink s{data + off[r]};
  any_cell<CANON>(s, b, info, rows[r]);
  s.flush();
}

// json.Marshal(string) of a Go string's bytes: appendString with escapeHTML.  Unlike a string DECODED from JSON (emit_go_string: unquote has made
// every invalid byte a real U+FFFD already), a byte that is no UTF-8 here is written as the six-character escape of U+FFFD
template <class S> __device__ __forceinline__ void emit_go_plain(S &o, const uint8_t *base, uint32_t a, uint32_t e) {
  o.put('"');
  for (uint32_t p = a; p < e;) {
    uint32_t c = base[p];
    if (c >= 0x80) {  // utf8.DecodeRuneInString
      uint32_t need = 0, cp = 0, lo = 0x80, hi = 0xBF;
      if (c >= 0xC2 && c <= 0xDF) { need = 1; cp = c & 0x1F; }
      else if (c >= 0xE0 && c <= 0xEF) { need = 2; cp = c & 0x0F; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
      else if (c >= 0xF0 && c <= 0xF4) { need = 3; cp = c & 0x07; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
      bool ok = need > 0 && e - p > need;
      if (ok) for (uint32_t k = 1; k <= need; k++) {
        const uint32_t d = base[p + k], l = k == 1 ? lo : 0x80u, h = k == 1 ? hi : 0xBFu;
        if (d < l || d > h) { ok = false; break; }
        cp = (cp << 6) | (d & 0x3F);
      }
      if (!ok) { sr::put_hex4(o, 0xFFFD); p++; continue; }
      p += need + 1;
      c = cp;
    } else p++;
    if (c < 0x80) {
      if (c >= 0x20 && c != '"' && c != '\\' && c != '<' && c != '>' && c != '&') { o.put(c); continue; }
      switch (c) {
        case '"': o.put('\\'); o.put('"'); break; case '\\': o.put('\\'); o.put('\\'); break; case '\b': o.put('\\'); o.put('b'); break;
        case '\f': o.put('\\'); o.put('f'); break; case '\n': o.put('\\'); o.put('n'); break; case '\r': o.put('\\'); o.put('r'); break;
        case '\t': o.put('\\'); o.put('t'); break;
        default: sr::put_hex4(o, c);
      }
    } else if (c == 0x2028 || c == 0x2029) sr::put_hex4(o, c);
    else sr::put_utf8(o, c);
  }
  o.put('"');
}
struct Headers {
  const uint8_t *data; const uint64_t *pair_start; const tfgpu_header_pair *pairs; const uint8_t *nil;
  const int32_t *rows; int64_t nrows;
  uint32_t *len; const uint32_t *off; uint8_t *out;
};
__device__ __forceinline__ int key_cmp(const uint8_t *d, const tfgpu_header_pair &x, const tfgpu_header_pair &y) {  // Go's string order: bytes
  const uint32_t n = x.key_len < y.key_len ? x.key_len : y.key_len;
  for (uint32_t i = 0; i < n; i++) { const uint32_t a = d[x.key_off + i], b = d[y.key_off + i]; if (a != b) return a < b ? -1 : 1; }
  return x.key_len < y.key_len ? -1 : x.key_len > y.key_len ? 1 : 0;
}
// the map's pairs by selection: the smallest key above the one written last, the last pair among equal keys (no storage per pair)
template <class S> __device__ __forceinline__ void headers_cell(S &s, const Headers &h, int64_t m) {
  if (!h.pair_start || bit_of(h.nil, m)) { s.put('n'); s.put('u'); s.put('l'); s.put('l'); return; }  // a nil map inside the interface
  const uint64_t p0 = h.pair_start[m], p1 = h.pair_start[m + 1];
  s.put('{');
  // (the pairs are named by index and every verdict of key_cmp passes through a register the optimizer cannot see into: with the pair structs held
  //  in registers, hipcc -O3 built a counting kernel that disagreed with the writing kernel wherever a key repeats — measured on the MI355X as
  //  cells 1 and 5 bytes longer than their text; the CPU build of the same source agreed with itself.  The cause inside the compiler was not found)
  uint64_t prev = p1;  // p1: nothing written yet
  for (;;) {
    uint64_t best = p1;
    for (uint64_t p = p0; p < p1; p++) {
      if (prev != p1) { int c = key_cmp(h.data, h.pairs[p], h.pairs[prev]); TF_OPAQUE(c); if (c <= 0) continue; }
      if (best != p1) { int c = key_cmp(h.data, h.pairs[p], h.pairs[best]); TF_OPAQUE(c); if (c > 0) continue; }
      best = p;
    }
    if (best == p1) break;
    if (prev != p1) s.put(',');
    const tfgpu_header_pair b = h.pairs[best];
    emit_go_plain(s, h.data, b.key_off, b.key_off + b.key_len);
    s.put(':');
    emit_go_plain(s, h.data, b.val_off, b.val_off + b.val_len);
    prev = best;
  }
  s.put('}');
}
template <bool COUNT> __global__ void __launch_bounds__(256) rawtt_headers(Headers h) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= h.nrows) return;
  if constexpr (COUNT) { sr::CountSink s; headers_cell(s, h, h.rows[r]); h.len[r] = s.n; }
  else { sr::ByteSink s{h.out + h.off[r]}; headers_cell(s, h, h.rows[r]); s.flush(); }
}

// byte cells: MODE 0 the message's key / value as it is, MODE 1 the failure text of the row's reason code
template <int MODE> __global__ void __launch_bounds__(256) rawtt_copy_cells(const uint32_t *dst_off, int64_t nrows, const int32_t *rows, Bytes b, const uint8_t *reason,
                                                                            const uint32_t *reason_off, const uint8_t *src, uint8_t *dst) {
  __shared__ uint32_t doff[256 + 1];
  __shared__ uint32_t soff[256];
  auto so = [&](int64_t r) -> uint32_t {
    const int64_t m = rows[r];
    if constexpr (MODE == 0) return bit_of(b.nil, m) || b.start[m + 1] == b.start[m] ? SEG_NONE : (uint32_t)b.start[m];
    else return reason_off[reason[m] & R_MASK];
  };
  segcopy_run<1>(dst_off, nrows, (int64_t)blockIdx.x * 256, src, dst, so, doff, soff);
}
__global__ void __launch_bounds__(256) rawtt_topic(const uint8_t *topic, uint32_t tlen, int64_t nrows, uint32_t *off, uint8_t *data) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nrows) off[i] = (uint32_t)i * tlen;
  if (i < nrows * (int64_t)tlen) data[i] = topic[i % tlen];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static const char *type_text(int t) { return t == RT_BYTES ? "bytes" : t == RT_STRING ? "string" : "json"; }
static int type_of(const std::string &s) { return s == "bytes" ? RT_BYTES : s == "string" ? RT_STRING : s == "json" ? RT_JSON : -1; }

// the failure texts by reason code (sendToDLQReason: key first, joined with '|')
static std::string reason_text(uint32_t c) {
  std::string o;
  auto add = [&](const char *who, const char *what) { if (!o.empty()) o += "|"; o += std::string(who) + " is configured as " + what; };
  if (c & R_KEY_UTF8) add("key", "string, but it isn't valid UTF-8");
  if (c & R_KEY_JSON) add("key", "JSON, but it isn't valid JSON");
  if (c & R_VAL_UTF8) add("value", "string, but it isn't valid UTF-8");
  if (c & R_VAL_JSON) add("value", "JSON, but it isn't valid JSON");
  return o;
}

struct Col { std::string name; int dtype; uint32_t flags; };
static std::vector<Col> table_columns(const tfgpu_raw_to_table &h, bool dlq) {  // BuildTableSchemaAndColumnNames
  const bool ts = dlq || h.ts, hd = dlq || h.headers, key = dlq || h.key;
  const int kt = dlq ? RT_BYTES : h.key_type, vt = dlq ? RT_BYTES : h.value_type;
  auto dt = [](int t) { return t == RT_BYTES ? TFGPU_T_BYTES : t == RT_STRING ? TFGPU_T_UTF8 : TFGPU_T_ANY; };
  std::vector<Col> c{{"topic", TFGPU_T_UTF8, TFGPU_COL_KEY | TFGPU_COL_REQUIRED}, {"partition", TFGPU_T_UINT32, TFGPU_COL_KEY | TFGPU_COL_REQUIRED},
                     {"offset", TFGPU_T_UINT32, TFGPU_COL_KEY | TFGPU_COL_REQUIRED}};
  if (ts) c.push_back({"timestamp", TFGPU_T_TIMESTAMP, TFGPU_COL_REQUIRED});
  if (hd) c.push_back({"headers", TFGPU_T_ANY, 0u});
  if (key) c.push_back({"key", dt(kt), 0u});
  c.push_back({"value", dt(vt), 0u});
  if (dlq) c.push_back({"failure_reason", TFGPU_T_UTF8, 0u});
  return c;
}
static std::string table_name_of(const tfgpu_raw_to_table &h, bool dlq, const std::string &topic) {
  const std::string base = h.table_name.empty() ? topic : h.table_name;
  return dlq ? base + (h.dlq_suffix.empty() ? "_dlq" : h.dlq_suffix) : base;  // (a suffix without '_' is appended as it stands)
}

struct Staged {
  Bytes val{}, key{};
  Buf vdata, kdata, hdata, vstart, kstart, vnil, knil, hnil, pstart, pairs, offset, wt;
  const uint64_t *d_offset = nullptr, *d_pstart = nullptr; const int64_t *d_wt = nullptr;
  const tfgpu_header_pair *d_pairs = nullptr; const uint8_t *d_hnil = nullptr, *d_hdata = nullptr;
};

struct TableJob {  // one of the two result tables while it is built
  bool dlq; Buf rows; int64_t nrows = 0;
  bool ts, hd, key; int kt, vt;
  std::unique_ptr<tfgpu_dbatch> db;
  TextSegments text; int nseg = 0;  // the scanned columns of the table
  int seg_headers = -1, seg_key = -1, seg_val = -1, seg_reason = -1;
};

}  // namespace rawtt
}  // namespace tf

using namespace tf;
using namespace tf::rawtt;

static uint32_t long_bytes_now() {  // TFGPU_RAWTT_LONG_BYTES: measurement runs move the short / long switch (tools/rawtable_bench.py)
  const char *e = std::getenv("TFGPU_RAWTT_LONG_BYTES");
  const long v = e ? std::atol(e) : 0;
  return v >= 2 * RAWTT_CHUNK_BYTES ? (uint32_t)v : (uint32_t)RAWTT_LONG_BYTES;
}

extern "C" {

int tfgpu_rawtt_chunk_bytes(void) { return RAWTT_CHUNK_BYTES; }
int tfgpu_rawtt_long_bytes(void) { return (int)long_bytes_now(); }

int tfgpu_raw_to_table_create(const tfgpu_raw_to_table_config *c, tfgpu_raw_to_table **out) {
  TF_API_BEGIN
  if (!c || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_create: null argument");
  auto h = std::make_unique<tfgpu_raw_to_table>();
  h->table_name = c->table_name ? c->table_name : "";
  h->dlq_suffix = c->dlq_suffix ? c->dlq_suffix : "";
  h->key = c->is_key_enabled != 0; h->ts = c->is_timestamp_enabled != 0; h->headers = c->is_headers_enabled != 0;
  const std::string kt = c->key_type ? c->key_type : "", vt = c->value_type ? c->value_type : "";
  // CommonConfig.Validate: the key type only when the key is enabled
  if (h->key) { h->key_type = type_of(kt); if (h->key_type < 0) return tf::fail(TFGPU_ERR_CONFIG, "invalid parser config - unsupported key type: " + kt); }
  h->value_type = type_of(vt);
  if (h->value_type < 0) return tf::fail(TFGPU_ERR_CONFIG, "invalid parser config - unsupported value type: " + vt);
  *out = h.release();
  return TFGPU_OK;
  TF_API_END
}

// ParserConfigRawToTableCommon / ParserConfigRawToTableLb as encoding/json writes them (the Lb form has no key fields)
int tfgpu_raw_to_table_create_json(const char *config_json, tfgpu_raw_to_table **out) {
  TF_API_BEGIN
  if (!config_json || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_create_json: null argument");
  const Json j = Json::parse(config_json);
  if (j.type != Json::Obj) return tf::fail(TFGPU_ERR_CONFIG, "raw_to_table: the config is not a JSON object");
  const std::string tn = j.s("TableName"), kt = j.s("KeyType"), vt = j.s("ValueType"), sfx = j.s("DLQSuffix");
  tfgpu_raw_to_table_config c{};
  c.table_name = tn.c_str(); c.key_type = kt.c_str(); c.value_type = vt.c_str(); c.dlq_suffix = sfx.c_str();
  c.is_key_enabled = j.flag("IsKeyEnabled") ? 1 : 0; c.is_timestamp_enabled = j.flag("IsTimestampEnabled") ? 1 : 0; c.is_headers_enabled = j.flag("IsHeadersEnabled") ? 1 : 0;
  return tfgpu_raw_to_table_create(&c, out);
  TF_API_END
}

void tfgpu_raw_to_table_free(tfgpu_raw_to_table *h) { delete h; }

int tfgpu_raw_to_table_schema(const tfgpu_raw_to_table *h, int which, tfgpu_schema **out) {
  TF_API_BEGIN
  if (!h || !out || (which != TFGPU_RTT_MAIN && which != TFGPU_RTT_DLQ)) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_schema: bad argument");
  const std::vector<Col> cols = table_columns(*h, which == TFGPU_RTT_DLQ);
  auto dup = [](const char *s) { char *r = (char *)std::malloc(std::strlen(s) + 1); std::strcpy(r, s); return r; };
  auto *rs = (tfgpu_schema *)std::calloc(1, sizeof(tfgpu_schema));
  rs->cols = (tfgpu_colschema *)std::calloc(cols.size(), sizeof(tfgpu_colschema));
  for (auto &c : cols) {
    tfgpu_colschema &o = rs->cols[rs->ncols++];
    o.name = dup(c.name.c_str()); o.dtype = c.dtype; o.flags = c.flags;
    o.path = dup(""); o.original_type = dup(""); o.table_schema = dup(""); o.table_name = dup(""); o.expression = dup(""); o.properties_json = nullptr;
  }
  *out = rs;
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_raw_to_table_table_name(const tfgpu_raw_to_table *h, int which, const char *topic, char *buf, size_t cap) {
  TF_API_BEGIN
  if (!h || !buf || !cap || (which != TFGPU_RTT_MAIN && which != TFGPU_RTT_DLQ)) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_table_name: bad argument");
  const std::string n = table_name_of(*h, which == TFGPU_RTT_DLQ, topic ? topic : "");
  if (n.size() + 1 > cap) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_table_name: the name does not fit the buffer");
  std::memcpy(buf, n.c_str(), n.size() + 1);
  return TFGPU_OK;
  TF_API_END
}

// the refusals that need no byte of the batch (and no device)
int tfgpu_raw_to_table_check_sizes(const tfgpu_message_batch *b) {
  TF_API_BEGIN
  const char *T = "raw_to_table: ";
  if (!b) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "null batch");
  if (b->nmsg < 0) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "negative message count");
  if (b->nmsg > 0x7FFFFFFFll) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "more than 2^31-1 messages: split the batch");
  const uint64_t LIM = 0xFFFFFFF0ull;
  if (b->values_len >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the values reach 4 GiB (32-bit offsets): split the batch");
  if (b->keys_len >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the keys reach 4 GiB (32-bit offsets): split the batch");
  if (b->header_bytes_len >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the header bytes reach 4 GiB (32-bit offsets): split the batch");
  if (b->mem == TFGPU_MEM_HOST && b->nmsg > 0) {  // (offsets that claim more than the length says: what the last start says decides)
    if (b->value_start && b->value_start[b->nmsg] >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the values reach 4 GiB (32-bit offsets): split the batch");
    if (b->key_start && b->key_start[b->nmsg] >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the keys reach 4 GiB (32-bit offsets): split the batch");
  }
  const uint64_t tl = b->topic ? std::strlen(b->topic) : 0;
  if (tl * (uint64_t)b->nmsg >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the topic column reaches 4 GiB of text: split the batch");
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_raw_to_table_parse(const tfgpu_raw_to_table *h, const tfgpu_message_batch *b, tfgpu_dbatch **main_out, tfgpu_dbatch **dlq_out, int32_t *msg_codes, int64_t *nfallback) {
  TF_API_BEGIN
  const char *T = "raw_to_table: ";
  if (!h || !b || !main_out || !dlq_out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_raw_to_table_parse: null argument");
  if (const int rc = tfgpu_raw_to_table_check_sizes(b)) return rc;
  const int64_t n = b->nmsg, na = std::max<int64_t>(n, 1);
  if (n && !b->value_start) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "value_start is null");
  if ((b->values_len && !b->values) || (b->keys_len && !b->keys) || (b->header_bytes_len && !b->header_bytes)) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "a byte buffer is null");
  if (b->npairs < 0 || (b->npairs && (!b->header_pairs || !b->header_pair_start))) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "bad header pair list");
  if (b->mem != TFGPU_MEM_HOST && b->mem != TFGPU_MEM_DEVICE) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "bad mem");
  Context &cx = ctx();
  std::lock_guard<std::mutex> lk(cx.mu);
  hipStream_t st = cx.stream;
  const std::string topic = b->topic ? b->topic : "";

  // ---- the batch in HBM ---------------------------------------------------------------------------------------------------------------------------------
  Staged s;
  static const uint64_t ZERO1[1] = {0};
  s.val.data = stage_bytes(b->values, b->values_len, b->mem, s.vdata); s.val.len = b->values_len;
  s.val.start = n ? stage_array<uint64_t>(b->value_start, (size_t)n + 1, b->mem, s.vstart) : stage_array<uint64_t>(ZERO1, 1, TFGPU_MEM_HOST, s.vstart);
  s.val.nil = stage_array<uint8_t>(b->value_nil, (size_t)(n + 7) / 8, b->mem, s.vnil);
  s.key.data = stage_bytes(b->keys, b->keys_len, b->mem, s.kdata); s.key.len = b->keys_len;
  s.key.start = n ? stage_array<uint64_t>(b->key_start, (size_t)n + 1, b->mem, s.kstart) : nullptr;  // null: no message has a key (all nil)
  s.key.nil = stage_array<uint8_t>(b->key_nil, (size_t)(n + 7) / 8, b->mem, s.knil);
  s.d_hdata = stage_bytes(b->header_bytes, b->header_bytes_len, b->mem, s.hdata);
  s.d_pstart = n ? stage_array<uint64_t>(b->header_pair_start, (size_t)n + 1, b->mem, s.pstart) : nullptr;
  s.d_pairs = stage_array<tfgpu_header_pair>(b->header_pairs, (size_t)b->npairs, b->mem, s.pairs);
  s.d_hnil = stage_array<uint8_t>(b->headers_nil, (size_t)(n + 7) / 8, b->mem, s.hnil);
  s.d_offset = stage_array<uint64_t>(b->offset, (size_t)n, b->mem, s.offset);
  s.d_wt = stage_array<int64_t>(b->write_time_ns, (size_t)n, b->mem, s.wt);

  Buf status = dalloc_zero(16);
  uint32_t *dstatus = ptr<uint32_t>(status);
  {
    KernelTimer t("rawtt_check_batch", n);
    rawtt_check_batch<<<grid_for(std::max<int64_t>(n + 1, b->npairs), 256), 256, 0, st>>>(s.val, s.key, s.d_pstart, s.d_pairs, b->npairs, b->header_bytes_len, n, dstatus);
  }
  {
    const uint32_t *hs = d2h_u32(dstatus);
    tf::sync();
    if (*hs & ST_BAD_OFFSETS) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "message / header offsets must be ascending and inside their buffers");
  }

  // ---- who fits its type ------------------------------------------------------------------------------------------------------------------------------
  Buf reason = dalloc_zero((size_t)na + 16), vinfo, kinfo;
  uint8_t *dreason = ptr<uint8_t>(reason);
  const uint32_t long_bytes = long_bytes_now();
  auto check = [&](const Bytes &by, int type, uint32_t bit_utf8, uint32_t bit_json, Buf &info, uint64_t nbytes) {
    if (!n || !by.start) return;
    if (type == RT_STRING) {
      KernelTimer t("rawtt_utf8_valid", (int64_t)nbytes);
      rawtt_utf8_valid<<<grid_for(n, 256), 256, 0, st>>>(by, n, long_bytes, dreason, bit_utf8);
    } else if (type == RT_JSON) {
      info = dalloc((size_t)na + 16);
      KernelTimer t("rawtt_json_check", (int64_t)nbytes);
      rawtt_json_check<<<grid_for(n, 128), 128, 0, st>>>(by, n, dreason, bit_json, ptr<uint8_t>(info), dstatus);
    }
  };
  if (h->key) check(s.key, h->key_type, R_KEY_UTF8, R_KEY_JSON, kinfo, b->keys_len);
  check(s.val, h->value_type, R_VAL_UTF8, R_VAL_JSON, vinfo, b->values_len);

  // ---- the split ----------------------------------------------------------------------------------------------------------------------------------------
  const int64_t stride = ((n + 1 + 3) / 4) * 4;
  Buf keep = dalloc_zero((size_t)stride * 2 * 4 + 16), rows_main = dalloc((size_t)na * 4 + 16), rows_dlq = dalloc((size_t)na * 4 + 16), codes;
  if (n) {
    KernelTimer t("rawtt_split", n);
    rawtt_split_flags<<<grid_for(n, 256), 256, 0, st>>>(dreason, n, ptr<uint32_t>(keep), stride);
  }
  exclusive_scan_u32_segments(ptr<uint32_t>(keep), n, 2, stride);
  const uint32_t *hcount = segment_totals_to_host(ptr<uint32_t>(keep), n, 2, stride);
  if (n) {
    if (msg_codes) codes = dalloc((size_t)na * 4);
    KernelTimer t("rawtt_split", n);
    rawtt_rows<<<grid_for(n, 256), 256, 0, st>>>(dreason, n, ptr<uint32_t>(keep), stride, ptr<int32_t>(rows_main), ptr<int32_t>(rows_dlq), ptr<int32_t>(codes));
  }
  const uint32_t *hstatus = d2h_u32(dstatus);
  tf::sync();
  const int64_t nmain = hcount[0], ndlq = hcount[1];
  const bool any_canon = *hstatus & ST_CANON;
  if (nfallback) *nfallback = n - nmain - ndlq;
  if (msg_codes && n) {
    if (*hstatus & ST_FALLBACK) { d2h(msg_codes, codes->p, (size_t)n * 4); tf::sync(); }
    else std::memset(msg_codes, 0, (size_t)n * 4);
  }

  // ---- the two tables -------------------------------------------------------------------------------------------------------------------------------------
  std::vector<uint32_t> roff{0u};
  std::string rtext;
  for (uint32_t c = 0; c < 16; c++) { rtext += reason_text(c); roff.push_back((uint32_t)rtext.size()); }
  rtext.append(32, '\0');
  Buf broff = upload_const(roff.data(), roff.size() * 4), brtext = upload_const(rtext.data(), rtext.size());
  Buf btopic = upload_const(topic.empty() ? "\0" : topic.data(), std::max<size_t>(topic.size(), 1));

  TableJob jobs[2];
  for (int q = 0; q < 2; q++) {
    TableJob &j = jobs[q];
    j.dlq = q == 1;
    j.rows = q ? rows_dlq : rows_main; j.nrows = q ? ndlq : nmain;
    j.ts = j.dlq || h->ts; j.hd = j.dlq || h->headers; j.key = j.dlq || h->key;
    j.kt = j.dlq ? RT_BYTES : h->key_type; j.vt = j.dlq ? RT_BYTES : h->value_type;
    const int64_t nr = j.nrows, nra = std::max<int64_t>(nr, 1);
    const int32_t *rows = ptr<int32_t>(j.rows);
    j.db = std::make_unique<tfgpu_dbatch>();
    tfgpu_dbatch &db = *j.db;
    db.nrows = nr; db.table = table_name_of(*h, j.dlq, topic); db.src_row = j.rows;
    for (auto &c : table_columns(*h, j.dlq)) {
      DColumn d;
      d.name = c.name; d.dtype = c.dtype;
      d.repr = c.dtype == TFGPU_T_UTF8 ? TFGPU_R_STRING : c.dtype == TFGPU_T_BYTES ? TFGPU_R_BYTES : c.dtype == TFGPU_T_ANY ? TFGPU_R_JSON : c.dtype == TFGPU_T_TIMESTAMP ? TFGPU_R_TIME : TFGPU_R_UINT32;
      db.schema.emplace_back(c.name, c.dtype);
      if (c.flags & TFGPU_COL_KEY) db.key_names.push_back(c.name);
      db.cols.push_back(std::move(d));
    }
    auto col = [&](const char *name) -> DColumn & { for (auto &c : db.cols) if (c.name == name) return c; throw Error(TFGPU_ERR_INVALID, "raw_to_table: no such column"); };
    // the scanned columns of this table, one segment of `lens` each
    if (j.hd) j.seg_headers = j.nseg++;
    if (j.key) j.seg_key = j.nseg++;
    j.seg_val = j.nseg++;
    if (j.dlq) j.seg_reason = j.nseg++;
    j.text = TextSegments(j.nseg, nr);
    auto seg = [&](int sgi) { return j.text.seg(sgi); };
    col("offset").values = dalloc((size_t)nra * 4); col("partition").values = dalloc((size_t)nra * 4);
    if (j.ts) { col("timestamp").values = dalloc((size_t)nra * 8); col("timestamp").nanos = dalloc((size_t)nra * 4); }
    if (!nr) continue;
    Fixed f{};
    f.rows = rows; f.nrows = nr; f.offset = s.d_offset; f.wt = s.d_wt; f.partition = b->partition;
    f.col_offset = ptr<uint32_t>(col("offset").values); f.col_partition = ptr<uint32_t>(col("partition").values);
    if (j.ts) { f.ts_sec = ptr<int64_t>(col("timestamp").values); f.ts_nsec = ptr<int32_t>(col("timestamp").nanos); }
    f.key = s.key; f.val = s.val;
    if (j.key && j.kt != RT_JSON) f.key_len = seg(j.seg_key);
    if (j.vt != RT_JSON) f.val_len = seg(j.seg_val);
    if (j.dlq) { f.reason = dreason; f.reason_off = ptr<uint32_t>(broff); f.reason_len = seg(j.seg_reason); }
    { KernelTimer t("rawtt_fixed", nr); rawtt_fixed<<<grid_for(nr, 256), 256, 0, st>>>(f); }
    {
      KernelTimer t("rawtt_validity", nr);
      const unsigned g = grid_for((nr + 7) / 8, 256);
      if (j.key) {
        DColumn &c = col("key");
        c.validity = dalloc((size_t)((nra + 7) / 8) + 8);
        rawtt_validity<<<g, 256, 0, st>>>(rows, nr, s.key.nil, s.key.start ? 0 : 1, j.kt == RT_JSON ? ptr<uint8_t>(kinfo) : nullptr, ptr<uint8_t>(c.validity));
      }
      DColumn &c = col("value");
      c.validity = dalloc((size_t)((nra + 7) / 8) + 8);
      rawtt_validity<<<g, 256, 0, st>>>(rows, nr, s.val.nil, 0, j.vt == RT_JSON ? ptr<uint8_t>(vinfo) : nullptr, ptr<uint8_t>(c.validity));
    }
    if (j.hd) {
      Headers hh{s.d_hdata, s.d_pstart, s.d_pairs, s.d_hnil, rows, nr, seg(j.seg_headers), nullptr, nullptr};
      KernelTimer t("rawtt_headers_len", nr);
      rawtt_headers<true><<<grid_for(nr, 256), 256, 0, st>>>(hh);
    }
    auto any_len = [&](const Bytes &by, const Buf &info, int sgi) {
      { KernelTimer t("rawtt_any_len", nr); rawtt_any_len<false><<<grid_for(nr, 256), 256, 0, st>>>(by, ptr<uint8_t>(info), rows, nr, seg(sgi)); }
      if (any_canon) { KernelTimer t("rawtt_any_len_canon", nr); rawtt_any_len<true><<<grid_for(nr, 256), 256, 0, st>>>(by, ptr<uint8_t>(info), rows, nr, seg(sgi)); }
    };
    if (j.key && j.kt == RT_JSON && s.key.start) any_len(s.key, kinfo, j.seg_key);
    if (j.vt == RT_JSON) any_len(s.val, vinfo, j.seg_val);
    j.text.scan(true);
  }
  tf::sync();
  for (TableJob &j : jobs) {
    tfgpu_dbatch &db = *j.db;
    const int64_t nr = j.nrows;
    const int32_t *rows = ptr<int32_t>(j.rows);
    auto col = [&](const char *name) -> DColumn & { for (auto &c : db.cols) if (c.name == name) return c; throw Error(TFGPU_ERR_INVALID, "raw_to_table: no such column"); };
    auto text = [&](const char *name, int sgi) -> DColumn & {
      DColumn &c = col(name);
      if (text_total_exceeds(j.text.total(sgi))) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column " + name + " of table " + db.table + " reaches 4 GiB of text (32-bit offsets): split the batch");
      c.offsets = j.text.offsets(sgi);
      c.data_len = j.text.total(sgi);
      c.data = dalloc((size_t)c.data_len + 16);
      return c;
    };
    {
      DColumn &c = col("topic");
      c.offsets = dalloc((size_t)(nr + 1) * 4 + 16);
      c.data_len = (uint64_t)nr * topic.size();
      c.data = dalloc((size_t)c.data_len + 16);
      KernelTimer t("rawtt_topic", nr);
      rawtt_topic<<<grid_for(std::max<int64_t>(nr + 1, (int64_t)c.data_len), 256), 256, 0, st>>>(ptr<uint8_t>(btopic), (uint32_t)topic.size(), nr, ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.data));
    }
    auto bytes_cells = [&](const char *name, int sgi, const Bytes &by) {
      DColumn &c = text(name, sgi);
      if (!nr || !c.data_len) return;
      KernelTimer t("rawtt_copy_cells", (int64_t)c.data_len);
      rawtt_copy_cells<0><<<grid_for(nr, 256), 256, 0, st>>>(ptr<uint32_t>(c.offsets), nr, rows, by, nullptr, nullptr, by.data, ptr<uint8_t>(c.data));
    };
    auto any_cells = [&](const char *name, int sgi, const Bytes &by, const Buf &info) {
      DColumn &c = text(name, sgi);
      if (!nr || !by.start) return;
      { KernelTimer t("rawtt_any_write", (int64_t)c.data_len); rawtt_any_write<false><<<grid_for(nr, 256), 256, 0, st>>>(by, ptr<uint8_t>(info), rows, nr, ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.data)); }
      if (any_canon) { KernelTimer t("rawtt_any_write_canon", (int64_t)c.data_len); rawtt_any_write<true><<<grid_for(nr, 256), 256, 0, st>>>(by, ptr<uint8_t>(info), rows, nr, ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.data)); }
    };
    if (j.hd) {
      DColumn &c = text("headers", j.seg_headers);
      if (nr) {
        Headers hh{s.d_hdata, s.d_pstart, s.d_pairs, s.d_hnil, rows, nr, nullptr, ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.data)};
        KernelTimer t("rawtt_headers_write", (int64_t)c.data_len);
        rawtt_headers<false><<<grid_for(nr, 256), 256, 0, st>>>(hh);
      }
    }
    if (j.key) { if (j.kt == RT_JSON) any_cells("key", j.seg_key, s.key, kinfo); else bytes_cells("key", j.seg_key, s.key); }
    if (j.vt == RT_JSON) any_cells("value", j.seg_val, s.val, vinfo); else bytes_cells("value", j.seg_val, s.val);
    if (j.dlq) {
      DColumn &c = text("failure_reason", j.seg_reason);
      if (nr) {
        KernelTimer t("rawtt_copy_cells", (int64_t)c.data_len);
        rawtt_copy_cells<1><<<grid_for(nr, 256), 256, 0, st>>>(ptr<uint32_t>(c.offsets), nr, rows, Bytes{}, dreason, ptr<uint32_t>(broff), ptr<uint8_t>(brtext), ptr<uint8_t>(c.data));
      }
    }
    if (!nr) for (auto &c : db.cols) if (repr_is_var(c.repr) && c.name != "topic") TF_HIP(hipMemsetAsync(c.offsets->p, 0, 4, st));
  }
  tf::sync();  // (the staged copies of the batch go back to the pool behind the kernels that read them; pageable sources are fenced)
  *main_out = jobs[0].db.release();
  *dlq_out = jobs[1].db.release();
  return TFGPU_OK;
  TF_API_END
}

}  // extern "C"
