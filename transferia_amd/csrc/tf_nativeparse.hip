// tf_nativeparse.hip — the native parser on device (pkg/parsers/registry/native/parser_native.go: abstract.UnmarshalChangeItems, restore.go:344-373):
// queue messages that hold `[` ChangeItem.MarshalJSON() … `]` — what tfgpu_queue_serialize writes under TFGPU_QFMT_NATIVE — become one ordinary batch
// per group of like items, with the row meta, PartID and OldKeys.KeyTypes a batch cannot say.  A message the device does not follow in full is left
// to the stock parser whole (include/tfgpu.h, tfgpu_native_reason).
//
//   natp_check_batch   the batch's own offsets: ascending, inside the buffer (nothing below reads a byte before this has passed)
//   natp_cut<COUNT>    one wave per message, 64 bytes a step: ballots of quote, backslash and brackets; escaped quotes by the odd-backslash-run carry;
//                      the in-string mask by prefix-xor; depth by the popcount prefix of the bracket masks.  The tokens at depth 0 / 1 outside strings
//                      must spell `[`, `{`…`}` (`,` `{`…`}`)*, `]` between white space; COUNT counts the items, (scan), the second run writes their spans
//   natp_header        lane = item: utf8.Valid, the scanner grammar over the item, the top-level members (fixed fields, spans of the rest, kind), the
//                      128-bit hash of the group key
//   natp_tid_*         RestoreChangeItems reads the table_schema of the FIRST item of a (schema, table) in the message: items that differ from it fall back
//   natp_intern        open-addressing table over the group hashes; under an equal hash the key spans are compared (tf_tablesplit.hip's policy: a
//                      hash never decides alone); intern_first / _flag / _ids (tf_intern.hpp) number the groups by first appearance
//   natp_validate      lane = item: columnvalues / keyvalues against the group's conversion program; writes nothing final; the first reason of the
//                      lowest item per message by atomicMin of (item, column, reason)
//   natp_keep          items of flagged messages leave; (the groups are numbered again over the kept items, one stable sort gives the rows)
//   natp_cells<COUNT>  lane = kept item: text lengths, (scan), then fixed-width cells, validity, unescaped / base64-decoded text, OldKeys, meta
//   natp_any<COUNT, CANON>  `any` cells alone, so that the canonicaliser's container stack (scratch) stays out of natp_cells
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <array>
#include <map>
#include <unordered_map>

#include "tf_ingest.hpp"
#include "tf_intern.hpp"
#include "tf_jsonscan.hpp"
#include "tf_nativeparse.hpp"
#include "tf_devfmt.hpp"
#include "tf_utf8.hpp"

namespace tf {
namespace natp {

enum : uint32_t { SP_CN = 0, SP_CV, SP_TS, SP_KN, SP_KT, SP_KV, SP_SCHEMA, SP_TABLE, SP_PART, SP_TX, SP_QUERY, NSPAN };
enum : uint32_t { M_ID = 0, M_LSN, M_COMMIT, M_COUNTER, M_KIND, M_SCHEMA, M_TABLE, M_PART, M_CN, M_CV, M_TS, M_OLDKEYS, M_TX, M_QUERY, M_UNKNOWN };
enum : uint32_t { IT_HEADER_OK = 1u, IT_CANON = 2u };
constexpr uint64_t NOFLAG = ~0ull;

struct Item { uint32_t s, e, msg, idx; };  // the object's bytes inside the values, its message, its index inside the message
struct Hdr {
  uint32_t sp[NSPAN][2];  // [start, end) of a member's value; 0, 0 = absent or null
  uint64_t lsn, commit, h1, h2, tid, ts1, ts2;
  int64_t counter;
  uint32_t id, ncn, ncv, nkn, nkv, flags;
  uint8_t kind, names_form;
};
struct Cell { uint32_t s, e, vt; };

__device__ __forceinline__ bool bit_of(const uint8_t *bm, int64_t i) { return bm && ((bm[i >> 3] >> (i & 7)) & 1); }
__device__ __forceinline__ uint64_t flag_key(uint32_t item, int32_t column, uint32_t reason) { return ((uint64_t)item << 32) | ((uint64_t)(uint32_t)(column + 1) << 8) | reason; }

__global__ void __launch_bounds__(256) natp_check_batch(const uint64_t *start, uint64_t len, int64_t n, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = i <= n && (start[i] > len || (i < n && start[i] > start[i + 1]));
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1u);
}

// ---- the cut -----------------------------------------------------------------------------------------------------------------------------------------
// The characters a backslash escapes, from the mask of backslashes of this step and whether the step in front ended inside an odd run (the carry of
// the add tells the next step the same)
__device__ __forceinline__ uint64_t escaped_mask(uint64_t bs, uint64_t &carry) {
  const uint64_t EVEN = 0x5555555555555555ull;
  bs &= ~carry;  // a backslash that is itself escaped starts nothing
  const uint64_t follows = (bs << 1) | carry;
  const uint64_t odd_starts = bs & ~EVEN & ~follows;
  const uint64_t sum = odd_starts + bs;
  carry = sum < odd_starts ? 1ull : 0ull;
  return (EVEN ^ (sum << 1)) & follows;
}
__device__ __forceinline__ uint64_t prefix_xor(uint64_t x) {
  x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
  return x;
}
enum : uint32_t { TK_NONE = 0, TK_BEGIN, TK_OPEN, TK_CLOSE, TK_COMMA, TK_END };

template <bool COUNT> __global__ void __launch_bounds__(256) natp_cut(const uint8_t *__restrict__ data, const uint64_t *__restrict__ start, const uint8_t *__restrict__ nil,
                                                                       int64_t n, uint32_t *__restrict__ count, uint32_t *__restrict__ mstat,
                                                                       const uint32_t *__restrict__ base, Item *__restrict__ items) {
  const int64_t m = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (m >= n) return;
  if (bit_of(nil, m)) { if (COUNT && lane == 0) { count[m] = 0; mstat[m] = 0; } return; }  // a nil value: a message without items
  if (!COUNT && mstat[m]) return;
  const uint32_t s = (uint32_t)start[m], e = (uint32_t)start[m + 1];
  const uint32_t slot0 = COUNT ? 0u : base[m], nslots = COUNT ? 0u : base[m + 1] - base[m];
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t esc_carry = 0, in_str = 0;  // in_str: all ones while the step starts inside a string
  int depth = 0;
  uint32_t prev = TK_NONE, nitems = 0;
  bool bad = false;
  for (uint64_t pos = s; pos < e && !bad; pos += 64) {  // (64-bit: a message that ends within 64 bytes of 2^32 must not wrap)
    const uint64_t p = pos + lane;
    const uint32_t c = p < e ? data[p] : ' ';
    const uint64_t bs = __ballot(c == '\\');
    uint64_t q = __ballot(c == '"');
    q &= ~escaped_mask(bs, esc_carry);
    const uint64_t instr = prefix_xor(q) ^ in_str;  // bit i: byte i is inside a string (its opening quote counts, its closing quote does not)
    in_str = (uint64_t)((int64_t)instr >> 63);
    const bool out = !((instr >> lane) & 1ull) && !((q >> lane) & 1ull);
    const bool is_open = out && (c == '{' || c == '['), is_close = out && (c == '}' || c == ']');
    const uint64_t op = __ballot(is_open), cl = __ballot(is_close);
    const int d = depth + __popcll(op & below) - __popcll(cl & below);  // the depth in front of this byte
    uint32_t tk = TK_NONE;
    bool junk = false;
    if ((q >> lane) & 1ull) junk = d <= 1;  // a string at the message's own level
    else if (out) {
      if (c == '{') { if (d == 1) tk = TK_OPEN; else if (d == 0) junk = true; }
      else if (c == '[') { if (d == 0) tk = TK_BEGIN; else if (d == 1) junk = true; }
      else if (c == '}') { if (d == 2) tk = TK_CLOSE; else if (d <= 1) junk = true; }
      else if (c == ']') { if (d == 1) tk = TK_END; else if (d == 2 || d <= 0) junk = true; }
      else if (d <= 1) { if (c == ',' && d == 1) tk = TK_COMMA; else if (!sr::is_ws(c)) junk = true; }
    }
    const uint64_t mb = __ballot(tk == TK_BEGIN), mo = __ballot(tk == TK_OPEN), mc = __ballot(tk == TK_CLOSE), mm = __ballot(tk == TK_COMMA), me = __ballot(tk == TK_END);
    const uint64_t T = mb | mo | mc | mm | me;
    auto kind_at = [&](uint32_t l) -> uint32_t { return ((mb >> l) & 1) ? TK_BEGIN : ((mo >> l) & 1) ? TK_OPEN : ((mc >> l) & 1) ? TK_CLOSE : ((mm >> l) & 1) ? TK_COMMA : TK_END; };
    if (tk != TK_NONE) {  // the token in front of this one decides whether it may stand here
      const uint64_t pm = T & below;
      const uint32_t pk = pm ? kind_at(63u - (uint32_t)__clzll((long long)pm)) : prev;
      const bool ok = tk == TK_BEGIN ? pk == TK_NONE : tk == TK_OPEN ? (pk == TK_BEGIN || pk == TK_COMMA) : tk == TK_CLOSE ? pk == TK_OPEN : tk == TK_COMMA ? pk == TK_CLOSE
                                                                                                                                                   : (pk == TK_BEGIN || pk == TK_CLOSE);
      if (!ok) junk = true;
    }
    if (__any(junk)) { bad = true; break; }
    if (!COUNT) {
      const uint32_t k = nitems + (uint32_t)__popcll(mo & below);  // items opened in front of this byte
      if (tk == TK_OPEN && k < nslots) { Item &it = items[slot0 + k]; it.s = (uint32_t)p; it.msg = (uint32_t)m; it.idx = k; }
      if (tk == TK_CLOSE && k >= 1 && k - 1 < nslots) items[slot0 + k - 1].e = (uint32_t)p + 1;
    }
    nitems += (uint32_t)__popcll(mo);
    depth += __popcll(op) - __popcll(cl);
    if (T) prev = kind_at(63u - (uint32_t)__clzll((long long)T));
  }
  if (COUNT && lane == 0) {
    if (depth != 0 || in_str || prev != TK_END) bad = true;  // (an empty value is no JSON text either)
    count[m] = bad ? 0u : nitems;
    mstat[m] = bad ? 1u : 0u;
  }
}

// ---- the item header ----------------------------------------------------------------------------------------------------------------------------------
struct Hash128 {
  uint64_t h1 = 0x452821E638D01377ull, h2 = 0xBE5466CF34E90C6Cull;
  __device__ __forceinline__ void mix(uint64_t w) {
    h1 = (h1 ^ w) * 0x9E3779B97F4A7C15ull; h1 ^= h1 >> 32;
    h2 = (((h2 << 31) | (h2 >> 33)) ^ w) * 0xC2B2AE3D27D4EB4Full; h2 ^= h2 >> 29;
  }
  // the bytes [a, b) eight at a time, their count in front (so that two spans never run into each other)
  __device__ __forceinline__ void span(MemBytes &rd, uint32_t a, uint32_t b) {
    mix((uint64_t)(b - a) | 0xA500000000000000ull);
    for (; a + 8 <= b; a += 8) mix(rd.word(a));
    if (a < b) mix(rd.word(a) & ((1ull << (8 * (b - a))) - 1ull));
  }
  __device__ __forceinline__ void finish() {
    h1 ^= h1 >> 33; h1 *= 0xFF51AFD7ED558CCDull; h1 ^= h1 >> 33;
    h2 ^= h2 >> 33; h2 *= 0xC4CEB9FE1A85EC53ull; h2 ^= h2 >> 33;
  }
};
// a JSON string's DECODED bytes into the hash (two spellings of one name are one name)
__device__ __forceinline__ void hash_string(NameHash &h, MemBytes &rd, uint32_t a, uint32_t b) {
  if (a != b) sr::emit_unquoted(h, rd, a, b - a);  // (an absent or null member is the empty string)
  h.put(0xFE);
}
__device__ __forceinline__ bool lit_eq(MemBytes &rd, uint32_t at, const char *lit, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) if (rd.at(at + i) != (uint8_t)lit[i]) return false;
  return true;
}
__device__ __forceinline__ uint32_t member_of(MemBytes &rd, uint32_t a, uint32_t n) {  // the key's body [a, a + n)
  switch (n) {
    case 2: return lit_eq(rd, a, "id", 2) ? M_ID : M_UNKNOWN;
    case 4: return lit_eq(rd, a, "kind", 4) ? M_KIND : lit_eq(rd, a, "part", 4) ? M_PART : M_UNKNOWN;
    case 5: return lit_eq(rd, a, "table", 5) ? M_TABLE : lit_eq(rd, a, "tx_id", 5) ? M_TX : lit_eq(rd, a, "query", 5) ? M_QUERY : M_UNKNOWN;
    case 6: return lit_eq(rd, a, "schema", 6) ? M_SCHEMA : M_UNKNOWN;
    case 7: return lit_eq(rd, a, "nextlsn", 7) ? M_LSN : lit_eq(rd, a, "oldkeys", 7) ? M_OLDKEYS : M_UNKNOWN;
    case 10: return lit_eq(rd, a, "commitTime", 10) ? M_COMMIT : lit_eq(rd, a, "txPosition", 10) ? M_COUNTER : M_UNKNOWN;
    case 11: return lit_eq(rd, a, "columnnames", 11) ? M_CN : M_UNKNOWN;
    case 12: return lit_eq(rd, a, "columnvalues", 12) ? M_CV : lit_eq(rd, a, "table_schema", 12) ? M_TS : M_UNKNOWN;
    default: return M_UNKNOWN;
  }
}
__device__ __forceinline__ void skip_ws(MemBytes &rd, uint32_t &pos, uint32_t end) { while (pos < end && sr::is_ws(rd.at(pos))) pos++; }
// What read_header's one run of skip_value has validated is walked again without the scanner's stack: a string ends at its first unescaped quote, a
// container where its brackets balance, a number or literal at the next delimiter.  `vt`: the value's sr::VT_* type (no flags)
__device__ __forceinline__ void skip_str(MemBytes &rd, uint32_t &pos, uint32_t end) {
  for (pos++; pos < end;) {
    const uint32_t c = rd.at(pos);
    pos += c == '\\' ? 2u : 1u;
    if (c == '"') return;
  }
}
__device__ __forceinline__ void skip_valid(MemBytes &rd, uint32_t &pos, uint32_t end, uint32_t &vt) {
  const uint32_t c = rd.at(pos);
  if (c == '"') { vt = sr::VT_STR; skip_str(rd, pos, end); return; }
  if (c == '{' || c == '[') {
    vt = c == '{' ? sr::VT_OBJ : sr::VT_ARR;
    int depth = 0;
    while (pos < end) {
      const uint32_t d = rd.at(pos);
      if (d == '"') { skip_str(rd, pos, end); continue; }
      pos++;
      if (d == '{' || d == '[') depth++;
      else if ((d == '}' || d == ']') && --depth == 0) return;
    }
    return;
  }
  vt = c == 't' ? sr::VT_TRUE : c == 'f' ? sr::VT_FALSE : c == 'n' ? sr::VT_NULL : sr::VT_NUM;
  while (pos < end) { const uint32_t d = rd.at(pos); if (d == ',' || d == '}' || d == ']' || sr::is_ws(d)) return; pos++; }
}
// the next element of a validated array; pos stands behind `[` or behind the element in front.  false at `]`
__device__ __forceinline__ bool next_elem(MemBytes &rd, uint32_t &pos, uint32_t end, Cell &c) {
  skip_ws(rd, pos, end);
  if (pos >= end || rd.at(pos) == ']') return false;
  c.s = pos; c.vt = 0;
  skip_valid(rd, pos, end, c.vt);
  c.e = pos;
  skip_ws(rd, pos, end);
  if (pos < end && rd.at(pos) == ',') pos++;
  return true;
}
// a validated key at pos (its opening quote): pos -> behind it; false when it is written with an escape or a byte beyond ASCII
__device__ __forceinline__ bool plain_key(MemBytes &rd, uint32_t &pos, uint32_t end) {
  bool plain = true;
  for (pos++; pos < end;) {
    const uint32_t c = rd.at(pos);
    if (c == '"') { pos++; return plain; }
    if (c == '\\') { plain = false; pos += 2; continue; }
    if (c >= 0x80) plain = false;
    pos++;
  }
  return plain;
}
// digits of a validated number literal as a magnitude: false for a fraction, an exponent or more than 64 bits
__device__ __forceinline__ bool literal_u64(MemBytes &rd, uint32_t a, uint32_t b, bool &neg, uint64_t &mag) {
  neg = rd.at(a) == '-';
  if (neg) a++;
  mag = 0;
  for (; a < b; a++) {
    const uint32_t c = rd.at(a);
    if (c < '0' || c > '9') return false;
    if (mag > 1844674407370955161ull) return false;
    mag *= 10;
    if (mag > ~0ull - (c - '0')) return false;
    mag += c - '0';
  }
  return true;
}
// an array of strings (a []string field): its element count, or false
__device__ __forceinline__ bool string_array(MemBytes &rd, uint32_t a, uint32_t b, uint32_t &n) {
  uint32_t pos = a + 1;
  Cell c;
  n = 0;
  while (next_elem(rd, pos, b, c)) { if ((c.vt & sr::VT_MASK) != sr::VT_STR) return false; n++; }
  return true;
}

// One item.  Returns 0 or the reason the item's own form gives (column -1).
__device__ uint32_t read_header(MemBytes &rd, const Item &it, Hdr &h) {
  if (!utf8_valid_range(rd, it.s, it.e, it.e)) return TFGPU_NATIVE_UTF8;
  {
    uint32_t pos = it.s, vt = 0;
    const int rc = sr::skip_value(rd, pos, it.e, vt);
    if (rc == 2) return TFGPU_NATIVE_DEPTH;
    if (rc || pos != it.e) return TFGPU_NATIVE_SYNTAX;
  }
  uint32_t seen = 0, pos = it.s + 1;
  bool has_kind = false;
  for (;;) {
    skip_ws(rd, pos, it.e);
    if (rd.at(pos) == '}') break;
    const uint32_t ks = pos;
    if (!plain_key(rd, pos, it.e)) return TFGPU_NATIVE_KEY_FORM;
    const uint32_t mem = member_of(rd, ks + 1, pos - ks - 2);
    skip_ws(rd, pos, it.e);
    pos++;  // ':'
    skip_ws(rd, pos, it.e);
    Cell v{pos, 0, 0};
    skip_valid(rd, pos, it.e, v.vt);
    v.e = pos;
    skip_ws(rd, pos, it.e);
    if (rd.at(pos) == ',') pos++;
    if (mem == M_UNKNOWN) continue;  // decoded into a dummy
    if (seen & (1u << mem)) return TFGPU_NATIVE_DUP_MEMBER;
    seen |= 1u << mem;
    const uint32_t t = v.vt & sr::VT_MASK;
    auto span = [&](uint32_t which) { h.sp[which][0] = v.s; h.sp[which][1] = v.e; };
    switch (mem) {
      case M_ID: case M_LSN: case M_COMMIT: {
        if (t == sr::VT_NULL) break;
        bool neg; uint64_t mag;
        if (t != sr::VT_NUM || !literal_u64(rd, v.s, v.e, neg, mag) || neg) return TFGPU_NATIVE_HEADER_VALUE;
        if (mem == M_ID) { if (mag > 0xFFFFFFFFull) return TFGPU_NATIVE_HEADER_VALUE; h.id = (uint32_t)mag; }
        else if (mem == M_LSN) h.lsn = mag;
        else h.commit = mag;
        break;
      }
      case M_COUNTER:
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_NUM || !sr::number_int64(rd, v.s, v.e - v.s, &h.counter)) return TFGPU_NATIVE_HEADER_VALUE;
        break;
      case M_KIND:
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_STR) return TFGPU_NATIVE_HEADER_VALUE;
        if (v.e - v.s == 8 && lit_eq(rd, v.s + 1, "insert", 6)) { h.kind = TFGPU_K_INSERT; has_kind = true; }
        else if (v.e - v.s == 8 && lit_eq(rd, v.s + 1, "update", 6)) { h.kind = TFGPU_K_UPDATE; has_kind = true; }
        else if (v.e - v.s == 8 && lit_eq(rd, v.s + 1, "delete", 6)) { h.kind = TFGPU_K_DELETE; has_kind = true; }
        else has_kind = false;  // another kind, or one of the three spelled with escapes: the host decides
        break;
      case M_SCHEMA: case M_TABLE: case M_PART: case M_TX: case M_QUERY:
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_STR) return TFGPU_NATIVE_HEADER_VALUE;
        span(mem == M_SCHEMA ? SP_SCHEMA : mem == M_TABLE ? SP_TABLE : mem == M_PART ? SP_PART : mem == M_TX ? SP_TX : SP_QUERY);
        break;
      case M_CN:
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_ARR || !string_array(rd, v.s, v.e, h.ncn)) return TFGPU_NATIVE_HEADER_VALUE;
        span(SP_CN);
        break;
      case M_CV: {
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_ARR) return TFGPU_NATIVE_HEADER_VALUE;
        uint32_t q = v.s + 1; Cell c;
        while (next_elem(rd, q, v.e, c)) h.ncv++;
        span(SP_CV);
        break;
      }
      case M_TS:
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_ARR) return TFGPU_NATIVE_HEADER_VALUE;
        span(SP_TS);
        break;
      case M_OLDKEYS: {
        if (t == sr::VT_NULL) break;
        if (t != sr::VT_OBJ) return TFGPU_NATIVE_HEADER_VALUE;
        uint32_t q = v.s + 1, oseen = 0;
        for (;;) {
          skip_ws(rd, q, v.e);
          if (rd.at(q) == '}') break;
          const uint32_t oks = q;
          if (!plain_key(rd, q, v.e)) return TFGPU_NATIVE_KEY_FORM;
          const uint32_t kn = q - oks - 2;
          const uint32_t om = kn == 8 && lit_eq(rd, oks + 1, "keynames", 8) ? 0u : kn == 8 && lit_eq(rd, oks + 1, "keytypes", 8) ? 1u : kn == 9 && lit_eq(rd, oks + 1, "keyvalues", 9) ? 2u : 3u;
          skip_ws(rd, q, v.e);
          q++;
          skip_ws(rd, q, v.e);
          Cell ov{q, 0, 0};
          skip_valid(rd, q, v.e, ov.vt);
          ov.e = q;
          skip_ws(rd, q, v.e);
          if (rd.at(q) == ',') q++;
          if (om == 3) return TFGPU_NATIVE_HEADER_VALUE;  // (a struct field matches its key in any letter case: the host decides what this one is)
          if (oseen & (1u << om)) return TFGPU_NATIVE_DUP_MEMBER;
          oseen |= 1u << om;
          const uint32_t ot = ov.vt & sr::VT_MASK;
          if (ot == sr::VT_NULL) continue;
          if (ot != sr::VT_ARR) return TFGPU_NATIVE_HEADER_VALUE;
          if (om == 2) { uint32_t z = ov.s + 1; Cell c; while (next_elem(rd, z, ov.e, c)) h.nkv++; h.sp[SP_KV][0] = ov.s; h.sp[SP_KV][1] = ov.e; }
          else {
            uint32_t cnt = 0;
            if (!string_array(rd, ov.s, ov.e, cnt)) return TFGPU_NATIVE_HEADER_VALUE;
            if (om == 0) { h.nkn = cnt; h.sp[SP_KN][0] = ov.s; h.sp[SP_KN][1] = ov.e; } else { h.sp[SP_KT][0] = ov.s; h.sp[SP_KT][1] = ov.e; }
          }
        }
        break;
      }
      default: break;
    }
  }
  if (!has_kind) return TFGPU_NATIVE_KIND;
  if (h.ncn != h.ncv) return TFGPU_NATIVE_LENGTHS;
  if (h.kind == TFGPU_K_INSERT) { if (h.nkv) return TFGPU_NATIVE_INSERT_KEYVALUES; }
  else if (h.nkn != h.nkv) return TFGPU_NATIVE_LENGTHS;
  h.names_form = h.sp[SP_CN][1] == 0 ? 1 : h.ncn == 0 ? 2 : 0;
  return 0;
}

__global__ void __launch_bounds__(128) natp_header(const uint8_t *data, const Item *__restrict__ items, int64_t n, Hdr *__restrict__ hdrs, unsigned long long *mflag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  MemBytes rd(data);
  const Item it = items[i];
  Hdr &h = hdrs[i];  // (filled in place: a local copy indexed by member would sit in scratch)
  h = Hdr{};
  const uint32_t why = read_header(rd, it, h);
  if (why) atomicMin(&mflag[it.msg], (unsigned long long)flag_key(it.idx, -1, why));
  else {
    h.flags = IT_HEADER_OK;
    NameHash t;  // schema, table, part: decoded (one call site: the rune decoder is inlined once)
    for (uint32_t q = 0; q < 3; q++) {
      hash_string(t, rd, h.sp[SP_SCHEMA + q][0], h.sp[SP_SCHEMA + q][1]);
      if (q == 1) { NameHash id = t; id.finish(); h.tid = id.h1 ^ (id.h2 << 1); }
    }
    t.finish();
    Hash128 ts;
    ts.span(rd, h.sp[SP_TS][0], h.sp[SP_TS][1]);
    ts.finish();
    h.ts1 = ts.h1; h.ts2 = ts.h2;
    Hash128 g;
    g.mix(t.h1); g.mix(t.h2); g.mix(ts.h1); g.mix(ts.h2);
    g.span(rd, h.sp[SP_CN][0], h.sp[SP_CN][1]);
    g.span(rd, h.sp[SP_KN][0], h.sp[SP_KN][1]);
    g.span(rd, h.sp[SP_KT][0], h.sp[SP_KT][1]);
    g.finish();
    h.h1 = g.h1; h.h2 = g.h2;
  }
}

// ---- one table_schema per (message, schema, table) ----------------------------------------------------------------------------------------------------
// RestoreChangeItems builds its name -> ColSchema map from the FIRST item of a TableID in the message.  Slots are claimed by a 64-bit key of
// (message, table id hash); two ids that share a key can only send an item to the host that did not have to go.
__device__ bool spans_equal(MemBytes &rd, const uint32_t *a, const uint32_t *b) {
  if (a[1] - a[0] != b[1] - b[0]) return false;
  for (uint32_t i = 0, n = a[1] - a[0]; i < n; i++) if (rd.at(a[0] + i) != rd.at(b[0] + i)) return false;
  return true;
}
__device__ __forceinline__ uint64_t tid_key(const Item &it, const Hdr &h) {
  uint64_t k = (h.tid ^ ((uint64_t)it.msg * 0x9E3779B97F4A7C15ull));
  k ^= k >> 29;
  return k == 0 ? 1 : k;
}
__global__ void __launch_bounds__(256) natp_tid_insert(const Item *__restrict__ items, const Hdr *__restrict__ hdrs, int64_t n, unsigned long long *keys, uint32_t *first, uint32_t mask,
                                                       uint32_t *__restrict__ slotof) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Hdr &h = hdrs[i];
  if (!(h.flags & IT_HEADER_OK)) return;
  const unsigned long long k = tid_key(items[i], h);
  uint32_t slot = (uint32_t)(k >> 7) & mask;
  for (;;) {
    unsigned long long o = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == 0) o = atomicCAS(&keys[slot], 0ull, k);
    if (o == 0 || o == k) break;
    slot = (slot + 1) & mask;
  }
  slotof[i] = slot;
  atomicMin(&first[slot], (uint32_t)i);
}
__global__ void __launch_bounds__(256) natp_tid_check(const uint8_t *data, const Item *__restrict__ items, Hdr *__restrict__ hdrs, int64_t n, const uint32_t *__restrict__ first,
                                                      const uint32_t *__restrict__ slotof, unsigned long long *mflag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Hdr &h = hdrs[i];
  if (!(h.flags & IT_HEADER_OK)) return;
  const Hdr &f = hdrs[first[slotof[i]]];
  MemBytes rd(data);
  if (f.ts1 != h.ts1 || f.ts2 != h.ts2 || !spans_equal(rd, f.sp[SP_TS], h.sp[SP_TS])) {  // (a hash never decides alone)
    h.flags &= ~IT_HEADER_OK;
    atomicMin(&mflag[items[i].msg], (unsigned long long)flag_key(items[i].idx, -1, TFGPU_NATIVE_SCHEMA_DIFFERS));
  }
}

// ---- grouping ------------------------------------------------------------------------------------------------------------------------------------------
__device__ bool strings_equal(MemBytes &rd, const uint32_t *a, const uint32_t *b) {
  sr::RuneIter x{&rd, nullptr, a[1] ? a[0] + 1 : 0u, a[1] ? a[1] - 1 : 0u}, y{&rd, nullptr, b[1] ? b[0] + 1 : 0u, b[1] ? b[1] - 1 : 0u};  // (absent: the empty string)
  return sr::rune_compare(x, y) == 0;
}
__device__ bool same_group(MemBytes &rd, const Hdr &a, const Hdr &b) {
  return strings_equal(rd, a.sp[SP_SCHEMA], b.sp[SP_SCHEMA]) && strings_equal(rd, a.sp[SP_TABLE], b.sp[SP_TABLE]) && strings_equal(rd, a.sp[SP_PART], b.sp[SP_PART]) &&
         spans_equal(rd, a.sp[SP_CN], b.sp[SP_CN]) && spans_equal(rd, a.sp[SP_KN], b.sp[SP_KN]) && spans_equal(rd, a.sp[SP_KT], b.sp[SP_KT]) &&
         spans_equal(rd, a.sp[SP_TS], b.sp[SP_TS]);
}
__global__ void __launch_bounds__(256) natp_intern(const uint8_t *data, const Hdr *__restrict__ hdrs, int64_t n, uint32_t *owner, uint32_t mask, uint32_t *__restrict__ slotof, int weak) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Hdr &h = hdrs[j];
  if (!(h.flags & IT_HEADER_OK)) { slotof[j] = 0; return; }
  const uint64_t a = weak ? (h.h1 & 3ull) : h.h1, b = weak ? 0ull : h.h2;
  MemBytes rd(data);
  uint32_t slot = (uint32_t)(b ^ (a >> 17)) & mask;
  for (;;) {
    uint32_t o = __hip_atomic_load(&owner[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == NOROW) o = atomicCAS(&owner[slot], NOROW, (uint32_t)j);
    if (o == NOROW || o == (uint32_t)j) break;
    const Hdr &oh = hdrs[o];
    if ((weak ? (oh.h1 & 3ull) : oh.h1) == a && (weak ? 0ull : oh.h2) == b && same_group(rd, h, oh)) break;
    slot = (slot + 1) & mask;  // another key: probe on (the table has at least 2n slots for n items)
  }
  slotof[j] = slot;
}
__global__ void __launch_bounds__(256) natp_keep(const Item *__restrict__ items, const Hdr *__restrict__ hdrs, int64_t n, const unsigned long long *__restrict__ mflag,
                                                 uint32_t *__restrict__ keep, int final_round) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keep[i] = (hdrs[i].flags & IT_HEADER_OK) && (!final_round || mflag[items[i].msg] == NOFLAG) ? 1u : 0u;
}
// the sort keys: an item left out (NOROW) sorts behind the last group; start[] is preset to "no item" = n
__global__ void __launch_bounds__(256) natp_sort_keys(uint32_t *__restrict__ gid, int64_t n, uint32_t T, uint32_t *__restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && gid[i] >= T) gid[i] = T;
  if (i <= (int64_t)T) start[i] = (uint32_t)n;
}
__global__ void __launch_bounds__(256) natp_rows(const uint32_t *__restrict__ sgid, const uint32_t *__restrict__ sel, const uint32_t *__restrict__ start, int64_t n, uint32_t T,
                                                 int32_t *__restrict__ item_group, uint32_t *__restrict__ item_row) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const uint32_t g = sgid[q], i = sel[q];
  if (g < T) { item_group[i] = (int32_t)g; item_row[i] = (uint32_t)q - start[g]; }
  else { item_group[i] = -1; item_row[i] = 0; }
}

// ---- cells -----------------------------------------------------------------------------------------------------------------------------------------------
struct OutCol { void *values; int32_t *nanos; uint32_t *valid; uint32_t *seg; uint8_t *data; };  // seg: the text lengths, then (scanned in place) the offsets
struct GroupOut {
  const ColOp *ops; const OutCol *cols;  // ncols value columns, then nkeys OldKeys columns
  uint32_t ncols, nkeys, has_any, unreadable;
  uint8_t *kind, *names_form; uint32_t *present;
  uint32_t *id; uint64_t *lsn, *commit; int64_t *counter;
  uint32_t *tx_seg, *q_seg; uint8_t *tx_data, *q_data;
};

// the bytes between a string's quotes, one at a time; -1 behind the last.  Times and base64 are read as they are SPELLED: a spelling with an
// escape (or a byte beyond ASCII) is none of the forms below and goes to the host
struct RawChars {
  MemBytes &rd; uint32_t p, e;
  __device__ __forceinline__ int next() { return p < e ? (int)rd.at(p++) : -1; }
};
// time.Parse(time.RFC3339Nano, s) for the forms the device takes: 0, or TFGPU_NATIVE_TIME_FORM / _TIME_ZONE
__device__ __forceinline__ uint32_t parse_time(MemBytes &rd, const Cell &c, int64_t &sec, int32_t &ns) {
  RawChars it{rd, c.s + 1, c.e - 1};
  bool ok = true;
  auto num = [&](int digits) { int v = 0; for (int i = 0; i < digits; i++) { const int r = it.next(); if (r < '0' || r > '9') { ok = false; return 0; } v = v * 10 + (r - '0'); } return v; };
  auto lit = [&](int ch) { if (it.next() != ch) ok = false; };
  const int y = num(4); lit('-'); const int mo = num(2); lit('-'); const int d = num(2); lit('T');
  const int hh = num(2); lit(':'); const int mi = num(2); lit(':'); const int ss = num(2);
  if (!ok) return TFGPU_NATIVE_TIME_FORM;
  int r = it.next();
  int64_t frac = 0;
  if (r == '.') {
    int nd = 0;
    for (r = it.next(); r >= '0' && r <= '9'; r = it.next()) { if (++nd > 9) return TFGPU_NATIVE_TIME_FORM; frac = frac * 10 + (r - '0'); }
    if (nd == 0) return TFGPU_NATIVE_TIME_FORM;
    for (; nd < 9; nd++) frac *= 10;
  }
  const bool zone = r == '+' || r == '-';
  if (zone) { num(2); lit(':'); num(2); }
  else if (r != 'Z') return TFGPU_NATIVE_TIME_FORM;
  if (!ok || it.next() >= 0) return TFGPU_NATIVE_TIME_FORM;
  if (zone) return TFGPU_NATIVE_TIME_ZONE;
  if (mo < 1 || mo > 12 || d < 1 || d > (mo == 2 ? 28 + ((y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 1 : 0) : 30 + ((0x15AA >> mo) & 1)) || hh > 23 || mi > 59 || ss > 59) return TFGPU_NATIVE_TIME_FORM;
  sec = dev::days_from_civil(y, mo, d) * 86400ll + hh * 3600 + mi * 60 + ss;
  ns = (int32_t)frac;
  return 0;
}
// base64.StdEncoding over the string as it is spelled: true when it is padded standard base64 (white space is left to the host)
template <class S> __device__ __forceinline__ bool base64_cell(S &o, MemBytes &rd, const Cell &c) {
  RawChars it{rd, c.s + 1, c.e - 1};
  uint32_t acc = 0, k = 0, pads = 0;
  bool closed = false;
  for (int r; (r = it.next()) >= 0;) {
    if (closed) return false;
    uint32_t v;
    if (r >= 'A' && r <= 'Z') v = (uint32_t)r - 'A';
    else if (r >= 'a' && r <= 'z') v = (uint32_t)r - 'a' + 26;
    else if (r >= '0' && r <= '9') v = (uint32_t)r - '0' + 52;
    else if (r == '+') v = 62;
    else if (r == '/') v = 63;
    else if (r == '=') { if (k < 2) return false; v = 0; pads++; }
    else return false;
    if (pads && r != '=') return false;
    acc = (acc << 6) | v;
    if (++k == 4) {
      o.put(acc >> 16);
      if (pads < 2) o.put((acc >> 8) & 0xFF);
      if (pads < 1) o.put(acc & 0xFF);
      if (pads) closed = true;
      acc = 0; k = 0;
    }
  }
  return k == 0;
}
// a string element of an array, at any depth of arrays (Restore recurses into []any with the same column, not into maps)
__device__ bool array_has_string(MemBytes &rd, uint32_t a, uint32_t b) {
  for (uint32_t pos = a; pos < b;) {
    const uint32_t c = rd.at(pos);
    if (c == '"') return true;
    if (c == '{') { uint32_t vt; skip_valid(rd, pos, b, vt); continue; }
    pos++;
  }
  return false;
}
__device__ __forceinline__ bool int_fits(int dtype, bool neg, uint64_t mag) {
  if (neg && mag == 0) return true;  // -0
  switch (dtype) {
    case TFGPU_T_INT8: return neg ? mag <= 128ull : mag <= 127ull;
    case TFGPU_T_INT16: return neg ? mag <= 32768ull : mag <= 32767ull;
    case TFGPU_T_INT32: return neg ? mag <= 2147483648ull : mag <= 2147483647ull;
    case TFGPU_T_INT64: return neg ? mag <= 9223372036854775808ull : mag <= 9223372036854775807ull;
    case TFGPU_T_UINT8: return !neg && mag <= 0xFFull;
    case TFGPU_T_UINT16: return !neg && mag <= 0xFFFFull;
    case TFGPU_T_UINT32: return !neg && mag <= 0xFFFFFFFFull;
    default: return !neg;
  }
}
// Is the cell one the device takes?  0, or the reason.  `canon`: an `any` value whose objects do not hold their keys ascending
__device__ uint32_t check_cell(MemBytes &rd, const ColOp op, const Cell &c, bool &canon) {
  const uint32_t t = c.vt & sr::VT_MASK;
  if (op.op == OP_FALLBACK) return op.reason;
  if (t == sr::VT_NULL) return 0;
  if (t == sr::VT_ARR && op.op != OP_ANY) return TFGPU_NATIVE_VALUE_TYPE;  // Restore maps itself over []any: a list, which no column holds
  switch (op.op) {
    case OP_INT: case OP_INTERVAL: {
      if (t == sr::VT_STR) return op.op == OP_INT ? TFGPU_NATIVE_NUM_STRING : TFGPU_NATIVE_VALUE_TYPE;
      if (t != sr::VT_NUM) return TFGPU_NATIVE_VALUE_TYPE;
      bool neg; uint64_t mag;
      if (!literal_u64(rd, c.s, c.e, neg, mag) || !int_fits(op.op == OP_INT ? op.dtype : TFGPU_T_INT64, neg, mag)) return TFGPU_NATIVE_INT_FORM;
      return 0;
    }
    case OP_JSONNUM: return t == sr::VT_NUM ? 0 : t == sr::VT_STR ? TFGPU_NATIVE_NUM_STRING : TFGPU_NATIVE_VALUE_TYPE;
    case OP_BOOL: return t == sr::VT_TRUE || t == sr::VT_FALSE ? 0 : TFGPU_NATIVE_VALUE_TYPE;
    case OP_STRING: return t == sr::VT_STR ? 0 : TFGPU_NATIVE_STRING_NONSTRING;
    case OP_BASE64: {
      if (t == sr::VT_NUM && (op.flags & F_MYSQL_BIT)) return TFGPU_NATIVE_MYSQL_BIT;
      if (t != sr::VT_STR) return TFGPU_NATIVE_STRING_NONSTRING;
      sr::CountSink n;
      return base64_cell(n, rd, c) ? 0 : TFGPU_NATIVE_BASE64;
    }
    case OP_TIME: {
      if (t == sr::VT_NUM) return TFGPU_NATIVE_TIME_FORM;
      if (t != sr::VT_STR) return TFGPU_NATIVE_VALUE_TYPE;
      int64_t s; int32_t ns;
      return parse_time(rd, c, s, ns);
    }
    default: {  // OP_ANY
      const bool str = t == sr::VT_STR || (t == sr::VT_ARR && array_has_string(rd, c.s, c.e));
      if (str && !(op.flags & F_ANY_STRING_OK)) return (op.flags & F_ANY_PG_TIMESTAMP) ? TFGPU_NATIVE_ANY_PG_TIMESTAMP : TFGPU_NATIVE_ANY_STRING;
      if (t == sr::VT_OBJ || t == sr::VT_ARR) {
        const int ord = sr::any_keys_order(rd, c.s, c.e - c.s);
        if (ord == 2) return TFGPU_NATIVE_DEPTH;
        if (ord == 1) canon = true;
      }
      return 0;
    }
  }
}

__global__ void __launch_bounds__(128) natp_validate(const uint8_t *data, const Item *__restrict__ items, Hdr *__restrict__ hdrs, int64_t n, const uint32_t *__restrict__ gid,
                                                     const GroupOut *__restrict__ groups, unsigned long long *mflag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Hdr &h = hdrs[i];
  if (!(h.flags & IT_HEADER_OK)) return;
  const Item it = items[i];
  const GroupOut &G = groups[gid[i]];
  MemBytes rd(data);
  uint32_t why = 0; int32_t col = -1;
  bool canon = false;
  if (G.unreadable) why = TFGPU_NATIVE_SCHEMA_COLUMN;
  Cell c;
  if (!why && h.sp[SP_CV][1]) {
    uint32_t pos = h.sp[SP_CV][0] + 1;
    for (uint32_t k = 0; k < G.ncols && next_elem(rd, pos, h.sp[SP_CV][1], c); k++)
      if ((why = check_cell(rd, G.ops[k], c, canon))) { col = (int32_t)k; break; }
  }
  if (!why && h.kind != TFGPU_K_INSERT && h.sp[SP_KV][1]) {
    uint32_t pos = h.sp[SP_KV][0] + 1;
    for (uint32_t k = 0; k < G.nkeys && next_elem(rd, pos, h.sp[SP_KV][1], c); k++)
      if ((why = check_cell(rd, G.ops[G.ncols + k], c, canon))) { col = (int32_t)(G.ncols + k); break; }
  }
  if (why) atomicMin(&mflag[it.msg], (unsigned long long)flag_key(it.idx, col, why));
  else if (canon) h.flags |= IT_CANON;
}

__device__ __forceinline__ void set_valid(uint32_t *bits, uint32_t row) { atomicOr(&bits[row >> 5], 1u << (row & 31)); }

template <bool COUNT> __device__ __forceinline__ void put_cell(MemBytes &rd, const ColOp op, const OutCol &o, uint32_t row, const Cell &c) {
  const uint32_t t = c.vt & sr::VT_MASK;
  if (t == sr::VT_NULL) return;
  if (!COUNT && o.valid) set_valid(o.valid, row);
  switch (op.op) {
    case OP_INT: case OP_INTERVAL: {
      if (COUNT) return;
      bool neg; uint64_t mag;
      literal_u64(rd, c.s, c.e, neg, mag);
      const uint64_t v = neg ? 0ull - mag : mag;
      const int dt = op.op == OP_INT ? op.dtype : TFGPU_T_INT64;
      if (dt == TFGPU_T_INT8 || dt == TFGPU_T_UINT8) ((uint8_t *)o.values)[row] = (uint8_t)v;
      else if (dt == TFGPU_T_INT16 || dt == TFGPU_T_UINT16) ((uint16_t *)o.values)[row] = (uint16_t)v;
      else if (dt == TFGPU_T_INT32 || dt == TFGPU_T_UINT32) ((uint32_t *)o.values)[row] = (uint32_t)v;
      else ((uint64_t *)o.values)[row] = v;
      return;
    }
    case OP_BOOL: if (!COUNT) ((uint8_t *)o.values)[row] = t == sr::VT_TRUE ? 1 : 0; return;
    case OP_TIME: {
      if (COUNT) return;
      int64_t s = 0; int32_t ns = 0;
      parse_time(rd, c, s, ns);
      ((int64_t *)o.values)[row] = s; o.nanos[row] = ns;
      return;
    }
    case OP_JSONNUM:
      if (COUNT) o.seg[row] = c.e - c.s;
      else { sr::ByteSink s{o.data + o.seg[row]}; for (uint32_t p = c.s; p < c.e; p++) s.put(rd.at(p)); s.flush(); }
      return;
    case OP_STRING:
      if (COUNT) { sr::CountSink s; sr::emit_unquoted(s, rd, c.s, c.e - c.s); o.seg[row] = s.n; }
      else { sr::ByteSink s{o.data + o.seg[row]}; sr::emit_unquoted(s, rd, c.s, c.e - c.s); s.flush(); }
      return;
    case OP_BASE64:
      if (COUNT) { sr::CountSink s; base64_cell(s, rd, c); o.seg[row] = s.n; }
      else { sr::ByteSink s{o.data + o.seg[row]}; base64_cell(s, rd, c); s.flush(); }
      return;
    default: return;  // OP_ANY: natp_any
  }
}

struct CellsParams {
  const uint8_t *data; const Item *items; const Hdr *hdrs; int64_t n;
  const int32_t *item_group; const uint32_t *item_row; const GroupOut *groups;
};
template <bool COUNT> __global__ void __launch_bounds__(128) natp_cells(CellsParams P) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  const int32_t g = P.item_group[i];
  if (g < 0) return;
  const GroupOut &G = P.groups[g];
  const Hdr &h = P.hdrs[i];
  const uint32_t row = P.item_row[i];
  MemBytes rd(P.data);
  if (!COUNT) {
    G.kind[row] = h.kind; G.names_form[row] = h.names_form;
    G.id[row] = h.id; G.lsn[row] = h.lsn; G.commit[row] = h.commit; G.counter[row] = h.counter;
    if (G.nkeys && h.nkv) set_valid(G.present, row);
  }
  // every text of the item goes through ONE put_cell (so the rune decoder is inlined once and nothing is called): tx_id and query are the string
  // cells of two columns of their own in front of the value columns and the OldKeys columns
  uint32_t pcv = h.sp[SP_CV][1] ? h.sp[SP_CV][0] + 1 : 0u, pkv = h.kind != TFGPU_K_INSERT && h.sp[SP_KV][1] ? h.sp[SP_KV][0] + 1 : 0u;
  const uint32_t total = 2 + G.ncols + G.nkeys;
  for (uint32_t k = 0; k < total; k++) {
    Cell c; ColOp op; OutCol o;
    if (k < 2) {
      const uint32_t *sp = h.sp[SP_TX + k];
      if (!sp[1]) continue;
      c = Cell{sp[0], sp[1], sr::VT_STR}; op = ColOp{OP_STRING, 0, 0, 0};
      o = OutCol{nullptr, nullptr, nullptr, k ? G.q_seg : G.tx_seg, k ? G.q_data : G.tx_data};
    } else if (k - 2 < G.ncols) {
      if (!pcv || !next_elem(rd, pcv, h.sp[SP_CV][1], c)) { k = 1 + G.ncols; continue; }  // on to the OldKeys columns
      op = G.ops[k - 2]; o = G.cols[k - 2];
    } else {
      if (!pkv || !next_elem(rd, pkv, h.sp[SP_KV][1], c)) break;
      op = G.ops[k - 2]; o = G.cols[k - 2];
    }
    put_cell<COUNT>(rd, op, o, row, c);
  }
}

// `any` cells: json.Marshal of the decoded value.  CANON == false: the items whose `any` values hold their keys ascending (the source tokens, strings
// re-encoded); CANON == true: the others, through the sorting emitter — a launch of its own, made only when some item needs it
template <bool CANON, class S> __device__ __forceinline__ void any_cell(S &s, MemBytes &rd, const Cell &c) {
  if ((c.vt & sr::VT_MASK) == sr::VT_STR) sr::emit_go_string(s, rd, c.s, c.e - c.s);
  else if constexpr (CANON) sr::emit_any_canon(s, rd, c.s, c.e - c.s);
  else sr::emit_any(s, rd, c.s, c.e - c.s);
}
template <bool COUNT, bool CANON> __global__ void __launch_bounds__(128) natp_any(CellsParams P) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  const int32_t g = P.item_group[i];
  if (g < 0) return;
  const GroupOut &G = P.groups[g];
  const Hdr &h = P.hdrs[i];
  if (!G.has_any || ((h.flags & IT_CANON) != 0) != CANON) return;
  const uint32_t row = P.item_row[i];
  MemBytes rd(P.data);
  Cell c;
  for (int part = 0; part < 2; part++) {
    const uint32_t *sp = part ? h.sp[SP_KV] : h.sp[SP_CV];
    if (!sp[1] || (part && h.kind == TFGPU_K_INSERT)) continue;
    const uint32_t k0 = part ? G.ncols : 0u, kn = part ? G.nkeys : G.ncols;
    uint32_t pos = sp[0] + 1;
    for (uint32_t k = 0; k < kn && next_elem(rd, pos, sp[1], c); k++) {
      if (G.ops[k0 + k].op != OP_ANY || (c.vt & sr::VT_MASK) == sr::VT_NULL) continue;
      const OutCol &o = G.cols[k0 + k];
      if (COUNT) { sr::CountSink s; any_cell<CANON>(s, rd, c); o.seg[row] = s.n; }
      else { sr::ByteSink s{o.data + o.seg[row]}; any_cell<CANON>(s, rd, c); s.flush(); }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
struct HashKey { uint64_t a, b; bool operator<(const HashKey &o) const { return a != o.a ? a < o.a : b < o.b; } };
struct CacheEntry { std::string texts[7]; std::shared_ptr<const GroupInfo> info; };
static std::mutex g_cache_mu;
static std::map<HashKey, std::vector<CacheEntry>> g_cache;  // by the group hash; under an equal hash the texts decide

struct Group {
  std::shared_ptr<const GroupInfo> info;
  std::unique_ptr<tfgpu_dbatch> batch;
  tfgpu_row_meta meta{};
  Buf id, lsn, commit, counter, names_form;
  TextSegments text;  // tx_id, query, then the text columns
  std::vector<uint64_t> totals;  // their totals, copied out of the read-back ring
  Buf tx_data, q_data;
  int64_t nrows = 0;
};

}  // namespace natp
}  // namespace tf

struct tfgpu_native_parsed {
  int lane = 0;
  std::vector<tf::natp::Group> groups;
  std::vector<int64_t> item_msg, item_row;
  std::vector<int32_t> item_group;
  std::vector<tfgpu_native_unparsed> fallback;
};

using namespace tf;
using namespace tf::natp;

extern "C" {

int tfgpu_native_check_sizes(const tfgpu_message_batch *b) {
  TF_API_BEGIN
  const char *T = "native parser: ";
  if (!b) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "null batch");
  if (b->nmsg < 0) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "negative message count");
  if (b->mem != TFGPU_MEM_HOST && b->mem != TFGPU_MEM_DEVICE) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "bad mem");
  if (b->nmsg && !b->value_start) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "value_start is null");
  if (b->values_len && !b->values) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "the values buffer is null");
  if (b->nmsg > 0x7FFFFFFFll) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "more than 2^31-1 messages: split the batch");
  const uint64_t LIM = 0xFFFFFFF0ull;
  if (b->values_len >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the values reach 4 GiB (32-bit offsets; this also keeps the items below 2^31): split the batch");
  if (b->mem == TFGPU_MEM_HOST && b->nmsg > 0) {
    if (b->value_start[b->nmsg] >= LIM) return tf::fail(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the values reach 4 GiB (32-bit offsets; this also keeps the items below 2^31): split the batch");
    if (b->value_start[b->nmsg] > b->values_len) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "message offsets must be ascending and inside the buffer");
  }
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parse(const tfgpu_message_batch *b, tfgpu_native_parsed **out) {
  TF_API_BEGIN
  const char *T = "native parser: ";
  if (!out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parse: null argument");
  if (const int rc = tfgpu_native_check_sizes(b)) return rc;
  Context &cx = ctx();
  std::lock_guard<std::mutex> lk(cx.mu);
  hipStream_t st = cx.stream;
  const int64_t n = b->nmsg, na = std::max<int64_t>(n, 1);
  auto res = std::make_unique<tfgpu_native_parsed>();
  res->lane = current_lane();

  // ---- the batch in HBM -------------------------------------------------------------------------------------------------------------------------------
  Buf vdata, vstart, vnil;
  static const uint64_t ZERO1[1] = {0};
  const uint8_t *data = stage_bytes(b->values, b->values_len, b->mem, vdata);
  const uint64_t *start = n ? stage_array<uint64_t>(b->value_start, (size_t)n + 1, b->mem, vstart) : stage_array<uint64_t>(ZERO1, 1, TFGPU_MEM_HOST, vstart);
  const uint8_t *nil = stage_array<uint8_t>(b->value_nil, (size_t)(n + 7) / 8, b->mem, vnil);
  Buf status = dalloc_zero(16);
  { KernelTimer t("natp_check_batch", n); natp_check_batch<<<grid_for(n + 1, 256), 256, 0, st>>>(start, b->values_len, n, ptr<uint32_t>(status)); }
  {
    const uint32_t *hs = d2h_u32(status->p);
    tf::sync();
    if (*hs) return tf::fail(TFGPU_ERR_INVALID, std::string(T) + "message offsets must be ascending and inside the buffer");
  }

  // ---- the cut ------------------------------------------------------------------------------------------------------------------------------------------
  Buf count = dalloc_zero((size_t)(na + 1) * 4 + 16), mstat = dalloc_zero((size_t)na * 4 + 16), mflag = dalloc((size_t)na * 8 + 16);
  TF_HIP(hipMemsetAsync(mflag->p, 0xFF, (size_t)na * 8, st));
  if (n) { KernelTimer t("natp_cut_count", (int64_t)b->values_len); natp_cut<true><<<grid_for(n, 4), 256, 0, st>>>(data, start, nil, n, ptr<uint32_t>(count), ptr<uint32_t>(mstat), nullptr, nullptr); }
  exclusive_scan_u32(ptr<uint32_t>(count), ptr<uint32_t>(count), n, true);
  const uint32_t *htotal = d2h_u32(ptr<uint32_t>(count) + n);
  tf::sync();
  const int64_t ni = *htotal, nia = std::max<int64_t>(ni, 1);
  Buf items = dalloc((size_t)nia * sizeof(Item) + 16), hdrs = dalloc((size_t)nia * sizeof(Hdr) + 16);
  Buf item_group = dalloc((size_t)nia * 4 + 16), item_row = dalloc_zero((size_t)nia * 4 + 16);
  int64_t T_final = 0;
  std::vector<uint32_t> hstart;
  std::vector<std::shared_ptr<const GroupInfo>> infos;  // by final group
  if (ni) {
    { KernelTimer t("natp_cut_write", (int64_t)b->values_len); natp_cut<false><<<grid_for(n, 4), 256, 0, st>>>(data, start, nil, n, nullptr, ptr<uint32_t>(mstat), ptr<uint32_t>(count), ptr<Item>(items)); }
    { KernelTimer t("natp_header", ni); natp_header<<<grid_for(ni, 128), 128, 0, st>>>(data, ptr<Item>(items), ni, ptr<Hdr>(hdrs), ptr<unsigned long long>(mflag)); }
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)ni) cap <<= 1;
    Buf slotof = dalloc((size_t)ni * 4 + 16);
    {
      Buf keys = dalloc_zero((size_t)cap * 8), first = dalloc((size_t)cap * 4);
      TF_HIP(hipMemsetAsync(first->p, 0xFF, (size_t)cap * 4, st));
      KernelTimer t("natp_tid", ni);
      natp_tid_insert<<<grid_for(ni, 256), 256, 0, st>>>(ptr<Item>(items), ptr<Hdr>(hdrs), ni, ptr<unsigned long long>(keys), ptr<uint32_t>(first), (uint32_t)(cap - 1), ptr<uint32_t>(slotof));
      natp_tid_check<<<grid_for(ni, 256), 256, 0, st>>>(data, ptr<Item>(items), ptr<Hdr>(hdrs), ni, ptr<uint32_t>(first), ptr<uint32_t>(slotof), ptr<unsigned long long>(mflag));
    }
    // groups: slots, then ids by first appearance — once over the items whose header stands (the programs are compiled for these), once more over the
    // items that stay when the flagged messages have left
    static const bool weak = [] { const char *e = std::getenv("TFGPU_NATIVE_WEAK_HASH"); return e && e[0] == '1'; }();  // tests: almost every key collides, the spans decide
    Buf owner = dalloc((size_t)cap * 4), keep = dalloc((size_t)ni * 4 + 16), first = dalloc((size_t)cap * 4);
    Buf rank = dalloc((size_t)(ni + 1) * 4 + 16), gid = dalloc((size_t)ni * 4 + 16), reps = dalloc((size_t)ni * 4 + 16), idx = dalloc((size_t)ni * 4 + 16);
    {
      KernelTimer t("natp_intern", ni);
      TF_HIP(hipMemsetAsync(owner->p, 0xFF, (size_t)cap * 4, st));
      natp_intern<<<grid_for(ni, 256), 256, 0, st>>>(data, ptr<Hdr>(hdrs), ni, ptr<uint32_t>(owner), (uint32_t)(cap - 1), ptr<uint32_t>(slotof), weak ? 1 : 0);
    }
    auto number = [&](int final_round) -> int64_t {
      KernelTimer t("natp_ids", ni);
      natp_keep<<<grid_for(ni, 256), 256, 0, st>>>(ptr<Item>(items), ptr<Hdr>(hdrs), ni, ptr<unsigned long long>(mflag), ptr<uint32_t>(keep), final_round);
      TF_HIP(hipMemsetAsync(first->p, 0xFF, (size_t)cap * 4, st));
      intern_first<<<grid_for(ni, 256), 256, 0, st>>>(ptr<uint32_t>(slotof), ptr<uint32_t>(keep), ni, ptr<uint32_t>(first));
      intern_flag<<<grid_for(ni, 256), 256, 0, st>>>(ptr<uint32_t>(slotof), ptr<uint32_t>(keep), ptr<uint32_t>(first), ni, ptr<uint32_t>(rank));
      exclusive_scan_u32(ptr<uint32_t>(rank), ptr<uint32_t>(rank), ni, true);
      intern_ids<<<grid_for(ni, 256), 256, 0, st>>>(ptr<uint32_t>(slotof), ptr<uint32_t>(keep), ptr<uint32_t>(first), ptr<uint32_t>(rank), ni, NOROW, ptr<uint32_t>(gid), ptr<uint32_t>(reps), ptr<uint32_t>(idx));
      const uint32_t *hT = d2h_u32(ptr<uint32_t>(rank) + ni);
      tf::sync();
      return (int64_t)*hT;
    };
    const int64_t T0 = number(0);
    // host work once per distinct key: the representative's spans, read with the host JSON code, compiled to a program; kept across calls by the hash
    std::vector<std::shared_ptr<const GroupInfo>> info0((size_t)T0);
    std::vector<uint32_t> hreps((size_t)std::max<int64_t>(T0, 1));
    std::vector<Hdr> rep_hdr((size_t)T0);
    if (T0) {
      d2h(hreps.data(), reps->p, (size_t)T0 * 4);
      tf::sync();
      for (int64_t g = 0; g < T0; g++) d2h(&rep_hdr[(size_t)g], ptr<Hdr>(hdrs) + hreps[(size_t)g], sizeof(Hdr));
      tf::sync();
    }
    static const uint32_t WHICH[7] = {SP_SCHEMA, SP_TABLE, SP_PART, SP_CN, SP_TS, SP_KN, SP_KT};
    std::vector<std::array<std::string, 7>> all_texts((size_t)T0);  // every representative's texts, one sync for all of them
    for (int64_t g = 0; g < T0; g++)
      for (int q = 0; q < 7; q++) {
        const uint32_t a = rep_hdr[(size_t)g].sp[WHICH[q]][0], e = rep_hdr[(size_t)g].sp[WHICH[q]][1];
        if (e > a) { all_texts[(size_t)g][(size_t)q].resize(e - a); d2h(&all_texts[(size_t)g][(size_t)q][0], data + a, e - a); }
      }
    if (T0) tf::sync();
    for (int64_t g = 0; g < T0; g++) {
      const Hdr &h = rep_hdr[(size_t)g];
      const HashKey key{h.h1, h.h2};
      const std::array<std::string, 7> &texts = all_texts[(size_t)g];
      {
        std::lock_guard<std::mutex> cl(g_cache_mu);
        for (auto &ce : g_cache[key]) {
          bool same = true;
          for (int q = 0; q < 7; q++) same = same && ce.texts[q] == texts[q];
          if (same) { info0[(size_t)g] = ce.info; break; }
        }
      }
      if (!info0[(size_t)g]) {
        info0[(size_t)g] = compile_group(texts[0], texts[1], texts[2], texts[3], texts[4], texts[5], texts[6]);
        std::lock_guard<std::mutex> cl(g_cache_mu);
        if (g_cache.size() > 4096) g_cache.clear();
        CacheEntry ce;
        for (int q = 0; q < 7; q++) ce.texts[q] = texts[q];
        ce.info = info0[(size_t)g];
        g_cache[key].push_back(std::move(ce));
      }
    }
    // the programs on the device (upload_const: a steady stream uploads each once)
    std::vector<Buf> ops0((size_t)T0);
    std::vector<GroupOut> gout((size_t)std::max<int64_t>(T0, 1));
    for (int64_t g = 0; g < T0; g++) {
      const GroupInfo &gi = *info0[(size_t)g];
      GroupOut &o = gout[(size_t)g];
      o = GroupOut{};
      static const ColOp NONE{OP_FALLBACK, 0, 0, TFGPU_NATIVE_SCHEMA_COLUMN};
      ops0[(size_t)g] = gi.ops.empty() ? upload_const(&NONE, sizeof(ColOp)) : upload_const(gi.ops.data(), gi.ops.size() * sizeof(ColOp));
      o.ops = ptr<ColOp>(ops0[(size_t)g]);
      o.ncols = (uint32_t)gi.names.size(); o.nkeys = (uint32_t)gi.key_names.size(); o.has_any = gi.has_any; o.unreadable = gi.unreadable;
    }
    if (T0) {
      Buf dg = upload_small(gout.data(), gout.size() * sizeof(GroupOut));
      KernelTimer t("natp_validate", ni);
      natp_validate<<<grid_for(ni, 128), 128, 0, st>>>(data, ptr<Item>(items), ptr<Hdr>(hdrs), ni, ptr<uint32_t>(gid), ptr<GroupOut>(dg), ptr<unsigned long long>(mflag));
      tf::sync();  // (dg and gout are consumed)
    }
    T_final = T0 ? number(1) : 0;
    // rows: one stable sort of (group, item); the items that left carry T_final and sort behind the last group
    if (T_final) {
      std::vector<uint32_t> hreps1((size_t)T_final);
      d2h(hreps1.data(), reps->p, (size_t)T_final * 4);
      hstart.assign((size_t)T_final + 1, 0u);
      unsigned bits = 1;
      while ((1ull << bits) < (uint64_t)T_final + 1) bits++;
      Buf sgid = dalloc((size_t)ni * 4 + 16), sel = dalloc((size_t)ni * 4 + 16), dstart = dalloc((size_t)(T_final + 1) * 4 + 16);
      size_t tmp_bytes = 0;
      TF_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, ptr<uint32_t>(gid), ptr<uint32_t>(sgid), ptr<uint32_t>(idx), ptr<uint32_t>(sel), (size_t)ni, 0u, bits, st));
      Buf tmp = dalloc(tmp_bytes + 16);
      {
        KernelTimer t("natp_rows", ni);
        natp_sort_keys<<<grid_for(std::max<int64_t>(ni, T_final + 1), 256), 256, 0, st>>>(ptr<uint32_t>(gid), ni, (uint32_t)T_final, ptr<uint32_t>(dstart));
        TF_HIP(rocprim::radix_sort_pairs(tmp->p, tmp_bytes, ptr<uint32_t>(gid), ptr<uint32_t>(sgid), ptr<uint32_t>(idx), ptr<uint32_t>(sel), (size_t)ni, 0u, bits, st));
        intern_heads<<<grid_for(ni, 256), 256, 0, st>>>(ptr<uint32_t>(sgid), ni, ptr<uint32_t>(dstart));
        natp_rows<<<grid_for(ni, 256), 256, 0, st>>>(ptr<uint32_t>(sgid), ptr<uint32_t>(sel), ptr<uint32_t>(dstart), ni, (uint32_t)T_final, ptr<int32_t>(item_group), ptr<uint32_t>(item_row));
      }
      d2h(hstart.data(), dstart->p, hstart.size() * 4);
      // which compiled key each final group is: two items share a slot exactly when they share a key
      std::vector<uint32_t> hslot((size_t)ni);
      d2h(hslot.data(), slotof->p, (size_t)ni * 4);
      tf::sync();  // (hreps1, hstart, hslot; tmp)
      std::unordered_map<uint32_t, int64_t> by_slot;
      for (int64_t q = 0; q < T0; q++) by_slot[hslot[hreps[(size_t)q]]] = q;
      infos.resize((size_t)T_final);
      for (int64_t g = 0; g < T_final; g++) infos[(size_t)g] = info0[(size_t)by_slot.at(hslot[hreps1[(size_t)g]])];
    } else {
      TF_HIP(hipMemsetAsync(item_group->p, 0xFF, (size_t)ni * 4, st));
    }
  }

  // ---- the groups' batches ----------------------------------------------------------------------------------------------------------------------------------
  res->groups.resize((size_t)T_final);
  std::vector<GroupOut> gout((size_t)std::max<int64_t>(T_final, 1));
  std::vector<std::vector<OutCol>> ocols((size_t)T_final);
  std::vector<Buf> keepalive;
  bool any_cols = false;
  for (int64_t g = 0; g < T_final; g++) {
    Group &G = res->groups[(size_t)g];
    G.info = infos[(size_t)g];
    const GroupInfo &gi = *G.info;
    const int64_t nr = (int64_t)hstart[(size_t)g + 1] - (int64_t)hstart[(size_t)g], nra = std::max<int64_t>(nr, 1);
    G.nrows = nr;
    G.batch = std::make_unique<tfgpu_dbatch>();
    tfgpu_dbatch &db = *G.batch;
    db.nrows = nr; db.ns = gi.ns; db.table = gi.table;
    for (auto &c : gi.schema) { db.schema.emplace_back(c.name, c.dtype); if (c.flags & TFGPU_COL_KEY) db.key_names.push_back(c.name); }
    const int ncols = (int)gi.names.size(), nkeys = (int)gi.key_names.size();
    ValidityBlock vb(ncols + nkeys + 1, nr);
    int nseg = 2;
    for (auto &op : gi.ops) if (repr_is_var(repr_of(op))) nseg++;
    G.text = TextSegments(nseg, nr);
    std::vector<OutCol> &oc = ocols[(size_t)g];
    int seg = 2;
    for (int k = 0; k < ncols + nkeys; k++) {
      DColumn d;
      d.name = k < ncols ? gi.names[(size_t)k] : gi.key_names[(size_t)(k - ncols)];
      d.dtype = gi.ops[(size_t)k].dtype; d.repr = repr_of(gi.ops[(size_t)k]);
      d.validity = vb.col(k);
      OutCol o{};
      o.valid = ptr<uint32_t>(d.validity);
      if (repr_is_var(d.repr)) { o.seg = G.text.seg(seg); d.offsets = G.text.offsets(seg); seg++; }
      else {
        d.values = dalloc((size_t)nra * repr_width(d.repr) + 16);
        TF_HIP(hipMemsetAsync(d.values->p, 0, (size_t)nra * repr_width(d.repr), st));
        o.values = d.values->p;
        if (d.repr == TFGPU_R_TIME) { d.nanos = dalloc_zero((size_t)nra * 4 + 16); o.nanos = ptr<int32_t>(d.nanos); }
      }
      oc.push_back(o);
      (k < ncols ? db.cols : db.old_keys).push_back(std::move(d));
    }
    db.kind = dalloc((size_t)nra + 16);
    if (nkeys) db.old_present = vb.col(ncols + nkeys);
    G.id = dalloc((size_t)nra * 4 + 16); G.lsn = dalloc((size_t)nra * 8 + 16); G.commit = dalloc((size_t)nra * 8 + 16); G.counter = dalloc((size_t)nra * 8 + 16);
    G.names_form = dalloc((size_t)nra + 16);
    GroupOut &o = gout[(size_t)g];
    o = GroupOut{};
    Buf ops = gi.ops.empty() ? Buf() : upload_const(gi.ops.data(), gi.ops.size() * sizeof(ColOp));
    keepalive.push_back(ops);
    o.ops = ptr<ColOp>(ops);
    o.ncols = (uint32_t)ncols; o.nkeys = (uint32_t)nkeys; o.has_any = gi.has_any;
    any_cols = any_cols || gi.has_any;
    o.kind = ptr<uint8_t>(db.kind); o.names_form = ptr<uint8_t>(G.names_form); o.present = ptr<uint32_t>(db.old_present);
    o.id = ptr<uint32_t>(G.id); o.lsn = ptr<uint64_t>(G.lsn); o.commit = ptr<uint64_t>(G.commit); o.counter = ptr<int64_t>(G.counter);
    o.tx_seg = G.text.seg(0); o.q_seg = G.text.seg(1);
  }
  Buf dgroups, dcols;
  auto upload_tables = [&]() {
    size_t total = 0;
    for (auto &v : ocols) total += v.size();
    std::vector<OutCol> flat;
    flat.reserve(total + 1);
    std::vector<size_t> at;
    for (auto &v : ocols) { at.push_back(flat.size()); flat.insert(flat.end(), v.begin(), v.end()); }
    if (flat.empty()) flat.push_back(OutCol{});
    dcols = upload_small(flat.data(), flat.size() * sizeof(OutCol));
    for (int64_t g = 0; g < T_final; g++) gout[(size_t)g].cols = ptr<OutCol>(dcols) + at[(size_t)g];
    dgroups = upload_small(gout.data(), gout.size() * sizeof(GroupOut));
  };
  const int64_t ni_now = ni;  // (NOT *htotal again: the pinned ring has been written since)
  CellsParams P{data, ptr<Item>(items), ptr<Hdr>(hdrs), ni_now, ptr<int32_t>(item_group), ptr<uint32_t>(item_row), nullptr};
  if (T_final) {
    upload_tables();
    P.groups = ptr<GroupOut>(dgroups);
    { KernelTimer t("natp_cells_len", ni_now); natp_cells<true><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
    if (any_cols) {
      { KernelTimer t("natp_any_len", ni_now); natp_any<true, false><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
      { KernelTimer t("natp_any_len_canon", ni_now); natp_any<true, true><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
    }
    // The scans' totals come back through the pinned ring, which later read-backs reuse: they are copied out a bounded piece of the ring at a time
    {
      size_t from = 0, pinned = 0;
      auto collect = [&](size_t to) {
        tf::sync();
        for (size_t g = from; g < to; g++) {
          Group &G = res->groups[g];
          int nseg = 2;
          for (auto &op : G.info->ops) if (repr_is_var(repr_of(op))) nseg++;
          G.totals.resize((size_t)nseg);
          for (int q = 0; q < nseg; q++) G.totals[(size_t)q] = G.text.total(q);
        }
        from = to; pinned = 0;
      };
      for (size_t g = 0; g < res->groups.size(); g++) {
        Group &G = res->groups[g];
        G.text.scan(true);
        pinned += 64 + 8 * (G.info->ops.size() + 2);
        if (pinned > (256u << 10)) collect(g + 1);
      }
      collect(res->groups.size());  // (the tables are consumed too)
    }
    for (int64_t g = 0; g < T_final; g++) {
      Group &G = res->groups[(size_t)g];
      tfgpu_dbatch &db = *G.batch;
      auto sized = [&](int sgi, const std::string &what) -> Buf {
        if (text_total_exceeds(G.totals[(size_t)sgi])) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + what + " of table " + db.table + " reaches 4 GiB of text (32-bit offsets): split the batch");
        return dalloc((size_t)G.totals[(size_t)sgi] + 16);
      };
      G.tx_data = sized(0, "tx_id"); G.q_data = sized(1, "query");
      gout[(size_t)g].tx_data = ptr<uint8_t>(G.tx_data); gout[(size_t)g].q_data = ptr<uint8_t>(G.q_data);
      int seg = 2, k = 0;
      for (auto *list : {&db.cols, &db.old_keys})
        for (auto &c : *list) {
          if (repr_is_var(c.repr)) {
            c.data = sized(seg, "column " + c.name);
            c.data_len = G.totals[(size_t)seg];
            ocols[(size_t)g][(size_t)k].data = ptr<uint8_t>(c.data);
            seg++;
          }
          k++;
        }
    }
    upload_tables();
    P.groups = ptr<GroupOut>(dgroups);
    { KernelTimer t("natp_cells_write", ni_now); natp_cells<false><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
    if (any_cols) {
      { KernelTimer t("natp_any_write", ni_now); natp_any<false, false><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
      { KernelTimer t("natp_any_write_canon", ni_now); natp_any<false, true><<<grid_for(ni_now, 128), 128, 0, st>>>(P); }
    }
  }

  // ---- what goes back to the host: the item map and the flagged messages ----------------------------------------------------------------------------------------
  std::vector<Item> hitems((size_t)ni_now);
  std::vector<int32_t> hgroup((size_t)ni_now);
  std::vector<uint32_t> hrow((size_t)ni_now), hmstat((size_t)na);
  std::vector<unsigned long long> hflag((size_t)na);
  if (ni_now) { d2h(hitems.data(), items->p, (size_t)ni_now * sizeof(Item)); d2h(hgroup.data(), item_group->p, (size_t)ni_now * 4); d2h(hrow.data(), item_row->p, (size_t)ni_now * 4); }
  if (n) { d2h(hmstat.data(), mstat->p, (size_t)n * 4); d2h(hflag.data(), mflag->p, (size_t)n * 8); }
  tf::sync();  // (also: the staged copies of the batch go back to the pool behind the kernels that read them)
  res->item_msg.resize((size_t)ni_now); res->item_row.resize((size_t)ni_now); res->item_group = hgroup;
  for (int64_t i = 0; i < ni_now; i++) { res->item_msg[(size_t)i] = hitems[(size_t)i].msg; res->item_row[(size_t)i] = hgroup[(size_t)i] < 0 ? -1 : (int64_t)hrow[(size_t)i]; }
  for (int64_t m = 0; m < n; m++) {
    if (hmstat[(size_t)m]) res->fallback.push_back({m, TFGPU_NATIVE_SYNTAX, -1, -1});
    else if (hflag[(size_t)m] != NOFLAG) {
      const unsigned long long k = hflag[(size_t)m];
      res->fallback.push_back({m, (int32_t)(k & 0xFF), (int32_t)(k >> 32), (int32_t)((k >> 8) & 0xFFFFFF) - 1});
    }
  }
  for (auto &G : res->groups) {
    tfgpu_row_meta &mt = G.meta;
    mt.id = ptr<uint32_t>(G.id); mt.lsn = ptr<uint64_t>(G.lsn); mt.commit_time = ptr<uint64_t>(G.commit); mt.counter = ptr<int64_t>(G.counter);
    mt.tx_id_offsets = G.text.seg(0); mt.tx_id_data = ptr<uint8_t>(G.tx_data);
    mt.query_offsets = G.text.seg(1); mt.query_data = ptr<uint8_t>(G.q_data);
    mt.names_form = ptr<uint8_t>(G.names_form);
    mt.n = G.nrows; mt.mem = TFGPU_MEM_DEVICE;
  }
  *out = res.release();
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parsed_info(const tfgpu_native_parsed *h, int64_t *nitems, int32_t *ngroups, int64_t *nfallback_msgs) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_info: null handle");
  if (nitems) *nitems = (int64_t)h->item_msg.size();
  if (ngroups) *ngroups = (int32_t)h->groups.size();
  if (nfallback_msgs) *nfallback_msgs = (int64_t)h->fallback.size();
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parsed_group(const tfgpu_native_parsed *h, int32_t g, tfgpu_dbatch **batch, const tfgpu_row_meta **meta, const char **part, const char *const **key_types,
                              int32_t *n_key_types) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_group: null handle");
  if (g < 0 || (size_t)g >= h->groups.size()) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_group: group index out of range");
  if (current_lane() != h->lane) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_group: the handle belongs to the lane that made it");
  const Group &G = h->groups[(size_t)g];
  if (batch) *batch = shallow_copy(*G.batch).release();
  if (meta) *meta = &G.meta;
  if (part) *part = G.info->part.c_str();
  if (key_types) *key_types = G.info->key_type_ptrs.empty() ? nullptr : G.info->key_type_ptrs.data();
  if (n_key_types) *n_key_types = (int32_t)G.info->key_type_ptrs.size();
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parsed_group_schema(const tfgpu_native_parsed *h, int32_t g, const tfgpu_schema **schema, const char **table_schema_json) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_group_schema: null handle");
  if (g < 0 || (size_t)g >= h->groups.size()) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_group_schema: group index out of range");
  const GroupInfo &gi = *h->groups[(size_t)g].info;
  if (schema) *schema = &gi.cschema;
  if (table_schema_json) *table_schema_json = gi.table_schema_json.empty() ? nullptr : gi.table_schema_json.c_str();
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parsed_items(const tfgpu_native_parsed *h, int64_t *msg, int32_t *group, int64_t *row) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_items: null handle");
  const size_t n = h->item_msg.size();
  if (n && msg) std::memcpy(msg, h->item_msg.data(), n * 8);
  if (n && group) std::memcpy(group, h->item_group.data(), n * 4);
  if (n && row) std::memcpy(row, h->item_row.data(), n * 8);
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_native_parsed_fallback(const tfgpu_native_parsed *h, tfgpu_native_unparsed *list, int64_t cap, int64_t *n) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_native_parsed_fallback: null handle");
  if (n) *n = (int64_t)h->fallback.size();
  if (list) for (int64_t k = 0; k < cap && k < (int64_t)h->fallback.size(); k++) list[k] = h->fallback[(size_t)k];
  return TFGPU_OK;
  TF_API_END
}

void tfgpu_native_parsed_free(tfgpu_native_parsed *h) { delete h; }

}  // extern "C"
