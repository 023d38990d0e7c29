// tf_rawdoc.hip — raw_doc_grouper on device (pkg/transformer/registry/raw_doc_grouper/raw_doc_grouper.go:65-109, 158-193; raw_data_utils.go):
// a row keeps the columns named in `keys` / `fields`, every column it lists is folded into one `doc` value — a Go map[string]interface{}, which the
// ABI holds as its json.Marshal text (TFGPU_R_JSON: compact, members in byte order of the key, no HTML escaping) — and etl_updated_at is the row's
// CommitTime as a time.Time.
//
//   rawdoc_commit_time   lane = row: time.Unix(0, int64(CommitTime[src_row[r]])) as seconds + nanoseconds (floor division)
//   rawdoc_kinds         lane = row: non-row kinds, and who carries OldKeys (inPlaceRemoveOldKeys touches Update rows only)
//   rawdoc_len<REST>     lane = row: the doc's members rendered into a counting sink; NaN / Inf floats and `_rest` texts the splice cannot take are flagged
//   (scan)               exclusive_scan_u32 over the lengths, their sum taken in 64 bits first
//   rawdoc_write<REST>   lane = row: the same walk into a WriteSink at the row's offset
//
// The host sorts the column names once per batch and uploads the pre-rendered `"name":` literals in that order, so a row without `_rest` is one
// pass over the sorted columns.  REST = true is for batches that have a TFGPU_R_JSON column named `_rest`: a cell whose text starts with '{' is the
// map[string]interface{} collectParsedData splices (its members, already in key order — what the generic parser's AddRest produces and what the ABI
// says an `any` text is — merged with the sorted columns); the JSON scanner it needs stays out of the kernels every other batch runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "tf_plan.hpp"
#include "tf_rows.hpp"
#include "tf_devrow.hpp"
#include "tf_emit.hpp"
#include "tf_jsonscan.hpp"

namespace tf {

enum : uint32_t {
  RD_NONROW = 1u,        // a kind above Delete
  RD_OLD_UPDATE = 2u,    // a row with OldKeys that is an Update
  RD_OLD_OTHER = 4u,     // a row with OldKeys that is not
  RD_BACKSLASH = 8u,     // a spliced `_rest` member key holds a backslash
  RD_BAD_REST = 16u,     // a `_rest` text that starts with '{' and is no JSON object (or nests deeper than the scanner follows)
  RD_META_SHORT = 32u,   // src_row reaches past meta->n
  RD_HUGE_CELL = 64u     // one text cell whose JSON text may reach 4 GiB (the 32-bit cell counter would wrap)
};
struct RawDocStatus { uint32_t flags, pad; unsigned long long nan_first, total; };  // nan_first: min of (row << 20 | sorted column) over the NaN / Inf cells

struct RawDocParams {
  const DCol *cols;              // every column of the batch a doc may hold, sorted by name
  const uint8_t *const *absent;  // [ncols] ABSENT bitmaps or null entries; null: every row lists every column
  const uint32_t *lit_off;       // [ncols + 1] into lit
  const uint8_t *lit;            // "name": of every column, json.Marshal'ed (no HTML escaping)
  const uint32_t *name_off;      // [ncols + 1] into names (REST)
  const uint8_t *names;          // the names' own bytes (REST: compared with the rest members' keys)
  const uint8_t *after_rest;     // [ncols] the column stands behind `_rest` in the batch: on an equal key it overwrites the rest member (REST)
  int32_t ncols, rest;           // rest: the sorted index of `_rest`, -1 without
  int64_t n;
  uint32_t *len;                 // rawdoc_len: [n] out
  const uint32_t *off;           // rawdoc_write: [n + 1]
  uint8_t *data;
  RawDocStatus *st;
};

__device__ __forceinline__ bool rd_listed(const RawDocParams &p, int k, int64_t r) { return !(p.absent && p.absent[k] && ((p.absent[k][r >> 3] >> (r & 7)) & 1)); }

// one member from a column: [,] "name": value.  COUNT: the sink is emptied into row64 behind every member (the doc's length is summed in 64 bits)
template <bool COUNT, class S> __device__ __forceinline__ void rd_col_member(const RawDocParams &p, int k, int64_t r, S &s, bool &first, uint64_t &row64, RawDocStatus *st) {
  const DCol &c = p.cols[k];
  const CellBits b = load_cell(c, r);
  if (!first) s.put(','); first = false;
  put_bytes(s, p.lit + p.lit_off[k], p.lit_off[k + 1] - p.lit_off[k]);
  if constexpr (COUNT) {
    if (b.valid && (c.repr == TFGPU_R_FLOAT32 || c.repr == TFGPU_R_FLOAT64)) {
      const double f = cell_f64(c, b);
      if (!(f - f == 0.0)) atomicMin(&st->nan_first, ((unsigned long long)r << 20) | (unsigned long long)k);  // NaN / ±Inf: json.Marshal has no text for it
    }
    if (b.valid && c.offsets && (uint32_t)(b.v >> 32) - (uint32_t)b.v > 0x2A000000u) atomicOr(&st->flags, (uint32_t)RD_HUGE_CELL);  // six bytes of text a byte at the most
  }
  emit_json_cell(s, c, b, 0, false);
  if constexpr (COUNT) { row64 += s.n; s.n = 0; }
}

// bytes [a, b) of the rest text, as they are
template <class S> __device__ __forceinline__ void rd_copy(S &s, const uint8_t *base, uint32_t a, uint32_t b) { put_bytes(s, base + a, b - a); }

// <0, 0, >0: column k's name against the key bytes [ka, kb) of the rest text
__device__ __forceinline__ int rd_name_cmp(const RawDocParams &p, int k, MemBytes &rd, uint32_t ka, uint32_t kb) {
  const uint8_t *nm = p.names + p.name_off[k];
  const uint32_t nn = p.name_off[k + 1] - p.name_off[k], kn = kb - ka, m = nn < kn ? nn : kn;
  for (uint32_t i = 0; i < m; i++) { const uint32_t x = nm[i], y = rd.at(ka + i); if (x != y) return x < y ? -1 : 1; }
  return nn < kn ? -1 : nn > kn ? 1 : 0;
}

// json.Marshal(docData) of row r (collectParsedData, raw_doc_grouper.go:158-193)
template <bool REST, bool COUNT, class S> __device__ __forceinline__ void emit_doc(const RawDocParams &p, int64_t r, S &s, uint64_t &row64) {
  bool first = true;
  s.put('{');
  int k = 0;
  bool splice = false;
  if constexpr (REST) {
    const DCol &rc = p.cols[p.rest];
    splice = rd_listed(p, p.rest, r) && is_valid(rc, r) && rc.offsets[r + 1] > rc.offsets[r] && rc.data[rc.offsets[r]] == '{';  // restMap, ok := colValue.(map[string]interface{})
    if (splice) {
      // the members of the rest object in their own (ascending) order, the sorted columns merged in between; on an equal key the later write of
      // the reference's loop over ColumnNames stays: a column behind `_rest`, else the rest member
      const uint32_t mis = (uint32_t)((uintptr_t)rc.data & 7u);
      const uint8_t *base = rc.data - mis;  // (MemBytes reads aligned words)
      MemBytes rd(base);
      uint32_t pos = mis + rc.offsets[r] + 1;
      const uint32_t end = mis + rc.offsets[r + 1];
      uint32_t bad = 0;
      auto skip_ws = [&]() { while (pos < end && sr::is_ws(rd.at(pos))) pos++; };
      skip_ws();
      if (pos < end && rd.at(pos) == '}') pos++;
      else for (;;) {
        skip_ws();
        if (pos >= end || rd.at(pos) != '"') { bad = RD_BAD_REST; break; }
        const uint32_t kq = pos;
        bool plain = false;
        if (!sr::scan_string(rd, pos, end, &plain)) { bad = RD_BAD_REST; break; }
        const uint32_t ka = kq + 1, kb = pos - 1, kend = pos;
        if (!plain) for (uint32_t i = ka; i < kb; i++) if (rd.at(i) == '\\') bad |= RD_BACKSLASH;  // its place among the names is that of the decoded bytes
        skip_ws();
        if (pos >= end || rd.at(pos) != ':') { bad = RD_BAD_REST; break; }
        pos++;
        skip_ws();
        const uint32_t va = pos;
        uint32_t vt = 0;
        if (sr::skip_value(rd, pos, end, vt) != 0) { bad = RD_BAD_REST; break; }
        const uint32_t vb = pos;
        int cmp = 1;
        while (k < p.ncols) {
          if (k == p.rest || !rd_listed(p, k, r)) { k++; continue; }
          cmp = rd_name_cmp(p, k, rd, ka, kb);
          if (cmp >= 0) break;
          rd_col_member<COUNT>(p, k, r, s, first, row64, p.st);
          k++;
        }
        bool member = true;
        if (k < p.ncols && cmp == 0) {
          if (p.after_rest[k]) { rd_col_member<COUNT>(p, k, r, s, first, row64, p.st); member = false; }
          k++;
        }
        if (member) {
          if (!first) s.put(','); first = false;
          rd_copy(s, base, kq, kend); s.put(':'); rd_copy(s, base, va, vb);
          if constexpr (COUNT) { row64 += s.n; s.n = 0; }
        }
        skip_ws();
        if (pos < end && rd.at(pos) == ',') { pos++; continue; }
        if (pos < end && rd.at(pos) == '}') { pos++; break; }
        bad = RD_BAD_REST; break;
      }
      skip_ws();
      if (!bad && pos != end) bad = RD_BAD_REST;
      if constexpr (COUNT) { if (bad) atomicOr(&p.st->flags, bad); }
    }
  }
  for (; k < p.ncols; k++) {
    if (REST && splice && k == p.rest) continue;
    if (!rd_listed(p, k, r)) continue;
    rd_col_member<COUNT>(p, k, r, s, first, row64, p.st);
  }
  s.put('}');
}

template <bool REST> __global__ void __launch_bounds__(256) rawdoc_len(RawDocParams p) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  CountSink s;
  uint64_t row64 = 0;
  emit_doc<REST, true>(p, r, s, row64);
  row64 += s.n;
  p.len[r] = row64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)row64;  // (saturated: the 64-bit sum of the lengths then reaches 4 GiB, which the host refuses)
}
template <bool REST> __global__ void __launch_bounds__(256) rawdoc_write(RawDocParams p) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  WriteSink s{p.data + p.off[r]};
  uint64_t unused = 0;
  emit_doc<REST, false>(p, r, s, unused);
  s.flush();
}

// etl_updated_at = time.Unix(0, int64(CommitTime)): a CommitTime of 2^63 and more is a negative instant
__global__ void __launch_bounds__(256) rawdoc_commit_time(const int32_t *__restrict__ src_row, const uint64_t *__restrict__ ct, int64_t meta_n, int64_t n, int64_t *__restrict__ sec,
                                                          int32_t *__restrict__ nsec, RawDocStatus *st) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int64_t v = 0;
  if (ct) {
    const int64_t i = src_row ? (int64_t)src_row[r] : r;
    if (i < 0 || i >= meta_n) atomicOr(&st->flags, (uint32_t)RD_META_SHORT);
    else v = (int64_t)ct[i];
  }
  const int64_t q = dev::floordiv(v, 1000000000ll);
  sec[r] = q;
  nsec[r] = (int32_t)(v - q * 1000000000ll);
}
__global__ void __launch_bounds__(256) rawdoc_kinds(const uint8_t *__restrict__ kind, const uint8_t *__restrict__ old_present, int has_old, int64_t n, RawDocStatus *st) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t k = kind[r];
  uint32_t f = k > TFGPU_K_DELETE ? (uint32_t)RD_NONROW : 0u;
  if (has_old && (!old_present || ((old_present[r >> 3] >> (r & 7)) & 1))) f |= k == TFGPU_K_UPDATE ? (uint32_t)RD_OLD_UPDATE : (uint32_t)RD_OLD_OTHER;
  if (f & ~__hip_atomic_load(&st->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&st->flags, f);
}

// encoding/json appendString of a column name (escapeHTML off), the host's copy of emit_json_string
static std::string json_key_literal(const std::string &name) {
  static const char *HEX = "0123456789abcdef";
  std::string o = "\"";
  const size_t n = name.size();
  for (size_t i = 0; i < n;) {
    const uint32_t c = (uint8_t)name[i];
    if (c < 0x80) {
      if (c >= 0x20 && c != '"' && c != '\\') { o += (char)c; i++; continue; }
      o += '\\';
      switch (c) {
        case '"': o += '"'; break; case '\\': o += '\\'; break; case '\b': o += 'b'; break; case '\f': o += 'f'; break;
        case '\n': o += 'n'; break; case '\r': o += 'r'; break; case '\t': o += 't'; break;
        default: o += "u00"; o += HEX[c >> 4]; o += HEX[c & 15];
      }
      i++; continue;
    }
    uint32_t need = 0, cp = 0, lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) { need = 1; cp = c & 0x1F; }
    else if (c >= 0xE0 && c <= 0xEF) { need = 2; cp = c & 0x0F; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { need = 3; cp = c & 0x07; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    bool ok = need > 0 && i + need < n;
    if (ok) for (uint32_t k = 1; k <= need; k++) {
      const uint32_t d = (uint8_t)name[i + k], l = k == 1 ? lo : 0x80u, h = k == 1 ? hi : 0xBFu;
      if (d < l || d > h) { ok = false; break; }
      cp = (cp << 6) | (d & 0x3F);
    }
    if (!ok) { o += "\\ufffd"; i++; continue; }
    if (cp == 0x2028 || cp == 0x2029) { o += cp == 0x2028 ? "\\u2028" : "\\u2029"; i += need + 1; continue; }
    o.append(name, i, need + 1);
    i += need + 1;
  }
  return o + "\":";
}

static bool rd_has(const std::vector<std::string> &v, const std::string &n) { return std::find(v.begin(), v.end(), n) != v.end(); }

std::unique_ptr<tfgpu_dbatch> apply_raw_doc(const tfgpu_plan &p, const tfgpu_dbatch &in, ApplyCtx &ax) {
  const char *T = "raw_doc_grouper: ";
  const int64_t n = in.nrows;
  hipStream_t st = ctx().stream;
  if (n > 0x7FFFFFFFll) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "more than 2^31-1 rows: split the batch");
  if (in.cols.size() >= (1u << 20)) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "2^20 columns and more");
  // the TableSchema the item carries: (name, DataType) in order
  std::vector<std::pair<std::string, int>> schema = in.schema;
  if (schema.empty()) for (auto &c : in.cols) schema.emplace_back(c.name, c.dtype);
  if (schema.empty()) return shallow_copy(in);  // "some system event": an item without a TableSchema passes as it is (raw_doc_grouper.go:70-74)
  for (auto &c : in.cols)
    if (rawdoc_special(c.name))
      throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the batch already has a column named " + c.name + ": the reference would list that name twice in ColumnNames");
  // containsAllFields (raw_doc_grouper.go:76-83): an item whose TableSchema lacks a configured key or field is an error of its own, and nothing is transformed
  {
    bool all = true;
    for (auto *list : {&p.rd_keys, &p.rd_fields})
      for (auto &nm : *list) {
        if (rawdoc_special(nm)) continue;
        bool found = false;
        for (auto &sc : schema) if (sc.first == nm) { found = true; break; }
        all = all && found;
      }
    if (!all) {
      for (int64_t r = 0; r < n; r++) ax.errs.push_back(tfgpu_row_error{r, TFGPU_ROW_COLUMN_NOT_FOUND, ax.step, -1});
      Buf none = dalloc(4);
      return gather_rows(in, none, 0);
    }
  }
  materialize(in);

  // ---- the doc's columns: by name, the last of a repeated name (docData is a map) -----------------------------------------------------------------
  std::vector<int> order;
  for (size_t i = 0; i < in.cols.size(); i++) {
    bool later = false;
    for (size_t j = i + 1; j < in.cols.size(); j++)
      if (in.cols[j].name == in.cols[i].name) {
        if (in.cols[i].absent || in.cols[j].absent)
          throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column " + in.cols[i].name + " stands twice in the batch and some rows leave one of the two out (ABSENT cells): which value a row's doc holds is per row");
        later = true;
      }
    if (!later) order.push_back((int)i);
  }
  std::sort(order.begin(), order.end(), [&](int a, int b) { return in.cols[(size_t)a].name < in.cols[(size_t)b].name; });  // (bytes, as sort.Strings orders the map's keys)
  int rest = -1, rest_at = -1;
  for (size_t k = 0; k < order.size(); k++) if (in.cols[(size_t)order[k]].name == "_rest" && in.cols[(size_t)order[k]].repr == TFGPU_R_JSON) { rest = (int)k; rest_at = order[k]; }
  std::vector<DCol> cols;
  std::vector<const uint8_t *> absent;
  std::vector<uint32_t> lit_off{0u}, name_off{0u};
  std::vector<uint8_t> after_rest;
  std::string lit, names;
  bool any_absent = false;
  for (int i : order) {
    const DColumn &c = in.cols[(size_t)i];
    cols.push_back(dcol_of(c));
    absent.push_back(ptr<uint8_t>(c.absent)); any_absent = any_absent || c.absent;
    lit += json_key_literal(c.name); lit_off.push_back((uint32_t)lit.size());
    names += c.name; name_off.push_back((uint32_t)names.size());
    after_rest.push_back(i > rest_at ? 1 : 0);
  }
  if (lit.size() >> 31) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column names of 2 GiB");
  const int32_t ncols = (int32_t)cols.size();
  if (cols.empty()) { cols.push_back(DCol{}); absent.push_back(nullptr); after_rest.push_back(0); }  // (never read)
  Buf bcols = upload_const(cols.data(), cols.size() * sizeof(DCol)), blit = upload_const(lit.data(), lit.size()), blo = upload_const(lit_off.data(), lit_off.size() * 4);
  Buf babs = any_absent ? upload_const(absent.data(), absent.size() * sizeof(const uint8_t *)) : nullptr;
  Buf bnames, bno, bafter;
  if (rest >= 0) { bnames = upload_const(names.data(), names.size()); bno = upload_const(name_off.data(), name_off.size() * 4); bafter = upload_const(after_rest.data(), after_rest.size()); }
  const RawDocStatus init{0u, 0u, ~0ull, 0ull};
  Buf status = upload_small(&init, sizeof init);
  RawDocStatus *dst = reinterpret_cast<RawDocStatus *>(status->p);

  // ---- etl_updated_at, the kinds, the lengths -------------------------------------------------------------------------------------------------------
  DColumn etl;
  etl.name = "etl_updated_at"; etl.dtype = TFGPU_T_TIMESTAMP; etl.repr = TFGPU_R_TIME;
  etl.values = dalloc((size_t)n * 8 + 8); etl.nanos = dalloc((size_t)n * 4 + 4);
  if (ax.commit_time && !in.src_row && n > ax.meta_n)
    throw Error(TFGPU_ERR_INVALID, "tfgpu_apply_meta: meta->n = " + std::to_string(ax.meta_n) + " entries for a batch of " + std::to_string(n) + " rows");
  Buf len = dalloc((size_t)(n + 1) * 4);
  RawDocParams P{};
  P.cols = ptr<DCol>(bcols); P.absent = babs ? reinterpret_cast<const uint8_t *const *>(babs->p) : nullptr; P.lit_off = ptr<uint32_t>(blo); P.lit = ptr<uint8_t>(blit);
  P.name_off = ptr<uint32_t>(bno); P.names = ptr<uint8_t>(bnames); P.after_rest = ptr<uint8_t>(bafter);
  P.ncols = ncols; P.rest = rest; P.n = n; P.len = ptr<uint32_t>(len); P.st = dst;
  if (n) {
    {
      KernelTimer t("rawdoc_commit_time", n);
      rawdoc_commit_time<<<grid_for(n, 256), 256, 0, st>>>(ptr<int32_t>(in.src_row), ax.commit_time, ax.meta_n, n, ptr<int64_t>(etl.values), ptr<int32_t>(etl.nanos), dst);
      if (in.kind) rawdoc_kinds<<<grid_for(n, 256), 256, 0, st>>>(ptr<uint8_t>(in.kind), ptr<uint8_t>(in.old_present), in.old_keys.empty() ? 0 : 1, n, dst);
    }
    {
      KernelTimer t("rawdoc_len", n);
      if (rest >= 0) rawdoc_len<true><<<grid_for(n, 256), 256, 0, st>>>(P); else rawdoc_len<false><<<grid_for(n, 256), 256, 0, st>>>(P);
    }
    sum_u32_segments_u64(ptr<uint32_t>(len), n, 1, n, &dst->total);
  }
  const uint32_t *hs = d2h_u32(status->p, sizeof(RawDocStatus) / 4);
  sync();
  RawDocStatus got;
  std::memcpy(&got, hs, sizeof got);
  // ---- whole-call refusals: nothing has been written ---------------------------------------------------------------------------------------------------
  if (got.flags & RD_META_SHORT) throw Error(TFGPU_ERR_INVALID, "tfgpu_apply_meta: meta->n = " + std::to_string(ax.meta_n) + " entries, and a row's src_row lies beyond them");
  if (got.flags & RD_NONROW)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the batch holds non-row kinds (TFGPU_K_OTHER / TFGPU_K_SYNCHRONIZE): those items go through the stock transformer");
  if (got.nan_first != ~0ull)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "column " + in.cols[(size_t)order[(size_t)(got.nan_first & 0xFFFFFu)]].name + " holds NaN or Inf in row " + std::to_string(got.nan_first >> 20) +
                                           ": json.Marshal has no text for it (the reference fails the doc there)");
  if (got.flags & RD_BACKSLASH)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "a member key of a `_rest` object holds a backslash escape: its place among the column names is that of the decoded bytes, which the merge does not decode");
  if (got.flags & RD_BAD_REST)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "a `_rest` value starts with '{' and is not one compact JSON object (or nests deeper than 128 levels): an `any` cell holds json.Marshal's text");
  if ((got.flags & RD_HUGE_CELL) || got.total >> 32)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "the doc column reaches 4 GiB of text (or one text cell is above 704 MB): split the batch");

  auto out = shallow_copy(in);
  // ---- OldKeys: inPlaceRemoveOldKeys(&item.OldKeys, item.ColumnNames) on Update rows only (raw_data_utils.go:87-95, 127-142) ------------------------------
  auto kept = [&](const std::string &nm) { return rd_has(p.rd_keys, nm) || rd_has(p.rd_fields, nm); };  // keySet.Contains(colName) || slices.Contains(r.Fields, colName)
  if (!in.old_keys.empty()) {
    bool unlisted = false, ragged_absent = false;
    for (auto &ok : in.old_keys) {
      bool listed = rawdoc_special(ok.name);
      for (auto &c : in.cols) if (c.name == ok.name && kept(c.name)) { listed = true; if (c.absent) ragged_absent = true; }
      unlisted = unlisted || !listed;
    }
    const bool upd = got.flags & RD_OLD_UPDATE, other = got.flags & RD_OLD_OTHER;
    if (upd && ragged_absent)
      throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "ragged OldKeys: an OldKeys column is a kept column some rows do not list (ABSENT cells), so Update rows would drop it row by row");
    if (unlisted && upd && other)
      throw Error(TFGPU_ERR_UNSUPPORTED, std::string(T) + "ragged OldKeys: the batch's OldKeys name a column the result does not list, Update rows drop it (inPlaceRemoveOldKeys) and other rows "
                                                           "with OldKeys keep it: per-row KeyNames, which a columnar batch cannot express");
    if (unlisted && upd) {
      out->old_keys.clear();
      for (auto &ok : in.old_keys) {
        bool listed = rawdoc_special(ok.name);
        for (auto &c : in.cols) if (c.name == ok.name && kept(c.name)) listed = true;
        if (listed) out->old_keys.push_back(ok);
      }
      if (out->old_keys.empty()) out->old_present = nullptr;
    }
  }

  // ---- the result: kept columns (shared buffers), etl_updated_at, doc ---------------------------------------------------------------------------------
  out->cols.clear();
  for (auto &c : in.cols) if (kept(c.name)) out->cols.push_back(c);
  DColumn doc;
  doc.name = "doc"; doc.dtype = TFGPU_T_ANY; doc.repr = TFGPU_R_JSON;
  doc.data_len = got.total;
  doc.data = dalloc((size_t)got.total + 8);
  if (n) {
    {
      KernelTimer t("rawdoc_scan", n);
      exclusive_scan_u32(ptr<uint32_t>(len), ptr<uint32_t>(len), n, true);
    }
    P.off = ptr<uint32_t>(len); P.data = ptr<uint8_t>(doc.data);
    KernelTimer t("rawdoc_write", (int64_t)got.total);
    if (rest >= 0) rawdoc_write<true><<<grid_for(n, 256), 256, 0, st>>>(P); else rawdoc_write<false><<<grid_for(n, 256), 256, 0, st>>>(P);
  } else TF_HIP(hipMemsetAsync(len->p, 0, 4, st));
  doc.offsets = len;
  out->cols.push_back(std::move(etl));
  out->cols.push_back(std::move(doc));
  // resultSchema (raw_doc_grouper.go:129-152): keys in config order, then fields
  out->schema.clear(); out->key_names.clear();
  for (int is_key = 1; is_key >= 0; is_key--)
    for (auto &nm : is_key ? p.rd_keys : p.rd_fields) {
      int dtype = -1;
      for (auto &sc : schema) if (sc.first == nm) dtype = sc.second;
      if (dtype < 0) dtype = nm == "doc" ? TFGPU_T_ANY : TFGPU_T_TIMESTAMP;
      out->schema.emplace_back(nm, dtype);
      if (is_key) out->key_names.push_back(nm);
    }
  return out;  // (the tables and the status block go back to the lane's stream-ordered pool behind the kernels that read them)
}

}  // namespace tf
