// tf_byids.hip — filter_rows_by_ids (pkg/transformer/registry/filter_rows_by_ids/filter_rows_by_ids.go:78-168): a row is kept when some
// suitable text cell starts with one of the allowed IDs.  One lane per row; the lane walks the columns the host resolved (TableSchema
// order, AsMap's last column of a name, suitable DataType, column filter, text repr) and leaves at the first hit.
//
// Per cell a lane reads its two offsets and at most max_len bytes: FNV-1a extends by one byte at a time, so the walk passes the hash of
// every prefix, and at each allowed length it probes the open-addressing table (tf_byids.hpp) — in LDS when the table's image fits
// BYIDS_LDS_BUDGET, else in HBM.  A byte kernel: no MFMA, no scratch, nothing written but keep[r].
#include "tf_plan.hpp"
#include "tf_rows.hpp"
#include "tf_devrow.hpp"

namespace tf {

struct ByIdsCol {
  const uint32_t *offsets;
  const uint8_t *data;
  const uint8_t *validity;  // null: no nil
  const uint8_t *absent;    // null: every row lists the column
  int32_t form;             // BYIDS_TEXT: a Go string / []byte; BYIDS_JSON: a string only as a JSON string, by its decoded bytes; BYIDS_OTHER: never a string
  int32_t prev;             // the entry of the column that listed the same name before this one, read where this one is ABSENT; -1: none
};
enum : int32_t { BYIDS_TEXT = 0, BYIDS_JSON = 1, BYIDS_OTHER = 2 };
struct ByIdsParams {
  const ByIdsCol *cols;
  int32_t ncols;
  const uint32_t *table;  // the image in HBM
  uint32_t words;         // its size
  uint32_t nlen, mask;
  const uint8_t *kind;    // null: every row is an Insert
  int64_t nrows;
  uint32_t *keep;
};

// the image, wherever it lives
struct ByIdsView {
  const uint32_t *lens, *slots;
  const uint8_t *bytes;
  uint32_t nlen, mask;
};

__device__ __forceinline__ uint32_t byids_load4(const uint8_t *p) {  // (inside the cell: no alignment is promised)
  struct __attribute__((packed, aligned(1))) U32 { uint32_t v; };
  return reinterpret_cast<const U32 *>(p)->v;
}

// prefixes[ID[0:L]] (isIDAllowed :162): same(off) compares the ID's bytes at `off` with the cell's first L
template <class Same>
__device__ __forceinline__ bool byids_probe(const ByIdsView &t, uint32_t h, uint32_t L, Same same) {
  const uint32_t key = byids_key(h, L);
  for (uint32_t at = byids_home(key, t.mask);; at = (at + 1) & t.mask) {  // (at most half of the slots are taken: the walk ends)
    const uint32_t len = t.slots[3 * at + 2];
    if (len == BYIDS_EMPTY) return false;
    if (len == L && t.slots[3 * at] == key && same(t.slots[3 * at + 1])) return true;
  }
}

// a Go string / []byte of n bytes at p
__device__ __forceinline__ bool byids_text_allowed(const ByIdsView &t, const uint8_t *p, uint32_t n) {
  uint32_t h = BYIDS_FNV_INIT, i = 0;
  for (uint32_t k = 0;;) {
    const uint32_t L = t.lens[k];
    if (L > n) return false;  // (ascending: every further length is longer than the value too)
    for (; i + 4 <= L; i += 4) {
      const uint32_t w = byids_load4(p + i);
      h = byids_step(h, w & 0xFF); h = byids_step(h, (w >> 8) & 0xFF); h = byids_step(h, (w >> 16) & 0xFF); h = byids_step(h, w >> 24);
    }
    for (; i < L; i++) h = byids_step(h, p[i]);
    if (byids_probe(t, h, L, [&](uint32_t off) {
          for (uint32_t j = 0; j < L; j++) if (t.bytes[off + j] != p[j]) return false;
          return true;
        })) return true;
    if (++k == t.nlen) return false;
  }
}

// The bytes of the Go string a JSON string text decodes to (encoding/json unquote): the two-character escapes, \uXXXX with surrogate
// pairs joined and a lone surrogate read as U+FFFD, and raw bytes that are not well-formed UTF-8 coerced to U+FFFD one byte at a time.
// p stands behind the opening quote; next() is -1 at the closing quote (or where the text ends).  No buffer: at most four bytes wait in `pend`.
struct ByIdsJsonStr {
  const uint8_t *p, *e;
  uint32_t pend = 0, npend = 0;
  __device__ __forceinline__ ByIdsJsonStr(const uint8_t *b, const uint8_t *end) : p(b), e(end) {}
  __device__ __forceinline__ static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
  __device__ __forceinline__ int u4(const uint8_t *q) const {  // getu4: `\uXXXX` at q, or -1
    if (e - q < 6 || q[0] != '\\' || q[1] != 'u') return -1;
    int v = 0;
    for (int k = 2; k < 6; k++) { const int d = hex(q[k]); if (d < 0) return -1; v = v * 16 + d; }
    return v;
  }
  __device__ __forceinline__ int rune(uint32_t r) {  // utf8.EncodeRune: the first byte now, the rest waits
    if (r < 0x80) return (int)r;
    if (r < 0x800) { pend = 0x80 | (r & 0x3F); npend = 1; return (int)(0xC0 | r >> 6); }
    if (r < 0x10000) { pend = (0x80 | ((r >> 6) & 0x3F)) | (0x80 | (r & 0x3F)) << 8; npend = 2; return (int)(0xE0 | r >> 12); }
    pend = (0x80 | ((r >> 12) & 0x3F)) | (0x80 | ((r >> 6) & 0x3F)) << 8 | (0x80 | (r & 0x3F)) << 16; npend = 3;
    return (int)(0xF0 | r >> 18);
  }
  __device__ __forceinline__ int next() {
    if (npend) { const int b = (int)(pend & 0xFF); pend >>= 8; npend--; return b; }
    if (p >= e) return -1;
    const uint8_t c = *p;
    if (c == '"') return -1;
    if (c == '\\') {
      if (e - p < 2) { p = e; return -1; }
      const uint8_t x = p[1];
      if (x == 'u') {
        int r = u4(p);
        if (r < 0) { p = e; return -1; }  // (no JSON: the scanner of the reference would have refused the text)
        p += 6;
        if (r >= 0xD800 && r < 0xE000) {  // utf16.IsSurrogate
          const int r2 = u4(p);
          if (r < 0xDC00 && r2 >= 0xDC00 && r2 < 0xE000) { p += 6; return rune(0x10000u + (((uint32_t)r - 0xD800u) << 10) + ((uint32_t)r2 - 0xDC00u)); }
          return rune(0xFFFDu);  // invalid surrogate: the replacement rune, and the next escape is read on its own
        }
        return rune((uint32_t)r);
      }
      p += 2;
      switch (x) { case 'b': return '\b'; case 'f': return '\f'; case 'n': return '\n'; case 'r': return '\r'; case 't': return '\t'; }
      return x;  // `"`, `\`, `/`
    }
    if (c < 0x80) { p++; return c; }
    // utf8.DecodeRune: a well-formed sequence passes as it is, anything else is one byte read as U+FFFD
    const uint32_t left = (uint32_t)(e - p);
    uint32_t need = 0, lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c >= 0xE0 && c <= 0xEF) { need = 2; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { need = 3; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    bool ok = need != 0 && left > need && p[1] >= lo && p[1] <= hi;
    for (uint32_t k = 2; ok && k <= need; k++) ok = p[k] >= 0x80 && p[k] <= 0xBF;
    if (!ok) { p++; return rune(0xFFFDu); }
    pend = 0;
    for (uint32_t k = need; k >= 1; k--) pend = pend << 8 | p[k];
    npend = need;
    p += need + 1;
    return c;
  }
};

// an `any` cell held as JSON text: the Go value is a string only where the text is a JSON string
__device__ __forceinline__ bool byids_json_allowed(const ByIdsView &t, const uint8_t *p, uint32_t n) {
  const uint8_t *e = p + n;
  while (p < e && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
  if (p >= e || *p != '"') return false;  // an object, array, number, true, false or null
  p++;
  ByIdsJsonStr s(p, e);
  uint32_t h = BYIDS_FNV_INIT, i = 0;
  for (uint32_t k = 0;;) {
    const uint32_t L = t.lens[k];
    for (; i < L; i++) {
      const int b = s.next();
      if (b < 0) return false;  // the string is shorter than this length, and than every further one
      h = byids_step(h, (uint32_t)b);
    }
    if (byids_probe(t, h, L, [&](uint32_t off) {  // (a key that matches is rare: the prefix is decoded again for the comparison)
          ByIdsJsonStr again(p, e);
          for (uint32_t j = 0; j < L; j++) if ((int)t.bytes[off + j] != again.next()) return false;
          return true;
        })) return true;
    if (++k == t.nlen) return false;
  }
}

__device__ __forceinline__ bool byids_bit(const uint8_t *bits, int64_t r) { return (bits[r >> 3] >> (r & 7)) & 1; }

template <bool LDS>
__global__ void __launch_bounds__(256, 8) byids_keep_kernel(ByIdsParams p) {
  __shared__ uint32_t s_table[LDS ? BYIDS_LDS_BUDGET / 4 : 1];
  ByIdsView t;
  if (LDS) {
    for (uint32_t w = threadIdx.x; w < p.words; w += blockDim.x) s_table[w] = p.table[w];
    __syncthreads();
    t.lens = s_table;
  } else t.lens = p.table;
  t.nlen = p.nlen; t.mask = p.mask;
  t.slots = t.lens + p.nlen;
  t.bytes = reinterpret_cast<const uint8_t *>(t.slots + 3 * (size_t)(p.mask + 1));
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  // an item without ColumnNames has an empty AsMap(): a Delete, and every kind that is no row event
  const int kind = p.kind ? p.kind[r] : TFGPU_K_INSERT;
  uint32_t keep = 0;
  if (kind == TFGPU_K_INSERT || kind == TFGPU_K_UPDATE) {
    for (int c = 0; c < p.ncols && !keep; c++) {
      int q = c;  // AsMap()[name]: the last column of that name the row lists; none: no entry
      while (q >= 0 && p.cols[q].absent && byids_bit(p.cols[q].absent, r)) q = p.cols[q].prev;
      if (q < 0) continue;
      const ByIdsCol col = p.cols[q];
      if (col.form == BYIDS_OTHER) continue;                      // a number, a time, a bool, a json.Number
      if (col.validity && !byids_bit(col.validity, r)) continue;  // nil is no string
      const uint32_t a = col.offsets[r], n = col.offsets[r + 1] - a;
      keep = col.form == BYIDS_JSON ? byids_json_allowed(t, col.data + a, n) : byids_text_allowed(t, col.data + a, n);
    }
  }
  p.keep[r] = keep;
}

// the plan's table on this lane: uploaded with the lane's first batch (timed as filter_rows_by_ids_table_upload), found again after that.
// A lane keeps at most 16 images and at most BYIDS_LANE_CACHE_BYTES of them, whichever plans are still alive: the one used longest ago goes
// first (an image larger than the cap is kept alone, until the next one comes).
constexpr size_t BYIDS_LANE_CACHE_BYTES = (size_t)256 << 20;
static Buf byids_table_on_lane(const ByIdsTable &t) {
  Context &cx = ctx();
  for (auto &e : cx.plan_tables) if (e.id == t.id) { e.stamp = ++cx.const_clock; return e.mem; }
  const size_t bytes = t.image.size() * 4;
  auto held = [&] { size_t b = 0; for (auto &e : cx.plan_tables) b += e.mem->bytes; return b; };
  while (!cx.plan_tables.empty() && (cx.plan_tables.size() >= 16 || held() + bytes > BYIDS_LANE_CACHE_BYTES)) {
    size_t old = 0;
    for (size_t k = 1; k < cx.plan_tables.size(); k++) if (cx.plan_tables[k].stamp < cx.plan_tables[old].stamp) old = k;
    cx.plan_tables.erase(cx.plan_tables.begin() + (long)old);
  }
  KernelTimer kt("filter_rows_by_ids_table_upload", (int64_t)bytes);
  Buf m = upload_small(t.image.data(), bytes);
  cx.plan_tables.push_back(Context::PlanTable{t.id, m, ++cx.const_clock});
  return m;
}

// TFGPU_BYIDS_LDS=0: every table is probed in HBM (tests compare the two paths on one batch; A/B measurements)
static bool byids_lds_on() {
  const char *e = std::getenv("TFGPU_BYIDS_LDS");
  return !(e && e[0] == '0');
}

std::unique_ptr<tfgpu_dbatch> apply_filter_by_ids(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  // shouldKeep walks item.TableSchema.Columns() and reads the values through AsMap()[name]: the last column listing a name
  // (a batch does not tell a TableSchema of no columns from none at all — both arrive as an empty list, and the batch's own columns stand in;
  //  the reference would walk nothing and drop every row of the first, which no source produces)
  std::vector<std::pair<std::string, int>> own;
  if (in.schema.empty()) for (auto &c : in.cols) own.emplace_back(c.name, c.dtype);
  const auto &schema = in.schema.empty() ? own : in.schema;
  // one chain per suitable schema column: the batch's columns of that name from the last back to the first that every row lists
  auto form_of = [](const DColumn &c) { return c.repr == TFGPU_R_STRING || c.repr == TFGPU_R_BYTES ? BYIDS_TEXT : c.repr == TFGPU_R_JSON ? BYIDS_JSON : BYIDS_OTHER; };  // `default: continue`
  std::vector<std::vector<const DColumn *>> chains;
  std::vector<const DColumn *> read;
  for (auto &sc : schema) {
    if (byids_mongo_document(sc.first, sc.second))
      throw Error(TFGPU_ERR_UNSUPPORTED, "filter_rows_by_ids: Mongo `document` columns stay with the stock transformer (the filter looks inside the BSON document, which a device batch does not hold)");
    if (!byids_column_suitable(p, sc.first, sc.second)) continue;
    std::vector<const DColumn *> chain;
    for (size_t i = in.cols.size(); i-- > 0;) {
      if (in.cols[i].name != sc.first) continue;
      chain.push_back(&in.cols[i]);
      if (!in.cols[i].absent) break;
    }
    bool any_text = false;
    for (const DColumn *c : chain) any_text = any_text || form_of(*c) != BYIDS_OTHER;
    if (!any_text) continue;  // a schema column the batch does not carry, or one that never holds a string
    for (const DColumn *c : chain) if (form_of(*c) != BYIDS_OTHER) read.push_back(c);
    chains.push_back(std::move(chain));
  }
  materialize(in, &read);  // only what the kernel reads: the other text columns stay lazy / unscanned
  std::vector<ByIdsCol> cols(chains.size());  // the chains' heads first: the kernel walks [0, ncols) and follows `prev` behind them
  auto entry = [&](const DColumn &c) {
    const int32_t f = form_of(c);
    return f == BYIDS_OTHER ? ByIdsCol{nullptr, nullptr, nullptr, ptr<uint8_t>(c.absent), f, -1}
                            : ByIdsCol{ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.payload()), ptr<uint8_t>(c.validity), ptr<uint8_t>(c.absent), f, -1};
  };
  for (size_t k = 0; k < chains.size(); k++) {
    size_t at = k;
    cols[k] = entry(*chains[k][0]);
    for (size_t j = 1; j < chains[k].size(); j++) { cols[at].prev = (int32_t)cols.size(); at = cols.size(); cols.push_back(entry(*chains[k][j])); }
  }
  const ByIdsTable &t = *p.byids;
  const int64_t n = in.nrows;
  Buf bcols = upload_const(cols.data(), cols.size() * sizeof(ByIdsCol)), table = byids_table_on_lane(t);
  Buf keep = dalloc((size_t)(n + 1) * 4);
  ByIdsParams kp{ptr<ByIdsCol>(bcols), (int32_t)chains.size(), ptr<uint32_t>(table), (uint32_t)t.image.size(), t.nlen, t.cap - 1, ptr<uint8_t>(in.kind), n, ptr<uint32_t>(keep)};
  const bool lds = t.image.size() * 4 <= BYIDS_LDS_BUDGET && byids_lds_on();
  {  // (two names: the profile says which kernel ran)
    KernelTimer kt(lds ? "filter_rows_by_ids_lds" : "filter_rows_by_ids_hbm", n);
    if (n) {
      if (lds) byids_keep_kernel<true><<<grid_for(n, 256), 256, 0, ctx().stream>>>(kp);
      else byids_keep_kernel<false><<<grid_for(n, 256), 256, 0, ctx().stream>>>(kp);
    }
  }
  return compact(in, keep, true);  // syncs; the kept rows stay a selection until somebody reads them
}

}  // namespace tf
