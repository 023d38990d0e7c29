// tf_tablesplit.hip — table_splitter_transformer on device (pkg/transformer/registry/table_splitter/table_splitter.go:37-59, 80-94):
// every row gets the table name GenerateTableName builds from its own values, and the batch leaves as one batch per name.
//
// A batch is one table by construction, so the result is a handle (tfgpu_tablesplit) over the input: the distinct names in order of
// first appearance, every row's table, and ONE grouped selection from which a table's batch is gathered when it is asked for.
//
//   1. tsplit_hash         lane = row: the name (table, then per resolved column the splitter and SerializeToString of the value) is
//                          rendered into a hashing sink — 2 x 64 bits, its length counted in 64 bits.  No name text goes to HBM.
//   2. tsplit_intern       open-addressing table (>= 2n slots): a row's table is the slot its hash claims.  Equal hash and equal raw
//                          values = the same table; exactly one differing column, and that one an integer = another; any other raw
//                          difference under an equal hash ("a/b" + "c" against "a" + "b/c"; the integers 1, 11 against 11, 1 under the
//                          splitter "1") is put off to tsplit_intern_text, which compares the rendered bytes —
//                          the compare renders both names three times and stays out of the kernel every row runs.
//   3. first appearance    atomicMin of the row index per claimed slot, flags of the rows that are their slot's minimum, one scan:
//                          a row's table id = the rank of its slot's first row.  One read-back: T.
//   4. names               only the T first rows are rendered to text (length, scan, write); that text is downloaded once.
//   5. grouping            one stable radix sort of (table id, row) over ceil(log2 T) bits; the run heads give every table's start.
//                          No per-table pass, no per-table sync.  T = 1 skips the sort.
//
// tsplit_hash reads the named columns once; measured at 6-10 % of the HBM peak it is bound by formatting (fmt_date / fmt_i64) and the
// byte-at-a-time hashing sink, not by bandwidth.  tsplit_intern is a chain of dependent reads per row: slot, the owner's hash, the owner's
// values.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "tf_plan.hpp"
#include "tf_rows.hpp"
#include "tf_devrow.hpp"
#include "tf_intern.hpp"

struct tfgpu_tablesplit {
  int64_t nrows = 0;
  int lane = 0;                               // the lane that made it: its buffers, its stream
  std::vector<char> text;                     // the names' bytes back to back, in order of first appearance (one block: a batch of n distinct keys has n names)
  std::vector<uint32_t> name_off;             // [ntables + 1] into text; empty = no tables
  size_t ntables() const { return name_off.empty() ? 0 : name_off.size() - 1; }
  std::string name(size_t t) const { return std::string(text.data() + name_off[t], name_off[t + 1] - name_off[t]); }
  std::vector<uint32_t> start;                // table t = sel[start[t] .. start[t + 1]) (the last one: .. nrows)
  int64_t count(size_t t) const { return (t + 1 < start.size() ? (int64_t)start[t + 1] : nrows) - (int64_t)start[t]; }
  std::shared_ptr<const tfgpu_dbatch> src;    // the dense batch the rows are gathered from
  tf::Buf sel;                                // int32[nrows]: rows grouped by table, input order inside a table
  tf::Buf row_table;                          // uint32[nrows]: every row's table
};

namespace tf {

static inline unsigned tgrid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

struct SplitParams {
  const DCol *cols; int32_t ncols;  // the configured names the schema has, in config order (repr 0: a schema column the batch lacks — every value nil)
  const uint8_t *lit;               // the table name, then the splitter
  uint32_t tlen, slen;
  int64_t n;
  uint64_t *h;                      // [n][2]
  uint32_t *defer_n, *defer_list;   // rows whose place only a compare of the name texts decides (tsplit_intern_text)
  int32_t weak;
};

// ---- sinks ----------------------------------------------------------------------------------------------------------------
// (NameHash: tf_intern.hpp)
struct NameCount { uint64_t n = 0; __device__ __forceinline__ void put(uint32_t) { n++; } };
struct NameStore { uint8_t *dst; __device__ __forceinline__ void put(uint32_t c) { *dst++ = (uint8_t)c; } };
struct NameWindow {  // the bytes [lo, lo + 64) of a rendered name
  uint8_t *buf; uint64_t lo, pos = 0;
  __device__ __forceinline__ void put(uint32_t c) { if (pos - lo < 64ull) buf[pos - lo] = (uint8_t)c; pos++; }
};

// GenerateTableName (table_splitter.go:37-59) of row r
template <class S> __device__ __forceinline__ void emit_name(const SplitParams &p, int64_t r, S &s) {
  for (uint32_t i = 0; i < p.tlen; i++) s.put(p.lit[i]);
  for (int c = 0; c < p.ncols; c++) {
    if (c || p.tlen) for (uint32_t i = 0; i < p.slen; i++) s.put(p.lit[p.tlen + i]);
    const DCol &col = p.cols[c];
    if (col.repr == 0 || !is_valid(col, r)) {  // item[col] of a name the row does not have: nil
      if (col.dtype == TFGPU_T_ANY) { s.put('n'); s.put('u'); s.put('l'); s.put('l'); }  // json.Marshal(nil)
      else { s.put('<'); s.put('n'); s.put('i'); s.put('l'); s.put('>'); }
      continue;
    }
    if (col.offsets) {  // text: the cell's bytes as they are
      const uint32_t a = col.offsets[r], b = col.offsets[r + 1];
      for (uint32_t i = a; i < b; i++) s.put(col.data[i]);
      continue;
    }
    uint8_t buf[64]; const uint8_t *ext;
    const int len = serialize_small(col, r, buf, &ext);
    for (int i = 0; i < len; i++) s.put(buf[i]);
  }
}

__global__ void __launch_bounds__(256) tsplit_hash(SplitParams p) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  NameHash s;
  emit_name(p, r, s);
  s.finish();
  if (p.weak) { s.h1 &= 3ull; s.h2 = 0; }  // TFGPU_TABLESPLIT_WEAK_HASH=1 (tests): almost every name collides, the text compare decides
  p.h[2 * r] = s.h1;
  p.h[2 * r + 1] = s.h2;
}

// ---- 2. rows -> slots -------------------------------------------------------------------------------------------------------
__device__ bool name_text_equal(const SplitParams &p, int64_t a, int64_t b) {
  NameCount ca, cb;
  emit_name(p, a, ca); emit_name(p, b, cb);
  if (ca.n != cb.n) return false;
  uint8_t wa[64], wb[64];
  for (uint64_t lo = 0; lo < ca.n; lo += 64) {
    NameWindow sa{wa, lo}, sb{wb, lo};
    emit_name(p, a, sa); emit_name(p, b, sb);
    const uint32_t m = ca.n - lo < 64ull ? (uint32_t)(ca.n - lo) : 64u;
    for (uint32_t i = 0; i < m; i++) if (wa[i] != wb[i]) return false;
  }
  return true;
}
// values that print injectively: a differing raw value is a differing text (bools may hold any non-zero byte, floats several NaNs, a date any
// second of its day: those go to the texts)
__device__ __forceinline__ bool prints_injectively(const DCol &c) {
  if (c.repr >= TFGPU_R_INT8 && c.repr <= TFGPU_R_UINT64) return true;
  if (c.repr == TFGPU_R_DURATION) return true;
  return c.repr == TFGPU_R_TIME && c.dtype != TFGPU_T_DATE;
}
__device__ __forceinline__ int raw_width(int r) {
  switch (r) {
    case TFGPU_R_INT8: case TFGPU_R_UINT8: case TFGPU_R_BOOL: return 1;
    case TFGPU_R_INT16: case TFGPU_R_UINT16: return 2;
    case TFGPU_R_INT32: case TFGPU_R_UINT32: case TFGPU_R_FLOAT32: return 4;
    default: return 8;
  }
}
// Same name?  1 yes, 0 no.  TEXT = false (tsplit_intern, the kernel every row runs): 2 = "only the texts can tell".
// Every column raw-equal with the same nil state: the same name.  EXACTLY ONE column differs and it prints injectively: the names are
// prefix + X + suffix and prefix + Y + suffix with X != Y, so they differ.  Anything else is ambiguous — a component that prints injectively
// does not make the JOINED name injective: ("x", 5, "6/y") and ("x/5", 6, "y") both print x/5/6/y under "/", the integers (1, 11) and (11, 1)
// both print 11111 under the splitter "1" — and goes to the texts.
template <bool TEXT> __device__ int names_equal(const SplitParams &p, int64_t a, int64_t b) {
  bool need_text = false;
  int injective_diffs = 0;
  for (int c = 0; c < p.ncols; c++) {
    const DCol &col = p.cols[c];
    if (col.repr == 0) continue;  // nil in every row
    const bool va = is_valid(col, a), vb = is_valid(col, b);
    if (!va || !vb) { if (va != vb) need_text = true; continue; }  // (a text cell may read "<nil>" too)
    if (col.offsets) {
      const uint32_t oa = col.offsets[a], la = col.offsets[a + 1] - oa, ob = col.offsets[b], lb = col.offsets[b + 1] - ob;
      bool same = la == lb;
      for (uint32_t i = 0; same && i < la; i++) same = col.data[oa + i] == col.data[ob + i];
      if (!same) need_text = true;
    } else {
      const int w = raw_width(col.repr);
      const uint8_t *xa = (const uint8_t *)col.values + a * w, *xb = (const uint8_t *)col.values + b * w;
      bool same = true;
      for (int i = 0; i < w; i++) same = same && xa[i] == xb[i];
      if (col.repr == TFGPU_R_TIME && (col.nanos ? col.nanos[a] : 0) != (col.nanos ? col.nanos[b] : 0)) same = false;
      if (!same) { if (prints_injectively(col)) injective_diffs++; else need_text = true; }
    }
  }
  if (!need_text && injective_diffs == 0) return 1;
  if (!need_text && injective_diffs == 1) return 0;
  if constexpr (TEXT) return name_text_equal(p, a, b) ? 1 : 0;
  else return 2;
}
template <bool TEXT> __device__ __forceinline__ void intern_row(const SplitParams &p, int64_t j, uint32_t *owner, uint32_t mask, uint32_t *__restrict__ slotof) {
  const uint64_t *__restrict__ h = p.h;
  const uint64_t a = h[2 * j], b = h[2 * j + 1];
  uint32_t slot = (uint32_t)(b ^ (a >> 17)) & mask;
  for (;;) {
    uint32_t o = __hip_atomic_load(&owner[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == NOROW) o = atomicCAS(&owner[slot], NOROW, (uint32_t)j);
    if (o == NOROW || o == (uint32_t)j) { slotof[j] = slot; return; }
    if (h[2 * (int64_t)o] == a && h[2 * (int64_t)o + 1] == b) {
      const int eq = names_equal<TEXT>(p, j, (int64_t)o);
      if (eq == 1) { slotof[j] = slot; return; }
      if (eq == 2) { p.defer_list[atomicAdd(p.defer_n, 1u)] = (uint32_t)j; return; }  // it owns nothing yet: tsplit_intern_text files it as a late comer
    }
    slot = (slot + 1) & mask;  // another name: probe on (the table has at least 2n slots for n rows)
  }
}
__global__ void __launch_bounds__(256) tsplit_intern(SplitParams p, uint32_t *owner, uint32_t mask, uint32_t *__restrict__ slotof) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < p.n) intern_row<false>(p, j, owner, mask, slotof);
}
// the rows only the name TEXTS can place (usually none: the launch finds an empty list and leaves)
__global__ void __launch_bounds__(256) tsplit_intern_text(SplitParams p, uint32_t *owner, uint32_t mask, uint32_t *__restrict__ slotof) {
  const uint32_t n = *p.defer_n;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) intern_row<true>(p, (int64_t)p.defer_list[i], owner, mask, slotof);
}

// ---- 3. first-appearance ids: intern_first / intern_flag / intern_ids (tf_intern.hpp) over owner[] --------------------------------
// (owner[slot] is some row of the slot's table: the minimum over all of them is the table's first row)
__global__ void __launch_bounds__(256) tsplit_kinds(const uint8_t *__restrict__ kind, int64_t n, uint32_t *flag) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && kind[r] > TFGPU_K_DELETE) *flag = 1u;
}

// ---- 4. the T names ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tsplit_name_len(SplitParams p, const uint32_t *__restrict__ reps, int64_t T, uint32_t *__restrict__ len, unsigned long long *total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  NameCount s;
  emit_name(p, (int64_t)reps[t], s);
  len[t] = s.n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s.n;
  atomicAdd(total, (unsigned long long)s.n);
}
__global__ void __launch_bounds__(256) tsplit_name_write(SplitParams p, const uint32_t *__restrict__ reps, int64_t T, const uint32_t *__restrict__ off, uint8_t *text) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  NameStore s{text + off[t]};
  emit_name(p, (int64_t)reps[t], s);
}

// ---- 5. run heads of the sorted ids: intern_heads (tf_intern.hpp) ------------------------------------------------------------

// `cur`: the caller's own copy of the batch (the lane's mutex is held)
static std::unique_ptr<tfgpu_tablesplit> split_batch(const tfgpu_plan &p, std::unique_ptr<tfgpu_dbatch> cur) {
  if (p.kind != PK_TABLE_SPLITTER) throw Error(TFGPU_ERR_INVALID, "tfgpu_table_split: the plan is a " + p.type_name + ", not a table_splitter_transformer");
  if (cur->pending) dense_locked(*cur); else wait_dense(*cur);
  const tfgpu_dbatch &in = *cur;
  const int64_t n = in.nrows;
  if (in.col_order) throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: the batch's rows carry their own ColumnNames order (col_order: a collapsed batch), which the per-table gather does not carry");
  if (n > 0x7FFFFFFFll) throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: more than 2^31-1 rows: split the batch");
  auto res = std::make_unique<tfgpu_tablesplit>();
  res->nrows = n; res->lane = current_lane();

  // the configured names the schema has, in config order; values by name (AsMap: the last duplicate wins), a schema column the batch lacks is nil in every row
  std::vector<const DColumn *> picked;
  std::vector<int> picked_dtype;
  for (auto &name : p.split_cols) {
    const DColumn *found = nullptr;
    for (auto &c : in.cols) if (c.name == name) found = &c;
    int dtype = -1;
    if (in.schema.empty()) { if (found) dtype = found->dtype; }
    else for (auto &sc : in.schema) if (sc.first == name) { dtype = sc.second; break; }  // FastColumns: the first of that name
    if (dtype < 0) continue;  // not in the TableSchema: contributes nothing, not even a splitter
    picked.push_back(found); picked_dtype.push_back(dtype);
  }
  {
    std::vector<const DColumn *> need;
    for (auto *c : picked) if (c) need.push_back(c);
    materialize(in, &need);
  }
  std::vector<DCol> cols;
  for (size_t i = 0; i < picked.size(); i++) {
    DCol d{};
    d.repr = 0; d.dtype = picked_dtype[i];
    if (const DColumn *c = picked[i]) {
      require_serializable(*c, "table_splitter_transformer");
      if (picked_dtype[i] == TFGPU_T_ANY && (c->repr == TFGPU_R_FLOAT32 || c->repr == TFGPU_R_FLOAT64 || c->repr == TFGPU_R_TIME || c->repr == TFGPU_R_DURATION || c->repr == TFGPU_R_STRING))
        throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: column " + c->name + " is `any` holding floats, times, durations or Go strings (json.Marshal prints them otherwise than %v)");
      d = dcol_of(*c);
      d.dtype = picked_dtype[i];
    }
    cols.push_back(d);
  }
  res->src = std::shared_ptr<const tfgpu_dbatch>(std::move(cur));
  if (n == 0) return res;

  hipStream_t st = ctx().stream;
  static const bool weak = [] { const char *e = std::getenv("TFGPU_TABLESPLIT_WEAK_HASH"); return e && e[0] == '1'; }();
  const std::string splitter = p.splitter.empty() ? "/" : p.splitter;
  const std::string lit = in.table + splitter;
  if (lit.size() >> 31) throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: a table name or splitter of 2 GiB");
  Buf blit = upload_small(lit.data(), lit.size());
  const int32_t ncols = (int32_t)cols.size();
  if (cols.empty()) cols.push_back(DCol{});  // (never read)
  Buf bcols = upload_small(cols.data(), cols.size() * sizeof(DCol));  // in HBM: no cap on the number of configured columns
  Buf kflag = dalloc_zero(4);
  if (in.kind) tsplit_kinds<<<tgrid(n), 256, 0, st>>>(ptr<uint8_t>(in.kind), n, ptr<uint32_t>(kflag));

  Buf h = dalloc((size_t)n * 16), defer_n = dalloc_zero(4), defer_list = dalloc((size_t)n * 4);
  SplitParams sp{ptr<DCol>(bcols), ncols, ptr<uint8_t>(blit), (uint32_t)in.table.size(), (uint32_t)splitter.size(), n,
                 ptr<uint64_t>(h), ptr<uint32_t>(defer_n), ptr<uint32_t>(defer_list), weak ? 1 : 0};
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n) cap <<= 1;
  Buf owner = dalloc((size_t)cap * 4), slotof = dalloc((size_t)n * 4);
  Buf rank = dalloc((size_t)(n + 1) * 4), tid = dalloc((size_t)n * 4), reps = dalloc((size_t)n * 4), idx = dalloc((size_t)n * 4);
  {
    KernelTimer t("tsplit_hash", n);
    tsplit_hash<<<tgrid(n), 256, 0, st>>>(sp);
  }
  {
    KernelTimer t("tsplit_intern", n);
    TF_HIP(hipMemsetAsync(owner->p, 0xFF, (size_t)cap * 4, st));
    tsplit_intern<<<tgrid(n), 256, 0, st>>>(sp, ptr<uint32_t>(owner), (uint32_t)(cap - 1), ptr<uint32_t>(slotof));
    tsplit_intern_text<<<(unsigned)std::min<int64_t>(tgrid(n), 256), 256, 0, st>>>(sp, ptr<uint32_t>(owner), (uint32_t)(cap - 1), ptr<uint32_t>(slotof));
  }
  {
    KernelTimer t("tsplit_ids", n);
    intern_first<<<tgrid(n), 256, 0, st>>>(ptr<uint32_t>(slotof), nullptr, n, ptr<uint32_t>(owner));
    intern_flag<<<tgrid(n), 256, 0, st>>>(ptr<uint32_t>(slotof), nullptr, ptr<uint32_t>(owner), n, ptr<uint32_t>(rank));
    exclusive_scan_u32(ptr<uint32_t>(rank), ptr<uint32_t>(rank), n, true);
    intern_ids<<<tgrid(n), 256, 0, st>>>(ptr<uint32_t>(slotof), nullptr, ptr<uint32_t>(owner), ptr<uint32_t>(rank), n, NOROW, ptr<uint32_t>(tid), ptr<uint32_t>(reps), ptr<uint32_t>(idx));
  }
  const uint32_t *hT = d2h_u32(ptr<uint32_t>(rank) + n), *hk = d2h_u32(kflag->p);
  sync();
  if (*hk) throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: the batch holds non-row kinds (TFGPU_K_OTHER / TFGPU_K_SYNCHRONIZE): those items go through the stock transformer");
  const int64_t T = *hT;

  // the T names: rendered from each table's first row
  Buf off = dalloc((size_t)(T + 1) * 4), total = dalloc_zero(8);
  std::vector<uint32_t> &hoff = res->name_off;
  std::vector<char> &text = res->text;
  hoff.assign((size_t)T + 1, 0u);
  {
    // (the timers close before every host sync and download: "tsplit_names" is the three name kernels, "tsplit_sort" the sort and the run heads)
    {
      KernelTimer t("tsplit_names", T);
      tsplit_name_len<<<tgrid(T), 256, 0, st>>>(sp, ptr<uint32_t>(reps), T, ptr<uint32_t>(off), ptr<unsigned long long>(total));
    }
    const uint32_t *ht = d2h_u32(total->p, 2);
    sync();
    const uint64_t bytes = (uint64_t)ht[0] | ((uint64_t)ht[1] << 32);
    if (bytes >> 32) throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer: the generated table names together reach 4 GiB of text: split the batch");
    Buf dtext = dalloc((size_t)bytes + 8);
    {
      KernelTimer t("tsplit_names", T);
      exclusive_scan_u32(ptr<uint32_t>(off), ptr<uint32_t>(off), T, true);
      tsplit_name_write<<<tgrid(T), 256, 0, st>>>(sp, ptr<uint32_t>(reps), T, ptr<uint32_t>(off), ptr<uint8_t>(dtext));
    }
    text.resize((size_t)bytes + 1);  // (+1: a name's pointer is valid even where every name is empty)
    d2h(hoff.data(), off->p, hoff.size() * 4);
    if (bytes) d2h(text.data(), dtext->p, (size_t)bytes);
    // (the sync below covers both copies; dtext lives until then)
    // grouping: rows sorted by table id, input order kept inside a table
    std::vector<uint32_t> &hstart = res->start;
    hstart.assign((size_t)T, 0u);
    if (T > 1) {
      unsigned bits = 1;
      while ((1ull << bits) < (uint64_t)T) bits++;
      Buf stid = dalloc((size_t)n * 4), sel = dalloc((size_t)n * 4 + 4), start = dalloc((size_t)T * 4);
      size_t tmp_bytes = 0;
      TF_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, ptr<uint32_t>(tid), ptr<uint32_t>(stid), ptr<uint32_t>(idx), ptr<uint32_t>(sel), (size_t)n, 0u, bits, st));
      Buf tmp = dalloc(tmp_bytes + 16);
      {
        KernelTimer ts("tsplit_sort", n);
        TF_HIP(rocprim::radix_sort_pairs(tmp->p, tmp_bytes, ptr<uint32_t>(tid), ptr<uint32_t>(stid), ptr<uint32_t>(idx), ptr<uint32_t>(sel), (size_t)n, 0u, bits, st));
        intern_heads<<<tgrid(n), 256, 0, st>>>(ptr<uint32_t>(stid), n, ptr<uint32_t>(start));
      }
      d2h(hstart.data(), start->p, hstart.size() * 4);
      sync();
      res->sel = sel;
    } else {
      sync();
      res->sel = idx;
    }
  }
  res->row_table = tid;
  return res;
}

}  // namespace tf

using namespace tf;

static int check_handle(const tfgpu_tablesplit *s, int32_t t, bool need_table, const char *what) {
  if (!s) return tf::fail(TFGPU_ERR_INVALID, std::string(what) + ": null handle");
  if (need_table && (t < 0 || (size_t)t >= s->ntables())) return tf::fail(TFGPU_ERR_INVALID, std::string(what) + ": table index out of range");
  return TFGPU_OK;
}

extern "C" {

int tfgpu_table_split(const tfgpu_plan *plan, const tfgpu_dbatch *in, tfgpu_tablesplit **out) {
  TF_API_BEGIN
  tf::dense(in, true);  // its rows may still be a selection (tfgpu_dbatch::pending); an ABSENT cell reads nil, as AsMap makes it
  if (!plan || !in || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_table_split: null argument");
  std::lock_guard<std::mutex> lk(ctx().mu);
  *out = split_batch(*plan, tf::snapshot(*in)).release();
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_apply_split(tfgpu_plan *const *plans, int nplans, const tfgpu_dbatch *in, tfgpu_tablesplit **out, tfgpu_row_error *errs, int64_t errs_cap, int64_t *nerrs) {
  TF_API_BEGIN
  if (nplans < 1 || !plans) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_apply_split: null argument");
  for (int i = 0; i < nplans; i++) if (!plans[i]) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_apply_split: null plan");
  for (int i = 0; i + 1 < nplans; i++)
    if (plans[i]->kind == PK_TABLE_SPLITTER)
      return tf::fail(TFGPU_ERR_UNSUPPORTED, "tfgpu_apply_split: a table_splitter_transformer that is not the chain's last step (or a second one): the transformers behind it go over each "
                                             "table's batch — run them with tfgpu_apply over tfgpu_tablesplit_batch's results");
  if (chain_raw_doc(plans, nplans))
    return tf::fail(TFGPU_ERR_UNSUPPORTED, "tfgpu_apply_split: raw_doc_grouper writes etl_updated_at from the rows' CommitTime, which this entry does not see: run it with tfgpu_apply_meta "
                                           "and split its result with tfgpu_table_split");
  if (plans[nplans - 1]->kind != PK_TABLE_SPLITTER) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_apply_split: the last plan must be the chain's table_splitter_transformer");
  if (!in || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_apply_split: null argument");
  std::lock_guard<std::mutex> lk(ctx().mu);
  ApplyCtx ax;
  std::unique_ptr<tfgpu_dbatch> cur = run_chain(plans, nplans - 1, *in, ax);
  std::unique_ptr<tfgpu_tablesplit> s = split_batch(*plans[nplans - 1], std::move(cur));
  if (nerrs) *nerrs = (int64_t)ax.errs.size();
  if (errs) for (int64_t k = 0; k < errs_cap && k < (int64_t)ax.errs.size(); k++) errs[k] = ax.errs[(size_t)k];
  *out = s.release();
  return TFGPU_OK;
  TF_API_END
}

int64_t tfgpu_tablesplit_rows(const tfgpu_tablesplit *s) { return s ? s->nrows : -1; }
int32_t tfgpu_tablesplit_count(const tfgpu_tablesplit *s) { return s ? (int32_t)s->ntables() : -1; }
const char *tfgpu_tablesplit_name(const tfgpu_tablesplit *s, int32_t t, size_t *len) {
  if (!s || t < 0 || (size_t)t >= s->ntables()) { if (len) *len = 0; return nullptr; }
  if (len) *len = s->name_off[(size_t)t + 1] - s->name_off[(size_t)t];
  return s->text.data() + s->name_off[(size_t)t];
}
int tfgpu_tablesplit_table_rows(const tfgpu_tablesplit *s, int32_t t, int64_t *nrows) {
  TF_API_BEGIN
  if (int rc = check_handle(s, t, true, "tfgpu_tablesplit_table_rows")) return rc;
  if (!nrows) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_tablesplit_table_rows: null argument");
  *nrows = s->count((size_t)t);
  return TFGPU_OK;
  TF_API_END
}
int tfgpu_tablesplit_row_tables(const tfgpu_tablesplit *s, int32_t *ids) {
  TF_API_BEGIN
  if (int rc = check_handle(s, 0, false, "tfgpu_tablesplit_row_tables")) return rc;
  if (!s->nrows) return TFGPU_OK;
  if (!ids) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_tablesplit_row_tables: null argument");
  if (current_lane() != s->lane) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_tablesplit_row_tables: the handle belongs to the lane that made it");
  std::lock_guard<std::mutex> lk(ctx().mu);
  d2h(ids, s->row_table->p, (size_t)s->nrows * 4);
  tf::sync();
  return TFGPU_OK;
  TF_API_END
}
int tfgpu_tablesplit_batch(const tfgpu_tablesplit *s, int32_t t, tfgpu_dbatch **out) {
  TF_API_BEGIN
  if (int rc = check_handle(s, t, true, "tfgpu_tablesplit_batch")) return rc;
  if (!out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_tablesplit_batch: null argument");
  if (current_lane() != s->lane) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_tablesplit_batch: the handle belongs to the lane that made it");
  std::lock_guard<std::mutex> lk(ctx().mu);
  std::unique_ptr<tfgpu_dbatch> b;
  if (s->ntables() == 1) {  // every row, in order: the input's own buffers
    b = shallow_copy(*s->src);
    if (!b->src_row) b->src_row = s->sel;  // (the identity, written out as the gather of several tables writes it)
  }
  else {
    const int64_t m = s->count((size_t)t);
    b = gather_rows(*s->src, subbuf(s->sel, (size_t)s->start[(size_t)t] * 4, (size_t)m * 4), m);
  }
  b->table = s->name((size_t)t);
  *out = b.release();
  return TFGPU_OK;
  TF_API_END
}
void tfgpu_tablesplit_free(tfgpu_tablesplit *s) { delete s; }

}  // extern "C"
