// tf_transform.hip — device kernels behind abstract.Transformer.Apply for the
// row transformers of SURVEY.md §8a (a6–a13), plus the apply dispatcher (mask_field: tf_mask.hip, sql: tf_sqleval.hip,
// regex_replace_transformer: tf_regex.hip; raw_doc_grouper: tf_rawdoc.hip; filter_rows_by_ids: tf_byids.hip; the row machinery under all of them: tf_rows.hip).
//
// All kernels are byte/row kernels: one lane per row, column-major (Arrow)
// buffers so that neighbouring lanes touch neighbouring addresses.  None of
// them is a contraction, so there is no MFMA here; all of them are HBM bound.
#include "tf_plan.hpp"
#include "tf_rows.hpp"
#include "tf_devrow.hpp"

namespace tf {

// transformation.do runs the transformers in their configured order.  A filter_rows directly behind mask_field transformers whose
// columns it does not read gives the same Transformed rows, the same row errors and the same failed inputs (once those are masked:
// push_run does) when it runs FIRST — mask_field raises no row errors, changes no other column and drops no row — and the HMACs of
// the rows it drops are never computed (45 % of them on configs[1]).  Returns the execution sequence; hopped[k] = the masks the
// k-th executed plan (a filter) went in front of.
std::vector<int> chain_sequence(const tfgpu_plan *const *plans, int n, std::vector<std::vector<int>> *hopped) {
  static const bool off = [] { const char *e = std::getenv("TFGPU_CHAIN_REORDER"); return e && e[0] == '0'; }();
  std::vector<int> seq((size_t)n);
  for (int i = 0; i < n; i++) seq[(size_t)i] = i;
  if (hopped) hopped->assign((size_t)n, {});
  if (off) return seq;
  for (int j = 1; j < n; j++) {
    if (plans[seq[(size_t)j]]->kind != PK_FILTER_ROWS) continue;
    const tfgpu_plan &f = *plans[seq[(size_t)j]];
    int k = j;
    std::vector<int> over;
    while (k > 0 && plans[seq[(size_t)k - 1]]->kind == PK_MASK) {
      const tfgpu_plan &m = *plans[seq[(size_t)k - 1]];
      bool reads = false;
      for (auto &e : f.exprs) for (auto &t : e.terms) if (m.mask_has(t.attr)) reads = true;
      if (reads) break;
      over.insert(over.begin(), seq[(size_t)k - 1]);
      std::swap(seq[(size_t)k - 1], seq[(size_t)k]);
      k--;
    }
    if (hopped) (*hopped)[(size_t)k] = over;
  }
  return seq;
}

// ============================================================================
// a11  filter_rows — filter_rows.go:99-365
// ============================================================================
struct DTerm {
  int32_t col;      // batch column index, -1 = not present in ColumnNames
  int32_t op, vtype, is_list;
  int32_t nvals;
  int32_t ioff;     // into ints / floats
  int32_t soff;     // into str_off (nvals+1 entries) for FV_STRING
};
struct FilterParams {
  const DCol *cols;
  int32_t ncols;
  const DTerm *terms;
  const int32_t *expr_start;  // nexpr+1
  int32_t nexpr;
  const int64_t *ints;
  const double *floats;
  const uint32_t *str_off;
  const uint8_t *str_data;
  const uint8_t *kind;
  int64_t nrows;
  const uint8_t *const *absent;  // [ncols] ABSENT bitmaps (DColumn::absent) or null entries; null: every row lists every column
  uint32_t *keep;   // 0/1 per row
  uint8_t *err;     // tfgpu_rowerr per row
  int32_t *err_term;
  uint32_t *nerr;   // global counter
};

__device__ __forceinline__ int cmp_op_i(int64_t a, int64_t b, int op) {
  switch (op) { case F_EQ: return a == b; case F_NE: return a != b; case F_LT: return a < b; case F_LE: return a <= b; case F_GT: return a > b; case F_GE: return a >= b; }
  return -1;
}
__device__ __forceinline__ int cmp_op_f(double a, double b, int op) {
  switch (op) { case F_EQ: return a == b; case F_NE: return a != b; case F_LT: return a < b; case F_LE: return a <= b; case F_GT: return a > b; case F_GE: return a >= b; }
  return -1;
}
__device__ __forceinline__ bool bytes_contains(const uint8_t *h, uint32_t hn, const uint8_t *n, uint32_t nn) {
  if (nn == 0) return true;
  if (nn > hn) return false;
  for (uint32_t i = 0; i + nn <= hn; i++) {
    uint32_t k = 0;
    while (k < nn && h[i + k] == n[k]) k++;
    if (k == nn) return true;
  }
  return false;
}

// time.Parse over the layouts of stringToTime (filter_rows/util.go:15-39) that
// are fixed-shape numeric: "2006-01-02", "2006-01-02 15:04:05", "2006-01-02T15:04:05",
// RFC3339 / RFC3339Nano.  Returns 1 ok, 0 = does not look like any of them
// (the row is then handed back to the host path), 2 = one of these shapes with a field out of range (Feb 30, 24:00, +25:00): its own
// layout reports the range, every other layout of stringToTime stops at its first punctuation mark, so no layout parses it.
__device__ __forceinline__ bool is_dg(uint8_t c) { return c >= '0' && c <= '9'; }
__device__ int parse_time_subset(const uint8_t *s, uint32_t n, int64_t *sec, int32_t *nsec) {
  if (n < 10) return 0;
  if (!(is_dg(s[0]) && is_dg(s[1]) && is_dg(s[2]) && is_dg(s[3]) && s[4] == '-' && is_dg(s[5]) && is_dg(s[6]) && s[7] == '-' && is_dg(s[8]) && is_dg(s[9]))) return 0;
  int64_t y = (s[0] - '0') * 1000 + (s[1] - '0') * 100 + (s[2] - '0') * 10 + (s[3] - '0');
  int mo = (s[5] - '0') * 10 + (s[6] - '0'), d = (s[8] - '0') * 10 + (s[9] - '0');
  int h = 0, mi = 0, se = 0; int64_t ns = 0; int off = 0; bool zone_range = false;
  uint32_t k = 10;
  if (n > 10) {
    if (!(s[10] == 'T' || s[10] == ' ')) return 0;
    bool tform = s[10] == 'T';
    if (n < 19) return 0;
    if (!(is_dg(s[11]) && is_dg(s[12]) && s[13] == ':' && is_dg(s[14]) && is_dg(s[15]) && s[16] == ':' && is_dg(s[17]) && is_dg(s[18]))) return 0;
    h = (s[11] - '0') * 10 + (s[12] - '0'); mi = (s[14] - '0') * 10 + (s[15] - '0'); se = (s[17] - '0') * 10 + (s[18] - '0');
    k = 19;
    if (k + 1 < n && (s[k] == '.' || s[k] == ',') && is_dg(s[k + 1])) {
      k++; int nd = 0;
      while (k < n && is_dg(s[k])) { if (nd < 9) { ns = ns * 10 + (s[k] - '0'); nd++; } k++; }
      while (nd < 9) { ns *= 10; nd++; }
    }
    if (k < n) {
      if (!tform) return 0;  // "2006-01-02 15:04:05 -0700 MST" etc: host path
      if (s[k] == 'Z') k++;
      else if ((s[k] == '+' || s[k] == '-') && k + 6 <= n && is_dg(s[k + 1]) && is_dg(s[k + 2]) && s[k + 3] == ':' && is_dg(s[k + 4]) && is_dg(s[k + 5])) {
        int hh = (s[k + 1] - '0') * 10 + (s[k + 2] - '0'), mm = (s[k + 4] - '0') * 10 + (s[k + 5] - '0');
        zone_range = hh > 24 || mm > 60;
        off = (s[k] == '-' ? -1 : 1) * (hh * 3600 + mm * 60);
        k += 6;
      } else return 0;
      if (k != n) return 0;
    }
  }
  if (zone_range || mo < 1 || mo > 12 || d < 1 || d > dev::days_in_month(mo, y) || h > 23 || mi > 59 || se > 59) return 2;
  *sec = dev::days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + se - off;
  *nsec = (int32_t)ns;
  return 1;
}

// matchValue (filter_rows.go:180-365).  Returns 1/0, or -(tfgpu_rowerr).
__device__ int match_value(const FilterParams &p, const DTerm &t, int64_t r) {
  const DCol &c = p.cols[t.col];
  const bool valid = is_valid(c, r);
  const bool is_set = t.op == F_IN || t.op == F_NOTIN;
  bool isInt1 = false, isFloat1 = false, maybeFloat = false;
  int64_t int1 = 0; double float1 = 0;
  if (valid) {
    switch (c.repr) {  // toInt64E util.go:42-82, then cast.ToFloat64E
      case TFGPU_R_INT8: int1 = ((const int8_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_INT16: int1 = ((const int16_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_INT32: int1 = ((const int32_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_INT64: int1 = ((const int64_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_UINT8: int1 = ((const uint8_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_UINT16: int1 = ((const uint16_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_UINT32: int1 = ((const uint32_t *)c.values)[r]; isInt1 = true; break;
      case TFGPU_R_UINT64: { uint64_t u = ((const uint64_t *)c.values)[r]; if (u > 0x7FFFFFFFFFFFFFFFull) return -TFGPU_ROW_INT_OVERFLOW; int1 = (int64_t)u; isInt1 = true; break; }
      case TFGPU_R_FLOAT32: float1 = ((const float *)c.values)[r]; isFloat1 = true; break;
      case TFGPU_R_FLOAT64: float1 = ((const double *)c.values)[r]; isFloat1 = true; break;
      case TFGPU_R_BOOL: float1 = ((const uint8_t *)c.values)[r] ? 1.0 : 0.0; isFloat1 = true; break;
      case TFGPU_R_STRING: case TFGPU_R_JSONNUM: maybeFloat = true; break;  // strconv.ParseFloat of text
      case TFGPU_R_JSON: {
        // an `any` cell is the value encoding/json decoded from its text.  A map or a slice meets no case below ("Unsupported type pair"); a string,
        // a number or a bool is compared as such by the reference (checkColumnSuitable admits TypeAny for string constants): the host path's to decode
        if (t.vtype == FV_NULL) break;
        const uint8_t *a = c.data + c.offsets[r]; uint32_t an = c.offsets[r + 1] - c.offsets[r], k = 0;
        while (k < an && (a[k] == ' ' || a[k] == '\t' || a[k] == '\n' || a[k] == '\r')) k++;
        return (k < an && (a[k] == '{' || a[k] == '[')) ? -TFGPU_ROW_TYPE_PAIR : -TFGPU_ROW_HOST_FALLBACK;
      }
    }
  } else { float1 = 0; isFloat1 = true; }  // cast.ToFloat64E(nil) == 0
  int res;
  switch (t.vtype) {
    case FV_INT:
      if (isInt1) {
        if (is_set) { bool f = false; for (int i = 0; i < t.nvals; i++) f = f || p.ints[t.ioff + i] == int1; return t.op == F_IN ? f : !f; }
        res = cmp_op_i(int1, p.ints[t.ioff], t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      if (maybeFloat) return -TFGPU_ROW_HOST_FALLBACK;
      if (isFloat1) {
        if (is_set) {
          if (trunc(float1) == float1) {
            // Go leaves int64(float1) outside the int64 range to the implementation (amd64: MinInt64, arm64: saturated; this device: neither): the host path's to answer
            if (!(float1 >= -0x1p63 && float1 < 0x1p63)) return -TFGPU_ROW_HOST_FALLBACK;
            int64_t iv = (int64_t)float1; bool f = false; for (int i = 0; i < t.nvals; i++) f = f || p.ints[t.ioff + i] == iv; return t.op == F_IN ? f : !f;
          }
          return 0;
        }
        res = cmp_op_f(float1, (double)p.ints[t.ioff], t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      break;
    case FV_FLOAT:
      if (maybeFloat && !isInt1) return -TFGPU_ROW_HOST_FALLBACK;
      if (isInt1 || isFloat1) {
        double a = isInt1 ? (double)int1 : float1;
        if (is_set) { bool f = false; for (int i = 0; i < t.nvals; i++) f = f || p.floats[t.ioff + i] == a; return t.op == F_IN ? f : !f; }
        res = cmp_op_f(a, p.floats[t.ioff], t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      break;
    case FV_BOOL:
      if (valid && c.repr == TFGPU_R_BOOL) {
        res = cmp_op_i(((const uint8_t *)c.values)[r] ? 1 : 0, p.ints[t.ioff], t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      break;
    case FV_STRING:
      if (valid && (c.repr == TFGPU_R_BYTES || c.repr == TFGPU_R_STRING)) {
        const uint8_t *a = c.data + c.offsets[r]; uint32_t an = c.offsets[r + 1] - c.offsets[r];
        const uint32_t *so = p.str_off + t.soff;
        if (t.op == F_MATCH || t.op == F_NOTMATCH) { bool m = bytes_contains(a, an, p.str_data + so[0], so[1] - so[0]); return t.op == F_MATCH ? m : !m; }
        if (is_set) {
          bool f = false;
          for (int i = 0; i < t.nvals; i++) { uint32_t bn = so[i + 1] - so[i]; if (bn == an && bytes_compare(a, an, p.str_data + so[i], bn) == 0) f = true; }
          return t.op == F_IN ? f : !f;
        }
        int cr = bytes_compare(a, an, p.str_data + so[0], so[1] - so[0]);
        res = cmp_op_i(cr, 0, t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      break;
    case FV_TIME: {
      int64_t us1 = 0; bool have = false;
      if (valid && c.repr == TFGPU_R_TIME) { us1 = ((const int64_t *)c.values)[r] * 1000000 + (c.nanos ? c.nanos[r] : 0) / 1000; have = true; }
      else if (valid && c.repr == TFGPU_R_STRING) {
        int64_t s; int32_t ns;
        int shape = parse_time_subset(c.data + c.offsets[r], c.offsets[r + 1] - c.offsets[r], &s, &ns);
        if (shape == 0) return -TFGPU_ROW_HOST_FALLBACK;
        if (shape == 2) break;  // stringToTime finds no layout: "Unsupported type pair"
        us1 = s * 1000000 + ns / 1000; have = true;
      }
      if (have) {
        if (is_set) { bool f = false; for (int i = 0; i < t.nvals; i++) f = f || p.ints[t.ioff + i] == us1; return t.op == F_IN ? f : !f; }
        res = cmp_op_i(us1, p.ints[t.ioff], t.op); return res < 0 ? -TFGPU_ROW_TYPE_PAIR : res;
      }
      break;
    }
    case FV_NULL:
      if (t.op == F_EQ) return !valid;
      if (t.op == F_NE) return valid;
      break;
  }
  return -TFGPU_ROW_TYPE_PAIR;
}

__global__ void __launch_bounds__(256) filter_eval_kernel(FilterParams p) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  int kind = p.kind ? p.kind[r] : TFGPU_K_INSERT;
  uint32_t keep = 0; int err = 0, eterm = -1;
  if (kind == TFGPU_K_UPDATE || kind == TFGPU_K_DELETE) err = TFGPU_ROW_UNSUPPORTED_KIND;  // :103-107
  else if (kind != TFGPU_K_INSERT || p.nexpr < 0) keep = 1;                              // :110-113 (nexpr<0: table not matched)
  else {
    for (int e = 0; e < p.nexpr && !keep && !err; e++) {  // matchItem :132-143
      bool ok = true;
      for (int k = p.expr_start[e]; k < p.expr_start[e + 1] && ok && !err; k++) {  // matchExpression :145-178
        const DTerm &t = p.terms[k];
        if (p.ncols == 0) continue;  // a row without columns never enters the name loop
        if (p.absent) {  // rows that list their own columns: the name loop runs over THIS row's ColumnNames (filter_rows.go:147-154)
          bool any = false;
          for (int c = 0; c < p.ncols && !any; c++) any = !(p.absent[c] && ((p.absent[c][r >> 3] >> (r & 7)) & 1));
          if (!any) continue;
          if (t.col >= 0 && p.absent[t.col] && ((p.absent[t.col][r >> 3] >> (r & 7)) & 1)) { err = TFGPU_ROW_COLUMN_NOT_FOUND; eterm = k; break; }
        }
        if (t.col < 0) { err = TFGPU_ROW_COLUMN_NOT_FOUND; eterm = k; break; }
        int m = match_value(p, t, r);
        if (m < 0) { err = -m; eterm = k; } else if (!m) ok = false;
      }
      if (!err && ok) keep = 1;
    }
  }
  p.keep[r] = err ? 0 : keep;
  p.err[r] = (uint8_t)err;
  if (err) { p.err_term[r] = eterm; atomicAdd(p.nerr, 1u); }
}

static void collect_row_errors(const Buf &err, const Buf &err_term, int64_t n, ApplyCtx &ax) {
  std::vector<uint8_t> he((size_t)n);
  std::vector<int32_t> ht((size_t)n);
  d2h(he.data(), err->p, (size_t)n);
  if (err_term) d2h(ht.data(), err_term->p, (size_t)n * 4);
  sync();
  for (int64_t r = 0; r < n; r++) if (he[(size_t)r]) ax.errs.push_back(tfgpu_row_error{r, he[(size_t)r], ax.step, err_term ? ht[(size_t)r] : -1});
}

// The predicate program (an OR of ANDs of terms) over a batch, then the compaction of the kept rows.  `check_kinds`:
// filter_rows' rule that only Inserts may be filtered (Update / Delete rows are fatal row errors); the sql transformer
// evaluates its WHERE on every row event.
static std::unique_ptr<tfgpu_dbatch> apply_filter_rows(const tfgpu_plan &p, const tfgpu_dbatch &in, ApplyCtx &ax) {
  // pass-through conditions that hold for the whole batch (one table per batch)
  if (!p.tables.match_table(in.ns, in.table) || is_system_table(in.table)) {
    // impossible kinds still raise errors before the table check (filter_rows.go:103-113)
    if (!in.kind) return shallow_copy(in);
  }
  const bool table_applies = p.tables.match_table(in.ns, in.table) && !is_system_table(in.table);
  return run_filter(p.exprs, table_applies, true, in, ax);
}
std::unique_ptr<tfgpu_dbatch> run_filter(const std::vector<FExpr> &p_exprs, bool table_applies, bool check_kinds, const tfgpu_dbatch &in, ApplyCtx &ax) {
  int64_t n = in.nrows;
  hipStream_t st = ctx().stream;
  // device program
  std::vector<DTerm> terms; std::vector<int32_t> expr_start{0};
  std::vector<int64_t> ints; std::vector<double> floats; std::vector<uint32_t> soff; std::string sdata;
  if (table_applies) {
    for (auto &e : p_exprs) {
      for (auto &t : e.terms) {
        DTerm d{};
        d.col = -1;
        for (size_t i = 0; i < in.cols.size(); i++) if (in.cols[i].name == t.attr) { d.col = (int32_t)i; break; }
        d.op = t.op; d.vtype = t.vtype; d.is_list = t.is_list;
        switch (t.vtype) {
          case FV_FLOAT: d.nvals = (int32_t)t.floats.size(); d.ioff = (int32_t)floats.size(); floats.insert(floats.end(), t.floats.begin(), t.floats.end()); break;
          case FV_STRING:
            d.nvals = (int32_t)t.strs.size(); d.soff = (int32_t)soff.size();
            for (auto &s : t.strs) { soff.push_back((uint32_t)sdata.size()); sdata += s; }
            soff.push_back((uint32_t)sdata.size());
            break;
          default: d.nvals = (int32_t)t.ints.size(); d.ioff = (int32_t)ints.size(); ints.insert(ints.end(), t.ints.begin(), t.ints.end());
        }
        terms.push_back(d);
      }
      expr_start.push_back((int32_t)terms.size());
    }
  }
  {
    std::vector<const DColumn *> need;
    for (auto &t : terms) if (t.col >= 0) need.push_back(&in.cols[(size_t)t.col]);
    materialize(in, &need);
  }
  std::vector<DCol> cols;
  for (auto &c : in.cols) {
    if (c.lazy() || c.lens_only()) { DColumn shell = c; shell.view = nullptr; cols.push_back(dcol_of(shell)); }  // no term reads it: its payload stays unpacked, its lengths unscanned
    else cols.push_back(dcol_of(c));
  }
  auto up = [&](const void *src, size_t bytes) { return upload_const(src, bytes); };  // tables the kernels only read
  Buf bcols = up(cols.data(), cols.size() * sizeof(DCol)), bterms = up(terms.data(), terms.size() * sizeof(DTerm));
  Buf bexpr = up(expr_start.data(), expr_start.size() * 4), bints = up(ints.data(), ints.size() * 8), bfl = up(floats.data(), floats.size() * 8);
  Buf bsoff = up(soff.data(), soff.size() * 4), bsd = up(sdata.data(), sdata.size());
  Buf keep = dalloc((size_t)(n + 1) * 4), err = dalloc((size_t)n + 1), eterm = dalloc((size_t)n * 4 + 4), nerr = dalloc_zero(4);
  FilterParams fp;
  fp.cols = ptr<DCol>(bcols); fp.ncols = (int32_t)cols.size(); fp.terms = ptr<DTerm>(bterms); fp.expr_start = ptr<int32_t>(bexpr);
  fp.nexpr = table_applies ? (int32_t)p_exprs.size() : 0;
  fp.ints = ptr<int64_t>(bints); fp.floats = ptr<double>(bfl); fp.str_off = ptr<uint32_t>(bsoff); fp.str_data = ptr<uint8_t>(bsd);
  fp.absent = nullptr;
  Buf babs;
  {
    std::vector<const uint8_t *> abs;
    bool any = false;
    for (auto &c : in.cols) { abs.push_back(ptr<uint8_t>(c.absent)); any = any || c.absent; }
    if (any) { babs = up(abs.data(), abs.size() * sizeof(const uint8_t *)); fp.absent = reinterpret_cast<const uint8_t *const *>(babs->p); }
  }
  fp.kind = check_kinds ? ptr<uint8_t>(in.kind) : nullptr; fp.nrows = n; fp.keep = ptr<uint32_t>(keep); fp.err = ptr<uint8_t>(err); fp.err_term = ptr<int32_t>(eterm); fp.nerr = ptr<uint32_t>(nerr);
  if (!table_applies) fp.nexpr = -1;  // only the kind check applies: emulate with zero expressions and keep-all for inserts
  {
    KernelTimer t("filter_rows_eval");
    if (n) filter_eval_kernel<<<grid_for(n, 256), 256, 0, st>>>(fp);
  }
  const uint32_t *hn = d2h_u32(nerr->p);
  auto out = compact(in, keep, true);  // syncs; the kept rows stay a selection until somebody reads them
  if (*hn) collect_row_errors(err, eterm, n, ax);
  return out;
}

// ============================================================================
// a10 skip_events — skip_events.go:52-62
// ============================================================================
__global__ void kind_keep_kernel(const uint8_t *kind, int64_t n, uint32_t skip_mask, uint32_t *keep) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) keep[r] = ((skip_mask >> kind[r]) & 1u) ? 0u : 1u;
}
static std::unique_ptr<tfgpu_dbatch> apply_skip_events(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  uint32_t mask = (p.skip[0] ? 1u : 0) | (p.skip[1] ? 2u : 0) | (p.skip[2] ? 4u : 0);
  int64_t n = in.nrows;
  if (!in.kind) {  // all rows are inserts
    if (!(mask & 1u)) return shallow_copy(in);
    Buf sel = dalloc(4);
    return gather_rows(in, sel, 0);
  }
  Buf keep = dalloc((size_t)(n + 1) * 4);
  if (n) kind_keep_kernel<<<grid_for(n, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(in.kind), n, mask, ptr<uint32_t>(keep));
  return compact(in, keep, true);
}

// ============================================================================
// a6 convert_to_string — to_string.go:58-97
// ============================================================================
// nil_empty: a nil value has no text (strictify leaves nil alone; convert_to_string prints "<nil>")
__global__ void __launch_bounds__(256) tostring_len_kernel(DCol c, int64_t n, uint32_t *len, int nil_empty) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint8_t buf[64]; const uint8_t *ext;
  if (nil_empty && c.validity && !((c.validity[r >> 3] >> (r & 7)) & 1)) { len[r] = 0; return; }
  len[r] = (uint32_t)serialize_small(c, r, buf, &ext);
}
__global__ void __launch_bounds__(256) tostring_write_kernel(DCol c, int64_t n, const uint32_t *off, uint8_t *data, int nil_empty) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint8_t buf[64]; const uint8_t *ext;
  if (nil_empty && c.validity && !((c.validity[r >> 3] >> (r & 7)) & 1)) return;
  int len = serialize_small(c, r, buf, &ext);
  uint8_t *dst = data + off[r];
  const uint8_t *src = ext ? ext : buf;
  struct __attribute__((packed, aligned(1))) U64 { uint64_t v; };
  int i = 0;
  for (; i + 8 <= len; i += 8) reinterpret_cast<U64 *>(dst + i)->v = reinterpret_cast<const U64 *>(src + i)->v;  // unaligned 8-byte moves
  for (; i < len; i++) dst[i] = src[i];
}

DColumn column_to_string(const DColumn &c, int64_t n, bool to_bytes, int max_len_hint, int nil_empty) {
  hipStream_t st = ctx().stream;
  DColumn o;
  o.name = c.name; o.dtype = to_bytes ? TFGPU_T_BYTES : TFGPU_T_UTF8; o.repr = to_bytes ? TFGPU_R_BYTES : TFGPU_R_STRING;
  o.offsets = dalloc((size_t)(n + 1) * 4);
  DCol dc = dcol_of(c);  // callers materialise text columns first
  KernelTimer t("to_string");
  if (n) tostring_len_kernel<<<grid_for(n, 256), 256, 0, st>>>(dc, n, ptr<uint32_t>(o.offsets), nil_empty);
  exclusive_scan_u32(ptr<uint32_t>(o.offsets), ptr<uint32_t>(o.offsets), n, true);
  uint64_t cap = repr_is_var(c.repr) ? c.data_len + (uint64_t)n * 5 : (uint64_t)n * (uint64_t)max_len_hint;
  o.data = dalloc(cap);
  if (n) tostring_write_kernel<<<grid_for(n, 256), 256, 0, st>>>(dc, n, ptr<uint32_t>(o.offsets), ptr<uint8_t>(o.data), nil_empty);
  const uint32_t *tot = d2h_u32(ptr<uint32_t>(o.offsets) + n);
  sync();
  o.data_len = *tot;
  return o;
}

DColumn column_to_text(const DColumn &c, int64_t n, bool to_bytes) { DColumn o = column_to_string(c, n, to_bytes, 64, 1); o.validity = c.validity; return o; }  // for tfgpu_strictify (tf_strictify.hip)

static std::unique_ptr<tfgpu_dbatch> apply_to_string(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  if (p.skip_utc) {
    for (auto &c : in.cols) if (p.columns.match(c.name) && c.repr == TFGPU_R_TIME)
      throw Error(TFGPU_ERR_UNSUPPORTED, "convert_to_string skip_utc_conversion=true needs per-value time zones, which the columnar batch does not carry");
  }
  materialize_where(in, [&](const DColumn &c) { return p.columns.match(c.name) && c.validity; });
  auto out = shallow_copy(in);
  for (auto &sc : out->schema) if (p.columns.match(sc.first)) sc.second = p.to_bytes ? TFGPU_T_BYTES : TFGPU_T_UTF8;  // to_string.go:114-127
  for (auto &c : out->cols) {
    if (!p.columns.match(c.name)) continue;
    require_serializable(c, "convert_to_string");
    // already text with identical bytes: only the type tag changes
    if (repr_is_var(c.repr) && !c.validity) { c.dtype = p.to_bytes ? TFGPU_T_BYTES : TFGPU_T_UTF8; c.repr = p.to_bytes ? TFGPU_R_BYTES : TFGPU_R_STRING; continue; }
    const Buf ab = c.absent;   // the transformer converts the values of the names a row LISTS (to_string.go: it walks item.ColumnNames): an ABSENT cell stays one
    c = column_to_string(c, in.nrows, p.to_bytes, 64);
    if (ab) { c.absent = ab; c.validity = validity_minus_absent(nullptr, ab, in.nrows); }
  }
  return out;
}

// ============================================================================
// a7 convert_to_datetime — to_datetime.go:89-149
// ============================================================================
template <typename T>
__global__ void todatetime_kernel(const T *in, int64_t n, int64_t *out) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) out[r] = (int64_t)in[r];
}
bool todatetime_values(const DColumn &src, int64_t n, int64_t *out) {  // for apply_sql (tf_sqleval.hip); false: not held as a 32 / 64-bit integer
  hipStream_t st = ctx().stream;
  if (src.repr == TFGPU_R_INT32) todatetime_kernel<int32_t><<<grid_for(n, 256), 256, 0, st>>>(ptr<int32_t>(src.values), n, out);
  else if (src.repr == TFGPU_R_UINT32) todatetime_kernel<uint32_t><<<grid_for(n, 256), 256, 0, st>>>(ptr<uint32_t>(src.values), n, out);
  else if (src.repr == TFGPU_R_INT64 || src.repr == TFGPU_R_UINT64) todatetime_kernel<int64_t><<<grid_for(n, 256), 256, 0, st>>>(ptr<int64_t>(src.values), n, out);
  else return false;
  return true;
}
static std::unique_ptr<tfgpu_dbatch> apply_to_datetime(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  auto out = shallow_copy(in);
  int64_t n = in.nrows;
  for (auto &sc : out->schema) if (p.columns.match(sc.first) && (sc.second == TFGPU_T_INT32 || sc.second == TFGPU_T_UINT32)) sc.second = TFGPU_T_DATETIME;  // to_datetime.go:125-133
  for (auto &c : out->cols) {
    if (!(p.columns.match(c.name) && (c.dtype == TFGPU_T_INT32 || c.dtype == TFGPU_T_UINT32))) continue;
    DColumn o;
    o.name = c.name; o.dtype = TFGPU_T_DATETIME; o.repr = TFGPU_R_TIME;
    o.values = dalloc_zero((size_t)n * 8);  // SerializeToDateTime falls back to time.Unix(0,0) on a type mismatch
    KernelTimer t("to_datetime");
    if (n && ((c.dtype == TFGPU_T_INT32 && c.repr == TFGPU_R_INT32) || (c.dtype == TFGPU_T_UINT32 && c.repr == TFGPU_R_UINT32))) todatetime_values(c, n, ptr<int64_t>(o.values));
    // nil values also become time.Unix(0,0): the value.(int32) assertion fails — an ABSENT cell is no value at all (the loop walks item.ColumnNames): it stays one
    if (c.absent) { o.absent = c.absent; o.validity = validity_minus_absent(nullptr, c.absent, n); }
    c = std::move(o);
  }
  return out;
}

// ============================================================================
// a13 sharder_transformer — sharder.go:130-145 (CRC32-IEEE of '.'-joined strings)
// ============================================================================
__device__ __forceinline__ uint32_t crc32_update(uint32_t crc, uint8_t b, const uint32_t *tab) { return tab[(crc ^ b) & 0xFF] ^ (crc >> 8); }

struct SharderParams {
  const DCol *cols;   // in schema order, already resolved (repr==0 → missing → "<nil>")
  int32_t ncols;
  int64_t nrows;
  uint32_t shards;
  uint32_t *part_id;
};
__global__ void __launch_bounds__(256) sharder_kernel(SharderParams p) {
  __shared__ uint32_t tab[256];
  {  // build the IEEE table (reflected 0xEDB88320) once per block
    uint32_t c = threadIdx.x;
    for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    tab[threadIdx.x] = c;
  }
  __syncthreads();
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nrows) return;
  uint32_t crc = 0xFFFFFFFFu;
  for (int i = 0; i < p.ncols; i++) {
    if (i) crc = crc32_update(crc, '.', tab);
    {  // an integer key (the usual one): its digits go from registers into the CRC, most significant first — no text buffer
      const DCol &c = p.cols[i];
      bool isint = true, neg = false;
      uint64_t mag = 0;
      if (c.repr == 0 || !is_valid(c, r)) isint = false;
      else switch (c.repr) {
        case TFGPU_R_INT8: { const int64_t v = ((const int8_t *)c.values)[r]; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; break; }
        case TFGPU_R_INT16: { const int64_t v = ((const int16_t *)c.values)[r]; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; break; }
        case TFGPU_R_INT32: { const int64_t v = ((const int32_t *)c.values)[r]; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; break; }
        case TFGPU_R_INT64: { const int64_t v = ((const int64_t *)c.values)[r]; neg = v < 0; mag = neg ? (uint64_t)(-(v + 1)) + 1u : (uint64_t)v; break; }
        case TFGPU_R_UINT8: mag = ((const uint8_t *)c.values)[r]; break;
        case TFGPU_R_UINT16: mag = ((const uint16_t *)c.values)[r]; break;
        case TFGPU_R_UINT32: mag = ((const uint32_t *)c.values)[r]; break;
        case TFGPU_R_UINT64: mag = ((const uint64_t *)c.values)[r]; break;
        default: isint = false;
      }
      if (isint) {
        if (neg) crc = crc32_update(crc, '-', tab);
        bool started = false;
        auto piece = [&](uint32_t x, bool last) {  // nine digits of x < 10^9; leading zeros of the number are not part of its text
          uint32_t pw = 100000000u;
#pragma unroll
          for (int k = 0; k < 9; k++) {
            const uint32_t d = x / pw; x -= d * pw; pw /= 10u;
            started = started || d != 0 || (last && k == 8);
            if (started) crc = crc32_update(crc, (uint8_t)('0' + d), tab);
          }
        };
        if (mag >> 32) {
          const uint64_t q = mag / 1000000000ull;
          const uint32_t lo = (uint32_t)(mag - q * 1000000000ull);
          if (q >> 32) {
            const uint32_t q2 = (uint32_t)(q / 1000000000ull);
            const uint32_t d1 = q2 / 10u;  // q2 <= 18
            if (d1) crc = crc32_update(crc, (uint8_t)('0' + d1), tab);
            crc = crc32_update(crc, (uint8_t)('0' + (q2 - d1 * 10u)), tab);
            started = true;
            piece((uint32_t)(q - (uint64_t)q2 * 1000000000ull), false);
          } else {
            const uint32_t qq = (uint32_t)q;  // 1 .. 4 294 967 295: ten digits at most
            const uint32_t d9 = qq / 1000000000u;
            if (d9) { crc = crc32_update(crc, (uint8_t)('0' + d9), tab); started = true; }
            piece(qq - d9 * 1000000000u, false);
          }
          piece(lo, true);
        } else {
          const uint32_t x = (uint32_t)mag;
          const uint32_t d9 = x / 1000000000u;
          if (d9) { crc = crc32_update(crc, (uint8_t)('0' + d9), tab); started = true; }
          piece(x - d9 * 1000000000u, true);
        }
        continue;
      }
    }
    uint8_t buf[64]; const uint8_t *ext = nullptr; int len;
    if (p.cols[i].repr == 0) { buf[0] = '<'; buf[1] = 'n'; buf[2] = 'i'; buf[3] = 'l'; buf[4] = '>'; len = 5; }
    else len = serialize_small(p.cols[i], r, buf, &ext);
    if (ext) for (int k = 0; k < len; k++) crc = crc32_update(crc, ext[k], tab);
    else for (int k = 0; k < len; k++) crc = crc32_update(crc, buf[k], tab);
  }
  p.part_id[r] = (crc ^ 0xFFFFFFFFu) % p.shards;
}

static std::unique_ptr<tfgpu_dbatch> apply_sharder(const tfgpu_plan &p, const tfgpu_dbatch &in, const tfgpu_schema *schema_order) {
  auto out = shallow_copy(in);
  int64_t n = in.nrows;
  // Columns are visited in TableSchema order; without a separate schema the
  // batch column order stands in for it (they coincide for every source that
  // builds ColumnNames from the schema).
  materialize_where(in, [&](const DColumn &c) { return p.columns.match(c.name); });
  std::vector<DCol> cols;
  if (in.schema.empty()) {
    for (auto &c : in.cols) {
      if (!p.columns.match(c.name)) continue;
      require_serializable(c, "sharder_transformer");
      cols.push_back(dcol_of(c));
    }
  } else {  // item.TableSchema.Columns() in order, values through AsMap()[name]: a schema column without a value is nil
    for (auto &sc : in.schema) {
      if (!p.columns.match(sc.first)) continue;
      const DColumn *found = nullptr;
      for (auto &c : in.cols) if (c.name == sc.first) found = &c;  // AsMap: the last duplicate name wins
      if (!found) { DCol nil{}; nil.repr = 0; nil.dtype = sc.second; cols.push_back(nil); continue; }
      require_serializable(*found, "sharder_transformer");
      DCol d = dcol_of(*found);
      d.dtype = sc.second;
      cols.push_back(d);
    }
  }
  Buf bc = upload_small(cols.data(), cols.size() * sizeof(DCol));
  out->part_id = dalloc((size_t)n * 4 + 4);
  SharderParams sp{ptr<DCol>(bc), (int32_t)cols.size(), n, (uint32_t)p.shards, ptr<uint32_t>(out->part_id)};
  KernelTimer t("sharder_crc32");
  if (n) sharder_kernel<<<grid_for(n, 256), 256, 0, ctx().stream>>>(sp);
  return out;
}

// ============================================================================
// metadata-only transformers
// ============================================================================
static std::unique_ptr<tfgpu_dbatch> apply_rename(const tfgpu_plan &p, const tfgpu_dbatch &in) {  // rename.go:46-61
  auto out = shallow_copy(in);
  for (auto &r : p.renames) if (r[0] == in.ns && r[1] == in.table) { out->ns = r[2]; out->table = r[3]; break; }
  return out;
}
static std::unique_ptr<tfgpu_dbatch> apply_filter_columns(const tfgpu_plan &p, const tfgpu_dbatch &in) {  // filter_columns_transformer.go:51-79
  auto out = shallow_copy(in);
  out->cols.clear();
  for (auto &c : in.cols) if (p.columns.match(c.name)) out->cols.push_back(c);
  out->schema.clear();
  for (auto &sc : in.schema) if (p.columns.match(sc.first)) out->schema.push_back(sc);
  out->old_keys.clear();  // trimChangeItem also trims OldKeys (filter_columns_transformer.go:187-213)
  for (auto &c : in.old_keys) if (p.columns.match(c.name)) out->old_keys.push_back(c);
  return out;
}

__global__ void kind_is_kernel(const uint8_t *kind, int64_t n, uint8_t k, uint8_t *bits) {  // one thread per output byte
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b * 8 >= n) return;
  uint32_t v = 0;
  for (int j = 0; j < 8; j++) { const int64_t r = b * 8 + j; if (r < n && kind[r] == k) v |= 1u << j; }
  bits[b] = (uint8_t)v;
}
__global__ void kind_any_kernel(const uint8_t *kind, int64_t n, uint8_t k, uint32_t *flag) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && kind[r] == k) *flag = 1u;
}
__global__ void bitmap_or_kernel(uint8_t *a, const uint8_t *b, int64_t nbytes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nbytes) a[i] |= b[i];
}
// OldKeys of a run whose rows already carry some: an Update takes the key column's current value, any other row keeps its old one
// (one thread per validity byte = 8 rows)
__global__ void replace_pk_select_kernel(const uint8_t *kind, int64_t n, int w, const uint8_t *cur, const uint8_t *cur_valid, const uint8_t *old, const uint8_t *old_valid,
                                         uint8_t *out, uint8_t *out_valid) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b * 8 >= n) return;
  uint32_t v = 0;
  for (int j = 0; j < 8; j++) {
    const int64_t r = b * 8 + j;
    if (r >= n) break;
    const bool upd = kind[r] == TFGPU_K_UPDATE;
    const uint8_t *src = upd ? cur : old, *sv = upd ? cur_valid : old_valid;
    for (int k = 0; k < w; k++) out[r * w + k] = src[r * w + k];
    if (!sv || ((sv[r >> 3] >> (r & 7)) & 1)) v |= 1u << j;
  }
  out_valid[b] = (uint8_t)v;
}
// replace_primary_key.go:82-101: the TableSchema is replaced (keys first / flags rewritten); ColumnNames and ColumnValues
// stay as they are; an Update gets OldKeys = the NEW keys' current values (createOldKeys :51-80).
static std::unique_ptr<tfgpu_dbatch> apply_replace_pk(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  auto out = shallow_copy(in);
  std::vector<SchemaCol> cols;
  if (!in.schema.empty()) for (auto &c : in.schema) cols.push_back(SchemaCol{c.first, c.second, 0u});
  else for (auto &c : in.cols) cols.push_back(SchemaCol{c.name, c.dtype, 0u});
  plan_result_columns(p, cols);
  out->schema.clear(); out->key_names.clear();
  for (auto &c : cols) { out->schema.emplace_back(c.name, c.dtype); if (c.flags & TFGPU_COL_KEY) out->key_names.push_back(c.name); }
  bool has_update = false;
  if (in.kind && in.nrows) {  // one flag word read back, not the kinds
    Buf flag = dalloc_zero(4);
    kind_any_kernel<<<grid_for(in.nrows, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(in.kind), in.nrows, (uint8_t)TFGPU_K_UPDATE, ptr<uint32_t>(flag));
    const uint32_t *h = d2h_u32(flag->p);
    sync();
    has_update = *h != 0;
  }
  if (has_update) {
    std::vector<DColumn> cur;
    for (auto &k : p.new_keys)  // key order; a key missing from ColumnNames leaves a nil value in the reference — not modelled
      for (auto &c : in.cols) if (c.name == k) { cur.push_back(c); break; }
    if (cur.size() != p.new_keys.size()) throw Error(TFGPU_ERR_UNSUPPORTED, "replace_primary_key: a new key is not among the batch's columns");
    if (in.old_keys.empty()) {
      out->old_keys = cur;
      out->old_present = dalloc((size_t)(in.nrows + 7) / 8 + 8);
      kind_is_kernel<<<grid_for((in.nrows + 7) / 8, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(in.kind), in.nrows, (uint8_t)TFGPU_K_UPDATE, ptr<uint8_t>(out->old_present));
    } else {
      // the batch already carries OldKeys (every pg / Debezium CDC batch does): Updates get the NEW keys' current values, the other
      // rows keep theirs.  Columnar only when both sets have the same names, types and fixed-width representations (per-item
      // KeyNames otherwise: that run stays with the stock transformer)
      bool same = in.old_keys.size() == cur.size();
      for (size_t i = 0; same && i < cur.size(); i++)
        same = in.old_keys[i].name == cur[i].name && in.old_keys[i].repr == cur[i].repr && in.old_keys[i].dtype == cur[i].dtype && !repr_is_var(cur[i].repr) && cur[i].repr != TFGPU_R_TIME;
      if (!same) throw Error(TFGPU_ERR_UNSUPPORTED, "replace_primary_key: a run that mixes Updates with rows carrying OldKeys of other key names (or text / time keys) needs per-item KeyNames; not columnar");
      const int64_t n = in.nrows;
      out->old_keys.clear();
      for (size_t i = 0; i < cur.size(); i++) {
        DColumn d = in.old_keys[i];
        const int w = repr_width(cur[i].repr);
        d.values = dalloc((size_t)n * (size_t)w);
        d.validity = dalloc((size_t)(n + 7) / 8 + 8);
        replace_pk_select_kernel<<<grid_for((n + 7) / 8, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(in.kind), n, w, (const uint8_t *)cur[i].values->p, ptr<uint8_t>(cur[i].validity),
                                                                                      (const uint8_t *)in.old_keys[i].values->p, ptr<uint8_t>(in.old_keys[i].validity), (uint8_t *)d.values->p, ptr<uint8_t>(d.validity));
        out->old_keys.push_back(std::move(d));
      }
      if (in.old_present) {  // present = Update, or it was
        out->old_present = dalloc((size_t)(n + 7) / 8 + 8);
        kind_is_kernel<<<grid_for((n + 7) / 8, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(in.kind), n, (uint8_t)TFGPU_K_UPDATE, ptr<uint8_t>(out->old_present));
        bitmap_or_kernel<<<grid_for((n + 7) / 8, 256), 256, 0, ctx().stream>>>(ptr<uint8_t>(out->old_present), ptr<uint8_t>(in.old_present), (n + 7) / 8);
      }
    }
  }
  return out;
}

std::unique_ptr<tfgpu_dbatch> apply_plan(const tfgpu_plan &p, const tfgpu_dbatch &in, ApplyCtx &ax) {
  // transformers compute on values: an ABSENT cell is not a nil (the stock path takes the batch) — but for the sharder, which reads its key
  // columns through AsMap()[name] (sharder.go:134-143: a name the item does not list IS nil there) and passes every column on untouched
  // Since round 6 the transformers that walk an item's own ColumnNames do so here too: mask_field / convert_to_string / convert_to_datetime leave a
  // cell the row does not list as it is (hmac_hasher.go:56-63), filter_rows fails such a row ("Unable to find column", filter_rows.go:147-154),
  // the column droppers and the row filters carry the bitmaps.  `sql` (it serializes whole rows for clickhouse-local) and batches whose rows carry
  // their own name ORDER (col_order indexes the column list these transformers change) stay with the stock path.
  // regex_replace_transformer's rule is positional (the i-th value against the i-th schema column): rows that list their own columns stay with the stock path too.
  if (p.kind == PK_TABLE_SPLITTER)
    throw Error(TFGPU_ERR_UNSUPPORTED, "table_splitter_transformer files the rows under several tables and a batch is one table: it runs last, through tfgpu_apply_split");
  if (p.kind == PK_RAW_DOC_GROUPER) {  // it reads ABSENT cells itself (a row's doc holds the columns the row lists)
    if (!ax.has_meta)
      throw Error(TFGPU_ERR_UNSUPPORTED, "raw_doc_grouper writes etl_updated_at from the rows' CommitTime, which this entry does not see: run the chain with tfgpu_apply_meta");
    if (in.col_order)
      throw Error(TFGPU_ERR_UNSUPPORTED, "raw_doc_grouper: the batch's rows carry their own ColumnNames order (col_order: a collapsed batch), which the result's column list does not carry");
  }
  if (p.kind == PK_FILTER_ROWS_BY_IDS && in.col_order)  // (ABSENT cells it reads itself: AsMap has no entry for them)
    throw Error(TFGPU_ERR_UNSUPPORTED, "filter_rows_by_ids: the batch's rows carry their own ColumnNames order (col_order: a collapsed batch); such rows stay with the stock transformer");
  if (p.kind == PK_SQL || p.kind == PK_REGEX_REPLACE || (in.col_order && p.kind != PK_SHARDER)) refuse_absent(in);
  // `in` is the caller's OWN copy of the handle it was given (tfgpu_apply and push_run take it with snapshot(), under the transition's lock): nobody
  // else changes it.  A copy taken after another lane made the handle dense carries that lane's event: this lane's stream waits for it here.
  if (in.pending && (p.kind != PK_MASK || has_absent(in))) dense_locked(in);  // only mask_field reads through a selection
  else if (!in.pending) wait_dense(in);  // (the callers hold the lane's mutex)
  switch (p.kind) {
    case PK_MASK: return apply_mask(p, in);
    case PK_RENAME: return apply_rename(p, in);
    case PK_FILTER_COLUMNS: return apply_filter_columns(p, in);
    case PK_SKIP_EVENTS: return apply_skip_events(p, in);
    case PK_FILTER_ROWS: return apply_filter_rows(p, in, ax);
    case PK_TO_STRING: return apply_to_string(p, in);
    case PK_TO_DATETIME: return apply_to_datetime(p, in);
    case PK_SHARDER: return apply_sharder(p, in, nullptr);
    case PK_REPLACE_PK: return apply_replace_pk(p, in);
    case PK_SQL: return apply_sql(p, in, ax);
    case PK_REGEX_REPLACE: return apply_regex_replace(p, in);
    case PK_RAW_DOC_GROUPER: return apply_raw_doc(p, in, ax);
    case PK_FILTER_ROWS_BY_IDS: return apply_filter_by_ids(p, in);
    case PK_TABLE_SPLITTER: break;  // (refused above)
  }
  throw Error(TFGPU_ERR_INVALID, "unknown plan kind");
}

}  // namespace tf
