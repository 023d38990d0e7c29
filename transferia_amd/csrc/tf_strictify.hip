// tf_strictify.hip — tfgpu_strictify: strictify.Strictify (pkg/abstract/changeitem/strictify/strictify.go:17-157) over a device batch, what
// the strictifying serializers run before they serialize (pkg/serializer/strictify.go:24-36).  Every column named by the TableSchema is
// brought to the strict Go type of its DataType.  A text cell goes through strict_cell (tf_strictcell.hpp), the conversion the text
// ingests share; the integer and float families convert with Go's range rules.  Also the host half of tf_strictcell.hpp that needs
// kernels: the two system columns of the text ingests.
#include <algorithm>

#include "tf_strictcell.hpp"
#include "tf_plan.hpp"

using namespace tf;

namespace tf {

__global__ void fill_row_index(uint64_t *out, const uint32_t *rank, int64_t n, uint64_t base) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) out[r] = base + (rank ? (uint64_t)rank[r] : (uint64_t)r);  // the reader's line counter: CSV counts every line read, failed or not; nginx skips blank ones
}
__global__ void fill_const_text(uint32_t *off, uint8_t *data, int64_t n, const uint8_t *text, uint32_t len) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n) return;
  off[r] = (uint32_t)r * len;
  if (r < n) for (uint32_t i = 0; i < len; i++) data[(uint64_t)r * len + i] = text[i];
}
int fill_system_column(DColumn &d, int64_t nrows, const char *file_name, uint64_t row_number_base, const uint32_t *rank, bool hide, std::string *detail) {
  hipStream_t st = ctx().stream;
  auto blocks = [](int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); };
  const bool is_name = d.repr == TFGPU_R_STRING;
  if (!is_name) {
    d.values = dalloc((size_t)std::max<int64_t>(nrows, 1) * 8);
    if (nrows) fill_row_index<<<blocks(nrows), 256, 0, st>>>(ptr<uint64_t>(d.values), rank, nrows, row_number_base);
  } else {
    const std::string fn = file_name ? file_name : "";
    Buf btext = upload_small(fn.data(), fn.size());
    d.offsets = dalloc((size_t)(nrows + 1) * 4 + 16);
    d.data_len = (uint64_t)fn.size() * (uint64_t)nrows;
    if (d.data_len >> 32) { *detail = "__file_name column exceeds 4 GiB"; return TFGPU_ERR_UNSUPPORTED; }
    d.data = dalloc(d.data_len + 8);
    fill_const_text<<<blocks(nrows + 1), 256, 0, st>>>(ptr<uint32_t>(d.offsets), ptr<uint8_t>(d.data), nrows, ptr<uint8_t>(btext), (uint32_t)fn.size());
  }
  if (hide) {  // both are nil
    d.validity = dalloc_zero((size_t)(nrows + 7) / 8 + 8);
    if (is_name) { d.data_len = 0; TF_HIP(hipMemsetAsync(d.offsets->p, 0, (size_t)(nrows + 1) * 4, st)); }
  }
  return TFGPU_OK;
}

enum StrictMode : int32_t { SM_TEXT = 1, SM_TEXT_JSONNUM_OUT = 2, SM_INTS = 3, SM_JSONNUM_TO_TIME = 4, SM_FAIL = 5 /* no conversion exists: every value fails */,
                            SM_FLOATS = 6 /* Go float64 / float32 values under integer / bool / float DataTypes */ };
struct StrictCol {
  int32_t mode, src_repr;
  const void *values; const uint32_t *offsets; const uint8_t *data; const uint8_t *validity;
  StrictOut out;
};
__device__ __forceinline__ bool strict_load_int(const StrictCol &c, int64_t r, int64_t *v, uint64_t *u, bool *is_unsigned) {
  *is_unsigned = false;
  switch (c.src_repr) {
    case TFGPU_R_INT8: *v = ((const int8_t *)c.values)[r]; return true;
    case TFGPU_R_INT16: *v = ((const int16_t *)c.values)[r]; return true;
    case TFGPU_R_INT32: *v = ((const int32_t *)c.values)[r]; return true;
    case TFGPU_R_INT64: *v = ((const int64_t *)c.values)[r]; return true;
    case TFGPU_R_UINT8: case TFGPU_R_BOOL: *u = ((const uint8_t *)c.values)[r]; break;
    case TFGPU_R_UINT16: *u = ((const uint16_t *)c.values)[r]; break;
    case TFGPU_R_UINT32: *u = ((const uint32_t *)c.values)[r]; break;
    case TFGPU_R_UINT64: *u = ((const uint64_t *)c.values)[r]; break;
    default: return false;
  }
  *is_unsigned = true; *v = (int64_t)*u;
  return true;
}
// item = column * nrows + row; first_bad[column] = min over failing rows of (row << 8 | tfgpu_rowerr)
__global__ void __launch_bounds__(256) strictify_cells(GtSet cast_tp, const uint64_t *p128, const StrictCol *cols, int32_t ncols, int64_t nrows, unsigned long long *first_bad) {
  const int32_t j = (int32_t)blockIdx.y; const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (the column is the grid's y: a scalar)
  if (r >= nrows || j >= ncols) return;
  const StrictCol &c = cols[j];
  if (c.validity && !((c.validity[r >> 3] >> (r & 7)) & 1)) { if (c.mode != SM_TEXT_JSONNUM_OUT && c.mode != SM_FAIL) store_default(c.out, r); return; }  // nil stays nil
  int rc = 0;
  if (c.mode == SM_FAIL) rc = TFGPU_ROW_CAST;  // castx.ToByteSliceE of anything but []byte / string: "no known conversion"
  else if (c.mode == SM_FLOATS) {
    // cast.ToInt64E / ToUint64E / ToBoolE / ToFloat32E of a float: Go conversions (caste.go of spf13/cast); what a conversion of a NaN or of a
    // magnitude beyond the integer range yields is the machine's business, so those go back to the host
    const double f = c.src_repr == TFGPU_R_FLOAT32 ? (double)((const float *)c.values)[r] : ((const double *)c.values)[r];
    switch (c.out.kind) {
      case SK_INT:
        if (!(f > -9223372036854775808.0 && f < 9223372036854775808.0)) rc = TFGPU_ROW_HOST_FALLBACK;
        else { const int64_t x = (int64_t)f; if (x < c.out.lo || x > (int64_t)c.out.hi) rc = TFGPU_ROW_RANGE; else store_int(c.out, r, x); }
        break;
      case SK_UINT:
        if (f != f || f >= 18446744073709551616.0) rc = TFGPU_ROW_HOST_FALLBACK;
        else if (f < 0) rc = TFGPU_ROW_CAST;  // errNegativeNotAllowed
        else { const uint64_t x = (uint64_t)f; if (x > c.out.hi) rc = TFGPU_ROW_RANGE; else if (c.out.width == 8) ((uint64_t *)c.out.values)[r] = x; else store_int(c.out, r, (int64_t)x); }
        break;
      case SK_BOOL: ((uint8_t *)c.out.values)[r] = f != 0 ? 1 : 0; break;
      default: ((float *)c.out.values)[r] = (float)f;  // SK_F32
    }
  }
  else if (c.mode == SM_INTS) {
    int64_t v = 0; uint64_t u = 0; bool uns = false;
    strict_load_int(c, r, &v, &u, &uns);
    switch (c.out.kind) {
      case SK_INT:  // cast.ToInt64E of an integer kind is a Go conversion (a uint64 wraps), then toSignedInt's limits (strictify.go:159-169)
        if (v < c.out.lo || v > (int64_t)c.out.hi) rc = TFGPU_ROW_RANGE; else store_int(c.out, r, v);
        break;
      case SK_UINT:  // errNegativeNotAllowed, then toUnsignedInt's limit (:171-181)
        if (!uns && v < 0) rc = TFGPU_ROW_CAST;
        else { const uint64_t x = uns ? u : (uint64_t)v; if (x > c.out.hi) rc = TFGPU_ROW_RANGE; else if (c.out.width == 8) ((uint64_t *)c.out.values)[r] = x; else store_int(c.out, r, (int64_t)x); }
        break;
      case SK_BOOL: ((uint8_t *)c.out.values)[r] = (uns ? u != 0 : v != 0) ? 1 : 0; break;
      case SK_F32: ((float *)c.out.values)[r] = uns ? (float)(double)u : (float)(double)v; break;
      case SK_TIME: ((int64_t *)c.out.values)[r] = v; c.out.nanos[r] = 0; break;
      default: ((int64_t *)c.out.values)[r] = v;  // SK_INTERVAL: time.Duration(v)
    }
  } else {
    const uint32_t a = c.offsets[r], n = c.offsets[r + 1] - a;
    MemBytes rd(c.data);
    const Field fv{&rd, a, n};
    if (c.mode == SM_TEXT_JSONNUM_OUT) rc = json_number_ok(fv, 0, n) ? 0 : TFGPU_ROW_CAST;  // castx.ToJSONNumberE: the text itself is the json.Number
    else if (c.mode == SM_JSONNUM_TO_TIME) {  // cast.ToTimeE(json.Number): its Int64 as Unix seconds
      int64_t sec;
      if (parse_int64(fv, 0, n, false, &sec)) rc = TFGPU_ROW_CAST; else { ((int64_t *)c.out.values)[r] = sec; c.out.nanos[r] = 0; }
    } else rc = strict_cell(c.out, cast_tp, p128, r, fv, 0, n);
  }
  if (rc) atomicMin(&first_bad[j], ((unsigned long long)r << 8) | (unsigned long long)rc);
}

// castx.ToStringE of a Go float (caste.go:64-67): strconv.FormatFloat(f, 'f', -1, bits) — the text of a "utf8" column, and (through
// castx.ToJSONNumberE) the json.Number of a "double" one
__global__ void __launch_bounds__(256) strict_float_text(const void *values, int is32, const uint8_t *validity, int64_t n, uint32_t *off, uint8_t *data) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const bool nil = validity && !((validity[r >> 3] >> (r & 7)) & 1);
  const double f = is32 ? (double)((const float *)values)[r] : ((const double *)values)[r];
  if (!data) { dev::CountOut c; if (!nil) dev::fmt_float(c, f, 'f', is32 ? 32 : 64); off[r] = c.n; return; }
  if (nil) return;
  dev::StoreOut o{data + off[r]};
  dev::fmt_float(o, f, 'f', is32 ? 32 : 64);
}
static DColumn float_column_text(const DColumn &c, int64_t n) {
  hipStream_t st = ctx().stream;
  DColumn o;
  o.offsets = dalloc((size_t)(n + 1) * 4 + 16);
  const int is32 = c.repr == TFGPU_R_FLOAT32;
  if (n) strict_float_text<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(c.values->p, is32, ptr<uint8_t>(c.validity), n, ptr<uint32_t>(o.offsets), nullptr);
  exclusive_scan_u32(ptr<uint32_t>(o.offsets), ptr<uint32_t>(o.offsets), n, true);
  const uint32_t *tot = d2h_u32(ptr<uint32_t>(o.offsets) + n);
  tf::sync();
  o.data_len = *tot;
  o.data = dalloc((size_t)o.data_len + 16);
  if (n) strict_float_text<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(c.values->p, is32, ptr<uint8_t>(c.validity), n, ptr<uint32_t>(o.offsets), ptr<uint8_t>(o.data));
  o.validity = c.validity;
  return o;
}

}  // namespace tf

extern "C" int tfgpu_strictify(const tfgpu_dbatch *in, const tfgpu_schema *schema, tfgpu_dbatch **out, int64_t *bad_row, int32_t *bad_col) {
  TF_API_BEGIN
  tf::dense(in);  // its rows may still be a selection (tfgpu_dbatch::pending)
  if (!in || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_strictify: null argument");
  Context &cx = ctx();
  std::lock_guard<std::mutex> lk(cx.mu);
  hipStream_t st = cx.stream;
  materialize(*in);
  const int64_t n = in->nrows;
  if (bad_row) *bad_row = -1;
  if (bad_col) *bad_col = -1;
  auto dtype_of = [&](const DColumn &c) -> int {  // tableSchema[columnName]; a column the schema does not name is left alone
    if (schema) { for (int i = 0; i < schema->ncols; i++) if (schema->cols[i].name && c.name == schema->cols[i].name) return schema->cols[i].dtype; return -1; }
    if (!in->schema.empty()) { for (auto &p : in->schema) if (p.first == c.name) return p.second; return -1; }
    return c.dtype;
  };
  auto r = std::make_unique<tfgpu_dbatch>(*in);  // shares every buffer; converted columns are replaced below
  std::vector<StrictCol> sc; std::vector<int> which;
  std::vector<size_t> float_text;  // Go floats under "utf8" / "double": FormatFloat 'f'
  std::vector<size_t> to_text;  // columns whose strict form is their text (castx.ToStringE of a number / bool / time): made after the checks, they cannot fail
  bool need_p128 = false;
  for (size_t i = 0; i < in->cols.size(); i++) {
    const DColumn &c = in->cols[i];
    const int dt = dtype_of(c);
    if (dt < 0 || dt == TFGPU_T_ANY) continue;
    DColumn &d = r->cols[i];
    d.dtype = dt;
    StrictOut oc{};
    const int strict = strict_describe(dt, oc);
    if (strict == TFGPU_R_INVALID) return tf::fail(TFGPU_ERR_CONFIG, "tfgpu_strictify: cannot strictify value of unknown type (column " + c.name + ")");
    if (c.repr == strict) continue;  // already the strict Go type
    const bool text = c.repr == TFGPU_R_STRING || c.repr == TFGPU_R_JSONNUM;
    const bool ints = (c.repr >= TFGPU_R_INT8 && c.repr <= TFGPU_R_UINT64) || c.repr == TFGPU_R_BOOL;
    auto unsupported = [&]() { return tf::fail(TFGPU_ERR_UNSUPPORTED, "tfgpu_strictify: column " + c.name + ": a " + std::string(type_name(dt)) + " column holding Go values of representation " + std::to_string(c.repr) + " is converted on the host (cast." "To…E of that kind is not device-resident)"); };
    StrictCol s{};
    s.src_repr = c.repr; s.values = c.values ? c.values->p : nullptr; s.offsets = ptr<uint32_t>(c.offsets); s.data = ptr<uint8_t>(c.payload()); s.validity = ptr<uint8_t>(c.validity);
    if (text && (oc.kind == SK_STR)) {  // castx.ToStringE / ToByteSliceE of a string (or of a json.Number's text): the same bytes
      if (c.repr == TFGPU_R_JSONNUM && dt == TFGPU_T_BYTES) return unsupported();
      d.repr = strict;
      continue;
    }
    if (c.repr == TFGPU_R_BYTES && dt == TFGPU_T_UTF8) { d.repr = TFGPU_R_STRING; continue; }  // ToStringE([]byte) = string(b)
    if (text && oc.kind == SK_JSONNUM) { if (c.repr != TFGPU_R_STRING) continue; s.mode = SM_TEXT_JSONNUM_OUT; d.repr = TFGPU_R_JSONNUM; }
    else if (text) {
      if (c.repr == TFGPU_R_JSONNUM && oc.kind == SK_INTERVAL) return unsupported();
      s.mode = (c.repr == TFGPU_R_JSONNUM && oc.kind == SK_TIME) ? SM_JSONNUM_TO_TIME : SM_TEXT;
      if (oc.kind == SK_F32) need_p128 = true;
    } else if ((ints || c.repr == TFGPU_R_TIME || c.repr == TFGPU_R_DURATION) && dt == TFGPU_T_UTF8) {
      to_text.push_back(i);  // castx.ToStringE (caste.go:58-106): FormatInt / FormatUint / FormatBool, Time.String(), Duration.String()
      continue;
    } else if ((ints || c.repr == TFGPU_R_TIME || c.repr == TFGPU_R_DURATION || c.repr == TFGPU_R_FLOAT32 || c.repr == TFGPU_R_FLOAT64) && dt == TFGPU_T_BYTES) {
      s.mode = SM_FAIL;        // castx.ToByteSliceE (caste.go:16-28) takes []byte and string only: the first value fails the call
    } else if ((c.repr == TFGPU_R_FLOAT32 || c.repr == TFGPU_R_FLOAT64) && (dt == TFGPU_T_UTF8 || dt == TFGPU_T_FLOAT64)) {
      float_text.push_back(i);  // FormatFloat(f, 'f', -1, bits): the string, or — every such text parses (fastfloat takes "NaN" and "+Inf" too) — the json.Number
      continue;
    } else if ((c.repr == TFGPU_R_FLOAT32 || c.repr == TFGPU_R_FLOAT64) && (oc.kind == SK_INT || oc.kind == SK_UINT || oc.kind == SK_BOOL || oc.kind == SK_F32)) {
      s.mode = SM_FLOATS;
    } else if (ints) {
      if (oc.kind == SK_STR || oc.kind == SK_JSONNUM) return unsupported();                 // an integer under "double": castx.ToJSONNumberE of its text — host
      if (oc.kind == SK_INTERVAL && (c.repr >= TFGPU_R_UINT8 && c.repr <= TFGPU_R_UINT64)) return unsupported();
      if (c.repr == TFGPU_R_BOOL && (oc.kind == SK_TIME || oc.kind == SK_INTERVAL || oc.kind == SK_F32)) return unsupported();
      s.mode = SM_INTS;
    } else return unsupported();
    if (s.mode == SM_FAIL) {  // reached only when every row is nil: an all-nil []byte column
      d.values = nullptr; d.nanos = nullptr; d.view = nullptr; d.data_len = 0;
      d.offsets = dalloc_zero((size_t)(n + 1) * 4 + 16); d.data = dalloc(16);
      d.repr = strict;
    } else if (s.mode != SM_TEXT_JSONNUM_OUT) {
      d.values = dalloc((size_t)std::max<int64_t>(n, 1) * (size_t)oc.width);
      d.offsets = nullptr; d.data = nullptr; d.view = nullptr; d.data_len = 0; d.nanos = nullptr;
      if (oc.kind == SK_TIME) d.nanos = dalloc((size_t)std::max<int64_t>(n, 1) * 4);
      d.repr = strict;
      oc.values = d.values->p; oc.nanos = ptr<int32_t>(d.nanos);
    }
    s.out = oc;
    sc.push_back(s); which.push_back((int)i);
  }
  if (!sc.empty() && n > 0) {
    std::vector<GtOp> gops; std::string glits; std::vector<uint16_t> gstart;
    append_cast_layouts(gops, glits, gstart);
    Buf bgops = upload_const(gops.data(), gops.size() * sizeof(GtOp)), bglits = upload_const(glits.data(), glits.size()), bgs = upload_const(gstart.data(), gstart.size() * 2);
    const GtSet cast_tp{ptr<GtOp>(bgops), ptr<uint8_t>(bglits), ptr<uint16_t>(bgs), N_CAST_LAYOUTS};
    const uint64_t *p128 = need_p128 ? reinterpret_cast<const uint64_t *>(pow10_table() + 632) : nullptr;
    Buf bsc = upload_small(sc.data(), sc.size() * sizeof(StrictCol));
    Buf bad = dalloc(sc.size() * 8);
    TF_HIP(hipMemsetAsync(bad->p, 0xFF, sc.size() * 8, st));
    {
      KernelTimer t("strictify_cells");
      strictify_cells<<<dim3((unsigned)((n + 255) / 256), (unsigned)sc.size()), 256, 0, st>>>(cast_tp, p128, reinterpret_cast<const StrictCol *>(bsc->p), (int32_t)sc.size(), n, reinterpret_cast<unsigned long long *>(bad->p));
    }
    std::vector<uint64_t> hb(sc.size());
    d2h(hb.data(), bad->p, hb.size() * 8);
    tf::sync();
    // the first failing value in the reference's order: rows in order, a row's columns in order
    uint64_t best = ~0ull; int bcol = -1;
    for (size_t k = 0; k < hb.size(); k++) if (hb[k] != ~0ull && ((hb[k] >> 8) < (best >> 8) || best == ~0ull)) { best = hb[k]; bcol = which[k]; }
    if (bcol >= 0) {
      const int64_t row = (int64_t)(best >> 8); const int code = (int)(best & 0xFF);
      if (bad_row) *bad_row = row;
      if (bad_col) *bad_col = bcol;
      if (code == TFGPU_ROW_HOST_FALLBACK)
        return tf::fail(TFGPU_ERR_UNSUPPORTED, "tfgpu_strictify: row " + std::to_string(row) + ", column " + in->cols[(size_t)bcol].name + ": a value form the device does not decide (Go's decimal slow path, a free-form date): strictify this batch on the host");
      return tf::fail(TFGPU_ERR_INVALID, "failed to strictify the value of column [" + std::to_string(bcol) + "] \"" + in->cols[(size_t)bcol].name + "\": row " + std::to_string(row) + ": " + (code == TFGPU_ROW_RANGE ? "value is out of the type's range" : "unable to cast the value"));
    }
  }
  for (size_t i : float_text) {
    const int dt = r->cols[i].dtype;
    DColumn t = float_column_text(in->cols[i], n);
    t.name = in->cols[i].name; t.dtype = dt; t.repr = dt == TFGPU_T_FLOAT64 ? TFGPU_R_JSONNUM : TFGPU_R_STRING;
    r->cols[i] = std::move(t);
  }
  for (size_t i : to_text) {
    const int dt = r->cols[i].dtype;
    DColumn t = column_to_text(in->cols[i], n, false);
    t.name = in->cols[i].name; t.dtype = dt;
    r->cols[i] = std::move(t);
  }
  *out = r.release();
  return TFGPU_OK;
  TF_API_END
}
