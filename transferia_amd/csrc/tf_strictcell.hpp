// tf_strictcell.hpp — strictify.Strictify's strictifyValue of ONE string cell (pkg/abstract/changeitem/strictify/strictify.go:75-157),
// the step every text ingest and tfgpu_strictify share: cast.ToInt64E / ToUint64E plus the range limits, cast.ToTimeE over spf13/cast's
// layout list, cast.ToBoolE, ToFloat32E, ToDurationE, and castx.ToJSONNumberE's acceptance.  Where a TEXT cell is placed (lens / fstart,
// the doubled-quote bit, the column's flag word, patch) differs between the CSV views and the nginx views and stays with the caller.
// Host side: the one layout table, the one DataType -> descriptor switch, the two system columns (defined in tf_strictify.hip).
#pragma once
#include "tf_common.hpp"
#include "tf_devfmt.hpp"
#include "tf_devparse.hpp"
#include "tf_devfloat.hpp"
#include "tf_gotime.hpp"

namespace tf {

// (CsvKind of tf_csv.hip starts with these values: its tile kernels sort columns by kind)
enum StrictKind : int32_t { SK_INT = 0, SK_UINT = 1, SK_STR = 2, SK_JSONNUM = 3, SK_TIME = 4, SK_BOOL = 6, SK_F32 = 7, SK_INTERVAL = 9 };

// where a typed cell goes
struct StrictOut {
  int32_t kind;             // StrictKind
  int32_t width;            // bytes of the fixed-width output element
  int64_t lo; uint64_t hi;  // toSignedInt / toUnsignedInt limits (strictify.go:159-181)
  void *values;
  int32_t *nanos;           // time columns only
};

// spf13/cast trimZeroDecimal: "12.00" → "12"
template <class F> __device__ __forceinline__ uint32_t trim_zero_decimal(const F &f, uint32_t a, uint32_t b) {
  bool found_zero = false;
  for (uint32_t i = b; i > a; i--) {
    uint32_t c = f[i - 1];
    if (c == '.') { if (found_zero) return i - 1; }
    else if (c == '0') found_zero = true;
    else return b;
  }
  return b;
}

// cast.StringToDate (spf13/cast v1.7.1 timeFormats) for the fixed numeric shapes:
//   2006-01-02 | 2006-01-02T15:04:05[.frac][Z07:00] | 2006-01-02 15:04:05[.frac]
// returns 0 ok, TFGPU_ROW_CAST if the shape is one of these but the value is
// invalid, TFGPU_ROW_HOST_FALLBACK if the text has another shape.
template <class F> __device__ int parse_datetime(const F &f, uint32_t a, uint32_t b, int64_t *sec, int32_t *nsec) {
  uint32_t n = b - a;
  if (n < 10) return TFGPU_ROW_HOST_FALLBACK;
  for (int i = 0; i < 10; i++) {
    uint32_t c = f[a + i];
    if (i == 4 || i == 7) { if (c != '-') return TFGPU_ROW_HOST_FALLBACK; } else if (!dg(c)) return TFGPU_ROW_HOST_FALLBACK;
  }
  int64_t y = (f[a] - '0') * 1000 + (f[a + 1] - '0') * 100 + (f[a + 2] - '0') * 10 + (f[a + 3] - '0');
  int mo = (f[a + 5] - '0') * 10 + (f[a + 6] - '0'), d = (f[a + 8] - '0') * 10 + (f[a + 9] - '0');
  int h = 0, mi = 0, se = 0; int64_t ns = 0; int off = 0;
  if (n > 10) {
    uint32_t sep = f[a + 10];
    if (sep != 'T' && sep != ' ') return TFGPU_ROW_HOST_FALLBACK;
    uint32_t k = a + 11;
    // stdHour "15" takes one or two digits; minutes/seconds are fixed two digits
    if (k >= b || !dg(f[k])) return TFGPU_ROW_HOST_FALLBACK;
    h = f[k] - '0'; k++;
    if (k < b && dg(f[k])) { h = h * 10 + (f[k] - '0'); k++; }
    if (k + 6 > b || f[k] != ':' || !dg(f[k + 1]) || !dg(f[k + 2]) || f[k + 3] != ':' || !dg(f[k + 4]) || !dg(f[k + 5])) return TFGPU_ROW_HOST_FALLBACK;
    mi = (f[k + 1] - '0') * 10 + (f[k + 2] - '0'); se = (f[k + 4] - '0') * 10 + (f[k + 5] - '0');
    k += 6;
    if (k + 1 < b && (f[k] == '.' || f[k] == ',') && dg(f[k + 1])) {
      k++; int nd = 0;
      while (k < b && dg(f[k])) { if (nd < 9) { ns = ns * 10 + (f[k] - '0'); nd++; } k++; }
      while (nd < 9) { ns *= 10; nd++; }
    }
    if (k < b) {
      if (sep != 'T') return TFGPU_ROW_HOST_FALLBACK;  // "… 15:04:05 -0700", "…Z07:00" after a space: the layout list
      if (f[k] == 'Z' && k + 1 == b) k++;
      else if ((f[k] == '+' || f[k] == '-') && k + 6 == b && dg(f[k + 1]) && dg(f[k + 2]) && f[k + 3] == ':' && dg(f[k + 4]) && dg(f[k + 5])) {
        int hh = (f[k + 1] - '0') * 10 + (f[k + 2] - '0'), mm = (f[k + 4] - '0') * 10 + (f[k + 5] - '0');
        if (hh > 24 || mm > 60) return TFGPU_ROW_CAST;
        off = (f[k] == '-' ? -1 : 1) * (hh * 3600 + mm * 60);
        k += 6;
      } else return TFGPU_ROW_HOST_FALLBACK;
    }
  }
  if (mo < 1 || mo > 12 || d < 1 || d > dev::days_in_month(mo, y) || h > 23 || mi > 59 || se > 59) return TFGPU_ROW_CAST;
  *sec = dev::days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + se - off;
  *nsec = (int32_t)ns;
  return 0;
}

// castx.ToJSONNumberE acceptance (fastfloat.Parse grammar or ParseInt base 10)
template <class F> __device__ bool json_number_ok(const F &f, uint32_t a, uint32_t b) {
  if (a >= b) return false;
  uint32_t p = a;
  if (f[p] == '-' || f[p] == '+') p++;
  uint32_t d0 = p; while (p < b && dg(f[p])) p++;
  uint32_t nd = p - d0; bool ok = true;
  if (p < b && f[p] == '.') { p++; uint32_t f0 = p; while (p < b && dg(f[p])) p++; if (p == f0) nd = 0; else nd += p - f0; }
  if (nd > 0 && p < b && (f[p] == 'e' || f[p] == 'E')) { p++; if (p < b && (f[p] == '-' || f[p] == '+')) p++; uint32_t x0 = p; while (p < b && dg(f[p])) p++; if (p == x0) ok = false; }
  if (ok && nd > 0 && p == b) return true;
  // inf / infinity / nan, case-insensitive
  uint32_t q = a; if (f[q] == '-' || f[q] == '+') q++;
  uint32_t n = b - q;
  auto ci = [&](const char *s, uint32_t sl) { if (n != sl) return false; for (uint32_t i = 0; i < sl; i++) if (lower_(f[q + i]) != (uint32_t)s[i]) return false; return true; };
  return ci("inf", 3) || ci("infinity", 8) || ci("nan", 3);
}

__device__ __forceinline__ void store_int(const StrictOut &c, int64_t r, int64_t v) {
  switch (c.width) {
    case 1: ((int8_t *)c.values)[r] = (int8_t)v; break;
    case 2: ((int16_t *)c.values)[r] = (int16_t)v; break;
    case 4: ((int32_t *)c.values)[r] = (int32_t)v; break;
    default: ((int64_t *)c.values)[r] = v;
  }
}

// DefaultValue(col) (pkg/abstract/change_item_builders.go:88-109) after Strictify, for the typed kinds; also what a nil cell's slot holds
__device__ __forceinline__ void store_default(const StrictOut &c, int64_t r) {
  switch (c.kind) {
    case SK_TIME: ((int64_t *)c.values)[r] = 0; if (c.nanos) c.nanos[r] = 0; break;
    case SK_BOOL: ((uint8_t *)c.values)[r] = 0; break;
    case SK_F32: ((float *)c.values)[r] = 0.f; break;
    default: store_int(c, r, 0);
  }
}

// strictifyValue of the string fv[a, b) under a typed column, into row r.  `cast_tp` = the compiled cast layouts (append_cast_layouts),
// `p128` = Eisel-Lemire's 128-bit powers of ten (needed by float32 columns only).  Returns tfgpu_rowerr.
template <class F> __device__ int strict_cell(const StrictOut &c, const GtSet &cast_tp, const uint64_t *p128, int64_t r, const F &fv, uint32_t a, uint32_t b) {
  switch (c.kind) {
    case SK_INT: case SK_UINT: {  // cast.ToInt64E / ToUint64E (string) + range check
      uint32_t tb = trim_zero_decimal(fv, a, b);
      if (c.kind == SK_INT || c.hi != ~0ull) {
        int64_t v; int rc = parse_int64(fv, a, tb, true, &v);
        if (rc) return TFGPU_ROW_CAST;
        if (c.kind == SK_UINT) {
          if (v < 0) return TFGPU_ROW_CAST;  // errNegativeNotAllowed
          if ((uint64_t)v > c.hi) return TFGPU_ROW_RANGE;
        } else if (v < c.lo || v > (int64_t)c.hi) return TFGPU_ROW_RANGE;
        store_int(c, r, v);
      } else {  // uint64: cast.ToUint64E parses with ParseUint
        uint64_t v; int rc = parse_uint64(fv, a, tb, true, &v);
        if (rc) return TFGPU_ROW_CAST;
        ((uint64_t *)c.values)[r] = v;
      }
      return 0;
    }
    case SK_TIME: {  // cast.ToTimeE → StringToDate, the first of its layouts that parses (strictify.go:118-143)
      int64_t sec = 0; int32_t ns = 0;
      if (parse_datetime(fv, a, b, &sec, &ns)) { ns = 0; if (!gotime_parse_any(cast_tp, fv, a, b, &sec, &ns)) return TFGPU_ROW_CAST; }
      ((int64_t *)c.values)[r] = sec;
      c.nanos[r] = ns;
      return 0;
    }
    case SK_BOOL: {  // cast.ToBoolE
      int v = 0;
      if (parse_bool(fv, a, b, &v)) return TFGPU_ROW_CAST;
      ((uint8_t *)c.values)[r] = (uint8_t)v;
      return 0;
    }
    case SK_F32: {  // cast.ToFloat32E(string) = strconv.ParseFloat(s, 32), any error fails the row
      float v = 0;
      const int rc = parse_float32_go(fv, a, b, p128, &v);
      if (rc == 3) return TFGPU_ROW_HOST_FALLBACK;  // Go's decimal slow path (half-way cases, subnormals, the overflow edge), hex floats, '_'
      if (rc) return TFGPU_ROW_CAST;                // syntax or range: ToFloat32E returns the error
      ((float *)c.values)[r] = v;
      return 0;
    }
    case SK_INTERVAL: {  // cast.ToDurationE(string) (strictify.go:142-147)
      int64_t d;
      if (parse_duration_go(fv, a, b, &d)) return TFGPU_ROW_CAST;
      ((int64_t *)c.values)[r] = d;
      return 0;
    }
    default:  // text is placed by the caller
      return TFGPU_ROW_HOST_FALLBACK;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// spf13/cast v1.7.1 StringToDate's list (caste.go timeFormats) in its order
inline constexpr const char *CAST_LAYOUTS[] = {
    "2006-01-02", "2006-01-02T15:04:05Z07:00", "2006-01-02T15:04:05", "Mon, 02 Jan 2006 15:04:05 -0700", "Mon, 02 Jan 2006 15:04:05 MST",
    "02 Jan 06 15:04 -0700", "02 Jan 06 15:04 MST", "Monday, 02-Jan-06 15:04:05 MST", "2006-01-02 15:04:05.999999999 -0700 MST",
    "2006-01-02T15:04:05-0700", "2006-01-02 15:04:05Z0700", "2006-01-02 15:04:05", "Mon Jan _2 15:04:05 2006", "Mon Jan _2 15:04:05 MST 2006",
    "Mon Jan 02 15:04:05 -0700 2006", "2006-01-02 15:04:05Z07:00", "02 Jan 2006", "2006-01-02 15:04:05 -07:00", "2006-01-02 15:04:05 -0700",
    "3:04PM", "Jan _2 15:04:05", "Jan _2 15:04:05.000", "Jan _2 15:04:05.000000", "Jan _2 15:04:05.000000000"};
inline constexpr int32_t N_CAST_LAYOUTS = (int32_t)(sizeof CAST_LAYOUTS / sizeof *CAST_LAYOUTS);
// compiles them behind whatever `gops` / `glits` already hold; `start` gets the N_CAST_LAYOUTS + 1 op positions a GtSet of them points at
inline void append_cast_layouts(std::vector<GtOp> &gops, std::string &glits, std::vector<uint16_t> &start) {
  start.push_back((uint16_t)gops.size());
  for (const char *l : CAST_LAYOUTS) { gotime_compile(l, gops, glits); start.push_back((uint16_t)gops.size()); }
}

// The strict Go type of a DataType: fills kind / width / lo / hi of `c` and returns its TFGPU_R_*, or TFGPU_R_INVALID for a DataType
// strictifyValue does not know.  date / datetime / timestamp are all SK_TIME and `any` is text here: callers with a reader step of
// their own in front (CSV's parseTimestampValue, nginx's timeLocalLayout) or that leave `any` alone (tfgpu_strictify) say so themselves.
inline int strict_describe(int dtype, StrictOut &c) {
  auto set = [&](int kind, int width, int64_t lo, uint64_t hi, int repr) { c.kind = kind; c.width = width; c.lo = lo; c.hi = hi; return repr; };
  switch (dtype) {
    case TFGPU_T_INT8: return set(SK_INT, 1, INT8_MIN, INT8_MAX, TFGPU_R_INT8);
    case TFGPU_T_INT16: return set(SK_INT, 2, INT16_MIN, INT16_MAX, TFGPU_R_INT16);
    case TFGPU_T_INT32: return set(SK_INT, 4, INT32_MIN, INT32_MAX, TFGPU_R_INT32);
    case TFGPU_T_INT64: return set(SK_INT, 8, INT64_MIN, INT64_MAX, TFGPU_R_INT64);
    case TFGPU_T_UINT8: return set(SK_UINT, 1, 0, UINT8_MAX, TFGPU_R_UINT8);
    case TFGPU_T_UINT16: return set(SK_UINT, 2, 0, UINT16_MAX, TFGPU_R_UINT16);
    case TFGPU_T_UINT32: return set(SK_UINT, 4, 0, UINT32_MAX, TFGPU_R_UINT32);
    case TFGPU_T_UINT64: return set(SK_UINT, 8, 0, ~0ull, TFGPU_R_UINT64);
    case TFGPU_T_BOOLEAN: return set(SK_BOOL, 1, 0, 0, TFGPU_R_BOOL);
    case TFGPU_T_DATE: case TFGPU_T_DATETIME: case TFGPU_T_TIMESTAMP: return set(SK_TIME, 8, 0, 0, TFGPU_R_TIME);
    case TFGPU_T_FLOAT32: return set(SK_F32, 4, 0, 0, TFGPU_R_FLOAT32);
    case TFGPU_T_FLOAT64: return set(SK_JSONNUM, 0, 0, 0, TFGPU_R_JSONNUM);  // float64 → json.Number text
    case TFGPU_T_UTF8: case TFGPU_T_ANY: return set(SK_STR, 0, 0, 0, TFGPU_R_STRING);
    case TFGPU_T_BYTES: return set(SK_STR, 0, 0, 0, TFGPU_R_BYTES);
    case TFGPU_T_INTERVAL: return set(SK_INTERVAL, 8, 0, 0, TFGPU_R_DURATION);
    default: return TFGPU_R_INVALID;
  }
}

// constructCI's system columns (reader_csv.go:275-290, reader_nginx.go:227-238): fills `d` (whose repr says which of the two it is:
// TFGPU_R_STRING = __file_name, else __row_index = row_number_base + rank[r], or + r without `rank`) on the lane's stream; with
// `hide` (config.hideSystemCols) every cell is nil.  Returns TFGPU_OK, or an error code with `detail` to put behind the caller's prefix.
int fill_system_column(DColumn &d, int64_t nrows, const char *file_name, uint64_t row_number_base, const uint32_t *rank, bool hide, std::string *detail);  // tf_strictify.hip

}  // namespace tf
