// tf_devrow.hpp — what tf_mask.hip, tf_transform.hip, tf_sqleval.hip and tf_rows.hip share below their host entry points: the
// library is built without relocatable device code, so a device function two of them call lives here.
#pragma once
#include <algorithm>
#include "tf_devcol.hpp"
#include "tf_devfmt.hpp"
#include "tf_devfloat.hpp"

namespace tf {
// ============================================================================
// SerializeToString on device (to_string.go:145-178).  Formats value r of
// column c into `buf` (>= 64 bytes) unless the value is var-width text, in
// which case *ext points at the bytes in HBM.  Returns the length.
// ============================================================================
__device__ __forceinline__ int serialize_small(const DCol &c, int64_t r, uint8_t *buf, const uint8_t **ext) {
  *ext = nullptr;
  if (!is_valid(c, r)) { buf[0] = '<'; buf[1] = 'n'; buf[2] = 'i'; buf[3] = 'l'; buf[4] = '>'; return 5; }
  switch (c.repr) {
    case TFGPU_R_INT8: return dev::fmt_i64(buf, ((const int8_t *)c.values)[r]);
    case TFGPU_R_INT16: return dev::fmt_i64(buf, ((const int16_t *)c.values)[r]);
    case TFGPU_R_INT32: return dev::fmt_i64(buf, ((const int32_t *)c.values)[r]);
    case TFGPU_R_INT64: return dev::fmt_i64(buf, ((const int64_t *)c.values)[r]);
    case TFGPU_R_UINT8: return dev::fmt_u64(buf, ((const uint8_t *)c.values)[r]);
    case TFGPU_R_UINT16: return dev::fmt_u64(buf, ((const uint16_t *)c.values)[r]);
    case TFGPU_R_UINT32: return dev::fmt_u64(buf, ((const uint32_t *)c.values)[r]);
    case TFGPU_R_UINT64: return dev::fmt_u64(buf, ((const uint64_t *)c.values)[r]);
    case TFGPU_R_BOOL:
      if (((const uint8_t *)c.values)[r]) { buf[0] = 't'; buf[1] = 'r'; buf[2] = 'u'; buf[3] = 'e'; return 4; }
      buf[0] = 'f'; buf[1] = 'a'; buf[2] = 'l'; buf[3] = 's'; buf[4] = 'e'; return 5;
    case TFGPU_R_TIME: {
      int64_t s = ((const int64_t *)c.values)[r];
      int32_t ns = c.nanos ? c.nanos[r] : 0;
      if (c.dtype == TFGPU_T_DATE) return dev::fmt_date(buf, s);
      if (c.dtype == TFGPU_T_DATETIME || c.dtype == TFGPU_T_TIMESTAMP) return dev::fmt_rfc3339nano(buf, s, ns);
      return dev::fmt_time_string(buf, s, ns);
    }
    case TFGPU_R_DURATION: return dev::fmt_duration(buf, ((const int64_t *)c.values)[r]);
    // fmt.Sprintf("%v", float): %g with the shortest digits (to_string.go:170), at most 24 bytes
    case TFGPU_R_FLOAT32: { dev::StoreOut so{buf}; dev::fmt_float(so, (double)((const float *)c.values)[r], 'g', 32); return (int)so.n; }
    case TFGPU_R_FLOAT64: { dev::StoreOut so{buf}; dev::fmt_float(so, ((const double *)c.values)[r], 'g', 64); return (int)so.n; }
    case TFGPU_R_STRING: case TFGPU_R_JSONNUM: case TFGPU_R_JSON: case TFGPU_R_BYTES: {
      uint32_t a = c.offsets[r], b = c.offsets[r + 1];
      *ext = c.data + a;
      return (int)(b - a);
    }
  }
  return 0;
}
// Host-side check: can serialize_small reproduce SerializeToString for this column?
static void require_serializable(const DColumn &c, const char *what) {
  if (c.repr == TFGPU_R_BYTES && c.dtype != TFGPU_T_BYTES)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(what) + ": column " + c.name + " holds []byte under a non-\"string\" DataType (%v prints a byte list)");
  if (c.repr == TFGPU_R_STRING && c.dtype == TFGPU_T_ANY)
    throw Error(TFGPU_ERR_UNSUPPORTED, std::string(what) + ": column " + c.name + " is `any` holding Go strings (json.Marshal quoting)");
}
__device__ __forceinline__ int bytes_compare(const uint8_t *a, uint32_t an, const uint8_t *b, uint32_t bn) {
  uint32_t m = an < bn ? an : bn;
  for (uint32_t i = 0; i < m; i++) { if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1; }
  return an < bn ? -1 : an > bn ? 1 : 0;
}
}  // namespace tf
