// tf_nginx.hip — nginx access-log ingest (s3 reader registry "nginx", pkg/providers/s3/reader/registry/nginx): the log_format
// compiler and the schema resolver (host, no GPU), and the device front of tfgpu_nginx_parse: which lines are blank, every other
// line's lineCounter, the token walk (parseEntry) — one lane per line, the lines staged in LDS by the whole wave — and the cells:
// convertNginxValue, constructCI and strictify.Strictify over the cut fields, the system columns, the compaction, the error list.
// The text -> typed conversion is strict_cell (tf_strictcell.hpp), the one the CSV ingest and tfgpu_strictify run.
#include <algorithm>
#include <map>

#include "tf_common.hpp"
#include "tf_rows.hpp"
#include "tf_devfmt.hpp"
#include "tf_devparse.hpp"
#include "tf_devfloat.hpp"
#include "tf_f64range.hpp"
#include "tf_gotime.hpp"
#include "tf_strictcell.hpp"
#include "tf_textview.hpp"

using namespace tf;

// ---- the compiled format (host) ---------------------------------------------------------------------------------------------
struct NginxToken { bool is_variable; std::string value; };
struct tfgpu_nginx_format {
  std::vector<NginxToken> tokens;
  std::vector<std::string> fields;  // unique column names, one per variable
};

namespace {

// unicode.IsSpace at s[i, n): bytes of the white-space rune there, 0 if none ('\t' '\n' '\v' '\f' '\r' ' ' U+0085 U+00A0 U+1680
// U+2000-200A U+2028 U+2029 U+202F U+205F U+3000)
size_t host_space_at(const std::string &s, size_t i) {
  const size_t n = s.size();
  const unsigned c = (unsigned char)s[i];
  if (c == ' ' || (c >= 9 && c <= 13)) return 1;
  if (c == 0xC2 && i + 1 < n) { const unsigned d = (unsigned char)s[i + 1]; return (d == 0x85 || d == 0xA0) ? 2 : 0; }
  if (i + 2 < n && (c == 0xE1 || c == 0xE2 || c == 0xE3)) {
    const unsigned d = (unsigned char)s[i + 1], e = (unsigned char)s[i + 2];
    if (c == 0xE1) return (d == 0x9A && e == 0x80) ? 3 : 0;
    if (c == 0xE3) return (d == 0x80 && e == 0x80) ? 3 : 0;
    if (d == 0x80 && ((e >= 0x80 && e <= 0x8A) || e == 0xA8 || e == 0xA9 || e == 0xAF)) return 3;
    if (d == 0x81 && e == 0x9F) return 3;
  }
  return 0;
}
std::string host_trim_space(const std::string &s) {  // strings.TrimSpace
  size_t a = 0, b = s.size(), k;
  while (a < b && (k = host_space_at(s, a)) > 0 && a + k <= b) a += k;
  for (bool cut = true; cut && b > a;) {
    cut = false;
    for (size_t w = 1; w <= 3 && w <= b - a; w++)
      if (host_space_at(s.substr(0, b), b - w) == w) { b -= w; cut = true; break; }
  }
  return s.substr(a, b - a);
}
bool var_char(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_'; }

// tokenizeFormat (nginx_format.go:35-52)
std::vector<NginxToken> tokenize_format(const std::string &format) {
  const std::string t = host_trim_space(format);
  // multilineCollapseRegexp `[ \t]*\n[ \t]*` -> " ": the blanks on both sides of every '\n' go with it
  std::string f;
  size_t floor = 0;  // what earlier matches produced is not taken back
  for (size_t i = 0; i < t.size();) {
    if (t[i] != '\n') { f += t[i++]; continue; }
    while (f.size() > floor && (f.back() == ' ' || f.back() == '\t')) f.pop_back();
    f += ' ';
    floor = f.size();
    i++;
    while (i < t.size() && (t[i] == ' ' || t[i] == '\t')) i++;
  }
  // nginxVarRegexp `\$([A-Za-z0-9_]+)`
  std::vector<NginxToken> tokens;
  size_t last = 0;
  for (size_t i = 0; i < f.size();) {
    if (f[i] != '$' || i + 1 >= f.size() || !var_char(f[i + 1])) { i++; continue; }
    size_t e = i + 1;
    while (e < f.size() && var_char(f[e])) e++;
    if (i > last) tokens.push_back({false, f.substr(last, i - last)});
    tokens.push_back({true, f.substr(i + 1, e - i - 1)});
    last = e; i = e;
  }
  if (last < f.size()) tokens.push_back({false, f.substr(last)});
  return tokens;
}

char *dup_c(const std::string &s) {
  char *r = (char *)std::malloc(s.size() + 1);
  if (!r) throw std::bad_alloc();
  std::memcpy(r, s.c_str(), s.size() + 1);
  return r;
}
const char *dtype_name(int dtype) {  // ytschema type names (ColSchema.DataType)
  static const char *const N[] = {"", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float", "double", "boolean", "string", "utf8", "date", "datetime",
                                  "timestamp", "interval", "any"};
  return dtype > 0 && dtype < TFGPU_T__COUNT ? N[dtype] : "";
}

}  // namespace

extern "C" int tfgpu_nginx_format_compile(const char *log_format, tfgpu_nginx_format **out) {  // compileFormat (nginx_format.go:55-95)
  TF_API_BEGIN
  if (!log_format || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_nginx_format_compile: null argument");
  auto f = std::make_unique<tfgpu_nginx_format>();
  f->tokens = tokenize_format(log_format);
  if (f->tokens.empty()) return tf::fail(TFGPU_ERR_CONFIG, std::string("nginx: No tokens found in format, err: ") + log_format);
  std::map<std::string, int> used;
  for (auto &t : f->tokens) {
    if (!t.is_variable) continue;
    const int k = ++used[t.value];  // makeUniqueColumnName
    f->fields.push_back(k == 1 ? t.value : t.value + "_" + std::to_string(k));
  }
  if (f->fields.empty()) return tf::fail(TFGPU_ERR_CONFIG, std::string("nginx: No variable found in format, err: ") + log_format);
  *out = f.release();
  return TFGPU_OK;
  TF_API_END
}
extern "C" void tfgpu_nginx_format_free(tfgpu_nginx_format *f) { delete f; }
extern "C" int tfgpu_nginx_format_ntokens(const tfgpu_nginx_format *f) { return f ? (int)f->tokens.size() : 0; }
extern "C" int tfgpu_nginx_format_token(const tfgpu_nginx_format *f, int i, int *is_variable, const char **value) {
  if (!f || i < 0 || i >= (int)f->tokens.size()) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_nginx_format_token: no such token");
  if (is_variable) *is_variable = f->tokens[(size_t)i].is_variable ? 1 : 0;
  if (value) *value = f->tokens[(size_t)i].value.c_str();
  return TFGPU_OK;
}
extern "C" int tfgpu_nginx_format_nfields(const tfgpu_nginx_format *f) { return f ? (int)f->fields.size() : 0; }
extern "C" const char *tfgpu_nginx_format_field(const tfgpu_nginx_format *f, int i) {
  return (f && i >= 0 && i < (int)f->fields.size()) ? f->fields[(size_t)i].c_str() : nullptr;
}

// NewNginxSchemaResolver (nginx_schema_resolver.go:52-101)
extern "C" int tfgpu_nginx_resolve_schema(const tfgpu_nginx_format *f, const tfgpu_schema *output_schema, int hide_system_cols, tfgpu_schema **out) {
  TF_API_BEGIN
  if (!f || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_nginx_resolve_schema: null argument");
  struct Col { std::string name, path, orig, tschema, tname, expr; bool has_props = false; std::string props; int dtype; uint32_t flags; };
  std::vector<Col> cols;
  if (!output_schema || output_schema->ncols == 0) {
    // (ytschema.TypeString is the type "utf8": the OriginalType compileFormat formats is "nginx:utf8")
    for (size_t i = 0; i < f->fields.size(); i++) { Col c{}; c.name = f->fields[i]; c.path = std::to_string(i); c.orig = "nginx:utf8"; c.dtype = TFGPU_T_UTF8; c.flags = 0; cols.push_back(c); }
  } else {
    for (int i = 0; i < output_schema->ncols; i++) {
      const tfgpu_colschema &s = output_schema->cols[i];
      Col c{};
      c.name = s.name ? s.name : ""; c.path = s.path ? s.path : ""; c.orig = s.original_type ? s.original_type : "";
      c.tschema = s.table_schema ? s.table_schema : ""; c.tname = s.table_name ? s.table_name : ""; c.expr = s.expression ? s.expression : "";
      if (s.properties_json) { c.has_props = true; c.props = s.properties_json; }
      c.dtype = s.dtype; c.flags = s.flags;
      if (c.path.empty()) {
        size_t idx = f->fields.size();
        for (size_t k = 0; k < f->fields.size(); k++) if (f->fields[k] == c.name) { idx = k; break; }
        if (idx == f->fields.size()) continue;  // no field of that name: the column is dropped
        c.path = std::to_string(idx);
      }
      if (c.orig.empty()) c.orig = std::string("nginx:") + dtype_name(c.dtype);
      cols.push_back(c);
    }
  }
  bool has_key = false;
  for (auto &c : cols) has_key |= (c.flags & TFGPU_COL_KEY) != 0;
  const int nsys = hide_system_cols ? 0 : 2;
  auto *s = (tfgpu_schema *)std::calloc(1, sizeof(tfgpu_schema));
  if (!s) throw std::bad_alloc();
  s->cols = (tfgpu_colschema *)std::calloc(std::max<size_t>(cols.size() + (size_t)nsys, 1), sizeof(tfgpu_colschema));
  if (!s->cols) { std::free(s); throw std::bad_alloc(); }
  if (nsys) {  // s3_reader.AppendSystemColsTableSchema (util.go:210-215): in front, keys when the schema has none
    const uint32_t kf = has_key ? 0u : (uint32_t)TFGPU_COL_KEY;
    s->cols[0].name = dup_c("__file_name"); s->cols[0].dtype = TFGPU_T_UTF8; s->cols[0].flags = kf;
    s->cols[1].name = dup_c("__row_index"); s->cols[1].dtype = TFGPU_T_UINT64; s->cols[1].flags = kf;
    s->ncols = 2;
  }
  for (auto &c : cols) {
    tfgpu_colschema &o = s->cols[s->ncols++];
    o.name = dup_c(c.name); o.dtype = c.dtype; o.flags = c.flags; o.path = dup_c(c.path); o.original_type = dup_c(c.orig);
    o.table_schema = dup_c(c.tschema); o.table_name = dup_c(c.tname); o.expression = dup_c(c.expr);
    o.properties_json = c.has_props ? dup_c(c.props) : nullptr;
  }
  *out = s;
  return TFGPU_OK;
  TF_API_END
}

extern "C" void tfgpu_nginx_options_default(tfgpu_nginx_options *o) {
  std::memset(o, 0, sizeof *o);
  o->row_number_base = 1;  // reader_nginx.go: lineCounter starts at 1
}

// ---- device ---------------------------------------------------------------------------------------------------------------
namespace tf {

uint32_t newline_starts(const uint8_t *data, uint64_t len, Buf *out);           // tf_csv.hip
const double *pow10_table();                                                     // tf_json.hip
static constexpr uint8_t NG_BLANK = 0xFF;  // status of a line the reader skips (strings.TrimSpace(line) == ""): no row, no lineCounter

struct NgWalked {
  const uint8_t *data = nullptr;  // the chunk in HBM, 16-byte aligned, zero-padded past len
  uint64_t len = 0;
  Buf src;                        // the library-owned block that holds it: the text columns keep it alive
  int64_t nlines = 0;             // lines of the chunk, blank ones included: the rows before compaction
  Buf status;                     // u8[nlines]: 0, TFGPU_ROW_NGINX_FORMAT, TFGPU_ROW_NGINX_EXTRA or NG_BLANK
  Buf rank;                       // u32[nlines + 1]: non-blank lines in front of line i (lineCounter - row_number_base); [nlines] = their number
  const uint32_t *last_end = nullptr;  // device word: one past the chunk's last '\n'
  Buf fpos, flen;                 // u32[slot][stride]: where a stored field starts in the chunk, and its length
  int64_t stride = 0;
  std::vector<int32_t> col_slot;  // per schema column: its field's slot, -1 = the index is outside the fields (DefaultValue), -2 = system column
};

static constexpr int NG_TILE = 16 * 1024;  // bytes of lines one wave stages in LDS at a time; a longer line is walked from HBM
static constexpr int NG_LINES = 64;        // lines per workgroup (one wave: lane = line)
static constexpr int NG_MAXTOK = 192;      // tokens of a format the kernel arguments hold
static constexpr int NG_POOL = 1024;       // bytes of all its literals

struct NgTok { uint16_t off, len;    // literal: its bytes in the pool
               uint16_t doff, dlen;  // variable: the next non-empty literal (its delimiter); dlen 0 = runs to '\n' / '\r' / the end of the line
               int16_t slot;         // variable: where its position is stored, -1 = no column reads it
               uint8_t var, pad; };
struct NgProg { int32_t ntok; NgTok tok[NG_MAXTOK]; uint8_t pool[NG_POOL]; };
struct NgParams {
  const uint8_t *data; uint64_t len;
  const uint32_t *row_start;  // [nl + 1]
  const uint32_t *line_end;   // [nlines]: end of the line without its '\n' and trailing '\r's
  uint8_t *status;            // [nlines]: NG_BLANK on entry for blank lines
  int64_t nlines;
  uint32_t *fpos, *flen; int64_t stride;
  int32_t extra_err;          // NginxUnexpectedFieldBehaviorError
  NgProg prog;                // wave-uniform: read through scalar loads from the kernel arguments
};

// unicode.IsSpace at in[i, n): bytes of the white-space rune there, 0 if none
template <class B> __device__ __forceinline__ uint32_t ng_space_at(const B &in, uint32_t i, uint32_t n) {
  const uint32_t c = in[i];
  if (c == ' ' || (c >= 9 && c <= 13)) return 1;
  if (c < 0xC2) return 0;
  const uint32_t r = n - i;
  if (c == 0xC2 && r >= 2) { const uint32_t d = in[i + 1]; return (d == 0x85 || d == 0xA0) ? 2 : 0; }
  if (r >= 3 && (c == 0xE1 || c == 0xE2 || c == 0xE3)) {
    const uint32_t d = in[i + 1], e = in[i + 2];
    if (c == 0xE1) return (d == 0x9A && e == 0x80) ? 3 : 0;
    if (c == 0xE3) return (d == 0x80 && e == 0x80) ? 3 : 0;
    if (d == 0x80 && ((e >= 0x80 && e <= 0x8A) || e == 0xA8 || e == 0xA9 || e == 0xAF)) return 3;
    if (d == 0x81 && e == 0x9F) return 3;
  }
  return 0;
}
template <class B> __device__ __forceinline__ bool ng_all_space(const B &in, uint32_t a, uint32_t n) {
  while (a < n) { const uint32_t k = ng_space_at(in, a, n); if (!k) return false; a += k; }
  return true;
}
struct NgBytes {  // a line's bytes, in LDS or in HBM
  const uint8_t *b;
  __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return b[i]; }
};

// reader_nginx.go:121-125: lines are cut at '\n', lose their trailing '\r's, and are skipped when nothing but white space is left
__global__ void __launch_bounds__(256) nginx_line_flags(const uint8_t *__restrict__ data, uint64_t len, const uint32_t *__restrict__ row_start, int64_t nl, int64_t nlines,
                                                        uint32_t *__restrict__ line_end, uint8_t *__restrict__ status, uint32_t *__restrict__ nonblank) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nlines) return;
  const uint32_t s = row_start[r];
  uint32_t e = r < nl ? row_start[r + 1] - 1u : (uint32_t)len;  // (the line behind the last '\n' exists on the last round only)
  while (e > s && data[e - 1] == '\r') e--;
  const NgBytes in{data + s};
  const bool blank = ng_all_space(in, 0, e - s);
  line_end[r] = e;
  status[r] = blank ? NG_BLANK : 0;
  nonblank[r] = blank ? 0u : 1u;
}

// matchLiteral (nginx_format.go:154-176): bytes of in[pos, n) the literal takes, -1 on a mismatch.  A space of the format is one
// or more spaces / tabs of the line.
template <class B> __device__ __forceinline__ int ng_match(const B &in, uint32_t pos, uint32_t n, const uint8_t *lit, uint32_t ll) {
  uint32_t p = pos;
  for (uint32_t i = 0; i < ll; i++) {
    if (p >= n) return -1;
    const uint32_t lch = lit[i];
    uint32_t c = in[p];
    if (lch == ' ') {
      if (c != ' ' && c != '\t') return -1;
      p++;
      while (p < n && ((c = in[p]) == ' ' || c == '\t')) p++;
    } else {
      if (c != lch) return -1;
      p++;
    }
  }
  return (int)(p - pos);
}
// findDelimiter (:180-194): a backslash hides the byte behind it (but not a line feed)
template <class B> __device__ __forceinline__ int ng_find(const B &in, uint32_t pos, uint32_t n, const uint8_t *d, uint32_t dl) {
  for (uint32_t i = pos; i < n; i++) {
    if (in[i] == '\\') {
      const bool is_nl = i + 1 < n && in[i + 1] == '\n';
      if (!is_nl) { i++; continue; }
    }
    if (ng_match(in, i, n, d, dl) >= 0) return (int)(i - pos);
  }
  return -1;
}
// parseEntry (:99-138) + checkUnexpectedFields over one line in[0, n) that starts at chunk offset `abs0`; every lane of the wave
// calls it (idle ones with on = false): the token loop is the wave's, only where a field ends differs by lane
template <class B> __device__ __forceinline__ void ng_walk(const NgParams &p, const B &in, uint32_t n, uint32_t abs0, int64_t r, bool on) {
  uint32_t pos = 0; int st = 0;
  bool alive = on;
  const int ntok = p.prog.ntok;
  for (int t = 0; t < ntok; t++) {
    if (!__any(alive)) break;
    const NgTok &k = p.prog.tok[t];
    if (!alive) continue;
    if (!k.var) {
      const int m = ng_match(in, pos, n, p.prog.pool + k.off, k.len);
      if (m < 0) { st = TFGPU_ROW_NGINX_FORMAT; alive = false; } else pos += (uint32_t)m;
      continue;
    }
    uint32_t end = n - pos;
    if (k.dlen == 0) {  // indexOfNewline: the last variable runs to the first '\n' or '\r'
      for (uint32_t i = pos; i < n; i++) { const uint32_t c = in[i]; if (c == '\n' || c == '\r') { end = i - pos; break; } }
    } else {
      const int e = ng_find(in, pos, n, p.prog.pool + k.doff, k.dlen);
      if (e < 0) { st = TFGPU_ROW_NGINX_FORMAT; alive = false; continue; }
      end = (uint32_t)e;
    }
    if (k.slot >= 0) { p.fpos[(int64_t)k.slot * p.stride + r] = abs0 + pos; p.flen[(int64_t)k.slot * p.stride + r] = end; }
    pos += end;
  }
  if (!on) return;
  if (!st && p.extra_err && pos < n && !ng_all_space(in, pos, n)) st = TFGPU_ROW_NGINX_EXTRA;
  p.status[r] = (uint8_t)st;
}

// One wave per NG_LINES consecutive lines.  The wave stages NG_TILE bytes from the start of its first unwalked line with
// 16-byte loads; every lane whose line lies inside walks it out of LDS; the tile then moves on to the next unwalked line.  A line
// that cannot fit a tile is walked by its lane straight from HBM — same code, other byte source.
__global__ void __launch_bounds__(NG_LINES) nginx_parse_lines(NgParams p) {
  __shared__ uint4 tile[NG_TILE / 16];
  const int lane = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * NG_LINES + lane;
  const bool have = r < p.nlines;
  const uint32_t s = have ? p.row_start[r] : 0u, e = have ? p.line_end[r] : 0u;
  bool todo = have && p.status[r] != NG_BLANK;
  const bool lng = todo && (e - s) > (uint32_t)(NG_TILE - 16);
  if (__any(lng)) {
    const NgBytes in{p.data + s};
    ng_walk(p, in, e - s, s, r, lng);
    if (lng) todo = false;
  }
  for (;;) {
    const unsigned long long pending = __ballot(todo);
    if (!pending) break;
    const int first = __ffsll((long long)pending) - 1;
    const uint32_t t0 = (uint32_t)__shfl((int)s, first, 64) & ~15u;
    for (int i = lane; i < NG_TILE / 16; i += NG_LINES) {
      const uint64_t at = (uint64_t)t0 + (uint64_t)i * 16;
      tile[i] = at < p.len ? *reinterpret_cast<const uint4 *>(p.data + at) : make_uint4(0, 0, 0, 0);  // (the buffer is padded past len)
    }
    __syncthreads();
    const bool now = todo && (uint64_t)e <= (uint64_t)t0 + NG_TILE;  // lines ascend: the first pending one always fits
    const NgBytes in{reinterpret_cast<const uint8_t *>(tile) + (now ? s - t0 : 0u)};
    ng_walk(p, in, now ? e - s : 0u, s, r, now);
    if (now) todo = false;
    __syncthreads();
  }
}


// ---- cells: convertNginxValue, constructCI (reader_nginx_funcs.go:32-47, reader_nginx.go:217-279), strictify.Strictify --------
enum NgMode : int32_t { NGM_STRICT = 0 /* the string through Strictify */, NGM_LAYOUT = 1 /* date / datetime: time.Parse(timeLocalLayout) */,
                        NGM_DEFAULT = 2 /* the index is outside the fields: abstract.DefaultValue */ };
struct NgCol {
  StrictOut out;               // kind, width, limits, values, nanos
  int32_t slot, mode;
  int32_t schema_col, pad;     // the column's index in the schema: what a row error names
  uint32_t *lens, *fstart;     // text: content length (Arrow offsets after the scan) and where the cell sits in the chunk (tf_textview.hpp)
  unsigned long long *valid;   // bit r = the cell is not nil
};

// abstract.DefaultValue (change_item_builders.go:88-109) after Strictify; also what a nil cell's slot holds
__device__ __forceinline__ void ng_store_default(const NgCol &c, int64_t r, bool nil) {
  switch (c.out.kind) {
    case SK_STR: c.lens[r] = 0; c.fstart[r] = nil ? 0u : 0x7FFFFFFFu; break;
    case SK_JSONNUM: c.lens[r] = nil ? 0u : 1u; c.fstart[r] = nil ? 0u : 0x7FFFFFFFu; break;  // float64(0) is json.Number("0"): a cell that is no byte range
    default: store_default(c.out, r);
  }
}

// blockIdx.y = column (a scalar), lane = line.  errkey[r] = min over failing columns of (phase << 30 | column << 8 | tfgpu_rowerr):
// constructCI's conversions (phase 0) come before Strictify's (phase 1), each in schema order.
__global__ void __launch_bounds__(256) nginx_convert_cells(GtSet cast_tp, GtSet layout, const uint64_t *p128, const NgCol *cols, int64_t nrows, const uint8_t *data,
                                                           const uint8_t *status, const uint32_t *fpos, const uint32_t *flen, int64_t stride, uint32_t *errkey) {
  const int32_t j = (int32_t)blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const NgCol &c = cols[j];
  const bool text = c.out.kind == SK_STR || c.out.kind == SK_JSONNUM;
  bool valid = true;
  if (r < nrows) {
    if (status[r]) {  // no row: it contributes no text
      if (text) { c.lens[r] = 0; c.fstart[r] = 0; }
    } else if (c.mode == NGM_DEFAULT) {
      ng_store_default(c, r, false);
    } else {
      const uint32_t pos = fpos[(int64_t)c.slot * stride + r], n = flen[(int64_t)c.slot * stride + r];
      MemBytes rd(data);
      const Field fv{&rd, pos, n};
      uint32_t key = 0;
      if (n == 1 && fv[0] == '-') {  // convertNginxValue: a bare "-" is nil, whatever the type
        valid = false;
        ng_store_default(c, r, true);
      } else if (c.mode == NGM_LAYOUT) {
        int64_t sec = 0; int32_t ns = 0;
        if (gotime_parse_any(layout, fv, 0, n, &sec, &ns)) { ((int64_t *)c.out.values)[r] = sec; c.out.nanos[r] = ns; }  // a time.Time passes cast.ToTimeE as it is
        else key = ((uint32_t)j << 8) | (uint32_t)TFGPU_ROW_CAST;
      } else {  // strictifyValue; text stays where it is
        int rc = 0;
        if (!text) rc = strict_cell(c.out, cast_tp, p128, r, fv, 0, n);
        else if (c.out.kind == SK_JSONNUM && !json_number_ok(fv, 0, n)) rc = TFGPU_ROW_CAST;
        else { c.lens[r] = n; c.fstart[r] = pos; }
        if (rc) key = (1u << 30) | ((uint32_t)j << 8) | (uint32_t)rc;
      }
      if (key) atomicMin(&errkey[r], key);
    }
  }
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && r < nrows) c.valid[r >> 6] = m;
}

// the line's verdict: what the walk said, else its first failing column; a line that is no row holds no text in any column
__global__ void __launch_bounds__(256) nginx_finish_rows(const NgCol *cols, int32_t ncols, int64_t nrows, const uint32_t *errkey, uint8_t *status, int32_t *err_col, uint32_t *errflag,
                                                         uint32_t *nbad) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (r < nrows) {
    int st = status[r];
    int32_t col = -1;
    if (!st && errkey[r] != 0xFFFFFFFFu) { st = (int)(errkey[r] & 0xFFu); col = (int32_t)((errkey[r] >> 8) & 0x3FFFFFu); status[r] = (uint8_t)st; }
    err_col[r] = col < 0 ? -1 : cols[col].schema_col;
    errflag[r] = (st != 0 && st != NG_BLANK) ? 1u : 0u;  // a failed line is reported; a blank one was never counted
    bad = st != 0;
    if (bad) for (int32_t ci = 0; ci < ncols; ci++) if (cols[ci].lens) { cols[ci].lens[r] = 0; cols[ci].fstart[r] = 0; }
  }
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(nbad, (uint32_t)__popcll(m));
}

// the error list, in line order: errpos = exclusive scan of the failed-line flags; what does not fit `cap` is counted only
__global__ void nginx_emit_errors(const uint8_t *status, const int32_t *err_col, const uint32_t *errpos, const uint32_t *rank, int64_t n, uint64_t base, int64_t cap,
                                  tfgpu_row_error *out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int st = status[r];
  if (!st || st == NG_BLANK) return;
  const int64_t at = errpos[r];
  if (at < cap) out[at] = tfgpu_row_error{(int64_t)(base + rank[r]), st, 0, err_col[r]};
}
__global__ void nginx_keep_rows(const uint8_t *status, int64_t n, uint32_t *keep) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) keep[r] = status[r] ? 0u : 1u;
}
// one summary for the one read-back behind the kernels: [lines that are no row, non-blank lines, one past the last '\n', failed lines, bytes of every text column]
__global__ void nginx_collect(const uint32_t *nbad, const uint32_t *rank_total, const uint32_t *last_end, const uint32_t *nfailed, const uint32_t *lens_all, int64_t seg_stride,
                              int64_t nrows, int nstr, uint32_t *out) {
  const int i = threadIdx.x;
  if (i == 0) { out[0] = *nbad; out[1] = *rank_total; out[2] = *last_end; out[3] = *nfailed; }
  for (int s = i; s < nstr; s += blockDim.x) out[4 + s] = lens_all[(int64_t)s * seg_stride + nrows];
}

static std::unique_ptr<tfgpu_dbatch> nginx_cells(const NgWalked &w, const tfgpu_nginx_options &opts, const tfgpu_schema &schema, uint32_t *last_end, uint64_t *next_row_number,
                                                 tfgpu_row_error *errs, int64_t errs_cap, int64_t *nerrs) {
  Context &cx = ctx();
  hipStream_t st = cx.stream;
  const int64_t nrows = w.nlines;
  const int64_t n1 = std::max<int64_t>(nrows, 1);
  const int ncols = schema.ncols;
  auto blocks = [](int64_t n, int t) { return (unsigned)std::max<int64_t>(1, (n + t - 1) / t); };
  auto db = std::make_unique<tfgpu_dbatch>();
  db->nrows = nrows;
  int nstr = 0;
  for (int i = 0; i < ncols; i++) {
    const int k = schema.cols[i].dtype;
    if (w.col_slot[(size_t)i] != -2 && (k == TFGPU_T_UTF8 || k == TFGPU_T_BYTES || k == TFGPU_T_ANY || k == TFGPU_T_FLOAT64)) nstr++;
  }
  const int64_t seg_stride = ((nrows + 1 + 3) / 4) * 4, fstride = ((n1 + 3) / 4) * 4;
  Buf lens_all = dalloc((size_t)std::max(nstr, 1) * (size_t)seg_stride * 4 + 64);
  Buf fstart_all = dalloc((size_t)std::max(nstr, 1) * (size_t)fstride * 4 + 64);
  const size_t vbytes = (size_t)((n1 + 63) / 64) * 8;
  std::vector<NgCol> cols;
  std::vector<int> str_col_index;                  // schema index of the k-th text column
  std::vector<int> sys_cols;                       // schema indices of __file_name / __row_index
  bool need_p128 = false;
  int si = 0;
  for (int i = 0; i < ncols; i++) {
    const tfgpu_colschema &sc = schema.cols[i];
    DColumn d;
    d.name = sc.name ? sc.name : ""; d.dtype = sc.dtype;
    if (w.col_slot[(size_t)i] == -2) {
      d.repr = d.name == "__file_name" ? TFGPU_R_STRING : TFGPU_R_UINT64;
      sys_cols.push_back(i);
      db->cols.push_back(std::move(d));
      continue;
    }
    NgCol c{};
    c.slot = w.col_slot[(size_t)i];
    c.schema_col = i;
    c.mode = c.slot < 0 ? NGM_DEFAULT : NGM_STRICT;
    d.repr = strict_describe(sc.dtype, c.out);
    if (d.repr == TFGPU_R_INVALID) throw Error(TFGPU_ERR_CONFIG, "nginx: cannot strictify value of unknown type (column " + d.name + ")");
    // date / datetime: time.Parse(timeLocalLayout).  A timestamp column is a plain string into Strictify: cast.ToTimeE's layouts and nothing else (the CSV
    // reader's parseTimestampValue, which reads an integer as Unix seconds, is not on this path)
    if ((sc.dtype == TFGPU_T_DATE || sc.dtype == TFGPU_T_DATETIME) && c.slot >= 0) c.mode = NGM_LAYOUT;
    if (c.out.kind == SK_F32) need_p128 = true;
    if (c.out.kind == SK_STR || c.out.kind == SK_JSONNUM) {
      c.lens = ptr<uint32_t>(lens_all) + (int64_t)si * seg_stride;
      c.fstart = ptr<uint32_t>(fstart_all) + (int64_t)si * fstride;
      str_col_index.push_back(i);
      si++;
    } else {
      d.values = dalloc((size_t)n1 * (size_t)c.out.width + 64);
      c.out.values = d.values->p;
      if (d.repr == TFGPU_R_TIME) { d.nanos = dalloc((size_t)n1 * 4 + 64); c.out.nanos = ptr<int32_t>(d.nanos); }
    }
    d.validity = dalloc(vbytes + 8);
    c.valid = reinterpret_cast<unsigned long long *>(d.validity->p);
    cols.push_back(c);
    db->cols.push_back(std::move(d));
  }
  const int ndata = (int)cols.size();
  if (ndata >= (1 << 22)) throw Error(TFGPU_ERR_UNSUPPORTED, "nginx: too many columns");
  Buf err_col = dalloc((size_t)n1 * 4 + 16), errkey = dalloc((size_t)n1 * 4 + 16), nbad = dalloc_zero(4);
  Buf errpos = nrows ? dalloc((size_t)(nrows + 1) * 4 + 16) : dalloc_zero(16);  // u32[nrows + 1]: failed lines in front of line r; [nrows] = their number
  Buf bcols = upload_const(cols.data(), std::max<size_t>(cols.size(), 1) * sizeof(NgCol));
  if (nrows) {
    // the cast layouts, then timeLocalLayout
    std::vector<GtOp> gops; std::string glits; std::vector<uint16_t> gstart, gnginx;
    append_cast_layouts(gops, glits, gstart);
    gnginx.push_back((uint16_t)gops.size());
    gotime_compile("02/Jan/2006:15:04:05 -0700", gops, glits);
    gnginx.push_back((uint16_t)gops.size());
    Buf bgops = upload_const(gops.data(), gops.size() * sizeof(GtOp)), bglits = upload_const(glits.data(), glits.size());
    Buf bgs = upload_const(gstart.data(), gstart.size() * 2), bgn = upload_const(gnginx.data(), gnginx.size() * 2);
    const GtSet cast_tp{ptr<GtOp>(bgops), ptr<uint8_t>(bglits), ptr<uint16_t>(bgs), N_CAST_LAYOUTS};
    const GtSet layout{ptr<GtOp>(bgops), ptr<uint8_t>(bglits), ptr<uint16_t>(bgn), 1};
    const uint64_t *p128 = need_p128 ? reinterpret_cast<const uint64_t *>(pow10_table() + 632) : nullptr;
    TF_HIP(hipMemsetAsync(errkey->p, 0xFF, (size_t)nrows * 4, st));
    if (ndata) {
      KernelTimer t("nginx_convert_cells", nrows * ndata);
      nginx_convert_cells<<<dim3(blocks(nrows, 256), (unsigned)ndata), 256, 0, st>>>(cast_tp, layout, p128, reinterpret_cast<const NgCol *>(bcols->p), nrows, w.data, ptr<uint8_t>(w.status),
                                                                                   ptr<uint32_t>(w.fpos), ptr<uint32_t>(w.flen), w.stride, ptr<uint32_t>(errkey));
    }
    nginx_finish_rows<<<blocks(nrows, 256), 256, 0, st>>>(reinterpret_cast<const NgCol *>(bcols->p), ndata, nrows, ptr<uint32_t>(errkey), ptr<uint8_t>(w.status), ptr<int32_t>(err_col), ptr<uint32_t>(errpos),
                                                          ptr<uint32_t>(nbad));
    exclusive_scan_u32(ptr<uint32_t>(errpos), ptr<uint32_t>(errpos), nrows, true);
    if (nstr) exclusive_scan_u32_segments(ptr<uint32_t>(lens_all), nrows, nstr, seg_stride);
  } else if (nstr) {
    TF_HIP(hipMemsetAsync(lens_all->p, 0, (size_t)nstr * (size_t)seg_stride * 4, st));
  }
  Buf summary = dalloc((size_t)(nstr + 4) * 4);
  nginx_collect<<<1, 64, 0, st>>>(ptr<uint32_t>(nbad), ptr<uint32_t>(w.rank) + nrows, w.last_end, ptr<uint32_t>(errpos) + nrows, ptr<uint32_t>(lens_all), seg_stride, nrows, nstr,
                                  ptr<uint32_t>(summary));
  const uint32_t *hsum = d2h_u32(summary->p, (size_t)nstr + 4);
  tf::sync();
  const uint32_t hbad = hsum[0], counted = hsum[1];
  const int64_t ne = hsum[3];
  *last_end = hsum[2];
  if (next_row_number) *next_row_number = opts.row_number_base + counted;

  // ---- text columns: views into the chunk, as the CSV path's ----
  for (int s = 0; s < nstr; s++) {
    DColumn &d = db->cols[(size_t)str_col_index[(size_t)s]];
    d.data_len = hsum[4 + s];
    d.offsets = subbuf(lens_all, (size_t)s * (size_t)seg_stride * 4, (size_t)(nrows + 1) * 4);
    auto v = std::make_shared<TextView>();
    v->src = w.src;
    v->fstart = subbuf(fstart_all, (size_t)s * (size_t)fstride * 4, (size_t)n1 * 4);
    v->jsonnum = d.repr == TFGPU_R_JSONNUM;
    v->has_special = v->jsonnum && w.col_slot[(size_t)str_col_index[(size_t)s]] < 0;  // only a DefaultValue "0" is no byte range of the chunk
    v->quote = '"';
    d.view = std::move(v);
  }

  for (int i : sys_cols) {  // constructCI :227-238; lineCounter: blank lines do not advance it, failed ones do
    std::string detail;
    const int rc = fill_system_column(db->cols[(size_t)i], nrows, opts.file_name, opts.row_number_base, ptr<uint32_t>(w.rank), opts.hide_system_cols, &detail);
    if (rc) throw Error(rc, "nginx: " + detail);
  }
  if (nerrs) *nerrs = ne;
  if (!hbad) return db;
  // failed lines are left out of the batch and reported under their lineCounter; blank lines are left out and were never counted
  const int64_t ncopy = errs ? std::min<int64_t>(ne, std::max<int64_t>(errs_cap, 0)) : 0;
  Buf derrs = dalloc((size_t)std::max<int64_t>(ncopy, 1) * sizeof(tfgpu_row_error));
  if (ncopy) {
    nginx_emit_errors<<<blocks(nrows, 256), 256, 0, st>>>(ptr<uint8_t>(w.status), ptr<int32_t>(err_col), ptr<uint32_t>(errpos), ptr<uint32_t>(w.rank), nrows, opts.row_number_base, ncopy,
                                                          reinterpret_cast<tfgpu_row_error *>(derrs->p));
    d2h(errs, derrs->p, (size_t)ncopy * sizeof(tfgpu_row_error));
  }
  Buf keep = dalloc((size_t)(nrows + 1) * 4);
  nginx_keep_rows<<<blocks(nrows, 256), 256, 0, st>>>(ptr<uint8_t>(w.status), nrows, ptr<uint32_t>(keep));
  if (ncopy) tf::sync();  // (the caller's array is filled when the call returns)
  return compact_rows(*db, keep);
}

}  // namespace tf

extern "C" int tfgpu_nginx_tile_bytes(void) { return NG_TILE; }
extern "C" int tfgpu_nginx_workgroup_lines(void) { return NG_LINES; }

extern "C" int tfgpu_nginx_parse(const tfgpu_nginx_format *f, const tfgpu_nginx_options *opts, const tfgpu_schema *schema, const void *bytes, uint64_t len, int mem,
                                 tfgpu_dbatch **out, uint64_t *consumed, uint64_t *next_row_number, tfgpu_row_error *errs, int64_t errs_cap, int64_t *nerrs) {
  TF_API_BEGIN
  if (!f || !opts || !schema || !out || (len && !bytes)) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_nginx_parse: null argument");
  if (len >= 0x7FFFFFF0ull) return tf::fail(TFGPU_ERR_UNSUPPORTED, "tfgpu_nginx_parse: chunk must be < 2 GiB (the reference reads 20 MiB chunks, chunk_reader.go:12)");
  // ---- which field every column reads (constructCI :240-247) and the token program ----
  NgWalked w;
  const int nfields = (int)f->fields.size();
  std::vector<int32_t> slot_of_field((size_t)nfields, -1);
  int nslots = 0;
  for (int i = 0; i < schema->ncols; i++) {
    const tfgpu_colschema &sc = schema->cols[i];
    const std::string name = sc.name ? sc.name : "";
    if (name == "__file_name" || name == "__row_index") { w.col_slot.push_back(-2); continue; }
    const char *path = sc.path ? sc.path : "";
    char *endp = nullptr;
    const long idx = std::strtol(path, &endp, 10);
    if (endp == path || *endp) return tf::fail(TFGPU_ERR_CONFIG, "nginx: column " + name + ": ColSchema.Path is not an integer (strconv.Atoi)");
    if (idx < 0 || idx >= nfields) { w.col_slot.push_back(-1); continue; }
    if (slot_of_field[(size_t)idx] < 0) slot_of_field[(size_t)idx] = nslots++;
    w.col_slot.push_back(slot_of_field[(size_t)idx]);
  }
  auto prog = std::make_unique<NgParams>();
  std::memset(prog.get(), 0, sizeof(NgParams));
  NgProg &pg = prog->prog;
  if (f->tokens.size() > (size_t)NG_MAXTOK) return tf::fail(TFGPU_ERR_UNSUPPORTED, "nginx: a log_format of more than " + std::to_string(NG_MAXTOK) + " tokens is not device-resident");
  size_t pool = 0;
  for (size_t t = 0; t < f->tokens.size(); t++) {
    const NginxToken &tk = f->tokens[t];
    NgTok &k = pg.tok[t];
    if (tk.is_variable) continue;
    if (pool + tk.value.size() > (size_t)NG_POOL) return tf::fail(TFGPU_ERR_UNSUPPORTED, "nginx: the literals of the log_format exceed " + std::to_string(NG_POOL) + " bytes");
    k.off = (uint16_t)pool; k.len = (uint16_t)tk.value.size();
    std::memcpy(pg.pool + pool, tk.value.data(), tk.value.size());
    pool += tk.value.size();
  }
  for (size_t t = 0, fi = 0; t < f->tokens.size(); t++) {
    if (!f->tokens[t].is_variable) continue;
    NgTok &k = pg.tok[t];
    k.var = 1; k.slot = (int16_t)slot_of_field[fi++];
    for (size_t j = t + 1; j < f->tokens.size(); j++)  // nextDelimiter (:142-149)
      if (!f->tokens[j].is_variable && !f->tokens[j].value.empty()) { k.doff = pg.tok[j].off; k.dlen = pg.tok[j].len; break; }
  }
  pg.ntok = (int32_t)f->tokens.size();

  Context &cx = ctx();
  std::lock_guard<std::mutex> lk(cx.mu);
  hipStream_t st = cx.stream;
  // ---- input in HBM, padded so 16-byte loads never run off the allocation (as tfgpu_csv_parse) ----
  Buf staged;
  const uint8_t *data;
  if (mem == TFGPU_MEM_HOST) {
    staged = dalloc(len + 64);
    if (len) h2d(staged->p, bytes, len);
    TF_HIP(hipMemsetAsync((char *)staged->p + len, 0, 64, st));
    data = ptr<uint8_t>(staged);
  } else {
    data = (const uint8_t *)bytes;
    if (!find_device_block(data)) {  // a foreign device pointer is only trusted for the duration of the call: the views need a copy the library owns
      staged = dalloc(len + 64);
      if (len) d2d(staged->p, bytes, len);
      TF_HIP(hipMemsetAsync((char *)staged->p + len, 0, 64, st));
      data = ptr<uint8_t>(staged);
    } else if (reinterpret_cast<uintptr_t>(data) & 15) return tf::fail(TFGPU_ERR_INVALID, "nginx: device buffer must be 16-byte aligned");
  }
  // ---- line index: where every line starts; the bytes behind the last '\n' are a line on the last round only ----
  Buf row_start;
  const int64_t nl = newline_starts(data, len, &row_start);
  const int64_t nlines = nl + (opts->last_chunk ? 1 : 0);
  w.data = data; w.len = len; w.src = staged ? staged : find_device_block(data);
  w.nlines = nlines;
  w.stride = ((std::max<int64_t>(nlines, 1) + 3) / 4) * 4;
  w.status = dalloc((size_t)nlines + 16);
  w.rank = dalloc_zero((size_t)(nlines + 2) * 4);
  w.last_end = ptr<uint32_t>(row_start) + nl;
  w.fpos = dalloc((size_t)std::max(nslots, 1) * (size_t)w.stride * 4);
  w.flen = dalloc((size_t)std::max(nslots, 1) * (size_t)w.stride * 4);
  if (nlines) {
    Buf line_end = dalloc((size_t)nlines * 4 + 16);
    {
      KernelTimer t("nginx_line_flags", nlines);
      nginx_line_flags<<<(unsigned)((nlines + 255) / 256), 256, 0, st>>>(data, len, ptr<uint32_t>(row_start), nl, nlines, ptr<uint32_t>(line_end), ptr<uint8_t>(w.status), ptr<uint32_t>(w.rank));
    }
    exclusive_scan_u32(ptr<uint32_t>(w.rank), ptr<uint32_t>(w.rank), nlines, true);
    NgParams &p = *prog;
    p.data = data; p.len = len; p.row_start = ptr<uint32_t>(row_start); p.line_end = ptr<uint32_t>(line_end); p.status = ptr<uint8_t>(w.status);
    p.nlines = nlines; p.fpos = ptr<uint32_t>(w.fpos); p.flen = ptr<uint32_t>(w.flen); p.stride = w.stride; p.extra_err = opts->unexpected_field_error ? 1 : 0;
    {
      KernelTimer t("nginx_parse_lines", (int64_t)len);
      nginx_parse_lines<<<(unsigned)((nlines + NG_LINES - 1) / NG_LINES), NG_LINES, 0, st>>>(p);
    }
    uint32_t last_end = 0;
    std::unique_ptr<tfgpu_dbatch> db = nginx_cells(w, *opts, *schema, &last_end, next_row_number, errs, errs_cap, nerrs);
    if (consumed) *consumed = opts->last_chunk ? len : last_end;
    *out = db.release();
    return TFGPU_OK;
  }
  uint32_t last_end = 0;
  std::unique_ptr<tfgpu_dbatch> db = nginx_cells(w, *opts, *schema, &last_end, next_row_number, errs, errs_cap, nerrs);
  if (consumed) *consumed = 0;  // no complete line: everything is handed back
  *out = db.release();
  return TFGPU_OK;
  TF_API_END
}
