// tf_nativeschema.cpp — the native parser's host work, once per distinct group key (tf_nativeparse.hpp): the texts of the group's first item are read
// with the library's config JSON reader, the columns are looked up BY NAME in the item's table_schema as RestoreChangeItems does
// (restore.go:320-342: a map by ColumnName, so a later schema column of the same name stands), and every column gets the conversion Restore
// applies to it (restore.go:20-256) as far as the device follows it.  No kernels.
#include "tf_nativeparse.hpp"

#include <algorithm>

#include "tf_plan.hpp"

namespace tf {
namespace natp {

static bool starts_with(const std::string &s, const char *p) { return s.compare(0, std::strlen(p), p) == 0; }

// abstract.IsMysqlBinaryType (restore.go:282-306): the type trimmed at the first byte that is neither a-z nor ':'
static bool is_mysql_binary(const std::string &t) {
  size_t n = 0;
  while (n < t.size() && ((t[n] >= 'a' && t[n] <= 'z') || t[n] == ':')) n++;
  const std::string q = t.substr(0, n);
  for (const char *b : {"mysql:tinyblob", "mysql:blob", "mysql:mediumblob", "mysql:longblob", "mysql:binary", "mysql:varbinary", "mysql:bit", "mysql:geometry",
                        "mysql:geomcollection", "mysql:geometrycollection", "mysql:point", "mysql:multipoint", "mysql:linestring", "mysql:multilinestring",
                        "mysql:polygon", "mysql:multipolygon"})
    if (q == b) return true;
  return false;
}

static int dtype_of(const std::string &t) {
  static const char *N[] = {"invalid", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float", "double", "boolean", "string", "utf8",
                            "date", "datetime", "timestamp", "interval", "any"};
  for (int i = 1; i < TFGPU_T__COUNT; i++) if (t == N[i]) return i;
  return TFGPU_T_INVALID;
}

static ColOp op_of(int dtype, const std::string &ot) {
  ColOp o{OP_FALLBACK, (uint8_t)dtype, 0, TFGPU_NATIVE_SCHEMA_COLUMN};
  switch (dtype) {
    case TFGPU_T_INT8: case TFGPU_T_INT16: case TFGPU_T_INT32: case TFGPU_T_INT64:
    case TFGPU_T_UINT8: case TFGPU_T_UINT16: case TFGPU_T_UINT32: case TFGPU_T_UINT64: o.op = OP_INT; break;
    case TFGPU_T_FLOAT32: case TFGPU_T_FLOAT64: o.op = OP_JSONNUM; break;
    case TFGPU_T_BOOLEAN: o.op = OP_BOOL; break;
    case TFGPU_T_BYTES: case TFGPU_T_UTF8:
      o.op = OP_STRING;
      if (is_mysql_binary(ot) || ot == "pg:bytea" || ot == "ydb:String" || starts_with(ot, "mysql:binary") || starts_with(ot, "mysql:blob")) o.op = OP_BASE64;
      if (starts_with(ot, "mysql:bit")) o.flags |= F_MYSQL_BIT;
      break;
    case TFGPU_T_DATE: case TFGPU_T_DATETIME: case TFGPU_T_TIMESTAMP: o.op = OP_TIME; break;
    case TFGPU_T_INTERVAL: o.op = OP_INTERVAL; break;
    case TFGPU_T_ANY:
      o.op = OP_ANY;
      if (starts_with(ot, "mongo:bson")) { o.op = OP_FALLBACK; o.reason = TFGPU_NATIVE_MONGO_BSON; }
      else if (ot == "mysql:json" || starts_with(ot, "ch:Decimal(") || starts_with(ot, "ch:Nullable(Decimal(")) o.flags |= F_ANY_STRING_OK;
      else if (starts_with(ot, "pg:timestamp")) o.flags |= F_ANY_PG_TIMESTAMP;
      else if (starts_with(ot, "pg:")) o.flags |= F_ANY_STRING_OK;
      break;
    default: break;
  }
  return o;
}

int repr_of(const ColOp &o) {
  switch (o.op) {
    case OP_INT: return TFGPU_R_INT8 + (o.dtype - TFGPU_T_INT8);
    case OP_JSONNUM: return TFGPU_R_JSONNUM;
    case OP_BOOL: return TFGPU_R_BOOL;
    case OP_BASE64: return TFGPU_R_BYTES;
    case OP_TIME: return TFGPU_R_TIME;
    case OP_INTERVAL: return TFGPU_R_DURATION;
    case OP_ANY: return TFGPU_R_JSON;
    default: return TFGPU_R_STRING;  // OP_STRING; a column that only falls back never gets a row
  }
}

// encoding/json's appendString with escapeHTML, as the device writes an `any` string (tf_jsonscan.hpp emit_go_string)
static void go_quote(std::string &o, const std::string &s) {
  static const char *H = "0123456789abcdef";
  o += '"';
  for (size_t i = 0; i < s.size(); i++) {
    const unsigned char c = (unsigned char)s[i];
    if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
    else if (c == '\b') o += "\\b";
    else if (c == '\f') o += "\\f";
    else if (c == '\n') o += "\\n";
    else if (c == '\r') o += "\\r";
    else if (c == '\t') o += "\\t";
    else if (c < 0x20 || c == '<' || c == '>' || c == '&') { o += "\\u00"; o += H[c >> 4]; o += H[c & 15]; }
    else if (c == 0xE2 && i + 2 < s.size() && (unsigned char)s[i + 1] == 0x80 && ((unsigned char)s[i + 2] == 0xA8 || (unsigned char)s[i + 2] == 0xA9)) {
      o += (unsigned char)s[i + 2] == 0xA8 ? "\\u2028" : "\\u2029";
      i += 2;
    } else o += (char)c;
  }
  o += '"';
}
// json.Marshal of a value decoded with UseNumber: compact, map keys ascending (the last of a repeated key stands), number literals as written
static void marshal(std::string &o, const Json &j) {
  switch (j.type) {
    case Json::Null: o += "null"; break;
    case Json::Bool: o += j.b ? "true" : "false"; break;
    case Json::Num: o += j.str; break;
    case Json::Str: go_quote(o, j.str); break;
    case Json::Arr:
      o += '[';
      for (size_t i = 0; i < j.arr.size(); i++) { if (i) o += ','; marshal(o, j.arr[i]); }
      o += ']';
      break;
    case Json::Obj: {
      std::vector<size_t> at;
      for (size_t i = 0; i < j.obj.size(); i++) {
        bool later = false;
        for (size_t k = i + 1; k < j.obj.size(); k++) if (j.obj[k].first == j.obj[i].first) later = true;
        if (!later) at.push_back(i);
      }
      std::sort(at.begin(), at.end(), [&](size_t a, size_t b) { return j.obj[a].first < j.obj[b].first; });
      o += '{';
      for (size_t i = 0; i < at.size(); i++) { if (i) o += ','; go_quote(o, j.obj[at[i]].first); o += ':'; marshal(o, j.obj[at[i]].second); }
      o += '}';
      break;
    }
  }
}

// a string member / element as Go decodes it into a string: null is ""
static bool as_string(const Json &j, std::string &out) {
  if (j.type == Json::Null) { out.clear(); return true; }
  if (j.type != Json::Str) return false;
  out = j.str;
  return true;
}
static bool string_list(const std::string &text, std::vector<std::string> &out) {
  if (text.empty()) return true;
  const Json j = Json::parse(text);
  if (j.type == Json::Null) return true;
  if (j.type != Json::Arr) return false;
  for (auto &x : j.arr) { std::string s; if (!as_string(x, s)) return false; out.push_back(s); }
  return true;
}
// a `\ud…` escape: the config reader does not turn a lone surrogate into U+FFFD as encoding/json does
static bool has_surrogate_escape(const std::string &t) {
  for (size_t i = 0; i + 2 < t.size(); i++) if (t[i] == '\\' && t[i + 1] == 'u' && (t[i + 2] == 'd' || t[i + 2] == 'D')) return true;
  return false;
}

std::shared_ptr<const GroupInfo> compile_group(const std::string &schema, const std::string &table, const std::string &part, const std::string &columnnames,
                                               const std::string &table_schema, const std::string &keynames, const std::string &keytypes) {
  auto g = std::make_shared<GroupInfo>();
  bool readable = true;
  try {
    for (const std::string *t : {&schema, &table, &part, &columnnames, &table_schema, &keynames, &keytypes}) if (has_surrogate_escape(*t)) readable = false;
    auto one = [&](const std::string &text, std::string &out) { if (!text.empty() && !as_string(Json::parse(text), out)) readable = false; };
    if (readable) { one(schema, g->ns); one(table, g->table); one(part, g->part); }
    if (readable && !string_list(columnnames, g->names)) readable = false;
    if (readable && !string_list(keynames, g->key_names)) readable = false;
    if (readable && !string_list(keytypes, g->key_types)) readable = false;
    g->names_form = columnnames.empty() || columnnames == "null" ? 1 : g->names.empty() ? 2 : 0;
    if (readable && !table_schema.empty()) {
      const Json ts = Json::parse(table_schema);
      if (ts.type == Json::Arr) {
        for (auto &c : ts.arr) {
          if (c.type != Json::Obj) { readable = false; break; }
          GroupInfo::SCol sc;
          // a struct decoded by encoding/json: keys match case-insensitively and the last of a repeated key stands; a ColSchema spelled that way is
          // left to the host
          for (size_t i = 0; i < c.obj.size() && readable; i++) {
            const std::string &k = c.obj[i].first; const Json &v = c.obj[i].second;
            for (size_t q = 0; q < i; q++) if (c.obj[q].first == k) readable = false;
            auto str = [&](std::string &dst) { if (!as_string(v, dst)) readable = false; };
            auto flag = [&](uint32_t bit) { if (v.type == Json::Bool) { if (v.b) sc.flags |= bit; } else if (v.type != Json::Null) readable = false; };
            if (k == "name") str(sc.name);
            else if (k == "type") { std::string t; str(t); sc.dtype = dtype_of(t); }
            else if (k == "key") flag(TFGPU_COL_KEY);
            else if (k == "fake_key") flag(TFGPU_COL_FAKE_KEY);
            else if (k == "required") flag(TFGPU_COL_REQUIRED);
            else if (k == "path") str(sc.path);
            else if (k == "original_type") str(sc.original_type);
            else if (k == "table_schema") str(sc.table_schema);
            else if (k == "table_name") str(sc.table_name);
            else if (k == "expression") str(sc.expression);
            else if (k == "properties") { if (v.type == Json::Obj) { if (!v.obj.empty()) marshal(sc.properties_json, v); } else if (v.type != Json::Null) readable = false; }
            else {
              for (const char *known : {"name", "type", "key", "fake_key", "required", "path", "original_type", "table_schema", "table_name", "expression", "properties"}) {
                std::string lk = k;
                for (auto &ch : lk) ch = (char)std::tolower((unsigned char)ch);
                if (lk == known) readable = false;  // a case variant of a known tag
              }
            }
          }
          g->schema.push_back(std::move(sc));
        }
      } else if (ts.type != Json::Null) readable = false;
      g->table_schema_json = table_schema;
    }
  } catch (const Error &) { readable = false; }  // (the device has validated the JSON: what the config reader still refuses — nesting past its limit — is the host's)
  if (g->names.size() + g->key_names.size() > 65535 || g->schema.size() > 65535)
    throw Error(TFGPU_ERR_UNSUPPORTED, "native parser: a group of more than 65 535 columns (table " + g->table + "): such messages go through the stock parser");
  auto find = [&](const std::string &name) -> const GroupInfo::SCol * {
    const GroupInfo::SCol *hit = nullptr;
    for (auto &c : g->schema) if (c.name == name) hit = &c;
    return hit;
  };
  auto add = [&](const std::string &name) {
    const GroupInfo::SCol *c = readable ? find(name) : nullptr;
    ColOp o = c && c->dtype != TFGPU_T_INVALID ? op_of(c->dtype, c->original_type) : ColOp{OP_FALLBACK, 0, 0, TFGPU_NATIVE_SCHEMA_COLUMN};
    if (o.op == OP_ANY) g->has_any = true;
    g->ops.push_back(o);
  };
  for (auto &n : g->names) add(n);
  for (auto &n : g->key_names) add(n);
  g->unreadable = !readable;  // every item of the group falls back, blamed on the item itself (column -1)
  for (auto &t : g->key_types) g->key_type_ptrs.push_back(t.c_str());
  for (auto &c : g->schema) {
    tfgpu_colschema cc{};
    cc.name = c.name.c_str(); cc.dtype = c.dtype; cc.flags = c.flags; cc.path = c.path.c_str(); cc.original_type = c.original_type.c_str();
    cc.table_schema = c.table_schema.c_str(); cc.table_name = c.table_name.c_str(); cc.expression = c.expression.c_str();
    cc.properties_json = c.properties_json.empty() ? nullptr : c.properties_json.c_str();
    g->ccols.push_back(cc);
  }
  g->cschema.ncols = (int32_t)g->ccols.size();
  g->cschema.cols = g->ccols.data();
  return g;
}

}  // namespace natp
}  // namespace tf
