// tf_protodesc.cpp — the per-config half of the generic protobuf parser (pkg/parsers/registry/protobuf): a serialized FileDescriptorSet and a
// ParserConfigProtoCommon / ParserConfigProtoLb become the result TableSchema and the field table the device decodes by (tf_protoparse.hip).
//
//   ToProtoParserConfig                            parser_config_proto_common.go:33-77, parser_config_proto_lb.go:36-80
//   SetDescriptors, extractMessageDesc,            protoparser/proto_parser_config.go:57-135
//   extractEmbeddedRepeatedMsgDesc
//   NewProtoParser, makeLbExtraSchemas,            protoparser/proto_parser.go:396-562
//   makeAuxSchemas, protoFieldDescToYtType         protoparser/proto_parser.go:365-394
//
// descriptorpb and protodesc are dependencies of the reference, not part of it.  Restated here from the published descriptor.proto: the fields
// of FileDescriptorSet / FileDescriptorProto / DescriptorProto / FieldDescriptorProto the parser reads (names, numbers, labels, types, type
// names, oneof_index, proto3_optional, the map_entry and packed options), with type names resolved across the files of the set.
// Host code: no GPU is needed for anything in this file.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "tf_plan.hpp"
#include "tf_protodesc.hpp"

namespace tf {
namespace ppd {

struct BadDesc { std::string why; };

// ---- the wire form of the descriptor messages -----------------------------------------------------------------------------------------------------
struct Rd {
  const uint8_t *p, *e;
  bool varint(uint64_t &v) {
    v = 0;
    for (int s = 0; s < 70; s += 7) {
      if (p >= e) return false;
      const uint8_t c = *p++;
      v |= (uint64_t)(c & 0x7F) << s;
      if (!(c & 0x80)) return true;
    }
    return false;
  }
};
// f(number, wire type, varint / fixed value, bytes, len) for every field of [p, e)
template <class F> static void each_field(const uint8_t *p, size_t n, F f) {
  Rd r{p, p + n};
  while (r.p < r.e) {
    uint64_t tag, v = 0;
    if (!r.varint(tag)) throw BadDesc{"proto: cannot parse invalid wire-format data"};
    const int wt = (int)(tag & 7);
    const uint64_t num = tag >> 3;
    const uint8_t *b = nullptr; size_t len = 0;
    if (num == 0) throw BadDesc{"proto: cannot parse invalid wire-format data"};
    if (wt == 0) { if (!r.varint(v)) throw BadDesc{"proto: cannot parse invalid wire-format data"}; }
    else if (wt == 1) { if (r.e - r.p < 8) throw BadDesc{"proto: cannot parse invalid wire-format data"}; std::memcpy(&v, r.p, 8); r.p += 8; }
    else if (wt == 5) { if (r.e - r.p < 4) throw BadDesc{"proto: cannot parse invalid wire-format data"}; uint32_t x; std::memcpy(&x, r.p, 4); v = x; r.p += 4; }
    else if (wt == 2) {
      uint64_t l;
      if (!r.varint(l) || l > (uint64_t)(r.e - r.p)) throw BadDesc{"proto: cannot parse invalid wire-format data"};
      b = r.p; len = (size_t)l; r.p += l;
    } else throw BadDesc{"proto: cannot parse invalid wire-format data"};  // (descriptor.proto has no groups)
    f((uint32_t)num, wt, v, b, len);
  }
}
static std::string str(const uint8_t *b, size_t n) { return std::string((const char *)b, n); }

struct FieldD { std::string name, type_name; int32_t number = 0, label = 1, type = 0, oneof_index = -1; bool proto3_optional = false; };
struct MsgD {
  std::string name, full; std::vector<FieldD> fields; std::vector<std::unique_ptr<MsgD>> nested; bool map_entry = false; int noneof = 0;
  bool proto3 = false;
};
struct FileD { std::string name, package, syntax; std::vector<std::unique_ptr<MsgD>> messages; };

static FieldD read_field(const uint8_t *p, size_t n) {
  FieldD f;
  each_field(p, n, [&](uint32_t num, int wt, uint64_t v, const uint8_t *b, size_t len) {
    if (num == 1 && wt == 2) f.name = str(b, len);
    else if (num == 3 && wt == 0) f.number = (int32_t)v;
    else if (num == 4 && wt == 0) f.label = (int32_t)v;
    else if (num == 5 && wt == 0) f.type = (int32_t)v;
    else if (num == 6 && wt == 2) f.type_name = str(b, len);
    else if (num == 9 && wt == 0) f.oneof_index = (int32_t)v;
    else if (num == 17 && wt == 0) f.proto3_optional = v != 0;
    // (options.packed: both forms of a repeated scalar are accepted on the wire whatever it says)
  });
  return f;
}
static std::unique_ptr<MsgD> read_message(const uint8_t *p, size_t n, const std::string &scope, bool proto3) {
  auto m = std::make_unique<MsgD>();
  m->proto3 = proto3;
  each_field(p, n, [&](uint32_t num, int wt, uint64_t, const uint8_t *b, size_t len) { if (num == 1 && wt == 2) m->name = str(b, len); });
  m->full = scope.empty() ? m->name : scope + "." + m->name;
  each_field(p, n, [&](uint32_t num, int wt, uint64_t, const uint8_t *b, size_t len) {
    if (wt != 2) return;
    if (num == 2) m->fields.push_back(read_field(b, len));
    else if (num == 3) m->nested.push_back(read_message(b, len, m->full, proto3));
    else if (num == 7) each_field(b, len, [&](uint32_t n2, int w2, uint64_t v2, const uint8_t *, size_t) { if (n2 == 7 && w2 == 0) m->map_entry = v2 != 0; });
    else if (num == 8) m->noneof++;
  });
  return m;
}
static FileD read_file(const uint8_t *p, size_t n) {
  FileD f;
  each_field(p, n, [&](uint32_t num, int wt, uint64_t, const uint8_t *b, size_t len) {
    if (wt != 2) return;
    if (num == 1) f.name = str(b, len);
    else if (num == 2) f.package = str(b, len);
    else if (num == 12) f.syntax = str(b, len);
  });
  each_field(p, n, [&](uint32_t num, int wt, uint64_t, const uint8_t *b, size_t len) {
    if (wt == 2 && num == 4) f.messages.push_back(read_message(b, len, f.package, f.syntax == "proto3"));
  });
  return f;
}
static void index_messages(const MsgD &m, std::map<std::string, const MsgD *> &by_full) {
  by_full["." + m.full] = &m;
  for (auto &c : m.nested) index_messages(*c, by_full);
}

// FieldDescriptorProto.Type → TFGPU_PB_* (0: group)
static int ptype_of(int t) {
  switch (t) {
    case 1: return TFGPU_PB_DOUBLE; case 2: return TFGPU_PB_FLOAT; case 3: return TFGPU_PB_INT64; case 4: return TFGPU_PB_UINT64; case 5: return TFGPU_PB_INT32;
    case 6: return TFGPU_PB_FIXED64; case 7: return TFGPU_PB_FIXED32; case 8: return TFGPU_PB_BOOL; case 9: return TFGPU_PB_STRING; case 11: return TFGPU_PB_MESSAGE;
    case 12: return TFGPU_PB_BYTES; case 13: return TFGPU_PB_UINT32; case 14: return TFGPU_PB_ENUM; case 15: return TFGPU_PB_SFIXED32; case 16: return TFGPU_PB_SFIXED64;
    case 17: return TFGPU_PB_SINT32; case 18: return TFGPU_PB_SINT64; default: return 0;
  }
}
// protoFieldDescToYtType
static int yt_type(const FieldD &f) {
  if (f.label == 3) return TFGPU_T_ANY;  // IsList / IsMap
  switch (ptype_of(f.type)) {
    case TFGPU_PB_BOOL: return TFGPU_T_BOOLEAN;
    case TFGPU_PB_INT32: case TFGPU_PB_SINT32: case TFGPU_PB_SFIXED32: case TFGPU_PB_ENUM: return TFGPU_T_INT32;
    case TFGPU_PB_INT64: case TFGPU_PB_SINT64: case TFGPU_PB_SFIXED64: return TFGPU_T_INT64;
    case TFGPU_PB_UINT32: case TFGPU_PB_FIXED32: return TFGPU_T_UINT32;
    case TFGPU_PB_UINT64: case TFGPU_PB_FIXED64: return TFGPU_T_UINT64;
    case TFGPU_PB_FLOAT: return TFGPU_T_FLOAT32;
    case TFGPU_PB_DOUBLE: return TFGPU_T_FLOAT64;
    case TFGPU_PB_STRING: return TFGPU_T_UTF8;   // ytschema.TypeString = "utf8"
    case TFGPU_PB_BYTES: return TFGPU_T_BYTES;   // ytschema.TypeBytes = "string"
    default: return TFGPU_T_ANY;                 // message, group
  }
}

struct Compiler {
  std::map<std::string, const MsgD *> by_full;
  tfgpu_proto_parser &out;
  explicit Compiler(tfgpu_proto_parser &o) : out(o) {}

  const MsgD *resolve(const FieldD &f) const {
    auto it = by_full.find(f.type_name);
    if (it == by_full.end()) throw BadDesc{"could not resolve type " + f.type_name + " of field " + f.name};
    return it->second;
  }
  uint32_t put_name(const std::string &s) { const uint32_t at = (uint32_t)out.names.size(); out.names += s; return at; }

  // a one-level message of singular scalar members: its members sorted by name (json.Marshal's key order).  "" or why it is not in the subset
  std::string members_of(const MsgD &m, pbd::DField &d) {
    if (m.full.rfind("google.protobuf.", 0) == 0) return m.full;
    if (!m.proto3) return "a message of a proto2 file (" + m.full + ")";
    std::vector<const FieldD *> fs;
    for (auto &f : m.fields) {
      if (f.label == 3) return "a repeated or map field inside the nested message " + m.full;
      const int t = ptype_of(f.type);
      if (t == 0) return "a group inside the nested message " + m.full;
      if (t == TFGPU_PB_MESSAGE) return "nesting deeper than one level (" + m.full + "." + f.name + ")";
      if (f.oneof_index >= 0 && !f.proto3_optional) return "a oneof inside the nested message " + m.full;
      fs.push_back(&f);
    }
    std::sort(fs.begin(), fs.end(), [](const FieldD *a, const FieldD *b) { return a->name < b->name; });
    d.mem_off = (int32_t)out.members.size(); d.nmem = (int32_t)fs.size();
    for (auto *f : fs) out.members.push_back(pbd::DMember{f->number, ptype_of(f->type) | (f->proto3_optional ? MEMBER_EXPLICIT : 0), put_name(f->name), (uint32_t)f->name.size()});
    return "";
  }
  // one field of the event message: the table entry, or why the device does not take it
  std::string field_of(const FieldD &f, pbd::DField &d, uint32_t &flags) {
    d = pbd::DField{};
    d.number = f.number; d.name_off = put_name(f.name); d.name_len = (uint32_t)f.name.size();
    const int t = ptype_of(f.type);
    d.ptype = t;
    if (t == 0) return "a group field";
    if (f.label == 2) return "a proto2 required field";
    if (f.label == 3) {
      d.repeated = 1;
      if (t != TFGPU_PB_MESSAGE) return "";
      const MsgD *m = resolve(f);
      if (m->map_entry) {
        const FieldD *k = nullptr, *v = nullptr;
        for (auto &x : m->fields) { if (x.number == 1) k = &x; if (x.number == 2) v = &x; }
        if (!k || !v) throw BadDesc{"map entry " + m->full + " without key or value"};
        if (ptype_of(k->type) != TFGPU_PB_STRING) return "a map keyed by other than a string";
        const int vt = ptype_of(v->type);
        if (vt == TFGPU_PB_MESSAGE || vt == 0) return "a map with message values";
        d.repeated = 2; d.mem_off = (int32_t)out.members.size(); d.nmem = 2;
        out.members.push_back(pbd::DMember{1, TFGPU_PB_STRING, put_name("key"), 3});
        out.members.push_back(pbd::DMember{2, vt, put_name("value"), 5});
        return "";
      }
      return members_of(*m, d);
    }
    if (f.oneof_index >= 0 && !f.proto3_optional) d.oneof = f.oneof_index + 1;  // a member of a real oneof (a proto3 `optional` is a synthetic one of its own)
    if (t == TFGPU_PB_MESSAGE) { flags |= PF_EXPLICIT; return members_of(*resolve(f), d); }
    if (f.proto3_optional || d.oneof) flags |= PF_EXPLICIT;
    return "";
  }
};

struct Config {
  std::string desc, resource, message;
  std::vector<std::pair<std::string, bool>> include;
  std::vector<std::string> keys;
  int pkg = TFGPU_PROTO_PKG_SINGLE;
  bool null_keys = false, sys_cols = false, skip_dedup = false, synth_keys = false, nfe = false;
};

static std::unique_ptr<tfgpu_proto_parser> compile(const Config &c) {
  // ---- ToProtoParserConfig ------------------------------------------------------------------------------------------------------------------------
  if (c.desc.empty() && c.resource.empty()) throw Error(TFGPU_ERR_CONFIG, "desc file and desc resource are both empty");
  if (!c.resource.empty()) throw Error(TFGPU_ERR_UNSUPPORTED, "protobuf parser: DescResourceName (" + c.resource + ") is resolved by the shim: pass the resource's bytes as DescFile");
  if (c.pkg != TFGPU_PROTO_PKG_PROTOSEQ && c.pkg != TFGPU_PROTO_PKG_REPEATED && c.pkg != TFGPU_PROTO_PKG_SINGLE) throw Error(TFGPU_ERR_CONFIG, "protobuf parser: unknown PackageType");
  auto h = std::make_unique<tfgpu_proto_parser>();
  h->pkg = c.pkg; h->not_fill_empty = c.nfe;
  Compiler cc(*h);
  // ---- SetDescriptors: extractMessageDesc -----------------------------------------------------------------------------------------------------------
  const std::string SD = "SetDescriptors error: ", EX = "error extracting message descriptor from desc file: ";
  std::vector<FileD> files;
  try {
    each_field((const uint8_t *)c.desc.data(), c.desc.size(), [&](uint32_t num, int wt, uint64_t, const uint8_t *b, size_t len) { if (num == 1 && wt == 2) files.push_back(read_file(b, len)); });
  } catch (const BadDesc &e) { throw Error(TFGPU_ERR_CONFIG, SD + EX + "error unmarshaling proto desc file content: " + e.why); }
  for (auto &f : files) for (auto &m : f.messages) index_messages(*m, cc.by_full);
  const MsgD *root = nullptr; int found = 0;
  for (auto &f : files) for (auto &m : f.messages) if (m->name == c.message) { if (!root) root = m.get(); found++; }
  if (!root) throw Error(TFGPU_ERR_CONFIG, SD + EX + "message with provided name '" + c.message + "' not found");
  if (found > 1) throw Error(TFGPU_ERR_UNSUPPORTED, "protobuf parser: message name '" + c.message + "' is defined by more than one file of the descriptor set: which one the reference takes depends on its registry's order");
  const MsgD *ev = root;
  try {
    if (c.pkg == TFGPU_PROTO_PKG_REPEATED) {  // extractEmbeddedRepeatedMsgDesc: exactly one field, a list (no map) of messages
      const MsgD *el = nullptr;
      if (root->fields.size() == 1 && root->fields[0].label == 3 && ptype_of(root->fields[0].type) == TFGPU_PB_MESSAGE) { el = cc.resolve(root->fields[0]); if (el->map_entry) el = nullptr; }
      if (!el) throw Error(TFGPU_ERR_CONFIG, SD + "can't extract embedded repeated message descriptor while provided package type is repeated");
      h->wrapper_number = root->fields[0].number;
      ev = el;
    }
    h->message = ev->full;
    // ---- NewProtoParser ---------------------------------------------------------------------------------------------------------------------------------
    std::map<std::string, bool> params;
    for (auto &p : c.include) { if (params.count(p.first)) throw Error(TFGPU_ERR_CONFIG, "duplicate column name '" + p.first + "'"); params[p.first] = p.second; }
    auto by_name = [&](const std::string &n) -> int { for (size_t i = 0; i < ev->fields.size(); i++) if (ev->fields[i].name == n) return (int)i; return -1; };
    std::set<std::string> key_set;
    for (auto &k : c.keys) {
      key_set.insert(k);
      const int fi = by_name(k);
      if (fi < 0) throw Error(TFGPU_ERR_CONFIG, "given key field '" + k + "' not found in proto message desc");
      bool req = !c.null_keys;
      auto it = params.find(k);
      if (it != params.end()) { if (!c.null_keys && !it->second) throw Error(TFGPU_ERR_CONFIG, "key param '" + k + "' must be set as required"); req = it->second; }
      h->cols.push_back(Col{k, yt_type(ev->fields[(size_t)fi]), TFGPU_COL_KEY | (req ? TFGPU_COL_REQUIRED : 0u), fi, AUX_NONE, false});
    }
    if (c.include.empty()) {
      for (size_t i = 0; i < ev->fields.size(); i++) if (!key_set.count(ev->fields[i].name)) h->cols.push_back(Col{ev->fields[i].name, yt_type(ev->fields[i]), 0u, (int)i, AUX_NONE, false});
    } else for (auto &p : c.include) {
      const int fi = by_name(p.first);
      if (fi < 0) throw Error(TFGPU_ERR_CONFIG, "requested column " + p.first + " not found in proto descriptor");
      if (key_set.count(p.first)) continue;
      h->cols.push_back(Col{p.first, yt_type(ev->fields[(size_t)fi]), p.second ? TFGPU_COL_REQUIRED : 0u, fi, AUX_NONE, false});
    }
    if (c.sys_cols) {  // makeLbExtraSchemas
      std::set<std::string> have;
      for (auto &x : h->cols) have.insert(x.name);
      for (size_t i = 0; i < ev->fields.size(); i++) if (!have.count(ev->fields[i].name)) h->cols.push_back(Col{"_lb_extra_" + ev->fields[i].name, yt_type(ev->fields[i]), 0u, (int)i, AUX_NONE, true});
    }
    auto aux = [&](const char *name, int dtype, bool key, int kind) { h->cols.push_back(Col{name, dtype, key ? (TFGPU_COL_KEY | (c.null_keys ? 0u : TFGPU_COL_REQUIRED)) : 0u, -1, kind, false}); };
    if (c.synth_keys) { aux("_partition", TFGPU_T_UTF8, true, AUX_PARTITION); aux("_offset", TFGPU_T_UINT64, true, AUX_OFFSET); aux("_idx", TFGPU_T_UINT64, true, AUX_IDX); }
    if (c.sys_cols) { aux("_lb_ctime", TFGPU_T_DATETIME, !c.skip_dedup, AUX_CTIME); aux("_lb_wtime", TFGPU_T_DATETIME, !c.skip_dedup, AUX_WTIME); }
    // ---- the field table ---------------------------------------------------------------------------------------------------------------------------------
    std::vector<bool> is_col(ev->fields.size(), false);
    for (auto &x : h->cols) if (x.field >= 0) is_col[(size_t)x.field] = true;
    if (!ev->proto3) { h->code = TFGPU_ROW_HOST_FALLBACK; h->why = "a proto2 file defines " + ev->full; }
    for (size_t i = 0; i < ev->fields.size(); i++) {
      pbd::DField d; uint32_t fl = 0;
      const std::string why = cc.field_of(ev->fields[i], d, fl);
      if (!why.empty()) {
        fl |= PF_FOREIGN;
        if (is_col[i] && h->code == TFGPU_ROW_OK) { h->code = TFGPU_ROW_HOST_FALLBACK; h->why = "column " + ev->fields[i].name + ": " + why; }
      }
      h->fields.push_back(d); h->fflags.push_back(fl);
    }
    if (h->fields.size() > 4096) { h->code = TFGPU_ROW_HOST_FALLBACK; h->why = "more than 4096 fields"; }
  } catch (const BadDesc &e) { throw Error(TFGPU_ERR_CONFIG, SD + EX + "can't create new protoregistry files: " + e.why); }
  h->names.append(16, '\0');
  return h;
}

static std::string base64_decode(const std::string &s) {
  std::string o; uint32_t acc = 0; int bits = 0;
  for (unsigned char ch : s) {
    int v;
    if (ch >= 'A' && ch <= 'Z') v = ch - 'A'; else if (ch >= 'a' && ch <= 'z') v = ch - 'a' + 26; else if (ch >= '0' && ch <= '9') v = ch - '0' + 52;
    else if (ch == '+' || ch == '-') v = 62; else if (ch == '/' || ch == '_') v = 63; else if (ch == '=' || ch == '\n' || ch == '\r') continue;
    else throw Error(TFGPU_ERR_CONFIG, "protobuf parser: DescFile is not base64");
    acc = (acc << 6) | (uint32_t)v; bits += 6;
    if (bits >= 8) { bits -= 8; o.push_back((char)((acc >> bits) & 0xFF)); }
  }
  return o;
}

}  // namespace ppd
}  // namespace tf

using namespace tf;
using namespace tf::ppd;

extern "C" {

int tfgpu_proto_parser_create(const tfgpu_proto_parser_config *c, tfgpu_proto_parser **out) {
  TF_API_BEGIN
  if (!c || !out || (c->desc_file_len && !c->desc_file) || (c->n_include_columns > 0 && !c->include_columns) || (c->n_primary_keys > 0 && !c->primary_keys))
    return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_create: null argument");
  Config g;
  g.desc.assign((const char *)c->desc_file, (size_t)c->desc_file_len);
  g.resource = c->desc_resource_name ? c->desc_resource_name : "";
  g.message = c->message_name ? c->message_name : "";
  for (int i = 0; i < c->n_include_columns; i++) g.include.emplace_back(c->include_columns[i].name ? c->include_columns[i].name : "", c->include_columns[i].required != 0);
  for (int i = 0; i < c->n_primary_keys; i++) g.keys.emplace_back(c->primary_keys[i] ? c->primary_keys[i] : "");
  g.pkg = c->package_type;
  g.null_keys = c->null_keys_allowed != 0; g.sys_cols = c->add_system_columns != 0; g.skip_dedup = c->skip_dedup_keys != 0;
  g.synth_keys = c->add_synthetic_keys != 0; g.nfe = c->not_fill_empty_fields != 0;
  *out = compile(g).release();
  return TFGPU_OK;
  TF_API_END
}

// ParserConfigProtoCommon / ParserConfigProtoLb as encoding/json writes them (Common has no AddSystemColumns / SkipDedupKeys / AddSyntheticKeys)
int tfgpu_proto_parser_create_json(const char *config_json, tfgpu_proto_parser **out) {
  TF_API_BEGIN
  if (!config_json || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_create_json: null argument");
  const Json j = Json::parse(config_json);
  if (j.type != Json::Obj) return tf::fail(TFGPU_ERR_CONFIG, "protobuf parser: the config is not a JSON object");
  Config g;
  g.desc = base64_decode(j.s("DescFile"));
  g.resource = j.s("DescResourceName"); g.message = j.s("MessageName");
  if (const Json *ic = j.get("IncludeColumns")) if (ic->type == Json::Arr) for (auto &e : ic->arr) g.include.emplace_back(e.s("Name"), e.flag("Required"));
  g.keys = j.strings("PrimaryKeys");
  const std::string pt = j.s("PackageType");
  g.pkg = pt == "PackageTypeProtoseq" ? TFGPU_PROTO_PKG_PROTOSEQ : pt == "PackageTypeRepeated" ? TFGPU_PROTO_PKG_REPEATED : pt == "PackageTypeSingleMsg" ? TFGPU_PROTO_PKG_SINGLE : -1;
  g.null_keys = j.flag("NullKeysAllowed"); g.sys_cols = j.flag("AddSystemColumns"); g.skip_dedup = j.flag("SkipDedupKeys");
  g.synth_keys = j.flag("AddSyntheticKeys"); g.nfe = j.flag("NotFillEmptyFields");
  *out = compile(g).release();
  return TFGPU_OK;
  TF_API_END
}

void tfgpu_proto_parser_free(tfgpu_proto_parser *h) { delete h; }

int tfgpu_proto_parser_schema(const tfgpu_proto_parser *h, tfgpu_schema **out) {
  TF_API_BEGIN
  if (!h || !out) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_schema: null argument");
  auto dup = [](const char *s) { char *r = (char *)std::malloc(std::strlen(s) + 1); std::strcpy(r, s); return r; };
  auto *rs = (tfgpu_schema *)std::calloc(1, sizeof(tfgpu_schema));
  rs->cols = (tfgpu_colschema *)std::calloc(std::max<size_t>(h->cols.size(), 1), sizeof(tfgpu_colschema));
  for (auto &c : h->cols) {
    tfgpu_colschema &o = rs->cols[rs->ncols++];
    o.name = dup(c.name.c_str()); o.dtype = c.dtype; o.flags = c.flags;
    o.path = dup(""); o.original_type = dup(""); o.table_schema = dup(""); o.table_name = dup(""); o.expression = dup(""); o.properties_json = nullptr;
  }
  *out = rs;
  return TFGPU_OK;
  TF_API_END
}

int tfgpu_proto_parser_info(const tfgpu_proto_parser *h, int32_t *code, const char **why, const char **message, int32_t *ncolumns) {
  TF_API_BEGIN
  if (!h) return tf::fail(TFGPU_ERR_INVALID, "tfgpu_proto_parser_info: null argument");
  if (code) *code = h->code;
  if (why) *why = h->why.c_str();
  if (message) *message = h->message.c_str();
  if (ncolumns) *ncolumns = (int32_t)h->cols.size();
  return TFGPU_OK;
  TF_API_END
}

}  // extern "C"
