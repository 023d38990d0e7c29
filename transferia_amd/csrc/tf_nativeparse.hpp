// tf_nativeparse.hpp — what the native parser's device half (tf_nativeparse.hip) and its host schema work (tf_nativeschema.cpp) share: the
// per-column conversion program of a group and the group's parsed identity.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "tf_common.hpp"

namespace tf {
namespace natp {

// what Restore does to the cells of one column (restore.go:20-256), as far as the device follows it
enum Op : uint8_t { OP_FALLBACK = 0, OP_INT, OP_JSONNUM, OP_BOOL, OP_STRING, OP_BASE64, OP_TIME, OP_INTERVAL, OP_ANY };
enum : uint8_t { F_ANY_STRING_OK = 1, F_ANY_PG_TIMESTAMP = 2, F_MYSQL_BIT = 4 };
struct ColOp { uint8_t op, dtype, flags, reason; };  // reason: OP_FALLBACK's tfgpu_native_reason (every cell of the column falls back, a null too)

// One distinct group key, read once on the host from the texts of the group's first item and kept by the key's hash.
struct GroupInfo {
  std::string ns, table, part, table_schema_json;
  std::vector<std::string> names, key_names, key_types;
  int names_form = 0;  // tfgpu_row_meta.names_form of every row
  struct SCol { std::string name, path, original_type, table_schema, table_name, expression, properties_json; int dtype = 0; uint32_t flags = 0; };
  std::vector<SCol> schema;
  std::vector<ColOp> ops;  // names.size() value columns, then key_names.size() OldKeys columns
  bool has_any = false;
  bool unreadable = false;  // the host does not read the group's texts (a ColSchema spelled in a way only encoding/json decides, a surrogate escape in a name)
  // the C views handed out by tfgpu_native_parsed_group / _group_schema (they point into the members above)
  std::vector<const char *> key_type_ptrs;
  std::vector<tfgpu_colschema> ccols;
  tfgpu_schema cschema{};
};
// The texts are the JSON values as the message spells them ("" = the member is absent or null).  Throws Error(TFGPU_ERR_UNSUPPORTED) for a group of
// more than 65 535 columns; a table_schema the host does not read makes every column OP_FALLBACK (TFGPU_NATIVE_SCHEMA_COLUMN).
std::shared_ptr<const GroupInfo> compile_group(const std::string &schema, const std::string &table, const std::string &part, const std::string &columnnames,
                                               const std::string &table_schema, const std::string &keynames, const std::string &keytypes);
int repr_of(const ColOp &op);  // the column's tfgpu_repr

}  // namespace natp
}  // namespace tf
