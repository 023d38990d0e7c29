// tf_protodesc.hpp — the compiled protobuf parser (tfgpu_proto_parser): what tf_protodesc.cpp makes of a config and its FileDescriptorSet, and what
// tf_protoparse.hip decodes by.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tf_pbfields.hpp"

namespace tf {
namespace ppd {

enum : uint32_t { PF_EXPLICIT = 1u /* HasPresence: message, proto3 optional, oneof member */, PF_FOREIGN = 2u /* outside the device subset */ };
constexpr int32_t MEMBER_EXPLICIT = 0x100;  // in DMember.ptype: a proto3 `optional` member (Has() is the wire's word, not value != 0)
constexpr int32_t MEMBER_TYPE = 0xFF;
enum { AUX_NONE = 0, AUX_PARTITION, AUX_OFFSET, AUX_IDX, AUX_CTIME, AUX_WTIME };

struct Col {
  std::string name;
  int dtype = 0;
  uint32_t flags = 0;  // TFGPU_COL_*
  int field = -1;      // index into `fields`, -1 for an aux column
  int aux = AUX_NONE;
  bool extra = false;  // an `_lb_extra_` column: no Required / NotFillEmptyFields check of its own (makeValues' second loop)
};

}  // namespace ppd
}  // namespace tf

struct tfgpu_proto_parser {
  int pkg = 0;
  bool not_fill_empty = false;
  int32_t wrapper_number = 0;                 // repeated: the wrapper's only field
  std::vector<tf::pbd::DField> fields;        // EVERY field of the event message, in declaration order
  std::vector<uint32_t> fflags;               // PF_* per field
  std::vector<tf::pbd::DMember> members;
  std::string names;
  std::vector<tf::ppd::Col> cols;             // the result schema, in order
  int32_t code = 0;                           // TFGPU_ROW_OK / TFGPU_ROW_HOST_FALLBACK
  std::string why, message;                   // message: the event message's full name
};
