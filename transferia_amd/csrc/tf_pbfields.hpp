// tf_pbfields.hpp — the compiled field table of a protobuf message, as the device walks it (tf_pbwire.hpp).  Plain structs: the host compilers
// (tf_protoschema.cpp from .proto text, tf_protodesc.cpp from a FileDescriptorSet) fill them, the kernels read them.
#pragma once
#include <cstdint>

namespace tf {
namespace pbd {

struct DField { int32_t number, ptype, mem_off, nmem; uint32_t name_off, name_len; int32_t repeated, oneof; };  // members / names: offsets into the tables; repeated: 1 list, 2 map
struct DMember { int32_t number, ptype; uint32_t name_off, name_len; };

}  // namespace pbd
}  // namespace tf
