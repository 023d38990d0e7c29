// tf_utf8.hpp — utf8.Valid over a byte range in HBM, shared by the raw_to_table validator (tf_rawtable.hip) and the protobuf parser's proto3
// string check (tf_protoparse.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tf_devparse.hpp"

namespace tf {

// bytes [pos, stop) of a message that ends at `end` (stop <= end): every sequence that STARTS before stop is validated whole, its continuation bytes
// read up to `end` and never beyond it
__device__ __forceinline__ bool utf8_valid_range(MemBytes &rd, uint32_t pos, const uint32_t stop, const uint32_t end) {
  const uint64_t HI = 0x8080808080808080ull;
  while (pos < stop) {
    if (pos + 8 <= stop) {  // eight ASCII bytes a step
      const uint64_t hi = rd.word(pos) & HI;
      if (!hi) { pos += 8; continue; }
      pos += (uint32_t)(__ffsll((long long)hi) - 1) >> 3;
    }
    const uint32_t c = rd.at(pos);
    if (c < 0x80) { pos++; continue; }
    uint32_t need = 0, lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c >= 0xE0 && c <= 0xEF) { need = 2; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { need = 3; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    if (!need || end - pos <= need) return false;  // a continuation byte, C0 / C1, F5..FF, or a sequence cut short by the message's end
    const uint32_t d1 = rd.at(pos + 1);
    if (d1 < lo || d1 > hi) return false;
    for (uint32_t q = 2; q <= need; q++) { const uint32_t d = rd.at(pos + q); if (d < 0x80 || d > 0xBF) return false; }
    pos += need + 1;
  }
  return true;
}

}  // namespace tf
