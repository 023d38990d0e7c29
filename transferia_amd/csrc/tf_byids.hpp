// tf_byids.hpp — the allowed-ID tables of filter_rows_by_ids, as the plan builds them on the host (tf_plan.cpp) and the kernel
// probes them (tf_byids.hip): one image, read as 32-bit words from HBM or from LDS.
//
//   words [0, nlen)                    the distinct ID lengths, ascending
//   words [nlen, nlen + 3 * cap)       `cap` (a power of two, at least twice the IDs) open-addressing slots of three words
//                                      {key, off, len}: key = byids_key(FNV-1a of the ID's bytes, len), off = where the ID's bytes
//                                      start in the byte area, len == BYIDS_EMPTY in a free slot; linear probing from byids_home(key)
//   bytes from word nlen + 3 * cap     the distinct IDs' bytes, back to back
//
// FNV-1a extends by one byte at a time, so one walk over the first max_len bytes of a cell passes the hash of every prefix.
#pragma once
#include <cstdint>
#include <vector>

#include "tf_common.hpp"

namespace tf {

constexpr uint32_t BYIDS_FNV_INIT = 2166136261u, BYIDS_FNV_PRIME = 16777619u, BYIDS_EMPTY = 0xFFFFFFFFu;
// The table is copied into LDS, once per workgroup, when its image fits this budget; else the lanes probe it where it lies (a table of a few MB
// stays in L2 / the Infinity Cache).  16 KiB per workgroup of 256 lanes: eight workgroups — the CU's 32 waves, the eight waves per SIMD the
// kernel is bound to (__launch_bounds__(256, 8)) — take 128 KiB of the CU's 160 KiB, so the copy is not what limits occupancy.  The registers
// must allow eight waves as well: at most 64 VGPRs and at most 96 allocated SGPRs (next_free_sgpr + 6 for VCC, FLAT_SCRATCH, XNACK_MASK; left
// to itself hipcc took 112 and ran seven).  tests/test_byids_resources.py holds the kernel to all three from its descriptors.
constexpr uint32_t BYIDS_LDS_BUDGET = 16u << 10;

__host__ __device__ __forceinline__ uint32_t byids_step(uint32_t h, uint32_t byte) { return (h ^ byte) * BYIDS_FNV_PRIME; }
__host__ __device__ __forceinline__ uint32_t byids_key(uint32_t h, uint32_t len) { return h ^ (len * 0x9E3779B1u); }
__host__ __device__ __forceinline__ uint32_t byids_home(uint32_t key, uint32_t mask) { return (key ^ (key >> 15)) & mask; }

struct ByIdsTable {
  std::vector<uint32_t> image;  // the words above, the byte area padded to a whole word
  uint32_t nlen = 0, cap = 0;   // distinct lengths; slots
  uint64_t id = 0;              // names the image in a lane's table cache (Context::plan_tables): never reused
};

}  // namespace tf
