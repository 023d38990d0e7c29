// tf_intern.hpp — what the device groupings share (tf_tablesplit.hip: rows by generated table name; tf_nativeparse.hip: ChangeItems by group key):
// the 2 x 64-bit hashing sink, and the steps behind an open-addressing table that has given every item the slot of its key — first-appearance
// ids from an atomicMin per slot, one scan, and the run heads of the sorted ids.  The table itself (the probe loop and what "equal key" means
// under an equal hash) stays with each user: it is the part that differs.
//
// The kernels are `static`: each unit that includes this header carries its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tf {

static constexpr uint32_t NOROW = 0xFFFFFFFFu;

struct NameHash {
  uint64_t h1 = 0x452821E638D01377ull, h2 = 0xBE5466CF34E90C6Cull, acc = 0, len = 0;
  uint32_t k = 0;
  __device__ __forceinline__ void mix(uint64_t w) {
    h1 = (h1 ^ w) * 0x9E3779B97F4A7C15ull; h1 ^= h1 >> 32;
    h2 = (((h2 << 31) | (h2 >> 33)) ^ w) * 0xC2B2AE3D27D4EB4Full; h2 ^= h2 >> 29;
  }
  __device__ __forceinline__ void put(uint32_t c) {
    acc |= (uint64_t)(c & 0xFFu) << (8 * k); len++;
    if (++k == 8) { mix(acc); acc = 0; k = 0; }
  }
  __device__ __forceinline__ void finish() {
    mix(acc); mix(len);
    h1 ^= h1 >> 33; h1 *= 0xFF51AFD7ED558CCDull; h1 ^= h1 >> 33;
    h2 ^= h2 >> 33; h2 *= 0xC4CEB9FE1A85EC53ull; h2 ^= h2 >> 33;
  }
};

// ---- first-appearance ids ---------------------------------------------------------------------------------------------------
// slotof[r]: the slot of item r's key.  first[slot] (NOROW before the first launch, or some item of the slot) becomes the slot's lowest item;
// `keep` (optional) leaves items out: they take no part and get no id.
static __global__ void __launch_bounds__(256) intern_first(const uint32_t *__restrict__ slotof, const uint32_t *__restrict__ keep, int64_t n, uint32_t *first) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || (keep && !keep[r])) return;
  uint32_t *o = &first[slotof[r]];
  // (most items come after the item that claimed their slot: with few keys the atomics of a million items on a handful of addresses were the longest step)
  if (__hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)r) atomicMin(o, (uint32_t)r);
}
static __global__ void __launch_bounds__(256) intern_flag(const uint32_t *__restrict__ slotof, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ first, int64_t n,
                                                          uint32_t *__restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) flag[r] = (!keep || keep[r]) && first[slotof[r]] == (uint32_t)r ? 1u : 0u;
}
// rank = the exclusive scan of the flags (n + 1 entries): id[r] = the rank of its slot's first item (`none` for an item left out), reps[id] = that
// item, idx[r] = r (the values of the sort that groups the items)
static __global__ void __launch_bounds__(256) intern_ids(const uint32_t *__restrict__ slotof, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ first,
                                                         const uint32_t *__restrict__ rank, int64_t n, uint32_t none, uint32_t *__restrict__ id, uint32_t *__restrict__ reps,
                                                         uint32_t *__restrict__ idx) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  id[r] = (!keep || keep[r]) ? rank[first[slotof[r]]] : none;
  if (rank[r + 1] != rank[r]) reps[rank[r]] = (uint32_t)r;
  idx[r] = (uint32_t)r;
}
// run heads of the sorted ids: start[id] = where its run begins
static __global__ void __launch_bounds__(256) intern_heads(const uint32_t *__restrict__ sid, int64_t n, uint32_t *__restrict__ start) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n && (q == 0 || sid[q] != sid[q - 1])) start[sid[q]] = (uint32_t)q;
}

}  // namespace tf
