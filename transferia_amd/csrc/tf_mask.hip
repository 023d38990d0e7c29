// tf_mask.hip — a4 mask_field: hex(HMAC_SHA256(salt, SerializeToString(v))) — hmac_hasher.go:29-33.  INT32-ALU bound (2–3 SHA-256
// compressions per value).  A unit of its own: profiles/pmc_traffic.json stamps the kernel's counters against this file alone.
#include "tf_plan.hpp"
#include "tf_rows.hpp"
#include "tf_devrow.hpp"
#include "tf_emit.hpp"

namespace tf {
__constant__ uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) { return __builtin_rotateright32(x, n); }

__device__ __forceinline__ void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      uint32_t s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
      uint32_t s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
      w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
    }
    uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[i] + w[i & 15];
    uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

struct MaskParams {
  DCol col;
  uint32_t ipad[8], opad[8];
  int64_t nrows;
  uint8_t *out;  // nrows * 64 hex bytes
  uint32_t *offsets;  // nrows + 1 Arrow offsets of the digests: 64 * r
  const int32_t *sel;  // non-null: output row r hashes the column's row sel[r] (the batch's rows are still a selection)
};

// The text of an integer (or "<nil>") is at most 21 bytes: built in three registers as a little-endian byte string — the emitters of
// tf_emit.hpp hand over eight digits per word — it becomes the one message block of the inner hash with six byte swaps, instead of a
// scratch byte buffer read back byte by byte into a dynamically indexed w[] (that detour was a fifth of the kernel's instructions).
struct Text24 {
  uint64_t t0 = 0, t1 = 0, t2 = 0; uint32_t n = 0;
  __device__ __forceinline__ void put_word(uint64_t w, uint32_t k) {  // the low k (1..8) bytes of w, the rest zero
    const uint32_t at = n & 7u, sh = at * 8, seg = n >> 3;
    const uint64_t lo = w << sh, hi = (w >> 1) >> (63 - sh);            // (w >> 1) >> 63 == 0 when at == 0
    if (seg == 0) { t0 |= lo; t1 |= hi; } else if (seg == 1) { t1 |= lo; t2 |= hi; } else t2 |= lo;
    n += k;
  }
  __device__ __forceinline__ void put(uint32_t c) { put_word(c & 0xFFu, 1); }
};
__device__ __forceinline__ bool mask_small_int(const DCol &c, int64_t r, Text24 &s) {  // false: not an integer column
  if (!is_valid(c, r)) { s.put_word(0x3E6C696E3Cull /* "<nil>" */, 5); return true; }
  switch (c.repr) {
    case TFGPU_R_INT8: emit_i64(s, ((const int8_t *)c.values)[r]); return true;
    case TFGPU_R_INT16: emit_i64(s, ((const int16_t *)c.values)[r]); return true;
    case TFGPU_R_INT32: emit_i64(s, ((const int32_t *)c.values)[r]); return true;
    case TFGPU_R_INT64: emit_i64(s, ((const int64_t *)c.values)[r]); return true;
    case TFGPU_R_UINT8: emit_u64(s, ((const uint8_t *)c.values)[r]); return true;
    case TFGPU_R_UINT16: emit_u64(s, ((const uint16_t *)c.values)[r]); return true;
    case TFGPU_R_UINT32: emit_u64(s, ((const uint32_t *)c.values)[r]); return true;
    case TFGPU_R_UINT64: emit_u64(s, ((const uint64_t *)c.values)[r]); return true;
    default: return false;
  }
}

__global__ void __launch_bounds__(256) mask_hmac_kernel(MaskParams p) {
  const int64_t ro = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // the row written
  if (ro >= p.nrows) return;
  const int64_t r = p.sel ? (int64_t)p.sel[ro] : ro;                   // the row read
  uint32_t st[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = p.ipad[i];
  const bool small_int = p.col.repr >= TFGPU_R_INT8 && p.col.repr <= TFGPU_R_UINT64;  // (a property of the column: a scalar branch)
  if (small_int) {
    Text24 s;
    mask_small_int(p.col, r, s);
    const uint32_t len = s.n;
    s.put_word(0x80, 1);  // the padding byte right behind the text; the block's tail is zeros and the bit length (len <= 21 < 56)
    w[0] = __builtin_bswap32((uint32_t)s.t0); w[1] = __builtin_bswap32((uint32_t)(s.t0 >> 32));
    w[2] = __builtin_bswap32((uint32_t)s.t1); w[3] = __builtin_bswap32((uint32_t)(s.t1 >> 32));
    w[4] = __builtin_bswap32((uint32_t)s.t2); w[5] = __builtin_bswap32((uint32_t)(s.t2 >> 32));
#pragma unroll
    for (int i = 6; i < 15; i++) w[i] = 0;
    w[15] = (64 + len) * 8;
    sha256_compress(st, w);
  } else {
  uint8_t buf[64];
  const uint8_t *ext;
  int len = serialize_small(p.col, r, buf, &ext);
  // inner hash: the ipad block is already absorbed; stream the message
  int off = 0;
  uint64_t bits = (uint64_t)(64 + len) * 8;
  bool pad_done = false, len_done = false;
  while (!len_done) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    int take = len - off; if (take > 64) take = 64; if (take < 0) take = 0;
    for (int i = 0; i < take; i++) {
      uint32_t b = ext ? ext[off + i] : buf[off + i];
      w[i >> 2] |= b << (24 - 8 * (i & 3));
    }
    off += take;
    if (take < 64 && !pad_done) { w[take >> 2] |= 0x80u << (24 - 8 * (take & 3)); pad_done = true; if (take < 56) { w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; len_done = true; } }
    else if (pad_done) { w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; len_done = true; }
    sha256_compress(st, w);
  }
  }
  // outer hash: opad block absorbed; message = 32-byte inner digest
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = st[i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) w[i] = 0;
  w[15] = (64 + 32) * 8;
  uint32_t so[8];
#pragma unroll
  for (int i = 0; i < 8; i++) so[i] = p.opad[i];
  sha256_compress(so, w);
  // hex.EncodeToString: 64 lower-case hex chars, stored as 4 x 16 bytes
  uint4 *dst = reinterpret_cast<uint4 *>(p.out + ro * 64);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // 2 bytes of digest → 4 hex chars (little-endian packing of the output bytes)
      uint32_t word = so[q * 2 + (k >> 1)];
      uint32_t half = (k & 1) ? (word & 0xFFFF) : (word >> 16);
      uint32_t n0 = (half >> 12) & 15, n1 = (half >> 8) & 15, n2 = (half >> 4) & 15, n3 = half & 15;
      auto hx = [](uint32_t n) { return n + (n < 10 ? '0' : 'a' - 10); };
      o[k] = hx(n0) | hx(n1) << 8 | hx(n2) << 16 | hx(n3) << 24;
    }
    dst[q] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  // every digest is 64 bytes: the column's offsets need no launch of their own (the last row's thread also writes offsets[nrows])
  p.offsets[ro] = (uint32_t)(ro * 64);
  if (ro == p.nrows - 1) p.offsets[p.nrows] = (uint32_t)(p.nrows * 64);
}


// what apply_mask refuses for a whole batch, before anything is computed
void mask_precheck(const tfgpu_plan &p, const tfgpu_dbatch &in) {  // (`in`: the caller's own copy, as apply_plan's)
  for (auto &c : (in.pending ? in.pending->src->cols : in.cols)) {
    if (!p.mask_has(c.name)) continue;
    bool done = false;
    for (auto &r : in.replaced) if (r.name == c.name) done = true;  // (masked already: a string, always serializable)
    if (done) continue;
    require_serializable(c, "mask_field");
    if ((uint64_t)in.nrows * 64 > 0xFFFFFFFFull) throw Error(TFGPU_ERR_UNSUPPORTED, "mask_field: batch too large for 32-bit offsets; split the batch by rows");
  }
}

// `in`: a batch nobody else changes meanwhile (apply_plan)
std::unique_ptr<tfgpu_dbatch> apply_mask(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  hipStream_t st = ctx().stream;
  // The batch's rows may still be a selection over the batch a filter_rows read (tfgpu_dbatch::pending): the hash reads the masked
  // column's kept rows THROUGH the selection and its 64-byte digests are the first column of the result that exists densely —
  // the other hundred columns stay ungathered until somebody reads them.
  const tfgpu_dbatch &from = in.pending ? *in.pending->src : in;
  const int32_t *sel = in.pending ? ptr<int32_t>(in.pending->sel) : nullptr;
  auto replaced_at = [&](const std::string &name) -> int { for (size_t i = 0; i < in.replaced.size(); i++) if (in.replaced[i].name == name) return (int)i; return -1; };
  materialize_where(from, [&](const DColumn &c) { return p.mask_has(c.name) && replaced_at(c.name) < 0; });
  auto out = shallow_copy(in);  // (behind materialize: a text column's offsets may have been made just now, and the copy's columns are read below)
  for (auto &sc : out->schema) if (p.mask_has(sc.first)) sc.second = TFGPU_T_UTF8;  // hmac_hasher.go:35-46
  const int64_t n = in.nrows;
  auto mask_one = [&](const DColumn &c, const int32_t *through) {
    require_serializable(c, "mask_field");
    if ((uint64_t)n * 64 > 0xFFFFFFFFull) throw Error(TFGPU_ERR_UNSUPPORTED, "mask_field: batch too large for 32-bit offsets; split the batch by rows");
    DColumn o;
    o.name = c.name; o.dtype = TFGPU_T_UTF8; o.repr = TFGPU_R_STRING;
    o.data_len = (uint64_t)n * 64;
    o.data = dalloc(o.data_len);
    o.offsets = dalloc((size_t)(n + 1) * 4);
    MaskParams mp;
    mp.col = dcol_of(c);
    std::memcpy(mp.ipad, p.ipad_state, sizeof mp.ipad);
    std::memcpy(mp.opad, p.opad_state, sizeof mp.opad);
    mp.nrows = n; mp.out = ptr<uint8_t>(o.data); mp.offsets = ptr<uint32_t>(o.offsets); mp.sel = through;
    {
      KernelTimer t("mask_hmac_sha256", n);
      if (n) mask_hmac_kernel<<<grid_for(n, 256), 256, 0, st>>>(mp);
    }
    if (!n) TF_HIP(hipMemsetAsync(o.offsets->p, 0, 4, st));  // (an empty batch: offsets[0] alone)
    return o;
  };
  if (!in.pending) {
    for (auto &c : out->cols) if (p.mask_has(c.name)) {
      // HmacHasher.Apply walks the item's OWN ColumnNames (hmac_hasher.go:56-63): a row that does not list the column is left as it is — the digest
      // the kernel wrote for it is nobody's, the cell stays ABSENT (and reads nil)
      const Buf ab = c.absent;
      c = mask_one(c, nullptr);
      if (ab) { c.absent = ab; c.validity = validity_minus_absent(nullptr, ab, n); }
    }
    return out;
  }
  for (auto &c : from.cols) {
    if (!p.mask_has(c.name)) continue;
    const int ri = replaced_at(c.name);
    if (ri >= 0) out->replaced[(size_t)ri] = mask_one(in.replaced[(size_t)ri], nullptr);  // (already dense over the kept rows)
    else out->replaced.push_back(mask_one(c, sel));
  }
  return out;
}
}  // namespace tf
