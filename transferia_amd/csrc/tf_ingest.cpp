// tf_ingest.cpp — the host code the ingest entries share (tf_ingest.hpp).  No kernels: the scans and the row compaction live in tf_scan.hip and
// tf_rows.hip.
#include "tf_ingest.hpp"

#include <cstdlib>

#include "tf_rows.hpp"

namespace tf {

const uint8_t *stage_input(const void *bytes, uint64_t len, int mem, const char *who, Buf &keep) {
  if (len >= 0xFFFFFFF0ull) throw Error(TFGPU_ERR_UNSUPPORTED, std::string(who) + ": batch must be < 4 GiB (32-bit offsets)");
  if (mem != TFGPU_MEM_HOST) {
    if (reinterpret_cast<uintptr_t>(bytes) & 15) throw Error(TFGPU_ERR_INVALID, std::string(who) + ": device buffer must be 16-byte aligned");
    return static_cast<const uint8_t *>(bytes);
  }
  keep = dalloc(len + 64);
  h2d(keep->p, bytes, len);
  TF_HIP(hipMemsetAsync((char *)keep->p + len, 0, 64, ctx().stream));
  return ptr<uint8_t>(keep);
}

const uint8_t *stage_bytes(const void *src, uint64_t len, int mem, Buf &keep) {
  keep = dalloc((size_t)len + 64);
  if (mem == TFGPU_MEM_DEVICE) d2d(keep->p, src, (size_t)len); else h2d(keep->p, src, (size_t)len);
  TF_HIP(hipMemsetAsync((char *)keep->p + len, 0, 64, ctx().stream));
  return ptr<uint8_t>(keep);
}

MessageStarts stage_message_starts(const tfgpu_messages *msgs, uint64_t len, const char *who) {
  MessageStarts s;
  const int64_t nmsg = msgs ? msgs->nmsg : 1;
  s.host.assign((size_t)nmsg + 1, 0u);
  if (!msgs) s.host[1] = (uint32_t)len;
  else if (msgs->start)  // (null only with nmsg == 0)
    for (int64_t m = 0; m <= nmsg; m++) {
      if (msgs->start[m] > len || (m && msgs->start[m] < msgs->start[m - 1])) throw Error(TFGPU_ERR_INVALID, std::string(who) + ": message offsets must be ascending and inside the buffer");
      s.host[(size_t)m] = (uint32_t)msgs->start[m];
    }
  s.dev = dalloc(s.host.size() * 4 + 16);
  h2d(s.dev->p, s.host.data(), s.host.size() * 4);
  return s;
}

bool text_total_exceeds(uint64_t bytes) {
  static const uint64_t limit = [] { const char *e = std::getenv("TFGPU_TEST_TEXT_LIMIT"); return e && *e ? (uint64_t)std::strtoull(e, nullptr, 10) : 0xFFFFFFF0ull; }();
  return bytes >= limit;
}

void TextSegments::scan(bool sum64) {
  if (nseg_ <= 0) return;
  sum64_ = sum64;
  Buf tot64;
  if (sum64) {
    tot64 = dalloc_zero((size_t)nseg_ * 8 + 16);
    sum_u32_segments_u64(seg(0), len_, nseg_, stride(), ptr<unsigned long long>(tot64));
  }
  exclusive_scan_u32_segments(seg(0), len_, nseg_, stride());
  totals_ = sum64 ? d2h_u32(tot64->p, (size_t)nseg_ * 2) : segment_totals_to_host(seg(0), len_, nseg_, stride());
}

uint64_t TextSegments::total(int i) const {
  if (!totals_) return 0;
  return sum64_ ? (uint64_t)totals_[2 * i] | (uint64_t)totals_[2 * i + 1] << 32 : totals_[i];
}

std::vector<uint32_t> split_host_rows(std::unique_ptr<tfgpu_dbatch> &batch, const Buf &host_rows, const Buf &row_src, int64_t nrows) {
  std::vector<uint32_t> src;
  const uint32_t *hflag = any_nonzero_to_host(ptr<uint32_t>(host_rows), nrows);
  sync();
  if (!*hflag) return src;
  std::vector<uint32_t> hr((size_t)nrows), rs((size_t)nrows), keepv((size_t)nrows + 1, 0u);
  d2h(hr.data(), host_rows->p, (size_t)nrows * 4); d2h(rs.data(), row_src->p, (size_t)nrows * 4);
  sync();
  for (int64_t r = 0; r < nrows; r++) { if (hr[(size_t)r]) src.push_back(rs[(size_t)r]); else keepv[(size_t)r] = 1u; }
  if (src.empty()) return src;
  Buf dk = dalloc(keepv.size() * 4 + 16);
  h2d(dk->p, keepv.data(), keepv.size() * 4);
  batch = compact_rows(*batch, dk);  // syncs: keepv is consumed
  return src;
}

}  // namespace tf
