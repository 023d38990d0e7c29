// tf_ingest.hpp — what the ingest entries share on the host (tf_ingest.cpp; no kernels): between the C ABI and the first launch the input
// bytes and the message starts in HBM; between the last launch and the returned batch the two-pass text-column finish, the validity block
// and the rows that go back to the host.  The caller holds the lane's mutex; everything is enqueued on the lane's stream.
#pragma once
#include "tf_common.hpp"

namespace tf {

// The input bytes of a batch in HBM.  Host memory is copied into a block of our own (`keep`) with 64 zero bytes behind it; device memory
// is used where it is and must be 16-byte aligned.  Throws "<who>: batch must be < 4 GiB (32-bit offsets)" / "<who>: device buffer must
// be 16-byte aligned".  A pageable source is fenced by the caller's next sync().
const uint8_t *stage_input(const void *bytes, uint64_t len, int mem, const char *who, Buf &keep);
// the same, always a copy of our own (the scanners and the segmented copy read whole aligned words past the end)
const uint8_t *stage_bytes(const void *src, uint64_t len, int mem, Buf &keep);
// an array of the batch in HBM: a host array is copied, a device array is used where it is
template <class T> const T *stage_array(const void *src, size_t count, int mem, Buf &keep) {
  if (!src) return nullptr;
  if (mem == TFGPU_MEM_DEVICE) return reinterpret_cast<const T *>(src);
  keep = dalloc(count * sizeof(T) + 16);
  h2d(keep->p, src, count * sizeof(T));
  return ptr<T>(keep);
}

// The message starts narrowed to u32, nmsg + 1 of them, on both sides.  The entry keeps the struct until it returns: `host` is the pageable
// source of the upload.
struct MessageStarts {
  std::vector<uint32_t> host;
  Buf dev;
  int64_t nmsg() const { return (int64_t)host.size() - 1; }
};
// Without `msgs` the buffer is one message.  Throws "<who>: message offsets must be ascending and inside the buffer"; msgs->nmsg >= 0 and a
// non-null msgs->start (when nmsg > 0) are the caller's checks.
MessageStarts stage_message_starts(const tfgpu_messages *msgs, uint64_t len, const char *who);

// 32-bit offsets hold less than 4 GiB per column.  TFGPU_TEST_TEXT_LIMIT (tests only, read once) lowers the bound so that the refusal can be
// exercised without a 4 GiB batch.
bool text_total_exceeds(uint64_t bytes);

// The text columns of a batch while they are built: one zeroed block of `nseg` segments, seg_len + 1 entries each.  The length kernels write
// seg(i)[r]; scan() turns every segment into offsets in place and brings the totals to the host; the caller sizes `data` from total(i).
class TextSegments {
 public:
  TextSegments() = default;
  TextSegments(int nseg, int64_t seg_len) : TextSegments(nseg, seg_len, dalloc_zero(bytes(nseg, seg_len))) {}
  TextSegments(int nseg, int64_t seg_len, Buf zeroed) : block_(std::move(zeroed)), nseg_(nseg), len_(seg_len) {}  // `zeroed`: bytes(nseg, seg_len) of a larger zeroed block
  static int64_t stride(int64_t seg_len) { return ((seg_len + 1 + 3) / 4) * 4; }
  static size_t bytes(int nseg, int64_t seg_len) { return (size_t)std::max(nseg, 1) * (size_t)stride(seg_len) * 4 + 16; }
  int64_t stride() const { return stride(len_); }
  uint32_t *seg(int i) const { return ptr<uint32_t>(block_) + (int64_t)i * stride(); }
  Buf offsets(int i) const { return subbuf(block_, (size_t)i * (size_t)stride() * 4, (size_t)(len_ + 1) * 4); }
  // Enqueues: with sum64 the segments' sums in 64 bits (the 32-bit scan wraps at 4 GiB: callers that refuse such a column), the segmented
  // scan in place, one read-back of the totals.  Does not sync.
  void scan(bool sum64);
  uint64_t total(int i) const;  // after the caller's next sync(); 0 when nothing was scanned

 private:
  Buf block_;
  int nseg_ = 0;
  int64_t len_ = 0;
  bool sum64_ = false;
  const uint32_t *totals_ = nullptr;
};

// The columns' validity bitmaps as views of one block cleared by one fill (a fill per column was two dispatches each)
struct ValidityBlock {
  Buf all;
  size_t used, vbytes;  // a column's bitmap (whole 64-bit words and one more), and its 64-byte-rounded slot
  ValidityBlock(int ncols, int64_t nrows)
      : used((size_t)((std::max<int64_t>(nrows, 1) + 63) / 64) * 8 + 8), vbytes((used + 63) & ~(size_t)63) { all = dalloc_zero((size_t)std::max(ncols, 1) * vbytes); }
  Buf col(int j) const { return subbuf(all, (size_t)j * vbytes, used); }
};

// Rows the device marked for the host (host_rows[r] != 0): returns row_src[r] of each in row order and, when there are any, compacts `batch`
// to the other rows.  One flag word comes down first; the per-row marks only when it is set.  Syncs.
std::vector<uint32_t> split_host_rows(std::unique_ptr<tfgpu_dbatch> &batch, const Buf &host_rows, const Buf &row_src, int64_t nrows);

}  // namespace tf
