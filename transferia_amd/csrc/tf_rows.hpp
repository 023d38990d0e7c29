// tf_rows.hpp — the rows of a device batch (tf_rows.hip): what the ingest units and the transformers call to move them.
// The selection → dense hand-over (dense, dense_locked, snapshot, has_absent) is declared in tf_common.hpp.
#pragma once
#include "tf_common.hpp"

namespace tf {
std::unique_ptr<tfgpu_dbatch> gather_rows(const tfgpu_dbatch &in, const Buf &sel, int64_t m);  // all columns of `in` through sel (int32[m]: rows of `in`)
// keep flags (uint32 0/1, n+1 slots) → compacted batch; identity (shared buffers) if all are kept; syncs.  lazy: the kept rows are handed
// on as a selection over `in` (tfgpu_dbatch::pending) — the row filters; compact_rows is the dense form under its older name.
std::unique_ptr<tfgpu_dbatch> compact(const tfgpu_dbatch &in, Buf keep, bool lazy = false);
std::unique_ptr<tfgpu_dbatch> compact_rows(const tfgpu_dbatch &in, Buf keep);
std::unique_ptr<tfgpu_dbatch> partition_rows(const tfgpu_dbatch &in, int nparts, int64_t *counts);  // rows grouped by part_id, order kept inside a part
void refuse_absent(const tfgpu_dbatch &b);  // throws TFGPU_ERR_UNSUPPORTED ("ABSENT cells") when has_absent(b)
void wait_dense(const tfgpu_dbatch &b);     // a dense batch another lane gathered: this lane's stream waits for that gather (else nothing)
}  // namespace tf
