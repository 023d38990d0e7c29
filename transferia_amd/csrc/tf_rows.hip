// tf_rows.hip — the rows of a device batch: keep flags → selection → gather of every column, the selection → dense hand-over
// between lanes, the local half of the hash partition.  What the ingest units and the transformers call (tf_rows.hpp, tf_common.hpp).
#include <chrono>
#include <thread>

#include "tf_rows.hpp"
#include "tf_devrow.hpp"
#include "tf_segcopy.hpp"
#include "tf_textview.hpp"

namespace tf {
__global__ void __launch_bounds__(256) build_selection_kernel(const uint32_t *__restrict__ keep_scan, int64_t n, int32_t *__restrict__ sel) {
  // keep_scan[i] = exclusive prefix of keep; row i kept iff keep_scan[i+1] != keep_scan[i]
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t a = keep_scan[i], b = keep_scan[i + 1];
  if (a != b) sel[a] = (int32_t)i;
}

// All fixed-width arrays of a batch (values, nanos, kind, part_id, src_row) in ONE launch: lane = output
// row, wave-uniform loop over the arrays, so every store is coalesced and the selection vector is read once.
struct GFix { const void *in; void *out; int32_t width; int32_t pad; };
// the arrays arrive sorted by element width (n1 of one byte, then n2, n4, n8), so every loop below has one element type and
// no branch between its loads: a lane requests eight arrays' values before it stores the first — one wait for memory per
// eight arrays instead of one per array (the kernel used to be a chain of 78 round trips per lane)
template <class T> __device__ __forceinline__ void gather_run(const GFix *__restrict__ a, int lo, int hi, int32_t s, int64_t k) {
  constexpr int U = 8;
  int i = lo;
  for (; i + U <= hi; i += U) {
    T v[U];
#pragma unroll
    for (int q = 0; q < U; q++) v[q] = TF_GLOBAL_PTR(const T, a[i + q].in)[s];
#pragma unroll
    for (int q = 0; q < U; q++) TF_GLOBAL_PTR(T, a[i + q].out)[k] = v[q];
  }
  for (; i < hi; i++) TF_GLOBAL_PTR(T, a[i].out)[k] = TF_GLOBAL_PTR(const T, a[i].in)[s];
}
__global__ void __launch_bounds__(256) gather_fixed_all(const GFix *__restrict__ a, int n1, int n2, int n4, int n8, uint32_t *__restrict__ ident, const int32_t *__restrict__ sel, int64_t m) {
  int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int32_t s = sel[k];
  if (ident) ident[k] = (uint32_t)s;  // src_row of a batch that had none: the identity
  gather_run<uint8_t>(a, 0, n1, s, k);
  gather_run<uint16_t>(a, n1, n1 + n2, s, k);
  gather_run<uint32_t>(a, n1 + n2, n1 + n2 + n4, s, k);
  gather_run<uint64_t>(a, n1 + n2 + n4, n1 + n2 + n4 + n8, s, k);
}
// validity bitmaps of all columns in one launch: one thread per output byte (8 rows), blockIdx.y = bitmap
struct GBit { const uint8_t *in; uint8_t *out; };
__global__ void __launch_bounds__(256) gather_bitmap_all(const GBit *__restrict__ a, const int32_t *__restrict__ sel, int64_t m) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b * 8 >= m) return;
  const GBit g = a[blockIdx.y];
  uint32_t v = 0;
  for (int j = 0; j < 8; j++) { int64_t k = b * 8 + j; if (k < m) { int32_t s = sel[k]; v |= ((g.in[s >> 3] >> (s & 7)) & 1u) << j; } }
  g.out[b] = (uint8_t)v;
}
// Var-width columns: lengths of all columns in one launch (segmented layout, then one segmented scan),
// payload bytes of all columns in one launch.
// fstart != null: a late-materialised text column (TextView) — in_data is the SOURCE text and a kept cell is fetched from
// in_data + fstart[row]; cells that are not a plain byte range are left zero-filled for gather_text_special.
struct GVar { const uint32_t *in_off; const uint8_t *in_data; uint32_t *out_off; uint8_t *out_data; const uint32_t *fstart; uint32_t quote, jsonnum, has_special; };
__global__ void __launch_bounds__(256) gather_len_all(const GVar *__restrict__ v, int nv, const int32_t *__restrict__ sel, int64_t m) {
  int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int32_t s = sel[k];
  constexpr int U = 8;  // eight columns' offsets requested per wait (as in gather_fixed_all)
  int i = 0;
  for (; i + U <= nv; i += U) {
    uint32_t a[U], b[U];
#pragma unroll
    for (int q = 0; q < U; q++) { const uint32_t *off = TF_GLOBAL_PTR(const uint32_t, v[i + q].in_off); a[q] = off[s]; b[q] = off[s + 1]; }
#pragma unroll
    for (int q = 0; q < U; q++) TF_GLOBAL_PTR(uint32_t, v[i + q].out_off)[k] = b[q] - a[q];
  }
  for (; i < nv; i++) { const uint32_t *off = v[i].in_off; v[i].out_off[k] = off[s + 1] - off[s]; }
}
// Payload bytes of the kept rows, destination-centric (tf_segcopy.hpp): blockIdx.y = column, blockIdx.x = a run of
// 256 * RPT kept rows, whose cells are contiguous in the output and are fetched through the selection vector.
template <int RPT> __global__ void __launch_bounds__(256) gather_bytes_all(const GVar *__restrict__ v, const int32_t *__restrict__ sel, int64_t m) {
  __shared__ uint32_t doff[256 * RPT + 1];
  __shared__ uint32_t soff[256 * RPT];
  const GVar g = v[blockIdx.y];
  auto so = [&](int64_t k) {
    const int32_t s = sel[k];
    if (!g.fstart) return g.in_off[s];
    const uint32_t f = g.fstart[s];
    return cell_plain(f) ? f : SEG_NONE;
  };
  segcopy_run<RPT>(g.out_off, m, (int64_t)blockIdx.x * 256 * RPT, g.in_data, g.out_data, so, doff, soff);
}
// short, mostly empty cells: cell-centric, lane = kept row, (unaligned) 8-byte words
__global__ void __launch_bounds__(256) gather_bytes_cells(const GVar *__restrict__ v, const int32_t *__restrict__ sel, int64_t m) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const GVar g = v[blockIdx.y];
  const uint32_t o0 = g.out_off[k], n = g.out_off[k + 1] - o0;
  if (!n) return;
  struct __attribute__((packed, aligned(1))) U64 { uint64_t v; };
  uint32_t so = 0;
  if (g.fstart) { so = g.fstart[sel[k]]; if (!cell_plain(so)) return; }  // gather_text_special
  else so = g.in_off[sel[k]];
  const uint8_t *src = g.in_data + so;
  uint8_t *dst = g.out_data + o0;
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) reinterpret_cast<U64 *>(dst + i)->v = reinterpret_cast<const U64 *>(src + i)->v;
  if (i < n) { uint64_t x = reinterpret_cast<const U64 *>(src + i)->v; for (; i < n; i++) { dst[i] = (uint8_t)x; x >>= 8; } }
}
// the kept cells of late-materialised columns that need more than a byte copy (doubled quotes, DefaultValue)
__global__ void __launch_bounds__(256) gather_text_special(const GVar *__restrict__ v, const int32_t *__restrict__ sel, int64_t m) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const GVar g = v[blockIdx.y];
  uint32_t fsv = 0, o0 = 0, n = 0;
  if (k < m) {
    o0 = g.out_off[k]; n = g.out_off[k + 1] - o0;  // coalesced; most cells of a sparse column are empty
    if (n) { fsv = g.fstart[sel[k]]; if (cell_plain(fsv)) n = 0; }
  }
  text_copy_special_wave(g.in_data, g.quote, g.out_data, g.jsonnum != 0, fsv, o0, n, threadIdx.x & 63);
}
__global__ void collect_totals(const uint32_t *lens_all, int64_t seg_stride, int64_t m, int nv, uint32_t *out) {
  for (int s = threadIdx.x; s < nv; s += blockDim.x) out[s] = lens_all[(int64_t)s * seg_stride + m];
}

// Gather all columns of `in` through `sel` (m output rows).
static std::unique_ptr<tfgpu_dbatch> gather_batch(const tfgpu_dbatch &in, const Buf &sel, int64_t m, const std::vector<DColumn> *skip = nullptr) {
  // (skip: columns — by name — whose kept rows exist already: they are not gathered, their slot takes the given column)
  if (in.col_order) throw Error(TFGPU_ERR_UNSUPPORTED, "the batch's rows carry their own ColumnNames order (tfgpu_batch.col_order: a collapsed TOAST batch); row-moving steps do not carry it — "
                                                       "view / download, the native queue format and the Debezium emitter read it");
  auto out = std::make_unique<tfgpu_dbatch>();
  out->nrows = m; out->ns = in.ns; out->table = in.table; out->schema = in.schema;
  hipStream_t st = ctx().stream;
  const int32_t *sp = ptr<int32_t>(sel);
  unsigned g = grid_for(m, 256);
  KernelTimer t("compact_gather");
  static const bool eager_text = [] { const char *e = std::getenv("TFGPU_CSV_EAGER"); return e && e[0] == '1'; }();
  std::vector<GFix> fx; std::vector<GVar> vr; std::vector<size_t> var_cols; std::vector<GBit> bits;
  // ColumnValues and OldKeys columns move the same way; `all` lists them in that order
  const size_t ncur = in.cols.size(), nall = ncur + in.old_keys.size();
  auto col_at = [&](size_t i) -> const DColumn & { return i < ncur ? in.cols[i] : in.old_keys[i - ncur]; };
  out->cols.reserve(ncur); out->old_keys.reserve(in.old_keys.size());
  out->key_names = in.key_names;
  {  // packing kept cells now (TFGPU_CSV_EAGER=1), or a payload another handle packed already, is read through the source's offsets
    bool need = false;
    for (size_t i = 0; i < nall; i++) if (col_at(i).lens_only() && (eager_text || !col_at(i).lazy())) need = true;
    if (need) ensure_text_offsets(in);
  }
  // a lazy text column still in the lengths state (TextView::lens) leaves in that state: its kept rows' lengths are gathered like any
  // 4-byte array, nothing is scanned and nothing is read back for it
  auto stays_lens = [&](const DColumn &c) { return c.lens_only() && c.lazy() && !eager_text; };
  int nvar = 0, nlens = 0;
  for (size_t i = 0; i < nall; i++) if (repr_is_var(col_at(i).repr) && !(skip && i < ncur && [&] { for (auto &r : *skip) if (r.name == in.cols[i].name) return true; return false; }())) (stays_lens(col_at(i)) ? nlens : nvar)++;
  const int64_t seg_stride = ((m + 1 + 3) / 4) * 4;
  Buf lens_all = nvar ? dalloc((size_t)nvar * (size_t)seg_stride * 4 + 16) : nullptr;
  Buf lens_kept = nlens ? dalloc((size_t)nlens * (size_t)seg_stride * 4 + 16) : nullptr;  // the layout of lens_all: ensure_text_offsets scans these segments in one launch
  size_t li = 0;
  auto skipped = [&](size_t ai) -> const DColumn * {
    if (!skip || ai >= ncur) return nullptr;
    for (auto &r : *skip) if (r.name == in.cols[ai].name) return &r;
    return nullptr;
  };
  for (size_t ai = 0; ai < nall; ai++) {
    const DColumn &c = col_at(ai);
    if (const DColumn *have = skipped(ai)) { out->cols.push_back(*have); continue; }
    DColumn o;
    o.name = c.name; o.dtype = c.dtype; o.repr = c.repr;
    if (repr_is_var(c.repr) && stays_lens(c)) {
      if (!c.view->src) throw Error(TFGPU_ERR_INVALID, "internal: text column " + c.name + " lost its source text");
      auto v = std::make_shared<TextView>();
      v->src = c.view->src; v->fstart = dalloc((size_t)std::max<int64_t>(m, 1) * 4);
      v->has_special = c.view->has_special; v->quote = c.view->quote; v->jsonnum = c.view->jsonnum;
      v->lens = subbuf(lens_kept, li++ * (size_t)seg_stride * 4, (size_t)m * 4);
      fx.push_back(GFix{c.view->fstart->p, v->fstart->p, 4, 0});
      fx.push_back(GFix{c.view->lens->p, v->lens->p, 4, 0});
      o.view = std::move(v);
    } else if (repr_is_var(c.repr)) {
      if (c.lens_only()) throw Error(TFGPU_ERR_INVALID, "internal: text column " + c.name + " gathered before its lengths were scanned");
      size_t si = vr.size();
      o.offsets = subbuf(lens_all, si * (size_t)seg_stride * 4, (size_t)(m + 1) * 4);
      if (!c.lazy() || eager_text) o.data = dalloc(c.data_len + 8);  // the source size bounds the kept payload; exact length read back below
      o.data_len = c.data_len;
      if (c.lazy() && !eager_text) {
        // A kept row keeps pointing INTO the source text, as the kept ChangeItem's Go strings keep aliasing the chunk they
        // were cut from (filter_rows.go:99-125 appends the item, it copies no string bytes): the compacted column is again
        // (offsets, position of each cell in the text), packed when — and if — a consumer reads its bytes.
        if (!c.view->src) throw Error(TFGPU_ERR_INVALID, "internal: text column " + c.name + " lost its source text");
        auto v = std::make_shared<TextView>();
        v->src = c.view->src; v->fstart = dalloc((size_t)std::max<int64_t>(m, 1) * 4);
        v->has_special = c.view->has_special; v->quote = c.view->quote; v->jsonnum = c.view->jsonnum;
        fx.push_back(GFix{c.view->fstart->p, v->fstart->p, 4, 0});
        o.view = std::move(v);
        o.data = nullptr;
        vr.push_back(GVar{ptr<uint32_t>(c.offsets), nullptr, ptr<uint32_t>(o.offsets), nullptr, nullptr, 0, 0, 0});
      } else if (c.lazy()) {  // TFGPU_CSV_EAGER=1: kept cells are packed now, straight from the source text
        if (!c.view->src) throw Error(TFGPU_ERR_INVALID, "internal: text column " + c.name + " lost its source text");
        vr.push_back(GVar{ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.view->src), ptr<uint32_t>(o.offsets), ptr<uint8_t>(o.data), ptr<uint32_t>(c.view->fstart), c.view->quote, c.view->jsonnum ? 1u : 0u, c.view->has_special ? 1u : 0u});
      } else vr.push_back(GVar{ptr<uint32_t>(c.offsets), ptr<uint8_t>(c.payload()), ptr<uint32_t>(o.offsets), ptr<uint8_t>(o.data), nullptr, 0, 0, 0});
      var_cols.push_back(ai);
    } else {
      size_t w = repr_width(c.repr);
      o.values = dalloc((size_t)m * w);
      fx.push_back(GFix{c.values->p, o.values->p, (int32_t)w, 0});
      if (c.nanos) { o.nanos = dalloc((size_t)m * 4); fx.push_back(GFix{c.nanos->p, o.nanos->p, 4, 0}); }
    }
    if (c.validity) { o.validity = dalloc((size_t)(m + 7) / 8 + 1); bits.push_back(GBit{ptr<uint8_t>(c.validity), ptr<uint8_t>(o.validity)}); }
    if (c.absent) { o.absent = dalloc((size_t)(m + 7) / 8 + 1); bits.push_back(GBit{ptr<uint8_t>(c.absent), ptr<uint8_t>(o.absent)}); }  // a moved row keeps its ColumnNames
    (ai < ncur ? out->cols : out->old_keys).push_back(std::move(o));
  }
  auto out_at = [&](size_t i) -> DColumn & { return i < ncur ? out->cols[i] : out->old_keys[i - ncur]; };
  if (in.old_present) { out->old_present = dalloc((size_t)(m + 7) / 8 + 1); bits.push_back(GBit{ptr<uint8_t>(in.old_present), ptr<uint8_t>(out->old_present)}); }
  if (in.kind) { out->kind = dalloc((size_t)m); fx.push_back(GFix{in.kind->p, out->kind->p, 1, 0}); }
  if (in.part_id) { out->part_id = dalloc((size_t)m * 4); fx.push_back(GFix{in.part_id->p, out->part_id->p, 4, 0}); }
  out->src_row = dalloc((size_t)m * 4);
  if (in.src_row) fx.push_back(GFix{in.src_row->p, out->src_row->p, 4, 0});
  uint32_t *const ident = in.src_row ? nullptr : ptr<uint32_t>(out->src_row);

  if (m && !bits.empty()) {
    Buf bb = upload_const(bits.data(), bits.size() * sizeof(GBit));
    gather_bitmap_all<<<dim3(grid_for((m + 7) / 8, 256), (unsigned)bits.size()), 256, 0, st>>>(ptr<GBit>(bb), sp, m);
  }
  std::stable_sort(fx.begin(), fx.end(), [](const GFix &x, const GFix &y) { return x.width < y.width; });
  int nw[4] = {0, 0, 0, 0};
  for (auto &x : fx) nw[x.width == 1 ? 0 : x.width == 2 ? 1 : x.width == 4 ? 2 : 3]++;
  const int nfx[4] = {nw[0], nw[1], nw[2], nw[3]};
  if (fx.empty()) fx.push_back(GFix{nullptr, nullptr, 0, 0});  // (never read: every count is zero)
  Buf bfx = upload_const(fx.data(), fx.size() * sizeof(GFix));
  if (m) gather_fixed_all<<<g, 256, 0, st>>>(ptr<GFix>(bfx), nfx[0], nfx[1], nfx[2], nfx[3], ident, sp, m);
  if (nvar) {
    Buf bvr = upload_const(vr.data(), vr.size() * sizeof(GVar));
    if (m) gather_len_all<<<g, 256, 0, st>>>(ptr<GVar>(bvr), nvar, sp, m);
    exclusive_scan_u32_segments(ptr<uint32_t>(lens_all), m, nvar, seg_stride);
    if (m) {  // long cells: short runs of rows; short cells: long runs (the fixed latency of a run needs bytes to amortise over)
      std::vector<GVar> lng, sht;
      for (size_t i = 0; i < vr.size(); i++) if (vr[i].out_data) ((col_at(var_cols[i]).data_len >= (uint64_t)in.nrows * 8) ? lng : sht).push_back(vr[i]);
      Buf blng = upload_const(lng.data(), lng.size() * sizeof(GVar)), bsht = upload_const(sht.data(), sht.size() * sizeof(GVar));
      if (!lng.empty()) gather_bytes_all<1><<<dim3(grid_for(m, 256), (unsigned)lng.size()), 256, 0, st>>>(ptr<GVar>(blng), sp, m);
      if (!sht.empty()) gather_bytes_cells<<<dim3(grid_for(m, 256), (unsigned)sht.size()), 256, 0, st>>>(ptr<GVar>(bsht), sp, m);
      std::vector<GVar> lz;
      for (auto &x : vr) if (x.fstart && x.has_special) lz.push_back(x);
      if (!lz.empty()) {
        Buf blz = upload_const(lz.data(), lz.size() * sizeof(GVar));
        gather_text_special<<<dim3(grid_for(m, 256), (unsigned)lz.size()), 256, 0, st>>>(ptr<GVar>(blz), sp, m);
      }
    }
    Buf tot = dalloc((size_t)nvar * 4);
    collect_totals<<<1, 64, 0, st>>>(ptr<uint32_t>(lens_all), seg_stride, m, nvar, ptr<uint32_t>(tot));
    const uint32_t *h = d2h_u32(tot->p, (size_t)nvar);
    sync();
    for (int i = 0; i < nvar; i++) out_at(var_cols[(size_t)i]).data_len = h[i];
  }
  return out;
}

// Lengths → offsets for the text columns of `b` nobody has asked offsets of yet (DColumn::lens_only): the views without offsets are
// scanned OUT OF PLACE into a new buffer — copies of the column and a PendingRows::src share the view, and another lane may be gathering
// from `lens` meanwhile — with one launch per run of equally spaced segments (the parser's and gather_batch's layouts are one run), the
// totals come back in one read-back behind one sync, and the view is published; then the batch's own columns take offsets and data_len
// from their views (the handle's observable value does not change, as in dense_locked).  A handle that shares a scanned view only
// copies the two fields.  The publication is under a lock of its own; the scan is complete (synchronised) before it is published.
static std::mutex g_text_mu;
void ensure_text_offsets(const tfgpu_dbatch &b) {
  std::vector<DColumn *> cols;
  for (auto &c : b.cols) if (c.lens_only()) cols.push_back(const_cast<DColumn *>(&c));
  for (auto &c : b.old_keys) if (c.lens_only()) cols.push_back(const_cast<DColumn *>(&c));
  if (cols.empty()) return;
  std::lock_guard<std::mutex> tl(g_text_mu);
  const int64_t n = b.nrows;
  std::vector<TextView *> todo;
  for (auto *c : cols) {
    TextView *v = c->view.get();
    if ((int64_t)(v->lens->bytes / 4) != n) throw Error(TFGPU_ERR_INVALID, "internal: text column " + c->name + " holds lengths of another row count");
    if (!v->offsets && std::find(todo.begin(), todo.end(), v) == todo.end()) todo.push_back(v);
  }
  if (!todo.empty() && n == 0) {
    for (auto *v : todo) { v->total = 0; v->offsets = dalloc_zero(16); }
  } else if (!todo.empty()) {
    std::sort(todo.begin(), todo.end(), [](const TextView *x, const TextView *y) { return x->lens->p < y->lens->p; });
    struct Run { size_t first; int nseg; int64_t stride; Buf out; const uint32_t *tot; };
    std::vector<Run> runs;
    const int64_t own_stride = ((n + 1 + 3) / 4) * 4;
    for (size_t i = 0; i < todo.size();) {
      Run r{i, 1, own_stride, nullptr, nullptr};
      if (i + 1 < todo.size()) {
        const int64_t d = ptr<uint32_t>(todo[i + 1]->lens) - ptr<uint32_t>(todo[i]->lens);
        if (d >= n + 1 && d % 4 == 0 && d <= 2 * own_stride + 64) {  // (a far-away neighbour would only size the output for the gap)
          r.stride = d;
          while (r.first + (size_t)r.nseg < todo.size() && ptr<uint32_t>(todo[r.first + (size_t)r.nseg]->lens) - ptr<uint32_t>(todo[r.first + (size_t)r.nseg - 1]->lens) == d) r.nseg++;
        }
      }
      i += (size_t)r.nseg;
      runs.push_back(r);
    }
    for (auto &r : runs) {
      r.out = dalloc((size_t)r.nseg * (size_t)r.stride * 4 + 16);
      exclusive_scan_u32_segments(ptr<uint32_t>(todo[r.first]->lens), ptr<uint32_t>(r.out), n, r.nseg, r.stride);
      r.tot = segment_totals_to_host(ptr<uint32_t>(r.out), n, r.nseg, r.stride);
    }
    sync();
    for (auto &r : runs)
      for (int s = 0; s < r.nseg; s++) {
        TextView *v = todo[r.first + (size_t)s];
        v->total = r.tot[s];
        v->offsets = subbuf(r.out, (size_t)s * (size_t)r.stride * 4, (size_t)(n + 1) * 4);
      }
  }
  for (auto *c : cols) { c->data_len = c->view->total; c->offsets = c->view->offsets; }
}

std::unique_ptr<tfgpu_dbatch> gather_rows(const tfgpu_dbatch &in, const Buf &sel, int64_t m) { return gather_batch(in, sel, m); }

// TFGPU_LAZY_ROWS=0: the row filters gather their kept rows at once (the form of rounds 1-4; A/B measurements)
static bool lazy_rows_on() {
  static const bool off = [] { const char *e = std::getenv("TFGPU_LAZY_ROWS"); return e && e[0] == '0'; }();
  return !off;
}
// keep flags (uint32 0/1, n+1 slots) → compacted batch; identity if all kept.  lazy: the kept rows are handed on as a selection
// over `in` (tfgpu_dbatch::pending) and gathered when — and if — somebody reads them.
std::unique_ptr<tfgpu_dbatch> compact(const tfgpu_dbatch &in, Buf keep /* n+1 u32 */, bool lazy) {
  int64_t n = in.nrows;
  Buf sel = dalloc((size_t)n * 4 + 4);  // sized for every row: the selection is built while the count travels to the host
  const uint32_t *hm;
  if (select_kept_u32(ptr<uint32_t>(keep), n, ptr<int32_t>(sel), ptr<uint32_t>(keep) + n)) hm = d2h_u32(ptr<uint32_t>(keep) + n);
  else {  // an empty batch, or one too long for the two-launch form: the scan, then the selection from the scan
    exclusive_scan_u32(ptr<uint32_t>(keep), ptr<uint32_t>(keep), n, true);
    hm = d2h_u32(ptr<uint32_t>(keep) + n);
    if (n) build_selection_kernel<<<grid_for(n, 256), 256, 0, ctx().stream>>>(ptr<uint32_t>(keep), n, ptr<int32_t>(sel));
  }
  sync();
  const uint32_t m = *hm;
  if ((int64_t)m == n) return shallow_copy(in);
  if (lazy && lazy_rows_on() && !in.pending && m) {
    auto out = std::make_unique<tfgpu_dbatch>();
    out->nrows = m; out->ns = in.ns; out->table = in.table; out->schema = in.schema; out->key_names = in.key_names;
    auto pr = std::make_shared<PendingRows>();
    pr->src = std::make_shared<const tfgpu_dbatch>(in);  // (a shallow copy: the buffers are shared)
    pr->sel = sel;
    out->pending = std::move(pr);
    return out;
  }
  return gather_batch(in, sel, m);
}

// The selection → dense transition mutates a handle its callers hold as const, and one handle can be reached from two threads on two lanes (the
// Bufferer's collector concatenating a batch the pusher is serializing): the lane's mutex is the CALLING thread's, so the transition has a lock of
// its own (g_dense_mu: every read of `pending` / `replaced` / the columns of a handle that may still change happens under it, or on a snapshot()
// taken under it).  When the lock is released the gather is only QUEUED on the gathering lane's stream, with the lane's dense_event recorded behind
// it whenever a second lane exists; a lane made later synchronises the older lanes' streams as it is made (bind_lane), which covers the gathers
// queued while it did not exist.  Every other way into the dense columns — dense()'s first check, and the caller that lost the race and finds
// `pending` gone in dense_locked() — makes its own stream wait for that event before it returns.
// ADVICE r5, r6; tests/test_gpu_lane_handover.py.
static std::mutex g_dense_mu;
// TFGPU_DENSE_HOLD_MS=n (tests only, read once): a caller that has SEEN a selection (dense()) or copied one (snapshot()) sleeps n ms on the host before
// it goes on, with no lock held — two lanes that read one handle at the same moment then both see `pending`, one gathers, and the other certainly arrives behind it
// (tests/test_gpu_lane_handover.py).  Unset: nothing.
static void dense_hold() {
  static const int ms = [] { const char *e = std::getenv("TFGPU_DENSE_HOLD_MS"); return e ? std::atoi(e) : 0; }();
  if (ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(ms));
}
// a batch another lane made dense: this lane's stream waits for that gather (no-op on the gathering lane, and once that lane is gone: tfgpu_shutdown
// synchronised its stream before it destroyed the event)
static void wait_dense_nolock(const tfgpu_dbatch &b) {
  if (b.dense_done && b.dense_lane != current_lane() && b.dense_gen == lane_generation()) TF_HIP(hipStreamWaitEvent(ctx().stream, (hipEvent_t)b.dense_done, 0));
}
std::unique_ptr<tfgpu_dbatch> snapshot(const tfgpu_dbatch &b) {
  std::unique_ptr<tfgpu_dbatch> c;
  { std::lock_guard<std::mutex> dl(g_dense_mu); c = std::make_unique<tfgpu_dbatch>(b); }
  if (c->pending) dense_hold();  // (tests: the copy is held while another lane gathers the handle it was taken from)
  return c;
}
void dense_locked(const tfgpu_dbatch &b) {
  std::lock_guard<std::mutex> dl(g_dense_mu);
  if (!b.pending) { wait_dense_nolock(b); return; }  // another lane gathered since the caller looked: its kernels may still be queued there
  tfgpu_dbatch &mb = const_cast<tfgpu_dbatch &>(b);  // (the handle's observable value does not change: the same rows, now gathered)
  std::shared_ptr<PendingRows> pr = b.pending;
  std::unique_ptr<tfgpu_dbatch> g = gather_batch(*pr->src, pr->sel, b.nrows, b.replaced.empty() ? nullptr : &b.replaced);
  mb.cols = std::move(g->cols); mb.old_keys = std::move(g->old_keys); mb.old_present = g->old_present;
  mb.kind = g->kind; mb.src_row = g->src_row; mb.part_id = g->part_id;
  mb.replaced.clear();
  if (lanes_created() > 1) {  // the gather is QUEUED on this lane's stream: leave an event behind it for readers on other streams (a host sync here cost configs[4] 0.2 ms a pass)
    // ONE event a lane, recorded again at every transition: a reader that waits on a later record than its batch's waits for more than it must, never for less.
    // With one lane alive nothing is recorded (an event behind every transition cost the single-lane configs[4] line 6-10 % — one box, one visit,
    // two runs each: 670 / 638 M rows/s against 712 / 711 M): a lane made later is
    // counted FIRST and then waits for every older lane's stream (bind_lane), so a gather queued before this line saw it is complete before it reads.
    Context &cx = ctx();
    if (!cx.dense_event) TF_HIP(hipEventCreateWithFlags(&cx.dense_event, hipEventDisableTiming));
    TF_HIP(hipEventRecord(cx.dense_event, cx.stream));
    mb.dense_done = (void *)cx.dense_event;
    mb.dense_lane = current_lane();
    mb.dense_gen = lane_generation();
  }
  mb.pending.reset();
}
bool has_absent(const tfgpu_dbatch &b) {
  std::lock_guard<std::mutex> dl(g_dense_mu);
  if (b.col_order) return true;  // rows with their own ColumnNames order are ragged rows too
  for (auto &c : (b.pending ? b.pending->src->cols : b.cols)) if (c.absent) return true;
  return false;
}
void wait_dense(const tfgpu_dbatch &b) { std::lock_guard<std::mutex> dl(g_dense_mu); wait_dense_nolock(b); }
void refuse_absent(const tfgpu_dbatch &b) {
  if (has_absent(b))
    throw Error(TFGPU_ERR_UNSUPPORTED, "the batch holds ABSENT cells (rows whose ColumnNames leave a column out: TOASTed updates, tfgpu_column.absent); this entry computes on values and "
                                       "does not read them — tfgpu_collapse, tfgpu_keys_changed, tfgpu_partition, view / download do");
}
void dense(const tfgpu_dbatch *b, bool absent_ok) {
  if (!b) return;
  if (!absent_ok) refuse_absent(*b);
  { std::lock_guard<std::mutex> dl(g_dense_mu); if (!b->pending) { wait_dense_nolock(*b); return; } }
  dense_hold();
  std::lock_guard<std::mutex> lk(ctx().mu);
  dense_locked(*b);
}

std::unique_ptr<tfgpu_dbatch> compact_rows(const tfgpu_dbatch &in, Buf keep) { return compact(in, keep); }

// hash-partition, local half (config 5): rows grouped by PartID, original order kept inside a part
__global__ void part_keep_kernel(const uint32_t *part_id, int64_t n, uint32_t d, uint32_t *keep) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) keep[r] = part_id[r] == d ? 1u : 0u;
}
__global__ void part_scatter_kernel(const uint32_t *keep_scan, int64_t n, uint32_t base, int32_t *sel) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = keep_scan[i], b = keep_scan[i + 1];
  if (a != b) sel[base + a] = (int32_t)i;
}
std::unique_ptr<tfgpu_dbatch> partition_rows(const tfgpu_dbatch &in, int nparts, int64_t *counts) {
  if (!in.part_id) throw Error(TFGPU_ERR_INVALID, "tfgpu_partition: the batch has no part_id (apply sharder_transformer first)");
  const int64_t n = in.nrows;
  hipStream_t st = ctx().stream;
  Buf sel = dalloc((size_t)n * 4 + 4), keep = dalloc((size_t)(n + 1) * 4);
  uint32_t base = 0;
  KernelTimer t("partition_rows");
  for (int d = 0; d < nparts; d++) {
    if (n) part_keep_kernel<<<grid_for(n, 256), 256, 0, st>>>(ptr<uint32_t>(in.part_id), n, (uint32_t)d, ptr<uint32_t>(keep));
    exclusive_scan_u32(ptr<uint32_t>(keep), ptr<uint32_t>(keep), n, true);
    const uint32_t *h = d2h_u32(ptr<uint32_t>(keep) + n);
    sync();
    const uint32_t m = *h;
    if (n && m) part_scatter_kernel<<<grid_for(n, 256), 256, 0, st>>>(ptr<uint32_t>(keep), n, base, ptr<int32_t>(sel));
    counts[d] = m;
    base += m;
  }
  if ((int64_t)base != n) throw Error(TFGPU_ERR_INVALID, "tfgpu_partition: part_id outside [0, nparts)");
  return gather_batch(in, sel, n);
}
}  // namespace tf
