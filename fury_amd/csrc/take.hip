// take.hip -- gather selected rows of a row batch into a new batch (fury_row_take / fury_row_filter).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of BinaryRow.copy() (FMT/row/binary/BinaryRow.java:173-179: buffer.copyTo(baseOffset, copyBuf, 0,
// sizeInBytes)).  Every (offset << 32) | size slot of a row is relative to the row's own base, so a
// selected row is its bytes, unchanged, at a new position: only offsets and bytes are used and the
// schema may be anything (flat, wide, nested, a collection schema).
//
// MI355X design:
//   sizes      lane = output row: the index and the source extent are validated ("Decode bounds" of
//              kernels.h), the size (0 for a row that fails) goes to out_offsets[j]; device_scan in
//              place then makes the offsets, the total lands in out_offsets[n].
//   filter     per-tile popcount of the mask words (tiles at multiples of 64 rows), device_scan of
//              the tile counts (the total is *out_count), then lane = source row writes its number
//              and its size at tile base + popcount of the lower mask bits.  Entries at or past the
//              count are filled by the lane of that position (-1 / size 0), so every entry is
//              written exactly once.  The count stays on the device: everything after reads it there.
//   copy       (copy_rows of take_dev.h: an instance of write_spans, the one write pass that
//              extract, explode, select, zip, implode and map instantiate too)
//              output-parallel and balanced by bytes.  write_spans: a workgroup owns kTakeSpan bytes
//              of the output (grid-stride over spans), finds the first and last row of its span by a
//              64-ary search of out_offsets (one probe per lane, 4 dependent loads for 16 M rows) and
//              stages the rows' output starts and what else its caller keeps per row -- here the
//              source start -- in LDS, in rounds of kTakeRows: any number of 0-byte rows may sit in a
//              span.  store_split: lanes own 16-byte aligned output chunks, the unaligned head / tail
//              word of a round goes out as 8 bytes.  copy_rows' chunk: binary search in LDS for the
//              chunk's row (staged_row, as unframe_copy), one 16-byte load when source and
//              destination are congruent mod 16, else two 8-byte loads (the second one from the next
//              row when the chunk straddles two rows: rows are multiples of 8 bytes at 8-byte
//              alignment), kTakeInFlight chunks loaded before the first non-temporal 16-byte store.
//   fixed      rows of is_fixed schemas sit at j * fixed_size: no offsets, no scan, no search; the
//              chunk's row is its word index / words per row by multiply-high (as update.hip).
// Bounds: a source row is read only when its index is in [0, nrows) and its extent lies in
// [0, row_offsets[nrows]) with a non-negative size that is a multiple of 8 at an 8-byte aligned start;
// the output is written only inside [0, min(capacity, needed)).
#include "take_dev.h"

namespace fury {

namespace {

__global__ __launch_bounds__(kTakeThreads) void take_sizes(const int64_t* __restrict__ ro,
                                                           int64_t nrows,
                                                           const int64_t* __restrict__ idx, int64_t n,
                                                           int64_t* __restrict__ oo, uint32_t* err) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (j >= n) return;
  bool ok;
  const int64_t sz = row_extent(ro, nrows, gl(ro)[nrows], gl(idx)[j], &ok);
  if (!ok) raise_oob(err, j);
  gl(oo)[j] = sz;
}

// Mask bits [rb, rb + 64) read as 32-bit words (rb a multiple of 64, rb < nrows); bits at or past
// nrows are 0.
__device__ __forceinline__ uint64_t mask64(const uint8_t* mask, int64_t rb, int64_t nrows) {
  const auto* w = gl(reinterpret_cast<const uint32_t*>(mask)) + (rb >> 5);
  uint64_t v = w[0];
  if (rb + 32 < nrows) v |= static_cast<uint64_t>(w[1]) << 32;
  const int64_t rem = nrows - rb;
  if (rem < 64) v &= (1ull << rem) - 1;
  return v;
}

__global__ __launch_bounds__(kTakeThreads) void filter_count(const uint8_t* __restrict__ mask,
                                                             int64_t nrows, int64_t nt,
                                                             int64_t* __restrict__ tc) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (t < nt) gl(tc)[t] = __popcll(mask64(mask, t * 64, nrows));
}

// tc: exclusive scan of the tile counts, *count its total.  idx / oo may be NULL (not wanted).
__global__ __launch_bounds__(kTakeThreads) void filter_write(const uint8_t* __restrict__ mask,
                                                             const int64_t* __restrict__ ro,
                                                             int64_t nrows,
                                                             const int64_t* __restrict__ tc,
                                                             const int64_t* __restrict__ count,
                                                             int64_t* __restrict__ idx,
                                                             int64_t* __restrict__ oo, uint32_t* err) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (r >= nrows) return;
  const int lane = static_cast<int>(r & 63);
  const uint64_t m = mask64(mask, r - lane, nrows);
  if ((m >> lane) & 1) {
    const int64_t pos = gl(tc)[r >> 6] + __popcll(m & ((1ull << lane) - 1));
    if (idx) gl(idx)[pos] = r;
    if (oo) {
      bool ok;
      const int64_t sz = row_extent(ro, nrows, gl(ro)[nrows], r, &ok);
      if (!ok) raise_oob(err, r);
      gl(oo)[pos] = sz;
    }
  }
  if (r >= *gl(count)) {              // the entries past the count: this lane's own position
    if (idx) gl(idx)[r] = -1;
    if (oo) gl(oo)[r] = 0;
  }
}

// n output rows at oo[0..n] (oo[n] = bytes needed); output row j = source row idx[j].
__global__ __launch_bounds__(kTakeThreads) void take_copy(const uint8_t* __restrict__ rows,
                                                          const int64_t* __restrict__ ro,
                                                          const int64_t* __restrict__ idx, int64_t n,
                                                          uint8_t* __restrict__ out,
                                                          const int64_t* __restrict__ oo,
                                                          int64_t cap) {
  copy_rows(rows, [=](int64_t j) { return gl(ro)[gl(idx)[j]]; }, n, out, oo, cap);
}

// Fixed-size rows of W 8-byte words: output word w belongs to output row w / W (multiply-high by
// magic = 2^64 / W rounded up, exact for w < 2^64 / W), source row idx[w / W].  A row whose index is
// not in [0, nrows) is written as zeros and reported once (by the lane that holds its first word).
__global__ __launch_bounds__(kTakeThreads) void take_copy_fixed(const uint8_t* __restrict__ rows,
                                                                int64_t nrows,
                                                                const int64_t* __restrict__ idx,
                                                                int64_t n,
                                                                const int64_t* __restrict__ count,
                                                                uint64_t W, uint64_t magic,
                                                                uint8_t* __restrict__ out, int64_t cap,
                                                                uint32_t* err) {
  const int tid = threadIdx.x;
  const int64_t cnt = count ? *gl(count) : n;
  const int64_t lim = min(cnt * static_cast<int64_t>(W) * 8, cap & ~int64_t{7});
  const uintptr_t ob = reinterpret_cast<uintptr_t>(out);
  // source word of output word w, NULL when the row's index is bad
  auto source = [&](uint64_t w, int64_t* i_out) -> const uint8_t* {
    const uint64_t j = __umul64hi(w, magic), k = w - j * W;
    const int64_t i = gl(idx)[j];
    *i_out = i;
    if (i < 0 || i >= nrows) {
      if (k == 0) raise_oob(err, static_cast<int64_t>(j));
      return nullptr;
    }
    return rows + (static_cast<uint64_t>(i) * W + k) * 8;
  };
  auto word_at = [&](int64_t d) -> uint64_t {
    int64_t i;
    const uint8_t* p = source(static_cast<uint64_t>(d) >> 3, &i);
    return p ? ld8(p) : 0;
  };
  for (int64_t S = static_cast<int64_t>(blockIdx.x) * kTakeSpan; S < lim;
       S += static_cast<int64_t>(gridDim.x) * kTakeSpan) {
    const int64_t E = min(S + kTakeSpan, lim);
    int64_t A = S + static_cast<int64_t>((16 - ((ob + S) & 15)) & 15);
    int64_t B = E - static_cast<int64_t>((ob + E) & 15);
    if (A > B) A = B = E;
    if (tid == 0 && S < A) st8(out + S, word_at(S));
    if (tid == 64 && B < E) st8(out + B, word_at(B));
    for (int64_t d0 = A; d0 < B; d0 += kTakeStep) {
      const uint8_t* p0[kTakeInFlight];
      const uint8_t* p1[kTakeInFlight];
      v2q v[kTakeInFlight];
#pragma unroll
      for (int u = 0; u < kTakeInFlight; u++) {      // the index loads, all in flight
        const int64_t d = d0 + 16 * (tid + u * kTakeThreads);
        p0[u] = p1[u] = nullptr;
        if (d < B) {
          const uint64_t w = static_cast<uint64_t>(d) >> 3;
          const uint64_t j = __umul64hi(w, magic), k = w - j * W;
          int64_t i;
          p0[u] = source(w, &i);
          if (k + 1 < W) p1[u] = p0[u] ? p0[u] + 8 : nullptr;
          else p1[u] = source(w + 1, &i);
        }
      }
#pragma unroll
      for (int u = 0; u < kTakeInFlight; u++) {      // then the row loads
        v[u] = v2q{0, 0};
        if (p0[u] && p1[u] == p0[u] + 8 && (reinterpret_cast<uintptr_t>(p0[u]) & 15) == 0) {
          v[u] = ld16(p0[u]);
        } else {
          if (p0[u]) v[u].x = ld8(p0[u]);
          if (p1[u]) v[u].y = ld8(p1[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kTakeInFlight; u++) {
        const int64_t d = d0 + 16 * (tid + u * kTakeThreads);
        if (d < B) st16(out + d, v[u]);
      }
    }
  }
}

void copy_fixed(const TakeArgs& a, const int64_t* idx, int64_t n, const int64_t* count,
                hipStream_t stream) {
  const int64_t bytes = std::min(a.cap, n * a.fixed_size);
  if (!a.out || bytes < 8) return;
  const uint64_t W = static_cast<uint64_t>(a.fixed_size) / 8;
  const uint64_t magic = ~0ull / W + 1;
  hipLaunchKernelGGL(take_copy_fixed, dim3(copy_grid(bytes)), dim3(kTakeThreads), 0, stream, a.rows,
                     a.nrows, idx, n, count, W, magic, a.out, a.cap, a.err);
}

}  // namespace

int too_large(int64_t n, int64_t fixed_size) {
  // blocks_of() in 31 bits, and the fixed copy's multiply-high exact
  if (n >= (int64_t{1} << 38) || (fixed_size > 0 && n > (int64_t{1} << 52) / fixed_size))
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  return FURY_OK;
}

void copy_selected(const TakeArgs& a, const int64_t* idx, const int64_t* count, int64_t* sws,
                   hipStream_t stream) {
  const int64_t n = a.nrows;
  if (!a.row_offsets) {
    if (a.out_offsets)
      hipLaunchKernelGGL(fixed_offsets, dim3(blocks_of(n + 1)), dim3(kTakeThreads), 0, stream,
                         a.out_offsets, n, count, a.fixed_size);
    copy_fixed(a, idx, n, count, stream);
  } else {
    device_scan(a.out_offsets, n, a.out_offsets + n, sws, stream);
    if (a.out && a.cap >= 8)
      hipLaunchKernelGGL(take_copy, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a.rows,
                         a.row_offsets, idx, n, a.out, a.out_offsets, a.cap);
  }
}

int launch_take(const TakeArgs& a, hipStream_t stream) {
  const int64_t n = a.n;
  int st = too_large(std::max(n, a.nrows), a.fixed_size);
  if (st) return st;
  if (!a.row_offsets) {               // fixed-size rows
    if (a.out_offsets)
      hipLaunchKernelGGL(fixed_offsets, dim3(blocks_of(n + 1)), dim3(kTakeThreads), 0, stream,
                         a.out_offsets, n, static_cast<const int64_t*>(nullptr), a.fixed_size);
    if (n > 0) copy_fixed(a, a.indices, n, nullptr, stream);
    return check_hip(hipGetLastError(), "take launch");
  }
  if (n == 0) return check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
  int64_t* ws = nullptr;
  st = dev_alloc(scan_workspace(n) * 8, stream, reinterpret_cast<void**>(&ws));
  if (st) return st;
  hipLaunchKernelGGL(take_sizes, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a.row_offsets,
                     a.nrows, a.indices, n, a.out_offsets, a.err);
  device_scan(a.out_offsets, n, a.out_offsets + n, ws, stream);
  if (a.out && a.cap >= 8)
    hipLaunchKernelGGL(take_copy, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a.rows,
                       a.row_offsets, a.indices, n, a.out, a.out_offsets, a.cap);
  st = check_hip(hipGetLastError(), "take launch");
  dev_free(ws, stream);
  return st;
}

int launch_filter(const TakeArgs& a, const uint8_t* mask, int64_t* out_count, int64_t* out_indices,
                  hipStream_t stream) {
  const int64_t n = a.nrows;
  int st = too_large(n, a.fixed_size);
  if (st) return st;
  if (n == 0) {
    st = check_hip(hipMemsetAsync(out_count, 0, 8, stream), "memset");
    if (!st && a.out_offsets) st = check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
    return st;
  }
  const bool fixed = !a.row_offsets;
  const int64_t nt = (n + 63) / 64;
  const int64_t sw = scan_workspace(n);             // >= scan_workspace(nt): both scans use it
  const bool own_idx = a.out && !out_indices;       // the copy needs the row numbers
  int64_t* ws = nullptr;                            // [tile counts x nt][scan scratch][row numbers]
  st = dev_alloc((nt + sw + (own_idx ? n : 0)) * 8, stream, reinterpret_cast<void**>(&ws));
  if (st) return st;
  int64_t* tc = ws;
  int64_t* sws = ws + nt;
  int64_t* idx = own_idx ? sws + sw : out_indices;
  hipLaunchKernelGGL(filter_count, dim3(blocks_of(nt)), dim3(kTakeThreads), 0, stream, mask, n, nt, tc);
  device_scan(tc, nt, out_count, sws, stream);
  hipLaunchKernelGGL(filter_write, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, mask,
                     a.row_offsets, n, tc, out_count, idx, fixed ? nullptr : a.out_offsets, a.err);
  copy_selected(a, idx, out_count, sws, stream);
  st = check_hip(hipGetLastError(), "filter launch");
  dev_free(ws, stream);
  return st;
}

}  // namespace fury
