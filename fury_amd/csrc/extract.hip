// extract.hip -- nested struct, list and map fields of a row batch as batches (fury_row_extract).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of BinaryRow.getStruct / getArray / getMap (FMT/row/binary/UnsafeTrait.java:160-197, BinaryMap.pointTo
// FMT/row/binary/BinaryMap.java:62-77): one bitmap bit, one 8-byte slot and a pointTo(buffer,
// baseOffset + relativeOffset, size).  A nested row, array or map addresses its variable-length section
// relative to its own base, so the bytes the slot points at are a complete row of the child schema /
// a complete BinaryArray / a complete BinaryMap at any position: the value of a path of struct slots
// is a byte range of the source row, and the batch of them is a gather that needs no column tree.
//
// MI355X design:
//   locate     lane = source row walks the path once: per level the header bounds, the bitmap word of
//              the slot, the slot (the struct widths and slot numbers travel in the argument block
//              and are indexed wave-uniformly: scalar loads).  A wave is a 64-row tile: the ballot of
//              "has a value" goes out as the tile's two validity words, its count and its mask, and
//              every lane with a value stores (absolute source start, size) as one 16-byte word.
//              Nothing after this pass reads a row header again.
//   compact    device_scan of the tile counts (the total is *out_count), then lane = source row
//              writes its row number, source start and size at tile base + popcount of the lower
//              mask bits; entries at or past the count are filled by the lane of that position
//              (-1 / size 0), so every entry is written exactly once (as filter_write of take.hip).
//              device_scan of the sizes then makes out_offsets.
//   copy       extract_copy of extract_dev.h (explode.hip launches it too): copy_rows of take_dev.h,
//              the copy of take.hip, with the source start of output row j read from the compacted
//              array.
// Bounds ("Decode bounds" of kernels.h, per level; ExtractArgs): nothing outside [0, total) of the
// rows buffer is read, the output is written only inside [0, min(capacity, needed)).
#include "extract_dev.h"

namespace fury {

namespace {

static_assert(sizeof(ExtractArgs{}.nfields) / sizeof(int32_t) == kMaxNestLevels,
              "a path is as long as a schema is deep");

// tc[t] / masks[t]: count and ballot of tile t (rows [64 t, 64 t + 64)); loc[r] = (source start,
// size) of row r's value, written only when the row has one.  The walk itself: extract_dev.h.
__global__ __launch_bounds__(kTakeThreads) void extract_locate(ExtractArgs a,
                                                               int64_t* __restrict__ tc,
                                                               uint64_t* __restrict__ masks,
                                                               v2l* __restrict__ loc) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  const int64_t n = a.nrows;
  const int64_t total = gl(a.row_offsets)[n];
  int64_t base, size;
  bool bad;
  const bool live = walk_path(a, r, total, &base, &size, &bad);
  if (bad) raise_oob(a.err, r);
  const uint64_t m = __ballot(live);
  if (r >= n) return;
  if ((threadIdx.x & 63) == 0) put_tile(r >> 6, m, n, tc, masks, a.out_validity);
  if (live) gl(loc)[r] = v2l{base, size};
}

// tc: exclusive scan of the tile counts, *count its total.  idx / src may be NULL (not wanted).
__global__ __launch_bounds__(kTakeThreads) void extract_compact(const uint64_t* __restrict__ masks,
                                                                const v2l* __restrict__ loc,
                                                                int64_t nrows,
                                                                const int64_t* __restrict__ tc,
                                                                const int64_t* __restrict__ count,
                                                                int64_t* __restrict__ idx,
                                                                int64_t* __restrict__ src,
                                                                int64_t* __restrict__ oo) {
  compact_entries(masks, loc, nrows, tc, count, src, oo,
                  [=](int64_t pos, int64_t r) { if (idx) gl(idx)[pos] = r; },
                  [=](int64_t r) { if (idx) gl(idx)[r] = -1; });
}

}  // namespace

int launch_extract(const ExtractArgs& a, hipStream_t stream) {
  const int64_t n = a.nrows;
  if (n >= (int64_t{1} << 38))        // blocks_of() in 31 bits
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  if (n == 0) {
    int st = check_hip(hipMemsetAsync(a.out_count, 0, 8, stream), "memset");
    if (!st) st = check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
    return st;
  }
  const int64_t nt = (n + 63) / 64;
  const int64_t sw = (scan_workspace(n) + 1) & ~int64_t{1};   // >= scan_workspace(nt); even: loc is 16-byte aligned
  const bool copy = a.out && a.cap >= 8;
  int64_t* ws = nullptr;              // [tile counts x nt][tile masks x nt][scan scratch][loc x 2 n][source starts x n]
  int st = dev_alloc((2 * nt + sw + 2 * n + (copy ? n : 0)) * 8, stream, reinterpret_cast<void**>(&ws));
  if (st) return st;
  int64_t* tc = ws;
  uint64_t* masks = reinterpret_cast<uint64_t*>(ws + nt);
  int64_t* sws = ws + 2 * nt;
  v2l* loc = reinterpret_cast<v2l*>(sws + sw);
  int64_t* src = copy ? sws + sw + 2 * n : nullptr;
  hipLaunchKernelGGL(extract_locate, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, tc, masks,
                     loc);
  device_scan(tc, nt, a.out_count, sws, stream);
  hipLaunchKernelGGL(extract_compact, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, masks, loc, n,
                     tc, a.out_count, a.out_indices, src, a.out_offsets);
  device_scan(a.out_offsets, n, a.out_offsets + n, sws, stream);
  if (copy)
    hipLaunchKernelGGL(extract_copy, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a.rows, src,
                       n, a.out, a.out_offsets, a.cap);
  st = check_hip(hipGetLastError(), "extract launch");
  dev_free(ws, stream);
  return st;
}

}  // namespace fury
