// extract_dev.h -- what extract.hip (fury_row_extract), explode.hip (fury_row_explode), implode.hip
// and map.hip share: the walk along a path of struct slots, the compact step that turns per-tile
// ballots and per-lane (source start, size) pairs into a dense batch, and the two kernels that were the
// same in two files each: the rank of a validity bitmap's tiles (tile_rank) and the copy from
// compacted source starts (extract_copy).  The designs are described in the .hip files.
#pragma once

#include "take_dev.h"

namespace fury {

using v2l = __attribute__((ext_vector_type(2))) int64_t;

__device__ __forceinline__ int32_t header_bytes(int32_t nfields) {
  return (((nfields + 63) >> 6) << 3) + 8 * nfields;
}

// Row r of the batch: follows slot a.slot[k] of the struct of a.nfields[k] fields at level k, for
// a.nlevels levels (ExtractArgs / ExplodeArgs: the members have the same names).  Returns true with
// the value's span [*base, *base + *size) when every level has one; false for a null (or r >=
// nrows), and false with *bad set when a level fails the bounds rule of ExtractArgs (kernels.h).
// The level loop is wave-uniform: nfields / slot are scalar loads.
template <class Args>
__device__ __forceinline__ bool walk_path(const Args& a, int64_t r, int64_t total, int64_t* base_out,
                                          int64_t* size_out, bool* bad_out) {
  bool live = r < a.nrows, bad = false;
  int64_t base = live ? gl(a.row_offsets)[r] : 0;
  int64_t size = 0;
  if (live && (base & 7)) {
    bad = true;
    live = false;
  }
  for (int k = 0; k < a.nlevels; k++) {
    const int32_t nf = a.nfields[k], sl = a.slot[k];
    const int32_t bm = ((nf + 63) >> 6) << 3;
    const bool last = k + 1 == a.nlevels;
    const int32_t need = last ? a.min_size : header_bytes(a.nfields[k + 1]);
    if (!live) continue;
    live = false;
    if (!span_ok(base, bm + 8 * nf, total)) {
      bad = true;
      continue;
    }
    const uint64_t word = gl(reinterpret_cast<const uint64_t*>(a.rows + base))[sl >> 6];
    if ((word >> (sl & 63)) & 1) continue;          // null: nothing further of the row is read
    const uint64_t s = gl(reinterpret_cast<const uint64_t*>(a.rows + base + bm))[sl];
    const int32_t off = static_cast<int32_t>(s >> 32), len = static_cast<int32_t>(s);
    if (off < 0 || len < 0 || ((off | len) & 7) || !span_ok(base + off, len, total) || len < need ||
        (last && a.exact && len != need)) {
      bad = true;
      continue;
    }
    base += off;
    size = len;
    live = true;
  }
  *base_out = base;
  *size_out = size;
  *bad_out = bad;
  return live;
}

// Bits [64 t, 64 t + 64) of an Arrow bitmap of n bits read as 32-bit words (NULL: all set); bits at or
// past n are 0.  64 t < n.
__device__ __forceinline__ uint64_t tile_word(const uint32_t* bits, int64_t t, int64_t n) {
  uint64_t w = ~0ull;
  if (bits) {
    w = gl(bits)[2 * t];
    if (64 * t + 32 < n) w |= static_cast<uint64_t>(gl(bits)[2 * t + 1]) << 32;
  }
  const int64_t rem = n - 64 * t;
  return rem < 64 ? w & ((1ull << rem) - 1) : w;
}

namespace {

// The rank pass of implode.hip and map.hip's join, lane = 64-bit tile t of nt: tr[t] = the popcount
// of tile_word(bits, t, n), to be scanned.
__global__ __launch_bounds__(kTakeThreads) void tile_rank(const uint32_t* __restrict__ bits, int64_t n,
                                                          int64_t nt, int64_t* __restrict__ tr) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (t < nt) gl(tr)[t] = __popcll(tile_word(bits, t, n));
}

// The copy pass of extract.hip and explode.hip: n output rows at oo[0..n] (oo[n] = bytes needed);
// output row j = the bytes at src[j], the compacted source starts.
__global__ __launch_bounds__(kTakeThreads) void extract_copy(const uint8_t* __restrict__ rows,
                                                             const int64_t* __restrict__ src,
                                                             int64_t n, uint8_t* __restrict__ out,
                                                             const int64_t* __restrict__ oo,
                                                             int64_t cap) {
  copy_rows(rows, [=](int64_t j) { return gl(src)[j]; }, n, out, oo, cap);
}

}  // namespace

// The tile ballot of a locate pass: count, mask and the two validity words of tile t of an output of
// n positions (validity may be NULL).  Called by the first lane of the wave.
__device__ __forceinline__ void put_tile(int64_t t, uint64_t m, int64_t n, int64_t* tc, uint64_t* masks,
                                         uint32_t* validity) {
  gl(tc)[t] = __popcll(m);
  gl(masks)[t] = m;
  if (validity) {
    gl(validity)[2 * t] = static_cast<uint32_t>(m);
    if (64 * t + 32 < n) gl(validity)[2 * t + 1] = static_cast<uint32_t>(m >> 32);
  }
}

// The body of a compact kernel, lane = position r of n: tc = exclusive scan of the tile counts, *count
// its total.  A position whose mask bit is set writes its source start (src may be NULL) and size at
// tile base + popcount of the lower mask bits and calls put(pos, r); the positions at or past the
// count are filled by the lane of that position (size 0, fill(r)), so every entry is written exactly
// once (as filter_write of take.hip).
template <class Put, class Fill>
__device__ __forceinline__ void compact_entries(const uint64_t* __restrict__ masks,
                                                const v2l* __restrict__ loc, int64_t n,
                                                const int64_t* __restrict__ tc,
                                                const int64_t* __restrict__ count,
                                                int64_t* __restrict__ src, int64_t* __restrict__ oo,
                                                Put put, Fill fill) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (r >= n) return;
  const int lane = static_cast<int>(r & 63);
  const uint64_t m = gl(masks)[r >> 6];
  if ((m >> lane) & 1) {
    const int64_t pos = gl(tc)[r >> 6] + __popcll(m & ((1ull << lane) - 1));
    const v2l v = gl(loc)[r];
    put(pos, r);
    if (src) gl(src)[pos] = v.x;
    gl(oo)[pos] = v.y;
  }
  if (r >= *gl(count)) {              // the entries past the count: this lane's own position
    fill(r);
    gl(oo)[r] = 0;
  }
}

}  // namespace fury
