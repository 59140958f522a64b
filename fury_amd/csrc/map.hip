// map.hip -- the key and value arrays of a map field as two batches (fury_row_map_split) and two array
// batches back into maps (fury_row_map_join).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): split is the
// batch form of BinaryMap.pointTo + keyArray() / valueArray() (FMT/row/binary/BinaryMap.java:62-77,
// 101-108), join of the constructor BinaryMap(BinaryArray keys, BinaryArray values, Field)
// (BinaryMap.java:52-60) and of the writer's serializeForMap: writeDirectly(-1), the key array,
// writeDirectly(offset, keyArraySize), the value array.  A map is [int64 keyArrayBytes][key
// BinaryArray][value BinaryArray] and each array addresses its contents relative to its own base, so
// both directions are byte copies plus one generated 8-byte word.
//
// MI355X design, split (extract.hip's three passes, with two outputs):
//   locate     lane = source row: walk_path of extract_dev.h (or the entry's own extent for a
//              collection schema), the map header and the two array headers -- four 8-byte loads past
//              the walk.  A wave is a 64-row tile: the ballot of "has a map" goes out through put_tile,
//              a lane with one stores (start, size) of both arrays.
//   compact    device_scan of the tile counts, then lane = source row writes its row number and per
//              side its source start and size at tile base + popcount of the lower mask bits; entries
//              past the count are filled by the lane of that position.  device_scan per side makes the
//              offsets.
//   copy       ONE launch of copy_rows (take_dev.h) over both outputs: blockIdx.y picks the batch,
//              blockIdx.x the 16 KB span of its bytes, so either side spreads over as many workgroups
//              as it has spans whatever the other side holds.
// Join (implode.hip's fused variant with element = row and two runs per row):
//   rank       lane = 64-row tile: the popcount of its validity word (tile_rank of extract_dev.h,
//              implode's kernel), then device_scan.  Skipped without a bitmap.
//   rows       lane = row, O(1): the value index, both value checks, the two counts, the sizes; per
//              row (key start, key size | -1) and the value start.  device_scan makes out_offsets.
//   write      write_spans / store_located of take_dev.h, as implode_write: a workgroup owns
//              kTakeSpan output bytes, finds its rows by the 64-ary search of out_offsets, stages
//              them in LDS, and lanes own 16-byte chunks.  A word is GENERATED
//              (row bitmap, row slot, the key-size word, the empty map) or COPIED from the row's key or
//              value run: one 16-byte non-temporal load when the source aligns, else two 8-byte ones.
// Nothing loops over a row's bytes or entries: a 70,000-entry map among empty rows is as many copy /
// write workgroups as it has 16 KB spans.
// Bounds (MapSplitArgs / MapJoinArgs in kernels.h): split reads nothing outside [0, total) of the rows
// buffer, join nothing outside [0, KT) of keys and [0, VT) of values; every output is written only
// inside [0, min(capacity, needed)).
#include "extract_dev.h"

namespace fury {

namespace {

static_assert(sizeof(MapSplitArgs{}.nfields) / sizeof(int32_t) == kMaxNestLevels,
              "a path is as long as a schema is deep");

constexpr int64_t kMaxElems = (INT32_MAX - 15) / 8;      // BinaryArrayWriter.MAX_ROUNDED_ARRAY_LENGTH
constexpr int64_t kMaxSize = INT32_MAX - 7;

__device__ __forceinline__ int64_t word_at(const uint8_t* p, int64_t at) {
  return *gl(reinterpret_cast<const int64_t*>(p + at));
}

// [int64 numElements][bitmap][n slots of w bytes, padded to 8]: all of it inside asz bytes.
__device__ __forceinline__ bool header_fits(int64_t n, int64_t w, int64_t asz) {
  return 8 + (((n + 63) >> 6) << 3) + ((n * w + 7) & ~int64_t{7}) <= asz;
}

// ---- split ---------------------------------------------------------------------------------------
// tc[t] / masks[t]: count and ballot of tile t; lk[r] / lv[r] = (start, size) of row r's key / value
// array, written only when the row has a map.
__global__ __launch_bounds__(kTakeThreads) void map_locate(MapSplitArgs a, int64_t* __restrict__ tc,
                                                           uint64_t* __restrict__ masks,
                                                           v2l* __restrict__ lk, v2l* __restrict__ lv) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  const int64_t n = a.nrows;
  const int64_t total = gl(a.row_offsets)[n];
  int64_t V = 0, size = 0;
  bool bad = false, live;
  if (a.nlevels > 0) {
    live = walk_path(a, r, total, &V, &size, &bad);
  } else {                            // a collection schema: the entry is the map
    live = r < n;
    if (live) {
      V = gl(a.row_offsets)[r];
      size = gl(a.row_offsets)[r + 1] - V;
      if (((V | size) & 7) || !span_ok(V, size, total) || size < 8) {
        bad = true;
        live = false;
      }
    }
  }
  int64_t kb = 0;
  if (live) {                         // [int64 keyArrayBytes][key array][value array]
    kb = static_cast<int32_t>(word_at(a.rows, V));
    if (kb < 0 || (kb & 7) || 8 + kb > size || kb < 8 || size - 8 - kb < 8) {
      bad = true;
      live = false;
    }
  }
  bool counts = false;
  if (live) {
    const int32_t nk = static_cast<int32_t>(word_at(a.rows, V + 8));
    const int32_t nv = static_cast<int32_t>(word_at(a.rows, V + 8 + kb));
    counts = nk != nv;
    if (counts || nk < 0 || !header_fits(nk, a.keys.width, kb) ||
        !header_fits(nv, a.vals.width, size - 8 - kb)) {
      bad = true;
      live = false;
    }
  }
  if (bad) raise_at(a.err, kErrBounds, static_cast<uint64_t>(r) | (counts ? kErrCounts : 0));
  const uint64_t m = __ballot(live);
  if (r >= n) return;
  if ((threadIdx.x & 63) == 0) put_tile(r >> 6, m, n, tc, masks, a.out_validity);
  if (live) {
    gl(lk)[r] = v2l{V + 8, kb};
    gl(lv)[r] = v2l{V + 8 + kb, size - 8 - kb};
  }
}

// tc: exclusive scan of the tile counts, *count its total.  Per side, src (NULL: no copy follows) and
// oo (NULL: the side is skipped) receive start and size of entry pos; idx may be NULL.
__global__ __launch_bounds__(kTakeThreads) void map_compact(const uint64_t* __restrict__ masks,
                                                            const v2l* __restrict__ lk,
                                                            const v2l* __restrict__ lv, int64_t n,
                                                            const int64_t* __restrict__ tc,
                                                            const int64_t* __restrict__ count,
                                                            int64_t* __restrict__ idx,
                                                            int64_t* __restrict__ srck,
                                                            int64_t* __restrict__ ook,
                                                            int64_t* __restrict__ srcv,
                                                            int64_t* __restrict__ oov) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (r >= n) return;
  const int lane = static_cast<int>(r & 63);
  const uint64_t m = gl(masks)[r >> 6];
  if ((m >> lane) & 1) {
    const int64_t pos = gl(tc)[r >> 6] + __popcll(m & ((1ull << lane) - 1));
    if (idx) gl(idx)[pos] = r;
    if (ook) {
      const v2l v = gl(lk)[r];
      if (srck) gl(srck)[pos] = v.x;
      gl(ook)[pos] = v.y;
    }
    if (oov) {
      const v2l v = gl(lv)[r];
      if (srcv) gl(srcv)[pos] = v.x;
      gl(oov)[pos] = v.y;
    }
  }
  if (r >= *gl(count)) {              // the entries past the count: this lane's own position
    if (idx) gl(idx)[r] = -1;
    if (ook) gl(ook)[r] = 0;
    if (oov) gl(oov)[r] = 0;
  }
}

// blockIdx.y picks the batch (0: keys, 1: values; `first` shifts it when only the values are copied),
// blockIdx.x the span as in every copy_rows launch: the grid is as wide as the larger side has spans,
// and a workgroup of the smaller side past its last span has no iteration.
__global__ __launch_bounds__(kTakeThreads) void map_copy(const uint8_t* __restrict__ rows, int64_t n,
                                                         MapSide k, const int64_t* __restrict__ srck,
                                                         MapSide v, const int64_t* __restrict__ srcv,
                                                         unsigned first) {
  const bool second = blockIdx.y + first != 0;    // workgroup-uniform
  const int64_t* src = second ? srcv : srck;
  const MapSide s = second ? v : k;
  copy_rows(rows, [=](int64_t j) { return gl(src)[j]; }, n, s.out, s.out_offsets, s.cap);
}

// ---- join ----------------------------------------------------------------------------------------
__device__ __forceinline__ bool value_ok(int64_t s0, int64_t s1, int64_t T) {
  return s0 >= 0 && s0 <= s1 && s1 <= T && !((s0 | s1) & 7) && s1 - s0 >= 8;
}

// info[r] = (key run start, key run size) of output row r, size -1: the row is null or failed (rows
// form: 16 bytes, bit 0 set, slot 0; collection form: the empty map); vsrc[r] = the value run's start.
// out_offsets[r] = the row's size, to be scanned.
__global__ __launch_bounds__(kTakeThreads) void map_join_rows(MapJoinArgs a,
                                                              const int64_t* __restrict__ tr,
                                                              v2l* __restrict__ info,
                                                              int64_t* __restrict__ vsrc) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (r >= a.nrows) return;
  const int64_t t = r >> 6;
  const int lane = static_cast<int>(r & 63);
  const uint64_t w = tile_word(a.validity, t, a.nrows);
  int64_t size = a.prefix ? 16 : 24;
  v2l in{0, -1};
  int64_t vs = 0;
  bool counts = false;
  const bool present = (w >> lane) & 1;
  bool ok = false;
  if (present) {
    const int64_t v = a.validity ? gl(tr)[t] + __popcll(w & ((1ull << lane) - 1)) : r;
    if (v < a.num_values) {
      const int64_t k0 = gl(a.key_offsets)[v], k1 = gl(a.key_offsets)[v + 1];
      const int64_t v0 = gl(a.value_offsets)[v], v1 = gl(a.value_offsets)[v + 1];
      ok = value_ok(k0, k1, gl(a.key_offsets)[a.num_values]) &&
           value_ok(v0, v1, gl(a.value_offsets)[a.num_values]);
      if (ok) {
        const int64_t nk = word_at(a.keys, k0), nv = word_at(a.values, v0);
        counts = nk != nv;
        const int64_t M = 8 + (k1 - k0) + (v1 - v0);
        ok = !counts && nk >= 0 && nk <= kMaxElems && a.prefix + M <= kMaxSize;
        if (ok) {
          in = v2l{k0, k1 - k0};
          vs = v0;
          size = a.prefix + M;
        }
      }
    }
    if (!ok) raise_at(a.err, kErrBounds, static_cast<uint64_t>(r) | (counts ? kErrCounts : 0));
  }
  gl(a.out_offsets)[r] = size;
  gl(info)[r] = in;
  gl(vsrc)[r] = vs;
}

// Rows staged in LDS per round of the write pass: 16 KB, so that LDS leaves 8 workgroups a CU (an
// output row has at least 16 bytes: a 16 KB span is at most two rounds).
constexpr int kMapRows = 512;

struct MapShared {
  int64_t oo[kMapRows + 1];           // output start of the staged rows, and the end of the last one
  int64_t ksrc[kMapRows];             // key run start
  int64_t ksz[kMapRows];              // key run size, -1: a null row / the empty map
  int64_t vsrc[kMapRows];             // value run start
};

__global__ __launch_bounds__(kTakeThreads) void map_join_write(MapJoinArgs a,
                                                               const v2l* __restrict__ info,
                                                               const int64_t* __restrict__ vsrc) {
  __shared__ MapShared sh;
  const int P = a.prefix;
  auto stage = [&](int64_t r, int k) {
    const v2l in = gl(info)[r];
    sh.ksrc[k] = in.x;
    sh.ksz[k] = in.y;
    sh.vsrc[k] = gl(vsrc)[r];
  };
  // Byte x of staged row f (every row has bytes).  A byte of the key or value run: returns true with
  // its address and how many bytes of the run follow it; a generated word: returns false with the word.
  auto locate = [&](int f, int64_t x, uint64_t* word, const uint8_t** at, int64_t* left) {
    const int64_t ksz = sh.ksz[f];
    if (x < P) {                      // the one-field row's bitmap word and slot
      *word = x == 0 ? (ksz < 0 ? 1 : 0)
                     : (ksz < 0 ? 0 : (16ull << 32) | static_cast<uint64_t>(sh.oo[f + 1] - sh.oo[f] - 16));
      return false;
    }
    const int64_t y = x - P;
    if (ksz < 0) {                    // the empty map: [8][0][0]
      *word = y == 0 ? 8 : 0;
      return false;
    }
    if (y == 0) {
      *word = static_cast<uint64_t>(ksz);
      return false;
    }
    if (y < 8 + ksz) {
      *at = a.keys + sh.ksrc[f] + (y - 8);
      *left = 8 + ksz - y;
    } else {
      *at = a.values + sh.vsrc[f] + (y - 8 - ksz);
      *left = sh.oo[f + 1] - sh.oo[f] - x;
    }
    return true;
  };
  write_spans<kMapRows>(sh, a.nrows, a.out_offsets, a.cap, stage,
                        [&](int64_t, int kn, int64_t a0, int64_t b0) {
                          store_located<const uint8_t*>(a.out, a0, b0, sh.oo, kn, locate,
                                                        [](const uint8_t* p) { return p; });
                        });
}

}  // namespace

int launch_map_split(const MapSplitArgs& a, hipStream_t stream) {
  const int64_t n = a.nrows;
  if (n >= (int64_t{1} << 38))        // blocks_of() in 31 bits
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  int64_t* const ook = a.keys.out_offsets;
  int64_t* const oov = a.vals.out_offsets;
  if (n == 0) {
    int st = check_hip(hipMemsetAsync(a.out_count, 0, 8, stream), "memset");
    if (!st && ook) st = check_hip(hipMemsetAsync(ook, 0, 8, stream), "memset");
    if (!st && oov) st = check_hip(hipMemsetAsync(oov, 0, 8, stream), "memset");
    return st;
  }
  const int64_t nt = (n + 63) / 64;
  const int64_t sw = (scan_workspace(n) + 1) & ~int64_t{1};   // >= scan_workspace(nt); even: lk / lv are 16-byte aligned
  const bool ck = ook && a.keys.out && a.keys.cap >= 8, cv = oov && a.vals.out && a.vals.cap >= 8;
  int64_t* ws = nullptr;              // [tile counts x nt][tile masks x nt][scan scratch][lk x 2 n][lv x 2 n][key starts x n][value starts x n]
  int st = dev_alloc((2 * nt + sw + 4 * n + (ck ? n : 0) + (cv ? n : 0)) * 8, stream,
                     reinterpret_cast<void**>(&ws));
  if (st) return st;
  int64_t* tc = ws;
  uint64_t* masks = reinterpret_cast<uint64_t*>(ws + nt);
  int64_t* sws = ws + 2 * nt;
  v2l* lk = reinterpret_cast<v2l*>(sws + sw);
  v2l* lv = lk + n;
  int64_t* srck = ck ? sws + sw + 4 * n : nullptr;
  int64_t* srcv = cv ? sws + sw + 4 * n + (ck ? n : 0) : nullptr;
  hipLaunchKernelGGL(map_locate, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, tc, masks, lk, lv);
  device_scan(tc, nt, a.out_count, sws, stream);
  hipLaunchKernelGGL(map_compact, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, masks, lk, lv, n, tc,
                     a.out_count, a.out_indices, srck, ook, srcv, oov);
  if (ook) device_scan(ook, n, ook + n, sws, stream);
  if (oov) device_scan(oov, n, oov + n, sws, stream);
  if (ck || cv) {
    const unsigned gk = ck ? copy_grid(a.keys.cap) : 0, gv = cv ? copy_grid(a.vals.cap) : 0;
    hipLaunchKernelGGL(map_copy, dim3(std::max(gk, gv), ck && cv ? 2 : 1), dim3(kTakeThreads), 0, stream,
                       a.rows, n, a.keys, srck, a.vals, srcv, ck ? 0u : 1u);
  }
  st = check_hip(hipGetLastError(), "map split launch");
  dev_free(ws, stream);
  return st;
}

int launch_map_join(const MapJoinArgs& a, hipStream_t stream) {
  const int64_t n = a.nrows;
  if (n >= (int64_t{1} << 38))        // blocks_of() in 31 bits
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  if (n == 0) return check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
  const int64_t nt = (n + 63) / 64;
  const int64_t sw = (scan_workspace(n) + 1) & ~int64_t{1};   // even: info is 16-byte aligned
  int64_t* ws = nullptr;              // [info x 2 n][scan scratch][value starts x n][tile ranks x nt + 1]
  int st = dev_alloc((2 * n + sw + n + nt + 1) * 8, stream, reinterpret_cast<void**>(&ws));
  if (st) return st;
  v2l* info = reinterpret_cast<v2l*>(ws);
  int64_t* sws = ws + 2 * n;
  int64_t* vsrc = sws + sw;
  int64_t* tr = a.validity ? vsrc + n : nullptr;
  if (tr) {
    hipLaunchKernelGGL(tile_rank, dim3(blocks_of(nt)), dim3(kTakeThreads), 0, stream, a.validity, n, nt,
                       tr);
    device_scan(tr, nt, tr + nt, sws, stream);
  }
  hipLaunchKernelGGL(map_join_rows, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, tr, info, vsrc);
  device_scan(a.out_offsets, n, a.out_offsets + n, sws, stream);
  if (a.out && a.cap >= 8)
    hipLaunchKernelGGL(map_join_write, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a, info,
                       vsrc);
  st = check_hip(hipGetLastError(), "map join launch");
  dev_free(ws, stream);
  return st;
}

}  // namespace fury
