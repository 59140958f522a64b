// explode.hip -- the elements of a list or map field of a row batch as a batch (fury_row_explode).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of BinaryArray.getStruct / getArray / getMap (FMT/row/binary/BinaryArray.java:137-150, through
// UnsafeTrait.java:160-197) and of BinaryMap.keyArray() / valueArray() (FMT/row/binary/BinaryMap.java:
// 62-77,101-108).  An element slot is (offset << 32) | size relative to the ARRAY's base, and a nested
// row, array or map addresses its variable-length section relative to its own base: the bytes an
// element slot points at are a complete row of the element struct's schema / a complete BinaryArray /
// a complete BinaryMap, so the batch of all elements is a gather, as for extract.hip.
//
// MI355X design:
//   count      lane = source row: the path walk of extract (extract_dev.h) or, for a collection
//              schema, the entry's own extent; a map's keyArrayBytes picks the key or the value
//              array; the element count n is checked against the array's size, so that the header and
//              every slot lie inside the batch.  (A, n) is kept per row, n goes to out_list_offsets,
//              the ballot to out_entry_validity; device_scan makes the Arrow list offsets.
//   locate     lane = ELEMENT, a wave = a 64-element tile, so the work follows the elements and not
//              the rows: one 100,000-element list among empty rows is 1,563 tiles like any other
//              100,000 elements.  The tile finds the row that owns its first element by the
//              wave-cooperative 64-ary search of take_dev.h (last_le) over out_list_offsets, the row of
//              its last element by one 64-entry probe from there (a second search only when more than
//              63 rows end inside the tile), and every lane then advances from the first owner to
//              its own by a binary search of that window -- no steps when one list covers the tile, at
//              most 6 where no empty rows intervene, and never a serial walk over a run of empty rows.
//              Consecutive lanes read consecutive 8-byte slots of one array (coalesced) and share its
//              bitmap word (one address per wave and array: a broadcast).  The ballot of "produces an
//              entry" goes out as the tile's two validity words, its count and its mask; a producing
//              lane stores (absolute source start, size) and its owner row: extract's locate contract
//              with elements for rows.
//   compact    device_scan of the tile counts, compact_entries of extract_dev.h (out_parents /
//              out_ordinals are written here, the ordinal as element index - out_list_offsets[owner]),
//              device_scan of the sizes, then extract's copy (extract_copy of extract_dev.h: copy_rows
//              of take_dev.h over the compacted source starts).
// Row bytes are read with plain loads in count and locate (headers and slots share cache lines with
// the bytes the copy reads next); the copy's loads and stores are take_dev.h's non-temporal ones.
// Bounds (ExplodeArgs, kernels.h): nothing outside [0, total) of the rows buffer is read, the output
// is written only inside [0, min(capacity, needed)), per-element outputs only below elem_cap.
#include "extract_dev.h"

namespace fury {

namespace {

static_assert(sizeof(ExplodeArgs{}.nfields) / sizeof(int32_t) == kMaxNestLevels,
              "a path is as long as a schema is deep");

constexpr int kTileWaves = kTakeThreads / 64;     // element tiles per workgroup of the locate pass

__device__ __forceinline__ uint64_t word_at(const uint8_t* rows, int64_t p) {
  return *gl(reinterpret_cast<const uint64_t*>(rows + p));
}

// arr[r] = (array start A, element count n) of row r, written only when the row has an array;
// out_list_offsets[r] = n (0 for a null or malformed row), to be scanned.
__global__ __launch_bounds__(kTakeThreads) void explode_count(ExplodeArgs a, v2l* __restrict__ arr) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  const int64_t n = a.nrows;
  const int64_t total = gl(a.row_offsets)[n];
  int64_t V = 0, size = 0;
  bool bad = false, live;
  if (a.nlevels > 0) {
    live = walk_path(a, r, total, &V, &size, &bad);
  } else {                            // a collection schema: the entry is the array / map
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
  int64_t A = V, asz = size;
  if (live && a.is_map) {             // [int64 keyArrayBytes][key array][value array]
    const int32_t kb = static_cast<int32_t>(word_at(a.rows, V));
    if (kb < 0 || (kb & 7) || 8 + static_cast<int64_t>(kb) > size) {
      bad = true;
      live = false;
    } else {
      A = a.side ? V + 8 + kb : V + 8;
      asz = a.side ? size - 8 - kb : kb;
      if (asz < 8) {
        bad = true;
        live = false;
      }
    }
  }
  int64_t cnt = 0;
  if (live) {                         // [int64 numElements][bitmap][slots]: all of it inside the array
    const int32_t m = static_cast<int32_t>(word_at(a.rows, A));
    if (m < 0 || 8 + ((static_cast<int64_t>(m) + 63) >> 6) * 8 + 8 * static_cast<int64_t>(m) > asz) {
      bad = true;
      live = false;
    } else {
      cnt = m;
    }
  }
  if (bad) raise_oob(a.err, r);
  const uint64_t m = __ballot(live);
  if (r >= n) return;
  if ((threadIdx.x & 63) == 0 && a.out_entry_validity) {
    const int64_t t = r >> 6;
    gl(a.out_entry_validity)[2 * t] = static_cast<uint32_t>(m);
    if (r + 32 < n) gl(a.out_entry_validity)[2 * t + 1] = static_cast<uint32_t>(m >> 32);
  }
  gl(a.out_list_offsets)[r] = cnt;
  if (live) gl(arr)[r] = v2l{A, cnt};
}

// lo = out_list_offsets after the scan (lo[nrows] = E).  Tile t = elements [64 t, 64 t + 64) of
// min(E, elem_cap); tc[t] / masks[t]: its count and ballot; loc[e] = (source start, size) and
// owner[e] = the source row of element e, written only when the element produces an entry (owner
// may be NULL: not wanted).
__global__ __launch_bounds__(kTakeThreads) void explode_locate(ExplodeArgs a,
                                                               const v2l* __restrict__ arr,
                                                               int64_t* __restrict__ tc,
                                                               uint64_t* __restrict__ masks,
                                                               v2l* __restrict__ loc,
                                                               int64_t* __restrict__ owner) {
  const int lane = threadIdx.x & 63;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kTileWaves + (threadIdx.x >> 6);
  const int64_t cap = a.elem_cap;
  if (64 * t >= cap) return;          // the whole wave
  const int64_t n = a.nrows;
  const int64_t* lo = a.out_list_offsets;
  const int64_t total = gl(a.row_offsets)[n];
  const int64_t Em = min(gl(lo)[n], cap);
  const int64_t e0 = 64 * t, e = e0 + lane;
  bool live = false;
  if (e0 < Em) {                      // wave-uniform: the searches are wave-cooperative
    // rows [r0, rl]: the owner of element e0 ... the owner of the tile's last element.  lo[j] <= e <
    // lo[j + 1] makes row j the owner of e; an empty row never is, since e < E = lo[nrows].
    const int64_t klast = min(e0 + 63, Em - 1);
    const int64_t r0 = last_le(lo, 0, n, e0, lane);
    int64_t rl;
    {
      const bool le = r0 + lane < n && gl(lo)[r0 + lane] <= klast;
      const int c = max(__popcll(__ballot(le)) - 1, 0);
      rl = c < 63 ? r0 + c : last_le(lo, r0 + 63, n - (r0 + 63), klast, lane);
    }
    if (e < Em) {
      int64_t j = r0, hi = rl;
      while (j < hi) {
        const int64_t mid = (j + hi + 1) >> 1;
        if (gl(lo)[mid] <= e) j = mid;
        else hi = mid - 1;
      }
      const v2l an = gl(arr)[j];      // 0 <= i < an.y: the count pass checked header and slots
      const int64_t A = an.x, i = e - gl(lo)[j];
      const int64_t bm = ((an.y + 63) >> 6) << 3;
      if (!((word_at(a.rows, A + 8 + ((i >> 6) << 3)) >> (i & 63)) & 1)) {
        const uint64_t s = word_at(a.rows, A + 8 + bm + 8 * i);
        const int32_t off = static_cast<int32_t>(s >> 32), len = static_cast<int32_t>(s);
        if (off < 0 || len < 0 || ((off | len) & 7) || !span_ok(A + off, len, total) ||
            len < a.elem_min || (a.elem_exact && len != a.elem_min)) {
          raise_oob(a.err, j);
        } else {
          live = true;
          gl(loc)[e] = v2l{A + off, len};
          if (owner) gl(owner)[e] = j;
        }
      }
    }
  }
  const uint64_t m = __ballot(live);
  if (lane == 0) put_tile(t, m, cap, tc, masks, a.out_validity);
}

// tc: exclusive scan of the tile counts, *count its total.  parents / ordinals / src may be NULL.
__global__ __launch_bounds__(kTakeThreads) void explode_compact(const uint64_t* __restrict__ masks,
                                                                const v2l* __restrict__ loc,
                                                                int64_t cap,
                                                                const int64_t* __restrict__ tc,
                                                                const int64_t* __restrict__ count,
                                                                const int64_t* __restrict__ owner,
                                                                const int64_t* __restrict__ lo,
                                                                int64_t* __restrict__ parents,
                                                                int32_t* __restrict__ ordinals,
                                                                int64_t* __restrict__ src,
                                                                int64_t* __restrict__ oo) {
  compact_entries(masks, loc, cap, tc, count, src, oo,
                  [=](int64_t pos, int64_t e) {
                    if (!owner) return;
                    const int64_t j = gl(owner)[e];
                    if (parents) gl(parents)[pos] = j;
                    if (ordinals) gl(ordinals)[pos] = static_cast<int32_t>(e - gl(lo)[j]);
                  },
                  [=](int64_t e) {
                    if (parents) gl(parents)[e] = -1;
                    if (ordinals) gl(ordinals)[e] = -1;
                  });
}

}  // namespace

int launch_explode(const ExplodeArgs& a, hipStream_t stream) {
  const int64_t n = a.nrows;
  const bool fill = a.out_offsets != nullptr;     // not the count form
  const int64_t cap = fill ? a.elem_cap : 0;
  if (n >= (int64_t{1} << 38) || cap >= (int64_t{1} << 38))     // blocks_of() in 31 bits
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  int st = FURY_OK;
  if (n == 0 || (fill && cap == 0)) {
    if (fill) {
      st = check_hip(hipMemsetAsync(a.out_count, 0, 8, stream), "memset");
      if (!st) st = check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
    }
    if (n == 0) {
      if (!st) st = check_hip(hipMemsetAsync(a.out_list_offsets, 0, 8, stream), "memset");
      return st;
    }
    if (st) return st;
  }
  const int64_t nt = (cap + 63) / 64;
  // even: arr and loc are 16-byte aligned; >= scan_workspace(nt)
  const int64_t sw = (std::max(scan_workspace(n), scan_workspace(cap)) + 1) & ~int64_t{1};
  const bool copy = a.out && a.cap >= 8;
  const bool own = a.out_parents || a.out_ordinals;
  int64_t* ws = nullptr;              // [arr x 2 n][scan scratch][tile counts x nt][tile masks x nt][loc x 2 cap][source starts x cap][owners x cap]
  st = dev_alloc((2 * n + sw + 2 * nt + 2 * cap + (copy ? cap : 0) + (own ? cap : 0)) * 8, stream,
                 reinterpret_cast<void**>(&ws));
  if (st) return st;
  v2l* arr = reinterpret_cast<v2l*>(ws);
  int64_t* sws = ws + 2 * n;
  int64_t* tc = sws + sw;
  uint64_t* masks = reinterpret_cast<uint64_t*>(tc + nt);
  v2l* loc = reinterpret_cast<v2l*>(tc + 2 * nt);
  int64_t* src = copy ? tc + 2 * nt + 2 * cap : nullptr;
  int64_t* owner = own ? tc + 2 * nt + 2 * cap + (copy ? cap : 0) : nullptr;
  hipLaunchKernelGGL(explode_count, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, arr);
  device_scan(a.out_list_offsets, n, a.out_list_offsets + n, sws, stream);
  if (cap > 0) {
    hipLaunchKernelGGL(explode_locate, dim3(static_cast<unsigned>((nt + kTileWaves - 1) / kTileWaves)),
                       dim3(kTakeThreads), 0, stream, a, arr, tc, masks, loc, owner);
    device_scan(tc, nt, a.out_count, sws, stream);
    hipLaunchKernelGGL(explode_compact, dim3(blocks_of(cap)), dim3(kTakeThreads), 0, stream, masks, loc,
                       cap, tc, a.out_count, owner, a.out_list_offsets, a.out_parents, a.out_ordinals,
                       src, a.out_offsets);
    device_scan(a.out_offsets, cap, a.out_offsets + cap, sws, stream);
    if (copy)
      hipLaunchKernelGGL(extract_copy, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a.rows,
                         src, cap, a.out, a.out_offsets, a.cap);
  }
  st = check_hip(hipGetLastError(), "explode launch");
  dev_free(ws, stream);
  return st;
}

}  // namespace fury
