// partition.hip -- split the rows of a batch by a per-row partition id, and glue batches of one
// schema end to end (fury_row_partition / fury_row_concat).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): as take.hip, the
// batch form of BinaryRow.copy() (FMT/row/binary/BinaryRow.java:173-179).  A row is its bytes,
// unchanged, at a new position; only offsets and bytes are used and the schema may be anything.
//
// MI355X design.  Partition is a filter whose row list is a STABLE sort of the rows by key, key = the
// id of a kept row, num_parts (the drop bucket) otherwise: LSD radix passes of 8 bits, one when
// num_parts + 1 <= 256, else two.  A pass, over tiles of kPartTile rows in row order:
//   part_hist     digit counts of a tile (LDS integer atomics: counts do not depend on their order),
//                 stored digit-major, hist[digit][tile]
//   device_scan   over 256 x tiles entries: scanned[digit][tile] = rows that sort before the tile's
//                 rows of that digit
//   part_scatter  a wave owns kPartWaveRows consecutive rows of the tile.  Its digit counts (LDS
//                 atomics again) are prefixed over the tile's four waves on top of scanned[][tile],
//                 then the wave walks its rows 64 at a time in row order: the lanes that hold the
//                 same digit find each other by 8 ballots (one per digit bit), a lane's rank is the
//                 popcount of its peers below it, the lowest peer advances the wave's counter.  No
//                 returning atomic decides a position, so the order is the source order and every
//                 run gives the same buffers.
// The last pass writes, at a row's output position, its source row, its size (extent validated as in
// filter_write) and its key; part_finish then finds every partition's first row by a binary search of
// the sorted keys and fills the entries at or past the count by the lane of that position.  From
// there the call is launch_filter's second half (copy_selected: offsets scan, take_copy or the fixed
// copy with the count on the device).
// Concat is an instance of copy_rows: the source of output row j is found in the <= 32-entry table of
// row bases in the argument block, and a row start is carried relative to the first source's rows.
#include "take_dev.h"

namespace fury {

namespace {

constexpr int kPartRounds = 16;                           // rounds of 64 rows per wave
constexpr int kPartWaveRows = 64 * kPartRounds;
constexpr int kPartWaves = kTakeThreads / 64;
constexpr int kPartTile = kPartWaves * kPartWaveRows;     // 4096 rows

// Where a pass takes its rows from: the first pass reads the ids in row order, the second one the
// keys and row numbers the first pass left in its order.
struct PartIn {
  const int32_t* ids;
  const int32_t* keys;
  const int64_t* perm;
  int32_t num_parts;
  int32_t shift;                      // the pass's digit = (key >> shift) & 255
};

struct PartOut {
  int64_t* perm;                      // not the last pass: row numbers in this pass's order
  int32_t* keys;                      // keys in this pass's order
  const int64_t* ro;                  // the last pass (NULL: fixed-size rows) ...
  int64_t nrows;
  int64_t* idx;                       // optional
  int64_t* pos;                       // optional
  int64_t* oo;                        // sizes; NULL for fixed-size rows
  uint32_t* err;
};

template <bool kFirst>
__device__ __forceinline__ uint32_t part_key(const PartIn& in, int64_t i) {
  if (!kFirst) return static_cast<uint32_t>(gl(in.keys)[i]);
  const uint32_t id = static_cast<uint32_t>(gl(in.ids)[i]);
  const uint32_t np = static_cast<uint32_t>(in.num_parts);
  return id < np ? id : np;           // negative ids compare as large ones
}

// Orders a wave's own LDS accesses: what its lanes read before, the lowest peer may overwrite after.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <bool kFirst>
__global__ __launch_bounds__(kTakeThreads) void part_hist(PartIn in, int64_t n, int64_t nt,
                                                          int64_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kPartTile + tid;
  for (int r = 0; r < kPartTile / kTakeThreads; r++) {
    const int64_t i = i0 + r * kTakeThreads;
    if (i < n) atomicAdd(&h[(part_key<kFirst>(in, i) >> in.shift) & 255], 1u);
  }
  __syncthreads();
  gl(hist)[tid * nt + blockIdx.x] = h[tid];
}

template <bool kFirst, bool kLast>
__global__ __launch_bounds__(kTakeThreads) void part_scatter(PartIn in, int64_t n, int64_t nt,
                                                             const int64_t* __restrict__ scanned,
                                                             PartOut o) {
  __shared__ uint32_t cnt[kPartWaves][256];
  __shared__ int64_t base[kPartWaves][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int k = 0; k < kPartWaves; k++) cnt[k][tid] = 0;
  __syncthreads();
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kPartTile + w * kPartWaveRows + lane;
  for (int r = 0; r < kPartRounds; r++) {
    const int64_t i = i0 + r * 64;
    if (i < n) atomicAdd(&cnt[w][(part_key<kFirst>(in, i) >> in.shift) & 255], 1u);
  }
  __syncthreads();
  {                                   // thread = digit: the waves' bases, in wave order
    int64_t run = gl(scanned)[tid * nt + blockIdx.x];
    for (int k = 0; k < kPartWaves; k++) {
      base[k][tid] = run;
      run += cnt[k][tid];
    }
  }
  __syncthreads();
  for (int r = 0; r < kPartRounds; r++) {           // every lane runs every round: ballots
    const int64_t i = i0 + r * 64;
    const bool valid = i < n;
    const uint32_t key = valid ? part_key<kFirst>(in, i) : 0;
    const uint32_t d = (key >> in.shift) & 255;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint64_t below = peers & ((1ull << lane) - 1);
    int64_t p = -1;
    if (valid) p = base[w][d] + __popcll(below);
    wave_lds_sync();
    if (valid && below == 0) base[w][d] += __popcll(peers);
    wave_lds_sync();
    // p < n and src < n whenever the ids are what part_hist counted; ids changed under the call
    // write nothing outside the arrays
    if (!valid || static_cast<uint64_t>(p) >= static_cast<uint64_t>(n)) continue;
    const int64_t src = kFirst ? i : gl(in.perm)[i];
    if (!kFirst && static_cast<uint64_t>(src) >= static_cast<uint64_t>(n)) continue;
    gl(o.keys)[p] = static_cast<int32_t>(key);
    if (!kLast) {
      gl(o.perm)[p] = src;
    } else if (key < static_cast<uint32_t>(in.num_parts)) {
      if (o.idx) gl(o.idx)[p] = src;
      if (o.pos) gl(o.pos)[src] = p;
      if (o.oo) {
        bool ok;
        const int64_t sz = row_extent(o.ro, o.nrows, gl(o.ro)[o.nrows], src, &ok);
        if (!ok) raise_oob(o.err, src);
        gl(o.oo)[p] = sz;
      }
    } else if (o.pos) {
      gl(o.pos)[src] = -1;
    }
  }
}

// skeys: the keys in output order (non-decreasing, num_parts at or past the count).  Lane g <=
// num_parts: part_rows[g] = the first position whose key is >= g.  Lane g < n at or past the count:
// its own entries of idx / oo.
__global__ __launch_bounds__(kTakeThreads) void part_finish(const int32_t* __restrict__ skeys,
                                                            int64_t n, int32_t num_parts,
                                                            int64_t* __restrict__ part_rows,
                                                            int64_t* __restrict__ idx,
                                                            int64_t* __restrict__ oo) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (g < n && gl(skeys)[g] == num_parts) {
    if (idx) gl(idx)[g] = -1;
    if (oo) gl(oo)[g] = 0;
  }
  if (g <= num_parts) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (gl(skeys)[mid] < g) lo = mid + 1;
      else hi = mid;
    }
    gl(part_rows)[g] = lo;
  }
}

// ---- concat ------------------------------------------------------------------------------------
struct ConcatRow {
  const uint8_t* rows;
  const int64_t* ro;
  int64_t i, nrows;                   // row i of a source of nrows rows
};

// The source of output row j < a.n: the last one whose base is <= j (an empty source shares its base
// with the next one).  The table is read with wave-uniform indices only.
__device__ __forceinline__ ConcatRow concat_row(const ConcatArgs& a, int64_t j) {
  ConcatRow r{a.rows[0], a.ro[0], j, a.base[1]};
  for (int s = 1; s < a.nsrc; s++) {
    if (a.base[s] <= j) {
      r.rows = a.rows[s];
      r.ro = a.ro[s];
      r.i = j - a.base[s];
      r.nrows = a.base[s + 1] - a.base[s];
    }
  }
  return r;
}

__global__ __launch_bounds__(kTakeThreads) void concat_sizes(ConcatArgs a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (j >= a.n) return;
  const ConcatRow r = concat_row(a, j);
  bool ok;
  const int64_t sz = row_extent(r.ro, r.nrows, gl(r.ro)[r.nrows], r.i, &ok);
  if (!ok) raise_oob(a.err, j);
  gl(a.out_offsets)[j] = sz;
}

// oo: a.out_offsets, or the launcher's own offsets of fixed-size rows; anchor: the rows of the first
// source that has any, which copy_rows' source starts are relative to.
__global__ __launch_bounds__(kTakeThreads) void concat_copy(ConcatArgs a,
                                                            const uint8_t* __restrict__ anchor,
                                                            const int64_t* __restrict__ oo) {
  copy_rows(
      anchor,
      [&](int64_t j) {
        const ConcatRow r = concat_row(a, j);
        const int64_t at = r.ro ? gl(r.ro)[r.i] : r.i * a.fixed_size;
        return static_cast<int64_t>(reinterpret_cast<uintptr_t>(r.rows) -
                                    reinterpret_cast<uintptr_t>(anchor)) + at;
      },
      a.n, a.out, oo, a.cap);
}

}  // namespace

int launch_partition(const TakeArgs& a, const int32_t* part_ids, int32_t num_parts,
                     int64_t* out_part_rows, int64_t* out_indices, int64_t* out_positions,
                     hipStream_t stream) {
  const int64_t n = a.nrows;
  int st = too_large(n, a.fixed_size);
  if (st) return st;
  if (n == 0) {
    st = check_hip(hipMemsetAsync(out_part_rows, 0, (static_cast<size_t>(num_parts) + 1) * 8, stream),
                   "memset");
    if (!st && a.out_offsets) st = check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
    return st;
  }
  const bool fixed = !a.row_offsets;
  const bool two = num_parts + 1 > 256;             // passes: the keys are [0, num_parts]
  const int64_t nt = (n + kPartTile - 1) / kPartTile;
  const int64_t nh = 256 * nt;
  const int64_t sw = std::max(scan_workspace(nh), scan_workspace(n));
  const int64_t nk = (n + 1) / 2;                   // n int32 keys, in 8-byte words
  const bool own_idx = a.out && !out_indices;       // the copy needs the row numbers
  // [histogram x nh][its total][scan scratch][sorted keys][first pass: row numbers, keys][row numbers]
  int64_t* ws = nullptr;
  st = dev_alloc((nh + 1 + sw + nk + (two ? n + nk : 0) + (own_idx ? n : 0)) * 8, stream,
                 reinterpret_cast<void**>(&ws));
  if (st) return st;
  int64_t* hist = ws;
  int64_t* sws = hist + nh + 1;
  int32_t* skeys = reinterpret_cast<int32_t*>(sws + sw);
  int64_t* perm = sws + sw + nk;
  int32_t* keys0 = reinterpret_cast<int32_t*>(perm + n);
  int64_t* idx = own_idx ? sws + sw + nk + (two ? n + nk : 0) : out_indices;
  const dim3 grid(static_cast<unsigned>(nt)), block(kTakeThreads);
  PartIn in{part_ids, nullptr, nullptr, num_parts, 0};
  PartOut last{nullptr, skeys, a.row_offsets, n, idx, out_positions, fixed ? nullptr : a.out_offsets,
               a.err};
  hipLaunchKernelGGL(part_hist<true>, grid, block, 0, stream, in, n, nt, hist);
  device_scan(hist, nh, hist + nh, sws, stream);
  if (!two) {
    hipLaunchKernelGGL((part_scatter<true, true>), grid, block, 0, stream, in, n, nt, hist, last);
  } else {
    PartOut mid{};
    mid.perm = perm;
    mid.keys = keys0;
    hipLaunchKernelGGL((part_scatter<true, false>), grid, block, 0, stream, in, n, nt, hist, mid);
    in = PartIn{nullptr, keys0, perm, num_parts, 8};
    hipLaunchKernelGGL(part_hist<false>, grid, block, 0, stream, in, n, nt, hist);
    device_scan(hist, nh, hist + nh, sws, stream);
    hipLaunchKernelGGL((part_scatter<false, true>), grid, block, 0, stream, in, n, nt, hist, last);
  }
  hipLaunchKernelGGL(part_finish, dim3(blocks_of(std::max<int64_t>(n, num_parts + 1))), block, 0,
                     stream, skeys, n, num_parts, out_part_rows, idx,
                     fixed ? nullptr : a.out_offsets);
  copy_selected(a, idx, out_part_rows + num_parts, sws, stream);
  st = check_hip(hipGetLastError(), "partition launch");
  dev_free(ws, stream);
  return st;
}

int launch_concat(const ConcatArgs& a, hipStream_t stream) {
  const int64_t n = a.n;
  int st = too_large(n, a.fixed_size);
  if (st) return st;
  if (n == 0) return a.out_offsets ? check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset")
                                   : FURY_OK;
  const uint8_t* anchor = nullptr;
  for (int s = 0; s < a.nsrc && !anchor; s++)
    if (a.base[s + 1] > a.base[s]) anchor = a.rows[s];
  const bool copy = a.out && a.cap >= 8;
  int64_t* ws = nullptr;
  const int64_t* oo = a.out_offsets;
  if (a.fixed) {
    if (!oo && copy) {                // copy_rows wants the offsets the caller does not
      st = dev_alloc((n + 1) * 8, stream, reinterpret_cast<void**>(&ws));
      if (st) return st;
      oo = ws;
    }
    if (oo)
      hipLaunchKernelGGL(fixed_offsets, dim3(blocks_of(n + 1)), dim3(kTakeThreads), 0, stream,
                         const_cast<int64_t*>(oo), n, static_cast<const int64_t*>(nullptr),
                         a.fixed_size);
  } else {
    st = dev_alloc(scan_workspace(n) * 8, stream, reinterpret_cast<void**>(&ws));
    if (st) return st;
    hipLaunchKernelGGL(concat_sizes, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a);
    device_scan(a.out_offsets, n, a.out_offsets + n, ws, stream);
  }
  if (copy)
    hipLaunchKernelGGL(concat_copy, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a, anchor,
                       oo);
  st = check_hip(hipGetLastError(), "concat launch");
  if (ws) dev_free(ws, stream);
  return st;
}

}  // namespace fury
