// aggregate.hip -- per-group COUNT / SUM / MIN / MAX / ARGMIN / ARGMAX of value fields of one batch
// whose rows carry a group id (fury_row_aggregate): the last step of a GROUP BY.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading every
// row's value field with BinaryRow's getters (FMT/row/binary/BinaryRow.java, UnsafeTrait.java:68-197)
// and folding it into the accumulator of the row's group; the reference ships no aggregation, so the
// rules are this library's and are numbered in include/fury_row.h.  The value order is fury_row_compare's
// (order_fixed, value_compare in keys_dev.h).
//
// MI355X design.  Contention decides it, not the input: every adder on one address is an order of
// magnitude slower than spread adds, so values are combined on chip before anything reaches memory.
// Workspace: 3 words per (aggregate, group) cell -- accumulator, count, row number -- at
// ws[j * G + g], ws[N + ...], ws[2 N + ...], N = naggs * G.
//   init      one lane per cell: the accumulator's identity (0; ~0 for a minimum; NO_ROW for the
//             compare-and-swap cell of a var-length ARG), count 0, row NO_ROW.
//   combine   lane = row, 256-thread workgroups.  A lane reads its id and row offset, then the bitmap
//             word and the slot word of kKeyGroup aggregates with the loads in flight together, as
//             pair_keys_equal does for a key group; the descriptors are wave-uniform kernel arguments.
//             Ordered values travel as order_fixed words, so MIN / MAX / ARG of every fixed-width type
//             is one unsigned 64-bit min / max.
//             1. Wave: lanes are cut into runs of equal ids (a ballot of the run heads); unless every
//                lane is a run of its own, a segmented shuffle reduction (6 steps, value and count)
//                leaves each run's fold in its head lane.  One group, sorted ids and partitioned rows
//                come out as one operation per wave and aggregate.
//             2. LDS path, G * naggs <= kAggLdsCells (2048 cells, 16 bytes each, at most 32 KiB): at
//                most kAggMaxBlocks persistent workgroups walk the tiles; head lanes fold into the
//                workgroup's LDS cells with LDS atomics, and after one barrier the workgroup issues
//                one global atomic per touched cell and word.  Global atomics per call are bounded by
//                kAggMaxBlocks * cells, whatever nrows is.
//                Global path, more cells: one tile per workgroup, head lanes go to the workspace with
//                global atomics; ids spread over that many cells do not pile up on one address.
//             3. ARGMIN / ARGMAX of STRING / BINARY / DECIMAL cannot travel as a word: the cell holds a
//                row number.  As group.hip lowers a slot: a lane reads the cell, compares its value with
//                that row's (value_compare, ties to the smaller row number) and issues a
//                compare-and-swap only when it would win; a failed one returns the new holder, which is
//                strictly better, and the lane compares again.  A hot group costs a cached load and a
//                compare per row, not an atomic.  These cells live in the workspace on both paths.
//   resolve   only with an ARG over a fixed-width type or BOOL: lane = row, the rows whose order word
//             equals the group's winner lower the row cell with an unsigned atomicMin, issued only
//             when the cell read is greater (rule 5's tie-break).
//   finalise  one lane per cell: the order word back to the value's bytes (rule 4), the empty-group
//             values (rule 2), every out / out_count entry stored once (rule 6), plain vector stores.
// Dispatch is a pure function of the arguments: aggregate_uses_lds(num_groups, num_aggs) picks the
// path, the presence of a fixed-width ARG the resolve launch, of a var-length ARG the instantiation
// that compiles note 3 (VAR; the other one has no payload loop and no compare-and-swap).
// Orderings the atomics rely on: none beyond atomicity (relaxed, agent scope; LDS atomics are ordered
// before the flush by the workgroup barrier).  The batch and the ids are read-only and were written
// before the launch; workspace cells are read with plain loads only after a kernel boundary, but for
// the ARG cell, which is read with an atomic load inside the kernel.  No lane waits for another: the
// only retry loop is the compare-and-swap above, and each retry means the cell got strictly better.
// Results do not depend on scheduling, but for the float sums: integer add, min and max are
// associative and commutative, and the ARG cell ends at the least (value, row) pair whatever the order
// of arrival.  A float sum starts from +0.0 and adds in an unspecified order (rule 3).
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok); a row that holds an ARG
// cell passed them when it entered.  All address arithmetic is int64.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kAggThreads = 256;
constexpr int kAggMaxBlocks = 1024;               // LDS path: persistent workgroups
constexpr uint64_t kNoRow = ~uint64_t(0);         // as int64: -1, the ARG result of a group without values

using CAggRec = __attribute__((address_space(4))) const AggRec;

__device__ __forceinline__ CAggRec* recs_of(const AggArgs& a) { return (CAggRec*)(a.rec); }

__device__ __forceinline__ int64_t row_base(const AggArgs& a, int64_t r) {
  return a.side.row_offsets ? gl(a.side.row_offsets)[r] : r * a.side.fixed_size;
}

__device__ __forceinline__ uint64_t agg_identity(int combine) {
  return combine == kAggMin ? ~uint64_t(0) : combine == kAggArgVar ? kNoRow : 0;
}

__device__ __forceinline__ uint64_t agg_fold(int combine, uint64_t x, uint64_t y) {
  switch (combine) {
    case kAggAddInt: return x + y;
    case kAggAddFloat: return __double_as_longlong(__longlong_as_double(x) + __longlong_as_double(y));
    case kAggMin: return x < y ? x : y;
    case kAggMax: return x > y ? x : y;
    default: return 0;
  }
}

// Folds v into *cell (LDS or workspace) with the atomic of `combine`.
__device__ __forceinline__ void agg_apply(int combine, uint64_t* cell, uint64_t v) {
  switch (combine) {
    case kAggAddInt: atomicAdd(reinterpret_cast<unsigned long long*>(cell), v); break;
    case kAggAddFloat: atomicAdd(reinterpret_cast<double*>(cell), __longlong_as_double(v)); break;
    case kAggMin: atomicMin(reinterpret_cast<unsigned long long*>(cell), v); break;
    case kAggMax: atomicMax(reinterpret_cast<unsigned long long*>(cell), v); break;
    default: break;
  }
}

// The word a non-null kFixed / kBool value contributes: the sign-extended integer, the widened double,
// or the order word.
__device__ __forceinline__ uint64_t agg_value(CAggRec& c, uint64_t slot) {
  const int sh = 64 - 8 * c.width;
  switch (c.combine) {
    case kAggAddInt: return static_cast<uint64_t>(static_cast<int64_t>(slot << sh) >> sh);
    case kAggAddFloat:
      return c.width == 4 ? static_cast<uint64_t>(__double_as_longlong(
                                static_cast<double>(__uint_as_float(static_cast<uint32_t>(slot)))))
                          : slot;
    default: return c.kind == kBool ? static_cast<uint64_t>((slot & 0xff) != 0) : order_fixed(slot, c.width, c.cls);
  }
}

// order_fixed undone: the value's bytes as rule 4 stores them.
__device__ __forceinline__ uint64_t agg_unorder(CAggRec& c, uint64_t w) {
  if (c.kind == kBool) return w;
  const uint64_t mask = ~uint64_t(0) >> (64 - 8 * c.width);
  const uint64_t sign = uint64_t(1) << (8 * c.width - 1);
  if (c.cls == kOrdFloat) return (w & sign) ? w ^ sign : ~w & mask;
  const int sh = 64 - 8 * c.width;
  return static_cast<uint64_t>(static_cast<int64_t>((w ^ sign) << sh) >> sh);
}

// Design note 3: row i (base, slot word, n payload bytes; its span is inside the batch) offers itself
// to the ARG cell of its group.
__device__ __forceinline__ void arg_var_offer(const AggArgs& a, CAggRec& c, uint64_t* cell, int64_t i,
                                              int64_t base, uint64_t slot, int64_t n, int64_t total) {
  PairRow pr[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    pr[s].rows = a.side.rows;
    pr[s].total = total;
    pr[s].bitmap_bytes = a.side.bitmap_bytes;
    pr[s].ok = true;
    pr[s].base = base;
  }
  const bool want_max = c.op == FURY_AGG_ARGMAX;
  uint64_t w = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    if (w != kNoRow) {
      const int64_t r = static_cast<int64_t>(w);
      pr[1].base = row_base(a, r);
      const uint64_t held = load8(a.side.rows + pr[1].base + a.side.bitmap_bytes + 8 * static_cast<int64_t>(c.slot));
      bool bad = false;                           // the holder passed the bounds when it entered
      const int64_t m = slot_count(c.kind, c.width, held, pr[1].base, a.side.rows, total, &bad);
      if (bad) return;
      int cmp = value_compare<true>(c.kind, c.width, c.cls, pr, slot, held, n, m);
      if (want_max) cmp = -cmp;
      if (cmp > 0 || (cmp == 0 && r <= i)) return;    // the holder stays
    }
    const uint64_t seen = atomicCAS(reinterpret_cast<unsigned long long*>(cell), w, static_cast<uint64_t>(i));
    if (seen == w) return;
    w = seen;                                     // another lane made progress: compare with the new holder
  }
}

__global__ __launch_bounds__(kAggThreads) void agg_init(AggArgs a) {
  const int j = blockIdx.y;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kAggThreads + threadIdx.x;
  if (g >= a.num_groups) return;
  const int64_t N = a.num_groups * a.naggs, cell = j * a.num_groups + g;
  gl(a.ws)[cell] = agg_identity(recs_of(a)[j].combine);
  gl(a.ws)[N + cell] = 0;
  gl(a.ws)[2 * N + cell] = kNoRow;
}

// LDS: design note 2's LDS path (dynamic LDS: 2 words per cell), else the global path.  VAR: some
// aggregate is an ARG over STRING / BINARY / DECIMAL; VAR = false compiles no payload loop.
template <bool LDS, bool VAR>
__global__ __launch_bounds__(kAggThreads) void agg_combine(AggArgs a, int64_t ntiles) {
  extern __shared__ uint64_t lds[];
  const int64_t G = a.num_groups;
  const int64_t N = G * a.naggs;
  if (LDS) {
    for (int j = 0; j < a.naggs; j++) {
      const uint64_t id0 = agg_identity(recs_of(a)[j].combine);
      for (int64_t g = threadIdx.x; g < G; g += kAggThreads) {
        lds[j * G + g] = id0;
        lds[N + j * G + g] = 0;
      }
    }
    __syncthreads();
  }
  const int64_t total = a.side.row_offsets ? gl(a.side.row_offsets)[a.side.nrows]
                                           : a.side.nrows * a.side.fixed_size;
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i = t * kAggThreads + threadIdx.x;
    const bool active = i < a.side.nrows;
    int64_t id = -1, base = 0;
    if (active) {
      id = a.group_ids ? gl(a.group_ids)[i] : 0;
      base = row_base(a, i);
    }
    bool ok = active && static_cast<uint64_t>(id) < static_cast<uint64_t>(G);
    if (ok && !row_ok(base, a.side.fixed_size, total)) {
      raise_oob(a.err, i);
      ok = false;
    }
    if (!ok) id = -1;
    // runs of equal ids in the wave: [lane, end) is what is left of this lane's run
    const int64_t prev = __shfl_up(static_cast<long long>(id), 1);
    const bool head = lane == 0 || prev != id;
    const uint64_t heads = __ballot(head);
    const uint64_t after = lane == 63 ? 0 : heads >> (lane + 1);
    const int end = after ? lane + __ffsll(static_cast<unsigned long long>(after)) : 64;
    const bool solo = heads == ~uint64_t(0);      // wave-uniform: nothing to combine
    const uint8_t* hdr = a.side.rows + base;
    for (int j0 = 0; j0 < a.naggs; j0 += kKeyGroup) {
      uint64_t bits[kKeyGroup], slot[kKeyGroup];
#pragma unroll
      for (int u = 0; u < kKeyGroup; u++) {       // every header word of the group of aggregates
        bits[u] = ~uint64_t(0);                   // a row that takes no part: every value null
        slot[u] = 0;
        if (j0 + u < a.naggs && ok) {
          CAggRec& c = recs_of(a)[j0 + u];
          const int32_t f = c.slot;
          if (f < 0) {
            bits[u] = 0;                          // COUNT(*)
          } else {
            bits[u] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
            if (c.combine != kAggNone) slot[u] = load8(hdr + a.side.bitmap_bytes + 8 * static_cast<int64_t>(f));
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kKeyGroup; u++) {
        if (j0 + u >= a.naggs) break;
        const int j = j0 + u;
        CAggRec& c = recs_of(a)[j];
        const int combine = c.combine;
        const bool isnull = (bits[u] >> (c.slot & 63)) & 1;
        uint64_t v = agg_identity(combine);
        uint32_t cnt = 0;
        if (!isnull) {
          if (VAR && combine == kAggArgVar) {
            bool bad = false;
            const int64_t n = slot_count(c.kind, c.width, slot[u], base, a.side.rows, total, &bad);
            if (bad) {
              raise_oob(a.err, i);                // rule 7: null for this aggregate
            } else {
              cnt = 1;
              arg_var_offer(a, c, a.ws + j * G + id, i, base, slot[u], n, total);
            }
          } else {
            cnt = 1;
            if (combine != kAggNone) v = agg_value(c, slot[u]);
          }
        }
        if (!solo) {
          for (int d = 1; d < 64; d <<= 1) {
            const uint64_t ov = __shfl_down(static_cast<unsigned long long>(v), d);
            const uint32_t oc = __shfl_down(cnt, d);
            if (lane + d < end) {
              v = agg_fold(combine, v, ov);
              cnt += oc;
            }
          }
        }
        if (head && cnt) {                        // cnt > 0: the run's rows are ok, id is in [0, G)
          const int64_t cell = j * G + id;
          uint64_t* acc = LDS ? lds + cell : a.ws + cell;
          uint64_t* num = LDS ? lds + N + cell : a.ws + N + cell;
          if (combine != kAggNone && combine != kAggArgVar) agg_apply(combine, acc, v);
          atomicAdd(reinterpret_cast<unsigned long long*>(num), static_cast<unsigned long long>(cnt));
        }
      }
    }
  }
  if (LDS) {                                      // one global operation per touched cell and word
    __syncthreads();
    for (int j = 0; j < a.naggs; j++) {
      const int combine = recs_of(a)[j].combine;
      for (int64_t g = threadIdx.x; g < G; g += kAggThreads) {
        const int64_t cell = j * G + g;
        const uint64_t cnt = lds[N + cell];
        if (cnt == 0) continue;
        if (combine != kAggNone && combine != kAggArgVar) agg_apply(combine, a.ws + cell, lds[cell]);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.ws + N + cell), static_cast<unsigned long long>(cnt));
      }
    }
  }
}

// ARGMIN / ARGMAX over kFixed / kBool: the smallest row whose order word is the group's winner.
__global__ __launch_bounds__(kAggThreads) void agg_resolve(AggArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kAggThreads + threadIdx.x;
  if (i >= a.side.nrows) return;
  const int64_t G = a.num_groups, N = G * a.naggs;
  const int64_t total = a.side.row_offsets ? gl(a.side.row_offsets)[a.side.nrows]
                                           : a.side.nrows * a.side.fixed_size;
  const int64_t id = a.group_ids ? gl(a.group_ids)[i] : 0;
  const int64_t base = row_base(a, i);
  if (static_cast<uint64_t>(id) >= static_cast<uint64_t>(G)) return;
  if (!row_ok(base, a.side.fixed_size, total)) return;        // raised by the combine pass
  const uint8_t* hdr = a.side.rows + base;
  for (int j = 0; j < a.naggs; j++) {
    CAggRec& c = recs_of(a)[j];
    if (!c.resolve) continue;
    const uint64_t bits = load8(hdr + 8 * static_cast<int64_t>(c.slot >> 6));
    const uint64_t slot = load8(hdr + a.side.bitmap_bytes + 8 * static_cast<int64_t>(c.slot));
    if ((bits >> (c.slot & 63)) & 1) continue;
    const int64_t cell = j * G + id;
    if (agg_value(c, slot) != gl(a.ws)[cell]) continue;
    uint64_t* row = a.ws + 2 * N + cell;
    if (__hip_atomic_load(row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > static_cast<uint64_t>(i))
      atomicMin(reinterpret_cast<unsigned long long*>(row), static_cast<unsigned long long>(i));
  }
}

__global__ __launch_bounds__(kAggThreads) void agg_finalise(AggArgs a) {
  const int j = blockIdx.y;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kAggThreads + threadIdx.x;
  if (g >= a.num_groups) return;
  CAggRec& c = recs_of(a)[j];
  const int64_t N = a.num_groups * a.naggs, cell = j * a.num_groups + g;
  const uint64_t acc = gl(a.ws)[cell], cnt = gl(a.ws)[N + cell], row = gl(a.ws)[2 * N + cell];
  uint64_t out = 0;
  switch (c.op) {
    case FURY_AGG_COUNT: out = cnt; break;
    case FURY_AGG_SUM: out = acc; break;          // 0 / +0.0 for a group without values
    case FURY_AGG_MIN:
    case FURY_AGG_MAX: out = cnt ? agg_unorder(c, acc) : 0; break;
    default: out = c.combine == kAggArgVar ? acc : cnt ? row : kNoRow; break;
  }
  gl(c.out)[g] = out;
  if (c.out_count) gl(c.out_count)[g] = static_cast<int64_t>(cnt);
}

}  // namespace

int launch_aggregate(const AggArgs& args, hipStream_t stream) {
  AggArgs a = args;
  const int64_t G = a.num_groups, n = a.side.nrows;
  if (G == 0) return FURY_OK;
  if (n > 0x7fffffff || G > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  const int64_t N = G * a.naggs;
  DevBlock ws;                                    // [accumulators x N][counts x N][rows x N]
  int st = ws.alloc(N * 3 * 8, stream);
  if (st) return st;
  a.ws = ws.as<uint64_t>();
  const dim3 block(kAggThreads);
  const dim3 cells(static_cast<unsigned>((G + kAggThreads - 1) / kAggThreads), static_cast<unsigned>(a.naggs));
  hipLaunchKernelGGL(agg_init, cells, block, 0, stream, a);
  if (n > 0) {
    const int64_t ntiles = (n + kAggThreads - 1) / kAggThreads;
    bool resolve = false, var = false;
    for (int j = 0; j < a.naggs; j++) {
      resolve = resolve || a.rec[j].resolve;
      var = var || a.rec[j].combine == kAggArgVar;
    }
    if (aggregate_uses_lds(G, a.naggs)) {
      const dim3 grid(static_cast<unsigned>(ntiles < kAggMaxBlocks ? ntiles : kAggMaxBlocks));
      const size_t lds = static_cast<size_t>(N) * 16;
      if (var) {
        hipLaunchKernelGGL((agg_combine<true, true>), grid, block, lds, stream, a, ntiles);
      } else {
        hipLaunchKernelGGL((agg_combine<true, false>), grid, block, lds, stream, a, ntiles);
      }
    } else {
      const dim3 grid(static_cast<unsigned>(ntiles));
      if (var) {
        hipLaunchKernelGGL((agg_combine<false, true>), grid, block, 0, stream, a, ntiles);
      } else {
        hipLaunchKernelGGL((agg_combine<false, false>), grid, block, 0, stream, a, ntiles);
      }
    }
    if (resolve) hipLaunchKernelGGL(agg_resolve, dim3(static_cast<unsigned>(ntiles)), block, 0, stream, a);
  }
  hipLaunchKernelGGL(agg_finalise, cells, block, 0, stream, a);
  return check_hip(hipGetLastError(), "aggregate launch");
}

}  // namespace fury
