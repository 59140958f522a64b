// group.hip -- group ids and distinct rows of one batch by key fields (fury_row_group): the smallest
// row number of every row's group, the groups numbered in order of their first row.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading every
// row's key fields with BinaryRow's getters (FMT/row/binary/BinaryRow.java, UnsafeTrait.java:68-197)
// and putting the rows into a LinkedHashMap keyed by the values, null equal to null; the rules are
// numbered in include/fury_row.h.  Two rows are compared by pair_keys_equal (keys_dev.h), the
// comparison of fury_row_keys_equal under FURY_KEYS_NULL_EQUAL.
//
// MI355X design: one insert-only hash table per call, open addressing with linear probing, capacity
// the smallest power of two >= 2 nrows (load <= 0.5), one 64-bit word per slot: (hash << 32) | row.
// hipMemsetAsync to 0xFF marks every slot EMPTY; a real entry has row < 2^31, so it never equals
// EMPTY even with hash 0xFFFFFFFF.  A slot's key is the key of the row it holds; it never changes
// once the slot is taken, only the row is lowered to the smallest of the group.
//   probe    lane = row, 256-thread workgroups, no LDS.  A lane first examines its own key fields
//            (null bits, spans) kKeyGroup keys at a time, the bitmap word and the slot word of every
//            key of the group issued before the first is looked at; a row that fails the bounds is
//            never entered.  It then walks the slots from hash & (cap - 1): EMPTY -> atomicCAS of its
//            own word (a failed CAS returns the winner, examined at the same slot: a slot never
//            becomes empty again, so once per slot); another hash -> next slot; the same hash -> the
//            rows are compared, unequal -> next slot, equal -> the group's slot is found, and when
//            the slot's row is greater than the lane's a 64-bit unsigned atomicMin lowers it (same
//            hash in the high half, so min orders by row).  When the slot's row is already lower no
//            atomic is issued: a hot key costs one cached load per row, not one atomic per row on
//            one address.  A stale read only causes a redundant atomicMin.  The lane records its slot
//            index (4 bytes per row).
//            In flight before the first use: the lane's row offset; per group of keys 2 kKeyGroup
//            header words of its own row; per probed slot of the same hash 4 kKeyGroup header
//            words of both rows, then kPayWords payload words per side (pair_keys_equal).
//            Row loads are plain cached ones (gl()), not non-temporal: a group's representative is
//            re-read by every duplicate, and the lane's own header is read twice.
//   resolve  after the kernel boundary: out_first[i] = the row of the lane's slot (its own number
//            for a row that was not entered), flag[i] = (out_first[i] == i).
//   number   device_scan of the flags, then ids[i] = scan[out_first[i]], group_rows[scan[i]] = i for
//            a first row, -1 at and past the group count; plain vector stores.
// Orderings the atomics rely on: none beyond atomicity.  The batch is read-only and was written before
// the launch; the table is reached only through atomics (relaxed, agent scope) inside the probe
// kernel, and read with plain loads only after the kernel boundary.  No thread waits for another:
// every loop is bounded by the capacity, there is no spin-wait.  A probe that exhausts the table
// (impossible at load 0.5) is handled as a bounds failure: own group, kErrBounds.
// The result does not depend on scheduling: whichever row takes a slot first, the slot ends at the
// minimum of its group, and which slot a group lives in is never an output.
// The hash only chooses where probing starts and which slots are compared: equal keys with unequal
// hashes (a caller's mistake) may end in two groups, nothing else.
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok) as hash.hip applies
// them; all address arithmetic is int64.
// fury_row_index_build (launch_index_build) is the same table kept: the caller's memory instead of
// workspace, the same hash, memset and probe (build_table), the slot indices and resolve only when
// out_first is wanted.  lookup.hip reads that table after the kernel boundary, as resolve does.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kGroupThreads = 256;

__device__ __forceinline__ CKeyRec* keys_of(const GroupArgs& a) { return (CKeyRec*)(a.key); }

__device__ __forceinline__ int64_t row_base(const GroupArgs& a, int64_t r) {
  return a.side.row_offsets ? gl(a.side.row_offsets)[r] : r * a.side.fixed_size;
}

// VAR: some key is STRING / BINARY / DECIMAL.
template <bool VAR>
__global__ __launch_bounds__(kGroupThreads) void group_probe(GroupArgs a, const uint32_t* __restrict__ hashes,
                                                             uint64_t* __restrict__ table, uint64_t cap,
                                                             uint32_t* __restrict__ slot_of) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupThreads + threadIdx.x;
  if (i >= a.side.nrows) return;
  const int64_t total = a.side.row_offsets ? gl(a.side.row_offsets)[a.side.nrows]
                                           : a.side.nrows * a.side.fixed_size;
  const uint32_t h = gl(hashes)[i];
  PairRow pr[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    pr[s].rows = a.side.rows;
    pr[s].total = total;
    pr[s].bitmap_bytes = a.side.bitmap_bytes;
    pr[s].ok = true;
    pr[s].base = 0;
  }
  pr[0].base = row_base(a, i);
  bool ok = row_ok(pr[0].base, a.side.fixed_size, total);
  if (VAR && ok) {
    bool any_null = false;                        // of no interest here: null equals null
    ok = own_keys_ok<true>(pr[0], keys_of(a), a.nkeys, any_null);
  }
  uint32_t found = kNoSlot;
  if (ok) {
    const uint64_t mine = (static_cast<uint64_t>(h) << 32) | static_cast<uint64_t>(i);
    const uint32_t mask = static_cast<uint32_t>(cap - 1);
    uint32_t s = h & mask;
    for (uint64_t step = 0; step < cap; step++, s = (s + 1) & mask) {
      if (s == kNoSlot) continue;
      uint64_t w = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == kEmpty) {
        w = atomicCAS(reinterpret_cast<unsigned long long*>(table + s), kEmpty, mine);
        if (w == kEmpty) {
          found = s;
          break;
        }
      }
      if (static_cast<uint32_t>(w >> 32) != h) continue;
      const int64_t r = static_cast<int64_t>(w & 0xffffffffu);
      // an entered row passed the bounds where it was entered, so the comparison cannot fail
      pr[1].base = row_base(a, r);
      bool fail = false;
      if (!pair_keys_equal<VAR>(pr, keys_of(a), a.nkeys, true, fail)) continue;
      if (r > i) atomicMin(reinterpret_cast<unsigned long long*>(table + s), mine);
      found = s;
      break;
    }
  }
  if (found == kNoSlot) raise_oob(a.err, i);
  if (slot_of) gl(slot_of)[i] = found;           // fury_row_index_build without out_first: not wanted
}

__global__ __launch_bounds__(kGroupThreads) void group_resolve(int64_t n, const uint64_t* __restrict__ table,
                                                               const uint32_t* __restrict__ slot_of,
                                                               int64_t* __restrict__ out_first,
                                                               int64_t* __restrict__ flags) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = gl(slot_of)[i];
  const int64_t first = s == kNoSlot ? i : static_cast<int64_t>(gl(table)[s] & 0xffffffffu);
  gl(out_first)[i] = first;
  if (flags) gl(flags)[i] = first == i;
}

// scan[i] = the number of first rows before row i, *count = the number of groups.
__global__ __launch_bounds__(kGroupThreads) void group_number(int64_t n, const int64_t* __restrict__ first,
                                                              const int64_t* __restrict__ scan,
                                                              const int64_t* __restrict__ count,
                                                              int64_t* __restrict__ out_ids,
                                                              int64_t* __restrict__ out_rows,
                                                              int64_t* __restrict__ out_num) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t g = gl(count)[0];
  const int64_t f = gl(first)[i];
  if (out_ids) gl(out_ids)[i] = gl(scan)[f];
  if (out_rows) {
    if (f == i) gl(out_rows)[gl(scan)[i]] = i;    // scan[i] < g: entry scan[i] is this lane's alone
    if (i >= g) gl(out_rows)[i] = -1;
  }
  if (out_num && i == 0) gl(out_num)[0] = g;
}

}  // namespace

int64_t group_table_slots(int64_t nrows) {
  int64_t cap = 2;
  while (cap < 2 * nrows) cap <<= 1;
  return cap;
}

int64_t group_workspace_bytes(int64_t nrows, bool own_hashes, bool numbered) {
  const int64_t words = group_table_slots(nrows) + (numbered ? nrows + 1 + scan_workspace(nrows) : 0);
  return words * 8 + ((nrows + 1) / 2) * 8 * (own_hashes ? 2 : 1);
}

namespace {

// What launch_group and launch_index_build share: the keys hashed into `own` when the caller gave no
// hashes, every slot of `table` EMPTY, then the probe; slot_of NULL: the slot indices are not wanted.
int build_table(const GroupArgs& a, const ProjArgs* hash_args, uint32_t* own, uint64_t* table, int64_t cap,
                uint32_t* slot_of, hipStream_t stream) {
  const int64_t n = a.side.nrows;
  const uint32_t* hashes = a.hashes;
  int st;
  if (!hashes) {
    ProjArgs h = *hash_args;
    h.err = a.err;
    st = launch_hash(h, a.side.rows, a.side.row_offsets, 0, 1, own, nullptr, stream);
    if (st) return st;
    hashes = own;
  }
  if ((st = check_hip(hipMemsetAsync(table, 0xff, static_cast<size_t>(cap) * 8, stream), "group: memset")))
    return st;
  bool var = false;
  for (int k = 0; k < a.nkeys; k++) var = var || a.key[k].kind >= kBytes;
  const dim3 grid(static_cast<unsigned>((n + kGroupThreads - 1) / kGroupThreads)), block(kGroupThreads);
  if (var) {
    hipLaunchKernelGGL(group_probe<true>, grid, block, 0, stream, a, hashes, table,
                       static_cast<uint64_t>(cap), slot_of);
  } else {
    hipLaunchKernelGGL(group_probe<false>, grid, block, 0, stream, a, hashes, table,
                       static_cast<uint64_t>(cap), slot_of);
  }
  return FURY_OK;
}

}  // namespace

int launch_group(const GroupArgs& a, const ProjArgs* hash_args, hipStream_t stream) {
  const int64_t n = a.side.nrows;
  if (n == 0) return FURY_OK;
  if (n > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  const bool numbered = a.out_group_ids || a.out_group_rows || a.out_num_groups;
  const bool own_hashes = a.hashes == nullptr;
  const int64_t cap = group_table_slots(n);
  // [table x cap][scan x n][count][scan scratch][slot_of x n (uint32)][hashes x n (uint32)]
  DevBlock ws;
  int st = ws.alloc(group_workspace_bytes(n, own_hashes, numbered), stream);
  if (st) return st;
  uint64_t* table = ws.as<uint64_t>();
  int64_t* scan = reinterpret_cast<int64_t*>(table + cap);
  int64_t* count = scan + n;
  int64_t* sws = count + 1;
  uint32_t* slot_of = reinterpret_cast<uint32_t*>(numbered ? sws + scan_workspace(n) : scan);
  uint32_t* own = slot_of + ((n + 1) / 2) * 2;
  if ((st = build_table(a, hash_args, own, table, cap, slot_of, stream))) return st;
  const dim3 grid(static_cast<unsigned>((n + kGroupThreads - 1) / kGroupThreads)), block(kGroupThreads);
  hipLaunchKernelGGL(group_resolve, grid, block, 0, stream, n, table, slot_of, a.out_first,
                     numbered ? scan : nullptr);
  if (numbered) {
    device_scan(scan, n, count, sws, stream);
    hipLaunchKernelGGL(group_number, grid, block, 0, stream, n, a.out_first, scan, count,
                       a.out_group_ids, a.out_group_rows, a.out_num_groups);
  }
  return check_hip(hipGetLastError(), "group launch");
}

int launch_index_build(const GroupArgs& a, const ProjArgs* hash_args, uint64_t* table, int64_t cap,
                       hipStream_t stream) {
  const int64_t n = a.side.nrows;
  if (n > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  if (n == 0)                                     // the two slots of an empty index
    return check_hip(hipMemsetAsync(table, 0xff, static_cast<size_t>(cap) * 8, stream), "index build: memset");
  const bool own_hashes = a.hashes == nullptr, resolve = a.out_first != nullptr;
  // [slot_of x n (uint32), when out_first is wanted][hashes x n (uint32), when the call hashes]
  DevBlock ws;
  const int64_t per = ((n + 1) / 2) * 2;
  if (own_hashes || resolve) {
    const int st = ws.alloc(per * 4 * ((own_hashes ? 1 : 0) + (resolve ? 1 : 0)), stream);
    if (st) return st;
  }
  uint32_t* slot_of = resolve ? ws.as<uint32_t>() : nullptr;
  uint32_t* own = own_hashes ? ws.as<uint32_t>() + (resolve ? per : 0) : nullptr;
  const int st = build_table(a, hash_args, own, table, cap, slot_of, stream);
  if (st) return st;
  if (resolve) {
    const dim3 grid(static_cast<unsigned>((n + kGroupThreads - 1) / kGroupThreads)), block(kGroupThreads);
    hipLaunchKernelGGL(group_resolve, grid, block, 0, stream, n, table, slot_of, a.out_first,
                       static_cast<int64_t*>(nullptr));
  }
  return check_hip(hipGetLastError(), "index build launch");
}

}  // namespace fury
