// lookup.hip -- the probe side of a hash join (fury_row_lookup): for every row of a probe batch, the
// smallest row of a build batch with equal key fields, or -1, answered from a table that
// fury_row_index_build (group.hip) made of the build batch once.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading the key
// fields of every build row with BinaryRow's getters (FMT/row/binary/BinaryRow.java,
// UnsafeTrait.java:68-197) into a HashMap with putIfAbsent, then get() with every probe row's key
// fields; the rules are numbered in include/fury_row.h.  A probe row is compared with a build row by
// pair_keys_equal (keys_dev.h), the comparison of fury_row_keys_equal under the call's flags.
//
// MI355X design: group.hip's table -- open addressing, linear probing, a power of two of 8-byte words
// (hash << 32) | row, all ones = EMPTY, one slot per distinct key that holds the key's smallest row
// once the build kernel has ended -- read-only here.
//   lookup_probe  lane = probe row, 256-thread workgroups, no LDS, no atomics.  A lane loads its hash
//            and row offset, checks its header (row_ok), then examines its own key fields kKeyGroup at
//            a time, the bitmap word (and, VAR, the slot word) of every key of the group issued before
//            the first is looked at (own_keys_ok): spans inside the batch, and whether any key is
//            null.  Without FURY_KEYS_NULL_EQUAL a row with a null key matches nothing and does not
//            walk.  The walk starts at hash & (cap - 1): EMPTY -> -1; another hash -> next slot; the
//            same hash -> the slot's row is range-checked, its offset loaded, its header checked,
//            then pair_keys_equal with the probe as pr[0] / left_slot and the build row as pr[1] /
//            right_slot: equal ends the walk, unequal moves on.  At capacity 2^32 the slot kNoSlot is
//            skipped, as the build skips it.
//            In flight before the first use: the lane's hash and row offset; per group of keys
//            kKeyGroup (VAR: 2 kKeyGroup) header words of its own row; per probed slot of the same
//            hash 4 kKeyGroup header words of both rows, then kPayWords payload words per side.
//            Loads are plain cached ones (gl()): a build row is re-read by every probe row of its
//            key, the probe lane's own header is read twice, and the table was written by an earlier
//            kernel, so nothing needs more than the kernel boundary.
//   mask     one ballot per wave = two whole mask words, as keys_equal.hip writes out_mask.
// Nothing in the table is trusted (it is the caller's memory): a slot's row is compared with the
// build row count before its offset is loaded, the row's header and key spans are checked before a
// payload byte is read (pair_keys_equal does not read payloads once `fail` is set), and the walk ends
// after cap steps.  A result >= 0 is therefore always a build row whose keys were compared equal.
// No thread waits for another; there is no store but the two outputs and the error word.
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok) per side, against that
// side's own total; all address arithmetic is int64.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kLookupThreads = 256;

__device__ __forceinline__ CKeyRec* keys_of(const LookupArgs& a) { return (CKeyRec*)(a.key); }

__device__ __forceinline__ int64_t row_base(const KeySide& sd, int64_t r) {
  return sd.row_offsets ? gl(sd.row_offsets)[r] : r * sd.fixed_size;
}

// VAR: some key is STRING / BINARY / DECIMAL.
template <bool VAR>
__global__ __launch_bounds__(kLookupThreads) void lookup_probe(LookupArgs a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kLookupThreads + threadIdx.x;
  const bool active = j < a.side[0].nrows;
  const bool null_equal = (a.flags & FURY_KEYS_NULL_EQUAL) != 0;
  PairRow pr[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const KeySide& sd = a.side[s];
    pr[s].rows = sd.rows;
    pr[s].bitmap_bytes = sd.bitmap_bytes;
    pr[s].total = 0;                              // an empty batch has no offsets to read
    if (sd.nrows > 0) pr[s].total = sd.row_offsets ? gl(sd.row_offsets)[sd.nrows] : sd.nrows * sd.fixed_size;
    pr[s].ok = false;
    pr[s].base = 0;
    // Two batches' constants and the exec masks of the comparison's nested branches do not fit the
    // scalar registers (4 to 6 spilled); the totals are kept in vector registers, which are not short.
    if (VAR) asm volatile("" : "+v"(pr[s].total));
  }
  uint32_t h = 0;
  if (active) {
    h = gl(a.hashes)[j];
    pr[0].base = row_base(a.side[0], j);
    pr[0].ok = row_ok(pr[0].base, a.side[0].fixed_size, pr[0].total);
  }
  bool fail = active && !pr[0].ok;
  bool any_null = false;
  if (pr[0].ok && (VAR || !null_equal)) {
    if (!own_keys_ok<VAR>(pr[0], keys_of(a), a.nkeys, any_null)) fail = true;
  }
  int64_t found = -1;
  // a lane that does not walk takes no step: one loop, no branch around it
  const uint64_t steps = active && !fail && (null_equal || !any_null) ? a.cap : 0;
  const uint32_t mask = static_cast<uint32_t>(a.cap - 1);
  uint32_t s = h & mask;
  for (uint64_t step = 0; step < steps; step++, s = (s + 1) & mask) {
    if (s == kNoSlot) continue;
    const uint64_t w = gl(a.table)[s];
    if (w == kEmpty) break;
    if (static_cast<uint32_t>(w >> 32) != h) continue;
    const int64_t r = static_cast<int64_t>(w & 0xffffffffu);
    pr[1].ok = r < a.side[1].nrows;               // else: not a table of this batch
    if (pr[1].ok) {
      // VAR: the test `row_offsets != NULL`, hoisted out of the loop as a lane mask, was a scalar pair
      // that spilled; behind the asm it is made here, from a vector register
      const int64_t* build_offs = a.side[1].row_offsets;
      if (VAR) asm volatile("" : "+v"(build_offs));
      pr[1].base = build_offs ? gl(build_offs)[r] : r * a.side[1].fixed_size;
      pr[1].ok = row_ok(pr[1].base, a.side[1].fixed_size, pr[1].total);
    }
    // the probe row's spans were checked above: only the build row can fail in the comparison
    fail = !pr[1].ok;
    const bool eq = pr[1].ok && pair_keys_equal<VAR>(pr, keys_of(a), a.nkeys, null_equal, fail);
    if (fail) break;
    if (eq) {
      found = r;
      break;
    }
  }
  if (fail) {
    raise_oob(a.err, j);
    found = -1;
  }
  if (active && a.out_rows) gl(a.out_rows)[j] = found;
  if (a.out_mask) {
    // one ballot = this wave's 64 rows = two whole mask words, which no other wave or workgroup
    // writes (a workgroup covers a multiple of 64 rows); 4-byte stores: out_mask is 4-byte aligned
    const uint64_t m = __ballot(found >= 0);
    const int lane = threadIdx.x & 63;
    const int64_t w = (j - lane) >> 5;            // the wave's first word
    const int64_t nw = (a.side[0].nrows + 31) >> 5;
    if (lane == 0 && w < nw) gl(a.out_mask)[w] = static_cast<uint32_t>(m);
    if (lane == 32 && w + 1 < nw) gl(a.out_mask)[w + 1] = static_cast<uint32_t>(m >> 32);
  }
}

}  // namespace

int launch_lookup(const LookupArgs& a, const ProjArgs* hash_args, hipStream_t stream) {
  const int64_t n = a.side[0].nrows;
  if (n == 0) return FURY_OK;
  const int64_t nb = (n + kLookupThreads - 1) / kLookupThreads;
  if (nb > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  LookupArgs la = a;
  DevBlock ws;                                    // the probe rows' hashes when the caller gave none
  if (!la.hashes) {
    int st = ws.alloc(((n + 1) / 2) * 8, stream);
    if (st) return st;
    ProjArgs h = *hash_args;
    h.err = a.err;
    st = launch_hash(h, a.side[0].rows, a.side[0].row_offsets, 0, 1, ws.as<uint32_t>(), nullptr, stream);
    if (st) return st;
    la.hashes = ws.as<uint32_t>();
  }
  bool var = false;
  for (int k = 0; k < a.nkeys; k++) var = var || a.key[k].kind >= kBytes;
  const dim3 grid(static_cast<unsigned>(nb)), block(kLookupThreads);
  if (var) {
    hipLaunchKernelGGL(lookup_probe<true>, grid, block, 0, stream, la);
  } else {
    hipLaunchKernelGGL(lookup_probe<false>, grid, block, 0, stream, la);
  }
  return check_hip(hipGetLastError(), "lookup launch");
}

}  // namespace fury
