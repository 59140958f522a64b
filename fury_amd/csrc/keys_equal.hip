// keys_equal.hip -- key equality of row pairs: do the key fields of row L of one batch equal the key
// fields of row R of another (fury_row_keys_equal)?  The verify step of an equi-join, a group-by or
// a de-duplication whose candidates come from fury_row_hash.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading both
// rows' key fields with BinaryRow's getters (FMT/row/binary/BinaryRow.java, UnsafeTrait.java:68-197)
// and comparing the values; the rules are numbered in include/fury_row.h.  The bytes compared are the
// bytes fury_row_project would produce for the fields, the bytes hash.hip hashes.
//
// MI355X design: lane = pair, 256-thread workgroups, no LDS.  Indexed pairs are a gather: a lane's
// two rows sit anywhere in their batches, so hash.hip's tile staging (consecutive rows, one byte
// range) does not apply; where a side has no indices the same loads simply coalesce better.  What
// makes a gather fast is independent loads in flight, so a lane
//   - loads both indices (coalesced 8-byte loads), then issues both sides' row-offset gathers
//     together;
//   - takes the keys kKeyGroup at a time and issues the bitmap word and the slot word of every key of
//     the group, on both sides, before the first compare: 4 kKeyGroup independent 8-byte loads;
//   - compares payloads (VAR) kPayWords 8-byte words per side at a time, all loaded before the first
//     is compared, and stops reading a pair's payloads once it is unequal.
// The per-pair comparison itself is pair_keys_equal in keys_dev.h, which group.hip shares.
// Loads are plain cached ones through gl(), not non-temporal: join candidates revisit rows
// (duplicate keys), and a row's bitmap and key slots share 64-byte lines.
// Two instantiations, chosen by the launcher from the key kinds: VAR = false (every key is
// fixed-width or BOOL) compiles no payload loop; VAR = true: some key is STRING / BINARY / DECIMAL.
// A value is compared by one lane however long it is.
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok) as hash.hip applies
// them, per side against that side's own total; all address arithmetic is int64.  Every key of a
// pair is examined for its null bit and bounds whatever the earlier keys gave, so whether a pair
// raises does not depend on the data of the other keys.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kEqThreads = 256;

__device__ __forceinline__ CKeyRec* keys_of(const KeysEqualArgs& a) { return (CKeyRec*)(a.key); }

template <bool VAR>
__global__ __launch_bounds__(kEqThreads) void keys_equal(KeysEqualArgs a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kEqThreads + threadIdx.x;
  const bool active = j < a.num_pairs;
  PairRow pr[2];
  int64_t row[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {                   // both indices, then both row offsets
    const KeySide& sd = a.side[s];
    row[s] = j;
    if (active && sd.indices) row[s] = gl(sd.indices)[j];
  }
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const KeySide& sd = a.side[s];
    pr[s].rows = sd.rows;
    pr[s].bitmap_bytes = sd.bitmap_bytes;
    pr[s].total = sd.row_offsets ? gl(sd.row_offsets)[sd.nrows] : sd.nrows * sd.fixed_size;
    pr[s].ok = active && row[s] >= 0 && row[s] < sd.nrows;
    pr[s].base = 0;
    if (pr[s].ok) pr[s].base = sd.row_offsets ? gl(sd.row_offsets)[row[s]] : row[s] * sd.fixed_size;
  }
#pragma unroll
  for (int s = 0; s < 2; s++)
    pr[s].ok = pr[s].ok && row_ok(pr[s].base, a.side[s].fixed_size, pr[s].total);
  bool fail = active && !(pr[0].ok && pr[1].ok);
  const bool eq = pair_keys_equal<VAR>(pr, keys_of(a), a.nkeys, (a.flags & FURY_KEYS_NULL_EQUAL) != 0,
                                       fail);
  if (fail) raise_oob(a.err, j);
  const bool res = active && eq && !fail;
  if (active && a.out_equal) gl(a.out_equal)[j] = res ? 1 : 0;
  if (a.out_mask) {
    // one ballot = this wave's 64 pairs = two whole mask words, which no other wave or workgroup
    // writes (a workgroup covers a multiple of 64 pairs); 4-byte stores: out_mask is 4-byte aligned
    const uint64_t m = __ballot(res);
    const int lane = threadIdx.x & 63;
    const int64_t w = (j - lane) >> 5;            // the wave's first word
    const int64_t nw = (a.num_pairs + 31) >> 5;
    if (lane == 0 && w < nw) gl(a.out_mask)[w] = static_cast<uint32_t>(m);
    if (lane == 32 && w + 1 < nw) gl(a.out_mask)[w + 1] = static_cast<uint32_t>(m >> 32);
  }
}

}  // namespace

int launch_keys_equal(const KeysEqualArgs& a, hipStream_t stream) {
  if (a.num_pairs == 0) return FURY_OK;
  const int64_t nb = (a.num_pairs + kEqThreads - 1) / kEqThreads;
  if (nb > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  bool var = false;
  for (int k = 0; k < a.nkeys; k++) var = var || a.key[k].kind >= kBytes;
  const dim3 grid(static_cast<unsigned>(nb)), block(kEqThreads);
  if (var) {
    hipLaunchKernelGGL(keys_equal<true>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(keys_equal<false>, grid, block, 0, stream, a);
  }
  return check_hip(hipGetLastError(), "keys_equal launch");
}

}  // namespace fury
