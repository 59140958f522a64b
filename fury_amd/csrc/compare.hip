// compare.hip -- the order of row pairs: do the key fields of row L of one batch sort before, with or
// after the key fields of row R of another (fury_row_compare)?  The comparator of ORDER BY, of a
// sortedness check, of a binary search (range partitioning, merge joins) and of a merge.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading both
// rows' key fields with BinaryRow's getters (FMT/row/binary/BinaryRow.java, UnsafeTrait.java:68-197)
// and comparing the values key after key; the reference ships no comparator of rows, so the order is
// this library's and is numbered in include/fury_row.h.  It is 0 exactly where fury_row_keys_equal
// with FURY_KEYS_NULL_EQUAL says equal.
//
// MI355X design: keys_equal.hip's, for its reasons: lane = pair, 256-thread workgroups, no LDS; the
// pairs are a gather, so a lane loads both indices, then both row offsets, then the bitmap word and
// the slot word of kKeyGroup keys on both sides (4 kKeyGroup independent 8-byte loads) before the
// first compare, and reads payloads kPayWords 8-byte words per side at a time.  What differs from
// equality is the decision: the first differing word decides through a byte swap and an unsigned
// compare (a row's bytes are little-endian in a register, the order is by the first byte), the tail
// word is masked to the shorter length and the lengths break a tie; a pair that is decided reads no
// further payloads, but every key's null bit and bounds are still examined.  The per-pair comparison
// is pair_keys_compare in keys_dev.h.  Loads are plain cached ones: a binary search revisits the
// middle rows, and a row's bitmap and key slots share 64-byte lines.
// Two instantiations, as keys_equal: VAR = false (every key fixed-width or BOOL) compiles no payload
// loop.  Bounds follow "Decode bounds" in kernels.h per side against that side's own total; all
// address arithmetic is int64.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kCmpThreads = 256;

__device__ __forceinline__ COrderKey* keys_of(const CompareArgs& a) { return (COrderKey*)(a.key); }

template <bool VAR>
__global__ __launch_bounds__(kCmpThreads) void row_compare(CompareArgs a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kCmpThreads + threadIdx.x;
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
  const int res = pair_keys_compare<VAR>(pr, keys_of(a), a.nkeys, fail);
  if (fail) raise_oob(a.err, j);
  if (active) gl(a.out_cmp)[j] = static_cast<int8_t>(res);
}

}  // namespace

int launch_compare(const CompareArgs& a, hipStream_t stream) {
  if (a.num_pairs == 0) return FURY_OK;
  const int64_t nb = (a.num_pairs + kCmpThreads - 1) / kCmpThreads;
  if (nb > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  bool var = false;
  for (int k = 0; k < a.nkeys; k++) var = var || a.key[k].kind >= kBytes;
  const dim3 grid(static_cast<unsigned>(nb)), block(kCmpThreads);
  if (var) {
    hipLaunchKernelGGL(row_compare<true>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(row_compare<false>, grid, block, 0, stream, a);
  }
  return check_hip(hipGetLastError(), "row_compare launch");
}

}  // namespace fury
