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

#include "project_dev.h"

namespace fury {

namespace {

constexpr int kEqThreads = 256;
constexpr int kKeyGroup = 4;                   // keys whose header words are in flight together
constexpr int kPayWords = 4;                   // payload words per side in flight together

using CKeyRec = __attribute__((address_space(4))) const KeyRec;
__device__ __forceinline__ CKeyRec& kr(const KeysEqualArgs& a, int k) {
  return ((CKeyRec*)(a.key))[k];
}

__device__ __forceinline__ uint64_t load8(const uint8_t* p) {
  return *gl(reinterpret_cast<const uint64_t*>(p));
}

// The 8 batch bytes at s, [s, s + 8) inside [0, total): one aligned load when `al`.
__device__ __forceinline__ uint64_t pay_word(const uint8_t* rows, int64_t s, int64_t total, bool al) {
  return al ? load8(rows + s) : batch_word(rows, s, total);
}

// The `rem` (1..7) bytes at s, [s, s + rem) inside [0, total), in the low bytes of the result: one
// word when it lies inside the batch, else (the batch's last bytes) by byte -- hash_span's rule.
__device__ __forceinline__ uint64_t pay_tail(const uint8_t* rows, int64_t s, int rem, int64_t total,
                                             bool al) {
  uint64_t v = 0;
  if (s + 8 <= total) {
    v = pay_word(rows, s, total, al);
  } else {
    for (int i = 0; i < rem; i++) v |= static_cast<uint64_t>(gl(rows)[s + i]) << (8 * i);
  }
  return v & (~uint64_t(0) >> (64 - 8 * rem));
}

// Batch bytes [pl, pl + n) of the left batch == [pr, pr + n) of the right one; both spans lie inside
// their batches (slot_count).
__device__ __forceinline__ bool same_bytes(const uint8_t* rl, int64_t pl, int64_t tl, const uint8_t* rr,
                                           int64_t pr, int64_t tr, int64_t n) {
  const bool al = ((pl | pr) & 7) == 0;           // every well-formed row: aligned 8-byte loads
  const int64_t nw = n >> 3;
  for (int64_t w0 = 0; w0 < nw; w0 += kPayWords) {
    uint64_t x[kPayWords], y[kPayWords];
#pragma unroll
    for (int u = 0; u < kPayWords; u++) {
      x[u] = y[u] = 0;
      if (w0 + u < nw) {
        x[u] = pay_word(rl, pl + 8 * (w0 + u), tl, al);
        y[u] = pay_word(rr, pr + 8 * (w0 + u), tr, al);
      }
    }
    uint64_t diff = 0;
#pragma unroll
    for (int u = 0; u < kPayWords; u++) diff |= x[u] ^ y[u];
    if (diff) return false;
  }
  const int rem = static_cast<int>(n & 7);
  if (rem == 0) return true;
  return pay_tail(rl, pl + 8 * nw, rem, tl, al) == pay_tail(rr, pr + 8 * nw, rem, tr, al);
}

// One side of a pair: the row, whether it can be read, its batch.
struct PairRow {
  const uint8_t* rows;
  int64_t base;                       // absolute row start
  int64_t total;                      // the batch's row bytes
  int32_t bitmap_bytes;
  bool ok;                            // index in [0, nrows) and header inside the batch
};

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
  bool eq = true;
  const bool null_equal = (a.flags & FURY_KEYS_NULL_EQUAL) != 0;
  for (int k0 = 0; k0 < a.nkeys; k0 += kKeyGroup) {
    uint64_t bits[kKeyGroup][2], slot[kKeyGroup][2];
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {         // every header word of the group, both sides
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bits[u][s] = ~uint64_t(0);                // a row that cannot be read: every key null
        slot[u][s] = 0;
        if (k0 + u < a.nkeys && pr[s].ok) {
          CKeyRec& c = kr(a, k0 + u);
          const int32_t f = s == 0 ? c.left_slot : c.right_slot;
          const uint8_t* hdr = pr[s].rows + pr[s].base;
          bits[u][s] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
          slot[u][s] = load8(hdr + pr[s].bitmap_bytes + 8 * static_cast<int64_t>(f));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {
      if (k0 + u >= a.nkeys) break;
      CKeyRec& c = kr(a, k0 + u);
      const int kind = c.kind, width = c.width;
      bool isnull[2];
      int64_t n[2];
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int32_t f = s == 0 ? c.left_slot : c.right_slot;
        isnull[s] = (bits[u][s] >> (f & 63)) & 1;
        n[s] = width;
        if (VAR && kind >= kBytes && !isnull[s]) {
          bool bad = false;
          n[s] = slot_count(kind, width, slot[u][s], pr[s].base, pr[s].rows, pr[s].total, &bad);
          if (kind == kDecimal) n[s] = 16;
          if (bad) {
            fail = true;
            isnull[s] = true;
          }
        }
      }
      if (isnull[0] || isnull[1]) {
        eq = eq && isnull[0] && isnull[1] && null_equal;
      } else if (VAR && kind >= kBytes) {
        eq = eq && n[0] == n[1];
        if (eq && !fail)
          eq = same_bytes(pr[0].rows, pr[0].base + static_cast<int32_t>(slot[u][0] >> 32), pr[0].total,
                          pr[1].rows, pr[1].base + static_cast<int32_t>(slot[u][1] >> 32), pr[1].total,
                          n[0]);
      } else if (kind == kBool) {
        eq = eq && ((slot[u][0] & 0xff) != 0) == ((slot[u][1] & 0xff) != 0);
      } else {                                    // kFixed: the `width` value bytes of the slot
        eq = eq && ((slot[u][0] ^ slot[u][1]) & (~uint64_t(0) >> (64 - 8 * width))) == 0;
      }
    }
  }
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
