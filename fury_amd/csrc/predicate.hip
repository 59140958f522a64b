// predicate.hip -- WHERE: which rows of a batch pass a conjunction of clauses over their fields, as a
// bit mask (fury_row_predicate)?  The producer of the mask that fury_row_filter, fury_row_update and a
// group-id rewrite in front of fury_row_aggregate consume.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): reading the named
// fields of every row with BinaryRow's getters (FMT/row/binary/BinaryRow.java, UnsafeTrait.java:68-197)
// and testing each value against a literal; the reference ships no predicate over rows, so the rules
// are this library's and are numbered in include/fury_row.h.  The comparison ops are fury_row_compare's
// order of the value against the literal; the pattern ops are byte-wise on the payload.
//
// MI355X design: lane = row, 256-thread workgroups, no gather, 16 bytes of LDS (the count only).  The terms and their literals
// travel in the kernel-argument block (PredArgs: 32 records of 32 bytes and a 2 KiB pool of literal
// words) and are indexed wave-uniformly through address_space(4), so a term's record and the literal
// words it compares against sit in SGPRs: a fixed-width term costs the lane its bitmap word, its slot
// word and a handful of VALU instructions.  A lane loads its row_mask word and its row offset, then the
// bitmap word and the slot word of kKeyGroup terms (2 kKeyGroup independent 8-byte loads in flight)
// before the first test, as pair_keys_compare does, and reads payloads kPayWords words at a time
// through pay_word / pay_tail.  The comparison ops reuse keys_dev.h's order (order_fixed,
// order_decimal, and order_spans with the literal as one side).  The pattern ops stand on one helper,
// ValueBytes::window: the 8 bytes at any byte offset of a value, two of the value's words
// funnel-shifted, bytes past the value's end zero; STARTS_WITH is the match at offset 0, ENDS_WITH at
// n - m, CONTAINS slides the window over the value, compares it with the literal's first word masked
// to min(m, 8) bytes and verifies the other literal words on a hit, loading the value's words again: the
// plain search, n * m / 8 word comparisons in the worst case (a repetitive literal in a repetitive
// value).  One lane scans one value however long it is, compare.hip's limit.  A row that is already
// decided (an earlier clause false, or its clause already true) reads no payload, but every term's null
// bit and bounds are still examined.
// The result: one 64-lane ballot is two finished mask words, stored by lanes 0 and 32 (vector
// stores), each only below the word count.  The count is one population count per ballot, summed in a
// register while the workgroup walks its tiles (at most kPredGrid workgroups are launched, tile t goes to
// workgroup t mod the grid), then summed over the workgroup's four waves through LDS and added with one
// 64-bit atomic per workgroup: every atomic lands on one word, which takes about 88 adds per
// microsecond, so one add per wave (15,625 for a million rows) cost 0.18 ms where half the rows pass.
// row_mask == out_mask works in place: a wave reads only the two words it writes, and its loads
// complete before its ballot.
// Two instantiations, as compare.hip: VAR = false (no term on a STRING / BINARY / DECIMAL field)
// compiles no payload loop.  Bounds follow "Decode bounds" in kernels.h; all address arithmetic is int64.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kPredThreads = 256;
constexpr int64_t kPredGrid = 2048;               // 8 workgroups per CU of 256

using CPredTerm = __attribute__((address_space(4))) const PredTerm;
using CPoolWord = __attribute__((address_space(4))) const uint64_t;

__device__ __forceinline__ CPredTerm* terms_of(const PredArgs& a) { return (CPredTerm*)(a.term); }
__device__ __forceinline__ CPoolWord* pool_of(const PredArgs& a) { return (CPoolWord*)(a.pool); }

__device__ __forceinline__ uint64_t low_bytes(int n) {      // n in 1..8
  return ~uint64_t(0) >> (64 - 8 * n);
}

// The n bytes of a non-null STRING / BINARY value whose span lies inside the batch (slot_count).
struct ValueBytes {
  BatchBytes b;
  int64_t n;
  // Bytes [8 w, 8 w + 8) of the value, those at or past n zero.  The last 1..7 bytes go through
  // pay_tail: nothing past the batch is read.
  __device__ __forceinline__ uint64_t word(int64_t w) const {
    const int64_t left = n - 8 * w;
    if (left <= 0) return 0;
    return left >= 8 ? b.word(w) : b.tail(w, static_cast<int>(left));
  }
  // Two neighbouring words funnel-shifted: the bytes at 8 w + sh / 8 when lo = word(w), hi = word(w + 1).
  static __device__ __forceinline__ uint64_t funnel(uint64_t lo, uint64_t hi, int sh) {
    return sh == 0 ? lo : (lo >> sh) | (hi << (64 - sh));
  }
  // The 8 bytes at byte offset o >= 0 of the value, those at or past n zero.
  __device__ __forceinline__ uint64_t window(int64_t o) const {
    const int64_t w = o >> 3;
    const int sh = static_cast<int>(o & 7) * 8;
    return funnel(word(w), sh ? word(w + 1) : 0, sh);
  }
};

// Literal words [from, ceil(m / 8)) equal the value's bytes at offset o + 8 from, ...: the last word
// masked to the literal's length.  o + m <= v.n.
__device__ __forceinline__ bool literal_at(const ValueBytes& v, int64_t o, CPoolWord* lit, int m, int from) {
  for (int w = from; 8 * w < m; w++) {
    const int left = m - 8 * w;
    const uint64_t mask = left >= 8 ? ~uint64_t(0) : low_bytes(left);
    if ((v.window(o + 8 * w) & mask) != lit[w]) return false;
  }
  return true;
}

// The literal (m >= 1 bytes) occurs at some byte offset of the value.
__device__ __forceinline__ bool contains(const ValueBytes& v, CPoolWord* lit, int m) {
  const int64_t last = v.n - m;                   // the last offset a match can start at
  if (last < 0) return false;
  const uint64_t mask0 = m >= 8 ? ~uint64_t(0) : low_bytes(m);
  const uint64_t lit0 = lit[0];
  uint64_t carry = v.word(0);
  for (int64_t w0 = 0; 8 * w0 <= last; w0 += kPayWords) {
    uint64_t x[kPayWords + 1];
    x[0] = carry;
#pragma unroll
    for (int u = 1; u <= kPayWords; u++) x[u] = v.word(w0 + u);      // zero past the value's end
#pragma unroll
    for (int u = 0; u < kPayWords; u++) {
      for (int b = 0; b < 8; b++) {
        const int64_t o = 8 * (w0 + u) + b;
        if (o > last) return false;
        if ((ValueBytes::funnel(x[u], x[u + 1], 8 * b) & mask0) == lit0 && literal_at(v, o, lit, m, 1))
          return true;
      }
    }
    carry = x[kPayWords];
  }
  return false;
}

// One term on a non-null value whose span lies inside the batch: the test of rules 3 and 4, before
// FURY_PRED_NOT.  `slot`: the row's slot word; n: the payload bytes of a kBytes value.
template <bool VAR>
__device__ __forceinline__ bool term_test(CPredTerm& c, CPoolWord* lit, const PairRow& me, uint64_t slot,
                                          int64_t n) {
  const int op = c.op, kind = c.kind, m = c.lit_len;
  if (VAR && kind == kBytes) {
    const int64_t p = me.base + static_cast<int32_t>(slot >> 32);
    const ValueBytes v{BatchBytes{me.rows, p, me.total, (p & 7) == 0}, n};
    if (op == FURY_PRED_STARTS_WITH) return n >= m && literal_at(v, 0, lit, m, 0);
    if (op == FURY_PRED_ENDS_WITH) return n >= m && literal_at(v, n - m, lit, m, 0);
    if (op == FURY_PRED_CONTAINS) return m == 0 || contains(v, lit, m);
    if (op == FURY_PRED_EQ && n != m) return false;
    const int c3 = order_spans(v.b, n, LiteralBytes{lit}, static_cast<int64_t>(m));
    return op == FURY_PRED_EQ ? c3 == 0 : op == FURY_PRED_LT ? c3 < 0 : op == FURY_PRED_LE ? c3 <= 0
           : op == FURY_PRED_GT ? c3 > 0 : c3 >= 0;
  }
  int c3;
  if (VAR && kind == kDecimal) {
    const int64_t p = me.base + static_cast<int32_t>(slot >> 32);
    const bool al = (p & 7) == 0;
    c3 = order_decimal(pay_word(me.rows, p, me.total, al), pay_word(me.rows, p + 8, me.total, al), lit[0], lit[1]);
  } else if (kind == kBool) {
    c3 = static_cast<int>((slot & 0xff) != 0) - static_cast<int>((lit[0] & 0xff) != 0);
  } else {                                        // kFixed
    const uint64_t x = order_fixed(slot, c.width, c.cls), y = order_fixed(lit[0], c.width, c.cls);
    c3 = x < y ? -1 : x > y ? 1 : 0;
  }
  return op == FURY_PRED_EQ ? c3 == 0 : op == FURY_PRED_LT ? c3 < 0 : op == FURY_PRED_LE ? c3 <= 0
         : op == FURY_PRED_GT ? c3 > 0 : c3 >= 0;
}

template <bool VAR>
__global__ __launch_bounds__(kPredThreads) void row_predicate(PredArgs a) {
  const KeySide& sd = a.side;
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (sd.nrows + kPredThreads - 1) / kPredThreads;
  uint32_t mine = 0;                              // lane 0: the rows of this wave that passed
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // uniform per workgroup
    const int64_t r = tile * kPredThreads + threadIdx.x;
    bool active = r < sd.nrows;
    if (active && a.row_mask) active = (gl(a.row_mask)[r >> 5] >> (r & 31)) & 1;
    PairRow me;
    me.rows = sd.rows;
    me.bitmap_bytes = sd.bitmap_bytes;
    me.total = sd.row_offsets ? gl(sd.row_offsets)[sd.nrows] : sd.nrows * sd.fixed_size;
    me.base = 0;
    if (active) me.base = sd.row_offsets ? gl(sd.row_offsets)[r] : r * sd.fixed_size;
    me.ok = active && row_ok(me.base, sd.fixed_size, me.total);
    bool fail = active && !me.ok;
    CPredTerm* term = terms_of(a);
    CPoolWord* pool = pool_of(a);
    bool pass = true, clause = true;                // the clauses before this one; this clause so far
    for (int k0 = 0; k0 < a.nterms; k0 += kKeyGroup) {
      uint64_t bits[kKeyGroup], slot[kKeyGroup];
#pragma unroll
      for (int u = 0; u < kKeyGroup; u++) {         // every header word of the group
        bits[u] = ~uint64_t(0);                     // a row that cannot be read: every field null
        slot[u] = 0;
        if (k0 + u < a.nterms && me.ok) {
          const int32_t f = term[k0 + u].slot;
          const uint8_t* hdr = me.rows + me.base;
          bits[u] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
          slot[u] = load8(hdr + me.bitmap_bytes + 8 * static_cast<int64_t>(f));
        }
      }
#pragma unroll
      for (int u = 0; u < kKeyGroup; u++) {
        if (k0 + u >= a.nterms) break;
        CPredTerm& c = term[k0 + u];
        const int kind = c.kind, flags = c.flags;
        bool isnull = (bits[u] >> (c.slot & 63)) & 1;
        int64_t n = c.width;
        if (VAR && kind >= kBytes && !isnull) {
          bool bad = false;
          n = slot_count(kind, c.width, slot[u], me.base, me.rows, me.total, &bad);
          if (bad) {
            fail = true;
            isnull = true;
          }
        }
        if (!(flags & FURY_PRED_OR)) {              // a new clause: the one before it is complete
          pass = pass && clause;
          clause = false;
        }
        const bool negate = (flags & FURY_PRED_NOT) != 0;
        bool tv;
        if (c.op == FURY_PRED_IS_NULL) {
          tv = isnull != negate;
        } else if (isnull || !pass || clause) {     // rule 5; or decided: no payload is read
          tv = false;
        } else {
          tv = term_test<VAR>(c, pool + c.lit_word, me, slot[u], n) != negate;
        }
        clause = clause || tv;
      }
    }
    pass = active && pass && clause;
    if (fail) raise_oob(a.err, r);
    // one ballot = this wave's 64 rows = two whole mask words, which no other wave or workgroup writes
    // (a workgroup covers a multiple of 64 rows); 4-byte stores: out_mask is 4-byte aligned
    const uint64_t m = __ballot(pass);
    const int64_t w = (r - lane) >> 5;              // the wave's first word
    const int64_t nw = (sd.nrows + 31) >> 5;
    if (lane == 0 && w < nw) gl(a.out_mask)[w] = static_cast<uint32_t>(m);
    if (lane == 32 && w + 1 < nw) gl(a.out_mask)[w + 1] = static_cast<uint32_t>(m >> 32);
    if (lane == 0) mine += static_cast<uint32_t>(__popcll(m));
  }
  if (a.out_count) {                              // one sum per workgroup: one atomic, not one per wave
    __shared__ uint32_t part[kPredThreads / 64];
    if (lane == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t sum = 0;
#pragma unroll
      for (int i = 0; i < kPredThreads / 64; i++) sum += part[i];
      if (sum) atomicAdd(a.out_count, static_cast<unsigned long long>(sum));
    }
  }
}

}  // namespace

int launch_predicate(const PredArgs& a, hipStream_t stream) {
  if (a.out_count) {
    const int st = check_hip(hipMemsetAsync(a.out_count, 0, 8, stream), "memset");
    if (st) return st;
  }
  if (a.side.nrows == 0) return FURY_OK;
  const int64_t nb = (a.side.nrows + kPredThreads - 1) / kPredThreads;
  if (nb > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  bool var = false;
  for (int k = 0; k < a.nterms; k++) var = var || a.term[k].kind >= kBytes;
  // at most kPredGrid workgroups walk the tiles: the count costs one atomic per workgroup on one word
  const dim3 grid(static_cast<unsigned>(nb < kPredGrid ? nb : kPredGrid)), block(kPredThreads);
  if (var) {
    hipLaunchKernelGGL(row_predicate<true>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(row_predicate<false>, grid, block, 0, stream, a);
  }
  return check_hip(hipGetLastError(), "row_predicate launch");
}

}  // namespace fury
