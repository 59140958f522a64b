// keys_dev.h -- the comparison of two rows' key fields, shared by the kernels that decide key
// equality from the row bytes (keys_equal.hip: pairs of two batches; group.hip: a row against the
// representative of a hash-table slot; lookup.hip: a probe row against the build row of a slot), and
// the check of a lane's own keys that the two table kernels make first.  One implementation of rule 2 of fury_row_keys_equal: header
// words in flight, slot_count, same_bytes and the tail rule.  Design notes: keys_equal.hip.
// Below it the order of two rows' key fields (compare.hip) and the pieces order.hip shares with it: one
// implementation of rules 1-4 of fury_row_compare, pair_keys_compare beside pair_keys_equal; its
// value-against-value step, value_compare, is also the order of aggregate.hip's ARGMIN / ARGMAX, and
// its pieces (order_fixed, order_decimal, order_spans) order a value against a literal in predicate.hip.
#pragma once

#include "project_dev.h"

namespace fury {

namespace {

constexpr int kKeyGroup = 4;                   // keys whose header words are in flight together
constexpr int kPayWords = 4;                   // payload words per side in flight together

using CKeyRec = __attribute__((address_space(4))) const KeyRec;

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

// A hash-table word of group.hip / lookup.hip: (hash << 32) | row.  A real entry has row < 2^31, so it
// never equals kEmpty even with hash 0xFFFFFFFF.
constexpr uint64_t kEmpty = ~uint64_t(0);
// The slot index recorded for a row that is in no slot.  Never probed either: at capacity 2^32 the
// last slot stays empty, so the value is unambiguous.
constexpr uint32_t kNoSlot = 0xffffffffu;

// Rule 5 for a lane's own row `me` (its header is inside the batch: row_ok), keys read at
// key[k].left_slot: every non-null STRING / BINARY / DECIMAL key value lies inside the batch.
// `any_null` is set (never cleared) when a key is null.  VAR = false reads no slot words: no key has a
// span to check, only the null bits are looked at.
template <bool VAR>
__device__ __forceinline__ bool own_keys_ok(const PairRow& me, CKeyRec* key, int nkeys, bool& any_null) {
  bool ok = true;
  for (int k0 = 0; k0 < nkeys; k0 += kKeyGroup) {
    uint64_t bits[kKeyGroup], slot[kKeyGroup];
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {
      bits[u] = ~uint64_t(0);
      slot[u] = 0;
      if (k0 + u < nkeys) {
        const int32_t f = key[k0 + u].left_slot;
        const uint8_t* hdr = me.rows + me.base;
        bits[u] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
        if (VAR) slot[u] = load8(hdr + me.bitmap_bytes + 8 * static_cast<int64_t>(f));
      }
    }
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {
      if (k0 + u >= nkeys) break;
      CKeyRec& c = key[k0 + u];
      const bool isnull = (bits[u] >> (c.left_slot & 63)) & 1;
      any_null = any_null || isnull;
      if (VAR && c.kind >= kBytes && !isnull) {
        bool bad = false;
        (void)slot_count(c.kind, c.width, slot[u], me.base, me.rows, me.total, &bad);
        ok = ok && !bad;
      }
    }
  }
  return ok;
}

// Every key position of the pair pr[0] / pr[1] equal under rule 2 (key[k].left_slot of pr[0] against
// key[k].right_slot of pr[1]).  Every key is examined for its null bit and bounds whatever the
// earlier keys gave; `fail` is set (never cleared) when a value's span leaves its batch, and payloads
// are not read from then on.  A side that is not ok has every key null.  `key` is indexed
// wave-uniformly (scalar loads).  `fail` is a reference, not a pointer or a returned pair: as a
// pointer the VAR instantiation of keys_equal took one more VGPR.
template <bool VAR>
__device__ __forceinline__ bool pair_keys_equal(const PairRow (&pr)[2], CKeyRec* key, int nkeys,
                                                bool null_equal, bool& fail) {
  bool eq = true;
  for (int k0 = 0; k0 < nkeys; k0 += kKeyGroup) {
    uint64_t bits[kKeyGroup][2], slot[kKeyGroup][2];
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {         // every header word of the group, both sides
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bits[u][s] = ~uint64_t(0);                // a row that cannot be read: every key null
        slot[u][s] = 0;
        if (k0 + u < nkeys && pr[s].ok) {
          CKeyRec& c = key[k0 + u];
          const int32_t f = s == 0 ? c.left_slot : c.right_slot;
          const uint8_t* hdr = pr[s].rows + pr[s].base;
          bits[u][s] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
          slot[u][s] = load8(hdr + pr[s].bitmap_bytes + 8 * static_cast<int64_t>(f));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {
      if (k0 + u >= nkeys) break;
      CKeyRec& c = key[k0 + u];
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
  return eq;
}

// ---- the order of two rows' key fields (compare.hip, order.hip): rules of fury_row_compare ----------------
using COrderKey = __attribute__((address_space(4))) const OrderKey;

// A kFixed slot's `width` value bytes as an unsigned integer that ranks as rule 3 does: two's
// complement with the sign bit flipped; a float with the usual total-order transform (negative: all
// bits flipped, else the sign bit set).
__device__ __forceinline__ uint64_t order_fixed(uint64_t slot, int width, int cls) {
  const uint64_t mask = ~uint64_t(0) >> (64 - 8 * width);
  const uint64_t sign = uint64_t(1) << (8 * width - 1);
  const uint64_t v = slot & mask;
  if (cls == kOrdFloat && (v & sign)) return ~v & mask;
  return v ^ sign;
}

// -1 / 0 / +1 of two words whose memory bytes rank lexicographically: the first byte in memory is the
// low byte of the word, so the bytes are swapped and the words compared unsigned.
__device__ __forceinline__ int order_word_cmp(uint64_t x, uint64_t y) {
  const uint64_t bx = __builtin_bswap64(x), by = __builtin_bswap64(y);
  return bx < by ? -1 : bx > by ? 1 : 0;
}

// A side of the bytes order: where its 8-byte words come from.  BatchBytes: a value's span inside a
// batch (slot_count), read through pay_word / pay_tail.  LiteralBytes (predicate.hip): words in the
// kernel-argument block, zero-padded to whole words, read through scalar loads where the index is
// wave-uniform.
struct BatchBytes {
  const uint8_t* rows;
  int64_t p;                          // absolute start of the span
  int64_t total;                      // the batch's row bytes
  bool al;                            // aligned 8-byte loads
  __device__ __forceinline__ uint64_t word(int64_t w) const { return pay_word(rows, p + 8 * w, total, al); }
  __device__ __forceinline__ uint64_t tail(int64_t w, int rem) const {
    return pay_tail(rows, p + 8 * w, rem, total, al);
  }
};
struct LiteralBytes {
  __attribute__((address_space(4))) const uint64_t* words;
  __device__ __forceinline__ uint64_t word(int64_t w) const { return words[w]; }
  __device__ __forceinline__ uint64_t tail(int64_t w, int rem) const {
    return words[w] & (~uint64_t(0) >> (64 - 8 * rem));
  }
};

// The nl bytes of `l` against the nr bytes of `r`, unsigned lexicographic, a proper prefix first.  The
// first differing 8-byte word decides; the tail is masked and the lengths break a tie.
template <class L, class R>
__device__ __forceinline__ int order_spans(const L& l, int64_t nl, const R& r, int64_t nr) {
  const int64_t n = nl < nr ? nl : nr;
  const int64_t nw = n >> 3;
  for (int64_t w0 = 0; w0 < nw; w0 += kPayWords) {
    uint64_t x[kPayWords], y[kPayWords];
#pragma unroll
    for (int u = 0; u < kPayWords; u++) {
      x[u] = y[u] = 0;
      if (w0 + u < nw) {
        x[u] = l.word(w0 + u);
        y[u] = r.word(w0 + u);
      }
    }
#pragma unroll
    for (int u = 0; u < kPayWords; u++)
      if (x[u] != y[u]) return order_word_cmp(x[u], y[u]);
  }
  const int rem = static_cast<int>(n & 7);
  if (rem) {
    const int c = order_word_cmp(l.tail(nw, rem), r.tail(nw, rem));
    if (c) return c;
  }
  return nl < nr ? -1 : nl > nr ? 1 : 0;
}

// Batch bytes [pl, pl + nl) of the left batch against [pr, pr + nr) of the right one; both spans lie
// inside their batches (slot_count).
__device__ __forceinline__ int order_bytes(const uint8_t* rl, int64_t pl, int64_t tl, int64_t nl,
                                           const uint8_t* rr, int64_t pr, int64_t tr, int64_t nr) {
  const bool al = ((pl | pr) & 7) == 0;           // every well-formed row: aligned 8-byte loads
  return order_spans(BatchBytes{rl, pl, tl, al}, nl, BatchBytes{rr, pr, tr, al}, nr);
}

// Two DECIMAL values, 16 bytes little-endian two's complement each, as (low word, high word).
__device__ __forceinline__ int order_decimal(uint64_t lo0, uint64_t hi0, uint64_t lo1, uint64_t hi1) {
  const uint64_t h0 = hi0 ^ (uint64_t(1) << 63), h1 = hi1 ^ (uint64_t(1) << 63);
  return h0 != h1 ? (h0 < h1 ? -1 : 1) : lo0 < lo1 ? -1 : lo0 > lo1 ? 1 : 0;
}

// Rule 3 of fury_row_compare, ascending, for one pair of non-null values whose spans lie inside their
// batches: -1 / 0 / +1 of the value of pr[0] (slot word s0, n0 payload bytes) against that of pr[1].
// Shared by pair_keys_compare and the ARGMIN / ARGMAX of aggregate.hip.
template <bool VAR>
__device__ __forceinline__ int value_compare(int kind, int width, int cls, const PairRow (&pr)[2], uint64_t s0,
                                             uint64_t s1, int64_t n0, int64_t n1) {
  if (VAR && kind == kBytes)
    return order_bytes(pr[0].rows, pr[0].base + static_cast<int32_t>(s0 >> 32), pr[0].total, n0,
                       pr[1].rows, pr[1].base + static_cast<int32_t>(s1 >> 32), pr[1].total, n1);
  if (VAR && kind == kDecimal) {                  // 16 bytes, little-endian two's complement
    const int64_t pl = pr[0].base + static_cast<int32_t>(s0 >> 32);
    const int64_t pq = pr[1].base + static_cast<int32_t>(s1 >> 32);
    const bool al = ((pl | pq) & 7) == 0;
    const uint64_t lo0 = pay_word(pr[0].rows, pl, pr[0].total, al);
    const uint64_t hi0 = pay_word(pr[0].rows, pl + 8, pr[0].total, al);
    const uint64_t lo1 = pay_word(pr[1].rows, pq, pr[1].total, al);
    const uint64_t hi1 = pay_word(pr[1].rows, pq + 8, pr[1].total, al);
    return order_decimal(lo0, hi0, lo1, hi1);
  }
  if (kind == kBool) return static_cast<int>((s0 & 0xff) != 0) - static_cast<int>((s1 & 0xff) != 0);
  const uint64_t x = order_fixed(s0, width, cls), y = order_fixed(s1, width, cls);    // kFixed
  return x < y ? -1 : x > y ? 1 : 0;
}

// The order of the pair pr[0] / pr[1] over the key positions (key[k].left_slot of pr[0] against
// key[k].right_slot of pr[1]): -1 / 0 / +1, the first position that differs decides.  As in
// pair_keys_equal every key is examined for its null bit and bounds whatever the earlier keys gave,
// `fail` is set (never cleared) when a value's span leaves its batch, and a side that is not ok has
// every key null; here a failed value simply ranks as a null, so the result stays a total preorder.
// Payloads are read only while the pair is undecided.  `key` is indexed wave-uniformly.
template <bool VAR>
__device__ __forceinline__ int pair_keys_compare(const PairRow (&pr)[2], COrderKey* key, int nkeys,
                                                 bool& fail) {
  int res = 0;
  for (int k0 = 0; k0 < nkeys; k0 += kKeyGroup) {
    uint64_t bits[kKeyGroup][2], slot[kKeyGroup][2];
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {         // every header word of the group, both sides
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bits[u][s] = ~uint64_t(0);                // a row that cannot be read: every key null
        slot[u][s] = 0;
        if (k0 + u < nkeys && pr[s].ok) {
          COrderKey& c = key[k0 + u];
          const int32_t f = s == 0 ? c.left_slot : c.right_slot;
          const uint8_t* hdr = pr[s].rows + pr[s].base;
          bits[u][s] = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
          slot[u][s] = load8(hdr + pr[s].bitmap_bytes + 8 * static_cast<int64_t>(f));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kKeyGroup; u++) {
      if (k0 + u >= nkeys) break;
      COrderKey& c = key[k0 + u];
      const int kind = c.kind, width = c.width, flags = c.flags;
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
          if (bad) {
            fail = true;
            isnull[s] = true;
          }
        }
      }
      if (res != 0) continue;                     // decided: only the null bits and bounds above
      if (isnull[0] || isnull[1]) {               // rule 2: absolute, DESC does not flip it
        if (isnull[0] != isnull[1]) res = (isnull[0] != ((flags & FURY_ORDER_NULLS_LAST) != 0)) ? -1 : 1;
        continue;
      }
      const int c3 = value_compare<VAR>(kind, width, c.cls, pr, slot[u][0], slot[u][1], n[0], n[1]);
      res = (flags & FURY_ORDER_DESC) ? -c3 : c3;
    }
  }
  return res;
}

}  // namespace

}  // namespace fury
