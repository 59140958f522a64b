// order.hip -- order words: chunk `chunk` of one key field of every selected row as a signed 64-bit
// word whose integer order is the rows' order on that key (fury_row_order_words).  The piece that lets
// an integer sort (torch.sort, rocPRIM, any radix sort) order rows by STRING, BINARY, DECIMAL and
// multi-field keys: sort by the words of chunk 0, refine the rows that tie and continue with chunk 1.
//
// Reference semantics: the order is fury_row_compare's (include/fury_row.h).  The normalised key
// bytes NK of a value are a byte string whose unsigned lexicographic order, prefix first, is rule 3:
// a fixed-width value big-endian with the sign bit flipped (floats: the total-order transform,
// order_fixed in keys_dev.h), BOOL one byte, DECIMAL 16 bytes big-endian with the sign flipped, STRING
// / BINARY the payload.  Word = NK[7 chunk, 7 chunk + 7) big-endian in bits 63..8, zero-padded; low
// byte 1 + the value bytes in the chunk, 9 when more follow; DESC complements the word; a null is the
// minimum (NULLS_LAST: the maximum) of the encoding; last the top bit is flipped for signed order.
//
// MI355X design: lane = output row, 256-thread workgroups, no LDS, no atomics.  A gather with a
// dependent chain index -> row offset -> (bitmap word, slot word) -> at most two payload words; the
// two header words are issued together, and so are the two aligned payload words that cover the
// chunk's 7 bytes wherever the value starts (a funnel shift joins them).  Every lane carries one
// chain, so the latency is hidden by occupancy: the kernel keeps its registers low enough for 8
// waves per SIMD.  The word stores are coalesced.  *out_more is written without an atomic: a ballot,
// then one plain store of 1 by one lane of every wave that has a continuing row (every writer stores
// the same value; the launcher zeroes the word on the stream first).
// Bounds follow "Decode bounds" in kernels.h as hash.hip applies them; address arithmetic is int64.
#include <hip/hip_runtime.h>

#include "keys_dev.h"

namespace fury {

namespace {

constexpr int kOrdThreads = 256;

// The `cnt` (1..7) batch bytes at s, [s, s + cnt) inside [0, total), first byte in the top byte of the
// result, the rest zero: the aligned words that cover them (rows is 8-byte aligned), or, for the
// batch's last bytes when total is no multiple of 8, by byte.
__device__ __forceinline__ uint64_t chunk_bytes(const uint8_t* rows, int64_t s, int cnt, int64_t total) {
  const int sh = static_cast<int>(s & 7) * 8;
  const int64_t al = s & ~int64_t(7);
  const bool need2 = (s & 7) + cnt > 8;
  const bool two = al + 16 <= total;
  uint64_t v = 0;
  if (al + 8 <= total && (two || !need2)) {
    const uint64_t lo = load8(rows + al);
    const uint64_t hi = two ? load8(rows + al + 8) : 0;
    v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
  } else {
    for (int i = 0; i < cnt; i++) v |= static_cast<uint64_t>(gl(rows)[s + i]) << (8 * i);
  }
  v &= ~uint64_t(0) >> (64 - 8 * cnt);
  return __builtin_bswap64(v);
}

__global__ __launch_bounds__(kOrdThreads) void order_words(OrderWordsArgs a) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kOrdThreads + threadIdx.x;
  const bool active = j < a.num_out;
  const KeySide& sd = a.side;
  int64_t row = j;
  if (active && sd.indices) row = gl(sd.indices)[j];
  const int64_t total = sd.row_offsets ? gl(sd.row_offsets)[sd.nrows] : sd.nrows * sd.fixed_size;
  bool ok = active && row >= 0 && row < sd.nrows;
  int64_t base = 0;
  if (ok) base = sd.row_offsets ? gl(sd.row_offsets)[row] : row * sd.fixed_size;
  ok = ok && row_ok(base, sd.fixed_size, total);
  bool fail = active && !ok;
  const int32_t f = a.key.left_slot;
  const int kind = a.key.kind, width = a.key.width;
  uint64_t bits = ~uint64_t(0), slot = 0;         // a row that cannot be read: the key is null
  if (ok) {
    const uint8_t* hdr = sd.rows + base;
    bits = load8(hdr + 8 * static_cast<int64_t>(f >> 6));
    slot = load8(hdr + sd.bitmap_bytes + 8 * static_cast<int64_t>(f));
  }
  bool isnull = (bits >> (f & 63)) & 1;
  int64_t len = width;                            // NK's length
  if (kind >= kBytes && !isnull) {
    bool bad = false;
    len = slot_count(kind, width, slot, base, sd.rows, total, &bad);
    if (kind == kDecimal) len = 16;
    if (bad) {
      fail = true;
      isnull = true;
    }
  }
  const int64_t off = 7 * static_cast<int64_t>(a.chunk);
  uint64_t word = (a.key.flags & FURY_ORDER_NULLS_LAST) ? ~uint64_t(0) : 0;
  bool more = false;
  if (!isnull) {
    uint64_t top = 0;                             // the chunk's bytes, big-endian in bits 63..8
    int cnt = 0;
    if (off < len) {
      const int64_t left = len - off;
      more = left > 7;
      cnt = more ? 7 : static_cast<int>(left);
      const int sh = kind == kBytes ? 0 : static_cast<int>(off) * 8;   // < 128: off < len <= 16 there
      if (kind == kBytes) {
        top = chunk_bytes(sd.rows, base + static_cast<int32_t>(slot >> 32) + off, cnt, total);
      } else if (kind == kDecimal) {              // 16 bytes, little-endian two's complement
        const int64_t p = base + static_cast<int32_t>(slot >> 32);
        const bool al = (p & 7) == 0;
        const uint64_t lo = pay_word(sd.rows, p, total, al);
        const uint64_t hi = pay_word(sd.rows, p + 8, total, al) ^ (uint64_t(1) << 63);
        top = sh == 0 ? hi : sh < 64 ? (hi << sh) | (lo >> (64 - sh)) : lo << (sh - 64);
      } else if (kind == kBool) {
        top = static_cast<uint64_t>((slot & 0xff) != 0) << 56;
      } else {                                    // kFixed: left-aligned, then shifted to the chunk
        top = (order_fixed(slot, width, a.key.cls) << (64 - 8 * width)) << sh;
      }
      top &= ~uint64_t(0xff);
    }
    word = top | static_cast<uint64_t>(more ? 9 : 1 + cnt);
    if (a.key.flags & FURY_ORDER_DESC) word = ~word;
  }
  if (fail) raise_oob(a.err, j);
  if (active) gl(a.out_words)[j] = static_cast<int64_t>(word ^ (uint64_t(1) << 63));
  if (a.out_more) {
    const uint64_t m = __ballot(active && more);
    if (m && (threadIdx.x & 63) == __builtin_ctzll(m)) gl(a.out_more)[0] = 1u;
  }
}

}  // namespace

int launch_order_words(const OrderWordsArgs& a, hipStream_t stream) {
  if (a.out_more) {
    const int st = check_hip(hipMemsetAsync(a.out_more, 0, 4, stream), "memset");
    if (st) return st;
  }
  if (a.num_out == 0) return FURY_OK;
  const int64_t nb = (a.num_out + kOrdThreads - 1) / kOrdThreads;
  if (nb > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  hipLaunchKernelGGL(order_words, dim3(static_cast<unsigned>(nb)), dim3(kOrdThreads), 0, stream, a);
  return check_hip(hipGetLastError(), "order_words launch");
}

}  // namespace fury
