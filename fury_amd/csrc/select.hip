// select.hip -- a subset of a row batch's top-level fields, as rows (fury_row_select).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): per row, a fresh
// BinaryRowWriter of the selected schema fed from BinaryRow's getters.  A fixed-width field is
// write(ordinal, <primitive>): putInt64(offset, 0) and the narrow put, so the slot is the value's own
// bytes zero-extended (FMT/row/binary/writer/BinaryRowWriter.java:86-129); a variable-length field is
// writeUnaligned / write(ordinal, BinaryRow | BinaryArray | BinaryMap) -> writeAlignedBytes / copyTo
// (FMT/row/binary/writer/BinaryWriter.java:161-212,243-245): the value's bytes at the 8-aligned writer
// index, zero padding to the next multiple of 8, and the slot (writer index - row start) << 32 | size.
// A value addresses everything below it relative to its own base, so its bytes move unchanged.
//
// MI355X design:
//   fixed      the selection has no variable-length field (always so for an is_fixed source): output
//              row r sits at r * F', no scan.  Lanes own consecutive 16-byte chunks of the output (two
//              8-byte words; one 8-byte word at either end when the buffer is 8 mod 16), a word's row is
//              its index / words per row by multiply-high (as take_copy_fixed).  A bitmap word gathers
//              its up-to-64 source bits -- by its own lane for narrow selections, by a ballot of the
//              wave (lane l = field 64 q + l) from kSelCoopFields fields on --, a slot word is the
//              source slot masked to the field's width.
//   measure    lane = row, the selected fields in order (the table is indexed wave-uniformly: scalar
//              loads): only the bitmap words and slots of selected fields are read, each variable-length
//              value is validated once, and the pass leaves behind everything the write pass needs to
//              agree with it: the row's OUTPUT bitmap words (a failed value or row is already a set
//              bit there), the value start W of every selected variable-length field, the row size.
//   scan       device_scan of the sizes in out_offsets.
//   write      output-parallel and balanced by bytes: an instance of write_spans (take_dev.h), the
//              write pass copy_rows is an instance of too -- a workgroup owns kTakeSpan output bytes,
//              finds its rows by the 64-ary search of out_offsets, stages (output start, source
//              start) in LDS, and lanes own 16-byte chunks, two words each (store_words).
//              Each 8-byte word finds its row by binary search in LDS and then its segment: a bitmap
//              word (loaded from the measure pass), a slot (null: 0; fixed-width: the masked source
//              slot; variable-length: W << 32 | size) or payload -- binary search of the row's W list for
//              the value, whose source slot gives where its bytes are; the value's last word is masked
//              to the bytes it has, so source padding never reaches the output.  A 70 KB value is
//              copied by as many lanes as it has words.
// The selection table sits in LDS for the per-lane lookups when it has at most kSelLdsWords words.
// Bounds (SelectArgs in kernels.h): nothing outside [0, total) of the rows buffer is read, the output
// is written only inside [0, min(capacity, needed)).
#include "select_dev.h"

namespace fury {

namespace {

constexpr int kSelLdsWords = 2560;                // 10 KB: 512 selected fields, all variable-length
// Fixed-width selections of at least this many fields make their bitmap words by ballot.  Measured
// (DESIGN 4k): with the owning lane gathering 64 bits alone, 97 of 100 fields of 1M rows took 1.67
// ms, with the ballot 0.87; at 10 fields a wave holds 12 bitmap words of 10 bits, which 12 lanes
// gather at once.
constexpr int kSelCoopFields = 16;

// Output rows of Wn 8-byte words at r * Wn; magic = 2^64 / Wn rounded up (exact for the word counts
// launch_select admits).
__global__ __launch_bounds__(kTakeThreads) void select_fixed(SelectArgs a, uint64_t Wn,
                                                             uint64_t magic) {
  __shared__ int32_t tl[kSelLdsWords];
  const StagedTable T = stage_table(table_of(a), 4 * a.nsel + a.nvar, tl, kSelLdsWords);
  const int64_t n = a.nrows;
  const int64_t total = a.row_offsets ? gl(a.row_offsets)[n] : n * a.fixed_size;
  const int nbw = a.out_bitmap_bytes >> 3;
  auto word_of = [&](uint64_t g) -> uint64_t {
    const uint64_t r = __umul64hi(g, magic);
    const int q = static_cast<int>(g - r * Wn);
    int64_t B;
    if (!source_row(a, static_cast<int64_t>(r), total, &B)) {
      if (q == 0) raise_oob(a.err, static_cast<int64_t>(r));
      return q < nbw ? all_null(q, a.nsel) : 0;
    }
    const uint8_t* row = a.rows + B;
    if (q < nbw) {                    // gather the source bits of fields [64 q, 64 q + 64)
      uint64_t bits = 0, sw = 0;
      int at = -1;
      const int je = min(64 * q + 64, a.nsel);
      for (int j = 64 * q; j < je; j++) {
        const int k = T[4 * j];
        if ((k >> 6) != at) {
          at = k >> 6;
          sw = word(row + 8 * at);
        }
        bits |= ((sw >> (k & 63)) & 1) << (j & 63);
      }
      return bits;
    }
    const int j = q - nbw;
    const int k = T[4 * j];
    if ((word(row + 8 * (k >> 6)) >> (k & 63)) & 1) return 0;
    return fixed_slot(word(row + a.bitmap_bytes + 8 * k), T[4 * j + 1]);
  };
  const uint64_t nw = static_cast<uint64_t>(n) * Wn;
  const uint64_t head = (reinterpret_cast<uintptr_t>(a.out) >> 3) & 1;     // words before 16-byte alignment
  const uint64_t nchunks = (nw - head) >> 1;
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (g0 == 0) {
    if (head) st8(a.out, word_of(0));
    if ((nw - head) & 1) st8(a.out + 8 * (nw - 1), word_of(nw - 1));
  }
  // A wave owns 128 consecutive words per step.  From kSelCoopFields selected fields on, the bitmap
  // words among them are made by the whole wave -- lane l tests field 64 q + l, the ballot is the
  // word -- so that no lane walks 64 fields while 63 wait; below that the owning lane gathers them.
  const bool coop = a.nsel >= kSelCoopFields;
  const int lane = threadIdx.x & 63;
  for (uint64_t cb = g0 - lane; cb < nchunks; cb += static_cast<uint64_t>(gridDim.x) * kTakeThreads) {
    const uint64_t g = head + 2 * (cb + lane);
    v2q v{0, 0};
    bool have_x = false, have_y = false;
    if (coop) {
      const uint64_t w0 = head + 2 * cb, w1 = min(w0 + 128, head + 2 * nchunks);
      for (uint64_t r = __umul64hi(w0, magic); r * Wn < w1; r++) {     // the same rows in every lane
        int64_t B;
        const bool ok = source_row(a, static_cast<int64_t>(r), total, &B);
        for (int q = 0; q < nbw; q++) {
          const uint64_t gq = r * Wn + q;
          if (gq < w0 || gq >= w1) continue;
          uint64_t m = all_null(q, a.nsel);
          if (ok) {
            const int j = 64 * q + lane;
            bool bit = false;
            if (j < a.nsel) {
              const int k = T[4 * j];
              bit = (word(a.rows + B + 8 * (k >> 6)) >> (k & 63)) & 1;
            }
            m = __ballot(bit);
          } else if (q == 0 && lane == 0) {
            raise_oob(a.err, static_cast<int64_t>(r));
          }
          const int o = static_cast<int>(gq - w0);
          if (lane == (o >> 1)) {
            if (o & 1) {
              v.y = m;
              have_y = true;
            } else {
              v.x = m;
              have_x = true;
            }
          }
        }
      }
    }
    if (cb + lane < nchunks) {
      if (!have_x) v.x = word_of(g);
      if (!have_y) v.y = word_of(g + 1);
      st16(a.out + 8 * g, v);
    }
  }
}

// wbm[r * nbw + q]: bitmap word q of output row r; wW[r * nvar + v]: where in the output row the value
// of the v-th selected variable-length field starts (a null one: where the next one does).
__global__ __launch_bounds__(kTakeThreads) void select_measure(SelectArgs a,
                                                               uint64_t* __restrict__ wbm,
                                                               int32_t* __restrict__ wW) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  const int64_t n = a.nrows;
  if (r >= n) return;
  CI32* T = table_of(a);
  const int64_t total = gl(a.row_offsets)[n];
  const int nbw = a.out_bitmap_bytes >> 3;
  int64_t B;
  const bool ok = source_row(a, r, total, &B);
  const uint8_t* row = a.rows + B;
  int64_t W = a.out_fixed_size;
  bool fail = !ok, bad = false;
  uint64_t bits = 0, sw = 0;
  int at = -1;
  for (int j = 0; j < a.nsel; j++) {
    const int k = T[4 * j];
    bool null = true;
    if (ok) {
      if ((k >> 6) != at) {
        at = k >> 6;
        sw = word(row + 8 * at);
      }
      null = (sw >> (k & 63)) & 1;
    }
    if (T[4 * j + 1] == kSelVar) {
      const int32_t rule = T[4 * j + 2], need = rule & kSelNeed;
      const int64_t start = W;
      if (!null) {
        const uint64_t s = word(row + a.bitmap_bytes + 8 * k);
        const int32_t off = static_cast<int32_t>(s >> 32), size = static_cast<int32_t>(s);
        const bool valid = off >= 0 && size >= 0 && !(off & 7) && span_ok(B + off, size, total) &&
                           size >= need && (!(rule & kSelMod8) || !(size & 7)) &&
                           (!(rule & kSelExact) || size == need);
        if (valid) {
          W += (static_cast<int64_t>(size) + 7) & ~int64_t{7};
          if (W > INT32_MAX - 7) fail = true;
        } else {
          null = bad = true;
        }
      }
      gl(wW)[r * a.nvar + T[4 * j + 3]] = static_cast<int32_t>(min<int64_t>(start, INT32_MAX));
    }
    bits |= static_cast<uint64_t>(null) << (j & 63);
    if ((j & 63) == 63 || j == a.nsel - 1) {
      gl(wbm)[r * nbw + (j >> 6)] = bits;
      bits = 0;
    }
  }
  if (fail) {                         // every field null: the row is its header
    for (int q = 0; q < nbw; q++) gl(wbm)[r * nbw + q] = all_null(q, a.nsel);
    W = a.out_fixed_size;
  }
  if (fail || bad) raise_oob(a.err, r);
  gl(a.out_offsets)[r] = W;
}

__global__ __launch_bounds__(kTakeThreads) void select_write(SelectArgs a,
                                                             const uint64_t* __restrict__ wbm,
                                                             const int32_t* __restrict__ wW) {
  __shared__ TakeShared sh;
  __shared__ int32_t tl[kSelLdsWords];
  const StagedTable T = stage_table(table_of(a), 4 * a.nsel + a.nvar, tl, kSelLdsWords);
  const int64_t n = a.nrows;
  const int64_t total = gl(a.row_offsets)[n];
  const int nbw = a.out_bitmap_bytes >> 3;
  auto stage = [&](int64_t r, int k) { sh.src[k] = gl(a.row_offsets)[r]; };
  auto round = [&](int64_t r0, int kn, int64_t a0, int64_t b0) {
    store_words(a.out, a0, b0, [&](int64_t d) -> uint64_t {
      const int lo = staged_row(sh.oo, kn, d);      // every row has bytes
      const int64_t r = r0 + lo;
      // 64-bit until it is used: narrowed here, the compiler split the narrowing over the
      // subtraction and a row that starts below 2^31 and ends above it read 2^32 bytes low
      const int64_t x = d - sh.oo[lo];
      const uint8_t* row = a.rows + sh.src[lo];
      if (x < a.out_bitmap_bytes) return gl(wbm)[r * nbw + (x >> 3)];
      if (x < a.out_fixed_size) {
        const int j = static_cast<int>((x - a.out_bitmap_bytes) >> 3);
        if ((gl(wbm)[r * nbw + (j >> 6)] >> (j & 63)) & 1) return 0;
        const int32_t width = T[4 * j + 1];
        const uint64_t s = word(row + a.bitmap_bytes + 8 * T[4 * j]);
        if (width != kSelVar) return fixed_slot(s, width);
        const uint64_t W = static_cast<uint32_t>(gl(wW)[r * a.nvar + T[4 * j + 3]]);
        return (W << 32) | static_cast<uint32_t>(s);
      }
      // payload: the last variable-length field that starts at or before x has bytes there
      const int32_t* Wr = wW + r * a.nvar;
      int vl = 0, vh = a.nvar - 1;
      while (vl < vh) {
        const int mid = (vl + vh + 1) >> 1;
        if (gl(Wr)[mid] <= x) vl = mid;
        else vh = mid - 1;
      }
      const uint64_t s = word(row + a.bitmap_bytes + 8 * T[4 * T[4 * a.nsel + vl]]);
      const int64_t pos = x - gl(Wr)[vl];
      const int64_t left = static_cast<int32_t>(s) - pos;           // >= 1 bytes of the value
      const int64_t p = sh.src[lo] + static_cast<int32_t>(s >> 32) + pos;
      if (left >= 8) return ld8(a.rows + p);
      uint64_t v = 0;
      if (p + 8 <= total) {
        v = ld8(a.rows + p) & ((1ull << (8 * left)) - 1);
      } else {                        // the value ends the batch: no byte past it is read
        for (int i = 0; i < left; i++) v |= static_cast<uint64_t>(gl(a.rows)[p + i]) << (8 * i);
      }
      return v;
    });
  };
  write_spans<kTakeRows>(sh, n, a.out_offsets, a.cap, stage, round);
}

}  // namespace

int launch_select(const SelectArgs& args, const int32_t* table, int nwords, hipStream_t stream) {
  SelectArgs a = args;
  const int64_t n = a.nrows;
  DeviceTable dt;
  int st = place_table(&a, table, nwords, stream, &dt);
  if (st) return st;
  if (a.nvar == 0) {                  // fixed-width selection: row r at r * out_fixed_size
    if (a.out_offsets)
      hipLaunchKernelGGL(fixed_offsets, dim3(blocks_of(n + 1)), dim3(kTakeThreads), 0, stream,
                         a.out_offsets, n, static_cast<const int64_t*>(nullptr),
                         static_cast<int64_t>(a.out_fixed_size));
    if (a.out && n > 0) {
      const uint64_t Wn = static_cast<uint64_t>(a.out_fixed_size) / 8;
      const int64_t chunks = (n * static_cast<int64_t>(Wn) + 1) / 2;
      const unsigned grid = static_cast<unsigned>(
          std::min<int64_t>((chunks + kTakeThreads - 1) / kTakeThreads, kTakeMaxGrid));
      hipLaunchKernelGGL(select_fixed, dim3(grid), dim3(kTakeThreads), 0, stream, a, Wn,
                         ~0ull / Wn + 1);
    }
    return check_hip(hipGetLastError(), "select launch");
  }
  if (n == 0) return check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
  SelectWorkspace w;
  st = alloc_workspace(a, stream, &w);
  if (st) return st;
  hipLaunchKernelGGL(select_measure, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, w.wbm, w.wW);
  device_scan(a.out_offsets, n, a.out_offsets + n, w.ws, stream);
  if (a.out && a.cap >= 8)
    hipLaunchKernelGGL(select_write, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a, w.wbm,
                       w.wW);
  st = check_hip(hipGetLastError(), "select launch");
  dev_free(w.ws, stream);
  return st;
}

}  // namespace fury
