// zip.hip -- the fields of several row batches joined row by row, as rows (fury_row_zip).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): per row, the
// getters of several BinaryRows feeding one fresh BinaryRowWriter of the combined schema: a fixed-width
// field is write(ordinal, <primitive>) (FMT/row/binary/writer/BinaryRowWriter.java:86-129), a
// variable-length one writeUnaligned / write(ordinal, BinaryRow | BinaryArray | BinaryMap)
// (FMT/row/binary/writer/BinaryWriter.java:161-212,243-245).  It is select.hip with the source row
// looked up per pick: a value addresses everything below it relative to its own base, so its bytes move
// unchanged whichever row they came from.
//
// MI355X design (the three kernels of select.hip, each word finding its source first):
//   fixed      no pick is variable-length: output row r sits at r * F', no scan.  Lanes own 16-byte
//              chunks, a word's row comes by multiply-high.  A slot word checks and reads the row of its
//              own source only; a bitmap word gathers its picks' bits from their sources -- by its own
//              lane below kZipCoopFields picks, by a ballot of the wave (lane l = pick 64 q + l) from
//              there on, the row starts of the <= 4 sources being the same in every lane.
//   measure    lane = row, the picks in order (the table is indexed wave-uniformly, so the source of a
//              pick is a scalar and its row start a select among four registers: the row starts are
//              read once per source, never indexed dynamically).  Leaves the row's OUTPUT bitmap words
//              (a failed source row or value is already a set bit there), the start W of every
//              variable-length pick, and the row size.
//   scan       device_scan of the sizes in out_offsets.
//   write      select_write with the staged rows' starts kept per source, the same instance of
//              write_spans / store_words (take_dev.h) with its own LDS struct: a workgroup owns kTakeSpan
//              output bytes, kZipRows rows are staged per round (20 KB of LDS with the four source
//              starts, 30 KB with the table: five workgroups a CU), each 8-byte word is made from its
//              segment; a payload word finds its value in the row's W list, then that value's source.
// The table sits in LDS for the per-lane lookups when it has at most kZipLdsWords words, and so do the
// per-source arguments (ZipLds): a lane whose source index differs from its neighbour's reads its
// source's pointers and sizes from LDS, which measured 4-11 % faster than choosing them by selects
// (DESIGN 4l).
// Bounds (ZipArgs in kernels.h): nothing outside [0, total_s) of source s is read, a source no pick
// names is never read, the output is written only inside [0, min(capacity, needed)).
#include "select_dev.h"

namespace fury {

namespace {

constexpr int kZipLdsWords = 2560;                // 10 KB: 512 fixed-width picks
constexpr int kZipCoopFields = 16;                // as kSelCoopFields (select.hip)
constexpr int kZipRows = 512;                     // rows staged in LDS per round of the write pass

// One of four values by source index: selects, never an indexed register array.  Used where the index
// is wave-uniform (the measure pass) and for the row starts, which live in registers.
template <class V>
__device__ __forceinline__ V by_source(int s, V v0, V v1, V v2, V v3) {
  return s == 0 ? v0 : s == 1 ? v1 : s == 2 ? v2 : v3;
}
__device__ __forceinline__ ZipSource source_of(const ZipArgs& a, int s) {
  ZipSource z;
  z.rows = by_source(s, a.src[0].rows, a.src[1].rows, a.src[2].rows, a.src[3].rows);
  z.row_offsets = by_source(s, a.src[0].row_offsets, a.src[1].row_offsets, a.src[2].row_offsets,
                            a.src[3].row_offsets);
  z.bitmap_bytes = by_source(s, a.src[0].bitmap_bytes, a.src[1].bitmap_bytes, a.src[2].bitmap_bytes,
                             a.src[3].bitmap_bytes);
  z.fixed_size = by_source(s, a.src[0].fixed_size, a.src[1].fixed_size, a.src[2].fixed_size,
                           a.src[3].fixed_size);
  return z;
}

// The bytes of each source that some pick names (0 for the others, which are never read).
struct ZipTotals {
  int64_t t0, t1, t2, t3;
  __device__ __forceinline__ int64_t of(int s) const { return by_source(s, t0, t1, t2, t3); }
};
__device__ __forceinline__ int64_t total_of(const ZipArgs& a, int s) {
  if (!((a.used >> s) & 1)) return 0;
  return a.src[s].row_offsets ? gl(a.src[s].row_offsets)[a.nrows] : a.nrows * a.src[s].fixed_size;
}
__device__ __forceinline__ ZipTotals totals_of(const ZipArgs& a) {
  return ZipTotals{total_of(a, 0), total_of(a, 1), total_of(a, 2), total_of(a, 3)};
}

// The per-source arguments and totals in LDS, for lookups by a per-lane source index.
struct ZipLds {
  ZipSource z[kZipMaxSources];
  int64_t tot[kZipMaxSources];
};
__device__ __forceinline__ void stage_sources(const ZipArgs& a, const ZipTotals& t, ZipLds* L) {
  if (threadIdx.x < kZipMaxSources) {
    const int s = threadIdx.x;
    L->z[s] = source_of(a, s);
    L->tot[s] = t.of(s);
  }
  lds_barrier();
}

// Row r of every source that is used: the starts, and bit s of `ok` when the row of s may be read.
struct ZipRow {
  int64_t b0, b1, b2, b3;
  uint32_t ok;
  __device__ __forceinline__ int64_t start(int s) const { return by_source(s, b0, b1, b2, b3); }
};
__device__ __forceinline__ ZipRow row_of(const ZipArgs& a, int64_t r, const ZipTotals& t) {
  ZipRow w{0, 0, 0, 0, 0};
  if ((a.used & 1) && source_row(a.src[0], r, t.t0, &w.b0)) w.ok |= 1;
  if ((a.used & 2) && source_row(a.src[1], r, t.t1, &w.b1)) w.ok |= 2;
  if ((a.used & 4) && source_row(a.src[2], r, t.t2, &w.b2)) w.ok |= 4;
  if ((a.used & 8) && source_row(a.src[3], r, t.t3, &w.b3)) w.ok |= 8;
  return w;
}

// Output rows of Wn 8-byte words at r * Wn; magic = 2^64 / Wn rounded up (exact for the word counts
// launch_zip admits).
__global__ __launch_bounds__(kTakeThreads) void zip_fixed(ZipArgs a, uint64_t Wn, uint64_t magic) {
  __shared__ int32_t tl[kZipLdsWords];
  const StagedTable T = stage_table(table_of(a), 5 * a.nsel + a.nvar, tl, kZipLdsWords);
  const int64_t n = a.nrows;
  const ZipTotals tot = totals_of(a);
  __shared__ ZipLds L;
  stage_sources(a, tot, &L);
  const int nbw = a.out_bitmap_bytes >> 3;
  auto word_of = [&](uint64_t g) -> uint64_t {
    const uint64_t r = __umul64hi(g, magic);
    const int q = static_cast<int>(g - r * Wn);
    if (q < nbw) {                    // gather the bits of picks [64 q, 64 q + 64) from their sources
      const ZipRow w = row_of(a, static_cast<int64_t>(r), tot);
      if (q == 0 && w.ok != a.used) raise_oob(a.err, static_cast<int64_t>(r));
      uint64_t bits = 0, sw = 0;
      int at = -1;
      const int je = min(64 * q + 64, a.nsel);
      for (int j = 64 * q; j < je; j++) {
        const int k = T[5 * j], s = T[5 * j + 4];
        uint64_t bit = 1;
        if ((w.ok >> s) & 1) {
          const int key = (s << 26) | (k >> 6);
          if (key != at) {
            at = key;
            sw = word(L.z[s].rows + w.start(s) + 8 * (k >> 6));
          }
          bit = (sw >> (k & 63)) & 1;
        }
        bits |= bit << (j & 63);
      }
      return bits;
    }
    const int j = q - nbw;
    const int k = T[5 * j], s = T[5 * j + 4];
    const ZipSource z = L.z[s];
    int64_t B;
    if (!source_row(z, static_cast<int64_t>(r), L.tot[s], &B)) return 0;     // raised with word 0
    const uint8_t* row = z.rows + B;
    if ((word(row + 8 * (k >> 6)) >> (k & 63)) & 1) return 0;
    return fixed_slot(word(row + z.bitmap_bytes + 8 * k), T[5 * j + 1]);
  };
  const uint64_t nw = static_cast<uint64_t>(n) * Wn;
  const uint64_t head = (reinterpret_cast<uintptr_t>(a.out) >> 3) & 1;     // words before 16-byte alignment
  const uint64_t nchunks = (nw - head) >> 1;
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (g0 == 0) {
    if (head) st8(a.out, word_of(0));
    if ((nw - head) & 1) st8(a.out + 8 * (nw - 1), word_of(nw - 1));
  }
  // A wave owns 128 consecutive words per step; from kZipCoopFields picks on, the bitmap words among
  // them are made by the whole wave: lane l tests pick 64 q + l in its source, the ballot is the word.
  const bool coop = a.nsel >= kZipCoopFields;
  const int lane = threadIdx.x & 63;
  for (uint64_t cb = g0 - lane; cb < nchunks; cb += static_cast<uint64_t>(gridDim.x) * kTakeThreads) {
    const uint64_t g = head + 2 * (cb + lane);
    v2q v{0, 0};
    bool have_x = false, have_y = false;
    if (coop) {
      const uint64_t w0 = head + 2 * cb, w1 = min(w0 + 128, head + 2 * nchunks);
      for (uint64_t r = __umul64hi(w0, magic); r * Wn < w1; r++) {     // the same rows in every lane
        const ZipRow w = row_of(a, static_cast<int64_t>(r), tot);
        for (int q = 0; q < nbw; q++) {
          const uint64_t gq = r * Wn + q;
          if (gq < w0 || gq >= w1) continue;
          const int j = 64 * q + lane;
          bool bit = false;
          if (j < a.nsel) {
            const int k = T[5 * j], s = T[5 * j + 4];
            bit = true;
            if ((w.ok >> s) & 1)
              bit = (word(L.z[s].rows + w.start(s) + 8 * (k >> 6)) >> (k & 63)) & 1;
          }
          const uint64_t m = __ballot(bit);
          if (q == 0 && lane == 0 && w.ok != a.used) raise_oob(a.err, static_cast<int64_t>(r));
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
// of the v-th variable-length pick starts (a null one: where the next one does).
__global__ __launch_bounds__(kTakeThreads) void zip_measure(ZipArgs a, uint64_t* __restrict__ wbm,
                                                            int32_t* __restrict__ wW) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  const int64_t n = a.nrows;
  if (r >= n) return;
  CI32* T = table_of(a);
  const ZipTotals tot = totals_of(a);
  const int nbw = a.out_bitmap_bytes >> 3;
  const ZipRow w = row_of(a, r, tot);
  int64_t W = a.out_fixed_size;
  bool fail = false, bad = w.ok != a.used;
  uint64_t bits = 0, sw = 0;
  int at = -1;
  for (int j = 0; j < a.nsel; j++) {
    const int k = T[5 * j], s = T[5 * j + 4];     // wave-uniform: the source is a scalar
    const ZipSource z = source_of(a, s);
    const int64_t B = w.start(s), total = tot.of(s);
    const uint8_t* row = z.rows + B;
    bool null = true;
    if ((w.ok >> s) & 1) {
      const int key = (s << 26) | (k >> 6);
      if (key != at) {
        at = key;
        sw = word(row + 8 * (k >> 6));
      }
      null = (sw >> (k & 63)) & 1;
    }
    if (T[5 * j + 1] == kSelVar) {
      const int32_t rule = T[5 * j + 2], need = rule & kSelNeed;
      const int64_t start = W;
      if (!null) {
        const uint64_t sl = word(row + z.bitmap_bytes + 8 * k);
        const int32_t off = static_cast<int32_t>(sl >> 32), size = static_cast<int32_t>(sl);
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
      gl(wW)[r * a.nvar + T[5 * j + 3]] = static_cast<int32_t>(min<int64_t>(start, INT32_MAX));
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

struct ZipShared {
  int64_t oo[kZipRows + 1];           // output start of the staged rows, and the end of the last one
  int64_t src[kZipMaxSources][kZipRows];   // their start in every source that is used
};

__global__ __launch_bounds__(kTakeThreads) void zip_write(ZipArgs a, const uint64_t* __restrict__ wbm,
                                                          const int32_t* __restrict__ wW) {
  __shared__ ZipShared sh;
  __shared__ int32_t tl[kZipLdsWords];
  const StagedTable T = stage_table(table_of(a), 5 * a.nsel + a.nvar, tl, kZipLdsWords);
  const ZipTotals tot = totals_of(a);
  __shared__ ZipLds L;
  stage_sources(a, tot, &L);
  const int nbw = a.out_bitmap_bytes >> 3;
  auto stage = [&](int64_t r, int k) {
#pragma unroll
    for (int s = 0; s < kZipMaxSources; s++) {
      if (!((a.used >> s) & 1)) continue;
      const ZipSource& z = a.src[s];
      sh.src[s][k] = z.row_offsets ? gl(z.row_offsets)[r] : r * z.fixed_size;
    }
  };
  auto round = [&](int64_t r0, int kn, int64_t a0, int64_t b0) {
    store_words(a.out, a0, b0, [&](int64_t d) -> uint64_t {
      const int lo = staged_row(sh.oo, kn, d);      // every row has bytes
      const int64_t r = r0 + lo;
      // 64-bit until it is used: narrowed here, the compiler split the narrowing over the
      // subtraction and a row that starts below 2^31 and ends above it read 2^32 bytes low
      const int64_t x = d - sh.oo[lo];
      if (x < a.out_bitmap_bytes) return gl(wbm)[r * nbw + (x >> 3)];
      if (x < a.out_fixed_size) {
        const int j = static_cast<int>((x - a.out_bitmap_bytes) >> 3);
        if ((gl(wbm)[r * nbw + (j >> 6)] >> (j & 63)) & 1) return 0;
        const int32_t width = T[5 * j + 1];
        const int s = T[5 * j + 4];
        const ZipSource z = L.z[s];
        const uint64_t sl = word(z.rows + sh.src[s][lo] + z.bitmap_bytes + 8 * T[5 * j]);
        if (width != kSelVar) return fixed_slot(sl, width);
        const uint64_t W = static_cast<uint32_t>(gl(wW)[r * a.nvar + T[5 * j + 3]]);
        return (W << 32) | static_cast<uint32_t>(sl);
      }
      // payload: the last variable-length pick that starts at or before x has bytes there
      const int32_t* Wr = wW + r * a.nvar;
      int vl = 0, vh = a.nvar - 1;
      while (vl < vh) {
        const int mid = (vl + vh + 1) >> 1;
        if (gl(Wr)[mid] <= x) vl = mid;
        else vh = mid - 1;
      }
      const int j = T[5 * a.nsel + vl];
      const int s = T[5 * j + 4];
      const ZipSource z = L.z[s];
      const int64_t B = sh.src[s][lo];
      const uint64_t sl = word(z.rows + B + z.bitmap_bytes + 8 * T[5 * j]);
      const int64_t pos = x - gl(Wr)[vl];
      const int64_t left = static_cast<int32_t>(sl) - pos;          // >= 1 bytes of the value
      const int64_t p = B + static_cast<int32_t>(sl >> 32) + pos;
      if (left >= 8) return ld8(z.rows + p);
      uint64_t v = 0;
      if (p + 8 <= L.tot[s]) {
        v = ld8(z.rows + p) & ((1ull << (8 * left)) - 1);
      } else {                        // the value ends its batch: no byte past it is read
        for (int i = 0; i < left; i++) v |= static_cast<uint64_t>(gl(z.rows)[p + i]) << (8 * i);
      }
      return v;
    });
  };
  write_spans<kZipRows>(sh, a.nrows, a.out_offsets, a.cap, stage, round);
}

}  // namespace

int launch_zip(const ZipArgs& args, const int32_t* table, int nwords, hipStream_t stream) {
  ZipArgs a = args;
  const int64_t n = a.nrows;
  DeviceTable dt;
  int st = place_table(&a, table, nwords, stream, &dt);
  if (st) return st;
  if (a.nvar == 0) {                  // fixed-width picks: row r at r * out_fixed_size
    if (a.out_offsets)
      hipLaunchKernelGGL(fixed_offsets, dim3(blocks_of(n + 1)), dim3(kTakeThreads), 0, stream,
                         a.out_offsets, n, static_cast<const int64_t*>(nullptr),
                         static_cast<int64_t>(a.out_fixed_size));
    if (a.out && n > 0) {
      const uint64_t Wn = static_cast<uint64_t>(a.out_fixed_size) / 8;
      const int64_t chunks = (n * static_cast<int64_t>(Wn) + 1) / 2;
      const unsigned grid = static_cast<unsigned>(
          std::min<int64_t>((chunks + kTakeThreads - 1) / kTakeThreads, kTakeMaxGrid));
      hipLaunchKernelGGL(zip_fixed, dim3(grid), dim3(kTakeThreads), 0, stream, a, Wn, ~0ull / Wn + 1);
    }
    return check_hip(hipGetLastError(), "zip launch");
  }
  if (n == 0) return check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
  SelectWorkspace w;
  st = alloc_workspace(a, stream, &w);
  if (st) return st;
  hipLaunchKernelGGL(zip_measure, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, w.wbm, w.wW);
  device_scan(a.out_offsets, n, a.out_offsets + n, w.ws, stream);
  if (a.out && a.cap >= 8)
    hipLaunchKernelGGL(zip_write, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a, w.wbm, w.wW);
  st = check_hip(hipGetLastError(), "zip launch");
  dev_free(w.ws, stream);
  return st;
}

}  // namespace fury
