// implode.hip -- element rows back into LIST values (fury_row_implode) and nested values back into a
// one-field row (fury_row_wrap): the inverses of explode.hip and extract.hip.
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): per row, the batch
// form of BinaryArrayWriter.reset(n) followed by write(ordinal, BinaryRow | BinaryArray | BinaryMap) /
// setNullAt(ordinal) (FMT/row/binary/writer/BinaryArrayWriter.java:91-129, BinaryWriter.java:106-114,
// 243-245) and, for the rows form and for wrap, of a one-field BinaryRowWriter.write(0, BinaryArray |
// BinaryRow | BinaryMap).  A nested row, array or map addresses everything below it relative to its
// own base, so a value moves into a container as its bytes and one generated slot (offset << 32) | size
// relative to the container's base.
//
// MI355X design (the fused variant: one output-parallel write pass, no separate header pass, so every
// output byte is stored once and the header words of short lists ride in the same 16-byte stores as
// the payload next to them):
//   rank       lane = 64-element tile: the popcount of its elem_validity word, then device_scan -- the
//              rank of an element is its tile's base + the popcount of the lower bits of its word.
//              Skipped without a bitmap (rank = index).
//   elems      lane = ELEMENT, a wave = a tile: the value index, the value check (ImplodeArgs,
//              kernels.h), then per element the kept size (0: null or failed) and the source start, per
//              tile the ballots "kept" and "failed" and the failed count.  device_scan of the sizes
//              gives the clean value offsets cs[0 .. E] -- the present, well-formed values back to back
//              -- and device_scan of the failed counts makes "how many values failed in [a, b)" two
//              lookups.
//   rows       lane = row, O(1): the list_offsets range check, kept bytes = cs[b] - cs[a], the array and
//              row size, the report (a failed range, or a failed value inside a present row), and
//              (first element, count) for the write pass.  value_offsets is an offsets array, so the
//              values a row without a failed value takes are ONE run of `values`: its start is kept
//              too (rsrc).  device_scan makes out_offsets.
//   write      an instance of write_spans (take_dev.h), the write pass of copy_rows and select_write: a
//              workgroup owns kTakeSpan output bytes, finds its rows by the 64-ary search of
//              out_offsets, stages (output start, first element, count, cs of the first element,
//              payload source) in LDS, and lanes own 16-byte chunks (store_located, which map.hip's
//              join shares).  A word finds its row by binary search in LDS and is then GENERATED
//              -- row bitmap, row slot, element count, an array bitmap word (64 bits of the kept ballots
//              at the row's first element, inverted), an element slot (from cs) -- or COPIED: a payload
//              byte of a row whose values are one run is at that run's start + its position in the
//              payload, with nothing else to look up (every row a writer's rows give, and every
//              wrapped row); in a row that skips a failed value its position in the clean value stream
//              finds its element by binary search of cs inside the row's range, and the element's
//              source start gives the byte.  A chunk inside one run is one 16-byte non-temporal load
//              when the source aligns, else two 8-byte ones.  A 70,000-element list among empty rows is
//              70,000 lanes in elems and as many workgroups in write as it has 16 KB spans; nothing
//              loops over a row's elements or bytes.
// fury_row_wrap is the same three passes with element = row: a container with one slot, a fixed
// 16-byte header and no array header (ImplodeArgs.wrap).
// Bounds (ImplodeArgs in kernels.h): nothing outside [0, VT) of the values buffer is read, the output is
// written only inside [0, min(capacity, needed)).
#include "extract_dev.h"

namespace fury {

namespace {

constexpr int kTileWaves = kTakeThreads / 64;     // element tiles per workgroup of the elems pass
constexpr int64_t kMaxElems = (INT32_MAX - 15) / 8;      // BinaryArrayWriter.MAX_ROUNDED_ARRAY_LENGTH
constexpr int64_t kMaxSize = INT32_MAX - 7;

// tr: exclusive scan of the tile popcounts (NULL without a bitmap).  cs[e] = the kept size of element
// e (to be scanned), src[e] = where its bytes start; km[t] / fm[t]: the ballots "kept" and "present but
// failed the value check" of tile t, tf[t] the popcount of fm[t] (to be scanned).
__global__ __launch_bounds__(kTakeThreads) void implode_elems(ImplodeArgs a,
                                                              const int64_t* __restrict__ tr,
                                                              int64_t* __restrict__ cs,
                                                              int64_t* __restrict__ src,
                                                              uint64_t* __restrict__ km,
                                                              uint64_t* __restrict__ fm,
                                                              int64_t* __restrict__ tf) {
  const int lane = threadIdx.x & 63;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kTileWaves + (threadIdx.x >> 6);
  const int64_t E = a.num_elements;
  if (64 * t >= E) return;            // the whole wave
  const int64_t e = 64 * t + lane;
  const uint64_t w = tile_word(a.elem_validity, t, E);
  const bool present = (w >> lane) & 1;
  bool kept = false;
  int64_t s0 = 0, s1 = 0;
  if (present) {
    const int64_t v = a.elem_validity ? gl(tr)[t] + __popcll(w & ((1ull << lane) - 1)) : e;
    if (v < a.num_values) {
      const int64_t VT = gl(a.value_offsets)[a.num_values];
      s0 = gl(a.value_offsets)[v];
      s1 = gl(a.value_offsets)[v + 1];
      kept = s0 >= 0 && s0 <= s1 && s1 <= VT && !((s0 | s1) & 7) && s1 - s0 >= a.least;
    }
  }
  if (e < E) {
    gl(cs)[e] = kept ? s1 - s0 : 0;
    gl(src)[e] = s0;
  }
  const uint64_t k = __ballot(kept), f = __ballot(present && !kept);
  if (lane == 0) {
    gl(km)[t] = k;
    gl(fm)[t] = f;
    gl(tf)[t] = __popcll(f);
  }
}

// info[r] = (first element, element count) of output row r; count -1: the row is null or failed (rows
// form and wrap: 16 bytes, bit 0 set, slot 0).  rsrc[r]: where in `values` the row's payload starts
// when it is one run of bytes there, else -1.  value_offsets is an offsets array, so consecutive
// values are back to back: a row none of whose present elements failed takes the values rank(first
// element) .. in order, and its payload is the span from value_offsets[that rank] on, unchanged.
// out_offsets[r] = the row's size, to be scanned.
__global__ __launch_bounds__(kTakeThreads) void implode_rows(ImplodeArgs a,
                                                             const int64_t* __restrict__ tr,
                                                             const int64_t* __restrict__ cs,
                                                             const int64_t* __restrict__ src,
                                                             const uint64_t* __restrict__ km,
                                                             const uint64_t* __restrict__ fm,
                                                             const int64_t* __restrict__ tf,
                                                             v2l* __restrict__ info,
                                                             int64_t* __restrict__ rsrc) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (r >= a.nrows) return;
  const int64_t E = a.num_elements, nt = (E + 63) >> 6;
  int64_t size = a.prefix, from = -1;
  v2l in{0, -1};
  bool report = false;
  if (a.wrap) {
    bool kept = (gl(km)[r >> 6] >> (r & 63)) & 1;
    report = (gl(fm)[r >> 6] >> (r & 63)) & 1;
    const int64_t sz = gl(cs)[r + 1] - gl(cs)[r];
    if (kept && 16 + sz > kMaxSize) {
      kept = false;
      report = true;
    }
    if (kept) {
      in = v2l{r, 1};
      size = 16 + sz;
      from = gl(src)[r];
    }
  } else if (!a.entry_validity || ((gl(a.entry_validity)[r >> 5] >> (r & 31)) & 1)) {
    const int64_t p = gl(a.list_offsets)[r], q = gl(a.list_offsets)[r + 1];
    bool ok = p >= 0 && p <= q && q <= E && q - p <= kMaxElems;
    int64_t A = 0, bytes = 0;
    if (ok) {
      const int64_t n = q - p;
      bytes = gl(cs)[q] - gl(cs)[p];
      A = 8 + (((n + 63) >> 6) << 3) + 8 * n + bytes;
      ok = a.prefix + A <= kMaxSize;
    }
    if (ok) {
      // values that failed in [p, q): the scanned tile counts and the lower bits of the two words
      auto failed_below = [&](int64_t e) {
        const int64_t t = e >> 6;
        if (t >= nt) return gl(tf)[nt];
        return gl(tf)[t] + __popcll(gl(fm)[t] & ((1ull << (e & 63)) - 1));
      };
      report = failed_below(q) > failed_below(p);
      in = v2l{p, q - p};
      size = a.prefix + A;
      if (!report && bytes > 0) {     // p < E, and the rank of p is the index of a checked value
        const int64_t t = p >> 6;
        const int64_t v = !a.elem_validity ? p : gl(tr)[t] + __popcll(tile_word(a.elem_validity, t, E) &
                                                                      ((1ull << (p & 63)) - 1));
        from = gl(a.value_offsets)[v];
      }
    } else {
      report = true;
      if (!a.prefix) {                // collection form: an empty array
        in = v2l{0, 0};
        size = 8;
      }
    }
  }
  if (report) raise_oob(a.err, r);
  gl(a.out_offsets)[r] = size;
  gl(info)[r] = in;
  gl(rsrc)[r] = from;
}

// Rows staged in LDS per round of the write pass: 20 KB, so that LDS leaves 8 workgroups a CU (an
// output row has at least 8 bytes: a 16 KB span is at most four rounds).
constexpr int kImpRows = 512;

struct ImplodeShared {
  int64_t oo[kImpRows + 1];           // output start of the staged rows, and the end of the last one
  int64_t first[kImpRows];            // first element
  int64_t cnt[kImpRows];              // element count, -1: a null row
  int64_t cs0[kImpRows];              // cs[first]
  int64_t from[kImpRows];             // rsrc
};

__global__ __launch_bounds__(kTakeThreads) void implode_write(ImplodeArgs a,
                                                              const int64_t* __restrict__ cs,
                                                              const int64_t* __restrict__ src,
                                                              const uint64_t* __restrict__ km,
                                                              const v2l* __restrict__ info,
                                                              const int64_t* __restrict__ rsrc) {
  __shared__ ImplodeShared sh;
  const int64_t nt = (a.num_elements + 63) >> 6;
  const int P = a.prefix;
  auto stage = [&](int64_t r, int k) {
    const v2l in = gl(info)[r];
    sh.first[k] = in.x;
    sh.cnt[k] = in.y;
    sh.cs0[k] = gl(cs)[in.x];
    sh.from[k] = gl(rsrc)[r];
  };
  // Byte x of staged row f (every row has bytes).  A payload byte: returns true with where in `values`
  // it is and how many bytes follow it there (to the end of the row's run, or of its value in a row
  // that skips one); a generated word: returns false with the word.
  auto locate = [&](int f, int64_t x, uint64_t* word, int64_t* at, int64_t* left) {
    const int64_t cnt = sh.cnt[f], p0 = sh.first[f];
    if (x < P) {                      // the one-field row's bitmap word and slot
      *word = x == 0 ? (cnt < 0 ? 1 : 0)
                     : (cnt < 0 ? 0 : (16ull << 32) | static_cast<uint64_t>(sh.oo[f + 1] - sh.oo[f] - 16));
      return false;
    }
    int64_t y = x - P, e = p0;
    const int64_t from = sh.from[f];
    if (!a.wrap) {
      if (y == 0) {
        *word = static_cast<uint64_t>(cnt);
        return false;
      }
      const int64_t bm = ((cnt + 63) >> 6) << 3, H = 8 + bm + 8 * cnt;
      if (y < 8 + bm) {               // null bits of elements [p0 + i0, p0 + i0 + 64), those below cnt
        const int64_t i0 = (y - 8) << 3, e0 = p0 + i0;
        const int64_t t = e0 >> 6;
        const int sft = static_cast<int>(e0 & 63);
        uint64_t kept = gl(km)[t] >> sft;
        if (sft && t + 1 < nt) kept |= gl(km)[t + 1] << (64 - sft);
        const int64_t c = cnt - i0;
        *word = ~kept & (c < 64 ? (1ull << c) - 1 : ~0ull);
        return false;
      }
      if (y < H) {
        const int64_t el = p0 + ((y - 8 - bm) >> 3);
        *word = 0;
        if ((gl(km)[el >> 6] >> (el & 63)) & 1) {
          const int64_t c0 = gl(cs)[el];
          *word = (static_cast<uint64_t>(H + (c0 - sh.cs0[f])) << 32) |
                  static_cast<uint64_t>(gl(cs)[el + 1] - c0);
        }
        return false;
      }
      y -= H;
      if (from >= 0) {                // the payload is one run of `values`
        *left = sh.oo[f + 1] - sh.oo[f] - x;
        *at = from + y;
        return true;
      }
      // the last element of the row whose clean offset is <= the byte's has bytes there
      const int64_t p = sh.cs0[f] + y;
      int64_t hi = p0 + cnt - 1;
      while (e < hi) {
        const int64_t mid = (e + hi + 1) >> 1;
        if (gl(cs)[mid] <= p) e = mid;
        else hi = mid - 1;
      }
      y = p - gl(cs)[e];
      *left = gl(cs)[e + 1] - p;
      *at = gl(src)[e] + y;
    } else {                          // a wrapped value: the row's payload
      *left = sh.oo[f + 1] - sh.oo[f] - x;
      *at = from + y;
    }
    return true;
  };
  write_spans<kImpRows>(sh, a.nrows, a.out_offsets, a.cap, stage,
                        [&](int64_t, int kn, int64_t a0, int64_t b0) {
                          store_located<int64_t>(a.out, a0, b0, sh.oo, kn, locate,
                                                 [&](int64_t at) { return a.values + at; });
                        });
}

}  // namespace

int launch_implode(const ImplodeArgs& a, hipStream_t stream) {
  const int64_t n = a.nrows, E = a.num_elements;
  if (n >= (int64_t{1} << 38) || E >= (int64_t{1} << 38))     // blocks_of() in 31 bits
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  if (n == 0) return check_hip(hipMemsetAsync(a.out_offsets, 0, 8, stream), "memset");
  const int64_t nt = (E + 63) / 64;
  // even: info is 16-byte aligned
  const int64_t sw = (std::max(scan_workspace(n), scan_workspace(E)) + 1) & ~int64_t{1};
  int64_t* ws = nullptr;              // [info x 2 n][scan scratch][clean offsets x E + 1][source starts x E][kept x nt][failed x nt][failed counts x nt + 1][tile ranks x nt + 1][row sources x n]
  int st = dev_alloc((2 * n + sw + (E + 1) + E + 2 * nt + 2 * (nt + 1) + n) * 8, stream,
                     reinterpret_cast<void**>(&ws));
  if (st) return st;
  v2l* info = reinterpret_cast<v2l*>(ws);
  int64_t* sws = ws + 2 * n;
  int64_t* cs = sws + sw;
  int64_t* src = cs + E + 1;
  uint64_t* km = reinterpret_cast<uint64_t*>(src + E);
  uint64_t* fm = km + nt;
  int64_t* tf = reinterpret_cast<int64_t*>(fm + nt);
  int64_t* tr = a.elem_validity ? tf + nt + 1 : nullptr;
  int64_t* rsrc = tf + 2 * (nt + 1);
  if (tr && nt > 0) {
    hipLaunchKernelGGL(tile_rank, dim3(blocks_of(nt)), dim3(kTakeThreads), 0, stream,
                       a.elem_validity, E, nt, tr);
    device_scan(tr, nt, tr + nt, sws, stream);
  }
  if (nt > 0)
    hipLaunchKernelGGL(implode_elems, dim3(static_cast<unsigned>((nt + kTileWaves - 1) / kTileWaves)),
                       dim3(kTakeThreads), 0, stream, a, tr, cs, src, km, fm, tf);
  device_scan(cs, E, cs + E, sws, stream);
  device_scan(tf, nt, tf + nt, sws, stream);
  hipLaunchKernelGGL(implode_rows, dim3(blocks_of(n)), dim3(kTakeThreads), 0, stream, a, tr, cs, src, km,
                     fm, tf, info, rsrc);
  device_scan(a.out_offsets, n, a.out_offsets + n, sws, stream);
  if (a.out && a.cap >= 8)
    hipLaunchKernelGGL(implode_write, dim3(copy_grid(a.cap)), dim3(kTakeThreads), 0, stream, a, cs, src,
                       km, info, rsrc);
  st = check_hip(hipGetLastError(), "implode launch");
  dev_free(ws, stream);
  return st;
}

}  // namespace fury
