// take_dev.h -- the byte-balanced, output-parallel write pass of every operator that makes a row
// batch, once: write_spans (the span loop, the row search, the staging rounds) and store_split (the
// 16-byte alignment of a round's stores); the design is described in take.hip.  Its instances:
//   copy_rows       a row is a run of source bytes: take.hip, partition.hip's concat, extract.hip,
//                   explode.hip and map.hip's split each give it their lookup of an output row's
//                   source start
//   select_write, zip_write              every 8-byte word is made on its own (store_words)
//   implode_write, map_join_write        a word is generated or copied from a run (store_located)
// take.hip and partition.hip include it directly, the other files through select_dev.h or extract_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace fury {

constexpr int kTakeThreads = 256;
constexpr int kTakeInFlight = 4;                  // 16-byte chunks per lane loaded before the first store
constexpr int64_t kTakeStep = static_cast<int64_t>(kTakeThreads) * 16 * kTakeInFlight;   // 16 KB
// Output bytes a workgroup owns, a multiple of kTakeStep.  Measured: 32 / 64 KB spans
// gain 12-16 % on 108-byte rows in row order, nothing on a permutation, and 64 KB costs the
// fixed-size copy 23 %.
constexpr int64_t kTakeSpan = kTakeStep;
constexpr int kTakeRows = 1024;                   // rows staged in LDS per round (16 KB)
constexpr int64_t kTakeMaxGrid = 1 << 20;         // copy workgroups per launch (grid-stride beyond)

using v2q = __attribute__((ext_vector_type(2))) uint64_t;

__device__ __forceinline__ uint64_t ld8(const uint8_t* p) {
  return __builtin_nontemporal_load(gl(reinterpret_cast<const uint64_t*>(p)));
}
__device__ __forceinline__ v2q ld16(const uint8_t* p) {
  return __builtin_nontemporal_load(gl(reinterpret_cast<const v2q*>(p)));
}
__device__ __forceinline__ void st8(uint8_t* p, uint64_t v) {
  __builtin_nontemporal_store(v, gl(reinterpret_cast<uint64_t*>(p)));
}
__device__ __forceinline__ void st16(uint8_t* p, v2q v) {
  __builtin_nontemporal_store(v, gl(reinterpret_cast<v2q*>(p)));
}

// Size of source row i, *ok = false (size 0) when the row may not be read.
__device__ __forceinline__ int64_t row_extent(const int64_t* ro, int64_t nrows, int64_t total,
                                              int64_t i, bool* ok) {
  *ok = false;
  if (i < 0 || i >= nrows) return 0;
  const int64_t b = gl(ro)[i], e = gl(ro)[i + 1];
  if (e < b || !span_ok(b, e - b, total) || ((b | e) & 7)) return 0;
  *ok = true;
  return e - b;
}

// The largest j in [lo, lo + len) with oo[j] <= key, for a non-decreasing oo with oo[lo] <= key:
// 64-ary search, one probe per lane.  Every lane of the wave must call it with the same arguments.
__device__ __forceinline__ int64_t last_le(const int64_t* oo, int64_t lo, int64_t len, int64_t key,
                                           int lane) {
  while (len > 1) {
    const int64_t step = (len + 63) >> 6;
    const int64_t at = lane * step;
    const bool le = at < len && gl(oo)[lo + at] <= key;
    const int c = max(__popcll(__ballot(le)) - 1, 0);
    const int64_t nlo = lo + c * step;
    len = min(step, lo + len - nlo);
    lo = nlo;
  }
  return lo;
}

// The staged row of a round that holds output byte d: the largest f in [0, kn) with soo[f] <= d, for
// the kn staged starts soo (LDS) with soo[0] <= d.  A row without bytes is never the answer.
__device__ __forceinline__ int staged_row(const int64_t* soo, int kn, int64_t d) {
  int lo = 0, hi = kn - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (soo[mid] <= d) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Stores output bytes [a, b) (multiples of 8; every thread of the workgroup calls it): chunks(A, B)
// stores the 16-byte aligned chunks [A, B), and the 8-byte word that an `out` at 8 mod 16 leaves at
// either end is word(d), stored by thread 0 and thread 64.  Less than one aligned chunk: A = B.
template <class Word, class Chunks>
__device__ __forceinline__ void store_split(uint8_t* out, int64_t a, int64_t b, Word word,
                                            Chunks chunks) {
  const int tid = threadIdx.x;
  const uintptr_t ob = reinterpret_cast<uintptr_t>(out);
  int64_t A = a + static_cast<int64_t>((16 - ((ob + a) & 15)) & 15);
  int64_t B = b - static_cast<int64_t>((ob + b) & 15);
  if (A > B) A = B = b;
  if (tid == 0 && a < A) st8(out + a, word(a));
  if (tid == 64 && B < b) st8(out + B, word(B));
  chunks(A, B);
}

// store_split with the plain chunk loop: a lane makes both words of its chunk with word(d).
template <class Word>
__device__ __forceinline__ void store_words(uint8_t* out, int64_t a, int64_t b, Word word) {
  store_split(out, a, b, word, [&](int64_t A, int64_t B) {
    for (int64_t d = A + 16 * threadIdx.x; d < B; d += 16 * kTakeThreads) {
      v2q v;
      v.x = word(d);
      v.y = word(d + 8);
      st16(out + d, v);
    }
  });
}

// store_split for rows whose words are GENERATED or COPIED from a run of source bytes.
// locate(f, x, &w, &at, &left), byte x of staged row f: true with where the source byte is (an At:
// addr(at) is its address) and how many bytes of its run follow there, or false with the generated
// word w.  A chunk inside one run is one 16-byte load when the source aligns, else two 8-byte ones.
template <class At, class Locate, class Addr>
__device__ __forceinline__ void store_located(uint8_t* out, int64_t a, int64_t b, const int64_t* soo,
                                              int kn, Locate locate, Addr addr) {
  auto word = [&](int64_t d) -> uint64_t {
    const int f = staged_row(soo, kn, d);
    uint64_t w;
    At at;
    int64_t left;
    if (!locate(f, d - soo[f], &w, &at, &left)) return w;
    return ld8(addr(at));
  };
  store_split(out, a, b, word, [&](int64_t A, int64_t B) {
    for (int64_t d = A + 16 * threadIdx.x; d < B; d += 16 * kTakeThreads) {
      v2q v;
      const int f = staged_row(soo, kn, d);
      uint64_t w;
      At at;
      int64_t left;
      if (locate(f, d - soo[f], &w, &at, &left)) {
        const uint8_t* p = addr(at);
        if (left >= 16) {
          if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            v = ld16(p);
          } else {
            v.x = ld8(p);
            v.y = ld8(p + 8);
          }
        } else {                      // the run ends with this word
          v.x = ld8(p);
          v.y = word(d + 8);
        }
      } else {
        v.x = w;
        v.y = word(d + 8);
      }
      st16(out + d, v);
    }
  });
}

// The output-parallel, byte-balanced write pass of a kernel of kTakeThreads threads: n output rows at
// oo[0..n] (oo[n] = bytes needed), written below min(oo[n], cap & ~7).  A workgroup owns kTakeSpan
// output bytes (grid-stride over spans), finds the rows [j0, jl] of its span by the 64-ary search,
// and stages them in rounds of kRows: sh.oo[0..kn] receives the kn rows' output starts and the end of
// the last one, stage(r, k) puts whatever else the caller keeps of row r into slot k of sh.  Between
// the round's two barriers round(r0, kn, a, b) stores the round's bytes [a, b) -- those of rows
// [r0, r0 + kn) inside the span -- through store_split or one of its two forms above.
template <int kRows, class Shared, class Stage, class Round>
__device__ __forceinline__ void write_spans(Shared& sh, int64_t n, const int64_t* __restrict__ oo,
                                            int64_t cap, Stage stage, Round round) {
  static_assert(sizeof(sh.oo) == (kRows + 1) * sizeof(int64_t), "sh.oo holds kRows starts and an end");
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t lim = min(gl(oo)[n], cap & ~int64_t{7});
  for (int64_t S = static_cast<int64_t>(blockIdx.x) * kTakeSpan; S < lim;
       S += static_cast<int64_t>(gridDim.x) * kTakeSpan) {
    const int64_t E = min(S + kTakeSpan, lim);
    // rows [j0, jl]: the row that holds byte S ... the last row that starts before E
    const int64_t j0 = last_le(oo, 0, n, S, lane);
    int64_t jl;
    {
      const bool lt = j0 + lane < n && gl(oo)[j0 + lane] < E;
      const int c = max(__popcll(__ballot(lt)) - 1, 0);
      jl = c < 63 ? j0 + c : last_le(oo, j0 + 63, n - (j0 + 63), E - 1, lane);
    }
    for (int64_t r0 = j0; r0 <= jl; r0 += kRows) {
      const int kn = static_cast<int>(min<int64_t>(kRows, jl + 1 - r0));
      for (int k = tid; k <= kn; k += kTakeThreads) {
        sh.oo[k] = gl(oo)[r0 + k];
        if (k < kn) stage(r0 + k, k);
      }
      lds_barrier();
      round(r0, kn, max(S, sh.oo[0]), min(E, sh.oo[kn]));
      lds_barrier();                  // the next round (or span) overwrites the staged rows
    }
  }
}

struct TakeShared {
  int64_t oo[kTakeRows + 1];          // output start of the staged rows, and the end of the last one
  int64_t src[kTakeRows];             // source start (0-byte rows: unused)
};

// The body of a copy kernel of kTakeThreads threads: n output rows at oo[0..n] (oo[n] = bytes
// needed); output row j = the oo[j + 1] - oo[j] bytes of `rows` at src_of(j).  src_of is asked only
// for rows that have bytes.  write_spans with kTakeInFlight chunks per lane loaded before the first
// store.
template <class SrcOf>
__device__ __forceinline__ void copy_rows(const uint8_t* __restrict__ rows, SrcOf src_of, int64_t n,
                                          uint8_t* __restrict__ out,
                                          const int64_t* __restrict__ oo, int64_t cap) {
  __shared__ TakeShared sh;
  write_spans<kTakeRows>(
      sh, n, oo, cap,
      [&](int64_t r, int k) { sh.src[k] = gl(oo)[r + 1] > gl(oo)[r] ? src_of(r) : 0; },
      [&](int64_t, int kn, int64_t a, int64_t b) {
        const int tid = threadIdx.x;
        auto word_at = [&](int64_t d) {
          const int f = staged_row(sh.oo, kn, d);
          return ld8(rows + sh.src[f] + (d - sh.oo[f]));
        };
        store_split(out, a, b, word_at, [&](int64_t A, int64_t B) {
          for (int64_t d0 = A; d0 < B; d0 += kTakeStep) {
            v2q v[kTakeInFlight];
#pragma unroll
            for (int u = 0; u < kTakeInFlight; u++) {
              const int64_t d = d0 + 16 * (tid + u * kTakeThreads);
              v[u] = v2q{0, 0};
              if (d < B) {
                const int f = staged_row(sh.oo, kn, d);
                const uint8_t* p = rows + sh.src[f] + (d - sh.oo[f]);
                if (sh.oo[f + 1] - d >= 16) {
                  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                    v[u] = ld16(p);
                  } else {
                    v[u].x = ld8(p);
                    v[u].y = ld8(p + 8);
                  }
                } else {              // the chunk's second word starts the next row that has bytes
                  int f2 = f + 1;
                  while (sh.oo[f2 + 1] <= d + 8) f2++;
                  v[u].x = ld8(p);
                  v[u].y = ld8(rows + sh.src[f2]);
                }
              }
            }
#pragma unroll
            for (int u = 0; u < kTakeInFlight; u++) {
              const int64_t d = d0 + 16 * (tid + u * kTakeThreads);
              if (d < B) st16(out + d, v[u]);
            }
          }
        });
      });
}

namespace {

// Offsets of fixed-size rows: oo[g] = min(g, count) * fixed_size for g in [0, n] (count NULL: n).
__global__ __launch_bounds__(kTakeThreads) void fixed_offsets(int64_t* __restrict__ oo, int64_t n,
                                                              const int64_t* __restrict__ count,
                                                              int64_t fixed_size) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kTakeThreads + threadIdx.x;
  if (g > n) return;
  const int64_t cnt = count ? *gl(count) : n;
  gl(oo)[g] = (g < cnt ? g : cnt) * fixed_size;
}

}  // namespace

inline unsigned blocks_of(int64_t n) {
  return static_cast<unsigned>((n + kTakeThreads - 1) / kTakeThreads);
}

inline unsigned copy_grid(int64_t bytes) {
  return static_cast<unsigned>(std::min<int64_t>((bytes + kTakeSpan - 1) / kTakeSpan, kTakeMaxGrid));
}

}  // namespace fury
