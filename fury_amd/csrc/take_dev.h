// take_dev.h -- the byte-balanced, output-parallel row copy shared by take.hip (fury_row_take /
// fury_row_filter), extract.hip (fury_row_extract) and explode.hip (fury_row_explode).  Each
// includes it (the last two through extract_dev.h) and instantiates copy_rows with its own lookup
// of an output row's source start; the design is described in take.hip.
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

struct TakeShared {
  int64_t oo[kTakeRows + 1];          // output start of the staged rows, and the end of the last one
  int64_t src[kTakeRows];             // source start (0-byte rows: unused)
};

// The body of a copy kernel of kTakeThreads threads: n output rows at oo[0..n] (oo[n] = bytes
// needed); output row j = the oo[j + 1] - oo[j] bytes of `rows` at src_of(j).  src_of is asked only
// for rows that have bytes.
template <class SrcOf>
__device__ __forceinline__ void copy_rows(const uint8_t* __restrict__ rows, SrcOf src_of, int64_t n,
                                          uint8_t* __restrict__ out,
                                          const int64_t* __restrict__ oo, int64_t cap) {
  __shared__ TakeShared sh;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t lim = min(gl(oo)[n], cap & ~int64_t{7});
  const uintptr_t ob = reinterpret_cast<uintptr_t>(out);
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
    for (int64_t r0 = j0; r0 <= jl; r0 += kTakeRows) {
      const int kn = static_cast<int>(min<int64_t>(kTakeRows, jl + 1 - r0));
      for (int k = tid; k <= kn; k += kTakeThreads) {
        const int64_t o = gl(oo)[r0 + k];
        sh.oo[k] = o;
        if (k < kn) sh.src[k] = gl(oo)[r0 + k + 1] > o ? src_of(r0 + k) : 0;
      }
      lds_barrier();
      auto find = [&](int64_t d) {    // the staged row that holds output byte d (its size is > 0)
        int lo = 0, hi = kn - 1;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (sh.oo[mid] <= d) lo = mid;
          else hi = mid - 1;
        }
        return lo;
      };
      auto word_at = [&](int64_t d) {
        const int f = find(d);
        return ld8(rows + sh.src[f] + (d - sh.oo[f]));
      };
      // this round's bytes [a, b): 16-byte aligned chunks [A, B), one 8-byte word at either end
      const int64_t a = max(S, sh.oo[0]), b = min(E, sh.oo[kn]);
      int64_t A = a + static_cast<int64_t>((16 - ((ob + a) & 15)) & 15);
      int64_t B = b - static_cast<int64_t>((ob + b) & 15);
      if (A > B) A = B = b;
      if (tid == 0 && a < A) st8(out + a, word_at(a));
      if (tid == 64 && B < b) st8(out + B, word_at(B));
      for (int64_t d0 = A; d0 < B; d0 += kTakeStep) {
        v2q v[kTakeInFlight];
#pragma unroll
        for (int u = 0; u < kTakeInFlight; u++) {
          const int64_t d = d0 + 16 * (tid + u * kTakeThreads);
          v[u] = v2q{0, 0};
          if (d < B) {
            const int f = find(d);
            const uint8_t* p = rows + sh.src[f] + (d - sh.oo[f]);
            if (sh.oo[f + 1] - d >= 16) {
              if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                v[u] = ld16(p);
              } else {
                v[u].x = ld8(p);
                v[u].y = ld8(p + 8);
              }
            } else {                  // the chunk's second word starts the next row that has bytes
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
      lds_barrier();                  // the next round (or span) overwrites the staged rows
    }
  }
}

inline unsigned blocks_of(int64_t n) {
  return static_cast<unsigned>((n + kTakeThreads - 1) / kTakeThreads);
}

inline unsigned copy_grid(int64_t bytes) {
  return static_cast<unsigned>(std::min<int64_t>((bytes + kTakeSpan - 1) / kTakeSpan, kTakeMaxGrid));
}

}  // namespace fury
