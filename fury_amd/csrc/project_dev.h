// project_dev.h -- the device helpers the kernels over a projected row header share (project.hip,
// hash.hip): the LDS image of the header words a selection needs, staged from the piece list
// (finish_plan), and the reads from it.  Design notes: project.hip.
#pragma once

#include "var_dev.h"

namespace fury {

namespace {

constexpr int kProjThreads = kThreads;         // 256: put_bits64 / block_excl_scan are sized by it
constexpr int kProjInFlight = 8;               // staged loads per lane before the first use
constexpr int kProjLong = 512;                 // payload bytes from which a whole wave copies a value
constexpr int kProjGroup = 8;                  // lanes per row for shorter values

using CProjCol = __attribute__((address_space(4))) const ProjCol;
__device__ __forceinline__ CProjCol& pc(const ProjArgs& a, int k) {
  return ((CProjCol*)(a.col))[k];
}

template <bool NT>
__device__ __forceinline__ uint64_t row_word(const uint8_t* p) {
  const auto* q = gl(reinterpret_cast<const uint64_t*>(p));
  if (NT) return __builtin_nontemporal_load(q);
  return *q;
}

struct ProjShared {
  int64_t rowbase[kProjThreads];     // absolute row start; -1: the row is outside the batch
  int32_t pos[kProjThreads + 1];     // tile-relative exclusive starts of one counted field; [T] total
  int32_t woff[2 * kMaxProjCols + 2];  // byte offset in the row of image word w
  int64_t tmp[kProjThreads / 64];
};

// Row starts + bounds, the word table, then the tile's header words into the LDS image.
template <bool NT>
__device__ __forceinline__ void stage_tile(const ProjArgs& a, const uint8_t* rows, const int64_t* offs,
                                           int64_t total, int64_t r0, int nr, ProjShared& sh,
                                           uint64_t* img) {
  const int tid = threadIdx.x;
  {
    int64_t base = -1;
    if (tid < nr) {
      const int64_t r = r0 + tid;
      base = offs ? gl(offs)[r] : r * a.fixed_size;
      if (!row_ok(base, a.fixed_size, total)) {
        raise_oob(a.err, r);
        base = -1;
      }
    }
    sh.rowbase[tid] = base;
  }
  if (tid < a.nwords) {               // word tid of the image <- its offset in the row
    int at = 0, off = 0;
    for (int p = 0; p < a.npieces; p++) {
      int32_t po, pw;
      if (a.ptab) {
        po = gl(a.ptab)[p].off;
        pw = gl(a.ptab)[p].words;
      } else {
        po = a.piece[p].off;
        pw = a.piece[p].words;
      }
      if (tid >= at && tid < at + pw) off = po + 8 * (tid - at);
      at += pw;
    }
    sh.woff[tid] = off;
  }
  lds_barrier();
  const uint32_t W = static_cast<uint32_t>(a.nwords), S = static_cast<uint32_t>(a.stride);
  const uint32_t items = static_cast<uint32_t>(nr) * W;
  for (uint32_t i0 = 0; i0 < items; i0 += kProjThreads * kProjInFlight) {
    uint64_t v[kProjInFlight];
    uint32_t at[kProjInFlight];
#pragma unroll
    for (int u = 0; u < kProjInFlight; u++) {
      const uint32_t i = i0 + u * kProjThreads + tid;
      v[u] = 0;
      at[u] = ~0u;
      if (i < items) {
        const uint32_t row = __umulhi(i, a.magic);     // i / W (exact: i < 2^16, W <= 2^8)
        const uint32_t w = i - row * W;
        at[u] = row * S + w;
        const int64_t base = sh.rowbase[row];
        if (base >= 0) v[u] = row_word<NT>(rows + base + sh.woff[w]);
      }
    }
#pragma unroll
    for (int u = 0; u < kProjInFlight; u++)
      if (at[u] != ~0u) img[at[u]] = v[u];
  }
  lds_barrier();
}

// Null bit and slot of column c for tile row t (base < 0: the row is outside the batch -> null).
__device__ __forceinline__ bool field_slot(CProjCol& c, const uint64_t* img, int stride, int t,
                                           int64_t base, uint64_t* slot) {
  *slot = 0;
  if (base < 0) return true;
  const uint64_t* row = img + static_cast<uint32_t>(t) * stride;
  const bool isnull = (row[c.img & 0xffff] >> (c.slot & 63)) & 1;
  if (!isnull) *slot = row[c.img >> 16];
  return isnull;
}

// 8 batch bytes at absolute offset s (any alignment), [s, s + 8) inside [0, total): two aligned
// words funnel-shifted when the second lies inside the batch too, else the unaligned word itself.
__device__ __forceinline__ uint64_t batch_word(const uint8_t* rows, int64_t s, int64_t total) {
  const int sh = static_cast<int>(s & 7) * 8;
  const int64_t al = s & ~int64_t(7);
  if (sh == 0 || al + 16 > total) return *gl(reinterpret_cast<const uint64_t*>(rows + s));
  const uint64_t lo = *gl(reinterpret_cast<const uint64_t*>(rows + al));
  const uint64_t hi = *gl(reinterpret_cast<const uint64_t*>(rows + al + 8));
  return (lo >> sh) | (hi << (64 - sh));
}

}  // namespace

}  // namespace fury
