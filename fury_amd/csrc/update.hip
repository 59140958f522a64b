// update.hip -- in-place update of selected fixed-width top-level fields of a row batch
// (fury_row_update).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of BinaryRow's setters.  setX(ordinal, v) = setNotNullAt(ordinal) + putX(getOffset(ordinal), v)
// writes the value's own 1 / 2 / 4 / 8 bytes at the start of the 8-byte slot and clears the field's
// bitmap bit (FMT/row/binary/UnsafeTrait.java:203-266); setNullAt(ordinal) sets the bit and zeroes
// the whole slot (FMT/row/binary/BinaryRow.java:130-150).  Nothing else of the row changes.
//
// MI355X design: project.hip run backwards, on its records (ProjArgs / ProjCol / ProjPiece) and its
// piece list (finish_plan).  Lane = row with one 8-byte store per lane at a row stride is never
// issued:
//   tile       a 256-thread workgroup owns 64 / 128 / 256 rows (tiles start at multiples of 64 rows,
//              so validity, BOOL and mask words are not shared between workgroups).  Row start, write
//              bounds and the row's mask bit go to LDS first (rowbase < 0: the row is not written).
//   staging    only what must be merged is read: the bitmap words that hold a selected bit, and the
//              slot words of fields narrower than 8 bytes (their bytes [w, 8) are kept).  Consecutive
//              lanes load consecutive words of a row's pieces into an odd-stride LDS image, up to 8
//              loads per lane in flight.  Slots of 8-byte fields are not read.
//   merge      in LDS, lane = row, one (image word, 64-row chunk) unit per wave at a time.  A slot
//              word belongs to one field; a BITMAP word may hold the bits of several selected fields,
//              so its unit loops over all of them: no two waves ever touch the same LDS word and no
//              LDS atomics are needed.  values[r] loads are coalesced, validity / BOOL words are one
//              wave-uniform 64-bit read per chunk.
//   write out  staging reversed: consecutive lanes store consecutive 8-byte words of a row's pieces,
//              then the next row's.  Pieces hold only bitmap words with a selected bit and selected
//              slots, so no unselected slot is rewritten; a bitmap word carries its other bits from
//              the staged old value.
// Bounds: "Decode bounds" of kernels.h applied to stores, see launch_update there.
#include <hip/hip_runtime.h>

#include "var_dev.h"

namespace fury {

namespace {

constexpr int kUpdThreads = kThreads;          // 256
constexpr int kUpdInFlight = 8;                // staged loads per lane before the first use
constexpr uint32_t kNoLoad = 0x80000000u;      // woff flag: the word is overwritten whole

using CUpdCol = __attribute__((address_space(4))) const ProjCol;
__device__ __forceinline__ CUpdCol& uc(const ProjArgs& a, int k) {
  return ((CUpdCol*)(a.col))[k];
}

struct UpdShared {
  int64_t rowbase[kUpdThreads];           // absolute row start; -1: the row is not written
  uint32_t woff[2 * kMaxProjCols + 2];    // byte offset in the row of image word w (| kNoLoad)
};

// Plain accesses, not non-temporal ones: a staged bitmap word's line then waits in L2 for the store
// that rewrites it, and the stores of one row's words meet there.  Measured: non-temporal
// loads and stores cost 1.6-2.3x at k <= 3 fields and are within 6 % at 32.
__device__ __forceinline__ uint64_t load_word(const uint8_t* p) {
  return *gl(reinterpret_cast<const uint64_t*>(p));
}

__device__ __forceinline__ void store_word(uint8_t* p, uint64_t v) {
  *gl(reinterpret_cast<uint64_t*>(p)) = v;
}

// Bits [rb, rb + 64) of a bitmap read as 32-bit words (rb a multiple of 64, rb < nrows; the bitmap
// is readable to a multiple of 4 bytes of its nrows bits).
__device__ __forceinline__ uint64_t bits64(const uint8_t* bits, int64_t rb, int64_t nrows) {
  const auto* w = gl(reinterpret_cast<const uint32_t*>(bits)) + (rb >> 5);
  uint64_t v = w[0];
  if (rb + 32 < nrows) v |= static_cast<uint64_t>(w[1]) << 32;
  return v;
}

__global__ __launch_bounds__(kUpdThreads) void update_rows(ProjArgs a, uint8_t* __restrict__ rows,
                                                           const int64_t* __restrict__ offs,
                                                           const uint8_t* __restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) uint64_t upd_img[];
  __shared__ UpdShared sh;
  uint64_t* img = upd_img;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * a.tile_rows;
  const int nr = static_cast<int>(min<int64_t>(a.tile_rows, a.nrows - r0));
  const int64_t total = offs ? gl(offs)[a.nrows] : a.nrows * a.fixed_size;

  // row starts: mask bit, then the write bounds
  {
    int64_t base = -1;
    if (tid < nr) {
      const int64_t r = r0 + tid;
      const bool sel = !mask || ((gl(reinterpret_cast<const uint32_t*>(mask))[r >> 5] >> (r & 31)) & 1);
      if (sel) {
        base = offs ? gl(offs)[r] : r * a.fixed_size;
        bool ok = row_ok(base, a.fixed_size, total);
        if (ok && offs) ok = gl(offs)[r + 1] >= base + a.fixed_size;   // the row's own extent
        if (!ok) {
          raise_oob(a.err, r);
          base = -1;
        }
      }
    }
    sh.rowbase[tid] = base;
  }
  if (tid < a.nwords) {               // word tid of the image <- its offset in the row, loaded or not
    int at = 0;
    uint32_t off = 0;
    for (int p = 0; p < a.npieces; p++) {
      int32_t po, pw;
      if (a.ptab) {
        po = gl(a.ptab)[p].off;
        pw = gl(a.ptab)[p].words;
      } else {
        po = a.piece[p].off;
        pw = a.piece[p].words;
      }
      if (tid >= at && tid < at + pw) off = static_cast<uint32_t>(po + 8 * (tid - at));
      at += pw;
    }
    for (int k = 0; k < a.ncols; k++) {
      CUpdCol& c = uc(a, k);
      if ((c.img >> 16) == tid && c.width == 8) off |= kNoLoad;
    }
    sh.woff[tid] = off;
  }
  lds_barrier();

  // staging: the old words that are merged
  const uint32_t W = static_cast<uint32_t>(a.nwords), S = static_cast<uint32_t>(a.stride);
  const uint32_t items = static_cast<uint32_t>(nr) * W;
  for (uint32_t i0 = 0; i0 < items; i0 += kUpdThreads * kUpdInFlight) {
    uint64_t v[kUpdInFlight];
    uint32_t at[kUpdInFlight];
#pragma unroll
    for (int u = 0; u < kUpdInFlight; u++) {
      const uint32_t i = i0 + u * kUpdThreads + tid;
      v[u] = 0;
      at[u] = ~0u;
      if (i < items) {
        const uint32_t row = __umulhi(i, a.magic);     // i / W (exact: i < 2^16, W <= 2^8)
        const uint32_t w = i - row * W;
        const uint32_t wo = sh.woff[w];
        const int64_t base = sh.rowbase[row];
        if (!(wo & kNoLoad)) {
          at[u] = row * S + w;
          if (base >= 0) v[u] = load_word(rows + base + wo);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kUpdInFlight; u++)
      if (at[u] != ~0u) img[at[u]] = v[u];
  }
  lds_barrier();

  // merge: image words [0, nbw) are bitmap words (they sort first), word nbw + k' the slot of one
  // field; unit j >= nbw handles column j - nbw and finds its slot word in c.img
  const int nbw = a.nwords - a.ncols;
  const int nch = (nr + 63) >> 6;
  for (int u = wave; u < a.nwords * nch; u += kUpdThreads / 64) {
    const int j = u / nch, ch = u - j * nch;
    const int t = ch * 64 + lane;
    const int64_t rb = r0 + ch * 64;
    const bool live = t < nr && sh.rowbase[t] >= 0;
    uint64_t* row = img + static_cast<uint32_t>(t) * S;
    if (j < nbw) {
      uint64_t w = live ? row[j] : 0;
      for (int k = 0; k < a.ncols; k++) {
        CUpdCol& c = uc(a, k);
        if ((c.img & 0xffff) != j) continue;
        const uint64_t vb = c.validity ? bits64(c.validity, rb, a.nrows) : ~0ull;
        const uint64_t bit = 1ull << (c.slot & 63);
        w = ((vb >> lane) & 1) ? (w & ~bit) : (w | bit);
      }
      if (live) row[j] = w;
    } else {
      CUpdCol& c = uc(a, j - nbw);
      const int si = c.img >> 16;
      const uint64_t vb = c.validity ? bits64(c.validity, rb, a.nrows) : ~0ull;
      const bool valid = (vb >> lane) & 1;
      const int64_t r = rb + lane;
      const uint8_t* src = c.values;
      uint64_t v = 0, keep = 0;
      if (c.width == 0) {                              // BOOL: one byte, 0 or 1
        v = (bits64(src, rb, a.nrows) >> lane) & 1;
        keep = ~0xffull;
      } else if (t < nr) {
        switch (c.width) {
          case 8: v = *gl(reinterpret_cast<const uint64_t*>(src) + r); break;
          case 4: v = *gl(reinterpret_cast<const uint32_t*>(src) + r); keep = ~0xffffffffull; break;
          case 2: v = *gl(reinterpret_cast<const uint16_t*>(src) + r); keep = ~0xffffull; break;
          default: v = gl(src)[r]; keep = ~0xffull; break;
        }
      }
      if (live) row[si] = valid ? ((row[si] & keep) | v) : 0;   // width 8: keep = 0
    }
  }
  lds_barrier();

  // write out: consecutive lanes on consecutive words of a row's pieces
  for (uint32_t i = tid; i < items; i += kUpdThreads) {
    const uint32_t row = __umulhi(i, a.magic);
    const uint32_t w = i - row * W;
    const int64_t base = sh.rowbase[row];
    if (base >= 0) store_word(rows + base + (sh.woff[w] & ~kNoLoad), img[row * S + w]);
  }
}

template <class K>
int allow_lds(K kern, size_t bytes) {
  if (bytes <= 48 * 1024) return FURY_OK;
  return check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(bytes)),
                   "update: LDS size");
}

}  // namespace

int launch_update(const ProjArgs& in, uint8_t* rows, const int64_t* offs, const uint8_t* mask,
                  hipStream_t stream) {
  if (in.nrows == 0) return FURY_OK;
  ProjArgs a = in;
  a.tile_rows = 0;
  DeviceTable dt;
  int st = finish_plan(&a, stream, &dt);
  if (st) return st;
  const int64_t nt = (a.nrows + a.tile_rows - 1) / a.tile_rows;
  if (nt > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  const size_t lds = static_cast<size_t>(a.tile_rows) * a.stride * 8;
  const dim3 grid(static_cast<unsigned>(nt)), block(kUpdThreads);
  st = allow_lds(update_rows, lds);
  if (!st) hipLaunchKernelGGL(update_rows, grid, block, lds, stream, a, rows, offs, mask);
  if (!st) st = check_hip(hipGetLastError(), "update_rows launch");
  return st;
}

}  // namespace fury
