// select_dev.h -- what select.hip (fury_row_select) and zip.hip (fury_row_zip) share: the word-level
// pieces of a BinaryRowWriter's output, the selection table staged in LDS, the check of a source row,
// and the host steps of their launchers that depend only on (nrows, out_fixed_size, nvar,
// out_bitmap_bytes) and the table.  SelectArgs and ZipArgs name those members alike.
#pragma once

#include "take_dev.h"

namespace fury {

__device__ __forceinline__ uint64_t word(const uint8_t* p) {
  return *gl(reinterpret_cast<const uint64_t*>(p));
}

// A fixed-width slot as write(ordinal, <primitive>) leaves it: putInt64(offset, 0), then the value's
// own bytes; putBoolean stores 1 or 0.
__device__ __forceinline__ uint64_t fixed_slot(uint64_t s, int32_t width) {
  if (width == kSelBool) return (s & 0xff) ? 1 : 0;
  return width >= 8 ? s : s & ((1ull << (8 * width)) - 1);
}

// Bitmap word q of a row whose n fields are all null.
__device__ __forceinline__ uint64_t all_null(int q, int n) {
  const int left = n - 64 * q;
  return left >= 64 ? ~0ull : (1ull << left) - 1;
}

using CI32 = __attribute__((address_space(4))) const int32_t;
template <class Args>
__device__ __forceinline__ CI32* table_of(const Args& a) {
  return a.tab ? (CI32*)(a.tab) : (CI32*)(a.tabi);
}

// The table for per-lane lookups: its nw words staged in `lds` when that has room for them
// (lds_words).  Every thread of the workgroup calls stage_table.
struct StagedTable {
  const int32_t* lds;
  CI32* mem;
  __device__ __forceinline__ int32_t operator[](int i) const { return lds ? lds[i] : mem[i]; }
};
__device__ __forceinline__ StagedTable stage_table(CI32* mem, int nw, int32_t* lds, int lds_words) {
  StagedTable t{nullptr, mem};
  if (nw <= lds_words) {
    for (int i = threadIdx.x; i < nw; i += kTakeThreads) lds[i] = mem[i];
    lds_barrier();
    t.lds = lds;
  }
  return t;
}

// Row r of source z, a SelectArgs or a ZipSource (row_offsets NULL: rows of fixed_size bytes): its
// start, and whether its header may be read ("Decode bounds": 8-byte aligned, [B, B + fixed_size)
// inside [0, total), the row's own extent no shorter than fixed_size).
template <class Source>
__device__ __forceinline__ bool source_row(const Source& z, int64_t r, int64_t total, int64_t* B) {
  if (!z.row_offsets) {
    *B = r * z.fixed_size;
    return true;
  }
  const int64_t b = gl(z.row_offsets)[r];
  *B = b;
  return !(b & 7) && span_ok(b, z.fixed_size, total) && gl(z.row_offsets)[r + 1] - b >= z.fixed_size;
}

// The launchers' first step: the batch-too-large test, then the table into the argument block, or
// uploaded (dt owns it) when it outgrows tabi.
template <class Args>
inline int place_table(Args* a, const int32_t* table, int nwords, hipStream_t stream, DeviceTable* dt) {
  // blocks_of() in 31 bits, and the fixed kernel's multiply-high exact
  if (a->nrows >= (int64_t{1} << 38) || a->nrows > (int64_t{1} << 52) / a->out_fixed_size)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  if (nwords <= static_cast<int>(sizeof(a->tabi) / sizeof(int32_t))) {
    std::copy(table, table + nwords, a->tabi);
    return FURY_OK;
  }
  const int st = upload_table(table, static_cast<size_t>(nwords) * 4, stream, dt);
  if (!st) a->tab = static_cast<const int32_t*>(dt->dev);
  return st;
}

// The workspace of the three-pass form: [scan scratch][bitmap words x n nbw][value starts x n nvar
// (int32)].  dev_free(ws) releases it.
struct SelectWorkspace {
  int64_t* ws = nullptr;
  uint64_t* wbm;
  int32_t* wW;
};
template <class Args>
inline int alloc_workspace(const Args& a, hipStream_t stream, SelectWorkspace* w) {
  const int64_t n = a.nrows, nbw = a.out_bitmap_bytes / 8, sw = scan_workspace(n);
  const int st = dev_alloc((sw + n * nbw + (n * a.nvar + 1) / 2) * 8, stream,
                           reinterpret_cast<void**>(&w->ws));
  if (st) return st;
  w->wbm = reinterpret_cast<uint64_t*>(w->ws + sw);
  w->wW = reinterpret_cast<int32_t*>(w->ws + sw + n * nbw);
  return FURY_OK;
}

}  // namespace fury
