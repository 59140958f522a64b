// select_dev.h -- the word-level pieces of a BinaryRowWriter's output that select.hip
// (fury_row_select) and zip.hip (fury_row_zip) share.
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

}  // namespace fury
