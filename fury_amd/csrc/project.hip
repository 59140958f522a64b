// project.hip -- projected decode: selected top-level fields of a row batch -> columns
// (fury_row_project / fury_row_project_measure).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of BinaryRow's getters -- isNullAt(ordinal) reads one bitmap bit, getInt64 / getString / getDecimal
// / getArray(ordinal) one 8-byte slot and, for variable-length values, the bytes it points at
// (FMT/row/binary/BinaryRow.java, FMT/row/binary/UnsafeTrait.java:68-197, BinaryArray.pointTo
// FMT/row/binary/BinaryArray.java:69-78).  Fields that are not selected are never read, so the
// schema may hold any kinds; per selected field the outputs are fury_row_decode's.
//
// MI355X design.  Lane = row with one 8-byte load per lane at a row stride is the access shape that
// runs an order of magnitude below the memory rate, so the rows are never read that way:
//   piece list   the host merges the 8-byte words of the row header the selection needs (the bitmap
//                words holding the selected bits, the selected slots) into runs of <= 16 words
//                (<= 128 B); they travel in the argument block (ProjArgs.piece).
//   staging      a 256-thread workgroup owns a tile of 64 / 128 / 256 rows.  Consecutive lanes load
//                consecutive words of a row's pieces and go on with the next row, so a
//                wave-instruction reads whole <= 128-B segments of several rows; up to 8 loads per
//                lane are in flight before the first is used.  The words land in an LDS image with
//                an odd stride of 8-byte words per row.
//   transpose    lane = row reads its bit and slot from the image (conflict-free: odd stride), one
//                (field, 64-row chunk) unit per wave at a time: fixed-width values leave as
//                contiguous column stores, validity / BOOL as __ballot words stored as 32-bit halves.
//   var fields   counts through slot_count (var_dev.h) from the same image; a count pass (only the
//                pieces of the counted fields) + device_scan give every tile its Arrow base without
//                a host sync, the write pass scans inside the tile.  STRING / BINARY payloads are
//                copied by 8 lanes per row (<= 512 B) or by the whole wave (longer), as aligned
//                8-byte destination words funnel-shifted from aligned source words, bytes at the two
//                ends; list elements go out in element order across the tile (find_row), their bits
//                by put_bits64; DECIMAL is one 16-byte copy per row.
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok): a selected value that
// fails decodes as null and raises kErrBounds; corrupt slots of unselected fields are never seen.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "project_dev.h"

namespace fury {

namespace {

// 64 rows' bits starting at row rbase (a multiple of 64), nlive of them inside the batch: whole
// 32-bit words, only those that hold a live row.
__device__ __forceinline__ void store_bits(uint8_t* bits, int64_t rbase, int nlive, uint64_t b) {
  const int lane = threadIdx.x & 63;
  if (lane < 2 && 32 * lane < nlive)
    gl(reinterpret_cast<uint32_t*>(bits))[(rbase >> 5) + lane] = static_cast<uint32_t>(b >> (32 * lane));
}

// Lanes li of a group of G copy batch bytes [p, p + n) to dst[0, n): aligned 8-byte destination
// words, byte stores at the two ends.  [p, p + n) lies inside the batch (slot_count).
__device__ __forceinline__ void copy_value(uint8_t* dst, const uint8_t* rows, int64_t p, int64_t n,
                                           int64_t total, int li, int G) {
  const int64_t head = min<int64_t>(n, (8 - (reinterpret_cast<uintptr_t>(dst) & 7)) & 7);
  const int64_t nw = (n - head) >> 3;
  const int64_t tail0 = head + 8 * nw;
  for (int64_t i = li; i < head; i += G) gl(dst)[i] = gl(rows)[p + i];
  for (int64_t i = tail0 + li; i < n; i += G) gl(dst)[i] = gl(rows)[p + i];
  for (int64_t w = li; w < nw; w += G)
    *gl(reinterpret_cast<uint64_t*>(dst + head + 8 * w)) = batch_word(rows, p + head + 8 * w, total);
}

// Count of the variable-length column c for tile row t (0 for null / bad; bad raises).
__device__ __forceinline__ int64_t var_count(const ProjArgs& a, CProjCol& c, const uint64_t* img, int t,
                                             int64_t base, int64_t r, const uint8_t* rows,
                                             int64_t total, bool* isnull, uint64_t* slot) {
  *isnull = field_slot(c, img, a.stride, t, base, slot);
  if (*isnull) return 0;
  bool bad = false;
  const int64_t n = slot_count(c.kind, c.width, *slot, base, rows, total, &bad);
  if (bad) {
    raise_oob(a.err, r);
    *isnull = true;
    *slot = 0;
  }
  return n;
}

// Count pass: every column of `a` is STRING / BINARY / LIST.  sums[q * nt + tile] = the tile's count
// of column q; kPos (fury_row_project_measure): offsets[r] = the row's start inside its tile.
template <bool NT, bool kPos>
__global__ __launch_bounds__(kProjThreads) void project_count(ProjArgs a,
                                                              const uint8_t* __restrict__ rows,
                                                              const int64_t* __restrict__ offs,
                                                              int64_t* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) uint64_t proj_img[];
  __shared__ ProjShared sh;
  const int tid = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * a.tile_rows;
  const int nr = static_cast<int>(min<int64_t>(a.tile_rows, a.nrows - r0));
  const int64_t total = offs ? gl(offs)[a.nrows] : a.nrows * a.fixed_size;
  stage_tile<NT>(a, rows, offs, total, r0, nr, sh, proj_img);
  const bool live = tid < nr;
  const int64_t base = live ? sh.rowbase[tid] : -1;
  for (int k = 0; k < a.ncols; k++) {
    CProjCol& c = pc(a, k);
    bool isnull;
    uint64_t slot;
    const int64_t cnt = var_count(a, c, proj_img, tid, base, r0 + tid, rows, total, &isnull, &slot);
    int64_t tot;
    const int64_t ex = block_excl_scan<kProjThreads>(cnt, &tot, sh.tmp);
    if (kPos && live) gl(c.offsets)[r0 + tid] = static_cast<int32_t>(ex);
    if (tid == 0) gl(sums)[static_cast<int64_t>(k) * gridDim.x + blockIdx.x] = tot;
  }
}

// fury_row_project_measure, after the scan of the tile sums: tile-relative starts -> Arrow offsets.
__global__ __launch_bounds__(kProjThreads) void project_measure_fix(ProjArgs a,
                                                                    const int64_t* __restrict__ sums,
                                                                    const int64_t* __restrict__ totals,
                                                                    int64_t nt) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kProjThreads + threadIdx.x;
  for (int k = 0; k < a.ncols; k++) {
    CProjCol& c = pc(a, k);
    if (r < a.nrows)
      gl(c.offsets)[r] += static_cast<int32_t>(gl(sums)[static_cast<int64_t>(k) * nt + r / a.tile_rows]);
    if (r == a.nrows - 1) gl(c.offsets)[a.nrows] = static_cast<int32_t>(gl(totals)[k]);
  }
}

// Write pass.  tbase[q * nt + tile]: Arrow base of the tile in the q-th STRING / BINARY / LIST column
// of the selection (NULL when it has none).
template <bool NT>
__global__ __launch_bounds__(kProjThreads) void project_write(ProjArgs a,
                                                              const uint8_t* __restrict__ rows,
                                                              const int64_t* __restrict__ offs,
                                                              const int64_t* __restrict__ tbase) {
  extern __shared__ __attribute__((aligned(16))) uint64_t proj_img[];
  __shared__ ProjShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * a.tile_rows;
  const int nr = static_cast<int>(min<int64_t>(a.tile_rows, a.nrows - r0));
  const int64_t total = offs ? gl(offs)[a.nrows] : a.nrows * a.fixed_size;
  stage_tile<NT>(a, rows, offs, total, r0, nr, sh, proj_img);

  // fixed-width and BOOL fields: one (field, 64-row chunk) unit per wave at a time
  const int nch = (nr + 63) >> 6;
  for (int u = wave; u < a.ncols * nch; u += kProjThreads / 64) {
    const int k = u / nch, ch = u - k * nch;
    CProjCol& c = pc(a, k);
    if (c.kind > kBool) continue;
    const int t = ch * 64 + lane;
    const bool live = t < nr;
    const int64_t r = r0 + t;
    uint64_t slot;
    const bool isnull = field_slot(c, proj_img, a.stride, t, live ? sh.rowbase[t] : -1, &slot);
    if (c.validity) store_bits(c.validity, r - lane, nr - ch * 64, __ballot(live && !isnull));
    uint8_t* dst = c.values;
    if (c.kind == kBool) {
      store_bits(dst, r - lane, nr - ch * 64, __ballot(live && (slot & 0xff) != 0));
    } else if (live) {
      switch (c.width) {
        case 8: *gl(reinterpret_cast<uint64_t*>(dst) + r) = slot; break;
        case 4: *gl(reinterpret_cast<uint32_t*>(dst) + r) = static_cast<uint32_t>(slot); break;
        case 2: *gl(reinterpret_cast<uint16_t*>(dst) + r) = static_cast<uint16_t>(slot); break;
        default: gl(dst)[r] = static_cast<uint8_t>(slot); break;
      }
    }
  }

  // variable-length fields: thread = row for the counts, then cooperative copies
  const bool live = tid < nr;
  const int64_t base = live ? sh.rowbase[tid] : -1;
  const int64_t r = r0 + tid;
  int q = 0;
  for (int k = 0; k < a.ncols; k++) {
    CProjCol& c = pc(a, k);
    if (c.kind < kBytes) continue;
    bool isnull;
    uint64_t slot;
    const int64_t cnt = var_count(a, c, proj_img, tid, base, r, rows, total, &isnull, &slot);
    if (c.validity) store_bits(c.validity, r - lane, nr - wave * 64, __ballot(live && !isnull));
    uint8_t* dst = c.values;
    if (c.kind == kDecimal) {
      if (live && dst) {
        uint64_t lo = 0, hi = 0;
        if (!isnull) {                                   // [p, p + 16) checked by slot_count
          const int64_t p = base + static_cast<int32_t>(slot >> 32);
          lo = *gl(reinterpret_cast<const uint64_t*>(rows + p));
          hi = *gl(reinterpret_cast<const uint64_t*>(rows + p + 8));
        }
        *gl(reinterpret_cast<uint64_t*>(dst + 16 * r)) = lo;
        *gl(reinterpret_cast<uint64_t*>(dst + 16 * r + 8)) = hi;
      }
      continue;
    }
    int64_t tot;
    const int64_t ex = block_excl_scan<kProjThreads>(cnt, &tot, sh.tmp);
    const int64_t gb = gl(tbase)[static_cast<int64_t>(q) * gridDim.x + blockIdx.x];
    q++;
    if (live) gl(c.offsets)[r] = static_cast<int32_t>(gb + ex);
    if (blockIdx.x == gridDim.x - 1 && tid == nr - 1)
      gl(c.offsets)[a.nrows] = static_cast<int32_t>(gb + tot);
    sh.pos[tid] = static_cast<int32_t>(ex);
    if (tid == 0) sh.pos[kProjThreads] = static_cast<int32_t>(tot);
    lds_barrier();
    const int64_t cap = c.capacity;
    if (tot > 0 && dst && c.kind == kBytes) {
      // short values: kProjGroup lanes per row; long ones: the whole wave
      const int g = tid / kProjGroup, li = tid % kProjGroup;
      for (int t = g; t < nr; t += kProjThreads / kProjGroup) {
        const int64_t at = gb + sh.pos[t];
        const int64_t len = min<int64_t>(sh.pos[t + 1] - sh.pos[t], cap - at);
        if (len <= 0 || sh.pos[t + 1] - sh.pos[t] > kProjLong) continue;
        const int64_t bt = sh.rowbase[t];
        const uint64_t sl = proj_img[static_cast<uint32_t>(t) * a.stride + (c.img >> 16)];
        copy_value(dst + at, rows, bt + static_cast<int32_t>(sl >> 32), len, total, li, kProjGroup);
      }
      for (int t = wave; t < nr; t += kProjThreads / 64) {
        const int64_t at = gb + sh.pos[t];
        const int64_t len = min<int64_t>(sh.pos[t + 1] - sh.pos[t], cap - at);
        if (len <= 0 || sh.pos[t + 1] - sh.pos[t] <= kProjLong) continue;
        const int64_t bt = sh.rowbase[t];
        const uint64_t sl = proj_img[static_cast<uint32_t>(t) * a.stride + (c.img >> 16)];
        copy_value(dst + at, rows, bt + static_cast<int32_t>(sl >> 32), len, total, lane, 64);
      }
    } else if (tot > 0 && dst) {
      // LIST of fixed-width elements -> child values + element validity, thread = element of the
      // tile.  A row owns elements only when its array passed the bounds check (else its count is 0).
      const int ew = c.width == 0 ? 1 : c.width;
      const int sh0 = static_cast<int>(gb & 63);
      const int64_t span = sh0 + tot;
      for (int64_t u0 = 0; u0 < span; u0 += kProjThreads) {
        const int64_t i = u0 + tid - sh0;                       // element index in the tile
        const bool act = i >= 0 && i < tot;
        bool valid = false;
        uint64_t v = 0;
        if (act) {
          const int t = find_row(sh.pos, nr, static_cast<int32_t>(i));
          const int64_t bt = sh.rowbase[t];
          const uint64_t sl = proj_img[static_cast<uint32_t>(t) * a.stride + (c.img >> 16)];
          const int64_t pa = bt + static_cast<int32_t>(sl >> 32);
          const int64_t n = static_cast<int32_t>(*gl(reinterpret_cast<const int64_t*>(rows + pa)));
          const int64_t j = i - sh.pos[t];
          valid = !((gl(rows)[pa + 8 + (j >> 3)] >> (j & 7)) & 1);
          if (valid) {
            const uint8_t* p = rows + pa + 8 + bm_bytes(n) + j * ew;
            switch (ew) {
              case 8: v = *gl(reinterpret_cast<const uint64_t*>(p)); break;
              case 4: v = *gl(reinterpret_cast<const uint32_t*>(p)); break;
              case 2: v = *gl(reinterpret_cast<const uint16_t*>(p)); break;
              default: v = *gl(p); break;
            }
          }
          const int64_t e = gb + i;
          if (e < cap) {
            switch (c.width) {
              case 8: *gl(reinterpret_cast<uint64_t*>(dst) + e) = v; break;
              case 4: *gl(reinterpret_cast<uint32_t*>(dst) + e) = static_cast<uint32_t>(v); break;
              case 2: *gl(reinterpret_cast<uint16_t*>(dst) + e) = static_cast<uint16_t>(v); break;
              case 1: gl(dst)[e] = static_cast<uint8_t>(v); break;
              default: break;                                 // bool elements: bits below
            }
          }
        }
        const uint64_t am = __ballot(act);
        const int64_t gbit0 = gb - sh0 + (u0 + tid - lane);     // 64-aligned
        if (c.elem_validity) put_bits64(c.elem_validity, gbit0, __ballot(act && valid), am, cap);
        if (c.width == 0) put_bits64(dst, gbit0, __ballot(act && valid && v != 0), am, cap);
      }
    }
    lds_barrier();                                  // sh.pos is rewritten by the next column
  }
}

bool is_counted(const ProjCol& c) { return c.kind == kBytes || c.kind == kListFixed; }

}  // namespace

// Piece list, image word of every column's bit and slot, row stride and tile rows of `a`
// (tile_rows > 0: keep it -- the count pass runs the write pass's tiles).
static void plan(ProjArgs* a, std::vector<ProjPiece>* pieces) {
  std::vector<int32_t> words;
  for (int k = 0; k < a->ncols; k++) {
    words.push_back(a->col[k].slot >> 6);
    words.push_back(a->bitmap_bytes / 8 + a->col[k].slot);
  }
  std::sort(words.begin(), words.end());
  words.erase(std::unique(words.begin(), words.end()), words.end());
  auto rank = [&](int32_t w) {
    return static_cast<int32_t>(std::lower_bound(words.begin(), words.end(), w) - words.begin());
  };
  for (int k = 0; k < a->ncols; k++) {
    ProjCol& c = a->col[k];
    c.img = rank(c.slot >> 6) | (rank(a->bitmap_bytes / 8 + c.slot) << 16);
  }
  pieces->clear();
  for (size_t i = 0; i < words.size(); i++) {
    if (!pieces->empty()) {
      ProjPiece& p = pieces->back();
      if (p.off + 8 * p.words == 8 * words[i] && p.words < 16) {
        p.words++;
        continue;
      }
    }
    pieces->push_back(ProjPiece{8 * words[i], 1});
  }
  a->nwords = static_cast<int32_t>(words.size());
  a->npieces = static_cast<int32_t>(pieces->size());
  a->stride = a->nwords | 1;
  a->magic = static_cast<uint32_t>((1ull << 32) / static_cast<uint32_t>(a->nwords)) + 1u;
  if (a->tile_rows <= 0) {
    // 256 rows within 48 KB of image, else 128 within 64 KB, else 64 (<= 129 words: 66 KB)
    a->tile_rows = a->stride * 8 * 256 <= 48 * 1024 ? 256 : a->stride * 8 * 128 <= 64 * 1024 ? 128 : 64;
  }
  for (int p = 0; p < a->npieces && p < kMaxProjPieces; p++) a->piece[p] = (*pieces)[p];
}

int finish_plan(ProjArgs* a, hipStream_t stream, DeviceTable* dt) {
  std::vector<ProjPiece> pieces;
  plan(a, &pieces);
  a->ptab = nullptr;
  if (a->npieces > kMaxProjPieces) {
    const int st = upload_table(pieces.data(), pieces.size() * sizeof(ProjPiece), stream, dt);
    if (st) return st;
    a->ptab = static_cast<const ProjPiece*>(dt->dev);
  }
  return FURY_OK;
}

namespace {

size_t image_bytes(const ProjArgs& a) { return static_cast<size_t>(a.tile_rows) * a.stride * 8; }

template <class K>
int allow_lds(K kern, size_t bytes) {
  if (bytes <= 48 * 1024) return FURY_OK;
  return check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(bytes)),
                   "project: LDS size");
}

// The STRING / BINARY / LIST columns of `a`, in selection order, as a selection of their own.
ProjArgs counted_columns(const ProjArgs& a) {
  ProjArgs b = a;
  b.ncols = 0;
  for (int k = 0; k < a.ncols; k++)
    if (is_counted(a.col[k])) b.col[b.ncols++] = a.col[k];
  return b;
}

// Count pass + scans: ws[q * nt + tile] = Arrow base of the tile in counted column q,
// ws[nseq * nt + q] = the column's total.  The caller frees *ws (dev_free).
int count_and_scan(const ProjArgs& b, const uint8_t* rows, const int64_t* offs, int64_t nt, bool pos,
                   hipStream_t stream, int64_t** ws) {
  const int nseq = b.ncols;
  int st = dev_alloc((nt * nseq + nseq + scan_workspace(nt)) * 8, stream, reinterpret_cast<void**>(ws));
  if (st) return st;
  const size_t lds = image_bytes(b);
  const dim3 grid(static_cast<unsigned>(nt)), block(kProjThreads);
#define FURY_PROJ_COUNT(NT, POS)                                                              \
  do {                                                                                        \
    st = allow_lds(project_count<NT, POS>, lds);                                              \
    if (!st) hipLaunchKernelGGL((project_count<NT, POS>), grid, block, lds, stream, b, rows, offs, *ws); \
  } while (0)
  if (b.nt) {
    if (pos) FURY_PROJ_COUNT(true, true);
    else FURY_PROJ_COUNT(true, false);
  } else {
    if (pos) FURY_PROJ_COUNT(false, true);
    else FURY_PROJ_COUNT(false, false);
  }
#undef FURY_PROJ_COUNT
  if (!st) st = check_hip(hipGetLastError(), "project_count launch");
  if (st) {
    dev_free(*ws, stream);
    *ws = nullptr;
    return st;
  }
  int64_t* totals = *ws + nt * nseq;
  for (int q = 0; q < nseq; q++) device_scan(*ws + q * nt, nt, totals + q, totals + nseq, stream);
  return FURY_OK;
}

int64_t tiles_of(const ProjArgs& a) { return (a.nrows + a.tile_rows - 1) / a.tile_rows; }

}  // namespace

int launch_project_measure(const ProjArgs& in, const uint8_t* rows, const int64_t* offs,
                           hipStream_t stream) {
  ProjArgs b = counted_columns(in);
  if (b.ncols == 0 || b.nrows == 0) return FURY_OK;
  b.tile_rows = 0;
  DeviceTable dt;
  int st = finish_plan(&b, stream, &dt);
  if (st) return st;
  const int64_t nt = tiles_of(b);
  if (nt > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  int64_t* ws = nullptr;
  st = count_and_scan(b, rows, offs, nt, true, stream, &ws);
  if (st) return st;
  const int64_t nb = (b.nrows + kProjThreads - 1) / kProjThreads;
  hipLaunchKernelGGL(project_measure_fix, dim3(static_cast<unsigned>(nb)), dim3(kProjThreads), 0, stream,
                     b, ws, ws + nt * b.ncols, nt);
  st = check_hip(hipGetLastError(), "project_measure_fix launch");
  dev_free(ws, stream);
  return st;
}

int launch_project(const ProjArgs& in, const uint8_t* rows, const int64_t* offs, hipStream_t stream) {
  if (in.nrows == 0) return FURY_OK;
  ProjArgs a = in;
  a.tile_rows = 0;
  DeviceTable dt, dtb;
  int st = finish_plan(&a, stream, &dt);
  if (st) return st;
  const int64_t nt = tiles_of(a);
  if (nt > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  int64_t* ws = nullptr;
  ProjArgs b = counted_columns(a);
  if (b.ncols > 0) {                 // the same tiles, only the counted columns' pieces
    st = finish_plan(&b, stream, &dtb);
    if (!st) st = count_and_scan(b, rows, offs, nt, false, stream, &ws);
    if (st) return st;
  }
  const size_t lds = image_bytes(a);
  const dim3 grid(static_cast<unsigned>(nt)), block(kProjThreads);
  if (a.nt) {
    st = allow_lds(project_write<true>, lds);
    if (!st) hipLaunchKernelGGL(project_write<true>, grid, block, lds, stream, a, rows, offs, ws);
  } else {
    st = allow_lds(project_write<false>, lds);
    if (!st) hipLaunchKernelGGL(project_write<false>, grid, block, lds, stream, a, rows, offs, ws);
  }
  if (!st) st = check_hip(hipGetLastError(), "project_write launch");
  if (ws) dev_free(ws, stream);
  return st;
}

}  // namespace fury
