// hash.hip -- key hash of a row batch: selected top-level fields of every row -> one 32-bit hash and
// a partition id per row (fury_row_hash).
//
// Reference semantics (FMT = java/fury-format/src/main/java/org/apache/fury/format): the batch form
// of reading a row's key fields with BinaryRow's getters (FMT/row/binary/BinaryRow.java,
// UnsafeTrait.java:68-197) and feeding them, in key order, to MurmurHash3.murmurhash3_x86_32
// (fury-core util/MurmurHash3.java), each value's hash seeding the next; the rules are numbered in
// include/fury_row.h.  The bytes hashed are the bytes fury_row_project would produce for the field.
//
// MI355X design.  The header words the keys need are staged exactly as the projected decode stages
// them (piece list, LDS image with an odd word stride: project_dev.h), never by lane = row loads at
// a row stride.  Then lane = row walks the chain over its keys from the image and stores 4 bytes per
// row per output, coalesced.  Two instantiations, chosen by the launcher from the key kinds:
//   fixed   every key is fixed-width or BOOL: the values are in the image, nothing else is read.
//   var     some key is STRING / BINARY / DECIMAL.  The rows of a tile are one byte range of the
//           batch, [row_offsets[r0], row_offsets[r0 + nr]): when it is at most kHashStage bytes the
//           workgroup copies it once into LDS with coalesced 16-byte loads (8-byte ones at an edge
//           that is not 16-byte aligned) and every lane hashes its values from LDS, 8 bytes per
//           read; a value outside the staged range (a larger tile, malformed offsets, a corrupt slot
//           pointing elsewhere) is hashed from global memory with aligned 8-byte loads
//           (batch_word).  Murmur's chain is serial per value, so a value stays on one lane.
// Unaligned values (only a corrupt slot produces one) are funnel-shifted from aligned words.
// Bounds follow "Decode bounds" in kernels.h (row_ok / slot_count / span_ok) as project.hip applies
// them: a failing row or value is a null key and raises kErrBounds; every read lies inside
// [0, total); corrupt slots of non-key fields are never seen.
#include <hip/hip_runtime.h>

#include "project_dev.h"

namespace fury {

namespace {

constexpr int kHashStage = 32 * 1024;          // bytes of rows a tile stages in LDS
constexpr int kHashInFlight = 4;               // 16-byte staging loads per lane before the first use

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The `rem` (1..7) low bytes of w: an optional block, then the 1-3 byte tail.
__device__ __forceinline__ uint32_t hash_rest(uint32_t h, uint64_t w, int rem) {
  uint32_t k = static_cast<uint32_t>(w);
  if (rem >= 4) {
    h = mm3_block(h, k);
    k = static_cast<uint32_t>(w >> 32);
    rem -= 4;
  }
  if (rem > 0) h = mm3_tail(h, k & (0xffffffffu >> (32 - 8 * rem)));
  return h;
}

// H(the `width` low bytes of v, h) for a value held in a register: width 1, 2, 4 or 8.
__device__ __forceinline__ uint32_t hash_scalar(uint32_t h, uint64_t v, int width) {
  if (width == 8) {
    h = mm3_block(mm3_block(h, static_cast<uint32_t>(v)), static_cast<uint32_t>(v >> 32));
  } else {
    h = hash_rest(h, v, width);
  }
  return mm3_fmix(h ^ static_cast<uint32_t>(width));
}

// The staged byte range of a tile: batch bytes [s0, s1) (multiples of 8) at LDS byte d + (x - s0).
struct Staged {
  const uint64_t* lds;
  int64_t s0, s1;                     // s1 <= s0: nothing is staged
  int32_t d;
};

// H(batch bytes [p, p + n), h); [p, p + n) lies inside the batch (slot_count).
__device__ __forceinline__ uint32_t hash_span(uint32_t h, const uint8_t* rows, int64_t p, int64_t n,
                                              int64_t total, const Staged& sg) {
  const int64_t nw = n >> 3;
  const int rem = static_cast<int>(n & 7);
  if (p >= sg.s0 && p + n <= sg.s1) {
    // from LDS: aligned words funnel-shifted (the word after the last staged one is never past the
    // buffer: kHashStage + 32 bytes are allocated)
    const int64_t q = p - sg.s0 + sg.d;
    const uint64_t* w = sg.lds + (q >> 3);
    const int sh = static_cast<int>(q & 7) * 8;
    if (sh == 0) {
      for (int64_t j = 0; j < nw; j++) {
        const uint64_t v = w[j];
        h = mm3_block(mm3_block(h, static_cast<uint32_t>(v)), static_cast<uint32_t>(v >> 32));
      }
      if (rem) h = hash_rest(h, w[nw], rem);
    } else {
      uint64_t lo = w[0];
      for (int64_t j = 0; j < nw; j++) {
        const uint64_t hi = w[j + 1];
        const uint64_t v = (lo >> sh) | (hi << (64 - sh));
        h = mm3_block(mm3_block(h, static_cast<uint32_t>(v)), static_cast<uint32_t>(v >> 32));
        lo = hi;
      }
      if (rem) h = hash_rest(h, (lo >> sh) | (w[nw + 1] << (64 - sh)), rem);
    }
  } else {
    for (int64_t j = 0; j < nw; j++) {
      const uint64_t v = batch_word(rows, p + 8 * j, total);
      h = mm3_block(mm3_block(h, static_cast<uint32_t>(v)), static_cast<uint32_t>(v >> 32));
    }
    if (rem) {
      const int64_t s = p + 8 * nw;
      uint64_t v = 0;
      if (s + 8 <= total) {
        v = batch_word(rows, s, total);
      } else {                                    // the batch's last bytes: by byte
        for (int i = 0; i < rem; i++) v |= static_cast<uint64_t>(gl(rows)[s + i]) << (8 * i);
      }
      h = hash_rest(h, v, rem);
    }
  }
  return mm3_fmix(h ^ static_cast<uint32_t>(n));
}

// Copies the tile's rows, batch bytes [lo, hi), into `stage` when they are one well-formed range of
// at most kHashStage bytes: whole 16-byte blocks of memory, the 8-byte half of a block at an edge.
// Only aligned 8-byte words inside [0, total) are read.
__device__ __forceinline__ Staged stage_rows(const uint8_t* rows, int64_t lo, int64_t hi, int64_t total,
                                             uint8_t* stage) {
  Staged sg;
  sg.lds = reinterpret_cast<const uint64_t*>(stage);
  sg.s0 = sg.s1 = 0;
  sg.d = 0;
  if (lo < 0 || lo > hi || hi > total) return sg;
  const int64_t s0 = lo & ~int64_t(7);
  const int64_t s1 = min((hi + 7) & ~int64_t(7), total & ~int64_t(7));
  if (s1 <= s0 || s1 - s0 > kHashStage) return sg;
  const int d = static_cast<int>((reinterpret_cast<uintptr_t>(rows) + s0) & 8);
  const int nblk = static_cast<int>((d + (s1 - s0) + 15) >> 4);
  const int64_t x00 = s0 - d;                     // batch offset of LDS byte 0: 16-byte aligned memory
  for (int c0 = 0; c0 < nblk; c0 += kProjThreads * kHashInFlight) {
    u32x4 v[kHashInFlight];
    int at[kHashInFlight];
#pragma unroll
    for (int u = 0; u < kHashInFlight; u++) {
      const int c = c0 + u * kProjThreads + static_cast<int>(threadIdx.x);
      at[u] = -1;
      v[u] = u32x4{0, 0, 0, 0};
      if (c < nblk) {
        const int64_t x = x00 + 16 * static_cast<int64_t>(c);
        const bool first = x >= s0, second = x + 16 <= s1;
        at[u] = c;
        if (first && second) {
          v[u] = __builtin_nontemporal_load(gl(reinterpret_cast<const u32x4*>(rows + x)));
        } else {
          const uint64_t w =
              __builtin_nontemporal_load(gl(reinterpret_cast<const uint64_t*>(rows + x + (first ? 0 : 8))));
          const uint32_t wl = static_cast<uint32_t>(w), wh = static_cast<uint32_t>(w >> 32);
          v[u] = first ? u32x4{wl, wh, 0, 0} : u32x4{0, 0, wl, wh};
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kHashInFlight; u++)
      if (at[u] >= 0) *reinterpret_cast<u32x4*>(stage + 16 * at[u]) = v[u];
  }
  sg.s0 = s0;
  sg.s1 = s1;
  sg.d = d;
  return sg;
}

// VAR: some key is STRING / BINARY / DECIMAL.  Dynamic LDS: the header image, then (VAR) the
// staged rows.
template <bool VAR>
__global__ __launch_bounds__(kProjThreads) void hash_rows(ProjArgs a, const uint8_t* __restrict__ rows,
                                                          const int64_t* __restrict__ offs,
                                                          uint32_t seed, uint32_t num_parts,
                                                          uint32_t* __restrict__ out_hashes,
                                                          int32_t* __restrict__ out_part_ids,
                                                          int32_t stage_at) {
  extern __shared__ __attribute__((aligned(16))) uint64_t hash_img[];
  __shared__ ProjShared sh;
  const int tid = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * a.tile_rows;
  const int nr = static_cast<int>(min<int64_t>(a.tile_rows, a.nrows - r0));
  const int64_t total = offs ? gl(offs)[a.nrows] : a.nrows * a.fixed_size;
  stage_tile<true>(a, rows, offs, total, r0, nr, sh, hash_img);
  Staged sg;
  sg.lds = nullptr;
  sg.s0 = sg.s1 = 0;
  sg.d = 0;
  if (VAR) {
    const int64_t lo = offs ? gl(offs)[r0] : r0 * a.fixed_size;
    const int64_t hi = offs ? gl(offs)[r0 + nr] : (r0 + nr) * a.fixed_size;
    sg = stage_rows(rows, lo, hi, total, reinterpret_cast<uint8_t*>(hash_img) + stage_at);
    lds_barrier();
  }
  if (tid >= nr) return;
  const int64_t base = sh.rowbase[tid];
  const int64_t r = r0 + tid;
  uint32_t h = seed;
  for (int k = 0; k < a.ncols; k++) {
    CProjCol& c = pc(a, k);
    uint64_t slot;
    bool isnull = field_slot(c, hash_img, a.stride, tid, base, &slot);
    if (c.kind == kBool) slot = (slot & 0xff) != 0;
    int64_t n = c.width;                          // kFixed: 1 / 2 / 4 / 8; kBool: 1 (launcher)
    if (VAR && c.kind >= kBytes && !isnull) {
      bool bad = false;
      n = slot_count(c.kind, c.width, slot, base, rows, total, &bad);
      if (c.kind == kDecimal) n = 16;
      if (bad) {
        raise_oob(a.err, r);
        isnull = true;
      }
    }
    if (isnull) {
      h = mm3_null(h);
    } else if (VAR && c.kind >= kBytes) {
      h = hash_span(h, rows, base + static_cast<int32_t>(slot >> 32), n, total, sg);
    } else {
      h = hash_scalar(h, slot, static_cast<int>(n));
    }
  }
  if (out_hashes) gl(out_hashes)[r] = h;
  if (out_part_ids) gl(out_part_ids)[r] = static_cast<int32_t>(h % num_parts);
}

template <class K>
int allow_lds(K kern, size_t bytes) {
  if (bytes <= 48 * 1024) return FURY_OK;
  return check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(bytes)),
                   "hash: LDS size");
}

}  // namespace

int launch_hash(const ProjArgs& in, const uint8_t* rows, const int64_t* offs, uint32_t seed,
                uint32_t num_parts, uint32_t* out_hashes, int32_t* out_part_ids, hipStream_t stream) {
  if (in.nrows == 0) return FURY_OK;
  ProjArgs a = in;
  a.tile_rows = 0;
  bool var = false;
  for (int k = 0; k < a.ncols; k++) {
    if (a.col[k].kind == kBool) a.col[k].width = 1;       // hashed as the one byte 0 / 1
    var = var || a.col[k].kind >= kBytes;
  }
  DeviceTable dt;
  int st = finish_plan(&a, stream, &dt);
  if (st) return st;
  const int64_t nt = (a.nrows + a.tile_rows - 1) / a.tile_rows;
  if (nt > 0x7fffffff) return set_error(FURY_ERR_INVALID_ARGUMENT, "batch too large");
  const size_t image = (static_cast<size_t>(a.tile_rows) * a.stride * 8 + 15) & ~size_t(15);
  const size_t lds = image + (var ? kHashStage + 32 : 0);
  const dim3 grid(static_cast<unsigned>(nt)), block(kProjThreads);
  if (num_parts == 0) num_parts = 1;              // unused without out_part_ids
  if (var) {
    st = allow_lds(hash_rows<true>, lds);
    if (!st)
      hipLaunchKernelGGL(hash_rows<true>, grid, block, lds, stream, a, rows, offs, seed, num_parts,
                         out_hashes, out_part_ids, static_cast<int32_t>(image));
  } else {
    st = allow_lds(hash_rows<false>, lds);
    if (!st)
      hipLaunchKernelGGL(hash_rows<false>, grid, block, lds, stream, a, rows, offs, seed, num_parts,
                         out_hashes, out_part_ids, static_cast<int32_t>(image));
  }
  if (!st) st = check_hip(hipGetLastError(), "hash_rows launch");
  return st;
}

}  // namespace fury
