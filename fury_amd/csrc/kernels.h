// kernels.h — launch interfaces between the C-ABI layer (capi.cpp) and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "internal.h"

namespace fury {

// The same pointer in the global address space: accesses through it are global_load /
// global_store, not flat (a flat access also counts against lgkmcnt, so every later LDS or scalar
// wait waits for it too).  Pointers loaded from argument blocks or tables are generic to the
// compiler.  Only for pointers into device / host memory, never LDS.
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gl(T* p) {
  return (__attribute__((address_space(1))) T*)(p);
}
// Pointer casts that keep the operand's address space (global via gl(), or a generic pointer the
// compiler resolves, e.g. into LDS), for code instantiated once per address space.
template <class T, class U>
__device__ __forceinline__ __attribute__((address_space(1))) T* cast_as(__attribute__((address_space(1))) U* p) {
  return (__attribute__((address_space(1))) T*)(p);
}
template <class T, class U>
__device__ __forceinline__ T* cast_as(U* p) {
  return (T*)(p);
}

// Columns per fixed-tile launch: the pointer table travels in the kernel argument block
// (scalar-loaded, no per-call device upload).  Wider schemas upload it (FixedArgs.tab).
constexpr int kMaxFixedCols = 128;

// Per-column record.  Every member is naturally aligned inside an 8-byte-aligned record: the
// kernels index this table with a wave-uniform column number, which the compiler turns into
// scalar (SMEM) loads; an int8 side array produced a byte-offset SMEM base that gfx950 masks
// to dword alignment (observed as an aperture fault), so keep all members >= 4 bytes.
struct FixedCol {
  const uint8_t* values;
  uint8_t* validity;                  // encode: input (NULL = all valid); decode: output or NULL
  int32_t width;                      // 1, 2, 4, 8; 0 = BOOL (bit-packed)
  int32_t pad_;
};

// Schemas wider than kMaxFixedCols take their column table from device memory (uploaded per
// call, FixedArgs.tab) and run the general tile kernel with 64-row tiles up to kMaxWideFixedCols
// (a 64-row tile, bitmap + 8 B per field per row, within the 160 KB of LDS); wider ones run the
// column-block kernels (64 rows x 64 fields per workgroup, no field limit).
constexpr int kMaxWideFixedCols = 315;

struct FixedArgs {
  FixedCol col[kMaxFixedCols];
  const FixedCol* tab;                // device table for > kMaxFixedCols fields, else NULL
  int32_t ncols;
  int32_t bitmap_bytes;
  int32_t row_size;
  int32_t tail_tiles;                 // fast-path encode: trailing tiles stored with the default
                                      // cache policy; filled by launch_encode_fixed, callers leave 0
  int64_t nrows;
};

// Host-direct mode of the calling thread (hostpath.cpp): plain instead of non-temporal accesses.
void set_thread_host_direct(bool on);
int launch_encode_fixed(const FixedArgs& a, uint8_t* rows, hipStream_t stream, bool fast);
int launch_decode_fixed(const FixedArgs& a, const uint8_t* rows, hipStream_t stream, bool fast);

// ---- variable-length schemas ----------------------------------------------------------------
constexpr int kMaxVarCols = 64;
// Wider schemas: column table in device memory (VarArgs.tab), LDS-DMA / ticketed kernels.
constexpr int kMaxWideVarCols = 256;

// One top-level field as seen by the var kernels.
struct VarCol {
  const uint8_t* values;     // fixed values / bytes payload / decimal values / list child values
  uint8_t* validity;         // field validity (Arrow bits) or NULL
  int32_t* offsets;          // bytes / list offsets (n + 1)
  uint8_t* elem_validity;    // list element validity or NULL
  int32_t kind;              // FieldKind
  int32_t width;             // fixed: 1/2/4/8, 0 = bool; list: element width (0 = bool elements)
  int32_t var_slot;          // index among var fields (decode measure scratch), -1 otherwise
  int32_t nullable;
  int64_t capacity;          // decode: payload bytes (STRING/BINARY) / child elements (LIST)
};

struct VarArgs {
  VarCol col[kMaxVarCols];
  const VarCol* tab;         // device table for > kMaxVarCols fields, else NULL
  const VarCol* htab;        // its host copy (launchers only; never read on the device)
  int32_t ncols;
  int32_t bitmap_bytes;
  int32_t fixed_size;
  int32_t nvar;
  int64_t nrows;
  int32_t tile_rows;         // rows per encode tile (encode_tile_rows)
  int32_t help_now;          // look-backs help a silent predecessor at once (test hook, tuning
                             // "lookback_help"); 0 in production
  int32_t skip;              // diagnostics (tuning "var_skip"): phases skipped, outputs WRONG
  int32_t dec_pipe;          // decode_var_reg: persistent workgroups, two row stages (var_dec_pipe)
  uint32_t* err;             // the launch stream's device error slot (device_error_word) or NULL
};

// Host-visible device error words: host-pinned, mapped memory, one slot of kErrWords 32-bit words
// PER STREAM (capi.cpp), that kernels set with system-scope STORES (no read-modify-write over
// PCIe) when they cannot produce a valid result:
//   [kErrLookBack]            a look-back that gave up (FURY_ERR_DEVICE)
//   [kErrBounds], [+2, +3]    a decode read that would leave the batch, and where (one 64-bit
//                             word: a row, or bit 63 | node << 40 | entry) (FURY_ERR_OUT_OF_BOUNDS)
//   [kErrMapCount], [+2, +3]  map key / value arrays of different lengths (FURY_ERR_UNSUPPORTED)
//   [kErrTooDeep], [+2, +3]   encode: a row too large for on-chip assembly in a schema nested
//                             deeper than the row interpreter reaches (FURY_ERR_UNSUPPORTED)
//   [kErrInternal], [+2, +3]  a decode plan the device could not follow (tile BFS: a write tile
//                             whose records outgrew the arena its count pass fitted) (FURY_ERR_DEVICE)
//   [kErrBudget], [+2, +3]    nested decode: a row whose slots alias other bytes so that the row
//                             walk would visit more than 2 x its bytes + 64 items -- the DEVICE's
//                             limit, not a reference exception (FURY_ERR_UNSUPPORTED with its own
//                             message; tuning counter "decode_budget_errors")
// device_error_word(stream, &w) gives the slot kernels launched on `stream` raise into (NULL if the
// runtime cannot map host memory; FURY_ERR_DEVICE when every slot is held by a live stream);
// release_error_slot(stream) frees it before the stream is destroyed; take_device_error(stream) takes that slot only (flag exchanged first,
// then its location) and sets the thread's last error when one was raised.
constexpr int kErrWords = 24;
constexpr int kErrLookBack = 0, kErrBounds = 4, kErrMapCount = 8, kErrTooDeep = 12, kErrBudget = 16,
              kErrInternal = 20;
int device_error_word(hipStream_t stream, uint32_t** out);
void release_error_slot(hipStream_t stream, bool sync = true);
int error_slots_in_use();
int error_slots_quarantined();
int thread_key_exits();
int last_assigned_key_kind();
void drain_error_quarantine();
int take_device_error(hipStream_t stream);
int64_t device_error_count();        // failures raised so far (taken or pending), no sync
// The nested decode's item-budget error (device limit): the status and message every engine
// reports it with, counted by tuning "decode_budget_errors".
int budget_error(const std::string& where);
int64_t budget_errors();

// Cached device workspace (capi.cpp): stream-ordered like hipMallocAsync / hipFreeAsync, without
// their per-call host cost.
int dev_alloc(int64_t bytes, hipStream_t stream, void** out);
void dev_free(void* p, hipStream_t stream);
int64_t dev_live_blocks();           // blocks handed out and not yet given back (tuning "workspace_live")
// One cached block and the stream it goes back on when the holder goes (move-only).
struct DevBlock {
  void* p = nullptr;
  hipStream_t stream = nullptr;
  DevBlock() = default;
  DevBlock(DevBlock&& o) noexcept : p(o.release()), stream(o.stream) {}
  DevBlock& operator=(DevBlock&& o) noexcept {
    if (this != &o) {
      reset();
      stream = o.stream;
      p = o.release();
    }
    return *this;
  }
  ~DevBlock() { reset(); }
  int alloc(int64_t bytes, hipStream_t s) {      // gives back the block it held
    reset();
    stream = s;
    return dev_alloc(bytes, s, &p);
  }
  void reset() { dev_free(release(), stream); }
  void* release() {
    void* q = p;
    p = nullptr;
    return q;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Decode bounds (round 3).  Every byte a decode reads lies in [0, total) of the rows buffer, total
// = the batch's row bytes (row_offsets[nrows]): the reference's getters read through MemoryBuffer,
// whose slice / get throw IndexOutOfBoundsException for a range past the buffer (fury-core
// memory/MemoryBuffer.java:2500-2519, through UnsafeTrait.getBuffer / getBinary,
// format/row/binary/UnsafeTrait.java:44-51,118-129, and the getInt64 of an array header,
// BinaryArray.pointTo :69-78).  A value that fails decodes as null, the kernel records where in the
// error words and the call reports FURY_ERR_OUT_OF_BOUNDS; nothing outside the batch is read.
// A negative size or element count (NegativeArraySizeException / a failed assert there) fails too.
__device__ __forceinline__ bool span_ok(int64_t p, int64_t len, int64_t total) {
  return p >= 0 && len >= 0 && len <= total - p;
}
// A workgroup barrier that orders LDS only: every wave's LDS / scalar operations complete, then
// s_barrier.  __syncthreads() adds a workgroup-scope release / acquire fence, which also waits
// for every outstanding GLOBAL store and atomic of the wave -- a tile whose column stores are in
// flight then waits out their HBM write latency at the barrier.  Use this one where the barrier
// only hands LDS data between waves (never after LDS-DMA, whose completion is counted by vmcnt).
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The location is one 64-bit store (concurrent raisers never mix halves), made visible before the
// flag by a release store of the flag; stores only -- no atomics over PCIe.
__device__ __forceinline__ void raise_at(uint32_t* err, int slot, uint64_t where) {
  if (!err) return;
  __hip_atomic_store(reinterpret_cast<uint64_t*>(err + slot + 2), where, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(err + slot, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void raise_oob(uint32_t* err, int64_t row) {
  raise_at(err, kErrBounds, static_cast<uint64_t>(row));
}
__device__ __forceinline__ uint64_t err_where_entry(int node, int64_t entry) {
  return (1ull << 63) | (static_cast<uint64_t>(node) << 40) | static_cast<uint64_t>(entry);
}

// Copies a host column table to device memory on `stream` (stream-ordered: through a pinned
// staging ring, no host synchronisation); the table is freed stream-ordered when the holder goes.
struct DeviceTable {
  void* dev = nullptr;
  hipStream_t stream = nullptr;
  std::vector<uint8_t> host;          // host copy of the table (for the launchers)
  DeviceTable() = default;
  DeviceTable(const DeviceTable&) = delete;
  DeviceTable& operator=(const DeviceTable&) = delete;
  ~DeviceTable();
};
int upload_table(const void* host, size_t bytes, hipStream_t stream, DeviceTable* out);

// Device scratch for scans; grown on demand (hipMalloc outside graph capture only).
struct Workspace {
  void* ptr = nullptr;
  size_t bytes = 0;
};
int workspace_reserve(size_t bytes, void** out);

// Rows per encode tile for this column set (the staged per-row inputs must fit the LDS pool).
int encode_tile_rows(const VarArgs& a);
int64_t lookback_timeouts();
int var_dec_rows_rejected();          // forced "var_dec_rows" tiles whose images did not fit (plan used)
// The wide decode's launch geometry: threads per tile, the LDS stage (~64 rows of the estimated row
// size) and the per-wave images, tiles, sequence (STRING / BINARY / LIST) fields.
struct WideGeom {
  int nseq = 0, th = 256;
  uint32_t stage = 0, imgs = 0;
  int64_t nt = 0;
};
// Plan form of the wide decode (fury_decode_prepare / _execute): the count pass + scan once, the
// per-tile bases kept for the write pass.
struct WidePlan {
  DevBlock ws;               // the scanned per-tile bases
  WideGeom g;                // what the prepare launched with; the execute's too, but for the stage
};
// batch_bytes: offs[nrows] where the caller has read it, -1: read here (one host sync)
int wide_prepare(const VarArgs& a, const uint8_t* rows, const int64_t* offs, hipStream_t stream,
                 int64_t batch_bytes, WidePlan* wp, std::vector<int64_t>* seq_totals);
int wide_execute(const VarArgs& a, const uint8_t* rows, const int64_t* offs, hipStream_t stream,
                 const WidePlan& wp);
void wide_free(WidePlan* wp);
// offsets_only: fury_row_decode_measure (the Arrow offsets of the variable-length fields only)
int launch_decode_wide(const VarArgs& a, const uint8_t* rows, const int64_t* offs, hipStream_t stream,
                       bool offsets_only);
int launch_encode_wide(const VarArgs& a, const int64_t* offs, uint8_t* rows, int64_t cap,
                       hipStream_t stream);
int launch_measure_rows(const VarArgs& a, int64_t* row_offsets, hipStream_t stream);
// Rows at the offsets fury_row_measure produced; never writes row bytes at or past `cap`.
int launch_encode_var(const VarArgs& a, const int64_t* row_offsets, uint8_t* rows, int64_t cap,
                      hipStream_t stream);
int launch_encode_measured_var(const VarArgs& a, int64_t* row_offsets, uint8_t* rows, int64_t cap,
                               hipStream_t stream);
int launch_decode_measure(const VarArgs& a, const uint8_t* rows, const int64_t* row_offsets,
                          hipStream_t stream);
// Single pass: computes the Arrow offsets itself (decoupled look-back scan across workgroups)
// and writes payloads clipped to each column's capacity.
int launch_decode_var(const VarArgs& a, const uint8_t* rows, const int64_t* row_offsets,
                      hipStream_t stream, bool arrow);
// ---- projected decode: project.hip -----------------------------------------------------------
constexpr int kMaxProjCols = 64;      // selected fields per call (the table is in the argument block)
constexpr int kMaxProjPieces = 40;    // pieces in the argument block; longer lists are uploaded

// One selected field: a VarCol-like record plus the field's slot index in the row.  Indexed
// wave-uniformly (scalar loads): every member >= 4 bytes, see FixedCol.
struct ProjCol {
  uint8_t* values;           // fixed values / BOOL bits / bytes payload / decimal values / list child values
  uint8_t* validity;         // field validity (Arrow bits) or NULL
  int32_t* offsets;          // bytes / list offsets (n + 1)
  uint8_t* elem_validity;    // list element validity or NULL
  int64_t capacity;          // payload bytes (STRING/BINARY) / child elements (LIST)
  int32_t kind;              // FieldKind
  int32_t width;             // fixed: 1/2/4/8; list: element width (0 = bool elements)
  int32_t slot;              // field index in the schema: bitmap bit, slot at bitmap_bytes + 8 * slot
  int32_t img;               // LDS image word of the bitmap word | of the slot << 16 (launcher)
};

// A run of 8-byte words of the row header that the selection reads: at most 16 words (128 B).
struct ProjPiece {
  int32_t off;               // byte offset in the row
  int32_t words;
};

struct ProjArgs {
  ProjCol col[kMaxProjCols];
  ProjPiece piece[kMaxProjPieces];
  const ProjPiece* ptab;     // device piece list when npieces > kMaxProjPieces, else NULL
  uint32_t* err;             // the launch stream's device error slot or NULL
  int64_t nrows;
  int32_t ncols;
  int32_t bitmap_bytes;
  int32_t fixed_size;
  int32_t nt;                // non-temporal row loads (0 for host-direct calls)
  // set by the launchers:
  int32_t npieces;
  int32_t nwords;            // image words per row (sum of the pieces)
  int32_t stride;            // image row stride in words (odd)
  int32_t tile_rows;         // 64 / 128 / 256
  uint32_t magic;            // 2^32 / nwords + 1: item / nwords by multiply-high
  int32_t pad_;
};
static_assert(sizeof(ProjArgs) <= 4096, "ProjArgs must fit the kernel argument block");

bool thread_host_direct();            // the calling thread's host-direct mode (fixed.hip)
// row_offsets NULL: row i at i * fixed_size (fixed schemas).  Both are asynchronous on `stream`.
int launch_project(const ProjArgs& a, const uint8_t* rows, const int64_t* row_offsets,
                   hipStream_t stream);
int launch_project_measure(const ProjArgs& a, const uint8_t* rows, const int64_t* row_offsets,
                           hipStream_t stream);
// The launcher-set members of `a` (piece list, image words, stride, tile rows; project.hip); a list
// longer than kMaxProjPieces is uploaded on `stream` and lives as long as *dt.
int finish_plan(ProjArgs* a, hipStream_t stream, DeviceTable* dt);

// ---- in-place update of selected fixed-width fields: update.hip ----------------------------------
// The mirror image of the projected decode, on the same records: ProjCol.values / .validity are the
// INPUT column of the field (read only; kind kFixed / kBool, width 0 = BOOL bits), the piece list is
// the list of row words that are rewritten.  row_mask: optional bitmap (bit r = 1: update row r),
// read as 32-bit words.  Write bounds = "Decode bounds" above applied to stores: a row whose header
// [base, base + fixed_size) leaves [0, total), or whose own extent (row_offsets[r + 1] - base) is
// shorter than fixed_size, is not written and raises kErrBounds.  Asynchronous on `stream`.
int launch_update(const ProjArgs& a, uint8_t* rows, const int64_t* row_offsets,
                  const uint8_t* row_mask, hipStream_t stream);

// ---- row selection: take.hip -------------------------------------------------------------------
// Gathers whole rows (BinaryRow.copy() over a batch): output row j = the bytes of source row
// indices[j].  row_offsets NULL: fixed-size rows (row i at i * fixed_size, output row j at
// j * fixed_size; out_offsets optional).  out NULL: the measure form, only out_offsets is written.
// Bounds = "Decode bounds" above: a source row is read only when its index is in [0, nrows) and its
// extent lies in [0, row_offsets[nrows]) with a size >= 0 that is a multiple of 8; otherwise the
// output row has size 0 (fixed-size rows: zero bytes) and kErrBounds is raised.  Output bytes at or
// past `cap` are never written while out_offsets is always complete.  Asynchronous on `stream`.
struct TakeArgs {
  const uint8_t* rows;
  const int64_t* row_offsets;         // NULL for fixed-size rows
  int64_t nrows;
  int64_t fixed_size;
  const int64_t* indices;             // take: n of them (device)
  int64_t n;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // take: n + 1 entries; filter: nrows + 1
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
int launch_take(const TakeArgs& a, hipStream_t stream);
// Keeps the rows whose mask bit (LSB-first, read as 32-bit words) is 1, in row order: *out_count
// rows; out_offsets entries past the count repeat the total, out_indices (optional, nrows entries)
// holds the kept row numbers and -1 past the count.  The count is never read by the host.
int launch_filter(const TakeArgs& a, const uint8_t* row_mask, int64_t* out_count,
                  int64_t* out_indices, hipStream_t stream);
// FURY_ERR_INVALID_ARGUMENT ("batch too large") for a row count the selection kernels cannot index.
int too_large(int64_t n, int64_t fixed_size);
// The second half of a selection whose row list and count live on the device (filter, partition):
// a.out_offsets[0, nrows) holds the sizes of the selected rows (0 at or past *count), idx[j] the
// source row of output row j < *count.  Scans the offsets in place (sws: scan_workspace(nrows))
// and copies; fixed-size rows: the offsets, when wanted, and the copy come from *count.
void copy_selected(const TakeArgs& a, const int64_t* idx, const int64_t* count, int64_t* sws,
                   hipStream_t stream);

// ---- rows by key, batches end to end: partition.hip ----------------------------------------------
// Stable P-way partition of a batch by a per-row id (filter from 2 ways to P): the kept rows (0 <=
// part_ids[i] < num_parts) sorted by (id, source row).  out_part_rows[p] (num_parts + 1 entries) =
// kept rows with id < p; out_indices / out_positions (optional, nrows entries) = the permutation and
// its inverse, -1 at or past the count / for a dropped row.  a.out_offsets, capacity, bounds and the
// fixed-size form as in launch_filter (a.n = nrows).  Nothing is read by the host.
constexpr int kPartitionMaxParts = 65535;
int launch_partition(const TakeArgs& a, const int32_t* part_ids, int32_t num_parts,
                     int64_t* out_part_rows, int64_t* out_indices, int64_t* out_positions,
                     hipStream_t stream);
// Batches of one schema end to end: output row base[k] + i = row i of source k (base[k] = rows of
// the sources before k, base[nsrc] = n).  ro[k] NULL: fixed-size rows.  A row is checked against
// its own source's [0, ro[k][nrows_k]); a failing one has size 0 and raises kErrBounds with its
// output position.  out NULL: the measure form.
constexpr int kConcatMaxSources = 32;
struct ConcatArgs {
  const uint8_t* rows[kConcatMaxSources];
  const int64_t* ro[kConcatMaxSources];
  int64_t base[kConcatMaxSources + 1];
  int32_t nsrc;
  int32_t fixed;                      // fixed-size rows: every ro[k] is NULL
  int64_t fixed_size;
  int64_t n;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // n + 1 entries; optional for fixed-size rows
  uint32_t* err;
};
int launch_concat(const ConcatArgs& a, hipStream_t stream);

// ---- key hash of a row batch: hash.hip -------------------------------------------------------------
// MurmurHash3_x86_32, the function the reference ships as MurmurHash3.murmurhash3_x86_32: 4-byte
// little-endian blocks, a 1-3 byte tail, fmix32(h ^ len).  One definition for the host entry points
// (fury_hash_bytes / fury_hash_null, capi.cpp) and the kernels.
__host__ __device__ inline uint32_t mm3_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ inline uint32_t mm3_scramble(uint32_t k) {
  return mm3_rotl(k * 0xcc9e2d51u, 15) * 0x1b873593u;
}
__host__ __device__ inline uint32_t mm3_block(uint32_t h, uint32_t k) {
  return mm3_rotl(h ^ mm3_scramble(k), 13) * 5u + 0xe6546b64u;
}
// `k`: the 1-3 tail bytes, zero-extended.
__host__ __device__ inline uint32_t mm3_tail(uint32_t h, uint32_t k) { return h ^ mm3_scramble(k); }
__host__ __device__ inline uint32_t mm3_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}
// A null key: a zero-length value whose length word is 0xFFFFFFFF (rule 2 of fury_row_hash).
__host__ __device__ inline uint32_t mm3_null(uint32_t h) { return mm3_fmix(h ^ 0xffffffffu); }

// hash[r] = the chain of rule 2 over the a.ncols key fields of row r in a.col order (ProjCol.kind /
// .width / .slot; the output members are unused), part_id[r] = (int32)(hash[r] % num_parts).  Either
// output may be NULL.  Bounds = "Decode bounds" above as the projected decode applies them: a row
// that fails row_ok has every key null, a value whose span fails is null, both raise kErrBounds with
// the row; every entry of the given outputs is written.  row_offsets NULL: fixed-size rows.
// Asynchronous on `stream`, no workspace.
int launch_hash(const ProjArgs& a, const uint8_t* rows, const int64_t* row_offsets, uint32_t seed,
                uint32_t num_parts, uint32_t* out_hashes, int32_t* out_part_ids, hipStream_t stream);

// ---- key equality of row pairs: keys_equal.hip ------------------------------------------------------
// Pair j: the key fields of row side[0].indices[j] (NULL: j) of the left batch against those of row
// side[1].indices[j] (NULL: j) of the right batch, key[k].left_slot against key[k].right_slot; the
// rules are numbered in include/fury_row.h.  out_equal[j] = 0 / 1, bit j of out_mask the same (whole
// 32-bit words, tail bits zero); either may be NULL.  Bounds = "Decode bounds" above per side, against
// that side's own total: an index outside [0, nrows), a row that fails row_ok or a key value that
// fails span_ok makes the pair unequal whatever the flags and raises kErrBounds with j.
// row_offsets NULL: fixed-size rows.  Asynchronous on `stream`, no workspace.
constexpr int kMaxEqualKeys = kMaxProjCols;
struct KeySide {
  const uint8_t* rows;
  const int64_t* row_offsets;         // NULL for fixed-size rows
  int64_t nrows;
  const int64_t* indices;             // num_pairs of them (device) or NULL
  int32_t bitmap_bytes;
  int32_t fixed_size;
};
// One key position.  Indexed wave-uniformly (scalar loads): every member >= 4 bytes, see FixedCol.
struct KeyRec {
  int32_t left_slot;                  // field index in the left schema
  int32_t right_slot;                 // ... in the right one
  int32_t kind;                       // FieldKind: kFixed / kBool / kBytes / kDecimal
  int32_t width;                      // kFixed: 1 / 2 / 4 / 8; kBool: 1; kDecimal: 16
};
struct KeysEqualArgs {
  KeySide side[2];
  KeyRec key[kMaxEqualKeys];
  int64_t num_pairs;
  int32_t nkeys;
  int32_t flags;                      // FURY_KEYS_NULL_EQUAL
  uint8_t* out_equal;
  uint32_t* out_mask;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(KeysEqualArgs) <= 4096, "KeysEqualArgs must fit the kernel argument block");
// FURY_ERR_INVALID_ARGUMENT ("batch too large") for a pair count the grid cannot index.
int launch_keys_equal(const KeysEqualArgs& a, hipStream_t stream);

// ---- group ids and distinct rows by key fields: group.hip ---------------------------------------------
// Rows of one batch (side; side.indices unused) grouped by the key fields key[k].left_slot (==
// .right_slot) under fury_row_keys_equal's rule 2 with FURY_KEYS_NULL_EQUAL; the rules are numbered
// in include/fury_row.h.  out_first[i] = the smallest row of row i's group; out_group_ids[i] = the
// groups whose first row is below out_first[i]; out_group_rows[g] = the first row of group g, -1 at
// and past the group count; *out_num_groups = the count.  All but out_first may be NULL.  hashes:
// nrows entries, equal for rows of equal keys, or NULL: launch_hash of hash_args (the keys as
// fury_row_hash builds them), seed 0, into workspace.  Bounds = "Decode bounds" above: a row that
// fails row_ok or a key value that fails span_ok is a group of its own, is never compared and raises
// kErrBounds with the row.  Asynchronous on `stream`; workspace: group_workspace_bytes.
struct GroupArgs {
  KeySide side;
  KeyRec key[kMaxEqualKeys];
  int32_t nkeys;
  int32_t pad_;
  const uint32_t* hashes;
  int64_t* out_first;
  int64_t* out_group_ids;
  int64_t* out_group_rows;
  int64_t* out_num_groups;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(GroupArgs) <= 4096, "GroupArgs must fit the kernel argument block");
int64_t group_table_slots(int64_t nrows);       // the smallest power of two >= 2 nrows
// 8 bytes per table slot (16 to 32 per row) + 4 per row, + 4 per row without caller hashes, + 8 per
// row and scan_workspace(nrows) words when any output but out_first is wanted: at most 48 per row.
int64_t group_workspace_bytes(int64_t nrows, bool own_hashes, bool numbered);
// FURY_ERR_INVALID_ARGUMENT ("batch too large") for nrows > 2^31 - 1: a slot holds 32 bits of row.
int launch_group(const GroupArgs& a, const ProjArgs* hash_args, hipStream_t stream);
// fury_row_index_build: launch_group's table, built by the same kernel, in the caller's `table` of
// `cap` == group_table_slots(nrows) slots; a.out_first optional (group_resolve), the other outputs
// unused.  nrows == 0 marks the slots empty.  Workspace: 4 bytes per row for the call's own hashes, 4
// per row of slot indices when out_first is given.
int launch_index_build(const GroupArgs& a, const ProjArgs* hash_args, uint64_t* table, int64_t cap,
                       hipStream_t stream);

// ---- hash-join probe against a built index: lookup.hip ---------------------------------------------------
// Probe row j (side[0], keys key[k].left_slot) against the rows of side[1] that `table` names (keys
// key[k].right_slot): out_rows[j] = the row of the first slot on j's walk whose hash half equals
// hashes[j] and whose row's keys equal j's under rule 2 of fury_row_keys_equal with `flags`, else -1;
// bit j of out_mask = out_rows[j] >= 0 (whole words, tail bits zero); either may be NULL.  The table
// is read, never written, and nothing in it is trusted: the rules are numbered in include/fury_row.h.
// hashes: side[0].nrows entries or NULL (launch_hash of hash_args, seed 0, into workspace).
// side[].indices unused.  Asynchronous on `stream`.
struct LookupArgs {
  KeySide side[2];                    // [0] the probe batch, [1] the build batch
  KeyRec key[kMaxEqualKeys];
  int32_t nkeys;
  int32_t flags;                      // FURY_KEYS_NULL_EQUAL
  const uint64_t* table;
  uint64_t cap;                       // group_table_slots(side[1].nrows)
  const uint32_t* hashes;
  int64_t* out_rows;
  uint32_t* out_mask;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(LookupArgs) <= 4096, "LookupArgs must fit the kernel argument block");
int launch_lookup(const LookupArgs& a, const ProjArgs* hash_args, hipStream_t stream);

// ---- the order of rows by key fields: compare.hip, order.hip ----------------------------------------------
// One key position of an ordering: KeyRec's members and what the order needs beyond equality, how the
// value bytes rank (`cls`) and the position's FURY_ORDER_* flags.  A record of its own: KeyRec and the
// argument blocks of the equality kernels stay as they are.  Indexed wave-uniformly (scalar loads).
enum OrderClass : int32_t {
  kOrdSigned = 0,                     // kFixed: two's complement at `width`; kDecimal: 128-bit
  kOrdFloat = 1,                      // kFixed, width 4 / 8: IEEE-754 totalOrder of the raw bits
  kOrdBytes = 2                       // kBytes: unsigned bytes, a prefix first; kBool: 0 / 1
};
struct OrderKey {
  int32_t left_slot;                  // field index in the left schema (order_words: the field)
  int32_t right_slot;                 // ... in the right one
  int32_t kind;                       // FieldKind: kFixed / kBool / kBytes / kDecimal
  int32_t width;                      // kFixed: 1 / 2 / 4 / 8; kBool: 1; kDecimal: 16
  int32_t cls;                        // OrderClass
  int32_t flags;                      // FURY_ORDER_DESC | FURY_ORDER_NULLS_LAST
};
// Pair j as launch_keys_equal defines it; out_cmp[j] = -1 / 0 / +1 under the order rules numbered in
// include/fury_row.h.  Bounds = "Decode bounds" above per side: an index outside [0, nrows) or a row
// that fails row_ok has every key null, a key value that fails span_ok is null, each raises kErrBounds
// with j, and the result is the rules' with those nulls.  Asynchronous on `stream`, no workspace.
struct CompareArgs {
  KeySide side[2];
  OrderKey key[kMaxEqualKeys];
  int64_t num_pairs;
  int32_t nkeys;
  int32_t pad_;
  int8_t* out_cmp;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(CompareArgs) <= 4096, "CompareArgs must fit the kernel argument block");
// FURY_ERR_INVALID_ARGUMENT ("batch too large") for a pair count the grid cannot index.
int launch_compare(const CompareArgs& a, hipStream_t stream);
// out_words[j] = the order word of chunk `chunk` of key.left_slot of row side.indices[j] (NULL: j),
// as fury_row_order_words defines it; *out_more (optional; zeroed on the stream by the launcher) = 1
// when any output row's value continues past the chunk.  Bounds as launch_compare, raising with j.
// Asynchronous on `stream`, no workspace.
struct OrderWordsArgs {
  KeySide side;
  OrderKey key;
  int64_t num_out;
  int32_t chunk;
  int32_t pad_;
  int64_t* out_words;
  uint32_t* out_more;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
int launch_order_words(const OrderWordsArgs& a, hipStream_t stream);

// ---- per-group aggregates of value fields: aggregate.hip ----------------------------------------------------
// Row i of `side` (side.indices unused) belongs to group group_ids[i] (NULL: group 0); ids outside
// [0, num_groups) take part in nothing.  For aggregate j, out[g] / out_count[g] as the rules numbered in
// include/fury_row.h define them; every entry of every given output is written once.  Bounds = "Decode
// bounds" above: a row that fails row_ok takes part in nothing, a STRING / BINARY / DECIMAL value of an
// ARG aggregate that fails span_ok is null for it, both raise kErrBounds with the row.  Asynchronous on
// `stream`; workspace: 3 words per group and aggregate.
constexpr int kMaxAggs = 16;          // FURY_AGG_MAX_AGGS
// How an aggregate folds a value into its accumulator word.
enum AggCombine : int32_t {
  kAggNone = 0,                       // COUNT: only the count word
  kAggAddInt = 1,                     // SUM of integers: 64-bit add
  kAggAddFloat = 2,                   // SUM of floats: double add
  kAggMin = 3,                        // MIN, ARGMIN of kFixed / kBool: unsigned min of order_fixed words
  kAggMax = 4,                        // MAX, ARGMAX of kFixed / kBool
  kAggArgVar = 5                      // ARGMIN / ARGMAX of kBytes / kDecimal: compare-and-swap of a row number
};
// One aggregate.  Indexed wave-uniformly (scalar loads): every member >= 4 bytes, see FixedCol.
struct AggRec {
  int32_t slot;                       // field index in the schema, -1: COUNT(*)
  int32_t op;                         // FURY_AGG_*
  int32_t kind;                       // FieldKind (kFixed where only the null bit is looked at)
  int32_t width;                      // kFixed: 1 / 2 / 4 / 8; kBool: 1; kDecimal: 16
  int32_t cls;                        // OrderClass
  int32_t combine;                    // AggCombine
  int32_t resolve;                    // ARGMIN / ARGMAX through kAggMin / kAggMax: the row-number pass
  int32_t pad_;
  uint64_t* out;
  int64_t* out_count;
};
struct AggArgs {
  KeySide side;
  AggRec rec[kMaxAggs];
  const int64_t* group_ids;
  int64_t num_groups;
  uint64_t* ws;                       // set by the launcher: [naggs][num_groups] accumulators, counts, rows
  int32_t naggs;
  int32_t pad_;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(AggArgs) <= 4096, "AggArgs must fit the kernel argument block");
// The path launch_aggregate takes: groups x aggregates up to kAggLdsCells are combined per workgroup in
// LDS (16 bytes per cell), more go to global atomics after the wave-level combine.
constexpr int64_t kAggLdsCells = 2048;
inline bool aggregate_uses_lds(int64_t num_groups, int naggs) { return num_groups * naggs <= kAggLdsCells; }
int launch_aggregate(const AggArgs& a, hipStream_t stream);

// ---- WHERE masks from conditions on the rows: predicate.hip ---------------------------------------------------
// Bit i of out_mask = row i of `side` (side.indices unused) passes the conjunction of clauses that
// term[0 .. nterms) spell, as the rules numbered in include/fury_row.h define it; whole 32-bit words,
// tail bits zero.  row_mask (optional, may be out_mask itself): a row whose bit is 0 is not read and
// fails.  *out_count (optional; zeroed on the stream by the launcher) = the bits set.  Bounds = "Decode
// bounds" above: a row that fails row_ok has every field null, a STRING / BINARY / DECIMAL value that
// fails span_ok is null, both raise kErrBounds with the row.  Asynchronous on `stream`, no workspace.
constexpr int kMaxPredTerms = 32;         // FURY_PRED_MAX_TERMS
constexpr int kPredPoolWords = 256;       // FURY_PRED_MAX_LITERAL_BYTES / 8
// One term.  Indexed wave-uniformly (scalar loads): every member >= 4 bytes, see FixedCol.
struct PredTerm {
  int32_t slot;                       // field index in the schema
  int32_t kind;                       // FieldKind: kFixed / kBool / kBytes / kDecimal
  int32_t width;                      // kFixed: 1 / 2 / 4 / 8; kBool: 1; kDecimal: 16
  int32_t cls;                        // OrderClass
  int32_t op;                         // FURY_PRED_*
  int32_t flags;                      // FURY_PRED_NOT | FURY_PRED_OR
  int32_t lit_word;                   // the literal's first word in PredArgs.pool
  int32_t lit_len;                    // its bytes; the words hold zeros past them
};
struct PredArgs {
  KeySide side;
  PredTerm term[kMaxPredTerms];
  uint64_t pool[kPredPoolWords];      // every literal, each padded with zeros to whole 8-byte words
  int32_t nterms;
  int32_t pad_;
  const uint32_t* row_mask;
  uint32_t* out_mask;
  unsigned long long* out_count;
  uint32_t* err;                      // the launch stream's device error slot or NULL
};
static_assert(sizeof(PredArgs) <= 4096, "PredArgs must fit the kernel argument block");
// FURY_ERR_INVALID_ARGUMENT ("batch too large") for a row count the grid cannot index.
int launch_predicate(const PredArgs& a, hipStream_t stream);

// ---- nested values as batches: extract.hip -------------------------------------------------------
// BinaryRow.getStruct / getArray / getMap over a batch, along a path of struct slots: the bytes each
// row's slot points at, unchanged, packed into a new batch (compact, in row order, shaped like
// launch_filter's outputs).  Level k of the path is a struct of nfields[k] fields whose slot slot[k]
// is followed; the host resolves both from the schema (resolve_extract_path, schema.cpp).  Bounds =
// "Decode bounds" above, per level: the struct's header [base, base + bitmap + 8 nfields) lies in
// [0, total) at an 8-byte aligned base, the slot's offset and size are >= 0 and multiples of 8, the
// value's span lies in [0, total) and is no shorter than `need` of the next level (the next struct's
// header; the last value: min_size, and exactly min_size when `exact`).  A value that fails is null
// and raises kErrBounds with its source row.  Asynchronous on `stream`.
struct ExtractArgs {
  const uint8_t* rows;
  const int64_t* row_offsets;
  int64_t nrows;
  uint8_t* out;                       // NULL: the measure form
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries
  int64_t* out_count;
  int64_t* out_indices;               // optional, nrows entries
  uint32_t* out_validity;             // optional, (nrows + 31) / 32 words
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t nlevels;                    // 1 .. kMaxNestLevels
  int32_t min_size;                   // STRUCT: the child's fixed_size; LIST / MAP: 8
  int32_t exact;                      // an is_fixed child struct: size == min_size
  int32_t pad_;
  int32_t nfields[64];                // kMaxNestLevels
  int32_t slot[64];
};
int launch_extract(const ExtractArgs& a, hipStream_t stream);

// ---- list and map elements as batches: explode.hip -----------------------------------------------
// BinaryArray.getStruct / getArray / getMap (ordinal) and BinaryMap.keyArray() / valueArray() over a
// batch: the bytes every non-null element slot of the chosen array points at, unchanged, packed into
// a new batch in (row, ordinal) order.  The array of row r is the LIST / MAP value the path reaches
// (the members the walk reads are ExtractArgs', min_size = 8) or, for a collection schema (nlevels
// 0), the batch entry itself; is_map / side pick the key or the value array of a BinaryMap.  Bounds =
// "Decode bounds" above: the array's header and slot region [A, A + 8 + bitmap + 8 n) lies inside the
// array's span, which lies in [0, total); an element's span is relative to A, its offset and size are
// >= 0 and multiples of 8, it lies in [0, total) and is no shorter than elem_min (exactly elem_min
// when elem_exact).  A row or element that fails is null and raises kErrBounds with the source row.
// Elements at or past elem_cap are neither produced nor counted.  Asynchronous on `stream`.
struct ExplodeArgs {
  const uint8_t* rows;
  const int64_t* row_offsets;
  int64_t nrows;
  int64_t* out_list_offsets;          // nrows + 1 entries: the Arrow list offsets of the column
  uint32_t* out_entry_validity;       // optional, (nrows + 31) / 32 words
  int64_t elem_cap;
  uint8_t* out;                       // NULL: the measure form
  int64_t cap;
  int64_t* out_offsets;               // elem_cap + 1 entries; NULL: the count form
  int64_t* out_count;
  int64_t* out_parents;               // optional, elem_cap entries
  int32_t* out_ordinals;              // optional, elem_cap entries
  uint32_t* out_validity;             // optional, (elem_cap + 31) / 32 words
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t nlevels;                    // 0 (collection schema) .. kMaxNestLevels
  int32_t min_size;                   // 8: the least LIST / MAP value
  int32_t exact;                      // 0
  int32_t is_map;                     // the value is a BinaryMap [int64 keyArrayBytes][keys][values]
  int32_t side;                       // 0: the LIST / the key array; 1: the value array
  int32_t elem_min;                   // STRUCT element: its fixed_size; LIST / MAP element: 8
  int32_t elem_exact;                 // an is_fixed element struct: size == elem_min
  int32_t pad_;
  int32_t nfields[64];                // kMaxNestLevels
  int32_t slot[64];
};
int launch_explode(const ExplodeArgs& a, hipStream_t stream);

// ---- a subset of a row's fields, as rows: select.hip ---------------------------------------------
// BinaryRow's getters feeding a fresh BinaryRowWriter of the selected schema, over a batch: output
// row r holds field fields[j] of source row r in slot j.  The selection travels as a table of int32
// words: 4 per selected field j -- [4 j] source slot, [4 j + 1] width (1 / 2 / 4 / 8 bytes, kSelBool,
// kSelVar), [4 j + 2] the least size of a variable-length value | kSelMod8 (size % 8 == 0) |
// kSelExact (size == least), [4 j + 3] its index among the selected variable-length fields or -1 --
// followed by one word per variable-length field: its j.  Up to kSelArgWords words sit in the
// argument block; a longer table is uploaded (SelectArgs.tab).  Bounds = "Decode bounds" above: a row
// whose header leaves [0, total), starts off an 8-byte boundary or is shorter than fixed_size comes
// out all null; a value whose slot is negative, misaligned, leaves [0, total) or misses its size rule
// comes out null; both raise kErrBounds with the row.  out NULL: the measure form; bytes at or past
// `cap` are never written while out_offsets is always complete.  Asynchronous on `stream`.
constexpr int kSelArgWords = 320;     // 64 selected fields, every one variable-length
constexpr int32_t kSelBool = 0, kSelVar = -1;
constexpr int32_t kSelMod8 = 1 << 30, kSelExact = 1 << 29, kSelNeed = kSelExact - 1;
struct SelectArgs {
  int32_t tabi[kSelArgWords];
  const int32_t* tab;                 // device table when it outgrows tabi, else NULL
  const uint8_t* rows;
  const int64_t* row_offsets;         // NULL: fixed-size source rows (row r at r * fixed_size)
  int64_t nrows;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries; optional when the selection is fixed-width
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t bitmap_bytes, fixed_size;   // source rows
  int32_t nsel, nvar;                 // selected fields, variable-length ones among them
  int32_t out_bitmap_bytes, out_fixed_size;
};
// `table`: the nwords words described above (host); copied into the argument block or uploaded.
int launch_select(const SelectArgs& a, const int32_t* table, int nwords, hipStream_t stream);

// ---- the fields of several row batches joined row by row: zip.hip ---------------------------------
// fury_row_select from several sources: output row r holds, in slot j, field picks[j] of row r of its
// source.  The table has 5 int32 words per pick j -- [5 j .. 5 j + 3] as in the selection table above,
// [5 j + 4] the source index -- followed by one word per variable-length pick: its j.  Up to
// kZipArgWords words sit in the argument block; a longer table is uploaded (ZipArgs.tab).  Bounds =
// "Decode bounds" above, per source s with its own total_s: a row of s that fails the row check nulls
// the picks of s alone, a failed value comes out null, both raise kErrBounds with the row; nothing
// outside [0, total_s) of source s is read and a source outside `used` is never read.  out, cap and
// out_offsets as in SelectArgs.  Asynchronous on `stream`.
constexpr int kZipMaxSources = 4;     // FURY_ZIP_MAX_SOURCES
constexpr int kZipArgWords = 384;     // 64 picks, every one variable-length
struct ZipSource {
  const uint8_t* rows;
  const int64_t* row_offsets;         // NULL: fixed-size rows (row r at r * fixed_size)
  int32_t bitmap_bytes, fixed_size;
};
struct ZipArgs {
  int32_t tabi[kZipArgWords];
  const int32_t* tab;                 // device table when it outgrows tabi, else NULL
  ZipSource src[kZipMaxSources];
  int64_t nrows;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries; optional when every pick is fixed-width
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t nsel, nvar;                 // picks, variable-length ones among them
  int32_t out_bitmap_bytes, out_fixed_size;
  uint32_t used;                      // bit s: some pick names source s
  int32_t pad_;
};
static_assert(sizeof(ZipArgs) <= 4096, "ZipArgs must fit the kernel argument block");
// `table`: the nwords words described above (host); copied into the argument block or uploaded.
int launch_zip(const ZipArgs& a, const int32_t* table, int nwords, hipStream_t stream);

// ---- element rows back into lists, nested values back into rows: implode.hip ---------------------
// BinaryArrayWriter.reset(n) + write(ordinal, BinaryRow | BinaryArray | BinaryMap) over a batch, and a
// one-field BinaryRowWriter around the array (prefix 16) or around a single value (wrap): the inverses
// of launch_explode and launch_extract.  values / value_offsets: a compact batch of num_values values
// (value_offsets[num_values] = VT); a present element -- elem_validity bit 1, NULL: all -- takes the
// value whose index is the rank of its bit.  Value check: 0 <= start <= end <= VT, start and size
// multiples of 8, size >= least, index < num_values; a value that fails makes its element (wrap: its
// row) null and raises kErrBounds with the output row, unless that row is null by entry_validity.
// Row r owns elements [list_offsets[r], list_offsets[r + 1]), which must lie in [0, num_elements] in
// order and number at most (INT32_MAX - 15) / 8, and its array (plus prefix) must not exceed INT32_MAX
// - 7: otherwise the row is null (prefix 16) or an empty array (prefix 0) and raises kErrBounds.  wrap:
// list_offsets and entry_validity are NULL, num_elements = nrows, row r owns element r and has no array
// header.  Nothing outside [0, VT) of values is read; out NULL: the measure form; bytes at or past
// `cap` are never written while out_offsets is always complete.  Asynchronous on `stream`.
struct ImplodeArgs {
  const uint8_t* values;
  const int64_t* value_offsets;       // num_values + 1 entries
  int64_t num_values;
  const int64_t* list_offsets;        // nrows + 1 entries; wrap: NULL
  int64_t nrows;
  const uint32_t* entry_validity;     // optional, rows form only
  const uint32_t* elem_validity;      // optional; wrap: the rows' validity
  int64_t num_elements;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t least;                      // STRUCT: the child's fixed_size; LIST / MAP: 8
  int32_t prefix;                     // 16: rows form and wrap ([bitmap][slot]); 0: collection form
  int32_t wrap;
  int32_t pad_;
};
int launch_implode(const ImplodeArgs& a, hipStream_t stream);

// ---- maps as key / value arrays and back: map.hip --------------------------------------------------
// BinaryMap.keyArray() / valueArray() over a batch: the map of row r is the MAP value the path reaches
// (the members the walk reads are ExtractArgs', min_size = 8) or, for a collection schema (nlevels 0),
// the batch entry itself; its two BinaryArrays go, unchanged, into two compact batches shaped like
// launch_extract's outputs with one shared count / indices / validity.  Bounds = "Decode bounds"
// above: the map header, keyArrayBytes (>= 0, a multiple of 8, 8 + kb <= size), both arrays >= 8 bytes,
// equal element counts n >= 0 and, per side, 8 + bitmap + round8(n * width) inside the array; nothing
// below the two array headers is read.  A map that fails is null and raises kErrBounds with its source
// row (kErrCounts set in the location when the counts differ).  A side whose out_offsets is NULL is
// skipped; out NULL: the measure form.  Asynchronous on `stream`.
constexpr uint64_t kErrCounts = 1ull << 62;       // in a kErrBounds row location: key / value counts differ
struct MapSide {
  uint8_t* out;                       // NULL: the measure form
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries; NULL: the side is skipped
  int64_t width;                      // slot width of the side's elements (8: variable-length / nested)
};
struct MapSplitArgs {
  const uint8_t* rows;
  const int64_t* row_offsets;
  int64_t nrows;
  MapSide keys, vals;
  int64_t* out_count;
  int64_t* out_indices;               // optional, nrows entries
  uint32_t* out_validity;             // optional, (nrows + 31) / 32 words
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t nlevels;                    // 0 (collection schema) .. kMaxNestLevels
  int32_t min_size;                   // 8
  int32_t exact;                      // 0
  int32_t pad_;
  int32_t nfields[64];                // kMaxNestLevels
  int32_t slot[64];
};
int launch_map_split(const MapSplitArgs& a, hipStream_t stream);
// The constructor BinaryMap(keys, values, field) / serializeForMap over a batch: [int64 key array
// bytes][key array][value array], inside a one-field row (prefix 16) or as the map itself (prefix 0).
// keys / values: two compact batches of num_values entries each; a present row -- validity bit 1, NULL:
// all -- takes entry v of both, v the rank of its bit.  Each entry passes ImplodeArgs' value check with
// least 8 against its own buffer's length, the int64 counts at the two starts are equal and in [0,
// (INT32_MAX - 15) / 8], and prefix + 8 + both sizes <= INT32_MAX - 7: otherwise the row is null (prefix
// 16) or the empty map (prefix 0) and raises kErrBounds.  Nothing outside the two buffers' lengths is
// read; out NULL: the measure form; bytes at or past `cap` are never written while out_offsets is
// always complete.  Asynchronous on `stream`.
struct MapJoinArgs {
  const uint8_t* keys;
  const int64_t* key_offsets;         // num_values + 1 entries
  const uint8_t* values;
  const int64_t* value_offsets;       // num_values + 1 entries
  int64_t num_values;
  const uint32_t* validity;           // optional, rows form only
  int64_t nrows;
  uint8_t* out;
  int64_t cap;
  int64_t* out_offsets;               // nrows + 1 entries
  uint32_t* err;                      // the launch stream's device error slot or NULL
  int32_t prefix;                     // 16: rows form ([bitmap][slot]); 0: collection form
  int32_t pad_;
};
int launch_map_join(const MapJoinArgs& a, hipStream_t stream);

// ---- generic (nested) schema engine: generic.hip --------------------------------------------
constexpr int kGenMaxNodes = 48;      // schema tree nodes in the argument block
constexpr int kGenMaxWideNodes = 4096;  // beyond 48: node table uploaded per call (GenArgs.tab)

struct GenNode {
  const uint8_t* values;   // fixed values / bytes payload / decimal values (bool: bit-packed)
  uint8_t* validity;       // Arrow validity or NULL
  int32_t* offsets;        // STRING/BINARY byte offsets, LIST/MAP entry offsets
  int32_t type;            // fury_type_id
  int32_t first_child;     // node index of the first child (children are contiguous)
  int32_t num_children;
  int32_t row_aligned;     // reached from the top through STRUCTs only: Arrow entry index = row
};

struct GenArgs {
  GenNode node[kGenMaxNodes];
  int32_t nnodes;
  int32_t ntop;            // top-level fields = nodes [0, ntop)
  int64_t nrows;
  int32_t* err;            // optional device flag (never NULL when set by the host)
  int32_t root;            // fury_schema.root: 0 rows, 1 top-level arrays, 2 top-level maps
  int32_t pad_;
  const GenNode* tab;      // device node table for > kGenMaxNodes nodes, else NULL
  const GenNode* htab;     // its host copy (launchers only; never read on the device)
};

// Nested encode (rowenc.hip): measure pass (row sizes) / build pass at the given row offsets, for
// any nesting depth (kRowEncMaxDepth levels inlined, deeper ones on an explicit stack).
int launch_gen_measure(const GenArgs& g, int64_t* sizes, hipStream_t stream);
int launch_gen_encode(const GenArgs& g, const int64_t* offs, uint8_t* rows, int64_t cap,
                      hipStream_t stream);
constexpr int kRowEncMaxDepth = 5;
constexpr int kMaxNestLevels = 64;     // schema nesting limit (schema.cpp)
int rowenc_launch(const GenArgs& g, const int64_t* offs, int64_t* sizes, uint8_t* rows,
                  int64_t cap, hipStream_t stream);
// Level-by-level nested decode (levels.hip): prepare = per-level count / scan / expand passes
// (totals[2 i] entries, totals[2 i + 1] payload bytes of node i), execute = one write pass into
// the outputs of gen_args' node table.
struct LvPlan;
int lv_prepare(const fury_schema* s, const uint8_t* rows, const int64_t* offs, int64_t nrows,
               hipStream_t hs, LvPlan** out, std::vector<int64_t>* totals);
int lv_execute(const LvPlan* p, const GenNode* outs, const uint8_t* rows, const int64_t* offs,
               hipStream_t hs);
void lv_free(LvPlan* p);
// The pinned landing buffer of a prepare's totals (n words or more): one per host thread, kept.
int64_t* pinned_totals(size_t n);
// Row-walk nested decode (tree.hip / walk.hip): prepare = pass 1 + tile scan + one host sync (*out NULL:
// the batch needs the level engine above), execute = pass 2 into gen_args' node table.
struct TreePlan;
// batch_bytes: offs[nrows] where the caller has read it, -1 otherwise.
int tree_prepare(const fury_schema* s, const uint8_t* rows, const int64_t* offs, int64_t nrows,
                 int64_t batch_bytes, hipStream_t hs, TreePlan** out, std::vector<int64_t>* totals);
int tree_execute(const TreePlan* p, const GenNode* outs, const uint8_t* rows, const int64_t* offs,
                 const std::vector<int64_t>& totals, hipStream_t hs);
void tree_free(TreePlan* p);
int64_t bfs_fallbacks();             // tile-BFS batches whose tiles overflowed the arena
int set_tree_debug(int on);          // tuning "tree_debug": phase accumulators on / off
uint64_t* tree_debug_buffer();
// Exclusive scan of s[0..n) with the total stored to *total (device); ws: scan_workspace(n).
int64_t scan_workspace(int64_t n);
void device_scan(int64_t* s, int64_t n, int64_t* total, int64_t* ws, hipStream_t stream);

int launch_frame_rows(const uint8_t* rows, const int64_t* row_offsets, int64_t nrows,
                      int64_t fixed_size, int64_t schema_hash, uint8_t* out,
                      int64_t* frame_offsets, hipStream_t stream);
int64_t unframe_walk_count();        // streams the sequential walk has parsed (tuning "unframe")
void keep_pool(int device);      // hostpath.cpp: keep freed stream-pool memory pooled
int64_t host_direct_count();     // hostpath.cpp: host calls run directly on pinned memory
int64_t unframe_repair_count();      // streams parsed by the parallel repair (pointer doubling)
int launch_unframe_rows(const uint8_t* in, int64_t in_len, int64_t nrows, int64_t schema_hash,
                        uint8_t* rows_out, int64_t* row_offsets, hipStream_t stream);

// Arrow IPC (ipc.hip): encapsulated Schema message (host bytes) and RecordBatch message of
// device columns written to device memory (out == NULL: *len only).
int type_width_of(int32_t type_id);
int ipc_schema_message(const fury_schema* s, std::vector<uint8_t>* out);
int ipc_record_batch(const fury_schema* s, const fury_column* cols, int64_t n, uint8_t* out,
                     int64_t cap, int64_t* len, hipStream_t stream);

// fury_decode_prepare into a plan the caller has made (capi.cpp): the host flavour's plan already
// owns its stream and staged rows.
int decode_prepare(fury_decode_plan* p, const fury_schema* s, const void* rows,
                   const int64_t* row_offsets, int64_t nrows, int64_t* node_entries,
                   int64_t* node_bytes, hipStream_t hs);

}  // namespace fury

// Decode plan of the two-step (nested) decode, device and host-memory flavours.  It owns its
// parts; the destructor (capi.cpp) gives them back in this order: the engine state, the staged
// rows, the private stream's error slot and the stream.
struct fury_decode_plan {
  template <class T>
  using EnginePtr = std::unique_ptr<T, void (*)(T*)>;
  const fury_schema* schema = nullptr;
  const uint8_t* rows = nullptr;
  const int64_t* offs = nullptr;
  int64_t nrows = 0;
  // at most one engine state is set; none when nrows = 0
  EnginePtr<fury::LvPlan> lv{nullptr, fury::lv_free};        // level-by-level engine (levels.hip)
  EnginePtr<fury::TreePlan> tree{nullptr, fury::tree_free};  // row walk / tile BFS (tree.hip)
  EnginePtr<fury::WidePlan> wide{nullptr, fury::wide_free};  // flat schemas of 17-256 fields (wide.hip)
  std::vector<int64_t> totals;     // per node: Arrow entries, payload bytes
  fury::DevBlock owned;            // host flavour: the staged rows + offsets
  hipStream_t owned_stream = nullptr;  // host flavour: its stream
  int32_t device = 0;
  ~fury_decode_plan();
};
