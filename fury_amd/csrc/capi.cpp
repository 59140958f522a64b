// capi.cpp — the extern "C" device entry points of include/fury_row.h: argument checks, then
// dispatch to the fixed-width tile kernels (fixed.hip) or the variable-length kernels (var.hip).
// Error statuses mirror the reference's exceptions (see fury_status).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

#include "internal.h"
#include "kernels.h"
#include "tuning.h"

namespace fury {

int check_hip(int hip_status, const char* what) {
  if (hip_status == hipSuccess) return FURY_OK;
  return set_error(FURY_ERR_DEVICE, std::string(what) + ": " +
                                        hipGetErrorString(static_cast<hipError_t>(hip_status)));
}

// Device error words (kernels.h): one slot of kErrWords words per stream, in host-pinned mapped
// memory.  A kernel raises into the slot of the stream it was launched on, and a call takes (reads
// and clears) only the slot of its own stream, so a malformed decode on one stream is never
// reported by -- or swallowed into -- an unrelated call on another stream / thread.
// The legacy null stream and hipStreamPerThread are keyed per host thread (two keys per thread,
// released when the thread exits).  Slots are assigned on first launch and go back to a free list
// when their stream is released: by the library when it destroys a stream it created (decode
// plans, host-path plans), by the caller through fury_stream_release (which synchronises the
// stream first, the null stream and hipStreamPerThread included) before it destroys one of its
// own.  A thread that exits makes no HIP call, so work it launched on its null-stream /
// per-thread keys may still be running: those slots go to a QUARANTINE, not the free list, and
// become free only after a device synchronisation that covers them (when the free slots run out,
// or fury_trim_workspace) -- a late error lands in the quarantined slot and is dropped there, never
// on an unrelated stream.  A call that needs a slot when all kErrSlots are held fails
// with FURY_ERR_DEVICE -- slots are never shared, so an error is reported on its own stream or not
// at all.
namespace {
constexpr int kErrSlots = 1024;
uint32_t* g_err_host = nullptr;     // host view of the slots
uint32_t* g_err_dev = nullptr;      // the same memory as kernels address it
std::once_flag g_err_once;
std::mutex g_slot_mu;
std::unordered_map<uintptr_t, int> g_slot_of;
std::vector<int> g_slot_free;       // released slots (words cleared)
std::vector<int> g_slot_quarantine; // released at thread exit, their work maybe still running
int g_slot_next = 0;                // slots [0, g_slot_next) have been handed out at least once

void release_key(uintptr_t k, bool quarantine = false);

// Per-thread keys of the null stream and of hipStreamPerThread (odd: never a stream handle, which
// is aligned); their slots are quarantined when the thread exits.
std::atomic<int> g_thread_key_exits{0};   // ThreadKeys destructors run (diagnostics)
struct ThreadKeys {
  char null_key = 0, per_thread_key = 0;
  ~ThreadKeys() {
    g_thread_key_exits.fetch_add(1);
    release_key(reinterpret_cast<uintptr_t>(&null_key) | 1, true);
    release_key(reinterpret_cast<uintptr_t>(&per_thread_key) | 1, true);
  }
};

uintptr_t stream_key(hipStream_t s) {
  if (s && s != hipStreamPerThread) return reinterpret_cast<uintptr_t>(s);
  thread_local ThreadKeys keys;
  return reinterpret_cast<uintptr_t>(s ? &keys.per_thread_key : &keys.null_key) | 1;
}

void init_err() {
  std::call_once(g_err_once, [] {
    void* p = nullptr;
    const size_t bytes = size_t(kErrSlots) * kErrWords * 4;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
      (void)hipHostFree(p);
      return;
    }
    std::memset(p, 0, bytes);
    g_err_host = static_cast<uint32_t*>(p);
    g_err_dev = static_cast<uint32_t*>(d);
  });
}

void clear_slot_words(int slot);
int assign_slot_locked(uintptr_t k);

// Every device synchronised: the quarantined slots' kernels have finished, so their words can be
// cleared (late errors dropped) and the slots reused.  Called without g_slot_mu held.
void drain_quarantine() {
  {
    std::lock_guard<std::mutex> lock(g_slot_mu);
    if (g_slot_quarantine.empty()) return;
  }
  int n = 0, cur = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return;
  (void)hipGetDevice(&cur);
  std::vector<int> q;
  {
    std::lock_guard<std::mutex> lock(g_slot_mu);
    q.swap(g_slot_quarantine);       // slots quarantined after this point wait for the next drain
  }
  for (int d = 0; d < n; d++)
    if (hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
  (void)hipSetDevice(cur);
  std::lock_guard<std::mutex> lock(g_slot_mu);
  for (int slot : q) {
    clear_slot_words(slot);
    g_slot_free.push_back(slot);
  }
}

// The slot of stream key k: its own, else a free or never-used one; when none is left, the
// quarantine is drained first (-1: all kErrSlots held by live streams).
// `assign` false: lookup only (a stream that never launched has nothing to report).
int error_slot(uintptr_t k, bool assign) {
  {
    std::lock_guard<std::mutex> lock(g_slot_mu);
    auto it = g_slot_of.find(k);
    if (it != g_slot_of.end()) return it->second;
    if (!assign) return -1;
    if (g_slot_free.empty() && g_slot_next >= kErrSlots && !g_slot_quarantine.empty()) {
      // fall through to the drain below (it synchronises: no lock held)
    } else {
      return assign_slot_locked(k);
    }
  }
  drain_quarantine();
  std::lock_guard<std::mutex> lock(g_slot_mu);
  auto it = g_slot_of.find(k);
  if (it != g_slot_of.end()) return it->second;
  return assign_slot_locked(k);
}

std::atomic<uintptr_t> g_last_assigned_key{0};   // diagnostics ("err_slot_last_key")

int assign_slot_locked(uintptr_t k) {
  g_last_assigned_key = k;
  int slot = -1;
  if (!g_slot_free.empty()) {
    slot = g_slot_free.back();
    g_slot_free.pop_back();
  } else if (g_slot_next < kErrSlots) {
    slot = g_slot_next++;
  } else {
    return -1;
  }
  g_slot_of.emplace(k, slot);
  return slot;
}

std::atomic<int64_t> g_err_dropped{0};   // look-back flags cleared by a release, never taken

void clear_slot_words(int slot) {
  if (!g_err_host) return;
  uint32_t* w = g_err_host + size_t(kErrWords) * slot;
  if (__atomic_exchange_n(w + kErrLookBack, 0u, __ATOMIC_ACQ_REL)) g_err_dropped.fetch_add(1);
  for (int i = 0; i < kErrWords; i++) __atomic_store_n(w + i, 0u, __ATOMIC_RELEASE);
}

void release_key(uintptr_t k, bool quarantine) {
  std::lock_guard<std::mutex> lock(g_slot_mu);
  auto it = g_slot_of.find(k);
  if (it == g_slot_of.end()) return;
  const int slot = it->second;
  g_slot_of.erase(it);
  if (quarantine) {
    g_slot_quarantine.push_back(slot);
    return;
  }
  clear_slot_words(slot);
  g_slot_free.push_back(slot);
}
}  // namespace

int thread_key_exits() { return g_thread_key_exits.load(); }
// 0: a stream handle, 1: a thread's null-stream key, 2: a thread's hipStreamPerThread key
int last_assigned_key_kind() {
  const uintptr_t k = g_last_assigned_key.load();
  if (!(k & 1)) return 0;
  return 1;   // (both thread keys are odd; which one is not distinguished)
}
int error_slots_quarantined() {
  std::lock_guard<std::mutex> lock(g_slot_mu);
  return static_cast<int>(g_slot_quarantine.size());
}
void drain_error_quarantine() { drain_quarantine(); }

int device_error_word(hipStream_t stream, uint32_t** out) {
  *out = nullptr;
  init_err();
  if (!g_err_dev) return FURY_OK;     // no mapped memory: kernels run without error reporting
  const int slot = error_slot(stream_key(stream), true);
  if (slot < 0)
    return set_error(FURY_ERR_DEVICE,
                     "device error slots exhausted: " + std::to_string(kErrSlots) +
                         " streams hold one; call fury_stream_release(stream) before destroying a "
                         "stream passed to this library");
  *out = g_err_dev + size_t(kErrWords) * slot;
  return FURY_OK;
}

// Forgets `stream`'s slot after the work on it has finished (its pending errors are dropped);
// `sync` false: the caller knows the stream is idle (thread exit: no HIP call).
void release_error_slot(hipStream_t stream, bool sync) {
  if (sync) (void)hipStreamSynchronize(stream);   // NULL / hipStreamPerThread: this thread's
  release_key(stream_key(stream));
}

int error_slots_in_use() {
  std::lock_guard<std::mutex> lock(g_slot_mu);
  return static_cast<int>(g_slot_of.size());
}

std::atomic<int64_t> g_err_taken{0};

int64_t device_error_count() {
  int64_t pending = 0;
  if (g_err_host) {
    std::lock_guard<std::mutex> lock(g_slot_mu);
    for (int i = 0; i < g_slot_next; i++)
      pending += __atomic_load_n(g_err_host + size_t(kErrWords) * i + kErrLookBack, __ATOMIC_ACQUIRE) ? 1 : 0;
  }
  return g_err_taken.load() + g_err_dropped.load() + pending;
}

// Where a kernel found the problem: a row index, or (bit 63 set) a nested schema node and Arrow
// entry (err_where_entry).
static std::string where_text(uint64_t w) {
  if (!(w >> 63)) return "row " + std::to_string(w);
  if ((w >> 62) & 1)           // err_where_tile: a nested entry of the tile that starts at a row
    return "schema node " + std::to_string((w >> 40) & 0x3fffff) + " in the rows from row " +
           std::to_string(w & ((1ull << 40) - 1));
  return "schema node " + std::to_string((w >> 40) & 0x7fffff) + ", Arrow entry " +
         std::to_string(w & ((1ull << 40) - 1));
}

// Takes one flag of the slot: the flag is exchanged for 0 first, then its location word is read
// and cleared (raise_at stores the location before it releases the flag).
static bool take_flag(uint32_t* w, int flag, uint64_t* where) {
  if (!__atomic_exchange_n(w + flag, 0u, __ATOMIC_ACQ_REL)) return false;
  if (where) *where = __atomic_exchange_n(reinterpret_cast<uint64_t*>(w + flag + 2), 0ull, __ATOMIC_ACQ_REL);
  return true;
}

int take_device_error(hipStream_t stream) {
  if (!g_err_host) return FURY_OK;
  const int slot = error_slot(stream_key(stream), false);
  if (slot < 0) return FURY_OK;       // nothing was ever launched on this stream
  uint32_t* w = g_err_host + size_t(kErrWords) * slot;
  uint64_t oob_at = 0, map_at = 0;
  const bool lb = take_flag(w, kErrLookBack, nullptr);
  const bool oob = take_flag(w, kErrBounds, &oob_at);
  const bool map = take_flag(w, kErrMapCount, &map_at);
  uint64_t deep_at = 0, budget_at = 0;
  const bool deep = take_flag(w, kErrTooDeep, &deep_at);
  const bool budget = take_flag(w, kErrBudget, &budget_at);
  uint64_t internal_at = 0;
  const bool internal = take_flag(w, kErrInternal, &internal_at);
  if (!lb && !oob && !map && !deep && !budget && !internal) return FURY_OK;
  if (internal)
    return set_error(FURY_ERR_DEVICE, "decode: the tile from " + where_text(internal_at) +
                                          " outgrew its on-chip plan (internal error); the outputs "
                                          "of that call are invalid");
  if (lb) {
    g_err_taken.fetch_add(1);
    return set_error(FURY_ERR_DEVICE,
                     "an earlier asynchronous launch failed on the device (a decoupled look-back "
                     "gave up waiting): the outputs of that call are invalid");
  }
  if (oob && !(oob_at >> 63) && (oob_at & kErrCounts))     // fury_row_map_split / fury_row_map_join
    return set_error(FURY_ERR_OUT_OF_BOUNDS,
                     "decode: " + where_text(oob_at & ~kErrCounts) +
                         " has map key and value arrays of different element counts "
                         "(BinaryMap.pointTo); the outputs of that call are invalid");
  if (oob)
    return set_error(FURY_ERR_OUT_OF_BOUNDS,
                     "decode: " + where_text(oob_at) +
                         " has a variable-length value, array or map header outside the batch's "
                         "row bytes (MemoryBuffer bounds check); the outputs of that call are "
                         "invalid");
  if (deep)
    return set_error(FURY_ERR_UNSUPPORTED,
                     "encode: " + where_text(deep_at) +
                         " is too large to assemble on chip and the schema is nested deeper than "
                         "the row interpreter reaches; the rows of that call are invalid");
  if (map)
    return set_error(FURY_ERR_UNSUPPORTED,
                     "decode: " + where_text(map_at) +
                         ": map key and value arrays have different element counts "
                         "(BinaryMap.pointTo); the outputs of that call are invalid");
  return budget_error(where_text(budget_at));
}

namespace {
std::atomic<int64_t> g_budget_errors{0};
}
int budget_error(const std::string& where) {
  g_budget_errors.fetch_add(1);
  return set_error(FURY_ERR_UNSUPPORTED,
                   "decode budget: " + where +
                       ": slots alias other bytes of the batch so that decoding would visit more "
                       "items than the rows hold (a device limit, not a reference exception: "
                       "the reference would decode such rows); the outputs of that call are "
                       "invalid");
}
int64_t budget_errors() { return g_budget_errors.load(); }

// Pinned staging ring for per-call column tables: the host table is copied into the ring, then
// DMA-ed to a stream-ordered device allocation on the caller's stream (no host synchronisation);
// a ring region is reused only after the event of the copy that read it has completed.
namespace {
std::mutex g_ring_mu;
uint8_t* g_ring = nullptr;
size_t g_ring_head = 0;
constexpr size_t kRingBytes = 4u << 20;
struct RingUse {
  size_t off, bytes;
  hipEvent_t ev;
};
std::vector<RingUse> g_ring_pending;
}  // namespace

// ---- device workspace cache -------------------------------------------------------------------
// Per-call workspaces (scan scratch, column tables, decode plans) come from size classes cached
// per device instead of hipMallocAsync / hipFreeAsync: on the box hipFreeAsync took ~110 us of
// host time per call (HIP API trace of scripts/ab_generic.py), more than most of the kernels it
// serves.  A freed block records an event on its stream; its next user's stream waits for that
// event on the device (hipStreamWaitEvent, no host sync) -- also when the handles are equal,
// since a destroyed stream's handle can be reused.  Classes: powers of two up to 64 MB, 2 MB
// multiples above (a 5.8 GB plan array is not rounded to 8 GB).  Cached free bytes are capped
// (kCacheCap, 2 GB: the cache exists for per-call workspaces, not for whole batches); beyond that
// blocks go back to the pool.  An allocation that fails releases every idle cached block and
// trims the stream pool, then retries once; fury_trim_workspace() does the same on request.
namespace {
struct CacheBlock {
  void* p;
  size_t cls;
  int device;
  hipEvent_t ev;
};
std::mutex g_cache_mu;
std::vector<CacheBlock> g_cache_free;
std::unordered_map<void*, std::pair<size_t, int>> g_cache_live;
size_t g_cache_bytes = 0;                     // bytes in g_cache_free
constexpr size_t kCacheCap = size_t(2) << 30;

size_t size_class(int64_t bytes) {
  const size_t b = static_cast<size_t>(bytes > 0 ? bytes : 1);
  constexpr size_t kBig = size_t(64) << 20, kStep = size_t(2) << 20;
  if (b > kBig) return (b + kStep - 1) / kStep * kStep;
  size_t cls = 4096;
  while (cls < b) cls <<= 1;
  return cls;
}

// Frees every idle cached block of `device` (after the work that last used it) and trims that
// device's stream pool.  Returns the bytes released.
size_t release_cached(int device) {
  std::vector<CacheBlock> drop;
  {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (size_t i = 0; i < g_cache_free.size();) {
      if (g_cache_free[i].device == device) {
        drop.push_back(g_cache_free[i]);
        g_cache_bytes -= g_cache_free[i].cls;
        g_cache_free[i] = g_cache_free.back();
        g_cache_free.pop_back();
      } else {
        i++;
      }
    }
  }
  size_t bytes = 0;
  for (CacheBlock& b : drop) {
    (void)hipEventSynchronize(b.ev);
    (void)hipEventDestroy(b.ev);
    (void)hipFree(b.p);
    bytes += b.cls;
  }
  hipMemPool_t pool = nullptr;
  if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) (void)hipMemPoolTrimTo(pool, 0);
  return bytes;
}
}  // namespace

int dev_alloc(int64_t bytes, hipStream_t stream, void** out) {
  *out = nullptr;
  const size_t cls = size_class(bytes);
  int device = 0;
  (void)hipGetDevice(&device);
  {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (size_t i = 0; i < g_cache_free.size(); i++) {
      CacheBlock b = g_cache_free[i];
      if (b.cls != cls || b.device != device) continue;
      g_cache_free[i] = g_cache_free.back();
      g_cache_free.pop_back();
      g_cache_bytes -= cls;
      // always wait on the device (free when already ordered): a stream handle can be reused
      // by a new stream after the old one is destroyed with work pending
      (void)hipStreamWaitEvent(stream, b.ev, 0);
      (void)hipEventDestroy(b.ev);
      g_cache_live[b.p] = {cls, device};
      *out = b.p;
      return FURY_OK;
    }
  }
  keep_pool(device);
  hipError_t e = hipMallocAsync(out, cls, stream);
  if (e != hipSuccess) {              // idle cached blocks may be what is missing: release, retry
    (void)hipGetLastError();
    release_cached(device);
    e = hipMallocAsync(out, cls, stream);
  }
  const int st = check_hip(e, "hipMallocAsync");
  if (st) return st;
  std::lock_guard<std::mutex> lock(g_cache_mu);
  g_cache_live[*out] = {cls, device};
  return FURY_OK;
}

void dev_free(void* p, hipStream_t stream) {
  if (!p) return;
  std::lock_guard<std::mutex> lock(g_cache_mu);
  auto it = g_cache_live.find(p);
  if (it == g_cache_live.end()) return;
  const size_t cls = it->second.first;
  const int device = it->second.second;
  g_cache_live.erase(it);
  hipEvent_t ev = nullptr;
  if (g_cache_bytes + cls > kCacheCap ||
      hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipFreeAsync(p, stream);
    return;
  }
  (void)hipEventRecord(ev, stream);
  g_cache_free.push_back(CacheBlock{p, cls, device, ev});
  g_cache_bytes += cls;
}

int64_t dev_live_blocks() {
  std::lock_guard<std::mutex> lock(g_cache_mu);
  return static_cast<int64_t>(g_cache_live.size());
}

DeviceTable::~DeviceTable() {
  if (dev) dev_free(dev, stream);
}

int upload_table(const void* host, size_t bytes, hipStream_t stream, DeviceTable* out) {
  if (bytes == 0 || bytes > kRingBytes)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "column table size");
  std::lock_guard<std::mutex> lock(g_ring_mu);
  if (!g_ring) {
    void* p = nullptr;
    int st = check_hip(hipHostMalloc(&p, kRingBytes, hipHostMallocDefault), "hipHostMalloc");
    if (st) return st;
    g_ring = static_cast<uint8_t*>(p);
  }
  size_t off = (g_ring_head + 255) & ~size_t(255);
  if (off + bytes > kRingBytes) off = 0;
  for (size_t i = 0; i < g_ring_pending.size();) {   // wait for copies still reading the region
    RingUse& u = g_ring_pending[i];
    const bool overlap = u.off < off + bytes && off < u.off + u.bytes;
    if (overlap || hipEventQuery(u.ev) == hipSuccess) {
      if (overlap) (void)hipEventSynchronize(u.ev);
      (void)hipEventDestroy(u.ev);
      g_ring_pending[i] = g_ring_pending.back();
      g_ring_pending.pop_back();
    } else {
      i++;
    }
  }
  std::memcpy(g_ring + off, host, bytes);
  out->host.assign(static_cast<const uint8_t*>(host), static_cast<const uint8_t*>(host) + bytes);
  g_ring_head = off + bytes;
  int st = dev_alloc(static_cast<int64_t>(bytes), stream, &out->dev);
  if (st) return st;
  out->stream = stream;
  st = check_hip(hipMemcpyAsync(out->dev, g_ring + off, bytes, hipMemcpyHostToDevice, stream),
                 "hipMemcpyAsync column table");
  if (st) return st;
  hipEvent_t ev;
  if ((st = check_hip(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate")))
    return st;
  (void)hipEventRecord(ev, stream);
  g_ring_pending.push_back(RingUse{off, bytes, ev});
  return FURY_OK;
}

namespace {

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// ---- the row operators' argument checks -----------------------------------------------------------
// What fury_row_hash ... fury_row_map_join check of their buffers, written once: an operator composes
// its checks from these, after its own schema / path / selection checks.  Every message starts with
// the entry point's name `f` (an empty f gives the bare message: the projected decode's wording).
int invalid(const std::string& f, const std::string& what) {
  return set_error(FURY_ERR_INVALID_ARGUMENT, f.empty() ? what : f + ": " + what);
}

int check_count(const std::string& f, const char* name, int64_t v) {
  return v < 0 ? invalid(f, std::string(name) + " < 0") : FURY_OK;
}

int check_required(const std::string& f, const char* name, const void* p) {
  return p ? FURY_OK : invalid(f, std::string(name) + " is null");
}

// Every pointer of the list is `a`-byte aligned (a null one is); the message names the whole list.
struct NamedPtr {
  const char* name;
  const void* p;
};
int check_aligned(const std::string& f, uintptr_t a, std::initializer_list<NamedPtr> ptrs) {
  bool bad = false;
  std::string names;
  for (const NamedPtr& n : ptrs) {
    bad = bad || misaligned(n.p, a);
    names += std::string(names.empty() ? "" : " / ") + n.name;
  }
  return bad ? invalid(f, names + " must be " + std::to_string(a) + "-byte aligned") : FURY_OK;
}

// How a source batch finds its rows: at i * fixed_size (row_offsets is ignored), or through row_offsets,
// which the rows of a variable-length schema need, and the paths of extract, explode and map split
// whatever the schema.
enum SourceRows { kFixedRows, kVariableRows, kOffsetRows };
SourceRows rows_of(const fury_schema* s) { return s->is_fixed ? kFixedRows : kVariableRows; }

// A source batch; `read`: the call reads at least one of its rows.  The alignment of row_offsets is the
// caller's: where an entry checks it, its message names further pointers.
int check_source(const std::string& f, const void* rows, const int64_t* row_offsets, SourceRows how,
                 bool read) {
  if (misaligned(rows, 8)) return invalid(f, "rows must be 8-byte aligned");
  if (how == kVariableRows && !row_offsets) return invalid(f, "variable-length rows need row_offsets");
  if (how == kOffsetRows && !row_offsets) return invalid(f, "row_offsets is null");
  if (read && !rows) return invalid(f, "rows is null");
  return FURY_OK;
}

// ... into an argument block that names the members as TakeArgs does.
template <class Args>
int check_source(const std::string& f, const void* rows, const int64_t* row_offsets, SourceRows how,
                 bool read, Args* a) {
  a->rows = static_cast<const uint8_t*>(rows);
  a->row_offsets = how == kFixedRows ? nullptr : row_offsets;    // row i at i * fixed_size
  return check_source(f, rows, row_offsets, how, read);
}

// An output batch, into an argument block that names the members as TakeArgs does.  `need_offsets`: what
// to say when out_offsets is null, or NULL when the output rows are `row_size` bytes each (row r at
// r * row_size, out_offsets optional): `n` of them must then fit a buffer that is given.  The alignment
// of out_offsets is the caller's, as check_source's.
template <class Args>
int check_output(const std::string& f, void* out_rows, int64_t out_capacity, int64_t* out_offsets, Args* a,
                 const char* need_offsets, int64_t n = 0, int64_t row_size = 0) {
  if (out_capacity < 0) return invalid(f, "out_capacity < 0");
  if (misaligned(out_rows, 8)) return invalid(f, "out_rows must be 8-byte aligned");
  if (need_offsets && !out_offsets) return invalid(f, need_offsets);
  if (!need_offsets && out_rows && row_size > 0 && out_capacity / row_size < n)
    return set_error(FURY_ERR_CAPACITY,
                     f + ": out_capacity " + std::to_string(out_capacity) + " < " + std::to_string(n) +
                         " rows of " + std::to_string(row_size) + " bytes");
  a->out = static_cast<uint8_t*>(out_rows);
  a->cap = out_rows ? out_capacity : 0;      // no buffer: the measure form
  a->out_offsets = out_offsets;
  return FURY_OK;
}
constexpr const char* kNeedOutOffsets = "variable-length rows need out_offsets";
constexpr const char* kOutOffsetsNull = "out_offsets is null";

// The end of every row operator, after its last argument check: the stream's pending device error,
// the error slot of this launch, the launch.
template <class Args, class Launch>
int launch_checked(hipStream_t hs, Args* a, Launch launch) {
  int st = take_device_error(hs);
  if (st) return st;
  if ((st = device_error_word(hs, &a->err))) return st;
  return launch();
}

int common_checks(const fury_schema* s, const void* cols, int64_t nrows, const char* fn,
                  hipStream_t hs) {
  if (!s) return set_error(FURY_ERR_INVALID_ARGUMENT, std::string(fn) + ": schema is null");
  if (nrows < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, std::string(fn) + ": nrows < 0");
  if (nrows > 0 && s->num_fields > 0 && !cols)
    return set_error(FURY_ERR_INVALID_ARGUMENT, std::string(fn) + ": columns is null");
  if (!s->device_ok)
    return set_error(FURY_ERR_UNSUPPORTED,
                     std::string(fn) + ": no device kernel for " + s->device_reason);
  return take_device_error(hs);
}

int fixed_args(const fury_schema* s, const fury_column* cols, int64_t nrows, bool decode,
               bool need_validity, FixedArgs* a, bool* fast, DeviceTable* dt, hipStream_t hs) {
  *a = FixedArgs{};
  a->ncols = s->num_fields;
  a->bitmap_bytes = s->bitmap_bytes;
  a->row_size = s->fixed_size;
  a->nrows = nrows;
  const bool wide = s->num_fields > kMaxFixedCols;
  std::vector<FixedCol> tab(wide ? s->num_fields : 0);
  bool all8 = true, anyv = false;
  for (int k = 0; k < s->num_fields; k++) {
    const FieldPlan& p = s->plan[k];
    const fury_column& c = cols[k];
    if (nrows > 0 && !c.values)
      return set_error(FURY_ERR_INVALID_ARGUMENT,
                       "column " + std::to_string(k) + " (" + s->fields[k].name + "): values is null");
    const int w = p.kind == kBool ? 0 : p.width;
    if (w > 1 && misaligned(c.values, static_cast<uintptr_t>(w)))
      return set_error(FURY_ERR_INVALID_ARGUMENT,
                       "column " + std::to_string(k) + ": values not " + std::to_string(w) +
                           "-byte aligned");
    if (need_validity && !c.validity)
      return set_error(FURY_ERR_INVALID_ARGUMENT,
                       "column " + std::to_string(k) + ": Arrow output needs a validity buffer");
    FixedCol& fc = wide ? tab[k] : a->col[k];
    fc.values = static_cast<const uint8_t*>(c.values);
    fc.validity = c.validity;
    fc.width = w;
    if (w != 8) all8 = false;
    if (c.validity) anyv = true;
  }
  (void)decode;
  *fast = all8 && !anyv && !wide;         // wide tables run the general tile kernel only
  if (wide) {
    const int st = upload_table(tab.data(), tab.size() * sizeof(FixedCol), hs, dt);
    if (st) return st;
    a->tab = static_cast<const FixedCol*>(dt->dev);
  }
  return FURY_OK;
}

int var_args(const fury_schema* s, const fury_column* cols, int64_t nrows, bool decode,
             bool need_validity, VarArgs* a, DeviceTable* dt, hipStream_t hs,
             bool shape_only = false) {
  if (s->num_fields > kMaxWideVarCols)
    return set_error(FURY_ERR_UNSUPPORTED, "variable-length device path handles at most " +
                                               std::to_string(kMaxWideVarCols) + " fields");
  *a = VarArgs{};
  a->ncols = s->num_fields;
  a->bitmap_bytes = s->bitmap_bytes;
  a->fixed_size = s->fixed_size;
  a->nrows = nrows;
  const bool wide = s->num_fields > kMaxVarCols;
  std::vector<VarCol> tab(wide ? s->num_fields : 0);
  int nvar = 0;
  for (int k = 0; k < s->num_fields; k++) {
    const FieldPlan& p = s->plan[k];
    static const fury_column kNoColumn{};
    const fury_column& c = shape_only ? kNoColumn : cols[k];
    VarCol& v = wide ? tab[k] : a->col[k];
    const std::string who = "column " + std::to_string(k) + " (" + s->fields[k].name + ")";
    v.kind = p.kind;
    v.nullable = p.nullable;
    v.var_slot = -1;
    v.validity = c.validity;
    if (decode && c.validity && misaligned(c.validity, 4))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": validity must be 4-byte aligned");
    if (need_validity && !c.validity)
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": Arrow output needs a validity buffer");
    switch (p.kind) {
      case kFixed:
      case kBool:
        v.width = p.kind == kBool ? 0 : p.width;
        v.values = static_cast<const uint8_t*>(c.values);
        if (!shape_only && nrows > 0 && !c.values) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values is null");
        if (v.width > 1 && misaligned(c.values, v.width))
          return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values misaligned");
        break;
      case kBytes:
        v.width = 1;
        v.values = static_cast<const uint8_t*>(c.values);
        v.offsets = c.offsets;
        v.var_slot = nvar++;
        v.capacity = c.values ? c.capacity : 0;
        if (!shape_only && nrows > 0 && !c.offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": offsets is null");
        break;
      case kDecimal:
        v.width = 16;
        v.values = static_cast<const uint8_t*>(c.values);
        v.var_slot = nvar++;
        if (!shape_only && nrows > 0 && !c.values) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values is null");
        break;
      case kListFixed: {
        v.width = p.elem_type == FURY_TYPE_BOOL ? 0 : p.elem_width;
        v.offsets = c.offsets;
        v.var_slot = nvar++;
        if (!shape_only && nrows > 0 && !c.offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": offsets is null");
        if (!c.child) {
          if (!shape_only && (!decode || nrows > 0))
            return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": list needs a child column");
        } else {
          v.values = static_cast<const uint8_t*>(c.child->values);
          v.elem_validity = c.child->validity;
          // child capacity is in bytes of values; the kernels bound element indices by it
          v.capacity = !c.child->values ? 0
                       : v.width == 0   ? c.child->capacity * 8
                                        : c.child->capacity / v.width;
          if (decode && (misaligned(c.child->validity, 4) ||
                         (v.width == 0 && misaligned(c.child->values, 4))))
            return set_error(FURY_ERR_INVALID_ARGUMENT,
                             who + ": element bitmaps must be 4-byte aligned");
          if (need_validity && !c.child->validity)
            return set_error(FURY_ERR_INVALID_ARGUMENT,
                             who + ": Arrow output needs element validity");
          if (v.width > 1 && misaligned(v.values, v.width))
            return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": element values misaligned");
        }
        break;
      }
      default:
        return set_error(FURY_ERR_UNSUPPORTED, who + ": no device kernel");
    }
  }
  a->nvar = nvar;
  if (wide) {                      // wider than the argument block: the table goes to the device
    const int st = upload_table(tab.data(), tab.size() * sizeof(VarCol), hs, dt);
    if (st) return st;
    a->tab = static_cast<const VarCol*>(dt->dev);
    a->htab = reinterpret_cast<const VarCol*>(dt->host.data());
    a->tile_rows = encode_tile_rows(*a);
  } else {
    a->tile_rows = encode_tile_rows(*a);
  }
  if (const int e = device_error_word(hs, &a->err)) return e;
  a->help_now = knob::lookback_help.load();
  a->skip = knob::var_skip.load();
  return FURY_OK;
}

// Generic engine arguments: schema nodes (breadth-first) + the column tree walked in the same
// order (LIST: child[0] = elements; STRUCT: child[0..n); MAP: child[0] keys, child[1] values).
int gen_args(const fury_schema* s, const fury_column* cols, int64_t nrows, bool decode,
             bool need_validity, GenArgs* g, DeviceTable* dt, hipStream_t hs) {
  const size_t nn = s->nodes.size();
  if (nn > static_cast<size_t>(kGenMaxWideNodes))
    return set_error(FURY_ERR_UNSUPPORTED, "nested schema has more than " +
                                               std::to_string(kGenMaxWideNodes) + " nodes");
  const bool wide = nn > static_cast<size_t>(kGenMaxNodes);
  std::vector<GenNode> tab(wide ? nn : 0);
  GenNode* nodes = nullptr;
  *g = GenArgs{};
  nodes = wide ? tab.data() : g->node;
  g->nnodes = static_cast<int32_t>(nn);
  g->ntop = s->num_fields;
  g->nrows = nrows;
  g->err = nullptr;
  g->root = s->root;
  if (s->root && !decode && cols && cols[0].validity)
    return set_error(FURY_ERR_INVALID_ARGUMENT,
                     "collection batch: the top-level column has no validity (toArray / toMap of a "
                     "null collection is not defined)");
  std::vector<const fury_column*> col(nn, nullptr);
  for (int k = 0; k < s->num_fields; k++) col[k] = &cols[k];
  for (size_t i = 0; i < nn; i++) {
    const GenTpl& t = s->nodes[i];
    const fury_column* c = col[i];
    const std::string who = "schema node " + std::to_string(i);
    if (!c) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": missing column");
    GenNode& n = nodes[i];
    n.values = static_cast<const uint8_t*>(c->values);
    n.validity = c->validity;
    n.offsets = c->offsets;
    n.type = t.type_id;
    n.first_child = t.first_child;
    n.num_children = t.num_children;
    // breadth-first order: a node's parent is set before it
    if (i < static_cast<size_t>(s->num_fields)) n.row_aligned = 1;
    if (n.row_aligned && t.type_id == FURY_TYPE_STRUCT)
      for (int j = 0; j < t.num_children; j++) nodes[t.first_child + j].row_aligned = 1;
    if (t.num_children > 0) {
      if (!c->child) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": child columns missing");
      for (int j = 0; j < t.num_children; j++) col[t.first_child + j] = &c->child[j];
    }
    const bool var = t.type_id == FURY_TYPE_STRING || t.type_id == FURY_TYPE_BINARY ||
                     t.type_id == FURY_TYPE_LIST || t.type_id == FURY_TYPE_MAP;
    if (nrows > 0 && var && !c->offsets)
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": offsets is null");
    if (need_validity && !c->validity)
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": Arrow output needs a validity buffer");
    if (decode && c->validity && misaligned(c->validity, 4))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": validity must be 4-byte aligned");
    if (decode && t.type_id == FURY_TYPE_BOOL && c->values && misaligned(c->values, 4))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": bool bitmap must be 4-byte aligned");
  }
  if (wide) {                      // more nodes than the argument block: table to the device
    const int st = upload_table(tab.data(), tab.size() * sizeof(GenNode), hs, dt);
    if (st) return st;
    g->tab = static_cast<const GenNode*>(dt->dev);
    g->htab = reinterpret_cast<const GenNode*>(dt->host.data());
  }
  return FURY_OK;
}

int gen_measure(const fury_schema* s, const fury_column* cols, int64_t nrows, int64_t* offs,
                hipStream_t stream) {
  GenArgs g;
  DeviceTable dt;
  int st = gen_args(s, cols, nrows, false, false, &g, &dt, stream);
  if (st) return st;
  if (nrows == 0) return check_hip(hipMemsetAsync(offs, 0, 8, stream), "memset");
  st = launch_gen_measure(g, offs, stream);
  if (st) return st;
  int64_t* ws = nullptr;
  st = dev_alloc(scan_workspace(nrows) * 8, stream, reinterpret_cast<void**>(&ws));
  if (st) return st;
  device_scan(offs, nrows, offs + nrows, ws, stream);
  st = check_hip(hipGetLastError(), "scan launch");
  dev_free(ws, stream);
  return st;
}

// Words [0, 3) of a selected field's table entry (SelectArgs in kernels.h): the slot, the width and the
// size rule of top-level field k of `s`; whether the field is variable-length.
bool selection_words(const fury_schema* s, int32_t k, int32_t* t) {
  const FieldPlan& p = s->plan[k];
  t[0] = k;
  t[2] = 0;
  if (p.width > 0) {
    t[1] = p.kind == kBool ? kSelBool : p.width;
    return false;
  }
  t[1] = kSelVar;
  switch (p.type_id) {
    case FURY_TYPE_DECIMAL: t[2] = 16 | kSelExact; break;
    case FURY_TYPE_STRUCT: {            // a row of the child's fields: at least its header
      const int64_t m = static_cast<int64_t>(s->fields[k].children.size());
      t[2] = static_cast<int32_t>(std::min<int64_t>(bitmap_bytes(m) + 8 * m, kSelNeed)) | kSelMod8;
      break;
    }
    case FURY_TYPE_LIST:
    case FURY_TYPE_MAP: t[2] = 8 | kSelMod8; break;      // [int64 numElements] / [int64 keyArrayBytes]
    default: break;                     // STRING / BINARY: any size
  }
  return true;
}

// The selection table of fury_row_select (stride 4) and fury_row_zip (stride 5, SelectArgs / ZipArgs in
// kernels.h): `stride` words per pick j of field_of(j) of schema_of(j) -- selection_words, then [3] its
// index among the variable-length picks or -1 -- to which finish_selection appends those picks' j.
struct Selection {
  std::vector<int32_t> table;
  std::vector<int32_t> var;           // the variable-length picks
  int32_t out_bitmap = 0;
  int64_t out_fixed = 0;              // the output row's header: its size when var is empty
};
template <class SchemaOf, class FieldOf>
Selection make_selection(int32_t n, int stride, SchemaOf schema_of, FieldOf field_of) {
  Selection sel;
  sel.table.resize(static_cast<size_t>(stride) * n);
  for (int32_t j = 0; j < n; j++) {
    int32_t* t = &sel.table[static_cast<size_t>(stride) * j];
    t[3] = -1;
    if (!selection_words(schema_of(j), field_of(j), t)) continue;
    t[3] = static_cast<int32_t>(sel.var.size());
    sel.var.push_back(j);
  }
  sel.out_bitmap = bitmap_bytes(n);
  sel.out_fixed = sel.out_bitmap + 8 * static_cast<int64_t>(n);
  return sel;
}

// What SelectArgs and ZipArgs say of the selection; the table is complete afterwards.
template <class Args>
void finish_selection(Selection* sel, int32_t n, Args* a) {
  sel->table.insert(sel->table.end(), sel->var.begin(), sel->var.end());
  a->nsel = n;
  a->nvar = static_cast<int32_t>(sel->var.size());
  a->out_bitmap_bytes = sel->out_bitmap;
  a->out_fixed_size = static_cast<int32_t>(sel->out_fixed);
}

// The path of fury_row_extract / fury_row_explode / fury_row_map_split in their argument blocks, which
// name the members alike (walk_path of extract_dev.h relies on that too).
template <class Args>
void set_path(Args* a, int32_t nlevels, const std::vector<int32_t>& nfields, const int32_t* path) {
  a->nlevels = nlevels;
  for (int32_t k = 0; k < nlevels; k++) {
    a->nfields[k] = nfields[k];
    a->slot[k] = path[k];
  }
}

}  // namespace
}  // namespace fury

using namespace fury;

extern "C" {

// The encode of a 17-256-field flat variable-length schema: the wide tiles (wide.hip) or the
// row-walk encode (rowenc.hip, as nested schemas), by tuning "wide_enc_engine" (tuning.cpp).
static bool wide_encode_by_walk(const fury_schema* s, const fury_column* cols, int64_t nrows) {
  if (s->generic || s->is_fixed || s->num_fields <= 16 || s->num_fields > kMaxWideVarCols ||
      !knob::var_wide.load() || !cols || nrows <= 0)
    return false;
  const int mode = knob::wide_enc_engine.load();
  if (mode != 0) return mode == 2;
  double row = s->fixed_size;
  for (int k = 0; k < s->num_fields; k++) {
    const int kind = s->plan[k].kind;
    if (kind == kBytes && cols[k].values) row += static_cast<double>(cols[k].capacity) / nrows + 4;
    if (kind == kDecimal) row += 16;
    if (kind == kListFixed && cols[k].child && cols[k].child->values)
      row += 16 + static_cast<double>(cols[k].child->capacity) / nrows;
  }
  return row > knob::wide_walk_row.load();
}

int fury_row_measure(const fury_schema* s, const fury_column* cols, int64_t nrows,
                     int64_t* row_offsets, void* stream) {
  int st = common_checks(s, cols, nrows, "fury_row_measure", static_cast<hipStream_t>(stream));
  if (st) return st;
  if (!row_offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, "row_offsets is null");
  if (misaligned(row_offsets, 8)) return set_error(FURY_ERR_INVALID_ARGUMENT, "row_offsets misaligned");
  if (s->generic || wide_encode_by_walk(s, cols, nrows))
    return gen_measure(s, cols, nrows, row_offsets, static_cast<hipStream_t>(stream));
  VarArgs a;
  DeviceTable dt;
  st = var_args(s, cols, nrows, false, false, &a, &dt, static_cast<hipStream_t>(stream));
  if (st) return st;
  return launch_measure_rows(a, row_offsets, static_cast<hipStream_t>(stream));
}

int fury_row_encode(const fury_schema* s, const fury_column* cols, int64_t nrows,
                    const int64_t* row_offsets, void* rows, void* stream) {
  int st = common_checks(s, cols, nrows, "fury_row_encode", static_cast<hipStream_t>(stream));
  if (st) return st;
  if (nrows == 0) return FURY_OK;
  if (!rows) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows is null");
  if (misaligned(rows, 16)) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows must be 16-byte aligned");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (s->is_fixed) {
    // Fixed schemas: rows are contiguous at i * fixed_size (row_offsets, when given, are those).
    FixedArgs a;
    bool fast = false;
    DeviceTable dt;
    st = fixed_args(s, cols, nrows, false, false, &a, &fast, &dt, hs);
    if (st) return st;
    return launch_encode_fixed(a, static_cast<uint8_t*>(rows), hs, fast);
  }
  if (!row_offsets)
    return set_error(FURY_ERR_INVALID_ARGUMENT,
                     "variable-length schema needs row_offsets from fury_row_measure");
  if (s->generic || wide_encode_by_walk(s, cols, nrows)) {
    GenArgs g;
    DeviceTable dt;
    st = gen_args(s, cols, nrows, false, false, &g, &dt, hs);
    if (st) return st;
    return launch_gen_encode(g, row_offsets, static_cast<uint8_t*>(rows), INT64_MAX, hs);
  }
  VarArgs a;
  DeviceTable dt;
  st = var_args(s, cols, nrows, false, false, &a, &dt, hs);
  if (st) return st;
  return launch_encode_var(a, row_offsets, static_cast<uint8_t*>(rows), INT64_MAX, hs);
}

int fury_row_encode_measured(const fury_schema* s, const fury_column* cols, int64_t nrows,
                             int64_t* row_offsets, void* rows, int64_t capacity, void* stream) {
  int st = common_checks(s, cols, nrows, "fury_row_encode_measured", static_cast<hipStream_t>(stream));
  if (st) return st;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (capacity < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "capacity < 0");
  if (nrows > 0 && !rows) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows is null");
  if (misaligned(rows, 16)) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows must be 16-byte aligned");
  if (s->is_fixed) {
    if (nrows > 0 && nrows > capacity / s->fixed_size)
      return set_error(FURY_ERR_CAPACITY, "rows need " + std::to_string(nrows * s->fixed_size) +
                                              " bytes, capacity is " + std::to_string(capacity));
    if (row_offsets) {
      st = fury_row_measure(s, cols, nrows, row_offsets, stream);
      if (st) return st;
    }
    return fury_row_encode(s, cols, nrows, nullptr, rows, stream);
  }
  if (!row_offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, "row_offsets is null");
  if (misaligned(row_offsets, 8)) return set_error(FURY_ERR_INVALID_ARGUMENT, "row_offsets misaligned");
  if (s->generic || wide_encode_by_walk(s, cols, nrows)) {
    st = gen_measure(s, cols, nrows, row_offsets, hs);
    if (st || nrows == 0) return st;
    GenArgs g;
    DeviceTable dt;
    st = gen_args(s, cols, nrows, false, false, &g, &dt, hs);
    if (st) return st;
    return launch_gen_encode(g, row_offsets, static_cast<uint8_t*>(rows), capacity, hs);
  }
  VarArgs a;
  DeviceTable dt;
  st = var_args(s, cols, nrows, false, false, &a, &dt, hs);
  if (st) return st;
  const int one = launch_encode_measured_var(a, row_offsets, static_cast<uint8_t*>(rows), capacity, hs);
  if (one >= 0) return one;
  st = launch_measure_rows(a, row_offsets, hs);
  if (st || nrows == 0) return st;
  return launch_encode_var(a, row_offsets, static_cast<uint8_t*>(rows), capacity, hs);
}

// An empty batch still yields valid Arrow offsets (offsets[0] = 0) in every top-level column that
// has an offsets buffer; for n > 0 the decode kernels write them, for n = 0 none is launched.
static int zero_empty_offsets(const fury_schema* s, fury_column* cols, hipStream_t hs) {
  if (!cols) return FURY_OK;
  for (int k = 0; k < s->num_fields; k++) {
    if (!cols[k].offsets) continue;
    const int st = check_hip(hipMemsetAsync(cols[k].offsets, 0, 4, hs), "memset");
    if (st) return st;
  }
  return FURY_OK;
}

int fury_row_decode_measure(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                            int64_t nrows, fury_column* cols, void* stream) {
  int st = common_checks(s, cols, nrows, "fury_row_decode_measure", static_cast<hipStream_t>(stream));
  if (st) return st;
  if (nrows == 0) return zero_empty_offsets(s, cols, static_cast<hipStream_t>(stream));
  if (s->is_fixed) return FURY_OK;   // nothing variable to size
  if (s->generic)
    return set_error(FURY_ERR_INVALID_ARGUMENT,
                     "nested (or > 256-field variable-length) schema: size outputs with "
                     "fury_decode_prepare / fury_decode_execute");
  if (!rows || !row_offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows/row_offsets null");
  VarArgs a;
  DeviceTable dt;
  st = var_args(s, cols, nrows, true, false, &a, &dt, static_cast<hipStream_t>(stream));
  if (st) return st;
  return launch_decode_measure(a, static_cast<const uint8_t*>(rows), row_offsets,
                               static_cast<hipStream_t>(stream));
}

static int decode_impl(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, fury_column* cols, void* stream, bool arrow,
                       const char* fn) {
  int st = common_checks(s, cols, nrows, fn, static_cast<hipStream_t>(stream));
  if (st) return st;
  if (nrows == 0) return zero_empty_offsets(s, cols, static_cast<hipStream_t>(stream));
  if (!rows) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows is null");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (s->is_fixed) {
    if (misaligned(rows, 16)) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows must be 16-byte aligned");
    FixedArgs a;
    bool fast = false;
    DeviceTable dt;
    st = fixed_args(s, cols, nrows, true, arrow, &a, &fast, &dt, hs);
    if (st) return st;
    return launch_decode_fixed(a, static_cast<const uint8_t*>(rows), hs, fast);
  }
  if (!row_offsets)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "variable-length rows need row_offsets");
  if (misaligned(rows, 8)) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows must be 8-byte aligned");
  if (s->generic)
    return set_error(FURY_ERR_INVALID_ARGUMENT,
                     "nested (or > 256-field variable-length) schema: decode with "
                     "fury_decode_prepare / fury_decode_execute");
  VarArgs a;
  DeviceTable dt;
  st = var_args(s, cols, nrows, true, arrow, &a, &dt, hs);
  if (st) return st;
  return launch_decode_var(a, static_cast<const uint8_t*>(rows), row_offsets, hs, arrow);
}

int fury_row_decode(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, fury_column* cols, void* stream) {
  return decode_impl(s, rows, row_offsets, nrows, cols, stream, false, "fury_row_decode");
}

int fury_rows_to_arrow(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, fury_column* cols, void* stream) {
  return decode_impl(s, rows, row_offsets, nrows, cols, stream, true, "fury_rows_to_arrow");
}

// The selection checks shared by the projected decode and the in-place update: `coll` / `many`
// finish the messages for a collection schema and for more than kMaxProjCols fields.
static int check_selection(const fury_schema* s, const int32_t* fields, int32_t nsel, int64_t nrows,
                           const void* cols, const std::string& f, const char* coll,
                           const char* many) {
  if (!s) return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": schema is null");
  if (nrows < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": nrows < 0");
  if (nsel <= 0) return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": num_selected <= 0");
  if (!fields) return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": fields is null");
  if (nrows > 0 && !cols) return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": columns is null");
  if (s->root != 0) return set_error(FURY_ERR_UNSUPPORTED, f + ": a collection schema " + coll);
  if (nsel > kMaxProjCols)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": at most " + std::to_string(kMaxProjCols) + " fields per call; for more, " + many);
  std::vector<char> seen(s->num_fields, 0);
  for (int j = 0; j < nsel; j++) {
    const int32_t k = fields[j];
    if (k < 0 || k >= s->num_fields)
      return set_error(FURY_ERR_INVALID_ARGUMENT, f + ": fields[" + std::to_string(j) + "] = " +
                                                      std::to_string(k) + " is not a field of the schema");
    if (seen[k])
      return set_error(FURY_ERR_INVALID_ARGUMENT,
                       f + ": field " + std::to_string(k) + " (" + s->fields[k].name + ") selected twice");
    seen[k] = 1;
  }
  return FURY_OK;
}

// Projected decode (project.hip).  Argument checks + the per-column records of the selection;
// `measure`: only the offsets of the STRING / BINARY / LIST columns are needed.  The column checks
// are var_args', with its wording.
static int project_args(const fury_schema* s, const int32_t* fields, int32_t nsel, const void* rows,
                        const int64_t* row_offsets, int64_t nrows, const fury_column* cols,
                        bool need_validity, bool measure, const char* fn, hipStream_t hs,
                        ProjArgs* a) {
  const std::string f(fn);
  int st = check_selection(s, fields, nsel, nrows, cols, f,
                           "has no row fields to select (decode it with fury_decode_prepare / "
                           "fury_decode_execute)",
                           "run the full decode (fury_row_decode / fury_decode_prepare)");
  if (st) return st;
  for (int j = 0; j < nsel; j++) {
    const int32_t k = fields[j];
    if (s->plan[k].kind == kOther)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": field " + std::to_string(k) + " (" + s->fields[k].name +
                           ") is a STRUCT / MAP / LIST of variable-length elements: decode it with "
                           "fury_decode_prepare / fury_decode_execute");
  }
  st = take_device_error(hs);
  if (st) return st;
  *a = ProjArgs{};
  a->ncols = nsel;
  a->bitmap_bytes = s->bitmap_bytes;
  a->fixed_size = s->fixed_size;
  a->nrows = nrows;
  a->nt = thread_host_direct() ? 0 : 1;
  static const fury_column kNoColumn{};
  for (int j = 0; j < nsel; j++) {
    const int32_t k = fields[j];
    const FieldPlan& p = s->plan[k];
    const fury_column& c = cols ? cols[j] : kNoColumn;
    ProjCol& v = a->col[j];
    const std::string who = "column " + std::to_string(j) + " (" + s->fields[k].name + ")";
    v.kind = p.kind;
    v.slot = k;
    v.validity = c.validity;
    if (c.validity && misaligned(c.validity, 4))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": validity must be 4-byte aligned");
    if (need_validity && !c.validity)
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": Arrow output needs a validity buffer");
    switch (p.kind) {
      case kFixed:
      case kBool:
        v.width = p.kind == kBool ? 0 : p.width;
        v.values = static_cast<uint8_t*>(c.values);
        if (!measure && nrows > 0 && !c.values) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values is null");
        if (misaligned(c.values, v.width > 1 ? v.width : v.width == 0 ? 4 : 1))
          return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values misaligned");
        break;
      case kBytes:
        v.width = 1;
        v.values = static_cast<uint8_t*>(c.values);
        v.offsets = c.offsets;
        v.capacity = c.values ? c.capacity : 0;
        if (nrows > 0 && !c.offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": offsets is null");
        break;
      case kDecimal:
        v.width = 16;
        v.values = static_cast<uint8_t*>(c.values);
        if (!measure && nrows > 0 && !c.values) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values is null");
        if (misaligned(c.values, 8)) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values misaligned");
        break;
      default: {                    // kListFixed
        v.width = p.elem_type == FURY_TYPE_BOOL ? 0 : p.elem_width;
        v.offsets = c.offsets;
        if (nrows > 0 && !c.offsets) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": offsets is null");
        if (!c.child) {
          if (!measure && nrows > 0)
            return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": list needs a child column");
        } else {
          v.values = static_cast<uint8_t*>(c.child->values);
          v.elem_validity = c.child->validity;
          // child capacity is in bytes of values; the kernels bound element indices by it
          v.capacity = !c.child->values ? 0
                       : v.width == 0   ? c.child->capacity * 8
                                        : c.child->capacity / v.width;
          if (misaligned(c.child->validity, 4) || (v.width == 0 && misaligned(c.child->values, 4)))
            return set_error(FURY_ERR_INVALID_ARGUMENT,
                             who + ": element bitmaps must be 4-byte aligned");
          if (need_validity && !measure && !c.child->validity)
            return set_error(FURY_ERR_INVALID_ARGUMENT,
                             who + ": Arrow output needs element validity");
          if (v.width > 1 && misaligned(v.values, v.width))
            return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": element values misaligned");
        }
        break;
      }
    }
  }
  if (nrows == 0) return FURY_OK;
  if ((st = check_source(std::string(), rows, row_offsets, rows_of(s), true))) return st;
  return device_error_word(hs, &a->err);
}

// An empty batch still yields valid Arrow offsets (offsets[0] = 0), as zero_empty_offsets.
static int zero_selected_offsets(int32_t nsel, fury_column* cols, hipStream_t hs) {
  if (!cols) return FURY_OK;
  for (int j = 0; j < nsel; j++) {
    if (!cols[j].offsets) continue;
    const int st = check_hip(hipMemsetAsync(cols[j].offsets, 0, 4, hs), "memset");
    if (st) return st;
  }
  return FURY_OK;
}

int fury_row_project(const fury_schema* s, const int32_t* fields, int32_t num_selected,
                     const void* rows, const int64_t* row_offsets, int64_t nrows,
                     fury_column* cols, int32_t arrow, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  ProjArgs a;
  const int st = project_args(s, fields, num_selected, rows, row_offsets, nrows, cols, arrow != 0,
                              false, "fury_row_project", hs, &a);
  if (st) return st;
  if (nrows == 0) return zero_selected_offsets(num_selected, cols, hs);
  // fixed schemas: row i at i * fixed_size, as in fury_row_decode
  return launch_project(a, static_cast<const uint8_t*>(rows), s->is_fixed ? nullptr : row_offsets, hs);
}

int fury_row_project_measure(const fury_schema* s, const int32_t* fields, int32_t num_selected,
                             const void* rows, const int64_t* row_offsets, int64_t nrows,
                             fury_column* cols, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  ProjArgs a;
  const int st = project_args(s, fields, num_selected, rows, row_offsets, nrows, cols, false, true,
                              "fury_row_project_measure", hs, &a);
  if (st) return st;
  if (nrows == 0) return zero_selected_offsets(num_selected, cols, hs);
  return launch_project_measure(a, static_cast<const uint8_t*>(rows),
                                s->is_fixed ? nullptr : row_offsets, hs);
}

// Key hash (hash.hip): BinaryRow's getters feeding MurmurHash3.murmurhash3_x86_32, key after key.
int fury_row_hash(const fury_schema* s, const int32_t* fields, int32_t num_keys, const void* rows,
                  const int64_t* row_offsets, int64_t nrows, uint32_t seed, int32_t num_parts,
                  uint32_t* out_hashes, int32_t* out_part_ids, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_hash");
  // `fields` stands in for the column table check_selection wants: this call has none
  int st = check_selection(s, fields, num_keys, nrows, fields, f,
                           "has no row fields to hash",
                           "there is no route (the seed is per call, not per row): hash a subset of the keys");
  if (st) return st;
  for (int j = 0; j < num_keys; j++) {
    const int32_t k = fields[j];
    if (s->plan[k].kind == kOther || s->plan[k].kind == kListFixed)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": field " + std::to_string(k) + " (" + s->fields[k].name +
                           ") is a LIST / STRUCT / MAP: its stored bytes are not canonical (null "
                           "slots keep stale contents), so it cannot be a hash key");
  }
  if (!out_hashes && !out_part_ids) return invalid(f, "out_hashes and out_part_ids are both null");
  if (out_part_ids && num_parts < 1)
    return invalid(f, "num_parts " + std::to_string(num_parts) + " is not in [1, 2147483647]");
  if ((st = check_aligned(f, 4, {{"out_hashes", out_hashes}, {"out_part_ids", out_part_ids}}))) return st;
  if (nrows == 0) return FURY_OK;
  if ((st = check_source(f, rows, row_offsets, rows_of(s), true))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}}))) return st;
  ProjArgs a{};
  a.ncols = num_keys;
  a.bitmap_bytes = s->bitmap_bytes;
  a.fixed_size = s->fixed_size;
  a.nrows = nrows;
  a.nt = 1;
  for (int j = 0; j < num_keys; j++) {
    const FieldPlan& p = s->plan[fields[j]];
    ProjCol& v = a.col[j];
    v.kind = p.kind;
    v.slot = fields[j];
    v.width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
  }
  // fixed schemas: row i at i * fixed_size, as in fury_row_project
  return launch_checked(hs, &a, [&] {
    return launch_hash(a, static_cast<const uint8_t*>(rows), s->is_fixed ? nullptr : row_offsets, seed,
                       out_part_ids ? static_cast<uint32_t>(num_parts) : 1u, out_hashes, out_part_ids, hs);
  });
}

// Rule 6 of fury_row_keys_equal for the two sides of a key comparison (fury_row_keys_equal: left / right;
// fury_row_lookup: probe / build): each side's selection, no LIST / STRUCT / MAP key, the same type_id
// at every key position.
static int check_key_sides(const std::string& f, const fury_key_side* const (&sides)[2],
                           const std::string (&names)[2], const char* first, const char* second,
                           int32_t num_keys) {
  for (int s = 0; s < 2; s++) {
    // `fields` stands in for the column table check_selection wants, as in fury_row_hash
    int st = check_selection(sides[s]->schema, sides[s]->fields, num_keys, sides[s]->nrows, sides[s]->fields,
                             names[s], "has no row fields to compare",
                             "there is no route: compare a subset of the keys and AND the results");
    if (st) return st;
    for (int j = 0; j < num_keys; j++) {
      const fury_schema* sc = sides[s]->schema;
      const int32_t k = sides[s]->fields[j];
      if (sc->plan[k].kind == kOther || sc->plan[k].kind == kListFixed)
        return set_error(FURY_ERR_UNSUPPORTED,
                         names[s] + ": field " + std::to_string(k) + " (" + sc->fields[k].name +
                             ") is a LIST / STRUCT / MAP: its stored bytes are not canonical (null "
                             "slots keep stale contents), so it cannot be a key");
    }
  }
  for (int j = 0; j < num_keys; j++) {
    const int32_t kl = sides[0]->fields[j], kr = sides[1]->fields[j];
    const FieldPlan &pl = sides[0]->schema->plan[kl], &pr = sides[1]->schema->plan[kr];
    if (pl.type_id != pr.type_id)
      return invalid(f, "key " + std::to_string(j) + ": " + first + " field " + std::to_string(kl) + " (" +
                            sides[0]->schema->fields[kl].name + ") has type " + std::to_string(pl.type_id) +
                            ", " + second + " field " + std::to_string(kr) + " (" +
                            sides[1]->schema->fields[kr].name + ") has type " + std::to_string(pr.type_id));
  }
  return FURY_OK;
}

// The key positions of a two-sided comparison: `left`'s fields against `right`'s.
static void fill_key_recs(const fury_key_side* left, const fury_key_side* right, int32_t num_keys, KeyRec* key) {
  for (int j = 0; j < num_keys; j++) {
    const FieldPlan& p = left->schema->plan[left->fields[j]];
    KeyRec& v = key[j];
    v.left_slot = left->fields[j];
    v.right_slot = right->fields[j];
    v.kind = p.kind;
    v.width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
  }
}

// Key equality of row pairs (keys_equal.hip): BinaryRow's getters on both rows, value against value.
int fury_row_keys_equal(const fury_key_side* left, const fury_key_side* right, int32_t num_keys,
                        int64_t num_pairs, int32_t flags, uint8_t* out_equal, uint32_t* out_mask,
                        void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_keys_equal");
  int st = check_required(f, "left", left);
  if (st) return st;
  if ((st = check_required(f, "right", right))) return st;
  const fury_key_side* sides[2] = {left, right};
  const std::string names[2] = {f + ": left", f + ": right"};
  if ((st = check_key_sides(f, sides, names, "left", "right", num_keys))) return st;
  if ((st = check_count(f, "num_pairs", num_pairs))) return st;
  for (int s = 0; s < 2; s++)
    if (!sides[s]->indices && sides[s]->nrows < num_pairs)
      return invalid(names[s], "nrows " + std::to_string(sides[s]->nrows) + " < num_pairs " +
                                   std::to_string(num_pairs) + " and there are no indices");
  if (flags & ~FURY_KEYS_NULL_EQUAL) return invalid(f, "unknown flags " + std::to_string(flags));
  if (!out_equal && !out_mask) return invalid(f, "out_equal and out_mask are both null");
  if ((st = check_aligned(f, 4, {{"out_mask", out_mask}}))) return st;
  for (int s = 0; s < 2; s++)
    if ((st = check_aligned(names[s], 8, {{"indices", sides[s]->indices},
                                          {"row_offsets", sides[s]->row_offsets}})))
      return st;
  if (num_pairs == 0) return FURY_OK;
  KeysEqualArgs a{};
  for (int s = 0; s < 2; s++) {
    const fury_schema* sc = sides[s]->schema;
    if ((st = check_source(names[s], sides[s]->rows, sides[s]->row_offsets, rows_of(sc), true, &a.side[s])))
      return st;
    a.side[s].nrows = sides[s]->nrows;
    a.side[s].indices = sides[s]->indices;
    a.side[s].bitmap_bytes = sc->bitmap_bytes;
    a.side[s].fixed_size = sc->fixed_size;
  }
  if ((num_pairs + 255) / 256 > INT32_MAX) return invalid(f, "batch too large");
  a.nkeys = num_keys;
  a.num_pairs = num_pairs;
  a.flags = flags;
  a.out_equal = out_equal;
  a.out_mask = out_mask;
  fill_key_recs(left, right, num_keys, a.key);
  return launch_checked(hs, &a, [&] { return launch_keys_equal(a, hs); });
}

static int check_key_fields(const std::string& f, const fury_schema* s, const int32_t* fields, int32_t num_keys,
                            int64_t nrows, const char* none, const char* route);

// One key position of an ordering: field `left_field` (of the plan `p`) against `right_field`.
static void fill_order_key(const FieldPlan& p, int32_t left_field, int32_t right_field, int32_t flags,
                           OrderKey* v) {
  v->left_slot = left_field;
  v->right_slot = right_field;
  v->kind = p.kind;
  v->width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
  v->cls = (p.type_id == FURY_TYPE_FLOAT32 || p.type_id == FURY_TYPE_FLOAT64) ? kOrdFloat
           : (p.kind == kBytes || p.kind == kBool)                            ? kOrdBytes
                                                                              : kOrdSigned;
  v->flags = flags;
}

// The order of row pairs (compare.hip): BinaryRow's getters on both rows, value against value, key after key.
int fury_row_compare(const fury_key_side* left, const fury_key_side* right, int32_t num_keys,
                     const int32_t* key_flags, int64_t num_pairs, int8_t* out_cmp, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_compare");
  int st = check_required(f, "left", left);
  if (st) return st;
  if ((st = check_required(f, "right", right))) return st;
  const fury_key_side* sides[2] = {left, right};
  const std::string names[2] = {f + ": left", f + ": right"};
  if ((st = check_key_sides(f, sides, names, "left", "right", num_keys))) return st;
  if ((st = check_count(f, "num_pairs", num_pairs))) return st;
  for (int s = 0; s < 2; s++)
    if (!sides[s]->indices && sides[s]->nrows < num_pairs)
      return invalid(names[s], "nrows " + std::to_string(sides[s]->nrows) + " < num_pairs " +
                                   std::to_string(num_pairs) + " and there are no indices");
  for (int j = 0; key_flags && j < num_keys; j++)
    if (key_flags[j] & ~(FURY_ORDER_DESC | FURY_ORDER_NULLS_LAST))
      return invalid(f, "key " + std::to_string(j) + ": unknown flags " + std::to_string(key_flags[j]));
  if ((st = check_required(f, "out_cmp", out_cmp))) return st;
  for (int s = 0; s < 2; s++)
    if ((st = check_aligned(names[s], 8, {{"indices", sides[s]->indices},
                                          {"row_offsets", sides[s]->row_offsets}})))
      return st;
  if (num_pairs == 0) return FURY_OK;
  CompareArgs a{};
  for (int s = 0; s < 2; s++) {
    const fury_schema* sc = sides[s]->schema;
    if ((st = check_source(names[s], sides[s]->rows, sides[s]->row_offsets, rows_of(sc), true, &a.side[s])))
      return st;
    a.side[s].nrows = sides[s]->nrows;
    a.side[s].indices = sides[s]->indices;
    a.side[s].bitmap_bytes = sc->bitmap_bytes;
    a.side[s].fixed_size = sc->fixed_size;
  }
  if ((num_pairs + 255) / 256 > INT32_MAX) return invalid(f, "batch too large");
  a.nkeys = num_keys;
  a.num_pairs = num_pairs;
  a.out_cmp = out_cmp;
  for (int j = 0; j < num_keys; j++)
    fill_order_key(left->schema->plan[left->fields[j]], left->fields[j], right->fields[j],
                   key_flags ? key_flags[j] : 0, &a.key[j]);
  return launch_checked(hs, &a, [&] { return launch_compare(a, hs); });
}

// Order words (order.hip): one chunk of one key field as integers whose order is fury_row_compare's.
int fury_row_order_words(const fury_schema* s, int32_t field, int32_t flags, int32_t chunk, const void* rows,
                         const int64_t* row_offsets, int64_t nrows, const int64_t* indices, int64_t num_out,
                         int64_t* out_words, uint32_t* out_more, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_order_words");
  int st = check_key_fields(f, s, &field, 1, nrows, "has no row fields to order by", "there is no route");
  if (st) return st;
  if (flags & ~(FURY_ORDER_DESC | FURY_ORDER_NULLS_LAST)) return invalid(f, "unknown flags " + std::to_string(flags));
  if (chunk < 0) return invalid(f, "chunk < 0");
  if ((st = check_count(f, "num_out", num_out))) return st;
  if (!indices && nrows < num_out)
    return invalid(f, "nrows " + std::to_string(nrows) + " < num_out " + std::to_string(num_out) +
                          " and there are no indices");
  if ((st = check_required(f, "out_words", out_words))) return st;
  if ((st = check_aligned(f, 8, {{"out_words", out_words}, {"indices", indices}, {"row_offsets", row_offsets}})))
    return st;
  if ((st = check_aligned(f, 4, {{"out_more", out_more}}))) return st;
  OrderWordsArgs a{};
  if (num_out > 0) {
    if ((st = check_source(f, rows, row_offsets, rows_of(s), true, &a.side))) return st;
    if ((num_out + 255) / 256 > INT32_MAX) return invalid(f, "batch too large");
  }
  a.side.nrows = nrows;
  a.side.indices = indices;
  a.side.bitmap_bytes = s->bitmap_bytes;
  a.side.fixed_size = s->fixed_size;
  a.num_out = num_out;
  a.chunk = chunk;
  a.out_words = out_words;
  a.out_more = out_more;
  fill_order_key(s->plan[field], field, field, flags, &a.key);
  if (num_out == 0 && !out_more) return FURY_OK;
  return launch_checked(hs, &a, [&] { return launch_order_words(a, hs); });
}

// Per-group aggregates (aggregate.hip): BinaryRow's getters folded into one accumulator per group.
int64_t fury_row_aggregate_lds_cells(void) { return kAggLdsCells; }

int fury_row_aggregate(const fury_schema* s, const void* rows, const int64_t* row_offsets, int64_t nrows,
                       const int64_t* group_ids, int64_t num_groups, const fury_agg* aggs, int32_t num_aggs,
                       void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_aggregate");
  static const char* const kOps[] = {"", "COUNT", "SUM", "MIN", "MAX", "ARGMIN", "ARGMAX"};
  if (!s) return invalid(f, "schema is null");
  int st = check_count(f, "nrows", nrows);
  if (st) return st;
  if ((st = check_required(f, "aggs", aggs))) return st;
  if (s->root != 0)
    return set_error(FURY_ERR_UNSUPPORTED, f + ": a collection schema has no row fields to aggregate");
  if (num_aggs < 1 || num_aggs > FURY_AGG_MAX_AGGS)
    return invalid(f, "num_aggs " + std::to_string(num_aggs) + " is not in [1, " +
                          std::to_string(FURY_AGG_MAX_AGGS) + "]");
  if ((st = check_count(f, "num_groups", num_groups))) return st;
  if (num_groups > INT32_MAX) return invalid(f, "num_groups " + std::to_string(num_groups) + " > 2^31 - 1");
  if (nrows > INT32_MAX) return invalid(f, "batch too large");
  if (!group_ids && num_groups != 1)
    return invalid(f, "group_ids is null: num_groups must be 1, not " + std::to_string(num_groups));
  AggArgs a{};
  for (int j = 0; j < num_aggs; j++) {
    const fury_agg& g = aggs[j];
    const std::string at = "aggs[" + std::to_string(j) + "]";
    if (g.op < FURY_AGG_COUNT || g.op > FURY_AGG_ARGMAX)
      return invalid(f, at + ": unknown op " + std::to_string(g.op));
    AggRec& v = a.rec[j];
    v.slot = g.field;
    v.op = g.op;
    v.kind = kFixed;
    v.width = 8;
    v.cls = kOrdSigned;
    v.combine = kAggNone;
    if (g.field == -1 && g.op == FURY_AGG_COUNT) continue;     // COUNT(*)
    if (g.field < 0 || g.field >= s->num_fields)
      return invalid(f, at + ": field " + std::to_string(g.field) + " is not a field of the schema");
    if (g.op == FURY_AGG_COUNT) continue;                      // only the null bit: any type
    const FieldPlan& p = s->plan[g.field];
    const std::string who = at + ": " + kOps[g.op] + " of field " + std::to_string(g.field) + " (" +
                            s->fields[g.field].name + ")";
    const bool isfloat = p.type_id == FURY_TYPE_FLOAT32 || p.type_id == FURY_TYPE_FLOAT64;
    const bool isint = p.type_id == FURY_TYPE_INT8 || p.type_id == FURY_TYPE_INT16 ||
                       p.type_id == FURY_TYPE_INT32 || p.type_id == FURY_TYPE_INT64;
    const bool word = p.kind == kFixed || p.kind == kBool;     // travels as one order word
    const bool arg = g.op == FURY_AGG_ARGMIN || g.op == FURY_AGG_ARGMAX;
    if (g.op == FURY_AGG_SUM && !(p.kind == kFixed && (isint || isfloat)))
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": " + who + ": SUM takes INT8 / INT16 / INT32 / INT64 / FLOAT32 / FLOAT64; DECIMAL "
                           "sums are out of scope, a BOOL sum is the COUNT of the field under ids that drop "
                           "the false rows");
    if ((g.op == FURY_AGG_MIN || g.op == FURY_AGG_MAX) && !word)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": " + who + ": MIN / MAX take the fixed-width types and BOOL; for STRING / BINARY / "
                           "DECIMAL use ARGMIN / ARGMAX, then fury_row_take at the rows whose count is not zero");
    if (arg && !word && p.kind != kBytes && p.kind != kDecimal)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": " + who + ": a LIST / STRUCT / MAP has no order (the key types of fury_row_compare)");
    v.kind = p.kind;
    v.width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
    v.cls = isfloat ? kOrdFloat : (p.kind == kBytes || p.kind == kBool) ? kOrdBytes : kOrdSigned;
    if (g.op == FURY_AGG_SUM) {
      v.combine = isfloat ? kAggAddFloat : kAggAddInt;
    } else if (!word) {
      v.combine = kAggArgVar;
    } else {
      v.combine = (g.op == FURY_AGG_MIN || g.op == FURY_AGG_ARGMIN) ? kAggMin : kAggMax;
      v.resolve = arg;
    }
  }
  std::vector<const void*> outs;
  for (int j = 0; j < num_aggs; j++) {
    const std::string at = "aggs[" + std::to_string(j) + "]";
    if (!aggs[j].out) return invalid(f, at + ".out is null");
    if ((st = check_aligned(f + ": " + at, 8, {{"out", aggs[j].out}, {"out_count", aggs[j].out_count}}))) return st;
    for (const void* p : {static_cast<const void*>(aggs[j].out), static_cast<const void*>(aggs[j].out_count)}) {
      if (!p) continue;
      for (const void* q : outs)
        if (p == q) return invalid(f, at + ": two outputs of one call are the same pointer");
      outs.push_back(p);
    }
    a.rec[j].out = static_cast<uint64_t*>(aggs[j].out);
    a.rec[j].out_count = aggs[j].out_count;
  }
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"group_ids", group_ids}}))) return st;
  if ((st = check_source(f, rows, row_offsets, nrows > 0 ? rows_of(s) : kFixedRows, nrows > 0 && num_groups > 0,
                         &a.side)))
    return st;
  if (num_groups == 0) return FURY_OK;
  a.side.nrows = nrows;
  a.side.bitmap_bytes = s->bitmap_bytes;
  a.side.fixed_size = s->fixed_size;
  a.group_ids = group_ids;
  a.num_groups = num_groups;
  a.naggs = num_aggs;
  return launch_checked(hs, &a, [&] { return launch_aggregate(a, hs); });
}

// WHERE masks (predicate.hip): BinaryRow's getters on every row, each value tested against a literal.
int fury_row_predicate(const fury_schema* s, const void* rows, const int64_t* row_offsets, int64_t nrows,
                       const fury_pred_term* terms, int32_t num_terms, const uint32_t* row_mask,
                       uint32_t* out_mask, int64_t* out_count, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_predicate");
  static const char* const kOps[] = {"",   "IS_NULL", "EQ",          "LT",        "LE",
                                     "GT", "GE",      "STARTS_WITH", "ENDS_WITH", "CONTAINS"};
  if (!s) return invalid(f, "schema is null");
  int st = check_count(f, "nrows", nrows);
  if (st) return st;
  if ((st = check_required(f, "terms", terms))) return st;
  if (s->root != 0)
    return set_error(FURY_ERR_UNSUPPORTED, f + ": a collection schema has no row fields to test");
  if (num_terms < 1 || num_terms > FURY_PRED_MAX_TERMS)
    return invalid(f, "num_terms " + std::to_string(num_terms) + " is not in [1, " +
                          std::to_string(FURY_PRED_MAX_TERMS) + "]");
  PredArgs a{};
  int64_t pool_bytes = 0;
  for (int j = 0; j < num_terms; j++) {
    const fury_pred_term& t = terms[j];
    const std::string at = "terms[" + std::to_string(j) + "]";
    if (t.op < FURY_PRED_IS_NULL || t.op > FURY_PRED_CONTAINS)
      return invalid(f, at + ": unknown op " + std::to_string(t.op));
    if (t.flags & ~(FURY_PRED_NOT | FURY_PRED_OR))
      return invalid(f, at + ": unknown flags " + std::to_string(t.flags));
    if (t.reserved != 0) return invalid(f, at + ": reserved is " + std::to_string(t.reserved) + ", not 0");
    if (j == 0 && (t.flags & FURY_PRED_OR))
      return invalid(f, at + ": FURY_PRED_OR on the first term: there is no clause to join");
    if (t.field < 0 || t.field >= s->num_fields)
      return invalid(f, at + ": field " + std::to_string(t.field) + " is not a field of the schema");
    const FieldPlan& p = s->plan[t.field];
    const std::string who = at + ": " + kOps[t.op] + " on field " + std::to_string(t.field) + " (" +
                            s->fields[t.field].name + ")";
    if (p.kind == kOther || p.kind == kListFixed)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": " + who + ": a LIST / STRUCT / MAP cannot be tested from the row bytes; decode "
                           "it with fury_row_project / fury_row_extract and test the decoded value");
    const bool pattern = t.op >= FURY_PRED_STARTS_WITH;
    if (pattern && p.kind != kBytes)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": " + who + ": STARTS_WITH / ENDS_WITH / CONTAINS take STRING / BINARY fields");
    if (t.literal_len < 0) return invalid(f, at + ": literal_len < 0");
    const int64_t need = t.op == FURY_PRED_IS_NULL ? 0
                         : p.kind == kFixed        ? p.width
                         : p.kind == kBool         ? 1
                         : p.kind == kDecimal      ? 16
                                                   : -1;
    if (need >= 0 && t.literal_len != need)
      return invalid(f, who + ": literal_len " + std::to_string(t.literal_len) + ", " + std::to_string(need) +
                            (t.op == FURY_PRED_IS_NULL ? " needed: IS_NULL takes no literal"
                                                       : " needed: the value's bytes as fury_row_project decodes them"));
    if (t.literal_len > 0 && !t.literal) return invalid(f, at + ": literal is null, literal_len is not 0");
    const int64_t padded = (t.literal_len + 7) & ~int64_t(7);
    if (padded > FURY_PRED_MAX_LITERAL_BYTES - pool_bytes)
      return invalid(f, at + ": the literals take more than " + std::to_string(FURY_PRED_MAX_LITERAL_BYTES) +
                            " bytes (each literal_len rounded up to a multiple of 8)");
    PredTerm& v = a.term[j];
    v.slot = t.field;
    v.kind = p.kind;
    v.width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
    v.cls = (p.type_id == FURY_TYPE_FLOAT32 || p.type_id == FURY_TYPE_FLOAT64) ? kOrdFloat
            : (p.kind == kBytes || p.kind == kBool)                            ? kOrdBytes
                                                                               : kOrdSigned;
    v.op = t.op;
    v.flags = t.flags;
    v.lit_word = static_cast<int32_t>(pool_bytes / 8);
    v.lit_len = static_cast<int32_t>(t.literal_len);
    pool_bytes += padded;
  }
  if ((st = check_required(f, "out_mask", out_mask))) return st;
  if ((st = check_aligned(f, 4, {{"row_mask", row_mask}, {"out_mask", out_mask}}))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"out_count", out_count}}))) return st;
  if ((nrows + 255) / 256 > INT32_MAX) return invalid(f, "batch too large");
  if ((st = check_source(f, rows, row_offsets, nrows > 0 ? rows_of(s) : kFixedRows, nrows > 0, &a.side))) return st;
  // the literals, copied now: the pool travels in the kernel-argument block (zeros pad each to whole words)
  for (int j = 0; j < num_terms; j++)
    if (terms[j].literal_len > 0)
      std::memcpy(reinterpret_cast<uint8_t*>(a.pool) + 8 * static_cast<int64_t>(a.term[j].lit_word),
                  terms[j].literal, static_cast<size_t>(terms[j].literal_len));
  a.side.nrows = nrows;
  a.side.bitmap_bytes = s->bitmap_bytes;
  a.side.fixed_size = s->fixed_size;
  a.nterms = num_terms;
  a.row_mask = row_mask;
  a.out_mask = out_mask;
  a.out_count = reinterpret_cast<unsigned long long*>(out_count);
  if (nrows == 0 && !out_count) return FURY_OK;
  return launch_checked(hs, &a, [&] { return launch_predicate(a, hs); });
}

// The key fields of one batch, as fury_row_group and fury_row_index_build check them: the selection, then
// no LIST / STRUCT / MAP key.  `fields` stands in for the column table check_selection wants, as in
// fury_row_hash.
static int check_key_fields(const std::string& f, const fury_schema* s, const int32_t* fields, int32_t num_keys,
                            int64_t nrows, const char* none, const char* route) {
  const int st = check_selection(s, fields, num_keys, nrows, fields, f, none, route);
  if (st) return st;
  for (int j = 0; j < num_keys; j++) {
    const int32_t k = fields[j];
    if (s->plan[k].kind == kOther || s->plan[k].kind == kListFixed)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": field " + std::to_string(k) + " (" + s->fields[k].name +
                           ") is a LIST / STRUCT / MAP: its stored bytes are not canonical (null "
                           "slots keep stale contents), so it cannot be a key");
  }
  return FURY_OK;
}

// The keys as fury_row_hash hashes them.
static void hash_key_args(const fury_schema* s, const int32_t* fields, int32_t num_keys, int64_t nrows,
                          ProjArgs* h) {
  h->ncols = num_keys;
  h->bitmap_bytes = s->bitmap_bytes;
  h->fixed_size = s->fixed_size;
  h->nrows = nrows;
  h->nt = 1;
  for (int j = 0; j < num_keys; j++) {
    const FieldPlan& p = s->plan[fields[j]];
    h->col[j].kind = p.kind;
    h->col[j].width = p.kind == kFixed ? p.width : p.kind == kDecimal ? 16 : 1;    // BOOL: one byte, 0 / 1
    h->col[j].slot = fields[j];
  }
}

// The batch and its keys into the argument block of group.hip's table kernels, after the source checks.
static int group_batch_args(const std::string& f, const fury_schema* s, const int32_t* fields, int32_t num_keys,
                            const void* rows, const int64_t* row_offsets, int64_t nrows,
                            const uint32_t* hashes, GroupArgs* a, ProjArgs* h) {
  int st = check_source(f, rows, row_offsets, rows_of(s), true, &a->side);
  if (st) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}}))) return st;
  a->side.nrows = nrows;
  a->side.bitmap_bytes = s->bitmap_bytes;
  a->side.fixed_size = s->fixed_size;
  a->nkeys = num_keys;
  a->hashes = hashes;
  hash_key_args(s, fields, num_keys, nrows, h);
  for (int j = 0; j < num_keys; j++) {
    a->key[j].left_slot = a->key[j].right_slot = fields[j];
    a->key[j].kind = h->col[j].kind;
    a->key[j].width = h->col[j].width;
  }
  return FURY_OK;
}

// Group ids and distinct rows (group.hip): BinaryRow's getters feeding a LinkedHashMap, null equal to null.
int fury_row_group(const fury_schema* s, const int32_t* fields, int32_t num_keys, const void* rows,
                   const int64_t* row_offsets, int64_t nrows, const uint32_t* hashes, int64_t* out_first,
                   int64_t* out_group_ids, int64_t* out_group_rows, int64_t* out_num_groups, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_group");
  int st = check_key_fields(f, s, fields, num_keys, nrows, "has no row fields to group by",
                            "there is no route: group by a subset of the keys, then each group by the rest");
  if (st) return st;
  if ((st = check_required(f, "out_first", out_first))) return st;
  if ((st = check_aligned(f, 8, {{"out_first", out_first}, {"out_group_ids", out_group_ids},
                                 {"out_group_rows", out_group_rows}, {"out_num_groups", out_num_groups}})))
    return st;
  if ((st = check_aligned(f, 4, {{"hashes", hashes}}))) return st;
  if (nrows > INT32_MAX) return invalid(f, "batch too large");
  GroupArgs a{};
  if (nrows == 0) {                               // no rows, no groups
    if (!out_num_groups) return FURY_OK;
    return launch_checked(hs, &a, [&] {
      return check_hip(hipMemsetAsync(out_num_groups, 0, 8, hs), "fury_row_group: memset");
    });
  }
  ProjArgs h{};
  if ((st = group_batch_args(f, s, fields, num_keys, rows, row_offsets, nrows, hashes, &a, &h))) return st;
  a.out_first = out_first;
  a.out_group_ids = out_group_ids;
  a.out_group_rows = out_group_rows;
  a.out_num_groups = out_num_groups;
  return launch_checked(hs, &a, [&] { return launch_group(a, &h, hs); });
}

// The slots of an index of nrows rows: group.hip's capacity.
int64_t fury_row_index_slots(int64_t nrows) {
  if (nrows < 0 || nrows > INT32_MAX) return -1;
  return group_table_slots(nrows);
}

// The table of fury_row_group, kept (group.hip): HashMap.putIfAbsent of every row's key fields.
int fury_row_index_build(const fury_schema* s, const int32_t* fields, int32_t num_keys, const void* rows,
                         const int64_t* row_offsets, int64_t nrows, const uint32_t* hashes, uint64_t* table,
                         int64_t table_slots, int64_t* out_first, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_index_build");
  int st = check_key_fields(f, s, fields, num_keys, nrows, "has no row fields to index",
                            "there is no route: index a subset of the keys and verify the rest with "
                            "fury_row_keys_equal");
  if (st) return st;
  if ((st = check_required(f, "table", table))) return st;
  if ((st = check_aligned(f, 8, {{"table", table}, {"out_first", out_first}}))) return st;
  if ((st = check_aligned(f, 4, {{"hashes", hashes}}))) return st;
  if (nrows > INT32_MAX) return invalid(f, "batch too large");
  if (table_slots != fury_row_index_slots(nrows))
    return invalid(f, "table_slots " + std::to_string(table_slots) + " is not fury_row_index_slots(" +
                          std::to_string(nrows) + ") = " + std::to_string(fury_row_index_slots(nrows)));
  GroupArgs a{};
  ProjArgs h{};
  if (nrows > 0) {
    if ((st = group_batch_args(f, s, fields, num_keys, rows, row_offsets, nrows, hashes, &a, &h))) return st;
    a.out_first = out_first;
  }
  return launch_checked(hs, &a, [&] { return launch_index_build(a, &h, table, table_slots, hs); });
}

// The probe of a hash join (lookup.hip): HashMap.get with every probe row's key fields.
int fury_row_lookup(const fury_key_side* probe, const fury_key_side* build, int32_t num_keys,
                    const uint64_t* table, int64_t table_slots, const uint32_t* probe_hashes, int32_t flags,
                    int64_t* out_rows, uint32_t* out_mask, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_lookup");
  int st = check_required(f, "probe", probe);
  if (st) return st;
  if ((st = check_required(f, "build", build))) return st;
  const fury_key_side* sides[2] = {probe, build};
  const std::string names[2] = {f + ": probe", f + ": build"};
  if ((st = check_key_sides(f, sides, names, "probe", "build", num_keys))) return st;
  for (int s = 0; s < 2; s++)
    if (sides[s]->indices) return invalid(names[s], "indices must be null: the call takes whole batches");
  if ((st = check_required(f, "table", table))) return st;
  if (build->nrows > INT32_MAX) return invalid(names[1], "batch too large");
  if (table_slots != fury_row_index_slots(build->nrows))
    return invalid(f, "table_slots " + std::to_string(table_slots) + " is not fury_row_index_slots(" +
                          std::to_string(build->nrows) + ") = " +
                          std::to_string(fury_row_index_slots(build->nrows)));
  if (flags & ~FURY_KEYS_NULL_EQUAL) return invalid(f, "unknown flags " + std::to_string(flags));
  if (!out_rows && !out_mask) return invalid(f, "out_rows and out_mask are both null");
  if ((st = check_aligned(f, 8, {{"table", table}, {"out_rows", out_rows}}))) return st;
  if ((st = check_aligned(f, 4, {{"probe_hashes", probe_hashes}, {"out_mask", out_mask}}))) return st;
  for (int s = 0; s < 2; s++)
    if ((st = check_aligned(names[s], 8, {{"row_offsets", sides[s]->row_offsets}}))) return st;
  if (probe->nrows == 0) return FURY_OK;
  if ((probe->nrows + 255) / 256 > INT32_MAX) return invalid(names[0], "batch too large");
  LookupArgs a{};
  for (int s = 0; s < 2; s++) {
    const fury_schema* sc = sides[s]->schema;
    // an empty build batch has no rows and no offsets to read: every probe row finds nothing
    const bool any = sides[s]->nrows > 0;
    if ((st = check_source(names[s], sides[s]->rows, sides[s]->row_offsets, any ? rows_of(sc) : kFixedRows, any,
                           &a.side[s])))
      return st;
    a.side[s].nrows = sides[s]->nrows;
    a.side[s].bitmap_bytes = sc->bitmap_bytes;
    a.side[s].fixed_size = sc->fixed_size;
  }
  a.nkeys = num_keys;
  a.flags = flags;
  a.table = table;
  a.cap = static_cast<uint64_t>(table_slots);
  a.hashes = probe_hashes;
  a.out_rows = out_rows;
  a.out_mask = out_mask;
  fill_key_recs(probe, build, num_keys, a.key);
  ProjArgs h{};
  hash_key_args(probe->schema, probe->fields, num_keys, probe->nrows, &h);
  return launch_checked(hs, &a, [&] { return launch_lookup(a, &h, hs); });
}

// H of rule 1 on the host: a CPU worker routes a lookup key to the partition the device chose.
uint32_t fury_hash_bytes(const void* bytes, int64_t len, uint32_t seed) {
  if (len < 0 || len > INT32_MAX || (len > 0 && !bytes)) {
    set_error(FURY_ERR_INVALID_ARGUMENT,
              "fury_hash_bytes: len " + std::to_string(len) + " is not in [0, 2147483647] or bytes is null");
    return 0;
  }
  const uint8_t* p = static_cast<const uint8_t*>(bytes);
  uint32_t h = seed;
  const int64_t nb = len >> 2;
  for (int64_t i = 0; i < nb; i++)
    h = mm3_block(h, static_cast<uint32_t>(p[4 * i]) | static_cast<uint32_t>(p[4 * i + 1]) << 8 |
                         static_cast<uint32_t>(p[4 * i + 2]) << 16 |
                         static_cast<uint32_t>(p[4 * i + 3]) << 24);
  uint32_t k = 0;
  for (int64_t i = len - 1; i >= 4 * nb; i--) k = (k << 8) | p[i];
  if (len & 3) h = mm3_tail(h, k);
  return mm3_fmix(h ^ static_cast<uint32_t>(len));
}

uint32_t fury_hash_null(uint32_t seed) { return mm3_null(seed); }

// In-place update of selected fixed-width fields (update.hip): BinaryRow's setters over a batch.
int fury_row_update(const fury_schema* s, const int32_t* fields, int32_t num_selected, void* rows,
                    const int64_t* row_offsets, int64_t nrows, const fury_column* cols,
                    const uint8_t* row_mask, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_update");
  int st = check_selection(s, fields, num_selected, nrows, cols, f,
                           "has no row fields to update (re-encode it with fury_row_encode)",
                           "re-encode the batch (fury_row_encode)");
  if (st) return st;
  for (int j = 0; j < num_selected; j++) {
    const int32_t k = fields[j];
    if (s->plan[k].kind != kFixed && s->plan[k].kind != kBool)
      return set_error(FURY_ERR_UNSUPPORTED,
                       f + ": field " + std::to_string(k) + " (" + s->fields[k].name +
                           ") is not fixed-width: variable-length values cannot be updated in "
                           "place (re-encode the batch with fury_row_encode)");
  }
  if ((st = check_aligned(f, 4, {{"row_mask", row_mask}}))) return st;
  st = take_device_error(hs);
  if (st) return st;
  ProjArgs a{};
  a.ncols = num_selected;
  a.bitmap_bytes = s->bitmap_bytes;
  a.fixed_size = s->fixed_size;
  a.nrows = nrows;                    // a.nt stays 0: the update's accesses are plain (update.hip)
  for (int j = 0; j < num_selected && cols; j++) {
    const int32_t k = fields[j];
    const FieldPlan& p = s->plan[k];
    const fury_column& c = cols[j];
    ProjCol& v = a.col[j];
    const std::string who = "column " + std::to_string(j) + " (" + s->fields[k].name + ")";
    v.kind = p.kind;
    v.slot = k;
    v.width = p.kind == kBool ? 0 : p.width;
    v.values = static_cast<uint8_t*>(c.values);       // inputs: the kernel only reads them
    v.validity = c.validity;
    if (c.validity && misaligned(c.validity, 4))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": validity must be 4-byte aligned");
    if (nrows > 0 && !c.values) return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values is null");
    if (misaligned(c.values, v.width > 1 ? v.width : v.width == 0 ? 4 : 1))
      return set_error(FURY_ERR_INVALID_ARGUMENT, who + ": values misaligned");
  }
  if (nrows == 0) return FURY_OK;
  if ((st = check_source(f, rows, row_offsets, rows_of(s), true))) return st;
  st = device_error_word(hs, &a.err);
  if (st) return st;
  // fixed schemas: row i at i * fixed_size, as in fury_row_project
  return launch_update(a, static_cast<uint8_t*>(rows), s->is_fixed ? nullptr : row_offsets, row_mask, hs);
}

// Row selection (take.hip): BinaryRow.copy() over a batch.  The source and output batch of take,
// filter and partition; `n` = output rows the copy may have to produce (take: num_selected, the others:
// nrows).
static int take_args(const std::string& f, const fury_schema* s, const void* rows,
                     const int64_t* row_offsets, int64_t nrows, int64_t n, void* out_rows,
                     int64_t out_capacity, int64_t* out_offsets, TakeArgs* a) {
  *a = TakeArgs{};
  int st = check_output(f, out_rows, out_capacity, out_offsets, a,
                        s->is_fixed ? nullptr : kNeedOutOffsets, n, s->fixed_size);
  if (st) return st;
  a->nrows = nrows;
  a->n = n;
  a->fixed_size = s->fixed_size;
  return check_source(f, rows, row_offsets, rows_of(s), n > 0 && nrows > 0 && out_rows, a);
}

int fury_row_take(const fury_schema* s, const void* rows, const int64_t* row_offsets, int64_t nrows,
                  const int64_t* indices, int64_t num_selected, void* out_rows,
                  int64_t out_capacity, int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_take");
  int st = check_required(f, "schema", s);
  if (st) return st;
  if ((st = check_count(f, "nrows", nrows))) return st;
  if ((st = check_count(f, "num_selected", num_selected))) return st;
  if (num_selected > 0 && (st = check_required(f, "indices", indices))) return st;
  if ((st = check_aligned(f, 8, {{"indices", indices}}))) return st;
  TakeArgs a;
  if ((st = take_args(f, s, rows, row_offsets, nrows, num_selected, out_rows, out_capacity, out_offsets, &a)))
    return st;
  a.indices = indices;
  return launch_checked(hs, &a, [&] { return launch_take(a, hs); });
}

int fury_row_filter(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, const uint8_t* row_mask, void* out_rows, int64_t out_capacity,
                    int64_t* out_offsets, int64_t* out_count, int64_t* out_indices, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_filter");
  int st = check_required(f, "schema", s);
  if (st) return st;
  if ((st = check_count(f, "nrows", nrows))) return st;
  if (nrows > 0 && (st = check_required(f, "row_mask", row_mask))) return st;
  if ((st = check_aligned(f, 4, {{"row_mask", row_mask}}))) return st;
  if ((st = check_required(f, "out_count", out_count))) return st;
  if ((st = check_aligned(f, 8, {{"out_count", out_count}, {"out_indices", out_indices}}))) return st;
  TakeArgs a;
  if ((st = take_args(f, s, rows, row_offsets, nrows, nrows, out_rows, out_capacity, out_offsets, &a)))
    return st;
  return launch_checked(hs, &a, [&] { return launch_filter(a, row_mask, out_count, out_indices, hs); });
}

// Rows split by a per-row partition id (partition.hip): filter from 2 ways to num_parts ways.
int fury_row_partition(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, const int32_t* part_ids, int32_t num_parts, void* out_rows,
                       int64_t out_capacity, int64_t* out_offsets, int64_t* out_part_rows,
                       int64_t* out_indices, int64_t* out_positions, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_partition");
  int st = check_required(f, "schema", s);
  if (st) return st;
  if ((st = check_count(f, "nrows", nrows))) return st;
  if (num_parts < 1 || num_parts > FURY_PARTITION_MAX_PARTS)
    return invalid(f, "num_parts " + std::to_string(num_parts) + " is not in [1, " +
                          std::to_string(FURY_PARTITION_MAX_PARTS) + "]");
  if (nrows > 0 && (st = check_required(f, "rows", rows))) return st;     // also to measure
  if (nrows > 0 && (st = check_required(f, "part_ids", part_ids))) return st;
  if ((st = check_aligned(f, 4, {{"part_ids", part_ids}}))) return st;
  if ((st = check_required(f, "out_part_rows", out_part_rows))) return st;
  if ((st = check_aligned(f, 8, {{"out_part_rows", out_part_rows}, {"out_indices", out_indices},
                                 {"out_positions", out_positions}})))
    return st;
  TakeArgs a;
  if ((st = take_args(f, s, rows, row_offsets, nrows, nrows, out_rows, out_capacity, out_offsets, &a)))
    return st;
  return launch_checked(hs, &a, [&] {
    return launch_partition(a, part_ids, num_parts, out_part_rows, out_indices, out_positions, hs);
  });
}

// Batches of one schema end to end (partition.hip): the vertical counterpart of fury_row_zip.
int fury_row_concat(const fury_schema* s, const fury_concat_source* sources, int32_t num_sources,
                    void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_concat");
  int st = check_required(f, "schema", s);
  if (st) return st;
  if ((st = check_required(f, "the source table", sources))) return st;
  if (num_sources < 1 || num_sources > FURY_CONCAT_MAX_SOURCES)
    return invalid(f, "num_sources " + std::to_string(num_sources) + " is not in [1, " +
                          std::to_string(FURY_CONCAT_MAX_SOURCES) + "]");
  ConcatArgs a{};
  for (int32_t k = 0; k < num_sources; k++) {
    const fury_concat_source& c = sources[k];
    const std::string src = f + ": source " + std::to_string(k);
    if ((st = check_count(src, "nrows", c.nrows))) return st;
    if (c.nrows > INT64_MAX - a.base[k]) return invalid(f, "batch too large");
    a.base[k + 1] = a.base[k] + c.nrows;
    if (c.nrows == 0) continue;       // an empty source is never read
    if ((st = check_source(src, c.rows, c.row_offsets, rows_of(s), true))) return st;
    if ((st = check_aligned(src, 8, {{"row_offsets", c.row_offsets}}))) return st;
    a.rows[k] = static_cast<const uint8_t*>(c.rows);
    a.ro[k] = s->is_fixed ? nullptr : c.row_offsets;    // fixed schemas: row i at i * fixed_size
  }
  a.nsrc = num_sources;
  a.fixed = s->is_fixed ? 1 : 0;
  a.fixed_size = s->fixed_size;
  a.n = a.base[num_sources];
  if ((st = too_large(a.n, s->fixed_size))) return set_error(st, f + ": batch too large");
  if ((st = check_aligned(f, 8, {{"out_offsets", out_offsets}}))) return st;
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a,
                         s->is_fixed ? nullptr : kNeedOutOffsets, a.n, s->fixed_size)))
    return st;
  return launch_checked(hs, &a, [&] { return launch_concat(a, hs); });
}

// A subset of the fields, as rows (select.hip): BinaryRow's getters feeding a BinaryRowWriter of the
// selected schema.  The host turns the selection into the int32 table SelectArgs describes.
int fury_row_select(const fury_schema* s, const int32_t* fields, int32_t num_selected,
                    const void* rows, const int64_t* row_offsets, int64_t nrows, void* out_rows,
                    int64_t out_capacity, int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_select");
  int st = check_field_selection(s, fields, num_selected, f);
  if (st) return st;
  if ((st = check_count(f, "nrows", nrows))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"out_offsets", out_offsets}}))) return st;
  Selection sel = make_selection(num_selected, 4, [&](int32_t) { return s; },
                                 [&](int32_t j) { return fields[j]; });
  SelectArgs a{};
  if ((st = check_source(f, rows, row_offsets, rows_of(s), nrows > 0, &a))) return st;
  // rows of a fixed-width selection sit at r * out_fixed: their capacity is checked before the launch
  const char* need = "a selection with a variable-length field needs out_offsets";
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a, sel.var.empty() ? nullptr : need, nrows,
                         sel.out_fixed)))
    return st;
  finish_selection(&sel, num_selected, &a);
  a.nrows = nrows;
  a.bitmap_bytes = s->bitmap_bytes;
  a.fixed_size = s->fixed_size;
  return launch_checked(hs, &a, [&] {
    return launch_select(a, sel.table.data(), static_cast<int>(sel.table.size()), hs);
  });
}

// The fields of several batches joined row by row (zip.hip): fury_row_select with a source per pick.
int fury_row_zip(const fury_zip_source* sources, int32_t num_sources, const int32_t* picks,
                 int32_t num_picks, int64_t nrows, void* out_rows, int64_t out_capacity,
                 int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_zip");
  if (!sources) return invalid(f, "the source table is null");
  const fury_schema* schemas[FURY_ZIP_MAX_SOURCES] = {};
  for (int32_t s = 0; s < num_sources && s < FURY_ZIP_MAX_SOURCES; s++) schemas[s] = sources[s].schema;
  int st = check_zip_picks(schemas, num_sources, picks, num_picks, f);
  if (st) return st;
  if ((st = check_count(f, "nrows", nrows))) return st;
  Selection sel = make_selection(num_picks, 5, [&](int32_t j) { return schemas[picks[2 * j]]; },
                                 [&](int32_t j) { return picks[2 * j + 1]; });
  ZipArgs a{};
  for (int32_t j = 0; j < num_picks; j++) {
    sel.table[5 * static_cast<size_t>(j) + 4] = picks[2 * j];     // the source word
    a.used |= 1u << picks[2 * j];
  }
  for (int32_t s = 0; s < num_sources; s++) {       // a source no pick names is never read
    if (!((a.used >> s) & 1)) continue;
    const std::string src = f + ": source " + std::to_string(s);
    if ((st = check_aligned(src, 8, {{"row_offsets", sources[s].row_offsets}}))) return st;
    if ((st = check_source(src, sources[s].rows, sources[s].row_offsets, rows_of(schemas[s]), nrows > 0,
                           &a.src[s])))
      return st;
    a.src[s].bitmap_bytes = schemas[s]->bitmap_bytes;
    a.src[s].fixed_size = schemas[s]->fixed_size;
  }
  if (sel.out_fixed > INT32_MAX - 7) return invalid(f, "the zipped row header exceeds 2 GiB");
  if ((st = check_aligned(f, 8, {{"out_offsets", out_offsets}}))) return st;
  const char* need = "picks with a variable-length field need out_offsets";
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a, sel.var.empty() ? nullptr : need, nrows,
                         sel.out_fixed)))
    return st;
  finish_selection(&sel, num_picks, &a);
  a.nrows = nrows;
  return launch_checked(hs, &a, [&] {
    return launch_zip(a, sel.table.data(), static_cast<int>(sel.table.size()), hs);
  });
}

// Nested values as batches (extract.hip): getStruct / getArray / getMap over a batch.  The path is
// resolved on the host (schema.cpp); the per-level widths travel in the argument block.
int fury_row_extract(const fury_schema* s, const int32_t* path, int32_t path_len, const void* rows,
                     const int64_t* row_offsets, int64_t nrows, void* out_rows,
                     int64_t out_capacity, int64_t* out_offsets, int64_t* out_count,
                     int64_t* out_indices, uint8_t* out_validity, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_extract");
  ExtractPath p;
  int st = resolve_extract_path(s, path, path_len, f, &p);
  if (st) return st;
  ExtractArgs a{};
  if ((st = check_count(f, "nrows", nrows))) return st;
  if ((st = check_source(f, rows, row_offsets, kOffsetRows, nrows > 0, &a))) return st;
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a, kOutOffsetsNull))) return st;
  if ((st = check_required(f, "out_count", out_count))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"out_offsets", out_offsets},
                                 {"out_count", out_count}, {"out_indices", out_indices}})))
    return st;
  if ((st = check_aligned(f, 4, {{"out_validity", out_validity}}))) return st;
  a.nrows = nrows;
  a.out_count = out_count;
  a.out_indices = out_indices;
  a.out_validity = reinterpret_cast<uint32_t*>(out_validity);
  set_path(&a, path_len, p.nfields, path);
  a.min_size = p.min_size;
  a.exact = p.exact;
  return launch_checked(hs, &a, [&] { return launch_extract(a, hs); });
}

// List and map elements as batches (explode.hip): BinaryArray.getStruct / getArray / getMap and
// BinaryMap.keyArray / valueArray over a batch.  Path, side and element type are resolved on the host
// (schema.cpp).
int fury_row_explode(const fury_schema* s, const int32_t* path, int32_t path_len, int32_t side,
                     const void* rows, const int64_t* row_offsets, int64_t nrows,
                     int64_t* out_list_offsets, uint8_t* out_entry_validity, int64_t elem_capacity,
                     void* out_rows, int64_t out_capacity, int64_t* out_offsets, int64_t* out_count,
                     int64_t* out_parents, int32_t* out_ordinals, uint8_t* out_validity,
                     void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_explode");
  ExplodePath p;
  int st = resolve_explode_path(s, path, path_len, side, f, &p);
  if (st) return st;
  ExplodeArgs a{};
  if ((st = check_count(f, "nrows", nrows))) return st;
  if ((st = check_source(f, rows, row_offsets, kOffsetRows, nrows > 0, &a))) return st;
  if ((st = check_required(f, "out_list_offsets", out_list_offsets))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"out_list_offsets", out_list_offsets}})))
    return st;
  if ((st = check_aligned(f, 4, {{"out_entry_validity", out_entry_validity}}))) return st;
  if (!out_offsets) {                 // the count form: no output batch, `a` keeps its zeros
    if (out_rows || out_count || out_parents || out_ordinals || out_validity)
      return invalid(f, "out_offsets is null (the count form): out_rows, out_count, out_parents, "
                        "out_ordinals and out_validity must be null too");
  } else {
    if ((st = check_count(f, "elem_capacity", elem_capacity))) return st;
    if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a, kOutOffsetsNull))) return st;
    if ((st = check_required(f, "out_count", out_count))) return st;
    if ((st = check_aligned(f, 8, {{"out_offsets", out_offsets}, {"out_count", out_count},
                                   {"out_parents", out_parents}})))
      return st;
    if ((st = check_aligned(f, 4, {{"out_ordinals", out_ordinals}, {"out_validity", out_validity}})))
      return st;
  }
  a.nrows = nrows;
  a.out_list_offsets = out_list_offsets;
  a.out_entry_validity = reinterpret_cast<uint32_t*>(out_entry_validity);
  a.elem_cap = out_offsets ? elem_capacity : 0;
  a.out_count = out_count;
  a.out_parents = out_parents;
  a.out_ordinals = out_ordinals;
  a.out_validity = reinterpret_cast<uint32_t*>(out_validity);
  set_path(&a, s->root != 0 ? 0 : path_len, p.path.nfields, path);
  a.min_size = 8;
  a.exact = 0;
  a.is_map = p.is_map;
  a.side = side;
  a.elem_min = p.elem_min;
  a.elem_exact = p.elem_exact;
  return launch_checked(hs, &a, [&] { return launch_explode(a, hs); });
}

// The checks fury_row_implode and fury_row_wrap share, after their schema checks; fills what both set.
static int implode_args(const OwnedField& value, const void* values, const int64_t* value_offsets,
                        int64_t num_values, int64_t nrows, void* out_rows, int64_t out_capacity,
                        int64_t* out_offsets, const std::string& f, ImplodeArgs* a) {
  *a = ImplodeArgs{};
  int st = check_count(f, "nrows", nrows);
  if (st) return st;
  if ((st = check_count(f, "num_values", num_values))) return st;
  if ((st = check_aligned(f, 8, {{"values", values}}))) return st;
  if ((st = check_required(f, "value_offsets", value_offsets))) return st;
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, a, kOutOffsetsNull))) return st;
  if ((st = check_aligned(f, 8, {{"value_offsets", value_offsets}, {"out_offsets", out_offsets}})))
    return st;
  if (num_values > 0 && (st = check_required(f, "values", values))) return st;
  a->values = static_cast<const uint8_t*>(values);
  a->value_offsets = value_offsets;
  a->num_values = num_values;
  a->nrows = nrows;
  a->least = 8;                       // [int64 numElements] / [int64 keyArrayBytes]
  if (value.type_id == FURY_TYPE_STRUCT) {
    const int64_t m = static_cast<int64_t>(value.children.size());
    a->least = static_cast<int32_t>(bitmap_bytes(m) + 8 * m);
  }
  return FURY_OK;
}

static bool is_nested(int32_t type_id) {
  return type_id == FURY_TYPE_STRUCT || type_id == FURY_TYPE_LIST || type_id == FURY_TYPE_MAP;
}

// Element rows back into LIST values (implode.hip): BinaryArrayWriter.reset(n) + write(ordinal,
// BinaryRow | BinaryArray | BinaryMap) over a batch, inside a one-field row or as the array itself.
int fury_row_implode(const fury_schema* s, const void* values, const int64_t* value_offsets,
                     int64_t num_values, const int64_t* list_offsets, int64_t nrows,
                     const uint8_t* entry_validity, const uint8_t* elem_validity,
                     int64_t num_elements, void* out_rows, int64_t out_capacity,
                     int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_implode");
  if (!s) return invalid(f, "schema is null");
  if (s->root == 0 && s->num_fields != 1)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": a row schema of " + std::to_string(s->num_fields) + " fields: the target "
                         "is a row schema with exactly one LIST field (join further fields with "
                         "fury_row_zip)");
  const OwnedField& list = s->fields[0];
  if (list.type_id == FURY_TYPE_MAP)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": the target " + list.name + " is a MAP: assembling a map needs a scalar "
                         "key array, which fury_row_explode does not produce");
  if (list.type_id != FURY_TYPE_LIST)
    return set_error(FURY_ERR_UNSUPPORTED, f + ": the target " + list.name + " is not a LIST");
  const OwnedField& elem = list.children[0];
  if (!is_nested(elem.type_id))
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": the elements of " + list.name + " are not STRUCT, LIST or MAP: such a list "
                         "encodes from a flat child column through fury_row_encode");
  if (s->root != 0 && entry_validity)
    return invalid(f, "entry_validity with a collection schema: an array entry is never null");
  int st = check_count(f, "num_elements", num_elements);
  if (st) return st;
  if ((st = check_required(f, "list_offsets", list_offsets))) return st;
  if ((st = check_aligned(f, 8, {{"list_offsets", list_offsets}}))) return st;
  if ((st = check_aligned(f, 4, {{"entry_validity", entry_validity}, {"elem_validity", elem_validity}})))
    return st;
  ImplodeArgs a;
  if ((st = implode_args(elem, values, value_offsets, num_values, nrows, out_rows, out_capacity,
                         out_offsets, f, &a)))
    return st;
  a.list_offsets = list_offsets;
  a.entry_validity = reinterpret_cast<const uint32_t*>(entry_validity);
  a.elem_validity = reinterpret_cast<const uint32_t*>(elem_validity);
  a.num_elements = num_elements;
  a.prefix = s->root == 0 ? 16 : 0;
  return launch_checked(hs, &a, [&] { return launch_implode(a, hs); });
}

// Nested values back into one-field rows (implode.hip): BinaryRowWriter.write(0, BinaryRow |
// BinaryArray | BinaryMap) over a batch.
int fury_row_wrap(const fury_schema* s, const void* values, const int64_t* value_offsets,
                  int64_t num_values, const uint8_t* validity, int64_t nrows, void* out_rows,
                  int64_t out_capacity, int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_wrap");
  if (!s) return invalid(f, "schema is null");
  if (s->root != 0)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": a collection schema: the target is a row schema with exactly one field");
  if (s->num_fields != 1)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": a row schema of " + std::to_string(s->num_fields) + " fields: the target "
                         "is a row schema with exactly one field (join further fields with "
                         "fury_row_zip)");
  const OwnedField& value = s->fields[0];
  if (!is_nested(value.type_id))
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": the target " + value.name + " is not a STRUCT, LIST or MAP");
  int st = check_aligned(f, 4, {{"validity", validity}});
  if (st) return st;
  ImplodeArgs a;
  if ((st = implode_args(value, values, value_offsets, num_values, nrows, out_rows, out_capacity,
                         out_offsets, f, &a)))
    return st;
  a.elem_validity = reinterpret_cast<const uint32_t*>(validity);
  a.num_elements = nrows;
  a.prefix = 16;
  a.wrap = 1;
  return launch_checked(hs, &a, [&] { return launch_implode(a, hs); });
}

// A map's key and value arrays as two batches (map.hip): BinaryMap.keyArray / valueArray over a batch.
// The path is resolved on the host (schema.cpp).
int fury_row_map_split(const fury_schema* s, const int32_t* path, int32_t path_len, const void* rows,
                       const int64_t* row_offsets, int64_t nrows, void* out_keys,
                       int64_t key_capacity, int64_t* out_key_offsets, void* out_values,
                       int64_t value_capacity, int64_t* out_value_offsets, int64_t* out_count,
                       int64_t* out_indices, uint8_t* out_validity, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_map_split");
  MapPath p;
  int st = resolve_map_path(s, path, path_len, f, &p);
  if (st) return st;
  MapSplitArgs a{};
  if ((st = check_count(f, "nrows", nrows))) return st;
  if ((st = check_count(f, "key_capacity", key_capacity))) return st;
  if ((st = check_count(f, "value_capacity", value_capacity))) return st;
  if ((st = check_source(f, rows, row_offsets, kOffsetRows, nrows > 0, &a))) return st;
  // the two output batches: a side is wanted when its offsets are given
  if ((st = check_aligned(f, 8, {{"out_keys", out_keys}, {"out_values", out_values}}))) return st;
  if (!out_key_offsets && !out_value_offsets)
    return invalid(f, "out_key_offsets and out_value_offsets are both null: no side is wanted");
  if ((out_keys && !out_key_offsets) || (out_values && !out_value_offsets))
    return invalid(f, "out_keys / out_values without its offsets (a side whose offsets are null "
                      "is skipped: its buffer must be null too)");
  if ((st = check_required(f, "out_count", out_count))) return st;
  if ((st = check_aligned(f, 8, {{"row_offsets", row_offsets}, {"out_key_offsets", out_key_offsets},
                                 {"out_value_offsets", out_value_offsets}, {"out_count", out_count},
                                 {"out_indices", out_indices}})))
    return st;
  if ((st = check_aligned(f, 4, {{"out_validity", out_validity}}))) return st;
  a.nrows = nrows;
  a.keys = MapSide{static_cast<uint8_t*>(out_keys), out_keys ? key_capacity : 0, out_key_offsets,
                   element_width(p.map->children[0].type_id)};
  a.vals = MapSide{static_cast<uint8_t*>(out_values), out_values ? value_capacity : 0,
                   out_value_offsets, element_width(p.map->children[1].type_id)};
  a.out_count = out_count;
  a.out_indices = out_indices;
  a.out_validity = reinterpret_cast<uint32_t*>(out_validity);
  set_path(&a, s->root != 0 ? 0 : path_len, p.path.nfields, path);
  a.min_size = 8;
  a.exact = 0;
  return launch_checked(hs, &a, [&] { return launch_map_split(a, hs); });
}

// Two array batches back into maps (map.hip): BinaryMap(keys, values, field) over a batch, inside a
// one-field row or as the map itself.
int fury_row_map_join(const fury_schema* s, const void* keys, const int64_t* key_offsets,
                      const void* values, const int64_t* value_offsets, int64_t num_values,
                      const uint8_t* validity, int64_t nrows, void* out_rows, int64_t out_capacity,
                      int64_t* out_offsets, void* stream) {
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const std::string f("fury_row_map_join");
  if (!s) return invalid(f, "schema is null");
  if (s->root == 0 && s->num_fields != 1)
    return set_error(FURY_ERR_UNSUPPORTED,
                     f + ": a row schema of " + std::to_string(s->num_fields) + " fields: the target "
                         "is a row schema with exactly one MAP field (join further fields with "
                         "fury_row_zip)");
  const OwnedField& map = s->fields[0];
  if (map.type_id != FURY_TYPE_MAP)
    return set_error(FURY_ERR_UNSUPPORTED, f + ": the target " + map.name + " is not a MAP");
  if (s->root != 0 && validity)
    return invalid(f, "validity with a collection schema: a map entry is never null");
  MapJoinArgs a{};
  int st = check_count(f, "nrows", nrows);
  if (st) return st;
  if ((st = check_count(f, "num_values", num_values))) return st;
  if ((st = check_aligned(f, 8, {{"keys", keys}, {"values", values}}))) return st;
  if ((st = check_required(f, "key_offsets", key_offsets))) return st;
  if ((st = check_required(f, "value_offsets", value_offsets))) return st;
  if ((st = check_output(f, out_rows, out_capacity, out_offsets, &a, kOutOffsetsNull))) return st;
  if ((st = check_aligned(f, 8, {{"key_offsets", key_offsets}, {"value_offsets", value_offsets},
                                 {"out_offsets", out_offsets}})))
    return st;
  if ((st = check_aligned(f, 4, {{"validity", validity}}))) return st;
  if (num_values > 0 && (st = check_required(f, "keys", keys))) return st;
  if (num_values > 0 && (st = check_required(f, "values", values))) return st;
  a.keys = static_cast<const uint8_t*>(keys);
  a.key_offsets = key_offsets;
  a.values = static_cast<const uint8_t*>(values);
  a.value_offsets = value_offsets;
  a.num_values = num_values;
  a.validity = reinterpret_cast<const uint32_t*>(validity);
  a.nrows = nrows;
  a.prefix = s->root == 0 ? 16 : 0;
  return launch_checked(hs, &a, [&] { return launch_map_join(a, hs); });
}

int fury_decode_prepare(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                        int64_t nrows, int64_t* node_entries, int64_t* node_bytes,
                        fury_decode_plan** plan, void* stream) {
  if (!s || !plan) return set_error(FURY_ERR_INVALID_ARGUMENT, "fury_decode_prepare: null argument");
  *plan = nullptr;
  std::unique_ptr<fury_decode_plan> p(new fury_decode_plan());
  const int st = decode_prepare(p.get(), s, rows, row_offsets, nrows, node_entries, node_bytes,
                                static_cast<hipStream_t>(stream));
  if (!st) *plan = p.release();
  return st;
}

}  // extern "C"

fury_decode_plan::~fury_decode_plan() {
  lv.reset();
  tree.reset();
  wide.reset();
  owned.reset();
  if (owned_stream) {
    release_error_slot(owned_stream);
    (void)hipStreamDestroy(owned_stream);
  }
}

int fury::decode_prepare(fury_decode_plan* p, const fury_schema* s, const void* rows,
                         const int64_t* row_offsets, int64_t nrows, int64_t* node_entries,
                         int64_t* node_bytes, hipStream_t hs) {
  if (nrows < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "nrows < 0");
  if (!s->device_ok) return set_error(FURY_ERR_UNSUPPORTED, "no device kernel for " + s->device_reason);
  if (nrows > 0 && (!rows || !row_offsets))
    return set_error(FURY_ERR_INVALID_ARGUMENT, "rows / row_offsets is null");
  if (const int e = take_device_error(hs)) return e;
  const int nn = static_cast<int>(s->nodes.size());
  p->schema = s;
  p->rows = static_cast<const uint8_t*>(rows);
  p->offs = row_offsets;
  p->nrows = nrows;
  std::vector<int64_t> totals(2 * nn, 0);
  // flat variable-length schemas of 17-256 fields: the wide kernels' count pass + scan, kept for
  // the execute (the tile bases), one host sync for the sequence fields' totals
  const bool wide_shape = nrows > 0 && !s->generic && !s->is_fixed && s->num_fields > 16 /* kRegCols: the register-staged kernels below */ &&
                          s->num_fields <= kMaxWideVarCols && knob::var_wide.load();
  int engine = knob::wide_engine.load();   // tuning.cpp: 0 auto, 1 the wide tiles, 2 the row walk
  int64_t bytes = -1;                      // the batch's bytes, row_offsets[nrows]: not read yet
  if (wide_shape && engine == 0) {
    int st = check_hip(hipMemcpyAsync(&bytes, row_offsets + nrows, 8, hipMemcpyDeviceToHost, hs),
                       "hipMemcpyAsync batch bytes");
    if (!st) st = check_hip(hipStreamSynchronize(hs), "hipStreamSynchronize");
    if (st) return st;
    engine = bytes > static_cast<int64_t>(knob::wide_walk_row.load()) * nrows ? 2 : 1;
  }
  const bool wide = wide_shape && engine != 2;
  if (wide) {
    VarArgs a;
    DeviceTable dt;
    std::vector<int64_t> seq;
    int st = var_args(s, nullptr, nrows, true, false, &a, &dt, hs, true);
    if (!st) {
      p->wide.reset(new WidePlan());
      st = wide_prepare(a, p->rows, row_offsets, hs, bytes, p->wide.get(), &seq);
    }
    if (!st) st = take_device_error(hs);
    if (st) return st;
    int q = 0;
    for (int k = 0; k < s->num_fields; k++) {
      totals[2 * k] = nrows;
      const int kind = s->plan[k].kind;
      if (kind != kBytes && kind != kListFixed) continue;
      if (kind == kBytes) totals[2 * k + 1] = seq[q];
      else totals[2 * s->nodes[k].first_child] = seq[q];
      q++;
    }
  } else if (nrows > 0) {
    // both engines synchronise `stream`: rows whose values leave the batch are reported here.
    // The tile-staged engine first; the level engine when it declines the batch.
    TreePlan* tree = nullptr;
    int st = tree_prepare(s, p->rows, row_offsets, nrows, bytes, hs, &tree, &totals);
    p->tree.reset(tree);
    if (!st && !tree) {
      if (const int e = take_device_error(hs)) {
        st = e;
      } else {
        totals.assign(2 * nn, 0);
        LvPlan* lv = nullptr;
        st = lv_prepare(s, p->rows, row_offsets, nrows, hs, &lv, &totals);
        p->lv.reset(lv);
      }
    }
    if (!st) {
      st = take_device_error(hs);
    } else {
      // the engine failed on the host (the level engine's element bound): errors its finished
      // kernels raised on the device come first (out of bounds > map count > budget, as the row
      // walk reports them), and no flag is left behind for the stream's next call
      const int e = take_device_error(hs);
      if (e && st != FURY_ERR_DEVICE) st = e;
    }
    if (st) return st;
  }
  for (int i = 0; i < nn; i++) {
    if (node_entries) node_entries[i] = totals[2 * i];
    if (node_bytes) node_bytes[i] = totals[2 * i + 1];
  }
  p->totals = totals;
  return FURY_OK;
}

extern "C" {

int fury_decode_execute(fury_decode_plan* p, fury_column* cols, int32_t arrow, void* stream) {
  if (!p) return set_error(FURY_ERR_INVALID_ARGUMENT, "fury_decode_execute: plan is null");
  GenArgs g;
  DeviceTable dt;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  int st = gen_args(p->schema, cols, p->nrows, true, arrow != 0, &g, &dt, hs);
  if (st) return st;
  if (p->nrows == 0) {              // an empty batch still yields valid Arrow offsets ([0])
    const GenNode* nodes = g.tab ? reinterpret_cast<const GenNode*>(dt.host.data()) : g.node;
    for (int i = 0; i < g.nnodes && !st; i++)
      if (nodes[i].offsets)
        st = check_hip(hipMemsetAsync(nodes[i].offsets, 0, 4, hs), "hipMemsetAsync offsets");
    return st;
  }
  const GenNode* outs = g.tab ? reinterpret_cast<const GenNode*>(dt.host.data()) : g.node;
  if (p->wide) {
    VarArgs a;
    DeviceTable vdt;
    st = var_args(p->schema, cols, p->nrows, true, arrow != 0, &a, &vdt, hs);
    if (st) return st;
    return wide_execute(a, p->rows, p->offs, hs, *p->wide);
  }
  if (p->tree) return tree_execute(p->tree.get(), outs, p->rows, p->offs, p->totals, hs);
  return lv_execute(p->lv.get(), outs, p->rows, p->offs, hs);
}

void fury_decode_plan_destroy(fury_decode_plan* p) { delete p; }

int fury_trim_workspace(int32_t device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "fury_trim_workspace: no such device");
  int cur = 0;
  (void)hipGetDevice(&cur);
  int st = check_hip(hipSetDevice(device), "hipSetDevice");
  if (st) return st;
  release_cached(device);
  st = check_hip(hipSetDevice(cur), "hipSetDevice");
  if (!st) drain_error_quarantine();
  return st;
}

int fury_device_status(void* stream) {
  const int st = check_hip(hipStreamSynchronize(static_cast<hipStream_t>(stream)),
                           "hipStreamSynchronize");
  if (st) return st;
  return take_device_error(static_cast<hipStream_t>(stream));
}

int fury_stream_release(void* stream) {
  release_error_slot(static_cast<hipStream_t>(stream));
  return FURY_OK;
}

int fury_frame_rows(const fury_schema* s, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, void* out, int64_t* frame_offsets, void* stream) {
  if (!s) return set_error(FURY_ERR_INVALID_ARGUMENT, "schema is null");
  if (s->root) return set_error(FURY_ERR_UNSUPPORTED, "row framing of a collection schema");
  if (nrows < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "nrows < 0");
  if (nrows == 0) return FURY_OK;
  if (!rows || !out) return set_error(FURY_ERR_INVALID_ARGUMENT, "rows/out is null");
  if (!s->is_fixed && !row_offsets)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "variable-length rows need row_offsets");
  return launch_frame_rows(static_cast<const uint8_t*>(rows), s->is_fixed ? nullptr : row_offsets,
                           nrows, s->fixed_size, s->schema_hash, static_cast<uint8_t*>(out),
                           frame_offsets, static_cast<hipStream_t>(stream));
}

int fury_unframe_rows(const fury_schema* s, const void* stream_bytes, int64_t stream_len,
                      int64_t nrows, void* rows_out, int64_t* row_offsets, void* stream) {
  if (!s) return set_error(FURY_ERR_INVALID_ARGUMENT, "schema is null");
  if (s->root) return set_error(FURY_ERR_UNSUPPORTED, "row framing of a collection schema");
  if (nrows < 0 || stream_len < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "negative size");
  if (nrows == 0) return FURY_OK;
  if (!stream_bytes || !rows_out || !row_offsets)
    return set_error(FURY_ERR_INVALID_ARGUMENT, "null buffer");
  return launch_unframe_rows(static_cast<const uint8_t*>(stream_bytes), stream_len, nrows,
                             s->schema_hash, static_cast<uint8_t*>(rows_out), row_offsets,
                             static_cast<hipStream_t>(stream));
}

int fury_arrow_ipc_schema(const fury_schema* s, uint8_t* out, int64_t cap, int64_t* len) {
  if (!s || !len) return set_error(FURY_ERR_INVALID_ARGUMENT, "schema/len is null");
  std::vector<uint8_t> msg;
  const int st = ipc_schema_message(s, &msg);
  if (st) return st;
  *len = static_cast<int64_t>(msg.size());
  if (!out) return FURY_OK;
  if (cap < *len) return set_error(FURY_ERR_CAPACITY, "IPC schema message needs " +
                                                          std::to_string(*len) + " bytes");
  std::memcpy(out, msg.data(), msg.size());
  return FURY_OK;
}

int fury_arrow_ipc_record_batch(const fury_schema* s, const fury_column* columns, int64_t nrows,
                                void* out, int64_t cap, int64_t* len, void* stream) {
  if (!s || !len) return set_error(FURY_ERR_INVALID_ARGUMENT, "schema/len is null");
  if (nrows < 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "nrows < 0");
  if (!columns && s->num_fields > 0) return set_error(FURY_ERR_INVALID_ARGUMENT, "columns is null");
  return ipc_record_batch(s, columns, nrows, static_cast<uint8_t*>(out), cap, len,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
