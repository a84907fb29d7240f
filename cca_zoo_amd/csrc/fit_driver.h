// Host side of a fit that is enqueued in chunks behind a device status word (ey.hip; als.hip, which also runs SCCA_ADMM;
// gfa.hip): the kernels of a chunk return at once when the fit has stopped, so the host never waits inside a chunk.  After each
// chunk the status is copied into one of two pinned slots behind an event; the call that reuses the slot (two chunks later)
// waits for it and reports what it holds.  The rest of the file is what every family needs around that: the state that owns
// the device buffers, the create-time checks, the dtype dispatch, the view table, the chunk call and the launch planning.
#pragma once

#include <algorithm>
#include <vector>

#include "hip_common.h"

namespace ccz {

// every kernel of a fit reads the status word first and returns at once after the stop
template <typename Status>
__device__ __forceinline__ bool fit_stopped(const Status* st) { return st->stopped != 0; }

template <typename Status>
struct ChunkDriver {
  Status* dev = nullptr;                 // the device status, written by the family's finish kernel
  PinMem<Status> pin[2];
  Event ev[2];
  bool used[2] = {false, false};
  int slot = 0;

  // throws on failure; what exists then goes with the state
  void create(ccz_ctx* c) {
    dev = static_cast<Status*>(dev_alloc(c, sizeof(Status)));
    for (int i = 0; i < 2; ++i) {
      CCZ_HIP(hipHostMalloc(pin[i].out(), sizeof(Status), hipHostMallocDefault));
      CCZ_HIP(hipEventCreateWithFlags(ev[i].out(), hipEventDisableTiming));
    }
  }
  // the handle's stream must be idle (the pinned slots and the events go with the state)
  void destroy(ccz_ctx* c) { dev_free(c, dev); }
  // a new fit on this state, after a handle sync: no slot holds a chunk any more
  void reset() { used[0] = used[1] = false; }
  // wait for the chunk published in slot s: its status copy (valid on the host now), or null when the slot is unused
  const Status* wait(int s) {
    if (!used[s]) return nullptr;
    CCZ_HIP(hipEventSynchronize(ev[s].get()));
    return pin[s].get();
  }
  // behind the chunk just enqueued: copy the status to the current slot, record its event, move to the other slot
  void publish(ccz_ctx* c) {
    CCZ_HIP(hipMemcpyAsync(pin[slot].get(), dev, sizeof(Status), hipMemcpyDeviceToHost, stream(c)));
    CCZ_HIP(hipEventRecord(ev[slot].get(), stream(c)));
    used[slot] = true;
    slot ^= 1;
  }
};

// what every fit state holds; the family derives from it and adds its own buffers and parameters
template <typename Status>
struct FitState {
  int dtype = 0, M = 0;
  int64_t chunk = 0;
  std::vector<int64_t> p;
  ChunkDriver<Status> drv;
  std::vector<void*> allocs;

  // `count` (at least one) elements of device memory, freed by release()
  template <typename T = double>
  T* get(ccz_ctx* c, size_t count) {
    allocs.push_back(dev_alloc(c, std::max<size_t>(count, 1) * sizeof(T)));
    return static_cast<T*>(allocs.back());
  }
  void release(ccz_ctx* c) {
    sync(c);
    for (void* a : allocs) dev_free(c, a);
    allocs.clear();
    drv.destroy(c);
  }
  // a new fit on this state: the pinned status slots may still be in use by an earlier one
  void restart(ccz_ctx* c) {
    sync(c);
    drv.reset();
  }
};

template <typename State>
void free_state(ccz_ctx* c, State* S) {
  S->release(c);
  delete S;
}
// a new State filled by `fill` (its checks, its allocations, drv.create); when that throws, whatever it got is freed
template <typename State, typename Fill>
State* new_state(ccz_ctx* c, Fill fill) {
  State* S = new State();
  try {
    fill(*S);
  } catch (...) {
    free_state(c, S);
    throw;
  }
  return S;
}

// create-time checks; `fam` ("ey", "als", "gfa") leads the messages
inline void check_dtype(const char* fam, int dtype) {
  if (dtype != CCZ_F32 && dtype != CCZ_F64) fail(CCZ_EUNSUP, "%s: dtype must be CCZ_F32 or CCZ_F64", fam);
}
inline void check_view_count(const char* fam, int M, int most) {
  if (M < 1 || M > most) fail(CCZ_EUNSUP, "%s: 1 to %d views are supported, got %d", fam, most, M);
}
inline void check_no_empty_view(const char* fam, int M, const int64_t* p) {
  for (int i = 0; i < M; ++i)
    if (p[i] < 1) fail(CCZ_EINVAL, "%s: view %d has no columns", fam, i);
}

// f(T()) with T the element type of the views
template <typename F>
decltype(auto) by_dtype(int dtype, F&& f) {
  return dtype == CCZ_F32 ? f(float()) : f(double());
}

// at most `most` chunks of at least 64 rows each: rc rows per chunk, nchunk chunks
inline void row_chunks(int64_t n, int64_t most, int* nchunk, int* rc) {
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(most, (n + 63) / 64));
  *rc = int((n + want - 1) / want);
  *nchunk = int((n + *rc - 1) / *rc);
}

// column splits of a kernel that takes `rows_per_workgroup` rows x one column range per workgroup: enough workgroups to fill
// the device when there are few rows; every split at least 4096 columns wide
inline int column_splits(int64_t n, int rows_per_workgroup, int64_t p, int most) {
  const int64_t rowgroups = (n + rows_per_workgroup - 1) / rows_per_workgroup;
  const int64_t cs = std::min<int64_t>((2048 + rowgroups - 1) / rowgroups, std::max<int64_t>(1, p / 4096));
  return int(std::max<int64_t>(1, std::min<int64_t>(cs, most)));
}

// the view arguments of a call against the widths p of the fit state, into X / mu / ld of the family's view table
template <typename Views>
void fill_views(const char* fam, Views& vw, const ccz_view* views, const void* const* means, const std::vector<int64_t>& p) {
  if (!views) fail(CCZ_EINVAL, "%s: null views", fam);
  for (int i = 0; i < int(p.size()); ++i) {
    if (!views[i].data) fail(CCZ_EINVAL, "%s: null view %d", fam, i);
    if (views[i].cols != p[i])
      fail(CCZ_EINVAL, "%s: view %d has %lld columns, the fit state %lld", fam, i, (long long)views[i].cols, (long long)p[i]);
    if (views[i].ld < views[i].cols) fail(CCZ_EINVAL, "%s: view %d: ld < cols", fam, i);
    vw.X[i] = views[i].data;
    vw.mu[i] = means ? means[i] : nullptr;
    vw.ld[i] = views[i].ld;
  }
}

template <typename State>
State* as_state(const char* fam, void* st) {
  if (!st) fail(CCZ_EINVAL, "%s: null fit state", fam);
  return static_cast<State*>(st);
}

// One chunk of n units (`unit` names the argument in the message).  `prepare()` runs the family's own checks and returns its
// view table; the chunk that used the current slot is waited for and reported (`count` is the counter of the status, -1 when
// the slot is unused); `staged(slot)` may ride on the free slot; `enqueue(views, t)` runs n times; the status is published.
template <typename State, typename Status, typename Prepare, typename Enqueue, typename Staged = void (*)(int)>
void run_chunk(ccz_ctx* c, const char* fam, const char* unit, State& S, int64_t n, int64_t* known, int* stopped_known,
               long long Status::*count, Prepare prepare, Enqueue enqueue, Staged staged = [](int) {}) {
  if (n < 0 || n > S.chunk) fail(CCZ_EINVAL, "%s: %s must be 0..%lld", fam, unit, (long long)S.chunk);
  const auto vw = prepare();
  const int slot = S.drv.slot;
  const Status* seen = S.drv.wait(slot);
  if (known) *known = seen ? seen->*count : -1;
  if (stopped_known) *stopped_known = seen ? seen->stopped : 0;
  staged(slot);
  for (int64_t t = 0; t < n; ++t) enqueue(vw, t);
  S.drv.publish(c);
}

}  // namespace ccz
