// Host side of a fit that is enqueued in chunks behind a device status word (ey.hip, als.hip): the kernels of a chunk return
// at once when the fit has stopped, so the host never waits inside a chunk.  After each chunk the status is copied into one of
// two pinned slots behind an event; the call that reuses the slot (two chunks later) waits for it and reports what it holds.
#pragma once

#include <vector>

#include "hip_common.h"

namespace ccz {

// every kernel of a fit reads the status word first and returns at once after the stop
template <typename Status>
__device__ __forceinline__ bool fit_stopped(const Status* st) { return st->stopped != 0; }

template <typename Status>
struct ChunkDriver {
  Status* dev = nullptr;                 // the device status, written by the family's finish kernel
  Status* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  int slot = 0;

  // throws on failure; destroy() then frees what exists
  void create(ccz_ctx* c) {
    dev = static_cast<Status*>(dev_alloc(c, sizeof(Status)));
    for (int i = 0; i < 2; ++i) {
      CCZ_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin[i]), sizeof(Status), hipHostMallocDefault));
      CCZ_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
  }
  // the handle's stream must be idle
  void destroy(ccz_ctx* c) {
    dev_free(c, dev);
    for (int i = 0; i < 2; ++i) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
  }
  // a new fit on this state, after a handle sync: no slot holds a chunk any more
  void reset() { used[0] = used[1] = false; }
  // wait for the chunk published in slot s: its status copy (valid on the host now), or null when the slot is unused
  const Status* wait(int s) {
    if (!used[s]) return nullptr;
    CCZ_HIP(hipEventSynchronize(ev[s]));
    return pin[s];
  }
  // behind the chunk just enqueued: copy the status to the current slot, record its event, move to the other slot
  void publish(ccz_ctx* c) {
    CCZ_HIP(hipMemcpyAsync(pin[slot], dev, sizeof(Status), hipMemcpyDeviceToHost, stream(c)));
    CCZ_HIP(hipEventRecord(ev[slot], stream(c)));
    used[slot] = true;
    slot ^= 1;
  }
};

// the view arguments of a step / sweep call against the widths p of the fit state; `fam` ("ey", "als") leads the messages
inline void check_views(const char* fam, const ccz_view* views, const std::vector<int64_t>& p) {
  if (!views) fail(CCZ_EINVAL, "%s: null views", fam);
  for (int i = 0; i < int(p.size()); ++i) {
    if (!views[i].data) fail(CCZ_EINVAL, "%s: null view %d", fam, i);
    if (views[i].cols != p[i])
      fail(CCZ_EINVAL, "%s: view %d has %lld columns, the fit state %lld", fam, i, (long long)views[i].cols, (long long)p[i]);
    if (views[i].ld < views[i].cols) fail(CCZ_EINVAL, "%s: view %d: ld < cols", fam, i);
  }
}

template <typename State>
State* as_state(const char* fam, void* st) {
  if (!st) fail(CCZ_EINVAL, "%s: null fit state", fam);
  return static_cast<State*>(st);
}

}  // namespace ccz
