// HIP (gfx950 / CDNA4) implementation of the device-op interface in ops.h: the handle's runtime.
//
// Memory pool + copies, short host waits, phase tracing without synchronisation, the calling thread's device, and
// the hipGraph replay of fixed-shape launch sequences.
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>
#include <cstdio>
#include <cstring>

#include "hip_common.h"

namespace ccz {

// ===========================================================================
// memory pool + copies
// ===========================================================================
void* dev_alloc(ccz_ctx* c, size_t bytes) {
  Impl* im = impl(c);
  if (bytes == 0) bytes = 8;
  bytes = (bytes + 255) & ~size_t(255);
  int best = -1;
  for (size_t i = 0; i < im->pool.size(); ++i) {
    PoolBlock& b = im->pool[i];
    if (!b.used && b.bytes >= bytes && b.bytes <= bytes + bytes / 4 + 4096) {
      if (best < 0 || b.bytes < im->pool[best].bytes) best = int(i);
    }
  }
  if (best >= 0) {
    im->pool[best].used = true;
    return im->pool[best].p.get();
  }
  DevMem<> p;
  if (env::once(env::TRACE_POOL)) fprintf(stderr, "[ccz] pool miss: hipMalloc(%zu) (%zu blocks cached)\n", bytes, im->pool.size());
  hipError_t e = hipMalloc(p.out(), bytes);
  if (e != hipSuccess) {
    // release cached blocks and retry once
    (void)hipGetLastError();
    pool_trim(c);
    e = hipMalloc(p.out(), bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); fail(CCZ_ENOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); }
  }
  im->pool.push_back({std::move(p), bytes, true});
  return im->pool.back().p.get();
}

size_t pool_trim(ccz_ctx* c) {
  Impl* im = impl(c);
  CCZ_HIP(hipStreamSynchronize(stream(c)));       // pooled blocks are recycled in stream order: nothing may still use them
  size_t freed = 0;
  for (auto it = im->pool.begin(); it != im->pool.end();) {
    if (!it->used) { freed += it->bytes; it = im->pool.erase(it); } else ++it;
  }
  return freed;
}

void dev_free(ccz_ctx* c, void* p) {
  if (!p) return;
  Impl* im = impl(c);
  for (auto& b : im->pool)
    if (b.p.get() == p) { b.used = false; return; }
  // not ours: stream-ordered work may still use it, so synchronise before freeing
  (void)hipStreamSynchronize(stream(c));
  (void)hipFree(p);
}

static void h2d_blocking(ccz_ctx* c, void* dst, const void* src, size_t bytes) {
  CCZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream(c)));
  CCZ_HIP(hipStreamSynchronize(stream(c)));  // src is pageable host memory owned by the caller
}
void h2d(ccz_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!bytes) return;
  // small copies (shifts, Ritz values, permutations: the solver's steering data) ride through the pinned ring and do not
  // make the host wait; the source may be reused as soon as this returns either way
  if (bytes <= Impl::kSmallBytes) { h2d_small(c, dst, src, bytes); return; }
  h2d_blocking(c, dst, src, bytes);
}
void h2d_small(ccz_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!bytes) return;
  Impl* im = impl(c);
  if (bytes > Impl::kSmallBytes) { h2d_blocking(c, dst, src, bytes); return; }
  // next slot of the ring whose previous copy has drained (a deep queue -- many enqueue-only calls behind a long
  // kernel -- must not make the host wait for the device: look for a free slot before blocking on the oldest one)
  int i = im->small_next;
  for (int t = 0; t < Impl::kSmallSlots; ++t) {
    const int j = (im->small_next + t) % Impl::kSmallSlots;
    if (!im->small_pin[j]) { i = j; break; }
    const hipError_t q = hipEventQuery(im->small_ev[j].get());
    if (q == hipSuccess) { i = j; break; }
    if (q != hipErrorNotReady) { (void)hipGetLastError(); }
  }
  if (!im->small_pin[i]) {
    if (hipHostMalloc(im->small_pin[i].out(), Impl::kSmallBytes, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(im->small_ev[i].out(), hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      im->small_pin[i].reset();
      h2d_blocking(c, dst, src, bytes);
      return;
    }
  } else {
    CCZ_HIP(hipEventSynchronize(im->small_ev[i].get()));      // (returns at once for a drained slot)
  }
  im->small_next = (i + 1) % Impl::kSmallSlots;
  std::memcpy(im->small_pin[i].get(), src, bytes);
  CCZ_HIP(hipMemcpyAsync(dst, im->small_pin[i].get(), bytes, hipMemcpyHostToDevice, stream(c)));
  CCZ_HIP(hipEventRecord(im->small_ev[i].get(), stream(c)));
}
// ---- short host waits ---------------------------------------------------------------------------------------------
// The solve is a chain of small launches with a handful of read-backs (pivot flags, residual norms, Ritz values).  A
// BLOCKING wait (hipStreamSynchronize: the thread sleeps on the completion interrupt) was measured to return 10 - 30 ms
// after the device had finished, in every OTHER fit of a back-to-back loop (DESIGN.md "the period-2 solve"): the device
// time of the phase was unchanged, the host sat in the wait.  Waits that are expected to be short therefore POLL the
// completion event (hipEventQuery) for up to `spin_ms` before they fall back to the blocking call.
// CCZ_SPIN_WAIT_MS=0 restores the blocking waits.
static double spin_budget_ms() { return env::once(env::SPIN_WAIT_MS); }
struct WaitStats { double total_ms = 0.0, max_ms = 0.0; long count = 0, fell_back = 0; };
static WaitStats& wait_stats() { static WaitStats w; return w; }

__global__ void k_copy_words(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) dst[i] = src[i];
  __threadfence_system();
}
// the same in 16-byte pieces (both pointers 16-byte aligned, n16 pieces): a store to host-mapped memory leaves the chip as one
// request per lane-group, and 8-byte lanes were seen to take 8 ms per 2 MB in some fits (bench extras: backproject 16 / 25 ms)
typedef unsigned int v4u32_copy __attribute__((ext_vector_type(4)));
__global__ void k_copy_words16(const v4u32_copy* __restrict__ src, v4u32_copy* __restrict__ dst, int64_t n16) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n16; i += int64_t(gridDim.x) * blockDim.x) dst[i] = src[i];
  __threadfence_system();
}

static void wait_stream_short(ccz_ctx* c) {
  Impl* im = impl(c);
  hipStream_t st = stream(c);
  const auto t0 = std::chrono::steady_clock::now();
  const double budget = spin_budget_ms();
  bool done = false;
  if (budget > 0.0) {
    if (!im->wait_ev) CCZ_HIP(hipEventCreateWithFlags(im->wait_ev.out(), hipEventDisableTiming));
    CCZ_HIP(hipEventRecord(im->wait_ev.get(), st));
    for (;;) {
      const hipError_t q = hipEventQuery(im->wait_ev.get());
      if (q == hipSuccess) { done = true; break; }
      if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
      if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > budget) break;
      __builtin_ia32_pause();
    }
  }
  if (!done) { CCZ_HIP(hipStreamSynchronize(st)); ++wait_stats().fell_back; }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  WaitStats& w = wait_stats();
  w.total_ms += ms;
  w.max_ms = std::max(w.max_ms, ms);
  ++w.count;
}

void d2h(ccz_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!bytes) return;
  Impl* im = impl(c);
  // small read-backs go through a pinned word buffer: the copy is then truly asynchronous (a pageable destination is
  // staged by the runtime, which may block inside the call) and the wait below polls
  if (bytes <= Impl::kD2hPinBytes && spin_budget_ms() > 0.0) {
    if (!im->d2h_pin) {
      if (hipHostMalloc(im->d2h_pin.out(), Impl::kD2hPinBytes, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
      } else if (hipHostGetDevicePointer(&im->d2h_pin_dev, im->d2h_pin.get(), 0) != hipSuccess) {
        (void)hipGetLastError();
        im->d2h_pin_dev = nullptr;
      }
    }
    const int mode = env::live(env::D2H_MODE);
    const bool trace = env::live(env::TRACE_D2H);
    hipEvent_t tev[2] = {im->d2h_tev[0].get(), im->d2h_tev[1].get()};
    const auto th0 = std::chrono::steady_clock::now();
    if (trace) {
      if (!tev[1]) {       // (the pair exists when its second event does)
        for (int i = 0; i < 2; ++i) { CCZ_HIP(hipEventCreate(im->d2h_tev[i].out())); tev[i] = im->d2h_tev[i].get(); }
      }
      CCZ_HIP(hipEventRecord(tev[0], stream(c)));
    }
    auto report = [&](const char* what) {
      if (!trace) return;
      float dev_ms = -1.f;
      (void)hipEventSynchronize(tev[1]);
      (void)hipEventElapsedTime(&dev_ms, tev[0], tev[1]);
      std::fprintf(stderr, "[ccz] d2h %s %zu bytes: device %.3f ms, host %.3f ms\n", what, bytes, dev_ms,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count());
    };
    if (mode == 4) {
      CCZ_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
      if (trace) { CCZ_HIP(hipEventRecord(tev[1], stream(c))); report("blocking"); }
      return;
    }
    if (im->d2h_pin) {
      // a KERNEL writes the pinned (host-mapped) buffer: no SDMA engine, hence no cross-engine dependency for the
      // runtime's helper thread to resolve -- with hipMemcpyAsync the event behind the copy was observed to complete
      // 15 - 19 ms late on the DEVICE time line in some fits (three read-backs of the back-projection phase)
      if (mode <= 1 && im->d2h_pin_dev && bytes % 8 == 0 && reinterpret_cast<uintptr_t>(src) % 8 == 0) {
        const int64_t words = int64_t(bytes / 8);
        if (mode == 1 && bytes % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0) {
          hipLaunchKernelGGL(k_copy_words16, dim3((unsigned)std::min<int64_t>((words / 2 + 255) / 256, 2048)), dim3(256), 0, stream(c),
                             static_cast<const v4u32_copy*>(src), static_cast<v4u32_copy*>(im->d2h_pin_dev), words / 2);
        } else {
          hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 2048)), dim3(256), 0, stream(c),
                             static_cast<const unsigned long long*>(src), static_cast<unsigned long long*>(im->d2h_pin_dev), words);
        }
        CCZ_LAUNCH_CHECK();
      } else {
        CCZ_HIP(hipMemcpyAsync(im->d2h_pin.get(), src, bytes, hipMemcpyDeviceToHost, stream(c)));
      }
      if (trace) CCZ_HIP(hipEventRecord(tev[1], stream(c)));
      if (mode == 3) CCZ_HIP(hipStreamSynchronize(stream(c)));
      else wait_stream_short(c);
      std::memcpy(dst, im->d2h_pin.get(), bytes);
      report(mode <= 1 ? "kernel" : "sdma");
      return;
    }
  }
  CCZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream(c)));
  CCZ_HIP(hipStreamSynchronize(stream(c)));
}
void d2d(ccz_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!bytes || dst == src) return;
  CCZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream(c)));
}
void zero(ccz_ctx* c, void* dst, size_t bytes) {
  if (!bytes) return;
  CCZ_HIP(hipMemsetAsync(dst, 0, bytes, stream(c)));
}
void sync(ccz_ctx* c) { CCZ_HIP(hipStreamSynchronize(stream(c))); }
void sync_short(ccz_ctx* c) { wait_stream_short(c); }
void wait_deferred(ccz_ctx* c) {
  Impl* im = impl(c);
  if (!im->deferred_event) return;
  hipEvent_t ev = static_cast<hipEvent_t>(im->deferred_event);
  im->deferred_event = nullptr;
  if (hipStreamWaitEvent(stream(c), ev, 0) != hipSuccess) {          // (an event destroyed meanwhile has nothing pending)
    (void)hipGetLastError();
    CCZ_HIP(hipDeviceSynchronize());
  }
}

// ---- phase tracing without synchronisation (ops.h: trace_mark / trace_flush) ----
__global__ void k_clock_probe(long long* out) {
  const long long c0 = __builtin_readcyclecounter(), w0 = wall_clock64();
  while (wall_clock64() - w0 < 2000) {}                     // 20 us of the constant 100 MHz counter
  if (threadIdx.x == 0) { out[0] = __builtin_readcyclecounter() - c0; out[1] = wall_clock64() - w0; }
}
namespace {
struct TraceMark { std::string name; hipEvent_t ev; double host_ms; };
struct TraceState {
  std::vector<TraceMark> marks;
  std::vector<hipEvent_t> spare;
  long long* probes = nullptr;      // 2 x 64 counters, device
  std::chrono::steady_clock::time_point t0;
};
TraceState& trace_state() { static TraceState s; return s; }
}  // namespace
void trace_mark(ccz_ctx* c, const char* name) {
  TraceState& ts = trace_state();
  if (ts.marks.size() >= 64) return;
  if (!ts.probes) CCZ_HIP(hipMalloc(reinterpret_cast<void**>(&ts.probes), 64 * 2 * sizeof(long long)));
  if (ts.marks.empty()) ts.t0 = std::chrono::steady_clock::now();
  hipEvent_t ev;
  if (!ts.spare.empty()) { ev = ts.spare.back(); ts.spare.pop_back(); }
  else CCZ_HIP(hipEventCreate(&ev));
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, stream(c), ts.probes + 2 * ts.marks.size());
  CCZ_HIP(hipEventRecord(ev, stream(c)));
  const double hm = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts.t0).count();
  ts.marks.push_back({name, ev, hm});
}
void trace_flush(ccz_ctx* c, const char* what) {
  TraceState& ts = trace_state();
  if (ts.marks.empty()) return;
  CCZ_HIP(hipStreamSynchronize(stream(c)));
  std::vector<long long> pr(ts.marks.size() * 2);
  CCZ_HIP(hipMemcpy(pr.data(), ts.probes, pr.size() * sizeof(long long), hipMemcpyDeviceToHost));
  std::string line;
  char buf[160];
  for (size_t i = 0; i < ts.marks.size(); ++i) {
    float dev_ms = 0.f;
    if (i > 0) (void)hipEventElapsedTime(&dev_ms, ts.marks[i - 1].ev, ts.marks[i].ev);
    const double mhz = pr[2 * i + 1] > 0 ? double(pr[2 * i]) / (double(pr[2 * i + 1]) / 100.0) : 0.0;
    snprintf(buf, sizeof(buf), " | %s dev %.2f host %.2f clk %.0f", ts.marks[i].name.c_str(), dev_ms,
             ts.marks[i].host_ms - (i > 0 ? ts.marks[i - 1].host_ms : 0.0), mhz);
    line += buf;
  }
  WaitStats& w = wait_stats();
  snprintf(buf, sizeof(buf), " || host waits: %ld, total %.2f ms, longest %.2f ms, %ld blocking", w.count, w.total_ms, w.max_ms, w.fell_back);
  line += buf;
  w = WaitStats{};
  fprintf(stderr, "[ccz] %s phases (ms; each phase includes a 20 us probe)%s\n", what, line.c_str());
  for (auto& m : ts.marks) ts.spare.push_back(m.ev);
  ts.marks.clear();
}
void activate(ccz_ctx* c) {
  CCZ_HIP(hipSetDevice(c->device));
  wave_kernels_init();
}
int device_current() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return dev;
}
void device_set(int dev) { (void)hipSetDevice(dev); }

// ---------------------------------------------------------------------------
// hipGraph replay of fixed-shape launch sequences.  `fn` must only enqueue work on the handle's stream
// (no allocation, no synchronisation, no host reads); the key must cover every value baked into the
// kernel arguments (shapes AND pointers).
// ---------------------------------------------------------------------------
static inline uint64_t key_mix(uint64_t h, uint64_t v) { return h ^ (v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)); }

template <typename F>
static void graph_run(ccz_ctx* c, uint64_t key, F&& fn) {
  Impl* im = impl(c);
  hipStream_t st = stream(c);
  if (!im->graphs_on || st == nullptr) { fn(); return; }
  for (auto& g : im->graphs)
    if (g.key == key) {
      g.tick = ++im->tick;
      CCZ_HIP(hipGraphLaunch(g.exec.get(), st));
      return;
    }
  if (env::once(env::TRACE_POOL)) fprintf(stderr, "[ccz] graph miss: capturing key %016llx (%zu cached)\n", (unsigned long long)key, im->graphs.size());
  if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) {
    (void)hipGetLastError();
    im->graphs_on = 0;
    fn();
    return;
  }
  hipGraph_t graph = nullptr;
  try {
    fn();
  } catch (...) {
    (void)hipStreamEndCapture(st, &graph);
    if (graph) (void)hipGraphDestroy(graph);
    throw;
  }
  CCZ_HIP(hipStreamEndCapture(st, &graph));
  GraphExec exec;
  if (hipGraphInstantiate(exec.out(), graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipGraphDestroy(graph);
    im->graphs_on = 0;
    fn();       // nothing ran during capture: run it for real
    return;
  }
  (void)hipGraphDestroy(graph);
  if (im->graphs.size() >= 96) {   // evict the least recently used
    size_t lru = 0;
    for (size_t i = 1; i < im->graphs.size(); ++i)
      if (im->graphs[i].tick < im->graphs[lru].tick) lru = i;
    im->graphs.erase(im->graphs.begin() + lru);
  }
  im->graphs.push_back({key, std::move(exec), ++im->tick});
  CCZ_HIP(hipGraphLaunch(im->graphs.back().exec.get(), st));
}

// the same for other translation units (evd_block.hip, potrf.hip): key helpers + a type-erased entry
uint64_t graph_key_mix(uint64_t h, uint64_t v) { return key_mix(h, v); }
void graph_run_fn(ccz_ctx* c, uint64_t key, const std::function<void()>& fn) { graph_run(c, key, fn); }

}  // namespace ccz

