// hip_owned.h — every HIP resource of the host code is owned by one of these
// types and released by its destructor: device arrays (DevBuf), pinned host
// arrays (PinnedBuf), events, streams, a device list with the host mirror of
// what it holds (DevList), a timed pair of events (TimedSpan), and the ordering
// of consecutive operations that may come on different streams (StreamOrder).
// No kernels;
// only <hip/hip_runtime.h> types and calls.  The live objects of each kind are
// counted process-wide, here and nowhere else (pt_debug_live_resources).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

struct HipLiveCounts {
  std::atomic<long long> device_arrays{0}, device_bytes{0}, pinned_arrays{0}, events{0}, streams{0};
};
inline HipLiveCounts& hip_live() {
  static HipLiveCounts counts;
  return counts;
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    DevBuf t(std::move(o));
    swap(t);
    return *this;
  }
  ~DevBuf() { release(); }
  void swap(DevBuf& o) noexcept { std::swap(p, o.p), std::swap(n, o.n); }
  hipError_t reserve(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipDeviceSynchronize();  // renders in flight on other streams may still read the old array
    release();
    T* q = nullptr;
    const size_t m = std::max<size_t>(count, 1);
    hipError_t e = hipMalloc((void**)&q, m * sizeof(T));
    if (e == hipSuccess) adopt(q, m);
    return e;
  }
  void release() {
    if (p) (void)hipFree(give());
  }
  void adopt(T* q, size_t count) {  // take ownership of a hipMalloc'd array
    release();
    p = q;
    n = count;
    if (p) ++hip_live().device_arrays, hip_live().device_bytes += (long long)(n * sizeof(T));
  }
  T* give() {  // hand the array out and forget it
    if (p) --hip_live().device_arrays, hip_live().device_bytes -= (long long)(n * sizeof(T));
    n = 0;
    return std::exchange(p, nullptr);
  }
};
template <class T>
void swap(DevBuf<T>& a, DevBuf<T>& b) noexcept { a.swap(b); }

// A device list with a host mirror of what it holds: uploaded (on `s`) only
// when it changed -- the lists rarely change between frames.  Never a null
// device list: an empty one (a launch may cull every block) still has an array.
template <class D, class T = D>
struct DevList {
  static_assert(sizeof(D) == sizeof(T), "the list uploads without conversion");
  DevBuf<D> dev;
  std::vector<T> host;  // what `dev` holds
  hipError_t sync(const T* list, size_t n, hipStream_t s) {
    const D* held = dev.p;
    const hipError_t r = dev.reserve(n);
    if (dev.p != held) host.clear();  // (a new array holds nothing yet)
    if (r != hipSuccess) return r;
    if (n == host.size() && (n == 0 || std::memcmp(list, host.data(), n * sizeof(T)) == 0)) return hipSuccess;
    host.assign(list, list + n);  // (the copy's source outlives the call)
    if (n == 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dev.p, host.data(), n * sizeof(T), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) host.clear();  // (not what the device holds)
    return e;
  }
};

template <class T>
struct PinnedBuf {  // hipHostMalloc'd; grows only
  T* p = nullptr;
  size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  hipError_t reserve(size_t count) {
    if (count <= n) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) n = count, ++hip_live().pinned_arrays;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p), --hip_live().pinned_arrays;
    p = nullptr;
    n = 0;
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e), --hip_live().events;
  }
  hipError_t create(unsigned flags = hipEventDefault) {  // nothing to do for one that exists
    if (e) return hipSuccess;
    hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r == hipSuccess) ++hip_live().events;
    else e = nullptr;
    return r;
  }
  operator hipEvent_t() const { return e; }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s), --hip_live().streams;
  }
  hipError_t create(unsigned flags) {  // nothing to do for one that exists
    if (s) return hipSuccess;
    hipError_t r = hipStreamCreateWithFlags(&s, flags);
    if (r == hipSuccess) ++hip_live().streams;
    else s = nullptr;
    return r;
  }
  operator hipStream_t() const { return s; }
};

// The device time between two points of a stream, read when asked for.
struct TimedSpan {
  Event ev[2];
  bool timed = false;  // begin() and end() were recorded
  hipError_t create() {
    const hipError_t e = ev[0].create();
    return e == hipSuccess ? ev[1].create() : e;
  }
  hipError_t begin(hipStream_t s) {
    const hipError_t e = create();
    return e == hipSuccess ? hipEventRecord(ev[0], s) : e;
  }
  hipError_t end(hipStream_t s) {
    const hipError_t e = hipEventRecord(ev[1], s);
    if (e == hipSuccess) timed = true;
    return e;
  }
  // Waits for the end; nothing timed yet: *out is left as it is.
  hipError_t ms(float* out) const {
    if (!timed) return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev[1]);
    return e == hipSuccess ? hipEventElapsedTime(out, ev[0], ev[1]) : e;
  }
};

// Consecutive operations on one object are ordered: one that comes on another
// stream than the last waits for the last one's event.
struct StreamOrder {
  Event ev;  // (created at the first end())
  hipStream_t last = nullptr;
  bool recorded = false;
  hipError_t begin(hipStream_t s) { return recorded && last != s ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  hipError_t end(hipStream_t s) {
    hipError_t e = ev.create(hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, s);
    if (e == hipSuccess) last = s, recorded = true;
    return e;
  }
};
