// A tiny stand-in for <hip/hip_runtime.h> (tests/owned/owned_driver.cpp): what
// csrc/hip_owned.h and csrc/tile_seam.cpp call, over malloc / free and counted
// dummy handles.  Every call is counted or logged in `fake`; the k-th
// allocation, copy or event synchronise can be made to fail, and event
// synchronises can be held at a gate.  Test code of this project; its include
// path goes before ROCm's.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct FakeEvent* hipEvent_t;
typedef struct FakeStream* hipStream_t;
struct FakeEvent {
  int id;
  float stamp = 0.f;  // the fake clock at the last record
};
struct FakeStream {
  int id;
};
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
struct int4 {
  int x, y, z, w;
};
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }

struct FakeHip {
  long long dev = 0, pinned = 0, events = 0, streams = 0;  // live now
  long long mallocs = 0, frees = 0, syncs = 0, events_made = 0;  // calls so far
  long long fail_at = 0;  // the k-th device or pinned allocation from now fails (0: none)
  std::vector<std::string> log;  // "sync", "free", "wait <stream> <event>", "record <event> <stream>"
  long long copies = 0, copy_fail_at = 0;  // hipMemcpyAsync calls so far; the k-th from now fails
  float clock = 0.f;  // + 1.5 at every record
  // hipEventSynchronize is the one call that comes from a second thread (the
  // seam's completion thread): what it touches is guarded by `mu`.
  std::mutex mu;
  std::condition_variable cv;
  bool gate = false;                // a synchronise waits for a permit
  long long permits = 0;
  long long evsync_fail_at = 0;     // the k-th synchronise from now fails
  std::vector<int> evsyncs;         // event ids, in the order the synchronises returned
};
inline FakeHip fake;

inline bool fake_alloc_fails() { return fake.fail_at > 0 && --fake.fail_at == 0; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (fake_alloc_fails()) return hipErrorOutOfMemory;
  if (bytes == 0) return hipErrorInvalidValue;  // (the owner never asks for nothing)
  *p = std::malloc(bytes);
  std::memset(*p, 0xCD, bytes);  // (a new array holds nothing yet)
  ++fake.dev, ++fake.mallocs;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  if (p) --fake.dev, ++fake.frees, fake.log.push_back("free");
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
  *p = nullptr;
  if (fake_alloc_fails()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  ++fake.pinned;
  return hipSuccess;
}
inline hipError_t hipHostFree(void* p) {
  if (p) --fake.pinned;
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  *e = new FakeEvent{(int)++fake.events_made};
  ++fake.events;
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  --fake.events;
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = new FakeStream{(int)++fake.streams + 100};
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  delete s;
  --fake.streams;
  return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() {
  ++fake.syncs;
  fake.log.push_back("sync");
  return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  fake.log.push_back("wait " + std::to_string(s->id) + " " + std::to_string(e->id));
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  e->stamp = fake.clock += 1.5f;
  fake.log.push_back("record " + std::to_string(e->id) + " " + std::to_string(s->id));
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  ++fake.copies;
  if (fake.copy_fail_at > 0 && --fake.copy_fail_at == 0) return hipErrorInvalidValue;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e) {
  std::unique_lock<std::mutex> lk(fake.mu);
  if (fake.gate) {
    fake.cv.wait(lk, [] { return fake.permits > 0; });
    --fake.permits;
  }
  fake.evsyncs.push_back(e->id);
  return fake.evsync_fail_at > 0 && --fake.evsync_fail_at == 0 ? hipErrorInvalidValue : hipSuccess;
}
inline void fake_permit(long long n) {  // lets n gated synchronises through
  {
    std::lock_guard<std::mutex> lk(fake.mu);
    fake.permits += n;
  }
  fake.cv.notify_all();
}
inline size_t fake_evsyncs() {
  std::lock_guard<std::mutex> lk(fake.mu);
  return fake.evsyncs.size();
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = b->stamp - a->stamp;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
