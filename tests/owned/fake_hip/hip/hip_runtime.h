// A tiny stand-in for <hip/hip_runtime.h> (tests/owned/owned_driver.cpp): what
// csrc/hip_owned.h calls, over malloc / free and counted dummy handles.  Every
// call is counted or logged in `fake`, and the k-th allocation can be made to
// fail.  Test code of this project; its include path goes before ROCm's.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct FakeEvent* hipEvent_t;
typedef struct FakeStream* hipStream_t;
struct FakeEvent {
  int id;
};
struct FakeStream {
  int id;
};
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0 };

struct FakeHip {
  long long dev = 0, pinned = 0, events = 0, streams = 0;  // live now
  long long mallocs = 0, frees = 0, syncs = 0, events_made = 0;  // calls so far
  long long fail_at = 0;  // the k-th device or pinned allocation from now fails (0: none)
  std::vector<std::string> log;  // "sync", "free", "wait <stream> <event>", "record <event> <stream>"
};
inline FakeHip fake;

inline bool fake_alloc_fails() { return fake.fail_at > 0 && --fake.fail_at == 0; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (fake_alloc_fails()) return hipErrorOutOfMemory;
  if (bytes == 0) return hipErrorInvalidValue;  // (the owner never asks for nothing)
  *p = std::malloc(bytes);
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
  fake.log.push_back("record " + std::to_string(e->id) + " " + std::to_string(s->id));
  return hipSuccess;
}
