// Stand-alone check of csrc/hip_owned.h (tests/test_hip_owned.py) against the
// fake HIP of tests/owned/fake_hip: built with AddressSanitizer +
// UndefinedBehaviorSanitizer, leaks detected.  Every CHECK that fails prints its
// line and the program exits 1; "owned ok" at the end.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <utility>

#include "hip_owned.h"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// The live counts of hip_owned.h equal the fake's own at every step
// (`unowned`: arrays handed out with give() and not yet adopted).
static void counts_agree(long long arrays, long long bytes, long long unowned = 0) {
  const HipLiveCounts& n = hip_live();
  CHECK(n.device_arrays + unowned == fake.dev && n.pinned_arrays == fake.pinned && n.events == fake.events &&
        n.streams == fake.streams);
  CHECK(n.device_arrays == arrays);
  CHECK(n.device_bytes == bytes);
}

static size_t count_log(const std::string& what) {
  size_t k = 0;
  for (const std::string& s : fake.log) k += s == what;
  return k;
}

static void test_reserve() {
  DevBuf<float> b;
  CHECK(b.reserve(0) == hipSuccess && b.p && b.n == 1);  // count 0 still yields an array
  counts_agree(1, 4);
  CHECK(fake.syncs == 0);
  float* first = b.p;
  CHECK(b.reserve(1) == hipSuccess && b.p == first && fake.mallocs == 1);  // no more than is held: left alone
  fake.log.clear();
  CHECK(b.reserve(10) == hipSuccess && b.n == 10 && fake.mallocs == 2 && fake.frees == 1);
  CHECK(fake.log.size() == 2 && fake.log[0] == "sync" && fake.log[1] == "free");  // freed after a device synchronise
  counts_agree(1, 40);
  b.p[9] = 1.0f;  // (the whole array is there)
  first = b.p;
  CHECK(b.reserve(7) == hipSuccess && b.p == first && b.n == 10 && fake.mallocs == 2);
  // a failed growth leaves nothing held
  fake.fail_at = 1;
  CHECK(b.reserve(11) == hipErrorOutOfMemory && !b.p && b.n == 0);
  counts_agree(0, 0);
  CHECK(b.reserve(3) == hipSuccess && b.n == 3);
  counts_agree(1, 12);
}

static void test_adopt_give() {
  DevBuf<int> a, b;
  CHECK(a.reserve(4) == hipSuccess && b.reserve(6) == hipSuccess);
  counts_agree(2, 40);
  const long long frees = fake.frees;
  int* q = b.give();  // leaves nothing to free
  CHECK(q && !b.p && b.n == 0);
  counts_agree(1, 16, 1);
  CHECK(fake.dev == 2 && fake.frees == frees);  // (the array lives on, unowned)
  a.adopt(q, 6);  // frees what was held
  CHECK(fake.frees == frees + 1 && a.p == q && a.n == 6);
  counts_agree(1, 24);
  { DevBuf<int> gone = std::move(b); }  // an empty one frees nothing
  CHECK(fake.frees == frees + 1);
  a.release();
  CHECK(!a.p && fake.frees == frees + 2);
  counts_agree(0, 0);
}

static void test_move_swap() {
  const long long frees = fake.frees;
  {
    DevBuf<double> a;
    CHECK(a.reserve(5) == hipSuccess);
    double* pa = a.p;
    DevBuf<double> b(std::move(a));  // move construction: one owner
    CHECK(!a.p && a.n == 0 && b.p == pa && b.n == 5);
    counts_agree(1, 40);
    DevBuf<double> c;
    CHECK(c.reserve(2) == hipSuccess);
    double* pc = c.p;
    counts_agree(2, 56);
    std::swap(b, c);  // through the moves
    CHECK(b.p == pc && b.n == 2 && c.p == pa && c.n == 5);
    swap(b, c);  // the type's own
    CHECK(b.p == pa && b.n == 5 && c.p == pc && c.n == 2);
    b.swap(c);
    CHECK(b.p == pc && c.p == pa);
    counts_agree(2, 56);
    CHECK(fake.frees == frees);
    c = std::move(b);  // move assignment frees the target's array and leaves the source empty
    CHECK(fake.frees == frees + 1 && !b.p && b.n == 0 && c.p == pc && c.n == 2);
    counts_agree(1, 16);
  }  // a moved-from object's destructor frees nothing: one more free, not three
  CHECK(fake.frees == frees + 2);
  counts_agree(0, 0);
}

// The shape of ptk_build_lbvh: several arrays, a failure half-way, outputs
// handed out on success only.
static hipError_t build(int** out_a, float** out_b) {
  DevBuf<int> s0, s1, a;
  DevBuf<float> b, s2;
  for (auto* d : {&s0, &s1, &a})
    if (hipError_t e = d->reserve(8)) return e;
  if (hipError_t e = b.reserve(8)) return e;
  if (hipError_t e = s2.reserve(8)) return e;
  *out_a = a.give();
  *out_b = b.give();
  return hipSuccess;
}

static void test_failed_kth_allocation() {
  for (int k = 1; k <= 5; ++k) {
    int* oa = nullptr;
    float* ob = nullptr;
    fake.fail_at = k;
    CHECK(build(&oa, &ob) == hipErrorOutOfMemory && !oa && !ob);
    counts_agree(0, 0);  // the k - 1 earlier ones went at the return
    CHECK(fake.dev == 0);
  }
  int* oa = nullptr;
  float* ob = nullptr;
  CHECK(build(&oa, &ob) == hipSuccess && oa && ob);
  counts_agree(0, 0, 2);
  CHECK(fake.dev == 2);  // the outputs alone live on, and are the caller's
  DevBuf<int> a;
  DevBuf<float> b;
  a.adopt(oa, 8);
  b.adopt(ob, 8);
  counts_agree(2, 64);
}

static void test_pinned() {
  PinnedBuf<float> p;
  CHECK(p.reserve(0) == hipSuccess && !p.p);
  CHECK(p.reserve(16) == hipSuccess && p.p && p.n == 16);
  counts_agree(0, 0);
  CHECK(fake.pinned == 1);
  float* q = p.p;
  CHECK(p.reserve(9) == hipSuccess && p.p == q && p.n == 16);  // grows only
  CHECK(p.reserve(17) == hipSuccess && p.n == 17 && fake.pinned == 1);
  p.p[16] = 1.0f;
  fake.fail_at = 1;
  CHECK(p.reserve(30) == hipErrorOutOfMemory && !p.p && p.n == 0 && fake.pinned == 0);
  counts_agree(0, 0);
  CHECK(p.reserve(2) == hipSuccess);
  counts_agree(0, 0);
}

static void test_event_stream_order() {
  {
    Event e;
    CHECK(!(hipEvent_t)e);
    CHECK(e.create() == hipSuccess && e.create(hipEventDisableTiming) == hipSuccess);  // twice: one event
    CHECK(fake.events == 1 && fake.events_made == 1 && (hipEvent_t)e);
    Stream s, t;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s.create(hipStreamNonBlocking) == hipSuccess);
    CHECK(t.create(hipStreamNonBlocking) == hipSuccess && fake.streams == 2);
    counts_agree(0, 0);

    StreamOrder o;
    fake.log.clear();
    CHECK(o.begin(s) == hipSuccess && fake.log.empty());  // the first begin waits for nothing
    CHECK(fake.events == 1);                              // (and needs no event)
    CHECK(o.end(s) == hipSuccess && fake.events == 2);    // created at the first end
    const std::string ev = std::to_string(((hipEvent_t)o.ev)->id), ids = std::to_string(((hipStream_t)s)->id),
                      idt = std::to_string(((hipStream_t)t)->id);
    CHECK(fake.log.size() == 1 && fake.log[0] == "record " + ev + " " + ids);
    CHECK(o.begin(s) == hipSuccess && fake.log.size() == 1);  // the same stream: nothing
    CHECK(o.end(s) == hipSuccess && fake.events == 2);
    fake.log.clear();
    CHECK(o.begin(t) == hipSuccess);  // another stream: exactly one wait, on the last event
    CHECK(fake.log.size() == 1 && fake.log[0] == "wait " + idt + " " + ev);
    CHECK(o.end(t) == hipSuccess && count_log("record " + ev + " " + idt) == 1);
    CHECK(o.begin(t) == hipSuccess && fake.log.size() == 2);
    CHECK(o.begin(s) == hipSuccess && fake.log.size() == 3 && fake.log[2] == "wait " + ids + " " + ev);
    counts_agree(0, 0);
  }
  CHECK(fake.events == 0 && fake.streams == 0);
  counts_agree(0, 0);
}

int main() {
  counts_agree(0, 0);
  test_reserve();
  counts_agree(0, 0);
  test_adopt_give();
  test_move_swap();
  test_failed_kth_allocation();
  counts_agree(0, 0);
  test_pinned();
  counts_agree(0, 0);
  test_event_stream_order();
  CHECK(fake.dev == 0 && fake.pinned == 0 && fake.events == 0 && fake.streams == 0);
  std::printf("owned ok\n");
  return 0;
}
