// Stand-alone check of csrc/hip_owned.h and csrc/tile_seam.cpp
// (tests/test_hip_owned.py) against the fake HIP of tests/owned/fake_hip,
// where the seam's renders are copies the driver makes: built with AddressSanitizer +
// UndefinedBehaviorSanitizer, leaks detected.  Every CHECK that fails prints its
// line and the program exits 1; "owned ok" at the end.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <utility>

#include "../../include/ptgpu.h"
#include "hip_owned.h"
#include "tile_seam.h"

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

static void test_dev_list() {
  {
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    DevList<int> l;
    int a[6] = {1, 2, 3, 4, 5, 6};
    fake.copies = 0;
    CHECK(l.sync(a, 0, s) == hipSuccess && l.dev.p && fake.copies == 0);  // an empty list still has an array
    CHECK(l.sync(a, 4, s) == hipSuccess && l.dev.n == 4 && fake.copies == 1 && std::memcmp(l.dev.p, a, 16) == 0);
    const int* held = l.dev.p;
    CHECK(l.sync(a, 4, s) == hipSuccess && fake.copies == 1 && l.dev.p == held);  // equal contents: no upload
    a[2] = 9;
    CHECK(l.sync(a, 4, s) == hipSuccess && fake.copies == 2 && l.dev.p[2] == 9);
    CHECK(l.sync(a, 2, s) == hipSuccess && fake.copies == 3 && l.dev.p == held && l.host.size() == 2);  // shorter: the same array
    a[0] = 7;  // the mirror is the copy's source, not the caller's list
    CHECK(l.host[0] == 1 && l.dev.p[0] == 1);
    CHECK(l.sync(a, 6, s) == hipSuccess && fake.copies == 4 && l.dev.p != held && std::memcmp(l.dev.p, a, 24) == 0);  // grown
    counts_agree(1, 24);
    // a failed copy: the mirror is not what the device holds, so the same list uploads again
    a[5] = 8;
    fake.copy_fail_at = 1;
    CHECK(l.sync(a, 6, s) == hipErrorInvalidValue && l.host.empty());
    CHECK(l.sync(a, 6, s) == hipSuccess && fake.copies == 6 && l.dev.p[5] == 8);
    // a failed growth leaves no array and no mirror; the next array is new and
    // holds nothing yet, so the list the mirror held before uploads again
    fake.fail_at = 1;
    CHECK(l.sync(a, 7, s) == hipErrorOutOfMemory && !l.dev.p && l.host.empty() && fake.copies == 6);
    CHECK(l.sync(a, 6, s) == hipSuccess && fake.copies == 7 && std::memcmp(l.dev.p, a, 24) == 0);
    // so does it when the array was replaced behind the list
    l.dev.release();
    CHECK(l.sync(a, 6, s) == hipSuccess && fake.copies == 8 && std::memcmp(l.dev.p, a, 24) == 0);
    // a list of another type of the same size uploads without conversion
    struct Rect {
      int x, y, w, h;
    };
    DevList<int4, Rect> r;
    const Rect rect[2] = {{1, 2, 3, 4}, {5, 6, 7, 8}};
    CHECK(r.sync(rect, 2, s) == hipSuccess && r.dev.p[1].x == 5 && r.dev.p[1].w == 8);
  }
  counts_agree(0, 0);
}

static void test_timed_span() {
  {
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    TimedSpan t;
    float ms = -1.f;
    CHECK(t.ms(&ms) == hipSuccess && ms == -1.f && fake.events == 0);  // nothing timed: left as it is
    CHECK(t.create() == hipSuccess && t.create() == hipSuccess && fake.events == 2);
    fake.log.clear();
    CHECK(t.begin(s) == hipSuccess && !t.timed && fake.events == 2);
    CHECK(t.ms(&ms) == hipSuccess && ms == -1.f);
    CHECK(t.end(s) == hipSuccess && t.timed && fake.log.size() == 2);
    const size_t syncs = fake_evsyncs();
    CHECK(t.ms(&ms) == hipSuccess && ms == 1.5f && fake_evsyncs() == syncs + 1);  // waits for the end (the fake clock: 1.5 per record)
    CHECK(fake.evsyncs.back() == ((hipEvent_t)t.ev[1])->id);
    fake.evsync_fail_at = 1;
    CHECK(t.ms(&ms) == hipErrorInvalidValue);
    TimedSpan lazy;  // begin() makes the events where create() was not called
    CHECK(lazy.begin(s) == hipSuccess && lazy.end(s) == hipSuccess && fake.events == 4);
  }
  CHECK(fake.events == 0);
}

// ---- the tile seam.  A "render" here: rows [y0, y0 + rows) of a W-wide frame
// filled with `value` in the batch's stage, and the batch's event recorded.
static int n_to_color = 0;
extern "C" int pt_to_color(const float*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, uint32_t*) {
  return ++n_to_color, PT_OK;  // (on the completion thread; read after drain())
}

constexpr int kW = 4, kRows = 2;

static TileBatch* launch_batch(TileSeam& seam, hipStream_t s, float* hdr, int y0, float value, uint32_t* rgba = nullptr) {
  std::unique_ptr<TileBatch> b = seam.acquire();
  CHECK(b && b->jobs.empty());
  CHECK(b->stage.reserve(kW * kRows * 3) == hipSuccess && b->ev.create(hipEventDisableTiming) == hipSuccess);
  std::fill(b->stage.p, b->stage.p + kW * kRows * 3, value);
  CHECK(hipEventRecord(b->ev, s) == hipSuccess);
  b->jobs.push_back(TileJob{make_int4(1, y0, 2, kRows), hdr, rgba});  // columns 1 and 2 of the rows
  b->y0 = y0, b->W = kW, b->H = 64;
  TileBatch* raw = b.get();
  seam.submit(std::move(b));
  return raw;
}

// rows [y0, y0 + kRows): columns 1 and 2 hold `value`, the others are untouched (-1)
static bool rows_hold(const std::vector<float>& hdr, int y0, float value) {
  for (int y = y0; y < y0 + kRows; ++y)
    for (int x = 0; x < kW; ++x)
      for (int ch = 0; ch < 3; ++ch)
        if (hdr[((size_t)y * kW + x) * 3 + ch] != (x == 1 || x == 2 ? value : -1.f)) return false;
  return true;
}

static void test_seam_queue_and_faults() {
  setenv("PT_TILE_BATCH", "2", 1);
  setenv("PT_FAULT_TILE_LAUNCH", "2", 1);
  TileSeam seam(0);
  unsetenv("PT_TILE_BATCH");
  unsetenv("PT_FAULT_TILE_LAUNCH");
  CHECK(!seam.queued());
  CHECK(!seam.push(TileJob{make_int4(0, 0, 1, 1), nullptr, nullptr}) && seam.queued());
  CHECK(seam.push(TileJob{make_int4(1, 0, 1, 1), nullptr, nullptr}));  // a full batch
  const std::vector<TileJob> jobs = seam.take_queue();
  CHECK(jobs.size() == 2 && jobs[1].t.x == 1 && !seam.queued());
  CHECK(!seam.fault_injected() && seam.fault_injected() && !seam.fault_injected());  // the second launch only
  std::string msg = "?";
  CHECK(seam.drain(&msg) == PT_OK && msg.empty());  // nothing submitted: nothing to wait for, no thread
  CHECK(seam.record_failure(PT_E_INVALID, "first") == PT_E_INVALID && seam.record_failure(PT_E_HIP, "second") == PT_E_HIP);
  CHECK(seam.drain(&msg) == PT_E_INVALID && msg == "first");  // the first error, once
  CHECK(seam.drain(&msg) == PT_OK && msg.empty());
}

static void test_seam_completion() {
  std::vector<float> hdr(64 * kW * 3, -1.f);
  std::string msg;
  std::atomic<bool> destroying{false};
  std::thread opener;
  {
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    TileSeam seam(0);
    // batches complete in launch order, each after its own event
    fake.gate = true;
    fake.evsyncs.clear();
    std::vector<int> ids;
    uint32_t rgba = 0;
    for (int k = 0; k < 3; ++k) ids.push_back(((hipEvent_t)launch_batch(seam, s, hdr.data(), 2 * k, (float)k, k == 1 ? &rgba : nullptr)->ev)->id);
    CHECK(fake_evsyncs() == 0);
    fake_permit(3);
    CHECK(seam.drain(&msg) == PT_OK && msg.empty());
    CHECK(fake.evsyncs == ids && ids[0] != ids[1] && ids[1] != ids[2]);
    for (int k = 0; k < 3; ++k) CHECK(rows_hold(hdr, 2 * k, (float)k));
    CHECK(n_to_color == 1);  // the one job with a frameBuffer
    CHECK(fake.pinned == 3 && fake.events == 3);  // kept for reuse

    // with kMaxBatchesInFlight in flight and none free, acquire waits until one completes
    std::vector<std::unique_ptr<TileBatch>> taken;  // (the three free ones, out of the way)
    for (int k = 0; k < 3; ++k) taken.push_back(seam.acquire());
    fake.evsyncs.clear();
    TileBatch* first = nullptr;
    for (int k = 0; k < TileSeam::kMaxBatchesInFlight; ++k) {
      TileBatch* b = launch_batch(seam, s, hdr.data(), 2 * k, 10.f + k);
      if (k == 0) first = b;
    }
    CHECK(fake.pinned == 3 + TileSeam::kMaxBatchesInFlight);
    std::atomic<bool> entering{false};
    std::thread helper([&] {
      while (!entering) std::this_thread::yield();
      fake_permit(1);
    });
    entering = true;
    std::unique_ptr<TileBatch> ninth = seam.acquire();
    CHECK(fake_evsyncs() >= 1 && ninth.get() == first && rows_hold(hdr, 0, 10.f));  // the completed one, reused
    CHECK(fake.pinned == 3 + TileSeam::kMaxBatchesInFlight);
    helper.join();
    seam.give_back(std::move(ninth));
    for (auto& b : taken) seam.give_back(std::move(b));
    fake_permit(TileSeam::kMaxBatchesInFlight - 1);
    CHECK(seam.drain(&msg) == PT_OK);
    for (int k = 0; k < TileSeam::kMaxBatchesInFlight; ++k) CHECK(rows_hold(hdr, 2 * k, 10.f + k));
    fake.gate = false;

    // a failed synchronise: its tiles are not copied; drain reports it once
    fake.evsync_fail_at = 2;
    launch_batch(seam, s, hdr.data(), 20, 30.f);
    launch_batch(seam, s, hdr.data(), 22, 31.f);
    launch_batch(seam, s, hdr.data(), 24, 32.f);
    CHECK(seam.drain(&msg) == PT_E_HIP && msg == "tile completion: fake error");
    CHECK(rows_hold(hdr, 20, 30.f) && rows_hold(hdr, 22, -1.f) && rows_hold(hdr, 24, 32.f));
    CHECK(seam.drain(&msg) == PT_OK && msg.empty());

    // destruction with batches pending completes them
    fake.gate = true;
    for (int k = 0; k < 3; ++k) launch_batch(seam, s, hdr.data(), 30 + 2 * k, 40.f + k);
    opener = std::thread([&] {
      while (!destroying) std::this_thread::yield();
      fake_permit(3);
    });
    destroying = true;
  }  // (the seam's destructor returns once the gate was opened and the three are complete)
  opener.join();
  fake.gate = false;
  for (int k = 0; k < 3; ++k) CHECK(rows_hold(hdr, 30 + 2 * k, 40.f + k));
  CHECK(fake.pinned == 0 && fake.events == 0 && fake.streams == 0);
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
  test_dev_list();
  test_timed_span();
  test_seam_queue_and_faults();
  test_seam_completion();
  CHECK(fake.dev == 0 && fake.pinned == 0 && fake.events == 0 && fake.streams == 0);
  std::printf("owned ok\n");
  return 0;
}
