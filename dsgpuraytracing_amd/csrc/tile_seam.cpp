// tile_seam.cpp — see tile_seam.h.
#include "tile_seam.h"

#include <cstdlib>
#include <cstring>

#include "../../include/ptgpu.h"

// Completion of one batch (on the completion thread, after the batch's event):
// the tiles' pixels go from the batch's stage into the caller's sampleBuffer
// and, as PathTracer::raytrace_tile does at its end (pathtracer.cpp:610),
// through toColor into its frameBuffer.
static void tile_complete(const TileBatch* b) {
  for (const TileJob& j : b->jobs) {
    for (int y = j.t.y; y < j.t.y + j.t.w; ++y) {
      const size_t dst = ((size_t)y * (size_t)b->W + (size_t)j.t.x) * 3;
      const size_t src = ((size_t)(y - b->y0) * (size_t)b->W + (size_t)j.t.x) * 3;
      std::memcpy(j.hdr + dst, b->stage.p + src, (size_t)j.t.z * 3 * sizeof(float));
    }
    if (j.rgba) (void)pt_to_color(j.hdr, b->W, b->H, j.t.x, j.t.y, j.t.x + j.t.z, j.t.y + j.t.w, j.rgba);
  }
}

TileSeam::TileSeam(int device) : device_(device) {
  if (const char* tb = std::getenv("PT_TILE_BATCH")) {  // tuning knob: tiles per asynchronous launch
    const int v = std::atoi(tb);
    if (v >= 1) batch_tiles_ = v;
  }
  if (const char* f = std::getenv("PT_FAULT_TILE_LAUNCH")) fault_at_ = std::atoi(f);
}

TileSeam::~TileSeam() {
  if (!worker_.joinable()) return;
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  worker_.join();  // drains the pending batches first
}

// Batches in launch order; each waits for its own event only, so completing
// batch k overlaps the render of batch k+1.
void TileSeam::run() {
  (void)hipSetDevice(device_);
  for (;;) {
    std::unique_ptr<TileBatch> b;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || !pending_.empty(); });
      if (pending_.empty()) return;  // stopping, nothing left to complete
      b = std::move(pending_.front());
      pending_.pop_front();
    }
    const hipError_t e = hipEventSynchronize(b->ev);
    if (e == hipSuccess) tile_complete(b.get());
    std::lock_guard<std::mutex> lk(mu_);
    if (e != hipSuccess && err_ == PT_OK) {
      err_ = PT_E_HIP;
      errmsg_ = std::string("tile completion: ") + hipGetErrorString(e);
    }
    b->jobs.clear();
    free_.push_back(std::move(b));
    --inflight_;
    cv_.notify_all();
  }
}

std::unique_ptr<TileBatch> TileSeam::acquire() {
  std::unique_ptr<TileBatch> b;
  {
    std::unique_lock<std::mutex> lk(mu_);
    if (!worker_.joinable()) worker_ = std::thread(&TileSeam::run, this);
    cv_.wait(lk, [&] { return !free_.empty() || inflight_ < kMaxBatchesInFlight; });
    if (!free_.empty()) {
      b = std::move(free_.back());
      free_.pop_back();
    }
  }
  if (!b) b.reset(new TileBatch());
  return b;
}

void TileSeam::give_back(std::unique_ptr<TileBatch> b) {
  std::lock_guard<std::mutex> lk(mu_);
  free_.push_back(std::move(b));
}

void TileSeam::submit(std::unique_ptr<TileBatch> b) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    pending_.push_back(std::move(b));
    ++inflight_;
  }
  cv_.notify_all();
}

int TileSeam::record_failure(int rc, const std::string& msg) {
  std::lock_guard<std::mutex> lk(mu_);
  if (err_ == PT_OK) {
    err_ = rc;
    errmsg_ = msg;
  }
  return rc;
}

int TileSeam::drain(std::string* msg) {
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait(lk, [&] { return inflight_ == 0; });  // every batch copied and completed
  const int err = err_;
  *msg = std::move(errmsg_);
  err_ = PT_OK;
  errmsg_.clear();
  return err;
}
