// tile_seam.h — the asynchronous one-tile seam (pt_tile_submit / pt_tile_finish).
// Submitted tiles wait in a queue until a batch is full, then render as ONE
// launch into the context's frame; the rows the batch spans are copied to the
// batch's own pinned stage and an event is recorded behind the copy.  A
// completion thread waits on that event and completes the batch -- copies its
// tiles into the caller's sampleBuffer and toColors them into its frameBuffer --
// OFF the stream, so the next batch's render never waits for host work (a
// stream host function would serialise them).
//
// Two threads use a TileSeam: the caller's (every method) and the completion
// thread.  The tile queue and the fault-injection counters are the caller's
// alone; everything both threads touch is private and guarded by `mu`.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_owned.h"

struct TileJob {
  int4 t;
  float* hdr;
  uint32_t* rgba;
};
struct TileBatch {
  std::vector<TileJob> jobs;
  PinnedBuf<float> stage;  // rows y0 .. y0 + rows - 1 of the frame
  int y0 = 0, W = 0, H = 0;
  Event ev;
};

class TileSeam {
 public:
  static constexpr int kMaxBatchesInFlight = 8;  // bounds the pinned staging memory
  // PT_TILE_BATCH (tiles per launch) and PT_FAULT_TILE_LAUNCH are read here.
  explicit TileSeam(int device);
  // Stops the completion thread, which completes the pending batches first.
  ~TileSeam();
  TileSeam(const TileSeam&) = delete;
  TileSeam& operator=(const TileSeam&) = delete;

  // The queue of submitted tiles: true when a batch is full.
  bool push(const TileJob& j) { return queue_.push_back(j), (int)queue_.size() >= batch_tiles_; }
  bool queued() const { return !queue_.empty(); }
  std::vector<TileJob> take_queue() { return std::move(queue_); }
  // PT_FAULT_TILE_LAUNCH=k: true for the k-th call (tests of the error path).
  bool fault_injected() { return fault_at_ > 0 && ++n_launches_ == fault_at_; }

  // A batch for the next launch: a completed one's stage and event where there
  // is one; waits while kMaxBatchesInFlight are in flight and none is free.
  // Starts the completion thread at first use.
  std::unique_ptr<TileBatch> acquire();
  // A batch that was not launched goes back for reuse.
  void give_back(std::unique_ptr<TileBatch> b);
  // A rendered batch, its event recorded behind the copy into its stage:
  // completed by the thread, in launch order.
  void submit(std::unique_ptr<TileBatch> b);
  // Keeps the first error for drain(); returns rc.
  int record_failure(int rc, const std::string& msg);
  // Waits until every submitted batch is completed; the first error since the
  // last drain (PT_OK: none), which is cleared.
  int drain(std::string* msg);

 private:
  void run();  // the completion thread

  const int device_;
  std::vector<TileJob> queue_;
  int batch_tiles_ = 256;  // 256 beat 16-128 and 1024 (profiles/r3/seam_native_batch_sweep.txt)
  int fault_at_ = 0, n_launches_ = 0;

  std::mutex mu_;  // guards everything below
  std::condition_variable cv_;
  std::deque<std::unique_ptr<TileBatch>> pending_;  // rendered batches awaiting completion, in launch order
  std::vector<std::unique_ptr<TileBatch>> free_;    // completed batches: stages and events for reuse
  int inflight_ = 0;                                // batches submitted and not yet completed
  int err_ = 0;                                     // first error (PT_OK: none)
  std::string errmsg_;
  bool stop_ = false;
  std::thread worker_;
};
