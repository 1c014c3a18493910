// launch_plan.h — the host policy of one render launch, as a pure function:
// from the frame, the camera, the scene box, the tile list, the device's
// occupancy numbers, an idle flag and the environment knobs to everything
// launch() (pt_api.cpp) enqueues.  Plain C++17, no HIP: it runs, and is
// tested (tests/test_launch_plan.py), without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ptgpu.h"
#include "pt_tuning.h"

struct PlanRect {  // (x, y, w, h): a tile or a block, laid out as the device's int4
  int x, y, w, h;
};

// The launch knobs: environment variables for A/Bs, tests and diagnostics
// (tools/knob_sweep.py), read by read_launch_knobs() and nowhere else.
struct LaunchKnobs {
  bool no_footprint_cull = false;  // PT_NO_FOOTPRINT_CULL (set): trace every pixel of the tiles
  int sample_group = 0;            // PT_SAMPLE_GROUP > 0: samples per work slot (clamped to spp); changes the summation order
  int tile_zorder = -1;            // PT_TILE_ZORDER=0/1: tiles in Z-order off / on (-1: by frame and tree size)
  bool census = false;             // PT_CENSUS (set): plain launches record per-wave census records, unpipelined
  int leaf_weight = 0;             // PT_LEAF_WEIGHT >= 1 (0: PT_LEAF_WEIGHT / PT_LEAF_WEIGHT_ENV)
  bool no_tri_only = false;        // PT_NO_TRI_ONLY (set): the kernel with the sphere test on triangle-only scenes
  bool no_helpers = false;         // PT_NO_HELPERS (set): drain helpers off
  int drain_div = 0;               // PT_DRAIN_DIV 0..64 (0: the 3/4 rule)
  int shade_batch = 0;             // PT_SHADE_BATCH 1..64 (0: PT_SHADE_BATCH / PT_SHADE_BATCH_ENV)
  bool debug_pixel = false;        // PT_DEBUG_PIXEL (set): frame batches render one frame per launch
  int debug_x = -1, debug_y = -1;  // PT_DEBUG_PIXEL=x,y: the kernel's printf trace of one pixel (-1: none)
  bool force_global_tables = false;  // PT_FORCE_GLOBAL_TABLES (set): the build with material tables in global memory
  bool waves_set = false;          // PT_WAVES_PER_CU (set): no halved grid for small launches, one wave budget
  int waves_per_cu = 0;            // PT_WAVES_PER_CU > 0: the resident grid (0: the kernel variant's occupancy)
  int chunk_slots = 0;             // PT_CHUNK_SLOTS 64..PT_CHUNK_BIG, a multiple of 64: the queue claim (0: by frame size)
  int queue_bands = -1;            // PT_QUEUE_BANDS=0/1: queue bands off / on (-1: by frame and tree size)
  // read once per process:
  bool pipeline = true;      // PT_PIPELINE=0: every render on the caller's stream, one slot
  bool small_launch = true;  // PT_SMALL_LAUNCH=0: no small-launch shape
  bool frame_batch = true;   // PT_FRAME_BATCH=0: pt_render_frames_device renders one frame per launch
};
LaunchKnobs read_launch_knobs();

struct PlanInput {
  int W = 0, H = 0, spp = 0;  // the frame
  pt_camera cam{};
  double box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};  // the scene box
  bool env = false;                                      // an environment light
  int n_bsdfs = 0, n_lights = 0;
  int64_t n_render_nodes = 0;  // 128-B nodes of the render tree
  int bvh_stack = 0;
  bool tri_only = false;
  int n_cu = 0, grid_plain = 0, grid_stats = 0;  // the device: CUs, resident waves of the plain / stats build
  int bpc_variant[4] = {0, 0, 0, 0};             // waves per CU of the plain builds [env * 2 + gtab]
  size_t stats_cap = 0;                          // u64 entries of the stats buffer (counters + per-wave records)
  const PlanRect* tiles = nullptr;               // clipped to the frame, in the caller's order
  size_t n_tiles = 0;
  int nf = 1;          // frames of the launch (a frame batch: > 1)
  uint32_t flags = 0;  // PT_FLAG_*
  bool gpu_idle = true;  // no earlier render of the context still running or queued
  LaunchKnobs knobs;
};

struct LaunchPlan {
  std::string error;  // not empty: the launch is refused (PT_E_INVALID), nothing else is valid
  // tile order: tile i of the launch is the caller's tile perm[i] (ztiles[i]); both empty without Z-order
  bool zorder = false;
  std::vector<int> perm;
  std::vector<PlanRect> ztiles;
  std::vector<PlanRect> blocks;  // <= 8x8 rectangles of each tile clipped to the cull rectangle, tile by tile
  std::vector<int> tile_block0;  // first block of tile i, then the end (n_tiles + 1)
  int64_t pixels = 0, culled_px = 0;  // of the tiles; of them outside the cull rectangle
  int cull[4] = {0, 0, 0, 0};         // (x0, y0, x1, y1) inclusive, not clamped to the frame
  int footprint[4] = {0, 0, 0, 0};    // the same inside the frame for pt_stats, (0, 0, -1, -1) when empty
  int group_spp = 1, n_groups = 1, group_shift = 0;
  uint32_t grp_m = 0, grp_sh = 0, frm_m = 0, frm_sh = 0;  // fastdiv by n_groups / by frame_slots
  int64_t frame_slots = 0, slots = 0;                     // work slots of one frame, of the launch (nf frames)
  int64_t want = 0;                                       // the resident grid asked for
  int grid = 1;                                           // workgroups launched
  bool gtab = false, stats = false, small = false;
  int chunk = PT_CHUNK, qbands = 0, sblocks = 0;
  int shade_batch = 0, leaf_weight = 0, drain_div = 0, tri_only = 0, helpers = 1, census = 0, dbg_pix = -1;
  // buffers to reserve: floats of this launch's group sums, ints of its stack
  // spill (0: none); for a frame batch also what EVERY render slot gets at once
  size_t partial_floats = 0, spill_ints = 0;
  size_t batch_partial_floats = 0, batch_spill_ints = 0;
};
LaunchPlan plan_launch(const PlanInput& in);

// The plain build with material tables in global memory (a kernel variant of its own).
bool global_tables(const PlanInput& in);
// Frames of in.tiles one launch of a frame batch takes, at most nf (in.nf is
// not read); `frame_slots`: the work slots of one frame it counted with.
int frames_that_fit(const PlanInput& in, int nf, int64_t* frame_slots = nullptr);

// Pieces of the plan, for the tests:
bool footprint_rect(const pt_camera& cam, const double lo[3], const double hi[3], int W, int H, int r[4]);
void screen_footprint(const PlanInput& in, int cull[4]);
int64_t traced_px(const PlanInput& in);
int group_size(int64_t traced, bool env, int spp, int sample_group, int64_t lanes, int64_t frame_blocks,
               int64_t budget_waves);
