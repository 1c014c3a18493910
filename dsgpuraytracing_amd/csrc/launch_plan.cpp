// launch_plan.cpp — the host policy of a render launch (launch_plan.h).
#include "launch_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

LaunchKnobs read_launch_knobs() {
  LaunchKnobs k;
  auto num = [](const char* name, int lo, int hi, int& out) {  // a value in [lo, hi], else the default stays
    if (const char* s = std::getenv(name)) {
      const int v = std::atoi(s);
      if (v >= lo && v <= hi) out = v;
    }
  };
  auto on = [](const char* name) {  // unset or non-zero
    const char* s = std::getenv(name);
    return !s || std::atoi(s) != 0;
  };
  k.no_footprint_cull = std::getenv("PT_NO_FOOTPRINT_CULL") != nullptr;
  num("PT_SAMPLE_GROUP", 1, INT32_MAX, k.sample_group);
  if (std::getenv("PT_TILE_ZORDER")) k.tile_zorder = on("PT_TILE_ZORDER") ? 1 : 0;
  k.census = std::getenv("PT_CENSUS") != nullptr;
  num("PT_LEAF_WEIGHT", 1, INT32_MAX, k.leaf_weight);
  k.no_tri_only = std::getenv("PT_NO_TRI_ONLY") != nullptr;
  k.no_helpers = std::getenv("PT_NO_HELPERS") != nullptr;
  num("PT_DRAIN_DIV", 0, 64, k.drain_div);
  num("PT_SHADE_BATCH", 1, 64, k.shade_batch);
  if (const char* dp = std::getenv("PT_DEBUG_PIXEL")) {  // diagnostics only
    k.debug_pixel = true;
    int dx = -1, dy = -1;
    if (std::sscanf(dp, "%d,%d", &dx, &dy) == 2 && dx >= 0 && dy >= 0) k.debug_x = dx, k.debug_y = dy;
  }
  k.force_global_tables = std::getenv("PT_FORCE_GLOBAL_TABLES") != nullptr;
  k.waves_set = std::getenv("PT_WAVES_PER_CU") != nullptr;
  num("PT_WAVES_PER_CU", 1, INT32_MAX, k.waves_per_cu);
  if (const char* cs = std::getenv("PT_CHUNK_SLOTS")) {  // (64..PT_CHUNK_BIG, a multiple of 64)
    const int v = std::atoi(cs);
    if (v >= 64 && v <= PT_CHUNK_BIG && v % 64 == 0) k.chunk_slots = v;
  }
  if (std::getenv("PT_QUEUE_BANDS")) k.queue_bands = on("PT_QUEUE_BANDS") ? 1 : 0;
  static const bool pipeline = on("PT_PIPELINE"), small_launch = on("PT_SMALL_LAUNCH"), frame_batch = on("PT_FRAME_BATCH");
  k.pipeline = pipeline;
  k.small_launch = small_launch;
  k.frame_batch = frame_batch;
  return k;
}

// Conservative pixel rectangle covering the scene box as seen by the camera.
// Camera::generate_ray (camera.cpp:113-129) sends every ray of every pixel
// through the pinhole `pos` with direction c2w * ((fx-.5)W/d, (fy-.5)H/d, -1);
// a box entirely in front of the pinhole projects inside the rectangle of its
// 8 projected corners.  Rays start one unit BEHIND the pinhole, so the
// rectangle is only used when the box lies in front of the pinhole plane;
// otherwise (false) no pixel can be culled.  One pixel of margin absorbs
// rounding.  r = (x0, y0, x1, y1), inclusive, NOT clamped to the frame.
bool footprint_rect(const pt_camera& cam, const double lo[3], const double hi[3], int W, int H, int r[4]) {
  for (int i = 0; i < 3; ++i)  // coordinates by dot products need an orthonormal c2w
    for (int j = 0; j < 3; ++j) {
      double dp = 0;
      for (int k = 0; k < 3; ++k) dp += cam.c2w[3 * k + i] * cam.c2w[3 * k + j];
      if (std::fabs(dp - (i == j ? 1.0 : 0.0)) > 1e-9) return false;
    }
  double ax = cam.screen_w / cam.screen_dist, ay = cam.screen_h / cam.screen_dist;
  double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
  for (int k = 0; k < 8; ++k) {
    double X[3] = {(k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]};
    double v[3] = {X[0] - cam.pos[0], X[1] - cam.pos[1], X[2] - cam.pos[2]};
    double cx = 0, cy = 0, cz = 0;  // coordinates along the c2w columns
    for (int i = 0; i < 3; ++i) {
      cx += v[i] * cam.c2w[3 * i + 0];
      cy += v[i] * cam.c2w[3 * i + 1];
      cz += v[i] * cam.c2w[3 * i + 2];
    }
    double depth = -cz;  // the view direction is -column 2
    if (!(depth > 1e-6 * (std::fabs(cx) + std::fabs(cy) + 1.0))) return false;  // behind / at the pinhole plane
    double fx = 0.5 + cx / depth / ax, fy = 0.5 + cy / depth / ay;
    x0 = std::min(x0, fx * W);
    x1 = std::max(x1, fx * W);
    y0 = std::min(y0, fy * H);
    y1 = std::max(y1, fy * H);
  }
  // pixel x covers [x, x+1) in fx*W
  r[0] = (int)std::max(-1.0, std::floor(x0) - 1);
  r[2] = (int)std::min((double)W, std::floor(x1) + 1);
  r[1] = (int)std::max(-1.0, std::floor(y0) - 1);
  r[3] = (int)std::min((double)H, std::floor(y1) + 1);
  return true;
}

// The culling rectangle: pixels outside [cull[0], cull[2]] x [cull[1],
// cull[3]] see no geometry (not traced, resolved to 0).
void screen_footprint(const PlanInput& in, int cull[4]) {
  cull[0] = 0;
  cull[1] = 0;
  cull[2] = in.W - 1;
  cull[3] = in.H - 1;
  if (in.knobs.no_footprint_cull) return;
  if (in.env) return;  // rays that miss the scene see the environment map
  int r[4];
  if (footprint_rect(in.cam, in.box_lo, in.box_hi, in.W, in.H, r)) std::copy(r, r + 4, cull);
}

// Pixels whose camera rays can reach the scene: the footprint's area inside
// the frame, or the whole frame with an environment light (misses see the
// map) or no footprint.  A property of the frame -- PT_NO_FOOTPRINT_CULL
// leaves it alone -- for the sample-group size.
int64_t traced_px(const PlanInput& in) {
  const int W = in.W, H = in.H;
  int r[4];
  if (in.env || !footprint_rect(in.cam, in.box_lo, in.box_hi, W, H, r)) return (int64_t)W * H;
  const int64_t w = std::min(W - 1, r[2]) - std::max(0, r[0]) + 1, h = std::min(H - 1, r[3]) - std::max(0, r[1]) + 1;
  return std::max<int64_t>(0, w) * std::max<int64_t>(0, h);
}

// Sample groups of a pixel (KParams: n_groups groups of group_spp samples,
// the last one possibly short).  The grouping decides the float summation
// order of a pixel, so it is a function of the FRAME only -- its size, spp,
// the pixels its camera rays can reach, the environment light -- never of
// the launch's tile set, of a stats build or of the device: any split of a
// frame into tile launches (raytrace_tile calls, the multi-GPU shards) and
// any device (a CPX partition, fewer resident waves) sums every pixel in the
// same order.  The slots-per-lane rule below counts the lanes of a whole
// MI355X at the default occupancy (PT_GROUP_REF_LANES: 256 CUs x 20 waves x
// 64), not the running device's.
//  * group_spp: 4 (C4 +4%, framed C3 +2% over 2), 2 with an environment
//    light (C5 +2.3%, c5big +2.1%), halved until the traced samples make >= 24
//    work slots per resident lane: C3's footprint-culled frame gets 2 (+1.5%
//    pipelined, its lone launch 1.70 -> 1.44 ms: half the work in flight when
//    the queue runs dry), C1 / C2 get 1 (profiles/r4/ab_group_size.txt);
//  * (a tail of one-sample groups handed out last, to end the launch on short
//    work slots, measured -2% pipelined for +2% on a lone frame: DESIGN.md §4).
//  * `sample_group` > 0 (PT_SAMPLE_GROUP) replaces the rule's answer.
//  * `budget_waves` bounds the 32-bit slot indices: the largest grid any
//    launch of the frame may use (plain or stats build), so a frame that fits
//    one build fits the other.
int group_size(int64_t traced, bool env, int spp, int sample_group, int64_t lanes, int64_t frame_blocks,
               int64_t budget_waves) {
  int gs = env ? PT_GROUP_SPP_ENV : PT_GROUP_SPP;
  while (gs > 1 && traced * ((spp + gs - 1) / gs) < lanes * PT_GROUP_MIN_SLOTS) gs /= 2;
  if (sample_group > 0) gs = sample_group;
  gs = std::max(1, std::min(gs, spp));
  for (;;) {
    // 32-bit slot indices (they may overshoot by a static and a claimed
    // chunk per wave) and a group-sum budget of PT_GROUP_SUM_GIB per render
    // slot, for the whole frame's blocks (so every tile split gets the same
    // layout)
    const int64_t slots = frame_blocks * 64 * ((spp + gs - 1) / gs);
    if ((slots + 2 * budget_waves * PT_CHUNK_MAX < (int64_t)INT32_MAX && slots * PT_SUM_BYTES <= ((int64_t)PT_GROUP_SUM_GIB << 30)) ||
        gs >= spp)
      break;
    gs = std::min(spp, gs * 2);
  }
  return gs;
}

bool global_tables(const PlanInput& in) {
  return in.n_bsdfs > PT_LDS_BSDFS || in.n_lights > PT_LDS_LIGHTS || in.knobs.force_global_tables;
}

// Render blocks: <= 8x8 rectangles of each tile clipped to the cull rectangle,
// tile by tile (tb0[i] = the first block of tile i, for the resolve).  Returns
// their number; `bl` null: only counts (the rest is not written).
static int64_t clip_blocks(const PlanRect* tl, size_t n, const int cull[4], std::vector<PlanRect>* bl = nullptr,
                           std::vector<int>* tb0 = nullptr) {
  int64_t blocks = 0;
  for (size_t i = 0; i < n; ++i) {
    const PlanRect& t = tl[i];
    const int x0 = std::max(t.x, cull[0]), x1 = std::min(t.x + t.w - 1, cull[2]);
    const int y0 = std::max(t.y, cull[1]), y1 = std::min(t.y + t.h - 1, cull[3]);
    if (x1 >= x0 && y1 >= y0) blocks += (int64_t)((x1 - x0 + 8) / 8) * ((y1 - y0 + 8) / 8);
    if (!bl) continue;
    tb0->push_back((int)bl->size());
    for (int by = y0; by <= y1; by += 8)
      for (int bx = x0; bx <= x1; bx += 8) bl->push_back({bx, by, std::min(8, x1 - bx + 1), std::min(8, y1 - by + 1)});
  }
  if (bl) tb0->push_back((int)bl->size());
  return blocks;
}

// Large launches over trees larger than two XCD L2s render their tiles in
// Z-order (the queue bands then deal each XCD a compact region rather than a
// strip of rows: C5 +2.5%, c5big +2.7%; C4's 4-MB tree, without bands, -0.5%
// in Z-order, keeps the rows: profiles/r6/ab_tile_zorder.txt).  Images are per
// pixel and sample, identical in any order; packed outputs keep the caller's
// tile index (KParams.tile_out).  PT_TILE_ZORDER=0/1 forces it (A/B, tests).
static void tile_order(const PlanInput& in, LaunchPlan& p) {
  const PlanRect* tl = in.tiles;
  const size_t n = in.n_tiles;
  int edge = 1;  // the tile edge: the largest tile's (clipped edge tiles are smaller)
  for (size_t i = 0; i < n; ++i) {
    p.pixels += (int64_t)tl[i].w * tl[i].h;
    edge = std::max(edge, std::max(tl[i].w, tl[i].h));
  }
  bool z = n > 1 && p.pixels >= ((int64_t)1 << 20) && in.n_render_nodes * 128 > ((int64_t)PT_BANDS_TREE_MIB << 20);
  if (in.knobs.tile_zorder >= 0) z = n > 1 && in.knobs.tile_zorder != 0;
  p.zorder = z;
  if (!z) return;
  std::vector<uint64_t> key(n);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t cx = (uint64_t)std::max(0, tl[i].x / edge), cy = (uint64_t)std::max(0, tl[i].y / edge);
    uint64_t k = 0;
    for (int b = 0; b < 21; ++b) k |= ((cx >> b) & 1ull) << (2 * b) | ((cy >> b) & 1ull) << (2 * b + 1);
    key[i] = k;
  }
  p.perm.resize(n);
  for (size_t i = 0; i < n; ++i) p.perm[i] = (int)i;
  std::stable_sort(p.perm.begin(), p.perm.end(), [&](int a, int b) { return key[a] < key[b]; });
  p.ztiles.resize(n);
  for (size_t i = 0; i < n; ++i) p.ztiles[i] = tl[p.perm[i]];
}

LaunchPlan plan_launch(const PlanInput& in) {
  LaunchPlan p;
  const LaunchKnobs& kn = in.knobs;
  const bool stats = p.stats = (in.flags & (PT_FLAG_STATS | PT_FLAG_REF_COUNTS)) != 0;
  // a census launch writes its per-wave records into the one shared trace
  // area, so it never overlaps another launch: it runs unpipelined
  const bool census_launch = kn.census && !stats;
  const bool pipelined = kn.pipeline && !census_launch;
  tile_order(in, p);
  const PlanRect* tl = p.zorder ? p.ztiles.data() : in.tiles;

  screen_footprint(in, p.cull);
  p.footprint[0] = std::max(0, p.cull[0]);
  p.footprint[1] = std::max(0, p.cull[1]);
  p.footprint[2] = std::min(in.W - 1, p.cull[2]);
  p.footprint[3] = std::min(in.H - 1, p.cull[3]);
  if (p.footprint[2] < p.footprint[0] || p.footprint[3] < p.footprint[1]) {
    p.footprint[0] = p.footprint[1] = 0;  // nothing visible: the empty rectangle
    p.footprint[2] = p.footprint[3] = -1;
  }
  p.shade_batch = kn.shade_batch ? kn.shade_batch : in.env ? PT_SHADE_BATCH_ENV : PT_SHADE_BATCH;
  p.leaf_weight = kn.leaf_weight ? kn.leaf_weight : in.env ? PT_LEAF_WEIGHT_ENV : PT_LEAF_WEIGHT;
  p.census = census_launch ? 1 : 0;  // diagnostics (tools/wave_trace.py --census)
  // triangle-only scenes take the render kernel without the sphere test
  // (branch-free leaf steps); PT_NO_TRI_ONLY forces the mixed one (A/B, tests)
  p.tri_only = in.tri_only && !kn.no_tri_only ? 1 : 0;
  p.helpers = kn.no_helpers ? 0 : 1;  // drain helpers
  p.drain_div = kn.drain_div;
  if (kn.debug_x >= 0 && kn.debug_x < in.W && kn.debug_y < in.H) p.dbg_pix = kn.debug_x + kn.debug_y * in.W;

  p.tile_block0.reserve(in.n_tiles + 1);
  clip_blocks(tl, in.n_tiles, p.cull, &p.blocks, &p.tile_block0);
  p.culled_px = p.pixels;
  for (const PlanRect& b : p.blocks) p.culled_px -= (int64_t)b.w * b.h;

  // Work slots are (pixel, group of group_spp samples): small enough that
  // the dynamic queue balances the waves (a whole pixel per slot left the
  // launch waiting on a few waves holding 64-sample pixels).
  // the launch fills the GPU with the resident waves of the kernel variant it
  // runs (environment light / global tables; the STATS build for counters)
  p.gtab = global_tables(in);
  int64_t want = stats ? in.grid_stats : (int64_t)std::max(8, in.bpc_variant[(in.env ? 2 : 0) + (p.gtab ? 1 : 0)]) * in.n_cu;
  if (kn.waves_per_cu > 0) want = (int64_t)kn.waves_per_cu * in.n_cu;  // tuning knob
  const int64_t want_plain = kn.waves_set ? want : in.grid_plain;
  const int64_t frame_blocks = (int64_t)((in.W + 7) / 8) * ((in.H + 7) / 8);
  const int64_t budget_waves = std::max({want, want_plain, (int64_t)in.grid_stats});
  p.group_spp = group_size(traced_px(in), in.env, in.spp, kn.sample_group, (int64_t)PT_GROUP_REF_LANES, frame_blocks,
                           budget_waves);
  p.n_groups = (in.spp + p.group_spp - 1) / p.group_spp;
  p.frame_slots = (int64_t)p.blocks.size() * 64 * p.n_groups;
  const int64_t slots = p.slots = p.frame_slots * in.nf;  // (a frame batch: every frame's slots, frame after frame)
  pt_fastdiv_init((uint32_t)std::max<int64_t>(p.frame_slots, 1), &p.frm_m, &p.frm_sh);
  // (slot indices reach past the end by up to a static chunk plus a claimed one per wave)
  if (slots + 2 * want * PT_CHUNK_MAX >= (int64_t)INT32_MAX) {
    p.error = "frame too large for one launch";
    return p;
  }
  // Small launches: at most PT_SMALL_SLOTS work slots per lane of the whole
  // resident grid (a strong split's share of the C3 frame: 12.8 at N = 2,
  // 3.2 at N = 8; the whole C3 frame has 25.6).  Each lane then renders only
  // a few slots, so a wave's slowest lane -- not the work -- sets the launch's
  // time.  They claim 64 slots at a time (one per lane: no wave holds two
  // while others have none), and when queued behind other frames they run on
  // half the resident grid with up to pt_ctx::kSlots frames in flight (more
  // slots per lane per launch, the next frames filling each launch's tail).
  // Measured on the split's share (one-GPU emulation,
  // profiles/r6/ab_small_launch*.txt): N = 8 0.38 -> 0.22 ms per frame, N = 4
  // 0.51 -> 0.39, N = 2 0.75 -> 0.66.  Neither the grid nor the claim changes a
  // value (the sample grouping is a function of the frame).
  // PT_SMALL_LAUNCH=0 turns it off.
  p.small = kn.small_launch && pipelined && !stats && slots <= (int64_t)PT_SMALL_SLOTS * in.grid_plain * PT_BLOCK;
  if (p.small && !in.gpu_idle && !kn.waves_set) want = std::max<int64_t>(in.n_cu, want / 2);
  p.want = want;
  pt_fastdiv_init((uint32_t)p.n_groups, &p.grp_m, &p.grp_sh);
  // queue claims: bigger for frames with many slots per lane (fewer atomics
  // on the heads; a lone small frame's drain prefers the smaller claim)
  // and for a frame queued behind another in the render pipeline
  // (profiles/r5/ab_chunk_busy.txt): its drain overlaps the previous frame's -- the
  // throughput case -- while a frame launched on an idle GPU, or with the
  // pipeline off (PT_PIPELINE=0: no two launches overlap), is the latency
  // case, whose end the smaller claim shortens
  // (C3: 256-slot claims +2.9% pipelined, lone launch +9%:
  // profiles/r5/ab_chunk_heads.txt).  A claim size never changes a value.
  const bool big_frame = slots >= (int64_t)PT_CHUNK_BIG_SLOTS * want_plain * PT_BLOCK;
  p.chunk = p.small ? PT_BLOCK : big_frame || (pipelined && !in.gpu_idle) ? PT_CHUNK_MAX : PT_CHUNK;
  // large frames claim PT_CHUNK_BIG (512) where the slot indices and the
  // one-block-per-chunk rule allow it: half the atomics again (C5 +1.0%, C4
  // +0.7%; C3's queued frames lose 7% at 512: profiles/r5/ab_chunk512.txt)
  if (big_frame && slots + 2 * want * PT_CHUNK_BIG < (int64_t)INT32_MAX && (64 * p.n_groups) % PT_CHUNK_BIG == 0)
    p.chunk = PT_CHUNK_BIG;
  if (kn.chunk_slots && slots + 2 * want * kn.chunk_slots < (int64_t)INT32_MAX) p.chunk = kn.chunk_slots;  // tuning knob
  // Large frames (PT_CHUNK_BIG_SLOTS slots per lane and more) over trees
  // larger than two XCD L2s (4 MB each): each queue head deals a contiguous
  // band of the frame, so an XCD's waves share BVH nodes in its L2 (C5's 17-MB
  // tree +1.8%, c5big's 68-MB +1.8%); C4's 4-MB tree loses 1.2% to the bands'
  // uneven ends, and a small frame keeps the interleaved sweep, whose heads
  // run dry together (C3 -5.5%, its lone launch +12%): profiles/r5/ab_bands*.txt.
  // PT_QUEUE_BANDS=0/1 forces it (A/B, tests).
  p.qbands = big_frame && in.n_render_nodes * 128 > ((int64_t)PT_BANDS_TREE_MIB << 20) ? 1 : 0;
  if (kn.queue_bands >= 0) p.qbands = kn.queue_bands;
  p.sblocks = (64 * p.n_groups) % p.chunk == 0 ? 1 : 0;  // every (aligned) chunk inside one block
  p.group_shift = -1;  // log2(group_spp) for a power of two
  for (int k = 0; k <= 30; ++k)
    if ((1 << k) == p.group_spp) p.group_shift = k;
  int64_t max_grid = std::max<int64_t>(1, (slots + PT_BLOCK - 1) / PT_BLOCK);
  int grid = (int)std::min<int64_t>(want, max_grid);
  if ((stats || p.census) && (size_t)grid * PT_WAVE_TRACE + PT_STATS_SLOTS > in.stats_cap)
    grid = (int)((in.stats_cap - PT_STATS_SLOTS) / PT_WAVE_TRACE);
  p.grid = std::max(1, grid);
  // group sums: 12 B per work slot of THIS launch (a rank's share of a split
  // frame holds only its own blocks' sums); the stack spill: the worst-case
  // depth beyond the LDS stack, per lane of the grid
  const size_t deep = in.bvh_stack > PT_STACK ? (size_t)(in.bvh_stack - PT_STACK) : 0;
  p.partial_floats = (size_t)std::max<int64_t>(slots, 1) * 3;
  p.spill_ints = deep * p.grid * PT_BLOCK;
  if (in.nf > 1) {
    // a frame batch: every render slot's group sums sized at once for the
    // largest batch of this tile set, and its spill area for the whole grid
    // (growing a buffer later synchronises the device -- inside the caller's
    // back-to-back frames)
    p.batch_partial_floats =
        (size_t)std::max<int64_t>(p.frame_slots, 1) * 3 * (size_t)std::max(in.nf, frames_that_fit(in, PT_MAX_FRAMES));
    p.batch_spill_ints = deep * std::max<int64_t>(want, in.grid_plain) * PT_BLOCK;
  }
  return p;
}

// Frames of the tile set in.tiles one launch of a frame batch takes.  A frame
// with more than PT_BATCH_SLOTS work slots per lane of a whole MI355X renders
// alone: it fills the GPU by itself, and batching measured slower there (C4
// -4.7%; C3's 25.6 slots per lane +2%, its strong split's shares +15..+45%:
// profiles/r6/ab_frame_batch.txt).  Otherwise as many as keep the work-slot
// indices 32-bit and the group sums within PT_GROUP_SUM_GIB.  The blocks are
// the launch's own (clip_blocks inside screen_footprint: the same per-frame
// slot count as plan_launch's frame_slots).  Its bounds differ from
// plan_launch's ON PURPOSE and stay as measured: it is asked before a launch
// is shaped, so its wave budget is the largest of the plain grid, the stats
// grid and 40 waves per CU (not the launch's own grid), and its overshoot the
// largest claim's, PT_CHUNK_BIG (not PT_CHUNK_MAX).
int frames_that_fit(const PlanInput& in, int nf, int64_t* frame_slots) {
  int cull[4];
  screen_footprint(in, cull);
  const int64_t blocks = clip_blocks(in.tiles, in.n_tiles, cull);
  const int64_t frame_blocks = (int64_t)((in.W + 7) / 8) * ((in.H + 7) / 8);
  const int64_t waves = std::max<int64_t>({(int64_t)in.grid_plain, (int64_t)in.grid_stats, (int64_t)40 * in.n_cu});
  const int gs = group_size(traced_px(in), in.env, in.spp, in.knobs.sample_group, (int64_t)PT_GROUP_REF_LANES,
                            frame_blocks, waves);
  const int64_t per = blocks * 64 * ((in.spp + gs - 1) / gs);
  if (frame_slots) *frame_slots = per;
  if (per > (int64_t)PT_BATCH_SLOTS * PT_GROUP_REF_LANES) return 1;
  while (nf > 1 && (per * nf + 2 * waves * PT_CHUNK_BIG >= (int64_t)INT32_MAX ||
                    per * nf * PT_SUM_BYTES > ((int64_t)PT_GROUP_SUM_GIB << 30)))
    --nf;
  return nf;
}
