// pt_tuning.h — the tuning constants the host's launch policy (launch_plan.cpp)
// shares with the kernels, and the layout of the launch counters.  Plain C++:
// no HIP header, so the policy compiles and runs without a GPU.
#pragma once
#include <stdint.h>

#ifndef PT_BLOCK
#define PT_BLOCK 64  // one wave64 per workgroup: the persistent queue is per wave
#endif
#ifndef PT_CHUNK
#define PT_CHUNK 128  // work slots a wave claims from the queue per atomic (KParams.chunk)
#endif
#ifndef PT_CHUNK_MAX
#define PT_CHUNK_MAX 256  // the claim for frames with >= PT_CHUNK_BIG_SLOTS slots per resident lane
#endif
#ifndef PT_CHUNK_BIG
#define PT_CHUNK_BIG 512  // the claim for large frames where it fits (launch_plan.cpp plan_launch)
#endif
#ifndef PT_BANDS_TREE_MIB
#define PT_BANDS_TREE_MIB 8  // queue bands for large frames over render trees above this size (launch_plan.cpp plan_launch)
#endif
// Frames per launch of pt_render_frames_device (KParams.seeds; include/ptgpu.h)
#ifndef PT_MAX_FRAMES
#define PT_MAX_FRAMES 8
#endif
#ifndef PT_BATCH_SLOTS
#define PT_BATCH_SLOTS 32  // a frame with more work slots per lane (of a whole MI355X) renders alone (launch_plan.cpp frames_that_fit)
#endif
#ifndef PT_SMALL_SLOTS
#define PT_SMALL_SLOTS 16  // launches with at most this many work slots per resident lane are small (launch_plan.cpp plan_launch)
#endif
#ifndef PT_CHUNK_BIG_SLOTS
#define PT_CHUNK_BIG_SLOTS 128  // C4 (184 slots per lane) +1.5%, C5 (1,620) +6.6%; C3 (26), framed C3 (51): their lone launches lose
#endif
static_assert(PT_CHUNK >= PT_BLOCK, "a refill must cover a whole wave's demand");
#define PT_QUEUE_WORDS 32  // a work-queue head, alone in its 128-B line
// Queue heads, interleaved chunk by chunk, a wave starting at its XCD's: with
// the drain helpers, 8 measured C3 +1.9% pipelined, lone launch -4.0%, C5
// +2.2%, C4 +-0 over one head (profiles/r5/ab_queue_heads.txt; a claim on the
// one head waited ~1 us: census_claims.txt).  The resolve zeroes a launch's
// heads for the render slot's next launch (pt_kernels.hip resolve_kernel).
// (Measured and removed: a tail of 64-slot claims from a second head, C3 -2.6%
// -- profiles/r5/ab_tail_claims.txt.)
#define PT_QUEUE_HEADS 8
#ifndef PT_GROUP_SPP
#define PT_GROUP_SPP 4  // default samples per work slot (launch_plan.cpp group_size; 8 or more: C3 -4%, C5 -10%)
#endif
#ifndef PT_GROUP_SPP_ENV
#define PT_GROUP_SPP_ENV 2  // with an environment light
#endif
#ifndef PT_GROUP_REF_LANES
#define PT_GROUP_REF_LANES (256 * 20 * 64)  // the group-size rule's lanes: a whole MI355X at 20 waves per CU (device-independent)
#endif
#ifndef PT_GROUP_MIN_SLOTS
#define PT_GROUP_MIN_SLOTS 24  // groups are halved until the traced samples make this many slots per lane
#endif
// A group sum in memory: a packed float3, 12 B (16-B records measured C3
// -1.5%: profiles/r5/ab_order_ballot.txt).
#define PT_SUM_BYTES 12
#ifndef PT_GROUP_SUM_GIB
#define PT_GROUP_SUM_GIB 8  // group-sum budget per render slot (GiB): a group size that needs more doubles
#endif
// Leave traversal when this many lanes finished their ray (shade them
// together).  Scenes with an environment light shade longer per round (map
// lookups on every miss, inverse-CDF light samples) and want larger rounds:
// same-session sweep (profiles/r3/ab_shade_batch.txt) C3 / framed C3 / C4
// +1.5 / +3.4 / +5.6% at 32 vs 48, C5 -4% at 36 and best at 48.
#ifndef PT_SHADE_BATCH
#define PT_SHADE_BATCH 32
#endif
#ifndef PT_SHADE_BATCH_ENV
#define PT_SHADE_BATCH_ENV 48
#endif
#ifndef PT_LDS_BSDFS
#define PT_LDS_BSDFS 16  // material tables up to this size are staged in LDS
#endif
#ifndef PT_LDS_LIGHTS
#define PT_LDS_LIGHTS 8
#endif
// leaf steps when leaf lanes >= node lanes * 16 / leaf weight; with 32-lane
// shading rounds 10 beat 16 (C3 +1.9%, framed C3 +1.8%, C4 +1.4%); C5 (the
// environment-light build) is flat between 10 and 16 and keeps 16
// (profiles/r3/ab_leaf_weight.txt).  Round 4, with two-sample groups on C3:
// 12 over 10, C3 +0.8% and its lone launch -0.9%, C4 / framed C3 flat
// (profiles/r4/ab_knobs_batch_leaf.txt)
#ifndef PT_LEAF_WEIGHT
#define PT_LEAF_WEIGHT 12
#endif
#ifndef PT_LEAF_WEIGHT_ENV
#define PT_LEAF_WEIGHT_ENV 16
#endif
#define PT_STATS_SLOTS 72  // launch counters (PtStat); per-wave trace records (PT_WAVE_TRACE u64 each) follow
#define PT_WAVE_TRACE 11
#ifndef PT_STACK
#define PT_STACK 24  // traversal stack entries per lane in LDS (lane-contiguous)
#endif
#ifndef PT_STACK_MAX
#define PT_STACK_MAX 256  // deepest worst-case stack accepted (entries past PT_STACK spill to global memory)
#endif

// Slots of the launch counters (KParams.stats, u64 each): the STATS build of
// the render kernel adds into them, finish_stats (pt_api.cpp) reads them into
// pt_stats.  The *_MIN slots are atomicMin targets: a launch starts them at ~0.
enum PtStat {
  // 0..10: the kernel's per-lane sums, written as one array in this order
  PT_STAT_CAMERA_RAYS = 0,
  PT_STAT_BOUNCE_RAYS,
  PT_STAT_SHADOW_RAYS,
  PT_STAT_NODE_VISITS,
  PT_STAT_TRI_TESTS,
  PT_STAT_SPHERE_TESTS,
  PT_STAT_EXT_HITS,
  PT_STAT_WAVE_TRAV_STEPS,
  PT_STAT_WAVE_ROUNDS,
  PT_STAT_LEAF_STEPS,
  PT_STAT_QUEUE_ATOMICS,
  PT_STAT_LANE_SUMS,  // (their count)
  PT_STAT_SHADE_CLOCKS = 11,
  PT_STAT_TRAV_CLOCKS,
  PT_STAT_MAX_WAVE_CLOCKS,
  PT_STAT_WAVE_WALL_SUM,
  PT_STAT_WAVE_WALL_MAX,
  PT_STAT_HITSHADE_CLOCKS,
  PT_STAT_SECTION_CLOCKS = 17,  // 4: hit, NEE, BSDF, fetch
  // the launch's shape (pt_stats.wave_span, relative to WAVE_START_MIN):
  // first / last wave start, first / last wave end, first / last empty queue
  PT_STAT_WAVE_START_MIN = 21,
  PT_STAT_WAVE_START_MAX,
  PT_STAT_WAVE_END_MIN,
  PT_STAT_WAVE_END_MAX,
  PT_STAT_WAVE_EMPTY_MIN,
  PT_STAT_WAVE_EMPTY_MAX,
  PT_STAT_LANE_ITERS = 27,  // 4, then
  PT_STAT_DEEP_STACK_STEPS = 31,
  PT_STAT_SLOT_LATENCY_HIST = 32,  // 32 buckets
  PT_STAT_NODE_CENSUS = 64,        // 8
};
static_assert(PT_STAT_LANE_SUMS == PT_STAT_SHADE_CLOCKS && PT_STAT_WAVE_EMPTY_MAX + 1 == PT_STAT_LANE_ITERS &&
                  PT_STAT_LANE_ITERS + 4 == PT_STAT_DEEP_STACK_STEPS && PT_STAT_NODE_CENSUS + 8 == PT_STATS_SLOTS,
              "the launch counters fill PT_STATS_SLOTS without overlap");

// q = u / d for u < 2^31 and a runtime divisor d >= 1, without a division:
// q = m ? mulhi(u, m) >> sh : u >> sh (Granlund & Montgomery 1994).  For d
// a power of two m = 0; otherwise with 2^(l-1) < d < 2^l, m = ceil(2^(31+l) / d)
// < 2^32 and sh = l - 1: u*m / 2^(31+l) = u/d + u*e / (d * 2^(31+l)) with
// e = m*d - 2^(31+l) < d, and the error term stays below 1/d for u < 2^31, so
// the floor is exact (tests/test_abi.py checks it exhaustively for small d).
inline void pt_fastdiv_init(uint32_t d, uint32_t* m, uint32_t* sh) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  if ((1ull << l) == d) {
    *m = 0;
    *sh = l;
  } else {
    *m = (uint32_t)((((uint64_t)1 << (31 + l)) + d - 1) / d);
    *sh = l - 1;
  }
}
