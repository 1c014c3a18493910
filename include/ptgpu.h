/* ptgpu.h — C ABI of the MI355X-native path-tracing hot path.
 *
 * This is the drop-in boundary for the reference's per-pixel radiance loop.
 * Every entry point names the reference interface it replaces:
 *
 *   pt_create / pt_destroy      CUDAPathTracer::CUDAPathTracer / ~CUDAPathTracer
 *                               (cuda_src/setup.h:90-148, setup.cu:92-115)
 *   pt_upload_scene             CUDAPathTracer::init -> loadPrimitives/loadLights/
 *                               loadBVH (setup.cu:181-201, 249-476, 689-774).  The
 *                               render tree is the library's own binned-SAH BVH over
 *                               the handed-over primitives (the nearest
 *                               hit does not depend on the tree); scene.nodes (the
 *                               reference's tree) is validated and kept for
 *                               PT_FLAG_REF_COUNTS, and rendered over when the
 *                               environment sets PT_BVH_BUILD=ref.  Primitive ids
 *                               reported anywhere stay in the caller's order.
 *   pt_upload_scene_lbvh        the same with the BVH built on the GPU: the reference's
 *                               PARALLEL_BUILD_BVH path CUDAPathTracer::buildBVH
 *                               (setup.cu:188-189, 478-686; kernel.cu:358-493) —
 *                               scene.nodes is ignored (may be NULL)
 *   pt_set_camera               CUDAPathTracer::loadCamera (setup.cu:221-247);
 *                               camera semantics of Camera::generate_ray
 *                               (src/camera.cpp:113-129)
 *   pt_set_params               CUDAPathTracer::loadParameters (setup.cu:777-811);
 *                               PathTracer::ns_aa/max_ray_depth/ns_area_light
 *                               (src/pathtracer.h:222-227)
 *   pt_render_tiles             PathTracer::raytrace_tile(tile_x,tile_y,tile_w,tile_h)
 *                               (src/pathtracer.h:181, src/pathtracer.cpp:585-611) for
 *                               one tile; whole-frame batches replace
 *                               CUDAPathTracer::startRayTracingPT + updateHostSampleBuffer
 *                               + PathTracer::updateBufferFromGPU (setup.cu:147-179,813-843)
 *   pt_tile_submit / pt_tile_finish   raytrace_tile from the reference's worker threads,
 *                               asynchronous: tiles batched into launches, each completed
 *                               (sampleBuffer + toColor) by a completion thread
 *   pt_render_tiles_device      same, output left in device memory on a caller stream
 *                               (used for the multi-GPU framebuffer reduction)
 *   pt_render_frames_device     several frames of one tile set (one seed each) in one
 *                               launch: CUDAPathTracer::startRayTracingPT called back to
 *                               back (setup.cu:147-179), without a drain between frames
 *   pt_intersect                BVHAccel::intersect(ray, isect) and BVHAccel::intersect(ray)
 *                               (src/bvh.cpp:331-362) as a batched query
 *   pt_get_stats                timers/counters (pathtracer.cpp:615-632, setup.cu:546-685)
 *   pt_last_error               replaces fprintf+exit(EXIT_FAILURE) (setup.cu:139-143, ...)
 *   pt_to_color_device          HDRImageBuffer::toColor (src/image.h:174-189) on the device
 *   pt_film_*                   no counterpart: a device-resident progressive film (accumulated
 *                               passes, per-pixel error, GPU resolve to HDR / RGBA8 / error) for
 *                               the display loop that redraws frameBuffer (application.cpp:142-160)
 *   pt_film_export* / pt_film_merge*   no counterpart: a film's records copied out, and another
 *                               film's records combined into it (two Welford states merged per
 *                               pixel): films of a multi-GPU tile or sample split, checkpoints
 *   pt_render_features*         no counterpart: the camera ray's Intersection (trace_ray,
 *                               pathtracer.cpp:435-456) kept per pixel: normal, hit point, depth, BSDF
 *   pt_trace_rays* / pt_camera_rays_device   BVHAccel::intersect (src/bvh.cpp:331-362) for rays
 *                               and results in device memory, in stream order: closest-hit
 *                               records or occlusion bits; the feature pass's camera rays
 *   pt_render_rays* / pt_film_add_pass_rays   no counterpart: PathTracer::trace_ray
 *                               (pathtracer.cpp:415-553) along the caller's rays instead of
 *                               Camera::generate_ray's; the rays a render's samples took
 *   pt_denoise_* / pt_film_denoise*   no counterpart: an edge-avoiding filter of the film's mean,
 *                               guided by those records and the film's variance
 *   pt_reproject_* / pt_film_reproject   no counterpart: the film kept across a camera move, its
 *                               records gathered through the first hits of both cameras
 *
 * Conventions: plain C types and host pointers only; the caller owns every host
 * input and output; the library owns device memory until pt_destroy.  Calls on
 * one pt_ctx are serialised by the caller; different contexts (one per GPU) may
 * be driven from different host threads or processes.  Every function returns
 * PT_OK (0) or a negative PT_E_* code and never exits the process.
 * Image layout: float32 RGB, row-major, index (x + y*W)*3, y = 0 is the BOTTOM
 * row (HDRImageBuffer::update_pixel, src/image.h:113-117).
 */
#ifndef PTGPU_H
#define PTGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_E_INVALID (-1)  /* bad argument / unsupported scene content */
#define PT_E_HIP (-2)      /* HIP runtime error (message in pt_last_error) */
#define PT_E_NOSCENE (-3)  /* render/intersect before pt_upload_scene/pt_set_camera */
#define PT_E_ALLOC (-4)    /* device or host allocation failed */
#define PT_E_IO (-5)       /* file could not be read/written */

/* Primitive types follow Primitive::getType(): Sphere 0, Triangle 1. */
#define PT_PRIM_SPHERE 0
#define PT_PRIM_TRIANGLE 1
/* BSDF types follow BSDF::getType(): Diffuse 0, Mirror 1, Refraction 2, Glass 3, Emission 4. */
#define PT_BSDF_DIFFUSE 0
#define PT_BSDF_MIRROR 1
#define PT_BSDF_REFRACTION 2
#define PT_BSDF_GLASS 3
#define PT_BSDF_EMISSION 4
/* Light types follow SceneLight::getType(): Directional 0, Hemisphere 1, Point 2, Area 3;
 * Environment 4 (EnvironmentLight, src/static_scene/environment_light.cpp, whose own
 * getType() says 1) — its map is pt_scene.env_*; at most one (pt_upload_scene refuses a
 * second).  PathTracer::set_scene pushes it last (src/pathtracer.cpp:88-90), but its place
 * is not checked: trace_ray samples the lights in list order whatever their kind, and so
 * does the render kernel, so an environment light anywhere in the list is honoured. */
#define PT_LIGHT_DIRECTIONAL 0
#define PT_LIGHT_HEMISPHERE 1
#define PT_LIGHT_POINT 2
#define PT_LIGHT_AREA 3
#define PT_LIGHT_ENVIRONMENT 4

typedef struct pt_ctx pt_ctx;

/* One BSDF (src/bsdf.h).  albedo holds Diffuse::albedo, Mirror::reflectance and
 * Glass::reflectance; transmittance holds Refraction/Glass::transmittance;
 * emission holds EmissionBSDF::radiance. */
typedef struct pt_bsdf {
  int32_t type;
  float albedo[3];
  float transmittance[3];
  float emission[3];
  float ior;
  float roughness;
} pt_bsdf;

/* One light (src/static_scene/light.h).  Directional: direction = dirToLight.
 * Point: position.  Area: position, direction, dim_x, dim_y, area. */
typedef struct pt_light {
  int32_t type;
  float radiance[3];
  double position[3];
  double direction[3];
  double dim_x[3];
  double dim_y[3];
  float area;
} pt_light;

/* Camera (src/camera.h): pos, c2w(i,j) row-major, screenW/H/screenDist. */
typedef struct pt_camera {
  double pos[3];
  double c2w[9];
  double screen_w;
  double screen_h;
  double screen_dist;
} pt_camera;

/* One node of the reference BVH (src/bvh.h BVHNode), flattened: children by
 * index (-1 = NULL), primitives [start, start+range) of the BVH-ordered list. */
typedef struct pt_bvh_node {
  double bb_min[3];
  double bb_max[3];
  int64_t start;
  int64_t range;
  int64_t left;
  int64_t right;
} pt_bvh_node;

/* Flattened scene exactly as BVHAccel holds it: primitives in BVH order.
 * prim_geom: triangle p1,p2,p3 (9 doubles); sphere o.xyz, r (rest 0).
 * prim_norm: triangle vertex normals n1,n2,n3 (9 doubles); sphere ignored.
 * nodes[0] is the root. */
typedef struct pt_scene {
  int64_t n_prims;
  const int32_t* prim_type;
  const int32_t* prim_bsdf;
  const double* prim_geom;
  const double* prim_norm;
  int64_t n_nodes;
  const pt_bvh_node* nodes;
  int32_t n_bsdfs;
  const pt_bsdf* bsdfs;
  int32_t n_lights;
  const pt_light* lights;
  /* HDRImageBuffer of the environment light (NULL / 0 when there is none):
   * env_width x env_height float RGB, row 0 = +y (theta = (y+0.5)/h*pi). */
  int32_t env_width;
  int32_t env_height;
  const float* env_rgb;
} pt_scene;

/* Integrator settings (PathTracer members) and frame size. */
typedef struct pt_params {
  int32_t width;         /* 1 .. 65535 (and width * height <= 2^30) */
  int32_t height;        /* 1 .. 65535 */
  int32_t spp;           /* ns_aa */
  int32_t max_depth;     /* max_ray_depth, 0 .. 254 */
  int32_t ns_area_light; /* ns_area_light, 1 .. 255 */
  uint32_t seed;         /* counter-RNG key: (seed, pixel, sample) */
  uint32_t sample_base;  /* first sample index of this pass: samples sample_base .. sample_base+spp-1
                            are rendered and averaged (0 = the reference's single pass; progressive
                            passes / the multi-GPU sample split use disjoint ranges) */
} pt_params;

typedef struct pt_tile {
  int32_t x, y, w, h;
} pt_tile;

typedef struct pt_stats {
  int64_t pixels;       /* pixels rendered by the last call */
  int64_t samples;      /* pixels * spp */
  int64_t camera_rays;
  int64_t bounce_rays;
  int64_t shadow_rays;
  int64_t node_visits;  /* BVH2 internal-node fetches (64 B each in the reference layout) */
  int64_t tri_tests;
  int64_t sphere_tests;
  int64_t ext_hits;     /* nearest-hit rays that hit (shading-normal fetch) */
  double last_ms;       /* device time of the last render kernel (hipEvent) */
  int32_t counters_valid; /* 1 if the last call ran with PT_FLAG_STATS */
  int32_t grid_blocks;    /* persistent workgroups launched (PT_BLOCK lanes each) */
  int32_t blocks_per_cu;  /* resident workgroups per CU the occupancy query allows */
  int64_t wave_trav_steps; /* wave-level traversal steps (SIMD efficiency = node_visits / (64 * this)) */
  int64_t wave_rounds;     /* wave-level shading/refill rounds */
  int64_t culled_samples;  /* samples of pixels outside the scene's screen footprint (radiance 0, not traced) */
  int64_t queue_atomics;   /* work-queue atomics issued */
  int64_t shade_clocks;    /* shader clocks summed over waves: everything but traversal (shading, refill,
                              camera rays, loop overhead); shade_clocks + trav_clocks = the waves' summed
                              lifetimes.  All *_clocks come from the PT_FLAG_STATS build of the kernel,
                              which runs slower than the plain build (counters and clock stamps) */
  int64_t trav_clocks;     /* shader clocks summed over waves: traversal phases */
  int64_t max_wave_clocks; /* shader clocks of the slowest wave */
  int64_t wave_wall_sum;   /* wave lifetimes summed, device wall-clock ticks */
  int64_t wave_wall_max;   /* longest wave lifetime, device wall-clock ticks */
  int64_t leaf_steps;      /* of wave_trav_steps: leaf (primitive) steps */
  int64_t hitshade_clocks; /* of shade_clocks: hit records, NEE and bounces = section_clocks[0..2] */
  double resolve_ms;       /* device time of the sample-group resolve kernel */
  int32_t bvh_stack;       /* worst-case traversal stack entries of the uploaded BVH */
  int64_t bvh_nodes;       /* render-tree (BVH4) nodes uploaded */
  int64_t section_clocks[4]; /* of shade_clocks: hit record, light sampling, BSDF sampling + sample
                                completion, queue fetch (the rest of shade_clocks: camera rays and loop
                                overhead) */
  int64_t wave_span[5];    /* wall-clock ticks after the first wave started: last wave start,
                              first wave end, last wave end, first and last time a wave found
                              the work queue empty (launch ramp, queue drain and tail) */
  int32_t group_spp;       /* samples per work slot (pixel, sample group) of the last launch */
  int64_t lane_iters[4];   /* traversal lane-iterations (64 per wave iteration) spent at the other
                              step kind, finished and waiting for the shading round, retired
                              (queue drained), stepping a leaf; node steps = node_visits */
  int64_t deep_stack_steps; /* traversal lane-steps taken while the ray's stack held entries beyond the
                              PT_STACK (24) kept in LDS, i.e. in the global spill area */
  int64_t partial_bytes;   /* device bytes of the sample-group sums of the last launch: 12 B per work slot
                              of its own blocks (pixels * ceil(spp/group_spp) * 12 at most; a rank
                              rendering 1/N of a frame's tiles holds 1/N of them; two render slots
                              pipeline renders) */
  int32_t footprint[4];    /* the scene's screen footprint of the last launch, x0, y0, x1, y1 inclusive and
                              clamped to the frame: every pixel outside it has radiance 0 for every sample
                              (its camera ray misses the scene box; not traced).  The whole frame when
                              culling is off (environment light, camera not in front of the box); the
                              empty rectangle (0, 0, -1, -1) when the box is entirely off-screen. */
  int64_t slot_latency_hist[32]; /* PT_FLAG_STATS: work slots by wall-clock latency (first camera ray to the
                              group's store), bucket b = [2^(b-1), 2^b) microseconds (0: < 1 us, 31: the
                              rest) */
  int64_t node_census[8];  /* PT_FLAG_STATS: wave node steps of the traversal loop (root steps of fresh rays
                              apart); of them with every stepping lane at one node (a scalar-load
                              candidate); lanes at the first stepping lane's node; stepping lanes; steps and
                              lanes inside the top two BVH4 levels below the root (node index < 21 in the
                              breadth-first order); the same for three levels (< 85) */
  int32_t frames_per_launch; /* frames the last render launch held (pt_render_frames_device batches: up to
                                PT_MAX_FRAMES; 1 otherwise) */
  int32_t tile_zorder; /* 1: the last launch rendered its tiles in Z-order (large frames over trees above
                          PT_BANDS_TREE_MIB; PT_TILE_ZORDER=0/1 forces it) -- the same image */
} pt_stats;

#define PT_FLAG_STATS 1u /* count rays / node visits / primitive tests (slower build of the kernel) */
#define PT_FLAG_REF_COUNTS 2u /* as PT_FLAG_STATS, but traverse the reference's binary BVH so node_visits
                                 and primitive tests follow SURVEY.md §8(d)'s reference-layout cost model */

#define PT_FLAG_PACKED 4u /* pt_render_tiles_device only: hdr_out_dev holds n_tiles*32*32*3 floats and
                             tile i's pixel (x, y) goes to [(i*1024 + (y-tile.y)*32 + (x-tile.x))*3]
                             (every tile 1..32 x 1..32 and inside the frame); the multi-GPU exchange
                             gathers these packed tiles instead of whole frames */
#define PT_FLAG_PACKED16 8u /* as PT_FLAG_PACKED with 16x16 slots: n_tiles*16*16*3 floats, tile i's pixel
                               (x, y) at [(i*256 + (y-tile.y)*16 + (x-tile.x))*3], every tile 1..16 x 1..16
                               (the strong split dealing 16x16 tiles: a rank's share spread more evenly) */

int pt_create(int device, pt_ctx** out);
int pt_destroy(pt_ctx* ctx);
int pt_upload_scene(pt_ctx* ctx, const pt_scene* scene);
/* Uploads the scene and builds a linear BVH on the device (Morton codes,
 * radix sort, Karras tree, bottom-up boxes, leaves of <= 4 primitives, then
 * the 4-wide layout).  Primitive indices reported by pt_intersect stay those
 * of the uploaded arrays. */
int pt_upload_scene_lbvh(pt_ctx* ctx, const pt_scene* scene);
int pt_set_camera(pt_ctx* ctx, const pt_camera* cam);
int pt_set_params(pt_ctx* ctx, const pt_params* params);
/* Renders the listed tiles into a host framebuffer of width*height*3 floats;
 * only pixels inside the tiles are written.  flags: PT_FLAG_* */
int pt_render_tiles(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, float* hdr_out_host,
                    uint32_t flags);
/* Same, into a device framebuffer (width*height*3 floats) on `stream`
 * (hipStream_t, NULL = the context's stream).  Returns after the kernel is
 * queued, without waiting for it (a PT_FLAG_STATS / PT_FLAG_REF_COUNTS call
 * waits, to read its counters); synchronise on the stream before reading.
 * The framebuffer is written in `stream` order: after the work queued on
 * `stream` before the call, before the work queued after it (the kernels
 * themselves run on the context's render streams).
 * Replaces CUDAPathTracer::startRayTracingPT (cuda_src/setup.cu:147-179)
 * minus its host copy-back. */
int pt_render_tiles_device(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, float* hdr_out_dev,
                           void* stream, uint32_t flags);
/* A frame batch: n_frames (1..PT_MAX_FRAMES = 8) renders of the same tiles, frame
 * f with pt_params.seed replaced by seeds[f], into hdr_outs_dev[f] (each as
 * pt_render_tiles_device's hdr_out_dev, PT_FLAG_PACKED allowed; counters are
 * not: PT_FLAG_STATS / PT_FLAG_REF_COUNTS return PT_E_INVALID).  Every image
 * is bit-identical to its own pt_render_tiles_device call with that seed;
 * the frames share ONE persistent launch, so a small frame's drain (a rank's
 * share of a split frame) is filled with the next frame's work.  Stream
 * semantics as pt_render_tiles_device. */
#define PT_MAX_FRAMES 8
int pt_render_frames_device(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, int32_t n_frames,
                            const uint32_t* seeds, float* const* hdr_outs_dev, void* stream, uint32_t flags);
/* Asynchronous one-tile seam: PathTracer::raytrace_tile(tile_x, tile_y, tile_w, tile_h)
 * (src/pathtracer.cpp:585-611) as the reference's worker threads call it
 * (worker_thread, pathtracer.cpp:613-621), without one launch and one host
 * synchronisation per tile.  pt_tile_submit queues the tile and returns; queued
 * tiles render as ONE launch once PT_TILE_BATCH (default 256) are queued, or at
 * pt_tile_finish.  When a tile's launch completes, its pixels are written into
 * hdr_out_host (the width*height*3 sampleBuffer) and, if rgba_out_host is not
 * NULL, toColor'd into it (the width*height frameBuffer, as pt_to_color), by the
 * context's completion thread, which waits on each launch's event off the
 * render stream (so completing one batch overlaps the next batch's render) --
 * exactly what raytrace_tile leaves behind.  At most 8 launched batches await
 * completion; a submit beyond that waits for one.  The caller keeps
 * both buffers alive and does not write the tile's pixels until pt_tile_finish
 * returns.  pt_tile_finish renders what is still queued and waits for every
 * submitted tile.  Tiles render with the scene/camera/params of submission
 * (the setters and the synchronous renders first launch what is queued).  The
 * pixels equal those of a whole-frame pt_render_tiles bit for bit.  A failed
 * launch or completion is returned by the call that hit it (a launch) and
 * ALSO by the next pt_tile_finish: its tiles were not rendered.  Whatever it
 * returns, pt_tile_finish returns only after every launched batch has been
 * completed, so the caller's buffers stay in use until pt_tile_finish returns
 * and are free afterwards, on success or error. */
int pt_tile_submit(pt_ctx* ctx, const pt_tile* tile, float* hdr_out_host, uint32_t* rgba_out_host);
int pt_tile_finish(pt_ctx* ctx);
/* Batched BVHAccel::intersect.  Rays: origin o[3n], direction d[3n] (normalised),
 * max_t[n] for the any-hit query (clamped to 3.0e38, the traversal's "far":
 * +inf, the reference's default, is welcome).  Outputs (each nullable): nearest hit flag,
 * t, primitive index (the caller's BVH order, whatever tree renders), and the any-hit
 * flag within (0, max_t). */
int pt_intersect(pt_ctx* ctx, int64_t n, const double* o, const double* d, const double* max_t,
                 int32_t* hit, float* t, int32_t* prim, int32_t* any_hit);
/* Statistics of the last render (waits for its kernel-time events). */
int pt_get_stats(pt_ctx* ctx, pt_stats* out);
/* Kernel and resolve times in ms of the last min(cap, launches, 256) renders,
 * oldest first (waits for them); *n = how many were written.  resolve_ms may
 * be NULL.  No reference counterpart (its timers are host wall-clock,
 * application.cpp:776-780): the HIP-event view of the same launches. */
int pt_get_launch_times(pt_ctx* ctx, float* kernel_ms, float* resolve_ms, int32_t cap, int32_t* n);
/* Diagnostics (no reference counterpart): after a PT_FLAG_STATS launch, one
 * record of 11 int64 per wave -- device wall-clock start, first time the wave
 * found the work queue empty (~0 if never), end, (XCC id << 32 | HW_ID), the
 * camera samples it started, the sum and maximum of its work slots'
 * latencies (claim to partial-sum store, wall-clock ticks), the most
 * traversal iterations one ray stepped in (<< 32) | sat out, the most
 * traversal phases one ray spanned, and the traversal iterations and shading
 * rounds it ran after it saw the queue drained.  out == NULL: only *n_waves
 * is set. */
int pt_get_wave_trace(pt_ctx* ctx, int64_t* out, int64_t cap, int64_t* n_waves);
/* Diagnostics (no reference counterpart): the render tree as it lies in
 * device memory -- whichever is loaded: the GPU-built tree (the default and
 * pt_upload_scene_lbvh), the host SAH tree (PT_BVH_BUILD=sah) or the caller's
 * (=ref).  Read-only; no render path does any work for it.
 * pt_debug_bvh_info: the sizes to allocate for pt_debug_read_bvh, the
 * worst-case traversal stack the uploads computed and the root box.
 * PT_E_NOSCENE before an upload, PT_E_INVALID for a NULL argument. */
typedef struct pt_bvh_info {
  int64_t n_prims;      /* primitives (and 9-float normal records, and prim_map entries) */
  int64_t n_nodes4;     /* 4-wide nodes of the render tree */
  int64_t n_nodes2;     /* binary nodes of the reference-count launch */
  int32_t bvh_stack;    /* worst-case traversal stack entries (pt_stats.bvh_stack) */
  int32_t has_prim_map; /* 1: the tree has its own primitive order and a map back to the caller's */
  float root_lo[3], root_hi[3];
} pt_bvh_info;
int pt_debug_bvh_info(pt_ctx* ctx, pt_bvh_info* out);
/* Copies the context's current buffers to host memory after waiting for the
 * context's stream; any pointer may be NULL and is skipped (prim_map is also
 * skipped when has_prim_map is 0).  Little-endian records:
 *   nodes4: n_nodes4 x 128 B.  Six float[4] at byte 0, 16, .. 80: lo.x, hi.x,
 *     lo.y, hi.y, lo.z, hi.z, element k of each belonging to child slot k;
 *     int32[4] child references at byte 96; 16 B of padding.  A reference
 *     >= 0 is a node index, < 0 a leaf cursor ~((first << 3) | (count - 1)):
 *     primitives [first, first + count) of `prims`, count <= 8.  An unused
 *     slot has all six planes at +inf.
 *   nodes2: n_nodes2 x 64 B.  float[4] a = (c0.lo.x, c0.hi.x, c0.lo.y,
 *     c0.hi.y), b = the same of child 1, c = (c0.lo.z, c0.hi.z, c1.lo.z,
 *     c1.hi.z), int32[4] e = (c0 reference, c1 reference, 0, 0).  After
 *     pt_upload_scene_lbvh its leaf cursors index `prims`; after
 *     pt_upload_scene it is the caller's tree over the caller's order.
 *   prims: n_prims x 48 B, three float[4].  Triangle: v0 = (p1, meta),
 *     e1 = (p2 - p1, 0), e2 = (p3 - p1, 0); sphere: v0 = (centre, meta),
 *     e1 = (r, r*r, 0, 0), e2 = 0.  meta is an int32 in a float's bits:
 *     (bsdf << 1) | is_triangle.
 *   norms: n_prims x 9 floats (the three vertex normals; 0 for spheres).
 *   prim_map: n_prims int32, position in `prims` -> the caller's index. */
int pt_debug_read_bvh(pt_ctx* ctx, void* nodes4, void* nodes2, void* prims, float* norms, int32_t* prim_map);
/* Diagnostics: the HIP resources this library holds at the moment, in the
 * whole process (every context and film, and a GPU tree build in progress):
 * device arrays and their bytes, pinned host arrays, events and streams.
 * Each is owned by one object and counted where it is acquired and released,
 * so a context's pt_destroy brings every count back to its value before that
 * context's pt_create.  Needs no context and no device; PT_E_INVALID for a
 * NULL argument. */
typedef struct pt_resource_counts {
  int64_t device_arrays;
  int64_t device_bytes;
  int64_t pinned_arrays;
  int64_t events;
  int64_t streams;
} pt_resource_counts;
int pt_debug_live_resources(pt_resource_counts* out);
const char* pt_last_error(void);

/* Output row, host side (no device needed):
 * HDRImageBuffer::toColor(target, x0, y0, x1, y1) (src/image.h:174-189) of the
 * HDR buffer `hdr` (width*height*3 float, the sampleBuffer layout) into the
 * RGBA8 `frame` (width*height uint32, ImageBuffer::data: r | g<<8 | b<<16 |
 * a<<24, image.h:49-58), with the reference's float arithmetic (powf; NaN ->
 * 255).  Pixels outside [x0,x1) x [y0,y1) are left untouched. */
int pt_to_color(const float* hdr, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                uint32_t* frame);
/* The 255 steps of pt_to_color's channel code (host only, no device): a channel's
 * 8-bit code is a non-decreasing step function of the float's bit pattern, and
 * thr_bits[k], k = 1..255, is the smallest non-negative float's bits whose code
 * reaches k, found with the reference arithmetic itself; thr_bits[0] = 0.  So
 * code(s) = #{k >= 1 : bits(s) >= thr_bits[k]} for every s without the sign
 * bit (a positive NaN: 255); with it, -0.0f gives 0 and everything else 255.
 * This is the whole table the device tonemap (pt_to_color_device, the film's
 * resolve) searches. */
int pt_to_color_thresholds(uint32_t thr_bits[256]);
/* pt_to_color on the device: the RGBA8 codes of the device HDR buffer hdr_dev
 * (width*height*3 float) into rgba_dev (width*height uint32) for the pixels
 * of [x0,x1) x [y0,y1), clamped to the frame as pt_to_color clamps it; the
 * rest is left untouched.  Equal to pt_to_color bit for bit, for every float
 * (pt_to_color stays the definition).  Queued on `stream` (NULL = the
 * context's stream) as pt_render_tiles_device queues its work; returns
 * without waiting. */
int pt_to_color_device(pt_ctx* ctx, const float* hdr_dev, int32_t width, int32_t height, int32_t x0, int32_t y0,
                       int32_t x1, int32_t y1, uint32_t* rgba_dev, void* stream);

/* ---- Progressive film (no reference counterpart: the reference renders one
 * pass and forgets it; its display loop, Application::render ->
 * PathTracer::update_screen, application.cpp:142-160, pathtracer.cpp:129-148,
 * redraws frameBuffer).  A film is device memory of one frame size owned by a
 * context: it accumulates passes, keeps a per-pixel error estimate, and
 * resolves on the GPU to the HDR mean, to pt_to_color's RGBA8 codes and to
 * the error, so a display loop copies 4 B per pixel instead of 12 and
 * tonemaps nothing on the host, and a caller can drop converged tiles.
 *
 * Per-pixel state: sum[3] f32, n u32, mu f32, M2 f32, k u32, all zero when
 * clear.  For a pixel inside a pass's tiles whose pass value is m -- exactly
 * what pt_render_tiles_device writes for the context's params with
 * sample_base = the film's next sample index -- and w = (float)spp, each line
 * one separately rounded IEEE f32 operation per operator, nothing fused:
 *   sum_c = sum_c + m_c * w                              c = r, g, b
 *   n     = n + spp
 *   L     = (0.2126f*m_r + 0.7152f*m_g) + 0.0722f*m_b    (Spectrum::illum)
 *   W     = (float)n
 *   d     = L - mu
 *   mu    = mu + d * (w / W)
 *   M2    = M2 + (w * d) * (L - mu)
 *   k     = k + 1
 * Resolve: hdr_c = n ? sum_c / (float)n : 0;  rgba = pt_to_color(hdr)
 * (0xFF000000 for a pixel never rendered);
 *   err = k < 2 ? +inf
 *               : sqrtf((fmaxf(M2, 0) / (float)n) / (float)(k - 1)) / fmaxf(mu, PT_FILM_LUM_FLOOR)
 * the standard error of the pass-weighted mean luminance relative to that
 * mean (floored).
 *
 * Calls on a context and its films are serialised by the caller.  Stream
 * semantics are pt_render_tiles_device's: a call returns when its work is
 * queued, results are written in `stream` order (NULL = the context's
 * stream); when consecutive operations on one film come on different streams
 * the library orders them with an event.  pt_destroy frees a context's
 * remaining films (their handles are dead afterwards). */
#define PT_FILM_LUM_FLOOR 1e-3f
typedef struct pt_film pt_film;
typedef struct pt_film_info {
  int32_t width;
  int32_t height;
  int64_t passes;        /* pt_film_add_pass calls since creation / the last pt_film_clear */
  uint64_t next_sample;  /* sample index the next pass starts at (0 .. 2^32) */
  double accumulate_ms;  /* device time of the last accumulate kernel (hipEvent; 0: none yet) */
  double resolve_ms;     /* device time of the last resolve kernel (hipEvent; 0: none yet) */
} pt_film_info;
int pt_film_create(pt_ctx* ctx, int32_t width, int32_t height, pt_film** out);
int pt_film_destroy(pt_film* film); /* NULL is PT_OK */
/* As freshly created: every record zero, the next sample index back to 0. */
int pt_film_clear(pt_film* film, void* stream);
/* Renders the listed tiles with the context's scene, camera and pt_params --
 * except sample_base, for which the film substitutes its next sample index --
 * into a pass buffer the film owns, and accumulates them.  The index then
 * advances by spp whatever the tile list, so K passes of s samples draw
 * exactly the sample set of one K*s-sample render.  The context's params are
 * unchanged afterwards.  PT_E_INVALID (film unchanged): the params' frame
 * size differs from the film's, tiles of one call overlap (a sample set would
 * count twice), or next_sample + spp > 2^32. */
int pt_film_add_pass(pt_film* film, const pt_tile* tiles, int32_t n_tiles, void* stream);
/* Whole-frame resolve into device buffers, each nullable, laid out as the
 * frame: hdr W*H*3 float (y = 0 at the bottom), rgba W*H uint32 as pt_to_color
 * writes it, err W*H float. */
int pt_film_resolve_device(pt_film* film, float* hdr_dev, uint32_t* rgba_dev, float* err_dev, void* stream);
/* The same into host buffers; waits.  A display loop passes only rgba_host. */
int pt_film_resolve(pt_film* film, float* hdr_host, uint32_t* rgba_host, float* err_host);
/* err_host[i] = the maximum of err over tile i clipped to the frame: +inf while
 * any of its pixels has fewer than two passes, 0 for an empty clipped tile.  Waits. */
int pt_film_tile_error(pt_film* film, const pt_tile* tiles, int32_t n_tiles, float* err_host);
/* Waits for the last accumulate and resolve kernels (their times). */
int pt_film_get_info(pt_film* film, pt_film_info* out);
/* Sets the sample index the next pass starts at (a film that continues an
 * earlier render, or one rank's share of a sample split).  Host state only. */
int pt_film_set_next_sample(pt_film* film, uint32_t next_sample);

/* ---- The film's records out and in: export and merge (no reference
 * counterpart).  A record buffer of a W x H film is 2*W*H*16 bytes in the
 * film's own layout, pixel p = x + y*W, y = 0 the bottom row:
 *   rec[p]       = {sum.r, sum.g, sum.b, n}   f32 f32 f32 u32
 *   rec[W*H + p] = {mu, M2, k, pad}           f32 f32 u32 u32
 * pt_film_export* copies the film's records out.  pt_film_merge* combines
 * incoming records into the film, film <- film (+) rec: per pixel the pairwise
 * combine of two Welford states (Chan, Golub, LeVeque 1979).  With it the
 * films of a multi-GPU split are joined (each rank's film over its own tiles,
 * or one film per sample range set with pt_film_set_next_sample), and a film
 * is checkpointed: restore = pt_film_create + pt_film_merge of the saved
 * records + pt_film_set_next_sample; the merge into a clear film takes every
 * pixel bit for bit.
 *
 * Like the film's, the arithmetic is a definition: every operator one
 * separately rounded IEEE f32 operation in the order written, nothing fused,
 * `/` correctly rounded.  For pixel p, a = the film's two records, b = the
 * incoming ones; each pixel falls into exactly one class:
 *   empty    n_b == 0:                      a is unchanged
 *   taken    n_a == 0, n_b > 0:             both records become b's bit for bit, pad included
 *   refused  n_a + n_b does not fit in 32 bits:   a is unchanged
 *   merged   otherwise:
 *     sum_c = sum_a_c + sum_b_c                           c = r, g, b
 *     n     = n_a + n_b
 *     W     = (float)n
 *     d     = mu_b - mu_a
 *     mu    = mu_a + d * ((float)n_b / W)
 *     M2    = (M2_a + M2_b) + (d * d) * (((float)n_a * (float)n_b) / W)
 *     k     = k_a + k_b
 *     pad   = pad_a
 * The merge is NOT bitwise commutative or associative (a (+) b and b (+) a
 * round differently): a caller who needs reproducible bits merges in a fixed
 * order, as dist.FilmExchange merges ranks 1 .. N-1 into rank 0 in rank order.
 * Where the two films cover disjoint pixels every pixel is taken or empty and
 * the order does not matter.
 *
 * passes, next_sample, the feature records and their presence are not
 * touched: a caller who continues a render calls pt_film_set_next_sample.
 * The incoming records must be a film's (finite, k <= n): the kernel checks
 * nothing but the overflow of n.  PT_E_INVALID, film unchanged: a NULL film or
 * buffer, or a device buffer that overlaps the film's own records.  Stream
 * semantics and cross-stream ordering as the other film calls: the _device
 * calls return when queued and read / write the caller's buffer in `stream`
 * order; the host calls wait (pt_film_merge stages through a buffer the film
 * owns). */
typedef struct pt_film_merge_info {
  int64_t merged;   /* pixels of the last merge per class; the four sum to W*H */
  int64_t taken;
  int64_t empty;
  int64_t refused;
  double merge_ms;  /* device time of the last merge kernel (hipEvent) */
} pt_film_merge_info;
int pt_film_export_device(pt_film* film, void* rec_out_dev, void* stream);
int pt_film_export(pt_film* film, void* rec_out_host);
int pt_film_merge_device(pt_film* film, const void* rec_dev, void* stream);
int pt_film_merge(pt_film* film, const void* rec_host);
/* Of the film's last merge (all zero before the first); waits for it. */
int pt_film_get_merge_info(pt_film* film, pt_film_merge_info* out);
/* Diagnostics: the device address of the film's own records at the moment
 * (a pt_film_reproject swaps them for another allocation), so that a test can
 * hand pt_film_merge_device / pt_film_export_device a buffer that overlaps
 * them.  Not for reading or writing the records: export and merge do that in
 * stream order. */
int pt_debug_film_records(pt_film* film, void** rec_dev);

/* ---- First-hit feature buffers (no reference counterpart: the reference's
 * Intersection of the camera ray, trace_ray pathtracer.cpp:435-456, never
 * leaves trace_ray).  A feature buffer of a W x H frame is two planes of 16-B
 * records in one allocation of 2*W*H*16 bytes, laid out as the film: pixel
 * p = x + y*W, y = 0 the bottom row:
 *   feat[p]       = {N.x, N.y, N.z, bsdf}   f32 f32 f32 i32   unit shading normal, BSDF index
 *   feat[W*H + p] = {P.x, P.y, P.z, z}      f32 x4            hit point, ray parameter t of the hit
 * of the nearest hit of the ray pt_render_tiles traces through the pixel's
 * CENTRE (its jitter replaced by 0.5, 0.5; the origin on the screen plane, the
 * direction normalised, so z is a distance from the screen plane's point).  P
 * is rebuilt from the primitive as the renderer's hit point is (barycentrics /
 * sphere reprojection); N is the interpolated vertex normal, flipped to face
 * the ray on a triangle and outward on a sphere, normalised (the zero vector
 * if it has no length).  A miss writes {0, 0, 0, -1} and {0, 0, 0, 0}.
 * The records describe the FIRST hit only: on a mirror or glass surface they
 * are the mirror's or the glass's own, not those of what is seen in or
 * through it.
 *
 * Frame size, scene and camera are the context's (PT_E_NOSCENE before
 * pt_upload_scene / pt_set_camera / pt_set_params); tiles are clipped to the
 * frame and only records of pixels inside them are written.  Stream semantics
 * are pt_render_tiles_device's; the kernel runs on `stream` itself. */
int pt_render_features_device(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, void* feat_dev, void* stream);
/* The same into a host buffer of 2*width*height*16 bytes; waits. */
int pt_render_features(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, void* feat_host);

/* ---- Ray queries on the device (BVHAccel::intersect, src/bvh.cpp:331-362, for
 * rays and results that live in device memory, in stream order; pt_intersect
 * stays the host-side diagnostic).  A ray is 32 bytes, two float4:
 *   ray[2i]     = {o.x, o.y, o.z, tmax}
 *   ray[2i + 1] = {d.x, d.y, d.z, unused}
 * d is of unit length (the caller's contract, as pt_intersect's: it is neither
 * checked nor normalised).  tmax is clamped to 3.0e38, the traversal's "far",
 * so +inf is welcome.  A ray is INVALID, is never traversed, reports a miss /
 * unoccluded and is counted in pt_trace_info.invalid when a component of o or
 * d is not finite, d is all zero, tmax is NaN or <= 0, or o over d overflows
 * f32 on all three axes (origins beyond 1e38 at unit directions).
 *
 * PT_TRACE_CLOSEST: the nearest hit in (0, tmax), 32 bytes per ray:
 *   out[2i]     = {t, u, v, prim}        f32 f32 f32 i32
 *   out[2i + 1] = {N.x, N.y, N.z, bsdf}  f32 f32 f32 i32
 * prim is the primitive's index in the caller's order (whatever tree renders),
 * u and v the triangle test's barycentrics (0 on a sphere), {N, bsdf} the
 * feature record pt_render_features* writes for that hit.  A miss is
 * {-1, 0, 0, -1} and {0, 0, 0, -1}.
 * PT_TRACE_OCCLUDED: whether anything lies in (0, tmax), one bit per ray: ray
 * i is bit i % 32 of the uint32 word i / 32.  The output is ceil(n / 64) * 2
 * words; bits at or past n are written as zero.
 *
 * pt_trace_rays_device queues the kernel on `stream` (NULL: the context's) and
 * returns; the results are in stream order (pt_render_features_device's
 * semantics).  n == 0 is PT_OK and launches nothing.  PT_E_INVALID: a NULL
 * context or buffer, n < 0 or > 2^40, an unknown mode, ray and output ranges
 * that overlap; PT_E_NOSCENE before pt_upload_scene.  The grid is bounded by
 * what the device holds at once (and by the environment variable
 * PT_TRACE_WAVES, read at each call: a testing knob), each wave taking every
 * grid-th chunk of 64 rays; the context's spill area and counter are reused
 * from call to call, and a trace on another stream than the last waits for it. */
#define PT_TRACE_CLOSEST 0
#define PT_TRACE_OCCLUDED 1
typedef struct pt_trace_info {
  int64_t rays, hits, invalid; /* of the last trace: rays given, hits / occluded rays, invalid rays */
  double trace_ms;             /* its kernel, between HIP events */
} pt_trace_info;
int pt_trace_rays_device(pt_ctx* ctx, int64_t n, const void* rays_dev, void* out_dev, int32_t mode, void* stream);
/* The same from and into host buffers: stages, waits. */
int pt_trace_rays(pt_ctx* ctx, int64_t n, const void* rays_host, void* out_host, int32_t mode);
/* The ray pt_render_features* traces through the centre of each pixel of the
 * listed tiles (clipped to the frame), written at ray[2p], p = x + y*W, of a
 * buffer of width*height rays, with tmax = 3.0e38; pixels outside the tiles
 * are left alone.  Frame size, scene and camera are the context's
 * (PT_E_NOSCENE before pt_upload_scene / pt_set_camera / pt_set_params);
 * PT_E_INVALID for a NULL context or buffer or n_tiles < 0.  Queued on
 * `stream`. */
int pt_camera_rays_device(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, void* rays_dev, void* stream);
/* Of the context's last trace (all zero before the first, and after one of
 * n == 0); waits for it. */
int pt_get_trace_info(pt_ctx* ctx, pt_trace_info* out);

/* ---- Path tracing along the caller's rays (no reference counterpart: the
 * reference's radiance loop, PathTracer::trace_ray pathtracer.cpp:415-553, is
 * only reachable through Camera::generate_ray).  The third ray query: after
 * "what does this ray hit" and "is it occluded", "what radiance arrives along
 * it" -- light probes, lightmap texels, other camera models, an environment map
 * baked from inside a scene.
 *
 * rays_dev holds width*height rays in pt_trace_rays_device's layout, ray p at
 * ray[2p], p = x + y*W: exactly what pt_camera_rays_device writes.  Frame size,
 * spp, max_depth, ns_area_light, seed and sample_base are the context's
 * pt_params; the output and the tiles are pt_render_tiles_device's (W*H*3
 * floats, only pixels inside the tiles are written).
 *
 * Replay (flags == 0): every sample k = 0 .. spp-1 of pixel p follows ray p.
 * Its random stream is the camera path's, keyed by (seed, p, sample_base + k);
 * the two jitter draws are taken and discarded, so every later draw has the
 * dimension it has on the camera path.  o and d are used as given (d of unit
 * length: the caller's contract, as pt_trace_rays').  tmax is clamped to
 * 3.0e38 and bounds the FIRST segment only: when nothing is hit inside it the
 * sample is a miss -- it sees the environment map if there is one, else
 * nothing.  A ray that pt_trace_rays* calls INVALID (a component not finite, a
 * zero direction, tmax NaN or <= 0, o over d overflowing on all three axes) is
 * never traversed and every one of its samples contributes exactly 0, with an
 * environment light too.  No screen-footprint cull applies, and the context's
 * camera plays no part: replay needs a scene and params only.
 *
 * Capture (PT_FLAG_RAYS_CAPTURE; spp must be 1): the same kernel generates
 * each pixel's ray as pt_render_tiles_device does for sample sample_base,
 * stores {o, 3.0e38} and {d, 0} into rays_dev and renders it: the image is
 * pt_render_tiles_device's bit for bit, the rays are the ones its samples
 * took, and a replay of them gives the same image again.  Rays of pixels
 * outside the tiles are left alone.
 *
 * PT_E_INVALID, nothing launched: a NULL context or buffer, n_tiles < 0, a
 * flag other than 0 / PT_FLAG_RAYS_CAPTURE, capture with spp != 1, a ray
 * buffer that overlaps the output.  PT_E_NOSCENE before pt_upload_scene or
 * pt_set_params, and for a capture before pt_set_camera.
 *
 * Stream semantics are pt_render_tiles_device's, and the rays are READ in
 * `stream` order too: after everything queued on `stream` before the call
 * (the render kernel, on a stream of the context's, waits for it).  Captured
 * rays and the image are complete in `stream` order. */
#define PT_FLAG_RAYS_CAPTURE 16u
int pt_render_rays_device(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, void* rays_dev, float* hdr_out_dev,
                          void* stream, uint32_t flags);
/* The same from and into host buffers (the rays are written back after a
 * capture): stages, waits. */
int pt_render_rays(pt_ctx* ctx, const pt_tile* tiles, int32_t n_tiles, void* rays_host, float* hdr_out_host,
                   uint32_t flags);
/* pt_film_add_pass with the pass rendered by replay of rays_dev: the same
 * sample numbering, accumulation and refusals (and a NULL ray buffer, or one
 * that overlaps the film's pass buffer: PT_E_INVALID).  A film may mix camera
 * passes and ray passes. */
int pt_film_add_pass_rays(pt_film* film, const pt_tile* tiles, int32_t n_tiles, const void* rays_dev, void* stream);

/* ---- Denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010)
 * guided by the feature records and, as the spatial pass of SVGF, by the
 * variance of the pixel's mean luminance, which the film already keeps.  No
 * reference counterpart.  Like the film's, the arithmetic is a definition:
 * every operator below is one separately rounded IEEE f32 operation, in the
 * order written, nothing fused, `/` and sqrtf correctly rounded, no
 * transcendental.
 *
 * Working record per pixel: cv[p] = {r, g, b, v}, 16 B; v is the variance of
 * the mean luminance, v == +inf means unknown (fewer than two passes), and
 * !(v >= 0) marks an invalid pixel (never rendered, or NaN): it is never used
 * as a tap and comes out as {0, 0, 0, -1}.
 *
 * Iteration i = 0 .. iterations-1 reads one cv buffer and writes another with
 * step s = 1 << i.  For a valid centre p with records c_p = cv[p].rgb,
 * v_p = cv[p].v, N_p, bsdf_p, P_p, z_p (a centre whose colour is not finite is
 * copied through unchanged), and L(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b:
 *
 * Variance prefilter, only when v_p is finite: 3x3 taps at distance 1
 * whatever s is, dy = -1..1 outer, dx = -1..1 inner; a tap counts if it is in
 * the frame, valid and its v finite; weights g = 1/4 centre, 1/8 edge, 1/16
 * corner; sums start at 0 and a tap adds sv = sv + g*v, sg = sg + g;
 *   vf = sv / sg;  sd = sqrtf(vf);  den = sigma_l*sd + 1e-6f
 *
 * Taps: dy = -2..2 outer, dx = -2..2 inner, q = p + s*(dx, dy),
 * k[0] = 0.375f, k[1] = 0.25f, k[2] = 0.0625f, h = k[|dx|]*k[|dy|].  q is
 * skipped when it is outside the frame, invalid, any channel of c_q is not
 * finite, or bsdf_q != bsdf_p (which also separates hit from miss, and the
 * emitter quad from the coplanar ceiling).  The centre tap has w = h.  Otherwise
 *   bsdf_p >= 0:  c   = fmaxf(0, (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z)
 *                 c   = c*c, normal_squarings times;  w_n = c
 *                 d   = P_q - P_p
 *                 x_p = fabsf((N_p.x*d.x + N_p.y*d.y) + N_p.z*d.z) / (sigma_p * z_p)
 *                 w_p = fmaxf(0, 1 - x_p)
 *   bsdf_p <  0:  w_n = w_p = 1
 *   x_l = fabsf(L(c_q) - L(c_p)) / den;  w_l = 1 / (1 + x_l*x_l)    (w_l = 1 when v_p is +inf)
 *   w   = ((h*w_n)*w_p)*w_l
 *   vq  = v_q == +inf ? v_p : v_q
 *   sum_c = sum_c + w*c_q (c = r, g, b);  sum_w = sum_w + w;  sum_v = sum_v + (w*w)*vq
 * (sums start at 0; a skipped tap leaves them untouched).  Output:
 *   out.rgb = sum_c / sum_w;   out.v = v_p == +inf ? +inf : sum_v / (sum_w*sum_w)
 *
 * Limitation: the guides are first-hit features.  On mirror and glass
 * surfaces they are constant where the reflected or refracted image has
 * edges, so only the luminance weight keeps those edges, and the filter gains
 * less there (measured: DESIGN.md). */
typedef struct pt_denoise_params {
  int32_t iterations;        /* 1 .. 6 */
  int32_t normal_squarings;  /* 0 .. 10: the normal weight is cos^(2^normal_squarings) */
  float sigma_l;             /* > 0: luminance differences are measured in sigma_l standard deviations */
  float sigma_p;             /* > 0: plane distances are measured in sigma_p * z_p */
} pt_denoise_params;
#define PT_DENOISE_SIGMA_P 0.05f
/* iterations 5, normal_squarings 7 (sigma_n = 128), sigma_l 4 (SVGF's), sigma_p PT_DENOISE_SIGMA_P
 * (the best of 0.005, 0.01, 0.02, 0.05 on the quality test's scenes: DESIGN.md). */
int pt_denoise_params_default(pt_denoise_params* out);
/* The filter on caller buffers: cv_dev (width*height*4 float) and feat_dev (a
 * feature buffer) in, out_cv_dev (width*height*4 float) out; input and output
 * must not overlap.  params NULL: the defaults; out-of-range values, or
 * sigma_l / sigma_p not > 0: PT_E_INVALID.  The iterations' ping-pong
 * buffers belong to the context (grown on demand, freed by pt_destroy).
 * Queued on `stream` (NULL = the context's stream); returns without waiting. */
int pt_denoise_device(pt_ctx* ctx, const float* cv_dev, const void* feat_dev, int32_t width, int32_t height,
                      const pt_denoise_params* params, float* out_cv_dev, void* stream);

/* ---- The film, denoised.  The film lazily owns a feature buffer and two cv
 * buffers.  pt_film_set_features renders the feature records of the listed
 * tiles with the context's current camera (the params' frame must be the
 * film's: PT_E_INVALID otherwise); a pixel never covered keeps the miss
 * record.  pt_film_clear marks the features absent again (when the camera
 * moves a display loop clears, or keeps the film with pt_film_reproject below).
 * pt_film_denoise_device: the film's records -> cv (prepare), the iterations,
 * then hdr_dev (W*H*3 float) and rgba_dev (W*H uint32, pt_to_color of hdr),
 * either of which may be NULL; the film's records are not changed.  Prepare:
 *   n == 0:  {0, 0, 0, -1}
 *   rgb = sum / (float)n
 *   v   = k >= 2 ? (fmaxf(M2, 0) / (float)n) / (float)(k - 1) : +inf
 * (the quantity under the film error's square root).  An invalid pixel comes
 * out as rgb 0, rgba 0xFF000000, as the resolve gives for a pixel never
 * rendered.  PT_E_INVALID: no features set since creation / the last clear,
 * the params' frame differs from the film's, bad parameters (NULL = the
 * defaults).  Stream semantics and ordering as the other film calls. */
int pt_film_set_features(pt_film* film, const pt_tile* tiles, int32_t n_tiles, void* stream);
int pt_film_denoise_device(pt_film* film, const pt_denoise_params* params, float* hdr_dev, uint32_t* rgba_dev,
                           void* stream);
/* The same into host buffers; waits.  A display loop passes only rgba_host. */
int pt_film_denoise(pt_film* film, const pt_denoise_params* params, float* hdr_host, uint32_t* rgba_host);

/* ---- Reprojection: the film kept across a camera move (the temporal half of
 * SVGF; the denoiser above is the spatial half).  No reference counterpart.
 * Instead of pt_film_clear, every pixel of the NEW camera's frame looks up
 * the pixel of the OLD camera's frame that saw the same surface point and
 * takes over its records; a pixel whose point the old frame did not see, or
 * whose radiance depends on the view, is reset.  Like the film's, the
 * arithmetic is a definition: every operator below is one separately rounded
 * IEEE f32 operation, in the order written, nothing fused, `/` correctly
 * rounded.
 *
 * Inputs for a W x H frame: the old records rec (the film's two 16-B planes,
 * {sum.r, sum.g, sum.b, n} and {mu, M2, k, pad}), the old feature buffer fo,
 * the new feature buffer fn, the old camera as f32 -- pos, the columns c0, c1,
 * c2 of c2w, ax = (float)(screen_w / screen_dist), ay likewise, each double
 * rounded once, the values the feature pass traces with -- and keep[b] per
 * BSDF index: 1 for PT_BSDF_DIFFUSE and PT_BSDF_EMISSION, 0 for mirror,
 * refraction and glass, whose radiance depends on the view.
 *
 * New pixel p, {N_p, bsdf_p} = fn[p], {P_p, z_p} = fn[W*H + p], is RESET (both
 * records all zero) unless every test passes; then it is KEPT:
 *   bsdf_p >= 0 && bsdf_p < n_bsdfs && keep[bsdf_p]      (a miss is reset: without an environment
 *                                                         light it converges in one pass, with one its
 *                                                         radiance depends on the direction)
 *   v  = P_p - pos
 *   cx = (v.x*c0.x + v.y*c0.y) + v.z*c0.z;  cy, cz likewise with c1, c2
 *   cz < 0                                                (in front of the old camera)
 *   iz = 0 - cz
 *   u  = ((cx / iz) / ax + 0.5f) * (float)W
 *   w  = ((cy / iz) / ay + 0.5f) * (float)H
 *   u >= 0 && u < (float)W && w >= 0 && w < (float)H      (a NaN fails)
 *   q  = (int)u + (int)w * W                              (the nearest tap: Welford states do not
 *                                                         interpolate, and one tap is bit-exact)
 *   {N_q, bsdf_q} = fo[q], {P_q, z_q} = fo[W*H + q]
 *   bsdf_q == bsdf_p
 *   c = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z;  c >= normal_cos_min
 *   d = P_q - P_p
 *   fabsf((N_p.x*d.x + N_p.y*d.y) + N_p.z*d.z) <= sigma_p * z_p     (occluders and disocclusions)
 *   rec[q].n > 0
 * A kept pixel takes q's two records bit for bit when max_samples == 0 or
 * n <= max_samples; otherwise, with n' = max_samples:
 *   f = (float)n' / (float)n;  sum'_c = sum_c * f;  mu' = mu;  M2' = M2 * f
 *   k' = max(1, (uint32)(((uint64)k * n') / n));  n' replaces n, pad is kept
 * so the per-pass variance M2 / n stays and the confidence shrinks: fresh
 * passes outweigh the history sooner.
 *
 * Limitation: the old samples were shaded for the old view; for the kept BSDF
 * types the first hit's outgoing radiance does not depend on it.  Geometry
 * does not move between the two feature buffers. */
typedef struct pt_reproject_params {
  float normal_cos_min;  /* -1 .. 1: the least cosine between the two first hits' normals */
  float sigma_p;         /* > 0: the plane distance allowed, in units of z_p */
  uint32_t max_samples;  /* 0: no cap; else a kept pixel's n is cut to this many samples */
} pt_reproject_params;
#define PT_REPROJECT_NORMAL_COS_MIN 0.9f
#define PT_REPROJECT_SIGMA_P 0.02f
/* normal_cos_min PT_REPROJECT_NORMAL_COS_MIN, sigma_p PT_REPROJECT_SIGMA_P, max_samples 0.  The
 * candidates {0.8, 0.9, 0.95} x {0.005, 0.01, 0.02, 0.05} all keep the same pixels on the quality
 * test's scenes, where the BSDF index already separates the surfaces; the middle ones were taken
 * (DESIGN.md has the table and the argument). */
int pt_reproject_params_default(pt_reproject_params* out);
/* The gather on caller buffers: rec_dev (2*W*H records), feat_old_dev and
 * feat_new_dev (feature buffers) in, rec_out_dev (2*W*H records) out, which
 * must not overlap rec_dev.  old_cam's c2w must be orthonormal within 1e-9
 * (projection by dot products needs it).  bsdf_types_host: n_bsdfs PT_BSDF_*
 * values, read before the call returns; NULL: the uploaded scene's BSDFs
 * (PT_E_NOSCENE without one; n_bsdfs is ignored).  params NULL: the defaults;
 * a NaN, normal_cos_min outside [-1, 1] or sigma_p not > 0: PT_E_INVALID.
 * counts_dev (nullable): two uint64 on the device, overwritten with the kept
 * and the reset pixels.  Queued on `stream` (NULL = the context's stream);
 * returns without waiting. */
int pt_reproject_device(pt_ctx* ctx, const pt_camera* old_cam, const void* rec_dev, const void* feat_old_dev,
                        const void* feat_new_dev, int32_t width, int32_t height, const int32_t* bsdf_types_host,
                        int32_t n_bsdfs, const pt_reproject_params* params, void* rec_out_dev, uint64_t* counts_dev,
                        void* stream);
/* The film across a camera move: the caller has called pt_set_camera with the
 * NEW camera.  pt_film_set_features remembers the camera it rendered with;
 * pt_film_reproject renders the whole frame's features with the context's
 * current camera into a second feature buffer, gathers (records, features,
 * remembered camera) into a second record buffer, then swaps both pairs and
 * remembers the current camera (the second buffers are allocated at first use
 * and freed with the film).  passes and next_sample are not touched: fresh
 * passes keep drawing fresh sample indices.  PT_E_INVALID, film unchanged: no
 * features set since creation / the last clear, the params' frame differs
 * from the film's, the remembered camera's c2w is not orthonormal, bad
 * parameters (NULL = the defaults).  Stream semantics and ordering as the
 * other film calls. */
int pt_film_reproject(pt_film* film, const pt_reproject_params* params, void* stream);
typedef struct pt_reproject_info {
  int64_t kept;         /* pixels of the last pt_film_reproject that took over records */
  int64_t reset;        /* pixels it reset; kept + reset = width * height */
  double reproject_ms;  /* device time of its gather kernel alone (hipEvent; 0: none yet) */
} pt_reproject_info;
/* Of the film's last pt_film_reproject (all zero before the first); waits for it. */
int pt_film_get_reproject_info(pt_film* film, pt_reproject_info* out);

/* Diagnostics for pt_to_color's tabulated codes: the number of float bit patterns in
 * [lo_bits, hi_bits) whose tabulated 8-bit code differs from the direct evaluation
 * code8(powf(s * exposure, 1 / 2.2)) (0 = the table is exact there). */
int64_t pt_to_color_check(uint32_t lo_bits, uint32_t hi_bits);
/* Diagnostics for the environment light's inverse-CDF sampling (host only): builds
 * EnvironmentLight's tables (src/static_scene/environment_light.cpp:6-48) for the
 * width x height float RGB map and replays the kernel's guide-record search
 * (pt_device.h record_lower_bound) for n query pairs (u1[i], u2[i]) in [0, 1)
 * against std::lower_bound, as importanceSampling's two searches
 * (environment_light.cpp:69-115): returns how many searches disagreed in the index
 * or the interpolation pair (0 = exact), or a negative PT_E_*; *long_windows (nullable)
 * receives how many searches took the window-halving path. */
int64_t pt_env_search_check(const float* rgb, int32_t width, int32_t height, int64_t n, const float* u1,
                            const float* u2, int64_t* long_windows);
/* Diagnostics (host only, no context): EnvironmentLight's float tables for the
 * width x height float RGB map exactly as an upload builds them and sends them to
 * the device -- p_theta[height] (pTheta, running sums over rows), p_phi[height *
 * width] (pPhiGivenTheta, running sums within each row) and pdf[height * width]
 * (pThetaPhi).  Any output pointer may be NULL and is skipped.  PT_E_INVALID for a
 * NULL map or a non-positive size. */
int pt_env_tables(const float* rgb, int32_t width, int32_t height, float* p_theta, float* p_phi, float* pdf);
/* Diagnostics (no reference counterpart): the render kernel's own environment-light
 * device functions on the uploaded scene's tables, one lane per query; waits.
 * For each of n pairs (u1[i], u2[i]) in [0, 1): the row and column that the two
 * inverse-CDF searches of the sampler return (pt_device.h record_lower_bound, called
 * with the sampler's arguments) and their interpolation pairs row_pair[2i], [2i+1] =
 * (prev, cur), col_pair likewise; then the sampler itself: wi[3i..], pdf[i] and the
 * texel coordinates (tu[i], tv[i]) it drew at, and radiance[3i..], the bilinear
 * lookup at those coordinates.  For each of m unit directions dirs[3j..]:
 * dir_radiance[3j..], the lookup by direction (EnvironmentLight::sample_dir).
 * Nothing is launched unless every query is valid: PT_E_INVALID for a negative or
 * too large (> 2^24) count, a NULL pointer with a positive count, a u outside
 * [0, 1), a non-finite direction or one whose length is not within 1e-3 of 1, and
 * for a scene without an environment light; PT_E_NOSCENE before an upload. */
int pt_debug_env_probe(pt_ctx* ctx, int64_t n, const float* u1, const float* u2, int32_t* row, int32_t* col,
                       float* row_pair, float* col_pair, float* wi, float* pdf, float* tu, float* tv, float* radiance,
                       int64_t m, const float* dirs, float* dir_radiance);

#ifdef __cplusplus
}
#endif

#endif /* PTGPU_H */
