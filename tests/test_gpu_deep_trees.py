"""Every kernel that walks the BVH, over trees deeper than the LDS stack.

The first PT_STACK (24) entries of a lane's traversal stack live in LDS, the
rest in a per-lane spill area in global memory; each client sizes its own
area on the host and strides it by its own grid in the kernel:

  render_kernel  plain / STATS / TRI / seam / small launch   RenderSlot::spill   test_render_*, test_tile_seam_*
  render_kernel  MF (frame batches)                          every slot's        test_frame_batch
  render_kernel  RAYS (the caller's rays)                    the slot's          test_render_plain_and_its_variants
  render_kernel  BIN + node_step2 (reference counts)         the slot's          test_reference_count_launch
  intersect_kernel (pt_intersect)                            q_spill             test_ray_queries
  features_kernel                                            f_spill             test_feature_pass
  trace_kernel<OCC>                                          tr_spill            test_ray_queries, test_ray_queries_regrid

The scenes are tests/deep_trees.py's ragged chain (96 layers under a chain
tree, uploaded with PT_BVH_BUILD=ref so that the chain itself is walked) and
its variant with a sphere, 64 x 64 frames at 2 spp, depth 4; the rays are the
frame's camera rays, then deep_rays.  That a launch really ran past entry
PT_STACK is asserted each time: by pt_stats.deep_stack_steps of a STATS
launch, or by stack_walk of the launch's own rays over the read-back tree
(tests/test_deep_trees_host.py checks the walk and the rays' coverage of the
boundary cases on the CPU).  Values are compared with the float64 brute force
(ray queries, features: the tolerances and the graze rule of
tests/test_gpu_trace.py), with the restatement (renders: the criterion of
test_hip_deep_bvh_stack_spill_vs_restatement), or bit for bit with a client
that is so compared.

A deep tree built on the GPU ("fat"): the staircase of tests/lbvh_scenes.py
reports a stack of 31, but no straight ray comes near it (its leaves lie along
three lines; test_gpu_built_deep_tree asserts the bound and the rays' highest
stack).  deep_trees.fat_staircase keeps the staircase's Morton cells, so the
GPU builds the same chain, with leaves that share a cube: its rays do go past
PT_STACK, and the ray-query and feature tests run over it as well.

Measured on an MI355X: the comment under VARIANTS below."""
import os

import numpy as np
import pytest

from dsgpuraytracing_amd import native, ptdump
from dsgpuraytracing_amd.pathtracer import Device, Scene, tile_fifo
from tests import bvh_check as bc
from tests import deep_trees as dt
from tests import lbvh_scenes as ls
from tests import trace_helpers as th
from tests.deep_trees import PT_STACK
from tests.film_helpers import bits, tile_mask
from tests.test_gpu_features import EXCUSED, brute_force, compare

pytestmark = pytest.mark.gpu

W = H = 64
SPP, DEPTH, NS_AREA, SEED = 2, 4, 1, 1
TILES32 = tile_fifo(W, H)  # four 32 x 32 tiles
RAGGED = [(33, 17, 5, 3), (0, 0, 32, 16)]
VARIANTS = ("chain", "sphere")

# What the assertions below state as inequalities, as observed on an MI355X:
#   ragged chain / sphere variant: 32 nodes, reported stack 95 = recomputed; of deep_rays 53.8 % / 53.4 %
#     peak at >= PT_STACK + 4, 37.4 % / 39.0 % at <= PT_STACK - 4, the rarest (height, pushes) pair in 68
#     node steps; 49.1 % / 48.7 % of the frame's camera rays and 49.1 % / 48.6 % of the captured
#     (jittered) rays go above PT_STACK; the highest stack of any ray is 95 / 94.
#   deep_stack_steps of the 64 x 64 x 2 spp STATS launch: 226,703 of 459,527 node visits / 232,388 of
#     537,449; of the reference-count launch over the binary chain: 428,094 of 1,352,304.
#   near-exact share against the restatement: 1.0 (plain, both variants, and the reference-count launch).
#   brute force: 0 rays excused on every scene (graze flags: 3 camera + 10 deep; fat staircase 332 + 55).
#   fat staircase (PT_LBVH_PASSES=0): 11 nodes, reported stack 31 = recomputed; every camera ray and
#     50 % of fat_staircase_rays go above PT_STACK, the highest stack is 30; deep_stack_steps 111,114
#     of 184,315 node visits.  The staircase itself: stack 31, its own rays' highest stack 3.


CHAIN_KNOBS = {"PT_BVH_BUILD": "ref"}  # the caller's chain itself (the SAH rebuild would balance it)
LBVH_KNOBS = {"PT_LBVH_PASSES": "0", "PT_COLLAPSE": None, "PT_LBVH_MAXLEAF": None, "PT_LBVH_CI": None}  # the bare Karras tree


def new_device(sc, gpu_bvh=False, knobs=CHAIN_KNOBS):
    """A context with the scene uploaded under the tree knobs (None: unset;
    the upload reads them, they are put back at once), the scene's camera and
    the frame."""
    old = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        dev = Device(0)
        dev.upload_scene(sc, gpu_bvh=gpu_bvh)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    dev.set_camera(sc.camera)
    dev.set_params(W, H, SPP, DEPTH, NS_AREA, SEED)
    return dev


def near_exact(img, ref):
    """Share of pixels within 1e-3 * max(1, |ref|) of the restatement."""
    return float((np.abs(img - ref).max(axis=2) <= 1e-3 * np.maximum(1.0, np.abs(ref).max(axis=2))).mean())


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Ctx:
    """One deep tree on one device -- the ragged chain ("chain"), its sphere
    variant ("sphere"), or the fat staircase built on the GPU ("fat") --: its
    ray set, the read-back tree, the walk of the rays over that tree, and
    what several tests share (the brute force, the plain render, the
    restatement), each computed once."""

    def __init__(self, variant, tmp):
        self.variant = variant
        if variant == "fat":
            self.d = dt.fat_staircase().dump()
            self.d["cam"] = dt.fat_staircase_camera(self.d["cam"])
            self.upload = dict(gpu_bvh=True, knobs=LBVH_KNOBS)
            extra = dt.fat_staircase_rays()
        else:
            self.d = dt.ragged_chain(sphere=variant == "sphere")
            self.upload = dict(gpu_bvh=False, knobs=CHAIN_KNOBS)
            extra = dt.deep_rays()
        self.path = str(tmp / f"{variant}.ptd")
        ptdump.write(self.path, self.d)
        self.sc = Scene(native.SceneArrays(self.d))
        self.dev = self.new_device()
        self.tree = self.dev.read_bvh()
        self.cam_rays = self.dev.camera_rays()
        self.n_cam = len(self.cam_rays)
        self.rays = np.concatenate([self.cam_rays, extra])
        self.walk_cam, self.walk_deep = self.walked(self.cam_rays), self.walked(self.rays[self.n_cam:])
        self.peak = np.concatenate([self.walk_cam["peak"], self.walk_deep["peak"]])  # of every ray of the set
        self.closest = self.dev.trace_rays(self.rays)
        self.occluded = self.dev.trace_rays(self.rays, mode="occluded")
        self._cache = {}

    def new_device(self):
        return new_device(self.sc, **self.upload)

    def walked(self, rays):
        return dt.stack_walk(self.tree["nodes4"], self.tree["prims"], *dt.as_doubles(rays))

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def reference(self):
        o, d, _ = dt.as_doubles(self.rays)
        return self.once("brute", lambda: th.brute_force_rays(self.sc.arrays, o, d))

    def restated(self, restate, spp=SPP):
        return self.once(("restated", spp), lambda: restate.render(self.path, W, H, spp, DEPTH, NS_AREA, SEED, rng_mode=1,
                                                                   threads=2)[0])

    def render(self, dev=None, tiles=((0, 0, W, H),), stats=False, spp=SPP, seed=SEED):
        dev = dev or self.dev
        dev.set_params(W, H, spp, DEPTH, NS_AREA, seed)
        img = np.zeros((H, W, 3), np.float32)
        dev.render_tiles(list(tiles), img, stats=stats)
        dev.set_params(W, H, SPP, DEPTH, NS_AREA, SEED)
        return img

    def plain(self, spp=SPP, seed=SEED):
        return self.once(("plain", spp, seed), lambda: self.render(spp=spp, seed=seed))


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """variant -> Ctx, made on first use."""
    have = {}
    tmp = tmp_path_factory.mktemp("deep")

    def get(variant):
        if variant not in have:
            have[variant] = Ctx(variant, tmp)
        return have[variant]

    yield get
    for c in have.values():
        c.dev.close()


@pytest.fixture(params=VARIANTS)
def ctx(request, made):
    return made(request.param)


@pytest.fixture(params=VARIANTS + ("fat",))
def any_ctx(request, made):
    return made(request.param)


@pytest.fixture
def chain(made):
    return made("chain")


def check_closest(got, ref, parts):
    """Closest-hit records against brute_force_rays: the tolerances and the
    EXCUSED / graze rule of tests/test_gpu_trace.py test_against_brute_force,
    per part (name, slice) of the ray set.  Returns the excused rays."""
    hit = got["prim"] >= 0
    z = np.where(ref["hit"], ref["t"], 1.0)
    with np.errstate(all="ignore"):
        bad = (hit != ref["hit"]) | (got["bsdf"] != ref["bsdf"])
        bad |= ref["hit"] & ~(np.abs(got["t"] - ref["t"]) <= 1e-4 * z)
        bad |= ~(np.abs(got["normal"] - ref["N"]).max(-1) <= 1e-4)
        sure = ref["hit"] & (ref["t2"] - ref["t"] > 1e-4 * z)
        bad |= sure & (got["prim"] != ref["prim"])
    miss = np.array([-1.0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    miss[[3, 7]] = np.int32(-1).view(np.float32)
    assert (bits(got["records"][~hit]) == bits(miss)).all()
    for what, sl in parts:
        print(what, "excused", int(bad[sl].sum()), "graze", int(ref["graze"][sl].sum()), "hit", int(hit[sl].sum()), "of",
              hit[sl].size, "prim compared", int(sure[sl].sum()))
        assert bad[sl].sum() <= EXCUSED, np.argwhere(bad[sl])
        assert ref["graze"][sl][bad[sl]].all(), np.argwhere(bad[sl] & ~ref["graze"][sl])
    assert sure.sum() > 0.9 * ref["hit"].sum()
    return bad


# ---- a. the tree

def test_tree_and_counter(ctx):
    t = ctx.tree
    assert bc.check_bvh4(t["nodes4"], t["prims"], t["info"], 8) == []
    assert t["prim_map"] is None  # the caller's chain, the caller's order
    stack = t["info"]["bvh_stack"]
    assert stack == bc.recomputed_stack(t["nodes4"]) == dt.chain_stack() and stack >= PT_STACK + 8
    # the rays of every test below reach the spill code, and every boundary case of it
    c = dt.coverage(ctx.walk_deep)
    cam = ctx.walk_cam["peak"]
    print(ctx.variant, "stack", stack, "deep_rays", c, "camera rays above PT_STACK", float((cam > PT_STACK).mean()),
          "highest", int(ctx.peak.max()))
    assert c["deep"] >= 0.40 and c["shallow"] >= 0.25 and c["rarest"] >= 16 and c["mixed"]
    assert (cam > PT_STACK).mean() >= 0.25 and (cam <= PT_STACK - 3).mean() >= 0.25
    img = ctx.render(stats=True)
    st = ctx.dev.stats()
    print(ctx.variant, "deep_stack_steps", st["deep_stack_steps"], "node_visits", st["node_visits"], "grid", st["grid_blocks"])
    assert st["counters_valid"] == 1 and st["deep_stack_steps"] > 0 and st["bvh_stack"] == stack
    assert same(img, ctx.plain())  # the STATS build's image


# ---- b. ray queries: trace_kernel<false / true> (tr_spill), intersect_kernel (q_spill)

def test_ray_queries(any_ctx):
    ctx = any_ctx
    dev, rays, got = ctx.dev, ctx.rays, ctx.closest
    n = len(rays)
    ref = ctx.reference()
    bad = check_closest(got, ref, (("camera", slice(0, ctx.n_cam)), ("deep", slice(ctx.n_cam, None))))
    assert ref["hit"][ctx.n_cam:].sum() > 500
    assert ((ctx.occluded != ref["hit"]) & ~bad).sum() == 0
    if ctx.variant == "sphere":
        assert (got["prim"] == dt.N_CHAIN - 1).sum() > 100
    # pt_intersect: the same walk from another kernel with another spill area, bit for bit
    o, d, _ = dt.as_doubles(rays)
    hit, t, prim, _ = dev.intersect(o, d, np.full(n, np.inf))
    assert np.array_equal(got["prim"] >= 0, hit == 1) and np.array_equal(got["prim"], prim)
    assert np.array_equal(bits(got["t"]), bits(t))
    # occlusion bits, tmax drawn around the hit distance: pt_intersect's any-hit
    rng = np.random.default_rng(5)
    tmax = np.where(hit == 1, t * rng.uniform(0.3, 1.7, n), 1.0).astype(np.float32)
    short = rays.copy()
    short[:, 3] = tmax
    _, _, _, any_hit = dev.intersect(o, d, tmax.astype(np.float64))
    occ = dev.trace_rays(short, mode="occluded")
    assert np.array_equal(occ, any_hit == 1) and 100 < occ.sum() < n - 100
    assert dev.trace_info()["hits"] == occ.sum()
    # (boxes beyond tmax are not entered, so fewer of the shortened rays go deep; hundreds still do)
    assert (ctx.walked(short)["peak"] > PT_STACK).sum() >= 256


def _guarded_trace(dev, rays):
    """(records, occlusion words) of the rays through the device entry point,
    64 guard words before and after each output checked (test_sizes' way)."""
    import torch
    n = len(rays)
    pad, words = 64, (n + 63) // 64 * 2
    r = torch.from_numpy(rays).to("cuda:0")
    rec = torch.full((pad + n * 8 + pad,), -7.0, dtype=torch.float32, device="cuda:0")
    occ = torch.full((pad + words + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dev.trace_rays(r, out=rec[pad:pad + n * 8].view(n, 8))
    dev.trace_rays(r, mode="occluded", out=occ[pad:pad + words])
    torch.cuda.synchronize()
    rec, occ = rec.cpu().numpy(), occ.cpu().numpy()
    assert (rec[:pad] == -7.0).all() and (rec[pad + n * 8:] == -7.0).all()
    assert (occ[:pad] == 0x5A5A5A5A).all() and (occ[pad + words:] == 0x5A5A5A5A).all()
    mask = np.unpackbits(occ[pad:pad + words].view(np.uint8), bitorder="little")
    assert (mask[n:] == 0).all()
    return rec[pad:pad + n * 8].reshape(n, 8), mask[:n].astype(bool)


def test_ray_queries_regrid(any_ctx, monkeypatch):
    """The spill area follows the grid: PT_TRACE_WAVES=3 (three waves, each
    over >= 10 chunks of 64 rays on the same spill columns), the knob unset
    (one wave per chunk: the area grows), 3 again -- on the context that has
    traced already, and on a fresh one whose first area is the small one.  A
    ragged last chunk (the set without its last 27 rays) rides along."""
    ctx = any_ctx
    rays = np.ascontiguousarray(ctx.rays[:len(ctx.rays) - 27])
    n = len(rays)
    assert (n + 63) // 64 >= 3 * 10 and n % 64
    want = ctx.closest["records"][:n], ctx.occluded[:n]
    assert (ctx.peak[n - n % 64:n] > PT_STACK).any()  # the ragged chunk goes deep too
    fresh = ctx.new_device()
    try:
        for dev in (ctx.dev, fresh):
            for knob in ("3", None, "3"):
                if knob is None:
                    monkeypatch.delenv("PT_TRACE_WAVES", raising=False)
                else:
                    monkeypatch.setenv("PT_TRACE_WAVES", knob)
                rec, occ = _guarded_trace(dev, rays)
                assert same(rec, want[0]), (dev is fresh, knob)
                assert np.array_equal(occ, want[1]), (dev is fresh, knob)
                assert dev.trace_info()["rays"] == n
    finally:
        fresh.close()


# ---- c. the feature pass: features_kernel (f_spill)

def _features_into(dev, tiles, sentinel):
    buf = np.full((2, H, W, 4), sentinel, np.float32)
    keep, arr = Device._tiles(tiles)
    native.check(native.lib().pt_render_features(dev.handle, arr, len(keep), buf.ctypes.data))
    return buf


def test_feature_pass(any_ctx):
    ctx = any_ctx
    dev = ctx.dev
    f = dev.render_features()
    compare(f, brute_force(ctx.sc.arrays, W, H))
    hit = f["bsdf"].reshape(-1) >= 0
    assert hit.sum() > 0.5 * W * H
    # the frame's camera rays through the ray queries: the same records bit for bit
    got, n_cam = ctx.closest, ctx.n_cam
    assert np.array_equal(got["bsdf"][:n_cam], f["bsdf"].reshape(-1))
    assert np.array_equal(bits(got["normal"][:n_cam]), bits(f["normal"].reshape(-1, 3)))
    assert np.array_equal(bits(got["t"][:n_cam][hit]), bits(f["depth"].reshape(-1)[hit]))
    # a ragged two-tile list into a sentinel-filled buffer (as given and reversed: the tile whose
    # rays all spill takes the first 16 blocks' columns of the area, then the next 16), after the
    # whole frame and -- on a fresh context, whose spill area then grows between the launches --
    # before it
    sentinel = np.float32(-12345.5)
    m = tile_mask(W, H, RAGGED)
    assert m.sum() == 5 * 3 + 32 * 16
    x, y, w, h = RAGGED[0]
    assert (ctx.walk_cam["peak"].reshape(H, W)[y:y + h, x:x + w] > PT_STACK).all()
    full = f["records"]
    fresh = ctx.new_device()
    try:
        parts = [_features_into(d, t, sentinel) for d in (dev, fresh) for t in (RAGGED, RAGGED[::-1])]
        whole = _features_into(fresh, TILES32, sentinel)
    finally:
        fresh.close()
    for buf in parts:
        assert same(buf[:, m], full[:, m]) and (buf[:, ~m] == sentinel).all()
    assert same(whole, full)


# ---- d. the render clients

def test_render_plain_and_its_variants(ctx, restate, monkeypatch):
    """render_kernel plain (TRI on the chain, the mixed kernel on the sphere
    variant) against the restatement; PT_NO_TRI_ONLY, the launch shape without
    the small-launch claim, and the RAYS kernel (capture, replay) bit for bit."""
    dev = ctx.dev
    img = ctx.plain()
    ref = ctx.restated(restate)
    close = near_exact(img, ref)
    print(ctx.variant, "near-exact share", close, "mean", float(img.mean()), "restatement", float(ref.mean()))
    assert np.isfinite(img).all() and (img.max(-1) > 0).mean() > 0.5 and close >= 0.99
    assert same(ctx.render(), img)  # (the next render slot, its own spill area)
    if ctx.variant == "chain":
        monkeypatch.setenv("PT_NO_TRI_ONLY", "1")
        assert same(ctx.render(), img)
        monkeypatch.delenv("PT_NO_TRI_ONLY")
        monkeypatch.setenv("PT_SMALL_LAUNCH", "0")
        assert same(ctx.render(), img)
        monkeypatch.delenv("PT_SMALL_LAUNCH")
    # capture (spp 1) is the renderer, the replay of the captured rays is the capture
    one = ctx.plain(spp=1)
    assert near_exact(one, ctx.restated(restate, 1)) >= 0.99 and one.any()
    dev.set_params(W, H, 1, DEPTH, NS_AREA, SEED)
    try:
        rays = np.full((W * H, 8), -5.0, np.float32)
        cap = dev.render_rays(rays, capture=True)
        assert same(cap, one)
        assert (rays[:, 3] == th.FAR).all() and not same(rays, ctx.cam_rays)  # (jittered)
        keep = rays.copy()
        assert same(dev.render_rays(rays), cap) and same(rays, keep)
    finally:
        dev.set_params(W, H, SPP, DEPTH, NS_AREA, SEED)
    peak = ctx.walked(rays)["peak"]
    print(ctx.variant, "captured rays above PT_STACK", float((peak > PT_STACK).mean()))
    assert (peak > PT_STACK).mean() >= 0.25


def test_frame_batch(chain):
    """render_kernel<MF>: three frames, seeds s, s + 1, s + 2, in one launch,
    on a context whose first launch it is (every slot's area is reserved by
    the batch), against the three single-frame launches."""
    import torch
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    dev = chain.new_device()
    try:
        arr = np.asarray(TILES32, np.int32).reshape(-1, 4)
        seeds = [SEED, SEED + 1, SEED + 2]
        outs = [torch.full((H * W * 3,), -1.0, dtype=torch.float32, device="cuda:0") for _ in seeds]
        dev.render_frames_device(arr, [o.data_ptr() for o in outs], seeds, stream.cuda_stream, out_floats=H * W * 3)
        torch.cuda.synchronize()
        assert dev.stats()["frames_per_launch"] == 3
        for s, o in zip(seeds, outs):
            assert same(o.cpu().numpy().reshape(H, W, 3), chain.plain(seed=s)), s
        assert not torch.equal(outs[0], outs[1])
        # and once more, now behind single-frame launches on the same slots
        for s in seeds:
            assert same(chain.render(dev, seed=s), chain.plain(seed=s))
        dev.render_frames_device(arr, [o.data_ptr() for o in outs[::-1]], seeds, stream.cuda_stream, out_floats=H * W * 3)
        torch.cuda.synchronize()
        for s, o in zip(seeds, outs[::-1]):
            assert same(o.cpu().numpy().reshape(H, W, 3), chain.plain(seed=s)), s
    finally:
        dev.close()


def test_tile_seam_and_single_tile(chain):
    """The tile seam (pt_tile_submit / pt_tile_finish over 32 x 32 tiles) and
    one 32 x 32 tile launched alone (a quarter of the frame's work slots: the
    small-launch shape), against the whole frame."""
    whole = chain.plain()
    dev = chain.new_device()
    try:
        x, y, w, h = TILES32[2]
        img = np.full((H, W, 3), -7.0, np.float32)
        dev.render_tiles([TILES32[2]], img)
        inside = tile_mask(W, H, [TILES32[2]])
        assert same(img[inside], whole[inside]) and (img[~inside] == -7.0).all() and whole[inside].any()
        hdr = np.zeros((H, W, 3), np.float32)
        for t in TILES32[::-1]:
            dev.submit_tile(t, hdr)
        dev.finish_tiles()
        assert same(hdr, whole)
    finally:
        dev.close()


# ---- e. the reference-count launch: render_kernel<BIN>, node_step2 over the binary chain

def test_reference_count_launch(chain, restate):
    ref = chain.restated(restate)
    chain.render(stats=True)
    st = chain.dev.stats()
    img = chain.render(stats="ref")
    rc = chain.dev.stats()
    close = near_exact(img, ref)
    print("reference counts: near-exact share", close, "deep_stack_steps", rc["deep_stack_steps"], "against",
          st["deep_stack_steps"], "node visits", rc["node_visits"], "against", st["node_visits"])
    assert np.isfinite(img).all() and img.any() and close >= 0.99
    assert rc["counters_valid"] == 1 and rc["camera_rays"] == st["camera_rays"] > 0
    assert rc["deep_stack_steps"] > 0
    assert len(chain.tree["nodes2"]) == dt.N_CHAIN - 1  # the binary chain: its stack reaches n - 1


# ---- f. a deep tree built on the GPU

def test_gpu_built_deep_tree(made, monkeypatch):
    """The Karras chain of the fat staircase (PT_LBVH_PASSES=0), read back:
    sound, its reported stack the tree's worst case and beyond PT_STACK, and
    -- unlike the staircase's own -- reached by real rays.  test_ray_queries,
    test_ray_queries_regrid and test_feature_pass run over this tree too."""
    ctx = made("fat")
    t = ctx.tree
    assert t["prim_map"] is not None
    assert bc.check_bvh4(t["nodes4"], t["prims"], t["info"], 4, exact_stack=True) == []
    assert bc.check_bvh2(t["nodes2"], t["nodes4"], t["prims"], t["info"], 4) == []
    stack = t["info"]["bvh_stack"]
    assert stack > PT_STACK
    deep, cam = ctx.walk_deep["peak"], ctx.walk_cam["peak"]
    g = deep.reshape(-1, 64)
    print("fat staircase: nodes", t["info"]["n_nodes4"], "stack", stack, "rays above PT_STACK", float((deep > PT_STACK).mean()),
          "camera rays", float((cam > PT_STACK).mean()), "highest", int(ctx.peak.max()))
    assert (deep > PT_STACK).mean() >= 0.10 and (cam > PT_STACK).mean() >= 0.10
    assert ((g > PT_STACK).any(1) & (g <= PT_STACK - 3).any(1)).all()  # deep and shallow lanes in every wave
    img = ctx.render(stats=True)
    st = ctx.dev.stats()
    print("fat staircase: deep_stack_steps", st["deep_stack_steps"], "node_visits", st["node_visits"])
    assert st["counters_valid"] == 1 and st["deep_stack_steps"] > 0 and st["bvh_stack"] == stack
    assert np.isfinite(img).all() and same(img, ctx.plain())
    # the staircase itself: the same chain and a bound beyond PT_STACK, but its leaves lie along
    # three lines -- a straight ray meets one axis' ten boxes, the origin's and the far corner's
    sc = ls.scene("staircase")
    dev = new_device(Scene(native.SceneArrays(sc.dump())), gpu_bvh=True, knobs=LBVH_KNOBS)
    try:
        s = dev.read_bvh()
    finally:
        dev.close()
    assert s["info"]["bvh_stack"] > PT_STACK
    o, d, _ = sc.rays()
    own = dt.stack_walk(s["nodes4"], s["prims"], o, d, np.full(len(o), float(dt.FAR)))["peak"]
    print("staircase: stack", s["info"]["bvh_stack"], "its own rays' highest stack", int(own.max()))
    assert own.max() <= 12
