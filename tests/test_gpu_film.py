"""The device-resident progressive film (include/ptgpu.h: pt_film_*) against
the numpy float32 restatement of its arithmetic (tests/film_helpers.py), bit
for bit: any FMA contraction, a wrong weight on unequal spp, a wrong clip at
the 6-wide / 5-high edge tiles of the 70x37 frame or a tonemap threshold off
by one ulp fails the uint32 comparisons."""
import ctypes
import os

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.pathtracer import Device, PathTracer, Scene, tile_fifo, to_color
from tests.film_helpers import FilmRestatement, bits, tile_mask, tile_max
from tests.oracle_helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAE = os.path.join(ROOT, "assets", "CBspheres_lambertian.dae")

pytestmark = pytest.mark.gpu

W, H, SEED = 70, 37, 5  # 3 x 2 tiles of widths 32 / 32 / 6 and heights 32 / 5
PASSES = ((4, 0), (2, 4), (8, 6))  # (spp, first sample index) of consecutive passes
FIFO = tile_fifo(W, H)
NEVER = 0xFF000000  # rgba of a pixel never rendered


def params(dev, spp, w=W, h=H, sample_base=12345):
    """The film substitutes its own sample index: the context's is a decoy."""
    dev.set_params(w, h, spp, 4, 1, SEED, sample_base=sample_base)


def render(dev, spp, base, w=W, h=H):
    params(dev, spp, w, h, sample_base=base)
    img = np.zeros((h, w, 3), np.float32)
    dev.render_tiles(tile_fifo(w, h), img)
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def odd():
    """One context on the all-diffuse scene at 70x37 and the independent
    renders of each pass, (spp, base) -> image, shared read-only."""
    sc = Scene.from_dae(DAE, W, H)
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    imgs = {sb: render(dev, *sb) for sb in PASSES + ((8, 0),)}
    assert all(np.isfinite(v).all() for v in imgs.values())
    yield dev, imgs
    dev.close()


def add_passes(dev, film, plan):
    """plan: (spp, tiles) per pass."""
    for spp, tiles in plan:
        params(dev, spp)
        film.add_pass(tiles)


def restate(imgs, plan, w=W, h=H):
    """The restatement of the same plan from the independent renders."""
    r = FilmRestatement(w, h)
    base = 0
    for spp, tiles in plan:
        r.add_pass(imgs[(spp, base)], spp, tile_mask(w, h, tiles))
        base += spp
    return r


def assert_film_equals(film, r):
    hdr, rgba, err = film.resolve()
    assert np.array_equal(bits(hdr), bits(r.hdr()))
    assert np.array_equal(bits(err), bits(r.err()))
    assert np.array_equal(rgba, to_color(hdr))
    return hdr, rgba, err


def same(a, b):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def test_film_accumulate_bit_exact(odd):
    dev, imgs = odd
    plan = [(spp, FIFO) for spp, _ in PASSES]
    film = dev.film(W, H)
    add_passes(dev, film, plan)
    _, _, err = assert_film_equals(film, restate(imgs, plan))
    assert np.isfinite(err).all()
    info = film.info()
    assert (info["width"], info["height"], info["passes"], info["next_sample"]) == (W, H, 3, 14)
    assert info["accumulate_ms"] > 0 and info["resolve_ms"] > 0
    film.close()


def test_film_partial_coverage_and_tile_error(odd):
    dev, imgs = odd
    one = [(33, 17, 5, 3)]
    plan = [(4, FIFO), (2, FIFO[::2]), (8, one)]
    film = dev.film(W, H)
    add_passes(dev, film, plan)
    r = restate(imgs, plan)
    _, _, err = assert_film_equals(film, r)
    twice = tile_mask(W, H, FIFO[::2]) | tile_mask(W, H, one)
    assert np.isfinite(err[twice]).all() and np.isinf(err[~twice]).all()
    # per-tile maxima, clipped: a tile hanging off the frame's corner, tiles wholly outside, an empty one
    tiles = FIFO + one + [(60, 30, 32, 32), (W, 0, 5, 5), (-10, -10, 5, 5), (3, 3, 0, 7), (0, 0, 32, 16)]
    te = film.tile_error(tiles)
    assert np.array_equal(bits(te), bits(tile_max(err, tiles)))
    n = len(FIFO)
    assert np.isfinite(te[[0, 2, 4, n, n + 5]]).all() and np.isinf(te[[1, 3, 5]]).all()
    assert te[n + 1] == tile_max(err, [(60, 30, 10, 7)])[0]
    assert (te[n + 2:n + 5] == 0).all()
    film.close()
    # a film that only ever received the small tile
    lone = dev.film(W, H)
    add_passes(dev, lone, [(8, one)])
    hdr, rgba, err = assert_film_equals(lone, restate(imgs, [(8, one)]))
    out = ~tile_mask(W, H, one)
    assert (bits(hdr)[out] == 0).all() and (rgba.view(np.uint32)[..., 0][out] == NEVER).all()
    assert np.isinf(err).all() and (err > 0).all()
    assert (hdr[~out] > 0).any()
    lone.close()


def test_film_passes_draw_the_samples_of_one_render():
    """4 passes x 4 spp against one 16-spp render: the same sample set, only
    the float summation order differs (the tolerance of
    test_gpu_render.py::test_hip_sample_passes_add_up, the same property)."""
    w = h = 64
    sc = Scene.from_dump(golden("c1_default_64x64.scene.ptd"))
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    ref = render(dev, 16, 0, w, h)
    film = dev.film(w, h)
    for _ in range(4):
        params(dev, 4, w, h)
        film.add_pass(tile_fifo(w, h))
    hdr, _, _ = film.resolve()
    assert np.allclose(hdr, ref, rtol=1e-5, atol=1e-6)
    assert film.info()["next_sample"] == 16
    dev.close()


def test_film_clear_and_isolation(odd):
    import torch
    dev, imgs = odd
    plan = [(4, FIFO), (2, FIFO[::2])]
    a = dev.film(W, H)
    add_passes(dev, a, [(8, FIFO)] + plan)
    a.clear()
    assert a.info()["passes"] == 0 and a.info()["next_sample"] == 0
    add_passes(dev, a, plan)
    fresh = dev.film(W, H)
    add_passes(dev, fresh, plan)
    assert same(a.resolve(), fresh.resolve())
    assert_film_equals(a, restate(imgs, plan))
    # the context's own sample_base survives a pass
    params(dev, 2, sample_base=4)
    frames = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dev.render_tiles_device(FIFO, frames[0].data_ptr())
    fresh.add_pass(FIFO)
    dev.render_tiles_device(FIFO, frames[1].data_ptr())
    torch.cuda.synchronize()
    got = frames.cpu().numpy()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.array_equal(bits(got[0]), bits(imgs[(2, 4)]))
    fresh.close()
    # two films of one context, interleaved
    a.clear()
    b = dev.film(W, H)
    plan_b = [(4, FIFO[1::2]), (2, [(20, 3, 30, 30)])]
    for (spp, ta), (_, tb) in zip(plan, plan_b):
        params(dev, spp)
        a.add_pass(ta)
        b.add_pass(tb)
    assert_film_equals(a, restate(imgs, plan))
    assert_film_equals(b, restate(imgs, plan_b))
    a.close()
    b.close()


def test_film_stream_order(odd):
    """Three passes and a resolve queued on a caller's stream without a host
    synchronisation in between (the film was cleared on the context's stream:
    the library orders the two)."""
    import torch
    dev, imgs = odd
    plan = [(spp, FIFO) for spp, _ in PASSES]
    film = dev.film(W, H)
    hdr = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    err = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ts = torch.cuda.Stream(device=0)
    for spp, tiles in plan:
        params(dev, spp)
        film.add_pass(tiles, stream=ts.cuda_stream)
    film.resolve_device(hdr.data_ptr(), rgba.data_ptr(), err.data_ptr(), stream=ts.cuda_stream)
    ts.synchronize()
    got = (hdr.cpu().numpy(), rgba.cpu().numpy().view(np.uint8).reshape(H, W, 4), err.cpu().numpy())
    assert same(got, film.resolve())
    assert_film_equals(film, restate(imgs, plan))
    film.close()


def test_film_errors_leave_the_film_unchanged(odd):
    dev, imgs = odd
    L = native.lib()
    film = dev.film(W, H)
    add_passes(dev, film, [(4, FIFO), (2, FIFO)])
    before, info = film.resolve(), film.info()

    def refused(tiles, what):
        with pytest.raises(native.PtError) as e:
            film.add_pass(tiles)
        assert e.value.code == native.PT_E_INVALID and "pt_film_add_pass" in str(e.value) and what in str(e.value)
        after = film.info()
        assert (after["passes"], after["next_sample"]) == (info["passes"], info["next_sample"])
        assert same(film.resolve(), before)

    params(dev, 8, w=64)
    refused(FIFO, "differs")
    params(dev, 8)
    refused([(0, 0, 32, 32), (31, 31, 4, 4)], "overlap")
    refused(FIFO + [(69, 36, 40, 40)], "overlap")
    t = native.pt_tile(0, 0, 1, 1)
    assert L.pt_film_add_pass(None, ctypes.byref(t), 1, None) == native.PT_E_INVALID
    assert b"NULL film" in L.pt_last_error()
    assert same(film.resolve(), before)
    film.close()
    # the sample range ends at 2^32: a 1x1 film, its index set near the end
    one = dev.film(1, 1)
    params(dev, 4, 1, 1)
    one.set_next_sample(2 ** 32 - 3)
    with pytest.raises(native.PtError) as e:
        one.add_pass([(0, 0, 1, 1)])
    assert e.value.code == native.PT_E_INVALID and "overflow" in str(e.value)
    assert one.info()["passes"] == 0 and one.info()["next_sample"] == 2 ** 32 - 3
    assert (one.resolve()[1].view(np.uint32) == NEVER).all()
    params(dev, 3, 1, 1)
    one.add_pass([(0, 0, 1, 1)])  # samples 2^32 - 3 .. 2^32 - 1: the last ones
    assert one.info()["next_sample"] == 2 ** 32
    params(dev, 1, 1, 1)
    with pytest.raises(native.PtError):
        one.add_pass([(0, 0, 1, 1)])
    one.close()


def test_film_one_pixel(odd):
    dev, _ = odd
    imgs = {(3, 0): render(dev, 3, 0, 1, 1), (5, 3): render(dev, 5, 3, 1, 1)}
    plan = [(3, [(0, 0, 1, 1)]), (5, [(-4, -4, 40, 40)])]
    film = dev.film(1, 1)
    for spp, tiles in plan:
        params(dev, spp, 1, 1)
        film.add_pass(tiles)
    r = restate(imgs, plan, 1, 1)
    hdr, rgba, err = film.resolve()
    assert np.array_equal(bits(hdr), bits(r.hdr())) and np.array_equal(bits(err), bits(r.err()))
    assert np.array_equal(rgba, to_color(hdr))
    assert np.array_equal(bits(film.tile_error([(0, 0, 1, 1)])), bits(err.reshape(1)))
    film.close()


def test_destroying_the_context_frees_its_films():
    L = native.lib()
    ctx, films = ctypes.c_void_p(), [ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()]
    native.check(L.pt_create(0, ctypes.byref(ctx)))
    for f, (w, h) in zip(films, ((W, H), (1, 1), (64, 64))):
        native.check(L.pt_film_create(ctx, w, h, ctypes.byref(f)))
    info = native.pt_film_info()
    native.check(L.pt_film_get_info(films[2], ctypes.byref(info)))
    assert (info.width, info.height, info.passes, info.next_sample, info.accumulate_ms) == (64, 64, 0, 0, 0.0)
    native.check(L.pt_film_destroy(films[1]))  # one by hand, the rest with the context
    assert L.pt_film_create(ctx, 0, 5, ctypes.byref(films[1])) == native.PT_E_INVALID and films[1].value is None
    assert L.pt_destroy(ctx) == native.PT_OK


def test_render_progressive():
    spp, n_pass = 4, 4
    sc = Scene.from_dae(DAE, W, H)
    pt = PathTracer(ns_aa=spp, max_ray_depth=4, ns_area_light=1, seed=SEED)
    pt.set_frame_size(W, H)
    pt.set_camera(sc.camera)
    pt.set_scene(sc)
    dev = pt._device()
    imgs = [render(dev, spp, p * spp) for p in range(n_pass)]

    def check_buffers():
        lp = pt.last_progressive
        assert lp["tiles"] == FIFO and lp["spp"] == spp
        r = FilmRestatement(W, H)
        for p in range(int(lp["passes"].max())):
            r.add_pass(imgs[p], spp, tile_mask(W, H, [t for t, c in zip(FIFO, lp["passes"]) if c > p]))
        assert np.array_equal(bits(pt.sampleBuffer), bits(r.hdr()))
        assert np.array_equal(pt.frameBuffer, to_color(pt.sampleBuffer))
        assert np.array_equal(bits(lp["tile_error"]), bits(tile_max(r.err(), FIFO)))
        return lp

    pt.render_progressive(n_pass, target_error=float("inf"))
    assert (check_buffers()["passes"] == 2).all()
    pt.render_progressive(n_pass, target_error=0.0)
    lp = check_buffers()
    assert ((lp["passes"] == n_pass) | (lp["tile_error"] == 0)).all()
    pt.render_progressive(n_pass, target_error=0.05)
    lp = check_buffers()
    assert ((lp["passes"] >= 2) & (lp["passes"] <= n_pass)).all()
    assert ((lp["passes"] == n_pass) | (lp["tile_error"] <= 0.05)).all()
    pt.render_progressive(3)
    assert (check_buffers()["passes"] == 3).all()
