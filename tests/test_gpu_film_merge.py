"""The film's records out and in (include/ptgpu.h: pt_film_export*,
pt_film_merge*) against the numpy restatements of the film
(tests/film_helpers.py) and of the merge (tests/film_merge_helpers.py), bit
for bit: an FMA contraction in the combine, a swapped n_a / n_b, a pad that
is not carried, a wrong clip at the 6-wide / 5-high edge tiles of the 70x37
frame or a miscounted class fails the uint32 comparisons.  On top: the tile
split and the checkpoint are exact, the sample split is within the bound of
two summation orders, the calls are ordered across streams and every buffer
goes with the film.  C1 at 64x64 (and stretched to 70x37), passes of 1-5 spp."""
import ctypes
import gc

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.dist import FilmExchange, film_passes_sample_split, film_passes_tile_split
from dsgpuraytracing_amd.pathtracer import Device, Film, Scene, tile_fifo
from tests.film_helpers import FilmRestatement, bits, tile_mask
from tests.film_merge_helpers import CLASSES, classes, from_records, merge_records, records
from tests.oracle_helpers import golden

pytestmark = pytest.mark.gpu

SEED = 5
OW, OH = 70, 37  # 3 x 2 tiles of widths 32 / 32 / 6 and heights 32 / 5
OFIFO = tile_fifo(OW, OH)
ONE = [(33, 17, 5, 3)]
SW = SH = 64
SFIFO = tile_fifo(SW, SH)
TOP = 2 ** 32 - 1


def params(dev, w, h, spp, sample_base=12345):
    """The film substitutes its own sample index: the context's is a decoy."""
    dev.set_params(w, h, spp, 4, 1, SEED, sample_base=sample_base)


@pytest.fixture(scope="module")
def ctx():
    """One context on C1 and the independent renders of single passes,
    (w, h, spp, base) -> image, rendered once each and shared read-only."""
    sc = Scene.from_dump(golden("c1_default_64x64.scene.ptd"))
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    cache = {}

    def image(w, h, spp, base):
        if (w, h, spp, base) not in cache:
            params(dev, w, h, spp, sample_base=base)
            img = np.zeros((h, w, 3), np.float32)
            dev.render_tiles(tile_fifo(w, h), img)
            assert np.isfinite(img).all() and img.mean() > 0
            img.setflags(write=False)
            cache[(w, h, spp, base)] = img
        return cache[(w, h, spp, base)]

    yield dev, image
    dev.close()


def run_plan(dev, w, h, plan, film=None):
    """plan: (spp, tiles) per pass, on a new film unless one is given."""
    film = film or dev.film(w, h)
    for spp, tiles in plan:
        params(dev, w, h, spp)
        film.add_pass(tiles)
    return film


def restate(image, w, h, plan) -> FilmRestatement:
    """The restatement of the same plan from the independent renders."""
    r = FilmRestatement(w, h)
    base = 0
    for spp, tiles in plan:
        r.add_pass(image(w, h, spp, base), spp, tile_mask(w, h, tiles))
        base += spp
    return r


def to_device(rec: np.ndarray):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def to_host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def test_export_bit_exact(ctx):
    import torch
    dev, image = ctx
    plan = [(2, OFIFO[:4]), (3, OFIFO[::2]), (1, ONE)]  # tile 5 is never covered
    film = run_plan(dev, OW, OH, plan)
    r = restate(image, OW, OH, plan)
    rec = film.export()
    assert rec.shape == (2, OH, OW, 4) and rec.dtype == np.uint32
    assert np.array_equal(rec, records(r))
    assert (rec[1, ..., 3] == 0).all() and (rec[0, ..., 3] == r.n).all() and (rec[1, ..., 2] == r.k).all()
    assert set(np.unique(r.n)) == {0, 2, 3, 5} and (r.n[tile_mask(OW, OH, OFIFO[5:])] == 0).all()
    buf = torch.full((2, OH, OW, 4), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ts = torch.cuda.Stream(device=0)
    film.export_device(buf.data_ptr(), ts.cuda_stream)
    ts.synchronize()
    assert np.array_equal(to_host(buf), rec)
    assert film.merge_info() == {"merged": 0, "taken": 0, "empty": 0, "refused": 0, "merge_ms": 0.0}
    film.close()


def test_merge_bit_exact_all_four_classes(ctx):
    dev, image = ctx
    plan_a = [(2, OFIFO[:4]), (2, OFIFO[::2])]  # tiles 0 .. 4
    plan_b = [(3, OFIFO[2:]), (3, [(20, 3, 30, 30)])]  # tiles 2 .. 5 and a rectangle over 0, 1, 3, 4
    a, a2, b = (run_plan(dev, OW, OH, p) for p in (plan_a, plan_a, plan_b))
    ra, rb = restate(image, OW, OH, plan_a), restate(image, OW, OH, plan_b)
    rec_a, rec_b = a.export(), b.export()
    assert np.array_equal(rec_a, records(ra)) and np.array_equal(rec_b, records(rb))
    # B's records as they go in: three pixels both films hold get n = 2^32 - 1, and a pad to carry
    incoming = rec_b.copy()
    for (y, x) in ((5, 40), (20, 69), (36, 33)):
        assert rec_a[0, y, x, 3] > 0 and rec_b[0, y, x, 3] > 0
        incoming[0, y, x, 3] = TOP
    incoming[1, ..., 3] = np.arange(OW * OH, dtype=np.uint32).reshape(OH, OW) + 1
    cls = classes(ra, from_records(incoming))
    assert all(cls[name].any() for name in CLASSES) and cls["refused"].sum() == 3
    want, counts = merge_records(rec_a, incoming)
    dev_in = to_device(incoming)
    a.merge_device(dev_in.data_ptr())
    got = a.export()
    assert np.array_equal(got, want)
    info = a.merge_info()
    assert {name: info[name] for name in CLASSES} == counts and sum(counts.values()) == OW * OH
    assert info["merge_ms"] > 0
    # merged pixels keep A's pad (0), taken ones carry B's
    assert (got[1, ..., 3][cls["taken"]] == incoming[1, ..., 3][cls["taken"]]).all()
    assert (got[1, ..., 3][~cls["taken"]] == 0).all()
    # B and the incoming buffer are unchanged, A's counters too
    assert np.array_equal(b.export(), rec_b) and np.array_equal(to_host(dev_in), incoming)
    ia = a.info()
    assert (ia["passes"], ia["next_sample"]) == (2, 4)
    # the same from host records
    a2.merge(incoming)
    assert np.array_equal(a2.export(), want)
    assert {name: a2.merge_info()[name] for name in CLASSES} == counts
    with pytest.raises(ValueError):
        a2.merge(incoming[:, :-1])
    for f in (a, a2, b):
        f.close()


def one_film(dev, tiles, passes, spp):
    params(dev, SW, SH, spp)
    film = dev.film(SW, SH)
    for _ in range(passes):
        film.add_pass(tiles)
    return film


@pytest.mark.parametrize("world,edge", [(2, 32), (3, 16)])
def test_tile_split_is_exact(ctx, world, edge):
    dev, _ = ctx
    tiles, K, spp = tile_fifo(SW, SH, edge), 3, 2
    whole = one_film(dev, tiles, K, spp)
    params(dev, SW, SH, spp)
    films = [dev.film(SW, SH) for _ in range(world)]
    shares = [film_passes_tile_split(f, tiles, K, r, world, spp=spp) for r, f in enumerate(films)]
    assert sorted(sum(shares, [])) == sorted(tiles) and all(shares)
    total = {name: 0 for name in CLASSES}
    for f in films[1:]:
        films[0].merge(f.export())
        mi = films[0].merge_info()
        assert mi["merged"] == 0 and mi["refused"] == 0 and mi["taken"] == sum(w * h for _, _, w, h in shares[films.index(f)])
        total["taken"] += mi["taken"]
    assert total["taken"] == SW * SH - sum(w * h for _, _, w, h in shares[0])
    assert np.array_equal(films[0].export(), whole.export())
    got, want = films[0].resolve(), whole.resolve()
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    assert np.array_equal(bits(got[2]), bits(want[2])) and want[0].mean() > 0
    for f in films + [whole]:
        f.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sample_split(ctx, world):
    dev, _ = ctx
    K, spp = 4, 2
    one = one_film(dev, SFIFO, world * K, spp)
    params(dev, SW, SH, spp)
    films = [dev.film(SW, SH) for _ in range(world)]
    ranges = [film_passes_sample_split(f, SFIFO, K, spp, r, world) for r, f in enumerate(films)]
    assert ranges == [(r * K * spp, (r + 1) * K * spp) for r in range(world)]
    recs = [f.export() for f in films]
    bufs = [to_device(r) for r in recs[1:]]
    want = recs[0]
    for r, buf in zip(recs[1:], bufs):  # rank order
        films[0].merge_device(buf.data_ptr())
        want, counts = merge_records(want, r)
        assert counts == {"merged": SW * SH, "taken": 0, "empty": 0, "refused": 0}
    got = films[0].export()
    assert np.array_equal(got, want)
    rec_one = one.export()
    assert np.array_equal(got[0, ..., 3], rec_one[0, ..., 3]) and (got[0, ..., 3] == world * K * spp).all()
    assert np.array_equal(got[1, ..., 2], rec_one[1, ..., 2]) and (got[1, ..., 2] == world * K).all()
    hdr, hdr_one = films[0].resolve(err=False)[0].astype(np.float64), one.resolve(err=False)[0].astype(np.float64)
    bound = (2 * world * K + 2) * 2.0 ** -24 * hdr_one
    worst = (np.abs(hdr - hdr_one)[bound > 0] / bound[bound > 0]).max()
    print(f"sample split N {world}: largest |hdr_merge - hdr_one| is {worst:.3f} of its bound")
    assert (np.abs(hdr - hdr_one) <= bound).all() and hdr_one.mean() > 0
    for f in films + [one]:
        f.close()


def test_checkpoint_resumes_bit_for_bit(ctx, tmp_path):
    dev, _ = ctx
    K, spp = 3, 2
    whole = one_film(dev, SFIFO, 2 * K, spp)
    film = one_film(dev, SFIFO[:3], K, spp)  # (one tile never rendered: its records are zero in the file too)
    rest = one_film(dev, SFIFO[:3], 2 * K, spp)
    path = str(tmp_path / "film.npz")
    film.save(path)
    saved = film.export()
    film.close()
    with np.load(path) as z:
        assert sorted(z.files) == ["height", "next_sample", "records", "width"]
        assert (int(z["width"]), int(z["height"]), int(z["next_sample"])) == (SW, SH, K * spp)
        assert np.array_equal(z["records"], saved)
    back = Film.load(dev, path)
    assert (back.width, back.height) == (SW, SH) and back.info()["next_sample"] == K * spp
    mi = back.merge_info()
    assert mi["taken"] == 3 * 32 * 32 and mi["empty"] == 32 * 32 and mi["merged"] == 0
    assert np.array_equal(back.export(), saved)
    params(dev, SW, SH, spp)
    for _ in range(K):
        back.add_pass(SFIFO[:3])
    assert np.array_equal(back.export(), rest.export())
    done = tile_mask(SW, SH, SFIFO[:3])
    assert np.array_equal(back.export()[:, done], whole.export()[:, done])
    for f in (back, rest, whole):
        f.close()


def test_refusals_leave_the_film_unchanged(ctx):
    import torch
    dev, _ = ctx
    L = native.lib()
    film = run_plan(dev, OW, OH, [(2, OFIFO), (1, OFIFO[::2])])
    before = film.export()
    own = ctypes.c_void_p()
    native.check(L.pt_debug_film_records(film.handle, ctypes.byref(own)))
    nbytes = before.nbytes
    other = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ok_ptr = ctypes.c_void_p(other.data_ptr())
    host = np.zeros_like(before)
    for call, what in ((lambda: L.pt_film_merge_device(None, ok_ptr, None), b"pt_film_merge_device: NULL"),
                       (lambda: L.pt_film_merge_device(film.handle, None, None), b"pt_film_merge_device: NULL"),
                       (lambda: L.pt_film_export_device(None, ok_ptr, None), b"pt_film_export_device: NULL"),
                       (lambda: L.pt_film_export_device(film.handle, None, None), b"pt_film_export_device: NULL"),
                       (lambda: L.pt_film_merge(None, host.ctypes.data), b"pt_film_merge: NULL"),
                       (lambda: L.pt_film_merge(film.handle, None), b"pt_film_merge: NULL"),
                       (lambda: L.pt_film_export(None, host.ctypes.data), b"pt_film_export: NULL"),
                       (lambda: L.pt_film_export(film.handle, None), b"pt_film_export: NULL"),
                       (lambda: L.pt_film_get_merge_info(film.handle, None), b"pt_film_get_merge_info: NULL"),
                       (lambda: L.pt_debug_film_records(None, ctypes.byref(own)), b"pt_debug_film_records: NULL")):
        assert call() == native.PT_E_INVALID and what in L.pt_last_error()
    # a buffer that shares its last / its first record with the film's own, and the film's own
    for off in (16 - nbytes, nbytes - 16, 0):
        ptr = ctypes.c_void_p(own.value + off)
        assert L.pt_film_merge_device(film.handle, ptr, None) == native.PT_E_INVALID
        assert b"overlap" in L.pt_last_error()
        assert L.pt_film_export_device(film.handle, ptr, None) == native.PT_E_INVALID
        assert b"overlap" in L.pt_last_error()
    assert np.array_equal(film.export(), before) and film.merge_info()["merge_ms"] == 0.0
    film.close()
    # n = 2^32 - 1: taken into a clear film as it is, refused the second time
    rng = np.random.default_rng(11)
    syn = np.zeros((2, OH, OW, 4), np.uint32)
    full = rng.random((OH, OW)) < 0.6
    syn[0, ..., :3][full] = rng.random((int(full.sum()), 3), np.float32).view(np.uint32)
    syn[0, ..., 3][full] = TOP
    syn[1, ..., :2][full] = rng.random((int(full.sum()), 2), np.float32).view(np.uint32)
    syn[1, ..., 2][full] = 9
    syn[1, ..., 3][full] = 0xDEADBEEF
    clear = dev.film(OW, OH)
    clear.merge(syn)
    n_full = int(full.sum())
    assert clear.merge_info()["taken"] == n_full and clear.merge_info()["empty"] == OW * OH - n_full
    assert np.array_equal(clear.export(), syn)
    clear.merge(syn)
    mi = clear.merge_info()
    assert (mi["refused"], mi["empty"], mi["merged"], mi["taken"]) == (n_full, OW * OH - n_full, 0, 0)
    assert np.array_equal(clear.export(), syn)
    clear.close()


def test_merge_and_export_stream_order(ctx):
    """A pass on one stream, then the merge and the export on another, with no
    host wait between (the film was cleared on the context's stream): the
    library orders the three."""
    import torch
    dev, _ = ctx
    other = run_plan(dev, OW, OH, [(3, OFIFO[1:])])
    rec_b = other.export()
    other.close()
    serial = run_plan(dev, OW, OH, [(2, OFIFO[:5])])
    serial.merge(rec_b)
    want = serial.export()
    serial.close()
    dev_b = to_device(rec_b)
    out = torch.full((2, OH, OW, 4), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    film = dev.film(OW, OH)
    params(dev, OW, OH, 2)
    film.add_pass(OFIFO[:5], stream=s1.cuda_stream)
    film.merge_device(dev_b.data_ptr(), stream=s2.cuda_stream)
    film.export_device(out.data_ptr(), stream=s2.cuda_stream)
    s2.synchronize()
    assert np.array_equal(to_host(out), want)
    assert np.array_equal(film.export(), want)
    film.close()


KINDS = [k for k, _ in native.pt_resource_counts._fields_]


def live():
    gc.collect()
    n = native.pt_resource_counts()
    assert native.lib().pt_debug_live_resources(ctypes.byref(n)) == native.PT_OK
    return {k: getattr(n, k) for k in KINDS}


@pytest.mark.parametrize("by_context", [False, True])
def test_merge_buffers_go_with_the_film(by_context):
    """The staging buffer, the counts and the merge's two timing events are
    the film's, allocated at the first merge: pt_film_destroy frees them, and
    so does pt_destroy with the film alive."""
    import torch
    sc = Scene.from_dump(golden("c1_default_64x64.scene.ptd"))
    before = live()
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    film = run_plan(dev, SW, SH, [(1, SFIFO)])
    idle = live()
    rec = film.export()
    assert live() == idle  # the export needs nothing of its own
    buf = torch.zeros((2, SH, SW, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    film.export_device(buf.data_ptr())
    film.merge_device(buf.data_ptr())
    dev_only = live()
    assert dev_only["device_arrays"] == idle["device_arrays"] + 1 and dev_only["events"] == idle["events"] + 2
    film.merge(rec)
    both = live()
    assert both["device_arrays"] == dev_only["device_arrays"] + 1
    assert both["device_bytes"] == dev_only["device_bytes"] + rec.nbytes and both["events"] == dev_only["events"]
    assert film.merge_info()["merged"] == SW * SH and (film.export()[0, ..., 3] == 3).all()
    if by_context:
        film.handle = None  # (the wrapper would destroy it first: pt_destroy is to free it)
        dev._films.remove(film)
    else:
        film.close()
        assert live()["device_bytes"] < idle["device_bytes"]
    dev.close()
    assert live() == before


def test_rccl_one_rank_film_exchange(ctx):
    """FilmExchange as every rank of an N-GPU run issues it, on one rank: the
    export queued behind the pass on a dedicated current stream, the gather
    through RCCL, the merge behind it -- no host wait between."""
    import os
    import socket

    import torch
    import torch.distributed as dist

    dev, _ = ctx
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        assert dist.get_backend() == "nccl"
        ex = FilmExchange(SW, SH, 0, 1, torch.device("cuda", 0))
        src, dst = dev.film(SW, SH), dev.film(SW, SH)
        calls = []
        ex.merge_to_root(lambda b: calls.append("export"), lambda b: calls.append("merge"))
        assert calls == []  # one rank: its film is the joined film
        params(dev, SW, SH, 2)
        src.add_pass(SFIFO, stream=stream.cuda_stream)
        src.add_pass(SFIFO[:2], stream=stream.cuda_stream)
        recv = ex.gather(lambda b: src.export_device(b.data_ptr(), stream.cuda_stream))
        dst.merge_device(recv[0].data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        want = src.export()
        assert np.array_equal(dst.export(), want) and np.array_equal(to_host(recv[0]), want)
        assert set(np.unique(want[0, ..., 3])) == {2, 4} and dst.merge_info()["taken"] == SW * SH
        src.close()
        dst.close()
    finally:
        dist.destroy_process_group()
        torch.cuda.set_stream(torch.cuda.default_stream(0))
