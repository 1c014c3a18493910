"""Reprojection without a GPU: the argument checks of the C ABI
(pt_reproject_params_default, pt_reproject_device, pt_film_reproject,
pt_film_get_reproject_info), the pure host parts (csrc/reproject_host.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone driver
(tests/reproject/host_driver.cpp), and the properties that make the numpy
restatement (tests/reproject_helpers.py) a reprojection at all -- the GPU
tests compare the device with it bit for bit, so what it computes is checked
here."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from tests import reproject_helpers as rh
from tests.film_helpers import FilmRestatement, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsgpuraytracing_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
F = np.float32
COS_SET = (F(0.8), F(0.9), F(0.95))
SIGMA_SET = (F(0.005), F(0.01), F(0.02), F(0.05))
PRM = dict(normal_cos_min=0.9, sigma_p=0.02)
SKEW = [1, 0, 0, 1e-6, 1, 0, 0, 0, 1]  # columns 0 and 1 are 1e-6 from orthogonal


def defaults():
    p = native.pt_reproject_params()
    assert native.lib().pt_reproject_params_default(ctypes.byref(p)) == native.PT_OK
    return p


def test_default_params():
    L = native.lib()
    p = defaults()
    assert F(p.normal_cos_min) in COS_SET and F(p.sigma_p) in SIGMA_SET and p.max_samples == 0
    assert L.pt_reproject_params_default(None) == native.PT_E_INVALID
    assert b"pt_reproject_params_default" in L.pt_last_error()
    assert ctypes.sizeof(native.pt_reproject_params) == 12 and ctypes.sizeof(native.pt_reproject_info) == 24


def test_invalid_arguments():
    L = native.lib()
    buf = (ctypes.c_uint32 * 64)()
    ptr = ctypes.addressof(buf)  # (never dereferenced: every call below is refused first)
    cam = rh.make_camera((0, 0, 0), np.eye(3))
    types = (ctypes.c_int32 * 2)(0, 4)

    def call(p=None, ctx=None, cam=cam, rec=ptr, fo=ptr, fn=ptr, w=1, h=1, types=types, n=2, out=ptr + 32):
        return L.pt_reproject_device(ctx, None if cam is None else ctypes.byref(cam), rec, fo, fn, w, h, types, n,
                                     None if p is None else ctypes.byref(p), out, None, None)

    bad = [("normal_cos_min", 1.5, b"normal_cos_min"), ("normal_cos_min", -1.01, b"normal_cos_min"),
           ("normal_cos_min", float("nan"), b"normal_cos_min"), ("sigma_p", 0.0, b"sigma_p"),
           ("sigma_p", -0.1, b"sigma_p"), ("sigma_p", float("nan"), b"sigma_p")]
    for field, value, word in bad:
        p = defaults()
        setattr(p, field, value)
        assert call(p) == native.PT_E_INVALID
        msg = L.pt_last_error()
        assert b"pt_reproject_device" in msg and word in msg, (field, msg)
        # a film is needed before the parameters are looked at
        assert L.pt_film_reproject(None, ctypes.byref(p), None) == native.PT_E_INVALID
    # the ends of the ranges are valid: the refusal is the NULL context's
    for field, value in (("normal_cos_min", -1.0), ("normal_cos_min", 1.0), ("sigma_p", 1e-30), ("max_samples", 2**32 - 1)):
        p = defaults()
        setattr(p, field, value)
        assert call(p) == native.PT_E_INVALID and b"NULL context" in L.pt_last_error(), field
    # NULL pointers
    for kw in (dict(cam=None), dict(rec=None), dict(fo=None), dict(fn=None), dict(out=None)):
        assert call(**kw) == native.PT_E_INVALID and b"NULL argument" in L.pt_last_error(), kw
    # sizes
    for w, h in ((0, 1), (1, 0), (-3, 4), (65536, 1), (40000, 40000)):
        assert call(w=w, h=h) == native.PT_E_INVALID and b"width and height" in L.pt_last_error()
    # overlap: 2 * W * H * 16 bytes each
    for w, h, off in ((1, 1, 0), (1, 1, 16), (1, 1, -16), (2, 1, 48), (2, 2, -112)):
        assert call(w=w, h=h, out=ptr + 128 + off, rec=ptr + 128) == native.PT_E_INVALID
        assert b"overlap" in L.pt_last_error(), (w, h, off)
    assert call(w=1, h=1, rec=ptr, out=ptr + 32) == native.PT_E_INVALID and b"NULL context" in L.pt_last_error()
    # the old camera
    for c2w in (SKEW, [2, 0, 0, 0, 1, 0, 0, 0, 1], [float("nan")] + [0] * 8, [0] * 9):
        assert call(cam=rh.make_camera((0, 0, 0), c2w)) == native.PT_E_INVALID
        assert b"orthonormal" in L.pt_last_error() and b"dot products" in L.pt_last_error()
    assert call(n=-1) == native.PT_E_INVALID and b"n_bsdfs" in L.pt_last_error()
    # NULL film
    assert L.pt_film_reproject(None, None, None) == native.PT_E_INVALID and b"NULL film" in L.pt_last_error()
    info = native.pt_reproject_info()
    assert L.pt_film_get_reproject_info(None, ctypes.byref(info)) == native.PT_E_INVALID
    assert b"pt_film_get_reproject_info" in L.pt_last_error()


# ---- the pure host parts, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("reproject") / "host_driver")
    srcs = [os.path.join(ROOT, "tests", "reproject", "host_driver.cpp"), os.path.join(CSRC, "reproject_host.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + SAN + [f"-I{ROOT}/include", f"-I{CSRC}"] + srcs +
                       ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env, timeout=60)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = [json.loads(ln) for ln in p.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def _cam_line(pos, c2w, sw, sh, sd):
    return "cam " + " ".join(repr(float(v)) for v in list(pos) + list(np.asarray(c2w, np.float64).reshape(9)) + [sw, sh, sd])


def test_host_parts_sanitized(driver):
    a = np.deg2rad(33.0)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cams = [((0.1, -0.2, 1 / 3), rot, 0.7, 0.9, 1.3, 1), ((1e40, 0, 0), np.eye(3), 1, 1, 3, 1),
            ((0, 0, 0), SKEW, 1, 1, 1, 0), ((0, 0, 0), np.eye(3) * (1 + 1e-8), 1, 1, 1, 0),
            ((0, 0, 0), np.eye(3) * (1 + 1e-10), 1, 1, 1, 1), ((0, 0, 0), [float("nan")] * 9, 1, 1, 1, 0),
            ((0, 0, 0), [float("inf")] + [0] * 8, 1, 1, 1, 0)]
    out = driver([_cam_line(*c[:5]) for c in cams])
    for (pos, c2w, sw, sh, sd, ortho), o in zip(cams, out):
        assert o["ortho"] == ortho, (c2w, o)
        with np.errstate(all="ignore"):
            f = rh.camera_f32(rh.make_camera(pos, c2w, sw, sh, sd))
            want = np.concatenate([f["pos"], f["c0"], f["c1"], f["c2"], [f["ax"], f["ay"]]]).astype(F)
        assert o["f32"] == bits(want).tolist()
    prm = [("0.9 0.02 0", ""), ("-1 1e-30 4294967295", ""), ("1 inf 7", ""), ("1.0001 0.02 0", "normal_cos_min"),
           ("nan 0.02 0", "normal_cos_min"), ("0.9 0 0", "sigma_p"), ("0.9 -1 0", "sigma_p"), ("0.9 nan 0", "sigma_p")]
    for (_, word), o in zip(prm, driver(["params " + p for p, _ in prm])):
        assert (o["error"] == "") if not word else (word in o["error"]), o
    types = [0, 1, 2, 3, 4, 0, 4, 7, -1]
    out = driver(["keep %d %s" % (len(types), " ".join(map(str, types))), "keep 0", "default"])
    assert out[0]["keep"] == [1, 0, 0, 0, 1, 1, 1, 0, 0] == rh.keep_table(types).astype(int).tolist()
    assert out[1]["keep"] == []
    p = defaults()
    assert out[2]["params"] == bits(np.array([p.normal_cos_min, p.sigma_p], F)).tolist() + [0]


# ---- properties of the restatement
def plane(cam, w, h, depth=4.0, bsdf=0, normal=(0, 0, 1)):
    return rh.plane_features(cam, w, h, (0.0, 0.0, -depth), normal, lambda p: np.full(p.shape[:-1], bsdf))


def same(a: FilmRestatement, b: FilmRestatement, where=None):
    where = np.ones(a.n.shape, bool) if where is None else where
    return all(np.array_equal(np.ascontiguousarray(getattr(a, k)).view(np.uint32)[where],
                              np.ascontiguousarray(getattr(b, k)).view(np.uint32)[where]) for k in ("sum", "n", "mu", "M2", "k"))


def is_reset(r: FilmRestatement, where):
    return not any(np.ascontiguousarray(getattr(r, k)).view(np.uint32)[where].any() for k in ("sum", "n", "mu", "M2", "k"))


def test_same_camera_is_the_identity_on_kept_hits():
    w, h = 37, 23
    rng = np.random.default_rng(1)
    a = np.deg2rad(20.0)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cam = rh.make_camera((0.3, -0.2, 5.0), rot, 1.2, 0.8, 1.1)
    types = list(rh.CASE_TYPES)
    feat = rh.plane_features(cam, w, h, (0.3, 0.0, -1.0), (0.3, -0.2, 1.0), lambda p: np.floor(p[..., 0] * 2 + 40).astype(int) % len(types))
    feat[:, :3, :5] = rh.feature_records(5, 3, 0, -1, 0, 0)  # a miss corner
    r = rh.random_film(w, h, rng, empty=0.0)
    out, kept = rh.reproject(r, feat, feat, cam, types, **PRM)
    bsdf = feat[0].view(np.int32)[..., 3]
    want = (bsdf >= 0) & np.isin(np.array(types + [-1])[bsdf], rh.KEPT_TYPES)
    assert want.any() and (~want).any() and (bsdf < 0).any()
    assert np.array_equal(kept, want)
    assert same(out, r, want) and is_reset(out, ~want)
    # an empty record is not history: the pixel counts as reset
    r.n[5, 7] = 0
    assert want[5, 7]
    _, kept2 = rh.reproject(r, feat, feat, cam, types, **PRM)
    assert not kept2[5, 7] and kept2.sum() == kept.sum() - 1


def test_sideways_shift_moves_the_records_by_whole_columns():
    w, h, depth = 32, 9, 4.0
    rng = np.random.default_rng(2)
    cam = rh.make_camera((0, 0, 0), np.eye(3))
    r = rh.random_film(w, h, rng, empty=0.0)
    fo = plane(cam, w, h, depth)
    px = depth * 1.0 / w  # a pixel's width on the plane: 0.125, exact
    for j in (1, 3, 31, -2):
        new = rh.moved(cam, j * px)
        fn = plane(new, w, h, depth)
        out, kept = rh.reproject(r, fo, fn, cam, [native.BSDF_DIFFUSE], **PRM)
        src = np.arange(w) + j  # the new pixel x sees what the old pixel x + j saw
        cover = (src >= 0) & (src < w)
        assert np.array_equal(kept, np.tile(cover, (h, 1))), j
        shifted = FilmRestatement(w, h)
        for k in ("sum", "n", "mu", "M2", "k"):
            getattr(shifted, k)[:, cover] = getattr(r, k)[:, src[cover]]
        assert same(out, shifted), j  # bit for bit, and the uncovered strip is reset
        assert is_reset(out, np.tile(~cover, (h, 1)))
    # the same along y
    new = rh.moved(cam, 2 * (depth / h), along=1)
    out, kept = rh.reproject(r, fo, plane(new, w, h, depth), cam, [native.BSDF_DIFFUSE], **PRM)
    assert kept[:h - 2].all() and not kept[h - 2:].any()
    assert np.array_equal(out.n[:h - 2], r.n[2:]) and np.array_equal(bits(out.M2[:h - 2]), bits(r.M2[2:]))


def test_an_occluder_in_the_old_view_resets_what_it_hid():
    w, h = 24, 16
    cam = rh.make_camera((0, 0, 0), np.eye(3))
    r = rh.random_film(w, h, np.random.default_rng(3), empty=0.0)
    far, near = plane(cam, w, h, 4.0), plane(cam, w, h, 3.0)
    hid = np.zeros((h, w), bool)
    hid[4:9, 10:17] = True
    fo = np.where(hid[None, :, :, None], near, far)
    out, kept = rh.reproject(r, fo, far, cam, [native.BSDF_DIFFUSE], **PRM)
    assert np.array_equal(kept, ~hid) and is_reset(out, hid) and same(out, r, ~hid)
    # and the other way round: what the new view's occluder covers has no history behind it
    out, kept = rh.reproject(r, far, fo, cam, [native.BSDF_DIFFUSE], **PRM)
    assert not kept[hid].any()
    # a plane distance within sigma_p * z is the same surface
    close = plane(cam, w, h, 4.0 * (1 + 0.5 * PRM["sigma_p"]))
    _, kept = rh.reproject(r, close, far, cam, [native.BSDF_DIFFUSE], **PRM)
    assert kept.all()
    # a turned normal is another surface
    tilt = plane(cam, w, h, 4.0)
    tilt[0, hid, :3] = np.array([np.sin(0.6), 0, np.cos(0.6)], F)  # cos 0.825 < 0.9
    _, kept = rh.reproject(r, tilt, far, cam, [native.BSDF_DIFFUSE], **PRM)
    assert np.array_equal(kept, ~hid)
    _, kept = rh.reproject(r, tilt, far, cam, [native.BSDF_DIFFUSE], normal_cos_min=0.8, sigma_p=0.02)
    assert kept.all()


def test_view_dependent_bsdfs_always_reset():
    w, h = 12, 7
    cam = rh.make_camera((0, 0, 0), np.eye(3))
    r = rh.random_film(w, h, np.random.default_rng(4), empty=0.0)
    feat = plane(cam, w, h)
    for t, keeps in ((native.BSDF_DIFFUSE, True), (native.BSDF_EMISSION, True), (native.BSDF_MIRROR, False),
                     (native.BSDF_REFRACTION, False), (native.BSDF_GLASS, False)):
        out, kept = rh.reproject(r, feat, feat, cam, [t], **PRM)
        assert kept.all() if keeps else (not kept.any() and is_reset(out, ~kept)), t
    # an index beyond the table, and an empty table
    _, kept = rh.reproject(r, plane(cam, w, h, bsdf=1), plane(cam, w, h, bsdf=1), cam, [native.BSDF_DIFFUSE], **PRM)
    assert not kept.any()
    _, kept = rh.reproject(r, feat, feat, cam, [], **PRM)
    assert not kept.any()


def test_cap_arithmetic():
    w, h, cap = 16, 8, 5
    cam = rh.make_camera((0, 0, 0), np.eye(3))
    r = rh.random_film(w, h, np.random.default_rng(5), n_max=40, empty=0.0)
    r.n[0, 0], r.k[0, 0] = 40, 1          # k * n' / n rounds down to 0: k' = 1
    r.n[0, 1], r.k[0, 1] = cap, cap       # at the cap: untouched
    r.n[0, 2], r.k[0, 2] = cap + 1, cap + 1
    r.n[0, 3], r.k[0, 3] = 2**32 - 1, 2**32 - 1  # the product needs 64 bits
    feat = plane(cam, w, h)
    free, _ = rh.reproject(r, feat, feat, cam, [native.BSDF_DIFFUSE], **PRM)
    assert same(free, r)
    out, kept = rh.reproject(r, feat, feat, cam, [native.BSDF_DIFFUSE], max_samples=cap, **PRM)
    assert kept.all()
    over = r.n > cap
    assert over.any() and (~over).any()
    assert same(out, r, ~over)
    assert (out.n[over] == cap).all() and (out.k >= 1).all()
    want_k = np.maximum(1, (r.k[over].astype(object) * cap) // r.n[over].astype(object))
    assert out.k[over].tolist() == want_k.tolist()
    assert out.k[0, 0] == 1 and out.k[0, 2] == cap and out.k[0, 3] == cap
    assert np.array_equal(bits(out.mu), bits(r.mu))
    # the mean and the per-pass variance M2 / n survive up to rounding
    mean0 = r.sum[over].astype(np.float64) / r.n[over][:, None]
    mean1 = out.sum[over].astype(np.float64) / out.n[over][:, None]
    assert np.allclose(mean1, mean0, rtol=4e-7, atol=0)
    var0 = r.M2[over].astype(np.float64) / r.n[over]
    var1 = out.M2[over].astype(np.float64) / out.n[over]
    assert np.allclose(var1, var0, rtol=4e-7, atol=0)
    # and the error estimate does not shrink: fewer passes on the same spread
    keep2 = over & (r.k >= 2) & (out.k >= 2)
    assert keep2.any() and (out.err()[keep2] >= r.err()[keep2] * F(0.999)).all()


def test_synthetic_case_takes_every_branch():
    """What tests/test_gpu_reproject.py compares the device on."""
    w, h = 70, 37
    r, fo, fn, old, types = rh.synthetic_case(w, h, 7)
    out, kept = rh.reproject(r, fo, fn, old, types, **PRM)
    assert 0.15 < kept.mean() < 0.9
    bn = fn[0].view(np.int32)[..., 3]
    assert np.isnan(fn[1]).any() and (bn >= len(types)).any() and (bn < 0).any() and (r.n == 0).any()
    assert not kept[np.isnan(fn[1]).any(-1)].any() and not kept[(bn < 0) | (bn >= len(types))].any()
    assert not kept[~np.isin(np.array(types)[np.clip(bn, 0, len(types) - 1)], rh.KEPT_TYPES)].any()
    c = rh.camera_f32(old)
    # seeded exactly on the old frame's far edges: refused; on its near edges: in the frame
    for pt, inside in (((2.0, 1.0, -4.0), False), ((1.0, 2.0, -4.0), False), ((-2.0, 1.0, -4.0), True), ((1.0, -2.0, -4.0), True)):
        at = (fn[1][..., :3] == np.array(pt, F)).all(-1)
        assert at.any()
        u = (F(pt[0]) / F(4) / c["ax"] + F(0.5)) * F(w)
        t = (F(pt[1]) / F(4) / c["ay"] + F(0.5)) * F(h)
        assert (u == w or t == h) if not inside else (u == 0 or t == 0)
        assert not kept[at].any() if not inside else True
    assert (fn[1][..., 2] > 0).any()
    capped, kept5 = rh.reproject(r, fo, fn, old, types, max_samples=5, **PRM)
    assert np.array_equal(kept5, kept) and (capped.n[kept] <= 5).all() and (out.n[kept] > 5).any()
    assert is_reset(out, ~kept) and is_reset(capped, ~kept)
