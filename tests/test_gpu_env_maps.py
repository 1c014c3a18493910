"""The environment light on the hard maps of tests/env_maps.py: the device's own
answers (pt_debug_env_probe runs the render kernel's record_lower_bound,
env_sample, env_uv and env_dir, one lane per query) against the float64
reference, and renders of the 25-primitive room against the restatement.
tests/test_env_maps_host.py proves on the CPU that the maps, queries and
directions reach what they aim at, and computes delta32, the float32 floor of
the lookup that the radiance tolerance here is built from.

Probe, every family: indices and interpolation pairs bit for bit; (tu, tv)
within 8 units of float32 rounding at max(w, h) of the float64 evaluation;
wi, and pdf through the sin(theta) it implies (table / (pdf * texel solid
angle factor): the estimator is radiance * sin(theta) * const / table, so the
absolute error of the fast __sincosf is what a render sees), within 16 times
the error of the numpy-float32 evaluation of the same expressions; radiance
within 4 * delta32 * (Dh + Dv) + 1e-6 * max|texel|, a tolerance that follows
the local contrast.

Measured on an MI355X (the tests print every figure):

  search          row, column, prev, cur identical on every query of every family
                  (65,536 uniform + 1 .. 4,095 targeted pairs per family)
  tu, tv          largest difference 1.2e-4 texel on `wide` (tolerance 1.0e-3),
                  6.1e-5 on black_row0 (4.9e-4), 3.8e-6 on black_half (4.6e-5),
                  1.9e-6 on the sun maps (3.1e-5), 2.7e-7 on tiny (3.3e-6)
  wi              4.4e-7 .. 8.2e-7 absolute; numpy float32 4.2e-7 .. 8.9e-7
  sin(theta)      2.5e-7 .. 4.5e-7 absolute through the pdf; numpy float32
                  2.1e-7 .. 4.2e-7: __sincosf costs nothing measurable here
  pdf             finite and positive for every u > 0 (before env_sample's
                  floor on sin(theta), u1 = 0.99999994 on sun_poles gave +inf:
                  test_probe_pdf_is_finite_and_positive)
  radiance        error / tolerance at most 9.3e-5 at the drawn coordinates
                  (black_row0) and 0.070 for directions (wide): the env_uv(tu, tv)
                  (with the 4 * delta32 tolerance of the issue; against the
                  coordinate bound the drawn lookups are now held to, at most
                  0.013): the env_uv(tu, tv) departure from the reference's
                  sample_dir(wi) round trip is not measurable, beside a sun too

Per-sample parity, samples within 1e-3 of 6,144 per scene (mean relative
difference): A0_ENV under sun_seam 99.984% (4.5e-6), sun_poles 99.984% (3.2e-6),
black_half 100% (3.6e-6), wide 99.967% (1.2e-6), black_row0 99.967% (1.8e-5),
tiny 100% (1.5e-6), one 100% (4.5e-6); ENV alone under sun_seam 100% (6.7e-7),
black_half 100% (9.0e-7), wide 99.935% (7.6e-8); L8_ENV under black_half 99.967%
(8.3e-6).  Grouped, 5 spp: sun_poles 99.902% of pixels, wide 100%.

Every sample outside the tolerance was traced on both sides (RS_DEBUG_PIXEL and
PT_DEBUG_PIXEL: the draws, pdfs and sun directions agree in all of them):
  * occlusion decided differently at an edge -- A0_ENV sun_seam (1,13) s4 and
    sun_poles (10,8) s4: the AREA light's shadow ray grazes a sphere (one side
    occluded); ENV sun_seam at seed 61, (18,31) s5: the sun's shadow ray passes
    the ceiling's edge within 5e-6 (tests/env_maps.py tells it; the seed moved);
  * a sun at grazing incidence -- A0_ENV wide (7,0) s3: cos 8.1e-4 against
    8.4e-4 on a sphere hit whose fp32 normal differs by 2e-5; 2e-4 absolute;
  * specular chains -- the other ten (wide (24,6) s5; black_row0 (12,4) s5,
    (24,28) s2; ENV wide (7,1) s5, (24,6) s4, (10,9) s5, (25,22) s3; L8_ENV
    black_half (15,0) s4, (26,21) s4; ENV sun_seam seed 61 (10,15) s0): same
    primitives and shadow outcomes, but two to four bounces inside the glass
    sphere or off the mirror spheres stretch fp32's 1e-6 to 1e-4 .. 1e-3 in the
    leaving direction, which these white-noise maps (neighbours differ by up to
    0.2; 334 texels per radian on `wide`) turn into 0.3 .. 2% of the sample, at
    most 1e-5 of a scene's sum.  Not a lookup error: the probe pins both lookups.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.pathtracer import Device
from tests import env_maps as E
from tests import shading_scenes as S
from tests.test_gpu_shading_sweep import _device, assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("env_maps_gpu")


# ------------------------------------------------------------------ the probe
_PROBE = {}


def probe(name):
    """The device's answers to every sample query and lookup direction of a
    family: one upload and one probe call per family, shared by the tests."""
    if name not in _PROBE:
        dev = _device(E.render_scene(("A0_ENV", name)))
        u1, u2 = E.all_queries(name)
        d, _ = E.lookup_dirs(name)
        got = dev.env_probe(u1, u2, d)
        want = E.ref(name).sample(u1, u2)
        for v in list(got.values()) + [v for v in want.values() if isinstance(v, np.ndarray)]:
            v.setflags(write=False)
        _PROBE[name] = (u1, u2, got, want)
    return _PROBE[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_search_is_bit_exact(name):
    u1, u2, got, want = probe(name)
    assert len(u1) >= E.N_UNIFORM + 2
    for k in ("row", "col"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (name, k, bad.size, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    for k in ("row_pair", "col_pair"):
        bad = np.flatnonzero((_bits(got[k]) != _bits(want[k])).any(axis=1))
        assert bad.size == 0, (name, k, bad.size, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_never_returns_a_dark_texel(name):
    u1, u2, got, _ = probe(name)
    R = E.ref(name)
    pos = (u1 > 0) & (u2 > 0)
    mass = np.diff(R.p_phi, axis=1, prepend=np.float32(0))
    assert (mass[got["row"][pos], got["col"][pos]] > 0).all()
    assert (np.diff(R.p_theta, prepend=np.float32(0))[got["row"][pos]] > 0).all()
    assert np.isfinite(got["wi"]).all() and np.isfinite(got["radiance"]).all() and np.isfinite(got["dir_radiance"]).all()


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_pdf_is_finite_and_positive(name):
    """Every pdf returned for u > 0 is finite and positive.

    This test found one that was not: u1 = 0.99999994 (the uniform set's edge
    value) on sun_poles.  Half of that map's mass lies in the last row, so
    y = 31 + (r1 - prev) / (cur - prev) = 31.9999999 rounds to 32.0f, theta =
    min(y / h, 1) * pi is float32 pi = 3.14159274, the fast __sincosf returned
    sin(theta) = 0 and the pdf was +inf, on one query of 69,631 (the reference's
    own formula takes sin((double)theta) = -8.74e-8 of that float theta and
    returns a negative pdf).  env_sample now keeps the sine of a latitude in
    (0, pi] at or above 2^-24."""
    u1, u2, got, _ = probe(name)
    pos = (u1 > 0) & (u2 > 0)
    bad = np.flatnonzero(pos & ~(np.isfinite(got["pdf"]) & (got["pdf"] > 0)))
    print(f"{name}: {bad.size} of {int(pos.sum())} pdfs not finite and positive", u1[bad[:4]], u2[bad[:4]], got["pdf"][bad[:4]])
    assert bad.size == 0, (name, bad[:8], u1[bad[:8]], u2[bad[:8]], got["pdf"][bad[:8]])


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_coordinates(name):
    """tu, tv = t + (r - prev) / (cur - prev) - 0.5 on the same float32 inputs:
    three correctly rounded operations and a min, held to 8 units of float32
    rounding (2^-24 relative) at max(w, h)."""
    _, _, got, want = probe(name)
    R = E.ref(name)
    ok = ~want["degenerate"]  # (u == 0 on a zero-mass first entry: 0 / 0 in the reference; indices only)
    tol = 8 * 2.0 ** -24 * max(R.w, R.h)
    eu = np.abs(got["tu"].astype(np.float64) - want["tu"])[ok].max()
    ev = np.abs(got["tv"].astype(np.float64) - want["tv"])[ok].max()
    print(f"{name}: |tu - ref| <= {eu:.3g}, |tv - ref| <= {ev:.3g} (tolerance {tol:.3g}); {int((~ok).sum())} degenerate")
    assert eu <= tol and ev <= tol


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_direction_and_pdf(name):
    u1, u2, got, want = probe(name)
    R = E.ref(name)
    f32 = R.sample(u1, u2, f32=True)
    ok = ~want["degenerate"]
    k = (2 * np.pi / R.w) * (np.pi / R.h)

    def implied_sin(s):  # table / (pdf * k): what the estimator multiplies the radiance by (0 where pdf is inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            return R.pdf[want["row"], want["col"]].astype(np.float64) / (np.asarray(s["pdf"], np.float64) * k)

    ref_sin = np.sin(want["theta"])
    floor_sin = np.abs(implied_sin(f32) - ref_sin)[ok].max()
    dev_sin = np.abs(implied_sin(got) - ref_sin)[ok].max()
    floor_wi = np.abs(f32["wi"].astype(np.float64) - want["wi"])[ok].max()
    dev_wi = np.abs(got["wi"].astype(np.float64) - want["wi"])[ok].max()
    pos = ok & (u1 > 0) & (u2 > 0)
    with np.errstate(invalid="ignore"):  # (inf - inf where both sides' theta is 0 or pi)
        rel_pdf = (np.abs(got["pdf"].astype(np.float64) - want["pdf"]) / want["pdf"])[pos].max()
    print(f"{name}: wi error {dev_wi:.3g} (numpy float32 {floor_wi:.3g}); implied sin(theta) error {dev_sin:.3g} "
          f"(numpy float32 {floor_sin:.3g}); largest relative pdf error {rel_pdf:.3g}")
    assert dev_wi <= 16 * floor_wi
    assert dev_sin <= 16 * floor_sin


@pytest.mark.parametrize("name", E.FAMILIES)
def test_probe_radiance(name):
    """env_uv at the drawn coordinates and env_dir of every direction against
    the float64 lookup; at the reference's discontinuities (the exact poles,
    d.x = +-0 and +-1e-30) inside what either side would blend.

    Directions are held to the issue's 4 * delta32 * (Dh + Dv): delta32 is the
    float32 acos floor, 0.14 texel on `wide` and 0.07 on black_row0, so on those
    two maps that tolerance is half and a quarter of a texel of contrast wide and
    a swapped pair of wrap texels passes it there (it fails on sun_seam,
    sun_poles, black_half and tiny).  The drawn coordinates have no acos behind
    them: they are held to the bound of test_probe_coordinates instead, 8 units
    of float32 rounding at max(w, h) -- 1e-3 texel on `wide` -- never wider than
    delta32."""
    _, _, got, want = probe(name)
    R = E.ref(name)
    delta = E.delta32(name)
    ok = ~want["degenerate"]
    err = np.abs(got["radiance"].astype(np.float64) - R.lookup(want["tu"], want["tv"])).max(axis=1)
    tol = R.lookup_tolerance(want["tu"], want["tv"], min(delta, 8 * 2.0 ** -24 * max(R.w, R.h)))
    worst_s = (err / tol)[ok].max()
    assert (err <= tol)[ok].all(), (name, "drawn", int((err > tol)[ok].sum()), worst_s)
    d, parts = E.lookup_dirs(name)
    cont = E.continuous(name)
    tu, tv = R.dir_coords(d)
    err = np.abs(got["dir_radiance"].astype(np.float64) - R.lookup(tu, tv)).max(axis=1)
    tol = R.lookup_tolerance(tu, tv, delta)
    worst_d = (err / tol)[cont].max()
    print(f"{name}: radiance error / tolerance at most {worst_s:.3g} (drawn coordinates), {worst_d:.3g} (directions); "
          f"delta32 {delta:.3g}")
    bad = np.flatnonzero((err > tol) & cont)
    assert bad.size == 0, (name, "directions", bad.size, bad[:5], d[bad[:5]], err[bad[:5]], tol[bad[:5]])
    lo, hi = R.blend_bounds(d[~cont])
    slack = 1e-6 * float(R.tex.max())
    g = got["dir_radiance"][~cont].astype(np.float64)
    assert np.isfinite(g).all() and (g >= lo - slack).all() and (g <= hi + slack).all()


def test_probe_refusals_on_a_device():
    """No environment light, no scene: refused before anything is launched."""
    L = native.lib()
    u = np.array([0.5], np.float32)
    dev = _device(S.light_scene("L1"))
    with pytest.raises(native.PtError) as e:
        dev.env_probe(u, u)
    assert e.value.code == native.PT_E_INVALID and "no environment light" in str(e.value)
    fresh = Device(0)
    with pytest.raises(native.PtError) as e:
        fresh.env_probe(u, u)
    assert e.value.code == native.PT_E_NOSCENE
    env = _device(E.render_scene(("A0_ENV", "tiny")))
    with pytest.raises(native.PtError) as e:
        env.env_probe([1.0], [0.5])
    assert e.value.code == native.PT_E_INVALID
    with pytest.raises(native.PtError) as e:
        env.env_probe(dirs=[[0.0, 2.0, 0.0]])
    assert e.value.code == native.PT_E_INVALID
    assert env.env_probe()["row"].size == 0  # nothing asked: nothing launched
    assert L.pt_last_error()


# ------------------------------------------------------------------ renders against the restatement
def _frame(dev, key, spp, sample_base=0, tiles=None):
    _, w, h, m, l, seed = E.scene_args(key)
    dev.set_params(w, h, spp, m, l, seed, sample_base=sample_base)
    img = np.zeros((h, w, 3), np.float32)
    dev.render_tiles([(0, 0, w, h)] if tiles is None else tiles, img)
    return img


def gpu_image(key, spp=4, tiles=None, gpu_bvh=False):
    return _frame(_device(E.render_scene(key), gpu_bvh), key, spp, tiles=tiles)


@pytest.mark.parametrize("key", list(E.RENDER_SCENES), ids=E.scene_id)
def test_per_sample_parity(restate, scene_dir, key):
    _, ref = E.reference(restate, scene_dir, key)
    dev = _device(E.render_scene(key))
    got = np.stack([_frame(dev, key, 1, sample_base=i) for i in range(E.N_SAMPLES)], axis=2)
    assert_parity(got, ref[:, :, :E.N_SAMPLES], f"{E.scene_id(key)} samples")


@pytest.mark.parametrize("group", ["1", "2", "5"])
@pytest.mark.parametrize("fam", ["sun_poles", "wide"])
def test_grouped_parity(restate, scene_dir, monkeypatch, fam, group):
    monkeypatch.setenv("PT_SAMPLE_GROUP", group)
    key = ("A0_ENV", fam)
    _, ref = E.reference(restate, scene_dir, key)
    got = gpu_image(key, spp=E.GROUP_SPP)
    assert_parity(got, S.sum_in_groups(ref[:, :, :E.GROUP_SPP], int(group)), f"{E.scene_id(key)} 5 spp group {group}")


@pytest.mark.parametrize("fam", E.FAMILIES)
def test_one_tile_equals_four_tiles(fam):
    key = ("A0_ENV", fam)
    a = gpu_image(key)
    b = gpu_image(key, tiles=[(0, 0, 16, 16), (16, 0, 16, 16), (0, 16, 16, 16), (16, 16, 16, 16)])
    assert a.any() and np.array_equal(a, b)


GTAB_FAMILIES = ["sun_seam", "wide"]


def _dump_forced(out):
    """(child process) the [A0, ENV] room under the two maps, 4 spp."""
    np.savez(out, **{f: gpu_image(("A0_ENV", f)) for f in GTAB_FAMILIES})


def test_forced_global_tables_are_identical(tmp_path):
    """PT_FORCE_GLOBAL_TABLES is read once per process: a child renders with it."""
    out = str(tmp_path / "gtab.npz")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_env_maps import _dump_forced; " \
           f"_dump_forced({out!r})"
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, PT_FORCE_GLOBAL_TABLES="1"), cwd=ROOT,
                   timeout=120)  # two 32x32 frames of 4 spp: seconds, most of them the child's start
    forced = np.load(out)
    for f in GTAB_FAMILIES:
        a = gpu_image(("A0_ENV", f))
        assert a.any() and np.array_equal(a, forced[f]), f


@pytest.mark.parametrize("build", ["sah", "ref", "lbvh"])
def test_wide_map_on_every_tree(restate, scene_dir, monkeypatch, build):
    if build == "lbvh":
        monkeypatch.delenv("PT_BVH_BUILD", raising=False)
    else:
        monkeypatch.setenv("PT_BVH_BUILD", build)
    key = ("A0_ENV", "wide")
    _, ref = E.reference(restate, scene_dir, key)
    got = gpu_image(key, spp=4, gpu_bvh=build == "lbvh")
    assert_parity(got, S.sum_in_order(ref[:, :, :4]), f"{E.scene_id(key)} on the {build} tree")
