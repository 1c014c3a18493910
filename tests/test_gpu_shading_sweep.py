"""The render kernel's shading round against the restatement, sample by sample,
on the scenes of tests/shading_scenes.py: light lists of 0 .. 12 lights of
every kind, coloured material tables of 16 and 20 BSDFs, ns_area_light = 255
and max_depth = 254 (tests/test_shading_scenes_host.py proves on the CPU that
every light, material and colour channel of these scenes reaches the samples).

Per-sample parity is SURVEY.md §8(c) criterion 2 applied to SAMPLES, each
scene on its own: >= 99.5% of samples within 1e-3 * max(1, |ref|), mean within
0.1%, all finite.  A wrong branch that a pixel average of 4 .. 16 spp hides
is a wrong sample here.

Measured on an MI355X (samples within tolerance, of 6144 per 32x32 scene):
all but L2_area_occluded, L5, L12 (one sample off each, 99.984%) and L3 (two,
99.967%); every one traced to a ray grazing a sphere silhouette or a panel
edge (tests/shading_scenes.py env_middle_scene tells one such trace).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.pathtracer import Device, Scene
from tests import shading_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shading_sweep")


def _device(d, gpu_bvh=False):
    sc = Scene(native.SceneArrays(d))
    dev = Device(0)
    dev.upload_scene(sc, gpu_bvh=gpu_bvh)
    dev.set_camera(sc.camera)
    return dev


def _frame(dev, case, spp, sample_base=0, tiles=None):
    _, w, h, m, l, seed = S.CASES[case]
    dev.set_params(w, h, spp, m, l, seed, sample_base=sample_base)
    img = np.zeros((h, w, 3), np.float32)
    dev.render_tiles([(0, 0, w, h)] if tiles is None else tiles, img)
    return img


def gpu_samples(d, case, n=S.N_SAMPLES):
    """(H, W, n, 3): the kernel's samples 0 .. n-1 of every pixel, one launch
    of spp = 1 with sample_base = i each (as tools/silhouette_samples.py)."""
    dev = _device(d)
    return np.stack([_frame(dev, case, 1, sample_base=i) for i in range(n)], axis=2)


def gpu_image(d, case, spp=4, tiles=None, gpu_bvh=False):
    return _frame(_device(d, gpu_bvh), case, spp, tiles=tiles)


def assert_parity(got, ref, what):
    """SURVEY.md §8(c) criterion 2 over the leading axes (samples or pixels)."""
    frac = S.within(got, ref).mean()
    rel_mean = abs(float(got.mean(dtype=np.float64)) - float(ref.mean(dtype=np.float64))) / \
        max(float(ref.mean(dtype=np.float64)), 1e-12)
    print(f"{what}: {frac * 100:.3f}% within 1e-3, mean rel diff {rel_mean:.2e}")
    assert np.isfinite(got).all(), what
    assert frac >= 0.995, (what, frac)
    assert rel_mean <= 1e-3, (what, rel_mean)


@pytest.mark.parametrize("name", list(S.CASES))
def test_per_sample_parity(restate, scene_dir, name):
    _, ref = S.reference(restate, scene_dir, name)
    got = gpu_samples(S.scene(name), name)
    assert_parity(got, ref[:, :, :S.N_SAMPLES], f"{name} samples")


@pytest.mark.parametrize("group", [None, "1", "2", "4", "5"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_grouped_parity(restate, scene_dir, monkeypatch, name, group):
    """spp = 5 in one launch with work slots of 1, 2 (2 + 2 + 1), 4 (4 + 1, a
    short last group) and 5 (one group) samples.  Inside a group the next
    sample's camera ray waits behind the sample's last shadow ray (SH_FOLLOW
    after `finish`), and a group's one store waits behind it with the next
    group's camera ray parked (SH_STORE, SH_STORE_FOLLOW): no spp = 1 launch
    and no group of one sample does the first.  The default group (None)
    resolves to 1 at these frame sizes (launch_plan.cpp group_size halves it
    until the frame fills the device): it is the issue's case, not a second
    grouping."""
    if group is None:
        monkeypatch.delenv("PT_SAMPLE_GROUP", raising=False)
    else:
        monkeypatch.setenv("PT_SAMPLE_GROUP", group)
    _, ref = S.reference(restate, scene_dir, name)
    got = gpu_image(S.scene(name), name, spp=S.GROUP_SPP)
    want = S.sum_in_groups(ref[:, :, :S.GROUP_SPP], int(group or 1))
    assert_parity(got, want, f"{name} {S.GROUP_SPP} spp group {group}")


# ---------------------------------------------------------------- exact identities
def _pad_table(d, n_extra=1):
    d = dict(d)
    d["bsdf_type"] = np.concatenate([d["bsdf_type"], np.full(n_extra, S.DIFFUSE, np.int32)])
    d["bsdf_params"] = np.concatenate([d["bsdf_params"], np.tile(np.float32([0.5, 0.25, 0.125] + [0] * 9), n_extra)])
    return d


def test_padded_table_is_identical():
    """16 BSDFs (LDS copy) and the same 16 plus one unused entry (17: the
    global-table variant): same arithmetic, same bits."""
    d = S.scene("M16")
    assert len(d["bsdf_type"]) == 16
    a = gpu_image(d, "M16")
    b = gpu_image(_pad_table(d), "M16")
    assert a.any() and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["M16", "M20"])
def test_permuted_table_is_identical(name):
    d = S.scene(name)
    n = len(d["bsdf_type"])
    perm = np.random.default_rng(7).permutation(n)  # new index of old entry i
    assert (perm != np.arange(n)).sum() > n // 2
    p = dict(d)
    inv = np.argsort(perm)
    p["bsdf_type"] = d["bsdf_type"][inv]
    p["bsdf_params"] = d["bsdf_params"].reshape(-1, 12)[inv].reshape(-1)
    p["prim_bsdf"] = perm[d["prim_bsdf"]].astype(np.int32)
    a = gpu_image(d, name)
    b = gpu_image(p, name)
    assert a.any() and np.array_equal(a, b)


SMALL_LISTS = [n for n, v in S.LIGHT_LISTS.items() if 2 <= len(v) <= 8]


def _dump_small_lists(out):
    """(child process) every multi-light scene of <= 8 lights, 4 spp."""
    np.savez(out, **{n: gpu_image(S.scene(n), n) for n in SMALL_LISTS})


def test_forced_global_tables_are_identical(tmp_path):
    """PT_FORCE_GLOBAL_TABLES (read once per process: a child renders with it)
    on every multi-light scene the LDS copy holds."""
    out = str(tmp_path / "gtab.npz")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_shading_sweep import _dump_small_lists; " \
           f"_dump_small_lists({out!r})"
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, PT_FORCE_GLOBAL_TABLES="1"), cwd=ROOT,
                   timeout=120)  # seven 32x32 frames of 4 spp: seconds, most of them the child's start
    forced = np.load(out)
    assert len(SMALL_LISTS) == 7
    for n in SMALL_LISTS:
        a = gpu_image(S.scene(n), n)
        assert a.any() and np.array_equal(a, forced[n]), n


def test_triangle_only_room_is_identical(monkeypatch):
    d = S.material_scene("full16", spheres=False)
    assert (d["prim_type"] == 1).all() and len(d["bsdf_type"]) == 11
    a = gpu_image(d, "M16")
    monkeypatch.setenv("PT_NO_TRI_ONLY", "1")
    b = gpu_image(d, "M16")
    assert a.any() and np.array_equal(a, b)


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c[1] == 32])
def test_one_tile_equals_four_tiles(name):
    d = S.scene(name)
    a = gpu_image(d, name)
    b = gpu_image(d, name, tiles=[(0, 0, 16, 16), (16, 0, 16, 16), (0, 16, 16, 16), (16, 16, 16, 16)])
    assert (a.any() or name == "L0") and np.array_equal(a, b)  # (L0 has no light: two black frames)


# ---------------------------------------------------------------- tree independence
@pytest.mark.parametrize("build", ["sah", "ref", "lbvh"])
@pytest.mark.parametrize("name", ["L5", "L12"])
def test_multi_light_scenes_on_every_tree(restate, scene_dir, monkeypatch, name, build):
    if build == "lbvh":
        monkeypatch.delenv("PT_BVH_BUILD", raising=False)
    else:
        monkeypatch.setenv("PT_BVH_BUILD", build)
    _, ref = S.reference(restate, scene_dir, name)
    got = gpu_image(S.scene(name), name, spp=4, gpu_bvh=build == "lbvh")
    assert_parity(got, S.sum_in_order(ref[:, :, :4]), f"{name} on the {build} tree")


def test_reference_multilight_scene_per_sample_parity(restate):
    """The scene test_oracle.py pins the restatement to the reference on (four
    lights of four kinds from one COLLADA file, coloured glass of ior 1.2)."""
    from tests.oracle_helpers import golden
    from dsgpuraytracing_amd import ptdump
    path = golden("CBspheres_multilight_64x64.scene.ptd")
    args = (None, 64, 64, 4, 1, 3)
    ref = S.ref_samples(restate, path, None, n=4, scene_args=args)
    dev = _device(ptdump.read(path))
    got = []
    for i in range(4):
        dev.set_params(64, 64, 1, 4, 1, 3, sample_base=i)
        img = np.zeros((64, 64, 3), np.float32)
        dev.render_tiles([(0, 0, 64, 64), ], img)
        got.append(img)
    assert_parity(np.stack(got, axis=2), ref, "CBspheres_multilight samples")


# ---------------------------------------------------------------- the environment light's place
def test_two_environment_lights_are_refused():
    d = S.assemble(S.room_prims(), S.plain_table(), [S.A0, S.ENV, S.ENV])
    with pytest.raises(native.PtError) as e:
        _device(d)
    assert e.value.code == native.PT_E_INVALID


def test_environment_light_anywhere_in_the_list(restate, scene_dir):
    """PathTracer::set_scene pushes the environment light last, but trace_ray
    samples the lights in list order whatever their kind: so does the
    restatement, and so does the kernel -- an environment light in the middle
    of the list is honoured, draws in list order."""
    d = S.env_middle_scene()
    _, w, h, m, l, seed = args = S.ENV_MIDDLE_ARGS
    assert d["light_type"].tolist() == [S.L_AREA, S.L_ENV, S.L_POINT]
    path = S.write_scene(d, scene_dir, "env_middle")
    ref = S.ref_samples(restate, path, None, scene_args=args)
    dev = _device(d)
    got = []
    for i in range(S.N_SAMPLES):
        dev.set_params(w, h, 1, m, l, seed, sample_base=i)
        img = np.zeros((h, w, 3), np.float32)
        dev.render_tiles([(0, 0, w, h)], img)
        got.append(img)
    assert_parity(np.stack(got, axis=2), ref, "environment light second of three")
