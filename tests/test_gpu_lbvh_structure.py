"""The GPU-built tree (csrc/lbvh.hip) read back and checked node by node
(tests/bvh_check.py; Device.read_bvh), at the sizes and inputs where a builder
goes wrong: n = 1 .. 9 (the single-leaf path, kLeafNumber, kTreelet), the wave
and block edges, equal Morton codes, a scene without extent, spheres among
triangles, the deepest chain, every collapse and leaf-size knob.  A tree with
one primitive missing from a leaf, a box one ulp short or a stack bound one
too low fails here; the render tests would pass it.

For every case: the 4-wide tree, the binary tree and the primitive order are
sound, and 2048 rays aimed at the primitives agree with a float64 brute force
over the same float primitives -- hit, primitive and occlusion exactly, t to
1e-5 -- on every ray the reference calls decided (tests/bvh_check.py
brute_force; at most 2 % are not: tests/test_bvh_check_host.py)."""
import os

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.pathtracer import Device, Scene
from tests import bvh_check as bc
from tests import lbvh_scenes as ls
from tests.deep_trees import PT_STACK
from tests.oracle_helpers import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("PT_LBVH_PASSES", "PT_COLLAPSE", "PT_LBVH_MAXLEAF", "PT_BVH_BUILD", "PT_LBVH_CI")


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


def _knobs(monkeypatch, passes=None, collapse=None, max_leaf=None, build=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in zip(KNOBS, (passes, collapse, max_leaf, build)):
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _check_case(dev, monkeypatch, sc, passes=None, collapse=None, max_leaf=None):
    """Builds sc on the GPU under the knobs; returns the read-back tree."""
    scene = Scene(native.SceneArrays(sc.dump()))
    _knobs(monkeypatch, build="ref")   # the caller's order, as the library converts it
    dev.upload_scene(scene)
    ref = dev.read_bvh()
    assert ref["prim_map"] is None
    assert bc.check_order(ref["prims"], ref["norms"], None, sc.prims, sc.norms) == []
    _knobs(monkeypatch, passes, collapse, max_leaf)
    dev.upload_scene(scene, gpu_bvh=True)
    t = dev.read_bvh()
    ml = 4 if max_leaf is None else int(max_leaf)
    what = f"{sc.name} passes={passes} collapse={collapse} max_leaf={max_leaf}"
    assert t["prim_map"] is not None, what
    assert bc.check_bvh4(t["nodes4"], t["prims"], t["info"], ml, exact_stack=True) == [], what
    assert bc.check_bvh2(t["nodes2"], t["nodes4"], t["prims"], t["info"], ml) == [], what
    assert bc.check_order(t["prims"], t["norms"], t["prim_map"], ref["prims"], ref["norms"]) == [], what
    o, d, max_t = sc.rays()
    want = sc.reference()   # over the caller-order primitives: ids as pt_intersect reports them
    hit, tt, prim, anyh = dev.intersect(o, d, max_t)
    ok = want["decided"]
    share = 1.0 - ok.mean()
    both = ok & want["hit"] & (hit == 1)
    terr = np.abs(tt[both] / want["t"][both] - 1.0).max() if both.any() else 0.0
    print(f"{what}: {t['info']['n_nodes4']} nodes, stack {t['info']['bvh_stack']}, undecided {share:.4f}, "
          f"hit mismatches {(hit[ok] != want['hit'][ok]).sum()}, prim {(prim[both] != want['prim'][both]).sum()}, "
          f"occlusion {(anyh[ok] != want['occluded'][ok]).sum()}, max t error {terr:.2e}")
    assert share <= 0.02, what
    assert np.array_equal(hit[ok] == 1, want["hit"][ok]), what
    assert np.array_equal(prim[both], want["prim"][both]), what
    assert np.array_equal(anyh[ok] == 1, want["occluded"][ok]), what
    assert np.allclose(tt[both], want["t"][both], rtol=1e-5, atol=0), what
    return t


def test_read_back_needs_a_scene_and_skips_null_pointers(dev, monkeypatch):
    fresh = Device(0)
    with pytest.raises(native.PtError) as e:
        fresh.read_bvh()
    assert e.value.code == native.PT_E_NOSCENE
    assert native.lib().pt_debug_read_bvh(fresh.handle, None, None, None, None, None) == native.PT_E_NOSCENE
    fresh.close()
    _knobs(monkeypatch)
    sc = ls.scene("random", 9)
    dev.upload_scene(Scene(native.SceneArrays(sc.dump())), gpu_bvh=True)
    t = dev.read_bvh()
    assert t["info"]["n_prims"] == 9 and t["info"]["n_nodes2"] == 8 and t["info"]["has_prim_map"] == 1
    pm = np.full(9, -1, np.int32)
    assert native.lib().pt_debug_read_bvh(dev.handle, None, None, None, None, pm.ctypes.data) == native.PT_OK
    assert np.array_equal(pm, t["prim_map"])
    assert native.lib().pt_debug_read_bvh(dev.handle, None, None, None, None, None) == native.PT_OK


@pytest.mark.parametrize("n", ls.RANDOM_SIZES)
def test_random_triangles(dev, monkeypatch, n):
    _check_case(dev, monkeypatch, ls.scene("random", n))


@pytest.mark.parametrize("n", ls.OTHER_SIZES)
@pytest.mark.parametrize("family", ["coincident", "coplanar", "clusters", "mixed"])
def test_families(dev, monkeypatch, family, n):
    _check_case(dev, monkeypatch, ls.scene(family, n))


GRID_SCENES = [("random", 5), ("random", 7), ("random", 9), ("random", 65), ("random", 257), ("coincident", 7),
               ("coincident", 65), ("coplanar", 5), ("coplanar", 65), ("clusters", 65), ("mixed", 4), ("mixed", 7),
               ("mixed", 65), ("staircase", None)]


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("collapse", [None, "dp"])
@pytest.mark.parametrize("passes", [0, 1, 3])
def test_knob_grid(dev, monkeypatch, passes, collapse, max_leaf):
    """Every treelet-pass count x greedy / DP collapse x leaf limit, over
    scenes of each family on both sides of the treelet and wave sizes."""
    for family, n in GRID_SCENES:
        _check_case(dev, monkeypatch, ls.scene(family, n), passes, collapse, max_leaf)


def test_staircase_deepest_chain(dev, monkeypatch):
    """The Karras tree of the staircase scene (PT_LBVH_PASSES=0: no
    restructuring) is a 30-deep chain of single-primitive leaves, three of
    them and the rest of the chain per 4-wide node.  Reported stack, as
    measured on an MI355X: 31 over 11 nodes with PT_LBVH_PASSES=0, 12 over 12
    nodes with the default three passes.  31 is beyond PT_STACK = 24: the
    bound is asserted.  The 2048 rays themselves stay far below it (their
    highest stack is 3: the leaves lie along three lines, and a straight ray
    meets the boxes of one); tests/test_gpu_deep_trees.py runs the spill path
    over a GPU-built chain whose leaves a ray can enter all at once."""
    t0 = _check_case(dev, monkeypatch, ls.scene("staircase"), passes=0)
    t3 = _check_case(dev, monkeypatch, ls.scene("staircase"))
    print(f"staircase: stack {t0['info']['bvh_stack']} (passes 0), {t3['info']['bvh_stack']} (default)")
    assert t0["info"]["bvh_stack"] > PT_STACK


@pytest.mark.parametrize("lo,hi,short", [(0.1, 0.7, False), (0.1, 0.8, True), (0.4, 0.6, True)])
def test_single_leaf_box_contains_its_triangle(dev, monkeypatch, lo, hi, short):
    """One triangle with corners lo and hi on each axis.  The single-leaf path
    used to box it by round_down(lo) + (float)(hi - lo), a float sum rounded
    to nearest, which can land below the float vertex v0 + e1 (and, for other
    inputs, v0): for 0.1 / 0.8 it gives 0.79999995 against 0.80000001, for
    0.4 / 0.6 0.59999996 against 0.60000001 (for 0.1 / 0.7 it happens to
    hold: 0.70000005).  The box now comes from the float primitives."""
    g = np.array([[lo, lo, lo, hi, lo, hi, lo, hi, hi]])
    sc = ls.TinyScene(f"corners_{lo}_{hi}", [ls.TRI], g, 1.0)
    top = (sc.prims[0, 0:3].astype(np.float64) + np.maximum(sc.prims[0, 4:7], sc.prims[0, 8:11]).astype(np.float64))
    smin = np.float32(lo)
    smin = np.nextafter(smin, np.float32(-np.inf)) if float(smin) > lo else smin   # round_down(lo)
    assert (float(np.float32(smin + np.float32(hi - lo))) < top.max()) == short    # the scene-box sum
    t = _check_case(dev, monkeypatch, sc)
    assert (t["info"]["root_hi"].astype(np.float64) >= top).all()
    assert t["info"]["n_nodes4"] == 1 and t["info"]["bvh_stack"] == 0


@pytest.mark.parametrize("build", ["sah", "ref"])
@pytest.mark.parametrize("name", ["c1_default_64x64", "CBspheres_64x64"])
def test_host_trees(dev, monkeypatch, name, build):
    """The host-built render trees (PT_BVH_BUILD=sah: render_tree.cpp's binned
    SAH tree; =ref: the caller's), collapsed by build_host_bvh."""
    scene = Scene.from_dump(golden(f"{name}.scene.ptd"))
    d = scene.arrays.d
    prims_in, norms_in = ls.device_prims(d["prim_type"], d["prim_bsdf"], d["prim_geom"], d["prim_norm"])
    _knobs(monkeypatch, build=build)
    dev.upload_scene(scene)
    t = dev.read_bvh()
    assert (t["prim_map"] is not None) == (build == "sah")
    assert bc.check_order(t["prims"], t["norms"], t["prim_map"], prims_in, norms_in) == []
    assert bc.check_bvh4(t["nodes4"], t["prims"], t["info"], 8) == []


@pytest.fixture(scope="module")
def bunny():
    return Scene.from_dae(os.path.join(ROOT, "assets", "CBbunny.dae"), 96, 96)


def test_bunny_builds_are_identical_and_sound(dev, monkeypatch, bunny):
    """28,576 triangles over many workgroups and XCDs, built three times on
    one context: the bottom-up passes race only if their ordering is wrong,
    and a race shows as a tree that differs from build to build or breaks a
    rule.  (Node numbers come from atomicAdd: compared in canonical order.)"""
    d = bunny.arrays.d
    prims_in, norms_in = ls.device_prims(d["prim_type"], d["prim_bsdf"], d["prim_geom"], d["prim_norm"])
    _knobs(monkeypatch)
    builds = []
    for _ in range(3):
        dev.upload_scene(bunny, gpu_bvh=True)
        builds.append(dev.read_bvh())
    t = builds[0]
    c0 = bc.canonical(t["nodes4"])
    for b in builds[1:]:
        assert b["info"]["n_nodes4"] == t["info"]["n_nodes4"] and b["info"]["bvh_stack"] == t["info"]["bvh_stack"]
        assert np.array_equal(bc.canonical(b["nodes4"]), c0)
        assert np.array_equal(b["prims"].view(np.uint32), t["prims"].view(np.uint32))
        assert np.array_equal(b["prim_map"], t["prim_map"])
    assert bc.check_bvh4(t["nodes4"], t["prims"], t["info"], 4, exact_stack=True) == []
    assert bc.check_bvh2(t["nodes2"], t["nodes4"], t["prims"], t["info"], 4) == []
    assert bc.check_order(t["prims"], t["norms"], t["prim_map"], prims_in, norms_in) == []


@pytest.mark.parametrize("which", ["bunny", "random257"])
def test_treelet_passes_do_not_raise_the_sah_cost(dev, monkeypatch, bunny, which):
    """Every treelet rebuild keeps the best of all topologies of its seven
    leaves, the present one among them, so a further pass cannot raise the
    tree's SAH cost -- but for rounding: the kernel chooses in float32 over
    sums of at most 2n - 1 positive terms, the test sums in float64; the
    slack is a relative 2n * 2^-24."""
    scene = bunny if which == "bunny" else Scene(native.SceneArrays(ls.scene("random", 257).dump()))
    costs = []
    for passes in (0, 1, 2, 3):
        _knobs(monkeypatch, passes=passes)
        dev.upload_scene(scene, gpu_bvh=True)
        t = dev.read_bvh()
        costs.append(bc.sah_cost(t["nodes2"], t["prims"], 1.0, 4))
    n = scene.arrays.n_prims
    print(f"{which}: SAH cost after 0, 1, 2, 3 passes: " + ", ".join(f"{c:.6g}" for c in costs))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1.0 + 2 * n * 2.0 ** -24), costs


def test_unbounded_max_t_equals_render_tmax(dev, monkeypatch):
    """max_t = +inf (the reference's default ray) and 1e300 answer as 3.0e38,
    the traversal's own `far' value: pt_intersect clamps max_t to it.
    Unclamped, a ray with no negative direction component enters the unused
    slots of a 4-wide node (their boxes are at +inf: inf <= inf), pushes the
    stack bound does not count.  Random n = 64: a stack far below PT_STACK."""
    sc = ls.scene("random", 64)
    _knobs(monkeypatch)
    dev.upload_scene(Scene(native.SceneArrays(sc.dump())), gpu_bvh=True)
    assert dev.read_bvh()["info"]["bvh_stack"] <= 12
    rng = np.random.default_rng(9)
    m = 1024
    p = sc.prims.astype(np.float64)
    pick = rng.integers(0, sc.n, m)
    b = rng.dirichlet([2.0, 2.0, 2.0], m)
    tgt = p[pick, 0:3] + p[pick, 4:7] * b[:, 1:2] + p[pick, 8:11] * b[:, 2:3]
    u = np.abs(rng.normal(size=(m, 3)))           # all three components positive
    u[m // 2:, 0] = 0.0                           # exact zero components: x ...
    u[3 * m // 4:, 1] = 0.0                       # ... and x, y: axis-parallel rays along +z
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = tgt - 2.0 * u
    base = dev.intersect(o, u, np.full(m, 3.0e38))
    assert base[0].mean() > 0.9 and base[3].mean() > 0.9
    for far in (np.inf, 1e300):
        got = dev.intersect(o, u, np.full(m, far))
        for a, w in zip(got, base):
            assert np.array_equal(a, w)
