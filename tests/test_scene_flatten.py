"""The host flattening of an uploaded scene (csrc/scene_flatten.cpp:
flatten_scene, read_flatten_knobs) on the CPU.

tests/flatten/flatten_driver.cpp is linked with csrc/scene_flatten.cpp,
render_tree.cpp, scene_host.cpp, exr_io.cpp and pt_error.cpp, built with
-fsanitize=address,undefined (no recovery), and run as a child process: any
sanitizer report fails the test (the recipe: tests/flatten_helpers.py, shared
with tests/test_deep_trees_host.py).  The driver writes every array of the
FlatScene as raw bytes and prints the scalars; this module hashes and checks
them:
 (a) the bytes of committed scenes against tests/golden/flatten_hashes.json,
     a pin of what pt_api.cpp produced before the code moved (the fixture's
     "source" says how each part was recorded),
 (b) the structure of the trees over tiny inputs (tests/bvh_check.py), and
     the primitive conversion against tests/lbvh_scenes.py device_prims,
 (c) the refusals and their messages."""
import hashlib
import json
import os

import numpy as np
import pytest

from dsgpuraytracing_amd import ptdump, scenes
from tests import bvh_check as bc
from tests import lbvh_scenes as ls
from tests.flatten_helpers import flatten_driver, load
from tests.oracle_helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = golden("flatten_hashes.json")
EMPTY = hashlib.sha256(b"").hexdigest()

PIN_SCENES = {  # name: (dae, environment map)
    "CBspheres": (os.path.join(ROOT, "assets", "CBspheres.dae"), None),
    "CBbunny": (os.path.join(ROOT, "assets", "CBbunny.dae"), None),
    "multilight": (golden("CBspheres_multilight.dae"), None),
    "c1env": (scenes.C1_DAE, golden("env_sky_64x32.exr")),
}
TREES = ("ref", "sah", "gpu")  # gpu: PT_BVH_BUILD unset (the GPU builds the render tree)
COLLAPSES = ("unset", "dp", "area", "count", "sah")
BOXES = ("root_lo", "root_hi", "root_lo_d", "root_hi_d", "scene_min", "scene_extent")


def knobs(tree, collapse="unset"):
    return ("" if tree == "gpu" else f" tree={tree}") + ("" if collapse == "unset" else f" collapse={collapse}")


def pin_cases():
    return [f"name={s}-{t}-{c} dae={dae}" + (f" env={env}" if env else "") + knobs(t, c)
            for s, (dae, env) in PIN_SCENES.items() for t in TREES for c in COLLAPSES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return flatten_driver(tmp_path_factory)  # (the build recipe: tests/flatten_helpers.py)


def summary(o):
    """What the fixture pins of one case: a flat dict of strings and numbers."""
    d = {f"sha256.{k}": v for k, v in o["sha256"].items() if v != EMPTY}  # (no key: the array is empty)
    d.update({k: o[k] for k in ("bvh_stack", "tri_only", "env_w", "env_h") if k in o})
    d.update({k: o[k] for k in BOXES if k in o and o[k] != ["0x0p+0"] * 3})  # (no key: unset for that tree)
    return d


# ---- (a) the bytes

def test_bytes_are_the_parents(driver):
    fx = json.load(open(FIXTURE))["cases"]
    out = driver(pin_cases())
    assert sorted(o["name"] for o in out) == sorted(fx)
    bad = []
    for o in out:
        assert o["rc"] == 0, o
        got, want = summary(o), {**fx[o["name"]]["parent"], **fx[o["name"]]["moved"]}
        assert sorted(got) == sorted(want), o["name"]
        bad += [(o["name"], k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, bad[:10]


def test_pinned_primitives_are_device_prims_of_the_dumps():
    # the parent could not expose its primitive records on the CPU: device_prims restates them
    fx = json.load(open(FIXTURE))["cases"]
    for name, dump in (("CBspheres", "CBspheres_64x64.scene.ptd"), ("c1env", "c1_default_64x64.scene.ptd")):
        d = ptdump.read(golden(dump))
        want_p, want_n = ls.device_prims(d["prim_type"], d["prim_bsdf"], d["prim_geom"], d["prim_norm"])
        assert fx[f"{name}-ref-unset"]["moved"]["sha256.prims"] == hashlib.sha256(want_p.tobytes()).hexdigest()
        assert fx[f"{name}-ref-unset"]["moved"]["sha256.norms"] == hashlib.sha256(want_n.tobytes()).hexdigest()


# ---- (b) structure on tiny inputs

TINY = [1, 2, 3, 4, 8, 9, 17]  # 9 and 17 cross the 8-primitive leaf split
CHAIN = 40


def chain_dump(n_inner, seed=3):
    """A right-leaning chain: inner node i = node 2i with a one-triangle leaf
    (node 2i + 1) on the left and the next inner node (the last: a leaf) on the
    right, boxes in double from the triangles."""
    sc = ls.random_scene(n_inner + 1, seed)
    d = sc.dump()
    g = sc.geom.reshape(-1, 3, 3)
    lo, hi = g.min(1), g.max(1)
    sub_lo = np.minimum.accumulate(lo[::-1])[::-1]  # box of primitives i ..
    sub_hi = np.maximum.accumulate(hi[::-1])[::-1]
    bb, info = [], []
    for i in range(n_inner):
        bb += [np.r_[sub_lo[i], sub_hi[i]], np.r_[lo[i], hi[i]]]
        info += [[i, n_inner + 1 - i, 2 * i + 1, 2 * i + 2], [i, 1, -1, -1]]
    bb.append(np.r_[lo[n_inner], hi[n_inner]])
    info.append([n_inner, 1, -1, -1])
    d["node_bb"] = np.concatenate(bb).astype(np.float64)
    d["node_info"] = np.array(info, np.int64).reshape(-1)
    return sc, d


@pytest.fixture(scope="module")
def tiny(driver, tmp_path_factory):
    """{(scene, tree, collapse): (TinyScene, driver record)}"""
    tmp = tmp_path_factory.mktemp("tiny")
    made = {f"mixed{n}": (ls.scene("mixed", n), ls.scene("mixed", n).dump()) for n in TINY}
    made[f"chain{CHAIN}"] = chain_dump(CHAIN)
    cases, keys = [], []
    for name, (sc, d) in made.items():
        ptdump.write(str(tmp / f"{name}.ptd"), d)
        for tree in TREES + ("lbvh",):  # lbvh: the upload came through pt_upload_scene_lbvh
            for col in ("unset", "area") if tree in ("ref", "sah") else ("unset",):
                keys.append((name, tree, col))
                cases.append(f"name={name}-{tree}-{col} dump={tmp / (name + '.ptd')}" + knobs(tree, col))
    return {k: (made[k[0]][0], o) for k, o in zip(keys, driver(cases))}


def _info(o, n4, n2, n):
    return {"n_nodes4": n4, "n_nodes2": n2, "n_prims": n, "bvh_stack": o["bvh_stack"],
            "root_lo": [float.fromhex(v) for v in o["root_lo"]], "root_hi": [float.fromhex(v) for v in o["root_hi"]]}


def _leaves2(nodes2):
    order, bad, used = bc._walk2(nodes2)
    assert bad == [] and sorted(order) == list(range(len(nodes2)))  # every node reached once
    ref = bc.refs2(nodes2)
    return [int(ref[i, c]) for i in order for c in (0, 1) if ref[i, c] < 0 and (c == 0 or used[i])]


@pytest.mark.parametrize("name", [f"mixed{n}" for n in TINY] + [f"chain{CHAIN}"])
def test_tiny_trees_are_sound(tiny, name):
    for (nm, tree, col), (sc, o) in tiny.items():
        if nm != name:
            continue
        what = (nm, tree, col)
        assert o["rc"] == 0, o
        prims, norms, n4, n2 = (load(o, k) for k in ("prims", "norms", "nodes4", "nodes2"))
        if tree == "lbvh":  # no caller's tree at all: the GPU builds both
            assert len(n2) == 0 and o["bvh_stack"] == 0, what
            n2 = load(tiny[(nm, "gpu", "unset")][1], "nodes2")
        # the caller's tree as binary nodes: every primitive in one leaf of <= 8, the double boxes rounded outward
        cover = np.zeros(sc.n, int)
        lo2, hi2 = bc.boxes2(n2)
        ref2 = bc.refs2(n2)
        for r in _leaves2(n2):
            first, count = bc.decode(r)
            assert 1 <= count <= 8 and first + count <= sc.n, what
            cover[first:first + count] += 1
            sub = ls.TinyScene("", sc.prim_type[first:first + count], sc.geom[first:first + count], 1.0)
            i, c = [(i, c) for i in range(len(n2)) for c in (0, 1) if ref2[i, c] == r][0]
            assert (lo2[i, c] <= sub.bounds()[0]).all() and (hi2[i, c] >= sub.bounds()[1]).all(), what
        assert (cover == 1).all(), what
        if tree in ("gpu", "lbvh"):
            assert len(n4) == 0 and len(load(o, "prim_map")) == 0 and len(load(o, "prims_ref")) == 0, what
            assert (prims.tobytes(), norms.tobytes()) == (sc.prims.tobytes(), sc.norms.tobytes()), what
            lo, hi = sc.bounds()
            smin = lo.astype(np.float32)  # rounded down
            smin = np.where(smin.astype(np.float64) > lo, np.nextafter(smin, np.float32(-np.inf)), smin)
            assert [float.fromhex(v) for v in o["scene_min"]] == smin.tolist(), what
            assert [float.fromhex(v) for v in o["scene_extent"]] == (hi - lo).astype(np.float32).tolist(), what
            continue
        # topology, leaf partition, containment without tolerance, stack bound, forward references
        assert bc.check_bvh4(n4, prims, _info(o, len(n4), len(n2), sc.n), 8) == [], what
        if tree == "ref":
            assert (prims.tobytes(), norms.tobytes()) == (sc.prims.tobytes(), sc.norms.tobytes()), what
            assert len(load(o, "prim_map")) == 0 and len(load(o, "prims_ref")) == 0, what
            assert set(_leaves2(n2)) == bc.leaf_cursors4(n4), what
        else:
            assert bc.check_order(prims, norms, load(o, "prim_map"), sc.prims, sc.norms) == [], what
            assert load(o, "prims_ref").tobytes() == sc.prims.tobytes(), what
            assert load(o, "norms_ref").tobytes() == sc.norms.tobytes(), what


def test_chain_needs_a_deep_stack(tiny):
    _, o = tiny[(f"chain{CHAIN}", "ref", "area")]
    assert bc.recomputed_stack(load(o, "nodes4")) > 16 and o["bvh_stack"] <= 256


# ---- (c) refusals

def _edit(d, **kw):
    d = dict(d)
    d.update(kw)
    return d


def _more_lights(d, types):
    k = len(types)
    return _edit(d, light_type=np.r_[d["light_type"], np.array(types, np.int32)],
                 light_rad=np.r_[d["light_rad"], np.ones(3 * k, np.float32)],
                 light_geom=np.r_[d["light_geom"], np.zeros(12 * k)],
                 light_area=np.r_[d["light_area"], np.zeros(k, np.float32)])


def refusals():
    sc = ls.scene("mixed", 9)
    d = sc.dump()
    n = sc.n
    lo, hi = sc.bounds()
    box = np.r_[lo, hi]
    env = dict(env_shape=np.array([2, 4], np.int64), env_rgb=np.ones(24, np.float32))
    two = np.concatenate([box, box]).astype(np.float64)

    def at0(a, v):
        a = a.copy()
        a[0] = v
        return a
    msg = "pt_upload_scene: "
    return {
        "half_empty": (_edit(d, node_bb=two, node_info=np.array([0, n, 1, -1, 0, n, -1, -1], np.int64)),
                       msg + "half-empty BVH node"),
        "child_range": (_edit(d, node_bb=two, node_info=np.array([0, n, 1, 2, 0, n, -1, -1], np.int64)),
                        msg + "BVH child out of range"),
        "leaf_range": (_edit(d, node_info=np.array([0, n + 1, -1, -1], np.int64)), msg + "bad leaf range"),
        "leaf_empty": (_edit(d, node_info=np.array([0, 0, -1, -1], np.int64)), msg + "bad leaf range"),
        "bsdf_index": (_edit(d, prim_bsdf=at0(d["prim_bsdf"], len(d["bsdf_type"]))),
                       msg + "primitive BSDF index out of range"),
        "prim_type": (_edit(d, prim_type=at0(d["prim_type"], 7)), msg + "unknown primitive type"),
        "bsdf_type": (_edit(d, bsdf_type=at0(d["bsdf_type"], 5)), msg + "unknown BSDF type"),
        "light_type": (_edit(d, light_type=at0(d["light_type"], 5)), msg + "unsupported light type"),
        "two_env": (_edit(_more_lights(d, [4, 4]), **env), msg + "more than one environment light"),
        "env_no_map": (_more_lights(d, [4]),
                       msg + "environment light without a map (env_rgb/env_width/env_height)"),
        "map_no_env": (_edit(d, **env), msg + "env_rgb given but no PT_LIGHT_ENVIRONMENT light"),
        "deep_chain": (chain_dump(400)[1], msg + "BVH needs a deeper traversal stack (400 > 256)"),
    }


def test_refusals(driver, tmp_path):
    cases, want = [], []
    for name, (d, message) in refusals().items():
        ptdump.write(str(tmp_path / f"{name}.ptd"), d)
        for tree in ("gpu", "ref"):
            cases.append(f"name={name}-{tree} dump={tmp_path / (name + '.ptd')}" + knobs(tree))
            want.append(message)
    for o, message in zip(driver(cases), want):
        assert (o["rc"], o["error"]) == (-1, message), o  # PT_E_INVALID
