"""The device holds exactly what the host flattener (csrc/scene_flatten.cpp)
produced: uploads read back with Device.read_bvh against the byte pins of
tests/golden/flatten_hashes.json (tests/test_scene_flatten.py checks the
flattener itself against them on the CPU).  No render."""
import hashlib
import json

import numpy as np
import pytest

from dsgpuraytracing_amd.pathtracer import Device, Scene
from tests.oracle_helpers import golden

pytestmark = pytest.mark.gpu
KNOBS = ("PT_BVH_BUILD", "PT_COLLAPSE", "PT_LBVH_PASSES", "PT_LBVH_MAXLEAF", "PT_LBVH_CI")
# dump: the fixture's scene (c1env is the C1 scene plus an environment light: the same geometry)
SCENES = {"c1_default_64x64": "c1env", "CBspheres_64x64": "CBspheres"}


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pins():
    return json.load(open(golden("flatten_hashes.json")))["cases"]


def _upload(dev, monkeypatch, name, build):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if build:
        monkeypatch.setenv("PT_BVH_BUILD", build)
    dev.upload_scene(Scene.from_dump(golden(f"{name}.scene.ptd")))
    return dev.read_bvh()


def _sha(a):
    return hashlib.sha256(b"" if a is None else np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("build", ["ref", "sah"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_trees_on_the_device_are_the_flatteners(dev, monkeypatch, pins, name, build):
    t = _upload(dev, monkeypatch, name, build)
    pin = pins[f"{SCENES[name]}-{build}-unset"]
    want = {**pin["parent"], **pin["moved"]}
    for k in ("nodes4", "nodes2", "prims", "norms", "prim_map"):
        assert _sha(t[k]) == want.get(f"sha256.{k}", _sha(None)), k  # (the fixture has no key for an empty array)
    assert t["info"]["bvh_stack"] == want["bvh_stack"]
    for k in ("root_lo", "root_hi"):
        assert t["info"][k].tolist() == [float.fromhex(v) for v in want[k]], k


@pytest.mark.parametrize("name", sorted(SCENES))
def test_default_tree_keeps_the_callers_binary_nodes(dev, monkeypatch, pins, name):
    t = _upload(dev, monkeypatch, name, None)
    assert _sha(t["nodes2"]) == pins[f"{SCENES[name]}-ref-unset"]["parent"]["sha256.nodes2"]
    assert _sha(t["nodes2"]) == pins[f"{SCENES[name]}-gpu-unset"]["parent"]["sha256.nodes2"]
