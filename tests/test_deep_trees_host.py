"""The inputs of tests/test_gpu_deep_trees.py on the CPU: the ragged chain of
tests/deep_trees.py flattened with PT_BVH_BUILD=ref by the flatten driver
(tests/flatten_helpers.py), and stack_walk over the flattened tree.

What is asserted here are conditions on the INPUTS, so that the GPU tests'
rays are known to take every branch at the boundary between the LDS stack and
the spill area; the walk itself is first checked against the float64 brute
force of tests/trace_helpers.py.

Observed (generator seed 11 for the layers, 5 for the rays), plain chain /
sphere variant: 32 nodes, bvh_stack 95 = recomputed; 53.8 % / 53.4 % of the
2048 rays peak at >= PT_STACK + 4, 37.4 % / 39.0 % at <= PT_STACK - 4; the
rarest of the 21 (height, pushes) pairs occurs in 68 / 68 node steps; every
group of 64 rays is mixed."""
import numpy as np
import pytest

from dsgpuraytracing_amd import ptdump
from tests import bvh_check as bc
from tests import deep_trees as dt
from tests import lbvh_scenes as ls
from tests import trace_helpers as th
from tests.deep_trees import PT_STACK
from tests.flatten_helpers import flatten_driver, load

VARIANTS = ("chain", "sphere")


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    """{variant: (driver record, nodes4, prims, stack_walk of deep_rays)}"""
    run = flatten_driver(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("deep")
    cases = []
    for v in VARIANTS:
        ptdump.write(str(tmp / f"{v}.ptd"), dt.ragged_chain(sphere=v == "sphere"))
        cases.append(f"name={v} dump={tmp / (v + '.ptd')} tree=ref")
    out = {}
    o, d, tmax = dt.as_doubles(dt.deep_rays())
    for v, rec in zip(VARIANTS, run(cases)):
        assert rec["rc"] == 0, rec
        n4, prims = load(rec, "nodes4"), load(rec, "prims")
        out[v] = (rec, n4, prims, dt.stack_walk(n4, prims, o, d, tmax))
    return out


def test_pt_stack_is_read_from_the_header():
    assert 8 <= PT_STACK < dt.PT_STACK_MAX


@pytest.mark.parametrize("variant", VARIANTS)
def test_walk_agrees_with_brute_force(flat, variant):
    """The walk's own check, over deep_rays and over rays cut short around
    the hit distance: hit, primitive and t of every ray whose nearest and
    second-nearest hits are more than 1e-9 apart."""
    _, n4, prims, walk = flat[variant]
    o, d, tmax = dt.as_doubles(dt.deep_rays())
    arrays = dt.float_arrays(prims)
    rng = np.random.default_rng(7)
    short = np.where(walk["hit"], walk["t"] * rng.uniform(0.3, 1.7, len(o)), 1.0)
    for tm, w in ((tmax, walk), (short, dt.stack_walk(n4, prims, o, d, short))):
        ref = th.brute_force_rays(arrays, o, d, tm)
        sure = ~ref["hit"] | (ref["t2"] - ref["t"] > 1e-9)
        assert sure.mean() > 0.95 and 0.3 < ref["hit"].mean()
        assert np.array_equal(w["hit"][sure], ref["hit"][sure])
        assert np.array_equal(w["prim"][sure], ref["prim"][sure])
        assert np.allclose(w["t"][sure], ref["t"][sure], rtol=1e-12, atol=0)
    if variant == "sphere":
        assert (walk["prim"] == len(prims) - 1).sum() > 50  # the sphere is seen


@pytest.mark.parametrize("variant", VARIANTS)
def test_flattened_chain_is_deep(flat, variant):
    rec, n4, prims, _ = flat[variant]
    assert rec["bvh_stack"] == bc.recomputed_stack(n4) == dt.chain_stack()
    assert rec["bvh_stack"] >= PT_STACK + 8
    assert rec["tri_only"] == (variant == "chain")
    assert len(prims) == dt.N_CHAIN and len(load(rec, "prim_map")) == 0  # the caller's order


@pytest.mark.parametrize("variant", VARIANTS)
def test_rays_cover_the_stack_boundary(flat, variant):
    rec, n4, _, walk = flat[variant]
    c = dt.coverage(walk)
    print(variant, "nodes", len(n4), "stack", rec["bvh_stack"], c)
    assert c["deep"] >= 0.40
    assert c["shallow"] >= 0.25
    assert c["pairs"] == 21 and c["rarest"] >= 16
    assert c["mixed"]


def test_fat_staircase_is_the_staircase_to_the_builder():
    """Same Morton cells as tests/lbvh_scenes.py staircase_scene, primitive by
    primitive (the builder codes the centre of a primitive's box), so the GPU
    builds the same chain; but every needle's box holds the shared cube, and
    the rays come in both kinds."""
    fat, stair = dt.fat_staircase(), ls.scene("staircase")
    cells = ls.morton_cells(fat)
    assert np.array_equal(cells[:-1], ls.morton_cells(stair)[:-1])
    assert (cells[-1] == 1023).sum() >= 2  # (the far corner pins the scene box: the largest code in both)
    lo, hi = fat.bounds()
    assert (lo == 0).all() and (hi >= dt.FAT_SCALE).all() and (hi < 1.001 * dt.FAT_SCALE).all()
    plo, phi = bc.prim_extent(fat.prims)
    assert (plo[1:-1] <= dt.FAT_CUBE[0]).all() and (phi[1:-1] >= dt.FAT_CUBE[1]).all()
    o, d, _ = dt.as_doubles(dt.fat_staircase_rays())
    t = (0.5 * (dt.FAT_CUBE[0] + dt.FAT_CUBE[1]) - o[:, 0]) / d[:, 0]  # where the ray crosses the cube's middle in x
    p = o + d * t[:, None]
    inside = ((p >= dt.FAT_CUBE[0]) & (p <= dt.FAT_CUBE[1])).all(1)
    assert inside[0::2].mean() > 0.5 and not inside[1::2].any()
