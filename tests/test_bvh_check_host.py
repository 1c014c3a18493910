"""The tree checker (tests/bvh_check.py) checked on the host: a hand-built
sound BVH4 / BVH2 over 12 primitives passes, and every single mutation a
builder could get subtly wrong is reported, by the rule named for it.  This is
what makes tests/test_gpu_lbvh_structure.py fail on a wrong builder."""
import numpy as np
import pytest

from tests import bvh_check as bc

F = np.float32
INF = np.inf


def _tri(p1, p2, p3, bsdf=0):
    p1, p2, p3 = (np.asarray(v, np.float64) for v in (p1, p2, p3))
    rec = np.zeros(12, F)
    rec[0:3] = p1
    rec[3] = np.int32((bsdf << 1) | 1).view(F)
    rec[4:7] = (p2 - p1).astype(F)
    rec[8:11] = (p3 - p1).astype(F)
    return rec


def _sphere(c, r, bsdf=0):
    rec = np.zeros(12, F)
    rec[0:3] = c
    rec[3] = np.int32(bsdf << 1).view(F)
    rec[4], rec[5] = r, F(r) * F(r)
    return rec


def _outward(lo, hi):
    """The tightest float32 box around a float64 one."""
    a, b = lo.astype(F), hi.astype(F)
    a = np.where(a.astype(np.float64) > lo, np.nextafter(a, F(-INF)), a)
    b = np.where(b.astype(np.float64) < hi, np.nextafter(b, F(INF)), b)
    return a, b


LEAVES = [(0, 2), (2, 1), (3, 4), (7, 2), (9, 3)]  # (first, count); primitive 2 is the sphere


@pytest.fixture()
def tree():
    """12 primitives along x; leaves L0..L4 as LEAVES.
    BVH4: node 0 = [L0, ->1, ->2, unused], node 1 = [L1, L2, -, -], node 2 = [L3, L4, -, -].
    BVH2: node 0 = (->1, ->2), node 1 = (L0, ->3), node 3 = (L1, L2), node 2 = (L3, L4); 11 entries."""
    rng = np.random.default_rng(3)
    prims = []
    for i in range(12):
        base = np.array([i * 1.1 + 0.1, 0.3, 0.7]) + rng.uniform(0, 0.1, 3)
        if i == 2:
            prims.append(_sphere(base, 0.37))
        else:
            prims.append(_tri(base, base + rng.uniform(0.1, 0.9, 3), base + rng.uniform(-0.5, 0.9, 3)))
    prims = np.array(prims, F)
    plo, phi = bc.prim_extent(prims)

    def leaf_box(j):
        f, c = LEAVES[j]
        return _outward(plo[f:f + c].min(0), phi[f:f + c].max(0))

    def union(*boxes):
        return np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)

    L = [leaf_box(j) for j in range(5)]
    cur = [bc.cursor(*LEAVES[j]) for j in range(5)]
    n4 = np.full((3, 32), INF, F)
    n4[:, 28:32] = 0

    def put4(i, k, box, ref):
        n4[i, k + 0], n4[i, k + 4] = box[0][0], box[1][0]
        n4[i, k + 8], n4[i, k + 12] = box[0][1], box[1][1]
        n4[i, k + 16], n4[i, k + 20] = box[0][2], box[1][2]
        n4[i, 24 + k:25 + k].view(np.int32)[0] = ref

    for i in range(3):
        for k in range(4):
            put4(i, k, (np.full(3, INF, F), np.full(3, INF, F)), bc.cursor(0, 1))
    put4(0, 0, L[0], cur[0])
    put4(0, 1, union(L[1], L[2]), 1)
    put4(0, 2, union(L[3], L[4]), 2)
    put4(1, 0, L[1], cur[1])
    put4(1, 1, L[2], cur[2])
    put4(2, 0, L[3], cur[3])
    put4(2, 1, L[4], cur[4])
    n2 = np.zeros((11, 16), F)

    def put2(i, c, box, ref):
        col = (0, 4)[c]
        n2[i, col + 0], n2[i, col + 1], n2[i, col + 2], n2[i, col + 3] = box[0][0], box[1][0], box[0][1], box[1][1]
        n2[i, 8 + 2 * c], n2[i, 9 + 2 * c] = box[0][2], box[1][2]
        n2[i, 12 + c:13 + c].view(np.int32)[0] = ref

    put2(0, 0, union(L[0], L[1], L[2]), 1)
    put2(0, 1, union(L[3], L[4]), 2)
    put2(1, 0, L[0], cur[0])
    put2(1, 1, union(L[1], L[2]), 3)
    put2(3, 0, L[1], cur[1])
    put2(3, 1, L[2], cur[2])
    put2(2, 0, L[3], cur[3])
    put2(2, 1, L[4], cur[4])
    root = union(*L)
    info = {"n_prims": 12, "n_nodes4": 3, "n_nodes2": 11, "bvh_stack": 3, "has_prim_map": 1,
            "root_lo": root[0], "root_hi": root[1]}
    return {"n4": n4, "n2": n2, "prims": prims, "info": info}


def _rules(violations):
    return {v.split(":")[0] for v in violations}


def _set_ref(nodes, row, col, ref):
    nodes[row, col:col + 1].view(np.int32)[0] = ref


def test_sound_trees_pass(tree):
    assert bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4, exact_stack=True) == []
    assert bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4) == []
    assert bc.recomputed_stack(tree["n4"]) == 3  # root: 3 used slots leave 2, node 1 or 2 one more
    assert bc.leaf_cursors4(tree["n4"]) == {bc.cursor(*l) for l in LEAVES}


def test_primitive_dropped_from_a_leaf(tree):
    _set_ref(tree["n4"], 1, 25, bc.cursor(3, 3))  # L2 = [3, 7) -> [3, 6): primitive 6 in no leaf
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert _rules(v) == {"leaves"} and any("primitive 6 is in no leaf" in s for s in v)
    _set_ref(tree["n2"], 3, 13, bc.cursor(3, 3))
    v = bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4)
    assert _rules(v) == {"leaves"} and any("primitive 6 is in no leaf" in s for s in v)


def test_primitive_in_two_leaves(tree):
    _set_ref(tree["n4"], 2, 24, bc.cursor(6, 3))  # L3 = [7, 9) -> [6, 9): primitive 6 twice
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert "leaves" in _rules(v) and any("primitive 6 is in 2 leaves" in s for s in v)
    _set_ref(tree["n2"], 2, 12, bc.cursor(6, 3))
    v = bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4)
    assert any("primitive 6 is in 2 leaves" in s for s in v)


@pytest.mark.parametrize("node,col,down", [(1, 1, False), (1, 5, True), (0, 9, False), (0, 14, True), (2, 16, False),
                                            (0, 22, True)])
def test_child_box_one_ulp_short(tree, node, col, down):
    """One plane of one used slot moved one ulp inward: a leaf's box, and an
    inner child's (which then misses its own children's boxes too)."""
    x = tree["n4"][node, col]
    tree["n4"][node, col] = np.nextafter(x, F(-INF) if down else F(INF))
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert _rules(v) == {"containment"}, v


def test_binary_child_box_one_ulp_short(tree):
    tree["n2"][3, 5] = np.nextafter(tree["n2"][3, 5], F(-INF))  # child 1 hi.x of binary node 3
    v = bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4)
    assert _rules(v) == {"containment"}, v


def test_root_box_one_ulp_short(tree):
    tree["info"]["root_hi"] = tree["info"]["root_hi"].copy()
    tree["info"]["root_hi"][0] = np.nextafter(tree["info"]["root_hi"][0], F(-INF))
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert _rules(v) == {"containment"} and "root box" in v[0]


def test_backward_reference(tree):
    _set_ref(tree["n4"], 2, 25, 1)  # node 2's second slot: node 1 in place of the leaf L4
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert "topology" in _rules(v) and any("node 2 slot 1: reference 1 is not forward" in s for s in v)
    _set_ref(tree["n4"], 2, 25, bc.cursor(9, 3))
    _set_ref(tree["n4"], 0, 25, 0)  # the root referring to itself
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert any("is not forward" in s for s in v) and any("root is referenced" in s for s in v)
    _set_ref(tree["n4"], 0, 25, 3)  # past the last node
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert any("node 0 slot 1: reference 3 is not forward" in s for s in v)


def test_node_referenced_twice(tree):
    _set_ref(tree["n4"], 0, 26, 1)  # both inner slots of the root -> node 1; node 2 orphaned
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert any(s.startswith("topology: node 1 is referenced 2 times") for s in v)
    assert any(s.startswith("topology: node 2 is referenced 0 times") for s in v)
    assert any(s.startswith("topology: node 2 is not reachable") for s in v)
    _set_ref(tree["n2"], 0, 13, 1)
    v = bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4)
    assert "topology" in _rules(v)


def test_leaf_count_beyond_the_limit(tree):
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 3)  # L2 holds 4 = max_leaf + 1
    assert _rules(v) == {"leaves"} and any("leaf of 4 primitives, more than 3" in s for s in v)
    # nine primitives do not fit a cursor's three count bits: the ninth spills
    # into `first`, and the partition shows it
    _set_ref(tree["n4"], 1, 25, ~((3 << 3) | 8))
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 8)
    assert "leaves" in _rules(v)
    _set_ref(tree["n4"], 1, 25, bc.cursor(3, 4))
    _set_ref(tree["n4"], 2, 25, bc.cursor(9, 4))  # L4 = [9, 12) -> [9, 13): past the last primitive
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert any("leaves [0, 12)" in s for s in v)


def test_unused_slot_with_a_finite_plane(tree):
    tree["n4"][2, 14] = 5.0  # hi.y of node 2's third slot
    v = bc.check_bvh4(tree["n4"], tree["prims"], tree["info"], 4)
    assert v == ["leaves: node 2 slot 2: unused slot with a finite plane"]


def test_stack_understated(tree):
    info = dict(tree["info"], bvh_stack=2)
    v = bc.check_bvh4(tree["n4"], tree["prims"], info, 4)
    assert _rules(v) == {"stack"}
    info = dict(tree["info"], bvh_stack=4)  # overstated: a bound holds, equality does not
    assert bc.check_bvh4(tree["n4"], tree["prims"], info, 4) == []
    assert _rules(bc.check_bvh4(tree["n4"], tree["prims"], info, 4, exact_stack=True)) == {"stack"}


def test_binary_leaves_differ_from_wide_leaves(tree):
    """The same primitives split differently: [7, 9) + [9, 12) as [7, 10) + [10, 12)."""
    _set_ref(tree["n2"], 2, 12, bc.cursor(7, 3))
    _set_ref(tree["n2"], 2, 13, bc.cursor(10, 2))
    v = bc.check_bvh2(tree["n2"], tree["n4"], tree["prims"], tree["info"], 4)
    assert any("differ from the 4-wide tree's" in s for s in v)


def test_order(tree):
    rng = np.random.default_rng(1)
    prims_in = tree["prims"]
    norms_in = rng.normal(size=(12, 9)).astype(F)
    pm = rng.permutation(12).astype(np.int32)
    prims, norms = prims_in[pm].copy(), norms_in[pm].copy()
    assert bc.check_order(prims, norms, pm, prims_in, norms_in) == []
    assert bc.check_order(prims_in, norms_in, None, prims_in, norms_in) == []
    bad = pm.copy()
    bad[4] = bad[5]  # a repeated entry
    v = bc.check_order(prims, norms, bad, prims_in, norms_in)
    assert _rules(v) == {"order"} and "not a permutation" in v[0]
    flip = prims.copy()
    flip[7:8, 5:6].view(np.uint32)[0] ^= 1  # one mantissa bit of one primitive
    v = bc.check_order(flip, norms, pm, prims_in, norms_in)
    assert v == [f"order: primitive 7 is not bit-identical to the caller's primitive {pm[7]}"]
    flip = norms.copy()
    flip[3:4, 8:9].view(np.uint32)[0] ^= 1
    v = bc.check_order(prims, flip, pm, prims_in, norms_in)
    assert len(v) == 1 and "normals of primitive 3" in v[0]
    # -0.0 for 0.0 is a changed bit too
    flip = prims.copy()
    flip[0, 7] = F(-0.0)
    assert len(bc.check_order(flip, norms, pm, prims_in, norms_in)) == 1


def test_canonical_ignores_node_numbering(tree):
    n4 = tree["n4"]
    swapped = n4.copy()
    swapped[[1, 2]] = n4[[2, 1]]
    _set_ref(swapped, 0, 25, 2)
    _set_ref(swapped, 0, 26, 1)
    assert not np.array_equal(n4.view(np.uint32), swapped.view(np.uint32))
    assert np.array_equal(bc.canonical(n4), bc.canonical(swapped))
    other = swapped.copy()
    other[1, 0] = np.nextafter(other[1, 0], F(-INF))
    assert not np.array_equal(bc.canonical(n4), bc.canonical(other))


def test_sah_cost_by_hand():
    """Two unit-cube leaves side by side under one root: the root's box is
    2 x 1 x 1 (half area 5), each leaf's half area 3."""
    n2 = np.zeros((1, 16), F)
    n2[0, 0:4] = [0, 1, 0, 1]
    n2[0, 4:8] = [1, 2, 0, 1]
    n2[0, 8:12] = [0, 1, 0, 1]
    _set_ref(n2, 0, 12, bc.cursor(0, 2))
    _set_ref(n2, 0, 13, bc.cursor(2, 1))
    assert bc.sah_cost(n2, None, ci=1.0) == 5 + 3 * 2 + 3 * 1
    assert bc.sah_cost(n2, None, ci=0.5) == 5 + 0.5 * (3 * 2 + 3 * 1)


def test_brute_force_by_hand():
    prims = np.array([_tri([0, 0, 1], [4, 0, 1], [0, 4, 1]),       # z = 1
                      _tri([0, 0, 3], [4, 0, 3], [0, 4, 3]),       # z = 3, behind it
                      _sphere([10, 0, 0], 1.0)], F)
    o = np.array([[1, 1, 0], [1, 1, 2], [1, 1, 5], [10, 0, -5], [10, 0, 0], [3, 3, 0], [2, 2, 0], [1, 1, 0],
                  [10, 1, -5], [1, 1, 0]], np.float64)
    d = np.array([[0, 0, 1]] * 10, np.float64)
    d[2] = [0, 0, -1]
    max_t = np.array([2.0, 0.5, 10, 5, 0.5, 9, 9, 1.0, 9, 1.00001])
    r = bc.brute_force(prims, o, d, max_t)
    #      ray 0: hits z=1 at t=1, occluded within 2
    #      ray 1: starts between the planes: hits z=3 at t=1, not occluded within 0.5
    #      ray 2: travelling -z from z=5: z=3 first, t=2
    #      ray 3: the sphere from outside: t=4; occlusion takes the far root 6 > 5
    #      ray 4: from the sphere's centre: the far root, t=1; not within 0.5
    #      ray 5: (3,3) is outside both triangles (u + v = 1.5): a clear miss
    #      ray 6: (2,2) lies on the hypotenuse of both: a hit, but not decided
    #      ray 7: max_t equal to the hit distance: not occluded (t < max_t), not decided
    #      ray 8: grazes the sphere (disc = 0): not decided
    #      ray 9: max_t within 1e-4 relative of t: occluded, not decided
    assert r["hit"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert r["prim"].tolist() == [0, 1, 1, 2, 2, -1, 0, 0, 2, 0]
    assert np.allclose(r["t"], [1, 1, 2, 4, 1, -1, 1, 1, 5, 1], rtol=1e-15)
    assert r["occluded"].tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 1, 1]
    assert r["decided"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    # two hits within 1e-4 relative of each other: the nearest is not decided
    prims[1] = _tri([0, 0, 1.00005], [4, 0, 1.00005], [0, 4, 1.00005])
    r = bc.brute_force(prims, o[:1], d[:1], max_t[:1])
    assert r["hit"][0] and r["prim"][0] == 0 and not r["decided"][0]


# ---- the scenes and rays of tests/test_gpu_lbvh_structure.py, checked here first
def _all_scenes():
    from tests import lbvh_scenes as ls
    return ls.all_scenes()


@pytest.mark.parametrize("family,n", _all_scenes())
def test_ray_generator_leaves_few_rays_undecided(family, n):
    """At most 2 % of a case's rays may be left out as undecided; the
    reference alone decides that share, so it is settled here, without a GPU.
    The rays also do their work: aimed at interiors, they all hit, and about
    half are occluded within max_t."""
    from tests import lbvh_scenes as ls
    sc = ls.scene(family, n)
    r = sc.reference()
    share = 1.0 - r["decided"].mean()
    print(f"{sc.name}: {sc.n} primitives, undecided {share:.4f}, hit {r['hit'].mean():.3f}, "
          f"occluded {r['occluded'].mean():.3f}")
    assert share <= 0.02
    assert r["hit"].mean() >= 0.99 and 0.3 <= r["occluded"].mean() <= 0.7
    assert set(np.unique(r["prim"][r["hit"]])) >= set(sc.targets.tolist()) or sc.n > 64  # every target is hit


def test_scene_families_are_what_they_claim():
    from tests import lbvh_scenes as ls
    for n in ls.OTHER_SIZES:
        cells = ls.morton_cells(ls.scene("coincident", n))
        assert len(np.unique(cells[1:] if n >= 2 else cells, axis=0)) == 1   # one Morton code
        lo, hi = ls.scene("coplanar", n).bounds()
        assert hi[2] == lo[2] == 0.25                                        # no extent in z
        if n >= 3:  # the corner sphere's normalised centre reaches 1 on some axis and is mapped to cell 0
            sc = ls.scene("mixed", n)
            corner = np.setdiff1d(np.arange(sc.n), sc.targets)
            assert len(corner) == 1 and (ls.morton_cells(sc)[corner[0]] == 0).any()
            assert not bc.is_triangle(sc.prims)[corner[0]]
        sc = ls.scene("mixed", n)
        tri = bc.is_triangle(sc.prims)
        assert tri.sum() == n // 2 and (n < 2 or 0 < tri.sum() < n)
    cells = ls.morton_cells(ls.scene("staircase"))
    code = [sum(((int(c[a]) >> j) & 1) << (3 * j + 2 - a) for a in range(3) for j in range(10)) for c in cells]
    assert sorted(code)[:31] == [0] + [1 << k for k in range(30)]
