"""Trees deeper than the traversal's LDS stack (csrc/pt_kernels.hip `Stack`:
the first PT_STACK entries of a lane in LDS, the rest in a per-lane spill area
in global memory), for tests/test_deep_trees_host.py and
tests/test_gpu_deep_trees.py: the scenes, the rays, the camera and a float64
walk of a 4-wide tree with the kernel's stack discipline.  numpy only, seeded.

The walk proves that the inputs reach the spill code (how high each ray's
stack goes, how many node steps push p entries from height h); it is never
the reference of a device value."""
import os
import re
import types

import numpy as np

from dsgpuraytracing_amd import ptdump
from tests import bvh_check as bc
from tests.oracle_helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING = os.path.join(ROOT, "dsgpuraytracing_amd", "csrc", "pt_tuning.h")
TRI, SPHERE = 1, 0
FAR = np.float32(3.0e38)  # the traversal's "far": what tmax is clamped to
SCENE_SEED, RAY_SEED = 11, 5
N_CHAIN, N_RAYS = 96, 2048


def _define(name):
    m = re.search(rf"^\s*#\s*define\s+{name}\s+(\d+)", open(TUNING).read(), re.M)
    assert m, f"{name} is not defined in {TUNING}"
    return int(m.group(1))


PT_STACK = _define("PT_STACK")          # stack entries per lane in LDS
PT_STACK_MAX = _define("PT_STACK_MAX")  # deepest stack an upload accepts


def ragged_chain(n=N_CHAIN, seed=SCENE_SEED, sphere=False):
    """A scene dump (c1's, its primitives and nodes replaced): n layers at
    z = linspace(-0.5, 0.5, n) under a CHAIN tree (node k: left = leaf
    {prim k}, right = node k + 1).  Layer k is the triangle (x0, y0, z),
    (1, y0, z), (x0, 1, z) with x0, y0 uniform in [-1, 0.5], so a ray that
    travels -z at (x, y) enters leaf k's box iff x >= x0 and y >= y0: every ray
    pushes its own sequence of 0 .. 3 entries per 4-wide node.  Node boxes are
    the exact unions of the leaves below them.  sphere: the last (nearest)
    leaf is a sphere of radius 0.3 at (0, 0, 0.5) -- the scene is then not
    triangle-only, and the mixed leaf step runs deep."""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(-1.0, 0.5, n), rng.uniform(-1.0, 0.5, n)
    z = np.linspace(-0.5, 0.5, n)
    geom = np.stack([x0, y0, z, np.ones(n), y0, z, x0, np.ones(n), z], 1)
    ptype = np.full(n, TRI, np.int32)
    lo, hi = np.stack([x0, y0, z], 1), np.stack([np.ones(n), np.ones(n), z], 1)
    if sphere:
        ptype[-1] = SPHERE
        geom[-1] = [0, 0, 0.5, 0.3, 0, 0, 0, 0, 0]
        lo[-1], hi[-1] = [-0.3, -0.3, 0.2], [0.3, 0.3, 0.8]
    sub_lo = np.minimum.accumulate(lo[::-1])[::-1]  # box of primitives k ..
    sub_hi = np.maximum.accumulate(hi[::-1])[::-1]
    bb, info = [], []
    for k in range(n - 1):  # inner node k at index 2k, leaf k at 2k + 1, the next inner node at 2k + 2
        bb += [np.r_[sub_lo[k], sub_hi[k]], np.r_[lo[k], hi[k]]]
        info += [[k, n - k, 2 * k + 1, 2 * k + 2], [k, 1, -1, -1]]
    bb.append(np.r_[lo[n - 1], hi[n - 1]])
    info.append([n - 1, 1, -1, -1])
    d = dict(ptdump.read(golden("c1_default_64x64.scene.ptd")))
    d["prim_type"] = ptype
    d["prim_bsdf"] = np.zeros(n, np.int32)
    d["prim_orig"] = np.arange(n, dtype=np.int32)
    d["prim_geom"] = geom.reshape(-1)
    d["prim_norm"] = np.tile([0, 0, 1.0], (n, 3)).reshape(-1)
    d["node_bb"] = np.concatenate(bb).astype(np.float64)
    d["node_info"] = np.array(info, np.int64).reshape(-1)
    d["cam"] = camera(d["cam"])
    # c1's area light (at y = 1.49, facing -y: beside the layers, whose normals
    # are +z) moved above them, facing -z: the layers are lit from where the
    # camera sees them, and every shadow ray climbs back through the chain
    d["light_geom"] = np.array([0, 0, 3.0, 0, 0, -1.0, 0.6, 0, 0, 0, 0.8, 0], np.float64)
    return d


def chain_stack(n=N_CHAIN):
    """The worst-case stack of a near-first walk of the chain, however it is
    collapsed into wider nodes: a ray that enters every box holds every leaf
    but one of the last node's on its stack at once."""
    return n - 1


def camera(cam):
    """c1's camera record moved to (0, 0, 2.5), looking down -z (the
    orientation of tests/trace_helpers.py unit_cube_camera): whether camera
    rays go deep is decided here, not by c1's own camera."""
    cam = np.array(cam, np.float64)
    cam[0:3] = [0.0, 0.0, 2.5]
    cam[3:12] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    return cam


def deep_rays(m=N_RAYS, seed=RAY_SEED):
    """(m, 8) float32 rays as Device.trace_rays takes them: origins uniform in
    [-0.99, 0.99]^2 at z = 2, directions (+-0.05, +-0.05, -1) normalised, tmax
    at the far mark (the rays of test_hip_deep_bvh_stack_spill_vs_restatement)."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.99, 0.99, m), rng.uniform(-0.99, 0.99, m), np.full(m, 2.0)], 1)
    d = np.stack([rng.uniform(-0.05, 0.05, m), rng.uniform(-0.05, 0.05, m), -np.ones(m)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((m, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o, FAR, d
    return r


FAT_SCALE = 128.0  # the fat staircase's scene box is [0, 128.06]^3 (the longest needles end just past 128)
_FAT_CELL = FAT_SCALE / 1024


def fat_staircase():
    """tests/lbvh_scenes.py staircase_scene with leaves a ray can enter many
    of.  The staircase's Karras tree is one chain (reported stack 31), but its
    3e-4 triangles lie along the three axes: a straight line meets the boxes
    of at most one axis' ten, so no ray's stack goes past a dozen entries
    (measured over the read-back tree: 3 for the scene's own rays) -- the
    bound is beyond PT_STACK, the walk never is.  Here every triangle keeps
    its box CENTRE in its single-bit Morton cell (the builder codes the box
    centre), so the tree is the same chain, but spans its box [~0, 2 centre]
    along its axis, 0.8 cells across: all thirty boxes share the cube
    [0.5, 0.88]^3 cells at the origin, and a ray through that cube from the
    positive octant enters every link's far box before its three leaves.
    Scaled by 128 so that rays a unit long resolve the 0.1-wide triangles.
    Returns a tests/lbvh_scenes.py TinyScene."""
    from tests import lbvh_scenes as ls
    s = 3e-4 * FAT_SCALE
    g = [np.array([0, 0, 0, s, 0, 0, 0, s, 0.0])]
    # (every axis reaches both faces of the box; the triangle's normal is (0, -1, 0) rolled to
    # the needle's axis, at 55 degrees to the cube's diagonal: no ray below grazes its plane)
    corners = np.array([[-1, -1, -1], [1, 1, -1], [-1, -1, 1]], float)
    for j in range(10):
        for ax in range(3):
            q = np.full(3, 0.5 * _FAT_CELL)
            q[ax] = ((1 << j) + 0.5) * _FAT_CELL
            r = np.full(3, 0.4 * _FAT_CELL)
            r[ax] = q[ax] * (1 - 2.0 ** -10)
            g.append((q + np.roll(corners, ax, axis=1) * r).reshape(-1))
    g.append(np.array([FAT_SCALE, FAT_SCALE, FAT_SCALE, FAT_SCALE - s, FAT_SCALE, FAT_SCALE, FAT_SCALE, FAT_SCALE - s,
                       FAT_SCALE]))
    return ls.TinyScene("fat_staircase", np.full(len(g), TRI), np.array(g), 1.0, seed=32)


FAT_CUBE = (0.5 * _FAT_CELL * 1.05, 0.88 * _FAT_CELL * 0.98)  # inside every needle's box, with a margin


def fat_staircase_camera(cam):
    """c1's camera record with its centre of projection in the middle of the
    shared cube, looking down the cube's diagonal from the positive octant:
    every pixel's ray starts a unit away inside the scene box and runs through
    the shared cube."""
    cam = np.array(cam, np.float64)
    cam[0:3] = 0.5 * (FAT_CUBE[0] + FAT_CUBE[1])
    c2w = np.stack([np.array([1, -1, 0]) / np.sqrt(2), np.array([1, 1, -2]) / np.sqrt(6), np.array([1, 1, 1]) / np.sqrt(3)], 1)
    cam[3:12] = c2w.reshape(-1)
    return cam


def fat_staircase_rays(m=N_RAYS, seed=RAY_SEED):
    """(m, 8) float32 rays over fat_staircase, two kinds in turn (every group
    of 64 holds both): through a point of the shared cube from 1 .. 2 away in
    the positive octant (deep), and from the same origins at a point of the
    cube [0.4, 4]^3, past the needles' crossing (shallow)."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(FAT_CUBE[0], FAT_CUBE[1], (m, 3))
    u = np.abs(rng.normal(size=(m, 3))) + 0.3
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = tgt + u * rng.uniform(1.0, 2.0, (m, 1))
    far = rng.uniform(0.4, 4.0, (m, 3))
    odd = (np.arange(m) % 2 == 1)[:, None]
    d = np.where(odd, far, tgt) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((m, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o, FAR, d
    return r


def as_doubles(rays):
    """(o, d, tmax) in float64 of (n, 8) float32 rays: the values the kernel reads."""
    r = np.asarray(rays, np.float32).astype(np.float64)
    return np.ascontiguousarray(r[:, 0:3]), np.ascontiguousarray(r[:, 4:7]), np.ascontiguousarray(r[:, 3])


def float_arrays(prims):
    """What tests/trace_helpers.py brute_force_rays reads of a scene, rebuilt
    from a tree's float32 primitive records (read back or flattened) in the
    tree's order: the brute force then sees the very geometry the walk sees."""
    p = np.asarray(prims, np.float32).astype(np.float64)
    tri = bc.is_triangle(np.asarray(prims, np.float32))
    n = len(p)
    geom = np.zeros((n, 9))
    geom[:, 0:3] = p[:, 0:3]
    geom[tri, 3:6] = p[tri, 0:3] + p[tri, 4:7]
    geom[tri, 6:9] = p[tri, 0:3] + p[tri, 8:11]
    geom[~tri, 3] = p[~tri, 4]
    flags = np.ascontiguousarray(np.asarray(prims, np.float32)[:, 3]).view(np.int32)
    return types.SimpleNamespace(n_prims=n, prim_type=np.where(tri, TRI, SPHERE).astype(np.int32),
                                 prim_bsdf=(flags >> 1).astype(np.int32), prim_geom=geom.reshape(-1),
                                 prim_norm=np.tile([0, 0, 1.0], (n, 3)).reshape(-1))


def _test_prim(p, tri, o, d, tmax):
    """(hit, t) of primitive records p (k, 12) float64 against k rays, by the
    arithmetic of tests/trace_helpers.py brute_force_rays."""
    with np.errstate(all="ignore"):
        v0, e1, e2 = p[:, 0:3], p[:, 4:7], p[:, 8:11]
        pv = np.cross(d, e2)
        det = (pv * e1).sum(-1)
        tv = o - v0
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        tt = (qv * e2).sum(-1) / det
        ok_t = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 0)
        r = p[:, 4]
        b = (tv * d).sum(-1)
        disc = b * b - ((tv * tv).sum(-1) - r * r)
        sq = np.sqrt(disc)
        t1, t2 = -b - sq, -b + sq
        ts = np.where(t1 > 0, t1, t2)
        ok_s = (disc >= 0) & (ts > 0)
        t = np.where(tri, tt, ts)
        return np.where(tri, ok_t, ok_s) & (t < tmax), t


def stack_walk(nodes4, prims, o, d, tmax):
    """Nearest hit of every ray by a walk of the 4-wide tree (layouts:
    tests/bvh_check.py) with the kernel's stack discipline, in float64, all
    rays in lockstep: a node step slab-tests the four slots clipped to
    [0, tmax], continues with the nearest entered child and pushes the others
    farthest first; a leaf cursor tests its primitives, two per step, and
    shrinks tmax; a ray that entered nothing, or finished a leaf, pops.

    Returns {"hit", "t", "prim" (the tree's index), "peak": the highest stack
    height of each ray, "steps": (heights, 4) int64 -- steps[h, p] node steps
    that began with h entries on the stack and pushed p}.  A ray's stack goes
    past the LDS part iff its peak > PT_STACK."""
    nodes4 = np.asarray(nodes4, np.float32)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    m, n4 = len(o), len(nodes4)
    ref = bc.refs4(nodes4).astype(np.int64)
    lo, hi = bc.boxes4(nodes4)
    used = ~np.isinf(nodes4[:, 0:24]).reshape(n4, 6, 4).any(axis=1)
    p = np.asarray(prims, np.float32).astype(np.float64)
    tri = bc.is_triangle(np.asarray(prims, np.float32))
    cap = bc.recomputed_stack(nodes4) + 4
    stack = np.zeros((m, cap), np.int64)
    node, sp, peak = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    tmax = np.array(tmax, np.float64).copy()
    prim = np.full(m, -1, np.int64)
    active = np.ones(m, bool)
    steps = np.zeros((cap + 1, 4), np.int64)
    with np.errstate(all="ignore"):
        inv = 1.0 / d

    def pop(i):
        done = sp[i] == 0
        active[i[done]] = False
        i = i[~done]
        sp[i] -= 1
        node[i] = stack[i, sp[i]]

    while active.any():
        idx = np.flatnonzero(active)
        i = idx[node[idx] >= 0]
        if len(i):
            nd = node[i]
            with np.errstate(all="ignore"):
                t0 = (lo[nd] - o[i, None, :]) * inv[i, None, :]
                t1 = (hi[nd] - o[i, None, :]) * inv[i, None, :]
                tn = np.maximum(np.minimum(t0, t1).max(-1), 0.0)
                tf = np.minimum(np.maximum(t0, t1).min(-1), tmax[i, None])
                entered = used[nd] & (tn <= tf)
            order = np.argsort(np.where(entered, tn, np.inf), axis=1, kind="stable")
            cnt = entered.sum(1)
            np.add.at(steps, (sp[i], np.maximum(cnt - 1, 0)), 1)
            for j in (3, 2, 1):  # the farthest first
                k = cnt > j
                stack[i[k], sp[i[k]]] = ref[nd[k], order[k, j]]
                sp[i[k]] += 1
            peak[i] = np.maximum(peak[i], sp[i])
            go = cnt > 0
            node[i[go]] = ref[nd[go], order[go, 0]]
            pop(i[~go])
        i = idx[node[idx] < 0]
        if len(i):
            cur = ~node[i]
            first, count = cur >> 3, (cur & 7) + 1
            for j in (0, 1):
                k = count > j
                q = first[k] + j
                got, t = _test_prim(p[q], tri[q], o[i[k]], d[i[k]], tmax[i[k]])
                tmax[i[k][got]] = t[got]
                prim[i[k][got]] = q[got]
            more = count > 2
            node[i[more]] = ~(((first[more] + 2) << 3) | (count[more] - 3))
            pop(i[~more])
    hit = prim >= 0
    return {"hit": hit, "t": np.where(hit, tmax, 0.0), "prim": prim, "peak": peak, "steps": steps}


def coverage(walk, group=64):
    """The shares and counts the coverage conditions are stated in, of one
    stack_walk: {"deep": share of rays that peak at >= PT_STACK + 4,
    "shallow": at <= PT_STACK - 4, "rarest": the fewest node steps of any pair
    (height on entry in [PT_STACK - 4, PT_STACK + 2], pushes in {1, 2, 3}),
    "mixed": every consecutive group of 64 rays holds a ray that peaks above
    PT_STACK and one that stays <= PT_STACK - 3, "spilled": share of rays
    above PT_STACK}."""
    peak = walk["peak"]
    g = peak[:len(peak) // group * group].reshape(-1, group)
    pairs = walk["steps"][PT_STACK - 4:PT_STACK + 3, 1:4]
    return {"deep": float((peak >= PT_STACK + 4).mean()), "shallow": float((peak <= PT_STACK - 4).mean()),
            "rarest": int(pairs.min()), "pairs": int(pairs.size),
            "mixed": bool(((g > PT_STACK).any(1) & (g <= PT_STACK - 3).any(1)).all()),
            "spilled": float((peak > PT_STACK).mean())}
