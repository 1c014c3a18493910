"""Scenes built from scratch for the shading round of the render kernel.

Every parity fixture under tests/golden/ descends from one Cornell box: one
light (plus, in three of them, the environment light), white mirror / glass,
ior 1.45, specular BSDFs on spheres only, tables of 8 entries.  The scenes
here are PTDUMP dicts (plain numpy, no GPU, no reference) over ONE small room
that vary what the shading state machine branches on:

  * light lists of 0 .. 12 lights of every kind and in several orders (the
    NEE cursor, emit_last, SH_RESUME / SH_FOLLOW / SH_STORE, the LDS / global
    table boundary at 8 lights, ENV x GTAB);
  * material tables of 8, 16 and 20 BSDFs with three distinct channel values
    in reflectance, transmittance and emission, ior in {0.8, 1.0, 1.2, 1.45,
    2.4}, every BSDF type on a triangle and on a sphere, diffuse albedos of 0
    (pterm == 1), 0.05 and (1.3, 1.2, 1.1) (f = a / pi: pterm is about 0.62,
    a bright wall, not the clamp); pterm == 0, the fmaxf(1 - illum(f), 0)
    clamp, is reached on the mirrors and glass (f = a / cos);
  * the 8-bit fields of the kernel's packed cursor at their limits:
    ns_area_light = 255 and max_depth = 254.

The room: x, y in [-1, 1], z in [-1, 2.7]; floor, back, left, right and front
walls, and a ceiling over the back part only (z < 0.2), so that directional,
hemisphere and environment light reach the inside through the open part --
12 wall triangles.  Five spheres stand in the back, four free-standing quads
hang in front of them (25 primitives), all under ONE root leaf: the upload
splits it (oversize leaf), the restatement tests every primitive -- no box
test decides anything on the CPU side.  Lights are kept away from surfaces
and from grazing directions; point lights float in free space.

Primitives carry a slot name; a material table maps slots to BSDF indices.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from dsgpuraytracing_amd import ptdump

HERE = os.path.dirname(os.path.abspath(__file__))

DIFFUSE, MIRROR, REFRACTION, GLASS, EMISSION = range(5)
L_DIR, L_HEMI, L_POINT, L_AREA, L_ENV = range(5)

# the per-sample comparison tolerance of tests/test_gpu_shading_sweep.py
# (SURVEY.md §8(c) criterion 2 on samples): |a - b| <= TOL * max(1, |b|)
TOL = 1e-3


def within(a, b):
    """Per sample (last axis = RGB): a within TOL * max(1, |b|) of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max(axis=-1) <= TOL * np.maximum(1.0, np.abs(b).max(axis=-1))


# ------------------------------------------------------------------ geometry
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _quad(slot_a, slot_b, p0, p1, p2, p3):
    return [("tri", (p0, p1, p2), slot_a), ("tri", (p0, p2, p3), slot_b)]


def _panel(slot_a, slot_b, centre, half_u, half_v):
    c, u, v = (np.asarray(x, np.float64) for x in (centre, half_u, half_v))
    return _quad(slot_a, slot_b, c - u - v, c + u - v, c + u + v, c - u + v)


Z0, Z1, ZC = -1.0, 2.7, 0.2  # back wall, front wall, where the ceiling ends


def room_prims(spheres=True, sph_d_dx=0.0):
    P = lambda x, y, z: np.array([x, y, z], np.float64)
    prims = []
    prims += _quad("floor", "floor", P(-1, -1, Z0), P(1, -1, Z0), P(1, -1, Z1), P(-1, -1, Z1))
    prims += _quad("ceil_a", "ceil_b", P(-1, 1, Z0), P(1, 1, Z0), P(1, 1, ZC), P(-1, 1, ZC))
    prims += _quad("back_a", "back_b", P(-1, -1, Z0), P(1, -1, Z0), P(1, 1, Z0), P(-1, 1, Z0))
    prims += _quad("left", "left", P(-1, -1, Z0), P(-1, -1, Z1), P(-1, 1, Z1), P(-1, 1, Z0))
    prims += _quad("right", "right", P(1, -1, Z0), P(1, -1, Z1), P(1, 1, Z1), P(1, 1, Z0))
    prims += _quad("front", "front", P(-1, -1, Z1), P(1, -1, Z1), P(1, 1, Z1), P(-1, 1, Z1))
    if spheres:
        prims += [("sph", (P(-0.66, -0.70, -0.50), 0.29), "sphA"),
                  ("sph", (P(0.02, -0.68, -0.58), 0.31), "sphB"),
                  ("sph", (P(0.67, -0.69, -0.44), 0.30), "sphC"),
                  ("sph", (P(-0.40 + sph_d_dx, 0.33, -0.55), 0.27), "sphD"),
                  ("sph", (P(0.52, 0.40, -0.60), 0.28), "sphE")]
    # free-standing panels, each turned away from the axes and from the camera
    prims += _panel("quad1_a", "quad1_b", P(-0.62, -0.12, 0.20), P(0.25, 0.02, 0.10), P(-0.03, 0.26, 0.02))
    prims += _panel("quad2_a", "quad2_b", P(0.63, -0.15, 0.25), P(0.19, -0.03, -0.10), P(0.02, 0.22, -0.03))
    prims += _panel("quad3_a", "quad3_b", P(0.05, 0.05, 0.10), P(0.22, 0.03, 0.05), P(-0.02, 0.20, 0.06))
    prims += _panel("quad4_a", "quad4_b", P(0.08, 0.70, 0.00), P(0.31, 0.02, -0.04), P(0.01, 0.17, 0.12))
    return prims


def camera(eye=(0.04, 0.06, 1.6), target=(0.0, -0.05, -1.0), screen=1.5):
    """pt_camera values (+ hFov, vFov as the dumps carry them).  Rays start on
    the screen plane one unit behind `eye` and pass through it."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = _unit(eye - target)
    x = _unit(np.cross([0.0, 1.0, 0.0], z))
    y = np.cross(z, x)
    c2w = np.stack([x, y, z], axis=1)  # columns: the camera's axes in world space
    fov = float(np.degrees(2 * np.arctan(screen / 2)))
    return np.concatenate([eye, c2w.reshape(-1), [screen, screen, 1.0, fov, fov]])


# ------------------------------------------------------------------ materials
def bsdf(kind, a=(0, 0, 0), t=(0, 0, 0), e=(0, 0, 0), ior=0.0):
    return (kind, [*a, *t, *e, ior, 0.0, 0.0])


def _table(entries):
    """entries: [(bsdf, [slots])] -> (bsdf list, slot -> index)."""
    slots = {}
    for i, (_, ss) in enumerate(entries):
        for s in ss:
            assert s not in slots, s
            slots[s] = i
    return [b for b, _ in entries], slots


def plain_table():
    """8 BSDFs, mostly diffuse: what the light-list scenes are shaded with."""
    return _table([
        (bsdf(DIFFUSE, (0.72, 0.68, 0.60)), ["floor", "front"]),
        (bsdf(DIFFUSE, (0.63, 0.065, 0.05)), ["left"]),
        (bsdf(DIFFUSE, (0.14, 0.45, 0.091)), ["right"]),
        (bsdf(DIFFUSE, (0.70, 0.72, 0.75)), ["back_a", "back_b", "ceil_a", "ceil_b"]),
        (bsdf(DIFFUSE, (0.30, 0.40, 0.80)), ["sphA", "sphD", "quad1_a", "quad1_b", "quad3_a", "quad3_b"]),
        (bsdf(MIRROR, (0.90, 0.80, 0.70)), ["sphB", "quad2_a", "quad2_b"]),
        (bsdf(GLASS, (0.90, 0.95, 0.85), (0.80, 0.90, 0.70), ior=1.45), ["sphC", "sphE"]),
        (bsdf(DIFFUSE, (0.80, 0.60, 0.20)), ["quad4_a", "quad4_b"]),
    ])


_FULL16 = [
    (bsdf(DIFFUSE, (0.72, 0.68, 0.60)), ["floor", "front"]),
    (bsdf(DIFFUSE, (0.05, 0.05, 0.05)), ["ceil_a"]),
    (bsdf(DIFFUSE, (1.30, 1.20, 1.10)), ["back_a"]),                # illum(a / pi) < 1 still; bright
    (bsdf(DIFFUSE, (0.63, 0.065, 0.05)), ["left"]),
    (bsdf(DIFFUSE, (0.14, 0.45, 0.091)), ["right"]),
    (bsdf(DIFFUSE, (0.0, 0.0, 0.0)), ["sphA"]),                    # pterm == 1
    (bsdf(MIRROR, (0.95, 0.70, 0.40)), ["sphB"]),
    (bsdf(REFRACTION, (0.20, 0.30, 0.40), (0.90, 0.60, 0.80), ior=1.45), ["sphC"]),
    (bsdf(GLASS, (0.85, 0.90, 0.60), (0.70, 0.95, 0.80), ior=0.8), ["sphD"]),  # TIR on entry at sin > 0.8
    (bsdf(EMISSION, e=(1.50, 0.90, 0.30)), ["sphE"]),
    (bsdf(MIRROR, (0.60, 0.90, 0.80)), ["quad1_a"]),
    (bsdf(REFRACTION, (0.30, 0.20, 0.10), (0.80, 0.90, 0.50), ior=1.2), ["quad2_a"]),
    (bsdf(GLASS, (0.90, 0.80, 0.70), (0.75, 0.85, 0.95), ior=1.0), ["quad3_a"]),  # ratio 1, Fresnel 0
    (bsdf(GLASS, (0.70, 0.90, 0.80), (0.90, 0.70, 0.60), ior=2.4), ["quad3_b"]),
    (bsdf(EMISSION, e=(0.40, 1.10, 0.70)), ["quad4_a"]),
    (bsdf(DIFFUSE, (0.40, 0.60, 0.70)), ["ceil_b"]),
]
# what the second triangle of a panel / wall uses: in the 16-entry table its
# sibling's entry, in the 20-entry table an entry of its own (indices 16 .. 19)
_SIBLING = {"quad1_b": "quad1_a", "quad2_b": "quad2_a", "quad4_b": "quad4_a", "back_b": "back_a"}
_EXTRA4 = [
    (bsdf(MIRROR, (0.90, 0.50, 0.70)), ["quad1_b"]),
    (bsdf(REFRACTION, (0.10, 0.20, 0.30), (0.50, 0.80, 0.90), ior=2.4), ["quad2_b"]),
    (bsdf(EMISSION, e=(0.90, 0.30, 1.20)), ["quad4_b"]),
    (bsdf(DIFFUSE, (0.50, 0.20, 0.60)), ["back_b"]),
]


def full16_table():
    """Exactly 16 BSDFs (the largest table the LDS copy holds), all used."""
    return _table([(b, ss + [k for k, v in _SIBLING.items() if v in ss]) for b, ss in _FULL16])


def full20_table():
    """20 BSDFs (global-table kernel variant), all used; indices 16 .. 19 are
    read by primitives of their own."""
    return _table(_FULL16 + _EXTRA4)


# ------------------------------------------------------------------ lights
def _light(kind, rad, pos=(0, 0, 0), d=(0, 0, 0), dimx=(0, 0, 0), dimy=(0, 0, 0), area=0.0):
    return dict(type=kind, rad=tuple(rad), geom=[*pos, *d, *dimx, *dimy], area=float(area))


def area_light(rad, pos, d, dimx, dimy):
    area = float(np.linalg.norm(dimx) * np.linalg.norm(dimy))
    return _light(L_AREA, rad, pos, _unit(d), dimx, dimy, area)


def point_light(rad, pos):
    return _light(L_POINT, rad, pos)


def dir_light(rad, to_light):
    return _light(L_DIR, rad, d=_unit(to_light))  # sample_L returns dirToLight as stored


def hemi_light(rad):
    return _light(L_HEMI, rad)


def env_light():
    return _light(L_ENV, (0, 0, 0))


A0 = area_light((6.0, 1.0, 0.2), (-0.30, 0.90, -0.35), (0, -1, 0), (0.5, 0, 0), (0, 0, 0.4))
A1 = area_light((0.3, 4.0, 1.0), (0.92, 0.15, 0.70), (-0.98, -0.15, -0.10), (0, 0.4, 0), (0, 0, 0.5))
A2 = area_light((1.0, 0.8, 6.0), (-0.92, -0.20, 1.00), (0.97, 0.10, -0.20), (0, 0.3, 0), (0, 0, 0.4))
A3 = area_light((4.0, 3.0, 0.6), (0.20, 0.85, 1.20), (0.10, -0.99, -0.05), (0.4, 0, 0), (0, 0, 0.3))
P0 = point_light((1.2, 0.4, 0.2), (0.35, 0.50, 0.80))
P1 = point_light((0.2, 0.9, 1.1), (-0.50, 0.10, 1.30))
P2 = point_light((0.9, 0.7, 0.2), (0.60, -0.30, 1.50))
P3 = point_light((1.0, 0.3, 0.9), (-0.20, 0.60, 0.65))
D0 = dir_light((0.9, 0.7, 0.3), (0.25, 0.85, 0.45))
D1 = dir_light((0.3, 0.5, 0.9), (-0.30, 0.80, 0.60))
H0 = hemi_light((0.2, 0.35, 0.6))
# built to contribute nothing: an area light above the room facing up
# (cosTheta > 0 from every point of the room: sample_L returns black, the
# kernel's lit == false), and a point light behind the back wall (it emits a
# shadow ray from every surface that faces it; every one is occluded)
AWAY = area_light((4.0, 3.0, 2.0), (0.20, 1.50, 0.30), (0, 1, 0), (0.5, 0, 0), (0, 0, 0.4))
OCCLUDED = point_light((3.0, 2.0, 1.0), (0.10, -0.20, -1.80))
ENV = env_light()

L8 = [A0, P0, D0, A1, P1, H0, A2, P2]
LIGHT_LISTS = {
    "L0": [],
    "L1": [A0],
    "L2_point_area": [P0, A0],
    "L2_area_point": [A0, P0],
    "L2_area_occluded": [A0, OCCLUDED],   # the last light emits and is shadowed
    "L2_area_away": [A0, AWAY],           # the last light never emits: SH_RESUME, then nothing
    "L3": [A0, A1, H0],
    "L5": [D0, A0, P0, H0, A1],
    "L8": L8,                             # the largest list the LDS copy holds
    "L9": L8 + [P3],                      # differs from L8 only in the ninth light: global tables
    "L9_env": L8 + [ENV],                 # ENV x GTAB
    "L12": L8 + [A3, AWAY, P3, D1],
}
NOTHING = (AWAY, OCCLUDED)  # by identity


def contributes_nothing(light):
    return any(light is n for n in NOTHING)


# ------------------------------------------------------------------ assembly
def env_map():
    d = ptdump.read(os.path.join(HERE, "golden", "env_sky_64x32.rgb.ptd"))
    h, w, _ = (int(v) for v in d["shape"])
    return np.array([h, w], np.int64), d["rgb"].astype(np.float32)


def assemble(prims, table, lights, cam=None):
    bsdfs, slots = table
    n = len(prims)
    ptype = np.zeros(n, np.int32)
    pbsdf = np.zeros(n, np.int32)
    geom = np.zeros((n, 9))
    norm = np.zeros((n, 9))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, (kind, data, slot) in enumerate(prims):
        pbsdf[i] = slots[slot]
        if kind == "tri":
            v = np.stack(data)
            ptype[i] = 1
            geom[i] = v.reshape(-1)
            norm[i] = np.tile(_unit(np.cross(v[1] - v[0], v[2] - v[0])), 3)
            lo, hi = np.minimum(lo, v.min(0)), np.maximum(hi, v.max(0))
        else:
            c, r = data
            geom[i, :3], geom[i, 3] = c, r
            lo, hi = np.minimum(lo, c - r), np.maximum(hi, c + r)
    assert sorted(set(pbsdf.tolist())) == list(range(len(bsdfs))), "every BSDF entry is used by a primitive"
    d = {
        "cam": camera() if cam is None else cam,
        "bsdf_type": np.array([b[0] for b in bsdfs], np.int32),
        "bsdf_params": np.array([b[1] for b in bsdfs], np.float32).reshape(-1),
        "light_type": np.array([l["type"] for l in lights], np.int32),
        "light_rad": np.array([l["rad"] for l in lights], np.float32).reshape(-1),
        "light_geom": np.array([l["geom"] for l in lights], np.float64).reshape(-1),
        "light_area": np.array([l["area"] for l in lights], np.float32),
        "prim_type": ptype, "prim_bsdf": pbsdf, "prim_orig": np.arange(n, dtype=np.int32),
        "prim_geom": geom.reshape(-1), "prim_norm": norm.reshape(-1),
        "node_bb": np.concatenate([lo, hi]), "node_info": np.array([0, n, -1, -1], np.int64),
    }
    if any(l["type"] == L_ENV for l in lights):
        d["env_shape"], d["env_rgb"] = env_map()
    return d


LIGHT_LISTS_ALL = {**LIGHT_LISTS, "L2_area_area": [A0, A1]}  # + the ns_area_light = 255 scene's list


def light_scene(name):
    return assemble(room_prims(), plain_table(), LIGHT_LISTS_ALL[name])


MATERIAL_LIGHTS = [A0, P0, H0]


def material_scene(table="full16", spheres=True):
    tab = {"full16": full16_table, "full20": full20_table, "plain": plain_table}[table]()
    prims = room_prims(spheres)
    if not spheres:  # the triangle-only room: the tables' sphere entries go
        used = sorted({tab[1][s] for _, _, s in prims})
        remap = {b: i for i, b in enumerate(used)}
        tab = ([tab[0][b] for b in used], {s: remap[b] for s, b in tab[1].items() if b in remap})
    return assemble(prims, tab, MATERIAL_LIGHTS)


def env_middle_scene():
    """The environment light SECOND of three lights (PathTracer::set_scene
    always pushes it last; trace_ray samples whatever order the list has).
    Sphere D stands 0.03 further right than in the room: with the room's own
    sphere, sample 2 of pixel (9, 24) at seed 41 sends a bounce ray within
    5e-6 of the sphere's silhouette -- fp32 hits it, fp64 misses it -- and
    that one sample carries 0.26% of this dim scene's mean (traced with
    RS_DEBUG_PIXEL and PT_DEBUG_PIXEL: same draws, same bounce direction,
    depth-2 hit sphere vs right wall)."""
    return assemble(room_prims(sph_d_dx=0.03), plain_table(), [A0, ENV, P0])


ENV_MIDDLE_ARGS = (env_middle_scene, 32, 32, 4, 1, 41)


def mirror_box_scene():
    """max_depth = 254: a sealed 2 x 2 x 2 box of albedo-1 mirrors (f = 1 / cos:
    pterm == 0, the throughput stays 1), one small diffuse patch floating over
    the floor and a point light over it.  A path is black until it finds the
    patch (0.17% of the surface): most run hundreds of bounces."""
    P = lambda x, y, z: np.array([x, y, z], np.float64)
    prims = []
    for a, b, c, d in (((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1)), ((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)),
                       ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), ((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)),
                       ((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1)), ((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1))):
        prims += _quad("wall", "wall", P(*a), P(*b), P(*c), P(*d))
    prims += _panel("patch", "patch", P(0.31, -0.90, -0.27), P(0.085, 0.0, 0.011), P(-0.011, 0.0, 0.085))
    table = _table([(bsdf(MIRROR, (1, 1, 1)), ["wall"]), (bsdf(DIFFUSE, (0.9, 0.7, 0.5)), ["patch"])])
    lights = [point_light((3.0, 2.0, 1.0), (0.22, 0.35, -0.15))]
    return assemble(prims, table, lights, camera(eye=(0.07, 0.11, -0.2), target=(0.3, -0.4, -1.0)))


# name -> (scene dict builder, W, H, max_depth, ns_area_light, seed)
def _cases():
    c = {}
    for i, name in enumerate(LIGHT_LISTS):
        # -l 2: an area light's second sample resumes at the same light (ls), -l 1 elsewhere
        c[name] = (functools.partial(light_scene, name), 32, 32, 4, 2 if name in ("L3", "L9", "L12") else 1, 11 + i)
    c["M16"] = (functools.partial(material_scene, "full16"), 32, 32, 6, 1, 31)
    c["M20"] = (functools.partial(material_scene, "full20"), 32, 32, 6, 1, 32)
    c["NS255"] = (functools.partial(light_scene, "L2_area_area"), 8, 8, 2, 255, 33)
    c["DEPTH254"] = (mirror_box_scene, 8, 8, 254, 1, 34)
    return c


CASES = _cases()
N_SAMPLES = 6   # per-sample parity: launches of spp = 1 with sample_base = 0 .. 5
GROUP_SPP = 5   # grouped parity


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


def write_scene(d, directory, name):
    path = os.path.join(str(directory), f"{name}.scene.ptd")
    ptdump.write(path, d)
    return path


def pixel_grid(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.reshape(-1).astype(np.int32), ys.reshape(-1).astype(np.int32)


def ref_samples(restate, path, name, n=N_SAMPLES, scene_args=None):
    """(H, W, n, 3): the restatement's radiance of samples 0 .. n-1 of every pixel."""
    _, w, h, m, l, seed = CASES[name] if scene_args is None else scene_args
    xs, ys = pixel_grid(w, h)
    return restate.pixel_samples(path, w, h, n, xs, ys, depth=m, ns_area_light=l, seed=seed).reshape(h, w, n, 3)


def sum_in_order(samples):
    """The pixel value of a render of samples.shape[2] spp: the float32 sum in
    sample order times (float)(1 / spp), as raytrace_pixel averages."""
    acc = np.zeros(samples.shape[:2] + (3,), np.float32)
    for i in range(samples.shape[2]):
        acc = acc + samples[:, :, i].astype(np.float32)
    return acc * np.float32(1.0 / samples.shape[2])


def sum_in_groups(samples, group):
    """The pixel value of a render whose work slots hold `group` samples: each
    group's float32 sum in sample order, the group sums added in group order,
    times (float)(1 / spp).  group = 1 is sum_in_order."""
    n = samples.shape[2]
    acc = np.zeros(samples.shape[:2] + (3,), np.float32)
    for g0 in range(0, n, group):
        part = np.zeros_like(acc)
        for i in range(g0, min(g0 + group, n)):
            part = part + samples[:, :, i].astype(np.float32)
        acc = acc + part
    return acc * np.float32(1.0 / n)


def first_hits(restate, path, d, w, h):
    """Primitive index (-1: none) and BSDF index seen first through every
    pixel's centre, by the restatement's intersection."""
    cam = d["cam"]
    pos, c2w = cam[:3], cam[3:12].reshape(3, 3)
    xs, ys = pixel_grid(w, h)
    sp = np.stack([-((xs + 0.5) / w - 0.5) * cam[12] / cam[14], -((ys + 0.5) / h - 0.5) * cam[13] / cam[14],
                   np.ones(len(xs))], axis=1)
    o = sp @ c2w.T + pos
    dr = -(sp @ c2w.T)
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    hit, t, prim, nrm, _ = restate.intersect(path, o.reshape(-1), dr.reshape(-1), np.full(len(xs), 1e30))
    prim = np.where(hit == 1, prim, -1)
    b = np.where(prim >= 0, d["prim_bsdf"][np.maximum(prim, 0)], -1)
    return prim.reshape(h, w), b.reshape(h, w), dr.reshape(h, w, 3), nrm.reshape(h, w, 3)


_REF = {}


def reference(restate, directory, name):
    """(scene file, the restatement's samples) of a case; computed once per
    test session and shared, never modified."""
    if name not in _REF:
        path = write_scene(scene(name), directory, name)
        ref = ref_samples(restate, path, name, max(N_SAMPLES, GROUP_SPP))
        ref.setflags(write=False)
        _REF[name] = (path, ref)
    return _REF[name]
