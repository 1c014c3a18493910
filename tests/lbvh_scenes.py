"""Tiny scenes and rays for the structural tests of the GPU-built tree
(tests/test_gpu_lbvh_structure.py), and the host restatement of the upload's
double -> float primitive conversion.  numpy only, seeded."""
import numpy as np

from dsgpuraytracing_amd import ptdump
from tests import bvh_check as bc
from tests.oracle_helpers import golden

F = np.float32
TRI, SPHERE = 1, 0
N_RAYS = 2048


def device_prims(prim_type, prim_bsdf, geom, norm):
    """pt_upload_scene's conversion (scene_flatten.cpp `convert_prims`) of the caller's
    float64 primitives: (n, 12) float32 records and (n, 9) float32 normals."""
    g = np.asarray(geom, np.float64).reshape(-1, 9)
    t = np.asarray(prim_type).reshape(-1)
    b = np.asarray(prim_bsdf, np.int32).reshape(-1)
    n = len(t)
    p = np.zeros((n, 12), F)
    tri = t == TRI
    p[:, 0:3] = g[:, 0:3]
    p[:, 3] = ((b << 1) | tri.astype(np.int32)).astype(np.int32).view(F)
    p[tri, 4:7] = (g[tri, 3:6] - g[tri, 0:3])
    p[tri, 8:11] = (g[tri, 6:9] - g[tri, 0:3])
    p[~tri, 4] = g[~tri, 3]
    p[~tri, 5] = (g[~tri, 3] * g[~tri, 3])
    nn = np.asarray(norm, np.float64).reshape(-1, 9).astype(F)
    nn[~tri] = 0
    return p, nn


class TinyScene:
    """prim_type / geom (n, 9) as pt_scene holds them, `reach`: the distance
    scale of the ray origins aimed at each primitive, `targets`: the primitives
    rays are aimed at."""

    def __init__(self, name, prim_type, geom, reach, targets=None, seed=0):
        self.name = name
        self.prim_type = np.asarray(prim_type, np.int32)
        self.geom = np.asarray(geom, np.float64).reshape(-1, 9)
        self.n = len(self.prim_type)
        self.reach = np.broadcast_to(np.asarray(reach, np.float64), (self.n,)).copy()
        self.targets = np.arange(self.n) if targets is None else np.asarray(targets)
        rng = np.random.default_rng(1000 + seed)
        nr = rng.normal(size=(self.n, 3, 3))
        self.norm = (nr / np.linalg.norm(nr, axis=2, keepdims=True)).reshape(self.n, 9)
        self.prim_bsdf = np.zeros(self.n, np.int32)
        self.prims, self.norms = device_prims(self.prim_type, self.prim_bsdf, self.geom, self.norm)
        self._rays = None
        self._ref = None

    def dump(self):
        """A scene dump with these primitives under a one-leaf caller tree
        (uploads split it; the GPU build ignores it)."""
        d = dict(ptdump.read(golden("c1_default_64x64.scene.ptd")))
        d["prim_type"] = self.prim_type
        d["prim_bsdf"] = self.prim_bsdf
        d["prim_orig"] = np.arange(self.n, dtype=np.int32)
        d["prim_geom"] = self.geom.reshape(-1)
        d["prim_norm"] = self.norm.reshape(-1)
        lo, hi = self.bounds()
        d["node_bb"] = np.concatenate([lo, hi]).astype(np.float64)
        d["node_info"] = np.array([0, self.n, -1, -1], np.int64)
        return d

    def bounds(self):
        g, tri = self.geom, self.prim_type == TRI
        lo = np.where(tri[:, None], g.reshape(-1, 3, 3).min(1), g[:, 0:3] - np.abs(g[:, 3:4]))
        hi = np.where(tri[:, None], g.reshape(-1, 3, 3).max(1), g[:, 0:3] + np.abs(g[:, 3:4]))
        return lo.min(0), hi.max(0)

    def rays(self):
        """N_RAYS rays (o, d, max_t: float32 values held in float64, so the
        kernel and the reference see the same rays) aimed at triangle
        interiors and sphere caps from origins reach x [1.5, 3] away, at
        least 17 degrees off the surface.  Half of them end before their
        target (max_t)."""
        if self._rays is None:
            rng = np.random.default_rng(77)
            m = N_RAYS
            p = self.prims.astype(np.float64)
            pick = rng.choice(self.targets, m)
            tri = bc.is_triangle(self.prims)[pick]
            v0, e1, e2 = p[pick, 0:3], p[pick, 4:7], p[pick, 8:11]
            w = rng.normal(size=(m, 3))
            w /= np.linalg.norm(w, axis=1, keepdims=True)
            b = rng.dirichlet([2.0, 2.0, 2.0], m)
            nt = np.cross(e1, e2)
            nt /= np.maximum(np.linalg.norm(nt, axis=1, keepdims=True), 1e-300)
            tgt = np.where(tri[:, None], v0 + e1 * b[:, 1:2] + e2 * b[:, 2:3], v0 + w * p[pick, 4:5])
            nrm = np.where(tri[:, None], nt, w)
            tang = np.cross(nrm, rng.normal(size=(m, 3)))
            tang /= np.linalg.norm(tang, axis=1, keepdims=True)
            c = rng.uniform(0.3, 1.0, m) * np.where(tri, rng.choice([-1.0, 1.0], m), 1.0)
            u = nrm * c[:, None] + tang * np.sqrt(1.0 - c * c)[:, None]
            L = self.reach[pick] * rng.uniform(1.5, 3.0, m)
            o = (tgt + u * L[:, None]).astype(F).astype(np.float64)
            d = tgt - o
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F).astype(np.float64)
            max_t = (L * rng.uniform(0.3, 1.7, m)).astype(F).astype(np.float64)
            self._rays = (o, d, max_t)
        return self._rays

    def reference(self):
        """brute_force over the caller-order float primitives, computed once."""
        if self._ref is None:
            self._ref = bc.brute_force(self.prims, *self.rays())
        return self._ref


def _tris(v0, rng, lo=0.1, hi=0.3):
    n = len(v0)
    e = rng.normal(size=(n, 2, 3))
    e *= (rng.uniform(lo, hi, (n, 2, 1)) / np.linalg.norm(e, axis=2, keepdims=True))
    return np.concatenate([v0, v0 + e[:, 0], v0 + e[:, 1]], axis=1)


def random_scene(n, seed=0):
    """Random small triangles (edges 0.1 .. 0.3) in the unit cube."""
    rng = np.random.default_rng([seed, n, 1])
    return TinyScene(f"random{n}", np.full(n, TRI), _tris(rng.uniform(0.15, 0.85, (n, 3)), rng), 1.0, seed=n)


def coincident_scene(n):
    """Triangles of different shapes whose boxes share one centre: their Morton
    codes are equal, the Karras tree is built from the index bits alone.  (For
    n >= 2 primitive 0 is a small triangle elsewhere: the centre of a scene
    of concentric boxes alone is the scene's, 0.5 after normalisation, a cell
    boundary that rounding would straddle.)"""
    rng = np.random.default_rng([n, 2])
    g = _tris(np.zeros((n, 3)), rng).reshape(n, 3, 3)
    g += (np.array([0.37, 0.41, 0.43]) - 0.5 * (g.min(1) + g.max(1)))[:, None, :]
    if n >= 2:
        g[0] = _tris(np.array([[0.9, 0.95, 0.85]]), rng, 0.02, 0.04).reshape(3, 3)
    return TinyScene(f"coincident{n}", np.full(n, TRI), g.reshape(n, 9), 1.0, seed=n)


def coplanar_scene(n):
    """n triangles side by side in the plane z = 0.25: the scene has no extent
    in z, and the Morton normalisation divides by zero there."""
    rng = np.random.default_rng([n, 3])
    k = int(np.ceil(np.sqrt(n)))
    cell = np.stack([np.arange(n) % k, np.arange(n) // k], 1) / k
    g = np.zeros((n, 3, 3))
    g[:, :, 2] = 0.25
    corner = rng.uniform(0.05, 0.2, (n, 3, 2)) / k
    g[:, 0, :2] = cell + corner[:, 0]
    g[:, 1, :2] = cell + corner[:, 1] + [0.6 / k, 0.1 / k]
    g[:, 2, :2] = cell + corner[:, 2] + [0.2 / k, 0.6 / k]
    return TinyScene(f"coplanar{n}", np.full(n, TRI), g.reshape(n, 9), 1.0, seed=n)


def clusters_scene(n):
    """One triangle spanning the scene and n - 1 triangles of 2e-5 .. 4e-5 in
    two clusters 1e-4 across at opposite corners: most of the tree lives in
    two Morton cells.  Rays at the clusters start 3e-4 .. 6e-4 away: from
    across the scene a float ray cannot resolve a 3e-5 triangle."""
    rng = np.random.default_rng([n, 4])
    m = n - 1
    centre = np.where((np.arange(m) % 2 == 0)[:, None], [0.1, 0.12, 0.14], [0.9, 0.88, 0.86])
    tiny = _tris(centre + rng.uniform(-4e-5, 4e-5, (m, 3)), rng, 2e-5, 4e-5)
    span = np.array([[0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0.5, 1.0]])
    reach = np.concatenate([[1.0], np.full(m, 2e-4)])
    return TinyScene(f"clusters{n}", np.full(n, TRI), np.concatenate([span, tiny]), reach, seed=n)


def mixed_scene(n):
    """Half spheres, half triangles, and (n >= 3) a sphere of radius 1e-9 centred
    on the maximum corner of the rest: its normalised centre rounds to 1, which
    the Morton code maps to 0 (the reference's quirk).  No ray is aimed at it."""
    rng = np.random.default_rng([n, 5])
    ns = (n + 1) // 2
    t = np.concatenate([np.full(ns, SPHERE), np.full(n - ns, TRI)])
    g = np.zeros((n, 9))
    g[:ns, 0:3] = rng.uniform(0.15, 0.85, (ns, 3))
    g[:ns, 3] = rng.uniform(0.03, 0.1, ns)
    if n > ns:
        g[ns:] = _tris(rng.uniform(0.15, 0.85, (n - ns, 3)), rng)
    targets = np.arange(n)
    if n >= 3:
        rest = TinyScene("", t[1:], g[1:], 1.0)
        g[0, 0:3] = rest.bounds()[1]
        g[0, 3] = 1e-9
        targets = targets[1:]
    perm = rng.permutation(n)  # spheres and triangles interleaved in the caller's order
    inv = np.argsort(perm)
    return TinyScene(f"mixed{n}", t[perm], g[perm], 1.0, targets=np.sort(inv[targets]), seed=n)


def morton_cells(sc):
    """The builder's Morton cell (x, y, z in 0..1023) of each primitive,
    restated in float32 (k_morton and build_gpu_bvh's scene box)."""
    lo, hi = sc.bounds()
    smin = lo.astype(F)
    smin = np.where(smin.astype(np.float64) > lo, np.nextafter(smin, F(-np.inf)), smin)
    ext = (hi - lo).astype(F)
    p = sc.prims
    tri = bc.is_triangle(p)[:, None]
    z = np.zeros_like(p[:, 4:7])
    mn = np.minimum(np.minimum(z, p[:, 4:7]), p[:, 8:11])
    mx = np.maximum(np.maximum(z, p[:, 4:7]), p[:, 8:11])
    c = np.where(tri, p[:, 0:3] + F(0.5) * (mn + mx), p[:, 0:3])
    with np.errstate(all="ignore"):
        x = (c - smin) / ext
    x = np.where(np.isnan(x) | (x < 0) | (x >= 1), F(0), x)
    return np.clip(x * F(1024), 0, 1023).astype(np.int64)


def staircase_scene():
    """One 3e-4 triangle per single-bit 30-bit Morton code -- centred in cell
    2^k of one axis and cell 0 of the others -- plus code 0 and, to pin the
    scene box to the unit cube, one at the far corner: 32 triangles whose
    Karras tree is one chain, the deepest 30-bit codes allow."""
    s = 3e-4
    cells = [(0, 0, 0)] + [tuple((1 << j) if a == ax else 0 for a in range(3)) for j in range(10) for ax in range(3)]
    g = []
    for cx in cells[1:]:
        c = (np.array(cx) + 0.5) / 1024
        g.append(np.concatenate([c + [-s / 2, -s / 2, 0], c + [s / 2, -s / 2, 0], c + [-s / 2, s / 2, 0]]))
    g.insert(0, np.array([0, 0, 0, s, 0, 0, 0, s, 0.0]))
    g.append(np.array([1, 1, 1, 1 - s, 1, 1, 1, 1 - s, 1.0]))
    return TinyScene("staircase", np.full(len(g), TRI), np.array(g), 2e-3, seed=31)


FAMILIES = {"random": random_scene, "coincident": coincident_scene, "coplanar": coplanar_scene,
            "clusters": clusters_scene, "mixed": mixed_scene}
RANDOM_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 257]
OTHER_SIZES = [1, 4, 5, 7, 65]
_cache = {}


def scene(family, n=None):
    key = (family, n)
    if key not in _cache:
        _cache[key] = staircase_scene() if family == "staircase" else FAMILIES[family](n)
    return _cache[key]


def all_scenes():
    out = [("random", n) for n in RANDOM_SIZES]
    out += [(f, n) for f in ("coincident", "coplanar", "clusters", "mixed") for n in OTHER_SIZES]
    return out + [("staircase", None)]
