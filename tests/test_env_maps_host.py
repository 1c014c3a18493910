"""The hard environment maps of tests/env_maps.py do what they claim (CPU only).

Before tests/test_gpu_env_maps.py asks the device anything: the host body of
the search (pt_env_search_check) is exact on every family with the uniform and
the targeted queries and takes the window-halving path on every family that
has windows to halve; the numpy reference searches the library's own tables
(pt_env_tables) with lower_bound semantics, so bad == 0 makes it one with the
host search; the targeted queries reach every row, the dimmest texels and the
CDF's exact ties; the special directions land in the wrap branch they were
aimed at; the render scenes are finite, repeatable and really lit by the map;
and the float32 evaluation of the reference's own formulas -- the floor no
fp32 kernel can be asked to beat -- stays inside the GPU test's tolerances.
"""
import ctypes

import numpy as np
import pytest

from dsgpuraytracing_amd import native
from tests import env_maps as E
from tests import shading_scenes as S


def _search_check(name, u1, u2):
    rgb = np.ascontiguousarray(E.env_map(name))
    h, w, _ = rgb.shape
    u1, u2 = np.ascontiguousarray(u1, np.float32), np.ascontiguousarray(u2, np.float32)
    longw = ctypes.c_int64(0)
    bad = native.lib().pt_env_search_check(rgb.ctypes.data, w, h, len(u1), u1.ctypes.data, u2.ctypes.data,
                                           ctypes.byref(longw))
    assert bad >= 0, native.lib().pt_last_error()
    return bad, longw.value


@pytest.mark.parametrize("name", E.FAMILIES)
def test_maps_are_as_described(name):
    m = E.env_map(name)
    w, h = E.SIZES[name]
    assert m.shape == (h, w, 3) and m.dtype == np.float32 and np.isfinite(m).all() and (m >= 0).all()
    assert np.array_equal(m, E.env_map.__wrapped__(name))  # deterministic
    p_theta, p_phi, pdf = E.ref(name).p_theta, E.ref(name).p_phi, E.ref(name).pdf
    assert (np.diff(p_theta) >= 0).all() and (np.diff(p_phi, axis=1) >= 0).all() and (pdf >= 0).all()
    if name in ("sun_seam", "sun_poles", "wide"):
        assert m.max() == E.SUN and np.median(m) < 0.25


@pytest.mark.parametrize("name", E.FAMILIES)
def test_host_search_is_exact_and_halves(name):
    """bad == 0: the host record_lower_bound returns std::lower_bound's index and
    pair on every query; the numpy reference is np.searchsorted(..., 'left') over
    the same float32 tables and the same float32 product, i.e. the same function."""
    bad_u, long_u = _search_check(name, *E.uniform_queries(name))
    tq = E.targeted_queries(name)
    bad_t, long_t = _search_check(name, tq[0], tq[1])
    print(f"{name}: halving path taken by {long_u} of {2 * E.N_UNIFORM} uniform and {long_t} of {2 * len(tq[0])} "
          f"targeted searches; ties achieved {tq[4]} of {len(tq[0]) // 2}")
    assert bad_u == 0 and bad_t == 0
    if name not in ("tiny", "one"):
        assert long_u > 0 and long_t > 0


@pytest.mark.parametrize("name", E.FAMILIES)
def test_targeted_queries_cover_rows_dim_texels_and_ties(name):
    R = E.ref(name)
    u1, u2, rows, cols, ties = E.targeted_queries(name)
    s = R.search(u1, u2)
    row_mass = np.diff(R.p_theta, prepend=np.float32(0))
    assert set(np.flatnonzero(row_mass > 0)) == set(s["row"].tolist())
    assert np.array_equal(s["row"], rows)
    mid = slice(0, None, 2)  # (queries come in pairs: the interval's middle, then its upper boundary)
    assert np.array_equal(s["col"][mid], cols[mid])
    if name != "one":
        assert ties >= 1
    # the dimmest texel selected, as a share of its row's total
    mass = np.diff(R.p_phi, axis=1, prepend=np.float32(0))
    share = mass[s["row"], s["col"]] / R.p_phi[s["row"], -1]
    print(f"{name}: smallest selected texel mass / row total {share.min():.3g}")
    if name in ("sun_poles", "wide"):
        assert share.min() < 1e-6
    if name == "sun_seam":
        # one sun texel of 1e4 over a base of at least 0.02: no texel of its row can
        # be below 2e-6 of the row's total; the dimmest ones are reached
        assert share.min() < 1e-5 and share.min() == (mass[3][mass[3] > 0] / R.p_phi[3, -1]).min()
    if name == "black_half":
        # a texel of zero mass is never selected (below), and the lit texels of a
        # row are within a factor of 11 of each other: what there is to reach are
        # the ends of the zero stretch, by an exact tie on its flat CDF
        k = s["col"] == 29
        assert k.any() and (s["r2"][k] == R.p_phi[s["row"][k], 59]).any() and (s["col"] == 60).any()
    # no query with u > 0 selects a texel of zero mass
    for u1q, u2q in ((u1, u2), E.uniform_queries(name)):
        q = R.search(u1q, u2q)
        pos = (np.asarray(u1q) > 0) & (np.asarray(u2q) > 0)
        assert (row_mass[q["row"][pos]] > 0).all() and (mass[q["row"][pos], q["col"][pos]] > 0).all()
        assert (R.pdf[q["row"][pos], q["col"][pos]] > 0).all()


@pytest.mark.parametrize("name", E.FAMILIES)
def test_special_directions_land_where_aimed(name):
    R = E.ref(name)
    d, parts = E.lookup_dirs(name)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6) and np.isfinite(d).all()
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
    assert (np.abs(d[parts["random"]][:, 1]) <= 0.999).all() and parts["random"].stop == E.N_DIRS
    tu, tv = R.dir_coords(d)
    _, _, _, _, _, _, bu, bv = R.footprint(tu, tv)
    for key, branch, axis in (("tu_lo", 0, bu), ("tu_hi", 1, bu), ("tv_lo", 0, bv), ("tv_hi", 1, bv)):
        n = int((axis[parts[key]] == branch).sum())
        print(f"{name}: {key} taken by {n} of {E.N_BRANCH} aimed directions")
        assert n >= 16, (name, key, n)
    # the ratio d.z / sin_theta exceeds 1 in float32 before the clamp
    r = d[parts["ratio_over_1"]].astype(np.float32)
    ratio = np.abs(r[:, 2] / np.sqrt(np.float32(1) - r[:, 1] * r[:, 1]))
    assert (ratio > 1).sum() >= 16
    assert (R.w * R.h <= 4096) == ("texels" in parts)
    seam = d[parts["seam"]]
    assert {float(x) for x in seam[:, 0]} == {0.0, float(np.float32(1e-30)), float(np.float32(-1e-30))}
    zeros = seam[seam[:, 0] == 0, 0]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    assert (seam[:, 2] > 0).any() and (seam[:, 2] < 0).any()


@pytest.mark.parametrize("name", E.FAMILIES)
def test_fp32_floor(name):
    """The reference's lookup and sampling formulas in numpy float32 against
    float64: delta32 (the yardstick the GPU test imports), and this float32
    model held to the GPU test's own lookup and per-sample criteria."""
    R = E.ref(name)
    delta = E.delta32(name)
    d, _ = E.lookup_dirs(name)
    d = d[E.continuous(name)]
    tu, tv = R.dir_coords(d)
    err = np.abs(R.lookup_dir(d, f32=True).astype(np.float64) - R.lookup(tu, tv)).max(axis=1)
    tol = R.lookup_tolerance(tu, tv, delta)
    worst = float((err / tol).max())
    # the estimator's environment factor radiance / pdf of the uniform draws, as the per-sample criterion reads it
    u1, u2 = E.uniform_queries(name)
    s64, s32 = R.sample(u1, u2), R.sample(u1, u2, f32=True)
    ok = ~s64["degenerate"]
    with np.errstate(invalid="ignore", divide="ignore"):
        f64 = (R.lookup(s64["tu"], s64["tv"]) / s64["pdf"][:, None])[ok]
        f32 = (R.lookup(s32["tu"], s32["tv"], f32=True) / s32["pdf"][:, None]).astype(np.float64)[ok]
    rel = np.abs(f32 - f64).max(axis=1) / np.maximum(1.0, np.abs(f64).max(axis=1))
    print(f"{name}: delta32 {delta:.3g} texel; float32 lookup error / tolerance at most {worst:.3f}; "
          f"float32 radiance / pdf relative difference at most {rel.max():.3g}")
    assert np.isfinite(f64).all() and np.isfinite(f32).all()
    # delta32 is set by float32 acos near +-1 (phi near 0 or pi): about sqrt(2^-23) rad, times w / 2 pi texels.  On
    # the small maps (0.04 .. 0.1 texel at 64 and 96 columns, 7e-4 on 7x5) a tolerance of 4 * delta32 tells
    # neighbouring texels apart; on `wide` (0.14) and black_row0 (0.07) it is half and a quarter of a texel wide, and
    # the lookup by DIRECTION has little power there.  The lookup at the DRAWN coordinates is held to the coordinate
    # bound instead (tests/test_gpu_env_maps.py test_probe_radiance), which is 1e-3 texel on `wide`.
    assert delta < 0.25
    assert worst <= 1.0
    assert (rel <= S.TOL).mean() >= 0.995


# ------------------------------------------------------------------ the render scenes, on the restatement alone
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("env_maps")


@pytest.mark.parametrize("key", list(E.RENDER_SCENES), ids=E.scene_id)
def test_render_scene_is_lit_by_the_map(restate, scene_dir, key):
    path, ref = E.reference(restate, scene_dir, key)
    ref = ref[:, :, :E.N_SAMPLES]
    assert np.isfinite(ref).all()
    assert np.array_equal(S.ref_samples(restate, path, None, scene_args=E.scene_args(key)), ref)
    bare = S.ref_samples(restate, S.write_scene(E.render_scene(key, with_env=False), scene_dir,
                                                "bare_" + E.scene_id(key)), None, scene_args=E.scene_args(key))
    moved = 1.0 - S.within(ref, bare).mean()
    lum = ref.max(axis=-1)
    peak = float(lum.max() / np.median(lum[lum > 0]))
    print(f"{E.scene_id(key)}: the map changes {moved * 100:.1f}% of the samples; brightest sample "
          f"{peak:.0f} x the median non-zero sample")
    assert moved >= 0.15
    if key[1] in ("sun_seam", "sun_poles"):
        assert peak > 100


# ------------------------------------------------------------------ the probe's refusals (nothing reaches a device)
# A context exists only on a device (pt_create fails without one), so the two refusals that need one -- a scene
# without an environment light, and no scene at all (PT_E_NOSCENE) -- are in tests/test_gpu_env_maps.py
# test_probe_refusals_on_a_device; the probe checks the queries before the context, so every other refusal is here.
def test_probe_refuses_bad_queries():
    L = native.lib()
    n = 4
    u = np.array([0.0, 0.25, 0.5, 0.75], np.float32)
    i32 = np.zeros(2 * n, np.int32)
    f = np.zeros(13 * n, np.float32)
    d = np.array([[0, 1, 0], [0.6, 0, 0.8]], np.float32)
    rad = np.zeros(6, np.float32)

    def call(n, u1, u2, m, dirs, rad_ptr, outs=True):
        o = [i32.ctypes.data, i32.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data,
             f.ctypes.data, f.ctypes.data, f.ctypes.data] if outs else [None] * 9
        return L.pt_debug_env_probe(None, n, u1, u2, *o, m, dirs, rad_ptr)

    def refused(rc, word):
        assert rc == native.PT_E_INVALID and word.encode() in L.pt_last_error(), (rc, L.pt_last_error())

    # valid queries get as far as the context check
    refused(call(n, u.ctypes.data, u.ctypes.data, 2, d.ctypes.data, rad.ctypes.data), "NULL context")
    refused(call(0, None, None, 0, None, None, outs=False), "NULL context")
    refused(call(-1, u.ctypes.data, u.ctypes.data, 0, None, None), "count")
    refused(call(n, u.ctypes.data, u.ctypes.data, (1 << 24) + 1, d.ctypes.data, rad.ctypes.data), "count")
    refused(call(n, None, u.ctypes.data, 0, None, None), "NULL sample")
    refused(call(n, u.ctypes.data, u.ctypes.data, 0, None, None, outs=False), "NULL sample")
    refused(call(0, None, None, 2, None, rad.ctypes.data, outs=False), "NULL direction")
    refused(call(0, None, None, 2, d.ctypes.data, None, outs=False), "NULL direction")
    for bad in (1.0, -1e-9, 1.5, np.nan, np.inf):
        b = u.copy()
        b[2] = bad
        refused(call(n, b.ctypes.data, u.ctypes.data, 0, None, None), "outside [0, 1)")
        refused(call(n, u.ctypes.data, b.ctypes.data, 0, None, None), "outside [0, 1)")
    for bad in ([0, np.nan, 1], [np.inf, 0, 0], [0, 0, 0], [0, 1.002, 0], [0.6, 0, 0.79], [1, 1, 1]):
        b = d.copy()
        b[1] = bad
        refused(call(0, None, None, 2, b.ctypes.data, rad.ctypes.data, outs=False), "not a unit vector")
    assert not i32.any() and not f.any() and not rad.any()


def test_env_tables_arguments():
    L = native.lib()
    m = np.ascontiguousarray(E.env_map("tiny"))
    assert L.pt_env_tables(None, 7, 5, None, None, None) == native.PT_E_INVALID
    assert L.pt_env_tables(m.ctypes.data, 0, 5, None, None, None) == native.PT_E_INVALID
    assert L.pt_env_tables(m.ctypes.data, 7, 5, None, None, None) == native.PT_OK
    pt = np.zeros(5, np.float32)
    assert L.pt_env_tables(m.ctypes.data, 7, 5, pt.ctypes.data, None, None) == native.PT_OK
    assert np.array_equal(pt, E.ref("tiny").p_theta) and pt[-1] > 0
