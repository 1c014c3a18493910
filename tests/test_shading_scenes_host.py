"""The scenes of tests/shading_scenes.py test what they claim (CPU only).

Everything here runs in the restatement alone: each scene loads and renders,
every light of every list moves the per-sample output (or, where it was built
to contribute nothing, leaves it bit-identical), every BSDF entry is seen,
every specular type carries light through a bounce, every colour channel of
every material and light reaches the image, the total-internal-reflection
branch of GlassBSDF is taken, and the deep scene really runs deep.  The GPU
twin (tests/test_gpu_shading_sweep.py) then compares the kernel with these
very samples.
"""
import numpy as np
import pytest

from tests import shading_scenes as S


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shading_scenes")


def _ref(restate, scene_dir, name):
    path, ref = S.reference(restate, scene_dir, name)
    return path, ref[:, :, :S.N_SAMPLES]


def _variant(restate, scene_dir, name, d, tag):
    return S.ref_samples(restate, S.write_scene(d, scene_dir, f"{name}_{tag}"), name)


def _moved(a, b):
    """Fraction of samples of a beyond the GPU comparison's tolerance of b."""
    return 1.0 - S.within(a, b).mean()


@pytest.mark.parametrize("name", list(S.CASES))
def test_scene_renders_finite_and_repeatable(restate, scene_dir, name):
    path, ref = _ref(restate, scene_dir, name)
    assert np.isfinite(ref).all()
    assert np.array_equal(S.ref_samples(restate, path, name), ref)
    _, w, h, m, l, seed = S.CASES[name]
    img, _ = restate.render(path, w, h, S.N_SAMPLES, m, l, seed, rng_mode=1, threads=2)
    assert np.array_equal(img, S.sum_in_order(ref))  # rs_pixel_samples is rs_render's loop without the average
    if name == "L0":
        assert not ref.any()
    else:
        assert (ref.max(axis=-1) > 0).mean() > 0.1


def test_list_lengths_and_orders():
    L = S.LIGHT_LISTS
    assert sorted({len(v) for v in L.values()}) == [0, 1, 2, 3, 5, 8, 9, 12]
    kinds = lambda name: [l["type"] for l in L[name]]
    assert kinds("L2_point_area") == [S.L_POINT, S.L_AREA] and kinds("L2_area_point") == [S.L_AREA, S.L_POINT]
    assert kinds("L3") == [S.L_AREA, S.L_AREA, S.L_HEMI]
    assert L["L2_area_occluded"][1] is S.OCCLUDED and L["L2_area_away"][1] is S.AWAY
    assert L["L9"][:8] == L["L8"] and L["L9_env"][:8] == L["L8"] and L["L9_env"][8]["type"] == S.L_ENV
    assert {l["type"] for l in L["L12"]} == {S.L_DIR, S.L_HEMI, S.L_POINT, S.L_AREA}
    for v in L.values():  # distinct, non-grey radiances
        rads = [l["rad"] for l in v if l["type"] != S.L_ENV]
        assert len(set(rads)) == len(rads)
        assert all(len(set(r)) == 3 for r in rads)


@pytest.mark.parametrize("name", [n for n in S.LIGHT_LISTS_ALL if S.LIGHT_LISTS_ALL[n]])
def test_every_light_matters(restate, scene_dir, name):
    """Light k's radiance zeroed (the draw order is unchanged): at least 5% of
    the samples move beyond the tolerance the GPU comparison grants -- a
    kernel that skipped light k could not pass it.  The two lights built to
    contribute nothing change nothing, bit for bit."""
    case = name if name in S.CASES else "NS255"
    _, ref = _ref(restate, scene_dir, case)
    lights = S.LIGHT_LISTS_ALL[name]
    for k, light in enumerate(lights):
        d = dict(S.scene(case))
        if light["type"] == S.L_ENV:
            # (the map scaled, not zeroed: its importance sampling, hence every draw, is scale-invariant)
            d["env_rgb"] = d["env_rgb"] * np.float32(2.0 ** -30)
        else:
            rad = d["light_rad"].copy()
            rad[3 * k:3 * k + 3] = 0
            d["light_rad"] = rad
        got = _variant(restate, scene_dir, case, d, f"no{k}")
        if S.contributes_nothing(light):
            assert np.array_equal(got, ref), (name, k)
        else:
            frac = _moved(got, ref)
            print(f"{name} light {k} (type {light['type']}): {frac * 100:.1f}% of samples move")
            assert frac >= 0.05, (name, k, frac)


@pytest.mark.parametrize("name", ["M16", "M20"])
def test_every_material_is_seen(restate, scene_dir, name):
    d = S.scene(name)
    path, ref = _ref(restate, scene_dir, name)
    _, w, h = S.CASES[name][:3]
    nb = len(d["bsdf_type"])
    assert nb == {"M16": 16, "M20": 20}[name]
    _, first, _, _ = S.first_hits(restate, path, d, w, h)
    counts = np.bincount(first[first >= 0], minlength=nb)
    print(name, "first-hit pixels per BSDF:", counts.tolist())
    assert counts.min() >= 16, counts
    ptype = np.asarray(d["prim_type"])
    for t in range(5):  # every type on a triangle and on a sphere
        on = {int(ptype[i]) for i in range(len(ptype)) if d["bsdf_type"][d["prim_bsdf"][i]] == t}
        assert on == {0, 1}, (t, on)
    par = d["bsdf_params"].reshape(-1, 12)
    iors = {round(float(p[9]), 3) for p, t in zip(par, d["bsdf_type"]) if t in (S.REFRACTION, S.GLASS)}
    assert iors == {0.8, 1.0, 1.2, 1.45, 2.4}
    for t, p in zip(d["bsdf_type"], par):  # three distinct channel values wherever a colour is read
        for lo in {S.DIFFUSE: [0], S.MIRROR: [0], S.REFRACTION: [3], S.GLASS: [0, 3], S.EMISSION: [6]}[int(t)]:
            assert len(set(p[lo:lo + 3].tolist())) == 3 or not p[lo:lo + 3].any() or np.allclose(p[lo:lo + 3], 0.05)
    albedos = {tuple(np.round(p[:3].astype(np.float64), 3).tolist()) for p, t in zip(par, d["bsdf_type"]) if t == S.DIFFUSE}
    assert {(0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (1.3, 1.2, 1.1)} <= albedos
    # a specular type made black ends every path at its bounce: the samples
    # that change are samples that took a bounce through it (and carried light)
    for t in (S.MIRROR, S.REFRACTION, S.GLASS):
        dd = dict(d)
        p2 = par.copy()
        p2[np.asarray(d["bsdf_type"]) == t, 0:6] = 0
        dd["bsdf_params"] = p2.reshape(-1)
        got = _variant(restate, scene_dir, name, dd, f"black{t}")
        frac = (got != ref).any(axis=-1).mean()
        print(f"{name}: {frac * 100:.2f}% of samples bounce through BSDF type {t}")
        assert frac >= 0.01, (t, frac)


def test_total_internal_reflection_quirk_occurs(restate, scene_dir):
    """GlassBSDF returns the TRANSMITTANCE on total internal reflection
    (bsdf.cpp:129-131).  Camera rays enter the ior-0.8 glass sphere; where
    1 - (1 / 0.8)^2 (1 - cos^2) < 0 they take that branch."""
    d = S.scene("M16")
    path, ref = _ref(restate, scene_dir, "M16")
    _, first, dr, nrm = S.first_hits(restate, path, d, 32, 32)
    glass = [i for i, (t, p) in enumerate(zip(d["bsdf_type"], d["bsdf_params"].reshape(-1, 12)))
             if t == S.GLASS and abs(p[9] - 0.8) < 1e-6]
    assert len(glass) == 1
    on = first == glass[0]
    cos = -(dr[on] * nrm[on]).sum(axis=1)
    assert (cos > 0).all()  # entering: the sphere's normal is outward
    tir = 1.0 - (1.0 / 0.8) ** 2 * (1.0 - cos * cos) < 0
    print(f"{on.sum()} pixels enter the ior-0.8 glass sphere, {tir.sum()} by total internal reflection")
    assert tir.sum() >= 4 and (~tir).sum() >= 4
    # on that branch the sample's value is the transmittance times what the mirrored ray sees:
    # scaling the transmittance's green alone moves TIR pixels' green (and no reflectance does)
    dd = dict(d)
    p2 = d["bsdf_params"].reshape(-1, 12).copy()
    p2[glass[0], 0:3] = 0  # no Fresnel reflection can carry light: what is left at TIR pixels is the quirk
    dd["bsdf_params"] = p2.reshape(-1)
    got = _variant(restate, scene_dir, "M16", dd, "tir")
    ys, xs = np.nonzero(on)
    lit = got[ys[tir], xs[tir]].max(axis=(1, 2)) > 0
    assert lit.any()


def test_emissive_sphere_is_seen_after_a_bounce(restate, scene_dir):
    d = S.scene("M16")
    path, ref = _ref(restate, scene_dir, "M16")
    _, first, _, _ = S.first_hits(restate, path, d, 32, 32)
    par = d["bsdf_params"].reshape(-1, 12)
    slot = S.full16_table()[1]["sphE"]
    assert d["bsdf_type"][slot] == S.EMISSION
    dd = dict(d)
    p2 = par.copy()
    p2[slot, 6:9] = 0
    dd["bsdf_params"] = p2.reshape(-1)
    got = _variant(restate, scene_dir, "M16", dd, "noemit")
    changed = (got != ref).any(axis=(-1, -2))
    assert (changed & (first != slot)).sum() >= 4  # reached through a mirror / glass bounce, not by the camera ray


def _channel_cases():
    out = []
    d = S.scene("M20")
    for i, (t, p) in enumerate(zip(d["bsdf_type"], d["bsdf_params"].reshape(-1, 12))):
        fields = {S.DIFFUSE: [0], S.MIRROR: [0], S.REFRACTION: [3], S.GLASS: [0, 3], S.EMISSION: [6]}[int(t)]
        if t == S.GLASS and p[9] == 1.0:
            fields = [3]  # Fresnel 0: the reflectance is never read
        out += [("bsdf", i, f + c) for f in fields for c in range(3)]
    return out


@pytest.mark.parametrize("what,i,k", _channel_cases())
def test_one_material_channel_changes_the_image(restate, scene_dir, what, i, k):
    d = S.scene("M20")
    _, ref = _ref(restate, scene_dir, "M20")
    p2 = d["bsdf_params"].reshape(-1, 12).copy()
    p2[i, k] = 0.5 * p2[i, k] if p2[i, k] != 0 else 0.5
    dd = dict(d)
    dd["bsdf_params"] = p2.reshape(-1)
    got = _variant(restate, scene_dir, "M20", dd, f"b{i}_{k}")
    bad = ~S.within(got, ref)
    assert bad.sum() >= 4, (i, k, int(bad.sum()))
    other = [c for c in range(3) if c != k % 3]
    if d["bsdf_type"][i] == S.EMISSION:  # emission is only ever added: the other channels stay
        assert np.array_equal(got[..., other], ref[..., other])


@pytest.mark.parametrize("k", [k for k, l in enumerate(S.LIGHT_LISTS["L12"]) if not S.contributes_nothing(l)])
@pytest.mark.parametrize("c", range(3))
def test_one_light_channel_changes_the_image(restate, scene_dir, k, c):
    d = S.scene("L12")
    _, ref = _ref(restate, scene_dir, "L12")
    rad = d["light_rad"].copy()
    rad[3 * k + c] *= 0.5
    dd = dict(d)
    dd["light_rad"] = rad
    got = _variant(restate, scene_dir, "L12", dd, f"l{k}_{c}")
    bad = ~S.within(got, ref)
    assert bad.sum() >= 4, (k, c, int(bad.sum()))
    other = [x for x in range(3) if x != c]
    assert np.array_equal(got[..., other], ref[..., other])  # the draws do not depend on a radiance


def test_mirror_box_paths_run_past_depth_127(restate, scene_dir):
    """max_depth = 254 lives in an 8-bit field: the scene must use its top bit.
    More than 128 rays per sample on average means paths deeper than 127."""
    path, ref = _ref(restate, scene_dir, "DEPTH254")
    _, w, h, m, l, seed = S.CASES["DEPTH254"]
    assert m == 254
    _, st = restate.render(path, w, h, S.N_SAMPLES, m, l, seed, rng_mode=1, threads=2)
    rays = st[0] / (w * h * S.N_SAMPLES)
    print(f"mirror box: {rays:.1f} rays per sample, {(ref.max(axis=-1) > 0).mean() * 100:.1f}% of samples lit")
    assert rays > 128
    img254, _ = restate.render(path, w, h, S.N_SAMPLES, 254, l, seed, rng_mode=1, threads=2)
    img127, _ = restate.render(path, w, h, S.N_SAMPLES, 127, l, seed, rng_mode=1, threads=2)
    assert (~S.within(img127, img254)).sum() >= 2  # light found beyond depth 127 reaches the image
    assert (ref.max(axis=-1) > 0).mean() > 0.05


def test_ns255_scene_has_two_area_lights():
    d = S.scene("NS255")
    assert d["light_type"].tolist() == [S.L_AREA, S.L_AREA] and S.CASES["NS255"][4] == 255
