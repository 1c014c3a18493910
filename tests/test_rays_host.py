"""The host side of path tracing along the caller's rays (no GPU): the probe's
rays, and the new prototypes, flag and ctypes bindings against include/ptgpu.h
(in the style of tests/test_abi.py)."""
import ctypes
import os
import re

import numpy as np

from dsgpuraytracing_amd import native
from dsgpuraytracing_amd.pathtracer import Device, Film, probe_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_render_rays_device", "pt_render_rays", "pt_film_add_pass_rays")


def header():
    txt = open(os.path.join(ROOT, "include", "ptgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_probe_rays_layout_and_directions():
    w, h = 16, 8
    origin = (0.25, -0.5, 2.0)
    r = probe_rays(origin, w, h)
    assert r.shape == (w * h, 8) and r.dtype == np.float32 and r.flags.c_contiguous
    assert (r[:, 0:3] == np.array(origin, np.float32)).all() and np.isinf(r[:, 3]).all() and (r[:, 7] == 0).all()
    d = r[:, 4:7].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    g = d.reshape(h, w, 3)
    # row 0 points up, the last row down, and a row is one latitude
    assert (g[0, :, 1] > 0.97).all() and (g[h - 1, :, 1] < -0.97).all()
    assert (np.diff(g[:, 0, 1]) < 0).all() and np.abs(g[:, :, 1] - g[:, :1, 1]).max() < 1e-6
    # ray p = x + y * w is texel (x, y)'s centre in the parameterisation the
    # kernel's env_dir reads a map with: theta from +y, phi = acos(d.z / sin
    # theta), mirrored to (pi, 2 pi) where d.x > 0; texel = angle / range * size - 0.5
    theta = np.arccos(np.clip(d[:, 1], -1, 1))
    phi = np.arccos(np.clip(d[:, 2] / np.sin(theta), -1, 1))
    phi = np.where(d[:, 0] > 0, 2 * np.pi - phi, phi)
    tu, tv = phi / (2 * np.pi) * w - 0.5, theta / np.pi * h - 0.5
    p = np.arange(w * h)
    assert np.abs(tu - p % w).max() < 1e-4 and np.abs(tv - p // w).max() < 1e-4


def test_flag_value_matches_header():
    m = re.search(r"#define\s+PT_FLAG_RAYS_CAPTURE\s+(\d+)u", header())
    assert m and int(m.group(1)) == native.PT_FLAG_RAYS_CAPTURE == 16
    others = [native.PT_FLAG_STATS, native.PT_FLAG_REF_COUNTS, native.PT_FLAG_PACKED, native.PT_FLAG_PACKED16]
    assert all(native.PT_FLAG_RAYS_CAPTURE & f == 0 for f in others)


C_TYPES = {"pt_ctx*": ctypes.c_void_p, "pt_film*": ctypes.c_void_p, "void*": ctypes.c_void_p,
           "const void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const pt_tile*": ctypes.POINTER(native.pt_tile),
           "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}


def test_prototypes_match_bindings():
    txt = header()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, f"{name} is not declared in ptgpu.h"
        params = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]
        res, args = native._SIGS[name]
        assert res is ctypes.c_int32
        assert [C_TYPES[p] for p in params] == list(args), (name, params)
    assert txt.index("pt_render_rays_device") > txt.index("pt_camera_rays_device")  # (with the ray queries)


def test_library_exports_and_refuses_null():
    L = native.lib()
    for name in NEW:
        assert hasattr(L, name), f"libptgpu.so does not export {name}"
    tile = native.pt_tile(0, 0, 4, 4)
    buf = np.zeros((16, 8), np.float32)
    out = np.zeros((4, 4, 3), np.float32)
    assert L.pt_render_rays_device(None, ctypes.byref(tile), 1, buf.ctypes.data, out.ctypes.data, None, 0) == native.PT_E_INVALID
    assert b"NULL context" in L.pt_last_error()
    assert L.pt_render_rays(None, ctypes.byref(tile), 1, buf.ctypes.data, out.ctypes.data, 0) == native.PT_E_INVALID
    assert L.pt_film_add_pass_rays(None, ctypes.byref(tile), 1, buf.ctypes.data, None) == native.PT_E_INVALID
    assert b"NULL film" in L.pt_last_error()


def test_python_layer_has_the_entry_points():
    assert callable(Device.render_rays) and callable(Film.add_pass_rays)
