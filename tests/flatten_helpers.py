"""The CPU flatten driver shared by tests/test_scene_flatten.py and
tests/test_deep_trees_host.py: tests/flatten/flatten_driver.cpp linked with
csrc/scene_flatten.cpp, render_tree.cpp, scene_host.cpp, exr_io.cpp and
pt_error.cpp, built with -fsanitize=address,undefined (no recovery) and run
as a child process; any sanitizer report fails the calling test.  Built once
per test session."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from dsgpuraytracing_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsgpuraytracing_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
DTYPES = {"prims": (np.float32, 12), "norms": (np.float32, 9), "prims_ref": (np.float32, 12),
          "norms_ref": (np.float32, 9), "prim_map": (np.int32, None), "nodes4": (np.float32, 32),
          "nodes2": (np.float32, 16)}

_exe = []  # the driver, once built


def _build(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    try:
        inc = build.rocm_include()  # the vector types of pt_records.h, as build.py finds them
    except RuntimeError:
        pytest.skip("no ROCm headers")
    if not os.path.exists(os.path.join(inc, "hip", "hip_vector_types.h")):
        pytest.skip("no ROCm headers")
    exe = str(tmp_path_factory.mktemp("flatten") / "flatten_driver")
    srcs = [os.path.join(ROOT, "tests", "flatten", "flatten_driver.cpp")] + \
        [os.path.join(CSRC, f) for f in ("scene_flatten.cpp", "render_tree.cpp", "scene_host.cpp", "exr_io.cpp", "pt_error.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__"] + SAN + \
        [f"-I{ROOT}/include", f"-I{CSRC}", f"-isystem{inc}"]
    jobs = [subprocess.Popen(cmd + ["-c", src, "-o", f"{exe}{k}.o"], stderr=subprocess.PIPE, text=True)
            for k, src in enumerate(srcs)]  # (side by side: the compile is the test's time)
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err[-3000:]
    r = subprocess.run(cmd + [f"{exe}{k}.o" for k in range(len(srcs))] + ["-lz", "-pthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def flatten_driver(tmp_path_factory):
    """run(cases): the driver over the case lines (flatten_driver.cpp has the syntax)."""
    if not _exe:
        _exe.append(_build(tmp_path_factory))
    exe = _exe[0]

    def run(cases):
        """One record per case: the driver's JSON line, `sha256` of each array
        it wrote and `dir` / `name` to load them from (load())."""
        out_dir = str(tmp_path_factory.mktemp("out"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe, out_dir], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env,
                           timeout=600)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = [json.loads(ln) for ln in p.stdout.splitlines()]
        assert len(out) == len(cases)
        for o in out:
            o["dir"] = out_dir
            o["sha256"] = {f[len(o["name"]) + 1:]: hashlib.sha256(open(os.path.join(out_dir, f), "rb").read()).hexdigest()
                           for f in sorted(os.listdir(out_dir)) if f.startswith(o["name"] + ".")}
        return out

    return run


def load(o, what):
    dt, cols = DTYPES[what]
    a = np.fromfile(os.path.join(o["dir"], f"{o['name']}.{what}"), dt)
    return a if cols is None else a.reshape(-1, cols)
