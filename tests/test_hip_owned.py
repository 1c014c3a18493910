"""The owning types of csrc/hip_owned.h (DevBuf, DevList, PinnedBuf, Event,
Stream, TimedSpan, StreamOrder and their live counts) and the tile seam of
csrc/tile_seam.cpp (its queue, its lock and its completion thread) on the CPU.

tests/owned/owned_driver.cpp includes the header against a fake HIP
(tests/owned/fake_hip/hip/hip_runtime.h: malloc / free, counted dummy handles,
logged synchronise / wait / record calls, switches that fail the k-th
allocation, copy or event synchronise, a gate that holds event synchronises),
is built together with tile_seam.cpp with -fsanitize=address,undefined (no recovery) and run
as a child process with leak detection: a failed assertion of the driver, a
sanitizer report or a leak fails the test."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsgpuraytracing_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_owned_types_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "owned_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + SAN + \
        [f"-I{ROOT}/tests/owned/fake_hip", f"-I{CSRC}", os.path.join(ROOT, "tests", "owned", "owned_driver.cpp"),
         os.path.join(CSRC, "tile_seam.cpp"), "-pthread", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0 and p.stdout.strip().endswith("owned ok"), (p.stdout[-2000:], p.stderr[-3000:])
    assert "ERROR" not in p.stderr, p.stderr[-3000:]


def test_no_hand_managed_hip_resource_in_csrc():
    """Every allocation, event and stream of csrc/ is made and released in hip_owned.h."""
    call = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree|EventCreate\w*|EventDestroy|StreamCreate\w*|StreamDestroy)\s*\(")
    found = [(f, m.group(0)) for f in sorted(os.listdir(CSRC)) if f != "hip_owned.h"
             for m in call.finditer(open(os.path.join(CSRC, f)).read())]
    assert found == []
