"""The host policy of a render launch (csrc/launch_plan.cpp: plan_launch,
frames_that_fit, the knobs) on the CPU.

tests/plan/plan_driver.cpp is linked with csrc/launch_plan.cpp alone, built
with -fsanitize=address,undefined (no recovery), and run as a child process
over the cases below: any sanitizer report fails the test.  The driver prints
each plan as JSON; what a plan must satisfy is asserted here, from the rules
in the comments of launch_plan.cpp and pt_tuning.h restated by hand."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsgpuraytracing_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

INT32_MAX = 2**31 - 1
REF_LANES = 256 * 20 * 64  # PT_GROUP_REF_LANES = 327,680
MIN_SLOTS = 24             # PT_GROUP_MIN_SLOTS
SMALL_SLOTS = 16           # PT_SMALL_SLOTS
BATCH_SLOTS = 32           # PT_BATCH_SLOTS
SUM_BYTES = 12
SUM_BUDGET = 8 << 30       # PT_GROUP_SUM_GIB
CHUNK_BIG = 512
BANDS_TREE = 8 << 20       # PT_BANDS_TREE_MIB
BIG_TREE = "nodes=70000"   # x 128 B = 8.96 MB > 8 MiB

# a camera at (0.3, -0.2, 5) turned 20 degrees about y, and a scene box in
# front of it that covers about the middle quarter of the screen
_a = np.deg2rad(20.0)
C2W = np.array([[np.cos(_a), 0, np.sin(_a)], [0, 1, 0], [-np.sin(_a), 0, np.cos(_a)]])
POS = np.array([0.3, -0.2, 5.0])
AX = AY = 1.0  # screen_w / screen_dist


def _cam(pos=POS, c2w=C2W, sw=1.0, sh=1.0, sd=1.0):
    return "cam=" + ",".join(repr(float(v)) for v in list(pos) + list(np.asarray(c2w).reshape(9)) + [sw, sh, sd])


def _box(lo, hi):
    return "box=" + ",".join(repr(float(v)) for v in list(lo) + list(hi))


# the box: 1.2 units wide at depth ~4.4 from the pinhole, centred on the view axis
_CENTRE = POS - 4.4 * C2W[:, 2]
BOX_LO, BOX_HI = _CENTRE - [0.9, 1.0, 0.6], _CENTRE + [0.9, 1.0, 0.6]
QUARTER = f"{_cam()} {_box(BOX_LO, BOX_HI)}"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    srcs = [os.path.join(ROOT, "tests", "plan", "plan_driver.cpp"), os.path.join(CSRC, "launch_plan.cpp")]
    cmd = [cxx, "-std=c++17", "-g", "-Wall"] + SAN + [f"-I{ROOT}/include", f"-I{CSRC}"]
    jobs = [subprocess.Popen(cmd + [opt, "-c", src, "-o", f"{exe}{k}.o"], stderr=subprocess.PIPE, text=True)
            for k, (src, opt) in enumerate(zip(srcs, ("-O0", "-O1")))]  # (side by side: the compile is the test's time)
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err[-3000:]
    r = subprocess.run(cmd + [f"{exe}0.o", f"{exe}1.o", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = [json.loads(ln) for ln in p.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def test_group_size_by_hand(driver):
    # traced = 2^18 (a 1024^2 frame culled to a quarter), 64 spp, no environment light:
    # groups of 4: 2^18 * 16 = 4.19 M slots <  327,680 * 24 = 7.86 M -> halve
    # groups of 2: 2^18 * 32 = 8.39 M slots >= 7.86 M                -> 2 (README: C3)
    assert 2**18 * 16 < REF_LANES * MIN_SLOTS <= 2**18 * 32
    g = "op=group spp=64 frame_blocks=16384"
    out = driver([f"{g} traced={2**18}", f"{g} traced={2**20}", f"{g} traced={2**20} env=1", f"{g} traced={2**18} env=1",
                  f"{g} traced=1000", f"{g} traced={2**20} sample_group=8", f"{g} traced={2**20} sample_group=128"])
    assert [o["group_spp"] for o in out] == [2, 4, 2, 2, 1, 8, 64]
    # the same through a plan: the quarter-frame camera, and PT_SAMPLE_GROUP clamped to spp
    q = f"W=1024 H=1024 spp=64 {QUARTER}"
    a, b, c, d = driver([q, f"{q} env.PT_SAMPLE_GROUP=16", f"{q} env.PT_SAMPLE_GROUP=100", f"{q} env=1"])
    assert 500 * 500 < a["traced_px"] < 560 * 560
    assert (a["group_spp"], a["n_groups"], a["group_shift"]) == (2, 32, 1)
    assert (b["group_spp"], b["n_groups"]) == (16, 4)
    assert (c["group_spp"], c["n_groups"], c["group_shift"]) == (64, 1, 6)
    assert d["traced_px"] == 1024 * 1024 and d["group_spp"] == 2


@pytest.mark.parametrize("w,spp", [(128, 16), (1024, 64)])
def test_grouping_is_a_function_of_the_frame_only(driver, w, spp):
    base = f"W={w} H={w} spp={spp} {QUARTER}"
    tile_sets = ["tiles=grid:32"] + [f"tiles=grid:32:{k}/3" for k in range(3)] + [f"tiles={w // 2},{w // 2},32,32"]
    cases = [f"{base} {t} flags={fl}" for t in tile_sets for fl in (0, 1)]
    cases += [f"{base} env.PT_WAVES_PER_CU={v}" for v in (1, 8, 20)]
    cases += [f"{base} ncu={n} flags={fl}" for n in (256, 32) for fl in (0, 1)]
    cases += [f"{base} idle=0", f"{base} env.PT_NO_FOOTPRINT_CULL=1", f"{base} nf=3"]
    out = driver(cases)
    assert all(o["error"] == "" for o in out)
    assert len({(o["group_spp"], o["n_groups"]) for o in out}) == 1, [(o["group_spp"], o["n_groups"]) for o in out]
    assert out[0]["n_groups"] == -(-spp // out[0]["group_spp"])
    assert len({o["grid"] for o in out}) > 1  # (the launches do differ)


def _check_blocks(o, W, H):
    tiles, blocks, tb0 = o["tiles"], o["blocks"], o["tile_block0"]
    launch_tiles = o["ztiles"] if o["zorder"] else tiles
    x0, y0, x1, y1 = o["cull"]
    want = np.zeros((H, W), np.int32)
    for (x, y, w, h) in tiles:
        want[y:y + h, x:x + w] += 1
    assert want.max() == 1  # (the test's tiles are disjoint)
    inside = np.zeros((H, W), bool)
    inside[max(0, y0):max(0, y1 + 1), max(0, x0):max(0, x1 + 1)] = True
    got = np.zeros((H, W), np.int32)
    for (x, y, w, h) in blocks:
        assert 1 <= w <= 8 and 1 <= h <= 8 and x >= 0 and y >= 0 and x + w <= W and y + h <= H
        got[y:y + h, x:x + w] += 1
    assert got.max(initial=0) <= 1, "blocks overlap"
    assert np.array_equal(got == 1, (want == 1) & inside), "blocks != tiles within the cull rectangle"
    assert len(tb0) == len(tiles) + 1 and tb0[0] == 0 and tb0[-1] == len(blocks) == o["n_blocks"]
    assert all(a <= b for a, b in zip(tb0, tb0[1:]))
    for i, (x, y, w, h) in enumerate(launch_tiles):  # tile i's blocks lie in tile i
        for (bx, by, bw, bh) in blocks[tb0[i]:tb0[i + 1]]:
            assert x <= bx and bx + bw <= x + w and y <= by and by + bh <= y + h
    assert o["pixels"] == int(want.sum())
    assert o["culled_px"] == o["pixels"] - sum(w * h for (_, _, w, h) in blocks)
    assert o["frame_slots"] == 64 * len(blocks) * o["n_groups"]


def test_blocks_cover_the_tiles_inside_the_cull_rectangle(driver):
    frames = [(100, 70), (128, 128), (333, 257)]
    cases, dims = [], []
    for (W, H) in frames:
        for t in ("tiles=grid:32", "tiles=grid:32:1/3", "tiles=grid:16", f"tiles=5,3,{W - 9},{H - 7}",
                  f"tiles={W // 2},{H // 2},1,1", "tiles=0,0,32,32"):
            for extra in ("", "env.PT_NO_FOOTPRINT_CULL=1", "env.PT_TILE_ZORDER=1"):
                cases.append(f"W={W} H={H} spp=4 {QUARTER} {t} {extra} lists=1")
                dims.append((W, H))
    out = driver(cases)
    for o, (W, H) in zip(out, dims):
        _check_blocks(o, W, H)
    assert any(o["culled_px"] > 0 for o in out) and any(o["culled_px"] == 0 for o in out)
    assert any(o["n_blocks"] == 0 for o in out)  # (the corner tile sees nothing)


def test_a_launch_that_is_entirely_culled(driver):
    # the box in front of the camera but far off to the side: no pixel sees it
    off = _CENTRE + 40 * C2W[:, 0]
    o, = driver([f"W=128 H=96 spp=8 {_cam()} {_box(off - 1, off + 1)} lists=1"])
    assert o["error"] == "" and o["n_blocks"] == 0 and o["blocks"] == [] and o["grid"] >= 1
    assert o["tile_block0"] == [0] * (o["n_tiles"] + 1)
    assert o["footprint"] == [0, 0, -1, -1]
    assert o["culled_px"] == o["pixels"] == 128 * 96 and o["slots"] == 0 and o["partial_floats"] >= 1


def _project(pts, W, H, pos=POS, c2w=C2W):
    """Camera::generate_ray inverted: the pixel a world point is seen through."""
    cc = (pts - pos) @ c2w  # coordinates along the c2w columns
    depth = -cc[:, 2]
    assert (depth > 0).all()
    return np.floor((0.5 + cc[:, 0] / depth / AX) * W), np.floor((0.5 + cc[:, 1] / depth / AY) * H)


def test_footprint_contains_every_projected_point(driver):
    rng = np.random.default_rng(5)
    pts = BOX_LO + rng.random((1000, 3)) * (BOX_HI - BOX_LO)
    pts[:8] = [[(BOX_HI if k >> i & 1 else BOX_LO)[i] for i in range(3)] for k in range(8)]  # the corners too
    for (W, H) in ((1024, 1024), (333, 257)):
        r, p = driver([f"op=rect W={W} H={H} {QUARTER}", f"W={W} H={H} spp=4 {QUARTER}"])
        assert r["ok"] == 1 and p["cull"] == r["rect"]
        px, py = _project(pts, W, H)
        x0, y0, x1, y1 = r["rect"]
        assert (px >= x0).all() and (px <= x1).all() and (py >= y0).all() and (py <= y1).all()
        assert x0 > 0 and y0 > 0 and x1 < W - 1 and y1 < H - 1  # (it does cull)
        assert x1 - x0 <= px.max() - px.min() + 4 and y1 - y0 <= py.max() - py.min() + 4  # and is tight
        assert p["traced_px"] == (x1 - x0 + 1) * (y1 - y0 + 1) and p["footprint"] == r["rect"]


def test_footprint_gives_no_cull_when_it_cannot(driver):
    W, H = 256, 192
    full = [0, 0, W - 1, H - 1]
    base = f"W={W} H={H} spp=16"
    behind = _box(BOX_LO, np.maximum(BOX_HI, POS + 0.5 * C2W[:, 2]))  # reaches behind the pinhole plane
    culled, a, b, c, d = driver([
        f"{base} {QUARTER}",
        f"{base} {_cam()} {behind}",
        f"{base} {_cam(c2w=C2W * 1.001)} {_box(BOX_LO, BOX_HI)}",  # not orthonormal
        f"{base} {QUARTER} env=1",
        f"{base} {QUARTER} env.PT_NO_FOOTPRINT_CULL=1"])
    assert culled["cull"] != full and culled["culled_px"] > 0 and culled["traced_px"] < W * H
    for o in (a, b, c):
        assert o["cull"] == full and o["footprint"] == full and o["culled_px"] == 0 and o["traced_px"] == W * H
    # the knob traces every pixel but leaves the frame's traced area -- and so the grouping -- alone
    assert d["cull"] == full and d["culled_px"] == 0
    assert d["traced_px"] == culled["traced_px"] and d["group_spp"] == culled["group_spp"]


def _morton(cx, cy):
    k = 0
    for b in range(21):
        k |= ((cx >> b) & 1) << (2 * b) | ((cy >> b) & 1) << (2 * b + 1)
    return k


def test_tile_zorder(driver):
    big = f"W=1024 H=1024 spp=1 {BIG_TREE}"
    on, dup, one, few_px, small_tree, forced_off, forced_on, forced_one = driver([
        f"{big} lists=1",
        f"W=96 H=64 spp=1 tiles=grid:32+grid:32+grid:16 env.PT_TILE_ZORDER=1 lists=1",  # equal keys: stability
        f"{big} tiles=0,0,1024,1024",
        f"W=1024 H=1023 spp=1 {BIG_TREE}",          # below 2^20 pixels
        f"W=1024 H=1024 spp=1 nodes={BANDS_TREE // 128}",  # a tree of exactly 8 MiB
        f"{big} env.PT_TILE_ZORDER=0",
        f"W=64 H=64 spp=1 env.PT_TILE_ZORDER=1",
        f"W=64 H=64 spp=1 tiles=0,0,32,32 env.PT_TILE_ZORDER=1"])
    for o in (on, dup):
        tiles, perm = o["tiles"], o["perm"]
        assert o["zorder"] == 1 and sorted(perm) == list(range(len(tiles)))
        assert o["ztiles"] == [tiles[i] for i in perm]
        edge = max(max(t[2], t[3]) for t in tiles)
        keys = [_morton(t[0] // edge, t[1] // edge) for t in tiles]
        assert perm == sorted(range(len(tiles)), key=lambda i: (keys[i], i))  # sorted by key, stable
    assert on["perm"][:6] == [0, 1, 32, 33, 2, 3]
    assert len(set(keys)) < len(keys)  # (the second case did have ties)
    for o in (one, few_px, small_tree, forced_off, forced_one):
        assert o["zorder"] == 0 and o["n_perm"] == 0
    assert forced_on["zorder"] == 1 and forced_on["n_perm"] == 4


def _sweep_cases():
    cases = []
    for w in (64, 200, 1024):
        for spp in (1, 3, 64, 1024):
            for nf in (1, 2, 8):
                for extra in ("", "idle=0", "flags=1"):
                    cases.append(f"W={w} H={w} spp={spp} nf={nf} {extra} {BIG_TREE}")
    # the larger frames: fewer cases (each lists up to millions of blocks)
    cases += [f"W=4096 H=4096 spp={spp} nf={nf} {extra} {BIG_TREE}"
              for spp, nf, extra in ((1, 1, ""), (1, 8, "idle=0"), (3, 2, "flags=1"), (64, 1, "idle=0"), (64, 8, ""), (1024, 2, ""))]
    cases += [f"W=8192 H=8192 spp={spp} nf={nf} {BIG_TREE}" for spp, nf in ((1, 8), (64, 1), (1024, 8))]
    cases += [f"W=16384 H=16384 spp={spp} nf={nf}" for spp, nf in ((64, 2), (1024, 1), (1, 8))]
    cases += [f"W=4096 H=4096 spp=64 env.PT_CHUNK_SLOTS={v}" for v in (64, 192, 512, 100, 1024)]
    cases += [f"W=4096 H=4096 spp=64 env.PT_WAVES_PER_CU={v}" for v in (1, 40)]
    return cases


def test_bounds_over_a_sweep(driver):
    cases = _sweep_cases()
    out = driver(cases)
    refused = [c for c, o in zip(cases, out) if o["error"]]
    for c, o in zip(cases, out):
        if o["error"]:
            assert o["error"] == "frame too large for one launch"
            continue
        chunk, ng = o["chunk"], o["n_groups"]
        assert o["slots"] + 2 * o["want"] * chunk < INT32_MAX, c
        if "PT_CHUNK_SLOTS" not in c:
            assert chunk in (64, 128, 256, 512), c
        assert chunk != CHUNK_BIG or (64 * ng) % CHUNK_BIG == 0, c
        assert o["sblocks"] == int((64 * ng) % chunk == 0), c
        assert o["frame_slots"] * SUM_BYTES <= SUM_BUDGET or ng == 1, c  # (n_groups 1: group_spp == spp)
        assert 1 <= o["grid"] <= o["want"] and o["partial_floats"] == 3 * max(1, o["slots"]), c
        assert o["slots"] == o["frame_slots"] * int(c.split("nf=")[1].split()[0] if "nf=" in c else 1), c
    # a 16384^2 frame has 2048^2 blocks x 64 = 2^28 work slots at one group per
    # pixel; eight frames of it are 2^31 > INT32_MAX whatever the spp
    assert 2048 * 2048 * 64 * 8 > INT32_MAX
    assert [c for c in cases if "W=16384" in c and "nf=8" in c] == [c for c in refused if "W=16384" in c]
    assert len(refused) >= 2 and len(refused) < len(cases) // 2
    by = dict(zip(cases, out))
    assert [by[f"W=4096 H=4096 spp=64 env.PT_CHUNK_SLOTS={v}"]["chunk"] for v in (64, 192, 512, 100, 1024)] == \
        [64, 192, 512, 512, 512]  # (out of range or no multiple of 64: the frame's own 512)
    assert {o["chunk"] for o in out} >= {64, 128, 256, 512}
    assert {o["qbands"] for o in out} == {0, 1}


def test_small_launches(driver):
    # 16 slots per lane of the plain grid: 16 * 5120 * 64 = 5,242,880 slots = a
    # 2560 x 2048 frame at 1 spp (one group per pixel)
    limit = SMALL_SLOTS * 5120 * 64
    assert limit == 2560 * 2048
    at, above, busy, busy_knob, busy8, stats, census, unpiped, off, big_busy = driver([
        "W=2560 H=2048 spp=1", "W=2568 H=2048 spp=1", "W=2560 H=2048 spp=1 idle=0",
        "W=2560 H=2048 spp=1 idle=0 env.PT_WAVES_PER_CU=20", "W=64 H=64 spp=1 idle=0 bpc=1,1,1,1",
        "W=2560 H=2048 spp=1 flags=1", "W=2560 H=2048 spp=1 env.PT_CENSUS=1", "W=2560 H=2048 spp=1 pipeline=0",
        "W=2560 H=2048 spp=1 small_launch=0", "W=2568 H=2048 spp=1 idle=0"])
    assert at["slots"] == limit and at["small"] == 1 and at["chunk"] == 64 and at["want"] == 5120
    assert above["slots"] > limit and above["small"] == 0 and above["chunk"] == 128
    assert busy["small"] == 1 and busy["chunk"] == 64 and busy["want"] == 5120 // 2
    assert busy_knob["small"] == 1 and busy_knob["want"] == 5120  # (a forced grid is not halved)
    assert busy8["small"] == 1 and busy8["want"] == max(256, 8 * 256 // 2) and busy8["want"] >= busy8["n_cu"]
    for o in (stats, census, unpiped, off):
        assert o["small"] == 0 and o["chunk"] != 64
    assert census["census"] == 1 and stats["stats"] == 1 and stats["want"] == 12 * 256
    assert big_busy["small"] == 0 and big_busy["want"] == 5120 and big_busy["chunk"] == 256  # (queued: the larger claim)


def test_frames_that_fit(driver):
    # more than 32 slots per lane of a whole MI355X: 32 * 327,680 = 10,485,760
    # = a 2560 x 2048 frame in two one-sample groups per pixel
    limit = BATCH_SLOTS * REF_LANES
    assert limit == 2560 * 2048 * 2
    cases = ["W=2560 H=2048 spp=2", "W=2568 H=2048 spp=2"]
    cases += [f"W={w} H={w} spp={spp} fit_nf={nf} {extra}" for w in (64, 480, 1024) for spp in (1, 16, 64, 1024)
              for nf in (1, 3, 8) for extra in ("", QUARTER, f"{QUARTER} tiles=grid:32:1/3", "ncu=32 grid_plain=640")]
    cases += [f"W=16384 H=16384 spp=1 fit_nf=8 {QUARTER} tiles=grid:32:0/64"]
    out = driver(cases)
    assert out[0]["frame_slots"] == limit and out[0]["fit"] == 8
    assert out[1]["frame_slots"] > limit and out[1]["fit"] == 1
    fits = set()
    for c, o in zip(cases, out):
        nf = int(c.split("fit_nf=")[1].split()[0]) if "fit_nf=" in c else 8
        per = o["fit_frame_slots"]
        assert per == o["frame_slots"], c  # the plan's own per-frame slot count
        if per > limit:
            assert o["fit"] == 1, c
            continue
        n_cu = o["n_cu"]
        waves = max(640 if "grid_plain=640" in c else 20 * n_cu, 12 * n_cu, 40 * n_cu)
        ok = lambda n: per * n + 2 * waves * CHUNK_BIG < INT32_MAX and per * n * SUM_BYTES <= SUM_BUDGET
        assert 1 <= o["fit"] <= nf and (o["fit"] == 1 or ok(o["fit"])), c
        assert o["fit"] == nf or not ok(o["fit"] + 1), c  # and no fewer than fit
        fits.add(o["fit"])
    assert fits >= {1, 3, 8}
