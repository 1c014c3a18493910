#!/usr/bin/env python3
"""Measurements of the progressive film (the film section) on the
C3 proxy at 1024x1024, whole frame, one GPU:

  * the accumulate and resolve kernels' HIP-event times (pt_film_info) against
    their byte counts;
  * wall clock per displayed pass: Film.add_pass + pt_film_resolve (RGBA only)
    against pt_render_tiles + host pt_to_color.

Prints one JSON line.  Usage: python tools/film_bench.py [--spp 64] [--passes 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0  # MI355X float4 copy rate


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from dsgpuraytracing_amd import native, scenes
    from dsgpuraytracing_amd.pathtracer import Device, Scene, tile_fifo
    import bench

    w = h = args.size
    dae = scenes.proxy_path(1, bench.scene_cache_dir())
    sc = Scene.from_dae(dae, w, h)
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    dev.set_params(w, h, args.spp, 4, 1, 1)
    tiles = np.asarray(tile_fifo(w, h), np.int32)
    L = native.lib()
    px = w * h

    # --- kernels: HIP-event times of the last accumulate / resolve
    film = dev.film(w, h)
    hdr = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
    rgba = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
    err = torch.empty((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    acc_ms, res_rgba_ms, res_all_ms = [], [], []
    for i in range(args.warmup + args.passes):
        film.add_pass(tiles)
        film.resolve_device(0, rgba.data_ptr(), 0)
        a = film.info()
        film.resolve_device(hdr.data_ptr(), rgba.data_ptr(), err.data_ptr())
        b = film.info()
        if i >= args.warmup:
            acc_ms.append(a["accumulate_ms"])
            res_rgba_ms.append(a["resolve_ms"])
            res_all_ms.append(b["resolve_ms"])
    acc_bytes = px * (12 + 32 + 32)
    res_rgba_bytes = px * (16 + 4)
    res_all_bytes = px * (32 + 12 + 4 + 4)

    def kernel(ms, nbytes):
        t = median(ms)
        return {"ms": round(t, 5), "min_ms": round(float(min(ms)), 5), "bytes": nbytes,
                "GBps": round(nbytes / t / 1e6, 1), "of_achievable_hbm": round(nbytes / t / 1e6 / HBM_ACHIEVABLE_GBS, 3),
                "floor_ms_at_achievable_hbm": round(nbytes / HBM_ACHIEVABLE_GBS / 1e6, 5)}

    # --- wall clock per displayed pass
    frame = np.zeros((h, w), np.uint32)
    film.clear()
    wall_film = []
    for i in range(args.warmup + args.passes):
        t0 = time.perf_counter()
        film.add_pass(tiles)
        native.check(L.pt_film_resolve(film.handle, None, frame.ctypes.data, None))
        t1 = time.perf_counter()
        if i >= args.warmup:
            wall_film.append((t1 - t0) * 1e3)
    film_frame = frame.copy()
    film.close()

    sample = np.zeros((h, w, 3), np.float32)
    wall_host, wall_copy, wall_tone = [], [], []
    for i in range(args.warmup + args.passes):
        dev.set_params(w, h, args.spp, 4, 1, 1, sample_base=i * args.spp)
        t0 = time.perf_counter()
        dev.render_tiles(tiles, sample)
        t1 = time.perf_counter()
        native.check(L.pt_to_color(sample.ctypes.data, w, h, 0, 0, w, h, frame.ctypes.data))
        t2 = time.perf_counter()
        if i >= args.warmup:
            wall_host.append((t2 - t0) * 1e3)
            wall_copy.append((t1 - t0) * 1e3)
            wall_tone.append((t2 - t1) * 1e3)
    render_ms = dev.stats()["last_ms"]
    dev.close()

    out = {
        "workload": f"C3 proxy {w}x{h}, {args.spp} spp per pass, whole frame, {args.passes} passes (median)",
        "accumulate": kernel(acc_ms, acc_bytes),
        "resolve_rgba_only": kernel(res_rgba_ms, res_rgba_bytes),
        "resolve_all_outputs": kernel(res_all_ms, res_all_bytes),
        "render_kernel_ms": round(float(render_ms), 4),
        "wall_ms_per_displayed_pass": {
            "film_add_pass_plus_resolve_rgba": round(median(wall_film), 4),
            "render_tiles_plus_host_to_color": round(median(wall_host), 4),
            "of_it_render_tiles_with_12B_per_pixel_copy": round(median(wall_copy), 4),
            "of_it_host_pt_to_color": round(median(wall_tone), 4),
        },
        "film_frame_nonblack_fraction": round(float(((film_frame & 0xFFFFFF) != 0).mean()), 4),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
