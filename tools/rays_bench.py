#!/usr/bin/env python3
"""What a ray launch costs beside the camera's ("Path tracing along
the caller's rays"): on the C3 proxy at 1024x1024, 64 spp, whole frame, one GPU,

  * replay: pt_render_rays_device over the rays captured from the camera
    (PT_FLAG_RAYS_CAPTURE, sample 0), and
  * camera: pt_render_tiles_device of the same tiles with
    PT_NO_FOOTPRINT_CULL=1 -- a ray launch has no footprint cull, so this is
    the same work --

each as one warm-up launch and then `--reps` launches, every launch waited
for, timed by the HIP events around its render kernel (pt_stats.last_ms).
`--arm camera` runs with a library that lacks the ray entry points too
(PT_LIB=<another build>: the parent commit's side of the comparison).

Prints one JSON line.  Usage: python tools/rays_bench.py [--arm both] [--reps 5] [--cam cam_bunny_framed.info]
(PT_SAMPLE_GROUP=n in the environment sets both arms to one sample grouping.)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="both", choices=["both", "camera", "replay"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--cam", default=None, help="camera file under assets/ (default: the scene's own camera)")
    args = ap.parse_args()
    os.environ["PT_NO_FOOTPRINT_CULL"] = "1"  # (read at every launch; a ray launch ignores it)

    import torch
    torch.cuda.init()
    from dsgpuraytracing_amd import native, scenes
    from dsgpuraytracing_amd.pathtracer import Device, Scene, tile_fifo
    import bench

    w = h = args.size
    cam = os.path.join(ROOT, "assets", args.cam) if args.cam else None
    sc = Scene.from_dae(scenes.proxy_path(1, bench.scene_cache_dir()), w, h, cam_info=cam)
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    tiles = tile_fifo(w, h)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)

    def timed(launch):
        ms, st = [], None
        for i in range(1 + args.reps):
            launch()
            stream.synchronize()
            st = dev.stats()
            if i:
                ms.append(round(float(st["last_ms"]), 4))
        mean = sum(ms) / len(ms)
        return {"kernel_ms": ms, "mean_ms": round(mean, 4), "spread_pct": round(100 * (max(ms) - min(ms)) / mean, 2),
                "grid_blocks": st["grid_blocks"], "blocks_per_cu": st["blocks_per_cu"], "group_spp": st["group_spp"],
                "mean_radiance": round(float(out.mean().item()), 6)}

    res = {"workload": f"C3 proxy {w}x{h}, {args.spp} spp, whole frame, camera {args.cam or 'default'}, PT_NO_FOOTPRINT_CULL=1, "
                       f"PT_SAMPLE_GROUP={os.environ.get('PT_SAMPLE_GROUP')}, {args.reps} launches after one warm-up, "
                       "HIP-event kernel time",
           "library": native.LIB_PATH}
    if args.arm in ("both", "camera"):
        dev.set_params(w, h, args.spp, 4, 1, 1)
        res["camera"] = timed(lambda: dev.render_tiles_device(tiles, out.data_ptr(), stream=stream.cuda_stream))
    if args.arm in ("both", "replay"):
        rays = torch.zeros((h * w, 8), dtype=torch.float32, device="cuda:0")
        dev.set_params(w, h, 1, 4, 1, 1)
        dev.render_rays(rays, tiles=tiles, out=out, capture=True, stream=stream.cuda_stream)
        dev.set_params(w, h, args.spp, 4, 1, 1)
        res["replay"] = timed(lambda: dev.render_rays(rays, tiles=tiles, out=out, stream=stream.cuda_stream))
        if "camera" in res:
            res["replay_over_camera"] = round(res["replay"]["mean_ms"] / res["camera"]["mean_ms"], 4)
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
