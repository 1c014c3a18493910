#!/usr/bin/env python3
"""Measurements of the film merge and export ("Mergeable films") on
the C3 proxy at 1024x1024, whole frame, one GPU, beside the accumulate kernel
of the same session:

  * film_merge_kernel's HIP-event time (pt_film_get_merge_info) for a merge of
    two films that both hold every pixel (every pixel `merged`: the full
    arithmetic, 64 B read + 32 B written per pixel);
  * the export's device-to-device copy (events on the caller's stream around
    pt_film_export_device: 32 B read + 32 B written per pixel);
  * film_accumulate_kernel's event time (pt_film_info), 76 B per pixel.

Prints one JSON line.  Usage: python tools/film_merge_bench.py [--spp 4] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from dsgpuraytracing_amd import scenes
    from dsgpuraytracing_amd.pathtracer import Device, Scene, tile_fifo
    import bench

    w = h = args.size
    sc = Scene.from_dae(scenes.proxy_path(1, bench.scene_cache_dir()), w, h)
    dev = Device(0)
    dev.upload_scene(sc)
    dev.set_camera(sc.camera)
    dev.set_params(w, h, args.spp, 4, 1, 1)
    tiles = np.asarray(tile_fifo(w, h), np.int32)
    px = w * h

    a, b = dev.film(w, h), dev.film(w, h)
    b.set_next_sample(1 << 20)
    b.add_pass(tiles)
    rec_b = torch.empty((2, h, w, 4), dtype=torch.int32, device="cuda:0")
    out = torch.empty_like(rec_b)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    b.export_device(rec_b.data_ptr())
    acc_ms, merge_ms, export_ms = [], [], []
    counts = None
    for i in range(args.warmup + args.reps):
        a.add_pass(tiles)
        a.merge_device(rec_b.data_ptr())
        mi = a.merge_info()  # (waits for the merge: the export's events then time the copy alone)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            a.export_device(out.data_ptr(), stream.cuda_stream)
            e1.record()
        e1.synchronize()
        if i >= args.warmup:
            acc_ms.append(a.info()["accumulate_ms"])
            merge_ms.append(mi["merge_ms"])
            export_ms.append(e0.elapsed_time(e1))
            counts = {k: mi[k] for k in ("merged", "taken", "empty", "refused")}
    n_last = int(a.export()[0, ..., 3].max())
    dev.close()

    def kernel(ms, nbytes):
        t = float(np.median(ms))
        return {"ms": round(t, 5), "min_ms": round(float(min(ms)), 5), "bytes": nbytes, "GBps": round(nbytes / t / 1e6, 1)}

    print(json.dumps({
        "workload": f"C3 proxy {w}x{h}, {args.spp} spp per pass, whole frame, {args.reps} repetitions (median)",
        "accumulate": kernel(acc_ms, px * 76),
        "merge": kernel(merge_ms, px * 96),
        "export_copy": kernel(export_ms, px * 64),
        "last_merge_counts": counts,
        "samples_per_pixel_at_the_end": n_last,
    }))


if __name__ == "__main__":
    main()
