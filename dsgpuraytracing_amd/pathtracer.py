"""Host-side mirror of the reference's PathTracer interface over the HIP path.

Reference: class PathTracer (src/pathtracer.h:55-272, src/pathtracer.cpp).
Same names, argument meaning and state machine for the part of the interface
that drives the hot path:

  PathTracer(ns_aa, max_ray_depth, ns_area_light, ns_diff, ns_glsy, ns_refr,
             num_threads, envmap)                       pathtracer.cpp:30-66
  set_scene / set_camera / set_frame_size               pathtracer.cpp:76-122
  start_raytracing  (all tiles of the 32x32 FIFO)       pathtracer.cpp:192-221
  raytrace_tile(tile_x, tile_y, tile_w, tile_h)         pathtracer.cpp:585-611
  raytrace_pixel(x, y)                                  pathtracer.cpp:555-583
  sampleBuffer (HDR, float32 HxWx3, row 0 = bottom)     image.h:79-205
  frameBuffer  (RGBA8 after toColor)                    image.h:174-189
  save_image(path)                                      pathtracer.cpp:649-674

Every pixel is computed by libptgpu.so on the GPU; nothing here falls back to
the CPU.  `num_threads` is accepted for interface parity and ignored (the GPU
schedules itself).  Randomness comes from the counter stream keyed by
(seed, pixel, sample) instead of std::rand() (see csrc/pt_rng.h).
"""
from __future__ import annotations

import ctypes
import enum
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import native, ptdump
from .native import check, lib

TILE = 32  # imageTileSize (pathtracer.cpp:57)


def _flags(stats) -> int:
    """stats=True: counters of the launch itself; stats="ref": counters of the
    reference's binary BVH (PT_FLAG_REF_COUNTS, SURVEY.md §8(d) cost model)."""
    if stats == "ref":
        return native.PT_FLAG_REF_COUNTS
    return native.PT_FLAG_STATS if stats else 0


class Device:
    """One pt_ctx on one GPU (CUDAPathTracer's device state, setup.h:90-148)."""

    def __init__(self, device: int = 0):
        self._lib = lib()
        h = ctypes.c_void_p()
        check(self._lib.pt_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device
        self._scene_keepalive = None
        self._films: List["Film"] = []

    def close(self):
        for f in list(getattr(self, "_films", [])):  # (pt_destroy would free them: their handles die with it)
            f.close()
        if self.handle:
            self._lib.pt_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene: "Scene", gpu_bvh: bool = False):
        """gpu_bvh: build a linear BVH on the device (pt_upload_scene_lbvh, the
        reference's PARALLEL_BUILD_BVH path) instead of using the scene's BVH."""
        fn = self._lib.pt_upload_scene_lbvh if gpu_bvh else self._lib.pt_upload_scene
        check(fn(self.handle, ctypes.byref(scene.arrays.scene)))
        self._scene_keepalive = scene

    def set_camera(self, cam: native.pt_camera):
        check(self._lib.pt_set_camera(self.handle, ctypes.byref(cam)))

    def set_params(self, width, height, spp, max_depth, ns_area_light, seed, sample_base=0):
        """sample_base: first sample index of this pass (pt_params.sample_base)."""
        p = native.pt_params(width=width, height=height, spp=spp, max_depth=max_depth,
                             ns_area_light=ns_area_light, seed=seed & 0xFFFFFFFF, sample_base=sample_base)
        check(self._lib.pt_set_params(self.handle, ctypes.byref(p)))
        self._frame = (int(height), int(width))

    @staticmethod
    def _tiles(tiles: Sequence[Tuple[int, int, int, int]]):
        """pt_tile[] view of the tile list (an int32 (n, 4) array; the caller
        keeps it alive for the duration of the call)."""
        if isinstance(tiles, np.ndarray) and tiles.dtype == np.int32 and tiles.flags.c_contiguous:
            arr = tiles.reshape(-1, 4)
        else:
            arr = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4))
        return arr, arr.ctypes.data_as(ctypes.POINTER(native.pt_tile))

    def _check_frame(self, arr: np.ndarray, channels: int, dtype, what: str):
        """The native side writes (x + y*W)*channels elements of `arr` for the
        frame of the last set_params: anything smaller is refused here."""
        hw = getattr(self, "_frame", None)
        if hw is None:  # no frame yet: the native call refuses to render (PT_E_NOSCENE)
            return
        if arr.dtype != dtype or not arr.flags.c_contiguous or arr.shape != (hw[0], hw[1], channels):
            raise ValueError(f"{what}: need a C-contiguous {np.dtype(dtype).name} array of shape "
                             f"{(hw[0], hw[1], channels)}, got {arr.dtype} {arr.shape}")

    def render_tiles(self, tiles, out: np.ndarray, stats: bool = False):
        self._check_frame(out, 3, np.float32, "render_tiles")
        keep, arr = self._tiles(tiles)
        flags = _flags(stats)
        check(self._lib.pt_render_tiles(self.handle, arr, len(keep), out.ctypes.data, flags))

    def render_tiles_device(self, tiles, out_ptr: int, stream: int = 0, stats: bool = False, packed: bool = False,
                            out_floats: Optional[int] = None):
        """packed=True (or 32): out_ptr holds len(tiles)*32*32*3 floats, tile
        i's pixel (x, y) at [(i*1024 + (y-ty)*32 + (x-tx))*3] (PT_FLAG_PACKED);
        packed=16: 16x16 slots (PT_FLAG_PACKED16, tiles <= 16x16); else a
        whole H x W x 3 frame.  out_floats: the buffer's size in floats, checked
        against what the layout writes (the library sees only a pointer)."""
        keep, arr = self._tiles(tiles)
        if out_floats is not None:
            if getattr(self, "_frame", None) is None:
                raise ValueError("render_tiles_device: set_params first")
            need = len(keep) * _slot(packed) ** 2 * 3 if packed else self._frame[0] * self._frame[1] * 3
            if out_floats < need:
                raise ValueError(f"render_tiles_device: output holds {out_floats} floats, the "
                                 f"{'packed' if packed else 'frame'} layout writes {need}")
        flags = _flags(stats) | _packed_flag(packed)
        check(self._lib.pt_render_tiles_device(self.handle, arr, len(keep), ctypes.c_void_p(out_ptr),
                                               ctypes.c_void_p(stream or None), flags))

    def render_frames_device(self, tiles, out_ptrs, seeds, stream: int = 0, packed: bool = False,
                             out_floats: Optional[int] = None):
        """pt_render_frames_device: len(seeds) (1..8) frames of the same tiles in
        one launch, frame f keyed by seeds[f] into out_ptrs[f] (each laid out as
        render_tiles_device's out_ptr); every image equals its own
        render_tiles_device call with that seed."""
        n = len(seeds)
        if n != len(out_ptrs) or not 1 <= n <= native.PT_MAX_FRAMES:
            raise ValueError(f"render_frames_device: 1..{native.PT_MAX_FRAMES} frames, one output each")
        keep, arr = self._tiles(tiles)
        if out_floats is not None:
            if getattr(self, "_frame", None) is None:
                raise ValueError("render_frames_device: set_params first")
            need = len(keep) * _slot(packed) ** 2 * 3 if packed else self._frame[0] * self._frame[1] * 3
            if out_floats < need:
                raise ValueError(f"render_frames_device: outputs hold {out_floats} floats, the "
                                 f"{'packed' if packed else 'frame'} layout writes {need}")
        sd = (ctypes.c_uint32 * n)(*[int(v) & 0xFFFFFFFF for v in seeds])
        op = (ctypes.c_void_p * n)(*[int(v) for v in out_ptrs])
        flags = _packed_flag(packed)
        check(self._lib.pt_render_frames_device(self.handle, arr, len(keep), n, sd, op,
                                                ctypes.c_void_p(stream or None), flags))

    def submit_tile(self, tile, hdr: np.ndarray, rgba: Optional[np.ndarray] = None):
        """pt_tile_submit: queue one tile; its pixels land in `hdr` ((H, W, 3)
        float32) and, toColor'd, in `rgba` ((H, W, 4) uint8) when its batch
        completes.  Both arrays must stay alive until finish_tiles() returns
        (whatever it returns: it waits for every launched batch first).  The
        completion thread writes them long after this call, so their shapes
        are checked against the frame of the last set_params here."""
        self._check_frame(hdr, 3, np.float32, "submit_tile (hdr)")
        if rgba is not None:
            self._check_frame(rgba, 4, np.uint8, "submit_tile (rgba)")
        t = native.pt_tile(*[int(v) for v in tile])
        check(self._lib.pt_tile_submit(self.handle, ctypes.byref(t), hdr.ctypes.data,
                                       None if rgba is None else rgba.ctypes.data))

    def finish_tiles(self):
        """pt_tile_finish: render what is queued, wait for every submitted tile."""
        check(self._lib.pt_tile_finish(self.handle))

    def intersect(self, o, d, max_t):
        o = np.ascontiguousarray(o, np.float64)
        d = np.ascontiguousarray(d, np.float64)
        max_t = np.ascontiguousarray(max_t, np.float64)
        n = len(max_t)
        hit = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.int32)
        anyh = np.zeros(n, np.int32)
        check(self._lib.pt_intersect(self.handle, n, o.ctypes.data, d.ctypes.data, max_t.ctypes.data,
                                     hit.ctypes.data, t.ctypes.data, prim.ctypes.data, anyh.ctypes.data))
        return hit, t, prim, anyh

    def read_bvh(self) -> dict:
        """The render tree as it lies in device memory (pt_debug_bvh_info and
        pt_debug_read_bvh; include/ptgpu.h has the byte layouts): `info` (the
        pt_bvh_info fields, root_lo / root_hi as float32 arrays), `nodes4`
        (n4, 32) float32 -- rows of lo.x, hi.x, lo.y, hi.y, lo.z, hi.z of the
        four slots, then the four references, read them with
        nodes4[:, 24:28].view(int32) --, `nodes2` (n2, 16) float32 likewise
        (references in columns 12:14), `prims` (n, 12) float32, `norms` (n, 9)
        float32 and `prim_map` (n,) int32, or None when the tree keeps the
        caller's order."""
        info = native.pt_bvh_info()
        check(self._lib.pt_debug_bvh_info(self.handle, ctypes.byref(info)))
        n = int(info.n_prims)
        nodes4 = np.zeros((int(info.n_nodes4), 32), np.float32)
        nodes2 = np.zeros((int(info.n_nodes2), 16), np.float32)
        prims = np.zeros((n, 12), np.float32)
        norms = np.zeros((n, 9), np.float32)
        prim_map = np.zeros(n, np.int32) if info.has_prim_map else None
        check(self._lib.pt_debug_read_bvh(self.handle, nodes4.ctypes.data, nodes2.ctypes.data if nodes2.size else None,
                                          prims.ctypes.data, norms.ctypes.data,
                                          None if prim_map is None else prim_map.ctypes.data))
        d = {k: int(getattr(info, k)) for k in ("n_prims", "n_nodes4", "n_nodes2", "bvh_stack", "has_prim_map")}
        d["root_lo"] = np.array(list(info.root_lo), np.float32)
        d["root_hi"] = np.array(list(info.root_hi), np.float32)
        return {"info": d, "nodes4": nodes4, "nodes2": nodes2, "prims": prims, "norms": norms, "prim_map": prim_map}

    def env_probe(self, u1=(), u2=(), dirs=()) -> dict:
        """pt_debug_env_probe: the render kernel's environment-light functions
        on the uploaded tables.  For the pairs (u1, u2) in [0, 1): `row`, `col`
        (int32), `row_pair`, `col_pair` ((n, 2) float32: prev, cur), `wi`
        (n, 3), `pdf`, `tu`, `tv` (n,) and `radiance` (n, 3); for the unit
        directions `dirs` (m, 3): `dir_radiance` (m, 3).  Invalid queries are
        refused (PtError) before anything runs on the device."""
        u1 = np.ascontiguousarray(u1, np.float32).reshape(-1)
        u2 = np.ascontiguousarray(u2, np.float32).reshape(-1)
        if len(u1) != len(u2):
            raise ValueError("env_probe: u1 and u2 differ in length")
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n, m = len(u1), len(d)
        o = {"row": np.zeros(n, np.int32), "col": np.zeros(n, np.int32), "row_pair": np.zeros((n, 2), np.float32),
             "col_pair": np.zeros((n, 2), np.float32), "wi": np.zeros((n, 3), np.float32), "pdf": np.zeros(n, np.float32),
             "tu": np.zeros(n, np.float32), "tv": np.zeros(n, np.float32), "radiance": np.zeros((n, 3), np.float32),
             "dir_radiance": np.zeros((m, 3), np.float32)}
        ptr = lambda a, k: a.ctypes.data if k else None
        check(self._lib.pt_debug_env_probe(
            self.handle, n, ptr(u1, n), ptr(u2, n), *[ptr(o[k], n) for k in ("row", "col", "row_pair", "col_pair", "wi",
                                                                            "pdf", "tu", "tv", "radiance")],
            m, ptr(d, m), ptr(o["dir_radiance"], m)))
        return o

    def render_features(self, tiles=None) -> dict:
        """First-hit feature buffers of `tiles` (the whole frame by default;
        pt_render_features, waits): `normal` (H, W, 3) float32, `position`
        (H, W, 3) float32, `depth` (H, W) float32 -- the ray parameter of the
        hit --, `bsdf` (H, W) int32 (-1: miss) and `albedo` (H, W, 3) float32,
        looked up from the scene's BSDF table (0 on a miss).  Pixels outside
        the tiles hold the miss record.  `records` is the raw (2, H, W, 4)
        float32 buffer as pt_denoise_device reads it."""
        hw = getattr(self, "_frame", None)
        if hw is None:
            raise ValueError("render_features: set_params first")
        h, w = hw
        rec = np.zeros((2, h, w, 4), np.float32)
        rec[0, :, :, 3] = np.int32(-1).view(np.float32)
        keep, arr = self._tiles(tile_fifo(w, h) if tiles is None else tiles)
        check(self._lib.pt_render_features(self.handle, arr, len(keep), rec.ctypes.data))
        bsdf = rec[0, :, :, 3].view(np.int32).copy()
        albedo = np.zeros((h, w, 3), np.float32)
        sc = self._scene_keepalive
        if sc is not None:
            table = np.array([list(b.albedo) for b in sc.arrays.bsdfs], np.float32).reshape(-1, 3)
            hit = bsdf >= 0
            albedo[hit] = table[bsdf[hit]]
        return {"normal": rec[0, :, :, :3].copy(), "position": rec[1, :, :, :3].copy(), "depth": rec[1, :, :, 3].copy(),
                "bsdf": bsdf, "albedo": albedo, "records": rec}

    def render_features_device(self, tiles, feat_ptr: int, stream: int = 0):
        """pt_render_features_device: the feature records of `tiles` into the
        device buffer at feat_ptr (2 * W * H records of 16 B); queued on `stream`."""
        keep, arr = self._tiles(tiles)
        check(self._lib.pt_render_features_device(self.handle, arr, len(keep), ctypes.c_void_p(feat_ptr or None),
                                                  ctypes.c_void_p(stream or None)))

    _TRACE_MODES = {"closest": native.PT_TRACE_CLOSEST, "occluded": native.PT_TRACE_OCCLUDED}

    @staticmethod
    def _trace_records(rec: np.ndarray) -> dict:
        """The (n, 8) float32 closest-hit records as named views."""
        return {"t": rec[:, 0], "u": rec[:, 1], "v": rec[:, 2], "prim": rec[:, 3].view(np.int32),
                "normal": rec[:, 4:7], "bsdf": rec[:, 7].view(np.int32), "records": rec}

    def trace_rays(self, rays, mode: str = "closest", out=None, stream: int = 0):
        """Casts the caller's rays through the uploaded scene (pt_trace_rays*).
        `rays` is (n, 8) float32: {o.x, o.y, o.z, tmax, d.x, d.y, d.z, unused},
        d of unit length.

        A numpy array goes through the host call, which waits: "closest"
        returns the dict {"t", "u", "v", "prim", "normal", "bsdf", "records"}
        of views of the (n, 8) float32 record array (a miss: t = -1, prim =
        bsdf = -1), "occluded" a boolean (n,) mask.

        An object with data_ptr() on the device (a torch tensor; torch is
        imported only then) goes to the device entry point, queued on `stream`
        (default: torch's current stream): "closest" returns the (n, 8)
        float32 record tensor, "occluded" the packed int32 words (ceil(n / 64)
        * 2; ray i is bit i % 32 of word i // 32), on the rays' device.  `out`
        is the array or tensor to write instead of a new one."""
        if mode not in self._TRACE_MODES:
            raise ValueError(f"trace_rays: mode must be 'closest' or 'occluded', got {mode!r}")
        m = self._TRACE_MODES[mode]
        if hasattr(rays, "data_ptr"):
            return self._trace_rays_torch(rays, m, out, stream)
        rays = np.ascontiguousarray(rays, np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"trace_rays: need an (n, 8) float32 array, got {rays.shape}")
        n = len(rays)
        words = (n + 63) // 64 * 2
        shape, dtype = ((n, 8), np.float32) if m == native.PT_TRACE_CLOSEST else ((words,), np.uint32)
        if out is None:
            out = np.zeros(shape, dtype)
        elif out.dtype != dtype or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"trace_rays: out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        check(self._lib.pt_trace_rays(self.handle, n, rays.ctypes.data if n else None, out.ctypes.data if n else None, m))
        if m == native.PT_TRACE_CLOSEST:
            return self._trace_records(out)
        return np.unpackbits(out.view(np.uint8), bitorder="little")[:n].astype(bool)

    def _trace_rays_torch(self, rays, m: int, out, stream: int):
        import torch
        if (not rays.is_cuda or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8
                or not rays.is_contiguous()):
            raise ValueError("trace_rays: need a contiguous (n, 8) float32 tensor on the device")
        if rays.device.index != self.device:
            raise ValueError(f"trace_rays: the rays are on {rays.device}, the context on device {self.device}")
        n = rays.shape[0]
        words = (n + 63) // 64 * 2
        shape, dtype = ((n, 8), torch.float32) if m == native.PT_TRACE_CLOSEST else ((words,), torch.int32)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=rays.device)
        elif (out.device != rays.device or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"trace_rays: out must be a contiguous {dtype} tensor of shape {shape} on {rays.device}")
        self._on_torch_stream(rays.device, stream, lambda s: check(self._lib.pt_trace_rays_device(
            self.handle, n, ctypes.c_void_p(rays.data_ptr() if n else None), ctypes.c_void_p(out.data_ptr() if n else None),
            m, ctypes.c_void_p(s))))
        return out

    def _on_torch_stream(self, device, stream: int, call):
        """Runs call(stream handle) in the order of `stream`, or of torch's
        current stream of `device`.  The library takes a NULL stream for the
        context's own, so torch's default stream (handle 0) cannot be handed
        over: the call then runs on a side stream of this Device that waits
        for the default stream and that the default stream waits for."""
        import torch
        if stream:
            return call(stream)
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream:
            return call(cur.cuda_stream)
        side = getattr(self, "_torch_side", None)
        if side is None:
            side = self._torch_side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        call(side.cuda_stream)
        cur.wait_stream(side)

    def camera_rays(self, tiles=None, out=None, stream: int = 0):
        """The pixel-centre camera rays render_features traces, of `tiles` (the
        whole frame by default), at row x + y * W of an (H * W, 8) float32 ray
        buffer as trace_rays takes it (pt_camera_rays_device).  Without `out`
        (or with a numpy array) the result is a numpy array, rows outside the
        tiles left as they were (zero in a new one), and the call waits; a
        device tensor `out` is filled on `stream` (default: torch's current
        stream) and returned."""
        hw = getattr(self, "_frame", None)
        if hw is None:
            raise ValueError("camera_rays: set_params first")
        h, w = hw
        keep, arr = self._tiles(tile_fifo(w, h) if tiles is None else tiles)
        if out is not None and hasattr(out, "data_ptr"):
            import torch
            if (not out.is_cuda or out.device.index != self.device or out.dtype != torch.float32
                    or tuple(out.shape) != (h * w, 8) or not out.is_contiguous()):
                raise ValueError(f"camera_rays: out must be a contiguous float32 tensor of shape {(h * w, 8)} on device "
                                 f"{self.device}")
            self._on_torch_stream(out.device, stream, lambda s: check(self._lib.pt_camera_rays_device(
                self.handle, arr, len(keep), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s))))
            return out
        import torch  # (the numpy form stages through a torch tensor: the library hands out no device memory)
        if out is None:
            out = np.zeros((h * w, 8), np.float32)
        elif out.dtype != np.float32 or out.shape != (h * w, 8) or not out.flags.c_contiguous:
            raise ValueError(f"camera_rays: out must be a C-contiguous float32 array of shape {(h * w, 8)}")
        dev = torch.device("cuda", self.device)
        t = torch.from_numpy(out).to(dev)
        self._on_torch_stream(dev, 0, lambda s: check(self._lib.pt_camera_rays_device(
            self.handle, arr, len(keep), ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(s))))
        out[...] = t.cpu().numpy()
        return out

    def render_rays(self, rays, tiles=None, out=None, capture: bool = False, stream: int = 0):
        """Path-traces the caller's rays (pt_render_rays*): pixel p = x + y * W
        of the frame of the last set_params follows row p of `rays`, an
        (H * W, 8) float32 ray buffer as trace_rays takes it and camera_rays
        writes it, with the params' spp, depth, seed and sample_base; returns
        the (H, W, 3) float32 radiance, written inside `tiles` (the whole frame
        by default) only.  capture=True (spp 1): the camera's rays of sample
        sample_base are generated, written into `rays` and rendered -- the
        image is render_tiles_device's.

        A numpy `rays` goes through the host call, which waits (a capture
        writes the array in place; `out` is a numpy array or a new one); a
        torch device tensor through the device call, queued on `stream`
        (default: torch's current stream), `out` a device tensor or a new,
        zeroed one."""
        hw = getattr(self, "_frame", None)
        if hw is None:
            raise ValueError("render_rays: set_params first")
        h, w = hw
        keep, arr = self._tiles(tile_fifo(w, h) if tiles is None else tiles)
        flags = native.PT_FLAG_RAYS_CAPTURE if capture else 0
        if hasattr(rays, "data_ptr"):
            import torch
            if (not rays.is_cuda or rays.device.index != self.device or rays.dtype != torch.float32
                    or tuple(rays.shape) != (h * w, 8) or not rays.is_contiguous()):
                raise ValueError(f"render_rays: need a contiguous float32 tensor of shape {(h * w, 8)} on device "
                                 f"{self.device}")
            if out is None:
                out = torch.zeros((h, w, 3), dtype=torch.float32, device=rays.device)
            elif (not hasattr(out, "data_ptr") or out.device != rays.device or out.dtype != torch.float32
                  or tuple(out.shape) != (h, w, 3) or not out.is_contiguous()):
                raise ValueError(f"render_rays: out must be a contiguous float32 tensor of shape {(h, w, 3)} on "
                                 f"{rays.device}")
            self._on_torch_stream(rays.device, stream, lambda s: check(self._lib.pt_render_rays_device(
                self.handle, arr, len(keep), ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(s), flags)))
            return out
        if (not isinstance(rays, np.ndarray) or rays.dtype != np.float32 or rays.shape != (h * w, 8)
                or not rays.flags.c_contiguous or (capture and not rays.flags.writeable)):
            raise ValueError(f"render_rays: need a C-contiguous float32 array of shape {(h * w, 8)}")
        if out is None:
            out = np.zeros((h, w, 3), np.float32)
        else:
            self._check_frame(out, 3, np.float32, "render_rays")
        check(self._lib.pt_render_rays(self.handle, arr, len(keep), rays.ctypes.data, out.ctypes.data, flags))
        return out

    def trace_info(self) -> dict:
        """pt_get_trace_info: {rays, hits, invalid, trace_ms} of the last trace (waits for it)."""
        i = native.pt_trace_info()
        check(self._lib.pt_get_trace_info(self.handle, ctypes.byref(i)))
        return {"rays": int(i.rays), "hits": int(i.hits), "invalid": int(i.invalid), "trace_ms": float(i.trace_ms)}

    def stats(self) -> dict:
        s = native.pt_stats()
        check(self._lib.pt_get_stats(self.handle, ctypes.byref(s)))
        out = {k: getattr(s, k) for k, _ in native.pt_stats._fields_}
        out["section_clocks"] = list(s.section_clocks)
        out["slot_latency_hist"] = list(s.slot_latency_hist)
        out["wave_span"] = list(s.wave_span)
        out["lane_iters"] = list(s.lane_iters)
        out["footprint"] = list(s.footprint)
        out["node_census"] = list(s.node_census)
        out["frames_per_launch"] = int(s.frames_per_launch)
        out["tile_zorder"] = int(s.tile_zorder)
        return out

    def launch_times(self, n: int = 256):
        """(kernel_ms, resolve_ms) arrays of the last <= n renders, oldest
        first, from HIP events recorded around each launch on its stream
        (pt_get_launch_times; waits for them)."""
        k = np.zeros(n, np.float32)
        r = np.zeros(n, np.float32)
        got = ctypes.c_int32(0)
        check(self._lib.pt_get_launch_times(self.handle, k.ctypes.data, r.ctypes.data, n, ctypes.byref(got)))
        return k[:got.value].copy(), r[:got.value].copy()

    def film(self, width: int, height: int) -> "Film":
        """A progressive film of this context (pt_film_create): device memory
        that accumulates passes and resolves on the GPU."""
        return Film(self, width, height)

    def wave_trace(self) -> np.ndarray:
        """Per-wave records of the last stats launch (pt_get_wave_trace):
        int64 (waves, 11) = start, first empty-queue time (-1: never), end,
        (XCC id << 32 | HW_ID), camera samples started, sum and max of the
        work-slot latencies (wall-clock ticks, 100 MHz), per-ray maxima of
        traversal iterations stepped (<< 32) | idle, and of traversal phases,
        traversal iterations and shading rounds after the queue drained."""
        n = ctypes.c_int64(0)
        check(self._lib.pt_get_wave_trace(self.handle, None, 0, ctypes.byref(n)))
        buf = np.zeros((n.value, 11), np.int64)
        check(self._lib.pt_get_wave_trace(self.handle, buf.ctypes.data, buf.size, ctypes.byref(n)))
        return buf


class Film:
    """One pt_film: the device-resident running result of progressive passes
    (include/ptgpu.h: the per-pixel arithmetic, stream semantics and errors)."""

    def __init__(self, dev: Device, width: int, height: int):
        self._lib = dev._lib
        self._dev = dev
        self.handle = None
        h = ctypes.c_void_p()
        check(self._lib.pt_film_create(dev.handle, int(width), int(height), ctypes.byref(h)))
        self.handle = h
        self.width, self.height = int(width), int(height)
        dev._films.append(self)

    def close(self):
        if self.handle:
            self._lib.pt_film_destroy(self.handle)
            self.handle = None
            if self in self._dev._films:
                self._dev._films.remove(self)

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass

    def clear(self, stream: int = 0):
        check(self._lib.pt_film_clear(self.handle, ctypes.c_void_p(stream or None)))

    def add_pass(self, tiles, stream: int = 0):
        """Render `tiles` with the context's params at the film's next sample
        index and accumulate them (pt_film_add_pass); returns once queued."""
        keep, arr = Device._tiles(tiles)
        check(self._lib.pt_film_add_pass(self.handle, arr, len(keep), ctypes.c_void_p(stream or None)))

    def add_pass_rays(self, rays, tiles, stream: int = 0):
        """add_pass with the pass rendered by replay of `rays` (pt_film_add_pass_rays):
        a contiguous (H * W, 8) float32 device tensor (anything with data_ptr())
        as Device.render_rays takes it; returns once queued."""
        if not hasattr(rays, "data_ptr"):
            raise ValueError("add_pass_rays: the rays are a device tensor")
        if (tuple(rays.shape) != (self.height * self.width, 8) or rays.element_size() != 4 or not rays.is_contiguous()):
            raise ValueError(f"add_pass_rays: need a contiguous float32 tensor of shape {(self.height * self.width, 8)}")
        keep, arr = Device._tiles(tiles)
        check(self._lib.pt_film_add_pass_rays(self.handle, arr, len(keep), ctypes.c_void_p(rays.data_ptr()),
                                              ctypes.c_void_p(stream or None)))

    def resolve(self, hdr: bool = True, rgba: bool = True, err: bool = True):
        """(hdr (H, W, 3) float32, rgba (H, W, 4) uint8, err (H, W) float32) of
        the whole frame (pt_film_resolve; waits).  An output switched off is
        None and is neither computed nor copied."""
        h, w = self.height, self.width
        o_hdr = np.empty((h, w, 3), np.float32) if hdr else None
        o_rgba = np.empty((h, w), np.uint32) if rgba else None
        o_err = np.empty((h, w), np.float32) if err else None
        check(self._lib.pt_film_resolve(self.handle, *[None if a is None else a.ctypes.data
                                                       for a in (o_hdr, o_rgba, o_err)]))
        return o_hdr, None if o_rgba is None else o_rgba.view(np.uint8).reshape(h, w, 4), o_err

    def resolve_device(self, hdr_ptr: int = 0, rgba_ptr: int = 0, err_ptr: int = 0, stream: int = 0):
        """pt_film_resolve_device: device pointers (0 = not wanted) of W*H*3
        float32, W*H uint32 and W*H float32; queued on `stream`."""
        check(self._lib.pt_film_resolve_device(self.handle, ctypes.c_void_p(hdr_ptr or None),
                                               ctypes.c_void_p(rgba_ptr or None), ctypes.c_void_p(err_ptr or None),
                                               ctypes.c_void_p(stream or None)))

    def tile_error(self, tiles) -> np.ndarray:
        """Per listed tile (clipped to the frame) the maximum of the error over
        its pixels: +inf while a pixel has fewer than two passes (waits)."""
        keep, arr = Device._tiles(tiles)
        out = np.zeros(len(keep), np.float32)
        check(self._lib.pt_film_tile_error(self.handle, arr, len(keep), out.ctypes.data))
        return out

    def set_features(self, tiles=None, stream: int = 0):
        """Render the first-hit feature records of `tiles` (the whole frame by
        default) with the context's current camera (pt_film_set_features);
        clear() marks them absent again."""
        keep, arr = Device._tiles(tile_fifo(self.width, self.height) if tiles is None else tiles)
        check(self._lib.pt_film_set_features(self.handle, arr, len(keep), ctypes.c_void_p(stream or None)))

    def denoise(self, params=None, hdr: bool = True, rgba: bool = True):
        """(hdr (H, W, 3) float32, rgba (H, W, 4) uint8) of the film's mean
        filtered by the edge-avoiding denoiser (pt_film_denoise; waits); the
        film itself is unchanged.  params: a native.pt_denoise_params, a dict
        of its fields over the defaults, or None for the defaults.  An output
        switched off is None."""
        h, w = self.height, self.width
        o_hdr = np.empty((h, w, 3), np.float32) if hdr else None
        o_rgba = np.empty((h, w), np.uint32) if rgba else None
        p = denoise_params(params)
        check(self._lib.pt_film_denoise(self.handle, None if p is None else ctypes.byref(p),
                                        *[None if a is None else a.ctypes.data for a in (o_hdr, o_rgba)]))
        return o_hdr, None if o_rgba is None else o_rgba.view(np.uint8).reshape(h, w, 4)

    def denoise_device(self, hdr_ptr: int = 0, rgba_ptr: int = 0, params=None, stream: int = 0):
        """pt_film_denoise_device: device pointers (0 = not wanted) of W*H*3
        float32 and W*H uint32; queued on `stream`."""
        p = denoise_params(params)
        check(self._lib.pt_film_denoise_device(self.handle, None if p is None else ctypes.byref(p),
                                               ctypes.c_void_p(hdr_ptr or None), ctypes.c_void_p(rgba_ptr or None),
                                               ctypes.c_void_p(stream or None)))

    def reproject(self, params=None, stream: int = 0):
        """Keep the film across a camera move (pt_film_reproject): the context
        already holds the NEW camera (Device.set_camera); every pixel takes
        over the records of the old frame's pixel that saw the same diffuse or
        emissive first hit, or is reset.  params: a native.pt_reproject_params,
        a dict of its fields over the defaults, or None; returns once queued."""
        p = reproject_params(params)
        check(self._lib.pt_film_reproject(self.handle, None if p is None else ctypes.byref(p),
                                          ctypes.c_void_p(stream or None)))

    def reproject_info(self) -> dict:
        """kept / reset pixel counts and the gather kernel's device time of the
        last reproject (pt_film_get_reproject_info; waits)."""
        i = native.pt_reproject_info()
        check(self._lib.pt_film_get_reproject_info(self.handle, ctypes.byref(i)))
        return {k: getattr(i, k) for k, _ in native.pt_reproject_info._fields_}

    def set_next_sample(self, next_sample: int):
        """The sample index the next pass starts at (pt_film_set_next_sample)."""
        check(self._lib.pt_film_set_next_sample(self.handle, int(next_sample)))

    def info(self) -> dict:
        i = native.pt_film_info()
        check(self._lib.pt_film_get_info(self.handle, ctypes.byref(i)))
        return {k: getattr(i, k) for k, _ in native.pt_film_info._fields_}

    def export(self) -> np.ndarray:
        """The film's records, (2, H, W, 4) uint32: plane 0 {sum.r, sum.g,
        sum.b, n}, plane 1 {mu, M2, k, pad}, floats as their bits
        (pt_film_export; waits)."""
        out = np.empty((2, self.height, self.width, 4), np.uint32)
        check(self._lib.pt_film_export(self.handle, out.ctypes.data))
        return out

    def export_device(self, ptr: int, stream: int = 0):
        """pt_film_export_device: the records into the device buffer at `ptr`
        (2 * H * W * 16 bytes); queued on `stream`."""
        check(self._lib.pt_film_export_device(self.handle, ctypes.c_void_p(ptr or None),
                                              ctypes.c_void_p(stream or None)))

    def merge(self, records: np.ndarray):
        """film <- film (+) records (pt_film_merge; waits): `records` as
        export() returns them, of a film of this frame size.  Not bitwise
        commutative: merge in a fixed order for reproducible bits."""
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        if rec.shape != (2, self.height, self.width, 4):
            raise ValueError(f"Film.merge: need records of shape {(2, self.height, self.width, 4)}, got {rec.shape}")
        check(self._lib.pt_film_merge(self.handle, rec.ctypes.data))

    def merge_device(self, ptr: int, stream: int = 0):
        """pt_film_merge_device: the records in the device buffer at `ptr`
        (not the film's own) merged into the film; queued on `stream`."""
        check(self._lib.pt_film_merge_device(self.handle, ctypes.c_void_p(ptr or None),
                                             ctypes.c_void_p(stream or None)))

    def merge_info(self) -> dict:
        """merged / taken / empty / refused pixel counts and the kernel's
        device time of the last merge (pt_film_get_merge_info; waits)."""
        i = native.pt_film_merge_info()
        check(self._lib.pt_film_get_merge_info(self.handle, ctypes.byref(i)))
        return {k: getattr(i, k) for k, _ in native.pt_film_merge_info._fields_}

    def save(self, path):
        """A checkpoint: the records, the frame size and the next sample index
        in one .npz (np.savez: a path without the suffix gets it)."""
        np.savez(path, records=self.export(), width=np.int64(self.width), height=np.int64(self.height),
                 next_sample=np.uint64(self.info()["next_sample"]))

    @classmethod
    def load(cls, dev: Device, path) -> "Film":
        """A new film of `dev` from a checkpoint of save(): the merge into the
        clear film takes every record bit for bit, then the next sample index
        is set, so further passes continue the saved render."""
        with np.load(path) as z:
            rec, w, h, nxt = z["records"], int(z["width"]), int(z["height"]), int(z["next_sample"])
        if not 0 <= nxt < 2 ** 32:  # (pt_film_set_next_sample takes a uint32: a film at 2^32 has no sample left)
            raise ValueError(f"Film.load: next_sample {nxt} of {path!r} is outside 0 .. 2^32 - 1")
        film = cls(dev, w, h)
        try:
            film.merge(rec)
            film.set_next_sample(nxt)
        except Exception:
            film.close()
            raise
        return film


def to_color_device(dev: Device, hdr_ptr: int, w: int, h: int, rgba_ptr: int, rect=None, stream: int = 0):
    """pt_to_color_device: to_color of the device buffer at hdr_ptr ((h, w, 3)
    float32) into rgba_ptr ((h, w) uint32) for rect = (x0, y0, x1, y1), the
    whole frame by default; queued on `stream`."""
    x0, y0, x1, y1 = (0, 0, w, h) if rect is None else (int(v) for v in rect)
    check(dev._lib.pt_to_color_device(dev.handle, ctypes.c_void_p(hdr_ptr or None), int(w), int(h), x0, y0, x1, y1,
                                      ctypes.c_void_p(rgba_ptr or None), ctypes.c_void_p(stream or None)))


def denoise_params(params=None):
    """None (the library's defaults), a native.pt_denoise_params, or a dict of
    its fields laid over pt_denoise_params_default."""
    if params is None or isinstance(params, native.pt_denoise_params):
        return params
    p = native.pt_denoise_params()
    check(lib().pt_denoise_params_default(ctypes.byref(p)))
    for k, v in dict(params).items():
        if k not in ("iterations", "normal_squarings", "sigma_l", "sigma_p"):
            raise ValueError(f"denoise_params: no field {k!r}")
        setattr(p, k, v)
    return p


def denoise_device(dev: Device, cv_ptr: int, feat_ptr: int, w: int, h: int, out_ptr: int, params=None, stream: int = 0):
    """pt_denoise_device: the filter on device buffers -- cv_ptr ((h, w, 4)
    float32: colour and the variance of the mean luminance) and feat_ptr (a
    feature buffer, 2 * w * h records) into out_ptr ((h, w, 4) float32, not
    overlapping cv_ptr); queued on `stream`."""
    p = denoise_params(params)
    check(dev._lib.pt_denoise_device(dev.handle, ctypes.c_void_p(cv_ptr or None), ctypes.c_void_p(feat_ptr or None),
                                     int(w), int(h), None if p is None else ctypes.byref(p),
                                     ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)))


def reproject_params(params=None):
    """None (the library's defaults), a native.pt_reproject_params, or a dict
    of its fields laid over pt_reproject_params_default."""
    if params is None or isinstance(params, native.pt_reproject_params):
        return params
    p = native.pt_reproject_params()
    check(lib().pt_reproject_params_default(ctypes.byref(p)))
    for k, v in dict(params).items():
        if k not in ("normal_cos_min", "sigma_p", "max_samples"):
            raise ValueError(f"reproject_params: no field {k!r}")
        setattr(p, k, v)
    return p


def reproject_device(dev: Device, old_camera: native.pt_camera, rec_ptr: int, feat_old_ptr: int, feat_new_ptr: int,
                     w: int, h: int, out_ptr: int, bsdf_types=None, params=None, counts_ptr: int = 0, stream: int = 0):
    """pt_reproject_device: the reprojection gather on device buffers -- the
    film records at rec_ptr ((2, h, w, 4) uint32) seen by old_camera with the
    features at feat_old_ptr, through the new camera's features at
    feat_new_ptr, into out_ptr (not overlapping rec_ptr).  bsdf_types: the
    PT_BSDF_* type per BSDF index (None: the uploaded scene's); counts_ptr: two
    uint64 on the device, overwritten with (kept, reset); queued on `stream`."""
    p = reproject_params(params)
    types = None if bsdf_types is None else np.ascontiguousarray(bsdf_types, dtype=np.int32)
    check(dev._lib.pt_reproject_device(dev.handle, ctypes.byref(old_camera), ctypes.c_void_p(rec_ptr or None),
                                       ctypes.c_void_p(feat_old_ptr or None), ctypes.c_void_p(feat_new_ptr or None),
                                       int(w), int(h), None if types is None else types.ctypes.data,
                                       0 if types is None else len(types), None if p is None else ctypes.byref(p),
                                       ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(counts_ptr or None),
                                       ctypes.c_void_p(stream or None)))


class Scene:
    """A flattened scene (what BVHAccel + the lights hand to the GPU seam)."""

    def __init__(self, arrays: native.SceneArrays):
        self.arrays = arrays

    @classmethod
    def from_dump(cls, path: str) -> "Scene":
        return cls(native.SceneArrays(ptdump.read(path)))

    @classmethod
    def from_dae(cls, path: str, width: int, height: int, cam_info: Optional[str] = None,
                 envmap: Optional[str] = None) -> "Scene":
        """envmap: OpenEXR lat-long map for the EnvironmentLight (the reference's -e)."""
        from . import scene_loader
        return cls(native.SceneArrays(scene_loader.load_dae(path, width, height, cam_info, envmap)))

    @property
    def camera(self) -> native.pt_camera:
        return self.arrays.camera


class State(enum.IntEnum):
    INIT = 0
    READY = 1
    VISUALIZE = 2
    RENDERING = 3
    DONE = 4


def _slot(packed) -> int:
    """Packed slot edge of a `packed` argument: True / 32 -> 32, 16 -> 16."""
    return 16 if packed == 16 else 32


def _packed_flag(packed) -> int:
    if not packed:
        return 0
    return native.PT_FLAG_PACKED16 if _slot(packed) == 16 else native.PT_FLAG_PACKED


def probe_rays(origin, w: int, h: int) -> np.ndarray:
    """The (h * w, 8) float32 rays of a lat-long probe at `origin`, in the
    environment map's own parameterisation (EnvironmentLight::sample_dir, as
    the kernel's env_dir reads a map): ray p = x + y * w looks along the centre
    of texel (x, y) of a w x h map, row 0 = +y, theta = (y + 0.5) / h * pi
    from +y, phi = (x + 0.5) / w * 2 pi, d = (-sin theta sin phi, cos theta,
    sin theta cos phi), tmax = +inf.  So the (h, w, 3) radiance
    Device.render_rays returns for these rays IS that map, row 0 on top as
    image_io.write_exr takes it: saved and loaded as the scene's environment
    light, a miss along d looks up what the probe saw along d."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    theta = (y + 0.5) / h * np.pi
    phi = (x + 0.5) / w * 2.0 * np.pi
    d = np.stack([-np.sin(theta) * np.sin(phi), np.cos(theta), np.sin(theta) * np.cos(phi)], -1)
    rays = np.zeros((h, w, 8), np.float32)
    rays[..., 0:3] = np.asarray(origin, np.float64).reshape(3)
    rays[..., 3] = np.inf
    d32 = d.astype(np.float32)
    d32 /= np.linalg.norm(d32.astype(np.float64), axis=-1, keepdims=True).astype(np.float32)
    rays[..., 4:7] = d32
    return rays.reshape(h * w, 8)


def tile_fifo(w: int, h: int, tile: int = TILE) -> List[Tuple[int, int, int, int]]:
    """The reference's row-major tile work queue (pathtracer.cpp:209-214)."""
    return [(x, y, tile, tile) for y in range(0, h, tile) for x in range(0, w, tile)]


def to_color(hdr: np.ndarray) -> np.ndarray:
    """HDRImageBuffer::toColor (image.h:174-189) + Color -> RGBA8
    (ImageBuffer::update_pixel, image.h:49-58) of a whole (H, W, 3) float32
    buffer, through libptgpu.so's pt_to_color (the reference's powf
    arithmetic, bit-exact: tests/test_output.py).  Returns (H, W, 4) uint8."""
    hdr = np.ascontiguousarray(hdr, dtype=np.float32)
    h, w = hdr.shape[:2]
    frame = np.zeros((h, w), np.uint32)
    native.check(native.lib().pt_to_color(hdr.ctypes.data, w, h, 0, 0, w, h, frame.ctypes.data))
    return frame.view(np.uint8).reshape(h, w, 4)


def env_tables(rgb: np.ndarray):
    """pt_env_tables: EnvironmentLight's float32 tables of an (H, W, 3) map as
    an upload builds them (host only): p_theta (H,), p_phi (H, W), pdf (H, W)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    p_theta, p_phi, pdf = np.zeros(h, np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    native.check(native.lib().pt_env_tables(rgb.ctypes.data, w, h, p_theta.ctypes.data, p_phi.ctypes.data,
                                            pdf.ctypes.data))
    return p_theta, p_phi, pdf


class PathTracer:
    def __init__(self, ns_aa: int = 1, max_ray_depth: int = 4, ns_area_light: int = 1, ns_diff: int = 1,
                 ns_glsy: int = 1, ns_refr: int = 1, num_threads: int = 1, envmap=None, device: int = 0,
                 seed: int = 1, gpu_bvh: bool = False):
        # envmap: an OpenEXR path or a float (h, w, 3) lat-long array; like the
        # reference (pathtracer.cpp:42-46, 88-90) it becomes an EnvironmentLight
        # appended to the scene's lights in set_scene.
        if isinstance(envmap, str):
            from . import scene_loader
            envmap = scene_loader.load_exr(envmap)
        self.envmap = None if envmap is None else np.ascontiguousarray(envmap, dtype=np.float32)
        self.state = State.INIT
        self.ns_aa = int(ns_aa)
        self.max_ray_depth = int(max_ray_depth)
        self.ns_area_light = int(ns_area_light)
        self.ns_diff, self.ns_glsy, self.ns_refr = ns_diff, ns_diff, ns_refr  # pathtracer.cpp:38-40 (sic)
        self.numWorkerThreads = int(num_threads)
        self.imageTileSize = TILE
        self.seed = int(seed)
        self.scene: Optional[Scene] = None
        self.camera: Optional[native.pt_camera] = None
        self.sampleBuffer = np.zeros((0, 0, 3), np.float32)
        self.frameBuffer = np.zeros((0, 0, 4), np.uint8)
        self._device_index = device
        self.gpu_bvh = bool(gpu_bvh)  # build the BVH on the GPU (PARALLEL_BUILD_BVH, setup.cu:188-189)
        self._dev: Optional[Device] = None
        self.last_stats: dict = {}
        self.last_progressive: dict = {}  # render_progressive: tiles, passes per tile, final tile errors

    # ---- configuration (pathtracer.cpp:76-127)
    def _device(self) -> Device:
        if self._dev is None:
            self._dev = Device(self._device_index)
        return self._dev

    def has_valid_configuration(self) -> bool:
        return self.scene is not None and self.camera is not None and self.sampleBuffer.size > 0

    def set_scene(self, scene: Scene):
        if self.state != State.INIT:
            return
        if self.envmap is not None and "env_rgb" not in scene.arrays.d:
            d = dict(scene.arrays.d)
            h, w, _ = self.envmap.shape
            d["light_type"] = np.append(d["light_type"], np.int32(native.PT_LIGHT_ENVIRONMENT)).astype(np.int32)
            d["light_rad"] = np.append(d["light_rad"], np.zeros(3, np.float32))
            d["light_geom"] = np.append(d["light_geom"], np.zeros(12))
            d["light_area"] = np.append(d["light_area"], np.float32(0))
            d["env_shape"] = np.array([h, w], np.int64)
            d["env_rgb"] = self.envmap.reshape(-1)
            scene = Scene(native.SceneArrays(d))
        self.scene = scene
        self._device().upload_scene(scene, gpu_bvh=self.gpu_bvh)
        if self.has_valid_configuration():
            self.state = State.READY

    def set_camera(self, camera: native.pt_camera):
        self.camera = camera
        self._device().set_camera(camera)
        if self.has_valid_configuration():
            self.state = State.READY

    def set_frame_size(self, width: int, height: int):
        self.sampleBuffer = np.zeros((height, width, 3), np.float32)
        self.frameBuffer = np.zeros((height, width, 4), np.uint8)
        if self.has_valid_configuration():
            self.state = State.READY

    def clear(self):
        if self.state != State.READY:
            return
        self.scene = None
        self.camera = None
        self.sampleBuffer = np.zeros((0, 0, 3), np.float32)
        self.frameBuffer = np.zeros((0, 0, 4), np.uint8)
        self.state = State.INIT

    # ---- rendering
    def _params(self):
        h, w = self.sampleBuffer.shape[:2]
        self._device().set_params(w, h, self.ns_aa, self.max_ray_depth, self.ns_area_light, self.seed)

    def raytrace_tile(self, tile_x: int, tile_y: int, tile_w: int, tile_h: int, stats: bool = False):
        """Drop-in for PathTracer::raytrace_tile: HDR for the tile, then toColor."""
        self.render_tiles([(tile_x, tile_y, tile_w, tile_h)], stats=stats)

    def render_tiles(self, tiles: Iterable[Tuple[int, int, int, int]], stats: bool = False):
        if not self.has_valid_configuration():
            raise RuntimeError("PathTracer is not configured (scene, camera, frame size)")
        tiles = list(tiles)
        self._params()
        dev = self._device()
        dev.render_tiles(tiles, self.sampleBuffer, stats=stats)
        self.last_stats = dev.stats()
        h, w = self.sampleBuffer.shape[:2]
        for (x, y, tw, th) in tiles:
            x1, y1 = min(x + tw, w), min(y + th, h)
            self.frameBuffer[y:y1, x:x1] = to_color(self.sampleBuffer[y:y1, x:x1])

    def render_tile_workers(self, num_threads: Optional[int] = None, asynchronous: bool = True,
                            tiles: Optional[Sequence[Tuple[int, int, int, int]]] = None):
        """The reference's tile workers (start_raytracing + worker_thread,
        pathtracer.cpp:192-221, 613-637): `num_threads` threads pop tiles from
        the 32x32 FIFO and call raytrace_tile on each, through ONE context
        (calls serialised by a lock, as INTEGRATION.md's adapter does).
        asynchronous=True: raytrace_tile is pt_tile_submit (tiles batched into
        launches, each completed into sampleBuffer/frameBuffer by the context's
        completion thread; the last worker's pt_tile_finish waits for all);
        asynchronous=False: one synchronous pt_render_tiles launch per tile."""
        import queue
        import threading
        if not self.has_valid_configuration():
            raise RuntimeError("PathTracer is not configured (scene, camera, frame size)")
        h, w = self.sampleBuffer.shape[:2]
        self._params()
        dev = self._device()
        work = queue.Queue()
        for t in (tile_fifo(w, h) if tiles is None else tiles):
            work.put(t)
        lock = threading.Lock()
        errors = []

        def worker():
            try:
                while True:
                    try:
                        t = work.get_nowait()
                    except queue.Empty:
                        return
                    if asynchronous:
                        with lock:
                            dev.submit_tile(t, self.sampleBuffer, self.frameBuffer)
                    else:
                        with lock:
                            dev.render_tiles([t], self.sampleBuffer)
                        x1, y1 = min(t[0] + t[2], w), min(t[1] + t[3], h)
                        self.frameBuffer[t[1]:y1, t[0]:x1] = to_color(self.sampleBuffer[t[1]:y1, t[0]:x1])
            except Exception as e:  # pragma: no cover - surfaced below
                errors.append(e)

        ths = [threading.Thread(target=worker) for _ in range(num_threads or self.numWorkerThreads)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        if asynchronous:
            dev.finish_tiles()
        if errors:
            raise errors[0]

    def raytrace_pixel(self, x: int, y: int) -> np.ndarray:
        self.raytrace_tile(x, y, 1, 1)
        return self.sampleBuffer[y, x].copy()

    def start_raytracing(self, stats: bool = False):
        """Whole frame: every tile of the FIFO in one batched launch."""
        if self.state != State.READY:
            return
        self.state = State.RENDERING
        self.sampleBuffer[...] = 0
        self.frameBuffer[...] = 0
        h, w = self.sampleBuffer.shape[:2]
        self.render_tiles(tile_fifo(w, h), stats=stats)
        self.state = State.DONE

    def render_progressive(self, passes: int, target_error: Optional[float] = None, denoise=False):
        """Progressive rendering on a device film: up to `passes` passes of
        ns_aa fresh samples each over the tiles still active, accumulated on
        the GPU.  With a target, after every pass from the second on a tile
        whose error (Film.tile_error: the largest relative standard error of
        its pixels' mean luminance) is <= target_error leaves the active set;
        it stops when the set is empty.  sampleBuffer / frameBuffer come from
        the film's resolve; self.last_progressive records the tiles, the
        passes each one received and its final error.  denoise (True, or the
        parameters Film.denoise takes): the film's first-hit features are set
        once, before the passes, and sampleBuffer / frameBuffer hold the
        denoised mean (Film.denoise) instead of the resolved one."""
        if not self.has_valid_configuration():
            raise RuntimeError("PathTracer is not configured (scene, camera, frame size)")
        h, w = self.sampleBuffer.shape[:2]
        self._params()
        dev = self._device()
        tiles = tile_fifo(w, h)
        counts = np.zeros(len(tiles), np.int64)
        active = list(range(len(tiles)))
        film = dev.film(w, h)
        try:
            if denoise:
                film.set_features(tiles)
            for p in range(int(passes)):
                if not active:
                    break
                film.add_pass([tiles[i] for i in active])
                counts[active] += 1
                if target_error is not None and p >= 1:
                    e = film.tile_error([tiles[i] for i in active])
                    active = [i for i, v in zip(active, e) if not v <= target_error]
            if denoise:
                hdr, rgba = film.denoise(None if denoise is True else denoise)
            else:
                hdr, rgba, _ = film.resolve(err=False)
            errors = film.tile_error(tiles)
            info = film.info()
        finally:
            film.close()
        self.sampleBuffer[...] = hdr
        self.frameBuffer[...] = rgba
        self.last_stats = dev.stats()
        self.last_progressive = {"tiles": tiles, "passes": counts, "tile_error": errors,
                                 "spp": self.ns_aa, "total_passes": int(info["passes"])}

    def render_interactive(self, cameras, passes_per_camera: int, denoise=False, reproject=True):
        """A display loop over a camera path on ONE device film (a generator).
        For each camera: set_camera; then the film's features are set (the
        first camera), the film is reprojected into the new view
        (Film.reproject: later cameras; reproject may be the parameters it
        takes), or, with reproject=False, cleared and its features set again;
        then passes_per_camera passes of ns_aa fresh samples; then
        sampleBuffer / frameBuffer take the film's resolve, or with denoise
        (True, or Film.denoise's parameters) its denoised mean.  Yields, per
        camera, Film.reproject_info() of that camera's reproject (zeros where
        none ran).  Sample indices go on across the whole path unless the film
        is cleared."""
        if self.scene is None or self.sampleBuffer.size == 0:
            raise RuntimeError("PathTracer is not configured (scene, frame size)")
        h, w = self.sampleBuffer.shape[:2]
        dev = self._device()
        tiles = tile_fifo(w, h)
        none = {k: 0 for k, _ in native.pt_reproject_info._fields_}
        film = None
        try:
            for i, cam in enumerate(cameras):
                self.set_camera(cam)
                self._params()
                info = dict(none)
                if film is None:
                    film = dev.film(w, h)
                    film.set_features(tiles)
                elif reproject:
                    film.reproject(None if reproject is True else reproject)
                    info = film.reproject_info()
                else:
                    film.clear()
                    film.set_features(tiles)
                for _ in range(int(passes_per_camera)):
                    film.add_pass(tiles)
                if denoise:
                    hdr, rgba = film.denoise(None if denoise is True else denoise)
                else:
                    hdr, rgba, _ = film.resolve(err=False)
                self.sampleBuffer[...] = hdr
                self.frameBuffer[...] = rgba
                yield info
        finally:
            if film is not None:
                film.close()

    def stop(self):
        if self.state in (State.RENDERING, State.DONE):
            self.state = State.READY

    def save_image(self, path: str):
        """Writes frameBuffer flipped vertically (pathtracer.cpp:662-672) as PNG."""
        from .image_io import write_png
        write_png(path, self.frameBuffer[::-1])
