#!/usr/bin/env python3
"""Cost of the traced ray differentials (zoic_ray_differentials_device) against the ray pass they follow: C2, C3, C5 at full
size, one JSON line.

    python tools/bench_differentials.py [--reps 3] [--precision fast|strict] [--arnold-rows 4194304]

Per config the frame runs in slabs of at most 2^28 rays (the buffers of a whole C5 frame would be 200 GB); every slab's samples are
synthesised on the device, then the ray pass and the differential pass are timed with device events on one stream, after one
warm-up frame.  ray_ms / diff_ms: the whole frame, the mean over --reps frames.  The differential pass reads 16 B (sample) + 32 B
(record) and writes 48 B per ray: diff_gbs = 96 B x rays / diff_ms (an upper bound of its DRAM traffic: a wave of dead rays skips
its samples).  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own.
arnold: rows/s of zoic_create_rays_arnold and zoic_create_rays_arnold_differentials on the same C2 rows (page-locked host arrays)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLAB = 1 << 28


def frame(torch, cam, c, n, bufs, stream, timed):
    """one frame in slabs: (ray ms, differential ms) by device events"""
    s, rays, out = bufs
    ray_ms = diff_ms = 0.0
    for base in range(0, n, SLAB):
        m = min(SLAB, n - base)
        cam.generate_samples(m, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base, out=s[:m], stream=stream.cuda_stream)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(stream)
        cam.create_rays(s[:m], ray_index_base=base, out=dict(rays=rays[:m]), stream=stream.cuda_stream)
        e[1].record(stream)
        cam.ray_differentials(s[:m], rays[:m], ray_index_base=base, out=out[:m], stream=stream.cuda_stream)
        e[2].record(stream)
        e[2].synchronize()
        if timed:
            ray_ms += e[0].elapsed_time(e[1])
            diff_ms += e[1].elapsed_time(e[2])
    return ray_ms, diff_ms


def arnold_rows(cam, n):
    import numpy as np
    from zoic_amd.camera import PinnedArray
    from zoic_amd.workloads import synthetic_samples
    import ctypes as C
    from zoic_amd import _capi
    s = synthetic_samples(n, 1920, 1080, 8, seed=1)
    inp, outp = PinnedArray((n, 7), np.float32), PinnedArray((n, 21), np.float32)
    inp.array[:] = 0.0
    inp.array[:, 0], inp.array[:, 1], inp.array[:, 4], inp.array[:, 5] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    inp.array[:, 2] = inp.array[:, 3] = 1.0 / 1080.0
    res = {}
    for name in ("zoic_create_rays_arnold", "zoic_create_rays_arnold_differentials"):
        fn = getattr(cam._lib, name)
        args = (cam._h, n, inp.array.ctypes.data_as(C.POINTER(_capi.CameraInput)), outp.array.ctypes.data_as(C.POINTER(_capi.CameraOutput)), 0)
        cam._check(fn(*args))   # warm-up
        t0 = time.perf_counter()
        for _ in range(3):
            cam._check(fn(*args))
        res[name] = round(3 * n / (time.perf_counter() - t0) / 1e6, 1)
    inp.free()
    outp.free()
    return {"rows": n, "mrows_per_s": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--arnold-rows", type=int, default=1 << 22)
    a = ap.parse_args()
    import torch
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_differentials: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_differentials", "precision": a.precision, "bytes_per_ray": {"in": 16 + 32, "out": 48}, "configs": []}
    cams = {}
    for cfg in a.configs.split(","):
        c = CONFIGS[cfg]
        n = c["width"] * c["height"] * c["spp"]
        cam = ZoicCamera(device=0)
        if c["bokeh"]:
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_FAST if a.precision == "fast" else PRECISION_STRICT)
        cam.update(**camera_params(cfg))
        m = min(n, SLAB)
        bufs = (torch.empty((m, 4), dtype=torch.float32, device=dev), torch.empty((m, 8), dtype=torch.float32, device=dev),
                torch.empty((m, 12), dtype=torch.float32, device=dev))
        frame(torch, cam, c, n, bufs, stream, False)
        ray_ms = diff_ms = 0.0
        for _ in range(a.reps):
            r, d = frame(torch, cam, c, n, bufs, stream, True)
            ray_ms += r / a.reps
            diff_ms += d / a.reps
        live = float((bufs[1][:m, 6] != 0).float().mean())
        result["configs"].append({"config": cfg, "rays": n, "ray_ms": round(ray_ms, 3), "diff_ms": round(diff_ms, 3),
                                  "diff_over_ray": round(diff_ms / ray_ms, 3), "diff_gbs": round(96.0 * n / diff_ms / 1e6, 1),
                                  "live_frac_last_slab": round(live, 4)})
        del bufs
        torch.cuda.empty_cache()
        cams[cfg] = cam
    if a.arnold_rows > 0:
        cam = cams.get("C2")
        if cam is None:
            cam = ZoicCamera(device=0)
            cam.update(**camera_params("C2"))
        result["arnold_C2"] = arnold_rows(cam, a.arnold_rows)
    for cam in cams.values():
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
