#!/usr/bin/env python3
"""Rate of the reverse projection (zoic_project_points_device) and latency of its host build (zoic_project_point), one JSON line.

    python tools/bench_reverse.py [--reps 5] [--host-points 20000]

Input per camera (C2 TESSAR, C3 DOUBLE_GAUSS, C5 PETZVAL and the thin lens of C1, STRICT): a 3840 x 2160 grid of points, the lines of
sight of the pixel centres through the paraxial pupil (Po = (sx t, sy t, -1) d with t = half the sensor width over the focal length),
placed at three depths d: near (2 focal lengths), focalDistance and 100 x focalDistance -- 24.9 M points per camera.  The batch call is
timed with device events on one stream after one warm-up; points/s is the mean over --reps calls of each depth.  projected: the
fraction of the points with flag bit 0.  Host: zoic_project_point on one thread over --host-points points of the focalDistance grid
(through ctypes: ~1 us of each call is the binding), median and p99 per call.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=20000)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera, _capi
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_reverse: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lib = _capi.load()
    xs = ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W * 2.0 - 1.0)
    ys = ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H * 2.0 - 1.0) * (H / W)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    n = W * H
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    scr = torch.empty((n, 2), dtype=torch.float32, device=dev)
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    result = {"tool": "bench_reverse", "grid": [W, H], "cameras": []}
    for name, cfg, over in (("C2", "C2", {}), ("C3", "C3", {}), ("C5", "C5", {}), ("thin", "C1", {})):
        p = camera_params(cfg)
        p.update(over)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_STRICT)
        cam.update(**p)
        t = 0.5 * p["sensorWidth"] / abs(p["focalLength"])
        row = {"camera": name, "lens": os.path.basename(p.get("lensDataPath") or "thin"), "depths": []}
        for label, d in (("near", 2.0 * abs(p["focalLength"])), ("focalDistance", p["focalDistance"]), ("100x", 100.0 * p["focalDistance"])):
            pts[:, 0] = (gx * t * d).reshape(-1)
            pts[:, 1] = (gy * t * d).reshape(-1)
            pts[:, 2] = -d
            torch.cuda.synchronize(dev)
            cam.project_points(pts, out=scr, flags=flags, stream=stream.cuda_stream)   # warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                cam.project_points(pts, out=scr, flags=flags, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            proj = float(((flags & 1) != 0).float().mean().item())
            row["depths"].append({"depth": label, "d_cm": d, "ms": round(ms, 4), "Gpoints_per_s": round(n / ms / 1e6, 3), "projected": round(proj, 5)})
            if label == "focalDistance":   # host latency on the same points
                hp = pts[:: max(1, n // a.host_points)][: a.host_points].cpu().numpy()
                vec = [_capi.Vec3(*map(float, q)) for q in hp]
                ps = (C.c_float * 2)()
                fl = C.c_uint32()
                fn, h = lib.zoic_project_point, cam._h
                lat = np.empty(len(vec))
                for i, v in enumerate(vec):
                    t0 = time.perf_counter_ns()
                    fn(h, C.byref(v), ps, C.byref(fl))
                    lat[i] = time.perf_counter_ns() - t0
                row["host_us_median"] = round(float(np.median(lat)) / 1e3, 3)
                row["host_us_p99"] = round(float(np.percentile(lat, 99)) / 1e3, 3)
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
